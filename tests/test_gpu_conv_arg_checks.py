"""GPU test of the STATUS CODES of the scn_conv_* entry points (and scn_clear_list / scn_clear_mask): which of SCN_ERR_BAD_ARG,
SCN_ERR_BAD_SHAPE, SCN_ERR_UNSUPPORTED and SCN_ERR_WORKSPACE an entry answers a faulty call with, and which of them wins where a
call has two faults.  The C-ABI wrappers of scn_conv.hip make these checks ahead of every launch, each entry its own set in its own
order, and callers (scone_gcn_amd/ops.py falls back on SCN_ERR_UNSUPPORTED and raises on the rest) depend on the answers.

One tiny blocked operator: 64 rows, identity + two value arrays on a tridiagonal pattern (ONE plan block), ns = 4, S = 2 slabs, 32
channels; a second one for the 16-channel (slab-pair) forms; a third with one value array for the power entries.  For every entry
there is one valid call (key "<entry>:ok", must be SCN_OK) and a list of single-fault calls -- each required pointer NULL in turn, an
element of a pointer array NULL, n_slabs = 0 and 65536, act = 4, ns = 3, 24 channels, a workspace one byte short, a unit list
without its count, a misaligned dx for the dzmask entry, the mask NULL where an entry then makes the plain call -- and a few
double-fault calls.

EXPECTED holds the codes as literals.  They were recorded from the library as it was BEFORE the wrappers were rewritten onto shared
helpers (the revision's build selected with SCN_LIB_PATH, this table run once), not from the code under test.

Every faulty call is one the wrappers reject before any launch, so no kernel ever sees a bad pointer or a slab count its tensors
do not have.  That is why some entries lack some faults: scn_conv_forward / _backward (and their _list forms without a list) hand
ns = 3 or 24 channels to the generic kernels, the blocked path of scn_conv_backward / _list / _accumulate does not look at W[s] and
dW[s], and scn_conv_forward_first, scn_conv_forward_power and scn_clear_mask have no cap on n_slabs.  Where an entry has no cap but a
workspace, n_slabs = 65536 is answered by the workspace test: the calls here pass EXACTLY the bytes the S = 2 call needs.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

E, S, NS = 64, 2, 4
TANH = 1

# "<entry><channels>:<fault>" -> status, recorded from the library as it was before the wrappers' rewrite (see above)
EXPECTED = {
    'forward32:ok': 0,
    'forward32:c=NULL': -1,
    'forward32:src=NULL': -1,
    'forward32:c_in=NULL': -1,
    'forward32:W=NULL': -1,
    'forward32:out=NULL': -1,
    'forward32:n_slabs=0': -2,
    'forward32:n_slabs=65536': -4,
    'forward32:src[0]=NULL': -1,
    'forward32:c_in[0]=0': -1,
    'forward32:W[1]=NULL': -1,
    'forward32:act=4': -2,
    'forward32:ns=0': -2,
    'forward32:n_slabs=65536+W[1]=NULL': -4,
    'forward32:n_slabs=0+out=NULL': -1,
    'forward_list32:ok': 0,
    'forward_list32:c=NULL': -1,
    'forward_list32:src=NULL': -1,
    'forward_list32:c_in=NULL': -1,
    'forward_list32:W=NULL': -1,
    'forward_list32:out=NULL': -1,
    'forward_list32:n_slabs=0': -2,
    'forward_list32:n_slabs=65536': -4,
    'forward_list32:wl.block=NULL': -1,
    'forward_list32:W[1]=NULL': -1,
    'forward_list32:act=4': -2,
    'forward_list32:ns=3': -4,
    'forward_list32:c=24': -4,
    'forward_keep32:ok': 0,
    'forward_keep32:keep=NULL': 0,
    'forward_keep32:c=NULL': -1,
    'forward_keep32:src=NULL': -1,
    'forward_keep32:c_in=NULL': -1,
    'forward_keep32:W=NULL': -1,
    'forward_keep32:out=NULL': -1,
    'forward_keep32:n_slabs=0': -2,
    'forward_keep32:n_slabs=65536': -4,
    'forward_keep32:src[0]=NULL': -1,
    'forward_keep32:W[1]=NULL': -1,
    'forward_keep32:act=4': -2,
    'forward_keep32:ns=3': -4,
    'forward_keep32:c=24': -4,
    'forward_keep_units32:ok': 0,
    'forward_keep_units32:no units': 0,
    'forward_keep_units32:keep=NULL, no units': 0,
    'forward_keep_units32:units without count': -1,
    'forward_keep_units32:count without units': -1,
    'forward_keep_units32:units without keep': -1,
    'forward_keep_units32:units without count+n_slabs=0': -1,
    'forward_keep_units32:c=NULL': -1,
    'forward_keep_units32:W=NULL': -1,
    'forward_keep_units32:out=NULL': -1,
    'forward_keep_units32:n_slabs=0': -2,
    'forward_keep_units32:n_slabs=65536': -4,
    'forward_keep_units32:ns=3': -4,
    'forward16:ok': 0,
    'forward_list16:ok': 0,
    'forward_keep16:ok': 0,
    'forward_keep16:keep=NULL': 0,
    'forward_keep_units16:ok': 0,
    'forward_accumulate:ok': 0,
    'forward_accumulate:c=NULL': -1,
    'forward_accumulate:src=NULL': -1,
    'forward_accumulate:c_in=NULL': -1,
    'forward_accumulate:W=NULL': -1,
    'forward_accumulate:out=NULL': -1,
    'forward_accumulate:partial=NULL': -1,
    'forward_accumulate:n_slabs=0': -2,
    'forward_accumulate:n_slabs=65536': -4,
    'forward_accumulate:src[0]=NULL': -1,
    'forward_accumulate:W[1]=NULL': -1,
    'forward_accumulate:act=4': -2,
    'forward_accumulate:ns=3': -4,
    'forward_accumulate:c=24': -4,
    'forward_accumulate:c=16': -4,
    'forward_accumulate:act=4+n_slabs=65536': -2,
    'backward32:ok': 0,
    'backward32:dx=NULL': 0,
    'backward32:c=NULL': -1,
    'backward32:dz=NULL': -1,
    'backward32:c_dz=NULL': -1,
    'backward32:W=NULL': -1,
    'backward32:aux=NULL': -1,
    'backward32:dW=NULL': -1,
    'backward32:workspace=NULL': -1,
    'backward32:n_slabs=0': -2,
    'backward32:n_slabs=65536': -6,
    'backward32:dz[0]=NULL': -1,
    'backward32:c_dz[0]=0': -1,
    'backward32:act=4': -2,
    'backward32:ns=0': -2,
    'backward32:workspace short': -6,
    'backward32:workspace short+act=4': -2,
    'backward32:workspace short+dz[0]=NULL': -1,
    'backward_list32:ok': 0,
    'backward_list32:c=NULL': -1,
    'backward_list32:dz=NULL': -1,
    'backward_list32:c_dz=NULL': -1,
    'backward_list32:W=NULL': -1,
    'backward_list32:aux=NULL': -1,
    'backward_list32:dW=NULL': -1,
    'backward_list32:workspace=NULL': -1,
    'backward_list32:n_slabs=0': -2,
    'backward_list32:n_slabs=65536': -6,
    'backward_list32:wl.block=NULL': -1,
    'backward_list32:act=4': -2,
    'backward_list32:ns=3': -4,
    'backward_list32:c=24': -4,
    'backward_list32:workspace short': -6,
    'backward_accumulate:ok': 0,
    'backward_accumulate:c=NULL': -1,
    'backward_accumulate:dz=NULL': -1,
    'backward_accumulate:c_dz=NULL': -1,
    'backward_accumulate:W=NULL': -1,
    'backward_accumulate:aux=NULL': -1,
    'backward_accumulate:dW=NULL': -1,
    'backward_accumulate:workspace=NULL': -1,
    'backward_accumulate:dx=NULL': -1,
    'backward_accumulate:dx_partial=NULL': -1,
    'backward_accumulate:n_slabs=0': -2,
    'backward_accumulate:n_slabs=65536': -6,
    'backward_accumulate:dz[0]=NULL': -1,
    'backward_accumulate:act=4': -2,
    'backward_accumulate:ns=3': -4,
    'backward_accumulate:c=24': -4,
    'backward_accumulate:c=16': -4,
    'backward_accumulate:workspace short': -6,
    'backward_accumulate:ns=3+workspace short': -4,
    'backward_dzmask:ok': 0,
    'backward_dzmask:mask=NULL': 0,
    'backward_dzmask:c=NULL': -1,
    'backward_dzmask:dz=NULL': -1,
    'backward_dzmask:c_dz=NULL': -1,
    'backward_dzmask:W=NULL': -1,
    'backward_dzmask:aux=NULL': -1,
    'backward_dzmask:dW=NULL': -1,
    'backward_dzmask:workspace=NULL': -1,
    'backward_dzmask:n_slabs=0': -2,
    'backward_dzmask:n_slabs=65536': -4,
    'backward_dzmask:dz[0]=NULL': -1,
    'backward_dzmask:W[1]=NULL': -1,
    'backward_dzmask:dW[2]=NULL': -1,
    'backward_dzmask:act=4': -2,
    'backward_dzmask:ns=3': -4,
    'backward_dzmask:c=24': -4,
    'backward_dzmask:c=16': -4,
    'backward_dzmask:workspace short': -6,
    'backward_dzmask:W[1]=NULL+n_slabs=65536': -4,
    'backward_dzmask:dW[2]=NULL+c=24': -1,
    'backward_dzmask:c=24+workspace short': -4,
    'backward_dzmask:dx misaligned': -4,
    'backward_dzmask:dx misaligned+workspace short': -4,
    'backward_dzmask:dx misaligned+W[1]=NULL': -1,
    'backward_visit:ok': 0,
    'backward_visit:mask=NULL': -1,
    'backward_visit:c=NULL': -1,
    'backward_visit:dz=NULL': -1,
    'backward_visit:c_dz=NULL': -1,
    'backward_visit:W=NULL': -1,
    'backward_visit:aux=NULL': -1,
    'backward_visit:dW=NULL': -1,
    'backward_visit:workspace=NULL': -1,
    'backward_visit:n_slabs=0': -2,
    'backward_visit:n_slabs=65536': -4,
    'backward_visit:dz[0]=NULL': -1,
    'backward_visit:W[1]=NULL': -1,
    'backward_visit:dW[2]=NULL': -1,
    'backward_visit:act=4': -2,
    'backward_visit:ns=3': -4,
    'backward_visit:c=24': -4,
    'backward_visit:c=16': -4,
    'backward_visit:workspace short': -6,
    'backward_visit:W[1]=NULL+n_slabs=65536': -4,
    'backward_visit:dW[2]=NULL+c=24': -1,
    'backward_visit:c=24+workspace short': -4,
    'backward16:ok': 0,
    'backward16:dx=NULL': 0,
    'backward_list16:ok': 0,
    'forward_first:ok': 0,
    'forward_first:ok, list': 0,
    'forward_first:ok, y only': 0,
    'forward_first:ok, 16': 0,
    'forward_first:c=NULL': -1,
    'forward_first:x=NULL': -1,
    'forward_first:W=NULL': -1,
    'forward_first:y_out=NULL': -1,
    'forward_first:n_slabs=0': -2,
    'forward_first:W[1]=NULL': -1,
    'forward_first:wl.block=NULL': -1,
    'forward_first:y only with a list': -4,
    'forward_first:act=4': -2,
    'forward_first:ns=3': -4,
    'forward_first:c_out=24': -4,
    'forward_first:act=4+ns=3': -2,
    'dw_first:ok': 0,
    'dw_first:ok, list': 0,
    'dw_first:ok, x only': 0,
    'dw_first:ok, y only': 0,
    'dw_first:c=NULL': -1,
    'dw_first:dz=NULL': -1,
    'dw_first:dW=NULL': -1,
    'dw_first:workspace=NULL': -1,
    'dw_first:n_slabs=0': -2,
    'dw_first:n_slabs=65536': -6,
    'dw_first:x=NULL+y=NULL': -1,
    'dw_first:list without y': -1,
    'dw_first:dW[2]=NULL': -1,
    'dw_first:ns=3': -4,
    'dw_first:c_dz=24': -4,
    'dw_first:workspace short': -6,
    'dw_first:c_dz=24+workspace short': -4,
    'fused_first32:ok': 0,
    'fused_first32:ok, list': 0,
    'fused_first32:c=NULL': -1,
    'fused_first32:dz=NULL': -1,
    'fused_first32:W=NULL': -1,
    'fused_first32:aux=NULL': -1,
    'fused_first32:y=NULL': -1,
    'fused_first32:dW=NULL': -1,
    'fused_first32:dW_first=NULL': -1,
    'fused_first32:workspace=NULL': -1,
    'fused_first32:n_slabs=0': -2,
    'fused_first32:n_slabs=65536': -4,
    'fused_first32:W[1]=NULL': -1,
    'fused_first32:dW[2]=NULL': -1,
    'fused_first32:dW_first[0]=NULL': -1,
    'fused_first32:wl.block=NULL': -1,
    'fused_first32:act=4': -2,
    'fused_first32:ns=3': -4,
    'fused_first32:channels=24': -4,
    'fused_first32:workspace short': -6,
    'fused_first32:workspace short+n_slabs=65536': -4,
    'fused_first32:workspace short+act=4': -2,
    'fused_first_from_y:ok': 0,
    'fused_first_from_y:c=NULL': -1,
    'fused_first_from_y:dz=NULL': -1,
    'fused_first_from_y:W=NULL': -1,
    'fused_first_from_y:W_first=NULL': -1,
    'fused_first_from_y:y=NULL': -1,
    'fused_first_from_y:dW=NULL': -1,
    'fused_first_from_y:dW_first=NULL': -1,
    'fused_first_from_y:workspace=NULL': -1,
    'fused_first_from_y:n_slabs=0': -2,
    'fused_first_from_y:n_slabs=65536': -4,
    'fused_first_from_y:W[1]=NULL': -1,
    'fused_first_from_y:W_first[0]=NULL': -1,
    'fused_first_from_y:dW[2]=NULL': -1,
    'fused_first_from_y:dW_first[0]=NULL': -1,
    'fused_first_from_y:act=4': -2,
    'fused_first_from_y:ns=3': -4,
    'fused_first_from_y:channels=24': -4,
    'fused_first_from_y:channels=16': -4,
    'fused_first_from_y:workspace short': -6,
    'fused_first_from_y:channels=16+workspace short': -4,
    'fused_first_from_y:ok, list': 0,
    'fused_first_from_y:wl.block=NULL': -1,
    'fused_first_from_y_visit:ok': 0,
    'fused_first_from_y_visit:c=NULL': -1,
    'fused_first_from_y_visit:dz=NULL': -1,
    'fused_first_from_y_visit:W=NULL': -1,
    'fused_first_from_y_visit:W_first=NULL': -1,
    'fused_first_from_y_visit:y=NULL': -1,
    'fused_first_from_y_visit:dW=NULL': -1,
    'fused_first_from_y_visit:dW_first=NULL': -1,
    'fused_first_from_y_visit:workspace=NULL': -1,
    'fused_first_from_y_visit:n_slabs=0': -2,
    'fused_first_from_y_visit:n_slabs=65536': -4,
    'fused_first_from_y_visit:W[1]=NULL': -1,
    'fused_first_from_y_visit:W_first[0]=NULL': -1,
    'fused_first_from_y_visit:dW[2]=NULL': -1,
    'fused_first_from_y_visit:dW_first[0]=NULL': -1,
    'fused_first_from_y_visit:act=4': -2,
    'fused_first_from_y_visit:ns=3': -4,
    'fused_first_from_y_visit:channels=24': -4,
    'fused_first_from_y_visit:channels=16': -4,
    'fused_first_from_y_visit:workspace short': -6,
    'fused_first_from_y_visit:channels=16+workspace short': -4,
    'fused_first_from_y_visit:visit=NULL': -1,
    'forward_from_y:ok': 0,
    'forward_from_y:c=NULL': -1,
    'forward_from_y:y=NULL': -1,
    'forward_from_y:W_first=NULL': -1,
    'forward_from_y:W=NULL': -1,
    'forward_from_y:out=NULL': -1,
    'forward_from_y:n_slabs=0': -2,
    'forward_from_y:n_slabs=65536': -4,
    'forward_from_y:W_first[0]=NULL': -1,
    'forward_from_y:W[1]=NULL': -1,
    'forward_from_y:act=4': -2,
    'forward_from_y:ns=3': -4,
    'forward_from_y:channels=24': -4,
    'forward_from_y:channels=16': -4,
    'forward_from_y_keep:ok': 0,
    'forward_from_y_keep:c=NULL': -1,
    'forward_from_y_keep:y=NULL': -1,
    'forward_from_y_keep:W_first=NULL': -1,
    'forward_from_y_keep:W=NULL': -1,
    'forward_from_y_keep:out=NULL': -1,
    'forward_from_y_keep:n_slabs=0': -2,
    'forward_from_y_keep:n_slabs=65536': -4,
    'forward_from_y_keep:W_first[0]=NULL': -1,
    'forward_from_y_keep:W[1]=NULL': -1,
    'forward_from_y_keep:act=4': -2,
    'forward_from_y_keep:ns=3': -4,
    'forward_from_y_keep:channels=24': -4,
    'forward_from_y_keep:channels=16': -4,
    'forward_from_y_keep:keep=NULL': 0,
    'forward_from_y_keep_units:ok': 0,
    'forward_from_y_keep_units:c=NULL': -1,
    'forward_from_y_keep_units:y=NULL': -1,
    'forward_from_y_keep_units:W_first=NULL': -1,
    'forward_from_y_keep_units:W=NULL': -1,
    'forward_from_y_keep_units:out=NULL': -1,
    'forward_from_y_keep_units:n_slabs=0': -2,
    'forward_from_y_keep_units:n_slabs=65536': -4,
    'forward_from_y_keep_units:W_first[0]=NULL': -1,
    'forward_from_y_keep_units:W[1]=NULL': -1,
    'forward_from_y_keep_units:act=4': -2,
    'forward_from_y_keep_units:ns=3': -4,
    'forward_from_y_keep_units:channels=24': -4,
    'forward_from_y_keep_units:channels=16': -4,
    'forward_from_y_keep_units:no units': 0,
    'forward_from_y_keep_units:units without count': -1,
    'forward_from_y_keep_units:count without units': -1,
    'forward_from_y_keep_units:units without keep': -1,
    'forward_from_y_keep_units:units without count+out=NULL': -1,
    'fused_first16:ok': 0,
    'fused_first16:ok, list': 0,
    'shifted_input_keep:ok': 0,
    'shifted_input_keep:c=NULL': -1,
    'shifted_input_keep:x=NULL': -1,
    'shifted_input_keep:y_out=NULL': -1,
    'shifted_input_keep:keep=NULL': -1,
    'shifted_input_keep:n_slabs=0': -2,
    'shifted_input_keep:n_slabs=65536': -4,
    'shifted_input_keep:ns=3': -4,
    'shifted_input_keep_units:ok': 0,
    'shifted_input_keep_units:no units': 0,
    'shifted_input_keep_units:units without count': -1,
    'shifted_input_keep_units:count without units': -1,
    'shifted_input_keep_units:c=NULL': -1,
    'shifted_input_keep_units:x=NULL': -1,
    'shifted_input_keep_units:y_out=NULL': -1,
    'shifted_input_keep_units:keep=NULL': -1,
    'shifted_input_keep_units:n_slabs=0': -2,
    'shifted_input_keep_units:n_slabs=65536': -4,
    'shifted_input_keep_units:ns=3': -4,
    'shifted_input_keep_units:n_slabs=0+keep=NULL': -1,
    'forward_power32:ok': 0,
    'forward_power32:c=NULL': -1,
    'forward_power32:x0=NULL': -1,
    'forward_power32:x=NULL': -1,
    'forward_power32:W=NULL': -1,
    'forward_power32:out=NULL': -1,
    'forward_power32:n_slabs=0': -2,
    'forward_power32:W[1]=NULL': -1,
    'forward_power32:act=4': -2,
    'forward_power32:ns=3': -4,
    'forward_power32:channels=24': -4,
    'forward_power32:two value arrays': -4,
    'backward_power32:ok': 0,
    'backward_power32:c=NULL': -1,
    'backward_power32:dz=NULL': -1,
    'backward_power32:g1=NULL': -1,
    'backward_power32:W=NULL': -1,
    'backward_power32:aux=NULL': -1,
    'backward_power32:dW=NULL': -1,
    'backward_power32:workspace=NULL': -1,
    'backward_power32:n_slabs=0': -2,
    'backward_power32:n_slabs=65536': -6,
    'backward_power32:W[1]=NULL': -1,
    'backward_power32:dW[2]=NULL': -1,
    'backward_power32:act=4': -2,
    'backward_power32:ns=3': -4,
    'backward_power32:channels=24': -4,
    'backward_power32:two value arrays': -4,
    'backward_power32:workspace short': -6,
    'backward_power32:channels=24+workspace short': -4,
    'forward_power16:ok': 0,
    'backward_power16:ok': 0,
    'clear_list:ok': 0,
    'clear_list:ok, empty list': 0,
    'clear_list:c=NULL': -1,
    'clear_list:tensor=NULL': -1,
    'clear_list:wl=NULL': -1,
    'clear_list:wl.block=NULL': -1,
    'clear_list:channels=0': -1,
    'clear_list:ns=3': -4,
    'clear_list:ns=3+channels=0': -1,
    'clear_mask:ok': 0,
    'clear_mask:c=NULL': -1,
    'clear_mask:tensor=NULL': -1,
    'clear_mask:mask=NULL': -1,
    'clear_mask:n_slabs=0': -2,
    'clear_mask:channels=0': -2,
    'clear_mask:ns=3': -4,
    'clear_mask:tensor misaligned': -4,
    'clear_mask:tensor misaligned+n_slabs=0': -2,
}


class _Entry:
    def __init__(self, lib, tag, name, args):
        self.tag, self.fn, self.args = tag, getattr(lib, name), args

    def __call__(self, **over):
        unknown = set(over) - {n for n, _ in self.args}
        assert not unknown, "%s has no argument %s" % (self.tag, sorted(unknown))
        return int(self.fn(*[over.get(n, v) for n, v in self.args]))


def _build():
    """(cases: key -> thunk, keep-alive list)"""
    import scipy.sparse as sp
    from scone_gcn_amd import _lib, ops
    from scone_gcn_amd._lib import WorkListDesc, i32_array, ptr_array

    lib = _lib.load()
    rs = np.random.RandomState(7)
    dev = "cuda"
    off = sp.diags([rs.randn(E - 1), rs.randn(E - 1)], [-1, 1], format="csr")
    A0, A1 = (sp.csr_matrix((rs.randn(off.nnz).astype(np.float32), off.indices, off.indptr), shape=(E, E)) for _ in range(2))
    op32 = ops.ConvOp(E, [{"mats": [A0, A1], "identity": True, "n_cols": E}])
    op16 = ops.ConvOp(E, [{"mats": [A0, A1], "identity": True, "n_cols": E}])
    opP = ops.ConvOp(E, [{"mats": [A0], "identity": True, "n_cols": E}])
    assert op32.plan_info()[0] == 1 and op16.plan_info()[0] == 1 and opP.plan_info()[0] == 1, "one plan block"
    alive = [op32, op16, opP]

    def t(*shape, scale=1.0):
        a = torch.from_numpy((scale * rs.randn(*shape)).astype(np.float32)).to(dev)
        alive.append(a)
        return a

    def d(x):
        return ctypes.c_void_p(x.data_ptr())

    def P(*ts):                                    # an array of device pointers; None stays NULL
        arr = ptr_array([x.data_ptr() if x is not None else None for x in ts])
        alive.append(arr)
        return arr

    def I(*vals):
        arr = i32_array(vals)
        alive.append(arr)
        return arr

    def ws_of(nbytes):
        assert nbytes > 0
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        alive.append(buf)
        return d(buf), int(nbytes)

    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    mask = torch.full((1, 1), 3, dtype=torch.int32, device=dev)               # one block, one word: both slabs
    units = torch.zeros(1, dtype=torch.int32, device=dev)                     # the mask's one non-empty word
    count = torch.ones(1, dtype=torch.int32, device=dev)
    wl = ops.WorkList(sp.csr_matrix(np.ones((S, 1), bool)), dev)              # block 0, slabs 0 and 1
    wl_empty = ops.WorkList(sp.csr_matrix(np.zeros((S, 1), bool)), dev)
    wl_bad = WorkListDesc(1, None, wl.ptr.data_ptr(), wl.slab.data_ptr())     # block = NULL: not a valid list
    alive += [mask, units, count, wl, wl_empty, wl_bad]
    WL, WL_BAD = ctypes.byref(wl.desc), ctypes.byref(wl_bad)

    T = {}
    for C in (32, 16):
        T[C] = dict(x=t(S, E, NS, C), out=t(S, E, NS, C), aux=torch.tanh(t(S, E, NS, C)), dz=t(S, E, NS, C), dx=t(S, E, NS, C),
                    part=t(S, E, NS, C), W=[t(C, C, scale=0.1) for _ in range(3)], dW=[t(C, C) for _ in range(3)],
                    W1=[t(1, C, scale=0.1) for _ in range(3)], dW1=[t(1, C) for _ in range(3)])
        alive.append(T[C]["aux"])
    x1, y = t(S, E, NS, 1), t(S, E, NS, 4)

    cases = {}

    def add(e, fault, **over):
        key = "%s:%s" % (e.tag, fault)
        assert key not in cases, key
        cases[key] = lambda: e(**over)

    def nulls(e, *names):
        for n in names:
            add(e, n + "=NULL", **{n: None})

    def slabs(e, cap=True):
        add(e, "n_slabs=0", n_slabs=0)
        if cap:
            add(e, "n_slabs=65536", n_slabs=65536)

    # ---------------- forward family
    for C, op in ((32, op32), (16, op16)):
        q, h = T[C], op.handle
        Wn1 = P(q["W"][0], None, q["W"][2])
        fwd_args = [("c", h), ("n_slabs", S), ("ns", NS), ("src", P(q["x"])), ("c_in", I(C)), ("W", P(*q["W"])), ("c_out", C),
                    ("act", TANH), ("out", d(q["out"]))]
        e = _Entry(lib, "forward%d" % C, "scn_conv_forward", fwd_args + [("stream", st)])
        add(e, "ok")
        if C == 32:
            nulls(e, "c", "src", "c_in", "W", "out")
            slabs(e)
            add(e, "src[0]=NULL", src=P(None))
            add(e, "c_in[0]=0", c_in=I(0))
            add(e, "W[1]=NULL", W=Wn1)
            add(e, "act=4", act=4)
            add(e, "ns=0", ns=0)
            add(e, "n_slabs=65536+W[1]=NULL", n_slabs=65536, W=Wn1)
            add(e, "n_slabs=0+out=NULL", n_slabs=0, out=None)
        e = _Entry(lib, "forward_list%d" % C, "scn_conv_forward_list", fwd_args + [("wl", WL), ("stream", st)])
        add(e, "ok")
        if C == 32:
            nulls(e, "c", "src", "c_in", "W", "out")
            slabs(e)
            add(e, "wl.block=NULL", wl=WL_BAD)
            add(e, "W[1]=NULL", W=Wn1)
            add(e, "act=4", act=4)
            add(e, "ns=3", ns=3)
            add(e, "c=24", c_in=I(24), c_out=24)
        e = _Entry(lib, "forward_keep%d" % C, "scn_conv_forward_keep", fwd_args + [("keep", d(mask)), ("stream", st)])
        add(e, "ok")
        add(e, "keep=NULL", keep=None)                                        # the plain call
        if C == 32:
            nulls(e, "c", "src", "c_in", "W", "out")
            slabs(e)
            add(e, "src[0]=NULL", src=P(None))
            add(e, "W[1]=NULL", W=Wn1)
            add(e, "act=4", act=4)
            add(e, "ns=3", ns=3)
            add(e, "c=24", c_in=I(24), c_out=24)
        e = _Entry(lib, "forward_keep_units%d" % C, "scn_conv_forward_keep_units",
                   fwd_args + [("keep", d(mask)), ("units", d(units)), ("unit_count", d(count)), ("stream", st)])
        add(e, "ok")
        if C == 32:
            add(e, "no units", units=None, unit_count=None)
            add(e, "keep=NULL, no units", keep=None, units=None, unit_count=None)     # the plain call
            add(e, "units without count", unit_count=None)
            add(e, "count without units", units=None)
            add(e, "units without keep", keep=None)
            add(e, "units without count+n_slabs=0", unit_count=None, n_slabs=0)
            nulls(e, "c", "W", "out")
            slabs(e)
            add(e, "ns=3", ns=3)
    q, h = T[32], op32.handle
    e = _Entry(lib, "forward_accumulate", "scn_conv_forward_accumulate",
               [("c", h), ("n_slabs", S), ("ns", NS), ("src", P(q["x"])), ("c_in", I(32)), ("W", P(*q["W"])), ("c_out", 32), ("act", TANH),
                ("partial", d(q["part"])), ("out", d(q["out"])), ("stream", st)])
    add(e, "ok")
    nulls(e, "c", "src", "c_in", "W", "out", "partial")
    slabs(e)
    add(e, "src[0]=NULL", src=P(None))
    add(e, "W[1]=NULL", W=P(q["W"][0], None, q["W"][2]))
    add(e, "act=4", act=4)
    add(e, "ns=3", ns=3)
    add(e, "c=24", c_in=I(24), c_out=24)
    add(e, "c=16", c_in=I(16), c_out=16)
    add(e, "act=4+n_slabs=65536", act=4, n_slabs=65536)

    # ---------------- backward family
    for C, op in ((32, op32), (16, op16)):
        q, h = T[C], op.handle
        cdz = I(C)
        need = int(lib.scn_conv_backward_workspace(h, S, NS, cdz, C))
        wsp, wsb = ws_of(need)
        Wn1, dWn2 = P(q["W"][0], None, q["W"][2]), P(q["dW"][0], q["dW"][1], None)
        head = [("c", h), ("n_slabs", S), ("ns", NS), ("dz", P(q["dz"])), ("c_dz", cdz), ("W", P(*q["W"])), ("aux", d(q["aux"])),
                ("c_aux", C), ("act", TANH)]
        tail = [("dx", d(q["dx"])), ("dW", P(*q["dW"])), ("workspace", wsp), ("workspace_bytes", wsb)]
        e = _Entry(lib, "backward%d" % C, "scn_conv_backward", head + tail + [("stream", st)])
        add(e, "ok")
        add(e, "dx=NULL", dx=None)                                            # weight gradients only: a valid call
        if C == 32:
            nulls(e, "c", "dz", "c_dz", "W", "aux", "dW", "workspace")
            slabs(e)                                                          # (no cap: the workspace test answers 65536)
            add(e, "dz[0]=NULL", dz=P(None))
            add(e, "c_dz[0]=0", c_dz=I(0))
            add(e, "act=4", act=4)
            add(e, "ns=0", ns=0)
            add(e, "workspace short", workspace_bytes=wsb - 1)
            add(e, "workspace short+act=4", workspace_bytes=wsb - 1, act=4)
            add(e, "workspace short+dz[0]=NULL", workspace_bytes=wsb - 1, dz=P(None))
        e = _Entry(lib, "backward_list%d" % C, "scn_conv_backward_list", head + tail + [("wl", WL), ("stream", st)])
        add(e, "ok")
        if C == 32:
            nulls(e, "c", "dz", "c_dz", "W", "aux", "dW", "workspace")
            slabs(e)
            add(e, "wl.block=NULL", wl=WL_BAD)
            add(e, "act=4", act=4)
            add(e, "ns=3", ns=3)
            add(e, "c=24", c_dz=I(24), c_aux=24)
            add(e, "workspace short", workspace_bytes=wsb - 1)
        if C == 16:
            continue                                                          # the entries below take 32 channels only
        e = _Entry(lib, "backward_accumulate", "scn_conv_backward_accumulate",
                   head + [("dx_partial", d(q["part"]))] + tail + [("stream", st)])
        add(e, "ok")
        nulls(e, "c", "dz", "c_dz", "W", "aux", "dW", "workspace", "dx", "dx_partial")
        slabs(e)
        add(e, "dz[0]=NULL", dz=P(None))
        add(e, "act=4", act=4)
        add(e, "ns=3", ns=3)
        add(e, "c=24", c_dz=I(24), c_aux=24)
        add(e, "c=16", c_dz=I(16), c_aux=16)
        add(e, "workspace short", workspace_bytes=wsb - 1)
        add(e, "ns=3+workspace short", ns=3, workspace_bytes=wsb - 1)
        for name, fn in (("backward_dzmask", "scn_conv_backward_dzmask"), ("backward_visit", "scn_conv_backward_visit")):
            e = _Entry(lib, name, fn, head + tail + [("mask", d(mask)), ("stream", st)])
            add(e, "ok")
            add(e, "mask=NULL", mask=None)                                    # dzmask: the plain call; visit: refused
            nulls(e, "c", "dz", "c_dz", "W", "aux", "dW", "workspace")
            slabs(e)
            add(e, "dz[0]=NULL", dz=P(None))
            add(e, "W[1]=NULL", W=Wn1)
            add(e, "dW[2]=NULL", dW=dWn2)
            add(e, "act=4", act=4)
            add(e, "ns=3", ns=3)
            add(e, "c=24", c_dz=I(24), c_aux=24)
            add(e, "c=16", c_dz=I(16), c_aux=16)
            add(e, "workspace short", workspace_bytes=wsb - 1)
            add(e, "W[1]=NULL+n_slabs=65536", W=Wn1, n_slabs=65536)
            add(e, "dW[2]=NULL+c=24", dW=dWn2, c_dz=I(24), c_aux=24)
            add(e, "c=24+workspace short", c_dz=I(24), c_aux=24, workspace_bytes=wsb - 1)
            if name == "backward_dzmask":
                odd = ctypes.c_void_p(q["dx"].data_ptr() + 4)
                add(e, "dx misaligned", dx=odd)
                add(e, "dx misaligned+workspace short", dx=odd, workspace_bytes=wsb - 1)
                add(e, "dx misaligned+W[1]=NULL", dx=odd, W=Wn1)

    # ---------------- the first layer and the layer behind it
    q, h = T[32], op32.handle
    e = _Entry(lib, "forward_first", "scn_conv_forward_first",
               [("c", h), ("n_slabs", S), ("ns", NS), ("x", d(x1)), ("W", P(*q["W1"])), ("c_out", 32), ("act", TANH), ("out", d(q["out"])),
                ("y_out", d(y)), ("wl", None), ("stream", st)])
    add(e, "ok")
    add(e, "ok, list", wl=WL)
    add(e, "ok, y only", out=None)
    add(e, "ok, 16", c_out=16, W=P(*T[16]["W1"]), out=d(T[16]["out"]))
    nulls(e, "c", "x", "W", "y_out")
    slabs(e, cap=False)
    add(e, "W[1]=NULL", W=P(q["W1"][0], None, q["W1"][2]))
    add(e, "wl.block=NULL", wl=WL_BAD)
    add(e, "y only with a list", out=None, wl=WL)
    add(e, "act=4", act=4)
    add(e, "ns=3", ns=3)
    add(e, "c_out=24", c_out=24)
    add(e, "act=4+ns=3", act=4, ns=3)
    need = int(lib.scn_conv_dw_first_workspace(h, S, NS, 32))
    wsp, wsb = ws_of(need)
    e = _Entry(lib, "dw_first", "scn_conv_dw_first",
               [("c", h), ("n_slabs", S), ("ns", NS), ("x", d(x1)), ("y", d(y)), ("dz", d(q["dz"])), ("c_dz", 32), ("dW", P(*q["dW1"])),
                ("workspace", wsp), ("workspace_bytes", wsb), ("wl", None), ("stream", st)])
    add(e, "ok")
    add(e, "ok, list", wl=WL)
    add(e, "ok, x only", y=None)
    add(e, "ok, y only", x=None)
    nulls(e, "c", "dz", "dW", "workspace")
    slabs(e)
    add(e, "x=NULL+y=NULL", x=None, y=None)
    add(e, "list without y", y=None, wl=WL)
    add(e, "dW[2]=NULL", dW=P(q["dW1"][0], q["dW1"][1], None))
    add(e, "ns=3", ns=3)
    add(e, "c_dz=24", c_dz=24)
    add(e, "workspace short", workspace_bytes=wsb - 1)
    add(e, "c_dz=24+workspace short", c_dz=24, workspace_bytes=wsb - 1)
    for C, op in ((32, op32), (16, op16)):
        q, h = T[C], op.handle
        need = int(lib.scn_conv_backward_fused_first_workspace(h, S, NS, C))
        wsp, wsb = ws_of(need)
        Wn1, dWn2, dW1n0 = P(q["W"][0], None, q["W"][2]), P(q["dW"][0], q["dW"][1], None), P(None, q["dW1"][1], q["dW1"][2])
        W1n0 = P(None, q["W1"][1], q["W1"][2])
        mid = [("channels", C), ("act", TANH), ("y", d(y)), ("dW", P(*q["dW"])), ("dW_first", P(*q["dW1"])), ("workspace", wsp),
               ("workspace_bytes", wsb)]
        e = _Entry(lib, "fused_first%d" % C, "scn_conv_backward_fused_first",
                   [("c", h), ("n_slabs", S), ("ns", NS), ("dz", d(q["dz"])), ("W", P(*q["W"])), ("aux", d(q["aux"]))] + mid +
                   [("wl", None), ("stream", st)])
        add(e, "ok")
        add(e, "ok, list", wl=WL)
        if C == 32:
            nulls(e, "c", "dz", "W", "aux", "y", "dW", "dW_first", "workspace")
            slabs(e)
            add(e, "W[1]=NULL", W=Wn1)
            add(e, "dW[2]=NULL", dW=dWn2)
            add(e, "dW_first[0]=NULL", dW_first=dW1n0)
            add(e, "wl.block=NULL", wl=WL_BAD)
            add(e, "act=4", act=4)
            add(e, "ns=3", ns=3)
            add(e, "channels=24", channels=24)
            add(e, "workspace short", workspace_bytes=wsb - 1)
            add(e, "workspace short+n_slabs=65536", workspace_bytes=wsb - 1, n_slabs=65536)
            add(e, "workspace short+act=4", workspace_bytes=wsb - 1, act=4)
        if C == 16:
            continue                                                          # the from-y forms take 32 channels only
        fy = [("c", h), ("n_slabs", S), ("ns", NS), ("dz", d(q["dz"])), ("W", P(*q["W"])), ("W_first", P(*q["W1"]))] + mid
        for name, fn, last in (("fused_first_from_y", "scn_conv_backward_fused_first_from_y", ("wl", None)),
                               ("fused_first_from_y_visit", "scn_conv_backward_fused_first_from_y_visit", ("visit", d(mask)))):
            e = _Entry(lib, name, fn, fy + [last, ("stream", st)])
            add(e, "ok")
            nulls(e, "c", "dz", "W", "W_first", "y", "dW", "dW_first", "workspace")
            slabs(e)
            add(e, "W[1]=NULL", W=Wn1)
            add(e, "W_first[0]=NULL", W_first=W1n0)
            add(e, "dW[2]=NULL", dW=dWn2)
            add(e, "dW_first[0]=NULL", dW_first=dW1n0)
            add(e, "act=4", act=4)
            add(e, "ns=3", ns=3)
            add(e, "channels=24", channels=24)
            add(e, "channels=16", channels=16)
            add(e, "workspace short", workspace_bytes=wsb - 1)
            add(e, "channels=16+workspace short", channels=16, workspace_bytes=wsb - 1)
            if last[0] == "wl":
                add(e, "ok, list", wl=WL)
                add(e, "wl.block=NULL", wl=WL_BAD)
            else:
                add(e, "visit=NULL", visit=None)
        from_y = [("c", h), ("n_slabs", S), ("ns", NS), ("y", d(y)), ("W_first", P(*q["W1"])), ("W", P(*q["W"])), ("channels", 32),
                  ("act", TANH), ("out", d(q["out"]))]
        for name, fn, extra in (("forward_from_y", "scn_conv_forward_from_y", []),
                                ("forward_from_y_keep", "scn_conv_forward_from_y_keep", [("keep", d(mask))]),
                                ("forward_from_y_keep_units", "scn_conv_forward_from_y_keep_units",
                                 [("keep", d(mask)), ("units", d(units)), ("unit_count", d(count))])):
            e = _Entry(lib, name, fn, from_y + extra + [("stream", st)])
            add(e, "ok")
            nulls(e, "c", "y", "W_first", "W", "out")
            slabs(e)
            add(e, "W_first[0]=NULL", W_first=W1n0)
            add(e, "W[1]=NULL", W=Wn1)
            add(e, "act=4", act=4)
            add(e, "ns=3", ns=3)
            add(e, "channels=24", channels=24)
            add(e, "channels=16", channels=16)
            if name == "forward_from_y_keep":
                add(e, "keep=NULL", keep=None)                                # the plain call
            if name == "forward_from_y_keep_units":
                add(e, "no units", units=None, unit_count=None)
                add(e, "units without count", unit_count=None)
                add(e, "count without units", units=None)
                add(e, "units without keep", keep=None)
                add(e, "units without count+out=NULL", unit_count=None, out=None)
    h = op32.handle
    sik = [("c", h), ("n_slabs", S), ("ns", NS), ("x", d(x1)), ("y_out", d(y)), ("keep", d(mask))]
    e = _Entry(lib, "shifted_input_keep", "scn_conv_shifted_input_keep", sik + [("stream", st)])
    add(e, "ok")
    nulls(e, "c", "x", "y_out", "keep")
    slabs(e)
    add(e, "ns=3", ns=3)
    e = _Entry(lib, "shifted_input_keep_units", "scn_conv_shifted_input_keep_units",
               sik + [("units", d(units)), ("unit_count", d(count)), ("stream", st)])
    add(e, "ok")
    add(e, "no units", units=None, unit_count=None)
    add(e, "units without count", unit_count=None)
    add(e, "count without units", units=None)
    nulls(e, "c", "x", "y_out", "keep")
    slabs(e)
    add(e, "ns=3", ns=3)
    add(e, "n_slabs=0+keep=NULL", n_slabs=0, keep=None)

    # ---------------- power layers (identity + ONE value array)
    for C in (32, 16):
        q, h = T[C], opP.handle
        Wn1, dWn2 = P(q["W"][0], None, q["W"][2]), P(q["dW"][0], q["dW"][1], None)
        e = _Entry(lib, "forward_power%d" % C, "scn_conv_forward_power",
                   [("c", h), ("n_slabs", S), ("ns", NS), ("x0", d(q["part"])), ("x", d(q["x"])), ("W", P(*q["W"])), ("channels", C),
                    ("act", TANH), ("out", d(q["out"])), ("stream", st)])
        add(e, "ok")
        if C == 32:
            nulls(e, "c", "x0", "x", "W", "out")
            slabs(e, cap=False)
            add(e, "W[1]=NULL", W=Wn1)
            add(e, "act=4", act=4)
            add(e, "ns=3", ns=3)
            add(e, "channels=24", channels=24)
            add(e, "two value arrays", c=op32.handle)
        need = int(lib.scn_conv_backward_power_workspace(h, S, NS, C))
        wsp, wsb = ws_of(need)
        e = _Entry(lib, "backward_power%d" % C, "scn_conv_backward_power",
                   [("c", h), ("n_slabs", S), ("ns", NS), ("dz", d(q["dz"])), ("g1", d(q["part"])), ("W", P(*q["W"])), ("aux", d(q["aux"])),
                    ("channels", C), ("act", TANH), ("dx", d(q["dx"])), ("dW", P(*q["dW"])), ("workspace", wsp), ("workspace_bytes", wsb),
                    ("stream", st)])
        add(e, "ok")
        if C == 32:
            nulls(e, "c", "dz", "g1", "W", "aux", "dW", "workspace")
            slabs(e)
            add(e, "W[1]=NULL", W=Wn1)
            add(e, "dW[2]=NULL", dW=dWn2)
            add(e, "act=4", act=4)
            add(e, "ns=3", ns=3)
            add(e, "channels=24", channels=24)
            add(e, "two value arrays", c=op32.handle)
            add(e, "workspace short", workspace_bytes=wsb - 1)
            add(e, "channels=24+workspace short", channels=24, workspace_bytes=wsb - 1)

    # ---------------- clears
    q, h = T[32], op32.handle
    e = _Entry(lib, "clear_list", "scn_clear_list", [("c", h), ("ns", NS), ("channels", 32), ("tensor", d(q["out"])), ("wl", WL), ("stream", st)])
    add(e, "ok")
    add(e, "ok, empty list", wl=ctypes.byref(wl_empty.desc))
    nulls(e, "c", "tensor", "wl")
    add(e, "wl.block=NULL", wl=WL_BAD)
    add(e, "channels=0", channels=0)
    add(e, "ns=3", ns=3)
    add(e, "ns=3+channels=0", ns=3, channels=0)
    e = _Entry(lib, "clear_mask", "scn_clear_mask",
               [("c", h), ("n_slabs", S), ("ns", NS), ("channels", 32), ("tensor", d(q["out"])), ("mask", d(mask)), ("stream", st)])
    add(e, "ok")
    nulls(e, "c", "tensor", "mask")
    slabs(e, cap=False)
    add(e, "channels=0", channels=0)
    add(e, "ns=3", ns=3)
    add(e, "tensor misaligned", tensor=ctypes.c_void_p(q["out"].data_ptr() + 4))
    add(e, "tensor misaligned+n_slabs=0", tensor=ctypes.c_void_p(q["out"].data_ptr() + 4), n_slabs=0)
    return cases, alive


def run_table():
    """key -> status of every call of the table, in table order (also what recorded EXPECTED)."""
    _need_gpu()
    cases, alive = _build()
    got = {k: f() for k, f in cases.items()}
    torch.cuda.synchronize()                       # a launch that should not have happened would surface here
    del alive
    return got


def test_conv_entry_status_codes():
    got = run_table()
    for k, v in got.items():
        print("%-60s %d" % (k, v))
    assert sorted(got) == sorted(EXPECTED), "the table and the recorded codes list different calls: %s" % sorted(set(got) ^ set(EXPECTED))
    not_ok = {k: v for k, v in got.items() if k.split(":")[1].startswith("ok") and v != 0}
    assert not not_ok, "valid calls refused: %s" % not_ok
    wrong = {k: (v, EXPECTED[k]) for k, v in got.items() if v != EXPECTED[k]}
    assert not wrong, "status (got, recorded) differs for %d calls: %s" % (len(wrong), wrong)
