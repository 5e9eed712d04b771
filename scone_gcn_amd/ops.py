"""Device-side operators: thin PyTorch-ROCm plumbing over the C-ABI (device memory, streams) -- no math here.

ConvOp wraps a scn_conv_t; SconePlan / BunchPlan hold everything one model needs on the device and
expose forward / backward over "flow slabs" ([n_slabs, rows, ns, C] fp32, see include/scone_hip.h).
"""
import ctypes
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import ACT, GroupDesc, WorkListDesc, check, i32_array, ptr_array
from .complex import Shift, union_pattern
from .synthetic_data_gen import SparseFlows

NS = 4   # trajectories per slab
Y_STRIDE = 4   # floats per point of the shifted first-layer input y = (x, S_lo x, S_up x, 0)   (include/scone_hip.h)


class KernelTimer:
    """Optional per-call timing with events on the launch stream (torch's current stream), used by bench.py to get
    the average duration of one kernel family live, together with the ALGORITHMIC bytes of every timed call (each operand
    tensor read once, each result written once, the operator's CSR arrays once -- SURVEY.md section 8d).  Disabled by
    default: no events, no overhead.  Timers nest (a stack): every active timer sees the calls made while it is open."""
    _stack = []

    def __init__(self):
        self.records = {}

    def __enter__(self):
        KernelTimer._stack.append(self)
        return self

    def __exit__(self, *a):
        KernelTimer._stack.remove(self)

    def summary(self):
        """key -> (launches, mean ms)."""
        torch.cuda.synchronize()
        return {k: (len(v), sum(a.elapsed_time(b) for a, b, _ in v) / max(len(v), 1)) for k, v in self.records.items()}

    def table(self):
        """key -> {"launches", "avg_ms", "alg_bytes" (mean per launch, None where no model is stated), "GB/s"}.  alg_bytes and GB/s are
        taken over the launches that state a model: a key may mix them with launches that state none (the kept last-layer forward
        shares the key of the layer below it)."""
        torch.cuda.synchronize()
        out = {}
        for k, v in self.records.items():
            t = [a.elapsed_time(b) for a, b, _ in v]
            ms = sum(t) / max(len(v), 1)
            nb = [n for _, _, n in v if n is not None]
            alg = sum(nb) / len(nb) if nb else None
            ms_nb = sum(x for x, (_, _, n) in zip(t, v) if n is not None) / max(len(nb), 1)
            out[k] = {"launches": len(v), "avg_ms": ms, "alg_bytes": alg,
                      "GB/s": (alg / (ms_nb * 1e-3) / 1e9) if (alg and ms_nb > 0) else None}
        return out


class _timed:
    def __init__(self, key, nbytes=None):
        self.key, self.nbytes = key, nbytes

    def __enter__(self):
        if KernelTimer._stack:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *a):
        if KernelTimer._stack:
            self.b.record()
            for t in KernelTimer._stack:
                t.records.setdefault(self.key, []).append((self.a, self.b, self.nbytes))


def _nbytes(*tensors):
    return float(sum(t.numel() * t.element_size() for t in tensors if t is not None))


# Module switches for tests and same-box A/B runs (set them from Python; the one environment variable read here is SCN_SMALL_STEP, once,
# at import).  The first six say how a plain scone stack runs.  They are read ONCE per step, in the forward, by stack_route() below --
# the one place that states where each applies -- and the backward follows the route in the forward's record (TOP_DZ_MASK and
# FUSE_FIRST, which only the backward acts on, included: a switch flipped between a forward and its backward is not seen).  Every one of
# them leaves every output bit as it is; DESIGN.md section 3 says what the kernels behind them do.
FUSE_FIRST = True      # False: separate scn_conv_backward + scn_conv_dw_first instead of the fused-first backward
RECOMPUTE_FIRST = True  # H1 is never stored: layer 1 writes the shifted input y only, layer 2 and its backward rebuild H1 from y.  False: stored
KEEP_LAST = True       # the last layer stores only the (plan block, slab) items the readout reads (the keep mask M0).  False: all of H_L
TOP_DZ_MASK = True     # the top layer's backward stages dZ_L only where hop(M0) is set.  False: the plain backward
READOUT_CONE = True    # every layer runs on the readout's cone M_k = hop^k(M0): kept forwards, visiting backwards.  False: only the top does
CONE_UNIT_LIST = True  # the cone's forward launches take their units from the masks' unit lists.  False: the static walk
# ... and two the library reads at every visiting backward of a cone (_visit_prefetch):
VISIT_PREFETCH = True  # a unit's prologue also fetches the next unit's source rows and first slab.  False: every unit's full prologue
VISIT_RECORDS = True   # a unit's top reads the block's packed 32-byte record.  False: the plan's separate arrays
# ... and one the trainer's micro-batch loop reads (SconePlan.step):
STEP_TAIL = True       # a cone step's readout chain is one launch, and its loss sum, dW reduces and clears one more.  False: nine launches
STEP_MASKS = True      # the cone masks of all of a step's micro-batches come from one launch ahead of the first.  False: five launches each
VISIT_ROWS = True      # ... and that launch also builds the visit masks V_k, the items of M_k a row of P^k R0 lies in, for the step's backwards.  False: M_k
# ... and one the path trainer's staging reads (path_train.py):
PATH_STAGE_SPARSE_CLEAR = True  # a restaged micro-batch buffer resets only the words its previous items wrote.  False: the dense zero fill
UNIT_COUNTERS = 4      # SCN_UNIT_COUNTERS (include/scone_hip.h): counter words behind the mask of scn_keep_mask_units
# Small complexes: the whole gradient step of a micro-batch in one launch (SconePlan.small_step, csrc/scn_small.hip), one workgroup per
# trajectory.  SCN_SMALL_STEP=0 turns it off, =force lifts the rule of small_step_pays() below.  Measured per graph-replayed optimiser
# step, one launch against the layer-by-layer kernels, ms (tools/small_step.py, profiles/r04_small_step_ab.txt):
#   |E| =  319:  160 trajectories 0.053 / 0.110   256: 0.061 / 0.118   512: 0.109 / 0.148   1000: 0.197 / 0.198
#   |E| =  639:  100 trajectories 0.086 / 0.110   256: 0.091 / 0.140   512: 0.163 / 0.197
#   |E| =  822:  100 trajectories 0.097 / 0.115          |E| = 926:  100 trajectories 0.107 / 0.115
#   |E| = 1001:  100 trajectories 0.119 / 0.120   128: 0.121 / 0.122   160: 0.123 / 0.144   256: 0.134 / 0.150   512: 0.242 / 0.193
# One workgroup's chain does not shorten with the batch, so the launch costs (rounds of 256 workgroups) x (chain of this |E|); the layer
# kernels grow with the work.  At |E| = 1001 the chain is eight row tiles per wave and layer: worth it for a full round, not beyond.
# Round 5: above 384 edges and up to CUs / 2 trajectories the library gives every trajectory TWO workgroups (half the row tiles each,
# rows handed over through memory after every layer; include/scone_hip.h), paired / one workgroup each / layer by layer, ms
# (tools/small_pair_ab.sh, profiles/r05_small_pair_ab.txt; the layer kernels themselves are round 5's):
#   |E| =  498:   64 trajectories 0.054 / 0.066 / 0.089   128: 0.057 / 0.068 / 0.100
#   |E| =  639:   64: 0.065 / 0.078 / 0.094   100: 0.067 / 0.079 / 0.101   128: 0.069 / 0.079 / 0.103
#   |E| =  822:   64: 0.069 / 0.091 / 0.097   100: 0.072 / 0.093 / 0.105   128: 0.073 / 0.093 / 0.107
#   |E| = 1001:   32: 0.076 / 0.106 / 0.089    64: 0.079 / 0.107 / 0.102   100: 0.081 / 0.110 / 0.109   128: 0.083 / 0.111 / 0.111
#   |E| = 1106:   64: 0.088 / 0.118 / 0.099   100: 0.093 / 0.119 / 0.121   128: 0.094 / 0.121 / 0.125
# -- wherever that form applies it is the fastest of the three.
SMALL_STEP = os.environ.get("SCN_SMALL_STEP", "1") != "0"
SMALL_STEP_MAX_EDGES = (1 << 30) if os.environ.get("SCN_SMALL_STEP") == "force" else 960     # up to here for any batch of one round


_N_CUS = {}


def device_cus(device=None):
    """Compute units of the device the step runs on (256 on a whole MI355X; fewer on a partitioned one), asked once per device."""
    idx = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    if idx not in _N_CUS:
        _N_CUS[idx] = int(torch.cuda.get_device_properties(idx).multi_processor_count)
    return _N_CUS[idx]


def small_step_pays(n_edges, n_traj, n_cus=256):
    """The size rule for the one-launch step (see the table above); n_traj counts the padded trajectories = workgroups, n_cus the
    device's compute units (callers pass device_cus(); the table was measured on 256)."""
    rounds = -(-n_traj // n_cus)
    if n_edges > 384 and 2 * n_traj <= n_cus:          # two workgroups per trajectory (the library's own condition, small_paired())
        return True
    if n_edges <= min(384, SMALL_STEP_MAX_EDGES):
        return rounds <= 4
    if n_edges <= min(768, SMALL_STEP_MAX_EDGES):
        return rounds <= 2
    if n_edges <= SMALL_STEP_MAX_EDGES:
        return rounds == 1 or (SMALL_STEP_MAX_EDGES >= (1 << 30) and rounds <= 2)
    return rounds == 1 and 2 * n_traj >= n_cus
FUSE_BUNCH = True      # False: per-shift SpMMs + dense-term kernels for every Bunch layer instead of the fused three-level kernels
FOLD_BUNCH = True      # False: the first two Bunch layers as ordinary layers instead of the rank-one fold (BunchPlan._fold_forward)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype=torch.float32):
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), "expected a contiguous CUDA tensor"
    return ctypes.c_void_p(t.data_ptr())


def _ptrs(tensors, dtype=torch.float32):
    """The array-of-device-pointers argument of a call: None entries stay NULL (an absent level or term), a 3 x 3 list of lists goes
    in row by row."""
    if tensors and isinstance(tensors[0], (list, tuple)):
        tensors = [t for row in tensors for t in row]
    return ptr_array([_dev(t, dtype).value if t is not None else None for t in tensors])


def _workspace(nbytes, device, floor=0):
    """The (pointer, size) argument pair of a call's scratch buffer of max(nbytes, floor) bytes; the pointer object keeps the buffer."""
    ws = torch.empty(max(int(nbytes), floor), device=device, dtype=torch.uint8)
    p = ctypes.c_void_p(ws.data_ptr())
    p.buffer = ws
    return p, ws.numel()


def _served(status, name):
    """False when the library does not take the shape (SCN_ERR_UNSUPPORTED: the caller falls back), any other error raises."""
    if status == _lib.SCN_ERR_UNSUPPORTED:
        return False
    check(status, name)
    return True


def _launch(key, nbytes, name, entry, *args, may_decline=False):
    """One launch of a library entry under the timer key `key` with its byte model (None: none stated); `name` is what an error
    message calls it.  may_decline: False where the library does not take the shape (_served) instead of raising."""
    with _timed(key, nbytes):
        status = entry(*args)
    if may_decline:
        return _served(status, name)
    check(status, name)
    return True


def _visit_prefetch(lib):
    """Hands VISIT_PREFETCH to the library ahead of a visiting backward (a build from before the switch has no unit pipeline)."""
    if hasattr(lib, "scn_conv_visit_prefetch"):
        lib.scn_conv_visit_prefetch(1 if VISIT_PREFETCH else 0)
    if hasattr(lib, "scn_conv_visit_records"):
        lib.scn_conv_visit_records(1 if VISIT_RECORDS else 0)


class WorkList:
    """Device copy of a (block, slab) work list of the zero-skipping mode (scn_work_list).  Built from a boolean
    scipy matrix A[slab, block]; `items` counts the (block, slab) pairs."""

    def __init__(self, A, device):
        import scipy.sparse as sp
        At = sp.csr_matrix(A).T.tocsr()                     # rows = blocks, column indices = slabs (ascending)
        At.sort_indices()
        nz = np.flatnonzero(np.diff(At.indptr) > 0)
        ptr = np.concatenate([[0], np.cumsum(np.diff(At.indptr)[nz])]).astype(np.int32)
        # (an empty list still needs valid pointers: pad the arrays with one unused element)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(np.append(a, 0), np.int32)).to(device)
        self.block, self.ptr, self.slab = to(nz), to(ptr), to(At.indices)
        self.n_work, self.items = int(len(nz)), int(At.nnz)
        self.desc = WorkListDesc(self.n_work, self.block.data_ptr(), self.ptr.data_ptr(), self.slab.data_ptr())

    def ref(self):
        return ctypes.byref(self.desc)


class DeviceWorkList:
    """A work list scn_field_lists left on the device: the same ref() / n_work / items as WorkList, over slices of the arrays that
    call filled (block, ptr, slab of one level); n_work and items come from the call's one copy back of its counts."""

    def __init__(self, block, ptr, slab, n_work, items):
        self.block, self.ptr, self.slab = block, ptr, slab
        self.n_work, self.items = int(n_work), int(items)
        self.desc = WorkListDesc(self.n_work, block.data_ptr(), ptr.data_ptr(), slab.data_ptr())

    def ref(self):
        return ctypes.byref(self.desc)


def field_tables(row0, pattern_csr, nbr, inc_ptr, inc_edge):
    """The two block-level CSR tables of the field-of-view lists (scn_field_lists), int32, block indices ascending in every row:
    ((top_ptr, top_blk), (adj_ptr, adj_blk)).
      top: node v -> T(v), the blocks holding a row the readout of v reads = the edges incident to a neighbour of v
           (nbr (V, D) padded with -1; inc_ptr / inc_edge: node -> rows of its incident edges);
      adj: block b -> A(b), the blocks holding a column some row of b has a pattern entry in, b itself included.
    row0: first row of every block and the row count (n_blocks + 1 entries); pattern_csr: the operator's STORED pattern, a scipy
    CSR matrix (explicit zeros count) or (rowptr, cols) -- rows read columns, so a non-symmetric pattern gives a non-symmetric A."""
    import scipy.sparse as sp
    row0 = np.asarray(row0, np.int64)
    nb, E = len(row0) - 1, int(row0[-1])
    blk_of = np.searchsorted(row0, np.arange(E), side="right") - 1
    rowptr, cols = (pattern_csr.indptr, pattern_csr.indices) if hasattr(pattern_csr, "indptr") else pattern_csr
    rowptr, cols = np.asarray(rowptr, np.int64), np.asarray(cols, np.int64)
    assert len(rowptr) == E + 1, "the pattern's rows are the blocks' rows"
    rows = np.repeat(np.arange(E), np.diff(rowptr))
    A = sp.csr_matrix((np.ones(len(rows) + nb, np.int32), (np.concatenate([blk_of[rows], np.arange(nb)]),
                                                         np.concatenate([blk_of[cols], np.arange(nb)]))), shape=(nb, nb))
    nbr, inc_ptr, inc_edge = np.asarray(nbr, np.int64), np.asarray(inc_ptr, np.int64), np.asarray(inc_edge, np.int64)
    V = nbr.shape[0]
    v, j = np.nonzero(nbr >= 0)
    u = nbr[v, j]
    deg = inc_ptr[u + 1] - inc_ptr[u]
    start = np.cumsum(deg) - deg
    pos = np.arange(int(deg.sum())) - np.repeat(start, deg) + np.repeat(inc_ptr[u], deg)     # the incidence ranges of every (v, u), in a row
    T = sp.csr_matrix((np.ones(len(pos), np.int32), (np.repeat(v, deg), blk_of[inc_edge[pos]])), shape=(V, nb))
    out = []
    for M in (T, A):
        M.sum_duplicates()
        M.sort_indices()
        out.append((np.ascontiguousarray(M.indptr, np.int32), np.ascontiguousarray(M.indices, np.int32)))
    return tuple(out)


VISIT_TABLES_MAX_WORK = 1 << 30    # multiplies of one sparse product of visit_tables (the benchmark's largest: 1.1e8); also keeps ptr in int32


def visit_tables(row0, pattern_csr, nbr, inc_ptr, inc_edge, hops, max_work=None):
    """The node -> blocks tables of the visit masks (scn_cone_masks_visits), int32 CSR pairs like `top` of field_tables, block indices
    ascending in every row: [(ptr, blk) of T_k for k = 1 .. hops], T_k(v) = the blocks holding a row of R_k(v) = P^k rows(v).
      rows(v): the rows behind T(v) of field_tables -- the edges incident to a neighbour of v, where the readout's backward writes;
      P:       the STORED pattern with the diagonal, rows read columns as in `adj`: R_k = R_{k-1} and every row with an entry in a column
               of R_{k-1} -- where the gather of the backward k layers down from the readout can be non-zero (symmetric shifts).
    T_k(v) is a subset of A^k(T(v)) by construction.  Sparse products, node by node through the incidence lists: rows(v) is the union
    of its neighbours' incidence ranges and P^k distributes over it, so the row-level product runs once per node, not once per pair.
    Arguments as field_tables.  None where a product would take more than max_work multiplies (default VISIT_TABLES_MAX_WORK):
    the caller then has no visit masks and the backwards visit M_k."""
    import scipy.sparse as sp
    max_work = VISIT_TABLES_MAX_WORK if max_work is None else max_work
    row0 = np.asarray(row0, np.int64)
    nb, E = len(row0) - 1, int(row0[-1])
    blk_of = np.searchsorted(row0, np.arange(E), side="right") - 1
    rowptr, cols = (pattern_csr.indptr, pattern_csr.indices) if hasattr(pattern_csr, "indptr") else pattern_csr
    rowptr, cols = np.asarray(rowptr, np.int64), np.asarray(cols, np.int64)
    assert len(rowptr) == E + 1, "the pattern's rows are the blocks' rows"
    rows = np.repeat(np.arange(E), np.diff(rowptr))
    # PT[c, r] != 0: row r reads column c (or r == c)
    PT = sp.csr_matrix((np.ones(len(rows) + E, np.int32), (np.concatenate([cols, np.arange(E)]), np.concatenate([rows, np.arange(E)]))),
                       shape=(E, E))
    PT.data[:] = 1
    B = sp.csr_matrix((np.ones(E, np.int32), (np.arange(E), blk_of)), shape=(E, nb))
    nbr, inc_ptr, inc_edge = np.asarray(nbr, np.int64), np.asarray(inc_ptr, np.int64), np.asarray(inc_edge, np.int64)
    V, U = nbr.shape[0], len(inc_ptr) - 1
    v, j = np.nonzero(nbr >= 0)
    N = sp.csr_matrix((np.ones(len(v), np.int32), (v, nbr[v, j])), shape=(V, U))
    X = sp.csr_matrix((np.ones(int(inc_ptr[U]), np.int32), (np.repeat(np.arange(U), np.diff(inc_ptr)), inc_edge[:inc_ptr[U]])),
                      shape=(U, E))                      # node u -> its incident edges, then hop by hop
    # every product is bounded BEFORE it is formed: its multiplies -- an upper bound of its entries -- are the left factor's entries
    # weighted by the right factor's row lengths.  An operator with a hub row makes P^2 dense; the tables are then refused, not built.
    work = lambda A, Bm: int(np.diff(Bm.indptr)[A.indices].sum())          # noqa: E731
    out = []
    for _ in range(hops):
        if work(X, PT) > max_work:
            return None
        X = (X @ PT).tocsr()
        X.data[:] = 1                                   # (a pattern: the counts would only grow)
        XB = (X @ B).tocsr()                            # (one block per row: no more entries than X)
        if work(N, XB) > max_work:
            return None
        T = (N @ XB).tocsr()
        T.sum_duplicates()
        T.sort_indices()
        out.append((np.ascontiguousarray(T.indptr, np.int32), np.ascontiguousarray(T.indices, np.int32)))
    return out


def visit_masks_host(nodes, ns, tables, n_blocks):
    """NumPy restatement of the visit masks of scn_cone_masks_visits (include/scone_hip.h): [V_1 .. V_hops], V_k = keep_mask_host
    against T_k of `tables` (visit_tables)."""
    return [keep_mask_host(nodes, ns, ptr, blk, n_blocks) for ptr, blk in tables]


def keep_mask_host(nodes, ns, top_ptr, top_blk, n_blocks):
    """NumPy restatement of scn_keep_mask (include/scone_hip.h): uint32 [n_blocks][ceil(n_slabs / 32)], bit s & 31 of word
    [b][s >> 5] set iff a leaf i of slab s = i // ns has block b in T(nodes[i]).  A node outside the table contributes nothing, nor
    does a block outside [0, n_blocks)."""
    nodes = np.asarray(nodes, np.int64)
    n_slabs = -(-len(nodes) // ns)
    mask = np.zeros((n_blocks, (n_slabs + 31) // 32), np.uint32)
    for i, v in enumerate(nodes):
        if 0 <= v < len(top_ptr) - 1:
            s = i // ns
            blk = np.asarray(top_blk[top_ptr[v]:top_ptr[v + 1]], np.int64)
            mask[blk[(blk >= 0) & (blk < n_blocks)], s >> 5] |= np.uint32(1 << (s & 31))
    return mask


def mask_hop_host(mask, adj_ptr, adj_blk):
    """NumPy restatement of scn_mask_hop (include/scone_hip.h): out[b] = OR of mask[b'] over b' in A(b) = adj_blk[adj_ptr[b] :
    adj_ptr[b + 1]], word by word.  A block outside the mask's rows contributes nothing."""
    mask = np.asarray(mask, np.uint32)
    out = np.zeros_like(mask)
    for b in range(mask.shape[0]):
        src = np.asarray(adj_blk[adj_ptr[b]:adj_ptr[b + 1]], np.int64)
        src = src[(src >= 0) & (src < mask.shape[0])]
        if len(src):
            out[b] = np.bitwise_or.reduce(mask[src], axis=0)
    return out


def cone_masks_host(nodes_list, ns, top_ptr, top_blk, adj_ptr, adj_blk, n_blocks, L):
    """NumPy restatement of scn_cone_masks (include/scone_hip.h): for every micro-batch's last nodes in nodes_list the tuple
    (masks, lists, counters) -- masks[k] = M_k, M0 = keep_mask_host, M_k = mask_hop_host(M_{k-1}); lists[k] = the indices b * words + w
    of the non-zero words of M_k, ascending; counters = their lengths for k < L and 0 behind, UNIT_COUNTERS words."""
    assert 1 <= L <= UNIT_COUNTERS
    out = []
    for nodes in nodes_list:
        masks = [keep_mask_host(nodes, ns, top_ptr, top_blk, n_blocks)]
        for _ in range(1, L):
            masks.append(mask_hop_host(masks[-1], adj_ptr, adj_blk))
        lists = [np.flatnonzero(m.reshape(-1)).astype(np.uint32) for m in masks]
        counters = np.zeros(UNIT_COUNTERS, np.uint32)
        counters[:L] = [len(u) for u in lists]
        out.append((masks, lists, counters))
    return out


def cone_masks_limit():
    """Words of one mask scn_cone_masks takes at most (the library's SCN_CONE_MASKS_MAX_WORDS: one mask in a workgroup's LDS)."""
    return int(_lib.load().scn_cone_masks_max_words())


class UnitList(NamedTuple):
    """The unit list of a keep mask (include/scone_hip.h, "Unit lists"): every non-empty word of the mask once, in no particular order."""
    units: object       # int32 [n_blocks * words] device buffer; entry = block * words + word
    count: object       # int32 [1] device: the number of entries


# The reduces a visiting backward leaves to ConvOp.step_epilogue (defer=): its layer's and, fused-first, the first layer's.  partial: device
# address of the per-workgroup partials; dWs: the three gradients summed into; ws: the launch's workspace, which keeps the partials alive.
ReduceJob = NamedTuple("ReduceJob", [("partial", int), ("n_wg", int), ("c_aux", int), ("c_dz", int), ("dWs", list), ("ws", object)])
FirstReduceJob = NamedTuple("FirstReduceJob", [("partial", int), ("n_wg", int), ("dWs", list), ("ws", object)])


class ZeroPool(dict):
    """{shape: [fp32 buffers]} of a plan.  A buffer in the pool is all-zero: whoever gives one back has wiped what was written into it
    (ConvOp.clear, clear_mask, scn_readout_clear_dz, the step epilogue), so a taker writes only the rows it needs.  The one exception: a
    readout gradient of at most SconePlan.SMALL_DZ_BYTES goes back as it is, and _readout_grad, its only taker, has it zeroed in the launch."""

    def __init__(self, device):
        self.device = device

    def take(self, like, zeroed=True):
        shape = tuple(getattr(like, "shape", like))     # (a shape or a tensor; zeroed=False: a fresh buffer is left uninitialised)
        return self[shape].pop() if self.get(shape) else (torch.zeros if zeroed else torch.empty)(shape, device=self.device, dtype=torch.float32)

    def give(self, t):
        self.setdefault(tuple(t.shape), []).append(t)


def deferred_clears(L):
    """Layers of an L-layer cone whose gradient buffer a step leaves for its epilogue to wipe: those with no layer below that takes a pooled
    buffer again -- layer j >= 2 takes one for its dx, layer 1 writes none: layers 2 and 1 -- so the pool's peak stays the separate calls'."""
    return set(range(1, min(L, 3)))


def _unit_ptrs(units):
    return (_dev(units.units, torch.int32), _dev(units.count, torch.int32)) if units is not None else (None, None)


class FieldTables(NamedTuple):
    """Device copies of field_tables for one plan."""
    n_blocks: int
    top_ptr: object
    top_blk: object
    adj_ptr: object
    adj_blk: object


class VisitTables(NamedTuple):
    """Device copies of visit_tables for one plan: ptr[k - 1], blk[k - 1] = T_k."""
    ptr: list
    blk: list


class ConvOp:
    """One shift-convolution operator (scn_conv_t).  groups: list of dicts
    {"mats": [scipy csr in DEVICE order] (0..2, same shape), "identity": bool, "n_cols": int}."""

    def __init__(self, n_rows, groups, block_start=None):
        lib = _lib.load()
        self.n_rows = int(n_rows)
        self.group_cols = []
        self.slot_group = []
        descs = (GroupDesc * len(groups))()
        keep = []
        for gi, g in enumerate(groups):
            mats = g["mats"]
            n_cols = int(g["n_cols"])
            if mats:
                rowptr, cols, vals = union_pattern(mats)
            else:
                rowptr, cols, vals = np.zeros(n_rows + 1, np.int32), np.zeros(0, np.int32), []
            rowptr = np.ascontiguousarray(rowptr, np.int32)
            cols = np.ascontiguousarray(cols, np.int32)
            vals = [np.ascontiguousarray(v, np.float32) for v in vals]
            keep += [rowptr, cols] + vals
            d = descs[gi]
            d.n_cols, d.identity, d.n_vals, d.nnz = n_cols, int(bool(g.get("identity"))), len(vals), len(cols)
            d.rowptr = rowptr.ctypes.data
            d.col = cols.ctypes.data if len(cols) else None
            d.val0 = vals[0].ctypes.data if len(vals) > 0 and len(cols) else None
            d.val1 = vals[1].ctypes.data if len(vals) > 1 and len(cols) else None
            self.group_cols.append(n_cols)
            self.slot_group += [gi] * (d.identity + d.n_vals)
        h = ctypes.c_void_p()
        if block_start is not None:                # layout hint that goes with the row order (Layout.block_starts)
            block_start = np.ascontiguousarray(block_start, np.uint8)
            assert len(block_start) == self.n_rows
            keep.append(block_start)
        check(lib.scn_conv_create_blocked(self.n_rows, len(groups), descs,
                                          block_start.ctypes.data if block_start is not None else None, ctypes.byref(h)),
              "scn_conv_create")
        self.handle = h
        self.n_groups = len(groups)
        self.n_slots = len(self.slot_group)
        self.nnz = [int(descs[g].nnz) for g in range(len(groups))]
        self.n_vals = [int(descs[g].n_vals) for g in range(len(groups))]
        # column indices + every value array + row pointers, once per launch
        self.csr_bytes = float(sum(4 * self.nnz[g] * (1 + self.n_vals[g]) + 4 * (self.n_rows + 1) for g in range(len(groups))))
        del keep

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().scn_conv_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def plan_info(self):
        nb, ms = ctypes.c_int32(0), ctypes.c_float(0)
        check(_lib.load().scn_conv_plan_info(self.handle, ctypes.byref(nb), ctypes.byref(ms)), "scn_conv_plan_info")
        return nb.value, ms.value

    def keep_mask(self, nodes, ns, n_nodes, tabs, key="keep_mask"):
        """The keep mask of a last layer's forward (scn_keep_mask): int32 words [n_blocks][ceil(n_slabs / 32)], bit (b, s) set iff a
        leaf of slab s stands on a node whose readout reads a row of plan block b.  nodes: int32 device tensor, one per trajectory;
        tabs: the plan's FieldTables.  A fresh buffer per call, filled on the current stream (nothing is kept on the operator).
        key: the timer's name of the launch (the top layer's backward builds the same mask under its own)."""
        n = nodes.numel()
        words = (-(-n // ns) + 31) // 32
        mask = torch.empty((tabs.n_blocks, words), device=nodes.device, dtype=torch.int32)
        _launch(key, _nbytes(mask, nodes), "scn_keep_mask", _lib.load().scn_keep_mask, n, ns, _dev(nodes, torch.int32), n_nodes,
                _dev(tabs.top_ptr, torch.int32), _dev(tabs.top_blk, torch.int32), tabs.n_blocks, _dev(mask, torch.int32), _stream())
        return mask

    def mask_hop(self, mask, tabs):
        """One hop out from a keep_mask() over the plan's block adjacency (scn_mask_hop): bit (b, s) set iff a block that b's rows
        stage has its bit set in `mask` -- the source mask of the top layer's backward.  A fresh buffer per call, as keep_mask."""
        out = torch.empty_like(mask)
        _launch("dz_mask_hop", _nbytes(mask, out), "scn_mask_hop", _lib.load().scn_mask_hop, tabs.n_blocks, mask.shape[1],
                _dev(tabs.adj_ptr, torch.int32), _dev(tabs.adj_blk, torch.int32), _dev(mask, torch.int32), _dev(out, torch.int32), _stream())
        return out

    def keep_mask_units(self, nodes, ns, n_nodes, tabs, key="keep_mask"):
        """keep_mask() that also writes the mask's unit list (scn_keep_mask_units): returns (mask, UnitList, counters).  The mask and
        UNIT_COUNTERS counter words behind it are ONE fresh buffer that the call's one memset clears; counters[0] is this list's
        count, counters[1:] are zero for the lists of the masks hopped from this one (mask_hop_units).  The entries are a fresh
        buffer per call too: nothing is kept on the operator, two forwards never share a list."""
        n = nodes.numel()
        words = (-(-n // ns) + 31) // 32
        n_words = tabs.n_blocks * words
        buf = torch.empty(n_words + UNIT_COUNTERS, device=nodes.device, dtype=torch.int32)
        mask, counters = buf[:n_words].view(tabs.n_blocks, words), buf[n_words:]
        units = torch.empty(n_words, device=nodes.device, dtype=torch.int32)
        _launch(key, _nbytes(mask, nodes), "scn_keep_mask_units", _lib.load().scn_keep_mask_units, n, ns, _dev(nodes, torch.int32), n_nodes,
                _dev(tabs.top_ptr, torch.int32), _dev(tabs.top_blk, torch.int32), tabs.n_blocks, _dev(mask, torch.int32),
                _dev(units, torch.int32), units.numel(), _stream())
        return mask, UnitList(units, counters[0:1]), counters

    def mask_hop_units(self, mask, tabs, counter):
        """mask_hop() that also writes the unit list of its result (scn_mask_hop_units): returns (out, UnitList).  counter: one int32
        device word that is zero (keep_mask_units hands them out)."""
        out = torch.empty_like(mask)
        units = torch.empty(mask.numel(), device=mask.device, dtype=torch.int32)
        _launch("dz_mask_hop", _nbytes(mask, out), "scn_mask_hop_units", _lib.load().scn_mask_hop_units, tabs.n_blocks, mask.shape[1],
                _dev(tabs.adj_ptr, torch.int32), _dev(tabs.adj_blk, torch.int32), _dev(mask, torch.int32), _dev(out, torch.int32),
                _dev(units, torch.int32), _dev(counter, torch.int32), units.numel(), _stream())
        return out, UnitList(units, counter)

    def cone_masks(self, last_devs, ns, n_nodes, tabs, L, visit_tabs=None):
        """The cones of several micro-batches in ONE launch (scn_cone_masks): for every int32 device tensor of last nodes in last_devs a
        Cone [M0 .. M_{L-1}] with every mask's UnitList, as keep_mask_units() and L - 1 mask_hop_units() build them (the lists
        ascending).  Masks, entries and counters are views into three fresh allocations of this call, none of them filled: the launch
        writes every mask word and every counter.  No memset, no host read.  None where the library declines (L above UNIT_COUNTERS, a
        mask above cone_masks_limit() words): nothing was launched.
        visit_tabs (VisitTables of at least L - 1 hops, L >= 2): the same launch also writes the visit masks (scn_cone_masks_visits), a
        fourth fresh allocation: Cone.visits = [None, V_1 .. V_{L-1}]."""
        n_mb = len(last_devs)
        words = [(-(-t.numel() // ns) + 31) // 32 for t in last_devs]
        n_words = [tabs.n_blocks * w for w in words]
        stride = -(-max(n_words) // 128) * 128                  # (every mask and list starts on 512 bytes, as an allocation of its own does)
        dev = last_devs[0].device
        masks = torch.empty((n_mb * L, stride), device=dev, dtype=torch.int32)
        units = torch.empty((n_mb * L, stride), device=dev, dtype=torch.int32)
        counters = torch.empty((n_mb * UNIT_COUNTERS, 1), device=dev, dtype=torch.int32)
        desc = (_lib.ConeMb * n_mb)()
        m0, u0, c0 = masks.data_ptr(), units.data_ptr(), counters.data_ptr()
        for i, t in enumerate(last_devs):
            d = desc[i]
            d.node, d.n, d.stride = _dev(t, torch.int32).value, t.numel(), stride
            d.masks, d.units, d.counters = m0 + 4 * i * L * stride, u0 + 4 * i * L * stride, c0 + 4 * UNIT_COUNTERS * i
        # bytes: every mask and counter written, the last nodes read, and per micro-batch the block adjacency once for each hop
        nb = 4.0 * L * sum(n_words) + _nbytes(counters, *last_devs) + n_mb * (L - 1) * _nbytes(tabs.adj_ptr, tabs.adj_blk)
        head = (n_mb, desc)
        tail = (ns, n_nodes, tabs.n_blocks, _dev(tabs.top_ptr, torch.int32), _dev(tabs.top_blk, torch.int32),
                _dev(tabs.adj_ptr, torch.int32), _dev(tabs.adj_blk, torch.int32), L)
        visits = None
        if visit_tabs is not None and L >= 2:
            assert len(visit_tabs.ptr) >= L - 1
            visits = torch.empty((n_mb * (L - 1), stride), device=dev, dtype=torch.int32)
            v0 = visits.data_ptr()
            nb += 4.0 * (L - 1) * sum(n_words)            # (every visit mask written; the tables' rows of the last nodes are not modelled)
            if not _launch("cone_masks", nb, "scn_cone_masks_visits", _lib.load().scn_cone_masks_visits, *head,
                           ptr_array([v0 + 4 * i * (L - 1) * stride for i in range(n_mb)]), *tail,
                           _ptrs(visit_tabs.ptr[:L - 1], torch.int32), _ptrs(visit_tabs.blk[:L - 1], torch.int32), _stream(),
                           may_decline=True):
                return None
        elif not _launch("cone_masks", nb, "scn_cone_masks", _lib.load().scn_cone_masks, *head, *tail, _stream(), may_decline=True):
            return None
        # the views, a few tensor calls for all of them (host time ahead of a step's first launch): row i * L + k of the buffers is
        # mask / list k of micro-batch i, row i * (L - 1) + k - 1 of `visits` is V_k
        rows = {w: (masks[:, :tabs.n_blocks * w].unflatten(1, (tabs.n_blocks, w)).unbind(0), units[:, :tabs.n_blocks * w].unbind(0),
                    visits[:, :tabs.n_blocks * w].unflatten(1, (tabs.n_blocks, w)).unbind(0) if visits is not None else None)
                for w in set(words)}
        count = counters.unbind(0)
        cones = []
        for i in range(n_mb):
            m, u, v = rows[words[i]]
            cone = Cone(m[i * L:(i + 1) * L])
            cone.units = [UnitList(u[i * L + k], count[i * UNIT_COUNTERS + k]) for k in range(L)]
            if v is not None:
                cone.visits = [None] + list(v[i * (L - 1):(i + 1) * (L - 1)])
            cones.append(cone)
        return cones

    def clear_mask(self, t, mask):
        """+0 over the (block, slab) items of a [S, rows, ns, C] tensor whose bit is set in `mask` (scn_clear_mask)."""
        _launch("clear_mask", None, "scn_clear_mask", _lib.load().scn_clear_mask, self.handle, t.shape[0], t.shape[2], t.shape[3], _dev(t),
                _dev(mask, torch.int32), _stream())

    def forward(self, srcs, Ws, c_out, act, out=None, wl=None, partial=None, keep=None, units=None):
        """wl: WorkList (zero-skipping): only the listed items of `out` are written; `out` must be given, all-zero.
        partial: tensor of the output's shape added to the pre-activation (scn_conv_forward_accumulate; out defaults to it, in place).
        keep: keep_mask() of the launch (last layer, dense): only the kept (block, slab) items of `out` are written, the rest of it
        holds whatever the buffer held; None when the shape is not served (scn_conv_forward_keep).
        units: the UnitList of `keep`: the workgroups take their units from it, with the same results (scn_conv_forward_keep_units)."""
        lib = _lib.load()
        assert wl is None or out is not None
        assert keep is None or (wl is None and partial is None)
        assert units is None or keep is not None
        if partial is not None:
            assert wl is None and tuple(partial.shape) == (srcs[0].shape[0], self.n_rows, srcs[0].shape[2], c_out)
            out = partial if out is None else out
        S, ns = srcs[0].shape[0], srcs[0].shape[2]
        assert len(srcs) == self.n_groups and len(Ws) == self.n_slots
        c_in = []
        for g, x in enumerate(srcs):
            assert x.shape[0] == S and x.shape[1] == self.group_cols[g] and x.shape[2] == ns, "source slab shape"
            c_in.append(x.shape[3])
        for s, w in enumerate(Ws):
            assert tuple(w.shape) == (c_in[self.slot_group[s]], c_out), "weight shape"
        if out is None:
            out = torch.empty((S, self.n_rows, ns, c_out), device=srcs[0].device, dtype=torch.float32)
        key = "conv_fwd c%s->%d" % ("+".join(map(str, c_in)), c_out)
        head = (self.handle, S, ns, _ptrs(srcs), i32_array(c_in), _ptrs(Ws), c_out, ACT[act])
        if partial is not None:
            _launch(key + " + partial", _nbytes(out, partial, *srcs) + self.csr_bytes, "scn_conv_forward_accumulate",
                    lib.scn_conv_forward_accumulate, *head, _dev(partial), _dev(out), _stream())
        elif keep is not None:
            # (the key of the plain forward.  32 channels: no byte model -- the launch moves the staged rows and the stored rows of the
            # KEPT items only, and their count is on the device; pricing it at the input tensor would print a rate above the HBM
            # peak.  16 channels: every tile is still staged, the input tensor is the model)
            if not _launch(key, None if c_in[0] == 32 else _nbytes(*srcs) + self.csr_bytes, "scn_conv_forward_keep",
                           lib.scn_conv_forward_keep_units, *head, _dev(out), _dev(keep, torch.int32), *_unit_ptrs(units), _stream(),
                           may_decline=True):
                return None
        else:
            _launch(key, None if wl is not None else _nbytes(out, *srcs) + self.csr_bytes, "scn_conv_forward",
                    lib.scn_conv_forward_list, *head, _dev(out), wl.ref() if wl is not None else None, _stream())
        return out

    def backward(self, dzs, Ws, aux, act, need_dx, dWs, dx=None, wl=None, dx_partial=None, dz_mask=None, visit=None, defer=None):
        """dWs: list of tensors ACCUMULATED into.  Returns dx or None.  wl: WorkList (zero-skipping): only the listed
        items of `dx` are written (it must be given, all-zero) and only they contribute to dWs.
        dx_partial: tensor of dx's shape ADDED to the input gradient (scn_conv_backward_accumulate; dx defaults to it, in place).
        dz_mask: mask_hop() of the keep mask outside whose items dzs[0] is all-zero (top layer, dense): dz is staged only where the
        mask is set, with the plain call's results; returns False (nothing launched, dWs untouched) when the shape is not served
        (scn_conv_backward_dzmask).
        visit: a mask V one hop out from a mask outside whose items dzs[0] is all-zero: only V's items are visited, with the plain
        call's dWs and its dx on V; `dx` must be given and every other row of it is left as it is; False when not served
        (scn_conv_backward_visit).
        defer (with visit): a list -- the launch leaves its weight-gradient partials in its workspace and appends their ReduceJob
        for step_epilogue (scn_conv_backward_visit_partial)."""
        lib = _lib.load()
        assert wl is None or (dx is not None or not need_dx)
        assert dz_mask is None or (wl is None and dx_partial is None)
        assert visit is None or (wl is None and dx_partial is None and dz_mask is None and (dx is not None or not need_dx))
        if dx_partial is not None:
            assert wl is None and need_dx and tuple(dx_partial.shape) == tuple(aux.shape)
            dx = dx_partial if dx is None else dx
        S, ns, c_aux = aux.shape[0], aux.shape[2], aux.shape[3]
        assert aux.shape[1] == self.n_rows and len(dzs) == self.n_groups
        c_dz = []
        for g, x in enumerate(dzs):
            assert x.shape[0] == S and x.shape[1] == self.group_cols[g] and x.shape[2] == ns, "dz slab shape"
            c_dz.append(x.shape[3])
        for s, (w, dw) in enumerate(zip(Ws, dWs)):
            assert tuple(w.shape) == (c_aux, c_dz[self.slot_group[s]]) and tuple(dw.shape) == tuple(w.shape)
        cdz = i32_array(c_dz)
        ws = _workspace(lib.scn_conv_backward_workspace(self.handle, S, ns, cdz, c_aux), aux.device, 256)
        if need_dx and dx is None:
            dx = torch.empty_like(aux)
        key = "conv_bwd c%s->%d" % ("+".join(map(str, c_dz)), c_aux)
        head = (self.handle, S, ns, _ptrs(dzs), cdz, _ptrs(Ws), _dev(aux), c_aux, ACT[act])
        if dx_partial is not None:
            _launch(key + " + partial", _nbytes(aux, dx, dx_partial, *dzs) + self.csr_bytes, "scn_conv_backward_accumulate",
                    lib.scn_conv_backward_accumulate, *head, _dev(dx_partial), _dev(dx), _ptrs(dWs), *ws, _stream())
            return dx
        # (the three forms below share the plain backward's key)
        key += "" if need_dx else " (dW only)"
        tail = (_dev(dx) if need_dx else None, _ptrs(dWs), *ws)
        if dz_mask is not None:                       # (the staged items are left out of the byte model, as the kept stores of the forward are)
            if not _launch(key, _nbytes(dx if need_dx else None) + self.csr_bytes, "scn_conv_backward_dzmask",
                           lib.scn_conv_backward_dzmask, *head, *tail, _dev(dz_mask, torch.int32), _stream(), may_decline=True):
                return False
        elif visit is not None and defer is not None:
            _visit_prefetch(lib)
            n_wg = ctypes.c_int32(0)
            if not _launch(key, None, "scn_conv_backward_visit_partial", lib.scn_conv_backward_visit_partial, *head,
                           _dev(dx) if need_dx else None, *ws, _dev(visit, torch.int32), ctypes.byref(n_wg), _stream(), may_decline=True):
                return False
            defer.append(ReduceJob(ws[0].value, n_wg.value, c_aux, c_dz[0], dWs, ws))
        elif visit is not None:                       # (no byte model: the visited items' count is on the device)
            _visit_prefetch(lib)
            if not _launch(key, None, "scn_conv_backward_visit",
                           lib.scn_conv_backward_visit, *head, *tail, _dev(visit, torch.int32), _stream(), may_decline=True):
                return False
        else:
            _launch(key, None if wl is not None else _nbytes(aux, dx if need_dx else None, *dzs) + self.csr_bytes, "scn_conv_backward",
                    lib.scn_conv_backward_list, *head, *tail, wl.ref() if wl is not None else None, _stream())
        return dx if need_dx else None

    def forward_first(self, x, Ws, c_out, act, out=None, y=None, wl=None):
        """First layer (one 1-channel input): returns (out, y) with y = (x, S_lo x, S_up x, 0) per point, or None when the
        shape is not served (scn_conv_forward_first).  wl: as in forward (out and y given, all-zero)."""
        lib = _lib.load()
        S, rows, ns, c_in = x.shape
        if c_in != 1 or self.n_groups != 1 or self.n_slots != 3:
            return None
        assert wl is None or (out is not None and y is not None)
        if out is None:
            out = torch.empty((S, self.n_rows, ns, c_out), device=x.device, dtype=torch.float32)
        if y is None:
            y = torch.empty((S, self.n_rows, ns, Y_STRIDE), device=x.device, dtype=torch.float32)
        ok = _launch("conv_fwd c1->%d" % c_out, None if wl is not None else _nbytes(x, out) + self.csr_bytes, "scn_conv_forward_first",
                     lib.scn_conv_forward_first, self.handle, S, ns, _dev(x), _ptrs(Ws), c_out, ACT[act], _dev(out), _dev(y),
                     wl.ref() if wl is not None else None, _stream(), may_decline=True)
        return (out, y) if ok else None

    def shifted_input(self, x, keep=None, units=None):
        """y = (x, S_lo x, S_up x, 0) per point of a 1-channel input WITHOUT the first layer's output (scn_conv_forward_first with
        out = NULL); None when the shape is not served.  keep: only the kept (block, slab) items of y are written, the rest of it is
        uninitialised memory (scn_conv_shifted_input_keep).  units: the UnitList of `keep`, as in forward."""
        lib = _lib.load()
        S, rows, ns, c_in = x.shape
        if c_in != 1 or self.n_groups != 1 or self.n_slots != 3:
            return None
        y = torch.empty((S, self.n_rows, ns, Y_STRIDE), device=x.device, dtype=torch.float32)
        if keep is not None:                          # (no byte model, see forward)
            ok = _launch("conv_fwd c1->y", None, "scn_conv_shifted_input_keep", lib.scn_conv_shifted_input_keep_units,
                         self.handle, S, ns, _dev(x), _dev(y), _dev(keep, torch.int32), *_unit_ptrs(units), _stream(), may_decline=True)
        else:
            dummy = _ptrs([x] * 3)                    # (the weights are not read without an output; the call checks them for NULL)
            ok = _launch("conv_fwd c1->y", _nbytes(x, y) + self.csr_bytes, "scn_conv_forward_first", lib.scn_conv_forward_first,
                         self.handle, S, ns, _dev(x), dummy, 32, ACT["none"], None, _dev(y), None, _stream(), may_decline=True)
        return y if ok else None

    def forward_from_y(self, y, Ws_first, Ws, act, keep=None, out=None, units=None):
        """The layer AFTER a 1-channel first layer from that layer's shifted input y and weights Ws_first: act(sum_s (S_s H1) Ws[s]) with
        H1 rebuilt inside the kernel (scn_conv_forward_from_y); None when the shape is not served.  keep: as in forward
        (scn_conv_forward_from_y_keep); units: the UnitList of `keep`, as in forward."""
        lib = _lib.load()
        S, rows, ns, _ = y.shape
        c = Ws[0].shape[1]
        if self.n_groups != 1 or self.n_slots != 3 or rows != self.n_rows or any(tuple(w.shape) != (c, c) for w in Ws) or \
                any(tuple(w.shape) != (1, c) for w in Ws_first):
            return None
        if out is None:
            out = torch.empty((S, self.n_rows, ns, c), device=y.device, dtype=torch.float32)
        # (the key of the plain C -> C forward: the same kernel family, and what callers that look for the fused layer kernels expect;
        # the launch is told apart by its neighbour "conv_fwd c1->y" and by its byte model: y in, not H1)
        key = "conv_fwd c%d->%d" % (c, c)
        head = (self.handle, S, ns, _dev(y), _ptrs(Ws_first), _ptrs(Ws), c, ACT[act], _dev(out))
        if keep is not None:                          # (no byte model, see forward)
            ok = _launch(key, None, "scn_conv_forward_from_y_keep", lib.scn_conv_forward_from_y_keep_units,
                         *head, _dev(keep, torch.int32), *_unit_ptrs(units), _stream(), may_decline=True)
        else:
            ok = _launch(key, _nbytes(y, out) + self.csr_bytes, "scn_conv_forward_from_y", lib.scn_conv_forward_from_y,
                         *head, _stream(), may_decline=True)
        return out if ok else None

    def forward_power(self, x0, x, Ws, act):
        """out = act(x0 W0 + x W1 + (S x) W2) for an operator with identity + one value array (scn_conv_forward_power);
        None when the shape is not served."""
        lib = _lib.load()
        S, rows, ns, c = x.shape
        out = torch.empty_like(x)
        ok = _launch("conv_fwd_power c%d" % c, _nbytes(x0, x, out) + self.csr_bytes, "scn_conv_forward_power", lib.scn_conv_forward_power,
                     self.handle, S, ns, _dev(x0), _dev(x), _ptrs(Ws), c, ACT[act], _dev(out), _stream(), may_decline=True)
        return out if ok else None

    def backward_power(self, dz, g1, Ws, aux, act, need_dx, dWs):
        """Backward of forward_power given g1 = S^T dz (scn_conv_backward_power); returns (served, dx)."""
        lib = _lib.load()
        S, rows, ns, c = dz.shape
        nbytes = int(lib.scn_conv_backward_power_workspace(self.handle, S, ns, c))
        if nbytes == 0:
            return False, None
        ws = _workspace(nbytes, dz.device)
        dx = torch.empty_like(aux) if need_dx else None
        _launch("conv_bwd_power c%d" % c, _nbytes(dz, g1, aux, dx) + self.csr_bytes, "scn_conv_backward_power", lib.scn_conv_backward_power,
                self.handle, S, ns, _dev(dz), _dev(g1), _ptrs(Ws), _dev(aux), c, ACT[act], _dev(dx) if need_dx else None, _ptrs(dWs), *ws,
                _stream())
        return True, dx

    def backward_fused_first(self, dz, Ws, aux, act, y, dWs, dWs_first, wl=None, Ws_first=None, visit=None, defer=None):
        """Backward of the layer after the first one, fused with the first layer's weight gradient: dWs (this layer) and
        dWs_first are accumulated, the input gradient is never written (scn_conv_backward_fused_first).  False when the shape
        is not served.  aux = None with Ws_first (the first layer's weights): the first layer's output is rebuilt from y
        inside the kernel instead of being read (scn_conv_backward_fused_first_from_y, 32 channels).  visit (with Ws_first, dense): as
        in backward (scn_conv_backward_fused_first_from_y_visit).  defer (with visit): a list that takes the launch's ReduceJob and
        FirstReduceJob, as in backward (scn_conv_backward_fused_first_from_y_visit_partial)."""
        lib = _lib.load()
        S, rows, ns, c = dz.shape
        if (aux is not None and tuple(aux.shape) != (S, rows, ns, c)) or tuple(y.shape) != (S, rows, ns, Y_STRIDE) or self.n_groups != 1:
            return False
        if aux is None and (Ws_first is None or c != 32):
            return False
        nbytes = int(lib.scn_conv_backward_fused_first_workspace(self.handle, S, ns, c))
        if nbytes == 0:
            return False
        ws = _workspace(nbytes, dz.device)
        key = "conv_bwd c%d->%d + dW_first" % (c, c)
        head = (self.handle, S, ns, _dev(dz), _ptrs(Ws))
        tail = (c, ACT[act], _dev(y), _ptrs(dWs), _ptrs(dWs_first), *ws)
        if visit is not None:
            if aux is not None or wl is not None:
                return False
            _visit_prefetch(lib)
            if defer is not None:
                n_wg = ctypes.c_int32(0)
                if not _launch(key, None, "scn_conv_backward_fused_first_from_y_visit_partial",
                               lib.scn_conv_backward_fused_first_from_y_visit_partial, *head, _ptrs(Ws_first), c, ACT[act], _dev(y), *ws,
                               _dev(visit, torch.int32), ctypes.byref(n_wg), _stream(), may_decline=True):
                    return False
                defer.append(ReduceJob(ws[0].value, n_wg.value, c, c, dWs, ws))
                defer.append(FirstReduceJob(ws[0].value + 4 * n_wg.value * 3 * c * c, n_wg.value, dWs_first, ws))   # (behind n_wg x 3 x c x c floats)
                return True
            return _launch(key, None, "scn_conv_backward_fused_first_from_y_visit", lib.scn_conv_backward_fused_first_from_y_visit,
                           *head, _ptrs(Ws_first), *tail, _dev(visit, torch.int32), _stream(), may_decline=True)
        wl_ref = wl.ref() if wl is not None else None
        if aux is None:
            return _launch(key, None if wl is not None else _nbytes(dz, y) + self.csr_bytes, "scn_conv_backward_fused_first_from_y",
                           lib.scn_conv_backward_fused_first_from_y, *head, _ptrs(Ws_first), *tail, wl_ref, _stream())
        return _launch(key, None if wl is not None else _nbytes(dz, aux, y) + self.csr_bytes, "scn_conv_backward_fused_first",
                       lib.scn_conv_backward_fused_first, *head, _dev(aux), *tail, wl_ref, _stream())

    def step_epilogue(self, loss, readout_dw, jobs, clears, readout_args):
        """All of a cone step that nothing waits for before the micro-batch ends, in ONE launch (scn_step_epilogue; under the masked clear's
        timer key, which it does, with no byte model as there).  loss = (logp, y, scale, out, overwrite): out[0] (fp64) += scale * <logp, y>,
        or = with overwrite; readout_dw = (d_logits, bh, dW): the readout's weight gradient, added to dW; jobs: what the deferred backwards
        left; clears: (tensor, mask) pairs, each wiped as clear_mask does -- mask None: a readout gradient, wiped as scn_readout_clear_dz
        does by readout_args = SconePlan._readout_args(last nodes, sign=False, edge_nodes=True), which is not looked at without one."""
        d = _lib.StepEpilogueDesc()
        ptr = lambda t, dtype=torch.float32: _dev(t, dtype).value
        logp, y, scale, out, overwrite = loss
        d.loss_n, d.logp, d.y, d.scale, d.loss, d.overwrite = logp.numel(), ptr(logp), ptr(y), float(scale), out.data_ptr(), 1 if overwrite else 0
        d_logits, bh, dW = readout_dw
        d.rd_nd, d.rd_c, d.rd_dl, d.rd_bh, d.rd_d_w = d_logits.numel(), bh.shape[2], ptr(d_logits), ptr(bh), ptr(dW)
        for job in jobs:
            if isinstance(job, ReduceJob):
                q = d.reduce[d.n_reduce]
                q.partial, q.n_wg, q.c_aux, q.c_dz, q.dW[:] = job.partial, job.n_wg, job.c_aux, job.c_dz, [ptr(t) for t in job.dWs]
                d.n_reduce += 1
            else:
                d.first_form, d.first_partial, d.first_n_wg, d.first_dW[:] = 1, job.partial, job.n_wg, [ptr(t) for t in job.dWs]
        for t, mask in clears:
            if mask is None:
                nbr, _, d.rc_max_deg, last, inc_ptr, inc_edge, nodes = readout_args
                d.rc_dz, (d.rc_n_slabs, d.rc_n_edges, d.rc_ns, d.rc_c) = ptr(t), t.shape
                d.rc_nbr, d.rc_last_nodes, d.rc_inc_ptr, d.rc_inc_edge, d.rc_edge_nodes = (p.value for p in (nbr, last, inc_ptr, inc_edge, nodes))
            else:
                d.clear[d.n_clear] = _lib.EpiClear(ptr(t), ptr(mask, torch.int32), t.shape[0], t.shape[2], t.shape[3])
                d.n_clear += 1
        _launch("clear_mask", None, "scn_step_epilogue", _lib.load().scn_step_epilogue, self.handle, ctypes.byref(d), _stream())

    def clear(self, t, wl):
        """Zero the listed items of a [S, rows, ns, C] tensor (scn_clear_list)."""
        check(_lib.load().scn_clear_list(self.handle, t.shape[2], t.shape[3], _dev(t), wl.ref(), _stream()), "scn_clear_list")

    def plan_blocks(self):
        nb = self.plan_info()[0]
        row0 = np.zeros(nb + 1, np.int32)
        check(_lib.load().scn_conv_plan_blocks(self.handle, row0.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
              "scn_conv_plan_blocks")
        return row0

    def window_scan_probe(self, mask, n_slabs, grid_x, slab0, n_it):
        """Diagnostic (scn_window_scan_probe): what each of grid_x workgroups of a masked launch would visit for the slab range
        [slab0, slab0 + n_it) of `mask` (int32 words [n_blocks][ceil(n_slabs / 32)]).  Returns (sequences, unit_block): sequences[g] =
        [(plan block, window), ...] of workgroup g in visiting order (window: bit j = slab slab0 + j, never zero), unit_block = the
        launch's unit -> block table (NumPy int32 [n_blocks])."""
        nb = self.plan_info()[0]
        cap = max(1, -(-(-(-nb // 8) + 1) // max(1, grid_x // 8)))   # units of a workgroup: its XCD's share over grid_x / 8, rounded up
        dev = mask.device
        blk = torch.full((grid_x, cap), -1, device=dev, dtype=torch.int32)
        win = torch.zeros((grid_x, cap), device=dev, dtype=torch.int64)
        cnt = torch.full((grid_x,), -1, device=dev, dtype=torch.int32)
        ub = torch.full((nb,), -1, device=dev, dtype=torch.int32)
        check(_lib.load().scn_window_scan_probe(self.handle, n_slabs, _dev(mask, torch.int32), grid_x, slab0, n_it, cap, _dev(blk, torch.int32),
                                                _dev(win, torch.int64), _dev(cnt, torch.int32), _dev(ub, torch.int32), _stream()),
              "scn_window_scan_probe")
        torch.cuda.synchronize()
        blk, win, cnt = blk.cpu().numpy(), win.cpu().numpy().view(np.uint64), cnt.cpu().numpy()
        assert int(cnt.min()) >= 0 and int(cnt.max()) <= cap, "a workgroup's sequence is longer than its units"
        return [[(int(blk[g, i]), int(win[g, i])) for i in range(cnt[g])] for g in range(grid_x)], ub.cpu().numpy()

    def dw_first_served(self, dz):
        """Whether dw_first takes this gradient tensor's shape (scn_conv_dw_first_workspace > 0)."""
        S, rows, ns, c = dz.shape
        return rows == self.n_rows and int(_lib.load().scn_conv_dw_first_workspace(self.handle, S, ns, c)) > 0

    def dw_first(self, x, y, dz, dWs, wl=None):
        """First-layer weight gradient through the forward operator (scn_conv_dw_first); y: the shifted input saved by
        forward_first (or None: recomputed from x).  False if the shape is not served."""
        lib = _lib.load()
        S, rows, ns, c = dz.shape
        assert rows == self.n_rows and (y is None or tuple(y.shape) == (S, rows, ns, Y_STRIDE))
        nbytes = int(lib.scn_conv_dw_first_workspace(self.handle, S, ns, c))
        if nbytes == 0:
            return False
        ws = _workspace(nbytes, dz.device)
        return _launch("conv_dw_first c%d" % c, None if wl is not None else _nbytes(dz) + 4.0 * S * rows * ns + self.csr_bytes,
                       "scn_conv_dw_first", lib.scn_conv_dw_first, self.handle, S, ns, _dev(x) if x is not None else None,
                       _dev(y) if y is not None else None, _dev(dz), c, _ptrs(dWs), *ws, wl.ref() if wl is not None else None, _stream())

    def spmm_dual(self, x, dual=True):
        lib = _lib.load()
        S, rows, k = x.shape
        assert rows == self.group_cols[0]
        ya = torch.empty((S, self.n_rows, k), device=x.device, dtype=torch.float32)
        yb = torch.empty_like(ya) if dual else None
        _launch("spmm_dual k%d" % k if dual else "spmm k%d" % k, _nbytes(x, ya, yb) + self.csr_bytes, "scn_spmm_dual", lib.scn_spmm_dual,
                self.handle, S, k, _dev(x), _dev(ya), _dev(yb) if dual else None, _stream())
        return ya, yb


class TermsOp:
    """The seven Bunch shifts of one direction as ONE operator on the concatenated row space [nodes | edges | faces]
    (scn_terms_create): blocks[(l, j)] = the shift (device order) from source level j to target level l, or absent."""

    def __init__(self, sizes, blocks, merged, bins, rows_per_wave):
        import scipy.sparse as sp
        lib = _lib.load()
        self.sizes = tuple(int(x) for x in sizes)
        self.bins = tuple(int(b) for b in bins)
        off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        grid = [[blocks.get((l, j)) for j in range(3)] for l in range(3)]
        for l in range(3):
            for j in range(3):
                if grid[l][j] is None:
                    grid[l][j] = sp.csr_matrix((self.sizes[l], self.sizes[j]))
        M = sp.bmat(grid, format="csr")
        M.sort_indices()
        R = int(off[3])
        rowptr = np.ascontiguousarray(M.indptr, np.int32)
        col = np.ascontiguousarray(M.indices, np.int32)
        val = np.ascontiguousarray(M.data, np.float32)
        term = ((col >= off[1]).astype(np.uint8) + (col >= off[2]).astype(np.uint8)).astype(np.uint8)
        lvl = np.ascontiguousarray(off, np.int32)
        if merged is None:                                     # no common curve known: level by level
            merged = np.concatenate([np.full(n, l, np.uint8) for l, n in enumerate(self.sizes)])
        merged = np.ascontiguousarray(merged, np.uint8)
        assert len(merged) == R
        binsa = np.ascontiguousarray(self.bins, np.int32)
        h = ctypes.c_void_p()
        check(lib.scn_terms_create(R, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, term.ctypes.data, lvl.ctypes.data,
                                   merged.ctypes.data, binsa.ctypes.data, int(rows_per_wave), ctypes.byref(h)), "scn_terms_create")
        self.handle = h
        self.nnz = int(M.nnz)
        self.csr_bytes = 4.0 * self.nnz * 2 + 4.0 * (R + 1)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().scn_conv_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def plan_info(self):
        nb, ms = ctypes.c_int32(0), ctypes.c_float(0)
        check(_lib.load().scn_conv_plan_info(self.handle, ctypes.byref(nb), ctypes.byref(ms)), "scn_conv_plan_info")
        return nb.value, ms.value

    def forward(self, xs, Ws, act, want):
        """xs[j]: level tensors [S, rows_j, ns, 32] or None (identically zero); Ws[l][j]: (32, 32) tensors or None; want[l]:
        compute level l.  Returns the list of outputs (None where not wanted)."""
        lib = _lib.load()
        ref = next(x for x in xs if x is not None)
        S, ns = ref.shape[0], ref.shape[2]
        outs = [torch.empty((S, self.sizes[l], ns, 32), device=ref.device, dtype=torch.float32) if want[l] else None
                for l in range(3)]
        nb = _nbytes(*[x for x in xs if x is not None], *[o for o in outs if o is not None]) + self.csr_bytes
        with _timed("terms_fwd c32", nb):
            check(lib.scn_terms_forward(self.handle, S, ns, _ptrs(xs), _ptrs(Ws), 32, ACT[act], _ptrs(outs), _stream()), "scn_terms_forward")
        return outs


def _terms_backward(op, dzs, Ws, auxs, act, want_dx, dWs):
    """TermsOp.backward (kept a function so the class above stays forward-only readable): dzs[j] / auxs[l] level tensors or
    None, Ws[l][j] / dWs[l][j] (32, 32) tensors or None, want_dx[l].  Returns the list of input gradients (None where not wanted)."""
    lib = _lib.load()
    ref = next(x for x in dzs if x is not None)
    S, ns = ref.shape[0], ref.shape[2]
    dxs = [torch.empty((S, op.sizes[l], ns, 32), device=ref.device, dtype=torch.float32) if want_dx[l] else None for l in range(3)]
    nbytes = int(lib.scn_terms_backward_workspace(op.handle, S, ns, 32))
    assert nbytes > 0, "terms backward not served"
    ws = _workspace(nbytes, ref.device)
    nb = _nbytes(*[x for x in dzs if x is not None], *[x for x in auxs if x is not None], *[x for x in dxs if x is not None]) + op.csr_bytes
    with _timed("terms_bwd c32", nb):
        check(lib.scn_terms_backward(op.handle, S, ns, _ptrs(dzs), _ptrs(Ws), _ptrs(auxs), 32, ACT[act], _ptrs(dxs), _ptrs(dWs), *ws,
                                     _stream()), "scn_terms_backward")
    return dxs


def _terms_backward_first(op, dzs, Ws, auxs, act, ys, dWs, dWs_first):
    """_terms_backward for the layer that follows the 1-channel first layer: no input gradients come back -- they are contracted
    with the first layer's shifted input ys[l] (S, rows_l, ns, 1) into dWs_first[l] (1, 32) inside the kernel
    (scn_terms_backward_fused_first)."""
    lib = _lib.load()
    ref = next(x for x in dzs if x is not None)
    S, ns = ref.shape[0], ref.shape[2]
    nbytes = int(lib.scn_terms_backward_workspace(op.handle, S, ns, 32))
    assert nbytes > 0, "terms backward not served"
    ws = _workspace(nbytes, ref.device)
    nb = _nbytes(*[x for x in dzs if x is not None], *[x for x in auxs if x is not None], *[x for x in ys if x is not None]) + op.csr_bytes
    with _timed("terms_bwd c32 + dW_first", nb):
        check(lib.scn_terms_backward_fused_first(op.handle, S, ns, _ptrs(dzs), _ptrs(Ws), _ptrs(auxs), 32, ACT[act], _ptrs(ys), _ptrs(dWs),
                                                 _ptrs(dWs_first), *ws, _stream()), "scn_terms_backward_fused_first")


def _pairable(widths, ns):
    """All widths 16: two consecutive points are one 32-channel point under block-diagonal weights diag(W, W), which is the
    shape the MFMA dense-term kernels take (the same trick as the paired C=16 convolution kernels)."""
    return ns % 2 == 0 and all(int(c) == 16 for c in widths)


DENSE_FWD_LDS = 64 * 1024      # scn_dense_terms_forward: bytes of LDS its weight matrices may take
DENSE_BWD_WW = 1024            # scn_dense_terms_backward: c_aux * c_k it serves (one 32 x 32 weight-gradient tile per term)


def dense_terms_forward(Gs, Ws, c_out, act):
    """out[p,:] = act(sum_k G_k[p,:] @ W_k) over slab tensors [S, rows, ns, c_k] (scn_dense_terms_forward)."""
    lib = _lib.load()
    S, R, ns = Gs[0].shape[:3]
    if _pairable([g.shape[3] for g in Gs] + [c_out], ns):
        out = dense_terms_forward([g.view(S, R, ns // 2, 32) for g in Gs], [torch.block_diag(w, w) for w in Ws], 32, act)
        return out.view(S, R, ns, 16)
    cins = [g.shape[3] for g in Gs]
    if max(cins + [c_out]) > 32 and c_out % 32 == 0 and all(c % 32 == 0 for c in cins):
        # widths above 32 (multiples of 32: promotion pads to them) as 32 x 32 blocks on the MFMA kernel -- the partial
        # pre-activations of an output block add up in scn_sum_act; the VALU kernel took 85 ms for one 64-wide launch at |E| = 1M
        nb_in = max(cins) // 32
        blocks = [[g if c == 32 else g[..., 32 * b:32 * b + 32].contiguous() for b in range(c // 32)] for g, c in zip(Gs, cins)]
        outs = []
        for j in range(c_out // 32):
            parts = []
            for b in range(nb_in):
                sel = [k for k, c in enumerate(cins) if c > 32 * b]
                parts.append(dense_terms_forward([blocks[k][b] for k in sel],
                                                 [Ws[k][32 * b:32 * b + 32, 32 * j:32 * j + 32].contiguous() for k in sel], 32,
                                                 act if nb_in == 1 else "none"))
            outs.append(parts[0] if len(parts) == 1 else sum_act(parts, act))
        return torch.cat(outs, dim=3)
    if 4 * c_out * sum(cins) > DENSE_FWD_LDS and c_out > 32:
        # the kernel keeps every W_k in LDS (64 KB): wider outputs run as column blocks of 32 (independent: no sums)
        return torch.cat([dense_terms_forward(Gs, [w[:, c0:c0 + 32].contiguous() for w in Ws], min(32, c_out - c0), act)
                          for c0 in range(0, c_out, 32)], dim=3)
    out = torch.empty((S, R, ns, c_out), device=Gs[0].device, dtype=torch.float32)
    with _timed("dense_fwd x%d ->%d" % (len(Gs), c_out), _nbytes(out, *Gs)):
        check(lib.scn_dense_terms_forward(S * R * ns, len(Gs), _ptrs(Gs), i32_array(cins), _ptrs(Ws), c_out, ACT[act], _dev(out), _stream()),
              "scn_dense_terms_forward")
    return out


def dense_terms_backward(Gs, Ws, aux, act, need_dx, dWs):
    lib = _lib.load()
    S, R, ns, c_aux = aux.shape
    if _pairable([g.shape[3] for g in Gs] + [c_aux], ns):
        wide = [torch.zeros((32, 32), device=aux.device, dtype=torch.float32) for _ in Gs]
        dx = dense_terms_backward([g.view(S, R, ns // 2, 32) for g in Gs], [torch.block_diag(w, w) for w in Ws],
                                  aux.view(S, R, ns // 2, 32), act, need_dx, wide)
        for d, w in zip(dWs, wide):                       # the two diagonal blocks of the virtual 32x32 gradient
            d.add_(w[:16, :16] + w[16:, 16:])
        return dx.view(S, R, ns, 16) if need_dx else None
    if any(c_aux * g.shape[3] > DENSE_BWD_WW for g in Gs) and max(c_aux, max(g.shape[3] for g in Gs)) > 1:
        return _dense_terms_backward_blocks(Gs, Ws, aux, act, need_dx, dWs)
    cs = i32_array([g.shape[3] for g in Gs])
    n_points = S * R * ns
    ws = _workspace(lib.scn_dense_terms_backward_workspace(n_points, len(Gs), cs, c_aux), aux.device, 256)
    dx = torch.empty_like(aux) if need_dx else None
    with _timed("dense_bwd x%d" % len(Gs), _nbytes(aux, dx, *Gs)):
        check(lib.scn_dense_terms_backward(n_points, len(Gs), _ptrs(Gs), cs, _ptrs(Ws), _dev(aux), c_aux, ACT[act],
                                           _dev(dx) if need_dx else None, _ptrs(dWs), *ws, _stream()), "scn_dense_terms_backward")
    return dx


# ----------------------------------------------------------------------------------------------
# slabs
# ----------------------------------------------------------------------------------------------

def pad_count(n, ns=NS):
    return (n + ns - 1) // ns * ns


def flows_to_slabs(flow, layout, device, ns=NS):
    """(N, E, 1) dense array/tensor or SparseFlows (caller's edge order) -> [S, E, ns, 1] in device row order."""
    lib = _lib.load()
    perm = layout.perm[1]
    if isinstance(flow, SparseFlows):
        N, E = len(flow), flow.n_edges
        S = pad_count(N, ns) // ns
        x = torch.empty((S, E, ns, 1), device=device, dtype=torch.float32)
        sample = np.repeat(np.arange(N, dtype=np.int32), np.diff(flow.ptr))
        sample_d = torch.from_numpy(sample).to(device)
        edge_d = torch.from_numpy(perm[flow.idx].astype(np.int32)).to(device)
        val_d = torch.from_numpy(np.ascontiguousarray(flow.val, np.float32)).to(device)
        check(lib.scn_scatter_flows(S, ns, E, len(sample), _dev(sample_d, torch.int32), _dev(edge_d, torch.int32),
                                    _dev(val_d), _dev(x), _stream()), "scn_scatter_flows")
        return x, N
    t = torch.as_tensor(flow)
    N, E = t.shape[0], t.shape[1]
    assert t.numel() == N * E, "flows must have one input channel (STM:261)"
    t = t.reshape(N, E).to(device=device, dtype=torch.float32)
    Np = pad_count(N, ns)
    if Np != N:
        t = torch.cat([t, t.new_zeros((Np - N, E))])
    order = torch.from_numpy(layout.order[1]).to(device)
    x = t.index_select(1, order).reshape(Np // ns, ns, E).permute(0, 2, 1).contiguous().unsqueeze(-1)
    return x, N


def slabs_to_batch(x, layout, level, n):
    """[S, rows, ns, C] (device order) -> (n, rows, C) in the caller's order (debug / tests)."""
    S, R, ns, C = x.shape
    perm = torch.from_numpy(layout.perm[level]).to(x.device)
    return x.permute(0, 2, 1, 3).reshape(S * ns, R, C)[:n].index_select(1, perm)


def batch_to_slabs(t, layout, level, ns=NS):
    """(N, rows, C) caller order -> [S, rows, ns, C] device order."""
    N, R, C = t.shape
    Np = pad_count(N, ns)
    if Np != N:
        t = torch.cat([t, t.new_zeros((Np - N, R, C))])
    order = torch.from_numpy(layout.order[level]).to(t.device)
    return t.index_select(1, order).reshape(Np // ns, ns, R, C).permute(0, 2, 1, 3).contiguous()


def remap_last_nodes(plan, last_nodes):
    """Last nodes as the plan's readout tables index them: the caller's node ids for a Bconds object; for a probed
    Bcond_func closure (complex.ProbedBconds) the rows of its table, probing nodes it has not seen yet."""
    bc = getattr(plan, "bconds", None)
    if bc is not None and hasattr(bc, "prepare"):
        ln = bc.prepare(last_nodes)
        plan.sync_readout()
        return ln
    return last_nodes


def _last_nodes_dev(last_nodes, n_pad, device):
    ln = np.zeros(n_pad, np.int32)
    a = last_nodes.detach().cpu().numpy() if torch.is_tensor(last_nodes) else np.asarray(last_nodes)
    ln[:len(a)] = a
    return torch.from_numpy(ln).to(device)


def _dense_terms_backward_blocks(Gs, Ws, aux, act, need_dx, dWs):
    """dense_terms_backward beyond the kernel's widths (c_aux * c_k > 1024): aux in channel blocks of <= 32 (independent: the
    block's rows of every W_k and dW_k), and where a term is wider than 32 its channels in blocks of 32 as well -- the partial
    input gradients of an aux block, each already times act'(aux), add up (scn_sum_act).  W_k: (c_aux, c_k)."""
    c_aux = aux.shape[3]
    cmax = max(g.shape[3] for g in Gs)
    kb = -(-cmax // 32) if cmax > 32 else 1             # channel blocks of the widest term
    dxs = []
    for a0 in range(0, c_aux, 32):
        a1 = min(c_aux, a0 + 32)
        aux_a = aux[..., a0:a1].contiguous()
        parts = []
        for j in range(kb):
            sel = [(k, 32 * j, min(g.shape[3], 32 * j + 32)) for k, g in enumerate(Gs) if g.shape[3] > 32 * j] if kb > 1 else \
                  [(k, 0, g.shape[3]) for k, g in enumerate(Gs)]
            if not sel:
                continue
            Gj = [Gs[k] if (c0 == 0 and c1 == Gs[k].shape[3]) else Gs[k][..., c0:c1].contiguous() for k, c0, c1 in sel]
            Wj = [Ws[k][a0:a1, c0:c1].contiguous() for k, c0, c1 in sel]
            dWj = [torch.zeros_like(w) for w in Wj]
            parts.append(dense_terms_backward(Gj, Wj, aux_a, act, need_dx, dWj))
            for (k, c0, c1), d in zip(sel, dWj):
                dWs[k][a0:a1, c0:c1] += d
        if need_dx:
            dxs.append(parts[0] if len(parts) == 1 else sum_act(parts, "none"))
    return torch.cat(dxs, dim=3) if need_dx else None


def spmm_chunked(op, x):
    """y = S x for a slab tensor x (S, R, ns, c) of ANY width: the LDS-blocked SpMM takes ns * c <= 128 columns per launch, wider
    operands go through it in channel blocks (the shift acts on every channel alike)."""
    S, R, ns, c = x.shape
    step = max(1, 128 // ns)
    if c <= step:
        y, _ = op.spmm_dual(x.view(S, R, ns * c), dual=False)
        return y.view(S, op.n_rows, ns, c)
    outs = []
    for c0 in range(0, c, step):
        w = min(step, c - c0)
        y, _ = op.spmm_dual(x[..., c0:c0 + w].contiguous().view(S, R, ns * w), dual=False)
        outs.append(y.view(S, op.n_rows, ns, w))
    return torch.cat(outs, dim=3)


# ----------------------------------------------------------------------------------------------
# hidden-width promotion
# ----------------------------------------------------------------------------------------------
# The MFMA kernels serve hidden widths 16 (on slab pairs) and 32.  Any other stack the reference documents -- mixed widths such
# as `-hidden_layers [(3, 32), (3, 16)]` (TE:51) or 3_8_3_8 (TE:82) -- runs on the SAME kernels with every hidden width
# zero-padded to one promoted width: no layer of this path has a bias and act(0) = 0 for every activation it uses, so the padded
# channels are exactly zero in every activation and every gradient, the real channels see the same sums (the extra terms
# are exact zeros), and the padded rows / columns of the weight gradients are dropped again on the way out.

WIDE_MAX = 128        # widest hidden layer served by the 32-channel-block decomposition (SconePlan._wide_stack)


def promoted_width(widths, wide=False):
    """Width every hidden layer is padded to, or None when the stack runs as it is (uniform 16 or 32; wider than 32 unless
    `wide`: then the next multiple of 32 up to WIDE_MAX -- such a stack runs in 32-channel blocks)."""
    ws = {int(c) for c in widths}
    if len(ws) == 1 and ws <= {16, 32}:
        return None
    m = max(ws)
    if m > 32:
        return -(-m // 32) * 32 if (wide and m <= WIDE_MAX) else None
    return 16 if m <= 16 else 32


def sum_act(terms, act, out=None):
    """out = act(terms[0] + terms[1] + ...) elementwise (scn_sum_act; out defaults to terms[0], in place)."""
    out = terms[0] if out is None else out
    check(_lib.load().scn_sum_act(out.numel(), len(terms), _ptrs(terms), ACT[act], _dev(out), _stream()),
          "scn_sum_act")
    return out


def promote_weights(weights, n_first, n_last, P):
    """Zero-padded copies: rows of every matrix but the first layer's n_first, columns of every matrix but the last n_last."""
    out, n = [], len(weights)
    for i, w in enumerate(weights):
        r = w.shape[0] if i < n_first else P
        c = w.shape[1] if i >= n - n_last else P
        out.append(w if (r, c) == tuple(w.shape) else torch.nn.functional.pad(w, (0, c - w.shape[1], 0, r - w.shape[0])).contiguous())
    return out


def demote_grads(grads, padded):
    for g, gp in zip(grads, padded):
        if gp is not g:
            g.add_(gp[:g.shape[0], :g.shape[1]])


# ----------------------------------------------------------------------------------------------
# what the callers ask of either plan family; what a forward hands its backward
# ----------------------------------------------------------------------------------------------

class Plan:
    """Common to SconePlan / PowerPlan / BunchPlan.  Each has forward(x, last_dev, weights) -> (logp, saved record), _backward of that
    record, promotion(weights) and n_rows = the rows of one trajectory's activation (all levels), which the micro-batch rule prices."""
    weights_per_layer = None      # 3 (scone / ebli: identity, lower, upper) or 7 (the Bunch shifts)

    def backward(self, saved, logp, d_logp, last_dev, weights, grads):
        """grads: list of tensors (same shapes as weights) accumulated into."""
        wp = saved.promoted
        if wp is None:
            return self._backward(saved, logp, d_logp, last_dev, weights, grads)
        gp = [torch.zeros_like(w) if w is not w0 else g for w, w0, g in zip(wp, weights, grads)]
        self._backward(saved, logp, d_logp, last_dev, wp, gp)      # gradients of the padded matrices, cut back afterwards
        demote_grads(grads, gp)
        return grads

    def layer_widths(self, weights):
        """[1, width of layer 1, ...] of a weight list (or the list of its shapes) as this plan runs it: with the promoted width in
        place of every hidden width where the stack is promoted."""
        shapes = _shapes(weights)
        k = self.weights_per_layer
        widths = [1] + [int(shapes[k * i][1]) for i in range(len(shapes) // k)]
        P = self.promotion(shapes)
        return [w if w == 1 else P for w in widths] if P else widths


def _shapes(weights):
    return [tuple(getattr(w, "shape", w)) for w in weights]


class SconeState(NamedTuple):
    """SconePlan / PowerPlan.forward -> backward / release."""
    hs: list            # [x, H_1 .. H_L]; H_1 is None where it is rebuilt from y0; wide: every entry the list of its 32-channel blocks.
                        # H_L has its full shape, but where the forward ran with a keep mask (ops.KEEP_LAST) only the (plan block, slab)
                        # items the readout of this forward's last nodes reads were written: every other row is uninitialised memory
    bh: object          # the readout's gathered rows (wide: one per block of H_L)
    y0: object          # the first layer's shifted input, or None
    activity: object    # work lists of the zero-skipping mode, or None
    promoted: object    # the zero-padded weights the stack ran on, or None
    wide: bool          # hidden widths above 32 ran in 32-channel blocks (_wide_stack / _wide_backward)
    cone: object = None  # ops.READOUT_CONE: the masks [M0 .. M_{L-1}] the forward ran on (layer l kept on M_{L-l}, y0 on M_{L-1}: every
                         # other row of hs[2:] and y0 is uninitialised memory), which the backward visits by; None: the stack ran in full
    route: object = None  # the StackRoute the forward ran by, which the backward follows; None: wide, PowerPlan


class Cone(list):
    """The masks [M0 .. M_{L-1}] of a readout's cone (SconeState.cone).  units: where the forward took its units from lists
    (ops.CONE_UNIT_LIST), units[k] = the UnitList of M_k (None: M_k has none); None otherwise.  They belong to this forward's record
    as the masks do: fresh buffers, shared with no other forward on the plan.
    visits: where the step's mask launch also built them (ops.VISIT_ROWS), visits[k] = V_k, the items of M_k holding a row the backward k
    layers down from the readout can gather a non-zero into (k >= 1; visits[0] is None): what that backward visits and what its dx is
    wiped on, in place of M_k.  None otherwise."""
    units = None
    visits = None


class StackRoute(NamedTuple):
    """How one step of a plain scone stack runs: filled once per forward by stack_route(), kept in SconeState.route, followed by the
    backward.  Every route computes the same bits."""
    first: str            # layers 1 and 2.  "from_y": layer 1 writes the shifted input y only, layer 2 and its backward rebuild H1 from y
                          # (hs[1] is None); "stored": forward_first stores H1 and y; "plain": an ordinary layer, no y (no 1-channel input)
    keep_last: bool       # the last layer's forward runs kept on M0, the keep mask of the last nodes
    cone: bool            # every layer runs on the readout's cone [M0 .. M_{L-1}]: kept forwards, visiting backwards, masked clears
    units: bool           # ... and the cone's forward launches take their units from the masks' lists
    top_dz_mask: bool     # off the cone, the top layer's backward stages dZ_L by hop(M0), rebuilt from the last nodes
    fused_first: bool     # layer 2's backward also sums the first layer's weight gradient from y (always after "from_y")

    def fallback(self):
        """The route to try where the library declines a launch of this one: the cone gives way to the stack in full, "from_y" to a
        stored H1.  (A kept last layer that is declined is rerun plainly on the spot: conv_stack.)"""
        if self.cone:
            return self._replace(cone=False, units=False)
        assert self.first == "from_y", "only a cone or a from-y pair can be declined"
        return self._replace(first="stored")


def stack_route(x_shape, w_shapes, *, activity, last_dev, fused_conv, symmetric, blocked, tables, tables_built, capturing,
                keep_last_min, small_dz, cone_min):
    """The StackRoute of one forward from plain facts (no tensor is touched, nothing is launched): the shapes of x and of the weights
    the stack runs on (promoted ones where it is promoted); activity: work lists are given; last_dev: (count, dtype) of the last
    nodes or None; fused_conv, symmetric (conv_T is conv), blocked: the plan's operator; tables: the plan has field tables (none for
    a probed closure), tables_built: already, capturing: the stream is under a graph capture; the three SconePlan bounds, each against
    its own tensor.  The module switches are read here, now."""
    S, E, ns, c_in = x_shape
    shapes = [tuple(s) for s in w_shapes]
    L = (len(shapes) - 1) // 3
    last = shapes[-2] if L >= 2 else None          # the last layer's weights, where it is not also the first
    # every form but the stored one: the plain scone plan on its blocked operator, dense launches, slabs of NS trajectories
    base = bool(fused_conv and blocked and not activity and ns == NS)
    from_y = (base and RECOMPUTE_FIRST and FUSE_FIRST and c_in == 1 and L >= 2
              and shapes[:-1] == [(1, 32)] * 3 + [(32, 32)] * (3 * (L - 1)))
    # M0 can be built: one int32 last node per trajectory, and the node -> blocks table (built on the host at first use: not under a capture)
    m0 = base and last_dev == (S * ns, torch.int32) and bool(tables) and (tables_built or not capturing)
    keep_last = m0 and KEEP_LAST and last in ((32, 32), (16, 16)) and S * E * ns * last[1] * 4 > keep_last_min      # H_L at its own width
    dz32 = S * E * ns * 32 * 4                     # a 32-channel gradient buffer; at or below small_dz the readout's backward zeroes it itself
    # (symmetric shifts: the plan's block adjacency is the forward operator's)
    top_dz_mask = m0 and TOP_DZ_MASK and symmetric and L >= 3 and last == (32, 32) and dz32 > small_dz
    # the cone: where both are served on a stack without a stored H1, at most 64 slabs (every masked launch is served whatever its grid)
    cone = keep_last and top_dz_mask and from_y and READOUT_CONE and S <= 64 and dz32 > cone_min
    return StackRoute(first="from_y" if from_y else "stored" if c_in == 1 else "plain", keep_last=keep_last, cone=cone,
                      units=cone and CONE_UNIT_LIST, top_dz_mask=top_dz_mask, fused_first=FUSE_FIRST and c_in == 1)


class BunchState(NamedTuple):
    """BunchPlan.forward -> backward."""
    states: list        # per layer boundary the three level tensors (None: not computed)
    zeros: list         # ... and which of them are identically zero
    first_g: dict       # slot k -> S_k x of the 1-channel input, where the first layer ran per shift
    fold: object        # slot k2 -> (S_k2 g^+, S_k2 g^-, k1) of the rank-one fold of the first two layers, or None
    promoted: object    # the zero-padded weights the stack ran on, or None


# ----------------------------------------------------------------------------------------------
# scone / ebli
# ----------------------------------------------------------------------------------------------

class SconePlan(Plan):
    """Device state of a scone/ebli model: the fused conv operator (identity + S_lower + S_upper on their shared
    pattern), its transpose when the shifts are not symmetric, and the readout tables."""
    weights_per_layer = 3
    fused_conv = True             # identity + both shifts as ONE operator (self.conv): what the recompute-first and wide stacks run on

    def __init__(self, S_lower, S_upper, bconds, act, device):
        assert isinstance(S_lower, Shift) and isinstance(S_upper, Shift), "shifts must come from SimplicialComplex"
        self.layout = S_lower.layout
        self.act = act
        self.device = device
        E = S_lower.shape[0]
        self.n_edges = self.n_rows = E
        self._init_operators(S_lower, S_upper)
        self.bconds = bconds
        self._dz_zero, self._zero_pool = ZeroPool(device), ZeroPool(device)    # readout gradients and a cone's dx; the zero-skipping mode's
        self._blocks = None                             # (block of row, block adjacency), built on first use
        self._act_cache = None                          # _trajectory_supports of the last data set
        self._field = None                              # device copies of field_tables, built on first use (field_tables_dev)
        self._visit = None                              # device copies of visit_tables, built on first use (visit_tables_dev)
        self._upload_readout()

    def _upload_readout(self):
        """Device copies of the readout tables (TE:279, 288, 298-303).  A ProbedBconds (plain Bcond_func closure) grows as
        new last nodes are probed: sync_readout() re-uploads when its version has moved."""
        bconds, device = self.bconds, self.device
        ptr, edge, sign, edge_nodes = bconds.incidence_tables()
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.inc_ptr, self.inc_edge, self.inc_sign, self.edge_nodes = to(ptr), to(edge), to(sign), to(edge_nodes)
        nbr = np.asarray(bconds.nbrhoods)
        if nbr.shape[0] == 0:
            nbr = -np.ones((1, 1), np.int64)
        self.nbr = to(nbr.astype(np.int32))
        self.n_nodes, self.max_deg = nbr.shape
        self._h_nbr, self._h_inc_ptr, self._h_inc_edge = nbr, np.asarray(ptr), np.asarray(edge)
        inc_deg = np.diff(np.asarray(ptr)).astype(np.int64)             # readout items of a last node: incident edges of its neighbours
        self.max_items = int(np.where(nbr >= 0, inc_deg[np.maximum(nbr, 0)], 0).sum(axis=1).max()) if inc_deg.size else 0
        self._ro_rows = None
        self._field = None                              # (its node -> blocks table follows the readout tables)
        self._visit = None
        self._readout_version = getattr(bconds, "version", 0)
        self._probed = hasattr(bconds, "prepare")

    def sync_readout(self):
        if getattr(self.bconds, "version", 0) != self._readout_version:
            self._upload_readout()

    def _init_operators(self, S_lower, S_upper):
        E = self.n_edges
        lo, up = S_lower.device_csr(), S_upper.device_csr()
        hint = self.layout.block_starts[S_lower.row_level]
        self._pattern = (abs(lo) + abs(up)).tocsr()
        self._shift_pair = (S_lower, S_upper)
        self.conv = ConvOp(E, [{"mats": [lo, up], "identity": True, "n_cols": E}], hint)
        if S_lower.is_symmetric() and S_upper.is_symmetric():
            self.conv_T = self.conv
        else:
            self.conv_T = ConvOp(E, [{"mats": [lo.T.tocsr(), up.T.tocsr()], "identity": True, "n_cols": E}], hint)
        self.nnz_pattern = self.conv.nnz[0]
        self.nnz_lower, self.nnz_upper = int(lo.nnz), int(up.nnz)

    # -- raw forward/backward over slabs (no autograd): used by the autograd Function and by the trainer
    # The three bounds of the masked forms, each against its own tensor (stack_route); tests set them to 0 to take the forms on small
    # complexes.  Up to KEEP_LAST_MIN_BYTES of H_L the last layer stores everything: the mask's two launches cost more than the stores
    # they save on the graph-replayed steps of small complexes.  SMALL_DZ_BYTES: see _readout_grad.  READOUT_CONE_MIN_BYTES is the same
    # bound under a name of its own, so that a test that sets the other two to 0 stays off the cone.  VISIT_ROWS_MIN_BYTES is that
    # bound once more, for the visit masks of step_cones, and for the same reason: tests/test_gpu_step_masks.py sets the other three to
    # 0 and pins the step's mask launch to ONE call of scn_cone_masks; with this bound left in place those steps visit M_k and make that
    # call, and tests/test_gpu_visit_rows.py sets it to 0 as well.  No step the plan serves on a cone by its own bounds is at or below
    # it (READOUT_CONE_MIN_BYTES is the same figure against the same tensor); what the tables cost on a small complex was not measured.
    KEEP_LAST_MIN_BYTES = 8 << 20
    SMALL_DZ_BYTES = 8 << 20      # below this the readout's backward zeroes the whole buffer itself instead of keeping it all-zero (small complexes)
    READOUT_CONE_MIN_BYTES = 8 << 20
    VISIT_ROWS_MIN_BYTES = 8 << 20

    def _route(self, x, weights, activity, last_dev):
        """stack_route() of this forward: the facts it takes, read off the plan and the arguments."""
        return stack_route(tuple(x.shape), _shapes(weights), activity=activity is not None,
                           last_dev=None if last_dev is None else (last_dev.numel(), last_dev.dtype), fused_conv=self.fused_conv,
                           symmetric=self.conv_T is self.conv, blocked=self._blocked(), tables=self._has_field_tables(),
                           tables_built=self._field is not None, capturing=torch.cuda.is_current_stream_capturing(),
                           keep_last_min=self.KEEP_LAST_MIN_BYTES, small_dz=self.SMALL_DZ_BYTES, cone_min=self.READOUT_CONE_MIN_BYTES)

    def _masks(self, route, last_dev, L):
        """The masks a route's forward runs by, as a Cone: [M0] for a kept last layer, [M0 .. M_{L-1}] (M_k one hop out from M_{k-1})
        for a cone, None without either.  With route.units every mask comes with its unit list (Cone.units): M0's own and
        UNIT_COUNTERS - 1 hops' share one allocation of counters, a stack deeper than they reach runs its lowest masks without one."""
        if not route.keep_last:
            return None
        tabs = self.field_tables_dev()
        if route.units:
            m0, u0, counters = self.conv.keep_mask_units(last_dev, NS, self.n_nodes, tabs)
        else:
            m0, u0, counters = self.conv.keep_mask(last_dev, NS, self.n_nodes, tabs), None, ()
        masks = Cone([m0])
        masks.units = [u0] if route.units else None
        for k in range(1, L if route.cone else 1):
            if k < len(counters):
                m, u = self.conv.mask_hop_units(masks[-1], tabs, counters[k:k + 1])
            else:
                m, u = self.conv.mask_hop(masks[-1], tabs), None
            masks.append(m)
            if route.units:
                masks.units.append(u)
        return masks

    def conv_stack(self, x, weights, activity=None, last_dev=None, out_last=None):
        """One pass over the layers by the route of this forward (stack_route); returns (hs, y0, cone, route), the route being the one
        that ran: where the library declines a launch of a cone or of a from-y pair the stack starts again on route.fallback().
        last_dev: the trajectories' last nodes (what the readout of this forward will take), which the masked routes need.
        out_last (dense stacks of two or more layers): the buffer H_L is written into instead of a fresh one -- a test pre-fills it
        to see which rows a forward wrote."""
        n_layers = (len(weights) - 1) / 3
        assert n_layers % 1 == 0, "wrong number of weights"                    # TE:141-142
        L = int(n_layers)
        route = self._route(x, weights, activity, last_dev)
        masks = self._masks(route, last_dev, L)
        while True:
            ran = self._layers(route, masks, x, weights, activity, out_last, L)
            if ran is not None:
                return ran
            route = route.fallback()

    def _layers(self, route, masks, x, weights, activity, out_last, L):
        """conv_stack's pass; None where a launch the route cannot do without is declined.  Layer l (1-based) of a cone runs kept on
        M_{L-l} and y on M_{L-1}; off the cone only the last layer has a mask, and reruns plainly where its kept form is declined."""
        S, E, ns, _ = x.shape
        cone = masks if route.cone else None
        hs, y0 = [x], None
        for i in range(L):
            w = weights[3 * i:3 * i + 3]
            c_out = w[0].shape[1]
            k = L - 1 - i
            keep = masks[k] if cone is not None or (route.keep_last and k == 0) else None
            units = cone.units[k] if cone is not None and cone.units is not None else None
            wl = activity["fwd"][i] if activity else None
            out = self._zero_pool.take((S, E, ns, c_out)) if activity else out_last if (k == 0 and i > 0) else None
            if i == 0 and route.first == "from_y":      # y only: H1 is never stored (hs[1] is None)
                y0, h = self.conv.shifted_input(x, keep=keep, units=units), None
                if y0 is None:
                    return None
            elif i == 0:
                first = None
                if route.first == "stored":             # 1-channel input: keep the shifted input for the weight gradient
                    first = self.conv.forward_first(x, w, c_out, self.act, out=out, wl=wl,
                                                    y=self._zero_pool.take((S, E, ns, Y_STRIDE)) if activity else None)
                assert first is not None or not activity
                if first is None:                       # an ordinary layer (also where forward_first is declined): no y, no fused-first backward
                    route = route._replace(first="plain", fused_first=False)
                    first = self.conv.forward([x], w, c_out, self.act, out=out, wl=wl), None
                h, y0 = first
            else:
                if i == 1 and route.first == "from_y":  # layer 2 expands y in LDS
                    call = lambda **kept: self.conv.forward_from_y(y0, weights[0:3], w, self.act, out=out, **kept)
                else:
                    call = lambda **kept: self.conv.forward([hs[-1]], w, c_out, self.act, out=out, wl=wl, **kept)
                h = call(keep=keep, units=units) if keep is not None else None
                if h is None and cone is None:
                    h = call()
                if h is None:
                    return None
            hs.append(h)
        return hs, y0, cone, route

    # -- zero-skipping mode ---------------------------------------------------------------------------------
    def _block_graph(self):
        """(block of row, row adjacency incl. self and transposes, rows -> blocks incidence, n_blocks)."""
        if self._blocks is None:
            import scipy.sparse as sp
            row0 = self.conv.plan_blocks()
            nb = len(row0) - 1
            E = self.n_edges
            blk_of = (np.searchsorted(row0, np.arange(E), side="right") - 1).astype(np.int64)
            pat = (self._pattern != 0).astype(np.int32)
            radj = ((pat + pat.T + sp.identity(E, dtype=np.int32, format="csr")) > 0).astype(np.int32).tocsr()
            to_blk = sp.csr_matrix((np.ones(E, np.int32), (np.arange(E), blk_of)), shape=(E, nb))
            self._blocks = (blk_of, radj, to_blk, nb)
        return self._blocks

    def _readout_rows(self):
        """(n_nodes x n_edges) 0/1: device rows of the edges incident to a neighbour of the node (what Bcond(node) reads)."""
        if self._ro_rows is None:
            import scipy.sparse as sp
            V, D = self._h_nbr.shape
            r, c = np.nonzero(self._h_nbr >= 0)
            nbr = sp.csr_matrix((np.ones(len(r), np.int32), (r, self._h_nbr[r, c])), shape=(V, V))
            deg = np.diff(self._h_inc_ptr)
            inc = sp.csr_matrix((np.ones(len(self._h_inc_edge), np.int32),
                                 (np.repeat(np.arange(V), deg), self._h_inc_edge)), shape=(V, self.n_edges))
            self._ro_rows = ((nbr @ inc) > 0).astype(np.int32).tocsr()
        return self._ro_rows

    def _trajectory_supports(self, flow, last_nodes, n_layers):
        """Per TRAJECTORY and layer l = 1..L, as 0/1 matrices (N x n_blocks): Z[l] blocks holding a row where H_l can be
        non-zero, D[l] blocks holding a row the loss can see (support of the gradient of layer l's pre-activation), F[l]
        blocks holding a row that is both.  Computed once per dataset (cached on a hash of the inputs' content): supports are
        tracked per ROW -- one hop = the operator's own pattern -- and only then mapped to plan blocks."""
        import scipy.sparse as sp
        import hashlib
        ln = np.asarray(last_nodes)
        h = hashlib.blake2b(digest_size=16)                  # keyed on CONTENT: an in-place edit of the inputs must miss
        if isinstance(flow, SparseFlows):
            for a in (flow.ptr, flow.idx, flow.val):
                h.update(np.ascontiguousarray(a).view(np.uint8))
        else:
            fa = flow.detach().cpu().numpy() if torch.is_tensor(flow) else np.asarray(flow)
            h.update(str(fa.shape).encode())
            h.update(np.ascontiguousarray(fa).view(np.uint8))
        h.update(np.ascontiguousarray(ln, np.int64).view(np.uint8))
        key = (n_layers, h.hexdigest())
        c = self._act_cache
        if c is not None and c["key"] == key:
            return c
        blk_of, radj, to_blk, nb = self._block_graph()
        perm = self.layout.perm[1]
        fl = flow if isinstance(flow, SparseFlows) else SparseFlows.fromdense(np.asarray(flow))
        N, E = len(fl), self.n_edges

        def ones(M):                                         # 0/1 pattern of a product, in place
            M = M.tocsr()
            M.data[:] = 1
            return M
        hop = lambda M: ones(M @ radj)
        blocks = lambda M: ones(M @ to_blk)
        traj = np.repeat(np.arange(N), np.diff(fl.ptr))
        rows = [ones(sp.csr_matrix((np.ones(len(traj), np.int32), (traj, perm[fl.idx])), shape=(N, E)))]
        for _ in range(n_layers):
            rows.append(hop(rows[-1]))                       # row support of H_1 .. H_L
        # rows the readout touches: edges incident to the neighbours of the last node (Bcond(last), TE:298-303)
        last = np.asarray(last_nodes)[:N]
        sel = sp.csr_matrix((np.ones(N, np.int32), (np.arange(N), last)), shape=(N, self.n_nodes))
        need = [None] * (n_layers + 1)
        need[n_layers] = ones(sel @ self._readout_rows())
        for l in range(n_layers - 1, 0, -1):
            need[l] = hop(need[l + 1])
        c = {"key": key, "N": N, "nb": nb,
             "Z": [None] + [blocks(rows[l]) for l in range(1, n_layers + 1)],
             "D": [None] + [blocks(need[l]) for l in range(1, n_layers + 1)],
             "F": [None] + [blocks(rows[l].multiply(need[l])) for l in range(1, n_layers + 1)]}
        self._act_cache = c
        return c

    def activity(self, flow, last_nodes, n_layers, hidden, mode, sel=None):
        """Work lists of one micro-batch = trajectories `sel` (default: all) of the dataset (flow, last_nodes).
        mode "zeros": every (block, slab) item that can hold a non-zero value (a layer's output is exactly zero outside the
        one-hop closure of its input's support); mode "field": additionally only what the loss can see (the readout reads H_L
        on the edges around the last nodes; each layer below needs one more hop).  None when the shape is not served by the
        work-list kernels."""
        import scipy.sparse as sp
        if mode in (None, "dense") or hidden not in (16, 32) or not self.conv.plan_info()[0] or self._probed:
            return None
        c = self._trajectory_supports(flow, last_nodes, n_layers)
        sel = np.arange(c["N"]) if sel is None else np.asarray(sel)
        n = len(sel)
        S = pad_count(n, NS) // NS
        agg = sp.csr_matrix((np.ones(n, np.int32), (np.arange(n) // NS, sel)), shape=(S, c["N"]))   # slab <- its trajectories
        dev = self.device
        fsrc = c["F"] if mode == "field" else c["Z"]
        fwd = [WorkList(agg @ fsrc[l], dev) for l in range(1, n_layers + 1)]
        bwd = [None] + [WorkList(agg @ c["D"][l], dev) for l in range(1, n_layers + 1)]
        total = S * c["nb"]
        return {"fwd": fwd, "bwd": bwd, "mode": mode,
                "active_fraction": {"fwd": [w.items / total for w in fwd], "bwd": [w.items / total for w in bwd[1:]]}}

    def _has_field_tables(self):
        return self.conv is not None and self.conv.plan_info()[0] > 0 and not self._probed

    def field_tables_dev(self):
        """FieldTables of this plan (built and uploaded once; dropped with the readout tables), or None where activity() serves
        nothing either: no blocked plan, a probed Bcond_func closure.  The pattern is the one `conv` stores (union_pattern of the two
        shifts, explicit zeros included): what a block's rows stage, and for non-symmetric shifts nothing more."""
        if not self._has_field_tables():
            return None
        if self._field is None:
            rowptr, cols, _ = union_pattern([s.device_csr() for s in self._shift_pair])
            (tp, tb), (ap, ab) = field_tables(self.conv.plan_blocks(), (rowptr, cols), self._h_nbr, self._h_inc_ptr, self._h_inc_edge)
            # (an empty table still needs a valid pointer: one unused element)
            to = lambda a: torch.from_numpy(np.ascontiguousarray(np.append(a, 0), np.int32)).to(self.device)
            self._field = FieldTables(len(ap) - 1, to(tp), to(tb), to(ap), to(ab))
        return self._field

    def visit_tables_dev(self, hops):
        """VisitTables of this plan for at least `hops` hops (built and uploaded once per depth asked for; dropped with the field tables),
        or None where they cannot be had now: no field tables, shifts that are not symmetric (the backward's operator then reads other
        columns than the pattern the tables hop over), or a stream under a graph capture with the tables not built yet -- the rule the
        field tables follow (stack_route) -- or an operator whose hops grow past VISIT_TABLES_MAX_WORK (a hub row; asked once per depth)."""
        if not self._has_field_tables() or self.conv_T is not self.conv or hops < 1:
            return None
        if isinstance(self._visit, int):                # the depth visit_tables refused at
            if hops >= self._visit:
                return None
            self._visit = None
        if self._visit is None or len(self._visit.ptr) < hops:
            if torch.cuda.is_current_stream_capturing():
                return None
            rowptr, cols, _ = union_pattern([s.device_csr() for s in self._shift_pair])
            tabs = visit_tables(self.conv.plan_blocks(), (rowptr, cols), self._h_nbr, self._h_inc_ptr, self._h_inc_edge, hops)
            if tabs is None:
                self._visit = hops
                return None
            to = lambda a: torch.from_numpy(np.ascontiguousarray(np.append(a, 0), np.int32)).to(self.device)
            self._visit = VisitTables([to(p) for p, _ in tabs], [to(b) for _, b in tabs])
        return self._visit

    def release(self, saved):
        """Forward-only use of the zero-skipping mode (prediction): hand the forward's pooled buffers back, all-zero again."""
        if saved.activity:
            for l in range(1, len(saved.hs)):
                self._give_back(saved.hs[l], saved.activity["fwd"][l - 1])
            self._give_back(saved.y0, saved.activity["fwd"][0])

    def _give_back(self, t, wl):
        self.conv.clear(t, wl)                              # all-zero again
        self._zero_pool.give(t)

    def _readout_args(self, last_dev, sign=True, edge_nodes=False):
        """The readout tables as every launch that reads them takes them: nbr, n_nodes, max_deg, last nodes, inc_ptr, inc_edge
        [, inc_sign][, edge_nodes].  last_dev = None: the one-launch step's form -- it takes the last nodes earlier and max_items here."""
        i32 = lambda t: _dev(t, torch.int32)
        return (i32(self.nbr), self.n_nodes, self.max_deg, self.max_items if last_dev is None else i32(last_dev), i32(self.inc_ptr),
                i32(self.inc_edge)) + ((_dev(self.inc_sign),) if sign else ()) + ((i32(self.edge_nodes),) if edge_nodes else ())

    def readout(self, H, w_last, last_dev):
        S, E, ns, C = H.shape
        assert tuple(w_last.shape) == (C, 1), "readout weight must be (C, 1) (STM:233, out_channels = 1)"
        bh = torch.empty((S * ns, self.max_deg, C), device=H.device, dtype=torch.float32)
        logits, logp = (torch.empty((S * ns, self.max_deg), device=H.device, dtype=torch.float32) for _ in range(2))
        check(_lib.load().scn_readout_forward(S, ns, E, C, _dev(H), _dev(w_last), *self._readout_args(last_dev), _dev(bh), _dev(logits),
                                              _dev(logp), _stream()), "scn_readout_forward")
        return logp, bh, logits

    def _readout_step(self, H, w_last, last_dev, yt, scale, zero_buf):
        """readout, d_logp = yt * scale and _readout_grad in ONE launch, which also zeroes zero_buf where given (scn_readout_step): dz as
        _readout_grad leaves it, and what the epilogue sums the loss and dW_last from.  dz None (nothing launched, the pool as it was): declined."""
        S, E, ns, C = H.shape
        bh = torch.empty((S * ns, self.max_deg, C), device=H.device, dtype=torch.float32)
        logits, logp, d_logp, d_logits = (torch.empty((S * ns, self.max_deg), device=H.device, dtype=torch.float32) for _ in range(4))
        dz = self._dz_zero.take(H)
        zero = (_dev(zero_buf), zero_buf.numel()) if zero_buf is not None else (None, 0)
        if not _served(_lib.load().scn_readout_step(S, ns, E, C, _dev(H), _dev(w_last), *self._readout_args(last_dev, edge_nodes=True), _dev(yt),
                                                    float(scale), ACT[self.act], _dev(bh), _dev(logits), _dev(logp), _dev(d_logp), _dev(d_logits),
                                                    _dev(dz), 1, *zero, _stream()), "scn_readout_step"):
            self._dz_zero.give(dz)                      # (declined before any launch: still all-zero)
            return None, None, None, None
        return dz, logp, d_logits, bh

    def _readout_grad(self, H, bh, logp, d_logp, last_dev, weights, grads):
        """Gradient of the readout w.r.t. the last layer's pre-activation, into a pooled all-zero buffer: zero except on the edges around the
        last nodes, which _wipe_and_keep wipes again (no 16 GB memset); up to SMALL_DZ_BYTES the launch zeroes it itself (dz_is_zero = 2)."""
        S, E, ns, C = H.shape
        small = H.numel() * 4 <= self.SMALL_DZ_BYTES
        dz_top = self._dz_zero.take(H, zeroed=not small)
        d_logits, d_logp = torch.empty_like(logp), d_logp.contiguous()
        check(_lib.load().scn_readout_backward(S, ns, E, C, _dev(H), _dev(weights[-1]), *self._readout_args(last_dev, edge_nodes=True), _dev(bh),
                                               _dev(d_logp), _dev(logp), ACT[self.act], _dev(d_logits), _dev(dz_top), 2 if small else 1,
                                               _dev(grads[-1]), _stream()), "scn_readout_backward")
        return dz_top

    def _wipe_and_keep(self, dz, last_dev, mask=None):
        """A layer is done with its gradient buffer: wipe the items written and keep it.  mask: the one a visiting backward wrote it on;
        None: a readout gradient, wiped on the rows around the last nodes (not where the launch zeroes the buffer itself)."""
        if mask is not None:
            self.conv.clear_mask(dz, mask)
        elif dz.numel() * 4 > self.SMALL_DZ_BYTES:
            S, E, ns, C = dz.shape
            check(_lib.load().scn_readout_clear_dz(S, ns, E, C, *self._readout_args(last_dev, sign=False, edge_nodes=True),
                                                   _dev(dz), _stream()), "scn_readout_clear_dz")
        self._dz_zero.give(dz)

    def _blocked(self):
        op = self.conv if self.conv is not None else self.op
        return op.plan_info()[0] > 0

    # -- small complexes: the whole gradient step of a micro-batch in one launch (scn_small_step, csrc/scn_small.hip)
    def small_step(self, x, last_dev, yt, scale, weights, grads, loss, overwrite=False, adam=None):
        """grads[k] += d/dW[k] of scale * sum_n <logp_n, yt_n> and loss[0] += that sum, with one workgroup per trajectory keeping
        the activations in LDS through all layers and both directions (the reference's own sizes, TE:86-90).  False when the
        shape is not served (hidden width other than 16, a complex too large for the LDS, ...): the caller then runs
        forward / scn_masked_ce / backward.  overwrite: grads and loss are SET instead of accumulated into.
        adam (with overwrite): (flat_w, m, v, lr, weight_decay, step_dev) -- the launch that sums the gradient also applies the
        optimiser step to the flat weight buffer `weights` are views of (scn_small_step_adam)."""
        if not SMALL_STEP or self.conv is None or self.conv.n_groups != 1 or len(weights) < 7 or (len(weights) - 1) % 3:
            return False
        L = (len(weights) - 1) // 3
        S, E, ns, c_in = x.shape
        if not small_step_pays(E, S * ns, device_cus(x.device)):
            return False
        hidden = weights[0].shape[1]
        shapes = [(1, hidden)] * 3 + [(hidden, hidden)] * (3 * (L - 1)) + [(hidden, 1)]
        if c_in != 1 or [tuple(w.shape) for w in weights] != shapes or tuple(yt.shape) != (S * ns, self.max_deg):
            return False
        lib = _lib.load()
        if not lib.scn_small_step_supported(self.conv.handle, L, hidden, self.max_deg, self.max_items):
            return False
        ws = _workspace(lib.scn_small_step_workspace(E, S * ns, L), x.device)
        # bytes the launch has to move at least: the input flows, the saved activations written and read back, the operator
        nb = x.numel() * 4 + 2 * (L - 1) * S * ns * E * hidden * 4 + self.conv.csr_bytes
        assert adam is None or overwrite, "the fused optimiser step takes the whole gradient of the batch"
        args = (self.conv.handle, self.conv_T.handle, S, ns, L, hidden, _dev(x), _dev(last_dev, torch.int32), _dev(yt), float(scale),
                *self._readout_args(None), _ptrs(weights), ACT[self.act], _ptrs(grads), ctypes.c_void_p(loss.data_ptr()))
        with _timed("small_step L%d c%d" % (L, hidden), nb):
            if adam is None:
                check(lib.scn_small_step(*args, 1 if overwrite else 0, *ws, _stream()), "scn_small_step")
            else:
                flat_w, m, v, lr, wd, step_dev = adam
                check(lib.scn_small_step_adam(*args, *ws, _dev(flat_w), _dev(m), _dev(v), float(lr), 0.9, 0.999, 1e-8,
                                              ctypes.c_void_p(step_dev.data_ptr()), float(wd), _stream()), "scn_small_step_adam")
        return True

    # -- the cone route: a micro-batch whose tail is two launches (scn_readout_step, scn_step_epilogue; STEP_TAIL)
    def _step_route(self, x, last_dev, yt, weights):
        """The route of a micro-batch that step() serves, or None: the facts step() declines on before it launches anything."""
        if not STEP_TAIL or not self.fused_conv or self.conv is None or last_dev is None or self.max_deg > 64:
            return None
        if len(weights) < 7 or (len(weights) - 1) % 3 or self.promotion(weights):
            return None
        L = (len(weights) - 1) // 3
        S, E, ns, _ = x.shape
        if tuple(yt.shape) != (S * ns, self.max_deg) or L - 1 > _lib.SCN_EPI_MAX_REDUCES:
            return None
        route = self._route(x, weights, None, last_dev)
        return route if route.cone and route.first == "from_y" else None

    def step_cones(self, staged_micro_batches, weights):
        """The cones of every micro-batch of a step -- staged_micro_batches: (x, last_dev, yt, activity) each -- from ONE launch
        (ConvOp.cone_masks; STEP_MASKS), to hand to step(cone=...) one by one.  None (nothing launched) where the switch is off, some
        micro-batch is not one step() serves on a cone with unit lists, or the library declines: step() then builds each micro-batch's
        masks itself.  Nothing is kept: the masks are built inside the step that uses them, from the batch staged for it.
        With VISIT_ROWS the record also carries every micro-batch's visit masks (Cone.visits), which step()'s backwards visit by."""
        if not STEP_MASKS or not staged_micro_batches:
            return None
        L = (len(weights) - 1) // 3
        served = {}                                     # (one look per shape: host time ahead of a step's first launch)
        for x, last_dev, yt, activity in staged_micro_batches:
            if activity is not None or last_dev is None:
                return None
            key = (tuple(x.shape), last_dev.numel(), last_dev.dtype, tuple(yt.shape))
            if key not in served:
                route = self._step_route(x, last_dev, yt, weights)
                served[key] = route is not None and route.units and x.shape[2] == NS
            if not served[key]:
                return None
        tabs = self.field_tables_dev()
        if L > UNIT_COUNTERS or max(tabs.n_blocks * ((m[0].shape[0] + 31) // 32) for m in staged_micro_batches) > cone_masks_limit():
            return None
        # the visit masks of the step's backwards from the same launch (VISIT_ROWS); without the tables the backwards visit M_k
        dz32 = min(m[0].shape[0] for m in staged_micro_batches) * self.n_edges * NS * 32 * 4
        visit_tabs = self.visit_tables_dev(L - 1) if VISIT_ROWS and dz32 > self.VISIT_ROWS_MIN_BYTES else None
        return self.conv.cone_masks([m[1] for m in staged_micro_batches], NS, self.n_nodes, tabs, L, visit_tabs=visit_tabs)

    def step(self, x, last_dev, yt, scale, weights, grads, part, overwrite=False, zero_buf=None, cone=None):
        """grads[k] += d/dW[k] of scale * sum_n <logp_n, yt_n> and part[0] += that sum (overwrite: part[0] = ...), as forward /
        scn_masked_ce_begin / backward compute them bit for bit, on the cone route of a plain stack at hidden 32: the forward stack, ONE
        readout launch (_readout_step; zero_buf: a fresh step's flat gradient buffer, or None), backward()'s walk with its reduces and lowest
        wipes deferred (_cone_backward) and ONE launch for those (ConvOp.step_epilogue).  False (nothing launched that changes grads, part or
        a pooled buffer): not served, the caller runs the separate calls.  cone: from step_cones(); None: the masks are built here, in five."""
        route = self._step_route(x, last_dev, yt, weights)
        L = (len(weights) - 1) // 3
        ran = route and self._layers(route, cone if cone is not None else self._masks(route, last_dev, L), x, weights, None, None, L)
        if ran is None:
            return False
        hs, y0, cone, route = ran
        assert cone is not None and hs[-1].numel() * 4 > self.SMALL_DZ_BYTES   # (what makes a cone: the gradient buffers are kept all-zero)
        dz, logp, d_logits, bh = self._readout_step(hs[-1], weights[-1], last_dev, yt, scale, zero_buf)
        if dz is None:
            return False
        jobs = []
        waiting = self._cone_backward(hs, y0, cone, dz, last_dev, weights, grads, defer=jobs)
        self.conv.step_epilogue((logp, yt, scale, part, overwrite), (d_logits, bh, grads[-1]), jobs, waiting,
                                self._readout_args(last_dev, sign=False, edge_nodes=True) if waiting[0][1] is None else None)
        for t, _ in waiting:
            self._dz_zero.give(t)
        return True

    def promotion(self, weights):
        """Promoted hidden width of this weight list on this plan (None: runs as it is)."""
        shapes = _shapes(weights)
        if len(shapes) < 4 or (len(shapes) - 1) % 3 or not self._blocked():
            return None
        # widths above 32 are padded to a multiple of 32 on both plans: the fused plan runs them in 32-channel blocks (_wide_stack), the
        # composed Ebli plan (PowerPlan) keeps its per-shift structure and runs its dense-term kernels as 32 x 32 MFMA blocks
        return promoted_width([sh[1] for sh in shapes[:-1]], wide=shapes[0][0] == 1)

    def forward(self, x, last_dev, weights, activity=None, out_last=None):
        """out_last: see conv_stack (plain dense stacks; ignored by the wide stack and the work-list modes)."""
        P = self.promotion(weights)
        wp = promote_weights(weights, 3, 1, P) if P else None
        w = wp if P else weights
        if P and P > 32 and self.fused_conv:
            hs, y0 = self._wide_stack(x, w, P)
            # the readout is linear in H: block by block with the block's rows of W_last, the logits added and normalised in one launch
            bhs, parts = [], []
            for j, Hj in enumerate(hs[-1]):
                _, bh, lg = self.readout(Hj, w[-1][32 * j:32 * j + 32], last_dev)
                bhs.append(bh)
                parts.append(lg)
            logp = torch.empty_like(parts[0])
            check(_lib.load().scn_logits_sum_log_softmax(logp.shape[0], self.max_deg, len(parts), _ptrs(parts),
                                                         _dev(parts[0]), _dev(logp), _stream()), "scn_logits_sum_log_softmax")
            return logp, SconeState(hs, bhs, y0, None, wp, wide=True)
        if not self.fused_conv:                         # (PowerPlan: every layer stores its whole output, no route)
            (hs, y0), cone, route = self.conv_stack(x, w), None, None
        else:
            hs, y0, cone, route = self.conv_stack(x, w, activity, last_dev, out_last)
        logp, bh, _ = self.readout(hs[-1], w[-1], last_dev)
        return logp, SconeState(hs, bh, y0, activity, wp, wide=False, cone=cone, route=route)

    # -- hidden widths above 32 (TE:103-110 accepts any): every activation is P / 32 separate 32-channel tensors and a layer is
    # its (input block i, output block j) pairs on the fused C = 32 kernels -- act(sum_i sum_s (S_s H_i) W_s[i, j]) (TE:143-149):
    # the partial pre-activations of an output block are added and activated by scn_sum_act; in the backward the partial input
    # gradients of an input block add up likewise (act' of the layer below is a common factor of the partial results).  The
    # same products in the same association order per 32 x 32 weight block; ~4x the hidden-32 step at hidden 64 instead of the
    # generic one-row-per-workgroup kernels (measured 236x, profiles/HISTORY.md section 3.3).
    @staticmethod
    def _wblock(W, i, j):
        r = slice(None) if W.shape[0] == 1 else slice(32 * i, 32 * i + 32)
        return W[r, 32 * j:32 * j + 32].contiguous()

    def _wide_stack(self, x, w, P):
        k, L = P // 32, (len(w) - 1) // 3
        hs, y0 = [[x]], None
        for l in range(L):
            W, prev, outs = w[3 * l:3 * l + 3], hs[-1], []
            for j in range(k):
                if l == 0:
                    first = self.conv.forward_first(x, [self._wblock(Ws, 0, j) for Ws in W], 32, self.act)
                    assert first is not None, "wide hidden layers need the first-layer fast path (1-channel flows)"
                    outs.append(first[0])
                    y0 = first[1] if y0 is None else y0
                else:
                    # input block by input block INTO the output block: the partial pre-activation of the blocks before is added
                    # inside the next launch (scn_conv_forward_accumulate, in place), the last launch applies the activation
                    acc = None
                    for i in range(len(prev)):
                        last = i == len(prev) - 1
                        acc = self.conv.forward([prev[i]], [self._wblock(Ws, i, j) for Ws in W], 32, self.act if last else "none",
                                                partial=acc)
                    outs.append(acc)
            hs.append(outs)
        return hs, y0

    def _wide_backward(self, saved, logp, d_logp, last_dev, w, grads):
        hs, bhs, y0 = saved.hs, saved.bh, saved.y0
        k, L = len(hs[-1]), len(hs) - 1
        # the readout's gradient block by block (d_logits depends on the summed logits only), each into its own pooled all-zero buffer
        dzs = [self._readout_grad(hs[-1][j], bhs[j], logp, d_logp, last_dev, [w[-1][32 * j:32 * j + 32]], [grads[-1][32 * j:32 * j + 32]])
                for j in range(k)]
        for l in reversed(range(1, L)):
            W, G = w[3 * l:3 * l + 3], grads[3 * l:3 * l + 3]
            new = []
            for i in range(len(hs[l])):
                acc = None                              # output block by output block INTO the input block's gradient (in place)
                for j in range(k):
                    gij = [torch.zeros((32, 32), device=self.device, dtype=torch.float32) for _ in range(3)]
                    acc = self.conv_T.backward([dzs[j]], [self._wblock(Ws, i, j) for Ws in W], hs[l][i], self.act, True, gij,
                                               dx_partial=acc)
                    for Gs, g in zip(G, gij):
                        Gs[32 * i:32 * i + 32, 32 * j:32 * j + 32] += g
                new.append(acc)
            if l == L - 1:                              # the top layer is done with the readout gradients: wipe and keep them
                for dz_top in dzs:
                    self._wipe_and_keep(dz_top, last_dev)
            dzs = new
        for j in range(k):                              # the first layer: dW_s[0, j] = sum_p (S_s x)[p] dz_j[p], one stream over dz per block
            gj = [torch.zeros((1, 32), device=self.device, dtype=torch.float32) for _ in range(3)]
            assert self.conv.dw_first(hs[0][0], y0, dzs[j], gj)
            for Gs, g in zip(grads[0:3], gj):
                Gs[:, 32 * j:32 * j + 32] += g
        if L == 1:                                      # (a single wide layer: the readout gradients were this layer's dz)
            for dz_top in dzs:
                self._wipe_and_keep(dz_top, last_dev)
        return grads

    def _cone_backward(self, hs, y0, cone, dz, last_dev, weights, grads, defer=None):
        """The walk down a cone [M0 .. M_{L-1}], layers L-1 .. 1, from a readout gradient dz already written: the one loop of backward() and
        step().  Layer l visits M_{L-l+1}, one hop out from the set its dZ_l was written on, and dX_l goes into a pooled all-zero buffer on the
        visited items only (layer 1 rebuilds H1 from y0 and sums dW_first in the same launch: no dx); then dZ_l is wiped on the mask the layer
        above visited and given back.  defer = None: every reduce inside its launch, every wipe after its layer.  defer = a list: it takes the
        reduces as jobs, and the wipes of deferred_clears(L) wait too: returned as step_epilogue's clears; the caller gives them back after it.
        A cone with visit masks (Cone.visits, step_cones): V_k stands in for M_k in both places -- every item of M_k outside V_k stages
        only +0, whatever the data, so the same sums are formed in the same order and dx is written, and wiped, on V_k alone."""
        L = len(hs) - 1
        waits, waiting = deferred_clears(L) if defer is not None else (), []
        visits = getattr(cone, "visits", None) or cone
        for i in reversed(range(1, L)):
            w, g = weights[3 * i:3 * i + 3], grads[3 * i:3 * i + 3]
            dx = self._dz_zero.take(dz) if i > 1 else None
            if i == 1:
                ok = self.conv_T.backward_fused_first(dz, w, None, self.act, y0, g, grads[0:3], Ws_first=weights[0:3], visit=visits[L - i], defer=defer)
            else:
                ok = self.conv_T.backward([dz], w, hs[i], self.act, True, g, dx=dx, visit=visits[L - i], defer=defer) is not False
            assert ok, "visiting backward of layer %d not served" % (i + 1)
            mask = visits[L - 1 - i] if i < L - 1 else None
            if i in waits:
                waiting.append((dz, mask))
            else:
                self._wipe_and_keep(dz, last_dev, mask)
            dz = dx
        return waiting

    def _backward(self, saved, logp, d_logp, last_dev, weights, grads):
        """On a cone _cone_backward, reducing and wiping as it goes; else one loop down the layers by the route the forward ran: the top
        layer stages dZ_L by hop(M0) where it says so -- the mask is built from the readout's last nodes, for this call alone."""
        if saved.wide:
            return self._wide_backward(saved, logp, d_logp, last_dev, weights, grads)
        hs, y0, activity, route = saved.hs, saved.y0, saved.activity, saved.route
        L = len(hs) - 1
        dz = self._readout_grad(hs[-1], saved.bh, logp, d_logp, last_dev, weights, grads)
        if saved.cone is not None:
            self._cone_backward(hs, y0, saved.cone, dz, last_dev, weights, grads)
            return grads
        for i in reversed(range(L)):
            w, g = weights[3 * i:3 * i + 3], grads[3 * i:3 * i + 3]
            wl_out = activity["bwd"][i] if (activity and i > 0) else None      # items of this layer's input gradient
            wl_in = activity["bwd"][i + 1] if activity else None                # support of dz
            if i == 1 and route.first == "from_y":      # H1 was never stored: aux is rebuilt from y0, dW_first in the same launch, no dx
                assert self.conv_T.backward_fused_first(dz, w, None, self.act, y0, g, grads[0:3], Ws_first=weights[0:3]), \
                    "aux-free fused-first backward not served"
                dx = None
            elif i == 1 and route.fused_first and self.conv_T.backward_fused_first(dz, w, hs[1], self.act, y0, g, grads[0:3], wl=wl_out):
                dx = None                               # dx of this layer only feeds dW_first: contracted in registers, never written
            elif i == 0 and hs[0].shape[3] == 1 and self.conv.dw_first(hs[0], y0, dz, g, wl=wl_in):
                dx = None                               # first layer: shifted 1-channel input x one stream over dz
            else:
                assert not activity or i > 0, "zero-skipping needs the first-layer fast path"
                dx = False                              # the top layer: dz staged only where the readout wrote it (False: not served)
                if i == L - 1 and route.top_dz_mask:
                    tabs = self.field_tables_dev()
                    m1 = self.conv.mask_hop(self.conv.keep_mask(last_dev, NS, self.n_nodes, tabs, key="dz_mask"), tabs)
                    dx = self.conv_T.backward([dz], w, hs[i], self.act, True, g, dz_mask=m1)
                if dx is False:
                    dx = self.conv_T.backward([dz], w, hs[i], self.act, i > 0, g, dx=self._zero_pool.take(hs[i]) if activity else None, wl=wl_out)
            if i == L - 1:                              # the top layer is done with the readout gradient: wipe and keep it
                self._wipe_and_keep(dz, last_dev)
            elif activity:
                self._give_back(dz, wl_in)
            if dx is None:                              # the first layer's weight gradient is out: nothing is left below
                break
            dz = dx
        self.release(saved)                             # (zero-skipping: the forward's buffers go back to the pool, all-zero again)
        return grads


class PowerPlan(SconePlan):
    """scone-like model whose second shift is the SQUARE of the first (Ebli / SNN: L1 and L1^2, TE:251-253), for complexes
    where the rows of the square no longer fit the LDS-blocked plan (> 128 distinct sources).  The square is never formed:
    per layer  G1 = S H,  G2 = S G1  on the LDS-blocked SpMM, then  act(H W0 + G1 W1 + G2 W2)  and its backward on the dense
    term kernels (scn_dense_terms_*) -- the same composition the Bunch plan uses."""
    fused_conv = False            # self.op is S alone (self.conv is None)

    def _init_operators(self, S_lower, S_upper):
        E = self.n_edges
        m = S_lower.device_csr()
        hint = self.layout.block_starts[S_lower.row_level]
        # identity slot on: the fused kernels read the staged tensor's own row as their middle term (the SpMM ignores it)
        self.op = ConvOp(E, [{"mats": [m], "identity": True, "n_cols": E}], hint)
        self.op_T = self.op if S_lower.is_symmetric() else ConvOp(E, [{"mats": [m.T.tocsr()], "identity": True, "n_cols": E}], hint)
        self.conv = self.conv_T = None
        self.nnz_pattern = self.nnz_lower = int(m.nnz)
        self.nnz_upper = int(S_upper.csr.nnz)

    @staticmethod
    def _shift(op, x):
        return spmm_chunked(op, x)

    def activity(self, *a, **k):
        return None

    def field_tables_dev(self):
        return None

    def conv_stack(self, x, weights):
        n_layers = (len(weights) - 1) / 3
        assert n_layers % 1 == 0, "wrong number of weights"                    # TE:159-160
        hs, y0 = [x], None
        for i in range(int(n_layers)):
            w = weights[3 * i:3 * i + 3]
            g1 = self._shift(self.op, hs[-1])
            out = self.op.forward_power(hs[-1], g1, w, self.act) if hs[-1].shape[3] == w[0].shape[1] else None
            if out is None:                            # widths the fused kernel does not take: shift again, dense terms
                g2 = self._shift(self.op, g1)
                out = dense_terms_forward([hs[-1], g1, g2], w, w[0].shape[1], self.act)
                if i == 0 and x.shape[3] == 1:
                    y0 = torch.cat([x, g1, g2, torch.zeros_like(x)], dim=3)  # the shifted input per point, for the first layer's weight gradient
            hs.append(out)
        return hs, y0

    def _backward(self, saved, logp, d_logp, last_dev, weights, grads):
        hs, bh, y0 = saved.hs, saved.bh, saved.y0
        dz = self._readout_grad(hs[-1], bh, logp, d_logp, last_dev, weights, grads)
        L = len(hs) - 1
        for i in reversed(range(L)):
            g1 = self._shift(self.op_T, dz) if not (i == 0 and y0 is not None) else None
            served, dx = (self.op_T.backward_power(dz, g1, weights[3 * i:3 * i + 3], hs[i], self.act, i > 0,
                                                   grads[3 * i:3 * i + 3])
                          if (g1 is not None and hs[i].shape[3] == dz.shape[3]) else (False, None))
            if not served and i == 0 and hs[0].shape[3] == 1 and y0 is not None \
                    and self.op.dw_first(None, y0, dz, grads[0:3]):
                dx = None                               # first layer: dW_k = sum_p (S^k x)[p] dz[p], one stream over dz
            elif not served:
                g1 = self._shift(self.op_T, dz) if g1 is None else g1
                g2 = self._shift(self.op_T, g1)
                dx = dense_terms_backward([dz, g1, g2], weights[3 * i:3 * i + 3], hs[i], self.act, i > 0,
                                          grads[3 * i:3 * i + 3])
            if i == L - 1:
                self._wipe_and_keep(dz, last_dev)
            dz = dx
        return grads


# ----------------------------------------------------------------------------------------------
# bunch
# ----------------------------------------------------------------------------------------------

BUNCH_SRC = [0, 1, 0, 1, 2, 1, 2]      # input level of weight slot k   (TE:184-192)
BUNCH_DST = [0, 0, 1, 1, 1, 2, 2]      # output level of weight slot k


class BunchPlan(Plan):
    """Device state of the Bunch (SCCONV) model.  Each of the seven shifts S_k (and its transpose for the backward) is a
    single-operator ConvOp served by the LDS-blocked SpMM; the per-level sum over shifts, the weights and the relu are
    one dense kernel (scn_dense_terms_*).  Shapes the blocked SpMM does not take (ns*C > 128) fall back to the generic
    multi-group kernels (one operator per output / input level)."""
    weights_per_layer = 7

    def __init__(self, shifts, nbrhoods, device):
        assert len(shifts) == 7 and all(isinstance(s, Shift) for s in shifts)
        self.layout = shifts[0].layout
        self.device = device
        self.sizes = self.layout.sizes
        self.n_edges = int(self.sizes[1])
        self.n_rows = sum(self.sizes)
        dev = [s.device_csr() for s in shifts]
        hints = self.layout.block_starts
        # a level without simplices (a complex without faces: B2 has no columns, BMM:71-135 still yields the seven shapes) carries
        # nothing: its shifts are empty operators, its tensors have no rows -- the shifts that touch it are left out altogether
        self._live = [self.sizes[BUNCH_SRC[k]] > 0 and self.sizes[BUNCH_DST[k]] > 0 for k in range(7)]
        self.term_fwd = [ConvOp(self.sizes[BUNCH_DST[k]], [{"mats": [dev[k]], "identity": False,
                                                           "n_cols": self.sizes[BUNCH_SRC[k]]}], hints[BUNCH_DST[k]])
                         if self._live[k] else None for k in range(7)]
        self.term_bwd = [ConvOp(self.sizes[BUNCH_SRC[k]], [{"mats": [dev[k].T.tocsr()], "identity": False,
                                                           "n_cols": self.sizes[BUNCH_DST[k]]}], hints[BUNCH_SRC[k]])
                         if self._live[k] else None for k in range(7)]
        self.fwd_slots = [[k for k in range(7) if BUNCH_DST[k] == lvl and self._live[k]] for lvl in range(3)]
        self.bwd_slots = [[k for k in range(7) if BUNCH_SRC[k] == lvl and self._live[k]] for lvl in range(3)]
        self._dev_csr = dev
        self._generic = None
        self._terms = None                              # fused-layer operators (forward, transposed), built on first use
        self._terms_nf = None                           # forward operator of a layer whose face output nothing reads
        self._terms_bwd_nf = None                       # transposed operator of a layer whose faces carry no gradient
        nb = np.asarray(nbrhoods)
        pn = self.layout.perm[0]
        # padding index -1 wraps to the LAST node of the caller's numbering (TE:201); resolve it here, in device order
        nbd = np.where(nb >= 0, pn[np.maximum(nb, 0)], pn[self.sizes[0] - 1])
        self.nbr = torch.from_numpy(np.ascontiguousarray(nbd, np.int32)).to(device)
        self.max_deg = nb.shape[1]

    def _generic_ops(self):
        if self._generic is None:
            dev = self._dev_csr
            fwd = [ConvOp(self.sizes[lvl], [{"mats": [dev[k]], "identity": False, "n_cols": self.sizes[BUNCH_SRC[k]]}
                                            for k in self.fwd_slots[lvl]]) for lvl in range(3)]
            bwd = [ConvOp(self.sizes[lvl], [{"mats": [dev[k].T.tocsr()], "identity": False,
                                             "n_cols": self.sizes[BUNCH_DST[k]]} for k in self.bwd_slots[lvl]])
                   for lvl in range(3)]
            self._generic = (fwd, bwd)
        return self._generic

    def _terms_ops(self):
        """The seven shifts as one operator on the concatenated row space, and its transpose (scn_terms_*): the fused layer.
        None when the plan builder cannot hold the complex (SCN_ERR_UNSUPPORTED: a single concatenated row with more than
        112 distinct sources, e.g. a hub node) -- the per-shift path then carries every layer, forward AND backward."""
        if self._terms is None and not all(self._live):
            self._terms = False                          # an empty level: the per-shift path (nothing to fuse across three levels)
        if self._terms is None:
            # bins: rows of (nodes, edges, faces) a block holds = the natural 0.37 : 1 : 0.67 proportions in wave units
            fwd = self._optional_terms(False, range(7), (12, 32, 20), 4)
            bwd = fwd and self._optional_terms(True, range(7), (16, 32, 16), 8)
            self._terms = (fwd, bwd) if bwd else False
        return self._terms or None

    def _optional_terms(self, transposed, slots, bins, rows_per_wave):
        """TermsOp of these shifts (transposed: of their transposes), or False when the plan builder cannot hold it
        (SCN_ERR_UNSUPPORTED): the caller then does without."""
        dev = self._dev_csr
        blocks = {(BUNCH_SRC[k], BUNCH_DST[k]): dev[k].T.tocsr() for k in slots} if transposed else \
                 {(BUNCH_DST[k], BUNCH_SRC[k]): dev[k] for k in slots}
        try:
            return TermsOp(self.sizes, blocks, self.layout.merged, bins, rows_per_wave)
        except _lib.SconeHipError as e:
            if e.status != _lib.SCN_ERR_UNSUPPORTED:
                raise
            return False

    def _terms_fwd_for(self, want):
        """Forward fused-layer operator for the wanted output levels: when the faces are not wanted (the layer before the last
        one: TE:198-201 reads only the nodes of the last layer, which the faces do not feed) a plan whose blocks hold node and
        edge rows only -- the face rows' share of every block goes to them (fewer blocks, fewer staged sources per output row)."""
        fwd = self._terms_ops()[0]
        if want[2] or not (want[0] and want[1]):
            return fwd
        if self._terms_nf is None:
            self._terms_nf = self._optional_terms(False, [k for k in range(7) if BUNCH_DST[k] != 2], (16, 48, 0), 4)
        return self._terms_nf or fwd

    def _terms_bwd_for(self, dz_present):
        """Transposed fused-layer operator for the levels whose gradient exists: when the faces carry none (the layer before the
        last one: its face output was never computed) the two shifts INTO the faces are left out of the operator, so no block
        spends staged sources on rows that are never staged."""
        bwd = self._terms_ops()[1]
        if dz_present[2] or not (dz_present[0] and dz_present[1]):
            return bwd
        if self._terms_bwd_nf is None:
            self._terms_bwd_nf = self._optional_terms(True, [k for k in range(7) if BUNCH_DST[k] != 2], (16, 32, 16), 8)
        return self._terms_bwd_nf or bwd

    def _fused_ok(self, ns, widths_out, widths_in):
        return (FUSE_BUNCH and ns == NS and set(widths_out) == {32} and set(widths_in) == {32} and self._terms_ops() is not None)

    @staticmethod
    def _slot(dst, src):
        return next((k for k in range(7) if BUNCH_DST[k] == dst and BUNCH_SRC[k] == src), None)

    @staticmethod
    def _blocked_ok(ns, c):
        return (ns * c) % 4 == 0                        # (any width: operands wider than 128 columns go in channel blocks)

    def _spmm(self, op, x):
        return spmm_chunked(op, x)

    def conv_stack(self, x, weights):
        """(states, zeros, first_g, fold): the fields of BunchState that the layers fill."""
        n_layers = len(weights) / 7
        assert n_layers % 1 == 0, "wrong number of weights"                    # TE:177-178
        S, E, ns, _ = x.shape
        cur = [torch.zeros((S, self.sizes[0], ns, 1), device=x.device), x,
               torch.zeros((S, self.sizes[2], ns, 1), device=x.device)]         # TE:179
        zero = [True, False, True]          # levels known to be identically zero (no bias terms: zeros stay zeros)
        # only the node level of the last layer is read (TE:198-201): walk the seven shifts backwards to find which level
        # outputs can reach it, and leave the others uncomputed (their gradient is identically zero as well)
        L = int(n_layers)
        need = [[False] * 3 for _ in range(L + 1)]
        need[L][0] = True
        for i in range(L - 1, 0, -1):
            for k in range(7):
                if self._live[k] and need[i + 1][BUNCH_DST[k]]:
                    need[i][BUNCH_SRC[k]] = True
        states, zeros = [cur], [zero]
        first_g, fold = {}, None
        if self._fold_ok(x, weights, L, ns):
            cur, zero, fold = self._fold_forward(x, weights, need[2])
            states += [[None] * 3, cur]                     # the first layer's output is never materialised
            zeros += [[False] * 3, zero]
        for i in range(2 if fold is not None else 0, L):
            nxt, nzero = [], []
            c_outs = {weights[7 * i + k].shape[1] for k in range(7)}
            c_ins = {cur[l].shape[3] for l in range(3) if not zero[l] and cur[l] is not None}
            if self._fused_ok(ns, c_outs, c_ins):
                # fused layer: one launch for the three levels (scn_terms_forward)
                xs = [None if (zero[l] or cur[l] is None) else cur[l] for l in range(3)]
                Ws = [[None] * 3 for _ in range(3)]
                for k in range(7):
                    if xs[BUNCH_SRC[k]] is not None:
                        Ws[BUNCH_DST[k]][BUNCH_SRC[k]] = weights[7 * i + k]
                outs = self._terms_fwd_for(need[i + 1]).forward(xs, Ws, "relu", need[i + 1])
                cur, zero = outs, [o is None for o in outs]
                states.append(cur)
                zeros.append(zero)
                continue
            for lvl in range(3):
                if not need[i + 1][lvl]:
                    nxt.append(None)
                    nzero.append(True)          # nothing downstream that matters reads it: treated like a zero level
                    continue
                ks = [k for k in self.fwd_slots[lvl] if not zero[BUNCH_SRC[k]]]
                c_out = weights[7 * i + self.fwd_slots[lvl][0]].shape[1]
                if not ks:
                    nxt.append(torch.zeros((S, self.sizes[lvl], ns, c_out), device=x.device))
                    nzero.append(True)
                    continue
                Ws = [weights[7 * i + k] for k in ks]
                if (FUSE_BUNCH and c_out == 1 and all(cur[BUNCH_SRC[k]].shape[3] > 1 for k in ks)
                        and self._blocked_ok(ns, 1)):
                    # one output channel (the last layer): project FIRST, then shift -- (S_k X_k) W_k = S_k (X_k W_k): every
                    # input level is read once and the shifts run on 1-channel tensors
                    ys = [dense_terms_forward([cur[BUNCH_SRC[k]]], [w], 1, "none") for k, w in zip(ks, Ws)]
                    Gs = [self._spmm(self.term_fwd[k], y) for k, y in zip(ks, ys)]
                    one = torch.ones((1, 1), device=x.device, dtype=torch.float32)
                    nxt.append(dense_terms_forward(Gs, [one] * len(Gs), 1, "relu"))
                    nzero.append(False)
                    continue
                if all(self._blocked_ok(ns, cur[BUNCH_SRC[k]].shape[3]) for k in ks):
                    Gs = [self._spmm(self.term_fwd[k], cur[BUNCH_SRC[k]]) for k in ks]
                    if i == 0 and x.shape[3] == 1:          # the shifted 1-channel input S_k x: all the first layer's weight
                        first_g.update(zip(ks, Gs))         # gradient needs (dW_k = sum_p (S_k x)[p] dz[p], one stream over dz)
                    nxt.append(dense_terms_forward(Gs, Ws, c_out, "relu"))
                else:
                    fwd, _ = self._generic_ops()
                    allk = self.fwd_slots[lvl]
                    nxt.append(fwd[lvl].forward([cur[BUNCH_SRC[k]] for k in allk], [weights[7 * i + k] for k in allk],
                                                c_out, "relu"))
                nzero.append(False)
            cur, zero = nxt, nzero
            states.append(cur)
            zeros.append(zero)
        return states, zeros, first_g, fold

    # -- the first TWO layers without a 32-channel gather --------------------------------------------------------------
    # bunch_func starts from [0, flow, 0] (TE:179): after the first layer every level is relu of ONE rank-one term,
    # H1_j = relu(g_j (x) w_j) with g_j = S_k1 x one channel wide (k1 = the slot that feeds level j from the edges), and
    #     relu(g w) = max(g, 0) relu(w) + min(g, 0) min(w, 0)
    # makes the second layer's pre-activation a sum of rank-one terms of SHIFTED SCALARS:
    #     (S_k H1_j) W2_k = (S_k g_j^+) (x) (relu(w_j) W2_k)  +  (S_k g_j^-) (x) (min(w_j, 0) W2_k).
    # So H1 is never formed: seven shifts of two one-channel tensors each (scn_spmm_dual), one rank-one expansion per level
    # (scn_dense_terms_forward) -- and in the backward ONE stream over the second layer's pre-activation gradient per level
    # (u_k^+- = sum_p (S_k g^+-)[p] dZ2[p][:], scn_dense_terms_backward) from which both layers' weight gradients follow by
    # scn_fold1_backward.  Same sums as TE:183-195 in another association order; relu'(0) = 0 as everywhere here.
    def _fold_ok(self, x, weights, L, ns):
        if not (FOLD_BUNCH and FUSE_BUNCH and L >= 3 and x.shape[3] == 1 and self._blocked_ok(ns, 1) and all(self._live)):
            return False
        c1 = {weights[k].shape[1] for k in range(7)}
        c2 = {weights[7 + k].shape[1] for k in range(7)}
        return len(c1) == 1 and len(c2) == 1 and next(iter(c2)) in (16, 32, 64) and all(weights[k].shape[0] == 1 for k in range(7))

    def _fold_forward(self, x, weights, need2):
        lib = _lib.load()
        c1, c2 = weights[0].shape[1], weights[7].shape[1]
        pm = {}                                            # level j -> (g^+, g^-, first-layer slot k1)
        for k1 in range(7):
            if BUNCH_SRC[k1] != 1:
                continue                                   # the node and face levels start at zero: their slots contribute nothing
            g = self._spmm(self.term_fwd[k1], x)
            S = g.shape[0]
            gpm = torch.empty((2 * S,) + tuple(g.shape[1:]), device=g.device, dtype=torch.float32)   # [g^+ slabs | g^- slabs]
            check(lib.scn_split_sign(g.numel(), _dev(g), _dev(gpm[:S]), _dev(gpm[S:]), _stream()), "scn_split_sign")
            pm[BUNCH_DST[k1]] = (gpm, k1)
        terms, outs = {}, []
        for lvl in range(3):
            if not need2[lvl]:
                outs.append(None)
                continue
            Gs, Ws = [], []
            for k2 in self.fwd_slots[lvl]:
                gpm, k1 = pm[BUNCH_SRC[k2]]
                spm = self._spmm(self.term_fwd[k2], gpm)   # both parts in one launch: they are just more slabs of a one-channel tensor
                sp, sm = spm[:spm.shape[0] // 2], spm[spm.shape[0] // 2:]
                ap = torch.empty((1, c2), device=x.device, dtype=torch.float32)
                am = torch.empty_like(ap)
                check(lib.scn_fold1_forward(_dev(weights[k1]), _dev(weights[7 + k2]), c1, c2, _dev(ap), _dev(am), _stream()),
                      "scn_fold1_forward")
                terms[k2] = (sp, sm, k1)
                Gs += [sp, sm]
                Ws += [ap, am]
            outs.append(dense_terms_forward(Gs, Ws, c2, "relu"))
        return outs, [o is None for o in outs], terms

    def _fold_backward(self, fold, dz, dzero, weights, grads):
        """Weight gradients of the first two layers from dz = the gradient of the second layer's pre-activation per level."""
        lib = _lib.load()
        c1, c2 = weights[0].shape[1], weights[7].shape[1]
        for lvl in range(3):
            if dzero[lvl] or dz[lvl] is None:
                continue
            ks = [k2 for k2 in self.fwd_slots[lvl] if k2 in fold]
            Gs, us = [], []
            for k2 in ks:
                Gs += [fold[k2][0], fold[k2][1]]
                us += [torch.zeros((c2, 1), device=dz[lvl].device, dtype=torch.float32) for _ in range(2)]
            dense_terms_backward(Gs, us, dz[lvl], "none", False, us)       # us[q][c] = sum_p Gs[q][p] dz[p][c]  (W unused: no dx)
            for q, k2 in enumerate(ks):
                k1 = fold[k2][2]
                check(lib.scn_fold1_backward(_dev(weights[k1]), _dev(weights[7 + k2]), _dev(us[2 * q]), _dev(us[2 * q + 1]), c1, c2,
                                             _dev(grads[7 + k2]), _dev(grads[k1]), _stream()), "scn_fold1_backward")

    def promotion(self, weights):
        shapes = _shapes(weights)
        if len(shapes) < 14 or len(shapes) % 7:
            return None
        return promoted_width([sh[1] for sh in shapes[:-7]], wide=True)   # above 32: multiples of 32 (32 x 32 MFMA blocks of the dense terms)

    def forward(self, x, last_dev, weights):
        lib = _lib.load()
        P = self.promotion(weights)
        wp = promote_weights(weights, 7, 7, P) if P else None
        states, zeros, first_g, fold = self.conv_stack(x, wp if P else weights)
        nodes_out = states[-1][0]
        S, V, ns, C = nodes_out.shape
        assert C == 1, "bunch readout needs one output channel (TE:198-201)"
        logits = torch.empty((S * ns, self.max_deg), device=x.device, dtype=torch.float32)
        logp = torch.empty_like(logits)
        check(lib.scn_node_readout_forward(S, ns, V, _dev(nodes_out), _dev(self.nbr, torch.int32), self.max_deg,
                                           _dev(last_dev, torch.int32), _dev(logits), _dev(logp), _stream()),
              "scn_node_readout_forward")
        return logp, BunchState(states, zeros, first_g, fold, wp)

    def _backward(self, saved, logp, d_logp, last_dev, weights, grads):
        lib = _lib.load()
        states, zeros, first_g, fold = saved.states, saved.zeros, saved.first_g, saved.fold
        nodes_out = states[-1][0]
        S, V, ns, _ = nodes_out.shape
        dz = [torch.empty_like(nodes_out), None, None]
        dzero = [False, True, True]             # only the node level feeds the loss (TE:198)
        check(lib.scn_node_readout_backward(S, ns, V, _dev(nodes_out), _dev(self.nbr, torch.int32), self.max_deg,
                                            _dev(last_dev, torch.int32), _dev(d_logp.contiguous()), _dev(logp),
                                            ACT["relu"], _dev(dz[0]), _stream()), "scn_node_readout_backward")
        L = len(states) - 1
        for i in reversed(range(L)):
            if i == 1 and fold is not None:             # the first two layers: no input gradients, one stream over dz per level
                self._fold_backward(fold, dz, dzero, weights, grads)
                break
            x, xzero = states[i], zeros[i]
            new_dz, new_zero = [None, None, None], [True, True, True]
            c_dz = {dz[l].shape[3] for l in range(3) if not dzero[l]}
            c_x = {x[l].shape[3] for l in range(3) if not xzero[l] and x[l] is not None}
            if self._fused_ok(ns, c_dz, c_x):
                # fused layer backward on the transposed operator (scn_terms_backward): rows = this layer's input rows
                dzs = [None if dzero[l] else dz[l] for l in range(3)]
                auxs = [None if (xzero[l] or x[l] is None) else x[l] for l in range(3)]
                Ws = [[None] * 3 for _ in range(3)]
                dWs = [[None] * 3 for _ in range(3)]
                for k in range(7):
                    a, b = BUNCH_SRC[k], BUNCH_DST[k]
                    if auxs[a] is not None and dzs[b] is not None:
                        Ws[a][b], dWs[a][b] = weights[7 * i + k], grads[7 * i + k]
                want = [i > 0 and auxs[l] is not None and any(w is not None for w in Ws[l]) for l in range(3)]
                # the layer after the 1-channel first layer: its input gradients feed the first layer's weight gradient and nothing
                # else -- contracted with the shifted input S_k x inside the kernel, never written (dW_k[0][c] = sum_p (S_k x)[p] dx[p][c])
                k_of = {BUNCH_DST[k]: k for k in first_g}
                if (i == 1 and FUSE_FIRST and first_g and all(not want[l] or l in k_of for l in range(3))
                        and all(first_g[k].shape[3] == 1 and weights[k].shape == (1, 32) for k in first_g)):
                    ys = [first_g[k_of[l]].contiguous() if (want[l] and l in k_of) else None for l in range(3)]
                    dWf = [grads[k_of[l]] if ys[l] is not None else None for l in range(3)]
                    _terms_backward_first(self._terms_ops()[1], dzs, Ws, auxs, "relu", ys, dWs, dWf)
                    break
                dxs = _terms_backward(self._terms_bwd_for([d is not None for d in dzs]), dzs, Ws, auxs, "relu", want, dWs)
                dz, dzero = dxs, [d is None for d in dxs]
                continue
            if i == 0 and FUSE_BUNCH and first_g and all(x[l] is None or x[l].shape[3] == 1 for l in range(3)):
                # first layer (one 1-channel input level): the shift sits on the 1-channel side, dW_k[0][c] = sum_p (S_k x)[p] dz[p][c]
                # -- dz of every level streamed once, no transposed SpMM, no gathered 32-channel tensor (scn_conv_dw_first)
                live = [(k, g, dz[BUNCH_DST[k]]) for k, g in first_g.items()
                        if not dzero[BUNCH_DST[k]] and dz[BUNCH_DST[k]] is not None]
                # all or nothing: the per-level loop below accumulates EVERY shift's gradient, so this path may only touch
                # `grads` when it serves all of them (every shift's operator builds its block plan on its own)
                if all(self.term_fwd[k].dw_first_served(d) for k, _, d in live):
                    for k, g, d in live:
                        y = torch.zeros((g.shape[0], g.shape[1], g.shape[2], Y_STRIDE), device=g.device, dtype=torch.float32)
                        y[..., 0] = g[..., 0]
                        dummy = [torch.zeros_like(grads[k]) for _ in range(2)]
                        served = self.term_fwd[k].dw_first(None, y, d, [grads[k]] + dummy)
                        assert served
                    break
            for lvl in range(3):
                ks = [k for k in self.bwd_slots[lvl] if not dzero[BUNCH_DST[k]]]
                if not ks or xzero[lvl]:
                    # a zero input level receives no weight gradient; its own gradient is only needed below layer 0
                    if i > 0 and ks and xzero[lvl]:
                        raise AssertionError("zero level above the first layer")
                    continue
                Ws = [weights[7 * i + k] for k in ks]
                dWs = [grads[7 * i + k] for k in ks]
                if all(self._blocked_ok(ns, dz[BUNCH_DST[k]].shape[3]) for k in ks):
                    Gs = [self._spmm(self.term_bwd[k], dz[BUNCH_DST[k]]) for k in ks]
                    new_dz[lvl] = dense_terms_backward(Gs, Ws, x[lvl], "relu", i > 0, dWs)
                else:
                    _, bwd = self._generic_ops()
                    allk = self.bwd_slots[lvl]
                    dzs = [dz[BUNCH_DST[k]] if not dzero[BUNCH_DST[k]]
                           else torch.zeros((S, self.sizes[BUNCH_DST[k]], ns, weights[7 * i + k].shape[1]), device=x[lvl].device)
                           for k in allk]
                    new_dz[lvl] = bwd[lvl].backward(dzs, [weights[7 * i + k] for k in allk], x[lvl], "relu", i > 0,
                                                    [grads[7 * i + k] for k in allk])
                new_zero[lvl] = False
            dz, dzero = new_dz, new_zero
        return grads


class PlanFn(torch.autograd.Function):
    """plan.forward / plan.backward of either family under autograd (the model functions of trajectory_experiments)."""
    @staticmethod
    def forward(ctx, plan, x, last_dev, *weights):
        logp, saved = plan.forward(x, last_dev, weights)
        ctx.plan, ctx.saved, ctx.last_dev = plan, saved, last_dev
        ctx.save_for_backward(logp, *weights)
        return logp

    @staticmethod
    def backward(ctx, d_logp):
        logp, *weights = ctx.saved_tensors
        grads = [torch.zeros_like(w) for w in weights]
        ctx.plan.backward(ctx.saved, logp, d_logp, ctx.last_dev, weights, grads)
        ctx.saved = None
        return (None, None, None, *grads)


# ----------------------------------------------------------------------------------------------
# plan cache + micro-batching
# ----------------------------------------------------------------------------------------------

def get_scone_plan(S_lower, S_upper, bconds, act, device):
    key = ("scone", id(S_upper), id(bconds), act, str(device))
    if key not in S_lower._cache:
        plan = None
        wide = S_upper.csr.nnz and int(np.diff(S_upper.csr.indptr).max()) >= 128      # such a row cannot enter a block
        if wide and _is_square_of(S_upper, S_lower):
            # rows of S^2 with more than 128 sources do not fit the LDS-blocked plan: compose S (S H) instead of fusing S^2
            plan = PowerPlan(S_lower, S_upper, bconds, act, device)
            if plan.op.plan_info()[0] == 0:
                plan = None
        S_lower._cache[key] = plan if plan is not None else SconePlan(S_lower, S_upper, bconds, act, device)
    return S_lower._cache[key]


def _is_square_of(S2, S):
    if S.shape[0] != S.shape[1] or S2.shape != S.shape:
        return False
    d = (S2.csr - S.csr @ S.csr).tocsr()
    scale = max(1.0, float(abs(S2.csr).max()) if S2.csr.nnz else 1.0)
    return d.nnz == 0 or float(abs(d).max()) <= 1e-9 * scale


def get_bunch_plan(shifts, nbrhoods, device):
    key = ("bunch",) + tuple(id(s) for s in shifts[1:]) + (str(device),)
    if key not in shifts[0]._cache:
        shifts[0]._cache[key] = BunchPlan(shifts, nbrhoods, device)
    return shifts[0]._cache[key]


def micro_batch_size(n_rows_total, widths, n, ns=NS, budget_bytes=None, device=None):
    """Trajectories per micro-batch so that saved activations + two gradient buffers fit the budget; the batch is
    cut into equal micro-batches (multiples of ns)."""
    if budget_bytes is None:
        free, total = torch.cuda.mem_get_info(device)
        budget_bytes = 0.35 * total
    per_sample = 4.0 * n_rows_total * (sum(widths) + 2 * max(widths))
    mb_max = int(budget_bytes // max(per_sample, 1.0))
    mb_max = max(ns, min(mb_max, 16384) // ns * ns)
    if mb_max >= 64:
        mb_max = mb_max // 64 * 64          # whole groups of 16 slabs: what the kernels' slab grouping and grid splits are tuned for
    n_pad = pad_count(n, ns)
    n_chunks = -(-n_pad // mb_max)
    return pad_count(-(-n_pad // n_chunks), ns)


def as_device_weights(weights, device):
    out = []
    for w in weights:
        t = w if torch.is_tensor(w) else torch.as_tensor(np.asarray(w))
        if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(device=device, dtype=torch.float32).contiguous()
        out.append(t)
    return out


def default_device():
    if not torch.cuda.is_available():
        raise RuntimeError("scone_gcn_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


# ----------------------------------------------------------------------------------------------
# multi-hop prediction (multihop.py): the plan-level pieces -- the forward-only call, its micro-batch rule and the field-of-view lists
# ----------------------------------------------------------------------------------------------

INT32_MAX = (1 << 31) - 1


def forward_micro_batch(plan, weights, n):
    """Trajectories per forward of the model functions and of a multi-hop level (multiple of NS): the training micro-batch rule
    (micro_batch_size) on the widths the plan runs."""
    return micro_batch_size(plan.n_rows, plan.layer_widths(weights), n, device=plan.device)


def field_served(plan, weights):
    """Hidden width (16 or 32) when the field-of-view lists serve this model on this plan, else None -- the conditions under which
    SconePlan.activity() serves a data set: a scone / ebli plan with a blocked fused operator (not PowerPlan, not Bunch, no probed
    closure), one 1-channel input and one hidden width of 16 or 32 throughout."""
    if not isinstance(plan, SconePlan) or plan.field_tables_dev() is None:
        return None
    shapes = _shapes(weights)
    L = (len(shapes) - 1) // 3
    if L < 1 or len(shapes) != 3 * L + 1:
        return None
    h = shapes[0][1]
    ok = h in (16, 32) and shapes == [(1, h)] * 3 + [(h, h)] * (3 * (L - 1)) + [(h, 1)]
    return h if ok else None


def field_activity(plan, node_dev, n, n_layers):
    """Field-of-view work lists of one forward over the n leaves node_dev[:n] (int32 device tensor; slab = leaf // NS; -1 = no leaf:
    a dead beam entry, padding), built on the device by scn_field_lists: {"fwd": the lists of layers 1 .. L, "input": the blocks
    of x layer 1 stages, "mode": "field", "active_fraction"}, in the form plan.forward takes as `activity`.  One small copy back (the
    counts).  None when the plan serves no lists (field_tables_dev) or the library does not take the size: the caller runs dense."""
    tabs = plan.field_tables_dev() if isinstance(plan, SconePlan) else None
    if tabs is None or n <= 0:
        return None
    lib = _lib.load()
    nb, S, n_levels = tabs.n_blocks, pad_count(n) // NS, n_layers + 1
    nbytes = int(lib.scn_field_lists_workspace(nb, S, n_levels))
    if nbytes == 0:
        return None
    dev = plan.device
    cap = nb * S                                            # every (block, slab): a level always fits
    i32 = lambda *shape: torch.empty(shape, device=dev, dtype=torch.int32)
    block, ptr, slab, counts = i32(n_levels, nb), i32(n_levels, nb + 1), i32(n_levels, cap), i32(n_levels, 2)
    p = lambda t: _dev(t, torch.int32)
    check(lib.scn_field_lists(n, NS, p(node_dev), plan.n_nodes, p(tabs.top_ptr), p(tabs.top_blk), nb, p(tabs.adj_ptr), p(tabs.adj_blk),
                              n_levels, p(block), p(ptr), p(slab), cap, p(counts), *_workspace(nbytes, dev), _stream()), "scn_field_lists")
    cnt = counts.cpu().numpy()
    lists = [DeviceWorkList(block[l], ptr[l], slab[l], cnt[l, 0], cnt[l, 1]) for l in range(n_levels)]
    total = float(S * nb)
    return {"fwd": lists[1:], "input": lists[0], "mode": "field",
            "active_fraction": {"fwd": [w.items / total for w in lists[1:]], "input": lists[0].items / total}}


def forward_logp(plan, x, last_dev, weights, activity=None):
    """Forward only (no autograd, nothing kept): log-probabilities [S * NS, D] of the slabs x.  activity: work lists
    (field_activity) -- only the listed items are computed, in pooled all-zero buffers that go back all-zero (plan.release)."""
    with torch.no_grad():
        if activity:
            logp, saved = plan.forward(x, last_dev, weights, activity)
            plan.release(saved)
            return logp
        logp, saved = plan.forward(x, last_dev, weights)
        del saved
    return logp
