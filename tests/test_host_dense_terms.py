"""The fp64 references of tests/test_gpu_dense_terms.py, each checked here without the kernels.

dense_terms_ref / dense_terms_bwd_ref are the two contractions of csrc/scn_dense.hip over tensors [..., points, channels]; both are held
against torch.autograd in float64.  fold1_forward_ref / fold1_backward_ref are the two formulas in that file's comment (the rank-one
fold of the first two Bunch layers), held against the unfolded computation relu(g w1^T) W2 and its float64 autograd gradients.
split_sign_ref is the kernel's rule for the positive and the negative part, bit for bit.  Products go through _mm (no BLAS: 0 * NaN must
be NaN); every reference returns each output's sum of |terms| for the bar."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_dispatch import ACT_NAMES, DACT
from tests.test_gpu_nonfinite import ACTS, _mm


def _f64(a):
    return np.asarray(a, np.float64)


def dense_terms_ref(Gs, Ws, act):
    """(act(sum_k G_k W_k), sum_k |G_k| |W_k|): G_k [..., points, c_k], W_k [c_k, c_out]."""
    with np.errstate(invalid="ignore", over="ignore"):
        z = sum(_mm(_f64(g), _f64(w)) for g, w in zip(Gs, Ws))
        s = sum(_mm(np.abs(_f64(g)), np.abs(_f64(w))) for g, w in zip(Gs, Ws))
        return ACTS[act](z), s


def dense_terms_bwd_ref(Gs, Ws, aux, act):
    """(dx, its sum of |terms|, [dW_k], [their sums of |terms|]): dx = (sum_k G_k W_k^T) act'(aux), dW_k = aux^T G_k with
    G_k [points, c_k], W_k [c_aux, c_k], aux [points, c_aux]; act' through the output value (DACT)."""
    a = _f64(aux)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = sum(_mm(_f64(g), _f64(w).T) for g, w in zip(Gs, Ws)) * DACT[act](a)
        sdx = sum(_mm(np.abs(_f64(g)), np.abs(_f64(w)).T) for g, w in zip(Gs, Ws))
        dW = [_mm(a.T, _f64(g)) for g in Gs]
        sdW = [_mm(np.abs(a).T, np.abs(_f64(g))) for g in Gs]
    return dx, sdx, dW, sdW


def _pos(w):
    """relu that keeps a NaN (the kernels' relu_nan)"""
    return np.where(w > 0, w, np.where(np.isnan(w), w, 0.0))


def _neg(w):
    return np.where(w < 0, w, np.where(np.isnan(w), w, 0.0))


def fold1_forward_ref(w1, W2):
    """((Ap, Am), (their sums of |terms|)): Ap[c] = sum_a relu(w1[a]) W2[a][c], Am[c] = sum_a min(w1[a], 0) W2[a][c]."""
    w1, W2 = _f64(w1), _f64(W2)
    with np.errstate(invalid="ignore"):
        Ap, Am = _mm(_pos(w1)[None, :], W2)[0], _mm(_neg(w1)[None, :], W2)[0]
        sp, sm = _mm(np.abs(_pos(w1))[None, :], np.abs(W2))[0], _mm(np.abs(_neg(w1))[None, :], np.abs(W2))[0]
    return (Ap, Am), (sp, sm)


def fold1_backward_ref(w1, W2, up, um):
    """((dW2, dw1), (their sums of |terms|)), the increments:
    dW2[a][c] = relu(w1[a]) up[c] + min(w1[a], 0) um[c],  dw1[a] = [w1[a] > 0] sum_c up[c] W2[a][c] + [w1[a] < 0] sum_c um[c] W2[a][c]."""
    w1, W2, up, um = _f64(w1), _f64(W2), _f64(up), _f64(um)
    wp, wm = _pos(w1), _neg(w1)
    with np.errstate(invalid="ignore"):
        dW2 = wp[:, None] * up[None, :] + wm[:, None] * um[None, :]
        sW2 = np.abs(wp)[:, None] * np.abs(up)[None, :] + np.abs(wm)[:, None] * np.abs(um)[None, :]
        dw1 = np.where(w1 > 0, _mm(W2, up[:, None])[:, 0], 0.0) + np.where(w1 < 0, _mm(W2, um[:, None])[:, 0], 0.0)
        sw1 = np.where(w1 > 0, _mm(np.abs(W2), np.abs(up)[:, None])[:, 0], 0.0) + \
            np.where(w1 < 0, _mm(np.abs(W2), np.abs(um)[:, None])[:, 0], 0.0)
    return (dW2, dw1), (sW2, sw1)


def split_sign_ref(v):
    """(positive part, negative part) in float32 as split_sign_kernel writes them: a NaN stays that NaN in both, +-0.0 gives +0.0 in both."""
    v = np.asarray(v, np.float32)
    zero = np.float32(0.0)
    with np.errstate(invalid="ignore"):
        return np.where(v <= 0, zero, v).astype(np.float32), np.where(v >= 0, zero, v).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------

TACT = {"none": lambda z: z, "tanh": torch.tanh, "relu": torch.relu, "leaky_relu": lambda z: torch.nn.functional.leaky_relu(z, 0.01)}


def _t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


@pytest.mark.parametrize("act", ACT_NAMES)
def test_dense_terms_refs_match_float64_autograd(act):
    """forward: act(sum_k G_k W_k); backward: with aux = act(zp) and L = sum_k <G'_k, aux W_k>, dL/dzp = dx and dL/dW_k = dW_k."""
    rs = np.random.RandomState(11)
    P, cs, c = 50, [5, 3, 1], 7
    Gs = [rs.randn(P, ck).astype(np.float32) for ck in cs]
    Wf = [(0.3 * rs.randn(ck, c)).astype(np.float32) for ck in cs]
    out, s = dense_terms_ref(Gs, Wf, act)
    want = TACT[act](sum(_t64(g) @ _t64(w) for g, w in zip(Gs, Wf))).numpy()
    assert out.shape == (P, c) and np.abs(out - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    assert (s >= np.abs(sum(_mm(_f64(g), _f64(w)) for g, w in zip(Gs, Wf))) - 1e-12).all() and (s > 0).all()

    zp = _t64(rs.randn(P, c), grad=True)
    Wb = [_t64(0.3 * rs.randn(c, ck), grad=True) for ck in cs]
    aux = TACT[act](zp)
    sum((_t64(g) * (aux @ w)).sum() for g, w in zip(Gs, Wb)).backward()
    dx, sdx, dW, sdW = dense_terms_bwd_ref(Gs, [w.detach().numpy() for w in Wb], aux.detach().numpy(), act)
    assert np.abs(dx - zp.grad.numpy()).max() <= 1e-13 * max(1.0, np.abs(dx).max()) and np.abs(dx).max() > 1e-3
    assert (sdx >= np.abs(dx) - 1e-12).all()
    for k in range(3):
        assert dW[k].shape == (c, cs[k]) and np.abs(dW[k] - Wb[k].grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(dW[k]).max())
        assert (sdW[k] >= np.abs(dW[k]) - 1e-12).all()


def test_dense_terms_refs_keep_zero_times_nan():
    """the references do not skip a zero operand: 0 * NaN is NaN down the weight's column, and in the row of dW a NaN of aux feeds"""
    G = np.zeros((4, 3), np.float32)
    W = np.ones((3, 2), np.float32)
    W[1, 1] = np.nan
    out, _ = dense_terms_ref([G], [W], "relu")
    assert np.isnan(out[:, 1]).all() and (out[:, 0] == 0).all()
    aux = np.ones((4, 2), np.float32)
    aux[2, 0] = np.nan
    dx, _, dW, _ = dense_terms_bwd_ref([G], [W.T.copy()], aux, "relu")
    assert np.isnan(dW[0][0]).all() and (dW[0][1] == 0).all()
    assert dx[2, 0] == 0 and np.isnan(dx[:, 1]).all()            # relu'(NaN) = 0 (NaN > 0 is false); 0 * NaN down W's NaN row


def _fold_case(rs, c1, c2, P=40):
    w1 = (0.5 * rs.randn(c1)).astype(np.float32)
    w1[::3] = 0.0                                                   # exact zeros: neither branch
    g = rs.randn(P).astype(np.float32)
    g[::4] = 0.0
    W2 = (0.3 * rs.randn(c1, c2)).astype(np.float32)
    return w1, W2, g


@pytest.mark.parametrize("c1,c2", [(1, 1), (7, 5), (32, 32), (5, 9)])
def test_fold1_refs_match_the_unfolded_layers(c1, c2):
    rs = np.random.RandomState(100 * c1 + c2)
    w1, W2, g = _fold_case(rs, c1, c2)
    if c1 == 1:
        w1[0] = -0.7
    (Ap, Am), (sp, sm) = fold1_forward_ref(w1, W2)
    gp, gm = (_f64(a) for a in split_sign_ref(g))
    z2 = np.maximum(_f64(g)[:, None] * _f64(w1)[None, :], 0.0) @ _f64(W2)
    folded = gp[:, None] * Ap[None, :] + gm[:, None] * Am[None, :]
    assert np.abs(folded - z2).max() <= 1e-13 * max(1.0, np.abs(z2).max()) and np.abs(z2).max() > 1e-3
    assert (sp >= np.abs(Ap)).all() and (sm >= np.abs(Am)).all()

    w1t, W2t = _t64(w1, grad=True), _t64(W2, grad=True)
    dZ2 = rs.randn(len(g), c2)
    (torch.relu(_t64(g)[:, None] * w1t[None, :]) @ W2t * _t64(dZ2)).sum().backward()
    up, um = gp @ dZ2, gm @ dZ2
    (dW2, dw1), (sW2, sw1) = fold1_backward_ref(w1, W2, up, um)
    assert np.abs(dW2 - W2t.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(dW2).max())
    assert np.abs(dw1 - w1t.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(dw1).max())
    assert (dw1[w1 == 0] == 0).all() and (dW2[w1 == 0] == 0).all()
    assert (sW2 >= np.abs(dW2)).all() and (sw1 >= np.abs(dw1) - 1e-12).all()


def test_fold1_refs_with_a_nan_weight():
    rs = np.random.RandomState(5)
    w1, W2, _ = _fold_case(rs, 6, 4)
    w1[2] = np.nan
    (Ap, Am), _ = fold1_forward_ref(w1, W2)
    assert np.isnan(Ap).all() and np.isnan(Am).all()
    (dW2, dw1), _ = fold1_backward_ref(w1, W2, rs.randn(4), rs.randn(4))
    assert np.isnan(dW2[2]).all() and np.isfinite(np.delete(dW2, 2, axis=0)).all()
    assert dw1[2] == 0 and np.isfinite(dw1).all()                  # neither w > 0 nor w < 0


def test_split_sign_ref_bits():
    big = np.finfo(np.float32).max
    nan = np.array([0x7FC00123], np.uint32).view(np.float32)[0]    # a NaN with a payload: it comes back bit for bit
    v = np.array([0.0, -0.0, 1.5, -2.5, 1e-45, -1e-45, 1e-39, -1e-39, big, -big, np.inf, -np.inf, nan], np.float32)
    gp, gm = split_sign_ref(v)
    assert gp.dtype == np.float32 and gm.dtype == np.float32
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
    assert (bits(gp[:2]) == 0).all() and (bits(gm[:2]) == 0).all()                  # +-0.0 -> +0.0 in both
    assert bits(gp[-1]) == 0x7FC00123 and bits(gm[-1]) == 0x7FC00123
    body = v[2:-1]
    pos = body > 0
    assert (bits(gp[2:-1])[pos] == bits(body)[pos]).all() and (bits(gm[2:-1])[pos] == 0).all()
    assert (bits(gm[2:-1])[~pos] == bits(body)[~pos]).all() and (bits(gp[2:-1])[~pos] == 0).all()
    with np.errstate(invalid="ignore"):
        assert (bits(gp + gm)[2:-1] == bits(body)).all()
