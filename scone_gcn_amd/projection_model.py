"""The harmonic projection baseline of Schaub et al. (the reference's trajectory_analysis/projection_model.py = PM) on the device.

PM projects every input flow onto the harmonic space ker(L1), L1 = B1^T B1 + B2 B2^T, reads the projected flow on the edges at the
trajectory's last node and soft-maxes those values over the neighbours; nothing is learned.  The reference takes the space from a
dense scipy.linalg.null_space of the (E, E) matrix (PM:58-71); here an orthonormal basis V (E, dim) is computed once per complex
without ever forming a dense matrix, all in double precision (include/scone_hip.h, "harmonic projection baseline";
csrc/scn_project.hip):

  * probes R = RandomState(seed).randn(E, n_probes), drawn on the host in the caller's edge order;
  * L1 X = L1 R by conjugate gradients from X = 0, all columns at once (scn_csr_apply_f64, scn_cg_update_xr, scn_cg_update_p: the
    step lengths never leave the device, the host reads one word every 32 iterations).  The system is consistent and the iterates
    stay in range(L1), so X -> L1^+ L1 R and H = R - X is the harmonic part of the probes;
  * the Gram matrix H^T H (scn_gram_f64) is diagonalised on the host; eigenvalues <= 1e-12 lambda_max are dropped (the kept ones
    are O(n_probes), the dropped ones rounding noise some fifteen orders below), V = H U Lambda^(-1/2), and the step is repeated
    once on V.  A Gram matrix whose lambda_max <= 1e-12 of the probes' own mean squared norm is noise altogether: dim = 0.
    The dropped eigenvalues are the squared errors of the solve, and those grow with the condition of L1: at |E| ~ 1M they reach
    1e-12 .. 8e-12 against kept ones of 4 and 7 (profiles/projection.txt), so the fixed threshold falls among them.  Hence a second
    look: where two consecutive kept eigenvalues lie more than GAP = 1e6 apart, everything below that gap is dropped as well.
    (Harmonic directions seen through n_probes Gaussian probes give eigenvalues within a few orders of each other -- a Wishart
    matrix's spread -- while the solve's errors lie ten or more orders below them);
  * if no eigenvalue was dropped the probes may be fewer than the dimension: n_probes doubles and the computation starts again, up
    to SCN_PROJECT_MAX_PROBES = 32; beyond that ValueError.

Prediction (PM:80-96, 108) is one launch, a wave per trajectory (scn_project_predict): c = V^T f over the flow's non-zero entries,
logit[slot(j)] = B1[j, e] (V[e, :] . c) for every edge e at the last node, soft-max over all D slots with the padding at logit 0,
first maximum.  Where the reference draws from NumPy's unseeded global stream -- the other neighbour of the 2-target test, PM:119
-- the draw is the Philox uniform of (seed, row), as in markov_model.Markov_Model.test_2_target.

Edge flips.  The result does not depend on -flip_edges: with F the diagonal of flips, F V spans the kernel of F L1 F, the flipped
flow is F f, and in the logit (B1 F)[j, e] ((F V)(F V)^T F f)[e] the signs cancel.  So the baseline always works on the unflipped
complex and the unflipped flows.

All math of the hot path runs in libscone_hip.so; nothing falls back to the CPU.  The (k, k) products around the eigendecomposition
and H U are torch fp64 calls.
"""
import ctypes

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib, ops
from ._lib import SCN_CG_FLAG_ALL_FROZEN, SCN_CG_FLAG_ITERATIONS, SCN_CG_FLAG_WORDS, SCN_CG_STATE_DOUBLES, SCN_PROJECT_MAX_K, check
from .complex import Shift, SimplicialComplex
from .ops import INT32_MAX
from .synthetic_data_gen import SparseFlows

SCN_PROJECT_MAX_PROBES = 32
DROP = 1e-12                  # eigenvalues of the Gram matrix at or below DROP * lambda_max are not part of the space
GAP = 1e6                     # nor are those below two consecutive kept eigenvalues that lie further apart than this factor
CHECK_EVERY = 32              # iterations between two reads of the all-frozen word

_F64, _I32 = torch.float64, torch.int32


def _p(t, dtype):
    return ops._dev(t, dtype) if t.numel() else None


def kept_eigenvalues(w, scale):
    """Which of the Gram matrix's eigenvalues w (ascending) span the harmonic space: those above DROP * lambda_max, without those
    below a gap wider than GAP among them; none at all when lambda_max <= DROP * scale, the probes' mean squared norm."""
    w = np.asarray(w, np.float64)
    if not w[-1] > DROP * scale:
        return np.zeros(len(w), bool)
    keep = w > DROP * w[-1]
    k = np.flatnonzero(keep)
    wide = np.flatnonzero(w[k[1:]] > GAP * w[k[:-1]])
    if len(wide):
        keep[:k[wide[-1] + 1]] = False
    return keep


class Projection_Model:
    def __init__(self, n_probes=8, seed=0, tol=1e-12, max_iter=50000, device=None):
        """
        :param n_probes: random probe columns the harmonic space is sifted from (doubled while none of them drops out)
        :param seed: of the probes' RandomState
        :param tol: a column is converged at |r| <= tol |r0|
        :param max_iter: conjugate-gradient iterations after which embed() raises RuntimeError
        """
        if int(n_probes) != n_probes or not 1 <= int(n_probes) <= SCN_PROJECT_MAX_PROBES:
            raise ValueError("n_probes must be an integer in 1 .. %d, got %r" % (SCN_PROJECT_MAX_PROBES, n_probes))
        if not 0.0 < tol < 1.0 or int(max_iter) < 1:
            raise ValueError("tol must lie in (0, 1) and max_iter be at least 1")
        self.n_probes, self.seed, self.tol, self.max_iter, self.device = int(n_probes), int(seed), float(tol), int(max_iter), device
        self.basis = self.dim = self.iterations = self.residual = self.n_probes_used = None
        self.gram_eigenvalues = None                            # of the last H^T H, ascending (what was kept and what was dropped)
        self._V = None                                          # (E, dim) fp64 on the device, device edge order

    # ---- plumbing ----
    def _up(self, a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device).to(dtype).contiguous()

    def _gram(self, a, b):
        """a^T b of two (n, k) fp64 device arrays (scn_gram_f64) as a (ka, kb) device tensor."""
        lib = _lib.load()
        n, ka, kb = a.shape[0], a.shape[1], b.shape[1]
        parts = torch.empty((lib.scn_gram_parts(n), ka * kb), dtype=_F64, device=self.device)
        out = torch.zeros((ka, kb), dtype=_F64, device=self.device)
        check(lib.scn_gram_f64(n, ka, kb, _p(a, _F64), _p(b, _F64), _p(parts, _F64), _p(out, _F64), ops._stream()), "scn_gram_f64")
        return out

    def _set_tables(self, n_nodes, n_edges, perm, tables, nbrhoods):
        inc_ptr, inc_edge, inc_sign, edge_nodes = tables
        nbr = np.ascontiguousarray(nbrhoods, np.int32)
        self.n_nodes, self.n_edges, self.width = int(n_nodes), int(n_edges), int(nbr.shape[1])
        self.perm = np.asarray(perm, np.int64)
        self.h_nbr, self.h_deg = nbr, (nbr >= 0).sum(axis=1).astype(np.int32)
        self._tab = [self._up(inc_ptr, _I32), self._up(inc_edge, _I32), self._up(inc_sign, torch.float32), self._up(edge_nodes, _I32),
                     self._up(nbr, _I32), self._up(self.h_deg, _I32)]

    def _solve(self, L, R):
        """X of L X = L R by conjugate gradients from 0 (all on the device): (X, iterations, largest relative residual, converged)."""
        lib = _lib.load()
        E, k = R.shape
        rowptr, col, val = self._up(L.indptr, _I32), self._up(L.indices, _I32), self._up(L.data, _F64)
        W = lib.scn_project_parts(E, k)
        x, r, p, ap = (torch.zeros((E, k), dtype=_F64, device=self.device) for _ in range(4))
        pap, rrp = (torch.zeros((W, k), dtype=_F64, device=self.device) for _ in range(2))
        state = torch.zeros((SCN_CG_STATE_DOUBLES,), dtype=_F64, device=self.device)
        flags = torch.zeros((SCN_CG_FLAG_WORDS,), dtype=_I32, device=self.device)
        flags[SCN_CG_FLAG_ITERATIONS] = -1
        st = ops._stream()
        csr = (_p(rowptr, _I32), _p(col, _I32), _p(val, _F64))
        P = lambda t: _p(t, _F64)
        check(lib.scn_csr_apply_f64(E, k, *csr, P(R), P(r), P(pap), st), "scn_csr_apply_f64")
        check(lib.scn_cg_update_xr(E, k, 0, 1, None, None, None, P(x), P(r), P(state), _p(flags, _I32), P(rrp), st), "scn_cg_update_xr")
        check(lib.scn_cg_update_p(E, k, 0, 1, self.tol, P(rrp), P(r), P(p), P(state), _p(flags, _I32), st), "scn_cg_update_p")
        done, it = bool(flags[SCN_CG_FLAG_ALL_FROZEN].item()), 0
        while not done and it < self.max_iter:
            it += 1
            check(lib.scn_csr_apply_f64(E, k, *csr, P(p), P(ap), P(pap), st), "scn_csr_apply_f64")
            check(lib.scn_cg_update_xr(E, k, it, 0, P(pap), P(p), P(ap), P(x), P(r), P(state), _p(flags, _I32), P(rrp), st),
                  "scn_cg_update_xr")
            check(lib.scn_cg_update_p(E, k, it, 0, self.tol, P(rrp), P(r), P(p), P(state), _p(flags, _I32), st), "scn_cg_update_p")
            if it % CHECK_EVERY == 0 or it == self.max_iter:
                done = bool(flags[SCN_CG_FLAG_ALL_FROZEN].item())
        s = state.cpu().numpy()
        rr, rr0 = s[((it + 1) & 1) * SCN_PROJECT_MAX_K:][:k], s[2 * SCN_PROJECT_MAX_K:][:k]
        rel = np.sqrt(rr[rr0 > 0] / rr0[rr0 > 0])
        return x, (int(flags[SCN_CG_FLAG_ITERATIONS].item()) if done else it), (float(rel.max()) if len(rel) else 0.0), done

    def _sift(self, H, scale):
        """The Gram step: (V = H U Lambda^(-1/2) over the kept eigenvalues, all eigenvalues ascending)."""
        w, U = np.linalg.eigh(self._gram(H, H).cpu().numpy())
        keep = kept_eigenvalues(w, scale)
        T = torch.from_numpy(np.ascontiguousarray(U[:, keep] / np.sqrt(w[keep]))).to(self.device)
        return (H @ T).contiguous(), w

    # ---- the basis ----
    def embed(self, sc, B2=None):
        """
        :param sc: a SimplicialComplex, or B1 with B2 as the second argument (dense or scipy.sparse, columns in sorted edge order)
        Computes the orthonormal basis of ker(L1) (PM:58-71) and sets dim, basis (E, dim) in the caller's edge order, iterations,
        residual (the largest |r| / |r0| of a column at the end) and n_probes_used.  RuntimeError, and no basis, when max_iter is
        reached; ValueError when SCN_PROJECT_MAX_PROBES probes do not exhaust the space.
        """
        if not isinstance(sc, SimplicialComplex):
            if B2 is None:
                raise TypeError("embed() takes a SimplicialComplex or B1, B2")
            sc = SimplicialComplex.from_incidence(sp.csr_matrix(sc), sp.csr_matrix(B2))
        if self.device is None:
            self.device = ops.default_device()
        self.basis = self.dim = self._V = None
        E = sc.cx.n_edges
        L_lo, L_up = sc.hodge_laplacians()
        L = Shift((L_lo + L_up).tocsr(), sc.layout, 1, 1).device_csr()
        if L.nnz >= INT32_MAX:
            raise ValueError("L1 holds %d entries; fewer than 2^31 - 1 are served" % L.nnz)
        order = sc.layout.order[1]
        n_probes = self.n_probes
        with torch.cuda.device(self.device):
            self._set_tables(sc.cx.n_nodes, E, sc.layout.perm[1], sc.bconds().incidence_tables(), sc.nbrhoods)
            while True:
                R_host = np.random.RandomState(self.seed).randn(E, n_probes)
                R = self._up(R_host[order], _F64)
                X, self.iterations, self.residual, done = self._solve(L, R)
                if not done:
                    raise RuntimeError("conjugate gradients did not converge in %d iterations: largest relative residual %.3e"
                                       % (self.max_iter, self.residual))
                V, w = self._sift(R - X, float((R_host ** 2).sum() / n_probes))
                if V.shape[1] < n_probes:
                    break
                if 2 * n_probes > SCN_PROJECT_MAX_PROBES:
                    raise ValueError("%d probes keep every eigenvalue: the harmonic space has at least %d dimensions"
                                     % (n_probes, n_probes))
                n_probes *= 2
            if V.shape[1]:
                V, _ = self._sift(V, 1.0)                        # once more: V^T V = I to rounding
            self._V, self.gram_eigenvalues, self.n_probes_used = V, w, n_probes
            self.dim = int(V.shape[1])
            self.basis = V.cpu().numpy()[sc.layout.perm[1]]
        return self

    @classmethod
    def from_basis(cls, V, B1, nbrhoods=None, device=None):
        """A model on a basis computed elsewhere (PM's project_flows(V, B1, ...)): V (E, dim) and B1 (V, E), dense or sparse, in the
        caller's edge order; the neighbour table is the graph's own unless given."""
        self = cls(device=device)
        self.device = ops.default_device() if device is None else device
        B1 = sp.csr_matrix(B1)
        B1.sort_indices()
        V = np.asarray(V, np.float64).reshape(B1.shape[1], -1)
        if V.shape[1] > SCN_PROJECT_MAX_K:
            raise ValueError("a basis of %d columns; at most %d are served" % (V.shape[1], SCN_PROJECT_MAX_K))
        csc = B1.tocsc()
        if not np.all(np.diff(csc.indptr) == 2):
            raise ValueError("every column of B1 must hold the two endpoints of an edge")
        edge_nodes = csc.indices.reshape(-1, 2).astype(np.int32)
        if nbrhoods is None:
            A = sp.coo_matrix((np.ones(2 * len(edge_nodes)), (np.r_[edge_nodes[:, 0], edge_nodes[:, 1]],
                                                              np.r_[edge_nodes[:, 1], edge_nodes[:, 0]])), shape=(B1.shape[0],) * 2).tocsr()
            A.sort_indices()
            deg = np.diff(A.indptr)
            nbrhoods = -np.ones((B1.shape[0], max(1, int(deg.max()))), np.int64)
            nbrhoods[np.repeat(np.arange(B1.shape[0]), deg), np.arange(A.nnz) - np.repeat(A.indptr[:-1], deg)] = A.indices
        with torch.cuda.device(self.device):
            self._set_tables(B1.shape[0], B1.shape[1], np.arange(B1.shape[1]),
                             (B1.indptr, B1.indices, B1.data.astype(np.float32), edge_nodes), nbrhoods)
            self._V = self._up(V, _F64)
        self.basis, self.dim = V, int(V.shape[1])
        return self

    # ---- flows ----
    def _need_basis(self):
        if self._V is None:
            raise RuntimeError("embed() first")

    def _flows(self, flows):
        """(ptr int32, device edge ids int32, values fp64) of a SparseFlows, an (E, N) array as PM holds it, or (N, E, 1)."""
        if not isinstance(flows, SparseFlows):
            X = np.asarray(flows.cpu() if torch.is_tensor(flows) else flows, np.float64)
            if X.ndim == 3 and X.shape[1:] == (self.n_edges, 1):
                X = X[:, :, 0].T
            if X.ndim != 2 or X.shape[0] != self.n_edges:
                raise ValueError("flows must be (E, N) with E = %d, (N, E, 1) or a SparseFlows" % self.n_edges)
            cols, rows = np.nonzero(X.T)
            ptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=X.shape[1]))])
            idx, val = rows, X[rows, cols]
        else:
            if flows.n_edges != self.n_edges:
                raise ValueError("the flows live on %d edges, the complex has %d" % (flows.n_edges, self.n_edges))
            ptr, idx, val = np.asarray(flows.ptr), np.asarray(flows.idx, np.int64), np.asarray(flows.val, np.float64)
        if ptr[-1] >= INT32_MAX:
            raise ValueError("the flows hold %d entries; fewer than 2^31 - 1 are served" % ptr[-1])
        if len(idx) and (idx.min() < 0 or idx.max() >= self.n_edges):
            raise ValueError("a flow names an edge outside the complex")
        return np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(self.perm[idx], np.int32), np.ascontiguousarray(val, np.float64)

    def project(self, flows):
        """The harmonic parts V V^T f of the flows, (N, E) in the caller's edge order (PM:84): V^T F through scn_gram_f64 on dense
        (E, <= 32) slices of the batch, V (V^T F) in torch."""
        self._need_basis()
        ptr, idx, val = self._flows(flows)
        N, E = len(ptr) - 1, self.n_edges
        out = np.zeros((N, E))
        if self.dim == 0 or N == 0:
            return out
        with torch.cuda.device(self.device):
            d_idx, d_val = self._up(idx, torch.int64), self._up(val, _F64)
            row = self._up(np.repeat(np.arange(N), np.diff(ptr)), torch.int64)
            for i0 in range(0, N, SCN_PROJECT_MAX_K):
                nb = min(SCN_PROJECT_MAX_K, N - i0)
                F = torch.zeros((E, nb), dtype=_F64, device=self.device)
                sl = slice(int(ptr[i0]), int(ptr[i0 + nb]))
                F.index_put_((d_idx[sl], row[sl] - i0), d_val[sl], accumulate=True)
                C = self._gram(self._V, F)
                out[i0:i0 + nb] = (self._V @ C).T.cpu().numpy()[:, self.perm]
        return out

    def predict_all(self, flows, last_nodes):
        """(probs (N, D), logits (N, D), argmax (N,)) of scn_project_predict as host arrays."""
        self._need_basis()
        ptr, idx, val = self._flows(flows)
        last = np.asarray(last_nodes.cpu() if torch.is_tensor(last_nodes) else last_nodes).astype(np.int64).ravel()
        N, D = len(ptr) - 1, self.width
        if len(last) != N:
            raise ValueError("flows and last_nodes disagree on the number of trajectories")
        if N and (last.min() < 0 or last.max() >= self.n_nodes):
            raise ValueError("a last node lies outside the complex")
        with torch.cuda.device(self.device):
            logits, probs = (torch.empty((N, D), dtype=_F64, device=self.device) for _ in range(2))
            arg = torch.empty((N,), dtype=_I32, device=self.device)
            err = torch.full((1,), INT32_MAX, dtype=_I32, device=self.device)
            d_ptr, d_idx, d_val, d_last = self._up(ptr, _I32), self._up(idx, _I32), self._up(val, _F64), self._up(last, _I32)
            t = self._tab
            check(_lib.load().scn_project_predict(N, self.dim, self.n_edges, _p(self._V, _F64), _p(d_ptr, _I32), _p(d_idx, _I32),
                                                  _p(d_val, _F64), _p(d_last, _I32), self.n_nodes, _p(t[0], _I32), _p(t[1], _I32),
                                                  _p(t[2], torch.float32), _p(t[3], _I32), D, _p(t[4], _I32), _p(t[5], _I32),
                                                  _p(logits, _F64), _p(probs, _F64), _p(arg, _I32), _p(err, _I32), ops._stream()),
                  "scn_project_predict")
            i = int(err.item())
            if i != INT32_MAX:
                raise ValueError("trajectory %d: its last node's edges and the neighbour table disagree" % i)
            return probs.cpu().numpy(), logits.cpu().numpy(), arg.cpu().numpy().astype(np.int64)

    # ---- whole paths: the teacher-forced score of every node (scn_project_path_scores) ----
    def path_records(self, paths, with_coef=False):
        """(ptr, nodes, logp, rank, mass, coef) of scn_project_path_scores on the host: one record per node position of the paths (a
        list of node lists or a (ptr, nodes) pair), coef (T, dim) only when asked for.  The paths go up in one buffer, one launch, and
        the records and the error word come back in one.  ValueError for a step between two nodes that share no edge."""
        from .markov_model import ragged
        self._need_basis()
        ptr, nodes = ragged(paths)
        P, T, k = len(ptr) - 1, len(nodes), self.dim
        if T == 0:
            return ptr, nodes, np.zeros(0), np.zeros(0, np.int32), np.zeros(0), (np.zeros((0, k)) if with_coef else None)
        n_coef = T * k if with_coef else 0
        with torch.cuda.device(self.device):
            up = self._up(np.concatenate([ptr, nodes]), _I32)
            d_ptr, d_nodes = up[:P + 1], up[P + 1:]
            out = torch.empty((2 * T + n_coef + T + 1,), dtype=_F64, device=self.device)   # logp | mass | coef | rank and err (int32)
            logp, mass, coef = out[:T], out[T:2 * T], out[2 * T:2 * T + n_coef]
            words = out[2 * T + n_coef:].view(_I32)
            rank, err = words[:T], words[T:T + 1]
            err.fill_(INT32_MAX)
            t = self._tab
            check(_lib.load().scn_project_path_scores(P, _p(d_ptr, _I32), _p(d_nodes, _I32), k, self.n_edges, _p(self._V, _F64),
                                                      self.n_nodes, _p(t[0], _I32), _p(t[1], _I32), _p(t[2], torch.float32),
                                                      _p(t[3], _I32), self.width, _p(t[4], _I32), _p(t[5], _I32), _p(logp, _F64),
                                                      _p(rank, _I32), _p(mass, _F64), _p(coef, _F64), _p(err, _I32), ops._stream()),
                  "scn_project_path_scores")
            host = out.cpu().numpy()
        words = host[2 * T + n_coef:].view(np.int32)
        bad = int(words[T])
        if bad != INT32_MAX:
            p = int(np.searchsorted(ptr, bad, side="right")) - 1
            raise ValueError("path %d, position %d: nodes %d and %d share no edge of the complex"
                             % (p, bad - int(ptr[p]), nodes[bad], nodes[bad + 1]))
        return ptr, nodes, host[:T], words[:T], host[T:2 * T], (host[2 * T:2 * T + n_coef].reshape(T, k) if with_coef else None)

    def path_step_log_probs(self, paths, min_prefix=2, normalise=False):
        """The teacher-forced scores of every step of every path under the projection, as Scone_GCN.path_step_log_probs gives the
        model's: a path_scores.PathScores over the items (path p, prefix of k = max(min_prefix, 1) .. len - 1 nodes), each predicting
        p[k] from the harmonic coefficients of the k - 1 steps before it.  No prefix flow is built: the coefficients are a running
        sum along the path.  logp is the log of predict()'s probability at the slot taken (the padding slots inside the soft-max),
        minus mass when normalised; rank counts the real neighbours the projection puts before it, mass is the log of the
        probability it leaves on real neighbours."""
        from . import path_scores
        ptr, _, logp, rank, mass, _ = self.path_records(paths)
        item_ptr, item_path, item_len = path_scores.path_items(ptr, min_prefix)
        at = path_scores.item_positions(ptr, item_path, item_len)
        logp, mass = logp[at], mass[at]
        return path_scores.PathScores(item_ptr, logp - mass if normalise else logp, rank[at].astype(np.int64), mass, item_len)

    def path_log_likelihood(self, paths, min_prefix=2, normalise=False):
        """(ll [P] float64 = the sum of every path's step log-probabilities, n_steps [P] int64)."""
        from . import path_scores
        sc = self.path_step_log_probs(paths, min_prefix, normalise)
        return path_scores.segment_sums(sc.logp, sc.ptr), np.diff(sc.ptr)

    def score_paths(self, paths, mask=None, min_prefix=2, normalise=False):
        """The dict of Scone_GCN.score_paths over the paths with mask == 1 (all without a mask): mean_step_logp, perplexity,
        accuracy (rank 0), n_steps."""
        from . import path_scores
        from .markov_model import select_paths
        return path_scores.summary(self.path_step_log_probs(select_paths(paths, mask), min_prefix, normalise))

    def predict(self, flows, last_nodes):
        """Probabilities (N, D) of the next node by slot of the last node's sorted neighbourhood (PM:80-96); the padding slots
        enter the soft-max with logit 0, as they do there."""
        return self.predict_all(flows, last_nodes)[0]

    @staticmethod
    def _rows(y, mask):
        y = np.asarray(y.cpu() if torch.is_tensor(y) else y, np.float64)
        y = y.reshape(y.shape[0], -1)
        rows = np.arange(len(y)) if mask is None else np.flatnonzero(np.asarray(mask) == 1)
        return y, rows

    def _select(self, flows, rows):
        if isinstance(flows, SparseFlows):
            return flows.select(rows)
        X = np.asarray(flows.cpu() if torch.is_tensor(flows) else flows)
        return X[rows] if X.ndim == 3 else X[:, rows]

    def test(self, flows, last_nodes, y, mask=None):
        """(loss, acc) over the rows with mask == 1 (all without a mask).  y: one-hot targets (N, D) or (N, D, 1).  The loss is
        PM:98-105 -- log 0 counts as 0, the sum is divided by the number of rows -- the accuracy PM:107-108."""
        y, rows = self._rows(y, mask)
        probs, _, arg = self.predict_all(self._select(flows, rows), np.asarray(last_nodes)[rows])
        return loss(y[rows].T, probs.T), float(np.average(np.argmax(y[rows], axis=1) == arg))

    def test_2_target(self, flows, last_nodes, y, n_nbrs, seed=0):
        """(2-target accuracy, drawn slots) (PM:110-126): the target's probability against that of one other neighbour of the last
        node, drawn on the device from (seed, row).  ValueError for a last node with a single neighbour (np.random.choice([])
        raises in the reference too)."""
        y, rows = self._rows(y, None)
        n_nbrs = np.asarray(n_nbrs).astype(np.int64).ravel()
        if len(n_nbrs) != len(y):
            raise ValueError("y and n_nbrs disagree on the number of trajectories")
        single = np.flatnonzero(n_nbrs < 2)
        if len(single):
            raise ValueError("trajectory %d ends at a node with no second neighbour to compare the target with" % int(single[0]))
        probs = self.predict(flows, last_nodes)
        n, D = probs.shape
        with torch.cuda.device(self.device):
            score = torch.empty((n,), dtype=torch.float32, device=self.device)
            other = torch.empty((n,), dtype=_I32, device=self.device)
            err = torch.full((1,), INT32_MAX, dtype=_I32, device=self.device)
            d_probs, d_t, d_n = self._up(probs, _F64), self._up(np.argmax(y, axis=1), _I32), self._up(n_nbrs, _I32)
            check(_lib.load().scn_project_two_target(n, D, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _p(d_probs, _F64), _p(d_t, _I32),
                                                     _p(d_n, _I32), _p(score, torch.float32), _p(other, _I32), _p(err, _I32),
                                                     ops._stream()), "scn_project_two_target")
            i = int(err.item())
            if i != INT32_MAX:
                raise ValueError("trajectory %d: %d neighbours for %d slots" % (i, n_nbrs[i], D))
            return float(score.cpu().numpy().astype(np.float64).sum()) / n, other.cpu().numpy().astype(np.int64)


# ----------------------------------------------------------------------------------------------
# the reference's module functions: same names and argument order (PM:16-194)
# ----------------------------------------------------------------------------------------------

def build_flow(G, path, edge_to_idx):
    """Builds a flow from this path on the given graph (PM:16-27): +1 along an edge's stored orientation, -1 against it."""
    flow = np.zeros(len(G.edges))
    for a, b in zip(path[:-1], path[1:]):
        if (a, b) in edge_to_idx:
            flow[edge_to_idx[(a, b)]] = 1
        else:
            flow[edge_to_idx[(b, a)]] = -1
    return flow


def embed(B1, B2):
    """Embeds the complex in the null space of its L1 matrix; returns (V, B1) (PM:58-71) -- V from the device, never a dense L1."""
    return Projection_Model().embed(B1, B2).basis, B1


def project_flows(V, B1, flows, last_nodes, nbrhoods, max_deg):
    """Project flows (E, N) onto the null space; return probabilities of each suffix for each flow, (max_deg, N) (PM:80-96).
    nbrhoods[i] must be the sorted neighbourhood of last_nodes[i], which is what PM:179 passes."""
    pm = Projection_Model.from_basis(V, B1)
    last = np.asarray(last_nodes).astype(np.int64).ravel()
    for i, nb in enumerate(nbrhoods):
        if not np.array_equal(np.asarray(nb), pm.h_nbr[last[i], :pm.h_deg[last[i]]]):
            raise ValueError("nbrhoods[%d] is not the sorted neighbourhood of node %d" % (i, last[i]))
    if max_deg < pm.width:
        raise ValueError("max_deg = %d, but a node has %d neighbours" % (max_deg, pm.width))
    if max_deg > pm.width:                                       # more padding: more zero logits in the soft-max
        wide = -np.ones((pm.n_nodes, int(max_deg)), np.int64)
        wide[:, :pm.width] = pm.h_nbr
        pm = Projection_Model.from_basis(V, B1, nbrhoods=wide)
    return pm.predict(flows, last).T


def loss(y, y_hat):
    """Cross-entropy of the predicted distributions y_hat (D, N) against the one-hot y (D, N): log 0 counts as 0 and the sum is
    divided by the number of columns (PM:98-105)."""
    y_hat = np.asarray(y_hat, np.float64)
    with np.errstate(divide="ignore"):
        lg = np.log(y_hat)
    lg[lg == -np.inf] = 0
    return float(-np.sum(lg * np.asarray(y)) / np.asarray(y).shape[1])


def accuracy(y, y_hat):
    return float(np.average(np.argmax(y, axis=0) == np.argmax(y_hat, axis=0)))              # PM:107-108


def accuracy_2target(y, preds, n_nbrs, seed=0):
    """The ratio of the time that the true suffix has higher predicted probability than a random other neighbour (PM:110-126);
    the draw is the device's, keyed by (seed, column)."""
    y, preds = np.asarray(y, np.float64), np.ascontiguousarray(np.asarray(preds, np.float64).T)
    n, D = preds.shape
    n_nbrs = np.asarray(n_nbrs).astype(np.int64).ravel()
    if np.any(n_nbrs < 2):
        raise ValueError("column %d has no second neighbour to compare the target with" % int(np.flatnonzero(n_nbrs < 2)[0]))
    dev = ops.default_device()
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(t).contiguous()
    with torch.cuda.device(dev):
        score, other = torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=_I32, device=dev)
        err = torch.full((1,), INT32_MAX, dtype=_I32, device=dev)
        d_p, d_t, d_n = up(preds, _F64), up(np.argmax(y, axis=0), _I32), up(n_nbrs, _I32)
        check(_lib.load().scn_project_two_target(n, D, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _p(d_p, _F64), _p(d_t, _I32),
                                                 _p(d_n, _I32), _p(score, torch.float32), _p(other, _I32), _p(err, _I32), ops._stream()),
              "scn_project_two_target")
        if int(err.item()) != INT32_MAX:
            raise ValueError("column %d: more neighbours than slots" % int(err.item()))
        return float(score.cpu().numpy().astype(np.float64).sum()) / n


def eval_dataset(G, paths, last_nodes, y, edge_to_idx, idx_to_edge, target_nodes, B1, B2, max_deg, flows=None, two_target=False,
                 target_nodes_2hop=None):
    """Runs the experiment on the given data set (PM:164-194): (ce, acc).  y is (D, N), flows (E, N) or built from paths."""
    pm = Projection_Model().embed(B1, B2)
    if flows is None:
        flows = np.array([build_flow(G, path, edge_to_idx) for path in paths]).T
    last = np.asarray(last_nodes).astype(np.int64).ravel()
    if max_deg != pm.width:
        preds = project_flows(pm.basis, B1, flows, last, [pm.h_nbr[n, :pm.h_deg[n]] for n in last], max_deg)
    else:
        preds = pm.predict(flows, last).T
    ce = loss(y, preds)
    acc = accuracy_2target(y, preds, pm.h_deg[last]) if two_target else accuracy(y, preds)
    return ce, acc
