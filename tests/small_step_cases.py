"""Seeded cases for the one-launch step (csrc/scn_small.hip) AT THE LIMITS OF ITS LAYOUT: graphs, hand-built shift pairs, data and the
kernel's host-side selection restated.  NumPy / SciPy only -- tests/test_host_small_step_limits.py proves on the CPU what every case
is, tests/test_gpu_small_step_limits.py runs them.

Graphs (synthetic_data_gen.Complex without faces; the shifts are hand-built, so nothing is triangulated):
  plain   a ring with chords (degree <= 3) and one node without edges
  hub     node 0 with 64 neighbours of degree 8 (the hub and 7 leaves each): max_deg = 64 = SM_MAXD and, for the hub as last node,
          64 x 8 = 512 = SM_ITEMS readout items; the edges beyond these 512 are a path through the leaves (degree <= 3) that goes on
          through new nodes; one node without edges
  hub24   the same with 24 neighbours of degree 9 (216 edges), for the twelve-wave sizes (|E| <= 384)

Operators: a pair (lower, upper) of |E| x |E| matrices on a shared pattern, built in DEVICE row order and carried to the caller's
order through the complex's layout.  Rows of exactly 0 / 1 / 11 / 12 / 13 / 24 / 25 / 60 / 100 entries (CLASSES; twelve entries of a
row live in registers, SM_CH) stand at row 0, rows 15 / 16, the first and last row of every 128-row block, the last row and every row
of a partial last tile (special_rows); a row of every class has an entry in column 0 and one in column |E| - 1, one present in the
lower array only and one in the upper only.  Every other row has at most 11 entries.  Values are randn / sqrt(row length), float32.
  sym     pattern and values symmetric (conv_T is conv)
  nonsym  sym with a seeded third of the entries below the diagonal dropped from the rows that are not special (the special rows keep
          their exact lengths in A; in A^T they are shorter): same_t = 0, two different overflow lists
  tonly   A = B^T for a B with the special rows and at most 11 entries per COLUMN: no row of A has a tail, rows of A^T do
          (n_ovf = 0 < n_ovf_t)
`extra` adds that many further rows of 100 entries at seeded places: it sets the length of the overflow list, which decides between
the LDS and memory for the list and for the first layer's shifted input.
"""
import numpy as np
import scipy.sparse as sp

SM_CH, SM_MAXD, SM_ITEMS, SM_MAXT = 12, 64, 512, 9
LDS_BYTES = 160 * 1024
CLASSES = (0, 1, 11, 12, 13, 24, 25, 60, 100)
ORDINARY_MAX = 11
ACTS = ("none", "tanh", "relu", "leaky_relu")

# ------------------------------------------------------------------------------------------------------------------
# the kernel's host-side selection, restated (small_waves / small_lds / small_blocks / small_form of csrc/scn_small.hip)
# ------------------------------------------------------------------------------------------------------------------


def restate_form(n_edges, n_ovf, n_ovf_t, paired, same_t):
    """dict with the fields of scn_small_step_layout for a launch on |E| = n_edges with overflow lists of n_ovf / n_ovf_t entries."""
    tiles = (n_edges + 15) // 16
    epad = 16 * tiles
    waves = 12 if tiles <= 24 else 8
    misc = (64 + 64 + 16 + 80 + 3 * SM_ITEMS + 64 * 16 + waves * 48) * 4
    buf, red = epad * 64, waves * 768 * 4
    total = 2 * buf + 768 * 4 + misc + epad * 4 + (0 if buf >= red else red)
    supported = n_edges <= 16 * 8 * SM_MAXT and total <= LDS_BYTES
    if not supported:
        return dict(supported=0)
    if waves == 8:
        assert total == 132 * epad + 15744
    longer = max(n_ovf, n_ovf_t)
    ovf_bytes = (longer * 12 + 15) // 16 * 16
    ovf_lds = longer > 0 and waves == 8 and total + ovf_bytes <= LDS_BYTES
    if ovf_lds:
        total += ovf_bytes
    y_lds = total + 8 * epad <= LDS_BYTES
    if y_lds:
        total += 8 * epad
    tpw = (tiles + waves - 1) // waves
    blocks = (tiles + 7) // 8
    can_pair = waves == 8 and blocks >= 2
    paired = bool(paired and can_pair)
    if paired:
        instance = min(max((blocks + 1) // 2, 2), 5)
    elif waves == 12:
        instance = 1 if tpw <= 1 else 2
    else:
        instance = 6 if tpw <= 6 else 8 if tpw <= 8 else SM_MAXT
    ovf_instance = waves == 8 and (paired or instance <= 8)
    return dict(supported=1, waves=waves, tiles_per_wave=tpw, instance=instance, paired=int(paired), n_ovf=n_ovf, n_ovf_t=n_ovf_t,
                ovf_lds=int(ovf_lds), y_lds=int(y_lds), ovf_in_kernel=int(ovf_instance and ovf_lds), same_t=int(same_t), lds_bytes=total,
                can_pair=can_pair, blocks=blocks, tiles=tiles)


LAYOUT_FIELDS = ("supported", "waves", "tiles_per_wave", "instance", "paired", "n_ovf", "n_ovf_t", "ovf_lds", "y_lds", "ovf_in_kernel",
                 "same_t", "lds_bytes")

# ------------------------------------------------------------------------------------------------------------------
# graphs
# ------------------------------------------------------------------------------------------------------------------


def build_graph(kind, n_edges):
    """(Complex, roles): roles names the last nodes a case uses -- hub / nbr / leaf (plain: a node with a chord / one without / its
    neighbour) and the node without edges."""
    from scone_gcn_amd.synthetic_data_gen import Complex
    E = n_edges
    if kind == "plain":
        assert E >= 5
        n_ch = E // 3
        V = E - n_ch
        edges = [(i, (i + 1) % V) for i in range(V)] + [(i, i + V // 2) for i in range(n_ch)]
        roles = dict(hub=0, nbr=V - 1, leaf=V // 2 - 1 if n_ch < V // 2 else 1, isolated=V)
        n_nodes = V + 1
    else:
        K, Lf = (64, 7) if kind == "hub" else (24, 8)
        base = K * (1 + Lf)
        assert kind in ("hub", "hub24") and E >= base
        leaves = K + 1 + np.arange(K * Lf).reshape(K, Lf)
        edges = [(0, j) for j in range(1, K + 1)] + [(j + 1, int(l)) for j in range(K) for l in leaves[j]]
        path = [int(v) for v in leaves.T.ravel()]                 # consecutive leaves hang on different neighbours
        nxt = K + 1 + K * Lf
        rest = E - base
        while rest > len(path) - 1:
            path.append(nxt)
            nxt += 1
        edges += [(path[i], path[i + 1]) for i in range(rest)]
        roles = dict(hub=0, nbr=K // 2, leaf=int(leaves[K // 2 - 1, 0]), isolated=nxt)
        n_nodes = nxt + 1
    e = np.array(sorted({(min(a, b), max(a, b)) for a, b in edges}), np.int64)
    assert len(e) == E and (e[:, 0] < e[:, 1]).all()
    return Complex(n_nodes=n_nodes, edges=e, faces=np.zeros((0, 3), np.int64)), roles


def readout_bounds(nbrhoods, edges, n_nodes):
    """(max_deg, max_items) by ops.SconePlan._upload_readout's formula: the items of a last node are the incident edges of its
    neighbours."""
    nbr = np.asarray(nbrhoods)
    inc_deg = np.bincount(np.asarray(edges).ravel(), minlength=n_nodes).astype(np.int64)
    return nbr.shape[1], int(np.where(nbr >= 0, inc_deg[np.maximum(nbr, 0)], 0).sum(axis=1).max())


# ------------------------------------------------------------------------------------------------------------------
# operators
# ------------------------------------------------------------------------------------------------------------------


def special_rows(E):
    rows = {0, 15, 16, E - 1}
    for b in range(0, E, 128):
        rows |= {b, min(b + 127, E - 1)}
    if E % 16:
        rows |= set(range(E - E % 16, E))
    return sorted(r for r in rows if 0 <= r < E)


def row_targets(E, extra, rs, prefer=None):
    """{device row: entries}: every class that fits at the special rows (more rows are made special when there are fewer than
    classes), row 0 and the last row long enough to hold the column-0 / column-(E-1) entries of every class.  prefer: device rows the
    readout of the case's fixed trajectories reads -- they
    take the classes first, so that a row of every class is read directly (a two-layer model sees an entry of a row only through that
    row and the rows that gather from it)."""
    classes = [c for c in CLASSES if c <= E - 4]
    pos = special_rows(E)
    spare = [int(r) for r in np.unique(np.linspace(1, E - 2, 40).astype(int)) if r not in pos]
    while len(pos) < len(classes) + 1:
        pos.append(int(spare.pop(len(spare) // 2)))
    first, last = (13, 25 if 25 in classes else 12)
    t = {0: first, E - 1: last}
    order = [c for c in rs.permutation([c for c in classes if c not in (first, last)])] + [first, last]
    others = [r for r in sorted(pos) if r not in t]
    if prefer is not None:                                        # the rows the fixed trajectories' readout reads come first: one of every class
        others = [r for r in others if r in prefer] + [r for r in others if r not in prefer]
    for i, r in enumerate(others):
        t[r] = int(order[i % len(order)])
    free = [r for r in rs.permutation(E) if r not in t]
    for r in free[:extra]:
        t[int(r)] = 100
    assert {t[r] for r in t} >= set(classes)
    return t


def _pattern(E, targets, sym, rs):
    """Rows as lists of columns.  sym: an entry (r, c) comes with (c, r), and a row other than the targets' takes at most ORDINARY_MAX;
    else: a COLUMN takes at most ORDINARY_MAX entries (the transpose has no long row)."""
    rows = [[] for _ in range(E)]
    have = [set() for _ in range(E)]
    col_cnt = np.zeros(E, np.int64)
    cap = np.full(E, ORDINARY_MAX, np.int64)
    for r, t in targets.items():
        cap[r] = t

    def room(c):
        return (cap[c] - len(rows[c])) if sym else (ORDINARY_MAX - col_cnt[c])

    def link(r, c):
        assert c not in have[r] and len(rows[r]) < cap[r] and (r == c or room(c) > 0), (r, c)
        rows[r].append(c)
        have[r].add(c)
        col_cnt[c] += 1
        if sym and c != r:
            rows[c].append(r)
            have[c].add(r)
            col_cnt[r] += 1

    # a row of every class reaches column 0 and column E - 1 (a class of one entry: one row each where it has two rows)
    link(0, 0)
    by_class = {}
    for r in sorted(targets):
        if r not in (0, E - 1):
            by_class.setdefault(targets[r], []).append(r)
    for c, rr in sorted(by_class.items()):
        if c >= 2:
            link(rr[0], 0)
            link(rr[0], E - 1)
        elif c == 1:
            link(rr[0], 0)
            if len(rr) > 1:
                link(rr[1], E - 1)
    if E - 1 not in have[0]:
        link(0, E - 1)
    if not sym:
        link(E - 1, 0)
    link(E - 1, E - 1)
    # the targets' rows, longest need first, then the others: 2 .. 6 entries of their own
    for r in sorted(targets, key=lambda r: -(targets[r] - len(rows[r]))):
        need = targets[r] - len(rows[r])
        if need <= 0:
            continue
        cand = [int(c) for c in rs.permutation(E) if c != r and c not in have[r] and room(c) > 0]
        pick = ([c for c in cand if c not in targets] + [c for c in cand if c in targets])[:need]      # other special rows last
        assert len(pick) == need, "row %d of %d entries finds no partners" % (r, targets[r])
        for c in pick:
            link(r, c)
    for r in range(E):
        if r in targets:
            continue
        want = int(rs.randint(2, 7))
        tries = 0
        while len(rows[r]) < want and tries < 40:
            tries += 1
            c = int(rs.randint(E))
            if c not in have[r] and c not in targets and c != r and room(c) > 0:
                link(r, c)
    for r, t in targets.items():
        assert len(rows[r]) == t, (r, t, len(rows[r]))
    return rows


def _values(E, rows, targets, sym, rs):
    """(lower, upper) float32 CSR in device order on the rows' pattern: every entry in both arrays, the lower or the upper only."""
    n = np.array([len(c) for c in rows])
    R = np.repeat(np.arange(E), n)
    C = np.concatenate([np.asarray(c, np.int64) for c in rows]) if n.sum() else np.zeros(0, np.int64)
    key = np.minimum(R, C) * E + np.maximum(R, C) if sym else R * E + C
    uk, inv = np.unique(key, return_inverse=True)
    kind = rs.choice(3, size=len(uk), p=[0.5, 0.25, 0.25])          # 0 both, 1 lower only, 2 upper only
    # the first two entries of a special row that lead to ordinary rows: lower only, upper only
    pos = {int(k): i for i, k in enumerate(uk)}
    for r in sorted(targets):
        own = [c for c in rows[r] if c not in targets][:2]
        for j, c in enumerate(own):
            kind[pos[int(min(r, c) * E + max(r, c)) if sym else int(r * E + c)]] = 1 + j
    scale = 1.0 / np.sqrt(np.maximum(np.maximum(n[R], n[C]) if sym else n[R], 1))
    a = (rs.randn(len(uk))[inv] * scale).astype(np.float32)
    b = (rs.randn(len(uk))[inv] * scale).astype(np.float32)
    k = kind[inv]
    a[k == 2] = 0
    b[k == 1] = 0
    assert ((a != 0) | (b != 0)).all()
    out = []
    for v in (a, b):
        m = sp.csr_matrix((v[v != 0], (R[v != 0], C[v != 0])), shape=(E, E))
        m.sort_indices()
        out.append(m)
    return out


def build_operator(E, variant, extra, seed, prefer=None):
    """dict(lo, up: float32 CSR in device order, targets: {device row: entries} of A (tonly: of A^T), sym)."""
    rs = np.random.RandomState(seed)
    targets = row_targets(E, extra, rs, prefer)
    if variant == "tonly":
        rows = _pattern(E, targets, False, rs)
        lo, up = (m.T.tocsr() for m in _values(E, rows, targets, False, rs))
    else:
        rows = _pattern(E, targets, True, rs)
        lo, up = _values(E, rows, targets, True, rs)
        if variant == "nonsym":
            drop = rs.rand(E, E) < 1.0 / 3
            special = np.zeros(E, bool)
            special[list(targets)] = True
            mats = []
            for m in (lo.tocoo(), up.tocoo()):
                keep = ~((m.col < m.row) & drop[m.row, m.col] & ~special[m.row])
                mats.append(sp.csr_matrix((m.data[keep], (m.row[keep], m.col[keep])), shape=(E, E)))
            lo, up = mats
        else:
            assert variant == "sym"
    for m in (lo, up):
        m.sort_indices()
    return dict(lo=lo, up=up, targets=targets, sym=variant == "sym")


def row_lengths(lo, up):
    return np.diff((abs(lo) + abs(up)).tocsr().indptr)


def overflow_entries(lo, up):
    return int(np.maximum(row_lengths(lo, up) - SM_CH, 0).sum())


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------

#        name            |E|  graph    variant  extra layers act [another draw: the first one that tests/test_host_small_step_limits.py admits]
CASES = [
    ("e17_sym", 17, "plain", "sym", 0, 2, "tanh", 1),
    ("e192_sym", 192, "plain", "sym", 0, 5, "relu"),
    ("e192_nonsym", 192, "plain", "nonsym", 0, 2, "none", 1),
    ("e193_sym", 193, "plain", "sym", 0, 3, "leaky_relu"),
    ("e193_nonsym", 193, "plain", "nonsym", 0, 6, "tanh"),
    ("e384_hub24", 384, "hub24", "sym", 0, 6, "none"),
    ("e385_sym", 385, "plain", "sym", 0, 4, "tanh", 2),
    ("e385_nonsym", 385, "plain", "nonsym", 0, 5, "leaky_relu"),
    ("e520_sym", 520, "hub", "sym", 0, 6, "relu"),
    ("e520_nonsym", 520, "hub", "nonsym", 0, 6, "tanh"),
    ("e520_tonly", 520, "hub", "tonly", 0, 6, "leaky_relu"),
    ("e768_sym", 768, "hub", "sym", 0, 3, "relu"),
    ("e769_sym", 769, "hub", "sym", 0, 5, "none"),
    ("e1001_nonsym_fits", 1001, "hub", "nonsym", 0, 3, "tanh", 2),
    ("e1001_nonsym_long", 1001, "hub", "nonsym", 12, 5, "relu"),
    ("e1024_sym", 1024, "hub", "sym", 0, 2, "leaky_relu", 3),
    ("e1024_nonsym", 1024, "hub", "nonsym", 0, 2, "relu"),
    ("e1025_sym", 1025, "hub", "sym", 0, 3, "tanh"),
    ("e1025_nonsym", 1025, "hub", "nonsym", 0, 5, "none"),
    ("e1040_sym", 1040, "hub", "sym", 0, 4, "relu"),
    ("e1040_nonsym", 1040, "hub", "nonsym", 0, 6, "none", 2),
    ("e1056_sym", 1056, "hub", "sym", 6, 3, "leaky_relu"),
    ("e1056_nonsym", 1056, "hub", "nonsym", 9, 4, "tanh"),
    ("e1057_sym", 1057, "hub", "sym", 0, 5, "tanh"),
    ("e1057_nonsym", 1057, "hub", "nonsym", 0, 3, "relu", 1),
    ("e1120_nonsym", 1120, "hub", "nonsym", 0, 4, "leaky_relu"),
    ("e1121_sym", 1121, "hub", "sym", 0, 3, "tanh"),
]
CASE_NAMES = [c[0] for c in CASES]

# what the case table of the issue says each case meets: the fields of restate_form that are asserted (unpaired form; "paired_instance"
# is the instance of the paired form where it applies)
REGIMES = {
    "e17_sym": dict(waves=12, tiles_per_wave=1, instance=1, ovf_in_kernel=0, y_lds=1, same_t=1),
    "e192_sym": dict(waves=12, tiles_per_wave=1, instance=1, ovf_in_kernel=0, same_t=1),
    "e192_nonsym": dict(waves=12, instance=1, ovf_in_kernel=0, same_t=0),
    "e193_sym": dict(waves=12, tiles_per_wave=2, instance=2, ovf_in_kernel=0, same_t=1),
    "e193_nonsym": dict(waves=12, instance=2, ovf_lds=0, ovf_in_kernel=0, same_t=0),
    "e384_hub24": dict(waves=12, tiles_per_wave=2, instance=2, same_t=1),
    "e385_sym": dict(waves=8, tiles_per_wave=4, instance=6, paired_instance=2, same_t=1),
    "e385_nonsym": dict(waves=8, instance=6, paired_instance=2, same_t=0),
    "e520_sym": dict(waves=8, instance=6, paired_instance=3, ovf_lds=1, ovf_in_kernel=1, y_lds=1, same_t=1),
    "e520_nonsym": dict(waves=8, instance=6, paired_instance=3, ovf_lds=1, ovf_in_kernel=1, y_lds=1, same_t=0),
    "e520_tonly": dict(waves=8, instance=6, paired_instance=3, n_ovf=0, ovf_lds=1, ovf_in_kernel=1, same_t=0),
    "e768_sym": dict(waves=8, tiles_per_wave=6, instance=6, paired_instance=3, same_t=1),
    "e769_sym": dict(waves=8, tiles_per_wave=7, instance=8, paired_instance=4, blocks=7, same_t=1),
    "e1001_nonsym_fits": dict(waves=8, instance=8, paired_instance=4, ovf_lds=1, ovf_in_kernel=1, same_t=0),
    "e1001_nonsym_long": dict(waves=8, instance=8, paired_instance=4, ovf_lds=0, ovf_in_kernel=0, y_lds=1, same_t=0),
    "e1024_sym": dict(waves=8, tiles_per_wave=8, instance=8, paired_instance=4, ovf_lds=1, ovf_in_kernel=1, same_t=1),
    "e1024_nonsym": dict(waves=8, instance=8, paired_instance=4, ovf_lds=1, ovf_in_kernel=1, same_t=0),
    "e1025_sym": dict(waves=8, tiles_per_wave=9, instance=9, paired_instance=5, ovf_lds=1, ovf_in_kernel=0, same_t=1),
    "e1025_nonsym": dict(waves=8, instance=9, paired_instance=5, ovf_lds=1, ovf_in_kernel=0, same_t=0),
    "e1040_sym": dict(waves=8, instance=9, paired_instance=5, ovf_lds=1, y_lds=0, same_t=1),
    "e1040_nonsym": dict(waves=8, instance=9, paired_instance=5, ovf_lds=1, y_lds=0, same_t=0),
    "e1056_sym": dict(waves=8, instance=9, paired_instance=5, ovf_lds=0, y_lds=1, same_t=1),
    "e1056_nonsym": dict(waves=8, instance=9, paired_instance=5, ovf_lds=0, y_lds=1, same_t=0),
    "e1057_sym": dict(waves=8, instance=9, paired_instance=5, y_lds=0, same_t=1),
    "e1057_nonsym": dict(waves=8, instance=9, paired_instance=5, y_lds=0, same_t=0),
    "e1120_nonsym": dict(waves=8, tiles_per_wave=9, instance=9, paired_instance=5, ovf_lds=0, y_lds=0, same_t=0),
    "e1121_sym": dict(supported=0),
}

_CACHE = {}


class Case:
    """One case, everything in the CALLER's order: cx / sc (the complex and its layout), S_lo / S_up (float64 CSR with float32
    values), dev_lo / dev_up (the same in device row order), targets, flows (N, E, 1), last_nodes, y (N, D, 1), weights (float64
    arrays holding float32 values), roles, and the positions of the special trajectories."""

    def __init__(self, name, E, graph, variant, extra, n_layers, act, bump=0):
        from scone_gcn_amd.complex import SimplicialComplex
        self.name, self.E, self.graph, self.variant, self.n_layers, self.act = name, E, graph, variant, n_layers, act
        seed = 1000 + CASE_NAMES.index(name) + 100 * bump          # bump: another draw, where the first one is not admitted (host test)
        rs = np.random.RandomState(seed)
        self.cx, self.roles = build_graph(graph, E)
        self.sc = SimplicialComplex(self.cx)
        self.max_deg, self.max_items = readout_bounds(self.sc.nbrhoods, self.cx.edges, self.cx.n_nodes)
        if graph == "hub":
            assert (self.max_deg, self.max_items) == (SM_MAXD, SM_ITEMS)
        elif graph == "hub24":
            assert (self.max_deg, self.max_items) == (24, 216)
        order = self.sc.layout.order[1]                           # order[device row] = the caller's row
        star = None
        if graph != "plain":                                      # the hub's readout reads the edges at its neighbours: the star
            K = self.max_deg
            is_star = ((self.cx.edges >= 1) & (self.cx.edges <= K)).any(axis=1)
            star = set(np.nonzero(is_star[order])[0].tolist())
        op = build_operator(E, variant, extra, seed, star)
        self.targets, self.dev_lo, self.dev_up = op["targets"], op["lo"], op["up"]
        # reps: the row of every class whose entries the host test zeroes -- the first one, rows the hub's readout reads first
        self.reps = {}
        for r in sorted(self.targets, key=lambda r: (star is not None and r not in star, r)):
            if r not in (0, E - 1):
                self.reps.setdefault(self.targets[r], r)
        P = sp.csr_matrix((np.ones(E), (order, np.arange(E))), shape=(E, E))
        self.S_lo = (P @ self.dev_lo.astype(np.float64) @ P.T).tocsr()
        self.S_up = (P @ self.dev_up.astype(np.float64) @ P.T).tocsr()
        self.n_ovf = overflow_entries(self.dev_lo, self.dev_up)
        self.n_ovf_t = overflow_entries(self.dev_lo.T.tocsr(), self.dev_up.T.tocsr())
        N = self.n_traj = (9, 10, 11, 13)[seed % 4]                # never whole slabs of four
        V = self.cx.n_nodes
        deg = np.bincount(self.cx.edges.ravel(), minlength=V)
        last = rs.choice(np.nonzero(deg > 0)[0], size=N)
        self.T_HUB, self.T_NBR, self.T_LEAF, self.T_ISOLATED, self.T_ZERO_Y, self.T_ZERO_FLOW = 0, 1, 2, 3, 4, 5
        if graph == "plain":                                      # a ring: the trajectories end next to the edges of the classes' rows
            ring = self.cx.n_nodes - 1
            cover = [(int(self.cx.edges[order[self.reps[k]], 0]) + 1) % ring for k in sorted(self.reps) if k >= 1]
            self.roles.update(dict(zip(("hub", "nbr", "leaf"), cover)))
            for k, v in zip(range(6, N), cover[3:]):
                last[k] = v
        for k, role in enumerate(("hub", "nbr", "leaf", "isolated")):
            last[k] = self.roles[role]
        self.last_nodes = last.astype(np.int64)
        self.flows = rs.randn(N, E, 1).astype(np.float32).astype(np.float64)
        self.flows[self.T_ZERO_FLOW] = 0.0
        nn = np.maximum(deg[last], 1)
        choice = (rs.randint(0, 1 << 20, size=N) % nn).astype(np.int64)
        self.y = np.zeros((N, self.max_deg, 1))
        self.y[np.arange(N), choice, 0] = 1.0
        self.y[self.T_ZERO_Y] = 0.0
        shapes = [(1, 16)] * 3 + [(16, 16)] * (3 * (n_layers - 1)) + [(16, 1)]
        self.weights = [(0.3 * rs.randn(*s)).astype(np.float32).astype(np.float64) for s in shapes]
        self.same_t = variant == "sym"

    def form(self, paired=False):
        return restate_form(self.E, self.n_ovf, self.n_ovf_t, paired, self.same_t)

    def oracle(self, S_lo=None, S_up=None, sel=None):
        """(loss, grads) of so.scone_loss_and_grad in fp64 on the case's trajectories (sel: on those alone, still over N)."""
        from oracle import scone_oracle as so
        B1 = _b1_dense(self.cx)
        Bc = so.make_Bconds(B1, np.asarray(self.sc.nbrhoods), None)
        mask = np.ones(self.n_traj, int)
        y = self.y
        if sel is not None:
            y = np.zeros_like(self.y)
            y[sel] = self.y[sel]
        return so.scone_loss_and_grad(self.weights, self.S_lo if S_lo is None else S_lo, self.S_up if S_up is None else S_up, Bc,
                                      self.last_nodes, self.flows, y, mask, 0.0, self.act)


def _b1_dense(cx):
    E = cx.n_edges
    B1 = np.zeros((cx.n_nodes, E))
    B1[cx.edges[:, 0], np.arange(E)] = -1.0
    B1[cx.edges[:, 1], np.arange(E)] = 1.0
    return B1


def get_case(name):
    if name not in _CACHE:
        _CACHE[name] = Case(*CASES[CASE_NAMES.index(name)])
    return _CACHE[name]


def reference(name):
    """The fp64 oracle's (loss, grads) of a case, computed once and shared."""
    key = ("ref", name)
    if key not in _CACHE:
        _CACHE[key] = get_case(name).oracle()
    return _CACHE[key]
