"""The brute-force reference and the point / query families shared by the CPU and GPU tests of the
1 m cell grids: the build (llsr_grid.hip) and the searches over it (knn5, nn1_shells, nn1_scan,
nn1_block_multi, llsr_search.h).

The reference is numpy float32 over ALL points: d = ((0 + tx^2) + ty^2) + tz^2 with t = q - p, one
rounded operation at a time (nanoflann's L2_Simple order), the winner the lexicographic minimum of
(d, index); a NaN distance never wins. It knows nothing of cells. Everything is generated from fixed
seeds and nothing here calls the library. Map order is shuffled in every family, so index order is
unrelated to cell order. No coordinate exceeds +-524 288.
"""
import functools

import numpy as np

F = np.float32
INF = F(np.inf)
INT_MAX = np.int32(2**31 - 1)
ONE_BELOW = np.nextafter(F(1), F(0))  # the largest float below 1.0
TRANSLATIONS = (0.0, 1000.0, 65536.0, -262144.0)


# ---- the reference --------------------------------------------------------------------------------
def dist2(q, pts):
    """[Q, N] float32 squared distances of q[Q, >= 3] to pts[N, >= 3], NaN replaced by +inf."""
    q, pts = np.asarray(q, F), np.asarray(pts, F)
    d = np.zeros((len(q), len(pts)), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            t = q[:, None, a] - pts[None, :, a]
            d = d + t * t
    d[np.isnan(d)] = INF
    return d


def brute_nn1(q, pts):
    """(D[Q], I[Q]): the (d, index) minimum over all points; (inf, INT_MAX) when no distance is finite."""
    if len(pts) == 0:
        return np.full(len(q), INF, F), np.full(len(q), INT_MAX, np.int32)
    d = dist2(q, pts)
    i = d.argmin(axis=1).astype(np.int32)  # the first of equal minima: the lowest index
    D = d[np.arange(len(q)), i]
    i[D == INF] = INT_MAX
    return D, i


def brute_knn5(q, pts, k=6):
    """The k smallest (d, index) pairs per query over all points with no cut-off: d[Q, k], idx[Q, k]
    (inf / INT_MAX past the cloud's size)."""
    d = dist2(q, pts)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]  # stable: equal distances stay in index order
    dk = np.take_along_axis(d, order, axis=1)
    ik = order.astype(np.int32)
    if dk.shape[1] < k:
        pad = k - dk.shape[1]
        dk = np.concatenate([dk, np.full((len(q), pad), INF, F)], 1)
        ik = np.concatenate([ik, np.full((len(q), pad), INT_MAX, np.int32)], 1)
    ik[dk == INF] = INT_MAX
    return dk, ik


def knn5_expected(q, pts):
    """What kNN-5 with d^2 < 1.0 must return: idx[Q, 5], d2[Q, 5] holding the (up to) five smallest
    (d, index) pairs with d < 1.0 (INT_MAX / inf in the places not filled), found[Q] = five exist,
    and sixth[Q] = the sixth smallest distance without the cut-off."""
    dk, ik = brute_knn5(q, pts, 6)
    d5, i5 = dk[:, :5].copy(), ik[:, :5].copy()
    out = ~(d5 < F(1))
    d5[out] = INF
    i5[out] = INT_MAX
    return i5, d5, d5[:, 4] < F(1), dk[:, 5]


# ---- helpers ----------------------------------------------------------------------------------------
def _xyzw(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    out = np.zeros((len(xyz), 4), F)
    out[:, :3] = xyz
    return out


def _shuffled(rng, xyz):
    return _xyzw(np.asarray(xyz, F)[rng.permutation(len(xyz))])


def _axis_grid(vals):
    g = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1).reshape(-1, 3)
    return g.astype(F)


def cell_of(xyz):
    """floor() cell of finite float32 coordinates."""
    return np.floor(np.asarray(xyz, F)[:, :3]).astype(np.int64)


# ---- kNN-5 / kNN-1 families: each returns (map[N, 4], {group: queries[Q, 4]}) -----------------------
@functools.lru_cache(maxsize=None)
def lattice(translate=0.0):
    """The half-integer lattice on [-3, 3]^3 (2197 points: cell faces, negative cells and, untranslated,
    -0.0f), moved by `translate` on all axes. Queries: lattice points, lattice points + 0.25 (inside
    the lattice), lattice points one ulp up and one ulp down."""
    rng = np.random.default_rng(11)
    base = _axis_grid(np.arange(-3.0, 3.01, 0.5))
    if translate == 0.0:
        zero = base == 0.0
        base[zero & (rng.random(base.shape) < 0.5)] = F(-0.0)
    else:  # (-0.0 + 0.0 would be +0.0)
        base = (base + F(translate)).astype(F)
    assert np.abs(base).max() <= 524288
    pick = lambda n, ok=None: base[rng.choice(np.flatnonzero(ok) if ok is not None else len(base), n, replace=False)]
    inside = (base < F(translate) + F(3)).all(axis=1)
    groups = {
        "on": pick(700),
        "quarter": (pick(700, inside) + F(0.25)).astype(F),
        "ulp_up": np.nextafter(pick(700), INF),
        "ulp_down": np.nextafter(pick(700), -INF),
    }
    return _shuffled(rng, base), {k: _xyzw(v) for k, v in groups.items()}


def _centre_line(rng, cells, n):
    """n random queries per cell and axis within 6e-6 of the point of the cell's centre line whose
    far four corners are at d^2 = 1: (cx + 0.5, cy + 0.5, cz + 1 - sqrt(0.5)) and its two axis
    permutations."""
    out = []
    for c in cells:
        for ax in range(3):
            q = np.asarray(c, np.float64) + 0.5 + rng.uniform(-2e-6, 2e-6, (n, 3))
            q[:, ax] = c[ax] + 1.0 - np.sqrt(0.5) + rng.uniform(-6e-6, 6e-6, n)
            out.append(q)
    return np.concatenate(out).astype(F)


@functools.lru_cache(maxsize=None)
def unit():
    """The integer lattice on [-3, 3]^3. Groups: `on` the points (self at 0, six neighbours at
    exactly 1.0: excluded, nothing found); `centre` the centres of the cells of [-4, 4]^3 (eight
    corners at 0.75 inside the lattice, fewer on its rim); `four_in` exactly four points inside
    and the fifth at a d^2 that rounds to exactly 1.0; `fifth_below` five or more inside, the fifth
    at nextafter(1, 0)."""
    rng = np.random.default_rng(12)
    pts = _axis_grid(np.arange(-3.0, 3.01, 1.0))
    # next to a lattice point: q - p rounds to exactly 1 on one side of each axis and stays below 1
    # on the other, so q's own point and one neighbour per axis are inside, the opposite three at 1.0
    e = F(2.0**-24)
    one_axis = np.array([e, -e, F(1) - e, F(-1) + e], F)
    four_in = _axis_grid(one_axis)
    # next to a cell's centre line: four corners near 0.5 + v^2, four near 0.5 + (1 - v)^2 with v
    # around 1 - sqrt(0.5); of many random such queries, those whose FIFTH float distance lands on the
    # wanted value exactly are kept
    cells = [(0, 0, 0), (-1, -1, -1), (1, -2, 0), (-3, 2, 1), (2, 2, 2), (-2, 0, -3)]
    cand = _centre_line(rng, cells, 1500)
    dk, _ = brute_knn5(cand, pts, 6)
    at_one = cand[(dk[:, 3] < F(1)) & (dk[:, 4] == F(1))][:60]
    below = cand[dk[:, 4] == ONE_BELOW][:60]
    groups = {
        "on": pts.copy(),
        "centre": _axis_grid(np.arange(-3.5, 3.51, 1.0)),
        "four_in": np.concatenate([four_in, at_one]),
        "fifth_below": below,
    }
    return _shuffled(rng, pts), {k: _xyzw(v) for k, v in groups.items()}


THRESHOLD_KINDS = ("corner", "edge", "face", "interior")


@functools.lru_cache(maxsize=None)
def threshold():
    """1000 queries around distinct cell corners 3 m apart, a quarter each within 1e-3 of the corner, of
    an edge, of a face, and interior; eight map points per query at d^2 in [0.97, 1.02] in random
    directions (other queries' points are farther than 1.08 m)."""
    rng = np.random.default_rng(13)
    corners = 3.0 * (_axis_grid(np.arange(10.0)).astype(np.float64) - 5.0)
    kind = rng.permutation(1000) % 4  # number of coordinates NOT pinned to the corner: 0 .. 3
    near = rng.uniform(-1e-3, 1e-3, (1000, 3))
    free = rng.uniform(0.1, 0.9, (1000, 3))
    axes = np.argsort(rng.random((1000, 3)), axis=1)  # which coordinates are free
    off = near.copy()
    for k in range(3):
        take = kind > k
        off[take, axes[take, k]] = free[take, axes[take, k]]
    q = (corners + off).astype(F)
    dirs = rng.normal(size=(1000, 8, 3))
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    r = np.sqrt(rng.uniform(0.97, 1.02, (1000, 8, 1)))
    pts = (q[:, None, :].astype(np.float64) + r * dirs).reshape(-1, 3)
    groups = {name: _xyzw(q[kind == k]) for k, name in enumerate(THRESHOLD_KINDS)}
    return _shuffled(rng, pts), groups


def _poison(rng, xyzw, share=0.01):
    out = xyzw.copy()
    rows = rng.choice(len(out), max(3, int(round(share * len(out)))), replace=False)
    out[rows, rng.integers(0, 3, len(rows))] = np.resize(np.array([np.nan, np.inf, -np.inf], F), len(rows))
    return out, rows


@functools.lru_cache(maxsize=None)
def nonfinite():
    """The lattice map with 1 % of the points given a NaN, +inf or -inf coordinate (cell_coord's
    sentinel cell), and the same share of the queries."""
    rng = np.random.default_rng(14)
    m, groups = lattice(0.0)
    m, _ = _poison(rng, m)
    q = np.concatenate(list(groups.values()))
    q, rows = _poison(rng, q)
    finite = np.ones(len(q), bool)
    finite[rows] = False
    return m, {"finite": q[finite], "poisoned": q[~finite]}


@functools.lru_cache(maxsize=None)
def sparse():
    """kNN-1 only: a 1 m thick slab of 2000 points and 600 queries 2.5 m to 6 m above and below it."""
    rng = np.random.default_rng(15)
    pts = np.stack([rng.uniform(-8, 8, 2000), rng.uniform(-8, 8, 2000), rng.uniform(-0.5, 0.5, 2000)], 1)
    h = rng.uniform(3.0, 6.0, 600) * np.where(rng.random(600) < 0.5, -1.0, 1.0)
    q = np.stack([rng.uniform(-7, 7, 600), rng.uniform(-7, 7, 600), h], 1)
    return _shuffled(rng, pts), {"off_slab": _xyzw(q)}


SAME_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
SAME_A, SAME_B = (0.5, 0.25, 0.75), (1.5, 0.25, 0.75)


@functools.lru_cache(maxsize=None)
def same(n, alternating):
    """kNN-1 only: n identical points (every answer is index 0), or two points alternating A, B, A, ...
    one cell apart (index 0 or 1; the query midway between them ties and goes to 0). Queries: on
    the points, next to them, midway, and 5 m and 50 m away (the scans)."""
    pts = np.tile(np.asarray(SAME_A, F), (n, 1))
    if alternating:
        pts[1::2] = np.asarray(SAME_B, F)
    q = np.array([SAME_A, SAME_B, (0.4, 0.3, 0.7), (1.75, 0.25, 0.5), (1.0, 0.25, 0.75), (1.0, 0.9, 0.1),
                  (-0.01, 0.25, 0.75), (2.01, 0.25, 0.75), (5.5, 0.25, 0.75), (0.5, -4.75, 0.75), (50.0, 50.0, 50.0)], F)
    return _xyzw(pts), {"all": _xyzw(q)}


def knn_families():
    """name -> (map, groups) of every family kNN-5 runs on with finite input."""
    out = {("lattice%+d" % t if t else "lattice"): lattice(t) for t in TRANSLATIONS}
    out["unit"] = unit()
    out["threshold"] = threshold()
    return out


def all_queries(groups):
    return np.concatenate(list(groups.values()))


# ---- grid build cases ---------------------------------------------------------------------------------
BUILD_SIZES = (1, 5, 63, 64, 65, 1023, 1024, 1025, 4097)


def _cloud(rng, n, side=None):
    """n random points, a few per cell, around the origin (negative cells included)."""
    side = side or max(1.0, (n / 4.0) ** (1.0 / 3.0))
    return _xyzw(rng.uniform(-side / 2, side / 2, (n, 3)))


def _own_cells(rng, n):
    """n points in n distinct cells."""
    side = int(np.ceil(n ** (1.0 / 3.0))) + 1
    cells = _axis_grid(np.arange(side) - side // 2)[rng.permutation(side**3)[:n]]
    return _xyzw(cells + rng.uniform(0.05, 0.95, (n, 3)).astype(F))


def _by_cell_sequence(rng, seq):
    """One point in cell (seq[k], -1, 2) for every k, in that order."""
    seq = np.asarray(seq, np.float64)
    xyz = np.stack([seq, np.full(len(seq), -1.0), np.full(len(seq), 2.0)], 1) + rng.uniform(0.05, 0.95, (len(seq), 3))
    return _xyzw(xyz)


def _one(cloud, cap=None):
    return dict(pts=cloud, off=np.array([0, len(cloud)], np.int64), cap=cap if cap is not None else max(1, len(cloud)))


def build_cases():
    """name -> (grid a, grid b, P): the two grids of one grid_build call, each a dict of pts[n, 4],
    off[P + 1] and cap."""
    rng = np.random.default_rng(16)
    cases = {}
    for n in BUILD_SIZES:  # cap = n next to cap = n + 100, the same cloud
        c = _cloud(rng, n)
        cases[f"n{n}"] = (_one(c), _one(c, n + 100), 1)
    cases["one_cell"] = (_one(_xyzw(rng.uniform(0.0, 1.0, (1500, 3)) + np.array([-3.0, 7.0, 0.0]))),
                         _one(_xyzw(rng.uniform(0.0, 1.0, (64, 3)))), 1)
    cases["own_cells"] = (_one(_own_cells(rng, 15)), _one(_own_cells(rng, 1023)), 1)  # tables one short of full
    cases["alternating_runs"] = (_one(_by_cell_sequence(rng, np.arange(2500) % 2)),
                                 _one(_by_cell_sequence(rng, rng.permutation(26)[np.arange(2600) // 100])), 1)
    sizes_a, sizes_b = (700, 0, 1300), (0, 65, 3)
    ragged = lambda sizes: dict(pts=_cloud(rng, sum(sizes), 6.0), off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                                cap=max(sizes))
    cases["ragged_P3"] = (ragged(sizes_a), ragged(sizes_b), 3)
    cases["caps_apart"] = (_one(_cloud(rng, 4097)), _one(_cloud(rng, 5)), 1)  # b's surplus blocks return early
    cases["nonfinite"] = (_one(_poison(rng, _cloud(rng, 2000))[0]), _one(_poison(rng, _cloud(rng, 300), 0.05)[0]), 1)
    return cases
