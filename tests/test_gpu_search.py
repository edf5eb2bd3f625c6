"""The device searches over the 1 m cell grids (llsr_search.h: knn5 of the scan-to-map LM; nn1_shells,
nn1_scan and nn1_block_multi of the scan-to-scan LM) against a brute force over all points
(tests/_search_cases.py), bit for bit, on geometry built to sit on the searches' pruning bounds:
neighbours across cell faces, edges and corners within rounding of the bound, ties at the fifth
place, d^2 at exactly 1.0 and one float below, large coordinates, non-finite input, sparse regions
the shells cannot settle, and clouds of equal points. tests/test_search_cases_host.py shows on the
CPU that each family reaches its edge. The diagnostics (llsr_search_debug.hip) build the grid with
the production grid_build and call the header's text; nothing is restated on the device side.

The last test drives the scan-to-scan kernel itself into the overflow of its fallback queue
(more than kFbMax = 256 queries of one pass left open by the shells -> the per-thread serial scan).
"""
import ctypes as C

import numpy as np
import pytest

import _search_cases as sc
import oracle_py
from llsr import Pipeline, lib

pytestmark = pytest.mark.gpu

F = np.float32
DIST_SQR = (25.0, 1.0, 0.0)  # nearest_feature_dist_sqr of the shipped configs, the cell size, the trivial rule


def gpu_knn5(m, q):
    f = lib().llsr_debug_knn5
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    m, q = np.ascontiguousarray(m, F), np.ascontiguousarray(q, F)
    idx, d2, found = np.zeros((len(q), 5), np.int32), np.zeros((len(q), 5), F), np.zeros(len(q), np.uint8)
    rc = f(m.ctypes.data, len(m), q.ctypes.data, len(q), idx.ctypes.data, d2.ctypes.data, found.ctypes.data)
    assert rc == 0, f"llsr_debug_knn5: {rc}"
    return idx, d2, found.astype(bool)


def gpu_nn1(m, q, dist_sqr, seed):
    f = lib().llsr_debug_nn1
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float] + [C.c_void_p] * 10
    m, q = np.ascontiguousarray(m, F), np.ascontiguousarray(q, F)
    seed = np.ascontiguousarray(seed, np.int32)
    n = len(q)
    settled = np.zeros(n, np.uint8)
    out = {k: (np.zeros(n, np.int32), np.zeros(n, F)) for k in ("shells", "scan", "multi256", "multi512")}
    ptrs = [a.ctypes.data for pair in out.values() for a in pair]
    rc = f(m.ctypes.data, len(m), q.ctypes.data, n, dist_sqr, seed.ctypes.data, settled.ctypes.data, *ptrs)
    assert rc == 0, f"llsr_debug_nn1: {rc}"
    return settled.astype(bool), out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check_knn5(name, m, q):
    idx, d2, found, _ = sc.knn5_expected(q, m)
    gi, gd, gf = gpu_knn5(m, q)
    errs = []
    for what, bad in (("found", gf != found), ("d2", (bits(gd) != bits(d2)).any(axis=1)), ("idx", (gi != idx).any(axis=1))):
        k = np.flatnonzero(bad)
        if len(k):
            j = k[0]
            errs.append(f"{name}: {what} differs for {len(k)} of {len(q)} queries, first {j} q={q[j, :3]!r}: "
                        f"device {gi[j]} {gd[j]!r} {gf[j]}, brute force {idx[j]} {d2[j]!r} {found[j]}")
    return errs


@pytest.mark.parametrize("name", list(sc.knn_families()))
def test_knn5_equals_brute_force(require_gpu, name):
    m, groups = sc.knn_families()[name]
    errs = check_knn5(name, m, sc.all_queries(groups))
    assert not errs, "\n".join(errs)


def test_knn5_nonfinite_equals_brute_force(require_gpu):
    m, groups = sc.nonfinite()
    errs = check_knn5("nonfinite", m, sc.all_queries(groups))
    assert not errs, "\n".join(errs)


def test_knn5_empty_map(require_gpu):
    q = sc.all_queries(sc.unit()[1])[:70]
    gi, gd, gf = gpu_knn5(np.zeros((0, 4), F), q)
    assert not gf.any() and (gi == sc.INT_MAX).all() and np.isposinf(gd).all()


def seeds_for(rng, kind, I, n):
    if kind == "none" or n == 0:
        return np.full(len(I), -1, np.int32)
    if kind == "random":
        return rng.integers(0, n, len(I)).astype(np.int32)
    return np.where(I == sc.INT_MAX, -1, I).astype(np.int32)  # the true nearest point


def check_nn1(name, m, q, seed_kinds=("none", "random", "nearest"), dist_sqrs=DIST_SQR):
    """Every rule of the kNN-1 on one cloud and query set; returns (findings, per-dist_sqr counts of
    unsettled queries and of queries settled with bd >= dist_sqr)."""
    D, I = sc.brute_nn1(q, m)
    rng = np.random.default_rng(17)
    errs, stats = [], {}
    for dist_sqr in dist_sqrs:
        for kind in seed_kinds:
            tag = f"{name} dist_sqr={dist_sqr} seed={kind}"
            settled, out = gpu_nn1(m, q, dist_sqr, seeds_for(rng, kind, I, len(m)))
            for k in ("scan", "multi256", "multi512"):  # exact for every query
                bi, bd = out[k]
                bad = np.flatnonzero((bits(bd) != bits(D)) | (bi != I))
                if len(bad):
                    j = bad[0]
                    errs.append(f"{tag}: nn1 {k} differs for {len(bad)} of {len(q)}, first {j} q={q[j, :3]!r}: "
                                f"({bd[j]!r}, {bi[j]}) vs ({D[j]!r}, {I[j]})")
            bi, bd = out["shells"]
            ds = F(dist_sqr)
            if dist_sqr > 0:
                near = settled & (D < ds)
                bad = np.flatnonzero(near & ((bits(bd) != bits(D)) | (bi != I)))
                if len(bad):
                    j = bad[0]
                    errs.append(f"{tag}: settled shells differ for {len(bad)}, first {j} q={q[j, :3]!r}: "
                                f"({bd[j]!r}, {bi[j]}) vs ({D[j]!r}, {I[j]})")
                bad = np.flatnonzero(settled & ~(D < ds) & ~(bd >= ds))
                if len(bad):
                    errs.append(f"{tag}: settled with bd < dist_sqr though nothing is that near, first {bad[0]}: {bd[bad[0]]!r}")
            else:
                if not settled.all():
                    errs.append(f"{tag}: {int((~settled).sum())} queries unsettled at dist_sqr 0")
                if (bd < ds).any():
                    errs.append(f"{tag}: a returned bd is below dist_sqr")
            if kind == "none":
                stats[dist_sqr] = (int((~settled).sum()), int((settled & (bd >= ds)).sum()))
    return errs, stats


@pytest.mark.parametrize("name", list(sc.knn_families()))
def test_nn1_equals_brute_force(require_gpu, name):
    m, groups = sc.knn_families()[name]
    q = sc.all_queries(groups)
    if name == "unit":  # the lattice's rim too: queries up to 2 cells outside it
        q = np.concatenate([q, (q[:200] * F(1.6)).astype(F)])
    errs, _ = check_nn1(name, m, q, dist_sqrs=(25.0, 1.0) if name.startswith("lattice") and name != "lattice" else DIST_SQR)
    assert not errs, "\n".join(errs)


def test_nn1_sparse(require_gpu):
    """Where the shells cannot settle: at dist_sqr = 25 two shells (r^2 <= 9) leave the queries with
    d^2 >= 9 open; at dist_sqr = 1 the exit r2 >= dist_sqr settles every one of them with nothing
    found (bd >= dist_sqr)."""
    m, groups = sc.sparse()
    errs, stats = check_nn1("sparse", m, sc.all_queries(groups))
    assert not errs, "\n".join(errs)
    assert stats[25.0][0] >= 1, "no sparse query came back unsettled"
    assert stats[1.0][1] >= 1, "no sparse query was settled through r2 >= dist_sqr with bd >= dist_sqr"


def test_nn1_nonfinite(require_gpu):
    """Seeds are real candidates (a previous pass's answer): none or the true nearest point, never
    a point with a NaN distance."""
    m, groups = sc.nonfinite()
    errs, _ = check_nn1("nonfinite", m, sc.all_queries(groups), seed_kinds=("none", "nearest"))
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("alternating", [False, True])
def test_nn1_same_points(require_gpu, alternating):
    errs = []
    for n in sc.SAME_SIZES:
        m, groups = sc.same(n, alternating)
        e, _ = check_nn1(f"same n={n} alternating={alternating}", m, groups["all"], dist_sqrs=(25.0,))
        errs += e
    assert not errs, "\n".join(errs)


def test_nn1_empty_cloud(require_gpu):
    q = sc.all_queries(sc.sparse()[1])[:130]
    settled, out = gpu_nn1(np.zeros((0, 4), F), q, 25.0, np.full(len(q), -1, np.int32))
    for k in ("scan", "multi256", "multi512"):
        assert (out[k][0] == sc.INT_MAX).all() and np.isposinf(out[k][1]).all(), k
    assert np.isposinf(out["shells"][1][settled]).all()


# ---- the fallback queue's overflow, end to end ---------------------------------------------------------
OVERFLOW_GUESS = np.array([0, 0, 0, 0.0, 4.0, 0.0], np.float32)  # pure translation, 4 m along the vertical axis


def test_scan2scan_fallback_queue_overflow(require_gpu):
    """One HDL-64E pair with a 4 m pure-translation initial guess: TransformToStart moves a point by
    s * t with s = 10 frac(intensity), so the flat queries of the sweep's later part start more than
    3 m from every point of the last surf cloud, the shells (two, r <= 3 m) leave them open and
    more than kFbMax = 256 of the first surf pass go to the serial scan beyond the queue. The
    result must still be the oracle's, bit for bit."""
    from test_gpu_fa_lm import _pairs, _same
    cfg, pairs = _pairs("hdl64e", [5, 6], 2048)
    sharp, flat, cl, sl = pairs[0]
    t = OVERFLOW_GUESS
    # on the CPU: the first surf pass's queries, p - s t in float32 (zero rotation), against the surf cloud
    w = flat[:, 3]
    s = F(10) * (w - np.trunc(w).astype(F))
    q = np.zeros_like(flat)
    for a in range(3):
        q[:, a] = flat[:, a] - s * t[3 + a]
    D, _ = sc.brute_nn1(q, sl)
    open_ = int((D >= F(9.0001)).sum())
    assert open_ >= 257, f"only {open_} of {len(flat)} flat queries start 3 m from the surf cloud"
    o = oracle_py.scan2scan(cfg, sharp, flat, cl, sl, t, 0)
    assert o["n_surf_corr"] >= 10, o
    pipe = Pipeline(cfg)
    g = pipe.scan2scan(sharp, flat, cl, sl, t, 0)
    pipe.close()
    errs = _same(g, o)
    assert not errs, "\n".join(errs)
