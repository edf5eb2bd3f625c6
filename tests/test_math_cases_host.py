"""CPU: the inputs of tests/_math_cases.py reach the branches they are built for, and the shared
numeric headers as hipcc's host compile has them (csrc/llsr_math_debug.hip, where = 0) equal their
independent references — a second compiler next to g++'s oracle/libm_check, tests/native/eigen_cross
and tests/native/pg_host_check:

* llsr_libm.h: glibc's bits (any two NaNs equal), and NaN from |x| = 120 on for tanf_ / sinf_ / cosf_;
* llsr_eigen.h: oracle_eigen.h's outputs and return codes bit for bit, every intermediate of the
  degeneracy chain included;
* llsr_pg.h's double trigonometry within 1 ulp of glibc on [-2 pi, 2 pi] (acosd on [-1, 1]). Both are
  within 1 ulp of the true value (fdlibm's stated bound; glibc's is tighter), so each returns one of
  the two doubles around it and they differ by at most one place: the bound pg_host_check asserts,
  here also at the multiples of pi/4 and the branch constants. Elsewhere only NaN-ness and finiteness
  are compared. Log(Exp(w)) returns w within pg_host_check's tolerance for its Log round trip:
  |back - w| <= 1e-9 (1 + |w|), or |back + w| <= 1e-7 (the other sign of the same rotation at pi).

The RANSAC margin is a property of the inputs alone: over every (K, cnt) of the domain with
k = log(0.01) / log(1 - (cnt / K)^3) <= 10002, glibc's k stays a relative 1e-11 or more away from
every integer, so a libm whose k differs from glibc's by less than that stops PCL's loop
(`iterations < k`) at the same iteration. Measured here: the closest approach is 1.508e-10 relative,
at K = 91693, cnt = 7492 (k = 8440.000001273); the assertion stands at a tenth of that, 1e-11.
tests/test_gpu_math_headers.py measures the device's deviation (2.2e-13 on the MI355X)."""
import numpy as np
import pytest

import _math_cases as mc


def _nonempty(name, masks):
    empty = [k for k, m in masks.items() if not m.any()]
    assert not empty, f"{name}: no input reaches {empty}"


# ---- the generators reach their edges ----------------------------------------------------------------
@pytest.mark.parametrize("fn", [k for k, n in enumerate(mc.LIBM_FNS) if n != "atan2f_"], ids=lambda k: mc.LIBM_FNS[k])
def test_libm_inputs_reach_every_branch(fn):
    x = mc.libm_unary(fn)
    assert 500_000 < len(x) <= mc.MAX_CASES
    _nonempty(mc.LIBM_FNS[fn], mc.libm_branches(fn, x))
    # both signs of every edge magnitude within 8 ulp, the edges themselves included
    e = mc.libm_edges().view(np.uint32)
    for m in mc.libm_edge_magnitudes():
        assert np.isin(np.uint32(m), e) and np.isin(np.uint32(m | 0x80000000), e)


def test_atan2_inputs_reach_every_branch():
    v = mc.atan2_list()
    assert len(v) == 1024 and np.isnan(v).any()
    for want in (0x0, 0x80000000, 0x1, 0x007fffff, 0x7f800000, 0xff800000):
        assert np.isin(np.uint32(want), v.view(np.uint32))
    mag = np.abs(v[np.isfinite(v) & (v != 0)])
    assert mag.min() < 1e-38 and mag.max() > 1e38 and len(np.unique(np.rint(np.log10(mag.astype(np.float64))))) >= 77
    y, x = mc.atan2_grid()
    assert len(y) == 1 << 20
    _nonempty("atan2f_ grid", mc.libm_branches(3, x, y))
    y, x = mc.atan2_gaps()
    q = np.abs(y.astype(np.float64) / x.astype(np.float64))
    for gap in (26, 60):
        for e in (-gap, gap):
            near = np.abs(q / 2.0 ** e - 1) < 2.0 ** -19
            assert near.sum() > 40_000
            k = (mc._ix(y)[near] - mc._ix(x)[near]) >> 23  # both sides of the exponent gap
            assert len(np.unique(k)) >= 2


@pytest.fixture(scope="module")
def eigen_ref():
    return {op: mc.ref_eigen(op, mc.eigen_cases(op)) for op in range(len(mc.EIGEN_OPS))}


def test_eigen_inputs_reach_every_class(eigen_ref):
    for op in (3, 4):  # eig3, eig6
        N = 3 if op == 3 else 6
        out, info = eigen_ref[op]
        ev = out[:, :N]
        ok = (info == 0) & np.isfinite(ev).all(1)
        with np.errstate(all="ignore"):
            _nonempty(mc.EIGEN_OPS[op], {
                "rank deficient": ok & (np.abs(ev[:, 0]) <= 1e-6 * np.abs(ev[:, -1])) & (ev[:, -1] > 0),
                "rank 1": ok & (np.abs(ev[:, -2]) <= 1e-6 * np.abs(ev[:, -1])) & (ev[:, -1] > 0),
                "two equal eigenvalues": ok & (ev[:, 1:] == ev[:, :-1]).any(1) & (ev[:, -1] != ev[:, 0]),
                "all eigenvalues equal": ok & (ev[:, -1] == ev[:, 0]) & (ev[:, 0] != 0),
                "zero matrix": ok & (ev == 0).all(1),
                "non-finite": ~np.isfinite(out).all(1),
                "info != 0": info != 0,
                "subnormal eigenvalue": ok & (np.abs(ev) < np.float32(1.1754944e-38)).any(1) & (ev != 0).any(1),
                "large": ok & (ev[:, -1] > 1e17),
            })
    for op in (0, 1, 2):  # the solves: a rank-deficient system leaves exact zeros in x
        out, _ = eigen_ref[op]
        _nonempty(mc.EIGEN_OPS[op], {"a dropped column": (out == 0).any(1) & (out != 0).any(1),
                                     "full rank": np.isfinite(out).all(1) & (out != 0).all(1), "non-finite": ~np.isfinite(out).all(1)})
    for op in (5, 6):
        out, _ = eigen_ref[op]
        _nonempty(mc.EIGEN_OPS[op], {"finite": np.isfinite(out).all(1), "zero pivot: inf / NaN": ~np.isfinite(out).all(1)})
    for op in (7, 8):  # the chain: rows of V2 zeroed or not
        N = 3 if op == 7 else 6
        out, info = eigen_ref[op]
        V, V2 = out[:, 2 * N:2 * N + N * N], out[:, 2 * N + N * N:2 * N + 2 * N * N]
        zeroed = ((V2.reshape(-1, N, N) == 0).all(1) & ~(V.reshape(-1, N, N) == 0).all(1)).sum(1)
        # (the eigenvalues ascend and the loop starts at the largest, so it zeroes every row or none)
        _nonempty(mc.EIGEN_OPS[op], {"no row zeroed": zeroed == 0, "every row zeroed": zeroed == N, "info != 0": info != 0})
    for op in (9, 10):
        p, q = mc.eigen_cases(op).T
        with np.errstate(all="ignore"):
            _nonempty(mc.EIGEN_OPS[op], {"q = 0": q == 0, "p = 0, q != 0": (p == 0) & (q != 0), "|p| > |q|": np.abs(p) > np.abs(q),
                                         "|p| <= |q|": (np.abs(p) <= np.abs(q)) & (q != 0) & (p != 0), "NaN": np.isnan(p) | np.isnan(q),
                                         "inf": np.isinf(p) | np.isinf(q), "subnormal": (np.abs(p) < 1.1754944e-38) & (p != 0)})


def test_pg_inputs_reach_every_branch():
    x, ok = mc.pg_trig_args()
    a = np.abs(x)
    _nonempty("trig", {"[-2 pi, 2 pi]": ok, "|x| <= pi/4": a <= np.pi / 4, "|x| < 2^-27": (a < 2.0 ** -27) & (a > 0),
                       "beyond the cutoff": np.isfinite(x) & (a > 2.0 ** 20 * np.pi / 2), "just inside the cutoff": (a > 1.6e6) & (a < 1.65e6),
                       "inf": np.isinf(x), "NaN": np.isnan(x), "subnormal": (a > 0) & (a < 2.3e-308)})
    for k in range(1, 17):  # both sides of every multiple of pi/4
        for s in (-1, 1):
            assert ((x > s * k * np.pi / 4 - 1e-13) & (x < s * k * np.pi / 4)).any() and ((x < s * k * np.pi / 4 + 1e-13) & (x > s * k * np.pi / 4)).any()
    x, ok = mc.pg_acos_args()
    _nonempty("acosd", {"|x| < 0.5": np.abs(x) < 0.5, "x < -0.5": (x < -0.5) & (x > -1), "x > 0.5": (x > 0.5) & (x < 1), "x = 1": x == 1,
                        "x = -1": x == -1, "|x| > 1": np.abs(x) > 1, "tiny": np.abs(x) <= 2.0 ** -57, "NaN": np.isnan(x)})
    assert ok.sum() > 200_000
    _nonempty("so3_log", mc.so3_log_branches(mc.so3_rotations()))
    t = mc.norm3(mc.so3_vectors())
    for want in mc.SO3_ANGLES:
        assert (np.abs(t - want) <= 1e-15 * max(want, 1e-300)).sum() >= 1538, want
    _nonempty("so3_exp", {"series": t * t < 1e-6, "sin / t": t * t >= 1e-6})
    pitch = mc.euler_angles()[:, 1]
    for g in mc.PITCH_GAPS:
        for s in (-1, 1):
            assert (pitch == s * (np.pi / 2 - g)).sum() == 200


# ---- where = 0 against the references ---------------------------------------------------------------------
@pytest.mark.parametrize("fn", range(len(mc.LIBM_FNS)), ids=lambda k: mc.LIBM_FNS[k])
def test_libm_host_compile_equals_glibc(fn):
    if mc.LIBM_FNS[fn] == "atan2f_":
        y, x = (np.concatenate(p) for p in zip(mc.atan2_grid(), mc.atan2_gaps()))
    else:
        x, y = mc.libm_unary(fn), None
    got, want = mc.debug_libm(fn, 0, x, y), mc.ref_libm32(fn, x, y)
    bad = ~mc.same_bits(got, want)
    assert not bad.any(), (f"{mc.LIBM_FNS[fn]}: {bad.sum()} of {len(x)} differ from glibc, first (x [y] got want): "
                           + mc.first_inputs(bad, x.view(np.uint32), *(() if y is None else (y.view(np.uint32),)), got, want))


@pytest.mark.parametrize("fn", [4, 5, 6], ids=lambda k: mc.LIBM_FNS[k])
def test_libm_trig_is_loud_from_120(fn):
    x = mc.libm_loud()
    assert len(x) > 50 and np.isnan(mc.debug_libm(fn, 0, x).view(np.float32)).all()


@pytest.mark.parametrize("op", range(len(mc.EIGEN_OPS)), ids=lambda k: mc.EIGEN_OPS[k])
def test_eigen_host_compile_equals_oracle(op, eigen_ref):
    inp = mc.eigen_cases(op)
    got, ginfo = mc.debug_eigen(op, 0, inp)
    want, winfo = eigen_ref[op]
    bad = ~mc.same_bits(got.view(np.uint32), want.view(np.uint32)).all(1) | (ginfo != winfo)
    j = np.flatnonzero(bad)[:1]
    assert not bad.any(), (f"{mc.EIGEN_OPS[op]}: {bad.sum()} of {len(inp)} cases differ from oracle_eigen, first case {j}: input "
                           f"{inp[j]!r}, first differing output {np.flatnonzero(got[j].view(np.uint32) != want[j].view(np.uint32))[:1]}, "
                           f"codes {ginfo[j]} / {winfo[j]}")


@pytest.mark.parametrize("name", list(mc.PG_REF))
def test_pg_trig_host_compile_within_one_ulp_of_glibc(name):
    assert (msg := mc.check_pg_trig(name, 0)) is None, msg


def test_pg_exp_then_log_returns_the_vector():
    w = mc.so3_vectors()
    back = mc.debug_pg(mc.PG_FNS.index("exp_then_log"), 0, w).view(np.float64)
    t = mc.norm3(w)[:, None]
    bad = ~((np.abs(back - w) <= 1e-9 * (1 + t)) | (np.abs(back + w) <= 1e-7)).all(1)
    assert not bad.any(), f"{bad.sum()} of {len(w)}, first (w back): " + mc.first_inputs(bad, w, back)


def test_pg_charts_compose_on_the_host():
    """so3_exp, so3_log, rot_rzryrx and rot_angles as separate calls: the round trip exp_then_log makes,
    and angles -> matrix -> angles away from the pitch singularity"""
    w = mc.so3_vectors()
    R = mc.debug_pg(mc.PG_FNS.index("so3_exp"), 0, w)
    back = mc.debug_pg(mc.PG_FNS.index("so3_log"), 0, R.view(np.float64))
    assert np.array_equal(back, mc.debug_pg(mc.PG_FNS.index("exp_then_log"), 0, w))
    e = mc.euler_angles()[:5000]
    e = e[np.abs(np.abs(e[:, 1]) - np.pi / 2) > 0.1]
    e = e[np.abs(e[:, 1]) < np.pi / 2]
    M = mc.debug_pg(mc.PG_FNS.index("rot_rzryrx"), 0, e).view(np.float64)
    np.testing.assert_allclose(M, mc._rzryrx(e[:, 0], e[:, 1], e[:, 2]), atol=1e-15)
    np.testing.assert_allclose(mc.debug_pg(mc.PG_FNS.index("rot_angles"), 0, M).view(np.float64), e, atol=1e-12)


# ---- ransac_k ---------------------------------------------------------------------------------------------
def test_ransac_k_host_compile_stops_where_the_oracle_does():
    K, cnt = mc.ransac_pairs()
    assert 11_000_000 < len(K) < 11_200_000
    got, want = mc.debug_ransac_k(0, K, cnt), mc.ref_ransac_k(K, cnt)
    bad = mc.stop_count(got) != mc.stop_count(want)
    assert not bad.any(), f"{bad.sum()} stopping counts differ, first (K cnt got want): " + mc.first_inputs(bad, K, cnt, got, want)
    assert mc.stop_count(want).min() == 1 and mc.stop_count(want).max() == mc.RANSAC_MAX_ITER


def test_ransac_k_margin_to_the_integers():
    K, cnt = mc.ransac_pairs()
    kk = mc.ref_ransac_k(K, cnt)
    dom = kk <= 10002
    assert dom.sum() > 10_000_000 and (kk[dom] > 0).all()
    rel = np.abs(kk[dom] - np.rint(kk[dom])) / kk[dom]
    j = np.argmin(rel)
    print(f"closest approach of k to an integer: {rel[j]:.3e} relative at K = {K[dom][j]}, cnt = {cnt[dom][j]}, k = {kk[dom][j]:.9f}")
    assert rel[j] >= 1e-11


# ---- the diagnostics' argument checks ------------------------------------------------------------------------
def test_diagnostics_refuse_bad_arguments():
    import ctypes as C
    from llsr import lib
    EINVAL = -22
    x, o32, o64, i32 = np.zeros(4, np.float32), np.zeros(4, np.uint32), np.zeros(16, np.uint64), np.zeros(4, np.int32)
    d, f = np.zeros(16, np.float64), np.zeros(64, np.float32)
    mc.debug_libm(0, 0, x)  # binds the argument types
    mc.debug_pg(0, 0, d[:4])
    mc.debug_eigen(9, 0, f[:8])
    mc.debug_ransac_k(0, np.array([3], np.int32), np.array([1], np.int32))
    L = lib()
    p = lambda a: a.ctypes.data  # noqa: E731
    for fn, where, n, px, py, po in ((9, 0, 4, p(x), None, p(o32)), (-1, 0, 4, p(x), None, p(o32)), (0, 2, 4, p(x), None, p(o32)),
                                     (0, 0, -1, p(x), None, p(o32)), (0, 0, (1 << 22) + 1, p(x), None, p(o32)),
                                     (0, 0, 4, None, None, p(o32)), (0, 0, 4, p(x), None, None), (3, 0, 4, p(x), None, p(o32))):
        assert L.llsr_debug_libm(fn, where, n, px, py, po) == EINVAL
    assert L.llsr_debug_eigen(11, 0, 1, p(f), p(f), p(i32)) == EINVAL
    assert L.llsr_debug_eigen(0, 0, 1, p(f), p(f), None) == EINVAL
    assert L.llsr_debug_eigen(0, 3, 1, p(f), p(f), p(i32)) == EINVAL
    assert L.llsr_debug_pg_math(10, 0, 1, p(d), p(o64)) == EINVAL
    assert L.llsr_debug_pg_math(0, 0, 1, None, p(o64)) == EINVAL
    assert L.llsr_debug_pg_math(0, 0, (1 << 22) + 1, p(d), p(o64)) == EINVAL
    K, c = np.array([3, 0], np.int32), np.array([1, 0], np.int32)
    assert L.llsr_debug_ransac_k(0, 2, p(K), p(c), p(o64)) == EINVAL  # K < 1
    K[1], c[1] = 3, 4
    assert L.llsr_debug_ransac_k(0, 2, p(K), p(c), p(o64)) == EINVAL  # cnt > K
    assert L.llsr_debug_ransac_k(0, 2, None, p(c), p(o64)) == EINVAL
    assert L.llsr_debug_libm(0, 0, 0, p(x), None, p(o32)) == 0  # n = 0 is a valid, empty call
