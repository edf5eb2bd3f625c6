"""Inputs for the call-by-call tests of the shared numeric headers (csrc/llsr_libm.h, llsr_eigen.h,
the double trigonometry and SO(3) charts of llsr_pg.h, llsr_device.h's ransac_k), and thin bindings
of the diagnostics that run them (csrc/llsr_math_debug.hip) and of the oracle's references
(oracle/oracle_math.cpp). numpy with fixed seeds, no files.

tests/test_math_cases_host.py shows on the CPU that every family reaches its branches and holds the
host compile to the references; tests/test_gpu_math_headers.py holds the gfx950 compile to both."""
import ctypes as C
import functools

import numpy as np

import oracle_py
from llsr import lib

F, D = np.float32, np.float64
U32, U64 = np.uint32, np.uint64
MAX_CASES = 1 << 22  # the diagnostics' bound per call

LIBM_FNS = ("asinf_", "acosf_", "atanf_", "atan2f_", "tanf_", "sinf_", "cosf_", "sqrt_", "ground_angle_deg")
EIGEN_OPS = ("qr33", "qr66", "qr53", "eig3", "eig6", "inv3", "inv6", "proj3", "proj6", "hypot", "givens")
EIGEN_IN = (12, 42, 20, 9, 36, 9, 36, 13, 43, 2, 2)
EIGEN_OUT = (3, 6, 3, 12, 42, 9, 36, 45, 162, 1, 2)
PG_FNS = ("sind", "cosd", "atand", "atan2d", "acosd", "so3_exp", "so3_log", "exp_then_log", "rot_rzryrx",
          "rot_angles")
PG_IN = (1, 1, 1, 2, 1, 3, 9, 3, 3, 9)
PG_OUT = (1, 1, 1, 1, 1, 9, 3, 3, 9, 3)
PG_REF = {"sind": 0, "cosd": 1, "atand": 2, "atan2d": 3, "acosd": 4}  # oracle_libm_f64's selector


# ---- bindings --------------------------------------------------------------------------------------
def _check(rc, what):
    assert rc == 0, f"{what}: {rc}"


def debug_libm(fn, where, x, y=None):
    """bits of LIBM_FNS[fn] on x (atan2f_(y, x) reads y)"""
    f = lib().llsr_debug_libm
    f.restype = C.c_int32
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    x = np.ascontiguousarray(x, F)
    y = None if y is None else np.ascontiguousarray(y, F)
    out = np.zeros(len(x), U32)
    _check(f(fn, where, len(x), x.ctypes.data, None if y is None else y.ctypes.data, out.ctypes.data),
           f"llsr_debug_libm({LIBM_FNS[fn]}, {where})")
    return out


def debug_eigen(op, where, inp):
    f = lib().llsr_debug_eigen
    f.restype = C.c_int32
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    inp = np.ascontiguousarray(inp, F).reshape(-1, EIGEN_IN[op])
    out, info = np.zeros((len(inp), EIGEN_OUT[op]), F), np.zeros(len(inp), np.int32)
    _check(f(op, where, len(inp), inp.ctypes.data, out.ctypes.data, info.ctypes.data),
           f"llsr_debug_eigen({EIGEN_OPS[op]}, {where})")
    return out, info


def debug_pg(fn, where, inp):
    f = lib().llsr_debug_pg_math
    f.restype = C.c_int32
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    inp = np.ascontiguousarray(inp, D).reshape(-1, PG_IN[fn])
    out = np.zeros((len(inp), PG_OUT[fn]), U64)
    _check(f(fn, where, len(inp), inp.ctypes.data, out.ctypes.data), f"llsr_debug_pg_math({PG_FNS[fn]}, {where})")
    return out


def debug_ransac_k(where, K, cnt):
    """kk of every pair as float64, MAX_CASES pairs a call"""
    f = lib().llsr_debug_ransac_k
    f.restype = C.c_int32
    f.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    out = np.zeros(len(K), U64)
    for s in range(0, len(K), MAX_CASES):
        k, c, o = K[s:s + MAX_CASES], cnt[s:s + MAX_CASES], out[s:s + MAX_CASES]
        _check(f(where, len(k), k.ctypes.data, c.ctypes.data, o.ctypes.data), f"llsr_debug_ransac_k({where})")
    return out.view(D)


def ref_libm32(fn, x, y=None):
    """glibc's float function of LIBM_FNS[fn]: bits"""
    x = np.ascontiguousarray(x, F)
    y = x if y is None else np.ascontiguousarray(y, F)
    out = np.zeros(len(x), F)
    _check(oracle_py.lib().oracle_libm_f32(fn, len(x), x.ctypes.data, y.ctypes.data, out.ctypes.data), "oracle_libm_f32")
    return out.view(U32)


def ref_libm64(fn, x, y=None):
    x = np.ascontiguousarray(x, D)
    y = x if y is None else np.ascontiguousarray(y, D)
    out = np.zeros(len(x), D)
    _check(oracle_py.lib().oracle_libm_f64(fn, len(x), x.ctypes.data, y.ctypes.data, out.ctypes.data), "oracle_libm_f64")
    return out


def ref_eigen(op, inp):
    inp = np.ascontiguousarray(inp, F).reshape(-1, EIGEN_IN[op])
    out, info = np.zeros((len(inp), EIGEN_OUT[op]), F), np.zeros(len(inp), np.int32)
    _check(oracle_py.lib().oracle_eigen_batch(op, len(inp), inp.ctypes.data, out.ctypes.data, info.ctypes.data),
           "oracle_eigen_batch")
    return out, info


def ref_ransac_k(K, cnt):
    out = np.zeros(len(K), D)
    oracle_py.lib().oracle_ransac_k(len(K), K.ctypes.data, cnt.ctypes.data, out.ctypes.data)
    return out


# ---- comparisons -------------------------------------------------------------------------------------
def same_bits(a, b):
    """per element: equal bit patterns, any two NaNs equal (the default NaN's sign differs between
    x86 and the GPU), signed zeros distinct; a, b uint32 or uint64 bits"""
    ft = F if a.dtype == U32 else D
    return (a == b) | (np.isnan(a.view(ft)) & np.isnan(b.view(ft)))


def ulps(got, want):
    """|got - want| in units of want's last place, as tests/native/pg_host_check.cpp measures it"""
    with np.errstate(all="ignore"):
        _, e = np.frexp(want)
        u = np.abs(got - want) / np.ldexp(1.0, e - 53)
    u = np.where(got == want, 0.0, u)
    both, one = np.isnan(got) & np.isnan(want), np.isnan(got) ^ np.isnan(want)
    return np.where(both, 0.0, np.where(one | np.isnan(u), 1e300, u))


def _show(v):
    if isinstance(v, np.ndarray):
        return "[" + " ".join(_show(e) for e in v.reshape(-1)) + "]"
    if isinstance(v, (np.uint32, np.uint64)):
        return f"{int(v):0{2 * v.itemsize}x}"
    return repr(v.item())


def first_inputs(bad, *cols):
    """the first five cases of `bad`, one column after the other (bit patterns in hex)"""
    return "; ".join(" ".join(_show(c[j]) for c in cols) for j in np.flatnonzero(bad)[:5])


def check_pg_trig(name, where):
    """-> message or None: PG_FNS name at `where` against glibc"""
    fn = PG_FNS.index(name)
    inp = pg_cases(fn)
    ok = {"acosd": pg_acos_args, "atan2d": pg_atan2_args}.get(name, pg_trig_args)()[1]
    got = debug_pg(fn, where, inp).view(np.float64)[:, 0]
    want = ref_libm64(PG_REF[name], inp[:, -1], inp[:, 0])  # atan2d's rows are (y, x)
    u = ulps(got, want)
    print(f"{name} where {where}: largest difference on the asserted domain {u[ok].max():.3f} ulp over {ok.sum()} arguments")
    bad = ok & (u > 1.0)
    if bad.any():
        return f"{name}: {bad.sum()} beyond 1 ulp of glibc, first (input got want): " + first_inputs(bad, inp, got, want)
    # outside: the rem_pio2 cutoff answers NaN where glibc answers a number, so only what both define
    cut = np.isfinite(inp).all(1) & (np.abs(inp) > 1.6e6).any(1) if name in ("sind", "cosd") else np.zeros(len(inp), bool)
    bad = ~ok & ~cut & ((np.isnan(got) != np.isnan(want)) | (np.isfinite(got) != np.isfinite(want)))
    if bad.any():
        return f"{name}: {bad.sum()} differ from glibc in NaN-ness or finiteness, first: " + first_inputs(bad, inp, got, want)
    if name in ("sind", "cosd"):
        beyond = np.isfinite(inp[:, 0]) & (np.abs(inp[:, 0]).view(np.uint64) >> np.uint64(32) > 0x413921fb)
        if not (beyond.any() and np.isnan(got[beyond]).all() and not np.isnan(got[cut & ~beyond]).any()):
            return f"{name}: NaN exactly beyond 2^20 pi/2 expected"
    return None


# ---- libm, unary ---------------------------------------------------------------------------------------
def _f32_bits(v):
    return np.asarray(v, F).reshape(-1).view(U32).astype(np.int64)


def _around(mag_bits, span=8):
    """bit patterns within `span` ulp of each magnitude, both sides, both signs"""
    b = (np.asarray(mag_bits, np.int64)[:, None] + np.arange(-span, span + 1)[None, :]).reshape(-1)
    b = np.unique(np.clip(b, 0, 0x7fffffff))
    return np.concatenate([b, b | 0x80000000]).astype(U32)


@functools.lru_cache(None)
def libm_edge_magnitudes():
    specials = [0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000, 0x7fc00000]
    pow2 = _f32_bits([2.0 ** k for k in range(-30, 8)])
    # the branch constants of llsr_libm.h
    hexes = [0x3f2ca140, 0x3f490fda, 0x39000000, 0x32000000, 0x3f79999a, 0x32800000, 0x4c000000, 0x31000000,
             0x42f00000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000]
    consts = _f32_bits([0.5, 1.0, 7 / 16, 11 / 16, 19 / 16, 39 / 16, 2.0 ** -29, 2.0 ** -31, 2.0 ** 25, 2.0 ** 34,
                        np.pi / 4, 2.0 ** -12, 2.0 ** -13, 120.0])
    halfpi = _f32_bits([k * np.pi / 2 for k in range(1, 77)])
    return np.unique(np.concatenate([specials, pow2, hexes, consts, halfpi]))


@functools.lru_cache(None)
def libm_edges():
    return _around(libm_edge_magnitudes()).view(F)


@functools.lru_cache(None)
def libm_unary(fn):
    """the strided sweep of the float bit space and the edge list; tanf_ / sinf_ / cosf_ keep |x| < 120
    and the non-finite values (the ports answer NaN from 120 on, test_math_cases_host.py holds that)"""
    x = np.concatenate([np.arange(0, 1 << 32, 4099, dtype=np.uint64).astype(U32).view(F), libm_edges()])
    if LIBM_FNS[fn] in ("tanf_", "sinf_", "cosf_"):
        x = x[~(np.abs(x) >= F(120.0)) | ~np.isfinite(x)]
    return x


def libm_loud():
    """finite |x| >= 120: tanf_ / sinf_ / cosf_ answer NaN"""
    x = libm_edges()
    return x[np.isfinite(x) & (np.abs(x) >= F(120.0))]


def _ix(x):
    return (np.asarray(x, F).view(U32) & U32(0x7fffffff)).astype(np.int64)


def _quadrant(x):
    """n of reduce_fast / tanf_'s reduction"""
    r = x.astype(D) * float.fromhex("0x1.45F306DC9C883p+23")
    return (r.astype(np.int32).astype(np.int64) + 0x800000) >> 24


def libm_branches(fn, x, y=None):
    """name -> mask of the inputs that take each branch of LIBM_FNS[fn] (the intervals of llsr_libm.h)"""
    name, ix, neg, nan = LIBM_FNS[fn], _ix(x), np.signbit(x), np.isnan(x)
    if name == "asinf_":
        return {"|x| = 1": ix == 0x3f800000, "|x| > 1 or NaN": ix > 0x3f800000, "tiny": ix < 0x32000000,
                "|x| < 0.5": (ix >= 0x32000000) & (ix < 0x3f000000), "0.5 <= |x| < 0.975": (ix >= 0x3f000000) & (ix < 0x3f79999a),
                "0.975 <= |x| < 1": (ix >= 0x3f79999a) & (ix < 0x3f800000)}
    if name in ("acosf_", "ground_angle_deg"):
        return {"x = 1": (ix == 0x3f800000) & ~neg, "x = -1": (ix == 0x3f800000) & neg, "|x| > 1 or NaN": ix > 0x3f800000,
                "tiny": ix <= 0x32800000, "|x| < 0.5": (ix > 0x32800000) & (ix < 0x3f000000),
                "x <= -0.5": (ix >= 0x3f000000) & (ix < 0x3f800000) & neg, "x >= 0.5": (ix >= 0x3f000000) & (ix < 0x3f800000) & ~neg}
    if name == "atanf_":
        cuts = [0x31000000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000, 0x4c000000]
        out = {"NaN": nan, "|x| >= 2^25": (ix >= 0x4c000000) & ~nan, "|x| < 2^-29": ix < 0x31000000}
        for k, nm in enumerate(("< 7/16", "< 11/16", "< 19/16", "< 39/16", "< 2^25")):
            out[nm] = (ix >= cuts[k]) & (ix < cuts[k + 1])
        return out
    if name == "tanf_":
        n = _quadrant(np.where(np.isfinite(x), x, F(0)))
        red = (ix > 0x3f490fda) & (ix < 0x42f00000)
        return {"|x| < 2^-13": ix < 0x39000000, "|x| < 0.6744": (ix >= 0x39000000) & (ix < 0x3f2ca140),
                "0.6744 <= |x| <= pi/4": (ix >= 0x3f2ca140) & (ix <= 0x3f490fda), "reduced, even": red & (n % 2 == 0),
                "reduced, odd": red & (n % 2 == 1), "non-finite": ix >= 0x7f800000}
    if name in ("sinf_", "cosf_"):
        top = ix >> 20
        n = _quadrant(np.where(np.isfinite(x), x, F(0)))
        red = (top >= (0x3f490fdb >> 20)) & (top < (0x42f00000 >> 20))
        out = {"|x| < 2^-12": top < (0x39800000 >> 20), "|x| < pi/4": (top >= (0x39800000 >> 20)) & (top < (0x3f490fdb >> 20)),
               "non-finite": top >= (0x7f800000 >> 20)}
        for q in range(4):
            out[f"reduced, n & 3 = {q}"] = red & ((n & 3) == q)
        return out
    if name == "sqrt_":
        return {"negative": neg & (ix > 0) & ~nan, "zero": ix == 0, "subnormal": (ix > 0) & (ix < 0x00800000) & ~neg,
                "normal": (ix >= 0x00800000) & (ix < 0x7f800000) & ~neg, "inf or NaN": ix >= 0x7f800000}
    # atan2f_(y, x)
    iy, ynan, xneg, yneg = _ix(y), np.isnan(y), np.signbit(x), np.signbit(y)
    fin = (ix < 0x7f800000) & (iy < 0x7f800000) & (ix > 0) & (iy > 0) & (np.asarray(x, F).view(U32) != 0x3f800000)
    k = (iy - ix) >> 23
    out = {"NaN": nan | ynan, "x = 1": (np.asarray(x, F).view(U32) == 0x3f800000) & ~ynan}
    for m in range(4):
        sel = (yneg == bool(m & 1)) & (xneg == bool(m & 2)) & ~nan & ~ynan & (np.asarray(x, F).view(U32) != 0x3f800000)
        out[f"y = 0, m = {m}"] = sel & (iy == 0)
        out[f"both inf, m = {m}"] = sel & (ix == 0x7f800000) & (iy == 0x7f800000)
        out[f"x inf, m = {m}"] = sel & (ix == 0x7f800000) & (iy < 0x7f800000) & (iy > 0)
        out[f"quotient, m = {m}"] = sel & fin & (k <= 60) & ~(xneg & (k < -60))
    out["x = 0"] = (ix == 0) & (iy > 0) & ~ynan
    out["y inf"] = (iy == 0x7f800000) & (ix < 0x7f800000) & (ix > 0)
    out["k > 60"] = fin & (k > 60)
    out["x < 0, k < -60"] = fin & xneg & (k < -60)
    return out


# ---- atan2f_ -----------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def atan2_list():
    """1024 values: the unary edge list thinned, keeping the zeros, subnormals, infinities, a NaN and
    every decade from 1e-38 to 1e38 in both signs"""
    keep = np.array([0x0, 0x1, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000, 0x3f800000, 0x3f000000], np.int64)
    keep = np.concatenate([keep, keep | 0x80000000, [0x7fc00000]]).astype(U32).view(F)
    dec = np.array([10.0 ** k for k in range(-38, 39)], D).astype(F)
    must = np.unique(np.concatenate([keep, dec, -dec]).view(U32))
    rest = np.setdiff1d(libm_edges().view(U32), must)
    pick = rest[np.linspace(0, len(rest) - 1, 1024 - len(must)).astype(np.int64)]
    out = np.concatenate([must, pick]).view(F)
    assert len(np.unique(out.view(U32))) == 1024
    return out


@functools.lru_cache(None)
def atan2_grid():
    """(y, x): the 1024 x 1024 grid"""
    v = atan2_list()
    return np.repeat(v, len(v)), np.tile(v, len(v))


@functools.lru_cache(None)
def atan2_gaps():
    """(y, x): random pairs with |y / x| within 2^-20 of 2^+-26 (10^5) and of 2^+-60, the exponent gap at
    which atan2f_ stops dividing (10^5)"""
    rng = np.random.default_rng(20)
    ys, xs = [], []
    for gap, span in ((26, 60), (60, 30)):
        n = 100_000
        x = np.exp2(rng.uniform(-span, span, n)) * rng.choice([-1.0, 1.0], n)
        e = rng.choice([-gap, gap], n)
        y = np.abs(x) * np.exp2(e.astype(D)) * (1.0 + rng.uniform(-2.0 ** -20, 2.0 ** -20, n)) * rng.choice([-1.0, 1.0], n)
        ys.append(y.astype(F))
        xs.append(x.astype(F))
    return np.concatenate(ys), np.concatenate(xs)


# ---- eigen -----------------------------------------------------------------------------------------------
def _colmajor(M):
    """(n, r, c) matrices -> (n, r * c) column-major"""
    return np.ascontiguousarray(np.swapaxes(M, 1, 2)).reshape(len(M), -1)


def normal_eq(W, n, seed, rows=32):
    """The four modes of tests/native/eigen_cross.cpp's normal_eq in float32: A^T A and A^T b of
    10..`rows` random Jacobian rows of width W at a scale of 10^-3..10^3; mode 1 one weak direction,
    2 two exactly dependent columns, 3 half the directions weak. -> AtA (n, W, W), AtB (n, W), mode"""
    rng = np.random.default_rng(seed)
    mode = np.arange(n) % 4
    scale = (10.0 ** rng.uniform(-3, 3, n)).astype(F)
    J = rng.uniform(-1, 1, (n, rows, W)).astype(F) * scale[:, None, None]
    J[mode == 1, :, W - 1] *= F(1e-3)
    J[mode == 2, :, 1] = J[mode == 2, :, 0] * F(0.5)
    J[mode == 3, :, W // 2:] *= F(1e-4)
    J[np.arange(rows)[None, :] >= rng.integers(10, rows + 1, n)[:, None]] = 0
    b = rng.uniform(-0.1, 0.1, (n, rows)).astype(F)
    AtA = np.matmul(np.swapaxes(J, 1, 2), J).astype(F)
    lo = np.tril(AtA)
    AtA = lo + np.swapaxes(np.tril(AtA, -1), 1, 2)
    AtB = np.matmul(np.swapaxes(J, 1, 2), b[:, :, None])[:, :, 0].astype(F)
    return AtA.astype(F), AtB, mode


def eigen_edges(N):
    """(A (m, N, N), b (m, N)): the matrices at which the restatement's branches turn"""
    rng = np.random.default_rng(30 + N)
    Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
    v = rng.uniform(0.5, 1.5, N)
    spd = (Q * np.geomspace(0.5, 50.0, N)) @ Q.T
    two = np.array([1.0, 1.0] + list(range(2, N)))
    three = np.array([2.0, 2.0, 2.0] + list(range(3, N)))
    zero_col = np.eye(N)
    zero_col[:, 2] = 0
    lead0 = np.eye(N)[::-1].copy()  # needs every row swap
    lead0[0, 0] = 0
    nan1, inf1 = spd.copy(), spd.copy()
    nan1[1, 0] = nan1[0, 1] = np.nan
    inf1[N - 1, N - 1] = np.inf
    mats = [np.zeros((N, N)), np.eye(N), np.diag(np.arange(1.0, N + 1)), np.outer(v, v), np.diag(two), (Q * two) @ Q.T,
            np.diag(three), (Q * three) @ Q.T, 3.0 * np.eye(N), zero_col, lead0, nan1, inf1]
    for s in (1e18, 1e-18, 1e-30, 1e-40, 1e-44):  # the last three carry entries into the subnormals
        mats += [spd * s, np.outer(v, v) * s, np.diag(np.arange(1.0, N + 1)) * s]
    with np.errstate(all="ignore"):
        A = np.array(mats).astype(F)
    b = np.tile(np.linspace(-1.0, 1.0, N).astype(F), (len(A), 1))
    return A, b


@functools.lru_cache(None)
def eigen_cases(op, n=20000):
    """the packed inputs of EIGEN_OPS[op] (n random cases per family next to the edge lists)"""
    name = EIGEN_OPS[op]
    if name in ("hypot", "givens"):
        v = atan2_list()[np.linspace(0, 1023, 256).astype(np.int64)]
        return np.stack([np.repeat(v, 256), np.tile(v, 256)], 1)
    if name == "qr53":
        A, b = plane_fits(n)
        return np.concatenate([_colmajor(A), b], 1)
    N = 3 if name.endswith("3") or name == "qr33" else 6
    A, b, _ = normal_eq(N, n, 40 + N)
    Ae, be = eigen_edges(N)
    A, b = np.concatenate([A, Ae]), np.concatenate([b, be])
    if name == "eig3":
        A = np.concatenate([A, covariances(n)])
    if name in ("inv3", "inv6"):
        # inverse() is applied to eigenvector matrices: orthonormal ones next to everything above
        rng = np.random.default_rng(50 + N)
        Q = np.linalg.qr(rng.normal(size=(n // 4, N, N)))[0].astype(F)
        A = np.concatenate([A, Q])
    flat = _colmajor(A)
    if name.startswith("qr"):
        return np.concatenate([flat, b], 1)
    if name.startswith("proj"):
        base = F(10.0) if N == 3 else F(100.0)  # FA:1968 / MO:1514's thresholds, and far above every value
        thr = np.where(np.arange(len(A)) % 2 == 1, base * F(1e6), base).astype(F)
        return np.concatenate([flat, b, thr[:, None]], 1)
    return flat


def plane_fits(n, seed=60):
    """MO:1398's 5 x 3 systems as eigen_cross.cpp draws them (random points, points on a plane, on a
    2 cm lattice, repeated xy), then five collinear and five coincident points, zero, NaN, inf and
    scaled ones; b = -1. -> A (m, 5, 3), b (m, 5)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    nrm, d = rng.uniform(-1, 1, (n, 3)).astype(F), rng.uniform(-30, 30, n).astype(F)
    x, y = rng.uniform(-40, 40, (n, 5)).astype(F), rng.uniform(-40, 40, (n, 5)).astype(F)
    z = np.where((t % 3 == 0)[:, None], rng.uniform(-3, 3, (n, 5)).astype(F),
                 -(d[:, None] + nrm[:, :1] * x + nrm[:, 1:2] * y) / nrm[:, 2:3]).astype(F)
    lat = (t % 3 == 2)[:, None]
    x, y, z = (np.where(lat, np.round(a * F(50)) / F(50), a).astype(F) for a in (x, y, z))
    rep = (t % 7 == 0)
    x[rep, 1:], y[rep, 1:] = x[rep, :1], y[rep, :1]
    A = np.stack([x, y, z], 2)
    s = np.linspace(-2, 2, 5)
    line = np.stack([1 + 0.5 * s, -2 + 0.25 * s, 0.5 - s], 1)
    point = np.tile([[3.0, -1.5, 0.25]], (5, 1))
    gen = rng.uniform(-5, 5, (5, 3))
    nan1, inf1 = gen.copy(), gen.copy()
    nan1[2, 1], inf1[4, 0] = np.nan, np.inf
    with np.errstate(all="ignore"):
        edges = np.array([line, point, np.zeros((5, 3)), nan1, inf1, gen * 1e18, gen * 1e-18, gen * 1e-42,
                          line * 1e-42, line * 1e18]).astype(F)
    A = np.concatenate([A, edges])
    return A, np.full((len(A), 5), -1, F)


def covariances(n, seed=70):
    """MO:1320's covariance of five points on / near a line, as eigen_cross.cpp draws them"""
    rng = np.random.default_rng(seed)
    dr, c = rng.uniform(-1, 1, (n, 3)).astype(F), rng.uniform(-50, 50, (n, 2)).astype(F)
    s = rng.uniform(-0.5, 0.5, (n, 5)).astype(F)
    nz = np.where((np.arange(n) % 2 == 1)[:, None], rng.uniform(-0.01, 0.01, (n, 5)), 0).astype(F)
    p = np.stack([c[:, :1] + s * dr[:, :1] + nz, c[:, 1:] + s * dr[:, 1:2] - nz, s * dr[:, 2:] + nz], 2).astype(F)
    a = p - (p.sum(1, dtype=F) / F(5))[:, None, :]
    return (np.matmul(np.swapaxes(a, 1, 2), a) / F(5)).astype(F)


# ---- pg math ---------------------------------------------------------------------------------------------
def _around64(vals, span=8):
    b = np.asarray(vals, D).view(np.int64)
    b = (b[:, None] + np.arange(-span, span + 1)[None, :]).reshape(-1)
    return np.unique(b).view(D)


@functools.lru_cache(None)
def pg_trig_args():
    """(x, asserted): asserted marks [-2 pi, 2 pi], where the 1-ulp bound holds; the rest (up to the
    2^20 pi/2 cutoff and beyond, inf, NaN) compares NaN class and finiteness only"""
    rng = np.random.default_rng(80)
    near = np.concatenate([_around64([k * np.pi / 4 for k in range(1, 17)]), _around64([7 / 16, 11 / 16, 19 / 16, 39 / 16,
                                                                                         2.0 ** -29, 2.0 ** -27, 2.0 ** 66])])
    cut = np.array([0x413921fbffffffff, 0x413921fc00000000, 0x413921fb00000000], np.int64).view(D)
    rest = np.array([0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e9, 1e300, np.inf, np.nan])
    x = np.concatenate([rng.uniform(-2 * np.pi, 2 * np.pi, 200_000), near, -near, cut, -cut, rest, -rest])
    return x, np.abs(x) <= 2 * np.pi


@functools.lru_cache(None)
def pg_acos_args():
    """(x, asserted): the trig arguments scaled into [-1, 1], +-1 +- 8 ulp, the |x| < 2^-57 branch"""
    x, ok = pg_trig_args()
    x = np.concatenate([x[ok] / (2 * np.pi), _around64([1.0, 0.5, 2.0 ** -57]), -_around64([1.0, 0.5, 2.0 ** -57]),
                        [0.0, -0.0, 2.0, np.inf, np.nan]])
    return x, np.abs(x) <= 1.0


@functools.lru_cache(None)
def pg_atan2_args():
    """((y, x) rows, asserted)"""
    x, ok = pg_trig_args()
    rng = np.random.default_rng(81)
    y = x[rng.permutation(len(x))]
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 5e-324, 1e-300, 1e300, -1e300, 2.0 ** -70, 3.0])
    pairs = np.concatenate([np.stack([y, x], 1), np.stack([np.repeat(sp, len(sp)), np.tile(sp, len(sp))], 1)])
    return pairs, (np.abs(pairs) <= 2 * np.pi).all(1)


SO3_ANGLES = (0.0, 1e-300, 1e-12, 1e-8, 1e-4, 1.0, np.pi - 1e-3, np.pi - 1e-5, np.pi - 1e-6 + 1e-9, np.pi - 1e-6 - 1e-9,
              np.pi - 1e-7, np.pi - 1e-9, np.pi)


@functools.lru_cache(None)
def so3_vectors():
    """~2 10^4 rotation vectors: every angle of SO3_ANGLES on each coordinate axis and on random axes"""
    rng = np.random.default_rng(82)
    ax = rng.normal(size=(1532, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ax = np.concatenate([np.eye(3), -np.eye(3), ax])
    return np.concatenate([t * ax for t in SO3_ANGLES])


def norm3(w):
    """|w| per row without squaring the tiniest rows into zero"""
    s = np.abs(w).max(1)
    s = np.where(s > 0, s, 1.0)
    return s * np.linalg.norm(w / s[:, None], axis=1)


def _rodrigues(w):
    t = norm3(w)
    with np.errstate(all="ignore"):
        a = np.where(t[:, None] > 0, w / t[:, None], 0.0)
    S = np.zeros((len(w), 3, 3))
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    return np.eye(3) + np.sin(t)[:, None, None] * S + (1 - np.cos(t))[:, None, None] * (S @ S)


@functools.lru_cache(None)
def so3_rotations():
    """rotations (n, 9) row-major at the same angles, by numpy's Rodrigues formula"""
    return _rodrigues(so3_vectors()).reshape(-1, 9)


def so3_log_branches(R):
    """name -> mask over rotations: which branch so3_log's chart takes"""
    v = np.stack([R[:, 7] - R[:, 5], R[:, 2] - R[:, 6], R[:, 3] - R[:, 1]], 1)
    c = 0.5 * (((R[:, 0] + R[:, 4]) + R[:, 8]) - 1.0)
    s2 = (v ** 2).sum(1)
    s = 0.5 * np.sqrt(s2)
    axis = (s < 1e-6) & (c < 0)
    small = ~axis & (s2 < 4e-6) & (c > 0)
    return {"axis from the diagonal": axis, "series": small, "atan2": ~axis & ~small}


def _rzryrx(a, b, c):
    sx, cx, sy, cy, sz, cz = np.sin(a), np.cos(a), np.sin(b), np.cos(b), np.sin(c), np.cos(c)
    return np.stack([cy * cz, sx * sy * cz - cx * sz, sx * sz + cx * sy * cz, cy * sz, cx * cz + sx * sy * sz,
                     cx * sy * sz - sx * cz, -sy, sx * cy, cx * cy], 1)


PITCH_GAPS = (1e-3, 1e-6, 1e-9, 0.0)


@functools.lru_cache(None)
def euler_angles():
    """(a, b, c) rows: 5000 random ones, then pitch b within PITCH_GAPS of +-pi/2, 200 each"""
    rng = np.random.default_rng(83)
    out = [rng.uniform(-np.pi, np.pi, (5000, 3))]
    for g in PITCH_GAPS:
        for sgn in (-1.0, 1.0):
            e = rng.uniform(-np.pi, np.pi, (200, 3))
            e[:, 1] = sgn * (np.pi / 2 - g)
            out.append(e)
    return np.concatenate(out)


@functools.lru_cache(None)
def euler_rotations():
    e = euler_angles()
    return _rzryrx(e[:, 0], e[:, 1], e[:, 2])


@functools.lru_cache(None)
def pg_cases(fn):
    name = PG_FNS[fn]
    if name in ("sind", "cosd", "atand"):
        return pg_trig_args()[0][:, None]
    if name == "acosd":
        return pg_acos_args()[0][:, None]
    if name == "atan2d":
        return pg_atan2_args()[0]
    if name in ("so3_exp", "exp_then_log"):
        return so3_vectors()
    if name == "so3_log":
        return np.concatenate([so3_rotations(), euler_rotations()])
    if name == "rot_rzryrx":
        return euler_angles()
    return np.concatenate([euler_rotations(), so3_rotations()])


# ---- ransac_k ---------------------------------------------------------------------------------------------
# (91693 is where a scan of this domain with other random K found k closest to an integer)
RANSAC_K_FIXED = (28799, 28800, 32768, 57600, 65536, 115200, 91693)
RANSAC_MAX_ITER = 10001  # the loop of k_ground_elev_ransac leaves at iterations > 10000 whatever k is


@functools.lru_cache(None)
def ransac_pairs():
    """(K, cnt) int32: every K in 3..4096, RANSAC_K_FIXED and 40 random K in 4097..115200, each with
    every cnt in 0..K"""
    rng = np.random.default_rng(90)
    Ks = np.concatenate([np.arange(3, 4097), RANSAC_K_FIXED, rng.integers(4097, 115201, 40)]).astype(np.int64)
    K = np.repeat(Ks, Ks + 1)
    start = np.repeat(np.cumsum(Ks + 1) - (Ks + 1), Ks + 1)
    cnt = np.arange(len(K)) - start
    return K.astype(np.int32), cnt.astype(np.int32)


def stop_count(kk):
    """min{n >= 0 : not (n < kk)}, clamped to RANSAC_MAX_ITER: the iteration at which `iterations < k` fails"""
    with np.errstate(all="ignore"):
        n = np.where(kk > 0, np.ceil(np.minimum(kk, RANSAC_MAX_ITER)), 0.0)
    return np.where(np.isnan(kk), 0, n).astype(np.int64)
