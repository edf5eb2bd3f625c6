"""The expected side of the loop closure's host entry points: the candidate of detectLoopClosure
(mapOptmization.cpp:902-919), one ICP iteration's rigid estimate (Eigen::umeyama without scaling)
and the pose constraint of performLoopClosure (MO:1056-1081), restated from DESIGN.md §16, not from
the library's code, in numpy float32 (one rounding per operation, no FMA) and Python floats (IEEE
double). It never calls the library. libm's float functions come from the host's libm.so.6 through
ctypes; the radius set comes from the oracle (oracle_py.keypose_radius).

Sequential sums are written as cumulative sums from an explicit zero: numpy's accumulate adds one
element at a time in the array's own type, which is the order §16 fixes."""
import ctypes

import numpy as np

import oracle_py

F = np.float32
_libm = ctypes.CDLL("libm.so.6")
for _n in ("sinf", "cosf", "asinf"):
    getattr(_libm, _n).argtypes = [ctypes.c_float]
    getattr(_libm, _n).restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.atan2f.restype = ctypes.c_float

FLT_MIN = F(1.17549435082228751e-38)
FLT_EPS = F(1.1920928955078125e-07)
ZERO, ONE = F(0.0), F(1.0)


def sinf(x): return F(_libm.sinf(float(x)))
def cosf(x): return F(_libm.cosf(float(x)))
def asinf(x): return F(_libm.asinf(float(x)))
def atan2f(y, x): return F(_libm.atan2f(float(y), float(x)))


def seq_sum(x, dtype):
    """Sequential sum from zero in `dtype`."""
    x = np.asarray(x, dtype)
    return np.cumsum(np.concatenate([np.zeros(1, dtype), x]), dtype=dtype)[-1]


def gemm_kc(k, m, n, l1=32 * 1024):
    """Eigen 3.3.7's depth block for an m x n result of depth k (SSE, mr = 8, nr = 4, float)."""
    if max(k, m, n) < 48:
        return k
    max_kc = max(((l1 - 8 * 4 * 4) // (8 * 4 + 4 * 4)) & ~7, 1)
    if k <= max_kc:
        return k
    if k % max_kc == 0:
        return max_kc
    return max_kc - 8 * ((max_kc - 1 - (k % max_kc)) // (8 * (k // max_kc + 1)))


# ---- the 3x3 SVD: two-sided Jacobi over the pairs (0,1), (0,2), (1,2) ------------------------------
def _rot_rows(M, p, q, c, s):
    x, y = M[p].copy(), M[q].copy()
    M[p] = c * x + s * y
    M[q] = c * y - s * x


def _rot_cols(M, p, q, c, s):
    x, y = M[:, p].copy(), M[:, q].copy()
    M[:, p] = c * x - s * y
    M[:, q] = s * x + c * y


def svd3(A):
    """A = U diag(sv) V^T in float32; sv non-negative, descending."""
    with np.errstate(over="ignore"):  # tau^2 may overflow to inf, which gives the rotation (1, 0)
        return _svd3(A)


def _svd3(A):
    M = np.array(A, np.float32).reshape(3, 3).copy()
    U, V = np.eye(3, dtype=np.float32), np.eye(3, dtype=np.float32)
    precision = F(2.0) * FLT_EPS
    maxd = max(abs(M[0, 0]), abs(M[1, 1]), abs(M[2, 2]))
    for _ in range(30):
        finished = True
        for p, q in ((0, 1), (0, 2), (1, 2)):
            thr = max(FLT_MIN, precision * maxd)
            b, c = M[p, q], M[q, p]
            if not max(abs(b), abs(c)) > thr:
                continue
            finished = False
            t, d = M[p, p] + M[q, q], c - b
            c1, s1 = ONE, ZERO
            if not abs(d) < FLT_MIN:
                u = t / d
                w = np.sqrt(ONE + u * u)
                s1, c1 = ONE / w, u / w
            _rot_rows(M, p, q, c1, s1)
            _rot_cols(U, p, q, c1, -s1)
            x, y, z = M[p, p], M[p, q], M[q, q]
            deno = F(2.0) * abs(y)
            c2, s2 = ONE, ZERO
            if not deno < FLT_MIN:
                tau = (x - z) / deno
                w = np.sqrt(tau * tau + ONE)
                tt = ONE / (tau + w) if tau > ZERO else ONE / (tau - w)
                n = ONE / np.sqrt(tt * tt + ONE)
                sg = (ONE if tt > ZERO else -ONE) * (ONE if y > ZERO else -ONE)
                s2, c2 = -sg * abs(tt) * n, n
            _rot_rows(M, p, q, c2, -s2)
            _rot_cols(M, p, q, c2, s2)
            _rot_cols(U, p, q, c2, s2)
            _rot_cols(V, p, q, c2, s2)
            maxd = max(maxd, abs(M[p, p]), abs(M[q, q]))
        if finished:
            break
    sv = np.array([M[0, 0], M[1, 1], M[2, 2]], np.float32)
    for k in range(3):
        if sv[k] < ZERO:
            sv[k] = -sv[k]
            U[:, k] = -U[:, k]
    for i in range(2):
        best = i
        for j in range(i + 1, 3):
            if sv[j] > sv[best]:
                best = j
        if best != i:
            sv[[i, best]] = sv[[best, i]]
            U[:, [i, best]] = U[:, [best, i]]
            V[:, [i, best]] = V[:, [best, i]]
    return U, sv, V


def _det3(m):
    return ((m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]))
            + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))


def umeyama(src, dst):
    """Eigen::umeyama without scaling of float32 correspondences src[n, 3] -> dst[n, 3]: 4x4 float32."""
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
    dst = np.ascontiguousarray(dst, np.float32).reshape(-1, 3)
    n = len(src)
    inv_n = ONE / F(n)
    sm = np.array([seq_sum(src[:, a], np.float32) * inv_n for a in range(3)], np.float32)
    dm = np.array([seq_sum(dst[:, a], np.float32) * inv_n for a in range(3)], np.float32)
    sd, dd = src - sm, dst - dm
    sigma = np.zeros((3, 3), np.float32)
    kc = gemm_kc(n, 3, 3)
    for k0 in range(0, n, kc):
        k1 = min(n, k0 + kc)
        for i in range(3):
            for j in range(3):
                sigma[i, j] = sigma[i, j] + inv_n * seq_sum(dd[k0:k1, i] * sd[k0:k1, j], np.float32)
    U, _, V = svd3(sigma)
    s2 = -ONE if _det3(U) * _det3(V) < ZERO else ONE
    T = np.zeros((4, 4), np.float32)
    for i in range(3):
        for j in range(3):
            T[i, j] = (U[i, 0] * V[j, 0] + U[i, 1] * V[j, 1]) + (U[i, 2] * s2) * V[j, 2]
        T[i, 3] = dm[i] - ((T[i, 0] * sm[0] + T[i, 1] * sm[1]) + T[i, 2] * sm[2])
    T[3, 3] = ONE
    return T


# ---- the candidate ------------------------------------------------------------------------------------
def sq_dist(poses4, pos):
    p = np.ascontiguousarray(poses4, np.float32).reshape(-1, 4)
    q = np.asarray(pos, np.float32)
    d = np.zeros(len(p), np.float32)
    for a in range(3):
        df = q[a] - p[:, a]
        d = d + df * df
    return d


def radius_sorted(poses4, pos, radius):
    """The radius set from the oracle, ordered by ascending float32 d^2, equal d^2 by index."""
    p = np.ascontiguousarray(poses4, np.float32).reshape(-1, 4)
    if not len(p):
        return np.zeros(0, np.int32)
    idx = np.sort(oracle_py.keypose_radius(p, pos, radius))
    d = sq_dist(p, pos)
    return idx[np.argsort(d[idx], kind="stable")].astype(np.int32)


def candidate(poses4, times, pos, now, radius, gap=30.0):
    times = np.asarray(times, np.float64)
    for k in radius_sorted(poses4, pos, radius):
        if abs(float(times[k]) - float(now)) > gap:  # NaN compares false
            return int(k)
    return -1


# ---- the pose constraint (MO:1056-1081) -----------------------------------------------------------
def get_transformation(x, y, z, roll, pitch, yaw):
    A, B, C, D, E, Fs = cosf(yaw), sinf(yaw), cosf(pitch), sinf(pitch), cosf(roll), sinf(roll)
    DE, DF = D * E, D * Fs
    return np.array([[A * C, A * DF - B * E, B * Fs + A * DE, F(x)],
                     [B * C, A * E + B * DF, B * DE - A * Fs, F(y)],
                     [-D, C * Fs, C * E, F(z)]], np.float32)


def get_translation_and_euler(t):
    return np.array([t[0, 3], t[1, 3], t[2, 3], atan2f(t[2, 1], t[2, 2]), asinf(-t[2, 0]), atan2f(t[1, 0], t[0, 0])],
                    np.float32)


def constraint(T, latest, closest, fitness):
    T = np.ascontiguousarray(T, np.float32).reshape(4, 4)
    latest, closest = np.asarray(latest, np.float32), np.asarray(closest, np.float32)
    c = get_translation_and_euler(T)
    L = get_transformation(c[2], c[0], c[1], c[5], c[3], c[4])
    W = get_transformation(latest[2], latest[0], latest[1], latest[5], latest[3], latest[4])
    R = np.zeros((3, 4), np.float32)
    for i in range(3):
        for j in range(3):
            R[i, j] = (L[i, 0] * W[0, j] + L[i, 1] * W[1, j]) + L[i, 2] * W[2, j]
        R[i, 3] = ((L[i, 0] * W[0, 3] + L[i, 1] * W[1, 3]) + L[i, 2] * W[2, 3]) + L[i, 3]
    pose_from = get_translation_and_euler(R)
    pose_to = np.array([closest[2], closest[0], closest[1], closest[5], closest[3], closest[4]], np.float32)
    return pose_from, pose_to, F(fitness)
