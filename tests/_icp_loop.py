"""The expected side of the loop closure's alignment: pcl::IterativeClosestPoint with an identity
guess as DESIGN.md §16 specifies it ("ICP loop", "Correspondences", "Estimate", "Point transform",
"Stop rule", "Fitness"), restated from that section and not from the library's code, in numpy float32
(one rounding per operation, no FMA) and Python floats (IEEE double). It never calls the library.

The nearest neighbour is a brute-force search over all targets with §16's d^2 and the lowest target
index among equal d^2 (np.argmin returns the first minimum), so it knows nothing of cells or shells.
The estimate and the pose constraint are the ones of _loop_closure.py."""
import numpy as np

from _loop_closure import F, ONE, constraint, seq_sum, umeyama  # noqa: F401  (constraint: re-exported)

STATES = ("none", "iterations", "transform", "abs_mse", "rel_mse", "no_correspondences")
NONE, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
DBL_MAX = float(np.finfo(np.float64).max)
CELL_LIMIT = F(1048000.0)


def in_grid(xyz):
    """Points every coordinate of which has floor() strictly inside +-1 048 000 (NaN: outside)."""
    with np.errstate(invalid="ignore"):
        f = np.floor(np.asarray(xyz, np.float32))
        return np.all((f > -CELL_LIMIT) & (f < CELL_LIMIT), axis=1)


def nearest(q, tgt):
    """(index, d^2) of the nearest target of every query, index -1 where there is none."""
    q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
    idx = np.full(len(q), -1, np.int64)
    d2 = np.zeros(len(q), np.float32)
    ok_t = in_grid(t)
    ok_q = in_grid(q)
    if not ok_t.any():
        return idx, d2
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(0, len(q), 256):
            c = q[b:b + 256]
            dx = t[None, :, 0] - c[:, None, 0]
            dy = t[None, :, 1] - c[:, None, 1]
            dz = t[None, :, 2] - c[:, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
            d[:, ~ok_t] = np.inf
            k = np.argmin(d, axis=1)
            idx[b:b + 256] = k
            d2[b:b + 256] = d[np.arange(len(c)), k]
    idx[~ok_q] = -1
    d2[~ok_q] = 0
    return idx, d2


def transform(M, xyz):
    M = np.asarray(M, np.float32)
    p = np.asarray(xyz, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)], axis=1)


def mul4(A, B):
    """A * B, each coefficient summed left to right over k."""
    R = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            R[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return R


def icp(src4, tgt4, max_iterations=100, eps_t=1e-6, eps_f=1e-6, max_dist=100.0):
    src4 = np.ascontiguousarray(src4, np.float32).reshape(-1, 4)
    tgt4 = np.ascontiguousarray(tgt4, np.float32).reshape(-1, 4)
    tgt = tgt4[:, :3]
    work = src4[:, :3].copy()
    final = np.eye(4, dtype=np.float32)
    iterations, state, converged, prev, n_pairs = 0, NONE, False, DBL_MAX, 0
    while state == NONE:
        idx, d2 = nearest(work, tgt)
        keep = (idx >= 0) & ~(d2.astype(np.float64) > max_dist * max_dist)
        n_pairs = int(keep.sum())
        if n_pairs < 3:
            state, converged = NO_CORRESPONDENCES, False
            break
        T = umeyama(work[keep], tgt[idx[keep]])
        work = transform(T, work)
        final = mul4(T, final)
        iterations += 1
        if iterations >= max_iterations:
            state, converged = ITERATIONS, True
            break
        cos = 0.5 * (((float(T[0, 0]) + float(T[1, 1])) + float(T[2, 2])) - 1.0)
        tx, ty, tz = float(T[0, 3]), float(T[1, 3]), float(T[2, 3])
        if cos >= 1.0 - eps_t and (tx * tx + ty * ty) + tz * tz <= eps_t:
            state, converged = TRANSFORM, True
            break
        mse = float(seq_sum(d2[keep], np.float64)) / n_pairs
        if abs(mse - prev) < 1e-12:
            state, converged = ABS_MSE, True
            break
        with np.errstate(divide="ignore", invalid="ignore"):  # IEEE: a previous mse of 0 gives inf or NaN
            rel = float(np.float64(abs(mse - prev)) / np.float64(prev))
        if rel < eps_f:
            state, converged = REL_MSE, True
            break
        prev = mse
    aligned = src4.copy()
    aligned[:, :3] = transform(final, src4[:, :3])
    idx, d2 = nearest(aligned[:, :3], tgt)
    n_fit = int((idx >= 0).sum())
    fitness = float(seq_sum(d2[idx >= 0], np.float64)) / n_fit if n_fit else DBL_MAX
    return {"T": final, "iterations": iterations, "state": state, "converged": converged, "n_pairs_last": n_pairs,
            "fitness": fitness, "aligned": aligned}
