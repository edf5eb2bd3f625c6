"""An independent numpy float64 restatement of the pose-graph optimiser's specification (DESIGN.md
§19): the same pose conversion, chart, noise, measurements and stop rule, but dense normal equations
solved by numpy.linalg.solve and the C library's trigonometry. It shares no code with csrc/llsr_pg.h.
`reverse=True` sums the factors into the normal equations and into the error in reversed order: the
difference between the two orders is this restatement's own rounding spread."""
import numpy as np

PRIOR_VAR = np.array([1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6])  # MO:1618, [rotation, translation]
STATES = ("clean", "absolute_tol", "relative_tol", "iterations", "error_rose", "failed")


def rzryrx(a, b, c):
    """Rot3::RzRyRx(a, b, c) = Rz(c) Ry(b) Rx(a)."""
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return rz @ ry @ rx


def from_gtsam6(g):
    g = np.asarray(g, np.float32).astype(np.float64)
    return rzryrx(g[3], g[4], g[5]), g[:3].copy()


def store_to_gtsam6(s):
    s = np.asarray(s, np.float32)
    return np.array([s[2], s[0], s[1], s[5], s[3], s[4]], np.float32)


def from_store6(s):
    return from_gtsam6(store_to_gtsam6(s))


def to_store6(T):
    """x, y, z, roll, pitch, yaw in double (the library narrows to float)."""
    R, t = T
    a = np.arctan2(R[2, 1], R[2, 2])
    b = np.arctan2(-R[2, 0], np.hypot(R[2, 1], R[2, 2]))
    c = np.arctan2(R[1, 0], R[0, 0])
    return np.array([t[1], t[2], t[0], b, c, a])


def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def so3_exp(w):
    t = np.linalg.norm(w)
    W = hat(w)
    if t < 1e-4:
        return np.eye(3) + (1 - t * t / 6) * W + (0.5 - t * t / 24) * (W @ W)
    return np.eye(3) + np.sin(t) / t * W + (1 - np.cos(t)) / (t * t) * (W @ W)


def so3_log(R):
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.linalg.norm(v), 0.5 * (np.trace(R) - 1)
    t = np.arctan2(s, c)
    if s < 1e-5:
        return 0.5 * (1 + t * t / 6) * v  # (the tests never come near pi)
    return t / (2 * s) * v


def jr_inv(w):
    t = np.linalg.norm(w)
    W = hat(w)
    g = 1 / 12 + t * t / 720 if t < 1e-3 else 1 / (t * t) - (1 + np.cos(t)) / (2 * t * np.sin(t))
    return np.eye(3) + 0.5 * W + g * (W @ W)


def between(Ti, Tj):
    return Ti[0].T @ Tj[0], Ti[0].T @ (Tj[1] - Ti[1])


def retract(T, d):
    return T[0] @ so3_exp(d[:3]), T[1] + T[0] @ d[3:]


def error(Z, H):
    return np.concatenate([so3_log(Z[0].T @ H[0]), Z[0].T @ (H[1] - Z[1])])


class Graph:
    def __init__(self):
        self.X, self.factors, self.loops = [], [], []  # factors: (i or None, j, Z, 1 / sigma)

    def append(self, poses6):
        for s in np.asarray(poses6, np.float32).reshape(-1, 6):
            T = from_store6(s)
            if not self.X:
                self.factors.append((None, 0, T, 1 / np.sqrt(PRIOR_VAR)))
            else:
                k = len(self.X)
                self.factors.append((k - 1, k, between(self.X[-1], T), 1 / np.sqrt(PRIOR_VAR)))
            self.X.append(T)

    def add_loop(self, frm, to, pose_from6, pose_to6, variance):
        Z = between(from_gtsam6(pose_from6), from_gtsam6(pose_to6))
        self.loops.append((frm, to, Z, np.full(6, 1 / np.sqrt(np.float64(np.float32(variance))))))

    def _all(self, reverse):
        f = self.factors + self.loops  # prior, odometry, loops by insertion
        return f[::-1] if reverse else f

    def loop_residual(self, X=None, l=0):
        X = self.X if X is None else X
        i, j, Z, _ = self.loops[l]
        return error(Z, between(X[i], X[j]))

    def total_error(self, X, reverse=False):
        e = 0.0
        for i, j, Z, w in self._all(reverse):
            r = error(Z, X[j] if i is None else between(X[i], X[j])) * w
            e = e + 0.5 * float(r @ r)
        return e

    def step(self, X, reverse=False):
        n = 6 * len(X)
        H, b = np.zeros((n, n)), np.zeros(n)
        for i, j, Z, w in self._all(reverse):
            Hm = X[j] if i is None else between(X[i], X[j])
            e = error(Z, Hm)
            E = Z[0].T @ Hm[0]
            Ji = jr_inv(e[:3])
            Aj = np.zeros((6, 6))
            Aj[:3, :3], Aj[3:, 3:] = Ji, E
            blocks = [(j, Aj * w[:, None])]
            if i is not None:
                Ai = np.zeros((6, 6))
                Ai[:3, :3] = -Ji @ Hm[0].T
                Ai[3:, :3] = Z[0].T @ hat(Hm[1])
                Ai[3:, 3:] = -Z[0].T
                blocks.append((i, Ai * w[:, None]))
            r = e * w
            for p, A in blocks:
                b[6 * p:6 * p + 6] -= A.T @ r
                for q, B in blocks:
                    H[6 * p:6 * p + 6, 6 * q:6 * q + 6] += A.T @ B
        d = np.linalg.solve(H, b)
        return [retract(T, d[6 * k:6 * k + 6]) for k, T in enumerate(X)]

    def optimize(self, max_iterations=100, rel_tol=1e-5, abs_tol=1e-5, reverse=False):
        """-> dict(state, iterations, error_before, error_after, X): the library's stop rule."""
        X = list(self.X)
        err0 = err = self.total_error(X, reverse)
        if not self.loops:
            return {"state": 0, "iterations": 0, "error_before": 0.0, "error_after": 0.0, "X": X}
        it, state = 0, 3
        while it < max_iterations:
            Xn = self.step(X, reverse)
            new = self.total_error(Xn, reverse)
            it += 1
            if not new <= err:
                state = 4
                break
            dec, old = err - new, err
            X, err = Xn, new
            if dec < abs_tol:
                state = 1
                break
            if dec / old < rel_tol:
                state = 2
                break
        return {"state": state, "iterations": it, "error_before": err0, "error_after": err, "X": X}


def square(K, drift_m=0.0, drift_rad=0.0, size=4.0):
    """K store poses (x, y, z, roll, pitch, yaw; float32) around a size x size square in the store's
    ground plane (z, x) with the heading (the store's pitch) turning once and +-2 degrees of roll / yaw;
    drift_m / drift_rad accumulate per step."""
    out = []
    for k in range(K):
        s = 4 * size * k / K
        side, u = int(s // size), s % size
        gx = (u, size, size - u, 0.0)[side]
        gy = (0.0, u, size, size - u)[side]
        out.append([gy + drift_m * k, 0.02 * np.sin(0.7 * k), gx + 0.5 * drift_m * k,
                    np.radians(2) * np.sin(1.3 * k), 2 * np.pi * k / K + drift_rad * k,
                    np.radians(2) * np.cos(0.9 * k)])
    return np.array(out, np.float32)
