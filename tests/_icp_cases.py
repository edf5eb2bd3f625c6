"""The alignment cases shared by the CPU and GPU tests of the loop closure's ICP: the smallest shapes
at which the search, the packing, the depth blocks of sigma and the stop rule can go wrong, and the
recovery scene (12 keyframes on a closed 40 m loop over one fixed set of world points, the last pose
moved by a planted drift). Everything is generated from fixed seeds; nothing calls the library."""
import numpy as np

import oracle_py
from _compare import diff_report

DRIFT = np.array([0.2, -0.15, 0.1, 0.01, 0.02, 0.03])  # x, y, z m; roll, pitch, yaw rad


# ---- generic clouds -------------------------------------------------------------------------------
def _xyzi(xyz, intensity=1.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = xyz
    out[:, 3] = intensity
    return out


def _structure(rng, n):
    """n points on a floor, two walls and a ridge inside +-20 m: random, so no lattice to lock on."""
    k = n // 4
    floor = np.stack([rng.uniform(-20, 20, k), rng.uniform(-20, 20, k), np.full(k, -1.5)], 1)
    wall1 = np.stack([np.full(k, 18.0), rng.uniform(-20, 20, k), rng.uniform(-1.5, 6, k)], 1)
    wall2 = np.stack([rng.uniform(-20, 20, k), np.full(k, -17.0), rng.uniform(-1.5, 6, k)], 1)
    m = n - 3 * k
    ridge = np.stack([rng.uniform(-10, 10, m), 0.3 * rng.uniform(-10, 10, m) + 4.0, rng.uniform(0, 3, m)], 1)
    return np.concatenate([floor, wall1, wall2, ridge])


def _rigid(angles, t):
    rx, ry, rz = angles
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    return R, np.asarray(t, np.float64)


def _moved(xyz, angles=(0.004, -0.003, 0.006), t=(0.05, -0.04, 0.03)):
    R, t = _rigid(angles, t)
    return xyz @ R.T + t


def pair_count_case(kept, seed=0):
    """`kept` source points near the target interleaved with points 150 m outside it (never a pair),
    so the packed order differs from the source order."""
    rng = np.random.default_rng(100 + kept + seed)
    tgt = _structure(rng, 3000)
    near = _moved(tgt[rng.choice(len(tgt), kept, replace=False)]) if kept else np.zeros((0, 3))
    n_far = max(4, kept // 12)
    far = np.stack([rng.uniform(170, 175, n_far), rng.uniform(-5, 5, n_far), rng.uniform(0, 2, n_far)], 1)
    src = np.zeros((kept + n_far, 3))
    far_at = np.sort(rng.choice(kept + n_far, n_far, replace=False))
    mask = np.zeros(kept + n_far, bool)
    mask[far_at] = True
    src[mask], src[~mask] = far, near
    return _xyzi(src), _xyzi(tgt)


def ties_case():
    """Integer-lattice targets present twice (two keyframes holding the same coordinates), queries
    midway between lattice points of different cells, and queries on lattice sites that are left out
    of the target: their best d^2 = 1 equals r^2 of shell 1, so the walk goes on to shell 2."""
    g = np.stack(np.meshgrid(np.arange(-3, 4), np.arange(-3, 4), np.arange(0, 4), indexing="ij"), -1).reshape(-1, 3)
    holes = {(0, 0, 1), (2, -1, 2), (-2, 2, 1)}
    lat = np.array([p for p in g.tolist() if tuple(p) not in holes], np.float64)
    tgt = np.concatenate([lat, lat[::-1][:200], lat[50:120]])
    q = [list(h) for h in sorted(holes)]
    q += [[0.5, 1, 1], [1, -1.5, 2], [-2, 0, 1.5], [0.5, 0.5, 1], [1.5, -0.5, 2.5], [-0.5, 2.5, 0.5], [-1.5, -1.5, 1.5]]
    rng = np.random.default_rng(7)
    q += (lat[rng.choice(len(lat), 40, replace=False)] + rng.uniform(-0.2, 0.2, (40, 3))).tolist()
    return _xyzi(q), _xyzi(tgt)


def shell_case():
    """A gappy target, a query 80 m outside its box and queries in empty cells inside it."""
    rng = np.random.default_rng(11)
    tgt = np.concatenate([_structure(rng, 400), [[-20, -20, -1.5], [20, 20, 6.0]]])
    src = _moved(tgt[rng.choice(400, 60, replace=False)])
    extra = np.array([[100.0, 0.5, 0.5], [0.5, 0.5, 4.5], [-12.5, 9.5, 5.5], [3.5, -3.5, 3.5], [0.5, -97.0, 2.0]])
    return _xyzi(np.concatenate([src[:30], extra, src[30:]])), _xyzi(tgt)


def one_cell_case():
    rng = np.random.default_rng(12)
    tgt = rng.uniform(0.1, 0.9, (7, 3)) + np.array([4.0, -3.0, 1.0])
    src = np.concatenate([_moved(tgt), rng.uniform(-6, 6, (9, 3)) + np.array([4.0, -3.0, 1.0])])
    return _xyzi(src), _xyzi(tgt)


def sparse_box_case():
    """40 targets in a 60 x 60 x 12 m box: almost every cell of every shell is empty."""
    rng = np.random.default_rng(13)
    tgt = np.stack([rng.uniform(-30, 30, 40), rng.uniform(-30, 30, 40), rng.uniform(-2, 10, 40)], 1)
    src = np.concatenate([_moved(tgt[:25]), np.stack([rng.uniform(-30, 30, 12), rng.uniform(-30, 30, 12),
                                                      rng.uniform(-2, 10, 12)], 1)])
    return _xyzi(src), _xyzi(tgt)


def odd_points_case():
    """A NaN coordinate and a point at 2e6 m in the source (and one of each in the target): dropped
    from the pairs and from the fitness mean."""
    rng = np.random.default_rng(14)
    tgt = _structure(rng, 600)
    src = _moved(tgt[rng.choice(600, 80, replace=False)])
    src = np.concatenate([src[:20], [[np.nan, 1.0, 2.0]], src[20:50], [[3.0, 2.0e6, 1.0]], src[50:]])
    tgt = np.concatenate([tgt[:100], [[1.0, np.nan, 0.0]], tgt[100:], [[-2.0e6, 0.0, 0.0]]])
    return _xyzi(src), _xyzi(tgt)


def subset_case():
    """The source is a subset of the target: the first estimate is (nearly) the identity."""
    rng = np.random.default_rng(15)
    tgt = _structure(rng, 900)
    return _xyzi(tgt[rng.choice(900, 300, replace=False)]), _xyzi(tgt)


# ---- the recovery scene -----------------------------------------------------------------------------
def pose_matrix(pose6):
    """transformPointCloud of a key pose (x, y, z, roll, pitch, yaw) as a float64 3x4: yaw about z, roll
    about x, pitch about y, then the translation."""
    x, y, z, roll, pitch, yaw = [float(v) for v in pose6]
    cy, sy, cr, sr, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    return np.concatenate([Ry @ Rx @ Rz, np.array([[x], [y], [z]])], 1)


class Scene:
    """12 keyframes on a closed 40 m loop; keyframe k holds the world points j with (j + k) % 5 != 0 in
    its own frame (edges as its corner cloud, planes as its surf cloud), so keyframes 0, 1 and 2
    together hold every point the last keyframe holds. `poses` carries the planted drift on the last
    pose, `true_poses` does not; times are 5 s apart."""

    K = 12

    def __init__(self):
        rng = np.random.default_rng(2024)
        planes = _structure(rng, 520)
        e = 24
        edges = np.concatenate([np.stack([np.full(e, x), np.full(e, y), np.linspace(-1.5, 5.4, e)], 1)
                                for x, y in ((9.3, 7.1), (-8.2, 11.4), (-11.7, -6.3), (7.6, -12.9))])
        edges = edges + rng.uniform(-0.03, 0.03, edges.shape)
        self.world = np.concatenate([edges, planes])
        self.n_edges = len(edges)
        radius = 40.0 / (2 * np.pi)
        self.true_poses = np.zeros((self.K, 6), np.float32)
        for k in range(self.K):
            a = 2 * np.pi * k / self.K
            self.true_poses[k] = [radius * np.cos(a), radius * np.sin(a), 0.1 * np.sin(2 * a), 0.01 * np.cos(a),
                                  0.02 * np.sin(a), a + np.pi / 2]
        self.poses = self.true_poses.copy()
        self.poses[-1] = (self.true_poses[-1].astype(np.float64) + DRIFT).astype(np.float32)
        self.times = 5.0 * np.arange(self.K)
        self.now = float(self.times[-1])
        self.frames = []
        for k in range(self.K):
            M = pose_matrix(self.true_poses[k])
            own = (self.world - M[:, 3]) @ M[:, :3]  # R^T (p - t)
            see = (np.arange(len(self.world)) + k) % 5 != 0
            corner = _xyzi(own[:self.n_edges][see[:self.n_edges]], 10 + k)
            surf = _xyzi(own[self.n_edges:][see[self.n_edges:]], 20 + k)
            outlier = _xyzi(own[self.n_edges::40] + 0.5, 30 + k)
            self.frames.append((corner, surf, outlier))

    def cloud(self, k, poses=None):
        """Keyframe k's corner then surf cloud through the oracle's transformPointCloud."""
        p = (self.poses if poses is None else poses)[k]
        c, s, _ = self.frames[k]
        return np.concatenate([oracle_py.transform_keyframe(p, c), oracle_py.transform_keyframe(p, s)])

    def submaps(self, closest, num, poses=None):
        """performLoopClosure's raw clouds: the latest keyframe, and keyframes closest - num .. closest + num."""
        ids = [closest + j for j in range(-num, num + 1) if 0 <= closest + j < self.K]
        return self.cloud(self.K - 1, poses), np.concatenate([self.cloud(k, poses) for k in ids])

    def corrected(self, T):
        """T applied to the drifted last pose, and the true one, as float64 3x4 matrices."""
        W = np.concatenate([pose_matrix(self.poses[-1]), [[0, 0, 0, 1]]])
        return (np.asarray(T, np.float64).reshape(4, 4) @ W)[:3], pose_matrix(self.true_poses[-1])


_SCENE = None


def scene():
    global _SCENE
    if _SCENE is None:
        _SCENE = Scene()
    return _SCENE


def recovery_case():
    return scene().submaps(0, 2)


def noisy_recovery_case():
    s, t = scene().submaps(0, 2)
    s = s.copy()
    s[:, :3] += np.random.default_rng(77).normal(0, 0.02, (len(s), 3)).astype(np.float32)
    return s, t


# name -> (builder, config overrides, expected final state or None)
CASES = {
    "pairs_0": (lambda: pair_count_case(0), {}, "no_correspondences"),
    "pairs_2": (lambda: pair_count_case(2), {}, "no_correspondences"),
    "pairs_3": (lambda: pair_count_case(3), {}, None),
    "pairs_5": (lambda: pair_count_case(5), {}, None),
    "pairs_680": (lambda: pair_count_case(680), {}, None),
    "pairs_681": (lambda: pair_count_case(681), {}, None),
    "pairs_1360": (lambda: pair_count_case(1360), {}, None),
    "pairs_1361": (lambda: pair_count_case(1361), {}, None),
    "ties": (ties_case, {}, None),
    "shells": (shell_case, {}, None),
    "one_cell": (one_cell_case, {}, None),
    "sparse_box": (sparse_box_case, {}, None),
    "odd_points": (odd_points_case, {}, None),
    "max_iterations_3": (lambda: pair_count_case(200, seed=5), {"icp_max_iterations": 3}, "iterations"),
    "subset": (subset_case, {}, "transform"),
    "recovery": (recovery_case, {}, None),
    # the transformation test switched off (a negative epsilon never passes), so the loop runs on to the
    # MSE tests: the recovery scene with 2 cm of noise on the source settles to a constant residual
    # (relative MSE); a source that is a subset of the target repeats an MSE of ~0 (absolute MSE)
    "recovery_rel_mse": (noisy_recovery_case, {"icp_transformation_epsilon": -1.0}, "rel_mse"),
    "subset_abs_mse": (subset_case, {"icp_transformation_epsilon": -1.0}, "abs_mse"),
    "empty_target": (lambda: (pair_count_case(5)[0], np.zeros((0, 4), np.float32)), {}, "no_correspondences"),
    "empty_source": (lambda: (np.zeros((0, 4), np.float32), pair_count_case(5)[1]), {}, "no_correspondences"),
}
KEPT = {"pairs_0": 0, "pairs_2": 2, "pairs_3": 3, "pairs_5": 5, "pairs_680": 680, "pairs_681": 681,
        "pairs_1360": 1360, "pairs_1361": 1361}

_BUILT = {}


def get(name):
    """(src, tgt, overrides, expected state) of a case, built once."""
    if name not in _BUILT:
        b, over, want = CASES[name]
        s, t = b()
        s.setflags(write=False)
        t.setflags(write=False)
        _BUILT[name] = (s, t, over, want)
    return _BUILT[name]


_EXPECTED = {}


def expected(name):
    """The restatement's result of a case (tests/_icp_loop.py), computed once."""
    import _icp_loop
    if name not in _EXPECTED:
        s, t, over, _ = get(name)
        kw = {"max_iterations": over.get("icp_max_iterations", 100),
              "eps_t": over.get("icp_transformation_epsilon", 1e-6)}
        _EXPECTED[name] = _icp_loop.icp(s, t, **kw)
    return _EXPECTED[name]


def check_result(got, want, name):
    """Every field of an alignment result against the restatement's, bit for bit."""
    errs = []
    for k in ("iterations", "state", "converged", "n_pairs_last"):
        if int(got[k]) != int(want[k]):
            errs.append(f"{k}: {got[k]} != {want[k]}")
    if np.float64(got["fitness"]).view(np.uint64) != np.float64(want["fitness"]).view(np.uint64):
        errs.append(f"fitness: {got['fitness']!r} != {want['fitness']!r}")
    for k in ("T", "aligned"):
        r = diff_report(k, np.ascontiguousarray(got[k], np.float32), np.ascontiguousarray(want[k], np.float32))
        if r:
            errs.append(r)
    assert not errs, (name, errs)
