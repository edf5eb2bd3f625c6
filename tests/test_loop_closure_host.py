"""CPU checks of the loop closure's host side (no device): llsr_umeyama3, llsr_loop_candidate,
llsr_loop_constraint and llsr_loop_config_lidar against the restatement of DESIGN.md §16 in
tests/_loop_closure.py, bit for bit, and llsr_umeyama3 against a float64 Kabsch solve."""
import numpy as np
import pytest

import _loop_closure as L
import llsr

# the depth-block edges of gemm_kc(n, 3, 3): one block up to 680, two from 681, three from 1361
EDGE_N = (3, 13, 14, 679, 680, 681, 1361)
# max |R - R64| and max |t - t64| of llsr_umeyama3 against float64 Kabsch measured on the CPU over
# _conditioned_sets: 1.04e-6 and 2.99e-4 (the translation carries the rounding of
# sequential float sums of up to 3000 coordinates around 100 m); the bounds are 4x that
R_BOUND, T_BOUND = 4.16e-6, 1.2e-3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rotation(rng, reflect=False):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if (np.linalg.det(q) < 0) != reflect:
        q[:, 0] = -q[:, 0]
    return q


def _random_sets():
    """10000 correspondence sets: mostly small, every depth-block edge, planar / collinear sources,
    reflected destinations (S = -1), noisy and exact ones."""
    rng = np.random.default_rng(20240318)
    sizes = list(EDGE_N) + [int(n) for n in rng.integers(3, 48, 10000 - len(EDGE_N))]
    for i, n in enumerate(sizes):
        kind = i % 8
        s = rng.normal(0.0, rng.uniform(0.1, 30.0), (n, 3))
        if kind == 1:
            s[:, 2] = 0.0                                    # coplanar
        elif kind == 2:
            s = np.outer(rng.normal(0, 5, n), rng.normal(size=3))  # collinear
        elif kind == 3:
            s[:, 1] = 0.25 * s[:, 0]                        # coplanar, oblique
        R = _rotation(rng, reflect=(kind == 4))
        d = s @ R.T + rng.uniform(-50, 50, 3)
        if kind in (5, 6):
            d = d + rng.normal(0, 0.05, d.shape)
        if kind == 7:
            s = s + rng.uniform(-200, 200, 3)                # far from the origin
        yield i, kind, s.astype(np.float32), d.astype(np.float32)


def test_umeyama_bit_equal_to_the_restatement():
    bad, reflected = [], 0
    seen_n = set()
    for i, kind, s, d in _random_sets():
        got, want = llsr.umeyama3(s, d), L.umeyama(s, d)
        seen_n.add(len(s))
        if kind == 4:
            # a reflected destination takes S = -1: the rotation part still has determinant +1
            reflected += int(np.linalg.det(got[:3, :3].astype(np.float64)) > 0.99)
        if not np.array_equal(_bits(got), _bits(want)):
            bad.append((i, kind, len(s), float(np.abs(got - want).max())))
    assert set(EDGE_N) <= seen_n
    assert reflected > 1000
    assert not bad, bad[:10]


def _conditioned_sets(count=400):
    """Sets with (sigma_2 + sigma_3) / sigma_1 >= 0.1 of the cross-covariance, sizes over the block edges."""
    rng = np.random.default_rng(7)
    out = []
    sizes = list(EDGE_N[1:]) + [int(n) for n in rng.integers(6, 3000, 4 * count)]
    for n in sizes:
        s = rng.normal(0.0, 1.0, (n, 3)) * rng.uniform(0.5, 20.0, 3) + rng.uniform(-100, 100, 3)
        d = s @ _rotation(rng).T + rng.uniform(-100, 100, 3) + rng.normal(0, 0.02, (n, 3))
        s32, d32 = s.astype(np.float32), d.astype(np.float32)
        s64, d64 = s32.astype(np.float64), d32.astype(np.float64)
        sv = np.linalg.svd((d64 - d64.mean(0)).T @ (s64 - s64.mean(0)) / n, compute_uv=False)
        if (sv[1] + sv[2]) / sv[0] >= 0.1:
            out.append((s32, d32))
        if len(out) == count:
            break
    assert len(out) == count
    return out


def _kabsch64(s, d):
    s, d = s.astype(np.float64), d.astype(np.float64)
    sm, dm = s.mean(0), d.mean(0)
    U, _, Vt = np.linalg.svd((d - dm).T @ (s - sm) / len(s))
    S = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = U @ S @ Vt
    return R, dm - R @ sm


def test_umeyama_against_float64_kabsch():
    worst_r = worst_t = 0.0
    for s, d in _conditioned_sets():
        T = llsr.umeyama3(s, d).astype(np.float64)
        R, t = T[:3, :3], T[:3, 3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(R) - 1.0) < 1e-5
        assert np.array_equal(T[3], [0, 0, 0, 1])
        R64, t64 = _kabsch64(s, d)
        worst_r = max(worst_r, float(np.abs(R - R64).max()))
        worst_t = max(worst_t, float(np.abs(t - t64).max()))
    print(f"umeyama vs float64 Kabsch: max|R - R64| = {worst_r:.3g}, max|t - t64| = {worst_t:.3g}")
    assert worst_r <= R_BOUND and worst_t <= T_BOUND


def test_umeyama_bad_arguments():
    assert llsr.lib().llsr_umeyama3(None, None, 3, None) == -22
    z = np.zeros((1, 3), np.float32)
    assert llsr.lib().llsr_umeyama3(z.ctypes.data, z.ctypes.data, 0, z.ctypes.data) == -22


def _poses(rng, n, scale):
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = rng.uniform(-scale, scale, (n, 3)).astype(np.float32)
    p[:, 3] = np.arange(n)
    return p


def test_candidate_random_against_the_restatement():
    rng = np.random.default_rng(5)
    hits = misses = 0
    for _ in range(300):
        K = int(rng.integers(1, 60))
        p = _poses(rng, K, 40.0)
        times = np.cumsum(rng.uniform(0.5, 6.0, K))
        times[rng.random(K) < 0.1] = np.nan
        pos = rng.uniform(-40, 40, 3).astype(np.float32)
        now = float(times[np.isfinite(times)].max()) if np.isfinite(times).any() else 0.0
        radius = float(rng.uniform(5, 60))
        want = L.candidate(p, times, pos, now, radius, 30.0)
        assert llsr.loop_candidate(p, times, pos, now, radius, 30.0) == want
        hits += want >= 0
        misses += want < 0
    assert hits > 50 and misses > 50


def test_candidate_ties_nan_and_time_gap():
    pos = np.zeros(3, np.float32)
    # poses 1, 3, 4 are equally far (d^2 = 4): ascending index decides; pose 0 is nearer but recent
    p = np.array([[1, 0, 0, 0], [0, 2, 0, 1], [9, 0, 0, 2], [0, 0, -2, 3], [-2, 0, 0, 4]], np.float32)
    d = L.sq_dist(p, pos)
    assert d[1] == d[3] == d[4]
    now = 100.0
    assert llsr.loop_candidate(p, [99.0, 10.0, 10.0, 10.0, 10.0], pos, now, 5.0) == 1 == \
        L.candidate(p, [99.0, 10.0, 10.0, 10.0, 10.0], pos, now, 5.0)
    # the first tied pose is recent, the second has no time: the third wins
    t = [99.0, 80.0, 10.0, float("nan"), 10.0]
    assert llsr.loop_candidate(p, t, pos, now, 5.0) == 4 == L.candidate(p, t, pos, now, 5.0)
    # a future time counts too (fabs)
    t = [99.0, 140.0, 10.0, 10.0, 10.0]
    assert llsr.loop_candidate(p, t, pos, now, 5.0) == 1 == L.candidate(p, t, pos, now, 5.0)
    # exactly the gap is not enough; hits only inside the gap; no hit in the radius; a NaN-only store
    assert llsr.loop_candidate(p, [70.0] * 5, pos, now, 5.0) == -1 == L.candidate(p, [70.0] * 5, pos, now, 5.0)
    assert llsr.loop_candidate(p, [95.0] * 5, pos, now, 5.0) == -1
    assert llsr.loop_candidate(p, [10.0] * 5, pos, now, 0.5) == -1 == L.candidate(p, [10.0] * 5, pos, now, 0.5)
    assert llsr.loop_candidate(p, [float("nan")] * 5, pos, now, 50.0) == -1
    # pose 2 (d = 9) is outside radius 5 even though it is old
    assert llsr.loop_candidate(p, [99.0, 99.0, 10.0, 99.0, 99.0], pos, now, 5.0) == -1
    assert llsr.loop_candidate(np.zeros((0, 4), np.float32), [], pos, now, 5.0) == -1
    assert llsr.lib().llsr_loop_candidate(None, None, 3, None, 0.0, 1.0, 30.0) == -22


def _pose_matrix(rng, angles=None):
    a = rng.uniform(-3.1, 3.1, 3) if angles is None else angles
    t = L.get_transformation(*rng.uniform(-20, 20, 3).astype(np.float32), *np.asarray(a, np.float32))
    return np.concatenate([t, np.array([[0, 0, 0, 1]], np.float32)])


def test_constraint_bit_equal_to_the_restatement():
    rng = np.random.default_rng(11)
    cases = [(_pose_matrix(rng), rng.uniform(-3, 3, 6).astype(np.float32), rng.uniform(-3, 3, 6).astype(np.float32))
             for _ in range(500)]
    half_pi = np.float32(np.pi / 2)
    for sign in (1.0, -1.0):
        for eps in (0.0, 1e-7, 1e-4, 1e-3, -1e-4):
            # pitch of the ICP transformation and of the key pose near +-pi/2
            T = _pose_matrix(rng, (0.3, sign * (half_pi - np.float32(eps)), -1.2))
            latest = np.array([1.0, -2.0, 0.5, 0.2, sign * (float(half_pi) - eps), 0.7], np.float32)
            cases.append((T, latest, rng.uniform(-3, 3, 6).astype(np.float32)))
    for T, latest, closest in cases:
        fitness = float(rng.uniform(0, 2))
        got = llsr.loop_constraint(T, latest, closest, fitness)
        want = L.constraint(T, latest, closest, fitness)
        for g, w, name in zip(got, want, ("pose_from", "pose_to", "variance")):
            assert np.array_equal(_bits(g), _bits(w)), (name, g, w)
    # identity correction: pose_from is the latest key pose in the lidar order, up to float rounding
    pf, pt, var = llsr.loop_constraint(np.eye(4, dtype=np.float32), [1, 2, 3, 0.1, 0.2, 0.3], [4, 5, 6, 0.4, 0.5, 0.6], 0.25)
    assert np.allclose(pf, [3, 1, 2, 0.3, 0.1, 0.2], atol=1e-6)
    assert pt.tolist() == [np.float32(v) for v in (6, 4, 5, 0.6, 0.4, 0.5)] and var == 0.25


@pytest.mark.parametrize("lidar,radius,num,score", [("vlp16", 15.0, 50, 0.5), ("vlp32c", 50.0, 40, 1.5),
                                                    ("hdl64e", 30.0, 30, 0.8)])
def test_loop_config_blocks(lidar, radius, num, score):
    c = llsr.loop_config(lidar)
    assert (c.search_radius, c.search_num, c.fitness_score) == (radius, num, np.float32(score))
    assert (c.leaf, c.min_time_gap, c.icp_max_iterations) == (np.float32(0.2), 30.0, 100)
    assert (c.icp_transformation_epsilon, c.icp_fitness_epsilon, c.icp_max_correspondence_distance) == (1e-6, 1e-6, 100.0)
    assert llsr.loop_config(lidar, search_num=2).search_num == 2


def test_restatement_svd_reconstructs():
    """The restated SVD is a singular value decomposition (float64 check of the float32 factors)."""
    rng = np.random.default_rng(2)
    for k in range(200):
        A = rng.normal(0, 10.0 ** rng.uniform(-3, 3), (3, 3)).astype(np.float32)
        if k % 4 == 0:
            A[2] = A[0] + A[1]  # rank 2
        U, sv, V = L.svd3(A)
        U, sv, V = U.astype(np.float64), sv.astype(np.float64), V.astype(np.float64)
        scale = max(float(np.abs(A).max()), 1e-30)
        assert np.abs(U @ np.diag(sv) @ V.T - A).max() <= 2e-5 * scale
        assert np.abs(U.T @ U - np.eye(3)).max() < 1e-5 and np.abs(V.T @ V - np.eye(3)).max() < 1e-5
        assert sv[0] >= sv[1] >= sv[2] >= 0
