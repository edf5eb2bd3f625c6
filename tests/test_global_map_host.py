"""CPU checks of the global map's host side: llsr_keypose_radius_sorted (publishGlobalMap's sorted
radius search, MO:787-789) against the numpy statement, llsr_global_map_config_default, and the
properties of the expected-side helper the GPU tests compare with (tests/_global_map.py)."""
import numpy as np

import _global_map as G
import llsr


def _poses(seed, n, scale):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = rng.uniform(-scale, scale, (n, 3)).astype(np.float32)
    p[:, 3] = np.arange(n)
    return p


def test_radius_sorted_distinct_distances():
    p = _poses(11, 64, 40.0)
    pos = np.array([1.5, -2.25, 0.75], np.float32)
    d = G.sq_dist(p, pos)
    assert len(np.unique(d)) == 64
    want = G.radius_sorted(p, pos, 35.0)
    assert 0 < len(want) < 64  # the radius cuts the set
    got = llsr.keypose_radius_sorted(p, pos, 35.0)
    assert got.tolist() == want.tolist()
    assert np.all(np.diff(d[got]) > 0)
    assert llsr.keypose_radius_sorted(p, pos, 5000.0).tolist() == np.argsort(d, kind="stable").tolist()


def test_radius_sorted_excludes_the_boundary():
    """d^2 == r^2 exactly (3-4-0 at radius 5) is outside: the test is d^2 < r^2."""
    p = np.array([[3, 4, 0, 0], [0, 0, 4.5, 1], [3, 4, 0.5, 2], [0, 3, 0, 3]], np.float32)
    pos = np.zeros(3, np.float32)
    assert G.sq_dist(p, pos)[0] == np.float32(25.0)
    got = llsr.keypose_radius_sorted(p, pos, 5.0)
    assert got.tolist() == G.radius_sorted(p, pos, 5.0).tolist() == [3, 1]


def test_radius_sorted_ties_in_index_order():
    p = np.array([[5, 0, 0, 0], [0, 2, 0, 1], [1, 0, 0, 2], [0, 0, -2, 3], [-2, 0, 0, 4], [0, 0, 0, 5]], np.float32)
    pos = np.zeros(3, np.float32)
    d = G.sq_dist(p, pos)
    assert d[1] == d[3] == d[4]
    got = llsr.keypose_radius_sorted(p, pos, 100.0)
    assert got.tolist() == G.radius_sorted(p, pos, 100.0).tolist() == [5, 2, 1, 3, 4, 0]


def test_radius_sorted_empty_and_bad_arguments():
    assert llsr.keypose_radius_sorted(np.zeros((0, 4), np.float32), [0, 0, 0], 1.0).tolist() == []
    assert llsr.lib().llsr_keypose_radius_sorted(None, 3, None, 1.0, None) == -22


def test_global_map_config_default():
    c = llsr.global_map_config()
    assert (c.search_radius, c.keypose_leaf, c.cloud_leaf) == (5000.0, 1.0, np.float32(0.4))
    assert (c.high_dense, c.first_call_raw) == (0, 1)
    assert llsr.global_map_config(high_dense=1).high_dense == 1


def _small_oracle(**kw):
    rng = np.random.default_rng(3)
    o = G.GlobalMapOracle(**kw)
    n_out = 0
    for k in range(6):
        pose = np.array([0.3 * k, 0.1 * k, 0.0, 0.01 * k, -0.02 * k, 0.3 * k], np.float32)
        c, s, ol = (rng.uniform(-3, 3, (n, 4)).astype(np.float32) for n in (40, 90, 25))
        o.add_keyframe(pose, c, s, ol)
        n_out += len(ol)
    return o, n_out


def test_helper_first_call_raw_second_downsampled():
    o, n_out = _small_oracle()
    a = o.global_map(np.zeros(3, np.float32))
    ra = a["report"]
    assert (ra["call"], ra["downsampled_poses"], ra["downsampled_cloud"]) == (1, 0, 0)
    assert ra["n_poses_used"] == ra["n_in_radius"] == 6
    assert ra["n_global"] == ra["n_global_raw"] == ra["n_edge"] + ra["n_planar"] + n_out
    # raw, in distance order: the nearest keyframe's corner cloud leads the global cloud
    assert np.array_equal(a["global"][:40], a["edge"][:40])
    b = o.global_map(np.zeros(3, np.float32))
    rb = b["report"]
    assert (rb["call"], rb["downsampled_poses"], rb["downsampled_cloud"], rb["passthrough"]) == (2, 1, 1, 0)
    assert rb["n_poses_used"] < 6 and rb["n_global"] < rb["n_global_raw"]
    assert len(b["edge"]) == rb["n_edge"] == 40 * rb["n_poses_used"]


def test_helper_switches():
    o, _ = _small_oracle(high_dense=1)
    for _ in range(2):
        r = o.global_map(np.zeros(3, np.float32))["report"]
        assert r["downsampled_cloud"] == 0 and r["n_global"] == r["n_global_raw"]
    o, _ = _small_oracle(first_call_raw=0)
    assert o.global_map(np.zeros(3, np.float32))["report"]["downsampled_cloud"] == 1
    e = G.GlobalMapOracle()
    assert e.global_map(np.zeros(3, np.float32))["report"]["call"] == 0 and e.calls == 0


def test_helper_passthrough_when_the_extent_overflows():
    o = G.GlobalMapOracle()
    rng = np.random.default_rng(5)
    for k, xyz in enumerate(([0, 0, 0], [2000, 0, 0], [0, 2000, 0], [1000, 1000, 300])):
        cl = [rng.uniform(-2, 2, (n, 4)).astype(np.float32) for n in (30, 50, 10)]
        o.add_keyframe(np.array(xyz + [0, 0, 0.1 * k], np.float32), *cl)
    o.global_map(np.zeros(3, np.float32))
    b = o.global_map(np.zeros(3, np.float32))
    r = b["report"]
    raw = np.concatenate([c for k in range(4) for c in o.world[k]])
    assert G.extent_product(raw, 0.4) > G.INT32_MAX
    assert r["passthrough"] == 1 and r["downsampled_cloud"] == 1 and r["n_global"] == r["n_global_raw"] == 360
    # key poses lie > 1 m apart: four voxels, nearest first after the VoxelGrid's own order
    assert r["n_poses_used"] == 4
