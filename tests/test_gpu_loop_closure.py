"""GPU checks of the store's half of the loop closure: llsr_map_set_keyframe_time /
llsr_map_keyframe_times (cloudKeyPoses6D.time, MO:1709) and llsr_map_set_key_poses (correctPoses,
MO:1757-1785). After the corrected poses come back, the next extract of the loop-closure branch
(MO:1099-1151), the global map and the saved maps must be what a fresh store with the corrected
poses gives, bit for bit (tests/_compare.py): the store keeps nothing that was transformed with the
old poses. The scene is small: 12 keyframes on a closed 40 m loop, 200-600 points each."""
import numpy as np
import pytest

import _global_map as G
import oracle_py
from _compare import diff_report
from llsr import LlsrError, LocalMap, loop_candidate, map_config

pytestmark = pytest.mark.gpu
K = 12


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def frames():
    """[(pose6, corner, surf, outlier)]: keyframe K - 1 comes back to keyframe 0; cloud sizes 200-600."""
    rng = np.random.default_rng(1)
    radius = 40.0 / (2 * np.pi)
    out = []
    for k in range(K):
        ang = 2 * np.pi * k / (K - 1)
        pos = np.array([radius * np.cos(ang), radius * np.sin(ang), 0.1 * np.sin(3 * ang)])
        pose = np.concatenate([pos, rng.uniform(-0.15, 0.15, 2), [ang + np.pi / 2]]).astype(np.float32)
        n = int(rng.integers(200, 601))
        cloud = rng.uniform(-6, 6, (n, 4)).astype(np.float32)
        cloud[:, 3] = rng.integers(0, 16, n) + rng.uniform(0, 0.1, n)
        nc, ns = n // 4, n // 2
        out.append((pose, cloud[:nc].copy(), cloud[nc:nc + ns].copy(), cloud[nc + ns:].copy()))
    return out


@pytest.fixture(scope="module")
def corrected(frames):
    """Key poses as a pose-graph update would return them: every pose moved, the last one most."""
    rng = np.random.default_rng(2)
    p = np.array([f[0] for f in frames], np.float32)
    p[:, :3] += rng.normal(0, 0.05, (K, 3)).astype(np.float32)
    p[:, 3:] += rng.normal(0, 0.01, (K, 3)).astype(np.float32)
    p[-1] += np.array([0.2, -0.15, 0.1, 0.01, 0.02, 0.03], np.float32)
    return p


def test_keyframe_times(require_gpu, frames):
    m = LocalMap(0)
    for f in frames[:5]:
        m.add_keyframe(*f)
    assert np.isnan(m.keyframe_times()).all() and len(m.keyframe_times()) == 5
    m.set_keyframe_time(1, 5.0)
    m.set_keyframe_time(4, 82.719)
    t = m.keyframe_times()
    assert t[1] == 5.0 and t[4] == 82.719 and np.isnan(t[[0, 2, 3]]).all()
    # the store's times feed the host-side candidate selection: keyframes without a time never match
    poses4 = np.array([np.append(f[0][:3], k) for k, f in enumerate(frames[:5])], np.float32)
    assert loop_candidate(poses4, t, frames[0][0][:3], 100.0, 15.0) == 1
    for bad in (-1, 5):
        with pytest.raises(LlsrError):
            m.set_keyframe_time(bad, 1.0)
    m.reset()
    assert len(m.keyframe_times()) == 0
    m.close()


def test_set_key_poses_refills_the_queue(require_gpu, frames, corrected):
    """The queue is dropped (MO:1759-1761): the next extract of the loop-closure branch equals the
    first extract of a fresh store with the corrected poses, and later extracts keep following it."""
    mcfg = map_config("hdl64e", surrounding_keyframe_search_num=5)
    m = LocalMap(0, mcfg)
    for f in frames[:K - 1]:
        m.add_keyframe(*f)
    pos = frames[-1][0][:3]
    m.extract(pos)
    assert m.keyframe_ids().tolist() == list(range(K - 6, K - 1))
    m.set_key_poses(corrected[:K - 1])
    assert m.keyframe_ids().tolist() == []
    fresh = oracle_py.OracleMap(loop_closure=True, search_num=5)
    for f, p in zip(frames[:K - 1], corrected):
        fresh.add_keyframe(p, *f[1:])
    errs = []
    for step in range(2):  # the refill, then one pop-oldest / push-newest with a new keyframe
        if step:
            m.add_keyframe(corrected[K - 1], *frames[K - 1][1:])
            fresh.add_keyframe(corrected[K - 1], *frames[K - 1][1:])
        gc, gs, rep = m.extract(pos)
        ec, es, ids, _ = fresh.extract(pos)
        assert m.keyframe_ids().tolist() == ids.tolist() and rep["n_transformed"] == (1 if step else 5)
        errs += [diff_report(f"extract {step} corner", _np(gc), ec), diff_report(f"extract {step} surf", _np(gs), es)]
    m.close()
    errs = [e for e in errs if e]
    assert not errs, "\n".join(errs)


def test_set_key_poses_reaches_every_map_product(require_gpu, frames, corrected):
    """The radius branch, the global map and the saved maps read the new poses; a prefix may be set."""
    m, o = LocalMap(0), G.GlobalMapOracle()
    for f in frames:
        m.add_keyframe(*f)
    m.extract(frames[0][0][:3])
    m.set_key_poses(corrected[:7])  # a prefix: keyframes 7.. keep their poses
    poses = np.concatenate([corrected[:7], np.array([f[0] for f in frames[7:]], np.float32)])
    ref = oracle_py.OracleMap()
    for f, p in zip(frames, poses):
        o.add_keyframe(p, *f[1:])
        ref.add_keyframe(p, *f[1:])
    pos = poses[3, :3]
    gc, gs, _ = m.extract(pos)
    ec, es, ids, _ = ref.extract(pos)
    assert m.keyframe_ids().tolist() == ids.tolist()
    errs = [diff_report("radius corner", _np(gc), ec), diff_report("radius surf", _np(gs), es)]
    got, exp = m.global_map(pos), o.global_map(pos)
    errs += [diff_report(k, _np(got[k]), exp[k]) for k in ("global", "edge", "planar")]
    (c, s), (ec, es) = m.save_map(), o.save_map()
    errs += [diff_report("save corner", _np(c), ec), diff_report("save surf", _np(s), es)]
    with pytest.raises(LlsrError):
        m.set_key_poses(np.zeros((K + 1, 6), np.float32))
    m.set_key_poses(np.zeros((0, 6), np.float32))
    m.close()
    errs = [e for e in errs if e]
    assert not errs, "\n".join(errs)
