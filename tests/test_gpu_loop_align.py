"""GPU: the loop closure on the keyframe store — llsr_map_loop_submaps (candidate, the two submaps,
the intensity filter, the VoxelGrid) against a numpy assembly from the frames with the oracle's
transformPointCloud and VoxelGrid, and llsr_map_loop_closure (submaps, llsr_icp_align, acceptance,
constraint) against the restatement of DESIGN.md §16 (tests/_icp_loop.py, tests/_loop_closure.py),
bit for bit (tests/_compare.py). The scene is tests/_icp_cases.py's: 12 keyframes on a closed 40 m
loop over shared world points, the last pose moved by a planted drift."""
import ctypes as C

import numpy as np
import pytest

import _global_map as G
import _icp_cases as K
import _icp_loop as R
import _loop_closure as L
import oracle_py
from _compare import diff_report
from llsr import LocalMap, _abi, lib, loop_config, map_config

pytestmark = pytest.mark.gpu
NUM = 2  # history_keyframe_search_num of these tests: a 5-keyframe window


def _np(t):
    return t.detach().cpu().numpy()


def _cfg(**kw):
    return loop_config("hdl64e", search_num=NUM, search_radius=8.0, **kw)


def _store(frames, poses, times):
    m = LocalMap(0, map_config("hdl64e"))
    for k, (f, p) in enumerate(zip(frames, poses)):
        m.add_keyframe(p, *f)
        if times is not None:
            m.set_keyframe_time(k, float(times[k]))
    return m


def _world(pose, cloud):
    return oracle_py.transform_keyframe(pose, cloud) if len(cloud) else G.EMPTY


def _expected_submaps(frames, poses, closest, leaf=0.2):
    """§16 "Candidate and submaps" steps 3-5 in numpy from the frames."""
    n = len(frames)
    raw = np.concatenate([_world(poses[n - 1], frames[n - 1][0]), _world(poses[n - 1], frames[n - 1][1])])
    w = raw[:, 3]
    with np.errstate(invalid="ignore"):
        source = raw[(w > np.float32(-1.0)) & (w < np.float32(2147483648.0))]  # cvttss2si(intensity) >= 0
    ids = [closest + j for j in range(-NUM, NUM + 1) if 0 <= closest + j < n]
    target = np.concatenate([np.concatenate([_world(poses[k], frames[k][0]), _world(poses[k], frames[k][1])]) for k in ids])
    return {"source": source, "target": target, "source_ds": G._vg(source, leaf), "target_ds": G._vg(target, leaf)}


def _check_submaps(got, want):
    errs = [diff_report(k, _np(got[k]), want[k]) for k in ("source", "target", "source_ds", "target_ds")]
    for k in ("source", "target", "source_ds", "target_ds"):
        if got["n_" + k] != len(want[k]):
            errs.append(f"n_{k}: {got['n_' + k]} != {len(want[k])}")
    errs = [e for e in errs if e]
    assert not errs, "\n".join(errs)


@pytest.fixture(scope="module")
def scene(require_gpu):
    return K.scene()


def test_submaps_window_clipped_at_zero(scene):
    m = _store(scene.frames, scene.poses, scene.times)
    got = m.loop_submaps(scene.poses[-1, :3], scene.now, _cfg())
    assert (got["found"], got["closest_id"], got["latest_id"]) == (1, 0, scene.K - 1)
    assert got["closest_id"] == L.candidate(np.c_[scene.poses[:, :3], np.arange(scene.K)], scene.times,
                                            scene.poses[-1, :3], scene.now, 8.0)
    _check_submaps(got, _expected_submaps(scene.frames, scene.poses, 0))
    # an ERANGE refusal (every capacity 1) followed by the retry equals a call that fitted at once
    big = m.loop_submaps(scene.poses[-1, :3], scene.now, _cfg(), caps=[4096] * 4)
    for k in ("source", "target", "source_ds", "target_ds"):
        assert not diff_report(k, _np(got[k]), _np(big[k]))
    rep = _abi.LoopReport()
    pos = np.ascontiguousarray(scene.poses[-1, :3], np.float32)
    cfg = _cfg()
    rc = lib().llsr_map_loop_submaps(m._m, C.byref(cfg), pos.ctypes.data, scene.now, C.byref(rep), None, 0, None, 0,
                                     None, 0, None, 0, None)
    assert rc == 0 and rep.n_source == got["n_source"] and rep.n_target_ds == got["n_target_ds"]  # sizes only
    m.close()


def test_submaps_window_clipped_at_the_end_and_holding_the_latest_keyframe(scene):
    """Every keyframe is old: the latest keyframe is its own candidate, the window ends at K - 1."""
    m = _store(scene.frames, scene.poses, scene.times)
    got = m.loop_submaps(scene.poses[-1, :3], scene.now + 100.0, _cfg())
    assert (got["found"], got["closest_id"]) == (1, scene.K - 1)
    _check_submaps(got, _expected_submaps(scene.frames, scene.poses, scene.K - 1))
    m.close()


def test_submaps_intensity_filter(scene):
    frames = [tuple(c.copy() for c in f) for f in scene.frames]
    corner, surf, _ = frames[-1]
    corner[3, 3], corner[10, 3], corner[11, 3], corner[40, 3] = -0.5, -1.0, np.nan, 3e9
    surf[0, 3], surf[7, 3], surf[100, 3], surf[-1, 3] = np.nan, -0.999, -2.5, 2147483648.0
    surf[50, 3] = 2147483520.0  # the largest float below 2^31 stays
    m = _store(frames, scene.poses, scene.times)
    got = m.loop_submaps(scene.poses[-1, :3], scene.now, _cfg())
    want = _expected_submaps(frames, scene.poses, 0)
    assert len(want["source"]) == len(corner) + len(surf) - 6
    _check_submaps(got, want)
    m.close()


def test_no_candidate_and_empty_store(scene):
    m = LocalMap(0, map_config("hdl64e"))
    r = m.loop_submaps([0, 0, 0], 10.0, _cfg())
    assert r["found"] == 0 and r["source"] is None and r["closest_id"] == -1
    assert m.loop_closure([0, 0, 0], 10.0, _cfg())["found"] == 0
    m.close()
    for times, now, radius in ((None, scene.now, 8.0), (scene.times, scene.now, 0.5), (scene.times, 30.0, 8.0)):
        m = _store(scene.frames, scene.poses, times)
        import torch
        sentinel = torch.full((64, 4), 7.0, dtype=torch.float32, device="cuda:0")
        rep = _abi.LoopReport()
        cfg = loop_config("hdl64e", search_num=NUM, search_radius=radius)
        pos = np.ascontiguousarray(scene.poses[-1, :3] + np.float32(2.0 if radius < 1 else 0.0), np.float32)
        p = C.c_void_p(sentinel.data_ptr())
        rc = lib().llsr_map_loop_closure(m._m, None, C.byref(cfg), pos.ctypes.data, now, C.byref(rep), p, 64, p, 64, None)
        assert rc == 0 and rep.found == 0 and rep.accepted == 0 and rep.n_source == 0
        assert bool((sentinel == 7.0).all())  # outputs untouched
        m.close()


def _expected_closure(scene, frames, poses, closest, cfg):
    sub = _expected_submaps(frames, poses, closest)
    icp = R.icp(sub["source"], sub["target"], cfg.icp_max_iterations, cfg.icp_transformation_epsilon,
                cfg.icp_fitness_epsilon, cfg.icp_max_correspondence_distance)
    return sub, icp


def _check_closure(got, sub, icp, poses, closest, cfg):
    K.check_result({k: (_np(got[k]) if k == "aligned" else got[k]) for k in
                    ("T", "iterations", "state", "converged", "n_pairs_last", "fitness", "aligned")}, icp, "closure")
    assert not diff_report("target_ds", _np(got["target_ds"]), sub["target_ds"])
    accepted = bool(icp["converged"]) and not icp["fitness"] > float(cfg.fitness_score)
    assert bool(got["accepted"]) == accepted
    if accepted:
        pf, pt, var = L.constraint(icp["T"], poses[-1], poses[closest], icp["fitness"])
        assert not diff_report("pose_from", got["pose_from"], pf) and not diff_report("pose_to", got["pose_to"], pt)
        assert np.float32(got["variance"]).view(np.uint32) == np.float32(var).view(np.uint32)
    else:
        assert not got["pose_from"].any() and not got["pose_to"].any() and got["variance"] == 0


def test_closure_report_acceptance_and_corrected_pose(scene):
    m = _store(scene.frames, scene.poses, scene.times)
    pos = scene.poses[-1, :3]
    cfg = _cfg()
    sub, icp = _expected_closure(scene, scene.frames, scene.poses, 0, cfg)
    got = m.loop_closure(pos, scene.now, cfg)
    assert (got["found"], got["closest_id"], got["latest_id"]) == (1, 0, scene.K - 1)
    _check_closure(got, sub, icp, scene.poses, 0, cfg)
    assert got["accepted"] == 1
    # the planted drift is recovered to the project's 1e-4 (the restatement's figure: DESIGN.md §16)
    fixed, true = scene.corrected(got["T"])
    assert float(np.abs(fixed - true).max()) <= 1e-4
    # the threshold from both sides: fitness itself still passes (<=), the next float below does not
    f32 = np.float32(icp["fitness"])
    at = f32 if float(f32) >= icp["fitness"] else np.nextafter(f32, np.float32(np.inf))
    for score, want in ((at, 1), (np.nextafter(at, np.float32(-np.inf)), 0)):
        c = _cfg(fitness_score=float(score))
        g = m.loop_closure(pos, scene.now, c)
        assert g["accepted"] == want
        _check_closure(g, sub, icp, scene.poses, 0, c)
        assert not diff_report("aligned", _np(g["aligned"]), icp["aligned"])  # written either way
    # the corrected pose through correctPoses: the next extract equals a fresh store's
    pf = got["pose_from"]
    new = scene.poses.copy()
    new[-1] = [pf[1], pf[2], pf[0], pf[4], pf[5], pf[3]]  # pose_from is z, x, y, yaw, roll, pitch of the store's order
    m.set_key_poses(new)
    fresh = oracle_py.OracleMap(loop_closure=True, search_num=5)
    m2 = LocalMap(0, map_config("hdl64e", surrounding_keyframe_search_num=5))
    for f, p in zip(scene.frames, new):
        fresh.add_keyframe(p, *f)
        m2.add_keyframe(p, *f)
    m2.set_key_poses(new)
    gc, gs, _ = m2.extract(pos)
    ec, es, ids, _ = fresh.extract(pos)
    assert m2.keyframe_ids().tolist() == ids.tolist()
    assert not diff_report("corner", _np(gc), ec) and not diff_report("surf", _np(gs), es)
    (c1, s1), (c2, s2) = m.save_map(), m2.save_map()
    assert not diff_report("save corner", _np(c1), _np(c2)) and not diff_report("save surf", _np(s1), _np(s2))
    m.close()
    m2.close()


def _bits_of(r):
    return {k: (_np(r[k]) if hasattr(r[k], "cpu") else r[k]) for k in r if k != "ms"}


def _same(a, b):
    a, b = _bits_of(a), _bits_of(b)
    errs = []
    for k in a:
        if isinstance(a[k], np.ndarray):
            e = diff_report(k, a[k], b[k])
            if e:
                errs.append(e)
        elif a[k] != b[k]:
            errs.append(f"{k}: {a[k]} != {b[k]}")
    assert not errs, "\n".join(errs)


def test_state_and_reuse(scene):
    cfg = _cfg()
    pos = scene.poses[-1, :3]
    # a small store first, so every workspace buffer is grown by the second call
    small = [tuple(c[:40] for c in f) for f in scene.frames]
    m = _store(small[:8], scene.poses[:8], scene.times[:8])
    first = m.loop_closure(scene.poses[7, :3], 100.0, loop_config("hdl64e", search_num=NUM, search_radius=30.0))
    assert first["found"] == 1
    m.reset()
    for k, (f, p) in enumerate(zip(scene.frames, scene.poses)):
        m.add_keyframe(p, *f)
        m.set_keyframe_time(k, float(scene.times[k]))
    a = m.loop_closure(pos, scene.now, cfg)
    b = m.loop_closure(pos, scene.now, cfg)
    _same(a, b)
    fresh = _store(scene.frames, scene.poses, scene.times)
    _same(a, fresh.loop_closure(pos, scene.now, cfg))
    # the map's own products are the same before and after a closure call (global_map counts its calls,
    # so the two stores run the same sequence, one of them with closure calls in between)
    for step in range(2):
        (ec, es, er), (fc, fs, fr) = m.extract(pos), fresh.extract(pos)
        er.pop("ms"), fr.pop("ms")
        assert er == fr and m.keyframe_ids().tolist() == fresh.keyframe_ids().tolist()
        assert not diff_report("corner", _np(ec), _np(fc)) and not diff_report("surf", _np(es), _np(fs))
        g1, g2 = m.global_map(pos), fresh.global_map(pos)
        for k in ("global", "edge", "planar"):
            assert not diff_report(k, _np(g1[k]), _np(g2[k]))
        assert g1["report"]["call"] == g2["report"]["call"] == step + 1
        (c1, s1), (c2, s2) = m.save_map(), fresh.save_map()
        assert not diff_report("save corner", _np(c1), _np(c2)) and not diff_report("save surf", _np(s1), _np(s2))
        m.loop_closure(pos, scene.now, cfg)
        assert m.num_keyframes == scene.K and m.keyframe_ids().tolist() == fresh.keyframe_ids().tolist()
    m.close()
    fresh.close()
