"""GPU: the mapping chain in localisation mode (llsr_mapping_set_prior / llsr_mapping_set_pose,
DESIGN.md §20) against its sequence restatement (tests/_prior_map.py: OraclePriorMapping).

A VLP-16 drive of 6 synthetic scans is mapped with one slot; its saved map (llsr_mapping_save_map,
cornerMap through the VoxelGrid 0.2) becomes the prior of a second handle whose three slots run 6
frames: slot 0 the same scans from pose zero; slot 1 the scans from scan 2 on, its pose set to the
mapping run's key pose of scan 2; slot 2 the same scans with its pose set 1000 m away.

Bar: bit-exact, as tests/test_gpu_mapping.py — frame and key-pose counts, lm_ran, the query and crop
sizes, the LM report, the four poses, the key poses, all under np.array_equal.
Radius 20 m, tile 5 m: the map spans about 30 x 15 x 105 m (corner) and 170 x 20 x 190 m (surf), and
the restatement run on the CPU gives corner crops of 886-889 of the prior's 1060 corner points at that
radius (1058 of 1060 at 50 m), so the crop really cuts; asserted below."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _prior_map as pm
import oracle_py
from llsr import LlsrError, Pipeline, PriorMap, _abi, default_config, synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF = os.path.join(REPO, "lego-loam-sr_amd", "libllsr_prof.so")
POSES = ("transform_sum", "transform_tobe_mapped", "transform_bef_mapped", "transform_aft_mapped")
SEED, FRAMES, RADIUS, TILE = 1, 6, 20.0, 5.0
FAR = np.array([0, 0, 0, 1000, 0, 0], np.float32)


def _cfg():
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    return cfg


def _batch(pipe, scans):
    import torch
    off = np.zeros(len(scans) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in scans])
    d_pts, d_off = torch.from_numpy(np.concatenate(scans)).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    pipe.mapping_batch(d_pts.data_ptr(), d_off.data_ptr(), len(scans))


@pytest.fixture(scope="module")
def mapped(require_gpu):
    """The mapping run: scans 0 .. 7 of the drive, the key poses of the first 6 and the saved map."""
    cfg = _cfg()
    scans = [synth.make_scan(SEED + k, "vlp16", motion=True) for k in range(FRAMES + 2)]
    pipe = Pipeline(cfg, max_batch=1, max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
    pipe.mapping_init(_abi.LLSR_MODE_LM_APPLIED)
    for k in range(FRAMES):
        _batch(pipe, [scans[k]])
    keyposes = pipe.mapping_keyposes(0)
    corner, surf = (a.cpu().numpy() for a in pipe.mapping_save_map(0))
    pipe.close()
    # the odometry of the two scan sequences the slots run (from scan 0, from scan 2), computed once:
    # it does not depend on the map, so every restatement below shares it
    odo = []
    for first in (0, 2):
        oo = oracle_py.OracleOdometry(cfg)
        odo.append([oo.process(scans[first + k]) for k in range(FRAMES)])
    return {"scans": scans, "keyposes": keyposes, "corner": corner, "surf": surf, "odo": odo}


def _slot_scans(scans, k):
    return [scans[k], scans[k + 2], scans[k]]


def _start(pipe, oras, keyposes):
    kp = keyposes[1]  # the key pose of scan 2: x, y, z, roll, pitch, yaw -> transform_aft_mapped's layout
    entry = np.array([kp[3], kp[4], kp[5], kp[0], kp[1], kp[2]], np.float32)
    for b, pose in ((1, entry), (2, FAR)):
        pipe.mapping_set_pose(b, pose)
        oras[b].set_pose(pose)


def _compare(g, o, ora, tag, errs):
    if g["frames"] != o["frames"]:
        errs.append(f"{tag}: frames {g['frames']} vs {o['frames']}")
    if g["mo_frames"] != ora.mo_frames or g["keyframes"] != len(ora.keyposes):
        errs.append(f"{tag}: MapOptimization frames / key poses {g['mo_frames']} / {g['keyframes']} vs "
                    f"{ora.mo_frames} / {len(ora.keyposes)}")
    if not o["step"]:
        return
    for key in ("keyframes", "n_corner_q", "n_surf_q"):
        if g[key] != o[key]:
            errs.append(f"{tag}: {key} {g[key]} vs {o[key]}")
    if bool(g["lm_ran"]) != bool(o["lm_ran"]):
        errs.append(f"{tag}: lm_ran {g['lm_ran']} vs {o['lm_ran']}")
    for key, want in o["map"].items():
        if g["map"][key] != want:
            errs.append(f"{tag}: map {key} {g['map'][key]} vs {want}")
    if o["lm_ran"]:
        for key in ("iterations", "converged", "degenerate", "n_corner_corr", "n_surf_corr"):
            if g["lm"][key] != o["lm"][key]:
                errs.append(f"{tag}: lm {key} {g['lm'][key]} vs {o['lm'][key]}")
    for key in POSES:
        if not np.array_equal(g[key], o[key]):
            errs.append(f"{tag}: {key} {g[key]} vs {o[key]} (max |d| {np.abs(g[key] - o[key]).max():.3g})")


def test_three_slots_localise_in_the_saved_map(mapped):
    cfg = _cfg()
    scans = mapped["scans"]
    prior = PriorMap.from_saved(mapped["corner"], mapped["surf"], corner_leaf=0.2, radius=RADIUS, tile=TILE)
    info = prior.info()
    n_corner = info["corner"]["n_points"]
    assert 0 < n_corner < len(mapped["corner"]) and info["surf"]["n_points"] == len(mapped["surf"])
    stored = prior.points("corner"), prior.points("surf")
    pipe = Pipeline(cfg, max_batch=3, max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
    pipe.mapping_init(_abi.LLSR_MODE_LM_APPLIED)
    host = PriorMap(radius=RADIUS, tile=TILE, device=None)
    with pytest.raises(LlsrError) as e:  # a prior on another device (here: the host twin)
        pipe.mapping_set_prior(host)
    assert e.value.code == _abi.LLSR_EINVAL
    host.close()
    pipe.mapping_set_prior(prior)
    runs = []
    for attempt in range(2):  # the second pass after mapping_reset, which keeps the prior
        oras = [pm.OraclePriorMapping(cfg, _abi.LLSR_MODE_LM_APPLIED, stored[0], stored[1], RADIUS) for _ in range(3)]
        _start(pipe, oras, mapped["keyposes"])
        errs, first_mo, cut = [], {}, False
        for k in range(FRAMES):
            sc = _slot_scans(scans, k)
            _batch(pipe, sc)
            for b, ora in enumerate(oras):
                o = ora.process(sc[b], odo=mapped["odo"][b == 1][k])
                g = pipe.mapping_fetch(b)
                _compare(g, o, ora, f"pass {attempt} slot {b} frame {k}", errs)
                if o["step"]:
                    first_mo.setdefault(b, g)
                    if b == 2:
                        assert not g["lm_ran"] and g["map"]["n_corner_map"] == 0 and g["map"]["n_surf_map"] == 0
                        assert g["lm"]["iterations"] == 0
                    else:
                        cut |= 0 < g["map"]["n_corner_map"] < n_corner
        assert not errs, "\n".join(errs)
        kps = [pipe.mapping_keyposes(b) for b in range(3)]
        for b, ora in enumerate(oras):
            assert np.array_equal(kps[b], np.array(ora.keyposes, np.float32).reshape(-1, 6)), f"slot {b}: key poses"
        # conditions: slots 0 and 1 have a local map and run the LM on their first MapOptimization frame
        assert first_mo[0]["lm_ran"] and first_mo[1]["lm_ran"] and first_mo[0]["mo_frames"] == 1
        assert cut, "no frame's corner crop is a proper part of the prior: the radius does not cut the map"
        # slot 2 never passes MO:1573, so only the odometry moves it: its first key pose is the set pose
        # carried forward by transformAssociateToMap (transformTobeMapped: near 1000 m, not exactly
        # there); every later one is transformAftMapped, which without an LM stays the set pose
        # (MO:1722-1733 copy it over transformTobeMapped), while transformSum keeps advancing
        far = kps[2][:, :3] - FAR[3:6]
        assert len(far) == FRAMES - 1 and 0 < np.abs(far[0]).max() < 5.0 and not far[1:].any()
        assert np.array_equal(first_mo[2]["transform_tobe_mapped"][3:], kps[2][0, :3])
        g2 = pipe.mapping_fetch(2)
        assert np.array_equal(g2["transform_aft_mapped"], FAR) and not g2["transform_bef_mapped"].any()
        runs.append((kps, [pipe.mapping_fetch(b) for b in range(3)]))
        if attempt == 0:
            # after a frame the prior can be neither attached nor detached; the calls that need
            # keyframe clouds are refused
            for p in (prior, None):
                with pytest.raises(LlsrError) as e:
                    pipe.mapping_set_prior(p)
                assert e.value.code == _abi.LLSR_EINVAL
            pipe.mapping_enable_pose_graph(True, 4)
            for call in (lambda: pipe.mapping_global_map(0), lambda: pipe.mapping_save_map(0),
                         lambda: pipe.mapping_loop_closure(3), lambda: pipe.mapping_close_loops(3)):
                with pytest.raises(LlsrError) as e:
                    call()
                assert e.value.code == _abi.LLSR_ENOSYS, str(e.value)
            pipe.mapping_enable_pose_graph(False)
            pipe.mapping_reset()
    (ka, fa), (kb, fb) = runs
    for b in range(3):
        assert np.array_equal(ka[b], kb[b]), f"slot {b}: the pass after mapping_reset differs"
        for key in POSES + ("lm_ran", "mo_frames", "keyframes"):
            assert np.array_equal(fa[b][key], fb[b][key]), (b, key)
        assert fa[b]["map"] == {**fb[b]["map"], "ms": fa[b]["map"]["ms"]}
    # detaching after a reset gives the mapping chain back: the store-based calls work again
    pipe.mapping_reset()
    pipe.mapping_set_prior(None)
    _batch(pipe, _slot_scans(scans, 0))
    _batch(pipe, _slot_scans(scans, 1))
    c, s = pipe.mapping_save_map(0)
    assert len(c) > 0 and len(s) > 0
    pipe.close()
    prior.close()


CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from llsr import LlsrError, Pipeline, PriorMap, _abi, default_config, synth
z = np.load(sys.argv[2])
cfg = default_config("vlp16")
cfg.mode = _abi.LLSR_MODE_LM_APPLIED
prior = PriorMap(radius=float(z["radius"]), tile=float(z["tile"]))
prior.load(z["corner"], z["surf"])
pipe = Pipeline(cfg, max_batch=2, max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
pipe.mapping_init(_abi.LLSR_MODE_LM_APPLIED)
pipe.mapping_set_prior(prior)
pipe.mapping_set_pose(1, z["entry"])
def state(b):
    f = pipe.mapping_fetch(b)
    f.pop("frames")
    out = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in f.items()}
    out["keyposes"] = pipe.mapping_keyposes(b).tolist()
    return out
res = {"failed_at": None, "frames": []}
for k in range(int(z["frames"])):
    scans = [synth.make_scan(int(z["seed"]) + k + d, "vlp16", motion=True) for d in (0, 2)]
    off = np.zeros(3, np.int64)
    off[1:] = np.cumsum([len(s) for s in scans])
    d_pts, d_off = torch.from_numpy(np.concatenate(scans)).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    snap = [state(b) for b in range(2)]
    try:
        pipe.mapping_batch(d_pts.data_ptr(), d_off.data_ptr(), 2)
    except LlsrError as e:
        res["failed_at"], res["error"], res["before"] = k, str(e), snap
        res["after"] = [state(b) for b in range(2)]
    res["frames"].append([state(b) for b in range(2)])
print(json.dumps(res, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o)))
"""


def test_rollback_of_a_failed_frame_in_localisation_mode(mapped, tmp_path):
    """libllsr_prof.so fails the call in which slot 0 reaches MapOptimization frame 3 (LLSR_MO_FAIL_AT),
    after its key poses were recorded: every slot's MapOptimization members and key-pose counts are as
    before the call, and the next frame matches the restatement that skipped that frame's
    MapOptimization (the odometry had advanced)."""
    assert os.path.exists(PROF), "libllsr_prof.so missing: run make -C lego-loam-sr_amd"
    cfg = _cfg()
    prior = PriorMap.from_saved(mapped["corner"], mapped["surf"], corner_leaf=0.2, radius=RADIUS, tile=TILE)
    stored = prior.points("corner"), prior.points("surf")
    prior.close()
    kp = mapped["keyposes"][1]
    entry = np.array([kp[3], kp[4], kp[5], kp[0], kp[1], kp[2]], np.float32)
    fix = str(tmp_path / "prior.npz")
    np.savez(fix, corner=stored[0], surf=stored[1], radius=RADIUS, tile=TILE, entry=entry, seed=SEED, frames=FRAMES)
    env = dict(os.environ, LLSR_LIB=PROF, LLSR_MO_FAIL_AT="3")
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REPO, "lego-loam-sr_amd"), fix], env=env,
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    fail = res["failed_at"]
    assert fail is not None and fail + 1 < FRAMES, "the injected failure never fired, or on the last frame"
    assert "injected MapOptimization failure" in res["error"]
    for b, (pre, post) in enumerate(zip(res["before"], res["after"])):
        assert len(pre["keyposes"]) >= 1, f"slot {b}: nothing to roll back"
        for key in pre:
            assert json.dumps(post[key]) == json.dumps(pre[key]), f"slot {b}: {key} changed by the failed call"
    oras = [pm.OraclePriorMapping(cfg, _abi.LLSR_MODE_LM_APPLIED, stored[0], stored[1], RADIUS) for _ in range(2)]
    oras[1].set_pose(entry)
    scans = mapped["scans"]
    errs = []
    for k in range(fail + 2):
        for b, ora in enumerate(oras):
            if k == fail:  # the failed call: the odometry advanced, MapOptimization did not
                continue
            o = ora.process(scans[k + 2 * b], odo=mapped["odo"][b][k])
            g = dict(res["frames"][k][b], frames=o["frames"])
            g = {key: (np.array(v, np.float32) if key in POSES else v) for key, v in g.items()}
            _compare(g, o, ora, f"slot {b} frame {k}", errs)
            if k == fail + 1:
                assert o["step"] and g["mo_frames"] == ora.mo_frames == k - 1
                assert np.array_equal(np.array(g["keyposes"], np.float32).reshape(-1, 6),
                                      np.array(ora.keyposes, np.float32).reshape(-1, 6)), f"slot {b}: key poses"
    assert not errs, "\n".join(errs)
