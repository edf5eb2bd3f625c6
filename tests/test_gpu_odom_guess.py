"""GPU parity of the odometry and mapping batches with updateInitialGuess in program order
(llsr_odometry_batch_odom / llsr_mapping_batch_odom; runFeatureAssociation FA:2781-2796) against
the faithful oracle chain of tests/_odom_guess.py (FaithfulOracleOdometry: oracle_py's feature
stage, scan-to-scan LM, integrateTransformation and TransformToEnd around the Python
updateInitialGuess).

Bar: bit-exact, as tests/test_gpu_odometry.py and tests/test_gpu_mapping.py: frame counts, LM skip
flag and counters, transformCur / transformSum / the LM's own transformCur, the four clouds, and for
the mapping chain every field tests/test_gpu_mapping.py compares plus the key poses.
"""
import copy
import functools

import numpy as np
import pytest

import _odom_guess
import oracle_py
from llsr import Pipeline, _abi, default_config, synth

pytestmark = pytest.mark.gpu
POSES = ("transform_sum", "transform_tobe_mapped", "transform_bef_mapped", "transform_aft_mapped")
VLP_SEEDS = [1, 65, 130]


def _cfg(lidar, mode=_abi.LLSR_MODE_LM_APPLIED):
    cfg = default_config(lidar, 2048 if lidar == "hdl64e" else None)
    cfg.mode = mode
    return cfg


@functools.lru_cache(maxsize=None)
def _scan(seed, lidar):
    return synth.make_scan(seed, lidar, motion=True)


def _first_message(lidar, slot):
    # VLP-16 slot 2's stream delivers its first message only before frame 2
    return 2 if (lidar == "vlp16" and slot == 2) else 0


@functools.lru_cache(maxsize=None)
def _samples(lidar, seed0, slot, frames):
    return _odom_guess.drive_samples(seed0, frames, _first_message(lidar, slot))


@functools.lru_cache(maxsize=None)
def _reference(lidar, seed0, slot, frames, faithful):
    """The oracle chain of one drive, computed once and shared (read-only) by the cases."""
    cfg = _cfg(lidar)
    if faithful:
        ora, smp = _odom_guess.FaithfulOracleOdometry(cfg), _samples(lidar, seed0, slot, frames)
        return [ora.process(_scan(seed0 + k, lidar), smp[k]) for k in range(frames)]
    ora = oracle_py.OracleOdometry(cfg)
    return [ora.process(_scan(seed0 + k, lidar)) for k in range(frames)]


def _upload(scans):
    import torch
    off = np.zeros(len(scans) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in scans])
    d_pts = torch.from_numpy(np.concatenate(scans)).cuda()
    d_off = torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    return d_pts, d_off


def _compare_slot(g, g_lm, o, tag, errs):
    if g["frames"] != o["frames"]:
        errs.append(f"{tag}: frames {g['frames']} vs {o['frames']}")
    if (g["lm"]["skipped"] == 1) != (o["lm"] is None):
        errs.append(f"{tag}: skipped {g['lm']['skipped']} vs oracle lm {o['lm'] is not None}")
    elif o["lm"] is not None:
        for key in ("surf_iterations", "corner_iterations", "n_surf_corr", "n_corner_corr", "degenerate"):
            if g["lm"][key] != o["lm"][key]:
                errs.append(f"{tag}: lm {key} {g['lm'][key]} vs {o['lm'][key]}")
    keys = ["transform_cur", "transform_sum"]
    if "transform_lm" in o:
        g = dict(g, transform_lm=g_lm)
        keys.append("transform_lm")
    for key in keys:
        if not np.array_equal(g[key], o[key]):
            errs.append(f"{tag}: {key} {g[key]} vs {o[key]} (max |d| {np.abs(g[key] - o[key]).max():.3g})")
    for key in ("corner_last", "surf_last", "corner_scan", "surf_scan"):
        ref = o[key] if o[key] is not None else np.zeros((0, 4), np.float32)
        if g[key].shape != ref.shape:
            errs.append(f"{tag}: {key} shape {g[key].shape} vs {ref.shape}")
        elif not np.array_equal(g[key], ref):
            errs.append(f"{tag}: {key} max |d| {np.abs(g[key] - ref).max():.3g}")


def _drive(lidar, seeds, frames, overwrite=None, mode=_abi.LLSR_MODE_LM_APPLIED):
    cfg = _cfg(lidar, mode)
    H, W = cfg.num_vertical_scans, cfg.num_horizontal_scans
    pipe = Pipeline(cfg, max_batch=len(seeds), max_points=H * W)
    flags = [1] * len(seeds) if overwrite is None else overwrite
    refs = [_reference(lidar, s0, b, max(frames, 4 if lidar == "vlp16" else frames), bool(flags[b]))
            for b, s0 in enumerate(seeds)]
    errs = []
    for k in range(frames):
        d_pts, d_off = _upload([_scan(s0 + k, lidar) for s0 in seeds])
        samples = [_samples(lidar, s0, b, len(refs[b]))[k] for b, s0 in enumerate(seeds)]
        pipe.odometry_batch_odom(d_pts.data_ptr(), d_off.data_ptr(), len(seeds), samples, overwrite)
        for b in range(len(seeds)):
            _compare_slot(pipe.odometry_fetch(b, clouds=True), pipe.odometry_fetch_lm(b), refs[b][k],
                          f"{lidar} slot {b} frame {k}", errs)
    pipe.close()
    return errs


def test_odom_vlp16_all_slots_flagged(require_gpu):
    """Case 1: three drives, four frames, every slot overwritten (slot 2 sees the zero sample on
    frames 0-1)."""
    errs = _drive("vlp16", VLP_SEEDS, 4)
    assert not errs, "\n".join(errs)


def test_odom_vlp16_per_slot_flags(require_gpu):
    """Case 2: overwrite = [1, 0, 1] in one launch: slot 1 is the lm_applied chain
    (oracle_py.OracleOdometry) bit for bit, slots 0 and 2 the faithful chain."""
    errs = _drive("vlp16", VLP_SEEDS, 4, overwrite=[1, 0, 1])
    assert not errs, "\n".join(errs)


def test_odom_partial_batch_and_reset(require_gpu):
    """Case 3: B = 2 on a max_batch 3 handle, llsr_odometry_reset, the same two frames again: the
    same results, and slot 2 untouched."""
    cfg = _cfg("vlp16")
    pipe = Pipeline(cfg, max_batch=3, max_points=16 * 1800)
    runs = []
    for _ in range(2):
        pipe.odometry_reset()
        for k in range(2):
            d_pts, d_off = _upload([_scan(s0 + k, "vlp16") for s0 in VLP_SEEDS[:2]])
            samples = [_samples("vlp16", s0, b, 4)[k] for b, s0 in enumerate(VLP_SEEDS[:2])]
            pipe.odometry_batch_odom(d_pts.data_ptr(), d_off.data_ptr(), 2, samples)
        runs.append([(pipe.odometry_fetch(b, clouds=True), pipe.odometry_fetch_lm(b)) for b in range(3)])
    errs = []
    for b in range(2):
        _compare_slot(runs[0][b][0], runs[0][b][1], _reference("vlp16", VLP_SEEDS[b], b, 4, True)[1],
                      f"first pass slot {b}", errs)
        (ga, la), (gb, lb) = runs[0][b], runs[1][b]
        assert np.array_equal(la, lb) and la.any()
        for key in ("transform_cur", "transform_sum", "corner_last", "surf_last", "corner_scan", "surf_scan"):
            assert np.array_equal(ga[key], gb[key]), (b, key)
        assert ga["frames"] == gb["frames"] == 2
    assert not errs, "\n".join(errs)
    for g, lm in (runs[0][2], runs[1][2]):
        assert g["frames"] == 0 and g["n_corner_last"] == 0 and g["n_surf_last"] == 0
        assert not g["transform_cur"].any() and not g["transform_sum"].any() and not lm.any()
    pipe.close()


def test_odom_faithful_mode_handle(require_gpu):
    """Case 4: a handle created with LLSR_MODE_FAITHFUL takes odometry_batch_odom (and still refuses
    odometry_batch); the first two frames equal case 1's."""
    errs = _drive("vlp16", VLP_SEEDS, 2, mode=_abi.LLSR_MODE_FAITHFUL)
    assert not errs, "\n".join(errs)


def test_odom_hdl64e_all_slots_flagged(require_gpu):
    """Case 5: HDL-64E 64 x 2048, two drives, three frames."""
    errs = _drive("hdl64e", [5, 70], 3)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("mo_mode", [_abi.LLSR_MODE_FAITHFUL, _abi.LLSR_MODE_LM_APPLIED], ids=["mo_faithful", "mo_applied"])
def test_mapping_chain_with_overwrite(require_gpu, mo_mode):
    """Case 6: VLP-16, two slots, four frames through mapping_batch_odom against OracleMapping with
    the faithful odometry plugged in. The MapOptimization-faithful chain runs on a handle created
    with LLSR_MODE_FAITHFUL, at iterCountThres 50 like tests/test_gpu_mapping.py's."""
    seeds, frames = VLP_SEEDS[:2], 4
    cfg = _cfg("vlp16")
    if mo_mode == _abi.LLSR_MODE_FAITHFUL:
        cfg.iterCountThres = 50
    hcfg = copy.copy(cfg)
    hcfg.mode = mo_mode
    pipe = Pipeline(hcfg, max_batch=len(seeds), max_points=16 * 1800)
    pipe.mapping_init(mo_mode)
    oras = []
    for _ in seeds:
        m = oracle_py.OracleMapping(cfg, mo_mode, loop_closure=False)
        m.odo = _odom_guess.FaithfulOracleOdometry(cfg)
        oras.append(m)
    errs = []
    for k in range(frames):
        d_pts, d_off = _upload([_scan(s0 + k, "vlp16") for s0 in seeds])
        samples = [_samples("vlp16", s0, b, 4)[k] for b, s0 in enumerate(seeds)]
        pipe.mapping_batch_odom(d_pts.data_ptr(), d_off.data_ptr(), len(seeds), samples)
        for b, ora in enumerate(oras):
            ora.odo.sample = samples[b]
            o = ora.process(_scan(seeds[b] + k, "vlp16"))
            g = pipe.mapping_fetch(b)
            tag = f"mo_mode {mo_mode} slot {b} frame {k}"
            if g["frames"] != o["frames"]:
                errs.append(f"{tag}: frames {g['frames']} vs {o['frames']}")
            if g["mo_frames"] != ora.mo_frames or g["keyframes"] != len(ora.keyposes):
                errs.append(f"{tag}: MapOptimization frames / keyframes {g['mo_frames']} / {g['keyframes']} vs "
                            f"{ora.mo_frames} / {len(ora.keyposes)}")
            go = pipe.odometry_fetch(b)
            for key in ("transform_cur", "transform_sum"):
                if not np.array_equal(go[key], o["odo"][key]):
                    errs.append(f"{tag}: odometry {key} {go[key]} vs {o['odo'][key]}")
            if not o["step"]:
                continue
            for key in ("keyframes", "n_corner_q", "n_surf_q"):
                if g[key] != o[key]:
                    errs.append(f"{tag}: {key} {g[key]} vs {o[key]}")
            if bool(g["lm_ran"]) != bool(o["lm_ran"]):
                errs.append(f"{tag}: lm_ran {g['lm_ran']} vs {o['lm_ran']}")
            if o["map"] is not None:
                for key, ok in (("n_corner_ds", "n_corner_map"), ("n_surf_ds", "n_surf_map")):
                    if g["map"][key] != o[ok]:
                        errs.append(f"{tag}: map {key} {g['map'][key]} vs {o[ok]}")
                for key in ("n_keyframes", "n_corner_map", "n_surf_map", "n_in_radius", "n_poses_ds"):
                    if g["map"][key] != o["map"][key]:
                        errs.append(f"{tag}: map {key} {g['map'][key]} vs {o['map'][key]}")
            if o["lm_ran"]:
                for key in ("iterations", "converged", "degenerate", "n_corner_corr", "n_surf_corr"):
                    if g["lm"][key] != o["lm"][key]:
                        errs.append(f"{tag}: lm {key} {g['lm'][key]} vs {o['lm'][key]}")
            for key in POSES:
                if not np.array_equal(g[key], o[key]):
                    errs.append(f"{tag}: {key} {g[key]} vs {o[key]} (max |d| {np.abs(g[key] - o[key]).max():.3g})")
    for b, ora in enumerate(oras):
        kg = pipe.mapping_keyposes(b)
        ko = np.array(ora.keyposes, np.float32).reshape(-1, 6)
        if kg.shape != ko.shape:
            errs.append(f"slot {b}: keyposes {kg.shape} vs {ko.shape}")
        elif not np.array_equal(kg, ko):
            errs.append(f"slot {b}: keyposes max |d| {np.abs(kg - ko).max():.3g}")
    assert all(len(ora.keyposes) == frames - 1 for ora in oras)
    pipe.close()
    assert not errs, "\n".join(errs)


def test_batch_without_overwrite_still_refuses_faithful_handles(require_gpu):
    """llsr_mapping_batch on a faithful-mode handle keeps LLSR_ENOSYS; mapping_init now accepts the handle."""
    from llsr import LlsrError
    pipe = Pipeline(_cfg("vlp16", _abi.LLSR_MODE_FAITHFUL), max_batch=1, max_points=16 * 1800)
    pipe.mapping_init(_abi.LLSR_MODE_FAITHFUL)
    d_pts, d_off = _upload([_scan(1, "vlp16")])
    with pytest.raises(LlsrError):
        pipe.mapping_batch(d_pts.data_ptr(), d_off.data_ptr(), 1)
    with pytest.raises(LlsrError):
        pipe.odometry_batch(d_pts.data_ptr(), d_off.data_ptr(), 1)
    assert pipe.odometry_fetch(0)["frames"] == 0
    pipe.close()
