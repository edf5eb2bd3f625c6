"""GPU: the loop closure of the mapping chain's slots — llsr_mapping_stage_times,
llsr_mapping_keyframe_times, llsr_mapping_loop_closure (one batched alignment for every slot) and
llsr_mapping_set_key_poses — on the drive of test_gpu_global_map.py::test_mapping_chain_global_map:
VLP-16, seeds (1, 65), six motion=True frames, two slots, frame k staged with the time k + 0.0 s.
Each slot's report must equal llsr_map_loop_closure (LocalMap.loop_closure) on a stand-alone store fed
the oracle chain's keyframes and the same times: every field but ms, the transformation bit for bit.

The drive gives one batch with an accepted and a rejected slot of different sizes and iteration
counts (figures from the oracle chain, llsr_loop_candidate and llsr_icp_align_host on the CPU): both
slots find candidate 2; slot 0 aligns 4042 points onto 11757 in 11 iterations to a fitness of 2.118
(rejected at 1.0), slot 1 aligns 4233 onto 12537 in 9 iterations to 0.655 (accepted); both converge by
the transformation criterion."""
import numpy as np
import pytest

import oracle_py
from _compare import diff_report
from llsr import LocalMap, Pipeline, _abi, default_config, loop_config, synth

pytestmark = pytest.mark.gpu
SEEDS = (1, 65)
INTS = ("found", "closest_id", "latest_id", "accepted", "n_source", "n_target", "n_source_ds", "n_target_ds",
        "converged", "state", "iterations", "n_pairs_last")
SHIFT = np.array([1.0, 2.0, 3.0, 0.0, 0.0, 0.0], np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _slot(pipe, b):
    st = pipe.mapping_fetch(b)
    return {"fetch": st, "keyposes": pipe.mapping_keyposes(b)}


@pytest.fixture(scope="module")
def drive(require_gpu):
    """The whole scenario, run once; the tests below assert on what it recorded."""
    import torch
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    hw = cfg.num_vertical_scans * cfg.num_horizontal_scans
    timed, plain = (Pipeline(cfg, max_batch=2, max_points=hw) for _ in range(2))
    for p in (timed, plain):
        p.mapping_init(_abi.LLSR_MODE_LM_APPLIED)
    oras = [oracle_py.OracleMapping(cfg, _abi.LLSR_MODE_LM_APPLIED) for _ in SEEDS]
    stored = [[] for _ in SEEDS]
    for ora, keep in zip(oras, stored):
        ora.map.add_keyframe = (lambda add, keep: lambda *a: (keep.append(tuple(np.array(x, np.float32) for x in a)),
                                                              add(*a))[1])(ora.map.add_keyframe, keep)

    def step(k, with_oracle):
        scans = [synth.make_scan(s0 + k, "vlp16", motion=True) for s0 in SEEDS]
        off = np.zeros(len(scans) + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in scans])
        d_pts, d_off = torch.from_numpy(np.concatenate(scans)).cuda(), torch.from_numpy(off).cuda()
        torch.cuda.synchronize()
        timed.mapping_stage_times([k + 0.0] * len(scans))
        for p in (timed, plain):
            p.mapping_batch(d_pts.data_ptr(), d_off.data_ptr(), len(scans))
        if with_oracle:
            for ora, s in zip(oras, scans):
                ora.process(s)

    for k in range(6):
        step(k, True)
    lcfg = loop_config("vlp16", min_time_gap=1.5, search_num=1, fitness_score=1.0)
    rec = {"cfg": lcfg, "stored": stored}
    rec["reports"] = timed.mapping_loop_closure(2, lcfg)
    rec["again"] = timed.mapping_loop_closure(2, lcfg)  # no map state changed: the same reports
    rec["unstaged"] = plain.mapping_loop_closure(2, lcfg)
    rec["times"] = [timed.mapping_keyframe_times(b) for b in (0, 1)]
    rec["times_unstaged"] = [plain.mapping_keyframe_times(b) for b in (0, 1)]
    rec["after6"] = [_slot(timed, b) for b in (0, 1)]
    rec["alone"] = []
    for b in (0, 1):
        alone = LocalMap(0)
        for i, f in enumerate(stored[b]):
            alone.add_keyframe(*f)
            alone.set_keyframe_time(i, i + 1.0)  # keyframe i is saved by frame i + 1
        r = alone.loop_closure(rec["after6"][b]["fetch"]["transform_aft_mapped"][3:6], 5.0, lcfg)
        r.pop("aligned"), r.pop("target_ds")
        rec["alone"].append(r)
        alone.close()
    # correctPoses with shifted poses on slot 1, next to the stand-alone store given the same poses
    kp = rec["after6"][1]["keyposes"] + SHIFT
    est = rec["after6"][1]["fetch"]["transform_aft_mapped"] + SHIFT[[3, 4, 5, 0, 1, 2]]
    timed.mapping_set_key_poses(1, kp, est)
    alone = LocalMap(0)
    for f in stored[1]:
        alone.add_keyframe(*f)
    alone.set_key_poses(kp)
    rec["shifted"] = {"keyposes": kp, "estimate": est, "slot": _slot(timed, 1), "global": timed.mapping_global_map(1),
                      "alone": alone.global_map(est[3:6])}
    alone.close()
    # correctPoses with slot 0's own key poses and its own transform_aft_mapped: nothing may change,
    # here or through slot 1's shift
    timed.mapping_set_key_poses(0, rec["after6"][0]["keyposes"], rec["after6"][0]["fetch"]["transform_aft_mapped"])
    for k in (6, 7):
        step(k, False)
    rec["after8"] = {"timed": _slot(timed, 0), "plain": _slot(plain, 0)}
    yield rec
    timed.close()
    plain.close()


def test_slot_reports_equal_the_standalone_store(drive):
    errs = []
    for b in (0, 1):
        got, exp = drive["reports"][b], drive["alone"][b]
        for k in INTS:
            if int(got[k]) != int(exp[k]):
                errs.append(f"slot {b} {k}: {got[k]} != {exp[k]}")
        for k in ("T", "pose_from", "pose_to"):
            r = diff_report(f"slot {b} {k}", np.asarray(got[k], np.float32), np.asarray(exp[k], np.float32))
            if r:
                errs.append(r)
        for k, t in (("fitness", np.float64), ("variance", np.float32)):
            if _bits(t(got[k])) != _bits(t(exp[k])):
                errs.append(f"slot {b} {k}: {got[k]!r} != {exp[k]!r}")
        again = drive["again"][b]
        if any(_bits(np.asarray(got[k])) != _bits(np.asarray(again[k])) for k in got if k != "ms"):
            errs.append(f"slot {b}: a second call reports something else")
    assert not errs, "\n".join(errs)


def test_one_batch_carries_an_accepted_and_a_rejected_slot(drive):
    r0, r1 = drive["reports"]
    print({k: (r0[k], r1[k]) for k in INTS + ("fitness",)})
    assert r0["found"] == r1["found"] == 1 and r0["closest_id"] == r1["closest_id"] == 2
    assert r0["latest_id"] == r1["latest_id"] == 4
    assert (r0["n_source"], r0["n_target"], r0["iterations"]) == (4042, 11757, 11)
    assert (r1["n_source"], r1["n_target"], r1["iterations"]) == (4233, 12537, 9)
    assert r0["state"] == r1["state"] == 2 and r0["converged"] and r1["converged"]
    assert abs(r0["fitness"] - 2.118) < 5e-4 and not r0["accepted"]
    assert abs(r1["fitness"] - 0.655) < 5e-4 and r1["accepted"]
    assert not np.any(r0["pose_from"]) and np.any(r1["pose_from"]) and r1["variance"] == np.float32(r1["fitness"])


def test_times_are_staged_per_keyframe_and_never_staged_means_no_candidate(drive):
    for b in (0, 1):
        assert np.array_equal(drive["times"][b], [1.0, 2.0, 3.0, 4.0, 5.0])
        assert len(drive["times_unstaged"][b]) == 5 and np.all(np.isnan(drive["times_unstaged"][b]))
        r = drive["unstaged"][b]
        assert r["found"] == 0 and r["closest_id"] == -1 and r["iterations"] == 0


def _same_slot(a, b):
    errs = []
    for k in ("transform_sum", "transform_tobe_mapped", "transform_bef_mapped", "transform_aft_mapped"):
        if _bits(a["fetch"][k]) != _bits(b["fetch"][k]):
            errs.append(f"{k}: {a['fetch'][k]} != {b['fetch'][k]}")
    for k in ("frames", "mo_frames", "keyframes", "lm_ran", "n_corner_q", "n_surf_q"):
        if a["fetch"][k] != b["fetch"][k]:
            errs.append(f"{k}: {a['fetch'][k]} != {b['fetch'][k]}")
    for k in a["fetch"]["lm"]:  # the LM report, bit for bit (ms is a wall time)
        x, y = (np.asarray(s["fetch"]["lm"][k]) for s in (a, b))
        if k != "ms" and _bits(x) != _bits(y):
            errs.append(f"lm.{k}: {x} != {y}")
    if _bits(a["keyposes"]) != _bits(b["keyposes"]):
        errs.append("key poses differ")
    return errs


def test_set_key_poses_with_the_slots_own_values_changes_nothing(drive):
    a, b = drive["after8"]["timed"], drive["after8"]["plain"]
    assert a["fetch"]["keyframes"] == 7 and a["fetch"]["lm"]["iterations"] > 0
    assert not _same_slot(a, b), _same_slot(a, b)


def test_set_key_poses_with_shifted_values_is_seen_by_the_chain(drive):
    sh = drive["shifted"]
    assert _bits(sh["slot"]["keyposes"]) == _bits(sh["keyposes"].astype(np.float32))
    for k in ("transform_aft_mapped", "transform_tobe_mapped"):
        assert _bits(sh["slot"]["fetch"][k]) == _bits(sh["estimate"].astype(np.float32)), k
    # the slot's global map is the stand-alone store's with the same poses, around the new position
    got, exp = sh["global"], sh["alone"]
    for k in ("call", "n_in_radius", "n_poses_used", "downsampled_poses", "downsampled_cloud", "passthrough", "n_edge",
              "n_planar", "n_global_raw", "n_global"):
        assert got["report"][k] == exp["report"][k], k
    assert got["report"]["n_global"] > 0
    errs = [diff_report(k, got[k].cpu().numpy(), exp[k].cpu().numpy()) for k in ("global", "edge", "planar")]
    assert not any(errs), errs
