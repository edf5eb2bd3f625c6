"""GPU: the mapping chain's pose graphs — llsr_mapping_enable_pose_graph, llsr_mapping_close_loops,
llsr_mapping_pose_graph_poses — on the drive of tests/test_gpu_mapping_loop.py, rebuilt here: VLP-16,
seeds (1, 65), six motion=True frames, frame k staged at k + 0.0 s,
loop_config("vlp16", min_time_gap=1.5, search_num=1, fitness_score=1.0). There slot 0's loop is
rejected (fitness 2.118) and slot 1's accepted (0.655).

The first scan of a slot saves no keyframe (FA:2781-2784), so six frames leave five key poses per slot
and eight frames seven (tests/test_gpu_mapping_loop.py pins the seven); the graph is checked against
those counts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from llsr import Pipeline, PoseGraph, _abi, default_config, loop_config, synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF = os.path.join(REPO, "lego-loam-sr_amd", "libllsr_prof.so")
SEEDS = (1, 65)
POSES = ("transform_sum", "transform_tobe_mapped", "transform_bef_mapped", "transform_aft_mapped")
COUNTS = ("frames", "mo_frames", "keyframes", "lm_ran", "n_corner_q", "n_surf_q")


def _slot(pipe, b):
    return {"fetch": pipe.mapping_fetch(b), "keyposes": pipe.mapping_keyposes(b)}


def _differences(a, b):
    errs = [k for k in POSES if a["fetch"][k].tobytes() != b["fetch"][k].tobytes()]
    errs += [k for k in COUNTS if a["fetch"][k] != b["fetch"][k]]
    errs += ["lm." + k for k in a["fetch"]["lm"] if k != "ms" and
             np.asarray(a["fetch"]["lm"][k]).tobytes() != np.asarray(b["fetch"]["lm"][k]).tobytes()]
    if a["keyposes"].tobytes() != b["keyposes"].tobytes():
        errs.append("keyposes")
    return errs


@pytest.fixture(scope="module")
def drive(require_gpu):
    import torch
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    hw = cfg.num_vertical_scans * cfg.num_horizontal_scans
    graph, plain = (Pipeline(cfg, max_batch=2, max_points=hw) for _ in range(2))
    for p in (graph, plain):
        p.mapping_init(_abi.LLSR_MODE_LM_APPLIED)
    graph.mapping_enable_pose_graph(True, max_loops=4)

    def step(k):
        scans = [synth.make_scan(s0 + k, "vlp16", motion=True) for s0 in SEEDS]
        off = np.zeros(len(scans) + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in scans])
        d_pts, d_off = torch.from_numpy(np.concatenate(scans)).cuda(), torch.from_numpy(off).cuda()
        torch.cuda.synchronize()
        for p in (graph, plain):
            p.mapping_stage_times([k + 0.0] * len(scans))
            p.mapping_batch(d_pts.data_ptr(), d_off.data_ptr(), len(scans))

    for k in range(6):
        step(k)
    lcfg = loop_config("vlp16", min_time_gap=1.5, search_num=1, fitness_score=1.0)
    rec = {"after6": {"graph": [_slot(graph, b) for b in (0, 1)], "plain": [_slot(plain, b) for b in (0, 1)]}}
    rec["pg_after6"] = [graph.mapping_pose_graph_poses(b) for b in (0, 1)]
    rec["loop"], rec["pg"] = graph.mapping_close_loops(2, lcfg)
    rec["closed"] = [_slot(graph, b) for b in (0, 1)]
    rec["pg_closed"] = [graph.mapping_pose_graph_poses(b) for b in (0, 1)]
    rec["global"] = {"graph": graph.mapping_global_map(0), "plain": plain.mapping_global_map(0)}
    for k in (6, 7):
        step(k)
    rec["after8"] = {"graph": [_slot(graph, b) for b in (0, 1)], "plain": _slot(plain, 0)}
    rec["pg_after8"] = [graph.mapping_pose_graph_poses(b) for b in (0, 1)]
    graph.mapping_reset()
    rec["pg_reset"] = [len(graph.mapping_pose_graph_poses(b)) for b in (0, 1)]
    graph.close()
    plain.close()
    return rec


def test_the_switch_alone_changes_nothing(drive):
    for b in (0, 1):
        d = _differences(drive["after6"]["graph"][b], drive["after6"]["plain"][b])
        assert not d, (b, d)
        assert drive["after6"]["graph"][b]["fetch"]["keyframes"] == 5
        # the graph holds the slot's key poses, bit for bit (no optimisation ran)
        assert drive["pg_after6"][b].tobytes() == drive["after6"]["graph"][b]["keyposes"].tobytes()


def test_one_slot_is_rejected_and_one_accepted(drive):
    r0, r1 = drive["loop"]
    assert r0["found"] and not r0["accepted"] and abs(r0["fitness"] - 2.118) < 5e-4
    assert r1["found"] and r1["accepted"] and abs(r1["fitness"] - 0.655) < 5e-4
    p0, p1 = drive["pg"]
    assert (p0["state"], p0["iterations"], p0["poses"], p0["loops"]) == (0, 0, 5, 0)
    assert p1["state"] in (1, 2) and p1["iterations"] >= 1 and (p1["poses"], p1["loops"]) == (5, 1)
    assert p1["error_after"] < p1["error_before"] and p1["moved"] and not p0["moved"]


def test_rejected_slot_is_untouched(drive):
    d = _differences(drive["closed"][0], drive["after6"]["plain"][0])
    assert not d, d
    assert drive["pg_closed"][0].tobytes() == drive["pg_after6"][0].tobytes()
    got, exp = drive["global"]["graph"], drive["global"]["plain"]
    for k in ("call", "n_in_radius", "n_poses_used", "n_edge", "n_planar", "n_global_raw", "n_global"):
        assert got["report"][k] == exp["report"][k], k
    assert got["report"]["n_global"] > 0
    for k in ("global", "edge", "planar"):
        assert got[k].cpu().numpy().tobytes() == exp[k].cpu().numpy().tobytes(), k
    # and it goes on as the plain pipeline does through two more frames
    d = _differences(drive["after8"]["graph"][0], drive["after8"]["plain"])
    assert not d, d


def test_accepted_slot_holds_the_host_graphs_poses(drive):
    r1 = drive["loop"][1]
    before = drive["after6"]["graph"][1]["keyposes"]
    host = PoseGraph(1, 8, 1, device=None)
    host.append(0, before)
    host.add_loop(0, r1["latest_id"], r1["closest_id"], r1["pose_from"], r1["pose_to"], r1["variance"])
    rep = host.optimize()[0]
    exp = host.poses(0)
    host.close()
    for k in ("state", "iterations", "poses", "loops", "moved"):
        assert rep[k] == drive["pg"][1][k], k
    for k in ("error_before", "error_after"):
        assert np.float64(rep[k]).tobytes() == np.float64(drive["pg"][1][k]).tobytes(), k
    got = drive["closed"][1]
    assert got["keyposes"].tobytes() == exp.tobytes()
    assert drive["pg_closed"][1].tobytes() == exp.tobytes()
    assert np.any(exp != before)
    newest = exp[-1][[3, 4, 5, 0, 1, 2]]  # transform_*'s layout: roll, pitch, yaw, x, y, z
    for k in ("transform_aft_mapped", "transform_tobe_mapped"):
        assert got["fetch"][k].tobytes() == newest.tobytes(), k


def test_two_more_frames_extend_the_graph(drive):
    s = drive["after8"]["graph"][1]
    assert s["fetch"]["keyframes"] == drive["closed"][1]["fetch"]["keyframes"] + 2 == 7
    assert s["fetch"]["lm"]["iterations"] > 0
    pg = drive["pg_after8"][1]
    assert len(pg) == 7
    assert pg[:5].tobytes() == drive["pg_closed"][1].tobytes()
    assert pg[5:].tobytes() == s["keyposes"][5:].tobytes()
    assert drive["pg_reset"] == [0, 0]


CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from llsr import LlsrError, Pipeline, _abi, default_config, synth
cfg = default_config("vlp16")
cfg.mode = _abi.LLSR_MODE_LM_APPLIED
seeds = [3, 40]
pipe = Pipeline(cfg, max_batch=len(seeds), max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
pipe.mapping_init(_abi.LLSR_MODE_LM_APPLIED)
pipe.mapping_enable_pose_graph(True, 2)
def look():
    return {"graph": [len(pipe.mapping_pose_graph_poses(b)) for b in range(len(seeds))],
            "keyframes": [pipe.mapping_fetch(b)["keyframes"] for b in range(len(seeds))],
            "same": [pipe.mapping_pose_graph_poses(b).tobytes() == pipe.mapping_keyposes(b).tobytes()
                     for b in range(len(seeds))]}
def frame(k):
    scans = [synth.make_scan(s0 + k, "vlp16", motion=True) for s0 in seeds]
    off = np.zeros(len(scans) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in scans])
    d_pts, d_off = torch.from_numpy(np.concatenate(scans)).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    pipe.mapping_batch(d_pts.data_ptr(), d_off.data_ptr(), len(scans))
res = {}
for k in range(3):
    frame(k)
res["before"] = look()
try:
    frame(3)
    res["error"] = None
except LlsrError as e:
    res["error"] = str(e)
res["after_failure"] = look()
frame(4)
res["next"] = look()
print(json.dumps(res))
"""


def test_failed_mapping_call_leaves_the_graphs_pose_count(require_gpu):
    """The diagnostics build's LLSR_MO_FAIL_AT (as tests/test_gpu_mapping_loop_rollback.py uses it): the
    call of frame 3 fails after its keyframes were added; the rollback takes them out of the graphs too."""
    assert os.path.exists(PROF), "libllsr_prof.so missing: run make -C lego-loam-sr_amd"
    env = dict(os.environ, LLSR_LIB=PROF, LLSR_MO_FAIL_AT="3")
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REPO, "lego-loam-sr_amd")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["error"] and "injected MapOptimization failure" in res["error"]
    assert res["before"] == {"graph": [2, 2], "keyframes": [2, 2], "same": [True, True]}
    assert res["after_failure"] == res["before"]
    assert res["next"] == {"graph": [3, 3], "keyframes": [3, 3], "same": [True, True]}
