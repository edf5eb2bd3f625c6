"""GPU: the staged scan times under llsr_mapping_batch's error contract. A call whose MapOptimization
part fails (the diagnostics build's LLSR_MO_FAIL_AT, as in tests/test_gpu_mapping_rollback.py) has
consumed its staged times, adds no keyframe time, and leaves every slot's `now` as before the call.

`now` shows only through the loop candidate, so the times are chosen to make it visible: frame k is
staged at 100 k seconds and the candidate needs a gap of more than 150 s. The call of frame 3 fails.
Before it the slots hold keyframes at 100 and 200 s and now = 200 s: no keyframe is 150 s away. Had the
failed call left now = 300 s, keyframe 0 would be a candidate. Frame 4 runs without staging (the failed
call consumed it): its keyframe has no time and still nothing is a candidate. Frame 5, staged at 500 s,
gives both slots a candidate. The drive runs in a child process (the library is chosen at import)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF = os.path.join(REPO, "lego-loam-sr_amd", "libllsr_prof.so")

CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from llsr import LlsrError, Pipeline, _abi, default_config, loop_config, synth
cfg = default_config("vlp16")
cfg.mode = _abi.LLSR_MODE_LM_APPLIED
seeds = [3, 40]
pipe = Pipeline(cfg, max_batch=len(seeds), max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
pipe.mapping_init(_abi.LLSR_MODE_LM_APPLIED)
lcfg = loop_config("vlp16", min_time_gap=150.0, search_num=1)
def look():
    reps = pipe.mapping_loop_closure(len(seeds), lcfg)
    return {"found": [r["found"] for r in reps], "closest": [r["closest_id"] for r in reps],
            "times": [pipe.mapping_keyframe_times(b).tolist() for b in range(len(seeds))]}
def frame(k, stage):
    scans = [synth.make_scan(s0 + k, "vlp16", motion=True) for s0 in seeds]
    off = np.zeros(len(scans) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in scans])
    d_pts, d_off = torch.from_numpy(np.concatenate(scans)).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    if stage:
        pipe.mapping_stage_times([100.0 * k] * len(scans))
    pipe.mapping_batch(d_pts.data_ptr(), d_off.data_ptr(), len(scans))
res = {}
for k in range(3):
    frame(k, True)
res["before"] = look()
try:
    frame(3, True)
    res["error"] = None
except LlsrError as e:
    res["error"] = str(e)
res["after_failure"] = look()
frame(4, False)  # the failed call consumed its staging: this keyframe gets no time, `now` stays
res["unstaged"] = look()
frame(5, True)
res["staged_again"] = look()
print(json.dumps(res))
"""


def test_failed_call_consumes_the_staged_times_and_restores_now(require_gpu):
    assert os.path.exists(PROF), "libllsr_prof.so missing: run make -C lego-loam-sr_amd"
    env = dict(os.environ, LLSR_LIB=PROF, LLSR_MO_FAIL_AT="3")
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REPO, "lego-loam-sr_amd")], env=env,
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["error"] and "injected MapOptimization failure" in res["error"]
    assert res["before"] == {"found": [0, 0], "closest": [-1, -1], "times": [[100.0, 200.0]] * 2}
    assert json.dumps(res["after_failure"]) == json.dumps(res["before"])  # no keyframe time added, now = 200 s
    # frame 4 without staging: a keyframe without a time (NaN), now still 200 s
    un = res["unstaged"]
    assert un["found"] == [0, 0] and all(t[:2] == [100.0, 200.0] and len(t) == 3 and t[2] != t[2] for t in un["times"])
    # frame 5 staged at 500 s: keyframes 0 and 1 are more than 150 s away; the nearest of them is the candidate
    ag = res["staged_again"]
    assert ag["found"] == [1, 1] and all(c in (0, 1) for c in ag["closest"])
    assert all(t[:2] == [100.0, 200.0] and t[3] == 500.0 for t in ag["times"])
