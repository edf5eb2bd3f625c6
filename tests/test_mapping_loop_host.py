"""CPU: the precondition of tests/test_gpu_mapping_loop.py, pinned without a GPU. On its drive (VLP-16,
seeds 1 and 65, six motion=True frames, frame k at k + 0.0 s) the oracle chain's key poses give a loop
candidate for both seeds under the test's configuration (15 m radius, a time gap of 1.5 s): keyframe 2,
the nearest of the three that are old enough, so the alignment window of search_num = 1 is keyframes 1-3."""
import numpy as np
import pytest

import llsr
import oracle_py
from llsr import _abi, default_config, synth


@pytest.mark.parametrize("seed", [1, 65])
def test_drive_has_a_loop_candidate(seed):
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    ora = oracle_py.OracleMapping(cfg, _abi.LLSR_MODE_LM_APPLIED)
    for k in range(6):
        ora.process(synth.make_scan(seed + k, "vlp16", motion=True))
    assert len(ora.keyposes) == 5
    poses4 = np.zeros((5, 4), np.float32)
    poses4[:, :3] = np.array(ora.keyposes)[:, :3]
    times = np.arange(1.0, 6.0)  # keyframe i is saved by frame i + 1
    lc = llsr.loop_config("vlp16", min_time_gap=1.5, search_num=1, fitness_score=1.0)
    got = llsr.loop_candidate(poses4, times, ora.robot, 5.0, lc.search_radius, lc.min_time_gap)
    assert got == 2
    # a slot that never got a time: no candidate
    nan = np.full(5, np.nan)
    assert llsr.loop_candidate(poses4, nan, ora.robot, float("nan"), lc.search_radius, lc.min_time_gap) == -1
    assert llsr.loop_candidate(poses4, times, ora.robot, float("nan"), lc.search_radius, lc.min_time_gap) == -1
