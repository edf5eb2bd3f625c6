"""publishGlobalMapThread through the node adapter's GlobalMap helper (integration/ros2/llsr_ros2.hpp,
tests/native/ros2_global_map_check.cpp): ten run() iterations, one keyframe each. The helper
publishes on cycles 5 and 10 only (MO:1913-1921), its clouds equal llsr_map_global's on a second map
(checked byte for byte by the program) and the program-order restatement's (tests/_global_map.py):
the first publish raw, the second downsampled."""
import os
import subprocess

import numpy as np
import pytest

import _global_map as G
from _compare import diff_report

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = os.path.join(REPO, "tests", "native", "llsr_ros2_global_map")
SIZES = (300, 0, 1025, 1, 256, 700, 1024, 90, 257, 2500)


@pytest.mark.gpu
def test_global_map_helper_publishes_every_fifth_cycle(require_gpu, tmp_path):
    assert os.path.exists(NODE), "build with make -C lego-loam-sr_amd"
    rng = np.random.default_rng(21)
    frames = []
    for k in range(10):
        pose = np.concatenate([[0.7 * k, 0.3 * k, 0.05 * k], rng.uniform(-0.3, 0.3, 3)]).astype(np.float32)
        frames.append((pose,) + tuple(rng.uniform(-12, 12, (SIZES[(k + 4 * a) % 10], 4)).astype(np.float32)
                                      for a in range(3)))
    fpath, opath = tmp_path / "frames.bin", tmp_path / "out.bin"
    with open(fpath, "wb") as f:
        np.int32(len(frames)).tofile(f)
        for pose, *clouds in frames:
            pose.tofile(f)
            for c in clouds:
                np.int32(len(c)).tofile(f)
                c.tofile(f)
    r = subprocess.run([NODE, str(fpath), str(opath)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    b = open(opath, "rb").read()
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(b, dtype, n, pos)
        pos += a.nbytes
        return a

    published = []
    for _ in range(int(take(np.int32, 1)[0])):
        cycle, call = (int(v) for v in take(np.int32, 2))
        clouds = []
        for _ in range(3):
            n = int(take(np.int32, 1)[0])
            clouds.append(take(np.float32, 4 * n).reshape(n, 4))
        published.append((cycle, call, clouds))
    assert pos == len(b)
    assert [(p[0], p[1]) for p in published] == [(5, 1), (10, 2)]
    ora = G.GlobalMapOracle()
    errs = []
    for k, f in enumerate(frames, 1):
        ora.add_keyframe(*f)
        if k % 5:
            continue
        exp = ora.global_map(f[0][:3])
        got = published[k // 5 - 1][2]
        assert exp["report"]["downsampled_cloud"] == (k == 10)
        errs += [diff_report(f"cycle {k} {key}", g, exp[key]) for key, g in zip(("global", "edge", "planar"), got)]
    assert not any(errs), [e for e in errs if e]
