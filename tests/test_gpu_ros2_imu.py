"""The node adapter's IMU input (integration/ros2/llsr_ros2.hpp: ImuInput, Projection::run with a
stamp; tests/native/ros2_imu_check.cpp).

CPU: the adapter compiles against stand-in message structs with sensor_msgs/Imu's field names, and
ImuInput fed from a second thread hands out the windows of the C entry points, also across the
ring's wrap. GPU: a four-frame VLP-16 drive in the adapter's thread layout, an /imu_type thread
feeding each frame's messages before the projection thread runs the scan, bit for bit against the
restatement (tests/_imu.py) of the same snapshots."""
import os
import subprocess

import numpy as np
import pytest

import _imu
import llsr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "ros2_imu_check.cpp")
NODE = os.path.join(REPO, "tests", "native", "llsr_ros2_imu")
F = np.float32
SEED0, FRAMES = 1, 4


def test_imu_input_compiles_and_matches_the_c_entry_points(tmp_path):
    exe = str(tmp_path / "ros2_imu_check")
    libdir = os.path.dirname(llsr.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++11", "-pthread", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "integration", "ros2"), "-o", exe, SRC, "-L", libdir, "-lllsr",
                    f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr


@pytest.mark.gpu
def test_adapter_drive_with_imu_thread(require_gpu, tmp_path):
    from llsr import _abi, default_config, synth
    assert os.path.exists(NODE), "build with make -C lego-loam-sr_amd"
    cfg = default_config("vlp16")
    scans = [np.ascontiguousarray(synth.make_scan(SEED0 + k, "vlp16", motion=True), F) for k in range(FRAMES)]
    stamps = [synth.scan_stamp(SEED0 + k) for k in range(FRAMES)]
    stream = synth.imu_stream(SEED0, 100, FRAMES)
    t = stream["sec"].astype(np.int64) * 10 ** 9 + stream["nanosec"]
    # frame k's messages: those stamped up to its end, except frame 1's, which arrive a frame late
    ends = [s[0] * 10 ** 9 + s[1] + 100_000_000 for s in stamps]
    cut = [int(np.searchsorted(t, e)) for e in ends]
    cut[1] = cut[0]
    per_frame = [stream[(cut[k - 1] if k else 0):cut[k]] for k in range(FRAMES)]
    fpath, ipath, outp = tmp_path / "frames.bin", tmp_path / "imu.bin", tmp_path / "out.bin"
    with open(fpath, "wb") as f:
        np.int32(FRAMES).tofile(f)
        for p, st in zip(scans, stamps):
            np.int32(st[0]).tofile(f)
            np.uint32(st[1]).tofile(f)
            np.int32(len(p)).tofile(f)
            p.tofile(f)
    with open(ipath, "wb") as f:
        for msgs in per_frame:
            np.int32(len(msgs)).tofile(f)
            for m in msgs:
                np.int32(m["sec"]).tofile(f)
                np.uint32(m["nanosec"]).tofile(f)
                np.concatenate([m["orientation"], m["angular_velocity"], m["linear_acceleration"]]).astype(np.float64).tofile(f)
    r = subprocess.run([NODE, "drive", str(_abi.LLSR_LIDAR_VLP16), str(fpath), str(ipath), str(outp)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    b = open(outp, "rb").read()
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(b, dtype, n, pos)
        pos += a.nbytes
        return a

    queue, carry, seen = _imu.Queue(cfg.scan_period), _imu.zero_carry(), 0
    for k in range(FRAMES):
        S = int(take(np.int32, 1)[0])
        seg, loam = take(F, 4 * S).reshape(S, 4), take(F, 4 * S).reshape(S, 4)
        ori, rep, messages = take(F, 3), take(F, 12).reshape(4, 3), int(take(np.int64, 1)[0])
        for m in per_frame[k]:
            queue.handler(m)
        seen += len(per_frame[k])
        assert messages == seen and S > 16000
        exp = queue.adjust_distortion(seg, ori, stamps[k], carry)
        assert loam.tobytes() == exp.tobytes(), f"frame {k}: loam_xyzi differs"
        for row, name in zip(rep, _imu.MEMBERS):
            assert row.tobytes() == np.asarray(carry[name], F).tobytes(), (k, name, row, carry[name])
        assert not np.array_equal(exp[1:, :3], _imu.loam_swap(seg, ori, cfg.scan_period)[0][1:, :3])
    assert pos == len(b)
