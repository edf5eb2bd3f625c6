"""CPU: the IMU de-skew's shared host / device body (csrc/llsr_imu.h) in a stand-alone program under
AddressSanitizer / UBSan — tests/native/imu_host_check.cpp: the per-point body over heap buffers of
exactly the window's and the cloud's sizes, every window length, the edge windows, the ring callback
across two wraps."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_imu_body_over_exact_size_buffers(tmp_path):
    exe = str(tmp_path / "imu_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "lego-loam-sr_amd", "csrc"), "-o", exe,
                    os.path.join(HERE, "native", "imu_host_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
