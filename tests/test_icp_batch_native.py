"""CPU: the loop-closure ICP's host driver on a table of many problems (csrc/llsr_icp.h, DESIGN.md §16
"Batch form") in a stand-alone program under AddressSanitizer / UBSan —
tests/native/icp_batch_host_check.cpp: icp_run_host over a table built by the device call's own layout
functions, on heap buffers of exactly the layout's sizes, against the same driver on every problem as a
table of one at its own table size, bit for bit."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_batch_driver_equals_single_driver_per_problem(tmp_path):
    exe = str(tmp_path / "icp_batch_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "lego-loam-sr_amd", "csrc"), "-o", exe,
                    os.path.join(HERE, "native", "icp_batch_host_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
