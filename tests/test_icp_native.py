"""CPU: the loop-closure ICP's shared host / device bodies (csrc/llsr_icp.h) in a stand-alone program
under AddressSanitizer / UBSan — tests/native/icp_host_check.cpp: the shell search against a
brute-force loop, the chains against umeyama3_host, and every launch's (block, thread) mapping (the
one driver, icp_run_host, on a table of one) over heap buffers of exactly icp_sizes."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_icp_bodies_search_chains_and_index_mappings(tmp_path):
    exe = str(tmp_path / "icp_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "lego-loam-sr_amd", "csrc"), "-o", exe,
                    os.path.join(HERE, "native", "icp_host_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
