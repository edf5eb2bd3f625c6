"""CPU: the pose-graph optimiser's shared host / device bodies (csrc/llsr_pg.h) in a
stand-alone program under AddressSanitizer / UBSan — tests/native/pg_host_check.cpp: the double trig
against the C library, the analytic Jacobians against central differences, the envelope Cholesky
against a dense one, and every launch's (block, thread) mapping over heap buffers of exactly the
device workspace's sizes."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_pg_bodies_trig_jacobians_cholesky_and_index_mappings(tmp_path):
    exe = str(tmp_path / "pg_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "lego-loam-sr_amd", "csrc"), "-o", exe,
                    os.path.join(HERE, "native", "pg_host_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
