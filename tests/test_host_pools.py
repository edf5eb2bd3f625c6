"""CPU: the C-ABI host layer's resource helpers (csrc/llsr_host.h) and pool layouts
(csrc/llsr_pools.h) in a stand-alone program under AddressSanitizer / UBSan, against a fake of the
HIP calls they use — tests/native/host_pool_check.cpp: every pool's measured size equals its
placed size with 256-aligned, ordered, non-overlapping pieces; a failure at any acquisition of a
build leaves nothing live and the sub-state empty; the owners release exactly once."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_pool_layouts_failure_paths_and_owners(tmp_path):
    exe = str(tmp_path / "host_pool_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + os.path.join(ROOT, "lego-loam-sr_amd", "csrc"), "-o", exe,
                    os.path.join(HERE, "native", "host_pool_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
