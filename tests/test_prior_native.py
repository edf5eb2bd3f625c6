"""CPU: the prior map's host path (csrc/llsr_prior.h) in a stand-alone program under
AddressSanitizer / UBSan — tests/native/prior_host_check.cpp: the index build and the serial crop, the
bodies the device kernels share, against a brute-force statement on the hand-built edge clouds and on
random clouds, with every output on the heap at exactly the reported size."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_prior_index_and_crop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "prior_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "lego-loam-sr_amd", "csrc"), "-o", exe,
                    os.path.join(HERE, "native", "prior_host_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
