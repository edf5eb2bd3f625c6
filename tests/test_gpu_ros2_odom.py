"""runFeatureAssociation in the reference's program order through the node adapter
(integration/ros2/llsr_ros2.hpp): Odometry::solve, OdomInput::apply (updateInitialGuess, FA:2790),
Odometry::finish, with /odom2 arriving on a fourth thread (tests/native/ros2_odom_check.cpp). Two
VLP-16 drives of four frames, one fed a message before most frames and one fed none, bit for bit
against the faithful oracle chain (tests/_odom_guess.py)."""
import os
import subprocess

import numpy as np
import pytest

import _odom_guess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = os.path.join(REPO, "tests", "native", "llsr_ros2_odom")
SEED0, FRAMES = 1, 4
HAS_MESSAGE = (1, 0, 1, 1)  # frame 1 arrives without a new message: the sample of frame 0 stays


def _read(path):
    b = open(path, "rb").read()
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(b, dtype, n, pos)
        pos += a.nbytes
        return a

    drives = []
    for _ in range(2):
        fa = []
        for _ in range(int(take(np.int32, 1)[0])):
            seq, lm, msgs = (int(v) for v in take(np.int32, 3))
            r = {"seq": seq, "lm": lm, "messages": msgs, "transform_lm": take(np.float32, 6),
                 "transform_cur": take(np.float32, 6), "transform_sum": take(np.float32, 6)}
            for key in ("corner_last", "surf_last", "corner_scan", "surf_scan"):
                n = int(take(np.int32, 1)[0])
                r[key] = take(np.float32, 4 * n).reshape(n, 4)
            fa.append(r)
        mo = []
        for _ in range(int(take(np.int32, 1)[0])):
            mo.append({"seq": int(take(np.int32, 1)[0]), "transform_sum": take(np.float32, 6)})
        drives.append((fa, mo))
    assert pos == len(b)
    return drives


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
def test_adapter_program_order_with_odom_thread(require_gpu, tmp_path):
    from llsr import _abi, default_config, synth
    assert os.path.exists(NODE), "build with make -C lego-loam-sr_amd"
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    scans = [np.ascontiguousarray(synth.make_scan(SEED0 + k, "vlp16", motion=True), np.float32) for k in range(FRAMES)]
    msgs = [synth.odom_message(SEED0 + k) for k in range(FRAMES)]
    fpath, opath, outp = tmp_path / "frames.bin", tmp_path / "odom.bin", tmp_path / "out.bin"
    with open(fpath, "wb") as f:
        np.int32(FRAMES).tofile(f)
        for p in scans:
            np.int32(len(p)).tofile(f)
            p.tofile(f)
    with open(opath, "wb") as f:
        for has, m in zip(HAS_MESSAGE, msgs):
            np.int32(has).tofile(f)
            np.ascontiguousarray(m[:7], np.float64).tofile(f)
    r = subprocess.run([NODE, "drive", str(_abi.LLSR_LIDAR_VLP16), str(fpath), str(opath), str(outp)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    drives = _read(outp)
    errs = []
    for name, (fa, mo), deliver in (("messages", drives[0], True), ("no message", drives[1], False)):
        assert [x["seq"] for x in fa] == list(range(FRAMES))
        inp, ora, seen = _odom_guess.OdomInput(), _odom_guess.FaithfulOracleOdometry(cfg), 0
        for k, g in enumerate(fa):
            if deliver and HAS_MESSAGE[k]:
                inp.callback(msgs[k])
                seen += 1
            o = ora.process(scans[k], inp.sample)
            tag = f"{name} frame {k}"
            if g["messages"] != seen:
                errs.append(f"{tag}: {g['messages']} messages seen vs {seen}")
            if g["lm"] != (o["lm"] is not None):
                errs.append(f"{tag}: lm ran {g['lm']} vs oracle {o['lm'] is not None}")
            for key in ("transform_lm", "transform_cur", "transform_sum", "corner_last", "surf_last"):
                if not _bits_equal(g[key], o[key]):
                    errs.append(f"{tag}: {key} differs")
            if k and np.array_equal(g["transform_lm"], g["transform_cur"]):
                errs.append(f"{tag}: apply left the LM's transformCur in place")
            for key in ("corner_scan", "surf_scan"):
                ref = o[key] if o[key] is not None else np.zeros((0, 4), np.float32)
                if not _bits_equal(g[key], ref):
                    errs.append(f"{tag}: {key} differs")
        assert mo, "MO received no AssociationOut"
        for m in mo:  # a non-blocking channel: MO sees a subset of the frames, each as FA sent it
            if not _bits_equal(m["transform_sum"], fa[m["seq"]]["transform_sum"]):
                errs.append(f"{name}: MO frame {m['seq']} transformSum differs from FA's")
    assert not errs, "\n".join(errs)
