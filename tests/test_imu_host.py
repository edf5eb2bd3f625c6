"""CPU tests of the IMU input's host entry points (include/llsr.h: llsr_imu_callback,
llsr_imu_scan_window, llsr_imu_deskew_host) against the numpy restatement of the reference's lines
(tests/_imu.py). Host-side code of libllsr.so, so no GPU is needed; the device copy of the same
per-point body (k_fa_points_imu) is compared with the restatement in tests/test_gpu_imu.py.

Bar: bit-exact. Both sides call the host glibc and keep the reference's float / double typing."""
import numpy as np
import pytest

import _imu
import llsr
from _imu_cases import SCAN0_NS, bits_equal, feed, make_msgs, seg_cloud, window_streams
from llsr import _abi, synth

F = np.float32
PERIOD = 0.1


def assert_state_equal(state, queue, tag=""):
    got, exp = state.arrays(), queue.arrays()
    assert set(got) == set(exp)
    for k in exp:
        if isinstance(exp[k], int):
            assert got[k] == exp[k], (tag, k, got[k], exp[k])
        else:
            assert bits_equal(got[k], exp[k]), (tag, k, np.argwhere(got[k] != exp[k])[:5])


def stream(n=450):
    """n (450) messages at 100 Hz from t = 1000.35 s: the ring wraps twice; gaps of 0.25 s and 0.5 s before
    messages 120 and 333 (>= scan_period: their nine accumulated entries are not written and keep the
    ring's content of 200 messages earlier, or zero); yaw ramps up through +pi (wrapping to -pi) and
    later down through -pi; roll and pitch wobble by a few degrees."""
    rng = np.random.default_rng(5)
    t = 1000_350_000_000 + np.arange(n, dtype=np.int64) * 10_000_000
    t[120:] += 250_000_000 - 10_000_000
    t[333:] += 500_000_000 - 10_000_000
    k = np.arange(n)
    yaw_unwrapped = np.where(k < 225, 2.6 + 0.006 * k, 2.6 + 0.006 * 225 - 0.009 * (k - 225))
    yaw = (yaw_unwrapped + np.pi) % (2 * np.pi) - np.pi
    assert (np.diff(yaw) < -np.pi).any() and (np.diff(yaw) > np.pi).any()
    rpy = np.stack([0.04 * np.sin(0.07 * k), 0.03 * np.cos(0.05 * k), yaw], axis=1)
    return make_msgs(t, rpy, rng)


def test_callback_matches_restatement_on_450_messages():
    msgs = stream()
    state, queue = llsr.ImuState(PERIOD), _imu.Queue(PERIOD)
    assert_state_equal(state, queue, "constructor")
    assert state.arrays()["pointer_last"] == -1 and state.arrays()["pointer_last_iteration"] == 0
    for i, m in enumerate(msgs):
        feed(state, queue, [m])
        if i in (0, 119, 120, 199, 200, 319, 320, 333, 399, 400, 449):
            assert_state_equal(state, queue, f"message {i}")
    assert_state_equal(state, queue, "end")
    # the skipped entries really are stale: entry 120 was written once more (message 320), entry
    # 333 % 200 = 133 keeps message 133's accumulation under message 333's angles
    q = queue.arrays()
    assert q["pointer_last"] == 449 % 200


def test_callback_rejects_bad_arguments():
    L = llsr.lib()
    assert L.llsr_imu_init(None) != 0
    assert L.llsr_imu_callback(None, None, F(PERIOD)) != 0
    st = llsr.ImuState(PERIOD)
    assert L.llsr_imu_scan_window(None, None, None) != 0
    st.state.pointer_last = 200
    assert L.llsr_imu_callback(st.state, _abi.ImuMsg(), F(PERIOD)) != 0


def expected_window(queue):
    """include/llsr.h's definition on the restated ring: entries (pointer_last_iteration - 1 + k) mod 200
    for k = 0 .. n, n = ((pointer_last - pointer_last_iteration) mod 200) + 1; empty before a message."""
    if queue.pointer_last < 0:
        return np.zeros(0, llsr.IMU_SAMPLE_DTYPE)
    first = max(queue.pointer_last_iteration, 0)
    n = (queue.pointer_last - first) % 200 + 1
    idx = (first - 1 + np.arange(n + 1)) % 200
    w = np.zeros(n + 1, llsr.IMU_SAMPLE_DTYPE)
    w["time"], w["roll"], w["pitch"], w["yaw"] = queue.time[idx], queue.roll[idx], queue.pitch[idx], queue.yaw[idx]
    w["velo"], w["shift"], w["angular_rotation"] = queue.velo[:, idx].T, queue.shift[:, idx].T, queue.angular_rotation[:, idx].T
    return w


def test_scan_window_after_0_1_199_200_230_messages():
    """The window between scans after 0 (no IMU ever), then 1, 199, 200, 230 and again 0 messages: its
    length, its entries as the ring holds them, and FA:788 afterwards."""
    msgs = stream(630)
    state, queue = llsr.ImuState(PERIOD), _imu.Queue(PERIOD)
    pos = 0
    lengths = []
    for count in (0, 1, 199, 200, 230, 0):
        feed(state, queue, msgs[pos:pos + count])
        pos += count
        exp = expected_window(queue)
        got = state.scan_window()
        lengths.append(len(got))
        assert bits_equal(got, exp), count
        queue.pointer_last_iteration = queue.pointer_last  # FA:788
        assert_state_equal(state, queue, f"after {count}")
    # no IMU: empty. First scan: pointer 0 -> 0: one candidate + its back. 199 more: 200 candidates.
    # 200 more: the pointers are equal again (one candidate, not "no IMU"). 230: 31. None since: 1.
    assert lengths == [0, 2, 201, 2, 32, 2]
    assert state.arrays()["pointer_last"] >= 0


# ---- de-skew --------------------------------------------------------------------------------
STREAMS = window_streams()
SIZES = (0, 1, 11, 2503)
CLOUDS = {S: [seg_cloud(S, 100 * S + k) for k in range(3)] for S in SIZES}


def report_of(carry):
    return {m: np.asarray(carry[m], F) for m in _imu.MEMBERS}


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_deskew_host_matches_restatement(name, S):
    cfg = llsr.default_config("vlp16")
    state, queue = llsr.ImuState(cfg.scan_period), _imu.Queue(cfg.scan_period)
    carry, exp_carry = _abi.ImuCarry(), _imu.zero_carry()
    for k in range(3):
        feed(state, queue, STREAMS[name][k])
        ns = SCAN0_NS + k * 100_000_000
        stamp = (ns // 10 ** 9, ns % 10 ** 9)
        seg, ori = CLOUDS[S][k]
        window = state.scan_window()
        assert (len(window) == 0) == (name == "no_imu" or (name == "late_imu" and k == 0))
        got, rep = llsr.imu_deskew_host(cfg, stamp, window, seg, ori, carry)
        exp = queue.adjust_distortion(seg, ori, stamp, exp_carry)
        assert bits_equal(got, exp), (name, S, k, np.argwhere(got.view(np.uint32) != exp.view(np.uint32))[:5])
        for m, v in report_of(exp_carry).items():
            assert bits_equal(rep[m], v), (name, S, k, m, rep[m], v)
        assert bits_equal(np.array(carry.angular_rotation_last, F), exp_carry["angular_rotation_last"]), (name, S, k)
        assert_state_equal(state, queue, f"{name} scan {k}")
        if len(window) and S > 1:
            plain, _ = _imu.loam_swap(seg, ori, cfg.scan_period)
            assert bits_equal(got[0], plain[0])           # point 0 is not rotated
            assert not bits_equal(got[1:, :3], plain[1:, :3])  # the others are
            assert bits_equal(got[:, 3], plain[:, 3])


def test_deskew_host_plain_path_equals_the_oracle_cloud():
    """With no window the host de-skew is FA:565-598 alone: the oracle's LOAM cloud of a generated
    scan, from the oracle's own segmented cloud and orientations."""
    import oracle_py
    cfg = llsr.default_config("vlp16")
    o = oracle_py.Oracle(cfg).process(synth.make_scan(2, "vlp16"))
    seg, ori = np.asarray(o["seg_xyzi"], F), np.asarray(o["orientation"], F)
    assert len(seg) > 10000
    carry = _abi.ImuCarry()
    got, rep = llsr.imu_deskew_host(cfg, (0, 0), None, seg, ori, carry)
    assert bits_equal(got, np.asarray(o["loam_xyzi"], F))
    assert bits_equal(_imu.loam_swap(seg, ori, cfg.scan_period)[0], np.asarray(o["loam_xyzi"], F))
    assert bits_equal(_imu.curvature(o["loam_xyzi"])[5:-5], np.asarray(o["curvature"], F)[5:len(seg) - 5])
    assert all(not v.any() for v in rep.values())
