"""Shared inputs of the IMU tests (tests/test_imu_host.py, tests/test_gpu_imu.py): message builders
and the edge windows, the messages that arrive before each of three consecutive scans."""
import numpy as np

import _imu
from llsr import synth

F = np.float32


def quat(roll, pitch, yaw):
    """setRPY's quaternion x, y, z, w (any attitude, yaw near +-pi included)."""
    cr, sr, cp, sp, cy, sy = (f(v / 2) for v in (roll, pitch, yaw) for f in (np.cos, np.sin))
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy])


def make_msgs(times_ns, rpy, rng):
    m = np.zeros(len(times_ns), synth.IMU_MSG_DTYPE)
    for i, ns in enumerate(times_ns):
        m[i]["sec"], m[i]["nanosec"] = int(ns) // 10 ** 9, int(ns) % 10 ** 9
        m[i]["orientation"] = quat(*rpy[i])
        m[i]["angular_velocity"] = rng.uniform(-0.5, 0.5, 3)
        m[i]["linear_acceleration"] = rng.uniform(-1.0, 1.0, 3) + (0.0, 0.0, 9.81)
    return m


def feed(state, queue, msgs):
    for m in msgs:
        state.callback(m["sec"], m["nanosec"], m["orientation"], m["angular_velocity"], m["linear_acceleration"])
        queue.handler(m)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return a.tobytes() == b.tobytes()


SCAN0_NS = 1000_400_000_000  # the first scan's stamp; scan k starts k periods later


def seg_cloud(S, seed):
    """A segmented cloud in the IP frame in sweep order: azimuth decreasing over one turn from just
    past the rear (like the sensor's), ring + col / 1e4 intensities; start / end orientation from the
    first and last point as imageProjection's findStartEndAngle does."""
    rng = np.random.default_rng(seed)
    if S == 0:
        return np.zeros((0, 4), F), np.array([0.0, 2 * np.pi, 2 * np.pi], F)
    az = np.pi - 0.01 - (2 * np.pi - 0.02) * (np.arange(S) / max(S - 1, 1))
    r = rng.uniform(2.0, 60.0, S)
    el = rng.uniform(-0.26, 0.26, S)
    p = np.zeros((S, 4), F)
    p[:, 0], p[:, 1], p[:, 2] = r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)
    p[:, 3] = rng.integers(0, 16, S) + rng.integers(0, 1800, S) / 1e4
    start = F(-_imu.atan2f(p[0, 1], p[0, 0]))
    end = F(np.float64(-_imu.atan2f(p[-1, 1], p[-1, 0])) + 2 * np.pi)
    if np.float64(end) - np.float64(start) > 3 * np.pi:
        end = F(np.float64(end) - 2 * np.pi)
    elif np.float64(end) - np.float64(start) < np.pi:
        end = F(np.float64(end) + 2 * np.pi)
    return p, np.array([start, end, end - start], F)


def window_streams():
    """name -> list of three message arrays, the messages that arrive before scans 0, 1 and 2."""
    rng = np.random.default_rng(9)

    def regular(rate_hz, lo_ns, hi_ns, yaw0=0.3):
        t = np.arange(lo_ns, hi_ns, int(round(1e9 / rate_hz)), dtype=np.int64)
        k = (t - SCAN0_NS) * 1e-8
        rpy = np.stack([0.03 * np.sin(2.1 * k), 0.02 * np.cos(1.3 * k), yaw0 + 0.05 * k], axis=1)
        return make_msgs(t, rpy, rng)

    def per_scan(fn):
        return [fn(k) for k in range(3)]

    P = 100_000_000
    out = {}
    # messages up to the scan's end have arrived when the scan is processed
    out["100hz"] = per_scan(lambda k: regular(100, SCAN0_NS + (k - 1) * P + 5_000_000, SCAN0_NS + (k + 1) * P))
    out["500hz"] = per_scan(lambda k: regular(500, SCAN0_NS + (k - 1) * P + 1_000_000, SCAN0_NS + (k + 1) * P))
    out["all_older"] = per_scan(lambda k: regular(100, SCAN0_NS + (k - 3) * P + 5_000_000, SCAN0_NS + (k - 2) * P))
    out["all_newer"] = per_scan(lambda k: regular(100, SCAN0_NS + (k + 2) * P + 5_000_000, SCAN0_NS + (k + 3) * P))

    def equal_stamps(k):
        m = regular(100, SCAN0_NS + (k - 1) * P + 5_000_000, SCAN0_NS + (k + 1) * P)
        m["sec"][11], m["nanosec"][11] = m["sec"][10], m["nanosec"][10]  # a zero divisor inside the scan
        return m
    out["equal_stamps"] = per_scan(equal_stamps)
    for name, yaw0, step in (("yaw_jump_up", 3.0, 0.4), ("yaw_jump_down", -3.0, -0.4)):
        def jump(k, yaw0=yaw0, step=step):
            t = np.arange(SCAN0_NS + (k - 1) * P + 5_000_000, SCAN0_NS + (k + 1) * P, 10_000_000, dtype=np.int64)
            yaw = yaw0 + step * np.arange(len(t)) / len(t)  # crosses +-pi inside every scan's window
            yaw = (yaw + np.pi) % (2 * np.pi) - np.pi
            assert (np.abs(np.diff(yaw)) > np.pi).any()
            return make_msgs(t, np.stack([np.full(len(t), 0.01), np.full(len(t), -0.02), yaw], axis=1), rng)
        out[name] = per_scan(jump)
    out["no_imu"] = [np.zeros(0, synth.IMU_MSG_DTYPE)] * 3
    out["late_imu"] = [np.zeros(0, synth.IMU_MSG_DTYPE)] + out["100hz"][1:]  # the first scan runs without IMU
    return out
