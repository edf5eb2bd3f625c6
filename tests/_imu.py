"""Independent numpy statement of the reference's IMU input and IMU de-skew, for the tests of that
branch (the oracle does not state it):

* `Queue.handler(msg)`: imuHandler + AccumulateIMUShiftAndRotation (featureAssociation.cpp = FA,
  lines 315-351, 452-489) on the 200-entry ring;
* `Queue.adjust_distortion(...)`: adjustDistortion (FA:565-690, 788) of one scan, the queue search as
  the ring walk the reference runs (not the library's linear window), VeloToStartIMU and
  TransformToStartIMU (FA:519-563);
* `curvature(loam)`: calculateSmoothnessOurs' cloudCurvature (FA:817-848).

Written from the reference's lines. Exactness: float32 / float64 + - * / in numpy are correctly
rounded and never fused, like the reference's x86-64 build; sinf / cosf / atan2f / sin / cos / asin /
atan2 are the host glibc's own (libm.so.6 through ctypes), which is what the reference calls. Every
expression keeps the reference's types and order: imuTime and timeScanCur are double, the other
members float; a double operand promotes the expression it sits in. The per-point part is evaluated
for all points at once (points are independent: imuPointerFront restarts for every point), with the
same scalar expressions element by element.
"""
import ctypes

import numpy as np

F = np.float32
D = np.float64
PI = D(np.pi)  # M_PI
QUEUE = 200

_libm = ctypes.CDLL("libm.so.6")
for _name, _n, _t in (("sinf", 1, ctypes.c_float), ("cosf", 1, ctypes.c_float), ("atan2f", 2, ctypes.c_float),
                      ("sin", 1, ctypes.c_double), ("cos", 1, ctypes.c_double), ("asin", 1, ctypes.c_double),
                      ("atan2", 2, ctypes.c_double)):
    _f = getattr(_libm, _name)
    _f.restype = _t
    _f.argtypes = [_t] * _n


def _f1(name, a):
    """A float libm function of one argument over a float32 array (or scalar)."""
    f = getattr(_libm, name)
    a = np.asarray(a, F)
    return np.array([f(float(v)) for v in a.ravel()], F).reshape(a.shape)


def sinf(a):
    return _f1("sinf", a)


def cosf(a):
    return _f1("cosf", a)


def atan2f(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.array([_libm.atan2f(float(u), float(v)) for u, v in zip(a.ravel(), b.ravel())], F).reshape(a.shape)


def _d(name, *a):
    return D(getattr(_libm, name)(*(float(v) for v in a)))


def get_rpy(q):
    """tf2::Matrix3x3(tf2::Quaternion(x, y, z, w)).getRPY(roll, pitch, yaw) in double
    (Matrix3x3::setRotation, Matrix3x3::getEulerYPR with solution 1)."""
    x, y, z, w = (D(v) for v in q)
    d = x * x + y * y + z * z + w * w
    s = D(2.0) / d
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    m00, m10, m20, m21, m22 = D(1.0) - (yy + zz), xy + wz, xz - wy, yz + wx, D(1.0) - (xx + yy)
    if abs(m20) >= 1:
        yaw = D(0.0)
        delta = _d("atan2", m21, m22)
        pitch = PI / D(2.0) if m20 < 0 else -PI / D(2.0)
        roll = delta
    else:
        pitch = -_d("asin", m20)
        cp = _d("cos", pitch)
        roll = _d("atan2", m21 / cp, m22 / cp)
        yaw = _d("atan2", m10 / cp, m00 / cp)
    return roll, pitch, yaw


MEMBERS = ("start", "angular_from_start", "cur", "velo_from_start")


def zero_carry():
    """The constructor's zeros of the members a scan hands to the next (FA:241-257)."""
    c = {m: np.zeros(3, F) for m in MEMBERS}
    c["angular_rotation_last"] = np.zeros(3, F)
    return c


class Queue:
    """FeatureAssociation's IMU members (featureAssociation.h:68-119) after the constructor."""

    def __init__(self, scan_period):
        self.scan_period = F(scan_period)
        self.pointer_last = -1
        self.pointer_last_iteration = 0
        self.time = np.zeros(QUEUE, D)
        self.roll, self.pitch, self.yaw = (np.zeros(QUEUE, F) for _ in range(3))
        self.acc, self.velo, self.shift, self.angular_velo, self.angular_rotation = (np.zeros((3, QUEUE), F)
                                                                                     for _ in range(5))

    def arrays(self):
        d = {"pointer_last": self.pointer_last, "pointer_last_iteration": self.pointer_last_iteration}
        for f in ("time", "roll", "pitch", "yaw", "acc", "velo", "shift", "angular_velo", "angular_rotation"):
            d[f] = getattr(self, f)
        return d

    def handler(self, msg):
        """imuHandler (FA:315-351); msg: a record with sec, nanosec, orientation, angular_velocity,
        linear_acceleration."""
        roll, pitch, yaw = get_rpy(msg["orientation"])
        la = [D(v) for v in msg["linear_acceleration"]]
        acc_x = F(la[1] - _d("sin", roll) * _d("cos", pitch) * D(9.81))
        acc_y = F(la[2] - _d("cos", roll) * _d("cos", pitch) * D(9.81))
        acc_z = F(la[0] + _d("sin", pitch) * D(9.81))
        self.pointer_last = (self.pointer_last + 1) % QUEUE
        p = self.pointer_last
        self.time[p] = D(int(msg["sec"])) + D(int(msg["nanosec"])) / D(1e9)
        self.roll[p], self.pitch[p], self.yaw[p] = F(roll), F(pitch), F(yaw)
        self.acc[:, p] = (acc_x, acc_y, acc_z)
        self.angular_velo[:, p] = [F(D(v)) for v in msg["angular_velocity"]]
        self._accumulate()

    def _accumulate(self):
        """AccumulateIMUShiftAndRotation (FA:452-489)."""
        p = self.pointer_last
        roll, pitch, yaw = self.roll[p], self.pitch[p], self.yaw[p]
        acc_x, acc_y, acc_z = self.acc[:, p]
        x1 = cosf(roll) * acc_x - sinf(roll) * acc_y
        y1 = sinf(roll) * acc_x + cosf(roll) * acc_y
        z1 = acc_z
        x2 = x1
        y2 = cosf(pitch) * y1 - sinf(pitch) * z1
        z2 = sinf(pitch) * y1 + cosf(pitch) * z1
        acc = (F(cosf(yaw) * x2 + sinf(yaw) * z2), F(y2), F(-sinf(yaw) * x2 + cosf(yaw) * z2))
        back = (p + QUEUE - 1) % QUEUE
        dt = self.time[p] - self.time[back]  # double
        if dt < D(self.scan_period):
            for k in range(3):
                a = D(acc[k])
                self.shift[k, p] = F(D(self.shift[k, back]) + D(self.velo[k, back]) * dt + a * dt * dt / D(2))
                self.velo[k, p] = F(D(self.velo[k, back]) + a * dt)
                self.angular_rotation[k, p] = F(D(self.angular_rotation[k, back]) + D(self.angular_velo[k, back]) * dt)

    # ---- adjustDistortion -------------------------------------------------------------------
    def _select(self, point_time, time_scan_cur):
        """FA:603-628 for an array of float32 pointTime: the ring walk from imuPointerLastIteration,
        then front / back ring indices, the `newer than front` flag and the two float ratios."""
        tp = D(time_scan_cur) + point_time.astype(D)
        # (imuPointerLastIteration is -1 after a scan without IMU, where the reference reads imuTime[-1];
        # include/llsr.h defines that walk to start at entry 0)
        walk = [max(self.pointer_last_iteration, 0)]
        while walk[-1] != self.pointer_last:
            walk.append((walk[-1] + 1) % QUEUE)
        walk = np.array(walk)
        # the walk stops at the first entry (before the last) whose time is above the point's
        stop = tp[:, None] < self.time[walk[:-1]][None, :]
        pos = np.where(stop.any(axis=1), stop.argmax(axis=1), len(walk) - 1) if len(walk) > 1 else np.zeros(len(tp), int)
        front = walk[pos]
        back = (front + QUEUE - 1) % QUEUE
        tf, tb = self.time[front], self.time[back]
        take = tp > tf
        with np.errstate(all="ignore"):
            rf = ((tp - tb) / (tf - tb)).astype(F)
            rb = ((tf - D(time_scan_cur) - point_time.astype(D)) / (tf - tb)).astype(F)
        return front, back, take, rf, rb

    @staticmethod
    def _blend(arr, sel):
        front, back, take, rf, rb = sel
        with np.errstate(all="ignore"):
            return np.where(take, arr[front], arr[front] * rf + arr[back] * rb).astype(F)

    def _blend_yaw(self, sel):
        front, back, take, rf, rb = sel
        yf, yb = self.yaw[front], self.yaw[back]
        with np.errstate(all="ignore"):
            diff = (yf - yb).astype(D)
            up = ((yf * rf).astype(D) + (yb.astype(D) + D(2) * PI) * rb.astype(D)).astype(F)
            dn = ((yf * rf).astype(D) + (yb.astype(D) - D(2) * PI) * rb.astype(D)).astype(F)
            mid = yf * rf + yb * rb
        return np.where(take, yf, np.where(diff > PI, up, np.where(diff < -PI, dn, mid))).astype(F)

    def adjust_distortion(self, seg_xyzi, orientation, scan_stamp, carry):
        """FA:565-690 and 788. seg_xyzi: the segmented cloud (IP frame); orientation: segInfo's
        start_orientation, end_orientation, orientation_diff; scan_stamp: (sec, nanosec) of the
        cloud's header; carry: zero_carry() or the previous scan's, updated in place. Returns the
        cloud after adjustDistortion, float32 [S, 4]."""
        seg = np.asarray(seg_xyzi, F).reshape(-1, 4)
        S = len(seg)
        loam, rel = loam_swap(seg, orientation, self.scan_period)
        if self.pointer_last >= 0 and S > 0:
            time_scan_cur = D(int(scan_stamp[0])) + D(int(scan_stamp[1])) / D(1e9)  # FA:2761
            point_time = rel * self.scan_period
            sel = self._select(point_time, time_scan_cur)
            cur = np.stack([self._blend(self.roll, sel), self._blend(self.pitch, sel), self._blend_yaw(sel)], axis=1)
            sel0 = tuple(v[:1] for v in sel)
            # i == 0 (FA:649-685)
            st = cur[0].copy()
            velo_start = np.array([self._blend(self.velo[k], sel0)[0] for k in range(3)], F)
            ar = np.array([self._blend(self.angular_rotation[k], sel0)[0] for k in range(3)], F)
            carry["angular_from_start"] = (ar - carry["angular_rotation_last"]).astype(F)
            carry["angular_rotation_last"] = ar
            carry["start"] = st
            c_st, s_st = cosf(st), sinf(st)  # roll, pitch, yaw
            carry["cur"] = cur[S - 1].copy()
            if S > 1:
                # VeloToStartIMU of the last point (FA:519-536): the member is overwritten by every point
                sel1 = tuple(v[S - 1:] for v in sel)
                velo_cur = np.array([self._blend(self.velo[k], sel1)[0] for k in range(3)], F)
                with np.errstate(all="ignore"):
                    fx, fy, fz = (velo_cur - velo_start).astype(F)
                    x1 = c_st[2] * fx - s_st[2] * fz
                    y1 = fy
                    z1 = s_st[2] * fx + c_st[2] * fz
                    x2 = x1
                    y2 = c_st[1] * y1 + s_st[1] * z1
                    z2 = -s_st[1] * y1 + c_st[1] * z1
                    carry["velo_from_start"] = np.array([c_st[0] * x2 + s_st[0] * y2, -s_st[0] * x2 + c_st[0] * y2, z2], F)
                # TransformToStartIMU of points 1 .. S-1 (FA:538-563)
                r, p, y = cur[1:, 0], cur[1:, 1], cur[1:, 2]
                cr, sr, cp, sp, cy, sy = cosf(r), sinf(r), cosf(p), sinf(p), cosf(y), sinf(y)
                px, py, pz = loam[1:, 0], loam[1:, 1], loam[1:, 2]
                zero = F(0)  # imuShiftFromStart*Cur: ShiftToStartIMU is never called
                with np.errstate(all="ignore"):
                    x1 = cr * px - sr * py
                    y1 = sr * px + cr * py
                    z1 = pz
                    x2 = x1
                    y2 = cp * y1 - sp * z1
                    z2 = sp * y1 + cp * z1
                    x3 = cy * x2 + sy * z2
                    y3 = y2
                    z3 = -sy * x2 + cy * z2
                    x4 = c_st[2] * x3 - s_st[2] * z3
                    y4 = y3
                    z4 = s_st[2] * x3 + c_st[2] * z3
                    x5 = x4
                    y5 = c_st[1] * y4 + s_st[1] * z4
                    z5 = -s_st[1] * y4 + c_st[1] * z4
                    loam[1:, 0] = c_st[0] * x5 + s_st[0] * y5 + zero
                    loam[1:, 1] = -s_st[0] * x5 + c_st[0] * y5 + zero
                    loam[1:, 2] = z5 + zero
        self.pointer_last_iteration = self.pointer_last  # FA:788
        return loam


def loam_swap(seg, orientation, scan_period):
    """FA:573-596 for every point: the LOAM-frame swap, the orientation with the halfPassed latch,
    relTime, intensity = int(intensity) + scan_period * relTime. Returns (cloud [S, 4], relTime)."""
    seg = np.asarray(seg, F).reshape(-1, 4)
    start, end, diff = (F(v) for v in orientation)
    scan_period = F(scan_period)
    out = np.empty_like(seg)
    out[:, 0], out[:, 1], out[:, 2] = seg[:, 1], seg[:, 2], seg[:, 0]
    if len(seg) == 0:
        return out, np.zeros(0, F)
    ori = -atan2f(out[:, 0], out[:, 2])
    od = ori.astype(D)
    # !halfPassed branch (FA:579-582)
    o1 = np.where(od < D(start) - PI / D(2), (od + D(2) * PI).astype(F),
                  np.where(od > D(start) + PI * D(3) / D(2), (od - D(2) * PI).astype(F), ori)).astype(F)
    passed = (o1 - start).astype(D) > PI  # FA:584
    first = int(passed.argmax()) if passed.any() else len(seg)  # the point that sets the latch
    # halfPassed branch (FA:586-591)
    o2 = (od + D(2) * PI).astype(F)
    o2d = o2.astype(D)
    o2 = np.where(o2d < D(end) - PI * D(3) / D(2), (o2d + D(2) * PI).astype(F),
                  np.where(o2d > D(end) + PI / D(2), (o2d - D(2) * PI).astype(F), o2)).astype(F)
    o = np.where(np.arange(len(seg)) <= first, o1, o2).astype(F)
    with np.errstate(all="ignore"):
        rel = ((o - start) / diff).astype(F)
        out[:, 3] = np.trunc(seg[:, 3]).astype(F) + scan_period * rel
    return out, rel


def curvature(loam):
    """cloudCurvature of calculateSmoothnessOurs (FA:817-848) on [5, S - 5); zeros elsewhere."""
    p = np.asarray(loam, F)
    S = len(p)
    cv = np.zeros(S, F)
    if S < 11:
        return cv
    idx = np.arange(5, S - 5)
    d = np.zeros((len(idx), 3), F)
    for m in range(-5, 6):  # diffX += points[i + m].x in the order i-5 .. i+5, one float add each
        d = d + p[idx + m, :3]
    d = d - F(11) * p[idx, :3]
    with np.errstate(all="ignore"):
        num = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        den = np.sqrt(p[idx, 0] * p[idx, 0] + p[idx, 1] * p[idx, 1] + p[idx, 2] * p[idx, 2])
        cv[idx] = num / den / F(10)
    return cv
