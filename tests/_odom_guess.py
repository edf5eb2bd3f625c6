"""Independent restatement of FeatureAssociation's /odom2 path for the tests: odomCallback
(featureAssociation.cpp:354-383), updateInitialGuess (FA:2370-2402) and runFeatureAssociation's
per-scan order with the overwrite in place (FA:2781-2796), written from the reference lines in
pure Python floats (IEEE double, no FMA) with numpy.float32 narrowing where the reference's
members are float. math.atan2 / math.sqrt / math.asin / math.cos are the host glibc's; the
half-angle cos / sin pairs go through glibc's sincos, which is what GCC -O3 emits for them.

Eigen 3.3.7 evaluation order assumed (unpinned, Eigen is not available):
AngleAxisd products are quaternion products (SSE2 double specialisation), the result becomes a
matrix through toRotationMatrix, and a fixed-size 3-term dot product is (p0 + p1) + p2 when both
operands are contiguous and p0 + (p1 + p2) when one is strided.
"""
import ctypes
import math

import numpy as np

import oracle_py

_libm = ctypes.CDLL("libm.so.6")
_libm.sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
_libm.sincos.restype = None


def _sincos(a):
    s, c = ctypes.c_double(), ctypes.c_double()
    _libm.sincos(a, ctypes.byref(s), ctypes.byref(c))
    return s.value, c.value


def _f32(x) -> float:
    return float(np.float32(x))


def _angle_axis_quat(angle, axis):
    """Eigen::Quaterniond(Eigen::AngleAxisd(angle, Vector3d::Unit<axis>())) as (x, y, z, w)."""
    s, c = _sincos(0.5 * angle)
    v = [s * 0.0, s * 0.0, s * 0.0]
    v[axis] = s * 1.0
    return (v[0], v[1], v[2], c)


def _quat_product(a, b):
    """Eigen 3.3.7 quat_product<Architecture::SSE, double>: packets (x, y) and (z, w)."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    t1 = (aw * bx + ay * bz, aw * by + ay * bw)
    t2 = (az * bx - ax * bz, az * by - ax * bw)
    x = t1[0] - t2[1]
    y = t1[1] + t2[0]
    t1 = (aw * bz - ay * bx, aw * bw - ay * by)
    t2 = (az * bz + ax * bx, az * bw + ax * by)
    w = t1[1] - t2[0]
    z = t1[0] + t2[1]
    return (x, y, z, w)


def _to_rotation_matrix(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def _zyx_matrix(az, ay, ax):
    """AngleAxisd(az, UnitZ) * AngleAxisd(ay, UnitY) * AngleAxisd(ax, UnitX) assigned to a Matrix3d."""
    q = _quat_product(_quat_product(_angle_axis_quat(az, 2), _angle_axis_quat(ay, 1)), _angle_axis_quat(ax, 0))
    return _to_rotation_matrix(q)


def update_initial_guess(sample, transform_sum) -> np.ndarray:
    """transformCur after FA:2370-2402. sample: odomRoll, odomPitch, odomYaw, odomPosX, odomPosY,
    odomPosZ at odomPointerLast (floats); transform_sum: float[6]."""
    roll, pitch, yaw, px, py, pz = (_f32(v) for v in sample)
    ts = [_f32(v) for v in transform_sum]
    now = _zyx_matrix(yaw, pitch, roll)
    last = _zyx_matrix(ts[1], ts[0], ts[2])
    # rotation_matrix_last.transpose() * rotation_matrix_now: (i, j) = sum_k last(k, i) * now(k, j)
    prod = [[(last[0][i] * now[0][j] + last[1][i] * now[1][j]) + last[2][i] * now[2][j] for j in range(3)]
            for i in range(3)]
    r = [[prod[j][i] for j in range(3)] for i in range(3)]  # transposeInPlace
    odom_x = _f32(math.atan2(r[2][1], r[2][2]))
    odom_y = _f32(math.atan2(-r[2][0], math.sqrt(r[2][1] * r[2][1] + r[2][2] * r[2][2])))
    odom_z = _f32(math.atan2(r[1][0], r[0][0]))
    tc = [0.0] * 6
    tc[0], tc[1], tc[2] = odom_y, odom_z, odom_x
    body = (0.08, 0.0, 0.0377)
    glob = [now[i][0] * body[0] + (now[i][1] * body[1] + now[i][2] * body[2]) for i in range(3)]
    tv = (ts[5] - (px + body[0] + glob[0]), ts[3] - (py + body[1] + glob[1]), ts[4] - (pz + body[2] + glob[2]))
    tvb = [(last[0][i] * tv[0] + last[1][i] * tv[1]) + last[2][i] * tv[2] for i in range(3)]
    tc[5], tc[3], tc[4] = _f32(tvb[0]), _f32(tvb[1]), _f32(tvb[2])
    return np.array(tc, np.float32)


def get_rpy(q):
    """tf2::Matrix3x3(tf2::Quaternion(x, y, z, w)).getRPY (setRotation + getEulerYPR, solution 1)."""
    x, y, z, w = (float(v) for v in q)
    d = x * x + y * y + z * z + w * w
    s = 2.0 / d
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    m00, m10, m20, m21, m22 = 1.0 - (yy + zz), xy + wz, xz - wy, yz + wx, 1.0 - (xx + yy)
    if abs(m20) >= 1:
        return math.atan2(m21, m22), (math.pi / 2.0 if m20 < 0 else -math.pi / 2.0), 0.0
    pitch = -math.asin(m20)
    return (math.atan2(m21 / math.cos(pitch), m22 / math.cos(pitch)), pitch,
            math.atan2(m10 / math.cos(pitch), m00 / math.cos(pitch)))


class OdomInput:
    """odomCallback's members (FA:277-287, 354-383): only the latest ring entry is ever read. Before
    the first message the sample is the zero pose (the project's definition of "no message yet")."""

    def __init__(self):
        self.initial_iter = 0
        self.origin = (0.0, 0.0, 0.0)
        self.sample = np.zeros(6, np.float32)

    def callback(self, msg) -> np.ndarray:
        m = [float(v) for v in msg]
        roll, pitch, yaw = get_rpy(m[0:4])
        if self.initial_iter == 0:
            self.origin = (m[4], m[5], m[6])
            self.initial_iter += 1
        self.sample = np.array([roll, pitch, yaw, m[4] - self.origin[0], m[5] - self.origin[1],
                                m[6] - self.origin[2]], np.float64).astype(np.float32)
        return self.sample.copy()


class FaithfulOracleOdometry:
    """runFeatureAssociation (FA:2742-2853) as the node runs it: like oracle_py.OracleOdometry, with
    updateInitialGuess between updateTransformation and integrateTransformation (FA:2789-2796).
    `sample` (roll, pitch, yaw, x, y, z) is the latest /odom2 sample at the time of the scan: pass it
    to process() or set the attribute (OracleMapping calls process(xyzi) only)."""

    def __init__(self, cfg, pcl_voxel_order: bool = True):
        self.cfg = cfg
        self.ora = oracle_py.Oracle(cfg, pcl_voxel_order)
        self.shadow = oracle_py.shadow_points()
        self.tcur = np.zeros(6, np.float32)
        self.tsum = np.zeros(6, np.float32)
        self.tlm = np.zeros(6, np.float32)
        self.deg = 0
        self.corner_last = None
        self.surf_last = None
        self.frames = 0
        self.sample = np.zeros(6, np.float32)

    def process(self, xyzi, sample=None) -> dict:
        if sample is not None:
            self.sample = np.asarray(sample, np.float32)
        r = self.ora.process(xyzi)
        loam = r["loam_xyzi"]
        sharp = loam[r["sharp_ind"]]
        flat = np.concatenate([loam[r["flat_ind"]], self.shadow])
        less_sharp, less_flat = loam[r["less_sharp_ind"]], r["less_flat_xyzi"]
        out = {"features": r}
        if self.corner_last is None:  # checkSystemInitialization, then `continue` (FA:2781-2784)
            self.corner_last = less_sharp.copy()
            self.surf_last = np.concatenate([less_flat, self.shadow])
            out["lm"] = None
            out["corner_scan"] = out["surf_scan"] = None
        else:
            lm = oracle_py.scan2scan(self.cfg, sharp, flat, self.corner_last, self.surf_last, self.tcur, self.deg)
            self.tlm, self.deg = lm["transform_cur"].copy(), lm["is_degenerate"]      # updateTransformation
            self.tcur = update_initial_guess(self.sample, self.tsum)                   # updateInitialGuess
            self.tsum = oracle_py.integrate_transformation(self.tsum, self.tcur)       # integrateTransformation
            self.corner_last = oracle_py.transform_to_end(self.tcur, less_sharp)       # publishCloudsLast
            self.surf_last = np.concatenate([oracle_py.transform_to_end(self.tcur, less_flat), self.shadow])
            out["lm"] = lm
            out["corner_scan"] = oracle_py.transform_to_end(self.tcur, sharp)
            out["surf_scan"] = oracle_py.transform_to_end(self.tcur, flat)
        self.frames += 1
        out.update(frames=self.frames, transform_cur=self.tcur.copy(), transform_sum=self.tsum.copy(),
                   transform_lm=self.tlm.copy(), corner_last=self.corner_last, surf_last=self.surf_last)
        return out


def drive_samples(seed0: int, frames: int, first_message: int = 0):
    """The /odom2 samples a slot's drive sees: before frame k >= first_message the message
    synth.odom_message(seed0 + k) arrives; earlier frames see the zero sample. Returns frames x 6."""
    from llsr import synth
    inp, out = OdomInput(), []
    for k in range(frames):
        if k >= first_message:
            inp.callback(synth.odom_message(seed0 + k))
        out.append(inp.sample.copy())
    return out
