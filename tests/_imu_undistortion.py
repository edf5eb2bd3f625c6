"""Independent restatement of FeatureAssociation's use_imu_undistortion == true branches for the
tests (the oracle states the switch-off branches only): featureAssociation.cpp = FA,

* `tail`: TransformToEnd's IMU tail (FA:1456-1483) after updateImuRollPitchYawStartSinCos (FA:491-498);
* `plugin_imu_rotation`: PluginIMURotation (FA:1492-1550);
* `integrate_transformation` / `integrate_transformation_imu`: integrateTransformation (FA:2537-2568)
  without and with the switch; `first_scan`: checkSystemInitialization's add (FA:2329-2332);
* `transform_to_end_imu`: the whole TransformToEnd with the switch on;
* `ImuOdometryChain`: runFeatureAssociation's per-scan order with the switch on (FA:2781-2796), in the
  shape of _odom_guess.FaithfulOracleOdometry, fed with a scan's feature outputs and IMU report.

Written from the reference's lines in numpy float32 (correctly rounded, never fused, like the
reference's x86-64 build) with the host glibc's sinf / cosf / asinf / atan2f through ctypes: the
reference calls sin / cos / asin / atan2 on float arguments, where <cmath>'s float overloads apply.
Every operand is wrapped as numpy.float32 so that no Python float widens an expression. The part of
TransformToEnd and integrateTransformation that does not depend on the switch is the oracle's
(oracle_py.transform_to_end / integrate_transformation). `dtype=numpy.float64` evaluates
PluginIMURotation in double with the double libm functions (for error figures, not for parity).

report: {"start": imuRoll / Pitch / YawStart, "cur": imuRoll / Pitch / YawCur of the last point}; the
pre-LM updateInitialGuess (FA:2786-2788) has copied cur to imuRoll / Pitch / YawLast before anything
here runs, and imuShiftFromStartX / Y / Z is 0 (ShiftToStartIMU is never called).
"""
import ctypes

import numpy as np

import _odom_guess
import oracle_py

F = np.float32
D = np.float64

_libm = ctypes.CDLL("libm.so.6")
for _name, _n, _t in (("sinf", 1, ctypes.c_float), ("cosf", 1, ctypes.c_float), ("asinf", 1, ctypes.c_float),
                      ("atan2f", 2, ctypes.c_float), ("sin", 1, ctypes.c_double), ("cos", 1, ctypes.c_double),
                      ("asin", 1, ctypes.c_double), ("atan2", 2, ctypes.c_double)):
    _f = getattr(_libm, _name)
    _f.restype = _t
    _f.argtypes = [_t] * _n


def _m(name, dtype, *a):
    """libm's `name` in the precision of dtype, on scalars."""
    f = getattr(_libm, name + "f" if dtype is F else name)
    return dtype(f(*(float(dtype(v)) for v in a)))


def tail(report, p6) -> np.ndarray:
    """FA:1458-1483 of rows (x6, y6, z6, int(intensity)); the intensity column passes through."""
    p = np.asarray(p6, F).reshape(-1, 4)
    roll_s, pitch_s, yaw_s = (F(v) for v in report["start"])
    roll_l, pitch_l, yaw_l = (F(v) for v in report["cur"])
    c_rs, c_ps, c_ys = (_m("cos", F, v) for v in (roll_s, pitch_s, yaw_s))  # FA:491-498
    s_rs, s_ps, s_ys = (_m("sin", F, v) for v in (roll_s, pitch_s, yaw_s))
    shift = F(0.0)  # imuShiftFromStartX / Y / Z
    x6, y6, z6 = p[:, 0], p[:, 1], p[:, 2]
    x7 = c_rs * (x6 - shift) - s_rs * (y6 - shift)
    y7 = s_rs * (x6 - shift) + c_rs * (y6 - shift)
    z7 = z6 - shift
    x8 = x7
    y8 = c_ps * y7 - s_ps * z7
    z8 = s_ps * y7 + c_ps * z7
    x9 = c_ys * x8 + s_ys * z8
    y9 = y8
    z9 = -s_ys * x8 + c_ys * z8
    c_yl, s_yl = _m("cos", F, yaw_l), _m("sin", F, yaw_l)
    c_pl, s_pl = _m("cos", F, pitch_l), _m("sin", F, pitch_l)
    c_rl, s_rl = _m("cos", F, roll_l), _m("sin", F, roll_l)
    x10 = c_yl * x9 - s_yl * z9
    y10 = y9
    z10 = s_yl * x9 + c_yl * z9
    x11 = x10
    y11 = c_pl * y10 + s_pl * z10
    z11 = -s_pl * y10 + c_pl * z10
    out = np.empty_like(p)
    out[:, 0] = c_rl * x11 + s_rl * y11
    out[:, 1] = -s_rl * x11 + c_rl * y11
    out[:, 2] = z11
    out[:, 3] = p[:, 3]
    assert out.dtype == F
    return out


def plugin_imu_rotation(bc, bl, al, dtype=F):
    """PluginIMURotation(bcx, bcy, bcz, blx, bly, blz, alx, aly, alz) -> (acx, acy, acz)."""
    T = dtype
    sbcx, sbcy, sbcz = (_m("sin", T, v) for v in bc)
    cbcx, cbcy, cbcz = (_m("cos", T, v) for v in bc)
    sblx, sbly, sblz = (_m("sin", T, v) for v in bl)
    cblx, cbly, cblz = (_m("cos", T, v) for v in bl)
    salx, saly, salz = (_m("sin", T, v) for v in al)
    calx, caly, calz = (_m("cos", T, v) for v in al)
    srx = (-sbcx*(salx*sblx + calx*caly*cblx*cbly + calx*cblx*saly*sbly)
           - cbcx*cbcz*(calx*saly*(cbly*sblz - cblz*sblx*sbly)
           - calx*caly*(sbly*sblz + cbly*cblz*sblx) + cblx*cblz*salx)
           - cbcx*sbcz*(calx*caly*(cblz*sbly - cbly*sblx*sblz)
           - calx*saly*(cbly*cblz + sblx*sbly*sblz) + cblx*salx*sblz))
    acx = -_m("asin", T, srx)
    srycrx = ((cbcy*sbcz - cbcz*sbcx*sbcy)*(calx*saly*(cbly*sblz - cblz*sblx*sbly)
              - calx*caly*(sbly*sblz + cbly*cblz*sblx) + cblx*cblz*salx)
              - (cbcy*cbcz + sbcx*sbcy*sbcz)*(calx*caly*(cblz*sbly - cbly*sblx*sblz)
              - calx*saly*(cbly*cblz + sblx*sbly*sblz) + cblx*salx*sblz)
              + cbcx*sbcy*(salx*sblx + calx*caly*cblx*cbly + calx*cblx*saly*sbly))
    crycrx = ((cbcz*sbcy - cbcy*sbcx*sbcz)*(calx*caly*(cblz*sbly - cbly*sblx*sblz)
              - calx*saly*(cbly*cblz + sblx*sbly*sblz) + cblx*salx*sblz)
              - (sbcy*sbcz + cbcy*cbcz*sbcx)*(calx*saly*(cbly*sblz - cblz*sblx*sbly)
              - calx*caly*(sbly*sblz + cbly*cblz*sblx) + cblx*cblz*salx)
              + cbcx*cbcy*(salx*sblx + calx*caly*cblx*cbly + calx*cblx*saly*sbly))
    with np.errstate(divide="ignore", invalid="ignore"):
        acy = _m("atan2", T, srycrx / _m("cos", T, acx), crycrx / _m("cos", T, acx))
        srzcrx = (sbcx*(cblx*cbly*(calz*saly - caly*salx*salz)
                  - cblx*sbly*(caly*calz + salx*saly*salz) + calx*salz*sblx)
                  - cbcx*cbcz*((caly*calz + salx*saly*salz)*(cbly*sblz - cblz*sblx*sbly)
                  + (calz*saly - caly*salx*salz)*(sbly*sblz + cbly*cblz*sblx)
                  - calx*cblx*cblz*salz) + cbcx*sbcz*((caly*calz + salx*saly*salz)*(cbly*cblz
                  + sblx*sbly*sblz) + (calz*saly - caly*salx*salz)*(cblz*sbly - cbly*sblx*sblz)
                  + calx*cblx*salz*sblz))
        crzcrx = (sbcx*(cblx*sbly*(caly*salz - calz*salx*saly)
                  - cblx*cbly*(saly*salz + caly*calz*salx) + calx*calz*sblx)
                  + cbcx*cbcz*((saly*salz + caly*calz*salx)*(sbly*sblz + cbly*cblz*sblx)
                  + (caly*salz - calz*salx*saly)*(cbly*sblz - cblz*sblx*sbly)
                  + calx*calz*cblx*cblz) - cbcx*sbcz*((saly*salz + caly*calz*salx)*(cblz*sbly
                  - cbly*sblx*sblz) + (caly*salz - calz*salx*saly)*(cbly*cblz + sblx*sbly*sblz)
                  - calx*calz*cblx*sblz))
        acz = _m("atan2", T, srzcrx / _m("cos", T, acx), crzcrx / _m("cos", T, acx))
    assert all(type(v) is T for v in (srx, srycrx, crycrx, srzcrx, crzcrx, acx, acy, acz))
    return acx, acy, acz


def integrate_transformation(transform_sum, transform_cur) -> np.ndarray:
    """FA:2537-2568 with the switch off: the oracle's."""
    return oracle_py.integrate_transformation(transform_sum, transform_cur)


def integrate_transformation_imu(transform_sum, transform_cur, report) -> np.ndarray:
    """FA:2537-2568 with the switch on: the translation from the un-plugged rx, ry, rz, then
    PluginIMURotation(rx, ry, rz, imuPitch / Yaw / RollStart, imuPitch / Yaw / RollLast)."""
    ts = oracle_py.integrate_transformation(transform_sum, transform_cur)
    st, la = report["start"], report["cur"]
    ts[0:3] = plugin_imu_rotation(ts[0:3], (st[1], st[2], st[0]), (la[1], la[2], la[0]))
    return ts


def first_scan(transform_sum, report) -> np.ndarray:
    ts = np.array(transform_sum, F)
    ts[0] = ts[0] + F(report["start"][1])
    ts[2] = ts[2] + F(report["start"][0])
    return ts


def transform_to_end_imu(transform_cur, report, xyzi) -> np.ndarray:
    a = np.ascontiguousarray(xyzi, F).reshape(-1, 4)
    if len(a) == 0:
        return a.copy()
    return tail(report, oracle_py.transform_to_end(transform_cur, a))


ZERO_REPORT = {"start": np.zeros(3, F), "cur": np.zeros(3, F)}


class ImuOdometryChain:
    """One slot's runFeatureAssociation with use_imu_undistortion == true. process() takes the scan's
    feature outputs (loam_xyzi, sharp_ind, flat_ind, less_sharp_ind, less_flat_xyzi; the oracle's or the
    device's), its IMU report after the feature stage, and, for a slot whose transformCur the /odom2
    guess overwrites (llsr_odometry_batch_odom's flag), the sample."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.shadow = oracle_py.shadow_points()
        self.tcur, self.tsum, self.tlm = np.zeros(6, F), np.zeros(6, F), np.zeros(6, F)
        self.deg = 0
        self.corner_last = self.surf_last = None
        self.frames = 0

    def process(self, r, report, sample=None) -> dict:
        loam = np.asarray(r["loam_xyzi"], F).reshape(-1, 4)
        sharp = loam[r["sharp_ind"]]
        flat = np.concatenate([loam[r["flat_ind"]], self.shadow])
        less_sharp, less_flat = loam[r["less_sharp_ind"]], np.asarray(r["less_flat_xyzi"], F).reshape(-1, 4)
        out = {"features": r}
        self.tlm = np.zeros(6, F)
        if self.corner_last is None:  # checkSystemInitialization (FA:2291-2335), then `continue`
            self.corner_last = less_sharp.copy()
            self.surf_last = np.concatenate([less_flat, self.shadow])
            self.tsum = first_scan(self.tsum, report)
            out["lm"] = None
            out["corner_scan"] = out["surf_scan"] = None
        else:
            if sample is not None:  # FA:2786-2788: the LM starts from the guess
                self.tcur = _odom_guess.update_initial_guess(sample, self.tsum)
            lm = oracle_py.scan2scan(self.cfg, sharp, flat, self.corner_last, self.surf_last, self.tcur, self.deg)
            self.tcur, self.deg = lm["transform_cur"].copy(), lm["is_degenerate"]     # updateTransformation
            if sample is not None:                                                     # FA:2790
                self.tlm = self.tcur.copy()
                self.tcur = _odom_guess.update_initial_guess(sample, self.tsum)
            self.tsum = integrate_transformation_imu(self.tsum, self.tcur, report)    # FA:2792
            self.corner_last = transform_to_end_imu(self.tcur, report, less_sharp)    # publishCloudsLast
            self.surf_last = np.concatenate([transform_to_end_imu(self.tcur, report, less_flat), self.shadow])
            out["lm"] = lm
            out["corner_scan"] = transform_to_end_imu(self.tcur, report, sharp)
            out["surf_scan"] = transform_to_end_imu(self.tcur, report, flat)
        self.frames += 1
        out.update(frames=self.frames, transform_cur=self.tcur.copy(), transform_sum=self.tsum.copy(),
                   transform_lm=self.tlm.copy(), corner_last=self.corner_last, surf_last=self.surf_last)
        return out
