"""CPU: the host entry points of the use_imu_undistortion == true branches
(llsr_integrate_transformation_imu, llsr_transform_to_end_imu, llsr_first_scan_imu: the functions of
csrc/llsr_odo.h that k_odo_finish_imu runs, compiled for the host) against the numpy restatement of
the reference's lines (tests/_imu_undistortion.py).

Bar: bit-exact against the restatement; the analytic pins hold for any evaluation order.
"""
import numpy as np

import _imu_undistortion as R
import llsr
import oracle_py
from _imu_cases import bits_equal

F = np.float32
D = np.float64
PI = np.pi


def _report(rng, amp=PI):
    return {"start": rng.uniform(-amp, amp, 3).astype(F), "cur": rng.uniform(-amp, amp, 3).astype(F)}


def _cloud(rng, n):
    p = np.empty((n, 4), F)
    p[:, :3] = rng.uniform(-60, 60, (n, 3))
    p[:, 3] = rng.integers(0, 16, n) + rng.uniform(0, 0.0999, n)  # ring + relTime / 10
    return p


def _pose(rng, ang=PI, lin=3.0):
    return np.concatenate([rng.uniform(-ang, ang, 3), rng.uniform(-lin, lin, 3)]).astype(F)


def test_integrate_imu_equals_restatement():
    """2000 seeded cases: transformSum's and the IMU's angles up to +-pi (the LM's transformCur up to
    +-0.5 rad and +-pi in a tenth of the cases), plus reports of all zeros."""
    rng = np.random.default_rng(1801)
    bad = []
    for k in range(2000):
        ts = _pose(rng, lin=50.0)
        tc = _pose(rng, PI if k % 10 == 0 else 0.5)
        rep = R.ZERO_REPORT if k % 50 == 1 else _report(rng)
        got, exp = llsr.integrate_transformation(ts, tc, imu=rep), R.integrate_transformation_imu(ts, tc, rep)
        if not bits_equal(got, exp):
            bad.append((k, got, exp))
    assert not bad, (len(bad), bad[:3])


def test_first_scan_add_equals_restatement():
    rng = np.random.default_rng(1802)
    for _ in range(200):
        ts, rep = _pose(rng), _report(rng)
        got, exp = llsr.first_scan_imu(ts, rep), R.first_scan(ts, rep)
        assert bits_equal(got, exp)
        assert bits_equal(got[[1, 3, 4, 5]], ts[[1, 3, 4, 5]])
    assert bits_equal(llsr.first_scan_imu(np.zeros(6, F), R.ZERO_REPORT), np.zeros(6, F))


def test_transform_to_end_imu_equals_restatement():
    """150 reports x 24 points (3600 points), clouds of 0 and 1 points, zero reports, in-place calls."""
    rng = np.random.default_rng(1803)
    for k in range(150):
        rep = R.ZERO_REPORT if k % 25 == 1 else _report(rng)
        tc = _pose(rng, 0.5 if k % 5 else PI)
        for n in ((24,) if k % 10 else (24, 0, 1)):
            p = _cloud(rng, n)
            exp = R.transform_to_end_imu(tc, rep, p)
            got = llsr.transform_to_end(tc, p, imu=rep)
            assert bits_equal(got, exp), (k, n)
            q = p.copy()
            assert llsr.transform_to_end(tc, q, imu=rep, out=q) is q  # out == in
            assert bits_equal(q, exp), (k, n, "in place")
            assert np.array_equal(got[:, 3], np.trunc(p[:, 3]))


def _quadrant(a):
    return (np.sin(D(a)) > 0, np.cos(D(a)) > 0)


def test_atan2_quadrants():
    """One hand-made case per quadrant of each of PluginIMURotation's two atan2: with an IMU at rest
    (zero report) acy / acz come back in the quadrant of transformSum's ry / rz."""
    seen = {1: set(), 2: set()}
    for which in (1, 2):
        for ang in (0.6, 2.4, -0.6, -2.4):
            ts = np.array([0.2, 0.1, -0.15, 1.0, 2.0, 3.0], F)
            ts[which] = ang
            tc = np.zeros(6, F)
            got = llsr.integrate_transformation(ts, tc, imu=R.ZERO_REPORT)
            assert bits_equal(got, R.integrate_transformation_imu(ts, tc, R.ZERO_REPORT))
            assert _quadrant(got[which]) == _quadrant(ang) and abs(got[which] - F(ang)) < 1e-5
            seen[which].add(_quadrant(got[which]))
    assert all(len(s) == 4 for s in seen.values())
    # and with a moving IMU: each quadrant of both outputs is reached and restated bit for bit
    rng = np.random.default_rng(1804)
    hit = {1: set(), 2: set()}
    for _ in range(64):
        ts, tc, rep = _pose(rng), _pose(rng, 0.3), _report(rng)
        got = llsr.integrate_transformation(ts, tc, imu=rep)
        assert bits_equal(got, R.integrate_transformation_imu(ts, tc, rep))
        for which in (1, 2):
            hit[which].add(_quadrant(got[which]))
    assert all(len(s) == 4 for s in hit.values())


def test_zero_report_tail_is_identity():
    """Analytic pin: with a zero report every plane rotation of the tail is x * 1 - y * 0, so finite
    points come back numerically equal (a -0 coordinate may come back +0: array_equal, not bits)."""
    rng = np.random.default_rng(1805)
    tc = _pose(rng, 0.3)
    p = _cloud(rng, 500)
    p[:8, :3] = [[0, 0, 0], [-0.0, 1, 2], [1, -0.0, 2], [1, 2, -0.0], [1e-30, -1e-30, 1e30], [-5, 0, 0], [0, -5, 0],
                 [0, 0, -5]]
    got = llsr.transform_to_end(tc, p, imu=R.ZERO_REPORT)
    assert np.array_equal(got, llsr.transform_to_end(tc, p))
    assert np.array_equal(got, oracle_py.transform_to_end(tc, p))
    z = np.zeros(6, F)  # transformCur 0: TransformToEnd itself returns the point (and int(intensity))
    got = llsr.transform_to_end(z, p, imu=R.ZERO_REPORT)
    assert np.array_equal(got[:, :3], p[:, :3]) and np.array_equal(got[:, 3], np.trunc(p[:, 3]))


def _rot(rx, ry, rz):
    """The rotation LOAM's (rx, ry, rz) stand for, R = Ry(ry) Rx(rx) Rz(rz), in double."""
    cx, sx, cy, sy, cz, sz = (f(D(v)) for v in (rx, ry, rz) for f in (np.cos, np.sin))
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def test_start_equals_last_plugin_is_identity():
    """Analytic pin: with imu*Start == imu*Last the plugged rotation is the input rotation
    (R_last^-1 R_start = I). Compared as rotation matrices built in double from the angles (the angles
    themselves are ill-conditioned near rx = +-pi/2 and wrap at +-pi), max-abs matrix entry. 400 seeded
    cases, angles up to +-pi (rx up to +-1.5). The plugin's input is the plain integrate's rotation
    (transformCur = 0), so only the plugin is pinned.

    The bound is not fixed in advance: it is the float rounding of the reference's own arithmetic on
    these cases, measured on the restatement alone before the library is called: twice the largest
    distance between the restatement evaluated in float and the same lines evaluated in double (twice:
    another evaluation order rounds differently, not more), plus the double evaluation's largest
    distance from the input, which must be analytic zero (< 1e-12). Figures of these cases: double
    restatement vs input 3.21e-15; float restatement vs double restatement 1.42e-06 (bound
    2.84e-06); the library's output vs input 1.42e-06."""
    rng = np.random.default_rng(1806)
    cases = []
    e_double = e_float = 0.0
    for _ in range(400):
        ts = np.zeros(6, F)
        ts[:3] = rng.uniform(-PI, PI, 3)
        ts[0] = rng.uniform(-1.5, 1.5)
        imu = rng.uniform(-PI, PI, 3).astype(F)
        mid = oracle_py.integrate_transformation(ts, np.zeros(6, F))[:3]
        bl = (imu[1], imu[2], imu[0])
        dd = R.plugin_imu_rotation(mid.astype(D), [D(v) for v in bl], [D(v) for v in bl], dtype=D)
        ff = R.plugin_imu_rotation(mid, bl, bl)
        e_double = max(e_double, np.abs(_rot(*dd) - _rot(*mid)).max())
        e_float = max(e_float, np.abs(_rot(*ff) - _rot(*dd)).max())
        cases.append((ts, imu, mid))
    assert e_double < 1e-12
    bound = 2 * e_float + e_double
    e_lib = 0.0
    for ts, imu, mid in cases:
        got = llsr.integrate_transformation(ts, np.zeros(6, F), imu={"start": imu, "cur": imu.copy()})
        e_lib = max(e_lib, np.abs(_rot(*got[:3]) - _rot(*mid)).max())
    print(f"start == last: double {e_double:.3g}, float {e_float:.3g}, bound {bound:.3g}, library {e_lib:.3g}")
    assert e_lib <= bound, (e_lib, bound)


def test_zero_report_transform_sum_equals_restatement_not_plain():
    """With a zero report transformSum goes through -asinf(sinf-products) and atan2f again, so it is
    not the plain integrate's bit for bit; the library equals the restatement there."""
    rng = np.random.default_rng(1807)
    differs = 0
    for _ in range(300):
        ts, tc = _pose(rng, lin=20.0), _pose(rng, 0.3)
        got = llsr.integrate_transformation(ts, tc, imu=R.ZERO_REPORT)
        assert bits_equal(got, R.integrate_transformation_imu(ts, tc, R.ZERO_REPORT))
        plain = llsr.integrate_transformation(ts, tc)
        assert bits_equal(got[3:], plain[3:])  # the translation is computed before the plugin
        differs += int(not bits_equal(got[:3], plain[:3]))
    assert differs > 0
