"""CPU tests of the /odom2 input and updateInitialGuess on the host side of the library
(llsr_odom_init / llsr_odom_callback / llsr_update_initial_guess; featureAssociation.cpp:354-383,
2370-2402) against the independent Python restatement tests/_odom_guess.py, plus the analytic pins
that hold whatever evaluation order Eigen takes, and the check that the overwrite is decisive on the
drives the GPU tests use (tests/test_gpu_odom_guess.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import _odom_guess
import llsr
import oracle_py
from llsr import _abi, synth


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(sample, tsum):
    g = llsr.update_initial_guess(sample, tsum)
    o = _odom_guess.update_initial_guess(sample, tsum)
    return np.array_equal(_bits(g), _bits(o)), g, o


def test_update_initial_guess_bit_exact_random():
    rng = np.random.default_rng(20240611)
    bad = []
    for k in range(3000):
        tsum = np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-50, 50, 3)]).astype(np.float32)
        sample = np.concatenate([rng.uniform(-0.3, 0.3, 2), rng.uniform(-math.pi, math.pi, 1),
                                 rng.uniform(-100, 100, 3)]).astype(np.float32)
        ok, g, o = _same(sample, tsum)
        if not ok:
            bad.append(f"case {k}: {g} vs {o}")
    assert not bad, f"{len(bad)} of 3000 differ:\n" + "\n".join(bad[:10])


def _sum_encoding(roll, pitch, yaw, x, y, z):
    """A transformSum whose rotation_matrix_last (FA:2378-2380) is the sample's rotation_matrix_now and
    whose translation cancels the sample's position: yaw -> [1], pitch -> [0], roll -> [2]."""
    return np.array([pitch, yaw, roll, y, z, x], np.float32)


HAND_CASES = [
    ("zero", (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0)),
    ("yaw +pi", (0, 0, math.pi, 1, 2, 3), (0.1, -0.2, 0.3, 1, 2, 3)),
    ("yaw -pi", (0, 0, -math.pi, 1, 2, 3), (0.1, -0.2, 0.3, 1, 2, 3)),
    ("pitch +pi/2", (0.1, math.pi / 2, 0.4, 1, 2, 3), (0, 0, 0, 0, 0, 0)),
    ("pitch -pi/2", (0.1, -math.pi / 2, 0.4, 1, 2, 3), (0.2, 0.1, -0.1, 3, 2, 1)),
    ("1e4 m", (0.01, -0.02, 1.0, 1e4, -1e4, 1e4), (0.02, 1.0, 0.01, -1e4 + 0.3, 1e4 - 0.2, 1e4 + 0.1)),
    ("sample == sum", (0.05, -0.03, 0.7, 12.5, -3.25, 0.5), tuple(_sum_encoding(0.05, -0.03, 0.7, 12.5, -3.25, 0.5))),
]


@pytest.mark.parametrize("name,sample,tsum", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_update_initial_guess_bit_exact_hand_cases(name, sample, tsum):
    ok, g, o = _same(np.array(sample, np.float32), np.array(tsum, np.float32))
    assert ok, f"{name}: {g} vs {o}"
    assert np.all(np.isfinite(g))


def test_zero_sample_zero_sum_is_twice_the_lever_arm():
    g = llsr.update_initial_guess(np.zeros(6, np.float32), np.zeros(6, np.float32))
    want = np.array([0, 0, 0, 0, np.float32(-0.0754), np.float32(-0.16)], np.float32)
    assert np.array_equal(g, want), g


@pytest.mark.parametrize("psi", [0.3, -1.1, 2.5])
def test_pure_yaw_lands_negated_in_entry_1(psi):
    g = llsr.update_initial_guess([0, 0, psi, 0, 0, 0], np.zeros(6, np.float32))
    assert abs(g[1] + psi) < 1e-6 and abs(g[0]) < 1e-6 and abs(g[2]) < 1e-6, g


@pytest.mark.parametrize("theta", [0.3, -1.1, 2.5])
def test_sum_entry_1_comes_back_in_entry_1(theta):
    tsum = np.array([0, theta, 0, 0, 0, 0], np.float32)
    g = llsr.update_initial_guess(np.zeros(6, np.float32), tsum)
    assert abs(g[1] - theta) < 1e-6, g


def test_update_initial_guess_null_arguments():
    L = llsr.lib()
    s, a = _abi.OdomSample(), np.zeros(6, np.float32)
    assert L.llsr_update_initial_guess(None, a.ctypes.data, a.ctypes.data) == -22
    assert L.llsr_update_initial_guess(C.byref(s), None, a.ctypes.data) == -22
    assert L.llsr_update_initial_guess(C.byref(s), a.ctypes.data, None) == -22


# ---- odomCallback ----

def _msg(q, p):
    return np.array(list(q) + list(p) + [0.0] * 6, np.float64)


def test_odom_init_is_the_zero_sample():
    st = llsr.odom_init()
    assert st.initial_iter == 0 and st.n_msgs == 0 and list(st.origin) == [0.0, 0.0, 0.0]
    assert np.array_equal(st.last.as_array(), np.zeros(6, np.float32))


def test_odom_callback_first_and_second_message():
    st = llsr.odom_init()
    q = synth.odom_message(70)[0:4]
    s1 = llsr.odom_callback(st, _msg(q, (10.0, -4.0, 2.0)))
    rpy = np.array(_odom_guess.get_rpy(q)).astype(np.float32)
    assert np.array_equal(s1[0:3], rpy) and np.array_equal(s1[3:6], np.zeros(3, np.float32))
    assert np.any(rpy != 0)
    s2 = llsr.odom_callback(st, _msg((0, 0, 0, 1), (10.5, -4.25, 2.125)))
    assert np.array_equal(s2, np.array([0, 0, 0, 0.5, -0.25, 0.125], np.float32))
    assert st.n_msgs == 2 and st.initial_iter == 1


def test_odom_callback_unnormalised_quaternion():
    q = synth.odom_message(200)[0:4]
    a = llsr.odom_callback(llsr.odom_init(), _msg(q, (0, 0, 0)))
    b = llsr.odom_callback(llsr.odom_init(), _msg(4.0 * q, (0, 0, 0)))  # a power of two: exact scaling
    assert np.array_equal(a, b)
    c = llsr.odom_callback(llsr.odom_init(), _msg(3.7 * q, (0, 0, 0)))
    assert np.allclose(a, c, atol=1e-6)


def test_odom_callback_bit_exact_random():
    rng = np.random.default_rng(77)
    bad = 0
    for _ in range(1000):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        p0, p1 = rng.uniform(-100, 100, 3), rng.uniform(-100, 100, 3)
        st, ref = llsr.odom_init(), _odom_guess.OdomInput()
        for p in (p0, p1):
            g, o = llsr.odom_callback(st, _msg(q, p)), ref.callback(_msg(q, p))
            bad += not np.array_equal(_bits(g), _bits(o))
    assert bad == 0


def test_odom_callback_null_arguments():
    L = llsr.lib()
    st, m = _abi.OdomState(), _abi.OdometryMsg()
    assert L.llsr_odom_init(None) == -22
    assert L.llsr_odom_callback(None, C.byref(m)) == -22
    assert L.llsr_odom_callback(C.byref(st), None) == -22


def test_synth_odom_message_varies_in_six_dof():
    a, b = synth.odom_message(1), synth.odom_message(2)
    assert np.array_equal(a, synth.odom_message(1))
    sa = _odom_guess.OdomInput()
    sa.callback(a)
    s = sa.callback(b)
    assert np.all(s != 0), s
    assert abs(np.linalg.norm(a[0:4]) - 1.0) < 1e-12


# ---- the overwrite is decisive on the drives of the GPU tests ----

def test_overwrite_is_decisive_on_the_gpu_drives():
    """On VLP-16 seeds [1, 65, 130], 4 frames (slot 2's first message before frame 2), the faithful
    chain's transformCur differs from the LM's own on every non-initial frame and its transformSum
    from the lm_applied chain's: otherwise a green GPU comparison would show nothing."""
    cfg = llsr.default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    for slot, s0 in enumerate([1, 65, 130]):
        samples = _odom_guess.drive_samples(s0, 4, first_message=2 if slot == 2 else 0)
        fa, lm = _odom_guess.FaithfulOracleOdometry(cfg), oracle_py.OracleOdometry(cfg)
        for k in range(4):
            scan = synth.make_scan(s0 + k, "vlp16", motion=True)
            f, o = fa.process(scan, samples[k]), lm.process(scan)
            if k == 0:
                assert f["lm"] is None and not f["transform_cur"].any()
                continue
            assert f["lm"] is not None and f["lm"]["skipped"] == 0
            assert not np.array_equal(f["transform_lm"], f["transform_cur"]), (s0, k)
            assert not np.array_equal(f["transform_sum"], o["transform_sum"]), (s0, k)
