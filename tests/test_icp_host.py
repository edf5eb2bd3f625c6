"""CPU checks of the loop closure's alignment on the host (no device): llsr_icp_align_host against
the restatement of DESIGN.md §16 in tests/_icp_loop.py on every case of tests/_icp_cases.py, bit for
bit (T and the fitness as bit patterns), and the recovery of a planted drift."""
import numpy as np
import pytest

import _icp_cases as K
import _icp_loop as R
import llsr
from _icp_cases import check_result

# the project's pose tolerance (the scan-to-map and smoke checks use the same 1e-4)
POSE_TOL = 1e-4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_expectation(name, want):
    """What the case was built to reach (the restatement's own result is checked, not the library's)."""
    state = K.get(name)[3]
    if state is not None:
        assert R.STATES[want["state"]] == state, R.STATES[want["state"]]
    if state == "no_correspondences":
        assert want["iterations"] == 0 and not want["converged"]
        assert np.array_equal(want["T"], np.eye(4, dtype=np.float32))
    if name in K.KEPT:
        assert want["n_pairs_last"] == K.KEPT[name]
    if name == "subset":
        assert want["iterations"] == 1
    if name == "odd_points":
        s, t = K.get(name)[:2]
        # the NaN and the 2e6 m source points are in no pair and not in the fitness mean
        assert want["n_pairs_last"] == len(s) - 2
        ok = R.in_grid(s[:, :3])
        assert ok.sum() == len(s) - 2
        idx, d2 = R.nearest(want["aligned"][ok, :3], t[:, :3])
        assert want["fitness"] == float(R.seq_sum(d2, np.float64)) / int(ok.sum())


@pytest.mark.parametrize("name", list(K.CASES))
def test_align_host_bit_equal_to_the_restatement(name):
    s, t, over, _ = K.get(name)
    want = K.expected(name)
    check_expectation(name, want)
    got = llsr.icp_align_host(s, t, llsr.loop_config("hdl64e", **over))
    print(f"{name}: n_src {len(s)} n_tgt {len(t)} iterations {want['iterations']} state {R.STATES[want['state']]} "
          f"pairs {want['n_pairs_last']} fitness {want['fitness']:.3g}")
    check_result(got, want, name)


def test_recovery_of_the_planted_drift():
    """The recovery scene: the corrected last pose T * (drifted pose) against the true pose."""
    sc = K.scene()
    want = K.expected("recovery")
    assert want["converged"]
    got_pose, true_pose = sc.corrected(want["T"])
    err = float(np.abs(got_pose - true_pose).max())
    s, t = K.get("recovery")[:2]
    got = llsr.icp_align_host(s, t, llsr.loop_config("hdl64e"))
    print(f"recovery: restatement |corrected - true| = {err:.3g} after {want['iterations']} iterations, "
          f"state {R.STATES[want['state']]}, fitness {want['fitness']:.3g}")
    assert np.array_equal(_bits(got["T"]), _bits(want["T"]))
    lib_pose, _ = sc.corrected(got["T"])
    assert float(np.abs(lib_pose - true_pose).max()) <= POSE_TOL
    assert err <= POSE_TOL
    # the drift really was there: the uncorrected pose is far off
    assert float(np.abs(K.pose_matrix(sc.poses[-1]) - true_pose).max()) > 0.1


def test_align_host_bad_arguments():
    z = np.zeros((3, 4), np.float32)
    cfg = llsr.loop_config()
    import ctypes as C
    res = llsr._abi.IcpResult()
    L = llsr.lib()
    assert L.llsr_icp_align_host(None, 3, z.ctypes.data, 3, C.byref(cfg), C.byref(res), None) == -22
    assert L.llsr_icp_align_host(z.ctypes.data, 3, z.ctypes.data, -1, C.byref(cfg), C.byref(res), None) == -22
    assert L.llsr_icp_align_host(z.ctypes.data, 3, z.ctypes.data, 3, None, C.byref(res), None) == -22
    assert L.llsr_icp_align_host(z.ctypes.data, 3, z.ctypes.data, 3, C.byref(cfg), C.byref(res), None) == 0
