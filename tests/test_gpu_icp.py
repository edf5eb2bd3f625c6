"""GPU: llsr_icp_align (the loop closure's ICP as kernels, csrc/llsr_icp.hip) against
llsr_icp_align_host and the restatement of DESIGN.md §16 (tests/_icp_loop.py) on every case of
tests/_icp_cases.py, bit for bit, on one workspace reused across the cases (so every buffer grows and
is reused at a smaller size)."""
import numpy as np
import pytest

import _icp_cases as K
import llsr
from _icp_cases import check_result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def icp(require_gpu):
    w = llsr.Icp(0)
    yield w
    w.close()


def _host(r):
    r = dict(r)
    r["aligned"] = r["aligned"].cpu().numpy()
    return r


# the largest case first, so the later ones run in buffers larger than they need
ORDER = ["pairs_1361"] + [n for n in K.CASES if n != "pairs_1361"]


@pytest.mark.parametrize("name", ORDER)
def test_align_equals_host_and_restatement(icp, name):
    s, t, over, _ = K.get(name)
    cfg = llsr.loop_config("hdl64e", **over)
    got = _host(icp.align(s, t, cfg))
    check_result(got, K.expected(name), name)
    check_result(got, llsr.icp_align_host(s, t, cfg), name)


def test_two_calls_and_a_fresh_workspace_give_identical_bits(icp, require_gpu):
    s, t, over, _ = K.get("recovery")
    a, b = _host(icp.align(s, t)), _host(icp.align(s, t))
    w = llsr.Icp(0)
    c = _host(w.align(s, t))
    w.close()
    check_result(b, a, "second call")
    check_result(c, a, "fresh workspace")
    tm = icp.last_times()
    assert tm["corr_ms"] > 0 and tm["solve_ms"] > 0 and tm["total_ms"] >= tm["corr_ms"] + tm["solve_ms"]


def test_align_bad_arguments(icp):
    import ctypes as C
    import torch
    z = torch.zeros((4, 4), dtype=torch.float32, device="cuda:0")
    cfg, res, L = llsr.loop_config(), llsr._abi.IcpResult(), llsr.lib()
    p = C.c_void_p(z.data_ptr())
    assert L.llsr_icp_align(icp._w, None, 3, p, 3, C.byref(cfg), C.byref(res), None, None) == -22
    assert L.llsr_icp_align(icp._w, C.c_void_p(z.data_ptr() + 4), 3, p, 3, C.byref(cfg), C.byref(res), None, None) == -22
    assert L.llsr_icp_align(None, p, 3, p, 3, C.byref(cfg), C.byref(res), None, None) == -22
    assert L.llsr_icp_align(icp._w, p, 3, p, 3, C.byref(cfg), C.byref(res), None, None) == 0
    # a count above LLSR_ICP_MAX_POINTS is a bad argument of this call (the batch call answers -34);
    # it is refused before anything is read or launched, and the workspace stays usable
    big = 100000000 + 1
    assert L.llsr_icp_align(icp._w, p, big, p, 3, C.byref(cfg), C.byref(res), None, None) == -22
    assert L.llsr_icp_align(icp._w, p, 3, p, 3, C.byref(cfg), C.byref(res), None, None) == 0
    assert L.llsr_icp_align(icp._w, p, 3, p, big, C.byref(cfg), C.byref(res), None, None) == -22
    assert L.llsr_icp_align(icp._w, p, 3, p, 3, C.byref(cfg), C.byref(res), None, None) == 0


def test_empty_cloud_with_a_null_pointer(icp):
    import ctypes as C
    import torch
    z = torch.zeros((4, 4), dtype=torch.float32, device="cuda:0")
    cfg, L, p = llsr.loop_config(), llsr.lib(), C.c_void_p(z.data_ptr())
    for src, n_src, tgt, n_tgt in ((None, 0, p, 4), (p, 4, None, 0)):
        res = llsr._abi.IcpResult()
        assert L.llsr_icp_align(icp._w, src, n_src, tgt, n_tgt, C.byref(cfg), C.byref(res), None, None) == 0
        assert res.state == 5 and res.iterations == 0 and res.converged == 0


def test_interior_pointers_give_the_same_bits(icp):
    """Clouds that are rows 5.. and 3.. of larger device tensors (16-byte aligned addresses off the
    allocations' starts) against the same clouds in tensors of their own."""
    import torch
    s, t, over, _ = K.get("recovery")
    cfg = llsr.loop_config("hdl64e", **over)
    s, t = np.asarray(s, np.float32).reshape(-1, 4), np.asarray(t, np.float32).reshape(-1, 4)
    buf = torch.from_numpy(np.concatenate([np.full((5, 4), 7.0, np.float32), s])).to("cuda:0")
    buf2 = torch.from_numpy(np.concatenate([np.full((3, 4), -9.0, np.float32), t])).to("cuda:0")
    a, b = buf[5:], buf2[3:]
    assert a.data_ptr() == buf.data_ptr() + 80 and b.data_ptr() == buf2.data_ptr() + 48
    got = _host(icp.align(a, b, cfg))
    check_result(got, _host(icp.align(s, t, cfg)), "interior pointers")
    check_result(got, K.expected("recovery"), "interior pointers")
