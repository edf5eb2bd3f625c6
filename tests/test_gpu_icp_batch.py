"""GPU: llsr_icp_align_batch (DESIGN.md §16 "Batch form") — every case of tests/_icp_cases.py as ONE
batch of 20 problems with a configuration per problem, against the restatement (tests/_icp_loop.py) and
llsr_icp_align_host, bit for bit; then the invariants of the batch form: the order of the problems, the
batch size (the table size of a problem's grid follows the largest target of its batch, and no result
depends on it), a reused workspace, the one-pass exit and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import _icp_cases as K
import llsr
from _icp_cases import check_result

pytestmark = pytest.mark.gpu

NAMES = list(K.CASES)


def _host(r):
    r = dict(r)
    r["aligned"] = r["aligned"].cpu().numpy()
    return r


def _batch(icp, names):
    cases = [K.get(n) for n in names]
    cfgs = [llsr.loop_config("hdl64e", **c[2]) for c in cases]
    return [_host(r) for r in icp.align_batch([c[0] for c in cases], [c[1] for c in cases], cfgs)]


@pytest.fixture(scope="module")
def icp(require_gpu):
    w = llsr.Icp(0)
    yield w
    w.close()


@pytest.fixture(scope="module")
def whole(icp):
    """The case table as one batch, run once; (results by name, passes of the loop)."""
    got = _batch(icp, NAMES)
    return dict(zip(NAMES, got)), icp.last_passes()


def test_whole_case_table_in_one_batch(whole):
    got, passes = whole
    assert len(got) == 20
    for name in NAMES:
        s, t, over, want = K.get(name)
        check_result(got[name], K.expected(name), name)
        check_result(got[name], llsr.icp_align_host(s, t, llsr.loop_config("hdl64e", **over)), name)
    its = [got[n]["iterations"] for n in NAMES]
    # problems that stop in the first pass next to ones that run tens of passes; the loop makes as
    # many passes as the longest problem has iterations
    assert min(its) == 0 and max(its) >= 10 and passes == max(its)
    assert {got[n]["state"] for n in NAMES} == {1, 2, 3, 4, 5}


def test_order_and_batch_size_do_not_change_a_bit(icp, whole):
    got, _ = whole
    rev = dict(zip(NAMES[::-1], _batch(icp, NAMES[::-1])))
    for name in NAMES:
        check_result(rev[name], got[name], f"{name} reversed")
        check_result(_batch(icp, [name])[0], got[name], f"{name} as P = 1")


def test_workspace_reuse_small_batch_then_single_call(icp, whole):
    got, _ = whole
    small = sorted(NAMES, key=lambda n: len(K.get(n)[0]) + len(K.get(n)[1]))[:2]
    for name, r in zip(small, _batch(icp, small)):
        check_result(r, got[name], f"{name} after the large batch")
    s, t, over, _ = K.get("recovery")
    check_result(_host(icp.align(s, t, llsr.loop_config("hdl64e", **over))), got["recovery"], "single call after batches")
    tm = icp.last_times()
    assert tm["corr_ms"] > 0 and tm["total_ms"] >= tm["corr_ms"] + tm["solve_ms"]


def test_batch_of_first_pass_stops_returns_after_one_pass(icp, whole):
    got, _ = whole
    names = ["pairs_0", "empty_target"]
    for name, r in zip(names, _batch(icp, names)):
        check_result(r, got[name], name)
        assert r["iterations"] == 0 and r["state"] == 5
    assert icp.last_passes() == 1
    tm = icp.last_times()
    assert tm["total_ms"] >= tm["corr_ms"] + tm["solve_ms"] > 0


def test_batch_bad_arguments(icp):
    import torch
    z = torch.zeros((8, 4), dtype=torch.float32, device="cuda:0")
    L, p = llsr.lib(), C.c_void_p(z.data_ptr())
    cfgs, res = (llsr._abi.LoopConfig * 2)(llsr.loop_config(), llsr.loop_config()), (llsr._abi.IcpResult * 2)()

    def call(w, P, src, so, tgt, to, n_cfgs, out=None):
        so, to = np.asarray(so, np.int64), np.asarray(to, np.int64)
        return L.llsr_icp_align_batch(w, P, src, so.ctypes.data, tgt, to.ctypes.data, cfgs, n_cfgs, res, out, None)

    ok = [0, 4, 8]
    assert call(icp._w, 2, p, ok, p, ok, 2) == 0
    assert call(icp._w, 2, p, ok, p, ok, 1) == 0
    assert call(None, 2, p, ok, p, ok, 2) == -22
    assert call(icp._w, 0, p, ok, p, ok, 1) == -22                      # P < 1
    assert call(icp._w, 2, p, [0, 5, 4], p, ok, 2) == -22               # decreasing offsets
    assert call(icp._w, 2, p, ok, p, [4, 4, 3], 2) == -22
    assert call(icp._w, 3, p, [0, 2, 4, 8], p, [0, 2, 4, 8], 2) == -22  # n_cfgs not in {1, P}
    assert call(icp._w, 2, C.c_void_p(z.data_ptr() + 4), ok, p, ok, 2) == -22  # misaligned clouds
    assert call(icp._w, 2, p, ok, p, ok, 2, C.c_void_p(z.data_ptr() + 8)) == -22
    assert call(icp._w, 2, None, ok, p, ok, 2) == -22
    big = 100000000  # LLSR_ICP_MAX_POINTS
    assert call(icp._w, 2, p, [0, 4, big + 5], p, ok, 2) == -34         # a problem above LLSR_ICP_MAX_POINTS
    assert call(icp._w, 2, p, ok, p, ok, 2) == 0                        # the workspace is still usable
