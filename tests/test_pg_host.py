"""CPU: the host pose graph (llsr_pg_create(LLSR_PG_HOST, ...): the loop bodies of csrc/llsr_pg.h run
serially over heap buffers) against tests/_pose_graph.py, the independent numpy restatement of
DESIGN.md §19 (dense normal equations, numpy.linalg.solve, the C library's trigonometry).

Pose tolerance. The systems mix weights of 1e8 (the odometry's translation variances of 1e-8) and ~1
(the loop factors), so the order of summation matters. The restatement's own spread — its estimate with
the factors summed in reversed order against forward order, over the graphs below, in the store's
layout in double, the largest over the graphs below — was measured at 8.9e-16 (metres / radians; 0 on
the two graphs that stop after one iteration). The host graph factorises differently (envelope
Cholesky against LU), so it is allowed 10 times that, 8.9e-15, and nothing more. llsr_pg_poses
narrows the estimate to float, so the bound is applied before the narrowing: with f the restatement's
double, every float of the host graph must lie in [float32(f - tol), float32(f + tol)], which is f's
float unless f sits within tol of a float rounding boundary. Measured: every float of the host graph
equals the narrowed restatement except components within 1e-18 of zero (largest difference 8.2e-19).
Iteration counts and final states must be equal.

The prior's bound. Gauss-Newton leaves error_after <= error_before, and the prior's share of the error
is half the squared whitened residual of pose 0, so component k of pose 0's residual against its prior
is at most sigma_k sqrt(2 error_after): sigma = 1e-3 rad for the rotation and (1e-4, 1e-4, 1e-3) m for
the translation (the variances 1e-6 / 1e-8 of MO:1618)."""
import numpy as np
import pytest

import _pose_graph as ref
from llsr import LlsrError, PoseGraph

EINVAL, ERANGE = -22, -34
SPREAD = 8.9e-16  # the restatement's own spread (see above)


def _loop_floats(truth, frm, to):
    return ref.store_to_gtsam6(truth[frm]), ref.store_to_gtsam6(truth[to])


CASES = {
    "pair": (2, [(1, 0)], 0.3),
    "square": (12, [(11, 0)], 0.3),
    "three_loops": (12, [(11, 0), (11, 4), (8, 1)], 0.3),
    "long": (70, [(69, 3)], 0.01),
}


def _build(name):
    K, loops, var = CASES[name]
    poses, truth = ref.square(K, 0.01, np.radians(0.2)), ref.square(K)
    g, h = ref.Graph(), PoseGraph(1, K, len(loops), device=None)
    g.append(poses)
    h.append(0, poses)
    for l, (frm, to) in enumerate(loops):
        pf, pt = _loop_floats(truth, frm, to)
        v = np.float32(var * (1 + 0.3 * l))
        g.add_loop(frm, to, pf, pt, v)
        h.add_loop(0, frm, to, pf, pt, v)
    return poses, g, h


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name in CASES:
        poses, g, h = _build(name)
        fwd, rev = g.optimize(), g.optimize(reverse=True)
        rep = h.optimize()[0]
        out[name] = {"poses": poses, "graph": g, "fwd": fwd, "rev": rev, "rep": rep, "host": h.poses(0),
                     "again": h.optimize()[0], "host_again": h.poses(0)}
        h.close()
    return out


def _store(X):
    return np.array([ref.to_store6(T) for T in X])


def _outside(host, f, tol):
    """Largest distance of the host graph's floats from [float32(f - tol), float32(f + tol)]."""
    lo, hi = (f - tol).astype(np.float32), (f + tol).astype(np.float32)
    h = host.astype(np.float64)
    return float(np.maximum(np.maximum(lo - h, h - hi), 0).max())


def test_host_graph_equals_the_restatement_within_its_own_spread(solved):
    errs = []
    spread = max(float(np.abs(_store(s["fwd"]["X"]) - _store(s["rev"]["X"])).max()) for s in solved.values())
    assert 0 < spread <= SPREAD, spread  # the docstring's figure still holds
    for name, s in solved.items():
        f = _store(s["fwd"]["X"])
        diff = np.abs(s["host"].astype(np.float64) - f.astype(np.float32).astype(np.float64))
        out = _outside(s["host"], f, 10 * spread)
        print(f"{name}: spread {spread:.3g}, host - float32(restatement) {diff.max():.3g}, outside the bracket "
              f"{out:.3g}, iterations {s['rep']['iterations']} / {s['fwd']['iterations']}, state "
              f"{s['rep']['state']} / {s['fwd']['state']}")
        if out > 0:
            errs.append(f"{name}: a pose lies {out:.3g} outside 10 x the spread {spread:.3g}")
        if (s["rep"]["iterations"], s["rep"]["state"]) != (s["fwd"]["iterations"], s["fwd"]["state"]):
            errs.append(f"{name}: {s['rep']} against {s['fwd']['iterations'], s['fwd']['state']}")
        for k in ("error_before", "error_after"):
            if abs(s["rep"][k] - s["fwd"][k]) > 1e-9 * s["fwd"][k]:
                errs.append(f"{name}: {k} {s['rep'][k]!r} against {s['fwd'][k]!r}")
    assert not errs, "\n".join(errs)


def test_a_second_optimize_without_a_new_loop_is_clean(solved):
    for name, s in solved.items():
        assert s["again"]["state"] == 0 and s["again"]["iterations"] == 0, name
        assert s["host_again"].tobytes() == s["host"].tobytes(), name
        assert (s["again"]["poses"], s["again"]["loops"]) == (CASES[name][0], len(CASES[name][1]))


@pytest.mark.parametrize("K", [1, 2, 12])
def test_clean_graph_returns_the_appended_floats(K):
    poses = ref.square(K, 0.01, np.radians(0.2))
    h = PoseGraph(2, 12, 1, device=None)
    h.append(1, poses[:1])
    h.append(1, poses[1:])
    reps = h.optimize()
    assert [r["state"] for r in reps] == [0, 0] and reps[1]["iterations"] == 0
    assert (reps[1]["poses"], reps[1]["loops"], reps[0]["poses"]) == (K, 0, 0)
    assert h.poses(1).tobytes() == poses.tobytes()
    assert h.poses(0).shape == (0, 6)
    h.close()


def test_drifting_square(solved):
    s = solved["square"]
    g = s["graph"]
    before = np.linalg.norm(g.loop_residual())
    after_ref = np.linalg.norm(g.loop_residual(s["fwd"]["X"]))
    host = [ref.from_store6(p) for p in s["host"]]
    after_host = np.linalg.norm(g.loop_residual(host))
    print(f"loop residual {before:.6g} -> restatement {after_ref:.6g}, host graph {after_host:.6g}; "
          f"error {s['rep']['error_before']:.6g} -> {s['rep']['error_after']:.6g}")
    assert after_ref < before
    # the host graph reaches the factor the restatement reaches. Its poses went through float32, so the
    # restatement's go through it too; what is left is the pose tolerance, 10 x the spread on each of
    # the twelve components of poses 11 and 0, which move the residual by at most 1 (translations) and
    # 1 + 6 (angles; the two poses are less than 6 m apart) times their own change
    narrowed = [ref.from_store6(p) for p in _store(s["fwd"]["X"]).astype(np.float32)]
    after_ref32 = np.linalg.norm(g.loop_residual(narrowed))
    assert abs(after_host - after_ref32) <= 10 * SPREAD * (6 * 1 + 6 * 7)
    assert abs(after_ref32 - after_ref) <= 48 * 4.8e-7  # and the narrowing itself, 48 float ulps at most
    assert s["rep"]["error_after"] < s["rep"]["error_before"]
    # pose 0 against its prior (the appended pose): sigma_k sqrt(2 error_after), plus the float32
    # narrowing of the estimate
    e0 = ref.error(ref.from_store6(s["poses"][0]), host[0])
    sigma = np.sqrt(ref.PRIOR_VAR)
    bound = sigma * np.sqrt(2 * s["rep"]["error_after"]) + 4.8e-7
    assert np.all(np.abs(e0) <= bound), (e0, bound)
    assert np.any(s["host"] != s["poses"])  # and the graph did move


def _unchanged(h, poses, K):
    assert h.poses(0).tobytes() == poses[:K].tobytes()
    rep = h.optimize()[0]
    assert (rep["state"], rep["poses"], rep["loops"]) == (0, K, 0)


def test_refusals_leave_the_graph_unchanged():
    poses = ref.square(6, 0.01)
    pf, pt = _loop_floats(poses, 5, 0)
    h = PoseGraph(1, 6, 1, max_envelope_blocks=2 * 6 - 1 + 2, device=None)
    h.append(0, poses[:5])

    def refused(code, fn, *a):
        with pytest.raises(LlsrError) as e:
            fn(*a)
        assert e.value.code == code, (e.value, code)
        _unchanged(h, poses, 5)

    bad = poses[5:6].copy()
    bad[0, 3] = np.nan
    refused(EINVAL, h.append, 0, bad)
    bad[0, 3] = np.inf
    refused(EINVAL, h.append, 0, bad)
    refused(ERANGE, h.append, 0, np.concatenate([poses[5:6]] * 2))  # a seventh pose
    refused(EINVAL, h.append, 1, poses[5:6])  # no such graph
    for frm, to in ((5, 0), (0, 5), (-1, 0), (2, 2)):
        refused(EINVAL, h.add_loop, 0, frm, to, pf, pt, 0.3)
    for var in (0.0, -1.0, np.nan, np.inf):
        refused(EINVAL, h.add_loop, 0, 4, 0, pf, pt, var)
    nf = pf.copy()
    nf[4] = np.nan
    refused(EINVAL, h.add_loop, 0, 4, 0, nf, pt, 0.3)
    refused(EINVAL, h.add_loop, 0, 4, 0, pf, nf, 0.3)
    h.append(0, poses[5:6])
    with pytest.raises(LlsrError) as e:
        h.add_loop(0, 4, 0, pf, pt, 0.3)  # the envelope: 11 blocks + 3 for the loop > 13
    assert e.value.code == ERANGE
    _unchanged(h, poses, 6)
    h.add_loop(0, 3, 1, pf, pt, 0.3)  # 11 blocks + 1
    with pytest.raises(LlsrError) as e:
        h.add_loop(0, 5, 3, pf, pt, 0.3)  # a second loop
    assert e.value.code == ERANGE
    rep = h.optimize()[0]
    assert (rep["poses"], rep["loops"]) == (6, 1) and rep["state"] in (1, 2)
    h.close()
    h = PoseGraph(1, 6, 1, max_envelope_blocks=8, device=None)
    h.append(0, poses[:4])  # 7 blocks
    with pytest.raises(LlsrError) as e:
        h.append(0, poses[4:5])  # 9
    assert e.value.code == ERANGE
    _unchanged(h, poses, 4)
    h.close()
    for args in ((0, 4, 1), (1, 0, 1), (1, 4, -1), (1, 4, 1, 0)):
        with pytest.raises(LlsrError):
            PoseGraph(*args, device=None)


def test_failed_state_leaves_the_poses():
    """The issue reaches "failed" with a loop variance of 1e-300. The ABI takes the variance as a float
    (llsr_loop_constraint's), where 1e-300 is 0 and is refused with LLSR_EINVAL; the smallest positive
    float, 1.4e-45, whitens the loop factor by 2.7e22, its 7e44 swamps the odometry's 1e8 in the
    normal equations, and a pivot of the factorisation cancels to a value that is not positive: state 5
    at iteration 0, the poses as they were. The pivot test is the specification's (finite and > 0)."""
    poses = ref.square(12, 0.01)
    pf, pt = _loop_floats(ref.square(12), 11, 0)
    h = PoseGraph(1, 12, 1, device=None)
    h.append(0, poses)
    with pytest.raises(LlsrError) as e:
        h.add_loop(0, 11, 0, pf, pt, 1e-300)
    assert e.value.code == EINVAL
    h.add_loop(0, 11, 0, pf, pt, np.float32(1.4e-45))
    rep = h.optimize()[0]
    print(rep)
    assert (rep["state"], rep["iterations"]) == (5, 0) and rep["error_after"] == rep["error_before"] > 1e40
    assert h.poses(0).tobytes() == poses.tobytes()
    assert h.optimize()[0]["state"] == 0  # the factor stays in the graph; nothing retries it unasked
    h.close()


def test_append_after_an_optimisation_measures_from_the_estimate():
    """The odometry measurement of a keyframe appended after a loop closure is taken from the corrected
    estimate of the keyframe before it (MO:1654-1664): it has no error at the appended pose, so a
    further loop optimises from there exactly as the restatement does."""
    poses, g, h = _build("square")
    h.optimize()
    g.X = g.optimize()["X"]
    more = ref.square(14, 0.01, np.radians(0.2))[12:]
    g.append(more)
    h.append(0, more[:0])
    with pytest.raises(LlsrError):
        h.append(0, more)  # capacity 12
    h.close()
    h2 = PoseGraph(1, 14, 2, device=None)
    truth = ref.square(12)
    h2.append(0, poses)
    h2.add_loop(0, 11, 0, *_loop_floats(truth, 11, 0), np.float32(0.3))
    h2.optimize()
    h2.append(0, more)
    assert h2.poses(0)[12:].tobytes() == more.tobytes()
    pf, pt = _loop_floats(ref.square(14), 13, 2)
    g.add_loop(13, 2, pf, pt, np.float32(0.2))
    h2.add_loop(0, 13, 2, pf, pt, np.float32(0.2))
    a, b = g.optimize(), h2.optimize()[0]
    assert (a["iterations"], a["state"]) == (b["iterations"], b["state"])
    assert _outside(h2.poses(0), _store(a["X"]), 10 * SPREAD) == 0
    h2.close()
