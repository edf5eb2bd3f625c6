"""GPU: the device pose graph (llsr_pg_create on a HIP device: k_pg_linearize, k_pg_error,
k_pg_assemble, k_pg_solve, k_pg_update over every problem per pass) against a host graph
(LLSR_PG_HOST) fed the same calls. Poses, reports (every field but ms) and iteration counts must be
equal bit for bit.

One batch of P = 4: K = 1 (prior only, never optimised), K = 2 with the loop (1, 0), K = 12 with three
loops — (11, 0) and (11, 4) end on the same row, (8, 1) crosses (11, 4) — and K = 70 with the loop
(69, 3): more block rows than one wave has lanes and more than 64 envelope columns in a row. The
graphs are tests/_pose_graph.py's drifting square (1 cm and 0.2 degrees per step); the K = 70 loop has
the variance 0.01 instead of 0.3, which costs it one more iteration, so the four problems stop after
0, 1, 2 and 3 iterations and a finished problem idles while the others go on."""
import numpy as np
import pytest

import _pose_graph as ref
from llsr import PoseGraph

pytestmark = pytest.mark.gpu
BATCH = ((1, [], 0.3), (2, [(1, 0)], 0.3), (12, [(11, 0), (11, 4), (8, 1)], 0.3), (70, [(69, 3)], 0.01))
FIELDS = ("state", "iterations", "error_before", "error_after", "poses", "loops", "moved")


def _feed(g, p, case):
    K, loops, var = case
    truth = ref.square(K)
    g.append(p, ref.square(K, 0.01, np.radians(0.2)))
    for l, (frm, to) in enumerate(loops):
        g.add_loop(p, frm, to, ref.store_to_gtsam6(truth[frm]), ref.store_to_gtsam6(truth[to]),
                   np.float32(var * (1 + 0.3 * l)))


def _bits(rep):
    return tuple(np.float64(rep[k]).tobytes() if isinstance(rep[k], float) else rep[k] for k in FIELDS)


@pytest.fixture(scope="module")
def run(require_gpu):
    """Every optimisation of the module, once: the batch on both sides, a second optimise, each problem
    alone on the device, and a smaller batch on the object that ran the larger one."""
    rec = {}
    dev, host = PoseGraph(4, 70, 3, 2 * 70 - 1 + 65), PoseGraph(4, 70, 3, 2 * 70 - 1 + 65, device=None)
    for g in (dev, host):
        for p, case in enumerate(BATCH):
            _feed(g, p, case)
    rec["dev"], rec["host"] = dev.optimize(), host.optimize()
    rec["dev_poses"] = [dev.poses(p) for p in range(4)]
    rec["host_poses"] = [host.poses(p) for p in range(4)]
    rec["again"] = dev.optimize()
    rec["again_poses"] = [dev.poses(p) for p in range(4)]
    rec["alone"] = []
    for case in BATCH:
        one = PoseGraph(1, case[0], max(len(case[1]), 1))
        _feed(one, 0, case)
        rec["alone"].append((one.optimize()[0], one.poses(0)))
        one.close()
    # the same object again with less in it: graphs 2 and 3 emptied, graph 0 now the pair, graph 1 a
    # 12-pose graph with one loop; whatever the larger batch left in the workspace must not show
    small = ((2, [(1, 0)], 0.3), (12, [(11, 0)], 0.3))
    for g in (dev, host):
        g.reset()
        for p, case in enumerate(small):
            _feed(g, p, case)
    rec["small_dev"], rec["small_host"] = dev.optimize(), host.optimize()
    rec["small_dev_poses"] = [dev.poses(p) for p in range(4)]
    rec["small_host_poses"] = [host.poses(p) for p in range(4)]
    fresh = PoseGraph(2, 12, 1, device=None)
    for p, case in enumerate(small):
        _feed(fresh, p, case)
    rec["small_fresh"] = fresh.optimize()
    rec["small_fresh_poses"] = [fresh.poses(p) for p in range(2)]
    for g in (dev, host, fresh):
        g.close()
    return rec


def test_batch_equals_the_host_graph_bit_for_bit(run):
    print([(r["state"], r["iterations"], r["error_before"], r["error_after"]) for r in run["host"]])
    for p in range(4):
        assert _bits(run["dev"][p]) == _bits(run["host"][p]), (p, run["dev"][p], run["host"][p])
        assert run["dev_poses"][p].tobytes() == run["host_poses"][p].tobytes(), p
        assert run["dev"][p]["ms"] > 0 or run["dev"][p]["state"] == 0


def test_problems_stop_after_different_iteration_counts(run):
    its = [r["iterations"] for r in run["host"]]
    assert its[0] == 0 and run["host"][0]["state"] == 0
    assert len(set(its)) == 4, its
    assert all(r["state"] in (1, 2) and r["error_after"] < r["error_before"] for r in run["host"][1:])
    truth = [ref.square(c[0], 0.01, np.radians(0.2)) for c in BATCH]
    assert run["host_poses"][0].tobytes() == truth[0].tobytes()
    assert all(np.any(run["host_poses"][p] != truth[p]) for p in (1, 2, 3))


def test_each_problem_alone_equals_its_slot(run):
    for p, (rep, poses) in enumerate(run["alone"]):
        assert _bits(rep) == _bits(run["dev"][p]), (p, rep, run["dev"][p])
        assert poses.tobytes() == run["dev_poses"][p].tobytes(), p


def test_second_optimize_without_a_new_loop_changes_nothing(run):
    for p in range(4):
        assert (run["again"][p]["state"], run["again"][p]["iterations"]) == (0, 0)
        assert run["again_poses"][p].tobytes() == run["dev_poses"][p].tobytes()


def test_smaller_batch_after_a_larger_one(run):
    for p in range(4):
        assert _bits(run["small_dev"][p]) == _bits(run["small_host"][p]), p
        assert run["small_dev_poses"][p].tobytes() == run["small_host_poses"][p].tobytes(), p
    for p in range(2):
        assert _bits(run["small_dev"][p]) == _bits(run["small_fresh"][p]), p
        assert run["small_dev_poses"][p].tobytes() == run["small_fresh_poses"][p].tobytes(), p
    assert [r["poses"] for r in run["small_dev"]] == [2, 12, 0, 0]
