"""The numpy statement of the use_vlp32c branch (tests/_vlp32c.py) against the oracle where the two
must agree, the beam layouts it is tested on, and the branch's own properties. No GPU.

The oracle refuses use_vlp32c, so it certifies the statement on the one input where the branch and
the plain one coincide: a "vlp32c_uniform" scan, whose 32 rings fall into 32 distinct bins in ring
order, so the rank of a bin IS the plain branch's row.
"""
import numpy as np
import pytest

import _vlp32c as V
import oracle_py
from llsr import synth

H, W = 32, 1800


@pytest.fixture(scope="module")
def uniform():
    pts = V.scan("vlp32c_uniform")
    return pts, V.project(V.config(), pts)


def test_statement_matches_oracle_on_plain_rows(uniform):
    pts, p = uniform
    assert p["vertical_raw2"].size == 32
    o = oracle_py.Oracle(V.config(use_vlp32c=0)).process(pts)
    assert np.array_equal(p["cell_point"], o["cell_point"])
    assert np.array_equal(p["range_image"].view(np.uint32), o["range_image"].view(np.uint32))
    assert (p["cell_point"] >= 0).sum() > 30000  # a real scan, every ring present
    assert set(p["row"][p["placed"]].tolist()) == set(range(32))


@pytest.mark.parametrize("rule,kitti", [("60/25", 1), (12.5, 0)])
def test_column_pass_ties_to_oracle_ground(uniform, rule, kitti):
    pts, p = uniform
    cfg = V.config(use_vlp32c=0, use_kitti=kitti)
    o = oracle_py.Oracle(cfg).process(pts)
    g = V.column_pass(cfg, p["full_cloud"], rule)
    assert (g == 0).sum() > 100 and (g == 1).sum() > 1000 and (g == -1).sum() > 100
    assert V.check_invariants(g, o["ground_image"], p["full_cloud"], cfg) == []


def test_column_pass_rules_differ(uniform):
    """The invariants above would not notice a statement that ignored its rule."""
    _, p = uniform
    g = {r: V.column_pass(V.config(), p["full_cloud"], r) for r in (12.5, 25, "60/25")}
    assert (g[12.5] != g[25]).any() and (g[12.5] != g["60/25"]).any()


def test_vlp32c_layout_bins():
    """The VLP-32C table falls into 32 distinct bins on generated float32 points, each ring into the
    bin of its nominal elevation; the uniform layout likewise."""
    cfg = V.config()
    for layout in ("vlp32c", "vlp32c_uniform"):
        elev, w = synth.beam_layout(layout)
        assert w == W and elev.size == 32
        q = (elev + 25.1) / 0.335
        frac = q - np.floor(q)
        assert np.minimum(frac, 1 - frac).min() > (0.004 if layout == "vlp32c" else 0.01)
        pts = V.scan(layout)
        temp, _, finite = V.bins_of(cfg, pts)
        ring = np.arange(pts.shape[0]) % 32           # firing order inside each azimuth
        want = np.floor(q).astype(np.int64)[ring]
        assert finite.sum() > 30000
        assert np.array_equal(temp[finite], want[finite])
        assert np.unique(temp[finite]).size == 32
    e = np.sort(synth.beam_layout("vlp32c_uniform")[0])
    assert np.allclose(np.diff(e), 40.0 / 31.0)


def _ring_of(pts):
    return np.arange(pts.shape[0]) % 32


def test_deleting_a_ring_shifts_higher_rows_down(uniform):
    pts, p = uniform
    order = np.argsort(synth.beam_layout("vlp32c_uniform")[0])   # ring of each row
    gone = order[10]
    cut = pts.copy()
    cut[_ring_of(pts) == gone] = np.nan
    q = V.project(V.config(), cut)
    assert q["vertical_raw2"].size == 31
    keep = p["placed"] & (_ring_of(pts) != gone)
    assert np.array_equal(q["placed"], keep)
    assert np.array_equal(q["row"][keep], p["row"][keep] - (p["row"][keep] > 10))
    assert np.array_equal(q["col"][keep], p["col"][keep])


def test_bins_are_claimed_before_the_other_tests(uniform):
    pts, p = uniform
    cfg = V.config()
    n = p["vertical_raw2"].size
    # one point above vertical_angle_top adds a bin (and, with 33 bins, the top rank overflows)
    el = np.deg2rad(40.0)
    above = np.array([[10 * np.cos(el), 0.0, 10 * np.sin(el), 1.0]], np.float32)
    q = V.project(cfg, np.concatenate([pts, above]))
    assert q["vertical_raw2"].size == n + 1 and q["row"][-1] == 32 and not q["placed"][-1]
    assert np.array_equal(q["cell_point"], p["cell_point"])
    # a point nearer than 0.1 m still occupies its bin, here an otherwise empty one. (The column
    # test, IP:409, cannot fail for a finite point: atan2f is finite and -round(.) + W / 2 lands in
    # [W / 4, 5 W / 4], which IP:406 folds into [0, W). The statement keeps the test all the same.)
    el = np.deg2rad(-21.5)    # between the rings at -22.4 and -21.1 deg: bin 10, unused
    near = np.array([[0.05 * np.cos(el), 0.0, 0.05 * np.sin(el), 1.0]], np.float32)
    q = V.project(cfg, np.concatenate([pts, near]))
    assert q["vertical_raw2"].size == n + 1 and q["bins"][-1] == 10 and not q["placed"][-1]
    # every row above the new bin moved up by one: the unplaced point still shifted the ranks
    assert np.array_equal(q["row"][:-1][p["placed"]], p["row"][p["placed"]] + (p["bins"][p["placed"]] > 10))
    # a point at the origin sets no bin
    q = V.project(cfg, np.concatenate([pts, np.zeros((1, 4), np.float32)]))
    assert q["bins"][-1] < 0 and q["vertical_raw2"].size == n
    assert np.array_equal(q["cell_point"], p["cell_point"])
