"""k_label<true> on images built cell by cell: the down links it resolves along a lane's column, the
right edges it leaves to the union pass (one bit per cell, the ladder rule dropping an edge below
another one between the same two vertical runs, the wave queues), against the CPU oracle, bit-exact.

Every scene is a 16 x 200 image (three blocks of 64 columns and one of 8) given as a level per cell:
a cell of level v holds a point at its bin centre at 8 m * 1.03 ** v, a cell of level -1 no point.
Neighbouring cells link exactly when their levels are equal: for equal ranges the BFS angle is
90 deg - alpha / 2 > 60 deg, and a range ratio of 1.03 gives atan(sin a / (1.03 - cos a)) = 46 deg
across columns (a = 1.8 deg) and 49 deg across rows (a = 2 deg), below segment_theta. Row 0 is
present everywhere and is every column's ground return (cell (0, 0) reads as empty in the ground
pass, so it is a label-0 cell of its own and column 0 loses its lowest cell above it instead); rows
from 1 lie on spheres round the sensor, steeper than the ground angle, beyond the 5 m of the
near-ground RANSAC: they are the label-0 cells. So the components are the 4-connected regions of
equal level in rows >= 1, and test_scene_has_its_property checks on the
oracle's own label image, without a GPU, that each scene holds what it is there for:

    comb_top      teeth (even columns) joined only through a bar in row 1; odd columns strips apart
    comb_bottom   the same with the bar in row 15: every tooth's run head is a root until the bar
    staircase     steps down to the left and down to the right: the smallest cell of a component
                  is not in its leftmost column; one crosses columns 127 / 128
    wrap          a band and a ladder that close only through column 199 -> 0
    blocks        ladders and single rows across columns 63 / 64, 127 / 128, 191 / 192, and a
                  component inside the last block of 8 columns
    broken_rows   rows in pairs of equal level: a down link in every other row only
    no_edges      a checkerboard: not one edge, every label-0 cell its own component
    one           one level: one component holds every label-0 cell
    thresholds    runs of 29 and 30 cells, columns of 4 and 5, five cells over three rows with and
                  without a second cell in the seed's row, five cells over two rows
"""
import functools

import numpy as np
import pytest

import _config_cases as cc
from _compare import diff_report

H, W = 16, 200
CASE = cc.Case((H, W, -15.0, 15.0))
BIG = 999999
ARRAYS = ("ground_image", "label_image", "start_ring_index", "end_ring_index", "seg_xyzi", "seg_ground_flag",
          "seg_col_ind", "seg_range", "seg_intensity", "outlier_xyzi", "outlier_intensity")
COUNTS = ("n_segmented", "n_outlier")


def _blank():
    lv = np.full((H, W), -1, np.int64)
    lv[0] = 0
    return lv


def _comb(bar):
    lv = _blank()
    teeth = slice(1, 15) if bar == 15 else slice(2, 16)
    lv[teeth, 10:151:2] = 0
    lv[teeth, 11:150:2] = 2
    lv[bar, 10:151] = 0
    return lv


def _staircase():
    lv = _blank()
    for k in range(14):  # down to the left from (1, 100), down to the right from (1, 120): across 127 / 128
        lv[1 + k:3 + k, 100 - k] = 1
        lv[1 + k:3 + k, 120 + k] = 2
    return lv


def _wrap():
    lv = _blank()
    lv[1, 0] = 0                        # (column 0's first return above (0, 0): ground)
    lv[5, 190:] = lv[5, :10] = 1        # a band: one right edge over the wrap
    lv[8:13, 196:] = lv[8:13, :4] = 2   # a ladder: five edges over the wrap, one kept
    lv[14, 150:] = lv[14, :3] = 1       # and a band that starts in the block before the last
    return lv


def _blocks():
    lv = _blank()
    lv[3:10, 60:68] = 1      # ladder over 63 / 64
    lv[12, 125:131] = 2      # one row over 127 / 128 ...
    lv[12:16, 127] = 2       # ... with a column on either side
    lv[10:13, 128] = 2
    lv[2:9, 186:198] = 0     # ladder over 191 / 192 into the block of 8
    lv[11:15, 193:199] = 1   # inside the last block
    lv[1, 40:90] = 2         # a run through a whole block's left and right ends
    return lv


def _broken_rows():
    lv = _blank()
    lv[1:] = (((np.arange(1, H) + 1) // 2) % 2)[:, None]
    return lv


def _no_edges():
    lv = _blank()
    lv[1:] = (np.arange(1, H)[:, None] + np.arange(W)[None, :]) % 2
    return lv


def _one():
    lv = _blank()
    lv[1:] = 0
    return lv


# name -> cells (row, column) of the shapes of the thresholds scene, and whether the oracle keeps them
SHAPES = {
    "run29": ([(3, j) for j in range(10, 39)], False),
    "run30": ([(5, j) for j in range(10, 40)], True),
    "run30_blocks": ([(7, j) for j in range(50, 80)], True),
    "col5": ([(i, 90) for i in range(2, 7)], True),
    "col4": ([(i, 95) for i in range(2, 6)], False),
    "five_rows3_seed_alone": ([(2, 100), (3, 100), (4, 100), (4, 101), (4, 102)], None),
    "five_rows3_seed_pair": ([(2, 110), (2, 111), (3, 110), (4, 110), (4, 111)], True),
    "five_rows2": ([(2, 120), (2, 121), (2, 122), (3, 120), (3, 121)], False),
    "col5_last_block": ([(i, 197) for i in range(9, 14)], True),
}


def _thresholds():
    lv = _blank()
    for cells, _ in SHAPES.values():
        for i, j in cells:
            lv[i, j] = 1
    return lv


SCENES = {"comb_top": lambda: _comb(1), "comb_bottom": lambda: _comb(15), "staircase": _staircase, "wrap": _wrap,
          "blocks": _blocks, "broken_rows": _broken_rows, "no_edges": _no_edges, "one": _one,
          "thresholds": _thresholds}


@functools.lru_cache(maxsize=None)
def _levels(name):
    lv = SCENES[name]()
    lv.setflags(write=False)
    return lv


@functools.lru_cache(maxsize=None)
def _points(name):
    """The scene's raw scan, float32 [n, 4], azimuth-major like cc.scan: a beam through every bin centre."""
    lv = _levels(name)
    e = np.deg2rad(np.linspace(CASE.geom[2], CASE.geom[3], H))
    phi = (W / 2 - np.arange(W, dtype=np.float64)) * (2.0 * np.pi / W)
    t, i = [a.ravel() for a in np.meshgrid(np.arange(W), np.arange(H), indexing="ij")]
    j = (W - t) % W  # the projection's column of azimuth phi[t]
    keep = lv[i, j] >= 0
    t, i, j = t[keep], i[keep], j[keep]
    r = 8.0 * 1.03 ** lv[i, j]
    pts = np.empty((t.size, 4), np.float32)
    pts[:, 0] = r * np.cos(phi[t]) * np.cos(e[i])
    pts[:, 1] = r * np.sin(phi[t]) * np.cos(e[i])
    pts[:, 2] = r * np.sin(e[i])
    pts[:, 3] = 10.0 + (i * 7 + t) % 90
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _oracle(name):
    import oracle_py
    return oracle_py.Oracle(cc.config(CASE)).process(_points(name))


def _lab(out):
    return np.asarray(out["label_image"]).reshape(H, W)


def _expected_label0(name):
    """Rows from 1 with a point, but for column 0's first return."""
    lv = _levels(name)
    m = lv >= 0
    m[0, 1:] = False  # (0, 0) reads as empty in the ground pass: not ground, a label-0 cell of its own
    if (lv[1:, 0] >= 0).any():
        m[int(np.nonzero(lv[1:, 0] >= 0)[0][0]) + 1, 0] = False
    return m


def _components(lab):
    """{label: cells [n, 2]} of the kept components."""
    return {int(v): np.argwhere(lab == v) for v in np.unique(lab) if 0 < v < BIG}


def _check_scene(name):
    """Asserts on the oracle's outputs alone."""
    o = _oracle(name)
    lv, lab = _levels(name), _lab(o)
    rng = np.asarray(o["range_image"]).reshape(H, W)
    want = np.where(lv >= 0, (8.0 * 1.03 ** np.maximum(lv, 0)), np.inf)
    have = np.where(rng == np.finfo(np.float32).max, np.inf, rng)
    assert np.allclose(have, want, rtol=1e-5), f"{name}: the points did not land in their cells"
    assert np.array_equal(lab != -1, _expected_label0(name)), f"{name}: label-0 cells are not rows >= 1 with a point"
    comps = _components(lab)
    for v, cells in comps.items():  # labels follow the smallest cell, and a component has one level
        assert len(set(lv[cells[:, 0], cells[:, 1]].tolist())) == 1, f"{name}: component {v} mixes levels"
    firsts = [tuple(c[0]) for _, c in sorted(comps.items())]
    assert firsts == sorted(firsts), f"{name}: labels not in the order of the smallest cells"
    rows = {v: np.unique(c[:, 0]).size for v, c in comps.items()}
    if name in ("comb_top", "comb_bottom"):
        bar = 1 if name == "comb_top" else 15
        big = [v for v, c in comps.items() if len(c) > 500]
        assert len(big) == 1 and rows[big[0]] == 15, f"{name}: no component of all teeth"
        c = comps[big[0]]
        per_row = np.bincount(c[:, 0], minlength=H)
        assert per_row[bar] == 141 and all(per_row[i] == 71 for i in range(1, H) if i != bar), f"{name}: {per_row}"
        assert len(comps) == 1 + 70, f"{name}: {len(comps)} components, expected the comb and 70 strips"
    elif name == "staircase":
        assert len(comps) == 2
        for v, c in comps.items():
            assert len(c) == 28 and rows[v] == 15
        left = comps[1]
        assert left[0].tolist() == [1, 100] and left[:, 1].min() == 87, "staircase: the smallest cell is leftmost"
        right = comps[2]
        assert right[:, 1].min() <= 127 < right[:, 1].max(), "staircase: does not cross 127 / 128"
    elif name == "wrap":
        over = [v for v, c in comps.items() if 0 in c[:, 1] and W - 1 in c[:, 1]]
        assert len(over) == 2 and len(comps) == 2, f"wrap: components over the wrap {over} of {sorted(comps)}"
        assert all(100 not in comps[v][:, 1] for v in over), "wrap: closes through the middle"
        assert sorted(len(comps[v]) for v in over) == [40, 53], f"wrap: {[len(comps[v]) for v in over]}"
        assert lab[5, 0] == BIG and lab[5, W - 1] == BIG and int((lab == BIG).sum()) == 21, \
            "wrap: the band of 20 cells is not whole (and dropped)"
    elif name == "blocks":
        spans = sorted((int(c[:, 1].min()), int(c[:, 1].max()), len(c)) for c in comps.values())
        assert spans == [(40, 89, 50), (60, 67, 56), (125, 130, 11), (186, 197, 84), (193, 198, 24)], f"blocks: {spans}"
    elif name == "broken_rows":
        assert len(comps) == 8 and sorted(rows.values()) == [1] + [2] * 7, f"broken_rows: {rows}"
        assert all(len(c) in (W, 2 * W, 2 * W - 1) for c in comps.values())
    elif name == "no_edges":
        assert not comps and int((lab == BIG).sum()) == 15 * W, "no_edges: a component was kept"
    elif name == "one":
        assert list(comps) == [1] and len(comps[1]) == 15 * W - 1 and int((lab == BIG).sum()) == 1, "one: not one component"
    elif name == "thresholds":
        for shape, (cells, kept) in SHAPES.items():
            got = {int(lab[i, j]) for i, j in cells}
            assert len(got) == 1, f"thresholds: {shape} is not one component: {got}"
            if kept is not None:
                assert (got.pop() != BIG) == kept, f"thresholds: {shape} kept = {not kept}"
        # the seed's row counts only through a second cell (the row set is that of the pushed cells)
        alone = int(lab[2, 100])
        assert alone == BIG, "thresholds: five cells over three rows, the seed alone in its row, were kept"


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_has_its_property(name):
    _check_scene(name)


def _diff(g, o):
    errs = [f"{k}: gpu={g[k]} oracle={o[k]}" for k in COUNTS if g[k] != o[k]]
    errs += [r for r in (diff_report(k, g[k], o[k]) for k in ARRAYS) if r]
    return errs


def _run(name):
    from llsr import Pipeline
    pipe = Pipeline(cc.config(CASE), max_points=H * W)
    g = pipe.process_scan(_points(name))
    pipe.close()
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_labels_bit_exact(require_gpu, name):
    _check_scene(name)
    errs = _diff(_run(name), _oracle(name))
    assert not errs, f"{name}:\n" + "\n".join(errs)


@pytest.mark.gpu
def test_two_handles_agree(require_gpu):
    for name in ("blocks", "wrap"):
        a, b = _run(name), _run(name)
        errs = _diff(a, b)
        assert not errs, f"{name}: two fresh handles differ:\n" + "\n".join(errs)


@pytest.mark.gpu
def test_smaller_batch_after_larger(require_gpu):
    """Four scenes as one batch, then one of them alone on the same handle: every output as from a
    fresh handle (nothing of the larger batch is left in the parent words or the edge masks)."""
    import torch
    from llsr import Pipeline
    names = ("one", "no_edges", "blocks", "comb_bottom")
    clouds = [_points(n) for n in names]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    d_pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    d_off = torch.from_numpy(off).cuda()
    pipe = Pipeline(cc.config(CASE), max_batch=len(names), max_points=H * W)
    pipe.process_batch(d_pts.data_ptr(), d_off.data_ptr(), len(names))
    failures = []
    for b, n in enumerate(names):
        failures += [f"batch of 4, {n}: {e}" for e in _diff(pipe.fetch(b), _oracle(n))]
    for n in ("wrap", "no_edges"):
        failures += [f"{n} alone after the batch: {e}" for e in _diff(pipe.process_scan(_points(n)), _oracle(n))]
    pipe.close()
    assert not failures, "\n".join(failures)
