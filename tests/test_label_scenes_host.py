"""The scenes of tests/_label_scenes.py on the CPU oracle alone: every (geometry, scene) lands its
points in their cells, the serial numpy BFS over the oracle's own label-0 mask gives the oracle's
label image cell for cell, and every named shape is one component of exactly its cells, in the bands
the scene states, kept or dropped as the scene states. A shape that cannot exist at a geometry is
listed with its reason and the reason is asserted (17 x 16 has no room for a row of 30 cells; a
16-row image cannot hold a run of 18 rows). Nothing here needs a GPU; tests/test_gpu_label_bands.py
compares the device with the same oracle outputs.
"""
import numpy as np
import pytest

import _label_scenes as ls


def check_scene(gname, sname):
    """Asserts on the oracle's outputs alone. Returns (components, kept components)."""
    g, sc = ls.GEOMS[gname], ls.scene(gname, sname)
    H, W = g.H, g.W
    o = ls.oracle(gname, sname)
    tag = f"{gname} {sname}"
    lv = sc.levels
    lab = np.asarray(o["label_image"]).reshape(H, W)
    rng = np.asarray(o["range_image"]).reshape(H, W)
    want = np.where(lv >= 0, 8.0 * g.K ** np.maximum(lv, 0).astype(np.float64), np.inf)
    have = np.where(rng == np.finfo(np.float32).max, np.inf, rng)
    assert np.allclose(have, want, rtol=1e-5), f"{tag}: the points did not land in their cells"
    bfs = ls.bfs(gname, sname)
    bad = np.argwhere(bfs != lab)
    assert not len(bad), f"{tag}: the BFS restatement differs from the oracle in {len(bad)} cells, first {bad[:5].tolist()}"
    comp = ls.bfs_components(lv, lab != -1)
    shape_ids = set()
    for name, sh in sc.shapes.items():
        i, j = sh.cells[:, 0], sh.cells[:, 1]
        assert (lab[i, j] != -1).all(), f"{tag}: {name} lost {int((lab[i, j] == -1).sum())} cells to the ground passes"
        ids = set(comp[i, j].tolist())
        assert len(ids) == 1, f"{tag}: {name} is {len(ids)} components"
        cid = ids.pop()
        n = int((comp == cid).sum()) - sum(comp[c] == cid for c in sc.spare)
        assert n == len(sh.cells), f"{tag}: {name}'s component has {n} cells, the shape {len(sh.cells)}"
        shape_ids.add(cid)
        kept = lab[i[0], j[0]] != ls.BIG
        assert kept == sh.kept, f"{tag}: {name} kept = {kept}, stated {sh.kept}"
        assert tuple(sorted({g.band_of(r) for r in i})) == sh.bands, f"{tag}: {name} is not in bands {sh.bands}"
    for name, (reason, holds) in sc.absent.items():
        assert holds, f"{tag}: {name} is left out ({reason}), but that does not hold here"
    assert sc.shapes or sc.absent or sname == "singles", f"{tag}: the scene is empty"
    ncomp = int(comp.max()) + 1
    nkept = int(np.unique(lab[(lab > 0) & (lab < ls.BIG)]).size)
    # every label-0 cell belongs to a named shape, but for cell (0, 0) (it reads as empty in the ground
    # pass: a label-0 cell of its own, dropped)
    named = sum(len(sh.cells) for sh in sc.shapes.values()) + sum(lab[c] != -1 for c in sc.spare)
    alone = len({int(comp[c]) for c in sc.spare if lab[c] != -1} - shape_ids)
    if sname == "singles":
        cells = int((lv[1:] >= 0).sum())
        assert nkept == 0 and ncomp == cells + 1 and int((lab == ls.BIG).sum()) == cells + 1, \
            f"{tag}: {ncomp} components of {cells} single cells, {nkept} kept"
    else:
        assert int((lab != -1).sum()) == named + 1 and ncomp == len(sc.shapes) + 1 + alone, \
            f"{tag}: {int((lab != -1).sum())} label-0 cells in {ncomp} components, the shapes hold {named}"
        assert nkept == sum(sh.kept for sh in sc.shapes.values())
    if sname == "one":
        assert nkept == 1 and sc.shapes["all"].bands == tuple(range(len(ls.bands(H, W)))), f"{tag}: not one component"
    return ncomp, nkept


@pytest.mark.parametrize("gname,sname", ls.PAIRS)
def test_scene_has_its_property(gname, sname):
    check_scene(gname, sname)


def test_band_layouts():
    """The layouts the geometries are there for."""
    rows = {n: [r1 - r0 for r0, r1 in ls.bands(g.H, g.W)] for n, g in ls.GEOMS.items()}
    assert rows == {"g17x16": [16, 1], "g16x2001": [9, 7], "g33x600": [16, 16, 1], "g64x288": [16] * 4,
                    "g64x1152": [16] * 4, "g64x1153": [15] * 4 + [4], "g64x2048": [9] * 7 + [1]}
    assert 16 * 1152 * 4 == 72 * 1024  # the LDS band at its full size


def test_bfs_labels_on_a_hand_made_image():
    """bfs_labels itself, on an image small enough to label by hand."""
    lv = np.full((5, 6), -1, np.int64)
    lv[1:4, 0] = 0               # 3 cells over the wrap ...
    lv[1, 5] = lv[2, 5] = 0      # ... with 2 more: 5 cells, seed (1, 0), pushed rows 1, 2, 3: kept
    lv[1, 2] = lv[1, 3] = 0      # 2 cells: dropped
    lv[3, 2:5] = 1
    lv[4, 2:4] = 1               # 5 cells, pushed rows 3, 4: dropped
    lv[3, 5] = 0                 # level 0 next to level 1, below (2, 5): joins the first component
    lab = ls.bfs_labels(lv, lv >= 0, 5, 3)
    want = np.full((5, 6), -1, np.int64)
    want[lv == 0] = 1
    want[1, 2] = want[1, 3] = ls.BIG
    want[lv == 1] = ls.BIG
    assert np.array_equal(lab, want)
    assert np.array_equal(ls.bfs_labels(lv, lv >= 0, 5, 2) == 2, lv == 1)  # two rows are enough: label 2


@pytest.mark.parametrize("gname", list(ls.GEOMS))
def test_every_boundary_is_crossed(gname):
    """Every band boundary is crossed by a kept component of a scene other than `one`."""
    g = ls.GEOMS[gname]
    crossed = set()
    for sname in ls.SCENES:
        if sname == "one":
            continue
        for sh in ls.scene(gname, sname).shapes.values():
            if sh.kept:
                cells = set(map(tuple, sh.cells.tolist()))
                crossed |= {b for b in g.boundaries if any((b - 1, j) in cells for i, j in cells if i == b)}
    assert crossed == set(g.boundaries), f"{gname}: boundaries {sorted(set(g.boundaries) - crossed)} are not crossed"
