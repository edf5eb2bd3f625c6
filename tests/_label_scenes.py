"""Label images built cell by cell for k_label<false>, the banded labelling of every image that does
not fit LDS (H > 16, or 16 rows of more than 2000 columns).

Helpers only: nothing here calls the product library or the oracle at import. A scene is a level per
cell, as in tests/test_gpu_label_columns.py: a cell of level v holds a point at its bin centre at
8 m * K ** v, a cell of level -1 no point; two neighbouring label-0 cells link exactly when their
levels are equal (`points` asserts the K that this needs at the geometry's column and row steps).
Row 0 is present in every column, at the level of the column's shapes, and is the column's ground
return; the shapes are single-level regions on an empty background in rows >= 1 (a radial step
between two vertically adjacent cells reads as ground at the fine row spacing of the 64-row
geometries, cells on one sphere never do). Which cells are label 0 is never predicted: it is taken
from the oracle's label image, and every shape asserts on the oracle that it kept its cells.

`bands(H, W)` restates the band layout of k_label<false>; the scenes place their shapes relative to
its boundaries. `bfs_labels` restates labelComponents serially in numpy, sharing nothing with the
kernel's band scheme. tests/test_label_scenes_host.py proves every scene's property on the oracle
(CPU); tests/test_gpu_label_bands.py compares the device with the oracle on the same scans.
DESIGN.md §2.2 lists geometries, scenes and the oracle's counts.
"""
from __future__ import annotations

import functools
from collections import deque
from dataclasses import dataclass, field

import numpy as np

import _config_cases as cc

BIG = 999999
HDL = (-24.8, 2.0)


@dataclass(frozen=True)
class Geom:
    H: int
    W: int
    bottom: float
    top: float
    kitti: bool = False   # the HDL-64E block instead of the VLP-16 one
    K: float = 1.03       # range ratio of one level

    @property
    def R(self):
        return bands(self.H, self.W)[0][1]

    @property
    def boundaries(self):
        """First rows r1 of every band but the first: the boundary lies between rows r1 - 1 and r1."""
        return [r0 for r0, _ in bands(self.H, self.W)[1:]]

    def band_of(self, row):
        return int(row) // self.R


GEOMS = {
    "g17x16": Geom(17, 16, -16.0, 16.0, K=1.3),
    "g16x2001": Geom(16, 2001, -15.0, 15.0),
    "g33x600": Geom(33, 600, -25.0, 15.0),
    "g64x288": Geom(64, 288, *HDL, kitti=True),
    "g64x1152": Geom(64, 1152, *HDL, kitti=True),
    "g64x1153": Geom(64, 1153, *HDL, kitti=True),
    "g64x2048": Geom(64, 2048, *HDL, kitti=True),
}


def bands(H, W):
    """[(r0, r1)] of k_label<false>'s LDS bands: lbl_band = max(1, min(H, 16, 18432 / W)) rows each,
    the last one what is left."""
    R = max(1, min(H, 16, 18432 // max(1, W)))
    return [(r0, min(r0 + R, H)) for r0 in range(0, H, R)]


def min_ratio(geom, theta_deg=60.0):
    """The range ratio above which two neighbouring cells do not link: the BFS keeps an edge when
    atan(d2 sin a / (d1 - d2 cos a)) > segment_theta, so it breaks for d1 / d2 >= cos a + sin a /
    tan(theta); a is the column step 2 pi / W or the row step, whichever asks for more."""
    t = np.tan(np.deg2rad(theta_deg))
    steps = (2.0 * np.pi / geom.W, np.deg2rad((geom.top - geom.bottom) / (geom.H - 1)))
    return max(np.cos(a) + np.sin(a) / t for a in steps)


def points(levels, geom, K=None):
    """The raw scan of a level image, float32 [n, 4], azimuth-major like _config_cases.scan: a beam
    through every bin centre, at 8 m * K ** level."""
    K = geom.K if K is None else K
    H, W = geom.H, geom.W
    lv = np.asarray(levels)
    assert lv.shape == (H, W)
    # unequal levels must not link (1 % of margin for float32), equal ones must: 90 deg - a / 2 > theta
    assert K > 1.01 * min_ratio(geom), f"K = {K} links unequal levels at {H} x {W}: needs > {min_ratio(geom):.4f}"
    assert 90.0 - 180.0 / W > 60.0 and 90.0 - (geom.top - geom.bottom) / (geom.H - 1) / 2 > 60.0
    e = np.deg2rad(np.linspace(geom.bottom, geom.top, H))
    # the projection's column is trunc(W / 2 - n) for the azimuth n columns from the middle: whole n are
    # the bin centres (at odd W, W / 2 - t itself would be the bins' edges)
    phi = (W // 2 - np.arange(W, dtype=np.float64)) * (2.0 * np.pi / W)
    t, i = [a.ravel() for a in np.meshgrid(np.arange(W), np.arange(H), indexing="ij")]
    j = (2 * (W // 2) - t) % W  # the projection's column of azimuth phi[t]
    keep = lv[i, j] >= 0
    t, i, j = t[keep], i[keep], j[keep]
    r = 8.0 * K ** lv[i, j].astype(np.float64)
    pts = np.empty((t.size, 4), np.float32)
    pts[:, 0] = r * np.cos(phi[t]) * np.cos(e[i])
    pts[:, 1] = r * np.sin(phi[t]) * np.cos(e[i])
    pts[:, 2] = r * np.sin(e[i])
    pts[:, 3] = 10.0 + (i * 7 + t) % 90
    return pts


def bfs_components(levels, label0_mask):
    """[H, W] int64: the number (from 0, in the order of the smallest linear index) of every label-0
    cell's component, -1 elsewhere. 4 neighbours, columns wrapping, rows not; two label-0 cells link
    when their levels are equal. Serial."""
    lv = np.asarray(levels, np.int64)
    H, W = lv.shape
    flat = lv.ravel().tolist()
    open_ = np.asarray(label0_mask, bool).ravel().tolist()
    comp = [-1] * (H * W)
    n = 0
    for seed in np.flatnonzero(np.asarray(label0_mask, bool).ravel()).tolist():
        if comp[seed] >= 0:
            continue
        comp[seed] = n
        queue = deque([seed])
        while queue:
            q = queue.popleft()
            i, j = divmod(q, W)
            v = flat[q]
            near = [i * W + (j + 1) % W, i * W + (j - 1) % W]
            if i + 1 < H:
                near.append(q + W)
            if i > 0:
                near.append(q - W)
            for p in near:
                if open_[p] and comp[p] < 0 and flat[p] == v:
                    comp[p] = n
                    queue.append(p)
        n += 1
    return np.asarray(comp, np.int64).reshape(H, W)


def bfs_labels(levels, label0_mask, point_num, line_num):
    """labelComponents restated: [H, W] int64, -1 where label0_mask is false, else the component's
    label. A component is kept when it has 30 cells, or point_num cells of which the pushed ones (all
    but the seed, the cell of the smallest linear index) lie in line_num rows; kept components are
    numbered from 1 in seed order, the cells of the others get 999999."""
    comp = bfs_components(levels, label0_mask)
    H, W = comp.shape
    lab = np.full((H, W), -1, np.int64)
    cells = np.flatnonzero(comp.ravel() >= 0).astype(np.int64)
    ids = comp.ravel()[cells]
    order = np.argsort(ids, kind="stable")  # cells of a component together, ascending linear index
    cells, ids = cells[order], ids[order]
    starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]]).astype(np.int64)
    ends = np.r_[starts[1:], np.int64(ids.size)]
    label = 0
    out = lab.ravel()
    for s, e in zip(starts.tolist(), ends.tolist()):
        size = e - s
        rows = np.unique(cells[s + 1:e] // W).size
        if size >= 30 or (size >= point_num and rows >= line_num):
            label += 1
            out[cells[s:e]] = label
        else:
            out[cells[s:e]] = BIG
    return lab


def rule_kept(cells, point_num=5, line_num=3):
    """The feasibility rule on one shape's own cells."""
    c = sorted((int(i), int(j)) for i, j in cells)
    return len(c) >= 30 or (len(c) >= point_num and len({i for i, _ in c[1:]}) >= line_num)


@dataclass
class Shape:
    cells: np.ndarray   # [n, 2] (row, column)
    kept: bool          # what the oracle has to say of it
    bands: tuple        # the bands it has cells in, as the scene states them


@dataclass
class Scene:
    levels: np.ndarray
    shapes: dict = field(default_factory=dict)   # name -> Shape: one component each, exactly these cells
    absent: dict = field(default_factory=dict)   # name -> (reason, the reason's condition at this geometry)
    over: dict = field(default_factory=dict)     # llsr_config overrides
    # column 0's first returns above cell (0, 0), which reads as empty in the ground pass: the oracle
    # takes one or two of them as ground; one that it leaves label 0 joins the shape next to it or is
    # a component of its own
    spare: tuple = ()


class _Canvas:
    """Draws shapes that may not touch (4 neighbours, column wrap) anything drawn before."""

    def __init__(self, geom, over=None):
        self.g = geom
        self.lv = np.full((geom.H, geom.W), -1, np.int64)
        self.scene = Scene(self.lv, over=dict(over or {}))
        self.x = 1  # next free column of the left-to-right layout (column 0 stays empty in rows >= 1)

    def fits(self, cells):
        H, W = self.g.H, self.g.W
        c = np.asarray(cells, np.int64).reshape(-1, 2)
        if c[:, 0].min() < 1 or c[:, 0].max() > H - 1 or c[:, 1].min() < 0 or c[:, 1].max() > W - 1:
            return False
        mine = np.zeros((H, W), bool)
        mine[c[:, 0], c[:, 1]] = True
        grown = mine | np.roll(mine, 1, 1) | np.roll(mine, -1, 1)
        grown[1:] |= mine[:-1]
        grown[:-1] |= mine[1:]
        return not (grown[1:] & (self.lv[1:] >= 0)).any()

    def put(self, name, cells, kept, bands, level=0):
        c = np.asarray(cells, np.int64).reshape(-1, 2)
        assert name not in self.scene.shapes and self.fits(c), f"{name} does not fit"
        assert len({(int(i), int(j)) for i, j in c}) == len(c)
        assert rule_kept(c, self.scene.over.get("segment_valid_point_num", 5),
                         self.scene.over.get("segment_valid_line_num", 3)) == kept, name
        self.lv[c[:, 0], c[:, 1]] = level
        self.scene.shapes[name] = Shape(c, kept, tuple(sorted(bands)))

    def take(self, width):
        """The first column of `width` free columns (and one empty column after them), or None."""
        x = self.x
        if x + width > self.g.W:
            return None
        self.x = x + width + 1
        return x

    def place(self, name, rel, row, width, kept, bands, level=0):
        """Shape `rel` (cells relative to (row, the next free column)) if its rows and columns exist."""
        H, W = self.g.H, self.g.W
        rows = [row + i for i, _ in rel]
        if min(rows) < 1 or max(rows) > H - 1:
            self.scene.absent[name] = (f"needs rows {min(rows)}..{max(rows)} of 1..{H - 1}",
                                       min(rows) < 1 or max(rows) > H - 1)
            return False
        x = self.take(width)
        if x is None:
            self.scene.absent[name] = (f"no {width} free columns left of {W}", self.x + width > W)
            return False
        self.put(name, [(row + i, x + j) for i, j in rel], kept, bands, level)
        return True

    def spares(self):
        self.lv[1, 0] = self.lv[2, 0] = 0
        self.scene.spare = ((1, 0), (2, 0))

    def done(self):
        """Row 0: every column's ground return, at the level of the column's shapes."""
        col = self.lv[1:].max(axis=0)
        low = np.where(self.lv[1:] >= 0, self.lv[1:], 99).min(axis=0)
        assert ((low == 99) | (low == col)).all(), "a column mixes levels"
        self.lv[0] = np.maximum(col, 0)
        self.lv.setflags(write=False)
        return self.scene


def _bset(g, rows):
    return {g.band_of(r) for r in rows}


def _one(g):
    cv = _Canvas(g)
    cells = [(i, j) for i in range(1, g.H) for j in range(g.W) if (i, j) not in ((1, 0), (2, 0))]
    cv.put("all", cells, True, range(len(bands(g.H, g.W))))
    cv.spares()
    return cv.done()


_FIVE = {  # the threshold shapes of test_gpu_label_columns.py; rows 0..2 (0..1), kept at 5 / 3
    "five_rows3_seed_alone": ([(0, 0), (1, 0), (2, 0), (2, 1), (2, 2)], False),
    "five_rows3_seed_pair": ([(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)], True),
    "five_rows2": ([(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)], False),
}


def _cross(g):
    """At every boundary: vertical runs of 5 (kept) and 4 (dropped) cells with the boundary between
    each pair of their rows in turn, and the three five-cell shapes with only their first row above
    the boundary (`_top`) and with only their last row below it (`_bot`)."""
    cv = _Canvas(g)
    for b in g.boundaries:
        k = g.band_of(b)
        for name, (rel, kept) in _FIVE.items():
            h = max(i for i, _ in rel) + 1
            w = max(j for _, j in rel) + 1
            cv.place(f"{name}_top@{b}", rel, b - 1, w, kept, {k - 1, k})
            if h > 2:
                cv.place(f"{name}_bot@{b}", rel, b - h + 1, w, kept, {k - 1, k})
        for n, kept in ((5, True), (4, False)):
            for t in range(n - 1):  # rows b - 1 - t .. : t + 1 cells above the boundary
                cv.place(f"run{n}_{t + 1}above@{b}", [(i, 0) for i in range(n)], b - 1 - t, 1, kept,
                         _bset(g, (b - 1, b + n - 2 - t)))
    return cv.done()


def _u_and_n(g):
    """`u`: two arms in band k - 1 joined only through a bar in band k (two band roots of band k - 1
    in one component, the left arm's head the seed); `n`: the bar in band k - 1, the arms in band k."""
    cv = _Canvas(g)
    for b in g.boundaries:
        k = g.band_of(b)
        u = [(i, j) for j in (0, 2) for i in range(-3, 0)] + [(0, 0), (0, 1), (0, 2)]
        cv.place(f"u@{b}", u, b, 3, True, {k - 1, k})
        a = min(3, g.H - b)  # the last band may be one row
        n = [(-1, 0), (-1, 1), (-1, 2)] + [(i, j) for j in (0, 2) for i in range(a)]
        cv.place(f"n@{b}", n, b, 3, a >= 2, {k - 1, k})  # one-cell arms: 5 cells, pushed rows b - 1 and b
    return cv.done()


def _comb(g, down):
    """Teeth of 4 cells (as many as the band below has rows, for comb_up) in every other column and a
    bar: comb_down has the teeth above the boundary and the bar below it, comb_up the bar above."""
    cv = _Canvas(g)
    bs = g.boundaries
    teeth = min(200, (g.W - 4) // 2)
    for b in dict.fromkeys((bs[0], bs[-1])):
        k = g.band_of(b)
        if down:
            rel = [(i, 2 * t) for t in range(teeth) for i in range(-4, 0)] + [(0, j) for j in range(2 * teeth - 1)]
        else:
            a = min(4, g.H - b)
            rel = [(-1, j) for j in range(2 * teeth - 1)] + [(i, 2 * t) for t in range(teeth) for i in range(a)]
        cv.x = 1
        # (teeth of one cell below the bar: two pushed rows, kept only from 30 cells)
        cv.place(f"comb@{b}", rel, b, 2 * teeth - 1, down or a >= 2 or len(rel) >= 30, {k - 1, k})
    return cv.done()


def _stairs(g):
    """A staircase one cell wide from row 1 to row H - 1, through every band: down to the left (the
    smallest cell is in the rightmost column) and, at level 1, down to the right."""
    cv = _Canvas(g)
    n = g.H - 2
    allb = range(len(bands(g.H, g.W)))
    left = [(1 + s + d, n - 1 - s) for s in range(n) for d in (0, 1)]
    right = [(1 + s + d, s) for s in range(n) for d in (0, 1)]
    cv.place("down_left", sorted(set(left)), 0, n, True, allb)
    cv.place("down_right", sorted(set(right)), 0, n, True, allb, level=1)
    return cv.done()


def _wrap(g):
    """`ring`: three rows of six cells that are one component only over column W - 1 -> 0, inside
    band 0; `hook`: a row over the wrap just above the last boundary, an arm up at its left end and
    an arm down over the boundary at its right end."""
    cv = _Canvas(g)
    W = g.W
    cols = [W - 3, W - 2, W - 1, 0, 1, 2]
    cv.put("ring", [(i, j) for i in (3, 4, 5) for j in cols], True, {0})
    b = g.boundaries[-1]
    a = min(3, g.H - b)
    hook = [(b - 1, j) for j in cols] + [(b - 2, W - 3)] + [(b + i, 2) for i in range(a)]
    if cv.fits(hook + [(b - 3, W - 3)]):  # (a second cell of the arm up where the ring leaves room)
        hook.append((b - 3, W - 3))
    cv.put("hook", hook, True, {g.band_of(b) - 1, g.band_of(b)})
    cv.spares()
    return cv.done()


def _thirty(g):
    """Two rows of 15 + 15 cells (kept: 30) and of 15 + 14 cells (dropped: 29 over two rows) with
    the boundary between them, at every boundary; 30 and 29 cells in one row of the last band."""
    cv = _Canvas(g)
    for b in g.boundaries:
        k = g.band_of(b)
        blk = [(i, j) for i in (-1, 0) for j in range(15)]
        cv.place(f"block30@{b}", blk, b, 15, True, {k - 1, k})
        cv.place(f"block29@{b}", blk[:-1], b, 15, False, {k - 1, k})
    last = len(bands(g.H, g.W)) - 1
    for n, kept in ((30, True), (29, False)):
        row = g.H - 1
        if g.W < n + 4:
            cv.scene.absent[f"row{n}_last_band"] = (f"{n} cells and the margins do not fit {g.W} columns", g.W < n + 4)
        else:
            cv.place(f"row{n}_last_band", [(0, j) for j in range(n)], row, n, kept, {last})
    return cv.done()


def _last_row(g):
    """Components in row H - 1 alone (5 cells: dropped; 30: kept where W allows) and columns of 5 and
    4 cells hanging into it from above."""
    cv = _Canvas(g)
    H = g.H
    cv.place("col5", [(i, 0) for i in range(5)], H - 5, 1, True, _bset(g, (H - 5, H - 1)))
    cv.place("col4", [(i, 0) for i in range(4)], H - 4, 1, False, _bset(g, (H - 4, H - 1)))
    cv.place("row5", [(0, j) for j in range(5)], H - 1, 5, False, _bset(g, (H - 1,)))
    cv.place("row30", [(0, j) for j in range(30)], H - 1, 30, True, _bset(g, (H - 1,)))
    cv.place("ell", [(i, 0) for i in range(-3, 1)] + [(0, 1), (0, 2)], H - 1, 3, True, _bset(g, (H - 4, H - 1)))
    return cv.done()


def _lines17(g):
    """segment_valid_line_num 17: vertical runs of 18 cells (17 pushed rows: kept) and of 17 cells
    (16: dropped), over one boundary and over two, and ending in row H - 1."""
    cv = _Canvas(g, dict(segment_valid_line_num=17))
    if g.H < 19:
        cv.scene.absent["runs"] = (f"no 18 rows in 1..{g.H - 1}", g.H - 1 < 18)
        return cv.done()
    R = g.R
    for b in g.boundaries:
        for n, kept in ((18, True), (17, False)):
            top = max(1, b - n // 2)
            rows = (top, top + n - 1)
            cv.place(f"run{n}_mid@{b}", [(i, 0) for i in range(n)], top, 1, kept,
                     set(range(g.band_of(rows[0]), g.band_of(rows[1]) + 1)))
            if R + 2 <= n:  # rows b - 1 .. b + R: both boundaries of band k
                if b + R >= g.H:
                    cv.scene.absent[f"run{n}_two@{b}"] = (f"the band from row {b} is the last", b + R >= g.H)
                    continue
                top = b + R + 1 - n
                rows = (top, top + n - 1)
                cv.place(f"run{n}_two@{b}", [(i, 0) for i in range(n)], top, 1, kept,
                         set(range(g.band_of(rows[0]), g.band_of(rows[1]) + 1)))
            else:
                cv.scene.absent[f"run{n}_two@{b}"] = (f"{n} cells span no whole band of {R} rows", R + 2 > n)
    for n, kept in ((18, True), (17, False)):
        cv.place(f"run{n}_last_row", [(i, 0) for i in range(n)], g.H - n, 1, kept,
                 set(range(g.band_of(g.H - n), g.band_of(g.H - 1) + 1)))
    return cv.done()


def _tile_ends(g):
    """Kept columns of 5 cells whose seeds sit at the linear indices 4096 m - 1 (`end`) and 4096 m
    (`start`): the rank scan's tiles of 4 x 1024 cells; those of even m also end and start the sweeps
    of 8 x 1024 cells. Up to three of each kind for odd and for even m."""
    cv = _Canvas(g)
    H, W = g.H, g.W
    cv.spares()  # for the seeds in column 0
    found = {}
    for m in range(1, H * W // 4096 + 1):
        # (the two cells are neighbours: each m gives one of them, which one comes first alternates)
        for kind, q in (("end", 4096 * m - 1), ("start", 4096 * m))[::1 if (m // 2) % 2 == 0 else -1]:
            i, j = divmod(q, W)
            cells = [(i + d, j) for d in range(5)]
            key = (kind, 4096 << (m % 2 == 0))
            if found.get(key, 0) < 3 and cv.fits(cells):
                cv.put(f"{kind}{q}", cells, True, _bset(g, (i, i + 4)))
                found[key] = found.get(key, 0) + 1
    for kind in ("end", "start"):
        for T in (4096, 8192):
            if not found.get((kind, T)):
                cv.scene.absent[f"{kind}{T}"] = (f"no column of 5 cells can {kind} a tile of {T} cells in {H} x {W}",
                                                 H * W < T + 5 * W)
    return cv.done()


def _singles(g):
    """Single cells every third row and column: every one a seed, no edge, all 999999."""
    cv = _Canvas(g)
    for i in range(1, g.H, 3):
        for j in range(1, g.W - 1, 3):
            cv.lv[i, j] = 0
    return cv.done()


SCENES = {
    "one": _one, "cross": _cross, "u_and_n": _u_and_n, "comb_down": lambda g: _comb(g, True),
    "comb_up": lambda g: _comb(g, False), "stairs": _stairs, "wrap": _wrap, "thirty": _thirty,
    "last_row": _last_row, "lines17": _lines17, "tile_ends": _tile_ends, "singles": _singles,
}
PAIRS = [(gn, sn) for gn in GEOMS for sn in SCENES]


@functools.lru_cache(maxsize=None)
def scene(gname, sname):
    return SCENES[sname](GEOMS[gname])


def case(gname, sname):
    g = GEOMS[gname]
    return cc.Case((g.H, g.W, g.bottom, g.top), dict(scene(gname, sname).over), kitti=g.kitti)


@functools.lru_cache(maxsize=None)
def scan(gname, sname):
    """The scene's raw scan (cached, read-only)."""
    pts = points(scene(gname, sname).levels, GEOMS[gname])
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def oracle(gname, sname):
    """The oracle's outputs on the scene through a fresh oracle (cached: the CPU and the GPU tests
    share them; read-only)."""
    import oracle_py
    return oracle_py.Oracle(cc.config(case(gname, sname))).process(scan(gname, sname))


@functools.lru_cache(maxsize=None)
def bfs(gname, sname):
    """bfs_labels over the oracle's own label-0 mask, at the scene's thresholds (cached)."""
    g, sc = GEOMS[gname], scene(gname, sname)
    cfg = cc.config(case(gname, sname))
    lab = np.asarray(oracle(gname, sname)["label_image"]).reshape(g.H, g.W)
    out = bfs_labels(sc.levels, lab != -1, cfg.segment_valid_point_num, cfg.segment_valid_line_num)
    out.setflags(write=False)
    return out
