"""The image-projection tail, k_ground_add and k_label, at the geometries where their lane, word and
block boundaries fall: ground image, label image and the two counts against the CPU oracle, bit-exact.

k_ground_add computes its add_test bits with lanes on interleaved columns (64 columns a mask word) and
scans chunks of ceil(W / 64) columns per lane; k_label<true> loads the range image in blocks of 64
columns, a column per lane, and adds a component's size once per run of neighbouring lanes. The cases:

    w65      16 x 65    one column beyond a wave: a block (and a mask word) of one column
    w130     16 x 130   two full blocks and one of two columns
    w321     16 x 321   five blocks and one column, at a width where add_test can pass (see below)
    h3_w64   3 x 64     H no multiple of 4, W exactly one wave (ground_scan_index 1)
    h2_w16   2 x 16     ADD's columns j < 2 and W - 3 within one lane chunk
    w1799    16 x 1799  odd W: the last block holds 7 columns, rows start at odd offsets
    w2000    16 x 2000  HW = 32000, the largest image k_label<true> takes
    h64      64 x 2048  k_ground_add with a full LDS row and 32 mask words (k_label<false> labels it)

Each case runs a flat hall scan without dropout (walls all round: components that close over the
column wrap W - 1 -> 0, long ground runs up to the walls) and a street scan (single-cell components,
components at the 30-cell and the segment_valid_point_num / segment_valid_line_num thresholds, ground
broken by kerbs and cars, so ADD has many `2` cells to promote). test_oracle_reaches_the_paths proves
on the oracle alone, without a GPU, that no case passes vacuously: a kept component holds cells in
column 0 and in column W - 1, and ADD changed a cell in a column >= 64. The oracle exposes neither its
ground bytes before ADD nor a switch for add_test, so ADD's effect is restated here: the column pass,
ADD's two loops and the elevation pass in numpy over the oracle's own cell -> point map, and that
restatement must give the oracle's ground image in every cell the later near-ground RANSAC cannot
touch (horizontal depth > 5 m).

Where a condition cannot hold, the test says so instead of passing silently:
  - add_test asks |p[j] - p[j +- 2]| <= 0.061 |p[j]|. Two columns are 4 pi / W rad apart, so with every
    beam at its bin centre no cell can pass below W = 207: at 16 x 65 and 16 x 130 (and 3 x 64,
    2 x 16) ADD changes nothing, which is asserted; there the kernel's candidate masks are all zero
    and the ground image still has to come out equal. w321 is the narrow image in which ADD works.
  - A column's first return is always ground, and cell (0, 0) reads as empty (its fullCloud
    intensity is 0), so in a 2-row image (1, 0) and (0, W - 1) are ground: no label-0
    component can hold cells in column 0 and in column W - 1, and h2_w16 has no wrap condition. The thresholds of the two small images are lowered (segment_valid_line_num 1,
    segment_valid_point_num 2 at 2 x 16) so that they keep components at all.
  - h64 is there for k_ground_add; its labels come from k_label<false> and carry no wrap condition.
"""
import functools

import numpy as np
import pytest

import _config_cases as cc

_HALL = dict(hall=8.0, dropout=0.0)
_STREET = dict()
_VLP = (-15.0, 15.0)

# name -> (Case, ((seed, scan keywords), ...)); the seeds were searched on the CPU for the two conditions
CASES = {
    "w65": (cc.Case((16, 65) + _VLP), ((1, _HALL), (2, _STREET))),
    "w130": (cc.Case((16, 130) + _VLP), ((1, _HALL), (2, _STREET))),
    "w321": (cc.Case((16, 321) + _VLP), ((1, _HALL), (2, _STREET))),
    "h3_w64": (cc.Case((3, 64, -15.0, 3.0), dict(ground_scan_index=1, segment_valid_line_num=1)),
               ((1, _HALL), (2, _STREET))),
    "h2_w16": (cc.Case((2, 16, -1.0, 10.0), dict(ground_scan_index=0, segment_valid_point_num=2,
                                                 segment_valid_line_num=1)), ((1, _HALL), (2, _STREET))),
    "w1799": (cc.Case((16, 1799) + _VLP), ((1, _HALL), (2, _STREET))),
    "w2000": (cc.Case((16, 2000) + _VLP), ((1, _HALL), (2, _STREET))),
    "h64": (cc.Case(cc.HDL64E_GEOM, kitti=True), ((5, _STREET),)),
}
KEYS = ("ground_image", "label_image", "n_segmented", "n_outlier")


@functools.lru_cache(maxsize=None)
def _scans(name):
    case, draws = CASES[name]
    out = tuple(cc.scan(seed, *case.geom, **kw) for seed, kw in draws)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's outputs on the case's scans, a fresh oracle per scan (cached and shared by the CPU
    and the GPU test; read-only)."""
    import oracle_py
    cfg = cc.config(CASES[name][0])
    return tuple(oracle_py.Oracle(cfg).process(p) for p in _scans(name))


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _ground_restated(cfg, pts, out):
    """groundRemovalOurs up to the elevation pass (IP:524-698) in float32 numpy over the oracle's
    cell -> point map. Returns (ground bytes after the elevation pass, cells ADD turned from 2 to 1,
    horizontal depth per cell), each [H, W]."""
    H, W = cfg.num_vertical_scans, cfg.num_horizontal_scans
    cp = np.asarray(out["cell_point"]).reshape(H, W)
    valid = cp >= 0
    valid[0, 0] = False  # fullCloud intensity row + col / 10000 == 0 reads as "empty" (IP:540)
    xyz = np.full((H, W, 3), np.nan, np.float32)
    xyz[cp >= 0] = np.asarray(pts, np.float32)[cp[cp >= 0], :3]
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    g = np.full((H, W), -1, np.int8)
    have = np.zeros(W, bool)
    rv = np.zeros((W, 3), np.float32)
    low = np.zeros((W, 3), np.float32)
    with np.errstate(all="ignore"):
        for i in range(H):
            m = valid[i]
            first, rest = m & ~have, m & have
            d0 = np.sqrt(x[i] * x[i] + y[i] * y[i])
            tv = xyz[i] - low
            dot = tv[:, 0] * rv[:, 0] + tv[:, 1] * rv[:, 1] + tv[:, 2] * rv[:, 2]
            den = np.sqrt(tv[:, 0] * tv[:, 0] + tv[:, 1] * tv[:, 1] + tv[:, 2] * tv[:, 2]) * \
                np.sqrt(rv[:, 0] * rv[:, 0] + rv[:, 1] * rv[:, 1] + rv[:, 2] * rv[:, 2])
            ang = _f32(np.arccos(_f32(dot / den)).astype(np.float64) / (np.pi / 180.0))
            lim = (60.0 if i < 16 else 25.0) if cfg.use_kitti else 12.5
            ok = rest & (ang <= np.float32(lim))
            g[i, first | ok] = 1
            g[i, rest & ~ok] = 0
            rv[ok] += tv[ok]
            rv[first] = np.stack([x[i] / d0, y[i] / d0, np.zeros(W, np.float32)], axis=1)[first]
            low[m] = xyz[i][m]
            have |= m
        obs = np.zeros(W, bool)
        for i in range(H):
            obs |= g[i] == 0
            g[i, obs & (g[i] == 1)] = 2
        # ADD (IP:631-671): both add_test results of every cell up front, then the two serial loops
        r = np.sqrt(x * x + y * y + z * z)

        def add_test(shift):
            q = np.roll(xyz, shift, axis=1)
            dx, dy, dz = x - q[..., 0], y - q[..., 1], z - q[..., 2]
            dr = np.sqrt(dx * dx + dy * dy + dz * dz)
            return (dr.astype(np.float64) <= 0.061 * r.astype(np.float64)) & (dz.astype(np.float64) <= 0.1)
        tf, tb = add_test(2), add_test(-2)
    before = g.copy()
    for i in range(H):
        row = g[i]
        for j in range(2, W):
            if row[j] == 2 and (row[j - 2] == 1 or row[j - 1] == 1) and tf[i, j]:
                row[j] = 1
        for j in range(W - 3, -1, -1):
            if row[j] == 2 and (row[j + 2] == 1 or row[j + 1] == 1) and tb[i, j]:
                row[j] = 1
    promoted = (before == 2) & (g == 1)
    # ELEVATION (IP:673-698): last-valid carry across columns
    eht = eh = np.float32(-1.3)
    for j in range(W):
        ones = np.nonzero(g[:, j] == 1)[0]
        if ones.size:
            eht = z[ones[-1], j]
        if ones.size >= 5:
            eh = eht
        two = g[:, j] == 2
        g[two, j] = (z[two, j].astype(np.float64) < float(eh) + 0.3).astype(np.int8)
    with np.errstate(all="ignore"):
        depth = np.sqrt(x * x + y * y)
    return g, promoted, depth


def _wrap_components(out, H, W):
    """Kept components of the label image (one label each) with cells in column 0 and in column W - 1."""
    lab = np.asarray(out["label_image"]).reshape(H, W)
    both = np.intersect1d(lab[:, 0], lab[:, W - 1])
    return [int(v) for v in both if 0 < v < 999999]


@functools.lru_cache(maxsize=None)
def _reach(name):
    """(kept components over the column wrap, cells ADD changed in columns >= 64 (any column where
    W <= 64), cells where the restated ground differs from the oracle's beyond 5 m), summed over the
    case's scans."""
    case = CASES[name][0]
    cfg = cc.config(case)
    H, W = case.geom[:2]
    wrap = changed = differ = 0
    for pts, o in zip(_scans(name), _oracle(name)):
        wrap += len(_wrap_components(o, H, W))
        g, promoted, depth = _ground_restated(cfg, pts, o)
        changed += int(promoted[:, 64:].sum() if W > 64 else promoted.sum())
        far = depth > 5.0
        differ += int((g[far] != np.asarray(o["ground_image"]).reshape(H, W)[far]).sum())
    return wrap, changed, differ


NO_WRAP = ("h2_w16", "h64")
ADD_MIN_W = 207  # 4 pi / W <= 0.061


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_reaches_the_paths(name):
    wrap, changed, differ = _reach(name)
    H, W = CASES[name][0].geom[:2]
    assert differ == 0, f"{name}: the restated ground pass differs from the oracle's in {differ} cells beyond 5 m"
    if name not in NO_WRAP:
        assert wrap > 0, f"{name}: no kept component holds cells in column 0 and column {W - 1}"
    if W >= ADD_MIN_W:
        assert changed > 0, f"{name}: ADD changed no cell in a column >= 64"
    else:
        assert changed == 0, f"{name}: ADD changed {changed} cells at W = {W}, below {ADD_MIN_W} columns"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_ground_and_labels_bit_exact(require_gpu, name):
    from llsr import Pipeline
    case = CASES[name][0]
    cfg = cc.config(case)
    failures = []
    for k, (pts, o) in enumerate(zip(_scans(name), _oracle(name))):
        pipe = Pipeline(cfg, max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
        g = pipe.process_scan(pts)
        pipe.close()
        for key in KEYS:
            if not np.array_equal(np.asarray(g[key]), np.asarray(o[key])):
                bad = np.nonzero(np.asarray(g[key]) != np.asarray(o[key]))[0] if np.ndim(o[key]) else []
                failures.append(f"scan {k} (seed {CASES[name][1][k][0]}): {key} differs"
                                + (f" in {len(bad)} cells, first {bad[:5].tolist()}: gpu "
                                   f"{np.asarray(g[key])[bad[:5]].tolist()} oracle {np.asarray(o[key])[bad[:5]].tolist()}"
                                   if len(bad) else f": gpu {g[key]} oracle {o[key]}"))
    assert not failures, f"{name}:\n" + "\n".join(failures)
