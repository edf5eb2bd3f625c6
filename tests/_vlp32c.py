"""Independent numpy statement of the reference's use_vlp32c branch, for the tests of that branch.

The oracle refuses use_vlp32c, so the expected side of the new branch is stated here:

* `project(cfg, pts)`: projectPointCloud's use_vlp32c branch (imageProjection.cpp:349-427) with the
  two definitions of include/llsr.h (a rank >= H claims no cell; range == 0 sets no bin);
* `column_pass(cfg, full_cloud, rule)`: groundRemovalOurs' per-column test and Filter (IP:524-629),
  `_ground_mat` before ADD / ELEVATION / NEAR, for the ground angle rule 12.5, 25 or "60/25".

Exactness: float32 + - * / sqrt in numpy are correctly rounded and never fused, like the reference's
x86-64 build; asinf, atan2f and acosf are the host glibc's own (libm.so.6 through ctypes), which is
what the reference calls. Every expression keeps the reference's types and order.
"""
import ctypes

import numpy as np

F = np.float32
DEG_TO_RAD = np.pi / 180.0  # utility.h:49, a double
INT_MIN = -2 ** 31
FLT_MAX = np.finfo(np.float32).max

_libm = ctypes.CDLL("libm.so.6")
for _name, _n in (("asinf", 1), ("acosf", 1), ("atan2f", 2)):
    _f = getattr(_libm, _name)
    _f.restype = ctypes.c_float
    _f.argtypes = [ctypes.c_float] * _n


def _libm1(name, a):
    f = getattr(_libm, name)
    return np.array([f(float(v)) for v in np.asarray(a, F).ravel()], F).reshape(np.shape(a))


def _libm2(name, a, b):
    f = getattr(_libm, name)
    return np.array([f(float(u), float(v)) for u, v in zip(np.asarray(a, F).ravel(), np.asarray(b, F).ravel())],
                    F).reshape(np.shape(a))


def _trunc_i32(q):
    """(int)double as x86-64's cvttsd2si does it: NaN and out-of-range give INT_MIN."""
    q = np.asarray(q, np.float64)
    bad = ~((q > -2147483649.0) & (q < 2147483648.0))
    return np.where(bad, INT_MIN, np.trunc(np.where(bad, 0.0, q))).astype(np.int64)


def _c_round(v):
    """C's round(): halves away from zero (np.round goes to even)."""
    return np.copysign(np.floor(np.abs(v) + 0.5), v)


def ang_bottom(cfg) -> np.float32:
    """_ang_bottom after IP:119, stored to float."""
    return F(-(float(cfg.vertical_angle_bottom) - 0.1) * DEG_TO_RAD)


def bins_of(cfg, pts):
    """temp of IP:354-356 for every raw point; INT_MIN for the points removeNaNFromPointCloud drops
    (IP:198) and, by definition 2, for range == 0. Also returns the float range."""
    pts = np.asarray(pts, F).reshape(-1, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    with np.errstate(all="ignore"):
        rng = np.sqrt(x * x + y * y + z * z)
        va = _libm1("asinf", z / rng)
        q = (va + ang_bottom(cfg)).astype(np.float64) / (0.335 * DEG_TO_RAD)
    temp = _trunc_i32(q)
    temp[~finite] = INT_MIN
    return temp, rng, finite


def project(cfg, pts) -> dict:
    """IP:349-427. Returns per raw point `bins` (temp; INT_MIN = none), `row` and `col` (-1 = none),
    `placed`; `vertical_raw2`; and per cell `range_image`, `cell_point` (raw index, -1 = empty) and
    `full_cloud` ([H * W, 4]: x, y, z, intensity row + col / 10000; NaN, NaN, NaN, 0 where empty)."""
    pts = np.asarray(pts, F).reshape(-1, 4)
    H, W = cfg.num_vertical_scans, cfg.num_horizontal_scans
    temp, rng, finite = bins_of(cfg, pts)
    raw2 = np.unique(temp[temp >= 0])                       # IP:366-369
    row = np.where(temp >= 0, np.searchsorted(raw2, temp), -1)   # IP:397-403
    res_x = F((np.pi * 2) / W)                              # IP:117
    with np.errstate(all="ignore"):
        ha = _libm2("atan2f", pts[:, 0], pts[:, 1])        # IP:404
        v = -_c_round((ha.astype(np.float64) - np.pi / 2) / np.float64(res_x)) + W * 0.5
    col = _trunc_i32(v)
    col = np.where(col >= W, col - W, col)                  # IP:406-408
    col_ok = (col >= 0) & (col < W)
    near = rng.astype(np.float64) < 0.1                     # IP:412
    placed = finite & (temp >= 0) & col_ok & ~near & (row < H)   # row < H: definition 1
    cell_point = np.full(H * W, -1, np.int32)
    idx = np.nonzero(placed)[0]
    cells = (col[idx] + row[idx] * W).astype(np.int64)
    np.maximum.at(cell_point, cells, idx.astype(np.int32))  # IP:415-425: the last writer wins
    won = cell_point >= 0
    range_image = np.full(H * W, FLT_MAX, F)
    range_image[won] = rng[cell_point[won]]
    full = np.full((H * W, 4), np.nan, F)
    full[:, 3] = 0.0
    full[won, :3] = pts[cell_point[won], :3]
    cw = np.nonzero(won)[0]
    full[won, 3] = ((cw // W).astype(F).astype(np.float64) + (cw % W).astype(F).astype(np.float64) / 10000.0).astype(F)
    return {"bins": temp, "vertical_raw2": raw2.astype(np.int32), "row": row, "col": np.where(col_ok, col, -1),
            "placed": placed, "range_image": range_image, "cell_point": cell_point, "full_cloud": full}


def column_pass(cfg, full_cloud, rule) -> np.ndarray:
    """_ground_mat [H, W] after IP:524-629 (the column test and Filter). rule: 12.5, 25 or "60/25"
    (use_kitti: 60 below row 16, else 25)."""
    H, W = cfg.num_vertical_scans, cfg.num_horizontal_scans
    fc = np.asarray(full_cloud, F).reshape(H, W, 4)
    g = np.full((H, W), -1, np.int8)
    have = np.zeros(W, bool)
    rv = np.zeros((3, W), F)
    low = np.zeros((3, W), F)
    with np.errstate(all="ignore"):
        for i in range(H):
            p = fc[i, :, :3].T                               # [3, W]
            valid = fc[i, :, 3] != 0                         # IP:535
            first = valid & ~have
            rest = valid & have
            d0 = np.sqrt(p[0] * p[0] + p[1] * p[1])
            rv[0] = np.where(first, p[0] / d0, rv[0])
            rv[1] = np.where(first, p[1] / d0, rv[1])
            rv[2] = np.where(first, F(0), rv[2])
            tv = p - low
            num = tv[0] * rv[0] + tv[1] * rv[1] + tv[2] * rv[2]
            den = np.sqrt(tv[0] * tv[0] + tv[1] * tv[1] + tv[2] * tv[2]) * np.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2])
            x = np.where(rest, num / den, F(1))
            ang = (_libm1("acosf", x).astype(np.float64) / DEG_TO_RAD).astype(F)   # IP:559
            D = F((60.0 if i < 16 else 25.0) if rule == "60/25" else rule)
            ok = rest & (ang <= D)
            rv = np.where(ok[None, :], rv + tv, rv)
            g[i] = np.where(first | ok, 1, np.where(rest, 0, -1))
            low = np.where(valid[None, :], p, low)
            have |= first
    obs = np.maximum.accumulate(g == 0, axis=0)               # Filter, IP:620-628
    g[(g == 1) & obs] = 2
    return g


def check_invariants(col_g, final_g, full_cloud, cfg) -> list:
    """The three ties between the column pass and the final ground image: ADD and ELEVATION touch
    only 2s and NEAR only cells with xy-depth <= 5 (IP:631-735). Returns mismatch descriptions."""
    H, W = cfg.num_vertical_scans, cfg.num_horizontal_scans
    fc = np.asarray(full_cloud, F).reshape(H, W, 4)
    fin = np.asarray(final_g).reshape(H, W)
    with np.errstate(all="ignore"):
        far = np.sqrt(fc[..., 0] * fc[..., 0] + fc[..., 1] * fc[..., 1]) > F(5)   # IP:705, 710: not depth <= 5
    errs = []
    for name, m, want in (("0 => 0", col_g == 0, 0), ("-1 => -1", col_g == -1, -1), ("far 1 => 1", (col_g == 1) & far, 1)):
        bad = m & (fin != want)
        if bad.any():
            i, j = np.argwhere(bad)[0]
            errs.append(f"{name}: {int(bad.sum())} cells, first (row {i}, col {j}) final {fin[i, j]}")
    return errs


# ---- shared inputs of tests/test_vlp32c_host.py and tests/test_gpu_vlp32c.py ---------------------
def config(**over):
    """The shipped VLP-32c block (loam_config.yaml:69-135) with field overrides, a fresh copy."""
    from llsr import _abi
    c = _abi.config_for("vlp32c")
    for k, v in over.items():
        setattr(c, k, v)
    return c


_SCANS = {}


def scan(layout: str, seed: int = 3, **kw):
    """synth.make_scan(seed, layout, **kw), ray-cast once per test session (read-only)."""
    from llsr import synth
    key = (layout, seed, tuple(sorted(kw.items())))
    if key not in _SCANS:
        a = synth.make_scan(seed, layout, **kw)
        a.setflags(write=False)
        _SCANS[key] = a
    return _SCANS[key]
