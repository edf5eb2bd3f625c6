"""Scans and cases for the parity tests across the configurations llsr_create accepts.

Helpers only: nothing here calls the product library or the oracle at import. `CASES` maps a name
to a `Case`: the range-image geometry, the llsr_config overrides, the scan seeds and a predicate on
the ORACLE's outputs which proves that the case reaches the code path it is there for
(tests/test_config_oracle.py asserts it on the CPU; tests/test_gpu_config_parity.py compares the
device with the oracle on the same scans). DESIGN.md §"Configuration cases" lists what each case
reaches and the oracle's counts.
"""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass, field

import numpy as np

VLP16_GEOM = (16, 1800, -15.0, 15.0)
HDL64E_GEOM = (64, 2048, -24.8, 2.0)
H32_GEOM = (32, 1024, -25.0, 15.0)
H17_GEOM = (17, 1800, -16.0, 16.0)


def scan(seed, H, W, bottom_deg, top_deg, hall=None, dropout=0.02, motion=False):
    """One raw scan, float32 [H * W, 4], of a sensor with H rings spaced evenly from bottom_deg to
    top_deg (fired bottom to top) and W columns phi = (W / 2 - t) * 2 pi / W, azimuth-major, cast
    through synth._Scene: sensor position, noise, dropout and intensity as synth.make_scan draws
    them, `motion` as make_scan applies synth.sensor_attitude. Every beam points at its range-image
    bin centre (row value r + 0.1 deg / resolution)."""
    from llsr import synth
    rng = np.random.default_rng(seed)
    scene = synth._Scene(np.random.default_rng(1000003 + seed // 64), None, hall)
    e = np.deg2rad(np.linspace(bottom_deg, top_deg, H))
    phi = (W / 2 - np.arange(W, dtype=np.float64)) * (2.0 * np.pi / W)
    ce, se = np.cos(e), np.sin(e)
    d = np.empty((W, H, 3))
    d[:, :, 0] = np.cos(phi)[:, None] * ce[None, :]
    d[:, :, 1] = np.sin(phi)[:, None] * ce[None, :]
    d[:, :, 2] = se[None, :]
    d = d.reshape(-1, 3)
    origin = np.array([0.5 * (seed % 64), rng.uniform(-0.5, 0.5), 0.0])
    if motion:
        dz, roll, pitch, yaw = synth.sensor_attitude(seed)
        origin[2] += dz
        t = scene.cast(origin, d @ synth._rot_zyx(roll, pitch, yaw).T, 100.0)
    else:
        t = scene.cast(origin, d, 100.0)
    r = t + rng.normal(0.0, 0.01, size=t.shape)
    drop = rng.random(t.shape) < dropout
    r[drop | ~np.isfinite(t)] = np.nan
    pts = np.empty((d.shape[0], 4), dtype=np.float32)
    pts[:, :3] = (d * r[:, None]).astype(np.float32)
    pts[:, 3] = rng.integers(0, 101, size=t.shape).astype(np.float32)
    return pts


@dataclass(frozen=True)
class Case:
    geom: tuple                      # (H, W, bottom_deg, top_deg)
    over: dict = field(default_factory=dict)   # llsr_config fields set after the geometry
    seeds: tuple = (1, 2)
    kitti: bool = False              # start from the HDL-64E block instead of the VLP-16 one
    scan_kw: dict = field(default_factory=dict)  # scan()'s hall / dropout
    expect: object = None            # predicate(case, oracle outputs) -> (ok, what the oracle gave)
    odometry: bool = False           # OracleOdometry on motion=True scans, LLSR_MODE_LM_APPLIED


def config(case):
    """The llsr_config of a case (its name or the Case): the VLP-16 block, or the HDL-64E block for
    the cases marked kitti, with H, W, both elevation angles and the case's overrides."""
    from llsr import _abi, default_config
    c = CASES[case] if isinstance(case, str) else case
    cfg = default_config("hdl64e" if c.kitti else "vlp16")
    H, W, bottom, top = c.geom
    cfg.num_vertical_scans, cfg.num_horizontal_scans = H, W
    cfg.vertical_angle_bottom, cfg.vertical_angle_top = bottom, top
    for k, v in c.over.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    if c.odometry:
        cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    return cfg


@functools.lru_cache(maxsize=None)
def _scans(name):
    c = CASES[name]
    out = tuple(scan(s, *c.geom, motion=c.odometry, **c.scan_kw) for s in c.seeds)
    for a in out:
        a.setflags(write=False)
    return out


def scans(name):
    """The case's raw scans, one per seed (cached, read-only)."""
    return _scans(name)


def _run(case, scan_list):
    import oracle_py
    cfg = config(case)
    ora = (oracle_py.OracleOdometry if case.odometry else oracle_py.Oracle)(cfg)
    return [copy.deepcopy(ora.process(p)) for p in scan_list]


@functools.lru_cache(maxsize=None)
def oracle_outputs(name):
    """The oracle's outputs on the case's scans through one oracle handle (cached: the CPU and the
    GPU test of a case share them; treat them as read-only)."""
    return _run(CASES[name], scans(name))


@functools.lru_cache(maxsize=None)
def baseline_outputs(name, keep=()):
    """The oracle on the same scans with the case's overrides left out, but for those in `keep`."""
    c = CASES[name]
    base = Case(c.geom, {k: v for k, v in c.over.items() if k in keep}, c.seeds, c.kitti, c.scan_kw, None, c.odometry)
    return _run(base, scans(name))


# ---- predicates: (case name, oracle outputs) -> (holds, description of what the oracle gave) ----

def _counts(outs, key):
    return [o[key] for o in outs]


def count_all(key, test, text):
    def p(name, outs):
        v = _counts(outs, key)
        return all(test(x) for x in v), f"{key} {v}, expected {text}"
    return p


def _less_sharp_between(lo, hi):
    return count_all("n_less_sharp", lambda m: lo < m <= hi, f"{lo} < M <= {hi}")


def _smallest(name, outs):
    feats = [o["n_less_sharp"] + o["n_sharp"] + o["n_flat"] + o["n_less_flat"] for o in outs]
    return all(o["n_segmented"] > 0 for o in outs) and not any(feats), \
        f"n_segmented {_counts(outs, 'n_segmented')}, features {feats}"


def _clusters(label_image, H, W):
    """{label: (points, rows)} of the kept clusters of a label image."""
    lab = np.asarray(label_image).reshape(H, W)
    out = {}
    for v in np.unique(lab):
        if v <= 0 or v == 999999:
            continue
        m = lab == v
        out[int(v)] = (int(m.sum()), int(m.any(axis=1).sum()))
    return out


def _bands_16bit(name, outs):
    """A kept cluster of fewer than 30 points (it passed the line test: 17 rows or more), and a
    cluster of fewer than 30 points which segment_valid_line_num 3 keeps and 17 drops."""
    c = CASES[name]
    H, W = c.geom[:2]
    base = baseline_outputs(name)
    kept = dropped = 0
    for o, b in zip(outs, base):
        kept += sum(1 for n, rows in _clusters(o["label_image"], H, W).values() if n < 30 and rows >= 17)
        lab_b = np.asarray(b["label_image"]).reshape(H, W)
        lab_o = np.asarray(o["label_image"]).reshape(H, W)
        for v, (n, rows) in _clusters(b["label_image"], H, W).items():
            if n < 30 and (lab_o[lab_b == v] == 999999).all():
                dropped += 1
    return kept > 0 and dropped > 0, f"{kept} small clusters kept over >= 17 rows, {dropped} dropped by the line test"


def _longest_ring(o):
    return int((np.asarray(o["end_ring_index"]) - np.asarray(o["start_ring_index"])).max())


def _full_ring(name, outs):
    ring = [_longest_ring(o) for o in outs]
    return all(r >= 2038 for r in ring) and all(o["n_less_sharp"] > 0 for o in outs), \
        f"longest ring {ring} (+ 10 = segmented points), n_less_sharp {_counts(outs, 'n_less_sharp')}"


def _full_ring_64(name, outs):
    ring = [_longest_ring(o) for o in outs]
    return all(r >= 1990 for r in ring) and all(o["n_segmented"] > 120000 for o in outs), \
        f"longest ring {ring}, n_segmented {_counts(outs, 'n_segmented')}"


def _dbfr_small(name, outs):
    return all(o["n_sharp"] < o["n_less_sharp"] / 2 for o in outs), \
        f"n_sharp {_counts(outs, 'n_sharp')} of n_less_sharp {_counts(outs, 'n_less_sharp')}"


def _dbfr_large(name, outs):
    small = oracle_outputs("dbfr_small")
    return all(o["n_sharp"] > s["n_sharp"] and o["n_less_sharp"] > 1024 for o, s in zip(outs, small)), \
        f"n_sharp {_counts(outs, 'n_sharp')} of n_less_sharp {_counts(outs, 'n_less_sharp')}"


def _dbscan_labels(largest, min_m):
    """M > min_m less-sharp points, the largest cluster label largest(M) (M: every point its own
    cluster; 0: no point has a neighbour, itself included), and no sharp point survives."""
    def p(name, outs):
        m = _counts(outs, "n_less_sharp")
        top = [int(np.max(o["dbscan_cluster"], initial=0)) for o in outs]
        return all(x > min_m for x in m) and top == [largest(x) for x in m] and not any(_counts(outs, "n_sharp")), \
            f"n_less_sharp {m}, largest cluster label {top}, n_sharp {_counts(outs, 'n_sharp')}"
    return p


def _fewer_than_default(key):
    def p(name, outs):
        base = baseline_outputs(name)
        return all(o[key] < b[key] for o, b in zip(outs, base)), \
            f"{key} {_counts(outs, key)} against {_counts(base, key)} at the defaults"
    return p


def _surf(all_flat):
    def p(name, outs):
        base = baseline_outputs(name)
        # the less-flat cloud takes every point that is no edge, flat or not: its count stays
        if all_flat:   # every curvature is below 1.0: sub-regions that had no flat pick now have one
            ok = all(o["n_flat"] > b["n_flat"] and o["n_less_flat"] == b["n_less_flat"] for o, b in zip(outs, base))
        else:          # no curvature is below 0: no flat pick
            ok = all(o["n_flat"] == 0 and b["n_flat"] > 0 and o["n_less_flat"] == b["n_less_flat"]
                     for o, b in zip(outs, base))
        return ok, (f"n_flat {_counts(outs, 'n_flat')} n_less_flat {_counts(outs, 'n_less_flat')} against "
                    f"{_counts(base, 'n_flat')} / {_counts(base, 'n_less_flat')} at the defaults")
    return p


def _ground_differs(name, outs):
    """use_kitti changes the ground angle (60 / 25 deg for rows below / from 16 against 12.5 deg)."""
    base = baseline_outputs(name)
    H, W = CASES[name].geom[:2]
    rows = set()
    for o, b in zip(outs, base):
        d = (np.asarray(o["ground_image"]) != np.asarray(b["ground_image"])).reshape(H, W)
        rows |= set(np.nonzero(d.any(axis=1))[0].tolist())
    low, high = [r for r in rows if r < 16], [r for r in rows if r >= 16]
    ok = bool(low) and (bool(high) if H > 16 else True)
    return ok, f"ground image differs from use_kitti 0 in {len(low)} rows below 16 and {len(high)} rows from 16"


def _gsi_zero(name, outs):
    base = baseline_outputs(name)
    return all(o["n_outlier"] > b["n_outlier"] for o, b in zip(outs, base)), \
        f"n_outlier {_counts(outs, 'n_outlier')} against {_counts(base, 'n_outlier')} at ground_scan_index 7"


def _odo_sizes(min_q, min_nc):
    def p(name, outs):
        q = [o["features"]["n_sharp"] for o in outs[1:]]
        nc = [len(o["corner_last"]) for o in outs[:-1]]
        return all(x > min_q for x in q) and all(x > min_nc for x in nc) and all(o["lm"] is not None for o in outs[1:]), \
            f"sharp queries {q} (> {min_q}), corner-last {nc} (> {min_nc})"
    return p


def _odo_fewer_corr(name, outs):
    base = baseline_outputs(name)
    a = [o["lm"]["n_corner_corr"] for o in outs[1:]]
    b = [o["lm"]["n_corner_corr"] for o in base[1:]]
    return all(x < y for x, y in zip(a, b)) and all(x > 0 for x in a), \
        f"corner correspondences {a} against {b} at 5 m and scan_period 0.1"


def _odo_runs(name, outs):
    return all(o["lm"] is not None for o in outs[1:]), f"frames {[o['frames'] for o in outs]}"


_HALL = dict(hall=8.0, dropout=0.0)
_EDGE0 = dict(edge_threshold=0.0)
_H32 = dict(ground_scan_index=12, use_vlp32c=0)

CASES = {
    # geometry, shipped thresholds unless stated
    "fused_max": Case((16, 2000, -15.0, 15.0), expect=count_all("n_segmented", lambda s: s > 15000, "> 15000")),
    "h16_unfused": Case((16, 2048, -15.0, 15.0), expect=count_all("n_segmented", lambda s: s > 15000, "> 15000")),
    "h17": Case(H17_GEOM, dict(ground_scan_index=8), expect=count_all("n_segmented", lambda s: s > 15000, "> 15000")),
    "h32_plain": Case(H32_GEOM, _H32, expect=count_all("n_segmented", lambda s: s > 15000, "> 15000")),
    # (64 x 288: a column is 1.25 deg wide, so the street scene's facades and poles break into
    # strips one column wide: no pole has to be added for clusters of < 30 points over >= 17 rows)
    "bands_16bit": Case((64, 288, -24.8, 2.0), dict(segment_valid_line_num=17), kitti=True, expect=_bands_16bit),
    "bands_tail": Case(HDL64E_GEOM, dict(segment_valid_line_num=17), seeds=(5, 6), kitti=True,
                       expect=count_all("n_segmented", lambda s: s > 40000, "> 40000")),
    "h8": Case((8, 900, -15.0, 13.0), dict(ground_scan_index=3), expect=count_all("n_segmented", lambda s: s > 1000, "> 1000")),
    "smallest": Case((2, 16, -15.0, -5.0), dict(ground_scan_index=0), expect=_smallest),
    "odd_w": Case((16, 1799, -15.0, 15.0), expect=count_all("n_segmented", lambda s: s > 10000, "> 10000")),
    "full_ring": Case((16, 2048, -3.0, 12.0), dict(ground_scan_index=0, edge_threshold=0.0), scan_kw=_HALL,
                      expect=_full_ring),
    "full_ring_64": Case((64, 2048, -2.0, 12.0), dict(ground_scan_index=0), seeds=(1,), scan_kw=_HALL,
                         expect=_full_ring_64),
    # thresholds, on 16 x 1800 with the VLP-16 elevations unless stated
    "dbscan_global": Case(VLP16_GEOM, _EDGE0, expect=_less_sharp_between(1024, 2048)),
    "dbscan_onfly": Case(HDL64E_GEOM, _EDGE0, seeds=(5,), kitti=True,
                         expect=count_all("n_less_sharp", lambda m: m > 2048, "> 2048")),
    "dbscan_global_h32": Case(H32_GEOM, dict(_H32, **_EDGE0), expect=_less_sharp_between(1024, 2048)),
    "dbfr_small": Case(VLP16_GEOM, dict(_EDGE0, DBFr=0.5), expect=_dbfr_small),
    "dbfr_large": Case(VLP16_GEOM, dict(_EDGE0, DBFr=50.0, RatioXY=1.0, RatioZ=1.0), expect=_dbfr_large),
    "segment_loose": Case(VLP16_GEOM, dict(segment_theta=30.0, segment_valid_point_num=2, segment_valid_line_num=1),
                          expect=count_all("n_outlier", lambda n: n < 50, "< 50")),
    "segment_strict": Case(VLP16_GEOM, dict(segment_theta=75.0, segment_valid_point_num=40, segment_valid_line_num=8),
                           expect=_fewer_than_default("n_segmented")),
    "gsi_above_h": Case(VLP16_GEOM, dict(ground_scan_index=20), expect=count_all("n_outlier", lambda n: n == 0, "0")),
    "gsi_zero": Case(VLP16_GEOM, dict(ground_scan_index=0), expect=_gsi_zero),
    "surf_all": Case(VLP16_GEOM, dict(surf_threshold=1.0), expect=_surf(True)),
    "surf_none": Case(VLP16_GEOM, dict(surf_threshold=0.0), expect=_surf(False)),
    "kitti_on_16": Case(VLP16_GEOM, dict(use_kitti=1), expect=_ground_differs),
    "kitti_on_32": Case(H32_GEOM, dict(_H32, use_kitti=1), expect=_ground_differs),
    # values at and beyond zero, which llsr_create accepts (include/llsr.h): the DBSCAN's degenerate ends
    "dbfr_zero": Case(VLP16_GEOM, dict(_EDGE0, DBFr=0.0), expect=_dbscan_labels(lambda m: m, 1024)),
    "dbfr_negative": Case(VLP16_GEOM, dict(_EDGE0, DBFr=-1.0), expect=_dbscan_labels(lambda m: 0, 1024)),
    "ratio_zero": Case(VLP16_GEOM, dict(RatioXY=0.0, RatioZ=0.0), expect=_dbscan_labels(lambda m: 0, 0)),
    "segment_any": Case(VLP16_GEOM, dict(segment_valid_point_num=-3, segment_valid_line_num=-1),
                        expect=count_all("n_outlier", lambda n: n == 0, "0")),
    # odometry: sizes of the scan-to-scan problem
    "odo_many_edges": Case(VLP16_GEOM, _EDGE0, seeds=(1, 2, 3), odometry=True, expect=_odo_sizes(1024, 1536)),
    "odo_rows_hbm": Case(HDL64E_GEOM, _EDGE0, seeds=(5, 6), kitti=True, odometry=True, expect=_odo_sizes(2560, 2048)),
    "odo_search_1m": Case(VLP16_GEOM, dict(nearest_feature_search_distance=1.0, scan_period=0.05), seeds=(1, 2, 3),
                          odometry=True, expect=_odo_fewer_corr),
    "odo_h17": Case(H17_GEOM, dict(ground_scan_index=8), seeds=(1, 2, 3), odometry=True, expect=_odo_runs),
}
