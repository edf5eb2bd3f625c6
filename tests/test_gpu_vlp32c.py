"""GPU tests of the VLP-32c support: rows by observed-elevation rank (use_vlp32c, IP:349-427) and
the ground angle D = 25 deg (IP:567-568).

The oracle refuses use_vlp32c. What pins which parity:
* the projection layer (range image, cell -> point map, vertical_raw2) on the VLP-32C's own rings:
  the numpy statement tests/_vlp32c.py, itself certified against the oracle where the branch and
  the plain one coincide (tests/test_vlp32c_host.py);
* everything behind the projection: the oracle with use_vlp32c = 0, on "vlp32c_uniform" scans,
  where the rank of a ring's bin is the plain branch's row;
* the ground rule: the statement's column pass, through the three invariants that tie it to the
  final ground image, on a scan where the rules provably differ; and a whole-pipeline run on a
  scan where the statement certifies that rules 25 and 60/25 agree in every cell, so that the
  oracle with use_kitti = 1 states the expected of the shipped block.
"""
import ctypes as C

import numpy as np
import pytest

import _vlp32c as V
import oracle_py
from _compare import compare
from llsr import Pipeline, _abi, default_config, lib, map_config

pytestmark = pytest.mark.gpu

H, W = 32, 1800


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- 1. H = 32 through the plain branch: every downstream kernel at 32 x 1800 ---------------------
@pytest.mark.parametrize("kitti", [0, 1])
def test_plain_branch_h32_matches_oracle(require_gpu, kitti):
    cfg = V.config(use_vlp32c=0, use_kitti=kitti)
    pts = V.scan("vlp32c_uniform")
    pipe = Pipeline(cfg, max_points=len(pts))
    g = pipe.process_scan(pts)
    pipe.close()
    assert compare(g, oracle_py.Oracle(cfg).process(pts)) == []


# ---- 2. the projection layer on the shipped block, non-uniform rings ------------------------------
def _dir(el_deg, az_deg, r):
    el, az = np.deg2rad(el_deg), np.deg2rad(az_deg)
    return [r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), 7.0]


def _projection_cases():
    base = V.scan("vlp32c")                              # 2 % dropout
    ring = np.arange(len(base)) % 32
    cut = base.copy()
    cut[np.isin(ring, (0, 9, 29))] = np.nan              # the rings at -25, 0.333 and 15 deg
    # ~50 points at four elevations between the rings' bins: 36 observed bins, the top ranks overflow
    extra = np.array([_dir(el, 7.3 * k + 1.0, 6.0 + 0.37 * k) for k in range(13) for el in (-20.0, -13.0, -10.0, 12.0)],
                     np.float32)
    rng = np.random.default_rng(5)
    over = np.insert(base, np.sort(rng.integers(0, len(base), len(extra))), extra, axis=0)
    # NaN / inf points, a point at the origin, and points nearer than 0.1 m in two otherwise empty bins
    odd = np.array([[np.nan, 1.0, 1.0, 1.0], [1.0, np.inf, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0],
                    _dir(-21.5, 40.0, 0.05), _dir(-21.5, 200.0, 0.09), _dir(12.0, 100.0, 0.02)], np.float32)
    deg = np.insert(base, [5, 777, 20000, 30001, 30001, len(base)], odd, axis=0)
    return {"dropout": (base, 32), "rings_removed": (cut, 29), "overflow": (over, 36), "degenerate": (deg, 34)}


@pytest.fixture(scope="module")
def shipped_pipe(require_gpu):
    pipe = Pipeline(V.config(), max_points=H * W + 64)
    yield pipe
    pipe.close()


@pytest.mark.parametrize("case", ["dropout", "rings_removed", "overflow", "degenerate"])
def test_projection_matches_statement(shipped_pipe, case):
    pts, n_bins = _projection_cases()[case]
    cfg = V.config()
    p = V.project(cfg, pts)
    assert p["vertical_raw2"].size == n_bins             # the case is what it claims to be
    if case == "overflow":
        assert (p["row"] >= H).sum() > 1000 and not p["placed"][p["row"] >= H].any()
    g = shipped_pipe.process_scan(pts)
    bins = shipped_pipe.row_bins(0)
    assert np.array_equal(bins, p["vertical_raw2"])
    assert np.array_equal(g["cell_point"], p["cell_point"])
    assert np.array_equal(_bits(g["range_image"]), _bits(p["range_image"]))
    assert g["n_points"] == int(np.isfinite(pts[:, :3]).all(axis=1).sum())


# ---- 3. whole pipeline, both flags: the ranked rows wired through to the end of FA ----------------
def test_pipeline_both_flags_matches_oracle(require_gpu):
    pts = V.scan("vlp32c_uniform")
    pipe = Pipeline(V.config(use_kitti=1), max_points=len(pts))
    g = pipe.process_scan(pts)
    assert pipe.row_bins(0).size == 32
    pipe.close()
    o = oracle_py.Oracle(V.config(use_vlp32c=0, use_kitti=1)).process(pts)
    assert compare(g, o) == []


# ---- 4. D = 25 deg on every row ------------------------------------------------------------------
def test_ground_rule_25_on_every_row(require_gpu):
    cfg = V.config()                                      # use_kitti 0, use_vlp32c 1
    pts = V.scan("vlp32c", ground_ramp=(6.0, 0.84))       # a 40 deg slope beyond 6 m
    p = V.project(cfg, pts)
    rules = {r: V.column_pass(cfg, p["full_cloud"], r) for r in (12.5, 25, "60/25")}
    assert (rules[25][:16] != rules["60/25"][:16]).sum() > 100   # decisive against use_kitti's rule
    assert (rules[25] != rules[12.5]).sum() > 100                # ... and against the plain one
    # decisive through the invariants too: a device on another rule would break one of them, in
    # cells that rule 25 rejects and 60/25 accepts beyond 5 m, or accepts beyond 5 m and 12.5 rejects
    fc = p["full_cloud"].reshape(H, W, 4)
    far = np.sqrt(fc[..., 0] * fc[..., 0] + fc[..., 1] * fc[..., 1]) > np.float32(5)
    assert ((rules[25] == 0) & (rules["60/25"] == 1) & far)[:16].sum() > 100
    assert ((rules[25] == 1) & (rules[12.5] == 0) & far).sum() > 100
    pipe = Pipeline(cfg, max_points=len(pts))
    g = pipe.process_scan(pts)
    pipe.close()
    assert np.array_equal(g["cell_point"], p["cell_point"])
    assert V.check_invariants(rules[25], g["ground_image"], p["full_cloud"], cfg) == []


# ---- 5. whole pipeline, shipped block ------------------------------------------------------------
def test_pipeline_shipped_block_matches_oracle(require_gpu):
    """Flat ground inside vertical walls 62 m away: the lower 16 rows see only ground, every
    ground-to-wall step falls into rows where use_kitti's rule is 25 deg too. The statement certifies
    it cell by cell; the oracle with use_kitti = 1 and plain rows (uniform rings: rank == row) is then
    the expected of use_kitti = 0, use_vlp32c = 1."""
    cfg = V.config()
    pts = V.scan("vlp32c_uniform", hall=62.0)
    p = V.project(cfg, pts)
    assert p["vertical_raw2"].size == 32 and (p["cell_point"] >= 0).sum() > 50000
    g25, g60 = V.column_pass(cfg, p["full_cloud"], 25), V.column_pass(cfg, p["full_cloud"], "60/25")
    assert np.array_equal(g25, g60)
    assert (g25 == 0).sum() > 1000 and (g25 == 1).sum() > 10000
    pipe = Pipeline(cfg, max_points=len(pts))
    g = pipe.process_scan(pts)
    pipe.close()
    o = oracle_py.Oracle(V.config(use_vlp32c=0, use_kitti=1)).process(pts)
    assert np.array_equal(o["cell_point"], p["cell_point"])
    assert compare(g, o) == []


# ---- 6. chain, defaults, error codes -------------------------------------------------------------
def test_odometry_chain_both_flags_matches_oracle(require_gpu):
    import torch
    from llsr import synth
    cfg = V.config(use_kitti=1, mode=_abi.LLSR_MODE_LM_APPLIED)
    ocfg = V.config(use_kitti=1, use_vlp32c=0, mode=_abi.LLSR_MODE_LM_APPLIED)
    pipe = Pipeline(cfg, max_batch=1, max_points=H * W)
    ora = oracle_py.OracleOdometry(ocfg)
    errs, its = [], []
    for k in range(3):
        scan = synth.make_scan(3 + k, "vlp32c_uniform", motion=True)
        d_pts = torch.from_numpy(scan).cuda()
        d_off = torch.tensor([0, len(scan)], dtype=torch.int64).cuda()
        torch.cuda.synchronize()
        pipe.odometry_batch(d_pts.data_ptr(), d_off.data_ptr(), 1)
        g = pipe.odometry_fetch(0, clouds=True)
        o = ora.process(scan)
        if g["frames"] != o["frames"] or (g["lm"]["skipped"] == 1) != (o["lm"] is None):
            errs.append(f"frame {k}: frames / skipped differ")
        elif o["lm"] is not None:
            its.append(o["lm"]["surf_iterations"] + o["lm"]["corner_iterations"])
            for key in ("surf_iterations", "corner_iterations", "n_surf_corr", "n_corner_corr", "degenerate"):
                if g["lm"][key] != o["lm"][key]:
                    errs.append(f"frame {k}: lm {key} {g['lm'][key]} vs {o['lm'][key]}")
        for key in ("transform_cur", "transform_sum"):
            if not np.array_equal(_bits(g[key]), _bits(o[key])):
                errs.append(f"frame {k}: {key} {g[key]} vs {o[key]}")
        for key in ("corner_last", "surf_last"):
            ref = o[key] if o[key] is not None else np.zeros((0, 4), np.float32)
            if g[key].shape != ref.shape or not np.array_equal(_bits(g[key]), _bits(ref)):
                errs.append(f"frame {k}: {key} differs ({g[key].shape} vs {ref.shape})")
    pipe.close()
    assert len(its) == 2 and min(its) >= 50   # the LM ran on both later frames
    assert errs == []


def test_vlp32c_defaults_and_row_bins_errors(require_gpu):
    c = default_config("vlp32c")
    want = dict(num_vertical_scans=32, num_horizontal_scans=1800, vertical_angle_bottom=-25.0, vertical_angle_top=15.0,
                sensor_mount_angle=0.0, ground_scan_index=7, use_kitti=0, use_vlp32c=1, segment_theta=60.0,
                segment_valid_point_num=5, segment_valid_line_num=3, scan_period=0.1, edge_threshold=0.005,
                surf_threshold=0.005, nearest_feature_search_distance=5.0, DBFr=5.0, RatioXY=0.5, RatioZ=2.5,
                mapping_frequency_divider=1, iterCountThres=50, step_size=1.0, stop_thres=0.05,
                mode=_abi.LLSR_MODE_FAITHFUL)
    assert {k for k, _ in _abi.Config._fields_} == set(want)
    py = _abi.config_for("vlp32c")
    for k, v in want.items():
        assert getattr(c, k) == np.float32(v) == getattr(py, k), k
    m = map_config("vlp32c")
    assert (m.enable_loop_closure, m.surrounding_keyframe_search_num, m.surrounding_radius) == (1, 50, 50.0)
    plain = Pipeline(default_config("vlp16"), max_points=1000)
    plain.process_scan(np.zeros((0, 4), np.float32))
    n, buf = C.c_int32(-1), np.zeros(8, np.int32)
    assert lib().llsr_row_bins(plain._h, 0, C.byref(n), buf.ctypes.data, 8) == _abi.LLSR_EINVAL
    plain.close()
    # a configuration whose bin bound exceeds the bitmap is refused
    h = C.c_void_p()
    wide = V.config(vertical_angle_bottom=-89.0)
    assert lib().llsr_create(C.byref(wide), 0, 1, 1000, C.byref(h)) == _abi.LLSR_EINVAL
    # the new kernel is in the kernel-time table of a use_vlp32c handle only
    names = [lib().llsr_kernel_name(k).decode() for k in range(14)]
    assert names[13] == "k_row_bins" and names[1] == "k_project"
