"""CPU side of the configuration cases (tests/_config_cases.py): every case's scans are valid input
for the oracle alone, and the oracle's output proves that the case reaches the code path it is
there for (a count over a kernel's threshold, a cluster only the line test keeps, a full ring ...).
Without this a GPU case could pass while silently missing its path."""
import numpy as np
import pytest

import _config_cases as cc
import test_gpu_config_parity as gpu_side


def test_gpu_file_runs_every_case():
    assert set(gpu_side.FEATURE_CASES) | set(gpu_side.ODOMETRY_CASES) == set(cc.CASES)
    assert not set(gpu_side.FEATURE_CASES) & set(gpu_side.ODOMETRY_CASES)
    assert set(gpu_side.FEATURE_CASES) == {n for n, c in cc.CASES.items() if not c.odometry}
    assert set(gpu_side.BATCH_CASES) == {"dbscan_global", "h16_unfused"}
    assert set(gpu_side.BATCH_CASES) <= set(gpu_side.FEATURE_CASES)


def test_scan_generator_layout():
    """scan(): H * W points, azimuth-major, every finite beam at its bin centre of the range image."""
    H, W, bottom, top = 17, 1800, -16.0, 16.0
    pts = cc.scan(3, H, W, bottom, top)
    assert pts.shape == (H * W, 4) and pts.dtype == np.float32
    k = np.nonzero(np.isfinite(pts[:, 0]))[0]
    x, y, z = (pts[k, a].astype(np.float64) for a in range(3))
    res = (top - bottom) / (H - 1)
    row = (np.rad2deg(np.arcsin(z / np.sqrt(x * x + y * y + z * z))) - bottom + 0.1) / res
    assert np.array_equal(np.floor(row).astype(int), k % H)
    assert np.abs(row - k % H - 0.1 / res).max() < 1e-3
    col = (-np.round((np.arctan2(x, y) - np.pi / 2) / (2 * np.pi / W)) + W / 2) % W
    assert np.array_equal(col.astype(int), (W - k // H) % W)  # clockwise from the rear, as synth.make_scan
    assert 0.01 < 1.0 - len(k) / (H * W) < 0.5  # dropout and misses


def test_config_sets_geometry_and_overrides():
    cfg = cc.config("kitti_on_32")
    assert (cfg.num_vertical_scans, cfg.num_horizontal_scans) == (32, 1024)
    assert (cfg.vertical_angle_bottom, cfg.vertical_angle_top, cfg.ground_scan_index) == (-25.0, 15.0, 12)
    assert cfg.use_kitti == 1 and cfg.use_vlp32c == 0 and cfg.DBFr == 5.0  # the VLP-16 block's DBFr
    assert cc.config("bands_16bit").DBFr == 7.5 and cc.config("bands_16bit").segment_valid_line_num == 17


@pytest.mark.parametrize("name", list(cc.CASES))
def test_case_reaches_its_path(name):
    case = cc.CASES[name]
    outs = cc.oracle_outputs(name)
    assert len(outs) == len(case.seeds)
    ok, what = case.expect(name, outs)
    print(f"{name}: {what}")
    assert ok, f"{name}: the oracle gives {what}"
