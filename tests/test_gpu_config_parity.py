"""GPU parity across the configurations llsr_create accepts (tests/_config_cases.py): geometries,
thresholds and point counts that move the kernels onto the code paths the three shipped blocks
never take, each against the CPU oracle on the same scans.

Bar: bit-exact, as tests/test_gpu_parity.py (tests/_compare.py) and tests/test_gpu_odometry.py.
Consecutive scans run through one handle so the FeatureAssociation carry-over state is used.
tests/test_config_oracle.py asserts on the oracle alone that every case reaches its path.
"""
import ctypes as C

import numpy as np
import pytest

import _config_cases as cc
from _compare import compare
from llsr import Pipeline, lib

pytestmark = pytest.mark.gpu

FEATURE_CASES = [
    "fused_max", "h16_unfused", "h17", "h32_plain", "bands_16bit", "bands_tail", "h8", "smallest", "odd_w",
    "full_ring", "full_ring_64",
    "dbscan_global", "dbscan_onfly", "dbscan_global_h32", "dbfr_small", "dbfr_large", "segment_loose",
    "segment_strict", "gsi_above_h", "gsi_zero", "surf_all", "surf_none", "kitti_on_16", "kitti_on_32",
    "dbfr_zero", "dbfr_negative", "ratio_zero", "segment_any",
]
BATCH_CASES = ["dbscan_global", "h16_unfused"]
# name -> the k_s2s_lm instantiation (llsr_debug_s2s_variant) the last frame must have run
ODOMETRY_CASES = {"odo_many_edges": 2048, "odo_rows_hbm": 2048, "odo_search_1m": 1024, "odo_h17": 1024}


def _pipeline(name, **kw):
    cfg = cc.config(name)
    return cfg, Pipeline(cfg, max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans, **kw)


@pytest.mark.parametrize("name", FEATURE_CASES)
def test_feature_stage_bit_exact(require_gpu, name):
    scans, want = cc.scans(name), cc.oracle_outputs(name)
    ok, what = cc.CASES[name].expect(name, want)
    assert ok, f"{name} misses its path: {what}"
    _, pipe = _pipeline(name)
    failures = []
    for k, (pts, o) in enumerate(zip(scans, want)):
        errs = compare(pipe.process_scan(pts), o)
        if errs:
            failures.append(f"scan {k} (seed {cc.CASES[name].seeds[k]}):\n  " + "\n  ".join(errs))
    pipe.close()
    assert not failures, f"{name} ({what}):\n" + "\n".join(failures)


@pytest.mark.parametrize("name", BATCH_CASES)
def test_batch_of_two_bit_exact(require_gpu, name):
    """Two distinct scans per batch (process_batch), two batches with the slots' scans swapped: the
    per-slot scratch (the global-scratch DBSCAN's ccl_a / ccl_b / shuf / edge_tmp / flat_tmp) and the
    per-slot carry-over state must not reach into the other slot."""
    import torch
    import oracle_py
    cfg, pipe = _pipeline(name, max_batch=2)
    a, b = cc.scans(name)
    oracles = [oracle_py.Oracle(cfg), oracle_py.Oracle(cfg)]
    failures = []
    for rep, batch in enumerate(((a, b), (b, a))):
        off = np.array([0, len(batch[0]), len(batch[0]) + len(batch[1])], np.int64)
        d_pts = torch.from_numpy(np.concatenate(batch)).cuda()
        d_off = torch.from_numpy(off).cuda()
        torch.cuda.synchronize()
        pipe.process_batch(d_pts.data_ptr(), d_off.data_ptr(), 2)
        for slot in range(2):
            errs = compare(pipe.fetch(slot), oracles[slot].process(batch[slot]))
            if errs:
                failures.append(f"batch {rep} slot {slot}:\n  " + "\n  ".join(errs))
    pipe.close()
    assert not failures, f"{name}:\n" + "\n".join(failures)


@pytest.mark.parametrize("name", list(ODOMETRY_CASES))
def test_odometry_bit_exact(require_gpu, name):
    """As tests/test_gpu_odometry.py's _sequence (frames, skip flag, LM counts, transformCur,
    transformSum, the four clouds), one sequence, without its iteration-count assertion: these
    drives are here for the sizes of their scan-to-scan problems."""
    import torch
    scans, want = cc.scans(name), cc.oracle_outputs(name)
    ok, what = cc.CASES[name].expect(name, want)
    assert ok, f"{name} misses its path: {what}"
    _, pipe = _pipeline(name)
    variant_of = lib().llsr_debug_s2s_variant
    variant_of.restype, variant_of.argtypes = C.c_int32, [C.c_void_p]
    errs = []
    for k, (pts, o) in enumerate(zip(scans, want)):
        d_pts = torch.from_numpy(np.array(pts)).cuda()  # a writable copy of the cached scan
        d_off = torch.tensor([0, len(pts)], dtype=torch.int64).cuda()
        torch.cuda.synchronize()
        pipe.odometry_batch(d_pts.data_ptr(), d_off.data_ptr(), 1)
        g = pipe.odometry_fetch(0, clouds=True)
        tag = f"frame {k}"
        if g["frames"] != o["frames"]:
            errs.append(f"{tag}: frames {g['frames']} vs {o['frames']}")
        if (g["lm"]["skipped"] == 1) != (o["lm"] is None):
            errs.append(f"{tag}: skipped {g['lm']['skipped']} vs oracle lm {o['lm'] is not None}")
        elif o["lm"] is not None:
            for key in ("surf_iterations", "corner_iterations", "n_surf_corr", "n_corner_corr", "degenerate"):
                if g["lm"][key] != o["lm"][key]:
                    errs.append(f"{tag}: lm {key} {g['lm'][key]} vs {o['lm'][key]}")
        for key in ("transform_cur", "transform_sum"):
            if not np.array_equal(g[key], o[key]):
                errs.append(f"{tag}: {key} {g[key]} vs {o[key]} (max |d| {np.abs(g[key] - o[key]).max():.3g})")
        for key in ("corner_last", "surf_last", "corner_scan", "surf_scan"):
            ref = o[key] if o[key] is not None else np.zeros((0, 4), np.float32)
            if g[key].shape != ref.shape:
                errs.append(f"{tag}: {key} shape {g[key].shape} vs {ref.shape}")
            elif not np.array_equal(g[key], ref):
                errs.append(f"{tag}: {key} max |d| {np.abs(g[key] - ref).max():.3g}")
    variant = variant_of(pipe._h)
    pipe.close()
    assert variant == ODOMETRY_CASES[name], f"{name}: k_s2s_lm<{variant}> ran, {what}"
    assert not errs, f"{name} ({what}):\n" + "\n".join(errs)
