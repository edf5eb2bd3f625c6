"""k_select_ring's PCL-order sort keys (vox_pcl_keys) on the device.

* llsr_debug_vox_keys runs the production key builder on one ring's worth of caller-given points.
  For every constructed case of tests/_vox_keys.py (the dx and dy dz bounds and one past them, row
  bitmaps that end on and one past a word, a row per candidate, one row, one voxel, a voxel
  revisited, (i2, i1) against i1 order, coordinates on voxel edges and -0.0f) at 1 .. 2048
  candidates, the keys must be order-isomorphic to the numpy voxel ids and the path taken must be
  the one numpy predicts from the grid. The same points forced onto the sorted-runs path must give
  keys that the production sort (llsr_debug_exact_sort32) puts in the same order.
* End to end: a street scan, the 1.5 m cylinder of tests/test_gpu_vox_ends.py and a scan whose upper
  rings span more than 1024 voxels in x, as one batch, against the oracle in PCL order; the slots'
  C_VOXRUNS against the ring count numpy predicts from the oracle's output; two fresh handles.
"""
import ctypes as C

import numpy as np
import pytest

import _vox_keys as vk
import oracle_py
from _compare import compare
from llsr import Pipeline, default_config, lib, synth
from test_gpu_vox_ends import _cylinder_scan

gpu = pytest.mark.gpu


def _device_keys(points, force_runs):
    f = lib().llsr_debug_vox_keys
    f.restype, f.argtypes = C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    pts = np.ascontiguousarray(points, np.float32)
    keys = np.zeros(len(pts), np.uint32)
    path = C.c_int32(-9)
    assert f(pts.ctypes.data, len(pts), 1 if force_runs else 0, keys.ctypes.data, C.byref(path)) == 0
    return keys, path.value


def _device_order(keys):
    """the candidates in the order the production top and leaf kernels sort the keys' upper bits"""
    f = lib().llsr_debug_exact_sort32
    f.restype, f.argtypes = C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p]
    ranks = np.ascontiguousarray(keys >> 11, np.uint32)
    out = np.zeros(len(ranks), np.int32)
    assert f(ranks.ctypes.data, len(ranks), out.ctypes.data) == 0
    return out


@gpu
@pytest.mark.parametrize("L", vk.SIZES)
def test_device_keys(require_gpu, L):
    bad = []
    for name, pts, want in vk.cases(L):
        ids = vk.voxel_ids(pts)
        predicted = vk.predicted_path(pts)
        if want is not None:
            assert predicted == want, (name, L)
        keys, path = _device_keys(pts, False)
        runs, rpath = _device_keys(pts, True)
        if path != predicted:
            bad.append(f"{name}: path {path}, numpy predicts {predicted}")
        if rpath != vk.RUNS:
            bad.append(f"{name}: forced path {rpath}")
        for what, k in (("keys", keys), ("forced-runs keys", runs)):
            why = vk.isomorphic(k, ids)
            if why:
                bad.append(f"{name}: {what}: {why}")
        if not np.array_equal(_device_order(keys), _device_order(runs)):
            bad.append(f"{name}: the two paths' keys sort to different candidate orders")
    assert not bad, f"L = {L}:\n  " + "\n  ".join(bad)


@pytest.fixture(scope="module")
def batch():
    cfg = default_config("vlp16")
    scans = [synth.make_scan(3, "vlp16"), _cylinder_scan(), vk.wide_scan()]
    want = [oracle_py.Oracle(cfg, pcl_voxel_order=True).process(p) for p in scans]
    return cfg, scans, want


def _run(cfg, scans):
    import torch
    pipe = Pipeline(cfg, max_batch=len(scans), max_points=40000)
    off = np.zeros(len(scans) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in scans])
    d_pts = torch.from_numpy(np.concatenate(scans, axis=0)).cuda()
    d_off = torch.from_numpy(off).cuda()
    pipe.process_batch(d_pts.data_ptr(), d_off.data_ptr(), len(scans))
    got = [pipe.fetch(b) for b in range(len(scans))]
    got = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g.items()} for g in got]
    f = lib().llsr_debug_vox_runs
    f.restype, f.argtypes = C.c_int32, [C.c_void_p, C.c_void_p]
    runs = np.full(len(scans), -1, np.int32)
    assert f(pipe._h, runs.ctypes.data) == 0
    pipe.close()
    return got, runs


@gpu
def test_batch_against_oracle(require_gpu, batch):
    cfg, scans, want = batch
    predicted = [vk.predicted_run_rings(o, 16) for o in want]
    wide = [vk.predicted_path(p) for p in vk.ring_candidates(want[2], 16) if p is not None and len(p)]
    assert vk.RUNS in wide and vk.BITMAP in wide, wide
    got, runs = _run(cfg, scans)
    for b, (g, o) in enumerate(zip(got, want)):
        errs = compare(g, o)
        assert not errs, f"slot {b}:\n  " + "\n  ".join(errs)
    assert runs.tolist() == predicted


@gpu
def test_two_fresh_handles_agree(require_gpu, batch):
    cfg, scans, _ = batch
    (ga, ra), (gb, rb) = _run(cfg, scans), _run(cfg, scans)
    assert ra.tolist() == rb.tolist()
    for b, (x, y) in enumerate(zip(ga, gb)):
        assert x["n_less_flat"] == y["n_less_flat"], b
        assert np.array_equal(x["less_flat_xyzi"].view(np.uint32), y["less_flat_xyzi"].view(np.uint32)), b
