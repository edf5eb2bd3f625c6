"""The two ends of the PCL-order VoxelGrid's sort: k_vox_top's partition steps above 512 elements
and k_vox_sum's centroids (one lane per voxel, its point loads in batches).

* Sort orders: llsr_debug_exact_sort32 (the production top and leaf kernels) against std::sort at
  sizes just above 512 and around multiples of 128 above it (a wave's partition step classifies
  128 elements per loop round), on the ring-like "sweep" ranks and on a closed sweep that starts at
  its extreme: first + 1, mid and last - 1 then give a near-extreme pivot, so the first steps peel
  a few elements off a range that stays above 512. A CPU replay of libstdc++'s recursion asserts
  that they do.
* Centroids on long runs: a scan on a vertical cylinder of radius 1.5 m puts 1800 points of a ring
  into 60-71 voxels (runs of tens of points, across several load batches and more than 256 sorted
  positions), in a batch with a street scan and an empty scan, against the oracle in PCL order;
  and the same batch on two fresh handles.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py
from _compare import compare
from llsr import Pipeline, default_config, lib, synth

gpu = pytest.mark.gpu  # the fixture checks (the replay, the ring counts) run on the CPU
SIZES = (513, 640, 641, 1025, 2047)
BIG = 512    # llsr_isort.h kBsBig: k_vox_top partitions the ranges above it
PEEL = 64    # a lopsided step: its smaller part has at most this many elements


def _sweep(rng, n):
    """tests/test_gpu_vox_split.py's pattern: a quantised sinusoid in runs of 1-6 equal ranks."""
    runs = rng.integers(1, 7, n)
    q = np.round(150.0 * (1.0 + np.sin(np.linspace(0.0, 4.0 * np.pi, n)))).astype(np.int64)
    return np.repeat(q, runs)[:n].astype(np.uint32)


def _closed_sweep(n):
    """One closed period of a cosine starting at its maximum, every rank distinct at the top: the
    median of (first + 1, mid, last - 1) is one of the largest ranks."""
    t = np.arange(n, dtype=np.float64)
    return np.round(4000.0 * (1.0 + np.cos(2.0 * np.pi * t / n))).astype(np.uint32)


def _steps_above_big(ranks):
    """Replay libstdc++'s __introsort_loop on the ranks while a range is above BIG: for every
    partition step, in the order the recursion runs them (left part first), the size of its
    smaller part."""
    v = [int(x) for x in ranks]
    n = len(v)
    small = []
    stack = [(0, n, 2 * (n.bit_length() - 1))] if n > BIG else []
    while stack:
        f, l, d = stack.pop()
        while l - f > BIG and d > 0:
            d -= 1
            a, b, c = f + 1, f + (l - f) // 2, l - 1  # __move_median_to_first
            if v[a] < v[b]:
                m = b if v[b] < v[c] else (c if v[a] < v[c] else a)
            else:
                m = a if v[a] < v[c] else (c if v[b] < v[c] else b)
            v[f], v[m] = v[m], v[f]
            p, i, j = v[f], f + 1, l  # __unguarded_partition
            while True:
                while v[i] < p:
                    i += 1
                j -= 1
                while p < v[j]:
                    j -= 1
                if not i < j:
                    break
                v[i], v[j] = v[j], v[i]
                i += 1
            small.append(min(i - f, l - i))
            stack.append((i, l, d))
            l = i
    return small


def _longest_lopsided(small):
    best = cur = 0
    for s in small:
        cur = cur + 1 if s <= PEEL else 0
        best = max(best, cur)
    return best


def test_lopsided_pattern_replay():
    """The fixture, without the device: from 640 elements on (at 513 one step ends the part above
    512) the closed sweep starts with at least three consecutive steps above 512 that peel off at
    most 64 elements."""
    for n in SIZES:
        if n < 640:
            continue
        small = _steps_above_big(_closed_sweep(n))
        assert _longest_lopsided(small) >= 3, (n, small)
        assert all(s <= PEEL for s in small[:3]), (n, small)


@gpu
def test_top_sort_matches_std_sort(require_gpu):
    f = lib().llsr_debug_exact_sort32
    f.restype, f.argtypes = C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p]
    rng = np.random.default_rng(77)
    bad = []
    for n in SIZES:
        closed = _closed_sweep(n)
        if n >= 640:
            assert _longest_lopsided(_steps_above_big(closed)) >= 3, n
        for name, v in (("sweep", _sweep(rng, n)), ("closed sweep", closed)):
            out = np.zeros(n, np.int32)
            assert f(v.ctypes.data, n, out.ctypes.data) == 0
            if not np.array_equal(out, oracle_py.std_sort_by_value(v.astype(np.float32))):
                bad.append((name, n))
    assert not bad, f"cases {bad} differ from std::sort"


RADIUS = 1.5


def _cylinder_scan():
    """16 rings x 1800 columns on a vertical cylinder of radius 1.5 m around the sensor, elevations
    -15 .. +15 degrees, 3 mm radial noise, column-major as synth.make_scan."""
    rng = np.random.default_rng(5)
    H, W = 16, 1800
    phi = (W / 2 - np.arange(W, dtype=np.float64)) * (2.0 * np.pi / W)
    e = np.deg2rad(np.linspace(-15.0, 15.0, H))
    rho = RADIUS + rng.normal(0.0, 0.003, size=(W, H))
    pts = np.empty((W, H, 4), np.float32)
    pts[:, :, 0] = (rho * np.cos(phi)[:, None]).astype(np.float32)
    pts[:, :, 1] = (rho * np.sin(phi)[:, None]).astype(np.float32)
    pts[:, :, 2] = (rho * np.tan(e)[None, :]).astype(np.float32)
    pts[:, :, 3] = rng.integers(0, 101, size=(W, H)).astype(np.float32)
    return pts.reshape(-1, 4)


@pytest.fixture(scope="module")
def batch():
    cfg = default_config("vlp16")
    scans = [_cylinder_scan(), synth.make_scan(46, "vlp16", motion=True), np.zeros((0, 4), np.float32)]
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
    pipe.close()
    return got


def _ring_counts(o):
    """Per ring of the cylinder scan, from the oracle's output alone: its segmented points (the ring
    index ranges leave five out at either end) and its less-flat points (a centroid of a ring's
    points lies at the ring's height, LOAM y; the rings are 5 cm apart)."""
    seg = o["end_ring_index"].astype(np.int64) - o["start_ring_index"].astype(np.int64) + 10
    zr = RADIUS * np.tan(np.deg2rad(np.linspace(-15.0, 15.0, 16)))
    y = o["less_flat_xyzi"][: int(o["n_less_flat"]), 1].astype(np.float64)
    ring = np.abs(y[:, None] - zr[None, :]).argmin(axis=1)
    assert np.abs(y - zr[ring]).max() < 0.015, "a less-flat centroid lies between two rings"
    return seg, np.bincount(ring, minlength=16)


def test_long_run_fixture(batch):
    """The condition on the fixture, not on the device: some ring yields at most 1/20 as many
    less-flat points as it has segmented points, so its voxels' runs are long."""
    seg, lflat = _ring_counts(batch[2][0])
    print("segmented per ring:", seg.tolist(), "less-flat per ring:", lflat.tolist())
    assert any(0 < 20 * v <= s for s, v in zip(seg, lflat)), (seg.tolist(), lflat.tolist())


@gpu
def test_centroids_on_long_runs(require_gpu, batch):
    cfg, scans, want = batch
    seg, lflat = _ring_counts(want[0])
    assert any(0 < 20 * v <= s for s, v in zip(seg, lflat)), (seg.tolist(), lflat.tolist())
    got = _run(cfg, scans)
    for b, (g, o) in enumerate(zip(got, want)):
        errs = compare(g, o)
        assert not errs, f"slot {b}:\n  " + "\n  ".join(errs)


@gpu
def test_two_fresh_handles_agree(require_gpu, batch):
    cfg, scans, _ = batch
    ga, gb = _run(cfg, scans), _run(cfg, scans)
    for b, (x, y) in enumerate(zip(ga, gb)):
        assert x["n_less_flat"] == y["n_less_flat"], b
        assert np.array_equal(x["less_flat_xyzi"].view(np.uint32), y["less_flat_xyzi"].view(np.uint32)), b
