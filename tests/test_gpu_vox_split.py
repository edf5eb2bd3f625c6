"""The PCL-order VoxelGrid's exact sort as three launches (k_vox_top, k_vox_leaf, k_vox_sum).

* llsr_debug_exact_sort32 runs the production kernels (top + leaf) on one array: the orders must be
  libstdc++'s std::sort's at every size where the code changes path (one range / a window of 64 /
  wave partitions / block-wide partitions above 512) and on key patterns from all-equal to the
  median-of-3 killer, which spends the depth limit in a range above 512: that range cannot be a
  leaf item and is finished inside k_vox_top (a CPU replay of the recursion shows which cases do).
* The leaf items of a batch are appended with atomics, so their order differs from run to run; the
  results must not. A batch of five different scans (one with an empty ring) on two fresh handles,
  then a smaller batch on the first handle (the list's counter is reset, stale items are not run),
  against the oracle in PCL order.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py
from llsr import Pipeline, default_config, lib, synth

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 2, 16, 17, 64, 65, 128, 129, 511, 512, 513, 1024, 1800, 2047, 2048)
BIG = 512  # llsr_isort.h kBsBig: ranges above it are partitioned by the whole workgroup


def _killer(n, ties):
    """tests/native/introsort_check.cpp's median-of-3 killer."""
    k = n // 2
    a = np.empty(n, np.int64)
    for i in range(k):
        a[i] = i + 1 if i % 2 == 0 else k + i + 1
        a[k + i] = 2 * (i + 1)
    return (a // 3 if ties else a).astype(np.uint32)


def _sweep(rng, n):
    """A quantised sinusoid in runs of 1-6 equal ranks, as a ring's voxel ranks along its sweep."""
    runs = rng.integers(1, 7, n)
    q = np.round(150.0 * (1.0 + np.sin(np.linspace(0.0, 4.0 * np.pi, n)))).astype(np.int64)
    return np.repeat(q, runs)[:n].astype(np.uint32)


def _cases():
    rng = np.random.default_rng(2024)
    cases = []
    for n in SIZES:
        cases += [("equal", np.full(n, 7, np.uint32)), ("two", rng.integers(0, 2, n).astype(np.uint32)),
                  ("ascending", np.arange(n, dtype=np.uint32)), ("descending", np.arange(n, dtype=np.uint32)[::-1].copy()),
                  ("sweep", _sweep(rng, n))]
    for n in (1000, 2048):
        cases += [("killer", _killer(n, False)), ("killer ties", _killer(n, True))]
    return cases


def _spent_above_big(ranks):
    """Replay libstdc++'s __introsort_loop on the ranks while a range is above BIG; the sizes of the
    ranges above BIG that reach depth limit 0 (the ones k_vox_top finishes itself)."""
    v = [int(x) for x in ranks]
    n = len(v)
    spent = []
    stack = [(0, n, 2 * (n.bit_length() - 1))] if n > BIG else []
    while stack:
        f, l, d = stack.pop()
        while l - f > BIG:
            if d == 0:
                spent.append(l - f)
                break
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
            stack.append((i, l, d))
            l = i
    return spent


def test_split_sort_matches_std_sort(require_gpu):
    f = lib().llsr_debug_exact_sort32
    f.restype, f.argtypes = C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p]
    bad, top_finished = [], []
    for name, v in _cases():
        out = np.zeros(len(v), np.int32)
        assert f(v.ctypes.data, len(v), out.ctypes.data) == 0
        if not np.array_equal(out, oracle_py.std_sort_by_value(v.astype(np.float32))):
            bad.append((name, len(v)))
        if _spent_above_big(v):
            top_finished.append((name, len(v)))
    print("finished inside k_vox_top:", top_finished)
    assert not bad, f"cases {bad} differ from std::sort"
    assert top_finished, "no case spends its depth limit in a range above 512"


@pytest.fixture(scope="module")
def batches():
    """Five VLP-16 scans of different seeds (scan 2 without its laser 5: an empty ring) and a second
    batch of two, with the oracle's per-slot results in PCL order (slot state carried over)."""
    cfg = default_config("vlp16")
    H = cfg.num_vertical_scans
    scans = [synth.make_scan(s, "vlp16", motion=True) for s in (41, 42, 43, 44, 45)]
    scans[2] = scans[2].copy()
    scans[2][5::H] = np.nan
    second = [scans[4], scans[2]]
    oracles = [oracle_py.Oracle(cfg, pcl_voxel_order=True) for _ in scans]
    keep = lambda r: (int(r["n_less_flat"]), r["less_flat_xyzi"].copy(), r["start_ring_index"].copy(),
                      r["end_ring_index"].copy())
    want5 = [keep(o.process(p)) for o, p in zip(oracles, scans)]
    want2 = [keep(o.process(p)) for o, p in zip(oracles, second)]
    return cfg, scans, second, want5, want2


def _run(pipe, scans):
    import torch
    off = np.zeros(len(scans) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in scans])
    d_pts = torch.from_numpy(np.concatenate(scans, axis=0)).cuda()
    d_off = torch.from_numpy(off).cuda()
    pipe.process_batch(d_pts.data_ptr(), d_off.data_ptr(), len(scans))
    got = []
    for b in range(len(scans)):
        r = pipe.fetch(b)
        got.append((int(r["n_less_flat"]), r["less_flat_xyzi"].copy()))
    return got


def _same(got, want, what):
    for b, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], f"{what} slot {b}: n_less_flat {g[0]} != {w[0]}"
        assert np.array_equal(g[1].view(np.uint32), w[1].view(np.uint32)), f"{what} slot {b}: less_flat_xyzi differs"


def test_batch_results_do_not_depend_on_item_order(require_gpu, batches):
    cfg, scans, second, want5, want2 = batches
    assert any(e - s <= 1 for s, e in zip(want5[2][2], want5[2][3])), "scan 2 should hold an empty ring"
    a = Pipeline(cfg, max_batch=5, max_points=40000)
    b = Pipeline(cfg, max_batch=5, max_points=40000)
    ga, gb = _run(a, scans), _run(b, scans)
    a.close()
    b.close()
    _same(ga, gb, "run 1 vs run 2,")
    _same(ga, want5, "device vs oracle,")


def test_smaller_batch_after_larger_on_one_handle(require_gpu, batches):
    """The list still holds the larger batch's items when the smaller batch runs."""
    cfg, scans, second, want5, want2 = batches
    pipe = Pipeline(cfg, max_batch=5, max_points=40000)
    g5, g2 = _run(pipe, scans), _run(pipe, second)
    pipe.close()
    _same(g5, want5, "first batch, device vs oracle,")
    _same(g2, want2, "second batch, device vs oracle,")
