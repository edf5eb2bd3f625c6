"""GPU: the lazily built and regrown state of the C-ABI host layer (csrc/llsr_capi*.hip) gives the
results of a fresh handle.

- Both single-problem calls (llsr_scan2scan, llsr_scan2map) on one handle: a small problem (tens of
  points per cloud), a larger one (hundreds: the buffer pool and the staging buffer both regrow),
  the small one again. Every report field but `ms` and the pose / transform are bit-identical to the
  same problem on a fresh handle, and equal the oracle as tests/test_gpu_fa_lm.py and
  tests/test_gpu_mo.py compare.
- llsr_mapping_init twice on one handle, then a 3-frame VLP-16 drive at max_batch = 2: every
  fetched field and key pose is bit-identical to a handle initialised once.
- llsr_odometry_reset before the odometry state exists, then 2 frames at B = 1: bit-identical to a
  handle that skipped the reset.

Allocation failures are not provoked here: tests/test_host_pools.py covers those paths on the CPU.
"""
import os

import numpy as np
import pytest

import oracle_py
from llsr import Pipeline, _abi, default_config, synth
from test_gpu_fa_lm import _pairs, _same

pytestmark = pytest.mark.gpu

MO_FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mo_map_vlp16.npz")
MO_KEYS = ("pose", "matX0", "min_lambda", "cf_mean", "iterations", "converged", "degenerate", "n_corner_corr",
           "n_surf_corr")


def _bits_differ(a, b, path=""):
    """Paths at which two fetched results (nested dicts of scalars / arrays) differ bitwise; `ms` is skipped."""
    if isinstance(a, dict):
        if a.keys() != b.keys():
            return [f"{path}: keys {sorted(a)} vs {sorted(b)}"]
        return [e for k in a if k != "ms" for e in _bits_differ(a[k], b[k], f"{path}/{k}")]
    a, b = np.asarray(a), np.asarray(b)
    same = a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return [] if same else [f"{path}: {a} vs {b}"]


def _every(a, n):
    """About n points of a cloud, evenly spaced, in order."""
    return a[::max(1, len(a) // n)][:n]


def _regrow_equals_fresh(cfg, problems, solve, oracle, same_as_oracle):
    """problems: small, large; run small, large, small on one handle and each on a fresh one."""
    order = [problems[0], problems[1], problems[0]]
    assert max(len(c) for c in problems[0][:4]) <= 120
    assert all(len(big) > len(small) for small, big in zip(problems[0][:4], problems[1][:4]))  # every capacity grows
    reused = Pipeline(cfg)
    got = [solve(reused, pr) for pr in order]
    reused.close()
    errs = []
    for k, pr in enumerate(order):
        fresh = Pipeline(cfg)
        errs += [f"call {k} vs fresh handle{e}" for e in _bits_differ(got[k], solve(fresh, pr))]
        fresh.close()
        errs += [f"call {k} vs oracle: {e}" for e in same_as_oracle(got[k], oracle(pr))]
    assert not errs, "\n".join(errs)


def test_scan2scan_regrow_equals_fresh(require_gpu):
    cfg, pairs = _pairs("vlp16", [1, 2])
    sharp, flat, cl, sl = pairs[0]
    t0 = np.zeros(6, np.float32)
    small = (_every(sharp, 20), _every(flat, 40), _every(cl, 60), _every(sl, 90), t0)
    large = (_every(sharp, 150), _every(flat, 300), _every(cl, 400), _every(sl, 600), t0)
    _regrow_equals_fresh(cfg, [small, large], lambda p, pr: p.scan2scan(*pr, 0),
                         lambda pr: oracle_py.scan2scan(cfg, *pr, 0), _same)


def test_scan2map_regrow_equals_fresh(require_gpu):
    fix = np.load(MO_FIX)
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    cq, sq, cm, sm, pose = (fix[k] for k in ("q0_corner", "q0_surf", "corner_map", "surf_map", "q0_init"))

    def nearest(cloud, n):  # a dense patch of the map around the pose, in the cloud's order
        d = np.linalg.norm(cloud[:, :3] - pose[3:6], axis=1)
        return cloud[np.sort(np.argsort(d, kind="stable")[:n])]

    small = (_every(cq, 40), _every(sq, 80), nearest(cm, 40), nearest(sm, 120), pose)
    large = (_every(cq, 200), _every(sq, 400), nearest(cm, 300), nearest(sm, 600), pose)

    def same(g, o):
        return [f"{k} {g[k]} vs {o[k]}" for k in MO_KEYS if not np.array_equal(np.asarray(g[k]), np.asarray(o[k]))]

    _regrow_equals_fresh(cfg, [small, large], lambda p, pr: p.scan2map(*pr),
                         lambda pr: oracle_py.scan2map(cfg, *pr), same)


def _upload(scans):
    import torch
    off = np.zeros(len(scans) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in scans])
    d_pts = torch.from_numpy(np.concatenate(scans)).cuda()
    d_off = torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    return d_pts, d_off


def test_repeated_mapping_init_equals_fresh(require_gpu):
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    seeds, frames = (1, 65), 3
    runs = []
    for inits in (2, 1):
        pipe = Pipeline(cfg, max_batch=len(seeds), max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
        for _ in range(inits):
            pipe.mapping_init(_abi.LLSR_MODE_LM_APPLIED)
        out = []
        for k in range(frames):
            d_pts, d_off = _upload([synth.make_scan(s0 + k, "vlp16", motion=True) for s0 in seeds])
            pipe.mapping_batch(d_pts.data_ptr(), d_off.data_ptr(), len(seeds))
            out.append({f"slot{b}": pipe.mapping_fetch(b) for b in range(len(seeds))})
        out.append({f"keyposes{b}": pipe.mapping_keyposes(b) for b in range(len(seeds))})
        pipe.close()
        runs.append(out)
    assert runs[1][frames - 1]["slot0"]["mo_frames"] == 2  # MapOptimization ran on frames 2 and 3
    errs = [f"frame {k}{e}" for k, (a, b) in enumerate(zip(*runs)) for e in _bits_differ(a, b)]
    assert not errs, "\n".join(errs)


def test_odometry_reset_before_first_batch_equals_none(require_gpu):
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    runs = []
    for reset_first in (True, False):
        pipe = Pipeline(cfg, max_batch=1, max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
        if reset_first:
            pipe.odometry_reset()  # nothing allocated yet: the first batch still builds the state
        out = []
        for k in range(2):
            d_pts, d_off = _upload([synth.make_scan(3 + k, "vlp16", motion=True)])
            pipe.odometry_batch(d_pts.data_ptr(), d_off.data_ptr(), 1)
            out.append(pipe.odometry_fetch(0, clouds=True))
        pipe.close()
        runs.append(out)
    assert runs[1][1]["frames"] == 2 and runs[1][1]["n_corner_scan"] > 0
    errs = [f"frame {k}{e}" for k, (a, b) in enumerate(zip(*runs)) for e in _bits_differ(a, b)]
    assert not errs, "\n".join(errs)
