"""k_label<false>, the banded labelling of every image that does not fit LDS, on the scenes of
tests/_label_scenes.py: images built cell by cell with their shapes placed across the band
boundaries (band unions in LDS with local indices, band roots in the global parent array, down edges
across boundaries, sizes and 64-bit row sets rebuilt from the per-band stats words, seed ranks over
tiles of 4 x 1024 cells, label sweeps of 8 x 1024), against the CPU oracle, bit-exact, and the label
image against the serial numpy BFS as well. tests/test_label_scenes_host.py proves on the oracle
alone that every scene holds what it is there for; its check runs here again before the comparison.
"""
import numpy as np
import pytest

import _config_cases as cc
import _label_scenes as ls
from _compare import diff_report
from test_gpu_label_columns import ARRAYS, COUNTS
from test_label_scenes_host import check_scene


def _diff(g, o):
    errs = [f"{k}: gpu={g[k]} oracle={o[k]}" for k in COUNTS if g[k] != o[k]]
    errs += [r for r in (diff_report(k, g[k], o[k]) for k in ARRAYS) if r]
    return errs


def _cfg(gname, sname="one"):
    return cc.config(ls.case(gname, sname))


def _pipe(gname, sname="one", **kw):
    from llsr import Pipeline
    g = ls.GEOMS[gname]
    return Pipeline(_cfg(gname, sname), max_points=g.H * g.W, **kw)


def _run(gname, sname):
    pipe = _pipe(gname, sname)
    g = pipe.process_scan(ls.scan(gname, sname))
    pipe.close()
    return g


def _against_oracle(tag, g, gname, sname):
    errs = [f"{tag}: {e}" for e in _diff(g, ls.oracle(gname, sname))]
    r = diff_report("label_image against the numpy BFS", np.asarray(g["label_image"], np.int64),
                    ls.bfs(gname, sname).ravel())
    return errs + ([f"{tag}: {r}"] if r else [])


@pytest.mark.gpu
@pytest.mark.parametrize("gname,sname", ls.PAIRS)
def test_labels_bit_exact(require_gpu, gname, sname):
    check_scene(gname, sname)
    errs = _against_oracle(f"{gname} {sname}", _run(gname, sname), gname, sname)
    assert not errs, "\n".join(errs)


@pytest.mark.gpu
def test_two_handles_agree(require_gpu):
    for sname in ("u_and_n", "stairs"):
        a, b = _run("g64x2048", sname), _run("g64x2048", sname)
        errs = _diff(a, b)
        assert not errs, f"g64x2048 {sname}: two fresh handles differ:\n" + "\n".join(errs)


@pytest.mark.gpu
@pytest.mark.parametrize("gname", list(ls.GEOMS))
def test_scenes_in_turn_on_one_handle(require_gpu, gname):
    """`one` fills the global parent words and the 64-bit row words of every cell; the scenes after
    it on the same handle must come out as from a fresh one."""
    pipe = _pipe(gname)
    failures = []
    for sname in ("one", "singles", "cross", "u_and_n"):
        failures += _against_oracle(f"{gname} {sname} after the others", pipe.process_scan(ls.scan(gname, sname)),
                                    gname, sname)
    pipe.close()
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("gname", list(ls.GEOMS))
def test_smaller_batch_after_larger(require_gpu, gname):
    """Four scenes as one batch (a workgroup each, its own slot of the parent and row words), then
    one scene alone on the same handle."""
    import torch
    names = ("one", "stairs", "comb_down", "thirty")
    clouds = [ls.scan(gname, n) for n in names]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    d_pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    d_off = torch.from_numpy(off).cuda()
    pipe = _pipe(gname, max_batch=len(names))
    pipe.process_batch(d_pts.data_ptr(), d_off.data_ptr(), len(names))
    failures = []
    for b, n in enumerate(names):
        failures += _against_oracle(f"{gname} batch of 4, {n}", pipe.fetch(b), gname, n)
    failures += _against_oracle(f"{gname} wrap alone after the batch", pipe.process_scan(ls.scan(gname, "wrap")),
                                gname, "wrap")
    pipe.close()
    assert not failures, "\n".join(failures)
