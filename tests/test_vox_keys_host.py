"""The two forms of the PCL-order VoxelGrid's sort keys, stated in numpy (tests/_vox_keys.py): the
dense rank of a candidate's voxel id, and the rank of its grid row (i1 + i2 dy) among the ring's
occupied rows with i0 below it. Both must order a ring's candidates as the voxel ids do: the same
stable argsort, the same equality pattern after sorting, the candidate index in the low 11 bits.

* On every ring of a few synthetic scans of both lidars (the oracle's segmented cloud and labels).
* On the constructed point sets tests/test_gpu_vox_keys.py sends through the device, where each
  must also lie on the side of the bounds (dx <= 1024, dy dz <= the bitmap's 128 Ki rows) it was
  built for: that is a condition on the fixture, checked here without a device.
"""
import numpy as np
import pytest

import _vox_keys as vk
import oracle_py
from llsr import default_config, synth


def _check(points, what):
    ids = vk.voxel_ids(points)
    why = vk.isomorphic(vk.dense_rank_keys(points), ids)
    assert why is None, f"{what}: dense rank: {why}"
    if vk.predicted_path(points) == vk.BITMAP:
        why = vk.isomorphic(vk.row_rank_keys(points), ids)
        assert why is None, f"{what}: row rank: {why}"


@pytest.mark.parametrize("lidar", ["vlp16", "hdl64e"])
def test_synthetic_rings(lidar):
    cfg = default_config(lidar, 2048 if lidar == "hdl64e" else None)
    H = cfg.num_vertical_scans
    rings = 0
    for seed in (1, 2):
        o = oracle_py.Oracle(cfg, pcl_voxel_order=True).process(synth.make_scan(seed, lidar))
        for i, pts in enumerate(vk.ring_candidates(o, H)):
            if pts is None or len(pts) == 0:
                continue
            assert len(pts) <= 2048
            assert vk.predicted_path(pts) == vk.BITMAP, (lidar, seed, i, vk.grid(pts)[1].tolist())
            _check(pts, f"{lidar} seed {seed} ring {i}")
            rings += 1
    assert rings >= H


@pytest.mark.parametrize("L", vk.SIZES)
def test_constructed_cases(L):
    names = set()
    for name, pts, want in vk.cases(L):
        assert pts.shape == (L, 4) and pts.dtype == np.float32
        if want is not None:
            assert vk.predicted_path(pts) == want, (name, L, vk.grid(pts)[1].tolist())
        _check(pts, f"{name}, L {L}")
        names.add(name)
    assert len(names) == 16


def test_case_grids_sit_on_their_bounds():
    """The boundary cases' grids are exactly what their names say (L >= 2 puts a point in both
    corners), i0 = 1023 is present at dx = 1024, and the word-boundary cases occupy the first and
    the last word of their bitmap and nothing between."""
    for L in (2, 65, 2048):
        byname = {n: p for n, p, _ in vk.cases(L)}
        for name, dims in (("dx 1024", (1024, 7, 5)), ("dx 1025", (1025, 7, 5)), ("rows 256x512", (9, 256, 512)),
                           ("rows 1x131072", (9, 1, 131072)), ("rows 3x43691", (9, 3, 43691)),
                           ("rows 1x131073", (9, 1, 131073))):
            assert vk.grid(byname[name])[1].tolist() == list(dims), (name, L)
        assert vk.grid(byname["dx 1024"])[2][:, 0].max() == 1023
        for nrows in (64, 65, 4096, 4097):
            _, div, c = vk.grid(byname[f"bitmap of {nrows} rows"])
            assert div[1] * div[2] == nrows
            words = np.unique((c[:, 1] + c[:, 2] * div[1]) // 64)
            assert set(words.tolist()) <= {0, (nrows - 1) // 64} and 0 in words and (nrows - 1) // 64 in words
    for L in (257, 2048):
        byname = {n: p for n, p, _ in vk.cases(L)}
        _, div, c = vk.grid(byname["a row each"])
        assert len(np.unique(c[:, 1] + c[:, 2] * div[1])) == L
        ids = vk.voxel_ids(byname["split run"])
        assert ids[0] == ids[2] != ids[1]
        _, div, c = vk.grid(byname["lexicographic"])
        assert np.corrcoef(c[:, 1], c[:, 2])[0, 1] < -0.9


def test_wide_scan_has_rings_on_both_sides():
    """The end-to-end scan of tests/test_gpu_vox_keys.py: from the oracle's output, at least one
    ring's candidates span more than 1024 voxels in x and at least one ring's do not."""
    cfg = default_config("vlp16")
    o = oracle_py.Oracle(cfg, pcl_voxel_order=True).process(vk.wide_scan())
    paths = [vk.predicted_path(p) for p in vk.ring_candidates(o, 16) if p is not None and len(p)]
    print("paths per ring:", paths)
    assert vk.RUNS in paths and vk.BITMAP in paths
    assert vk.predicted_run_rings(o, 16) == paths.count(vk.RUNS)
