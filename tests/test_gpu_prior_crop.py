"""GPU: the prior map's crop kernels (csrc/llsr_prior.hip: k_prior_count, k_prior_scan, k_prior_write;
DESIGN.md §20) against the host twin (LLSR_PRIOR_HOST) and the numpy statement (tests/_prior_map.py).

Bar: device == host twin == numpy, bit for bit, offsets included.
* the hand-built edge clouds (d2 == r2, tangent tile faces, tile boundaries at negative coordinates,
  a sphere off the map, one around it, non-finite positions, an empty kind);
* the recorded map at key poses 0, 380 and 722, radius 3 and 5 m, with P = 1, 3 and 65 positions in
  one call (65 segments per kind: more than one scan block, rows of very different lengths);
* a ~4.3 k-point cloud whose rows hold 0, 1, 63, 64, 65 points (one ballot), 255, 256, 257 (a wave's
  step of four loads) and 1023, 1024, 1025 (the block's four parts), all inside the sphere and cut by
  it;
* the count-only call and the LLSR_ERANGE-then-retry call."""
import numpy as np
import pytest

import _prior_map as pm
import _result_map
import llsr
from llsr import _abi

pytestmark = pytest.mark.gpu
KEYS = (0, 380, 722)


@pytest.fixture(scope="module")
def recorded():
    z = _result_map.load()
    c, s = (np.ascontiguousarray(z[k], np.float32) for k in ("corner_map", "surf_map"))
    return pm.stored_order(c, 1.0)[0], pm.stored_order(s, 1.0)[0], np.ascontiguousarray(z["key_poses"][:, :3], np.float32)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _three_way(corner, surf, radius, tile, positions, tag):
    """Device, host twin and numpy on one problem; returns the device result."""
    want = pm.crop_batch(pm.stored_order(corner, tile)[0], pm.stored_order(surf, tile)[0], positions, radius)
    res = []
    for device in (0, None):
        m = llsr.PriorMap(radius=radius, tile=tile, device=device)
        m.load(corner, surf)
        got = m.crop(positions)
        who = f"{tag}, {'device' if device == 0 else 'host twin'}"
        assert np.array_equal(got["corner_off"], want[1]), f"{who}: corner offsets {got['corner_off']} vs {want[1]}"
        assert np.array_equal(got["surf_off"], want[2]), f"{who}: surf offsets {got['surf_off']} vs {want[2]}"
        out = _np(got["out"])
        assert out.shape == want[0].shape and np.array_equal(out.view(np.uint32), want[0].view(np.uint32)), \
            f"{who}: points differ"
        res.append((m, got))
    res[1][0].close()
    return res[0]


@pytest.mark.parametrize("case", pm.edge_cases(), ids=lambda c: c[0])
def test_edge_clouds(require_gpu, case):
    name, corner, surf, radius, tile, positions = case
    m, _ = _three_way(corner, surf, radius, tile, positions, name)
    m.close()


@pytest.mark.parametrize("radius", [3.0, 5.0])
def test_recorded_map_p_1_3_65(require_gpu, recorded, radius):
    sc, ss, keys = recorded
    m = llsr.PriorMap(radius=radius, tile=1.0, device=0)
    m.load(sc, ss)  # (loading a stored cloud stores it unchanged: the sort is stable)
    assert np.array_equal(m.points("corner").view(np.uint32), sc.view(np.uint32))
    idx65 = sorted(set(range(0, 693, 11)) | set(KEYS))
    assert len(idx65) == 65, len(idx65)
    for idx in ([KEYS[0]], [KEYS[1]], [KEYS[2]], list(KEYS), idx65):
        pos = keys[idx]
        want = pm.crop_batch(sc, ss, pos, radius)
        got = m.crop(pos)
        assert np.array_equal(got["corner_off"], want[1]) and np.array_equal(got["surf_off"], want[2]), f"P {len(idx)}"
        assert np.array_equal(_np(got["out"]).view(np.uint32), want[0].view(np.uint32)), f"P {len(idx)}: points differ"
        st = m.last_crop()
        assert st["written"] == want[2][-1] and st["written"] <= st["tested"] < len(idx) * (len(sc) + len(ss))
    m.close()


@pytest.mark.parametrize("radius", [50.0, 3.0])
def test_row_lengths_around_ballot_step_and_part_sizes(require_gpu, radius):
    pts = pm.row_cloud()
    rows = np.bincount(pm.tile_coords(pts, 1.0)[:, 1], minlength=len(pm.ROW_COUNTS))
    assert tuple(rows) == pm.ROW_COUNTS and pts[:, 0].max() < 8 and 0 < pts[:, 2].min() and pts[:, 2].max() < 1
    pos = [(4, 7, 0.5), (1, 2.5, 0.5), (7.5, 10.2, 0.9)]
    m, got = _three_way(pts, pts[::3].copy(), radius, 1.0, pos, f"rows r {radius}")
    n = np.diff(got["corner_off"])
    if radius == 50.0:
        assert all(n == len(pts)), "the sphere was to contain every row"
    else:
        assert all((n > 0) & (n < len(pts))), "the sphere was to cut the rows"
    m.close()


def test_count_only_and_erange_then_retry(require_gpu):
    import torch
    pts = pm.row_cloud()
    surf = pts[::2].copy()
    m = llsr.PriorMap(radius=3.0, tile=1.0, device=0)
    m.load(pts, surf)
    pos = [(4, 6, 0.5), (2, 10, 0.5)]
    want = pm.crop_batch(pm.stored_order(pts, 1.0)[0], pm.stored_order(surf, 1.0)[0], pos, 3.0)
    total = int(want[2][-1])
    assert total > 10
    got = m.crop(pos, count_only=True)
    assert got["out"] is None
    assert np.array_equal(got["corner_off"], want[1]) and np.array_equal(got["surf_off"], want[2])
    with pytest.raises(llsr.LlsrError) as e:
        m.crop(pos, cap=total - 1)
    assert e.value.code == _abi.LLSR_ERANGE
    assert np.array_equal(e.value.offsets[0], want[1]) and np.array_equal(e.value.offsets[1], want[2])
    torch.cuda.synchronize()
    assert not bool(e.value.out.any()), "a refused crop wrote points"
    for cap in (total, total + 7):
        got = m.crop(pos, cap=cap)
        assert np.array_equal(got["corner_off"], want[1]) and np.array_equal(got["surf_off"], want[2])
        assert np.array_equal(_np(got["out"]).view(np.uint32), want[0].view(np.uint32))
    m.close()
