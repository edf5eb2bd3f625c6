"""CPU: the prior map's host twin (llsr_prior with LLSR_PRIOR_HOST, include/llsr.h)
against the numpy statement in tests/_prior_map.py — the stored order and its CSR, the crop, the
refusals and the capacity protocol. Bar: bit for bit, offsets included.

The recorded map (tests/golden/result_0318.npz) gives real geometry: at radius 5 m and tile 1 m every
tested key pose has tiles fully inside, cut by and fully outside the sphere for both kinds (asserted
below), so the tile skipping cannot go unexercised."""
import numpy as np
import pytest

import _prior_map as pm
import _result_map
import llsr
from llsr import _abi

KEYS = (0, 380, 722)


@pytest.fixture(scope="module")
def recorded():
    z = _result_map.load()
    return (np.ascontiguousarray(z["corner_map"], np.float32), np.ascontiguousarray(z["surf_map"], np.float32),
            np.ascontiguousarray(z["key_poses"][:, :3], np.float32))


@pytest.fixture(scope="module")
def stored(recorded):
    """tile -> ((corner stored, start, dims, origin), (surf ...)): computed once, never changed"""
    return {t: tuple(pm.stored_order(c, t) for c in recorded[:2]) for t in (1.0, 2.0)}


def _same_crop(got, want, tag):
    out, oc, os_ = want
    assert np.array_equal(got["corner_off"], oc), f"{tag}: corner offsets {got['corner_off']} vs {oc}"
    assert np.array_equal(got["surf_off"], os_), f"{tag}: surf offsets {got['surf_off']} vs {os_}"
    if got["out"] is not None:
        g = got["out"]
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.shape == out.shape, f"{tag}: {g.shape} vs {out.shape}"
        assert np.array_equal(g.view(np.uint32), out.view(np.uint32)), f"{tag}: points differ"


@pytest.mark.parametrize("tile", [1.0, 2.0])
def test_stored_order_and_csr_on_the_recorded_map(recorded, stored, tile):
    m = llsr.PriorMap(radius=5.0, tile=tile, device=None)
    m.load(recorded[0], recorded[1])
    info = m.info()
    assert info["device"] == _abi.LLSR_PRIOR_HOST and info["tile"] == tile
    for kind, (pts, start, dims, origin) in zip(m.KINDS, stored[tile]):
        assert info[kind]["dims"] == dims and info[kind]["origin"] == origin
        assert info[kind]["n_points"] == len(pts) and info[kind]["n_tiles"] == int(np.prod(dims))
        assert info[kind]["n_tiles_used"] == int((np.diff(start.astype(np.int64)) > 0).sum())
        assert np.array_equal(m.tile_starts(kind), start)
        assert np.array_equal(m.points(kind).view(np.uint32), pts.view(np.uint32))
    m.close()


@pytest.mark.parametrize("radius", [3.0, 5.0])
@pytest.mark.parametrize("tile", [1.0, 2.0])
def test_crops_at_recorded_key_poses(recorded, stored, radius, tile):
    m = llsr.PriorMap(radius=radius, tile=tile, device=None)
    m.load(recorded[0], recorded[1])
    sc, ss = stored[tile][0][0], stored[tile][1][0]
    pos = recorded[2][list(KEYS)]
    want = pm.crop_batch(sc, ss, pos, radius)
    assert all(np.diff(want[1]) > 0) and all(np.diff(want[2]) > 0), "an empty crop at a recorded key pose"
    assert all(np.diff(want[1]) < len(sc)) and all(np.diff(want[2]) < len(ss)), "a crop does not cut the map"
    _same_crop(m.crop(pos), want, f"r {radius} tile {tile}")
    for k in range(len(pos)):  # one position per call gives the same crops
        _same_crop(m.crop(pos[k:k + 1]), pm.crop_batch(sc, ss, pos[k:k + 1], radius), f"key {KEYS[k]}")
    st = m.last_crop()
    assert st["written"] == int(pm.crop_batch(sc, ss, pos[2:3], radius)[2][-1])  # (the last call: one position)
    assert st["written"] <= st["tested"] < len(sc) + len(ss), "the tile skipping skipped nothing"
    m.close()


def test_recorded_map_has_tiles_inside_cut_and_outside(recorded):
    """The condition the crop tests rest on (radius 5 m, tile 1 m): tiles fully inside, cut and fully
    outside the sphere at every tested key pose, for both kinds."""
    for cloud in recorded[:2]:
        for k in KEYS:
            inside, cut, outside = pm.tile_classes(cloud, 1.0, recorded[2][k], 5.0)
            assert inside > 0 and cut > 0 and outside > 0, (k, inside, cut, outside)
    got = [pm.tile_classes(recorded[0], 1.0, recorded[2][k], 5.0) for k in KEYS]
    assert got == [(123, 107, 200), (97, 97, 236), (106, 74, 250)], got


@pytest.mark.parametrize("case", pm.edge_cases(), ids=lambda c: c[0])
def test_edge_clouds(case):
    name, corner, surf, radius, tile, positions = case
    m = llsr.PriorMap(radius=radius, tile=tile, device=None)
    m.load(corner, surf)
    sc, ss = pm.stored_order(corner, tile), pm.stored_order(surf, tile)
    for kind, s in zip(m.KINDS, (sc, ss)):
        assert np.array_equal(m.tile_starts(kind), s[1]) and m.info()[kind]["origin"] == s[3]
        assert np.array_equal(m.points(kind).view(np.uint32), s[0].view(np.uint32))
    want = pm.crop_batch(sc[0], ss[0], positions, radius)
    got = m.crop(positions)
    _same_crop(got, want, name)
    kept = set(got["out"][:got["corner_off"][1], 3].astype(int))  # input indices of position 0's corner crop
    if name == "exact":
        # d2 == r2 is out, the inward float32 neighbours in y and z are in; point 2 (x one ulp inside
        # 3) is out as well: its 9 - 1.4e-6 + 16 rounds back to 25 in float32, which is the predicate
        assert kept == {1, 4, 6, 8}, kept
    elif name == "tangent":
        assert kept == {1, 4, 7, 9, 11}, kept       # the points on the tangent faces are out
    elif name == "miss_all_nan":
        assert got["surf_off"][-1] == 0, "a sphere off the map or a non-finite position kept points"
    elif name == "contains":
        assert got["corner_off"][1] == len(corner) and got["surf_off"][-1] == 2 * (len(corner) + len(surf))
    m.close()


def test_refusals():
    pts = pm.row_cloud()
    for bad in (dict(tile=0.0), dict(tile=-1.0), dict(tile=float("nan")), dict(radius=0.0), dict(radius=float("inf"))):
        with pytest.raises(llsr.LlsrError) as e:
            llsr.PriorMap(device=None, **bad)
        assert e.value.code == _abi.LLSR_EINVAL
    m = llsr.PriorMap(radius=3.0, tile=1.0, device=None)
    m.load(pts, pts[:100])
    before = m.points("corner")
    for k, v in ((7, np.nan), (0, np.inf)):
        bad = pts.copy()
        bad[k, 1] = v
        for args in ((bad, pts), (pts, bad)):
            with pytest.raises(llsr.LlsrError) as e:
                m.load(*args)
            assert e.value.code == _abi.LLSR_EINVAL and "non-finite" in str(e.value)
    # more than 2^24 tiles: two points 1000 m apart on each axis at tile 1 are 1001^3 tiles
    far = np.array([[0, 0, 0, 0], [1000, 1000, 1000, 1]], np.float32)
    with pytest.raises(llsr.LlsrError) as e:
        m.load(far, pts)
    assert e.value.code == _abi.LLSR_ERANGE and "a tile of 4 fits" in str(e.value), str(e.value)
    assert np.array_equal(m.points("corner"), before), "a refused load changed the object"
    fit = llsr.PriorMap(radius=3.0, tile=4.0, device=None)
    fit.load(far, pts)  # the size the message names does fit
    assert fit.info()["corner"]["n_tiles"] == 251 ** 3
    fit.close()
    # an empty kind, both ways, and an empty map
    for c, s in ((pts, pts[:0]), (pts[:0], pts), (pts[:0], pts[:0])):
        m.load(c, s)
        want = pm.crop_batch(pm.stored_order(c, 1.0)[0], pm.stored_order(s, 1.0)[0], [(4, 6, 0.5), (0, 0, 0)], 3.0)
        _same_crop(m.crop([(4, 6, 0.5), (0, 0, 0)]), want, "empty kind")
    m.close()


def test_capacity_protocol():
    pts = pm.row_cloud()
    m = llsr.PriorMap(radius=3.0, tile=1.0, device=None)
    m.load(pts, pts[::2])
    pos = [(4, 6, 0.5), (2, 10, 0.5)]
    want = pm.crop_batch(pm.stored_order(pts, 1.0)[0], pm.stored_order(pts[::2], 1.0)[0], pos, 3.0)
    total = int(want[2][-1])
    assert total > 10
    _same_crop(m.crop(pos, count_only=True), want, "count only")
    with pytest.raises(llsr.LlsrError) as e:
        m.crop(pos, cap=total - 1)
    assert e.value.code == _abi.LLSR_ERANGE
    assert np.array_equal(e.value.offsets[0], want[1]) and np.array_equal(e.value.offsets[1], want[2])
    assert not e.value.out.any(), "a refused crop wrote points"
    _same_crop(m.crop(pos, cap=total), want, "retry")
    _same_crop(m.crop(pos, cap=total + 5), want, "larger")
    m.close()
