"""The PCL-order VoxelGrid's sort keys in numpy, for tests/test_vox_keys_host.py and
tests/test_gpu_vox_keys.py: the grid of a ring's candidate points in the device's float32
arithmetic, the two key forms (dense rank of the voxel id; rank of the occupied row with i0 below
it), the path k_select_ring takes for a grid, and the constructed point sets at the places where
the key building can go wrong."""
import numpy as np

LEAF = np.float32(0.2)
INV = np.float32(1.0) / LEAF  # 5.0f
DX_MAX = 1024                 # i0 has 10 bits
ROW_BITS = 128 * 1024         # the row bitmap (llsr_fa.hip kVoxRowBits)
SIZES = (1, 2, 63, 64, 65, 257, 2047, 2048)
BITMAP, RUNS = 0, 1


def grid(points):
    """(minb, div, cells): PCL's min box and divisions of the points (float32 [L, >= 3]) and every
    point's (i0, i1, i2), as VoxelGrid::applyFilter computes them in float32."""
    p = np.ascontiguousarray(points, np.float32)[:, :3]
    f = np.floor(p * INV)  # float32
    minb = np.floor(p.min(axis=0) * INV).astype(np.int64)
    maxb = np.floor(p.max(axis=0) * INV).astype(np.int64)
    cells = (f - minb.astype(np.float32)).astype(np.int64)
    return minb, maxb - minb + 1, cells


def voxel_ids(points):
    _, div, c = grid(points)
    return c[:, 0] + c[:, 1] * div[0] + c[:, 2] * div[0] * div[1]


def predicted_path(points):
    _, div, _ = grid(points)
    return BITMAP if div[0] <= DX_MAX and div[1] * div[2] <= ROW_BITS else RUNS


def dense_rank_keys(points):
    """rank of the voxel id among the ring's ids << 11 | candidate"""
    ids = voxel_ids(points)
    rank = np.searchsorted(np.unique(ids), ids)
    return (rank.astype(np.int64) << 11) | np.arange(len(ids))


def row_rank_keys(points):
    """(rank of the row i1 + i2 dy among the occupied rows << 10 | i0) << 11 | candidate"""
    _, div, c = grid(points)
    assert div[0] <= DX_MAX
    row = c[:, 1] + c[:, 2] * div[1]
    rank = np.searchsorted(np.unique(row), row)
    assert rank.max() < 2048
    return (((rank.astype(np.int64) << 10) | c[:, 0]) << 11) | np.arange(len(row))


def isomorphic(keys, ids):
    """Why `keys` (order << 11 | candidate) are not order-isomorphic to the voxel ids, or None: the
    low 11 bits are the candidate index, the stable argsort of the upper bits is that of the ids, and
    the sorted upper bits are equal exactly where the sorted ids are."""
    keys = np.asarray(keys, np.int64)
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    if not np.array_equal(keys & 0x7FF, np.arange(n)):
        return "low 11 bits are not the candidate index"
    if keys.max() >> 32:
        return "a key exceeds 32 bits"
    hi = keys >> 11
    pk, pi = np.argsort(hi, kind="stable"), np.argsort(ids, kind="stable")
    if not np.array_equal(pk, pi):
        return f"orders differ at sorted position {int(np.nonzero(pk != pi)[0][0])}"
    if not np.array_equal(np.diff(hi[pk]) == 0, np.diff(ids[pi]) == 0):
        return "equality patterns differ"
    return None


def _centres(cells):
    """Points at the centres of integer voxel coordinates (i0, i1, i2): (i + 0.5) * 0.2 floors to i
    after the multiplication by 5 for every |i| < 2^20."""
    c = np.asarray(cells, np.float64)
    p = np.zeros((len(c), 4), np.float32)
    p[:, :3] = ((c + 0.5) * 0.2).astype(np.float32)
    p[:, 3] = np.arange(len(c)) % 101
    return p


def _span(cells, dx, dy, dz):
    """cells with the first at the origin corner and the last at (dx-1, dy-1, dz-1) when there are
    two or more, so the grid's divisions are exactly (dx, dy, dz)."""
    c = np.array(cells, np.int64).reshape(-1, 3)
    c[0] = (0, 0, 0)
    if len(c) > 1:
        c[-1] = (dx - 1, dy - 1, dz - 1)
    return c


def _random_cells(rng, n, dx, dy, dz):
    return np.stack([rng.integers(0, dx, n), rng.integers(0, dy, n), rng.integers(0, dz, n)], axis=1)


def _two_word_rows(rng, n, nrows, dy):
    """rows only in the first and the last 64-bit word of a bitmap of nrows rows"""
    last0 = (nrows - 1) // 64 * 64
    pool = np.concatenate([np.arange(0, min(64, nrows)), np.arange(last0, nrows)])
    row = rng.choice(np.unique(pool), n)
    return row % dy, row // dy


def cases(L):
    """[(name, points [L, 4], wanted path or None)] for L candidates. The wanted path is what the
    case is built to take (checked on the CPU against predicted_path, which is what the device's
    path is compared with); None where the case does not aim at a bound. One point always has a
    1 x 1 x 1 grid, so with L = 1 every case takes the bitmap."""
    rng = np.random.default_rng(1000 + L)
    out = []

    def add(name, cells, want, dims=None):
        c = _span(cells, *dims) if dims else np.asarray(cells, np.int64).reshape(-1, 3)
        out.append((name, _centres(c), want if L > 1 else BITMAP))

    # dx boundary: i0 = 1023 present on the bitmap path; dx = 1025 takes the runs
    add("dx 1024", _random_cells(rng, L, 1024, 7, 5), BITMAP, (1024, 7, 5))
    add("dx 1025", _random_cells(rng, L, 1025, 7, 5), RUNS, (1025, 7, 5))
    # dy dz at the bitmap size and one above it
    add("rows 256x512", _random_cells(rng, L, 9, 256, 512), BITMAP, (9, 256, 512))
    add("rows 1x131072", _random_cells(rng, L, 9, 1, 131072), BITMAP, (9, 1, 131072))
    add("rows 3x43691", _random_cells(rng, L, 9, 3, 43691), RUNS, (9, 3, 43691))
    add("rows 1x131073", _random_cells(rng, L, 9, 1, 131073), RUNS, (9, 1, 131073))
    # word boundaries: occupied rows only in the first and the last word
    for nrows, dy in ((64, 8), (65, 5), (4096, 64), (4097, 241)):
        i1, i2 = _two_word_rows(rng, L, nrows, dy)
        c = np.stack([rng.integers(0, 3, L), i1, i2], axis=1)
        add(f"bitmap of {nrows} rows", c, BITMAP, (3, dy, nrows // dy))
    # every candidate in a row of its own, in a shuffled order: row ranks up to L - 1
    row = rng.permutation(64 * 64)[:L]
    add("a row each", np.stack([rng.integers(0, 4, L), row % 64, row // 64], axis=1), None)
    # one row, shuffled i0 (distinct up to 1024 candidates)
    add("one row", np.stack([rng.permutation(max(L, 1024))[:L] % 1024, np.full(L, 3), np.full(L, 2)], axis=1), None)
    # one voxel
    add("one voxel", np.tile([[5, 4, 3]], (L, 1)), None)
    # a voxel revisited after another one: A A B A ...
    c = np.tile([[2, 1, 1]], (L, 1))
    c[1::3] = (0, 2, 0)
    add("split run", c, None)
    # (i2, i1) order against i1 order: high i2 with low i1 and the reverse
    i2 = rng.integers(0, 40, L)
    add("lexicographic", np.stack([rng.integers(0, 30, L), 39 - i2, i2], axis=1), None)
    # coordinates at exactly k * 0.2f and at -0.0f: floorf(p * 5) - minb on its edge values
    k = rng.integers(-40, 41, (L, 3)).astype(np.float32)
    p = np.zeros((L, 4), np.float32)
    p[:, :3] = k * LEAF
    p[::5, 0] = np.float32(-0.0)
    p[1::7, 1] = np.float32(-0.0)
    out.append(("edge values", p, None))
    return out


def ring_candidates(o, H):
    """Per ring of a scan's oracle (or device) output, the less-flat candidates' LOAM points: the
    positions k in [start, end - 1] of the ring with label <= 0 (featureAssociation.cpp:1262-1266);
    None for a ring the selection skips."""
    rings = []
    for i in range(H):
        sp, ep = int(o["start_ring_index"][i]), int(o["end_ring_index"][i]) - 1
        if sp >= ep:
            rings.append(None)
            continue
        k = np.arange(sp, ep + 1)
        rings.append(o["loam_xyzi"][k[o["label"][k] <= 0]])
    return rings


def wide_scan(r_inner=20.0, r_outer=104.0):
    """16 rings x 1800 columns on two vertical cylinders around the sensor, 3 mm radial noise,
    column-major as synth.make_scan: the lower eight rings at r_inner, the upper eight at r_outer,
    whose rings span more than 1024 voxels (204.8 m) in LOAM x."""
    rng = np.random.default_rng(9)
    H, W = 16, 1800
    phi = (W / 2 - np.arange(W, dtype=np.float64)) * (2.0 * np.pi / W)
    e = np.deg2rad(np.linspace(-15.0, 15.0, H))
    rho = np.where(np.arange(H) < 8, r_inner, r_outer)[None, :] + rng.normal(0.0, 0.003, size=(W, H))
    pts = np.empty((W, H, 4), np.float32)
    pts[:, :, 0] = (rho * np.cos(phi)[:, None]).astype(np.float32)
    pts[:, :, 1] = (rho * np.sin(phi)[:, None]).astype(np.float32)
    pts[:, :, 2] = (rho * np.tan(e)[None, :]).astype(np.float32)
    pts[:, :, 3] = rng.integers(0, 101, size=(W, H)).astype(np.float32)
    return pts.reshape(-1, 4)


def predicted_run_rings(o, H):
    """The number of rings of a scan whose keys come from the sorted runs, from its oracle output."""
    n = 0
    for pts in ring_candidates(o, H):
        if pts is not None and len(pts) and predicted_path(pts) == RUNS:
            n += 1
    return n
