"""The prior map's specification in numpy, independent of csrc/llsr_prior.h, and the
mapping chain's localisation mode as a sequence restatement.

* stored_order(cloud, tile): tile coordinate i = (int)floorf(c / tile) - min over the cloud per axis
  (one float32 divide), key = (iz ny + iy) nx + ix, the cloud stably sorted by key, the CSR over keys.
* crop(stored, pos, r): the stored points with d2 = ((0 + dx^2) + dy^2) + dz^2 < float(double(r)^2) in
  float32, in stored order. No tiles here: the predicate alone defines the result.
* OraclePriorMapping: oracle_py.OracleMapping.process with the three changes of localisation mode, and
  set_pose.
"""
import ctypes as C

import numpy as np

import oracle_py
from llsr import _abi

F = np.float32


def tile_coords(cloud, tile):
    """floorf(c / tile) per axis as int64, [n][3]; the divide in float32."""
    c = np.ascontiguousarray(cloud, F).reshape(-1, 4)[:, :3]
    return np.floor(c / F(tile)).astype(np.int64)


def stored_order(cloud, tile):
    """-> (stored cloud, tile_start[ntiles + 1] uint32, dims (nx, ny, nz), origin (ox, oy, oz))."""
    a = np.ascontiguousarray(cloud, F).reshape(-1, 4)
    if len(a) == 0:
        return a.copy(), np.zeros(1, np.uint32), (0, 0, 0), (0, 0, 0)
    t = tile_coords(a, tile)
    o = t.min(0)
    n = t.max(0) - o + 1
    i = t - o
    key = (i[:, 2] * n[1] + i[:, 1]) * n[0] + i[:, 0]
    order = np.argsort(key, kind="stable")
    start = np.zeros(int(n.prod()) + 1, np.int64)
    np.cumsum(np.bincount(key, minlength=int(n.prod())), out=start[1:])
    return a[order].copy(), start.astype(np.uint32), tuple(int(v) for v in n), tuple(int(v) for v in o)


def r_squared(r) -> np.float32:
    return F(np.float64(F(r)) * np.float64(F(r)))


def in_sphere(pts, pos, r):
    """The float32 predicate, one bool per point."""
    p = np.ascontiguousarray(pts, F).reshape(-1, 4)
    q = np.asarray(pos, F)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]
        d = F(0) + dx * dx
        d = d + dy * dy
        d = d + dz * dz
        return d < r_squared(r)


def crop(stored, pos, r):
    s = np.ascontiguousarray(stored, F).reshape(-1, 4)
    return s[in_sphere(s, pos, r)].copy()


def crop_batch(stored_corner, stored_surf, positions, r):
    """llsr_prior_crop_batch's output: (out, corner_off, surf_off)."""
    pos = np.asarray(positions, F).reshape(-1, 3)
    parts = [crop(stored_corner, p, r) for p in pos] + [crop(stored_surf, p, r) for p in pos]
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in parts])
    out = np.concatenate(parts) if off[-1] else np.zeros((0, 4), F)
    P = len(pos)
    return out, off[:P + 1].copy(), off[P:].copy()


def tile_classes(cloud, tile, pos, r):
    """Used tiles of `cloud` fully inside / cut by / fully outside the sphere, by the nearest and the
    farthest point of each tile's box in float64 (a condition on the data, not a specification)."""
    t = np.unique(tile_coords(cloud, tile), axis=0).astype(np.float64)
    lo, hi = t * tile, (t + 1) * tile
    p = np.asarray(pos, np.float64)
    near = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    far = np.maximum(np.abs(lo - p), np.abs(hi - p))
    inside = (far ** 2).sum(1) < r * r
    outside = (near ** 2).sum(1) >= r * r
    return int(inside.sum()), int((~inside & ~outside).sum()), int(outside.sum())


class OraclePriorMapping(oracle_py.OracleMapping):
    """MapOptimization::run in localisation mode, one sequence: the local map is the crop of the prior
    map's stored clouds at currentRobotPosPoint (from the first MapOptimization frame on), a keyframe
    stores its pose only, and the first-keyframe distinction counts key poses."""

    def __init__(self, cfg, mo_mode, stored_corner, stored_surf, radius, **kw):
        super().__init__(cfg, mo_mode, **kw)
        self.stored = (np.ascontiguousarray(stored_corner, F), np.ascontiguousarray(stored_surf, F))
        self.radius = radius

    def set_pose(self, pose6):
        p = np.ascontiguousarray(pose6, F).reshape(6)
        self.aft, self.tobe, self.last = p.copy(), p.copy(), p.copy()
        self.robot = p[3:6].copy()

    def process(self, xyzi, odo=None):
        """odo: this frame's OracleOdometry.process output when the caller already has it (the odometry
        does not depend on the map, so sequences over the same scans share it)."""
        lib, f4 = oracle_py.lib, oracle_py._f4
        o = odo if odo is not None else self.odo.process(xyzi)
        out = {"odo": o, "step": False, "frames": o["frames"]}
        if o["lm"] is None:
            return out
        self.cycle += 1
        if self.cycle != self.divider:
            return out
        self.cycle = 0
        lc, ls, lo = self.leaf
        self.transform_sum = oracle_py.odometry_to_transform(o["transform_sum"])
        lib().oracle_associate_to_map(self.transform_sum.ctypes.data, self.bef.ctypes.data, self.aft.ctypes.data,
                                      self.tobe.ctypes.data, self.incre.ctypes.data)
        # change 1: the crop takes extractSurroundingKeyFrames' place, keyframes or not
        cmap = crop(self.stored[0], self.robot, self.radius)
        smap = crop(self.stored[1], self.robot, self.radius)
        outlier = np.ascontiguousarray(o["features"]["outlier_xyzi"][:, [1, 2, 0, 3]])
        sl_ds = self._vg(o["surf_last"], ls)
        cs_ds = self._vg(o["corner_scan"], lc)
        ol_ds = self._vg(outlier, lo)
        tot_ds = self._vg(np.concatenate([sl_ds, ol_ds]), ls)
        rep = _abi.LmReport()
        pose = self.tobe.copy()
        cq, sq, cm, sm = (f4(a) for a in (cs_ds, tot_ds, cmap, smap))
        rc = lib().oracle_scan2map_carry(C.byref(self.cfg_mo), cq.ctypes.data, len(cq), sq.ctypes.data, len(sq),
                                         cm.ctypes.data, len(cm), sm.ctypes.data, len(sm), pose.ctypes.data,
                                         C.byref(self.deg), self.matP.ctypes.data, C.byref(rep))
        if rc != 0:
            raise RuntimeError(f"oracle_scan2map_carry: {rc}")
        lm_ran = len(cm) > 10 and len(sm) > 100
        if lm_ran:
            self.tobe = pose.copy()
            self.bef = self.transform_sum.copy()
            self.aft = self.tobe.copy()
        self.robot = self.aft[3:6].copy()
        first = not self.keyposes  # change 3: counts key poses
        est = (self.tobe if first else self.aft).copy()
        self.last = est.copy()
        if not first:
            self.tobe = self.aft.copy()
        kp = np.array([est[3], est[4], est[5], est[0], est[1], est[2]], F)
        self.keyposes.append(kp)  # change 2: the pose only, no clouds
        self.mo_frames += 1
        mrep = {"n_corner_map": len(cm), "n_corner_ds": len(cm), "n_surf_map": len(sm), "n_surf_ds": len(sm),
                "n_in_radius": 0, "n_poses_ds": 0, "n_keyframes": 0, "n_transformed": 0}
        out.update(step=True, lm=rep.as_dict(), lm_ran=lm_ran, map=mrep, n_corner_q=len(cq), n_surf_q=len(sq),
                   n_corner_map=len(cm), n_surf_map=len(sm), transform_sum=self.transform_sum.copy(),
                   transform_tobe_mapped=self.tobe.copy(), transform_bef_mapped=self.bef.copy(),
                   transform_aft_mapped=self.aft.copy(), keyframes=len(self.keyposes))
        return out


# ---- hand-built clouds shared by the host, native and device tests ---------------------------------
def _cloud(xyz):
    a = np.zeros((len(xyz), 4), F)
    a[:, :3] = np.asarray(xyz, F).reshape(-1, 3)
    a[:, 3] = np.arange(len(a), dtype=F)  # intensity = input index: an order mistake shows
    return a


def edge_cases():
    """[(name, corner, surf, radius, tile, positions)]"""
    dn = lambda v, to: np.nextafter(F(v), F(to))  # noqa: E731
    cases = []
    # d2 == r2 exactly is outside; the float32 neighbour towards the centre is inside
    exact = _cloud([(3, 4, 0), (3, dn(4, 0), 0), (dn(3, 0), 4, 0), (-3, -4, 0), (-3, dn(-4, 0), 0), (0, 0, 5),
                    (0, 0, dn(5, 0)), (0, 0, dn(5, 9)), (0, 0, 0)])
    cases.append(("exact", exact, exact[::-1].copy(), 5.0, 1.0, [(0, 0, 0)]))
    # a sphere tangent to the tile faces x = 5 and x = -5 with points on those faces
    tangent = _cloud([(5, 0, 0), (dn(5, 0), 0, 0), (dn(5, 9), 0, 0), (-5, 0, 0), (dn(-5, 0), 0, 0), (dn(-5, -9), 0, 0),
                      (0, 5, 0), (0, dn(5, 0), 0), (0, -5, 0), (0, dn(-5, 0), 0), (0, 0, -5), (0, 0, dn(-5, 0))])
    cases.append(("tangent", tangent, np.zeros((0, 4), F), 5.0, 1.0, [(0, 0, 0)]))
    cases.append(("tangent_tile5", tangent, tangent, 5.0, 5.0, [(0, 0, 0), (0.5, 0, 0)]))
    # points on tile boundaries, either side of them, at negative coordinates and at -0.0
    g = []
    for v in (-3.0, -2.0, -1.0, -0.0, 0.0, 1.0, 2.0):
        g += [dn(v, -9), F(v), dn(v, 9)]
    xs, ys, zs = np.meshgrid(g, g, (-1.0, dn(0, -9), 0.0, 0.5), indexing="ij")
    rng = np.random.default_rng(11)
    bnd = _cloud(rng.permutation(np.stack([xs.ravel(), ys.ravel(), zs.ravel()], 1)))
    pos = [(0, 0, 0), (-1, -1, 0), (-2.5, 1.5, -0.5), (1.0, -3.0, 0.25), (0.3, 0.3, 0.3)]
    cases.append(("boundaries_r2", bnd, bnd[::3].copy(), 2.0, 1.0, pos))
    cases.append(("boundaries_r1_tile05", bnd, bnd[1::2].copy(), 1.0, 0.5, pos))
    # a sphere that misses the map, one that contains all of it, a non-finite position
    cases.append(("miss_all_nan", bnd, bnd[::2].copy(), 3.0, 1.0,
                  [(1000, 0, 0), (0, -1000, 0), (0, 0, 1e30), (np.nan, 0, 0), (0, np.inf, 0)]))
    cases.append(("contains", bnd, bnd[::2].copy(), 100.0, 1.0, [(0, 0, 0), (3, 3, 3)]))
    return cases


ROW_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 0, 1023, 1024, 1025, 2, 300)


def row_cloud(seed=3):
    """~4.3 k points, tile 1: row j (y in [j, j + 1), z in [0, 1)) holds ROW_COUNTS[j] points with x in
    [0, 8): below, at and above 64 (one ballot), 256 (a wave's step) and 1024 (a block's four parts of
    256), and empty rows between full ones."""
    rng = np.random.default_rng(seed)
    pts = []
    for j, n in enumerate(ROW_COUNTS):
        p = np.stack([rng.uniform(0, 8, n), j + rng.uniform(0.01, 0.99, n), rng.uniform(0.01, 0.99, n)], 1)
        pts.append(p)
    return _cloud(rng.permutation(np.concatenate(pts)))
