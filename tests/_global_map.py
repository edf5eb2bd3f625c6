"""The expected side of the global map: publishGlobalMap (mapOptmization.cpp:775-892) and
saveMapService's save_key_feature_pcd == false branch (MO:382-395), restated in program order over
the oracle's primitives only (oracle_py.voxel_grid with PCL's order, oracle_py.transform_keyframe)
and a float32 numpy d^2. It never calls the library and keeps its own call counter.

publishGlobalMap's quirks, as include/llsr.h lists them: the sorted radius search (ties by index),
the key-pose and cloud VoxelGrids whose output only counts from the second call on (the shared
pointers are re-pointed at MO:807 / 836), (int)intensity naming a keyframe twice, PCL's pass-through
when the voxel extents overflow INT32_MAX."""
import numpy as np

import oracle_py

INT32_MAX = 2 ** 31 - 1
EMPTY = np.zeros((0, 4), np.float32)


def sq_dist(poses4, pos):
    """((0 + dx^2) + dy^2) + dz^2 in float32, one rounding per operation."""
    p = np.ascontiguousarray(poses4, np.float32).reshape(-1, 4)
    q = np.asarray(pos, np.float32)
    d = np.zeros(len(p), np.float32)
    for a in range(3):
        df = q[a] - p[:, a]
        d = d + df * df
    return d


def radius_sorted(poses4, pos, radius):
    """Indices with d^2 < float(double(r) * double(r)), ascending d^2, equal d^2 by ascending index."""
    d = sq_dist(poses4, pos)
    r = np.float64(np.float32(radius))
    idx = np.flatnonzero(d < np.float32(r * r))
    return idx[np.argsort(d[idx], kind="stable")].astype(np.int32)


def extent_product(cloud, leaf):
    """PCL's (int64(float((max - min) * inv)) + 1) product over the three axes, as a Python int."""
    c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    inv = np.float32(1.0) / np.float32(leaf)
    prod = 1
    for a in range(3):
        prod *= int((c[:, a].max() - c[:, a].min()) * inv) + 1
    return prod


def _vg(cloud, leaf):
    return oracle_py.voxel_grid(cloud, leaf, stable=False) if len(cloud) else EMPTY


def _cat(parts):
    return np.concatenate(parts) if parts else EMPTY


class GlobalMapOracle:
    def __init__(self, search_radius=5000.0, keypose_leaf=1.0, cloud_leaf=0.4, high_dense=0, first_call_raw=1,
                 surf_leaf=0.4):
        self.search_radius, self.keypose_leaf, self.cloud_leaf = search_radius, keypose_leaf, cloud_leaf
        self.high_dense, self.first_call_raw, self.surf_leaf = high_dense, first_call_raw, surf_leaf
        self.poses, self.world = [], []  # key poses; the three transformed clouds per keyframe
        self.calls = 0

    def add_keyframe(self, pose6, corner, surf, outlier):
        pose = np.ascontiguousarray(pose6, np.float32)
        self.poses.append(pose)
        self.world.append(tuple(oracle_py.transform_keyframe(pose, np.ascontiguousarray(c, np.float32).reshape(-1, 4))
                                for c in (corner, surf, outlier)))

    def reset(self):
        self.poses, self.world, self.calls = [], [], 0

    def global_map(self, robot_pos):
        rep = dict(call=self.calls, n_in_radius=0, n_poses_used=0, downsampled_poses=0, downsampled_cloud=0,
                   passthrough=0, n_edge=0, n_planar=0, n_global_raw=0, n_global=0)
        out = {"global": EMPTY, "edge": EMPTY, "planar": EMPTY, "report": rep}
        if not self.poses:  # MO:780
            return out
        K = len(self.poses)
        poses4 = np.concatenate([np.array(self.poses, np.float32)[:, :3], np.arange(K, dtype=np.float32)[:, None]], 1)
        near = radius_sorted(poses4, robot_pos, self.search_radius)
        ds = (not self.high_dense) and (self.calls >= 1 or not self.first_call_raw)
        sel = np.ascontiguousarray(poses4[near])
        if ds:
            sel = _vg(sel, self.keypose_leaf)
        ids = [int(w) for w in sel[:, 3]]  # (int)intensity truncates
        edge = _cat([self.world[k][0] for k in ids])
        planar = _cat([self.world[k][1] for k in ids])
        raw = _cat([c for k in ids for c in self.world[k]])
        glob = raw
        if ds and len(raw):
            rep["passthrough"] = int(extent_product(raw, self.cloud_leaf) > INT32_MAX)
            glob = _vg(raw, self.cloud_leaf)
        self.calls += 1
        rep.update(call=self.calls, n_in_radius=len(near), n_poses_used=len(ids), downsampled_poses=int(ds),
                   downsampled_cloud=int(ds), n_edge=len(edge), n_planar=len(planar), n_global_raw=len(raw),
                   n_global=len(glob))
        out.update({"global": glob, "edge": edge, "planar": planar})
        return out

    def save_map(self):
        corner = _cat([w[0] for w in self.world])
        surf = _cat([c for w in self.world for c in w[1:]])
        return corner, _vg(surf, self.surf_leaf)
