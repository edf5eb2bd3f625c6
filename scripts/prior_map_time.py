"""Times the prior map's crop (llsr_prior_crop_batch) and what the parent offers for a
frozen map, and writes the numbers, with the library's build id, to profiles/prior_map_time.json.

(a) The recorded map (tests/golden/result_0318.npz) at the recorded key positions, radius 5 m, tile
    1 m, with P = 1, 64 and 723 positions per call.
(b) For the 64 positions of (a): llsr_map_extract (extractSurroundingKeyFrames, radius 5 m) on a store
    of the 723 recorded keyframes (tests/_result_map.keyframes), one call per position — existing
    calls only.
(c) A synthetic map of 4 M points (1 M corner, 3 M surf, uniform over 2 km x 2 km x 20 m), 1024
    positions, radius 50 m, tile 10 m.

Crop times are the object's own HIP events (around the counting and scan kernels with the copy of the
totals, and around the writing kernel), median over reps; wall_ms is the whole call on the host. Bytes
moved are 16 B per point tested plus 16 B per point written, as a fraction of the HBM peak;
`bytes_read_twice` adds the second read of the tested points (the writing kernel repeats the test),
which is what the kernels load in all. The recorded map is 1.4 MB and the 723 positions overlap, so
its points come out of the caches: there the fraction is a rate against the HBM yardstick, not HBM
traffic.

    python scripts/prior_map_time.py [--reps 7] [--out profiles/prior_map_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lego-loam-sr_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
HBM_PEAK = 8.0e12  # MI355X HBM3E peak, bytes / s


def crop_leg(m, pos, reps):
    import numpy as np
    import torch
    first = m.crop(pos)  # sizes, and the warm-up
    total = int(first["surf_off"][-1])
    ms, wall = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.crop(pos, cap=total)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(m.last_crop()["ms"])
    st = m.last_crop()
    med = statistics.median(ms)
    moved = 16 * (st["tested"] + st["written"])
    return {"positions": int(len(pos)), "device_ms": med, "device_ms_min": min(ms), "wall_ms": statistics.median(wall),
            "device_us_per_position": med * 1e3 / len(pos), "points_tested": st["tested"],
            "points_written": st["written"], "corner_written": int(first["corner_off"][-1]),
            "bytes_moved": moved, "bytes_read_twice": moved + 16 * st["tested"],
            "bytes_per_s": moved / (med * 1e-3), "hbm_fraction": moved / (med * 1e-3) / HBM_PEAK,
            "mean_crop_points": float(np.diff(first["corner_off"]).mean() + np.diff(first["surf_off"]).mean())}


def main():
    import numpy as np
    import torch

    import _result_map as R
    import llsr

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "prior_map_time.json"))
    a = ap.parse_args()
    z = R.load()
    keys = np.ascontiguousarray(z["key_poses"][:, :3], np.float32)
    idx64 = np.linspace(0, len(keys) - 1, 64).astype(int)
    out = {"build_id": llsr.build_id(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "timing": "HIP events inside llsr_prior_crop_batch (both kernel groups), median of reps",
           "hbm_peak_bytes_per_s": HBM_PEAK}

    # (a) the recorded map, radius 5 m, tile 1 m
    m = llsr.PriorMap(radius=5.0, tile=1.0, device=0)
    t0 = time.perf_counter()
    m.load(z["corner_map"], z["surf_map"])
    info = m.info()
    out["recorded"] = {"load_ms": (time.perf_counter() - t0) * 1e3, "radius": 5.0, "tile": 1.0,
                       "corner": info["corner"], "surf": info["surf"],
                       "P1": crop_leg(m, keys[380:381], a.reps), "P64": crop_leg(m, keys[idx64], a.reps),
                       "P723": crop_leg(m, keys, a.reps)}
    m.close()

    # (b) the parent's way to a local map of a frozen map: extract on a store of the recorded keyframes
    frames = R.keyframes(z)
    lm = llsr.LocalMap(0, llsr.map_config(surrounding_radius=5.0))
    for f in frames:
        lm.add_keyframe(*f)
    for k in idx64[:4]:
        lm.extract(keys[k])  # warm-up: buffers grow
    ems, sizes = [], []
    for _ in range(max(1, a.reps // 3)):
        for k in idx64:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(lm._s)
            r = lm.extract(keys[k])
            e1.record(lm._s)
            e1.synchronize()
            ems.append(e0.elapsed_time(e1))
            sizes.append(len(r[0]) + len(r[1]))
    lm.close()
    out["parent_extract"] = {"positions": 64, "keyframes": len(frames), "radius": 5.0,
                             "device_ms_per_position": statistics.median(ems), "device_ms_min": min(ems),
                             "mean_local_map_points": float(np.mean(sizes)),
                             "note": "one llsr_map_extract per position (radius branch; its VoxelGrid runs per call)"}
    out["crop_vs_extract_per_position"] = {
        "extract_us": statistics.median(ems) * 1e3,
        "crop_us_P1": out["recorded"]["P1"]["device_us_per_position"],
        "crop_us_P64": out["recorded"]["P64"]["device_us_per_position"],
        "crop_us_P723": out["recorded"]["P723"]["device_us_per_position"]}

    # (c) synthetic: 4 M points, 1024 positions, radius 50 m, tile 10 m
    rng = np.random.default_rng(7)

    def cloud(n):
        c = np.zeros((n, 4), np.float32)
        c[:, 0], c[:, 1], c[:, 2] = rng.uniform(-1000, 1000, n), rng.uniform(-1000, 1000, n), rng.uniform(-10, 10, n)
        return c
    pos = np.stack([rng.uniform(-950, 950, 1024), rng.uniform(-950, 950, 1024), rng.uniform(-2, 2, 1024)], 1)
    m = llsr.PriorMap(radius=50.0, tile=10.0, device=0)
    t0 = time.perf_counter()
    m.load(cloud(1 << 20), cloud(3 << 20))
    info = m.info()
    out["synthetic"] = {"load_ms": (time.perf_counter() - t0) * 1e3, "radius": 50.0, "tile": 10.0,
                        "corner": info["corner"], "surf": info["surf"],
                        "P1024": crop_leg(m, pos.astype(np.float32), a.reps)}
    m.close()
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
