"""Times the loop closure on the recorded run: the 723 recorded keyframes (tests/_result_map.keyframes)
in one llsr_map with times at a fixed spacing, then llsr_map_loop_closure around the last key pose,
bracketed by HIP events on the map's stream (median of reps, after a warm-up call), the split of the
alignment's device time between the correspondence kernel and the solve kernels (llsr_icp_last_times),
and llsr_icp_align_host on the same two clouds on one host core. The search radius starts at the
HDL-64E block's and doubles until a candidate exists; the radius used is recorded. Prints the numbers
and writes them, with the library's build id, to profiles/loop_closure_time.json.

    python scripts/loop_closure_time.py [--reps 5] [--spacing 1.0] [--out profiles/loop_closure_time.json]
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


def main():
    import numpy as np
    import torch

    import _result_map as R
    import llsr

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spacing", type=float, default=1.0, help="seconds between keyframes")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loop_closure_time.json"))
    a = ap.parse_args()
    frames = R.keyframes(R.load())
    pos = frames[-1][0][:3]
    now = a.spacing * (len(frames) - 1)
    m = llsr.LocalMap(0, llsr.map_config("hdl64e"))
    for k, f in enumerate(frames):
        m.add_keyframe(*f)
        m.set_keyframe_time(k, a.spacing * k)
    cfg = llsr.loop_config("hdl64e")
    radius = float(cfg.search_radius)
    while not m.loop_submaps(pos, now, cfg)["found"]:
        radius *= 2.0
        if radius > 1.0e5:
            raise SystemExit("no keyframe is older than the time gap")
        cfg.search_radius = radius
    sub = m.loop_submaps(pos, now, cfg)
    icp = llsr.Icp(0)
    caps = [int(sub["n_source"]), int(sub["n_target_ds"])]  # capacities that fit without a retry
    r = m.loop_closure(pos, now, cfg, icp=icp, caps=caps)  # warm-up: every buffer grown

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(m._s)
        out = fn()
        e1.record(m._s)
        e1.synchronize()
        return e0.elapsed_time(e1), out

    call_ms, corr_ms, solve_ms, align_ms = [], [], [], []
    for _ in range(a.reps):
        ms, r = timed(lambda: m.loop_closure(pos, now, cfg, icp=icp, caps=caps))
        t = icp.last_times()
        call_ms.append(ms)
        corr_ms.append(t["corr_ms"])
        solve_ms.append(t["solve_ms"])
        align_ms.append(t["total_ms"])
    src, tgt = sub["source"].cpu().numpy(), sub["target"].cpu().numpy()
    host_ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        h = llsr.icp_align_host(src, tgt, cfg)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    same = bool(np.array_equal(h["T"].view(np.uint32), r["T"].view(np.uint32)) and h["fitness"] == r["fitness"]
                and h["iterations"] == r["iterations"])
    it = max(int(r["iterations"]), 1)
    corr, solve = statistics.median(corr_ms), statistics.median(solve_ms)
    out = {
        "build_id": llsr.build_id(), "device": torch.cuda.get_device_name(0), "keyframes": len(frames),
        "reps": a.reps, "keyframe_spacing_s": a.spacing,
        "timing": "HIP events on the map's stream around the whole llsr_map_loop_closure call, median of reps; "
                  "the split from llsr_icp_last_times (HIP events around the kernels, summed over the iterations)",
        "search_radius_m": radius, "search_num": int(cfg.search_num), "closest_id": int(r["closest_id"]),
        "n_source": int(r["n_source"]), "n_target": int(r["n_target"]), "n_source_ds": int(r["n_source_ds"]),
        "n_target_ds": int(r["n_target_ds"]), "iterations": int(r["iterations"]),
        "state": llsr._abi.ICP_STATES[int(r["state"])], "converged": bool(r["converged"]), "fitness": float(r["fitness"]),
        "accepted": bool(r["accepted"]), "n_pairs_last": int(r["n_pairs_last"]),
        "loop_closure_call_ms": statistics.median(call_ms), "loop_closure_call_ms_min": min(call_ms),
        "loop_closure_call_ms_max": max(call_ms), "icp_align_device_ms": statistics.median(align_ms),
        "corr_ms_per_iteration": corr / it, "solve_ms_per_iteration": solve / it,
        "iteration_bound_by": "correspondence search" if corr > solve else "solve (pack, chains, estimate)",
        "icp_align_host_ms": statistics.median(host_ms), "icp_align_host_ms_min": min(host_ms),
        "icp_align_host_ms_max": max(host_ms), "host_equals_device_bits": same,
        "device_over_host": statistics.median(align_ms) / statistics.median(host_ms),
    }
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    icp.close()
    m.close()


if __name__ == "__main__":
    main()
