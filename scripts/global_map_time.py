"""Times the global map on the recorded run: the 723 recorded keyframes (tests/_result_map.keyframes)
in one llsr_map, then llsr_map_global as a first call (raw) and as a later call (downsampled) and
llsr_map_save, bracketed by HIP events on the map's stream after a warm-up on a map of its own, and
the assembly kernel k_global_assemble alone (device time from the profiler's kernel records of a
raw call) against its compulsory traffic: 16 B read per source point plus 16 B per destination
written. Prints the numbers and writes them, with the library's build id, to
profiles/global_map_time.json.

    python scripts/global_map_time.py [--reps 5] [--out profiles/global_map_time.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lego-loam-sr_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
HBM_PEAK = 8.0e12  # MI355X HBM3E peak, bytes / s


def main():
    import torch

    import _result_map as R
    import llsr

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "global_map_time.json"))
    a = ap.parse_args()
    frames = R.keyframes(R.load())
    pos = frames[-1][0][:3]

    def fresh():
        m = llsr.LocalMap(0)
        for f in frames:
            m.add_keyframe(*f)
        return m

    def timed(m, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(m._s)
        r = fn()
        e1.record(m._s)
        e1.synchronize()
        return e0.elapsed_time(e1), r

    warm = fresh()
    for _ in range(3):
        warm.global_map(pos)
        warm.save_map()
    caps = list(warm._gm_caps)  # output capacities that fit every call below without a retry
    warm.close()
    first, later, save = [], [], []
    rep_first = rep_later = None
    for _ in range(a.reps):
        m = fresh()
        m._gm_caps = list(caps)
        ms, r = timed(m, lambda: m.global_map(pos))
        assert r["report"]["call"] == 1 and not r["report"]["downsampled_cloud"]
        first.append(ms)
        rep_first = r["report"]
        ms, r = timed(m, lambda: m.global_map(pos))
        assert r["report"]["call"] == 2 and r["report"]["downsampled_cloud"]
        later.append(ms)
        rep_later = r["report"]
        m.save_map()
        ms, (c, s) = timed(m, m.save_map)
        save.append(ms)
        n_save = (len(c), len(s))
        m.close()
    # the assembly kernel alone: a raw call (high_dense) under the profiler
    m = fresh()
    cfg = llsr.global_map_config(high_dense=1)
    m.global_map(pos, cfg)
    kernel_us = []
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for _ in range(a.reps):
            m.global_map(pos, cfg)
        torch.cuda.synchronize()
    for ev in prof.events():
        if "k_global_assemble" in ev.name:
            kernel_us.append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
    m.close()
    raw = rep_first["n_global_raw"]
    traffic = 16 * (raw + rep_first["n_edge"] + rep_first["n_planar"] + raw)
    out = {
        "build_id": llsr.build_id(), "device": torch.cuda.get_device_name(0), "keyframes": len(frames),
        "reps": a.reps, "timing": "HIP events on the map's stream around the whole call, median of reps",
        "first_call_ms": statistics.median(first), "later_call_ms": statistics.median(later),
        "save_ms": statistics.median(save), "first_call_report": rep_first, "later_call_report": rep_later,
        "save_points": {"corner": n_save[0], "surf": n_save[1]},
        "assemble_traffic_bytes": traffic,
    }
    if kernel_us:
        us = statistics.median(kernel_us)
        out.update(assemble_kernel_us=us, assemble_bytes_per_s=traffic / (us * 1e-6),
                   assemble_hbm_fraction=traffic / (us * 1e-6) / HBM_PEAK, hbm_peak_bytes_per_s=HBM_PEAK)
    else:
        out["assemble_kernel_us"] = None  # the profiler recorded no kernel: no bandwidth figure
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
