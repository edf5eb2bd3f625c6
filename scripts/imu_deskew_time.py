"""Times the IMU de-skew inside the feature stage: k_fa_points' interval per 1024 VLP-16 scans from
llsr_kernel_times_ms (HIP events around the kernel on the batch's stream) with nothing staged, with
10-sample windows (100 Hz) and with 50-sample windows (500 Hz) staged for every slot, next to
k_select_ring's; and the resources and occupancy of both k_fa_points kernels from
profiles/imu_kernel_resources.json (scripts/kres_linked.py). With windows staged the interval also
holds the three host-to-device copies of the staging (they are enqueued between the same events).
Writes profiles/imu_deskew_time.json.

    python scripts/imu_deskew_time.py [--batch 1024] [--reps 5] [--out profiles/imu_deskew_time.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lego-loam-sr_amd"))
LDS_PER_CU = 160 * 1024  # gfx950


def main():
    import numpy as np
    import torch

    import llsr
    from llsr import synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "imu_deskew_time.json"))
    a = ap.parse_args()
    B = a.batch
    cfg = llsr.default_config("vlp16")
    pts, off = synth.make_batch(B, "vlp16", distinct=8, seed0=1)
    d_pts, d_off = torch.from_numpy(pts).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    pipe = llsr.Pipeline(cfg, max_batch=B, max_points=40000)
    stamp = synth.scan_stamp(1)

    def window(rate_hz):
        st = llsr.ImuState(cfg.scan_period)
        for m in synth.imu_stream(1, rate_hz, 1, lead=1.0 / rate_hz):
            st.callback(m["sec"], m["nanosec"], m["orientation"], m["angular_velocity"], m["linear_acceleration"])
        return st.scan_window()

    cases = {"nothing_staged": None, "windows_10": window(100), "windows_50": window(500)}
    out = {"build_id": llsr.build_id(), "device": torch.cuda.get_device_name(0), "batch": B, "reps": a.reps,
           "timing": "llsr_kernel_times_ms: HIP events around the kernel, mean per batch, median of reps, "
                     "scaled to 1024 scans", "cases": {}}
    for name, w in cases.items():
        def run():
            if w is not None:
                pipe.stage_imu([stamp] * B, [w] * B)
            pipe.process_batch(d_pts.data_ptr(), d_off.data_ptr(), B)
        for _ in range(2):
            run()
        fa, sel = [], []
        for _ in range(a.reps):
            pipe.set_profiling(True)
            run()
            t = pipe.kernel_times()
            pipe.set_profiling(False)
            fa.append(t["k_fa_points"] * 1024.0 / B)
            sel.append(t["k_select_ring"] * 1024.0 / B)
        out["cases"][name] = {"window_entries": 0 if w is None else int(len(w)),
                              "k_fa_points_ms_per_1024": statistics.median(fa), "k_fa_points_ms_all": fa,
                              "k_select_ring_ms_per_1024": statistics.median(sel)}
    pipe.close()
    base = out["cases"]["nothing_staged"]
    out["todays_fa_points_plus_select_ring_ms"] = base["k_fa_points_ms_per_1024"] + base["k_select_ring_ms_per_1024"]
    kres = os.path.join(REPO, "profiles", "imu_kernel_resources.json")
    if os.path.exists(kres):
        res = {}
        for k in json.load(open(kres))["kernels"].values():
            if k["kernel"] in ("k_fa_points", "k_fa_points_imu"):
                wg_lds = LDS_PER_CU // max(k["lds_bytes"], 1)
                res[k["kernel"]] = dict(k, workgroups_per_cu_by_lds=wg_lds,
                                        waves_per_simd=min(k["waves_per_simd_by_registers"], wg_lds))  # 4 waves / WG, 4 SIMDs
        out["resources"] = res
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
