"""k_odo_finish_imu against k_odo_finish (and k_odo_inputs_imu against k_odo_inputs) on the same batch:
device durations from a rocprofv3 kernel trace of one run that drives 1024 VLP-16 sequences through
llsr_odometry_batch_odom, first with use_imu_undistortion off, then on, with the same IMU windows
staged in both halves (so the feature stage is the same and the reports are not zero).

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/imu_undistortion_time.py run
    python scripts/imu_undistortion_time.py reduce DIR [profiles/imu_undistortion_finish_time.json]
"""
import csv
import glob
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lego-loam-sr_amd"))
B, FRAMES, DISTINCT = 1024, 6, 8


def run():
    import numpy as np
    import torch

    import llsr
    from llsr import _abi, synth

    cfg = llsr.default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    frames = []
    for k in range(FRAMES):  # DISTINCT drives, repeated over the slots
        scans = [synth.make_scan(64 * d + 1 + k, "vlp16", motion=True) for d in range(DISTINCT)]
        off = np.arange(B + 1, dtype=np.int64) * len(scans[0])
        pts = np.concatenate([scans[b % DISTINCT] for b in range(B)])
        frames.append((torch.from_numpy(pts).cuda(), torch.from_numpy(off).cuda()))
    torch.cuda.synchronize()
    sample = [0.01, -0.02, 0.03, 0.4, 0.05, -0.02]
    for on in (False, True):
        pipe = llsr.Pipeline(cfg, max_batch=B, max_points=16 * 1800)
        pipe.set_imu_undistortion(on)
        st = llsr.ImuState(cfg.scan_period)
        stream = synth.imu_stream(1, 100, FRAMES)
        t = stream["sec"].astype(np.int64) * 10 ** 9 + stream["nanosec"]
        fed = 0
        for k, (d_pts, d_off) in enumerate(frames):
            stamp = synth.scan_stamp(1 + k)
            upto = int(np.searchsorted(t, stamp[0] * 10 ** 9 + stamp[1] + 100_000_000))
            for m in stream[fed:upto]:
                st.callback(m["sec"], m["nanosec"], m["orientation"], m["angular_velocity"], m["linear_acceleration"])
            fed = upto
            pipe.stage_imu([stamp] * B, [st.scan_window()] * B)
            pipe.odometry_batch_odom(d_pts.data_ptr(), d_off.data_ptr(), B, [sample] * B)
        g = pipe.odometry_fetch(0)
        print(json.dumps({"switch": on, "frames": g["frames"], "transform_sum": [float(v) for v in g["transform_sum"]]}))
        pipe.close()


def reduce(d, out_path):
    rows = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("llsr::", "").split("<")[0]
            if name.startswith("k_odo_"):
                rows.setdefault(name, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    out = {"what": "rocprofv3 --kernel-trace device durations, 1024 VLP-16 sequences per llsr_odometry_batch_odom, "
                   f"{FRAMES} frames per half (the first is each slot's initialisation scan and is left out), "
                   "IMU windows staged in both halves", "batch": B, "kernels_us": {}}
    for name, iv in sorted(rows.items()):
        iv.sort()
        dur = [(e - s) / 1e3 for s, e in iv][1:]  # without the initialisation scan
        out["kernels_us"][name] = {"launches": len(dur), "median": round(statistics.median(dur), 2),
                                   "min": round(min(dur), 2), "max": round(max(dur), 2)}
    k = out["kernels_us"]
    if "k_odo_finish" in k and "k_odo_finish_imu" in k:
        out["finish_imu_over_finish"] = round(k["k_odo_finish_imu"]["median"] / k["k_odo_finish"]["median"], 4)
    print(json.dumps(out, indent=1))
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 3 and sys.argv[1] == "reduce":
        reduce(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "imu_undistortion_finish_time.json"))
    else:
        sys.exit(__doc__)
