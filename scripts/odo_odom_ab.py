#!/usr/bin/env python3
"""A/B of the odometry batch with and without updateInitialGuess (llsr_odometry_batch vs
llsr_odometry_batch_odom with every slot flagged) on bench.py's VLP-16 odometry leg: the same B,
drives, frame count, warm-up and timed steps (read from bench.py's defaults), one process, one
handle. A round is bench.py's own leg (reset, warm-up, timed steps ending in a synchronise); the
rounds of the variants alternate (base, odom, odom with no slot flagged, base again) so that drift hits them alike, and
`--rounds` of them add up to a window of seconds per variant. The second base series gives the
spread of the same code against itself.

Writes profiles/odo_odom_ab_<build id>.json and prints it. Needs a HIP device.

  python scripts/odo_odom_ab.py [--rounds 40] [--out profiles/...json]
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lego-loam-sr_amd"))


def bench_defaults():
    """B of the VLP-16 odometry leg and its steps from bench.py's argument defaults; the leg runs 2
    drives, 2 warm-up steps and frames = 2 + steps (bench.py main(): odometry_leg(dev, lid, nb, 2,
    2 + s2m_steps, s2m_steps, 2, ...))."""
    # bench.py builds its parser inside main(), so the defaults are not importable: they are read
    # from its source, and any change of the three places read here stops the script
    src = open(os.path.join(REPO, "bench.py")).read()
    odo = re.search(r'"--odo",\s*default="([^"]*)"', src)
    steps = re.search(r'"--s2m-steps",\s*type=int,\s*default=(\d+)', src)
    call = re.search(r'odometry_leg\(dev,\s*lid,\s*int\(nb\),\s*(\d+),\s*(\d+)\s*\+\s*args\.s2m_steps,\s*'
                     r'args\.s2m_steps,\s*(\d+),', src)
    if not odo or not steps or not call:
        raise SystemExit("odo_odom_ab.py: bench.py's --odo / --s2m-steps defaults or its odometry_leg(...) call "
                         "changed; update bench_defaults() to match")
    seqs, extra, warmup = (int(v) for v in call.groups())
    if extra != warmup:
        raise SystemExit("odo_odom_ab.py: bench.py's odometry leg no longer runs frames = warm-up + steps")
    legs = dict(item.split(":") for item in odo.group(1).split(","))
    if "vlp16" not in legs:
        raise SystemExit("odo_odom_ab.py: bench.py's --odo default has no vlp16 leg")
    return int(legs["vlp16"]), seqs, int(steps.group(1)), warmup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("base", "odom"), default=None,
                    help="run one variant alone (for a profiler run of its own); writes no record")
    args = ap.parse_args()
    import torch
    import llsr
    from llsr import Pipeline, _abi, default_config, synth
    if not torch.cuda.is_available():
        raise SystemExit("odo_odom_ab.py: no HIP device")
    dev = torch.device("cuda", 0)
    B, seqs, steps, warmup = bench_defaults()
    frames = warmup + steps
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    H, W = cfg.num_vertical_scans, cfg.num_horizontal_scans
    seeds = [[1 + 64 * q + k for k in range(frames)] for q in range(seqs)]
    seq_scans = [[synth.make_scan(s, "vlp16", motion=True) for s in row] for row in seeds]
    batches, samples = [], []
    states = [llsr.odom_init() for _ in range(seqs)]
    for k in range(frames):
        scans = [seq_scans[b % seqs][k] for b in range(B)]
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum([len(a) for a in scans])
        batches.append((torch.from_numpy(np.concatenate(scans)).to(dev), torch.from_numpy(off).to(dev)))
        for q in range(seqs):  # one /odom2 message per drive and frame, before the frame
            llsr.odom_callback(states[q], synth.odom_message(seeds[q][k]))
        arr = (_abi.OdomSample * B)()
        for b in range(B):
            arr[b] = states[b % seqs].last
        samples.append(arr)
    pipe = Pipeline(cfg, device=0, max_batch=B, max_points=H * W)

    no_flags = np.zeros(B, np.uint8)

    def round_(odom, flags=None) -> float:
        pipe.odometry_reset()
        torch.cuda.synchronize(dev)
        for n in range(frames):
            if n == warmup:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
            d_pts, d_off = batches[n]
            if odom:
                pipe.odometry_batch_odom(d_pts.data_ptr(), d_off.data_ptr(), B, samples[n], flags)
            else:
                pipe.odometry_batch(d_pts.data_ptr(), d_off.data_ptr(), B)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    if args.only:
        for _ in range(args.rounds + 1):
            dt = round_(args.only == "odom")
        print(json.dumps({"only": args.only, "rounds": args.rounds, "last_round_scans_per_s": round(B * steps / dt, 1)}))
        pipe.close()
        return

    def lm_iterations(odom: bool) -> list:
        """surf + corner LM iterations of the two drives on each timed frame (untimed diagnostic
        round): the overwrite changes the last clouds and the initial guess, and so the LM's work."""
        pipe.odometry_reset()
        its = []
        for n in range(frames):
            d_pts, d_off = batches[n]
            if odom:
                pipe.odometry_batch_odom(d_pts.data_ptr(), d_off.data_ptr(), B, samples[n])
            else:
                pipe.odometry_batch(d_pts.data_ptr(), d_off.data_ptr(), B)
            if n >= warmup:
                lm = [pipe.odometry_fetch(q)["lm"] for q in range(seqs)]
                its.append([r["surf_iterations"] + r["corner_iterations"] for r in lm])
        return its

    for odom in (False, True, False):  # code objects, allocations, the LM instantiations
        round_(odom)
    round_(True, no_flags)
    # odom_unflagged: llsr_odometry_batch_odom with overwrite all zero computes what base computes,
    # through the new entry point's copies and kernel branch: the mechanism without the changed LM work
    t = {"base": [], "odom": [], "odom_unflagged": [], "base_again": []}
    for _ in range(args.rounds):
        t["base"].append(round_(False))
        t["odom"].append(round_(True))
        t["odom_unflagged"].append(round_(True, no_flags))
        t["base_again"].append(round_(False))
    s0 = pipe.odometry_fetch(0)
    its = {"base": lm_iterations(False), "odom": lm_iterations(True)}
    pipe.close()
    rate = {k: B * steps * len(v) / sum(v) for k, v in t.items()}
    med = {k: B * steps / statistics.median(v) for k, v in t.items()}
    spread = abs(rate["base"] - rate["base_again"]) / rate["base"]
    base_mean = 0.5 * (rate["base"] + rate["base_again"])
    deficit = 1.0 - rate["odom"] / base_mean
    rec = {
        "what": "VLP-16 odometry leg of bench.py: llsr_odometry_batch vs llsr_odometry_batch_odom (all slots flagged)",
        "build_id": llsr.build_id(), "device": torch.cuda.get_device_name(0),
        "B": B, "drives": seqs, "frames": frames, "warmup": warmup, "timed_steps": steps, "rounds": args.rounds,
        "window_s": {k: round(sum(v), 3) for k, v in t.items()},
        "scans_per_s": {k: round(v, 1) for k, v in rate.items()},
        "scans_per_s_median_round": {k: round(v, 1) for k, v in med.items()},
        "spread_base_vs_base": round(spread, 5),
        "odom_deficit_vs_base_mean": round(deficit, 5),
        "odom_deficit_exceeds_twice_spread": bool(deficit > 2.0 * spread),
        "odom_unflagged_deficit_vs_base_mean": round(1.0 - rate["odom_unflagged"] / base_mean, 5),
        "last_frames_slot0": int(s0["frames"]),
        "lm_iterations_per_timed_frame_and_drive": its,
        "lm_iterations_sum": {k: int(np.sum(v)) for k, v in its.items()},
    }
    out = args.out or os.path.join(REPO, "profiles", f"odo_odom_ab_{rec['build_id']}.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
