"""Times llsr_icp_align_batch against the same alignments as sequential llsr_icp_align calls, on pairs
cut from the recorded run: the 723 recorded keyframes (tests/_result_map.keyframes) at 1 s spacing, and
for P distinct "latest" keyframes the two raw clouds llsr_map_loop_submaps would cut for each — the
keyframe's corner then surf cloud in the map frame (points with (int)intensity >= 0), and keyframes
closest - search_num .. closest + search_num around the newest keyframe at least 30 s older (the
HDL-64E block's search_num). For P in {1, 4, 16, 64}, alternating in one session after a warm-up of
both: P sequential llsr_icp_align calls, and one llsr_icp_align_batch call, each bracketed by HIP events
on the workspace's stream; the median and the spread of reps runs. The results of the two forms are
compared bit for bit. Prints the numbers and writes them, with the library's build id, to
profiles/loop_closure_batch_time.json.

    python scripts/loop_closure_batch_time.py [--reps 5] [--out profiles/loop_closure_batch_time.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lego-loam-sr_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

SIZES = (1, 4, 16, 64)


def main():
    import numpy as np
    import torch

    import _result_map as R
    import llsr
    import oracle_py

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loop_closure_batch_time.json"))
    a = ap.parse_args()
    frames = R.keyframes(R.load())
    K = len(frames)
    cfg = llsr.loop_config("hdl64e")
    num, gap = int(cfg.search_num), int(cfg.min_time_gap)

    def cloud(k):  # keyframe k's corner then surf cloud through the oracle's transformPointCloud
        pose, corner, surf, _ = frames[k]
        return np.concatenate([oracle_py.transform_keyframe(pose, corner), oracle_py.transform_keyframe(pose, surf)])

    def pair(latest):
        closest = latest - gap - 1  # the newest keyframe more than `gap` seconds older, at 1 s spacing
        src = cloud(latest)
        src = src[(src[:, 3] > -1.0) & (src[:, 3] < 2147483648.0)]
        tgt = np.concatenate([cloud(k) for k in range(max(closest - num, 0), min(closest + num, K - 1) + 1)])
        return np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)

    P_max = max(SIZES)
    latest = np.linspace(gap + 1 + num, K - 1, P_max).astype(int)  # distinct, the last is the newest keyframe
    assert len(set(latest.tolist())) == P_max
    pairs = [pair(int(k)) for k in latest[::-1]]  # the newest first: P = 1 is the pair of loop_closure_time.py

    dev = torch.device("cuda", 0)
    icp = llsr.Icp(0)
    L, s = llsr.lib(), icp._s
    out = {"build_id": llsr.build_id(), "device": torch.cuda.get_device_name(0), "keyframes": K, "reps": a.reps,
           "keyframe_spacing_s": 1.0, "search_num": num, "min_time_gap_s": float(gap),
           "timing": "HIP events on the workspace's stream around P sequential llsr_icp_align calls and around one "
                     "llsr_icp_align_batch call, alternating, after one warm-up of each; median, min and max of reps",
           "sizes": {}}
    for P in SIZES:
        so, to = np.zeros(P + 1, np.int64), np.zeros(P + 1, np.int64)
        so[1:] = np.cumsum([len(p[0]) for p in pairs[:P]])
        to[1:] = np.cumsum([len(p[1]) for p in pairs[:P]])
        d_src = torch.from_numpy(np.concatenate([p[0] for p in pairs[:P]])).to(dev)
        d_tgt = torch.from_numpy(np.concatenate([p[1] for p in pairs[:P]])).to(dev)
        al_seq, al_bat = torch.zeros_like(d_src), torch.zeros_like(d_src)
        r_seq, r_bat = (llsr._abi.IcpResult * P)(), (llsr._abi.IcpResult * P)()
        torch.cuda.synchronize()

        def sequential():
            for p in range(P):
                rc = L.llsr_icp_align(icp._w, C.c_void_p(d_src.data_ptr() + 16 * int(so[p])), int(so[p + 1] - so[p]),
                                      C.c_void_p(d_tgt.data_ptr() + 16 * int(to[p])), int(to[p + 1] - to[p]),
                                      C.byref(cfg), C.byref(r_seq[p]), C.c_void_p(al_seq.data_ptr() + 16 * int(so[p])),
                                      C.c_void_p(s.cuda_stream))
                if rc != 0:
                    raise SystemExit(f"llsr_icp_align: {rc}")

        def batch():
            rc = L.llsr_icp_align_batch(icp._w, P, C.c_void_p(d_src.data_ptr()), so.ctypes.data,
                                        C.c_void_p(d_tgt.data_ptr()), to.ctypes.data, C.byref(cfg), 1, r_bat,
                                        C.c_void_p(al_bat.data_ptr()), C.c_void_p(s.cuda_stream))
            if rc != 0:
                raise SystemExit(f"llsr_icp_align_batch: {rc}: {L.llsr_icp_last_error(icp._w).decode()}")

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1)

        sequential(), batch()  # warm-up: every buffer grown, both forms
        seq_ms, bat_ms = [], []
        for _ in range(a.reps):
            seq_ms.append(timed(sequential))
            bat_ms.append(timed(batch))
        tm = icp.last_times()
        same = bool(torch.equal(al_seq, al_bat)) and all(
            bytes(r_seq[p]) == bytes(r_bat[p]) for p in range(P))
        its = [int(r_bat[p].iterations) for p in range(P)]
        out["sizes"][str(P)] = {
            "source_points": int(so[P]), "target_points": int(to[P]), "largest_source": int(np.diff(so).max()),
            "largest_target": int(np.diff(to).max()), "problems_with_an_iteration": sum(1 for i in its if i > 0),
            "iterations_min": min(its), "iterations_max": max(its), "iterations_sum": sum(its),
            "passes": int(icp.last_passes()),
            "sequential_ms": statistics.median(seq_ms), "sequential_ms_min": min(seq_ms), "sequential_ms_max": max(seq_ms),
            "batch_ms": statistics.median(bat_ms), "batch_ms_min": min(bat_ms), "batch_ms_max": max(bat_ms),
            "batch_corr_ms_per_pass": tm["corr_ms"] / max(icp.last_passes(), 1),
            "batch_solve_ms_per_pass": tm["solve_ms"] / max(icp.last_passes(), 1),
            "sequential_over_batch": statistics.median(seq_ms) / statistics.median(bat_ms),
            "results_bit_equal": same,
        }
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    icp.close()


if __name__ == "__main__":
    main()
