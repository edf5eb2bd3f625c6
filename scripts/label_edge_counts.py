"""Edge counts of the labelling's union-find on the CPU, from the oracle's range and ground images of
VLP-16 benchmark scans: what k_label<true> resolves in registers and what it leaves to uf_unite.

    python scripts/label_edge_counts.py [seed ...]        (default: seeds 1 2)

Per scan: label-0 cells, right edges (the wrap included) and down edges between two label-0 cells
that pass the BFS angle test, the vertical runs the down links leave, and the right edges left once
every edge below another one between the same two runs is dropped (the ladder rule of the load pass).
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lego-loam-sr_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import oracle_py  # noqa: E402
from llsr import default_config, synth  # noqa: E402


def edge(ra, rb, alpha, theta):
    d1, d2 = np.maximum(ra, rb), np.minimum(ra, rb)
    with np.errstate(all="ignore"):
        return np.arctan2(d2 * np.sin(alpha), d1 - d2 * np.cos(alpha)) > theta


def counts(cfg, out):
    H, W = cfg.num_vertical_scans, cfg.num_horizontal_scans
    r = np.asarray(out["range_image"], np.float64).reshape(H, W)
    g = np.asarray(out["ground_image"]).reshape(H, W)
    l0 = ~((g == 1) | (np.asarray(out["range_image"]).reshape(H, W) == np.finfo(np.float32).max))
    ax = np.deg2rad(360.0 / W)
    ay = np.deg2rad((cfg.vertical_angle_top - cfg.vertical_angle_bottom) / (H - 1))
    theta = np.deg2rad(cfg.segment_theta)
    rr, lr = np.roll(r, -1, axis=1), np.roll(l0, -1, axis=1)
    right = l0 & lr & edge(r, rr, ax, theta)
    down = np.zeros((H, W), bool)  # down[i] = cell (i, j) linked to (i - 1, j)
    down[1:] = l0[1:] & l0[:-1] & edge(r[:-1], r[1:], ay, theta)
    runs = int((l0 & ~down).sum())
    above = np.zeros((H, W), bool)
    above[1:] = right[:-1]
    kept = right & ~(above & down & np.roll(down, -1, axis=1))
    in_wave = right & ((np.arange(W) % 64) != 63)[None, :] & (np.arange(W) != W - 1)[None, :]
    return dict(label0=int(l0.sum()), right=int(right.sum()), right_in_wave=int(in_wave.sum()),
                down=int(down.sum()), vertical_runs=runs, right_kept=int(kept.sum()))


if __name__ == "__main__":
    cfg = default_config("vlp16")
    for seed in [int(a) for a in sys.argv[1:]] or [1, 2]:
        out = oracle_py.Oracle(cfg).process(synth.make_scan(seed, "vlp16"))
        print(seed, counts(cfg, out))
