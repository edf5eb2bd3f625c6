"""bench.py --gpus N (the driver's contract): without a launcher it starts torchrun as a child
process with one rank per GPU (never exec'ing itself), and it refuses a world size that does
not match --gpus, so an N-GPU line can never silently measure one GPU."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_launcher_command_line():
    cmd = bench.launcher_cmd(["--gpus", "4", "--steps", "7"], 4, 29517)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd and "--master-port=29517" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "7"]
    assert os.path.samefile(cmd[-5], os.path.join(REPO, "bench.py"))


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "4"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--gpus 4 but WORLD_SIZE=2" in r.stderr


HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                 "scaling", "vs_baseline", "build_id", "dtype", "data", "config"}


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps_last_step(require_gpu, tmp_path):
    """A plain run prints the headline keys only (nothing of --full), --steps sets the timed steps,
    and --dump-outputs writes what the handle of the last timed step holds: the same files as a
    replay of that handle's batches (warm-up step 0, timed steps 0 and 3 of 4 on 3 streams)."""
    import json
    import numpy as np
    import torch
    from llsr import Pipeline, _abi, default_config, synth
    B, steps, warmup, distinct = 24, 4, 1, 4
    got = tmp_path / "got"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--batch", str(B), "--distinct", str(distinct),
                        "--dump-outputs", str(got)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert set(line) == HEADLINE_KEYS
    assert line["steps"] == steps and line["unit"] == "scans/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(B / (line["ms_per_step"] * 1e-3), rel=1e-2)

    cfg = default_config("vlp16")
    pts, off = synth.make_batch(B, "vlp16", distinct=distinct, seed0=1)
    pipe = Pipeline(cfg, max_batch=B, max_points=int(np.diff(off).max()))
    pipe.set_voxel_order(bench.VOXEL_ORDERS["pcl"])
    d_pts, d_off = torch.from_numpy(pts).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    for _ in range(3):
        pipe.process_batch(d_pts.data_ptr(), d_off.data_ptr(), B)
    want = tmp_path / "want"
    bench.dump_outputs(str(want), pipe, B)
    names = sorted(os.listdir(want))
    assert sorted(os.listdir(got)) == names
    assert {"counts.npy", "sample_slots.npy", "scan_counts.npy"} | {a[0] + ".npy" for a in _abi.ARRAYS} <= set(names)
    total = 0
    for n in names:
        g, w = np.load(got / n), np.load(want / n)
        assert g.dtype in (np.float32, np.float64), n
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=True), n
        total += g.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    slots = np.load(got / "sample_slots.npy").astype(int)
    assert len(set(slots)) == len(slots) == min(bench.DUMP_SLOTS, B) and slots.max() < B
    assert np.array_equal(np.load(got / "counts.npy"), pipe.batch_counts(B))
    seg = np.concatenate([pipe.fetch(int(b))["seg_xyzi"] for b in slots])
    assert np.array_equal(np.load(got / "seg_xyzi.npy"), seg)
    pipe.close()


@pytest.mark.parametrize("n", [1])
def test_free_port(n):
    p = bench.free_port()
    assert 1024 < p < 65536
