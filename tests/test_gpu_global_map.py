"""GPU parity of the global map — llsr_map_global (publishGlobalMap, MO:775-892), llsr_map_save
(saveMapService, MO:382-395) and their mapping-chain entry points — against the program-order
restatement over the oracle's primitives (tests/_global_map.py). Every cloud is compared bit for
bit (tests/_compare.py) and every report field exactly; there are no tolerances.

The synthetic keyframes draw their cloud sizes from {0, 1, 255, 256, 257, 1023, 1024, 1025, 2500}:
empty clouds and both edges of the assembly kernel's 256-lane pass and 1024-point chunk occur in
each of the corner, surf and outlier clouds."""
import ctypes as C

import numpy as np
import pytest

import _global_map as G
import _result_map as R
import oracle_py
from _compare import diff_report
from llsr import LocalMap, Pipeline, _abi, default_config, global_map_config, lib, synth

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 255, 256, 257, 1023, 1024, 1025, 2500)
REPORT = ("call", "n_in_radius", "n_poses_used", "downsampled_poses", "downsampled_cloud", "passthrough",
          "n_edge", "n_planar", "n_global_raw", "n_global")
ORIGIN = np.zeros(3, np.float32)


def _cloud(rng, n, half=15.0):
    c = rng.uniform(-half, half, (n, 4)).astype(np.float32)
    c[:, 3] = rng.integers(0, 16, n) + rng.uniform(0, 0.1, n)
    return c


def _make_frames(seed, positions):
    """One keyframe per position: a seeded attitude, and cloud sizes that walk SIZES with a different
    phase per cloud kind, so every size occurs in every kind within nine keyframes."""
    rng = np.random.default_rng(seed)
    frames = []
    for k, xyz in enumerate(positions):
        pose = np.concatenate([np.asarray(xyz, np.float32), rng.uniform(-0.4, 0.4, 3).astype(np.float32)])
        frames.append((pose,) + tuple(_cloud(rng, SIZES[(k + 3 * a) % len(SIZES)]) for a in range(3)))
    return frames


@pytest.fixture(scope="module")
def frames():
    """40 keyframes on a wandering path with ~0.6 m steps: the 1.0 m key-pose VoxelGrid merges some."""
    rng = np.random.default_rng(42)
    steps = rng.normal(0.0, 0.35, (40, 3)).astype(np.float32) + np.array([0.45, 0.2, 0.02], np.float32)
    fr = _make_frames(7, np.cumsum(steps, axis=0))
    for a in range(3):
        assert {len(f[1 + a]) for f in fr} == set(SIZES)
    return fr


def _both(cfg=None, **okw):
    kw = {} if cfg is None else dict(search_radius=cfg.search_radius, keypose_leaf=cfg.keypose_leaf,
                                     cloud_leaf=cfg.cloud_leaf, high_dense=cfg.high_dense,
                                     first_call_raw=cfg.first_call_raw)
    return LocalMap(0), G.GlobalMapOracle(**kw, **okw)


def _add(m, o, fr):
    for f in fr:
        m.add_keyframe(*f)
        o.add_keyframe(*f)


def _np(t):
    return t.detach().cpu().numpy() if t is not None else None


def _errs(got, exp, tag):
    errs = [diff_report(f"{tag} {key}", _np(got[key]), exp[key]) for key in ("global", "edge", "planar")
            if got[key] is not None]
    errs += [f"{tag} report {k}: {got['report'][k]} vs {exp['report'][k]}" for k in REPORT
             if got["report"][k] != exp["report"][k]]
    return [e for e in errs if e]


def test_sequence_of_calls(require_gpu, frames):
    """Calls 1, 2, 3 with keyframes added in between: call 1 raw in distance order, then downsampled."""
    m, o = _both()
    errs, lo = [], 0
    for call, hi in enumerate((25, 33, 40), 1):
        _add(m, o, frames[lo:hi])
        lo = hi
        pos = frames[hi - 1][0][:3] + np.float32(0.25)
        got, exp = m.global_map(pos), o.global_map(pos)
        errs += _errs(got, exp, f"call {call}")
        r = got["report"]
        assert r["call"] == call and r["downsampled_cloud"] == (call > 1) and r["n_in_radius"] == hi
        if call == 1:
            assert r["n_global"] == r["n_global_raw"] and r["n_poses_used"] == hi
        else:
            assert r["n_poses_used"] < hi and 0 < r["n_global"] < r["n_global_raw"] and not r["passthrough"]
    m.close()
    assert not errs, "\n".join(errs)


def test_duplicate_keyframe(require_gpu):
    """Key poses 2 and 5 share a voxel (mean index 3.5 -> 3), pose 3 sits in the next one: on call 2
    keyframe 3 is appended twice, keyframes 2 and 5 not at all."""
    pos = [(10.5, 0.5, 0.5), (20.5, 0.5, 0.5), (0.2, 0.5, 0.5), (1.5, 0.5, 0.5), (30.5, 0.5, 0.5), (0.7, 0.5, 0.5)]
    fr = _make_frames(9, pos)
    m, o = _both()
    _add(m, o, fr)
    m.global_map(ORIGIN), o.global_map(ORIGIN)
    got, exp = m.global_map(ORIGIN), o.global_map(ORIGIN)
    r = got["report"]
    used = [0, 1, 3, 3, 4]
    assert (r["call"], r["n_in_radius"], r["n_poses_used"]) == (2, 6, 5)
    assert r["n_edge"] == sum(len(fr[k][1]) for k in used)
    assert r["n_planar"] == sum(len(fr[k][2]) for k in used)
    assert r["n_global_raw"] == sum(len(fr[k][1]) + len(fr[k][2]) + len(fr[k][3]) for k in used)
    w3 = oracle_py.transform_keyframe(fr[3][0], fr[3][1])
    edge = _np(got["edge"])
    hits = [i for i in range(len(edge) - len(w3) + 1) if np.array_equal(edge[i:i + len(w3)], w3)] if len(w3) else []
    assert len(w3) and len(hits) == 2, hits
    m.close()
    errs = _errs(got, exp, "call 2")
    assert not errs, "\n".join(errs)


def test_radius_subset_in_distance_order(require_gpu, frames):
    cfg = global_map_config(search_radius=4.0)
    m, o = _both(cfg)
    _add(m, o, frames)
    pos = frames[20][0][:3] + np.float32(0.1)
    poses4 = np.array([np.append(f[0][:3], k) for k, f in enumerate(frames)], np.float32)
    ids = G.radius_sorted(poses4, pos, 4.0).tolist()
    assert 2 < len(ids) < len(frames) and set(ids) != set(range(len(ids))) and ids != sorted(ids)
    got, exp = m.global_map(pos, cfg), o.global_map(pos)
    assert got["report"]["n_in_radius"] == got["report"]["n_poses_used"] == len(ids)
    lead = next(k for k in ids if len(frames[k][1]))  # the nearest keyframe with corner points leads edge
    w = oracle_py.transform_keyframe(frames[lead][0], frames[lead][1])
    assert np.array_equal(_np(got["edge"])[:len(w)], w)
    m.close()
    errs = _errs(got, exp, "subset")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("kw,raw", [(dict(high_dense=1), (True, True)), (dict(first_call_raw=0), (False, False))])
def test_config_switches(require_gpu, frames, kw, raw):
    """high_dense: raw on every call. first_call_raw = 0: downsampled from call 1."""
    cfg = global_map_config(**kw)
    m, o = _both(cfg)
    _add(m, o, frames[:18])
    errs = []
    for call, want_raw in enumerate(raw, 1):
        got, exp = m.global_map(ORIGIN, cfg), o.global_map(ORIGIN)
        assert got["report"]["downsampled_cloud"] == got["report"]["downsampled_poses"] == (not want_raw)
        assert (got["report"]["n_global"] == got["report"]["n_global_raw"]) == want_raw
        errs += _errs(got, exp, f"{kw} call {call}")
    m.close()
    assert not errs, "\n".join(errs)


def test_overflow_passthrough(require_gpu):
    """Key positions over 2 km x 2 km x 300 m: at leaf 0.4 the extent product exceeds INT32_MAX and
    PCL returns the global cloud unchanged, on the downsampling call 2."""
    pos = [(0, 0, 0), (2000, 0, 0), (0, 2000, 0), (1000, 1000, 300), (600, 1400, 120), (1999, 1999, 299)]
    fr = _make_frames(13, pos)
    m, o = _both()
    _add(m, o, fr)
    raw = np.concatenate([c for w in o.world for c in w])
    assert G.extent_product(raw, 0.4) > G.INT32_MAX
    first, _ = m.global_map(ORIGIN), o.global_map(ORIGIN)
    got, exp = m.global_map(ORIGIN), o.global_map(ORIGIN)
    r = got["report"]
    assert (r["call"], r["downsampled_cloud"], r["passthrough"]) == (2, 1, 1)
    assert r["n_global"] == r["n_global_raw"] == len(raw) and first["report"]["passthrough"] == 0
    m.close()
    errs = _errs(got, exp, "overflow")
    assert not errs, "\n".join(errs)


def _call(m, pos, caps, want=(True, True, True), cfg=None):
    """llsr_map_global with explicit capacities; returns (rc, report, [global, edge, planar] arrays)."""
    import torch
    bufs = [torch.zeros((max(c, 1), 4), dtype=torch.float32, device="cuda") if w else None for c, w in zip(caps, want)]
    args = []
    for b, c in zip(bufs, caps):
        args += [C.c_void_p(b.data_ptr()), c] if b is not None else [None, 0]
    rep = _abi.GlobalMapReport()
    p = np.ascontiguousarray(pos, np.float32)
    torch.cuda.synchronize()
    rc = lib().llsr_map_global(m._m, C.byref(cfg) if cfg is not None else None, p.ctypes.data, *args, C.byref(rep), None)
    out = [b.cpu().numpy()[:n] if b is not None else None
           for b, n in zip(bufs, (rep.n_global, rep.n_edge, rep.n_planar))]
    return rc, rep, out


def test_capacity_refusal_and_retry(require_gpu, frames):
    """A too-small cap_global: LLSR_ERANGE with the sizes, the counter unchanged, and the retry bit
    equal to a map that was never refused — on the raw call 1 and on the downsampled call 2 (there
    the refusal comes after the VoxelGrid, with the exact size). The never-refused map passes NULL
    edge / planar on call 2: the global cloud is the same."""
    fr = frames[:20]
    a, b = LocalMap(0), LocalMap(0)
    for f in fr:
        a.add_keyframe(*f)
        b.add_keyframe(*f)
    big = sum(len(f[1]) + len(f[2]) + len(f[3]) for f in fr)
    rc, rep, _ = _call(a, ORIGIN, (big - 1, big, big))
    assert rc == _abi.LLSR_ERANGE and rep.call == 0
    assert (rep.n_global_raw, rep.n_global) == (big, big) and rep.n_edge == sum(len(f[1]) for f in fr)
    rc, rep, ga = _call(a, ORIGIN, (big, big, big))
    rcb, repb, gb = _call(b, ORIGIN, (big, big, big))
    assert rc == rcb == 0 and rep.call == repb.call == 1 and not rep.downsampled_cloud
    for x, y, name in zip(ga, gb, ("global", "edge", "planar")):
        assert not diff_report(name, x, y)
    rcb, repb, gb = _call(b, ORIGIN, (big, 0, 0), want=(True, False, False))
    assert rcb == 0 and repb.call == 2 and repb.downsampled_cloud and 0 < repb.n_global < big
    assert repb.n_edge > 0 and repb.n_planar > 0 and gb[1] is None  # skipped clouds: counts still reported
    rc, rep, _ = _call(a, ORIGIN, (repb.n_global - 1, big, big))
    assert rc == _abi.LLSR_ERANGE and rep.call == 1 and rep.n_global == repb.n_global
    assert (rep.n_edge, rep.n_planar, rep.n_global_raw) == (repb.n_edge, repb.n_planar, repb.n_global_raw)
    rc, rep, ga = _call(a, ORIGIN, (repb.n_global, big, big))
    assert rc == 0 and rep.call == 2
    assert not diff_report("global after refusal", ga[0], gb[0])
    a.close()
    b.close()


def test_empty_store_and_reset(require_gpu, frames):
    m, o = _both()
    got = m.global_map(ORIGIN)
    assert all(got["report"][k] == 0 for k in REPORT) and len(got["global"]) == len(got["edge"]) == 0
    errs = []
    for rnd in range(2):  # after llsr_map_reset the next call is a first call again
        _add(m, o, frames[:12])
        for call in (1, 2):
            got, exp = m.global_map(ORIGIN), o.global_map(ORIGIN)
            assert got["report"]["call"] == call and got["report"]["downsampled_cloud"] == (call == 2)
            errs += _errs(got, exp, f"round {rnd} call {call}")
        m.reset()
        o.reset()
    m.close()
    assert not errs, "\n".join(errs)


def test_save_map(require_gpu, frames):
    m, o = _both()
    c, s = m.save_map()
    assert len(c) == len(s) == 0
    _add(m, o, frames)
    c, s = m.save_map()
    rc, rs = o.save_map()
    assert len(rc) == sum(len(f[1]) for f in frames) and 0 < len(rs) < sum(len(f[2]) + len(f[3]) for f in frames)
    errs = [diff_report("cornerMap", _np(c), rc), diff_report("surfaceMap", _np(s), rs)]
    m.close()
    assert not any(errs), errs


def test_save_map_on_recorded_keyframes(require_gpu):
    """The 723 recorded keyframes (tests/_result_map.keyframes partitions the recorded maps, so the
    corner points are conserved): cornerMap has the recorded cornerMap.pcd's 84644 points."""
    z = R.load()
    m, o = _both()
    _add(m, o, R.keyframes(z))
    c, s = m.save_map()
    rc, rs = o.save_map()
    assert len(c) == len(z["corner_map"]) == 84644
    errs = [diff_report("cornerMap", _np(c), rc), diff_report("surfaceMap", _np(s), rs)]
    m.close()
    assert not any(errs), errs


def test_mapping_chain_global_map(require_gpu):
    """llsr_mapping_global_map / llsr_mapping_save_map of each slot equal llsr_map_global /
    llsr_map_save on a stand-alone map fed the slot's key poses and keyframe clouds (the oracle
    chain's, which tests/test_gpu_mapping.py holds the device chain to); one counter per slot."""
    import torch
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    seeds = (1, 65)
    pipe = Pipeline(cfg, max_batch=2, max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
    pipe.mapping_init(_abi.LLSR_MODE_LM_APPLIED)
    oras = [oracle_py.OracleMapping(cfg, _abi.LLSR_MODE_LM_APPLIED) for _ in seeds]
    stored = [[] for _ in seeds]
    for ora, keep in zip(oras, stored):
        ora.map.add_keyframe = (lambda add, keep: lambda *a: (keep.append(tuple(np.array(x, np.float32) for x in a)),
                                                              add(*a))[1])(ora.map.add_keyframe, keep)

    def step(k, with_oracle=True):
        scans = [synth.make_scan(s0 + k, "vlp16", motion=True) for s0 in seeds]
        off = np.zeros(len(scans) + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in scans])
        d_pts, d_off = torch.from_numpy(np.concatenate(scans)).cuda(), torch.from_numpy(off).cuda()
        torch.cuda.synchronize()
        pipe.mapping_batch(d_pts.data_ptr(), d_off.data_ptr(), len(scans))
        if with_oracle:
            for ora, s in zip(oras, scans):
                ora.process(s)

    for k in range(6):
        step(k)
    errs = []
    for b, calls in ((0, 2), (1, 1)):
        st = pipe.mapping_fetch(b)
        assert st["keyframes"] == len(stored[b]) == 5
        assert np.array_equal(pipe.mapping_keyposes(b), np.array([f[0] for f in stored[b]]))
        alone = LocalMap(0)
        for f in stored[b]:
            alone.add_keyframe(*f)
        for call in range(1, calls + 1):
            got, exp = pipe.mapping_global_map(b), alone.global_map(st["transform_aft_mapped"][3:6])
            assert got["report"]["call"] == call and got["report"]["downsampled_cloud"] == (call == 2)
            errs += _errs(got, {k: (_np(v) if k != "report" else v) for k, v in exp.items()}, f"slot {b} call {call}")
        (c, s), (rc, rs) = pipe.mapping_save_map(b), alone.save_map()
        errs += [e for e in (diff_report(f"slot {b} cornerMap", _np(c), _np(rc)),
                             diff_report(f"slot {b} surfaceMap", _np(s), _np(rs))) if e]
        alone.close()
    pipe.mapping_reset()
    assert pipe.mapping_global_map(0)["report"]["call"] == 0  # an empty store again
    for k in range(3):
        step(k, with_oracle=False)
    for b in (0, 1):
        r = pipe.mapping_global_map(b)["report"]
        assert (r["call"], r["downsampled_cloud"], r["n_in_radius"]) == (1, 0, 2)
    pipe.close()
    assert not errs, "\n".join(errs)
