"""GPU: adjustDistortion's IMU de-skew inside the feature stage (llsr_stage_imu, k_fa_points_imu)
against the numpy restatement of the reference's lines (tests/_imu.py), and an identity IMU against
the oracle end to end.

Bar: bit-exact. The device runs the per-point body of csrc/llsr_imu.h with the glibc-exact sinf /
cosf ports of llsr_libm.h; the restatement calls the host glibc. The restatement de-skews the
segmented cloud the device itself reports (seg_xyzi, orientation: the projection stage, which the
IMU does not touch and tests/test_gpu_parity.py ties to the oracle)."""
import numpy as np
import pytest

import _imu
import oracle_py
from _compare import compare
from _imu_cases import SCAN0_NS, bits_equal, window_streams
from llsr import ImuState, Pipeline, _abi, default_config, lib, synth

pytestmark = pytest.mark.gpu
F = np.float32
P_NS = 100_000_000


def stamp_of(ns):
    return int(ns) // 10 ** 9, int(ns) % 10 ** 9


def feed(state, queue, msgs):
    for m in msgs:
        state.callback(m["sec"], m["nanosec"], m["orientation"], m["angular_velocity"], m["linear_acceleration"])
        if queue is not None:
            queue.handler(m)


def upload(scans):
    import torch
    off = np.zeros(len(scans) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in scans])
    d_pts = torch.from_numpy(np.concatenate(scans) if off[-1] else np.zeros((1, 4), F)).cuda()
    d_off = torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    return d_pts, d_off


def identity_msgs(lo_ns, hi_ns):
    t = np.arange(lo_ns, hi_ns, 10_000_000, dtype=np.int64)
    m = np.zeros(len(t), synth.IMU_MSG_DTYPE)
    m["sec"], m["nanosec"] = t // 10 ** 9, t % 10 ** 9
    m["orientation"][:, 3] = 1.0
    m["linear_acceleration"][:, 2] = 9.81
    return m


class IdentityImu:
    """An IMU at rest with orientation (0, 0, 0, 1), 100 Hz: every angle the de-skew blends is 0, so
    every rotation is exact: x * 1 - y * 0 = x for a finite y unless x is -0 (-0 - -0 = +0, and the
    closing + imuShiftFromStart*Cur turns any -0 into +0). A +0 survives every step (+0 - +-0 = +0,
    +0 + +-0 = +0), and the generator's VLP-16 scans all hold a few: the column that looks straight
    ahead has sin(azimuth) = 0 exactly, so its y is +0. `exact_on` therefore checks on the CPU what
    exactness needs: no coordinate of the segmented cloud is -0, and the restatement's de-skew of it
    under this IMU equals the oracle's LOAM cloud bit for bit."""

    def __init__(self, period):
        self.state, self.queue, self.carry, self.ns = ImuState(period), _imu.Queue(period), _imu.zero_carry(), SCAN0_NS
        feed(self.state, self.queue, identity_msgs(self.ns - 50_000_000, self.ns))

    def next(self):
        feed(self.state, self.queue, identity_msgs(self.ns, self.ns + P_NS))
        st, w = stamp_of(self.ns), self.state.scan_window()
        self.ns += P_NS
        assert len(w) >= 10
        self.stamp = st
        return st, w

    def exact_on(self, o):
        """o: the oracle's result of the scan `next` was just called for."""
        xyz = np.asarray(o["seg_xyzi"], F)[:, :3]
        exp = self.queue.adjust_distortion(o["seg_xyzi"], o["orientation"], self.stamp, self.carry)
        return not ((xyz == 0) & np.signbit(xyz)).any() and bits_equal(exp, np.asarray(o["loam_xyzi"], F))


# ---- 1. identity IMU: the whole downstream of k_fa_points_imu against the oracle ----------------
@pytest.mark.parametrize("lidar,horizontal,seeds", [("vlp16", None, (1, 2, 70)), ("hdl64e", 2048, (5,))])
def test_identity_imu_scan_equals_oracle(require_gpu, lidar, horizontal, seeds):
    cfg = default_config(lidar, horizontal)
    pipe = Pipeline(cfg, max_points=2 * cfg.num_vertical_scans * cfg.num_horizontal_scans)
    ora, imu = oracle_py.Oracle(cfg), IdentityImu(cfg.scan_period)
    for s in seeds:
        pts = synth.make_scan(s, lidar)
        o = ora.process(pts)
        st, w = imu.next()
        assert imu.exact_on(o)
        pipe.stage_imu([st], [w])
        errs = compare(pipe.process_scan(pts), o)
        assert not errs, f"{lidar} seed {s}:\n  " + "\n  ".join(errs)
        rep = pipe.fetch_imu_report(0)
        assert all(not v.any() for v in rep.values())
    pipe.close()


def test_identity_imu_odometry_equals_oracle(require_gpu):
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    seeds = (1, 65)
    pipe = Pipeline(cfg, max_batch=len(seeds), max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
    oras, imus = [oracle_py.OracleOdometry(cfg) for _ in seeds], [IdentityImu(cfg.scan_period) for _ in seeds]
    for k in range(4):
        scans = [synth.make_scan(s0 + k, "vlp16", motion=True) for s0 in seeds]
        d_pts, d_off = upload(scans)
        sw = [imu.next() for imu in imus]
        assert all(imu.exact_on(oracle_py.Oracle(cfg).process(p)) for imu, p in zip(imus, scans))
        pipe.stage_imu([s for s, _ in sw], [w for _, w in sw])
        pipe.odometry_batch(d_pts.data_ptr(), d_off.data_ptr(), len(scans))
        for b, ora in enumerate(oras):
            g, o = pipe.odometry_fetch(b, clouds=True), ora.process(scans[b])
            assert g["frames"] == o["frames"]
            for key in ("transform_cur", "transform_sum"):
                assert bits_equal(g[key], o[key]), (k, b, key)
            for key in ("corner_last", "surf_last", "corner_scan", "surf_scan"):
                ref = o[key] if o[key] is not None else np.zeros((0, 4), F)
                assert bits_equal(np.asarray(g[key], F), np.asarray(ref, F)), (k, b, key)
    pipe.close()


def test_identity_imu_mapping_equals_oracle(require_gpu):
    cfg = default_config("vlp16")
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    seeds = (1, 65)
    pipe = Pipeline(cfg, max_batch=len(seeds), max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
    pipe.mapping_init(_abi.LLSR_MODE_LM_APPLIED)
    oras = [oracle_py.OracleMapping(cfg, _abi.LLSR_MODE_LM_APPLIED, pcl_voxel_order=True, loop_closure=False,
                                    search_num=50) for _ in seeds]
    imus = [IdentityImu(cfg.scan_period) for _ in seeds]
    for k in range(3):
        scans = [synth.make_scan(s0 + k, "vlp16", motion=True) for s0 in seeds]
        d_pts, d_off = upload(scans)
        sw = [imu.next() for imu in imus]
        assert all(imu.exact_on(oracle_py.Oracle(cfg).process(p)) for imu, p in zip(imus, scans))
        pipe.stage_imu([s for s, _ in sw], [w for _, w in sw])
        pipe.mapping_batch(d_pts.data_ptr(), d_off.data_ptr(), len(scans))
        for b, ora in enumerate(oras):
            o, g = ora.process(scans[b]), pipe.mapping_fetch(b)
            assert g["frames"] == o["frames"] and g["keyframes"] == len(ora.keyposes)
            if not o["step"]:
                continue
            for key in ("transform_sum", "transform_tobe_mapped", "transform_bef_mapped", "transform_aft_mapped"):
                assert bits_equal(g[key], o[key]), (k, b, key)
    for b, ora in enumerate(oras):
        assert bits_equal(pipe.mapping_keyposes(b), np.array(ora.keyposes, F).reshape(-1, 6))
    pipe.close()


# ---- 2 / 3. moving IMU and edge windows against the restatement ----------------------------------
def check_slot(tag, g, queue, carry, stamp, rep):
    """Slot result g (llsr_fetch_scan) and report against the restatement's adjustDistortion of the
    same segmented cloud; advances `queue` / `carry`. Returns the restated cloud."""
    S = g["n_segmented"]
    exp = queue.adjust_distortion(g["seg_xyzi"], g["orientation"], stamp, carry)
    got = np.asarray(g["loam_xyzi"], F)
    assert bits_equal(got, exp), (tag, "loam_xyzi", np.argwhere((got.view(np.uint32) != exp.view(np.uint32)).any(axis=1))[:5].ravel())
    for m in _imu.MEMBERS:
        assert bits_equal(rep[m], np.asarray(carry[m], F)), (tag, m, rep[m], carry[m])
    if S > 10:  # FA:817-848 on the restated cloud: a halo point left raw would show at a tile boundary
        cv = _imu.curvature(exp)
        assert bits_equal(np.asarray(g["curvature"], F)[5:S - 5], cv[5:S - 5]), (tag, "curvature")
    return exp


@pytest.mark.parametrize("rate_hz", [100, 500])
def test_moving_imu_three_batches(require_gpu, rate_hz):
    """B = 3, three consecutive batches on one handle: slot 0 has a window in every batch, slot 1 never
    (it must equal a run with nothing staged), slot 2's IMU starts one frame late."""
    cfg = default_config("vlp16")
    seeds = (1, 65, 130)
    HW = cfg.num_vertical_scans * cfg.num_horizontal_scans
    pipe = Pipeline(cfg, max_batch=3, max_points=HW)
    plain = Pipeline(cfg, max_batch=3, max_points=HW)
    # slot 2's first message is stamped (and arrives) one frame late
    streams = {0: synth.imu_stream(seeds[0], rate_hz, 3), 2: synth.imu_stream(seeds[2] + 1, rate_hz, 2, lead=0.0)}
    states = {b: ImuState(cfg.scan_period) for b in (0, 2)}
    queues = {b: _imu.Queue(cfg.scan_period) for b in (0, 2)}
    carries = {b: _imu.zero_carry() for b in (0, 2)}
    fed = {0: 0, 2: 0}
    rotated = 0
    for k in range(3):
        scans = [synth.make_scan(s0 + k, "vlp16", motion=True) for s0 in seeds]
        stamps = [synth.scan_stamp(s0 + k) for s0 in seeds]
        windows = [None, None, None]
        for b in (0, 2):
            # the messages stamped up to the scan's end have arrived (slot 2, batch 0: none yet, the
            # window is empty and the scan takes the plain path on both sides)
            end = (stamps[b][0] * 10 ** 9 + stamps[b][1]) + P_NS
            t = streams[b]["sec"].astype(np.int64) * 10 ** 9 + streams[b]["nanosec"]
            upto = int(np.searchsorted(t, end))
            feed(states[b], queues[b], streams[b][fed[b]:upto])
            fed[b] = upto
            windows[b] = states[b].scan_window()
            assert len(windows[b]) > (6 if rate_hz == 100 else 30) or (b == 2 and k == 0 and len(windows[b]) == 0)
        d_pts, d_off = upload(scans)
        pipe.stage_imu(stamps, windows)
        pipe.process_batch(d_pts.data_ptr(), d_off.data_ptr(), 3)
        plain.process_batch(d_pts.data_ptr(), d_off.data_ptr(), 3)
        errs = compare(pipe.fetch(1), plain.fetch(1))
        assert not errs, f"batch {k} slot 1:\n  " + "\n  ".join(errs)
        for b in (0, 2):
            g = {key: np.copy(v) if isinstance(v, np.ndarray) else v for key, v in pipe.fetch(b).items()}
            assert g["n_segmented"] > 16 * 1012  # 17 tiles of k_fa_points
            rep = pipe.fetch_imu_report(b)
            if len(windows[b]) == 0:
                queues[b].adjust_distortion(g["seg_xyzi"], g["orientation"], stamps[b], carries[b])
                assert all(not v.any() for v in rep.values())
                assert bits_equal(np.asarray(g["loam_xyzi"], F), np.asarray(plain.fetch(b)["loam_xyzi"], F))
                continue
            exp = check_slot(f"{rate_hz} Hz batch {k} slot {b}", g, queues[b], carries[b], stamps[b], rep)
            rotated += int((exp[:, :3] != _imu.loam_swap(g["seg_xyzi"], g["orientation"], cfg.scan_period)[0][:, :3]).any())
    assert rotated == 5  # every staged scan really was rotated
    pipe.close()
    plain.close()


def small_scans():
    """A scan whose segmented cloud has 40 points (the first 8 columns of a generated scan, one
    return dropped) and one without any point."""
    p = synth.make_scan(3, "vlp16")
    p[8 * 16:] = np.nan
    p[4] = np.nan
    return p, np.full_like(p, np.nan)


def test_edge_windows(require_gpu):
    """The edge windows of the host test (tests/_imu_cases.py), one per slot, three consecutive
    batches; then the same windows over a 40-point scan and an empty scan."""
    cfg = default_config("vlp16")
    streams = window_streams()
    names = sorted(streams)
    B = len(names)
    HW = cfg.num_vertical_scans * cfg.num_horizontal_scans
    pipe = Pipeline(cfg, max_batch=B, max_points=HW)
    states = [ImuState(cfg.scan_period) for _ in names]
    queues = [_imu.Queue(cfg.scan_period) for _ in names]
    carries = [_imu.zero_carry() for _ in names]
    small, empty = small_scans()
    base = [synth.make_scan(1, "vlp16"), synth.make_scan(2, "vlp16"), small]
    sizes = []
    for k in range(3):
        scans = [base[k] if names[b] != "100hz" or k < 2 else empty for b in range(B)]
        stamp = stamp_of(SCAN0_NS + k * P_NS)
        windows = []
        for b, name in enumerate(names):
            feed(states[b], queues[b], streams[name][k])
            windows.append(states[b].scan_window())
        d_pts, d_off = upload(scans)
        pipe.stage_imu([stamp] * B, windows)
        pipe.process_batch(d_pts.data_ptr(), d_off.data_ptr(), B)
        for b, name in enumerate(names):
            g = {key: np.copy(v) if isinstance(v, np.ndarray) else v for key, v in pipe.fetch(b).items()}
            sizes.append(g["n_segmented"])
            check_slot(f"{name} batch {k}", g, queues[b], carries[b], stamp, pipe.fetch_imu_report(b))
    assert 40 in sizes and 0 in sizes and max(sizes) > 16 * 1012
    pipe.close()


# ---- 4. handle state -------------------------------------------------------------------------
def test_handle_state(require_gpu):
    cfg = default_config("vlp16")
    HW = cfg.num_vertical_scans * cfg.num_horizontal_scans
    pts = [synth.make_scan(s, "vlp16", motion=True) for s in (1, 2)]
    stream = synth.imu_stream(1, 100, 2)
    state = ImuState(cfg.scan_period)
    feed(state, None, stream)
    window = state.scan_window()
    stamp = synth.scan_stamp(1)
    pipe = Pipeline(cfg, max_batch=2, max_points=HW)
    fresh = Pipeline(cfg, max_batch=2, max_points=HW)
    d1, o1 = upload(pts[:1])
    d2, o2 = upload(pts[1:])
    d12, o12 = upload(pts)

    # a B mismatch is refused and leaves the staging in place
    pipe.stage_imu([stamp], [window])
    rc = lib().llsr_process_batch(pipe._h, d12.data_ptr(), o12.data_ptr(), 2, None)
    assert rc == -22  # LLSR_EINVAL
    pipe.process_batch(d1.data_ptr(), o1.data_ptr(), 1)
    staged = {k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in pipe.fetch(0).items()}
    rep1 = pipe.fetch_imu_report(0)
    assert any(v.any() for v in rep1.values())
    fresh.process_batch(d1.data_ptr(), o1.data_ptr(), 1)
    unstaged = {k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in fresh.fetch(0).items()}
    assert not bits_equal(staged["loam_xyzi"], unstaged["loam_xyzi"])

    # the staging does not stick: the next batch takes the plain path (its de-skew inputs do not
    # depend on the carried FA arrays)
    pipe.process_batch(d2.data_ptr(), o2.data_ptr(), 1)
    fresh.process_batch(d2.data_ptr(), o2.data_ptr(), 1)
    a, b = pipe.fetch(0), fresh.fetch(0)
    assert bits_equal(np.asarray(a["loam_xyzi"], F), np.asarray(b["loam_xyzi"], F))
    assert bits_equal(np.asarray(a["curvature"], F), np.asarray(b["curvature"], F))
    rep2 = pipe.fetch_imu_report(0)
    assert all(bits_equal(rep2[m], rep1[m]) for m in rep1)  # a scan without window reports the carried members

    # after llsr_reset_state the carry is zero again, and an unstaged batch equals a fresh handle's
    pipe.reset()
    assert all(not v.any() for v in pipe.fetch_imu_report(0).values())
    fresh2 = Pipeline(cfg, max_batch=2, max_points=HW)
    pipe.process_batch(d2.data_ptr(), o2.data_ptr(), 1)
    fresh2.process_batch(d2.data_ptr(), o2.data_ptr(), 1)
    errs = compare(pipe.fetch(0), fresh2.fetch(0))
    assert not errs, "\n  ".join(errs)
    # ... and the same staged scan reports what it did the first time (angular_from_start = Cur - 0)
    pipe.reset()
    pipe.stage_imu([stamp], [window])
    pipe.process_batch(d1.data_ptr(), o1.data_ptr(), 1)
    rep3 = pipe.fetch_imu_report(0)
    assert all(bits_equal(rep3[m], rep1[m]) for m in rep1)
    for p in (pipe, fresh, fresh2):
        p.close()
