"""GPU: the use_imu_undistortion == true branches of the scan-to-scan odometry
(llsr_set_imu_undistortion; k_odo_inputs_imu / k_odo_finish_imu) against the numpy restatement of the
reference's lines (tests/_imu_undistortion.py), and an identity IMU against the oracle.

Bar: bit-exact (numerically equal where an identity IMU meets the oracle: a signed zero may differ).
The restatement's chain is fed with the feature outputs and the IMU report the device itself returns
for the slot after the batch (the feature stage and the de-skew are tied to the oracle and to
tests/_imu.py by tests/test_gpu_parity.py and tests/test_gpu_imu.py), and runs the oracle's
scan-to-scan LM, the Python updateInitialGuess, and the restated integrateTransformation /
TransformToEnd in the reference's order."""
import functools

import numpy as np
import pytest

import _imu
import _imu_undistortion as R
import _odom_guess
import oracle_py
from _imu_cases import SCAN0_NS, bits_equal
from llsr import ImuState, Pipeline, _abi, default_config, synth

pytestmark = pytest.mark.gpu
F = np.float32
P_NS = 100_000_000
CLOUDS = ("corner_last", "surf_last", "corner_scan", "surf_scan")
LM_KEYS = ("surf_iterations", "corner_iterations", "n_surf_corr", "n_corner_corr", "degenerate")


def _cfg(lidar="vlp16"):
    cfg = default_config(lidar, 2048 if lidar == "hdl64e" else None)
    cfg.mode = _abi.LLSR_MODE_LM_APPLIED
    return cfg


@functools.lru_cache(maxsize=None)
def _scan(seed, lidar="vlp16"):
    return synth.make_scan(seed, lidar, motion=True)


@functools.lru_cache(maxsize=None)
def _oracle_chain(seed0, frames):
    """oracle_py.OracleOdometry over a drive, computed once and shared (read-only)."""
    ora = oracle_py.OracleOdometry(_cfg())
    return [ora.process(_scan(seed0 + k)) for k in range(frames)]


def _upload(scans):
    import torch
    off = np.zeros(len(scans) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in scans])
    d_pts = torch.from_numpy(np.concatenate(scans)).cuda()
    d_off = torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    return d_pts, d_off


def _feed(state, msgs):
    for m in msgs:
        state.callback(m["sec"], m["nanosec"], m["orientation"], m["angular_velocity"], m["linear_acceleration"])


class MovingImu:
    """synth.imu_stream at 100 Hz for a drive starting at frame `seed`; window(stamp) feeds the messages
    stamped up to the scan's end and takes the scan's window."""

    def __init__(self, cfg, seed, frames, lead=0.05):
        self.stream = synth.imu_stream(seed, 100, frames, lead=lead)
        self.t = self.stream["sec"].astype(np.int64) * 10 ** 9 + self.stream["nanosec"]
        self.state, self.fed = ImuState(cfg.scan_period), 0

    def window(self, stamp):
        upto = int(np.searchsorted(self.t, stamp[0] * 10 ** 9 + stamp[1] + P_NS))
        _feed(self.state, self.stream[self.fed:upto])
        self.fed = upto
        return self.state.scan_window()


def _identity_msgs(lo_ns, hi_ns):
    t = np.arange(lo_ns, hi_ns, 10_000_000, dtype=np.int64)
    m = np.zeros(len(t), synth.IMU_MSG_DTYPE)
    m["sec"], m["nanosec"] = t // 10 ** 9, t % 10 ** 9
    m["orientation"][:, 3] = 1.0
    m["linear_acceleration"][:, 2] = 9.81
    return m


class IdentityImu:
    """An IMU at rest with orientation (0, 0, 0, 1), 100 Hz (as tests/test_gpu_imu.py's): every angle
    is 0 and every rotation x * 1 - y * 0. `exact_on` checks on the CPU that the de-skew of the oracle's
    segmented cloud under this IMU is the oracle's LOAM cloud bit for bit (no -0 coordinate)."""

    def __init__(self, period):
        self.state, self.queue, self.carry, self.ns = ImuState(period), _imu.Queue(period), _imu.zero_carry(), SCAN0_NS
        self._feed(_identity_msgs(self.ns - 50_000_000, self.ns))

    def _feed(self, msgs):
        _feed(self.state, msgs)
        for m in msgs:
            self.queue.handler(m)

    def next(self):
        self._feed(_identity_msgs(self.ns, self.ns + P_NS))
        self.stamp = (int(self.ns) // 10 ** 9, int(self.ns) % 10 ** 9)
        self.ns += P_NS
        return self.stamp, self.state.scan_window()

    def exact_on(self, o):
        xyz = np.asarray(o["seg_xyzi"], F)[:, :3]
        exp = self.queue.adjust_distortion(o["seg_xyzi"], o["orientation"], self.stamp, self.carry)
        return not ((xyz == 0) & np.signbit(xyz)).any() and bits_equal(exp, np.asarray(o["loam_xyzi"], F))


def _copy(d):
    return {k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in d.items()}


def _compare_slot(g, g_lm, o, tag, errs):
    if g["frames"] != o["frames"]:
        errs.append(f"{tag}: frames {g['frames']} vs {o['frames']}")
    skipped = o["lm"] is None or o["lm"]["skipped"] == 1  # first scan, or last clouds too small (FA:2506)
    if (g["lm"]["skipped"] == 1) != skipped:
        errs.append(f"{tag}: skipped {g['lm']['skipped']} vs expected {skipped}")
    elif not skipped:
        for key in LM_KEYS:
            if g["lm"][key] != o["lm"][key]:
                errs.append(f"{tag}: lm {key} {g['lm'][key]} vs {o['lm'][key]}")
    g = dict(g, transform_lm=g_lm)
    for key in ("transform_cur", "transform_sum", "transform_lm"):
        if not bits_equal(g[key], o[key]):
            errs.append(f"{tag}: {key} {g[key]} vs {o[key]} (max |d| {np.abs(g[key] - o[key]).max():.3g})")
    for key in CLOUDS:
        ref = np.asarray(o[key] if o[key] is not None else np.zeros((0, 4), F), F)
        if g[key].shape != ref.shape:
            errs.append(f"{tag}: {key} shape {g[key].shape} vs {ref.shape}")
        elif not bits_equal(g[key], ref):
            errs.append(f"{tag}: {key} max |d| {np.abs(g[key] - ref).max():.3g}")


# ---- 1. identity IMU against the oracle ----------------------------------------------------------
def test_identity_imu_switch_on_equals_oracle(require_gpu):
    cfg = _cfg()
    seeds, frames = (1, 65), 4
    # on the CPU first: the restatement's chain over the oracle's features under a zero report gives
    # the oracle chain's transformCur and clouds numerically (the exact_on pattern)
    for s0 in seeds:
        chain = R.ImuOdometryChain(cfg)
        for k, o in enumerate(_oracle_chain(s0, frames)):
            e = chain.process(o["features"], R.ZERO_REPORT)
            assert np.array_equal(e["transform_cur"], o["transform_cur"]), (s0, k)
            for key in CLOUDS:
                assert (e[key] is None and o[key] is None) or np.array_equal(e[key], o[key]), (s0, k, key)
    pipe = Pipeline(cfg, max_batch=len(seeds), max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
    pipe.set_imu_undistortion(True)
    imus = [IdentityImu(cfg.scan_period) for _ in seeds]
    chains = [R.ImuOdometryChain(cfg) for _ in seeds]
    for k in range(frames):
        scans = [_scan(s0 + k) for s0 in seeds]
        d_pts, d_off = _upload(scans)
        sw = [imu.next() for imu in imus]
        assert all(imu.exact_on(_oracle_chain(s0, frames)[k]["features"]) for imu, s0 in zip(imus, seeds))
        pipe.stage_imu([s for s, _ in sw], [w for _, w in sw])
        pipe.odometry_batch(d_pts.data_ptr(), d_off.data_ptr(), len(scans))
        for b, s0 in enumerate(seeds):
            g, o = pipe.odometry_fetch(b, clouds=True), _oracle_chain(s0, frames)[k]
            assert all(not v.any() for v in pipe.fetch_imu_report(b).values())
            e = chains[b].process(o["features"], R.ZERO_REPORT)
            assert g["frames"] == o["frames"]
            assert np.array_equal(g["transform_cur"], o["transform_cur"]), (k, b)
            for key in CLOUDS:
                ref = o[key] if o[key] is not None else np.zeros((0, 4), F)
                assert np.array_equal(g[key], np.asarray(ref, F)), (k, b, key)
            assert bits_equal(g["transform_sum"], e["transform_sum"]), (k, b, g["transform_sum"], e["transform_sum"])
    pipe.close()


# ---- 2 / 7. moving IMU against the restatement's chain ---------------------------------------------
def _moving_drive(lidar, seeds, frames, flags, imu_from, switch=True):
    """One handle, `frames` batches of llsr_odometry_batch_odom. imu_from[b]: the first frame slot b's
    IMU delivers messages for (None: never staged). Returns per frame and slot (g, g_lm, features,
    report) copies."""
    cfg = _cfg(lidar)
    pipe = Pipeline(cfg, max_batch=len(seeds), max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
    pipe.set_imu_undistortion(switch)
    imus = [None if f is None else MovingImu(cfg, s0 + f, frames - f, lead=0.05 if f == 0 else 0.0)
            for s0, f in zip(seeds, imu_from)]
    samples = [_odom_guess.drive_samples(s0, frames) for s0 in seeds]
    out = []
    for k in range(frames):
        d_pts, d_off = _upload([_scan(s0 + k, lidar) for s0 in seeds])
        stamps = [synth.scan_stamp(s0 + k) for s0 in seeds]
        windows = [None if imu is None else imu.window(st) for imu, st in zip(imus, stamps)]
        for b, f in enumerate(imu_from):
            assert f is None or (len(windows[b]) > 6) == (k >= f), (b, k, len(windows[b]))
        pipe.stage_imu(stamps, windows)
        pipe.odometry_batch_odom(d_pts.data_ptr(), d_off.data_ptr(), len(seeds), [s[k] for s in samples], flags)
        out.append([(pipe.odometry_fetch(b, clouds=True), pipe.odometry_fetch_lm(b), _copy(pipe.fetch(b)),
                     pipe.fetch_imu_report(b)) for b in range(len(seeds))])
    pipe.close()
    return out, samples


def _check_drive(lidar, seeds, frames, flags, out, samples):
    cfg = _cfg(lidar)
    errs, moved = [], 0
    chains = [R.ImuOdometryChain(cfg) for _ in seeds]
    for k in range(frames):
        for b in range(len(seeds)):
            g, g_lm, feat, rep = out[k][b]
            e = chains[b].process(feat, rep, samples[b][k] if flags[b] else None)
            _compare_slot(g, g_lm, e, f"{lidar} slot {b} frame {k}", errs)
            if k >= 1 and rep["cur"].any():
                less_sharp = np.asarray(feat["loam_xyzi"], F)[feat["less_sharp_ind"]]
                moved += int(not np.array_equal(g["corner_last"], oracle_py.transform_to_end(g["transform_cur"], less_sharp)))
    assert not errs, "\n".join(errs)
    return moved


def test_moving_imu_three_slots(require_gpu):
    """B = 3, four frames, one launch per frame: slot 0 flagged and staged every frame, slot 1
    unflagged and never staged, slot 2 flagged with its IMU starting one frame late."""
    seeds, frames, flags, imu_from = (1, 65, 130), 4, [1, 0, 1], [0, None, 1]
    out, samples = _moving_drive("vlp16", seeds, frames, flags, imu_from)
    assert all(not v.any() for v in out[-1][1][3].values())       # slot 1 never had a report
    assert all(not v.any() for v in out[0][2][3].values()) and out[1][2][3]["start"].any()
    moved = _check_drive("vlp16", seeds, frames, flags, out, samples)
    assert moved >= 3  # the tail really moved the staged slots' last clouds
    # the pre-LM guess really was the LM's start: with the switch off the LM of frame 1 starts from the
    # carried transformCur (zero) and ends elsewhere
    off, _ = _moving_drive("vlp16", seeds, 2, flags, imu_from, switch=False)
    assert out[1][0][1].any() and off[1][0][1].any()
    assert not np.array_equal(out[1][0][1], off[1][0][1]) or out[1][0][0]["lm"] != off[1][0][0]["lm"]
    # ... while the unflagged, unstaged slot 1 of frame 1 does not see the switch at all
    assert bits_equal(out[1][1][0]["transform_cur"], off[1][1][0]["transform_cur"])


def test_moving_imu_hdl64e(require_gpu):
    """HDL-64E, 2048 columns, B = 1, three frames: a flagged, staged slot."""
    out, samples = _moving_drive("hdl64e", (5,), 3, [1], [0])
    assert _check_drive("hdl64e", (5,), 3, [1], out, samples) >= 2


# ---- 3. the switch goes off again -------------------------------------------------------------------
def _plain_frames(pipe, seeds, frames):
    res = []
    for k in range(frames):
        d_pts, d_off = _upload([_scan(s0 + k) for s0 in seeds])
        pipe.odometry_batch(d_pts.data_ptr(), d_off.data_ptr(), len(seeds))
        res.append([pipe.odometry_fetch(b, clouds=True) for b in range(len(seeds))])
    return res


def test_switch_off_equals_fresh_handle(require_gpu):
    cfg = _cfg()
    seeds, frames = (1, 65), 3
    HW = cfg.num_vertical_scans * cfg.num_horizontal_scans
    pipe, fresh = Pipeline(cfg, max_batch=2, max_points=HW), Pipeline(cfg, max_batch=2, max_points=HW)
    pipe.set_imu_undistortion(True)
    imus = [MovingImu(cfg, s0, 2) for s0 in seeds]
    for k in range(2):
        d_pts, d_off = _upload([_scan(s0 + k) for s0 in seeds])
        stamps = [synth.scan_stamp(s0 + k) for s0 in seeds]
        pipe.stage_imu(stamps, [imu.window(st) for imu, st in zip(imus, stamps)])
        pipe.odometry_batch(d_pts.data_ptr(), d_off.data_ptr(), 2)
    assert pipe.odometry_fetch(0)["transform_sum"][[0, 2]].any()
    pipe.set_imu_undistortion(False)
    pipe.odometry_reset()
    a, f = _plain_frames(pipe, seeds, frames), _plain_frames(fresh, seeds, frames)
    for k in range(frames):
        for b, s0 in enumerate(seeds):
            o = _oracle_chain(s0, 4)[k]
            assert a[k][b]["frames"] == f[k][b]["frames"] == o["frames"]
            for key in ("transform_cur", "transform_sum") + CLOUDS:
                assert bits_equal(a[k][b][key], f[k][b][key]), (k, b, key)
                ref = o[key] if o[key] is not None else np.zeros((0, 4), F)
                assert bits_equal(f[k][b][key], np.asarray(ref, F)), (k, b, key, "oracle")
    pipe.close()
    fresh.close()


# ---- 4. small clouds ----------------------------------------------------------------------------
def _small_scans():
    """A scan whose segmented cloud has 40 points (the first 8 columns of a generated scan, one
    return dropped) and one without any point (as tests/test_gpu_imu.py's)."""
    p = synth.make_scan(3, "vlp16")
    p[8 * 16:] = np.nan
    p[4] = np.nan
    return p, np.full_like(p, np.nan)


def test_small_and_empty_scans(require_gpu):
    cfg = _cfg()
    small, empty = _small_scans()
    scans = [_scan(1), _scan(2), small, empty]
    pipe = Pipeline(cfg, max_batch=1, max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
    pipe.set_imu_undistortion(True)
    imu, chain = MovingImu(cfg, 1, 4), R.ImuOdometryChain(cfg)
    samples = _odom_guess.drive_samples(1, 4)
    errs, sizes = [], []
    for k, p in enumerate(scans):
        d_pts, d_off = _upload([p])
        stamp = synth.scan_stamp(1 + k)
        pipe.stage_imu([stamp], [imu.window(stamp)])
        pipe.odometry_batch_odom(d_pts.data_ptr(), d_off.data_ptr(), 1, [samples[k]])
        g, feat, rep = pipe.odometry_fetch(0, clouds=True), _copy(pipe.fetch(0)), pipe.fetch_imu_report(0)
        sizes.append(feat["n_segmented"])
        before = chain.tsum.copy()
        e = chain.process(feat, rep, samples[k])
        _compare_slot(g, pipe.odometry_fetch_lm(0), e, f"frame {k}", errs)
        if k >= 2:  # no feature, and integrateTransformation still ran
            assert feat["n_sharp"] == 0 and feat["n_less_sharp"] == 0 and g["n_corner_last"] == 0
            assert not bits_equal(g["transform_sum"], before)
    assert sizes[2:] == [40, 0]
    assert not errs, "\n".join(errs)
    pipe.close()


# ---- 5. partial batch and reset: the first-scan add happens once per start ------------------------
def test_first_scan_add_once_per_start(require_gpu):
    cfg = _cfg()
    seeds = (1, 65, 130)
    pipe = Pipeline(cfg, max_batch=3, max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
    pipe.set_imu_undistortion(True)
    for run in range(2):
        imus = [MovingImu(cfg, seeds[0], 3), MovingImu(cfg, seeds[1], 3), MovingImu(cfg, seeds[2] + 1, 2)]
        chains = [R.ImuOdometryChain(cfg) for _ in seeds]
        errs = []
        for k, B in enumerate((2, 3, 2)):  # slot 2's first scan arrives in the second batch
            d_pts, d_off = _upload([_scan(s0 + k) for s0 in seeds[:B]])
            stamps = [synth.scan_stamp(s0 + k) for s0 in seeds[:B]]
            pipe.stage_imu(stamps, [imu.window(st) for imu, st in zip(imus[:B], stamps)])
            pipe.odometry_batch(d_pts.data_ptr(), d_off.data_ptr(), B)
            for b in range(B):
                g, rep = pipe.odometry_fetch(b, clouds=True), pipe.fetch_imu_report(b)
                e = chains[b].process(_copy(pipe.fetch(b)), rep)
                _compare_slot(g, np.zeros(6, F), e, f"run {run} batch {k} slot {b}", errs)
                if e["frames"] == 1:  # the add, once: transformSum = (imuPitchStart, 0, imuRollStart, 0, 0, 0)
                    want = np.array([rep["start"][1], 0, rep["start"][0], 0, 0, 0], F)
                    assert bits_equal(g["transform_sum"], want) and want.any(), (run, k, b)
            g2 = pipe.odometry_fetch(2)
            assert g2["frames"] == (0 if k == 0 else 1)
            if k == 2:  # slot 2 sat out the third batch: its sum is still the one add
                assert np.count_nonzero(g2["transform_sum"]) <= 2 and g2["transform_sum"].any()
        assert not errs, "\n".join(errs)
        pipe.odometry_reset()
        assert not pipe.odometry_fetch(0)["transform_sum"].any()
        assert all(not v.any() for v in pipe.fetch_imu_report(0).values())
    pipe.close()


# ---- 6. the mapping chain -------------------------------------------------------------------------
class _FedOdometry:
    """OracleMapping's odometry: the restatement's chain over what the device returned for the scan."""

    def __init__(self, cfg):
        self.chain = R.ImuOdometryChain(cfg)
        self.features = self.report = self.sample = None

    def process(self, xyzi):
        return self.chain.process(self.features, self.report, self.sample)


def test_mapping_chain_switch_on(require_gpu):
    cfg = _cfg()
    seeds, frames = (1, 65), 3
    pipe = Pipeline(cfg, max_batch=2, max_points=cfg.num_vertical_scans * cfg.num_horizontal_scans)
    pipe.set_imu_undistortion(True)
    pipe.mapping_init(_abi.LLSR_MODE_LM_APPLIED)
    oras = []
    for _ in seeds:
        m = oracle_py.OracleMapping(cfg, _abi.LLSR_MODE_LM_APPLIED, loop_closure=False)
        m.odo = _FedOdometry(cfg)
        oras.append(m)
    imus = [MovingImu(cfg, s0, frames) for s0 in seeds]
    samples = [_odom_guess.drive_samples(s0, frames) for s0 in seeds]
    errs = []
    for k in range(frames):
        d_pts, d_off = _upload([_scan(s0 + k) for s0 in seeds])
        stamps = [synth.scan_stamp(s0 + k) for s0 in seeds]
        pipe.stage_imu(stamps, [imu.window(st) for imu, st in zip(imus, stamps)])
        pipe.mapping_batch_odom(d_pts.data_ptr(), d_off.data_ptr(), 2, [s[k] for s in samples])
        for b, ora in enumerate(oras):
            ora.odo.features, ora.odo.report, ora.odo.sample = _copy(pipe.fetch(b)), pipe.fetch_imu_report(b), samples[b][k]
            o, g, go = ora.process(None), pipe.mapping_fetch(b), pipe.odometry_fetch(b)
            tag = f"slot {b} frame {k}"
            if g["frames"] != o["frames"] or g["keyframes"] != len(ora.keyposes):
                errs.append(f"{tag}: frames / keyframes {g['frames']} / {g['keyframes']} vs {o['frames']} / {len(ora.keyposes)}")
            for key in ("transform_cur", "transform_sum"):
                if not bits_equal(go[key], o["odo"][key]):
                    errs.append(f"{tag}: odometry {key} {go[key]} vs {o['odo'][key]}")
            if not o["step"]:
                continue
            for key in ("transform_sum", "transform_tobe_mapped", "transform_bef_mapped", "transform_aft_mapped"):
                if not bits_equal(g[key], o[key]):
                    errs.append(f"{tag}: {key} {g[key]} vs {o[key]}")
    for b, ora in enumerate(oras):
        kg, ko = pipe.mapping_keyposes(b), np.array(ora.keyposes, F).reshape(-1, 6)
        if not bits_equal(kg, ko):
            errs.append(f"slot {b}: keyposes {kg.shape} vs {ko.shape}")
    assert all(len(ora.keyposes) == frames - 1 for ora in oras)
    pipe.close()
    assert not errs, "\n".join(errs)
