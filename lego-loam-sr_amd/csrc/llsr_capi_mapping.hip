// llsr_capi_mapping.hip — C-ABI host side of the mapping chain (MapOptimization::run, MO:1854-1896):
// the odometry batch, then per slot the pose glue on the host (llsr_mapping.h) around batched
// device work — adjustOutlierCloud, one segmented VoxelGrid for every slot's
// downsampleCurrentScan, the slots' local maps, and one scan-to-map batch over all slots.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "llsr_handle.h"
#include "llsr_icp.h"
#include "llsr_pg.h"
#include "llsr_prior_internal.h"

namespace llsr {
// adjustOutlierCloud (FA:2600-2610): the IP outlier cloud of slot b (d.outl, [B][HW]) with
// x, y, z <- y, z, x, packed at off[b].
__global__ void k_mapping_outliers(const float4* outl, int HW, const int64_t* off, float4* out) {
  const int b = blockIdx.y;
  const int64_t o0 = off[b], n = off[b + 1] - o0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = outl[(size_t)b * HW + i];
    out[o0 + i] = make_float4(p.y, p.z, p.x, p.w);
  }
}
}  // namespace llsr

using namespace llsr;

// Grow a device point buffer to hold `need` points, keeping its first `keep` points.
static int32_t mp_grow(llsr_handle* h, GrowBuf& buf, size_t need, size_t keep, hipStream_t s) {
  if (need <= buf.cap && buf.mem) return LLSR_OK;
  size_t n = buf.cap ? buf.cap : (size_t)1 << 16;
  while (n < need) n *= 2;
  llsr_host::DevMem q;
  if (llsr_host::alloc(q, n * sizeof(float4)) != hipSuccess) return fail(h, LLSR_ENOMEM, "mapping buffers");
  if (buf.mem && keep) HIP_OK(h, hipMemcpyAsync(q, buf.mem, keep * sizeof(float4), hipMemcpyDeviceToDevice, s));
  HIP_OK(h, sync_handle_streams(h));
  HIP_OK(h, hipStreamSynchronize(s));
  buf.mem = std::move(q);  // frees the old buffer
  buf.cap = n;
  return LLSR_OK;
}

extern "C" int32_t llsr_mapping_reset(llsr_handle* h) {
  if (!h) return LLSR_EINVAL;
  auto& mp = h->mp;
  if (!mp.live) return fail(h, LLSR_EINVAL, "llsr_mapping_init not called");
  int32_t rc = llsr_odometry_reset(h);
  if (rc != LLSR_OK) return rc;
  for (auto& sl : mp.slot) {
    llsr_map* m = sl.map;
    if (llsr_map_reset(m) != LLSR_OK) return fail(h, LLSR_EINVAL, "llsr_map_reset");
    sl = llsr_handle::MapSlot{};  // (its `now` too: NaN again)
    sl.map = m;
  }
  mp.times.clear();
  mp.times_staged = false;
  mp.fresh = true;  // (the attached prior map stays)
  if (mp.pg) llsr_pg_reset(mp.pg, -1);
  const int B = (int)mp.slot.size();
  HIP_OK(h, hipMemset(mp.sm.d_deg, 0, sizeof(int) * B));      // isDegenerate = false (MO:285)
  HIP_OK(h, hipMemset(mp.sm.d_matP, 0, sizeof(float) * 36 * B));  // matP zeroed (MO:286)
  return LLSR_OK;
}

// (the point buffers outl / ds / tot / cmap stay: a later init reuses them)
void mapping_free(llsr_handle* h) {
  auto& mp = h->mp;
  for (auto& sl : mp.slot)
    if (sl.map) llsr_map_destroy(sl.map);
  mp.slot.clear();
  if (mp.vg) llsr_map_destroy(mp.vg);
  mp.vg = nullptr;
  if (mp.icp) llsr_icp_destroy(mp.icp);
  mp.icp = nullptr;
  if (mp.pg) llsr_pg_destroy(mp.pg);
  mp.pg = nullptr;
  mp.sm = llsr_handle::MapSmall{};
  mp.prior = nullptr;  // llsr_mapping_init drops the attachment
  mp.live = false;
}

extern "C" int32_t llsr_mapping_init(llsr_handle* h, int32_t mo_mode, const llsr_map_config* map_cfg) {
  if (!h) return LLSR_EINVAL;
  if (mo_mode != LLSR_MODE_FAITHFUL && mo_mode != LLSR_MODE_LM_APPLIED) return fail(h, LLSR_EINVAL, "mo_mode");
  // both handle modes: llsr_mapping_batch refuses the faithful one itself, llsr_mapping_batch_odom runs it
  llsr_map_config mcfg;
  if (map_cfg) mcfg = *map_cfg;  // NULL: the YAML block of the handle's lidar
  else  // a use_vlp32c handle gets its own block whatever its H
    llsr_map_config_lidar(&mcfg, h->cfg.use_vlp32c ? LLSR_LIDAR_VLP32C
                                 : h->dc.H == 64   ? LLSR_LIDAR_HDL64E : LLSR_LIDAR_VLP16);
  if (mcfg.enable_loop_closure && mcfg.surrounding_keyframe_search_num < 1)
    return fail(h, LLSR_EINVAL, "surrounding_keyframe_search_num must be >= 1 with loop closure");
  HIP_OK(h, hipSetDevice(h->device));
  int32_t rc = odo_alloc(h);
  if (rc != LLSR_OK) return rc;
  auto& mp = h->mp;
  HIP_OK(h, sync_handle_streams(h));
  mapping_free(h);  // a repeated init rebuilds everything with the new map config
  mp.mode = mo_mode;
  mp.mcfg = mcfg;
  const int B = h->max_batch;
  mp.slot.resize(B);
  for (auto& sl : mp.slot)
    if (!(sl.map = llsr_map_create(&mp.mcfg, h->device))) { mapping_free(h); return fail(h, LLSR_ENOMEM, "llsr_map_create"); }
  if (!(mp.vg = llsr_map_create(&mp.mcfg, h->device))) { mapping_free(h); return fail(h, LLSR_ENOMEM, "llsr_map_create"); }
  llsr_handle::MapSmall sm;  // built aside: mp.sm stays empty unless both allocations succeed
  if (llsr_host::alloc_pool(sm.dev, 0, [&](llsr_host::Carver& c) { llsr_host::mapping_layout(c, sm, B); }) != hipSuccess) {
    mapping_free(h);
    return fail(h, LLSR_ENOMEM, "mapping state");
  }
  if (llsr_host::alloc_pool(sm.host, 0, [&](llsr_host::Carver& c) { llsr_host::mapping_host_layout(c, sm, B); }) !=
      hipSuccess) {
    mapping_free(h);
    return fail(h, LLSR_ENOMEM, "mapping staging");
  }
  mp.sm = std::move(sm);
  mp.live = true;
  return llsr_mapping_reset(h);
}

// The slots' graphs start with room for 256 poses each and an envelope of four blocks per pose (two
// for the odometry chain, two for loops); a full object is replaced by a larger one: twice the poses,
// or twice the envelope up to what max_loops loops can need at most, (2 + max_loops) blocks per pose.
static int32_t pg_regrow(llsr_handle* h, int32_t max_poses, int64_t max_blocks) {
  auto& mp = h->mp;
  int32_t k, l;
  int64_t e;
  llsr_pg_capacity(mp.pg, &k, &l, &e);
  llsr_pg* g = llsr_pg_grown(mp.pg, std::max(k, max_poses), l, std::max(e, max_blocks));
  if (!g) return fail(h, LLSR_ENOMEM, "pose graph: no memory to grow");
  llsr_pg_destroy(mp.pg);
  mp.pg = g;
  return LLSR_OK;
}

// Keyframe `kp` of slot b into its graph (saveKeyFramesAndFactor's factors, MO:1641-1664)
static int32_t pg_append_slot(llsr_handle* h, int b, const float* kp) {
  auto& mp = h->mp;
  int32_t rc = llsr_pg_append(mp.pg, b, kp, 1);
  if (rc == LLSR_ERANGE) {  // poses or envelope: both double (a loop's span keeps its share)
    int32_t k, l;
    int64_t e;
    llsr_pg_capacity(mp.pg, &k, &l, &e);
    if ((rc = pg_regrow(h, 2 * k, 2 * e)) != LLSR_OK) return rc;
    rc = llsr_pg_append(mp.pg, b, kp, 1);
  }
  return rc == LLSR_OK ? rc : fail(h, rc, std::string("pose graph: ") + llsr_pg_last_error(mp.pg));
}

// The loop factor of slot b's accepted report (MO:1086-1088)
static int32_t pg_loop_slot(llsr_handle* h, int b, const llsr_loop_report& r) {
  auto& mp = h->mp;
  for (;;) {
    const int32_t rc = llsr_pg_add_loop(mp.pg, b, r.latest_id, r.closest_id, r.pose_from, r.pose_to, r.variance);
    if (rc == LLSR_OK) return rc;
    int32_t k, l;
    int64_t e;
    llsr_pg_capacity(mp.pg, &k, &l, &e);
    const int64_t most = (int64_t)(2 + l) * k;  // beyond this only the loop capacity can be what is full
    if (rc != LLSR_ERANGE || e >= most) return fail(h, rc, std::string("pose graph: ") + llsr_pg_last_error(mp.pg));
    const int32_t g = pg_regrow(h, k, std::min(2 * e, most));
    if (g != LLSR_OK) return g;
  }
}

// MapOptimization::run for the slots in `step` (their pose glue already applied by the caller);
// times: the staged timeLaserOdometry of the B scans (llsr_mapping_stage_times), or NULL.
static int32_t mapping_mo(llsr_handle* h, int32_t B, hipStream_t s, const std::vector<char>& step,
                          const double* times) {
  auto& mp = h->mp;
  auto& o = h->odo;
  int32_t rc = LLSR_OK;
  const int NB = o.B, nb = NB + 1;
  // this frame's AssociationOut clouds (the batch flipped o.cur to them)
  const int64_t* hs = o.h_off;                     // cloud_corner_scan (sharp, TransformToEnd)
  const int64_t* hf = o.h_off + nb;                // cloud_surf_scan (flat + shadow, TransformToEnd)
  const int64_t* hlc = o.h_off + (2 + o.cur) * nb; // cloud_corner_last
  const int64_t* hls = o.h_off + (4 + o.cur) * nb; // cloud_surf_last (+ shadow)
  // adjustOutlierCloud of this frame's IP outliers (FA:2720)
  int64_t* hol = mp.sm.h_off + 4 * (size_t)nb;
  hol[0] = 0;
  int maxO = 0;
  for (int b = 0; b < NB; ++b) {
    const int n = (b < B && step[b]) ? o.h_counts[(size_t)b * kCnt + C_O] : 0;
    hol[b + 1] = hol[b] + n;
    maxO = n > maxO ? n : maxO;
  }
  rc = mp_grow(h, mp.outl, (size_t)hol[NB] + 1, 0, s);
  if (rc != LLSR_OK) return rc;
  HIP_OK(h, hipMemcpyAsync(mp.sm.d_off + 4 * (size_t)nb, hol, sizeof(int64_t) * nb, hipMemcpyHostToDevice, s));
  if (maxO > 0) {
    const int gx = (maxO + 255) / 256 < 64 ? (maxO + 255) / 256 : 64;
    k_mapping_outliers<<<dim3(gx, B), 256, 0, s>>>(h->d.outl, h->dc.HW, mp.sm.d_off + 4 * (size_t)nb, mp.outl.p());
    HIP_OK(h, hipGetLastError());
  }
  // downsampleCurrentScan (MO:1234-1258) of every slot in one segmented VoxelGrid; segments by
  // kind so each kind's per-slot results are contiguous: [corner last][surf last, outlier]...
  // [corner scan][surf scan]
  const float lc = mp.mcfg.corner_leaf, lsf = mp.mcfg.surf_leaf, lo = mp.mcfg.outlier_leaf;
  const int S5 = 5 * NB;
  std::vector<const float4*> src(S5);
  std::vector<long long> cnt(S5, 0), dso(S5 + 1), toto(NB + 1);
  std::vector<float> leaf(S5);
  long long total = 0;
  for (int b = 0; b < NB; ++b) {
    const bool on = b < B && step[b];
    src[b] = o.last_c[o.cur] + hlc[b];          cnt[b] = on ? hlc[b + 1] - hlc[b] : 0;          leaf[b] = lc;
    src[NB + 2 * b] = o.last_s[o.cur] + hls[b]; cnt[NB + 2 * b] = on ? hls[b + 1] - hls[b] : 0; leaf[NB + 2 * b] = lsf;
    src[NB + 2 * b + 1] = mp.outl.p() + hol[b];     cnt[NB + 2 * b + 1] = hol[b + 1] - hol[b];      leaf[NB + 2 * b + 1] = lo;
    src[3 * NB + b] = o.scan_c + hs[b];         cnt[3 * NB + b] = on ? hs[b + 1] - hs[b] : 0;   leaf[3 * NB + b] = lc;
    src[4 * NB + b] = o.scan_s + hf[b];         cnt[4 * NB + b] = on ? hf[b + 1] - hf[b] : 0;   leaf[4 * NB + b] = lsf;
  }
  for (long long c : cnt) total += c;
  rc = mp_grow(h, mp.ds, (size_t)total + 1, 0, s);
  if (rc != LLSR_OK) return rc;
  rc = llsr_mapping::voxel_multi(mp.vg, src.data(), cnt.data(), leaf.data(), S5, mp.ds.p(), dso.data(), s);
  if (rc != LLSR_OK) return fail(h, rc, std::string("downsample: ") + llsr_map_last_error(mp.vg));
  // laserCloudSurfTotalLastDS = surf leaf over SurfLastDS + OutlierLastDS (MO:1260-1266)
  std::vector<const float4*> tsrc(NB);
  std::vector<long long> tcnt(NB);
  std::vector<float> tleaf(NB, lsf);
  for (int b = 0; b < NB; ++b) {
    tsrc[b] = mp.ds.p() + dso[NB + 2 * b];
    tcnt[b] = dso[NB + 2 * b + 2] - dso[NB + 2 * b];
  }
  rc = mp_grow(h, mp.tot, (size_t)(dso[3 * NB] - dso[NB]) + 1, 0, s);
  if (rc != LLSR_OK) return rc;
  rc = llsr_mapping::voxel_multi(mp.vg, tsrc.data(), tcnt.data(), tleaf.data(), NB, mp.tot.p(), toto.data(), s);
  if (rc != LLSR_OK) return fail(h, rc, std::string("downsample: ") + llsr_map_last_error(mp.vg));
  // extractSurroundingKeyFrames (MO:1096-1232) around currentRobotPosPoint, every slot with
  // keyframes in one pass (a slot without keyframes keeps an empty local map, MO:1097)
  // With a prior map attached: its crop around the same point, for every stepping slot, keyframes
  // or not
  std::vector<llsr_map*> emaps;
  std::vector<int> eslot;
  std::vector<float> epos;
  for (int b = 0; b < B; ++b) {
    auto& sl = mp.slot[b];
    if (!step[b]) continue;
    sl.mrep = llsr_map_report{};
    sl.n_cq = (int)(dso[3 * NB + b + 1] - dso[3 * NB + b]);
    sl.n_sq = (int)(toto[b + 1] - toto[b]);
    if (!mp.prior && llsr_map_num_keyframes(sl.map) == 0) continue;
    emaps.push_back(sl.map);
    eslot.push_back(b);
    epos.insert(epos.end(), sl.robot, sl.robot + 3);
  }
  const int nE = (int)emaps.size();
  std::vector<llsr_map_report> ereps(nE > 0 ? nE : 1);
  std::vector<long long> eoc(nE + 1, 0), eos(nE + 1, 0);
  const float4* lmap = nullptr;
  if (nE > 0 && mp.prior) {
    std::vector<int64_t> oc(nE + 1), os(nE + 1);
    rc = llsr_prior_ns::crop_begin(mp.prior, epos.data(), nE, oc.data(), os.data(), s);
    if (rc != LLSR_OK) return fail(h, rc, std::string("prior crop: ") + llsr_prior_ns::error_of(mp.prior));
    rc = mp_grow(h, mp.cmap, (size_t)os[nE] + 1, 0, s);
    if (rc != LLSR_OK) return rc;
    rc = llsr_prior_ns::crop_write(mp.prior, (float*)mp.cmap.p(), os[nE], s);
    if (rc != LLSR_OK) return fail(h, rc, std::string("prior crop: ") + llsr_prior_ns::error_of(mp.prior));
    lmap = mp.cmap.p();
    for (int e = 0; e <= nE; ++e) {
      eoc[e] = oc[e];
      eos[e] = os[e];
    }
    for (int e = 0; e < nE; ++e) {  // the crop is the local map as it is: no VoxelGrid (…Map = …DS)
      ereps[e].n_corner_map = ereps[e].n_corner_ds = oc[e + 1] - oc[e];
      ereps[e].n_surf_map = ereps[e].n_surf_ds = os[e + 1] - os[e];
    }
  } else if (nE > 0) {
    rc = llsr_mapping::extract_multi(mp.vg, emaps.data(), nE, epos.data(), ereps.data(), &lmap, eoc.data(),
                                     eos.data(), s);
    if (rc != LLSR_OK) return fail(h, rc, std::string("extract: ") + llsr_map_last_error(mp.vg));
  } else {
    rc = mp_grow(h, mp.cmap, 1, 0, s);  // a valid (empty) map base for the batch
    if (rc != LLSR_OK) return rc;
    lmap = mp.cmap.p();
  }
  int64_t* hcq = mp.sm.h_off;
  int64_t* hsq = mp.sm.h_off + nb;
  int64_t* hmc = mp.sm.h_off + 2 * (size_t)nb;
  int64_t* hms = mp.sm.h_off + 3 * (size_t)nb;
  long long mMc = 1, mMs = 1, mQc = 1, mQs = 1;
  {
    long long cc = eoc[0], cs = eos[0];
    int e = 0;
    for (int b = 0; b < NB; ++b) {
      hcq[b] = dso[3 * NB + b];
      hsq[b] = toto[b];
      hmc[b] = cc;
      hms[b] = cs;
      if (e < nE && eslot[e] == b) {
        mp.slot[b].mrep = ereps[e];
        cc = eoc[e + 1];
        cs = eos[e + 1];
        ++e;
      }
      mMc = std::max(mMc, (long long)(cc - hmc[b]));
      mMs = std::max(mMs, (long long)(cs - hms[b]));
      mQc = std::max(mQc, (long long)(dso[3 * NB + b + 1] - dso[3 * NB + b]));
      mQs = std::max(mQs, (long long)(toto[b + 1] - toto[b]));
    }
    hmc[NB] = cc;
    hms[NB] = cs;
    hcq[NB] = dso[4 * NB];
    hsq[NB] = toto[NB];
  }
  // scan2MapOptimization (MO:1572-1610): every slot is a problem; slots without a step, or whose
  // map fails MO:1573, stay inactive and keep their pose and LM members
  rc = llsr_scan2map_reserve(h, NB, (int32_t)mMc, (int32_t)mMs, (int32_t)mQc, (int32_t)mQs);
  if (rc != LLSR_OK) return rc;
  for (int b = 0; b < NB; ++b)
    for (int k = 0; k < 6; ++k) mp.sm.h_pose[6 * b + k] = mp.slot[b].pose.transformTobeMapped[k];
  HIP_OK(h, hipMemcpyAsync(mp.sm.d_pose, mp.sm.h_pose, sizeof(float) * 6 * NB, hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(mp.sm.d_off, mp.sm.h_off, sizeof(int64_t) * 4 * nb, hipMemcpyHostToDevice, s));
  llsr_s2m_batch sb{};
  sb.n_problems = NB;
  sb.corner_q = (const float*)mp.ds.p(); sb.corner_q_off = mp.sm.d_off;
  sb.surf_q = (const float*)mp.tot.p(); sb.surf_q_off = mp.sm.d_off + nb;
  sb.corner_map = (const float*)lmap; sb.corner_map_off = mp.sm.d_off + 2 * (size_t)nb;
  sb.surf_map = (const float*)lmap; sb.surf_map_off = mp.sm.d_off + 3 * (size_t)nb;
  sb.pose = mp.sm.d_pose;
  sb.report = mp.sm.d_rep;
  S2MOpts opt;
  opt.mode = mp.mode;
  opt.deg_in = opt.deg_out = mp.sm.d_deg;
  opt.matP_in = opt.matP_out = mp.sm.d_matP;
  rc = s2m_batch(h, &sb, s, opt);
  if (rc != LLSR_OK) return rc;
  HIP_OK(h, hipMemcpyAsync(mp.sm.h_pose, mp.sm.d_pose, sizeof(float) * 6 * NB, hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipMemcpyAsync(mp.sm.h_rep, mp.sm.d_rep, sizeof(llsr_lm_report) * NB, hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipStreamSynchronize(s));
  // transformUpdate (MO:1608) and saveKeyFramesAndFactor (MO:1612-1755)
  for (int b = 0; b < B; ++b) {
    if (!step[b]) continue;
    auto& sl = mp.slot[b];
    auto& P = sl.pose;
    sl.lm = mp.sm.h_rep[b];
    sl.lm_ran = (hmc[b + 1] - hmc[b] > 10 && hms[b + 1] - hms[b] > 100) ? 1 : 0;
    if (sl.lm_ran) {
      for (int k = 0; k < 6; ++k) P.transformTobeMapped[k] = mp.sm.h_pose[6 * b + k];
      llsr_mapping::transform_update(P);
    }
    for (int k = 0; k < 3; ++k) sl.robot[k] = P.transformAftMapped[3 + k];
    const bool first = llsr_map_num_keyframes(sl.map) == 0;
    const float* est = first ? P.transformTobeMapped : P.transformAftMapped;  // iSAM2's latestEstimate
    const float kp[6] = {est[3], est[4], est[5], est[0], est[1], est[2]};
    for (int k = 0; k < 6; ++k) {
      P.transformLast[k] = est[k];
      if (!first) P.transformTobeMapped[k] = P.transformAftMapped[k];
    }
    // (localisation: the key pose and its time only; the store then counts key poses, no clouds)
    const int kf = mp.prior ? llsr_map_add_keyframe(sl.map, kp, nullptr, 0, nullptr, 0, nullptr, 0, s)
                            : llsr_map_add_keyframe(
        sl.map, kp, (const float*)(o.scan_c + hs[b]), (int32_t)(hs[b + 1] - hs[b]),
        (const float*)(mp.ds.p() + dso[NB + 2 * b]), (int32_t)(dso[NB + 2 * b + 1] - dso[NB + 2 * b]),
        (const float*)(mp.ds.p() + dso[NB + 2 * b + 1]), (int32_t)(dso[NB + 2 * b + 2] - dso[NB + 2 * b + 1]), s);
    if (kf < 0) return fail(h, kf, std::string("add_keyframe: ") + llsr_map_last_error(sl.map));
    if (times) llsr_map_set_keyframe_time(sl.map, kf, times[b]);  // thisPose6D.time (MO:1706)
    sl.keyposes.insert(sl.keyposes.end(), kp, kp + 6);
    sl.mo_frames += 1;
    if (mp.pg && (rc = pg_append_slot(h, b, kp)) != LLSR_OK) return rc;
  }
#ifdef LLSR_S2S_PROF
  {  // diagnostics build only: fail this call's MapOptimization part once, after its keyframes were
     // added, when slot 0 reaches MapOptimization frame LLSR_MO_FAIL_AT (tests/test_gpu_mapping_rollback.py)
    static bool fired = false;
    const char* at = std::getenv("LLSR_MO_FAIL_AT");
    if (at && !fired && step[0] && mp.slot[0].mo_frames == std::atoi(at)) {
      fired = true;
      return fail(h, LLSR_EIO, "injected MapOptimization failure (LLSR_MO_FAIL_AT)");
    }
  }
#endif
  return LLSR_OK;
}

// llsr_mapping_batch (samples == nullptr) and llsr_mapping_batch_odom
static int32_t mapping_batch(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets, int32_t B,
                             const llsr_odom_sample* samples, const uint8_t* overwrite, void* hip_stream) {
  auto& mp = h->mp;
  if (!mp.live) return fail(h, LLSR_EINVAL, "llsr_mapping_init not called");
  if (B < 1 || B > h->max_batch) return fail(h, LLSR_ERANGE, "batch size outside [1, max_batch]");
  if (mp.times_staged && (int)mp.times.size() != B)
    return fail(h, LLSR_EINVAL, "the staged scan times (llsr_mapping_stage_times) are for another batch size");
  hipStream_t s;
  HIP_OK(h, enter(h, hip_stream, &s));
  mp.fresh = false;
  int32_t rc = odo_batch(h, d_xyzi, d_offsets, B, samples, overwrite, s);
  if (rc != LLSR_OK) return rc;
  // the staged scan times are consumed here, with the odometry's advance
  std::vector<double> times;
  const bool timed = mp.times_staged;
  times.swap(mp.times);
  mp.times_staged = false;
  auto& o = h->odo;
  HIP_OK(h, hipMemcpyAsync(mp.sm.h_frames, o.frames, sizeof(int) * B, hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipMemcpyAsync(mp.sm.h_tsum, o.tsum, sizeof(float) * 6 * B, hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipStreamSynchronize(s));
  rc = llsr_scan2scan_check(h);
  if (rc != LLSR_OK) return rc;
  // MapOptimization's members of the B slots before this frame: an error below restores them
  struct Snap {
    llsr_handle::MapSlot slot;  // (keyposes: only its length is restored)
    size_t n_keyposes;
    int n_keyframes;
    llsr_mapping::MapSel sel;
  };
  std::vector<Snap> snap(B);
  for (int b = 0; b < B; ++b) {
    const auto& sl = mp.slot[b];
    snap[b].slot.pose = sl.pose;
    std::memcpy(snap[b].slot.robot, sl.robot, sizeof sl.robot);
    snap[b].slot.mo_frames = sl.mo_frames; snap[b].slot.lm_ran = sl.lm_ran;
    snap[b].slot.n_cq = sl.n_cq; snap[b].slot.n_sq = sl.n_sq; snap[b].slot.cycle = sl.cycle;
    snap[b].slot.lm = sl.lm; snap[b].slot.mrep = sl.mrep; snap[b].slot.now = sl.now;
    snap[b].n_keyposes = sl.keyposes.size();
    snap[b].n_keyframes = llsr_map_num_keyframes(sl.map);
    snap[b].sel = llsr_mapping::map_selection(sl.map);
  }
  std::vector<char> step(o.B, 0);  // slots that receive an AssociationOut this call
  for (int b = 0; b < B; ++b) {
    auto& sl = mp.slot[b];
    sl.frames = mp.sm.h_frames[b];
    // FA:2781-2784: the first scan sends nothing; FA:2818-2821: every mapping_frequency_divider-th
    // frame after it sends an AssociationOut
    if (sl.frames >= 2 && ++sl.cycle == h->cfg.mapping_frequency_divider) {
      sl.cycle = 0;
      step[b] = 1;
    }
    if (!step[b]) continue;
    if (timed) sl.now = times[b];  // timeLaserOdometry of the AssociationOut MapOptimization receives
    llsr_mapping::odometry_roundtrip(mp.sm.h_tsum + 6 * b, sl.pose.transformSum);  // OdometryToTransform
    llsr_mapping::transform_associate_to_map(sl.pose);
  }
  bool any = false;
  for (char c : step) any |= c != 0;
  if (any) {  // the LM members (isDegenerate, matP) before this frame, restored if it fails
    HIP_OK(h, hipMemcpyAsync(mp.sm.d_deg_bak, mp.sm.d_deg, sizeof(int) * o.B, hipMemcpyDeviceToDevice, s));
    HIP_OK(h, hipMemcpyAsync(mp.sm.d_matP_bak, mp.sm.d_matP, sizeof(float) * 36 * o.B, hipMemcpyDeviceToDevice, s));
  }
  rc = any ? mapping_mo(h, B, s, step, timed ? times.data() : nullptr) : LLSR_OK;
  if (rc != LLSR_OK) {
    const std::string msg = h->err;
    (void)hipStreamSynchronize(s);
    for (int b = 0; b < B; ++b) {
      auto& sl = mp.slot[b];
      const auto& sn = snap[b].slot;
      sl.pose = sn.pose;
      std::memcpy(sl.robot, sn.robot, sizeof sl.robot);
      sl.mo_frames = sn.mo_frames; sl.lm_ran = sn.lm_ran; sl.n_cq = sn.n_cq; sl.n_sq = sn.n_sq;
      sl.cycle = sn.cycle; sl.lm = sn.lm; sl.mrep = sn.mrep; sl.now = sn.now;
      sl.keyposes.resize(snap[b].n_keyposes);
      if (mp.pg) (void)llsr_pg_truncate(mp.pg, b, (int32_t)(snap[b].n_keyposes / 6));
      llsr_mapping::truncate_keyframes(sl.map, snap[b].n_keyframes);
      llsr_mapping::set_map_selection(sl.map, snap[b].sel);
    }
    (void)hipMemcpy(mp.sm.d_deg, mp.sm.d_deg_bak, sizeof(int) * o.B, hipMemcpyDeviceToDevice);
    (void)hipMemcpy(mp.sm.d_matP, mp.sm.d_matP_bak, sizeof(float) * 36 * o.B, hipMemcpyDeviceToDevice);
    return fail(h, rc, msg);
  }
  HIP_OK(h, hipEventRecord(h->last_done, s));
  h->last_rec = true;
  h->last_stream = s;
  return LLSR_OK;
}

extern "C" int32_t llsr_mapping_batch(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets, int32_t B,
                                      void* hip_stream) {
  if (!h) return LLSR_EINVAL;
  if (h->cfg.mode != LLSR_MODE_LM_APPLIED)
    return fail(h, LLSR_ENOSYS, "the mapping chain runs the odometry, which needs LLSR_MODE_LM_APPLIED "
                                "(llsr_mapping_batch_odom takes the /odom2 input of the faithful mode)");
  return mapping_batch(h, d_xyzi, d_offsets, B, nullptr, nullptr, hip_stream);
}

extern "C" int32_t llsr_mapping_batch_odom(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets, int32_t B,
                                           const llsr_odom_sample* samples, const uint8_t* overwrite,
                                           void* hip_stream) {
  if (!h) return LLSR_EINVAL;
  if (!samples) return fail(h, LLSR_EINVAL, "llsr_mapping_batch_odom: samples is NULL");
  return mapping_batch(h, d_xyzi, d_offsets, B, samples, overwrite, hip_stream);
}

extern "C" int32_t llsr_mapping_fetch(llsr_handle* h, int32_t b, llsr_mapping_slot* out) {
  if (!h || !out) return LLSR_EINVAL;
  auto& mp = h->mp;
  if (!mp.live) return fail(h, LLSR_EINVAL, "llsr_mapping_init not called");
  if (b < 0 || b >= (int)mp.slot.size()) return fail(h, LLSR_ERANGE, "slot outside [0, max_batch)");
  const auto& sl = mp.slot[b];
  std::memset(out, 0, sizeof *out);
  out->frames = sl.frames;
  out->mo_frames = sl.mo_frames;
  out->keyframes = (int32_t)(sl.keyposes.size() / 6);
  out->lm_ran = sl.lm_ran;
  for (int k = 0; k < 6; ++k) {
    out->transform_sum[k] = sl.pose.transformSum[k];
    out->transform_tobe_mapped[k] = sl.pose.transformTobeMapped[k];
    out->transform_bef_mapped[k] = sl.pose.transformBefMapped[k];
    out->transform_aft_mapped[k] = sl.pose.transformAftMapped[k];
  }
  out->n_corner_q = sl.n_cq;
  out->n_surf_q = sl.n_sq;
  out->lm = sl.lm;
  out->map = sl.mrep;
  return LLSR_OK;
}

static const char kNoClouds[] = "a prior map is attached (llsr_mapping_set_prior): the slots keep no keyframe clouds";

// publishGlobalMap / saveMapService on slot b's store (llsr_map.hip), after the handle's own streams
static int32_t mapping_slot_map(llsr_handle* h, int32_t b, llsr_handle::MapSlot** sl) {
  auto& mp = h->mp;
  if (!mp.live) return fail(h, LLSR_EINVAL, "llsr_mapping_init not called");
  if (b < 0 || b >= (int)mp.slot.size()) return fail(h, LLSR_ERANGE, "slot outside [0, max_batch)");
  HIP_OK(h, hipSetDevice(h->device));
  HIP_OK(h, sync_handle_streams(h));
  *sl = &mp.slot[b];
  return LLSR_OK;
}

extern "C" int32_t llsr_mapping_global_map(llsr_handle* h, int32_t b, const llsr_global_map_config* cfg,
                                           float* d_global, int64_t cap_global, float* d_edge, int64_t cap_edge,
                                           float* d_planar, int64_t cap_planar, llsr_global_map_report* rep,
                                           void* hip_stream) {
  if (!h || !rep) return LLSR_EINVAL;
  if (h->mp.live && h->mp.prior) return fail(h, LLSR_ENOSYS, kNoClouds);
  llsr_handle::MapSlot* sl = nullptr;
  int32_t rc = mapping_slot_map(h, b, &sl);
  if (rc != LLSR_OK) return rc;
  rc = llsr_map_global(sl->map, cfg, sl->pose.transformAftMapped + 3, d_global, cap_global, d_edge, cap_edge,
                       d_planar, cap_planar, rep, hip_stream);
  return rc == LLSR_OK ? rc : fail(h, rc, std::string("global map: ") + llsr_map_last_error(sl->map));
}

extern "C" int32_t llsr_mapping_save_map(llsr_handle* h, int32_t b, float* d_corner, int64_t cap_corner,
                                         float* d_surf, int64_t cap_surf, int64_t* n_corner, int64_t* n_surf,
                                         void* hip_stream) {
  if (!h) return LLSR_EINVAL;
  if (h->mp.live && h->mp.prior) return fail(h, LLSR_ENOSYS, kNoClouds);
  llsr_handle::MapSlot* sl = nullptr;
  int32_t rc = mapping_slot_map(h, b, &sl);
  if (rc != LLSR_OK) return rc;
  rc = llsr_map_save(sl->map, d_corner, cap_corner, d_surf, cap_surf, n_corner, n_surf, hip_stream);
  return rc == LLSR_OK ? rc : fail(h, rc, std::string("save map: ") + llsr_map_last_error(sl->map));
}

extern "C" int32_t llsr_mapping_keyposes(llsr_handle* h, int32_t b, float* out, int32_t cap) {
  if (!h) return LLSR_EINVAL;
  auto& mp = h->mp;
  if (!mp.live) return fail(h, LLSR_EINVAL, "llsr_mapping_init not called");
  if (b < 0 || b >= (int)mp.slot.size()) return fail(h, LLSR_ERANGE, "slot outside [0, max_batch)");
  const auto& kp = mp.slot[b].keyposes;
  const int n = (int)(kp.size() / 6);
  if (out && cap > 0) std::memcpy(out, kp.data(), sizeof(float) * 6 * (size_t)(n < cap ? n : cap));
  return n;
}

// ---- loop closure of the slots (detectLoopClosure / performLoopClosure / correctPoses per slot) ----
extern "C" int32_t llsr_mapping_stage_times(llsr_handle* h, const double* seconds, int32_t B) {
  if (!h) return LLSR_EINVAL;
  auto& mp = h->mp;
  if (!mp.live) return fail(h, LLSR_EINVAL, "llsr_mapping_init not called");
  if (!seconds) return fail(h, LLSR_EINVAL, "llsr_mapping_stage_times: seconds is NULL");
  if (B < 1 || B > h->max_batch) return fail(h, LLSR_ERANGE, "batch size outside [1, max_batch]");
  mp.times.assign(seconds, seconds + B);
  mp.times_staged = true;
  return LLSR_OK;
}

extern "C" int32_t llsr_mapping_keyframe_times(llsr_handle* h, int32_t b, double* out, int32_t cap) {
  if (!h) return LLSR_EINVAL;
  auto& mp = h->mp;
  if (!mp.live) return fail(h, LLSR_EINVAL, "llsr_mapping_init not called");
  if (b < 0 || b >= (int)mp.slot.size()) return fail(h, LLSR_ERANGE, "slot outside [0, max_batch)");
  const int32_t n = llsr_map_keyframe_times(mp.slot[b].map, out, cap);
  return n >= 0 ? n : fail(h, n, "llsr_mapping_keyframe_times: bad arguments");
}

extern "C" int32_t llsr_mapping_loop_closure(llsr_handle* h, const llsr_loop_config* cfg, int32_t B,
                                             llsr_loop_report* reps, void* hip_stream) {
  if (!h || !reps) return LLSR_EINVAL;
  auto& mp = h->mp;
  if (!mp.live) return fail(h, LLSR_EINVAL, "llsr_mapping_init not called");
  if (mp.prior) return fail(h, LLSR_ENOSYS, kNoClouds);
  if (B < 1 || B > (int)mp.slot.size()) return fail(h, LLSR_ERANGE, "batch size outside [1, max_batch]");
  llsr_loop_config own;
  if (!cfg) {  // the block of the handle's lidar, chosen as llsr_mapping_init chooses the map's
    llsr_loop_config_lidar(&own, h->cfg.use_vlp32c ? LLSR_LIDAR_VLP32C : h->dc.H == 64 ? LLSR_LIDAR_HDL64E
                                                                                          : LLSR_LIDAR_VLP16);
    cfg = &own;
  }
  if (cfg->search_num < 0 || !(cfg->leaf > 0)) return fail(h, LLSR_EINVAL, "loop closure: bad configuration");
  const auto t0 = std::chrono::steady_clock::now();
  hipStream_t s;
  HIP_OK(h, enter(h, hip_stream, &s));
  HIP_OK(h, sync_handle_streams(h));
  // §16 steps 1-5 per slot, each in its store's own scratch (they stay valid: one store per slot)
  std::vector<const float4*> src(B, nullptr), tgt(B, nullptr);
  std::vector<int> found;
  std::vector<int64_t> soff(1, 0), toff(1, 0);
  for (int b = 0; b < B; ++b) {
    auto& sl = mp.slot[b];
    const int32_t rc = llsr_mapping::loop_submaps_raw(sl.map, cfg, sl.robot, sl.now, &reps[b], &src[b], &tgt[b], s);
    if (rc != LLSR_OK) return fail(h, rc, std::string("loop closure: ") + llsr_map_last_error(sl.map));
    if (!reps[b].found) continue;
    if (reps[b].n_source > LLSR_ICP_MAX_POINTS || reps[b].n_target > LLSR_ICP_MAX_POINTS)
      return fail(h, LLSR_ERANGE, "loop closure: more than LLSR_ICP_MAX_POINTS points to align");
    found.push_back(b);
    soff.push_back(soff.back() + reps[b].n_source);
    toff.push_back(toff.back() + reps[b].n_target);
  }
  const int P = (int)found.size();
  if (P > 0) {
    // MO:1011-1012: the raw clouds, not the downsampled ones, gathered in the batch's layout
    int32_t rc = mp_grow(h, mp.lsrc, (size_t)soff[P] + 1, 0, s);
    if (rc == LLSR_OK) rc = mp_grow(h, mp.ltgt, (size_t)toff[P] + 1, 0, s);
    if (rc != LLSR_OK) return rc;
    for (int i = 0; i < P; ++i) {
      const int b = found[i];
      if (reps[b].n_source > 0)
        HIP_OK(h, hipMemcpyAsync(mp.lsrc.p() + soff[i], src[b], (size_t)reps[b].n_source * sizeof(float4),
                                 hipMemcpyDeviceToDevice, s));
      if (reps[b].n_target > 0)
        HIP_OK(h, hipMemcpyAsync(mp.ltgt.p() + toff[i], tgt[b], (size_t)reps[b].n_target * sizeof(float4),
                                 hipMemcpyDeviceToDevice, s));
    }
    if (!mp.icp) mp.icp = llsr_icp_create(h->device);
    if (!mp.icp) return fail(h, LLSR_ENOMEM, "loop closure: no ICP workspace");
    std::vector<llsr_icp_result> res(P);
    rc = llsr_icp_align_batch(mp.icp, P, (const float*)mp.lsrc.p(), soff.data(), (const float*)mp.ltgt.p(), toff.data(),
                              cfg, 1, res.data(), nullptr, s);
    if (rc != LLSR_OK) return fail(h, rc, std::string("loop closure: ") + llsr_icp_last_error(mp.icp));
    for (int i = 0; i < P; ++i) {
      llsr_loop_report& rep = reps[found[i]];
      const auto& kp = mp.slot[found[i]].keyposes;
      rep.icp = res[i];
      llsr_loop::loop_accept(cfg, kp.data() + 6 * (size_t)rep.latest_id, kp.data() + 6 * (size_t)rep.closest_id, &rep);
    }
  }
  const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (int b = 0; b < B; ++b)
    if (reps[b].found) reps[b].ms = ms;
  return LLSR_OK;
}

extern "C" int32_t llsr_mapping_set_key_poses(llsr_handle* h, int32_t b, const float* poses6, int32_t n,
                                              const float* latest_estimate6) {
  if (!h) return LLSR_EINVAL;
  llsr_handle::MapSlot* sl = nullptr;
  int32_t rc = mapping_slot_map(h, b, &sl);
  if (rc != LLSR_OK) return rc;
  rc = llsr_map_set_key_poses(sl->map, poses6, n);  // validates poses6 / n against the store
  if (rc != LLSR_OK) return fail(h, rc, std::string("set key poses: ") + llsr_map_last_error(sl->map));
  if (n > 0) std::memcpy(sl->keyposes.data(), poses6, sizeof(float) * 6 * (size_t)n);
  if (latest_estimate6) {  // MO:1722-1733 with iSAM2's latestEstimate after the loop factor
    auto& P = sl->pose;
    for (int k = 0; k < 6; ++k)
      P.transformAftMapped[k] = P.transformLast[k] = P.transformTobeMapped[k] = latest_estimate6[k];
    for (int k = 0; k < 3; ++k) sl->robot[k] = P.transformAftMapped[3 + k];
  }
  return LLSR_OK;
}

// ---- localisation in a prior map ----
extern "C" int32_t llsr_mapping_set_prior(llsr_handle* h, llsr_prior* p) {
  if (!h) return LLSR_EINVAL;
  auto& mp = h->mp;
  if (!mp.live) return fail(h, LLSR_EINVAL, "llsr_mapping_init not called");
  if (!mp.fresh)
    return fail(h, LLSR_EINVAL, "llsr_mapping_set_prior: allowed only directly after llsr_mapping_init or "
                                "llsr_mapping_reset, before any frame");
  if (p && llsr_prior_ns::device_of(p) != h->device)
    return fail(h, LLSR_EINVAL, "llsr_mapping_set_prior: the prior map is not on the handle's device");
  mp.prior = p;
  return LLSR_OK;
}

// The /initialpose handler the reference left commented out (MO:437-456)
extern "C" int32_t llsr_mapping_set_pose(llsr_handle* h, int32_t b, const float pose6[6]) {
  if (!h) return LLSR_EINVAL;
  auto& mp = h->mp;
  if (!mp.live) return fail(h, LLSR_EINVAL, "llsr_mapping_init not called");
  if (!pose6) return fail(h, LLSR_EINVAL, "llsr_mapping_set_pose: pose6 is NULL");
  if (b < 0 || b >= (int)mp.slot.size()) return fail(h, LLSR_ERANGE, "slot outside [0, max_batch)");
  auto& sl = mp.slot[b];
  for (int k = 0; k < 6; ++k)
    sl.pose.transformAftMapped[k] = sl.pose.transformTobeMapped[k] = sl.pose.transformLast[k] = pose6[k];
  for (int k = 0; k < 3; ++k) sl.robot[k] = pose6[3 + k];
  return LLSR_OK;
}

// ---- the slots' pose graphs: the factor graph of MO:1086-1090 / 1612-1690 per slot ----
extern "C" int32_t llsr_mapping_enable_pose_graph(llsr_handle* h, int32_t on, int32_t max_loops) {
  if (!h) return LLSR_EINVAL;
  auto& mp = h->mp;
  if (!mp.live) return fail(h, LLSR_EINVAL, "llsr_mapping_init not called");
  if (on && max_loops < 1) return fail(h, LLSR_EINVAL, "pose graph: max_loops must be >= 1");
  HIP_OK(h, hipSetDevice(h->device));
  if (mp.pg) llsr_pg_destroy(mp.pg);
  mp.pg = nullptr;
  if (!on) return LLSR_OK;
  size_t most = 0;
  for (const auto& sl : mp.slot) most = std::max(most, sl.keyposes.size() / 6);
  int32_t max_poses = 256;
  while ((size_t)max_poses < most) max_poses *= 2;
  mp.pg = llsr_pg_create(h->device, (int32_t)mp.slot.size(), max_poses, max_loops, 4 * (int64_t)max_poses);
  if (!mp.pg) return fail(h, LLSR_ENOMEM, "llsr_pg_create");
  for (int b = 0; b < (int)mp.slot.size(); ++b) {  // the graphs start from the slots' key poses
    const auto& kp = mp.slot[b].keyposes;
    const int32_t rc = llsr_pg_append(mp.pg, b, kp.data(), (int32_t)(kp.size() / 6));
    if (rc != LLSR_OK) {
      const std::string msg = llsr_pg_last_error(mp.pg);
      llsr_pg_destroy(mp.pg);
      mp.pg = nullptr;
      return fail(h, rc, "pose graph: " + msg);
    }
  }
  return LLSR_OK;
}

extern "C" int32_t llsr_mapping_pose_graph_poses(llsr_handle* h, int32_t b, float* out6, int32_t cap) {
  if (!h) return LLSR_EINVAL;
  auto& mp = h->mp;
  if (!mp.live || !mp.pg) return fail(h, LLSR_EINVAL, "llsr_mapping_enable_pose_graph not called");
  if (b < 0 || b >= (int)mp.slot.size()) return fail(h, LLSR_ERANGE, "slot outside [0, max_batch)");
  return llsr_pg_poses(mp.pg, b, out6, cap);
}

extern "C" int32_t llsr_mapping_close_loops(llsr_handle* h, const llsr_loop_config* loop_cfg,
                                            const llsr_pg_config* pg_cfg, int32_t B, llsr_loop_report* loop_reps,
                                            llsr_pg_report* pg_reps, void* hip_stream) {
  if (!h || !loop_reps) return LLSR_EINVAL;
  auto& mp = h->mp;
  if (mp.live && mp.prior) return fail(h, LLSR_ENOSYS, kNoClouds);
  if (!mp.live || !mp.pg) return fail(h, LLSR_EINVAL, "llsr_mapping_enable_pose_graph not called");
  int32_t rc = llsr_mapping_loop_closure(h, loop_cfg, B, loop_reps, hip_stream);
  if (rc != LLSR_OK) return rc;
  for (int b = 0; b < B; ++b) {
    const llsr_loop_report& r = loop_reps[b];
    if (!r.found || !r.accepted) continue;
    if ((rc = pg_loop_slot(h, b, r)) != LLSR_OK) return rc;
  }
  hipStream_t s;
  HIP_OK(h, enter(h, hip_stream, &s));
  std::vector<llsr_pg_report> reps(mp.slot.size());
  rc = llsr_pg_optimize(mp.pg, pg_cfg, reps.data(), s);  // every slot's graph in one set of launches
  if (rc != LLSR_OK) return fail(h, rc, std::string("pose graph: ") + llsr_pg_last_error(mp.pg));
  if (pg_reps) std::copy(reps.begin(), reps.begin() + B, pg_reps);
  std::vector<float> poses;
  for (int b = 0; b < (int)mp.slot.size(); ++b) {
    if (!reps[b].moved) continue;
    const int32_t K = llsr_pg_poses(mp.pg, b, nullptr, 0);
    poses.resize(6 * (size_t)K);
    llsr_pg_poses(mp.pg, b, poses.data(), K);
    const float* kp = poses.data() + 6 * (size_t)(K - 1);
    const float latest[6] = {kp[3], kp[4], kp[5], kp[0], kp[1], kp[2]};  // MO:1722-1733
    rc = llsr_mapping_set_key_poses(h, b, poses.data(), K, latest);  // correctPoses (MO:1757-1785)
    if (rc != LLSR_OK) return rc;
  }
  return LLSR_OK;
}
