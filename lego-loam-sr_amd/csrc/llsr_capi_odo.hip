// llsr_capi_odo.hip — C-ABI host side of the end-to-end odometry (runFeatureAssociation,
// FA:2742-2853; kernels in llsr_odo.hip): the lazily built per-slot state, reset, the batch and
// the fetches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "llsr_handle.h"
#include "llsr_odo.h"
#include "llsr_odom_guess.h"

using namespace llsr;

// transformCur / transformSum, the flags and counters, offsets and reports of every slot to zero
static int32_t odo_zero(llsr_handle* h, llsr_handle::Odo& o) {
  for (const llsr_host::Span& z : o.zero)
    HIP_OK(h, hipMemset(static_cast<char*>(o.pool.get()) + z.off, 0, z.bytes));
  std::memset(o.h_off, 0, sizeof(int64_t) * 6 * (o.B + 1));
  o.cur = 0;
  return LLSR_OK;
}

int32_t odo_alloc(llsr_handle* h) {
  if (h->odo.pool) return LLSR_OK;
  return llsr_host::rebuild(h->odo, [&](llsr_handle::Odo& o) -> int32_t {
    const int B = h->max_batch;
    o.B = B;
    o.cap = (size_t)B * ((size_t)h->dc.HW + kShadow);
    if (llsr_host::alloc_pool(o.pool, 0, [&](llsr_host::Carver& c) { llsr_host::odo_layout(c, o, B, o.cap, kShadow); }) !=
        hipSuccess)
      return fail(h, LLSR_ENOMEM, "odometry buffers");
    if (llsr_host::alloc_pool(o.host, 0, [&](llsr_host::Carver& c) { llsr_host::odo_host_layout(c, o, B, kCnt); }) !=
        hipSuccess)
      return fail(h, LLSR_ENOMEM, "pinned odometry staging");
    float sh[4 * kShadow];
    llsr_shadow_points(sh);
    HIP_OK(h, hipMemcpy(o.shadow, sh, sizeof sh, hipMemcpyHostToDevice));
    const int32_t rc = llsr_reset_state(h);  // as llsr_odometry_reset
    return rc != LLSR_OK ? rc : odo_zero(h, o);
  });
}

extern "C" int32_t llsr_odometry_reset(llsr_handle* h) {
  if (!h) return LLSR_EINVAL;
  int32_t rc = llsr_reset_state(h);  // FA carry-over arrays (FA:167-198) of every slot
  if (rc != LLSR_OK || !h->odo.pool) return rc;
  HIP_OK(h, hipSetDevice(h->device));
  return odo_zero(h, h->odo);
}

// llsr_odometry_batch (samples == nullptr) and llsr_odometry_batch_odom: with samples, transformSum
// rides on the feature-count copy, updateInitialGuess (FA:2790) is evaluated on the host for the
// flagged slots and k_odo_finish swaps it in after the LM.
// With use_imu_undistortion (h->imu_undistortion) the guesses are evaluated and uploaded before the LM
// launch, k_odo_inputs_imu stores them as the LM's start (the pre-LM updateInitialGuess, FA:2786-2788)
// and k_odo_finish_imu reads the slots' IMU carry of this batch's feature stage.
int32_t odo_batch(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets, int32_t B,
                         const llsr_odom_sample* samples, const uint8_t* overwrite, void* hip_stream) {
  if (B < 1 || B > h->max_batch) return fail(h, LLSR_ERANGE, "batch size outside [1, max_batch]");
  hipStream_t s;
  HIP_OK(h, enter(h, hip_stream, &s));
  int32_t rc = odo_alloc(h);
  if (rc != LLSR_OK) return rc;
  auto& o = h->odo;
  rc = llsr_process_batch(h, d_xyzi, d_offsets, B, s);
  if (rc != LLSR_OK) return rc;
  // the feature counts size the packed clouds: one host sync per batch
  HIP_OK(h, hipMemcpyAsync(o.h_counts, h->d.counts, sizeof(int) * kCnt * B, hipMemcpyDeviceToHost, s));
  // the transformSum updateInitialGuess reads is the previous frame's: it does not depend on this
  // frame's LM, and llsr_process_batch ordered s after the previous call's k_odo_finish (last_done)
  if (samples) HIP_OK(h, hipMemcpyAsync(o.h_tsum, o.tsum, sizeof(float) * 6 * B, hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipStreamSynchronize(s));
  const int nb = o.B + 1;
  int64_t* hs = o.h_off;                       // sharp
  int64_t* hf = o.h_off + nb;                  // flat
  const int cur = o.cur, nxt = cur ^ 1;
  int64_t* hlc = o.h_off + (2 + cur) * nb;     // current last corner (from the previous batch)
  int64_t* hls = o.h_off + (4 + cur) * nb;
  int64_t* hnc = o.h_off + (2 + nxt) * nb;     // next last clouds
  int64_t* hns = o.h_off + (4 + nxt) * nb;
  int mMs = 0, mF = 0, mNc = 0, mNs = 0;
  hs[0] = hf[0] = hnc[0] = hns[0] = 0;
  for (int b = 0; b < B; ++b) {
    const int* c = o.h_counts + (size_t)b * kCnt;
    const int Ms = c[C_SHARP], F = c[C_F] + kShadow, M = c[C_M], L = c[C_L] + kShadow;
    hs[b + 1] = hs[b] + Ms;
    hf[b + 1] = hf[b] + F;
    hnc[b + 1] = hnc[b] + M;
    hns[b + 1] = hns[b] + L;
    mMs = Ms > mMs ? Ms : mMs;
    mF = F > mF ? F : mF;
    const int Nc = (int)(hlc[b + 1] - hlc[b]), Ns = (int)(hls[b + 1] - hls[b]);
    mNc = Nc > mNc ? Nc : mNc;
    mNs = Ns > mNs ? Ns : mNs;
  }
  // slots beyond B keep their (empty) ranges: offsets stay at the B-th value
  for (int b = B; b < o.B; ++b) {
    hs[b + 1] = hs[B]; hf[b + 1] = hf[B]; hnc[b + 1] = hnc[B]; hns[b + 1] = hns[B];
  }
  HIP_OK(h, hipMemcpyAsync(o.off, hs, sizeof(int64_t) * nb, hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(o.off + nb, hf, sizeof(int64_t) * nb, hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(o.off + (2 + nxt) * nb, hnc, sizeof(int64_t) * nb, hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(o.off + (4 + nxt) * nb, hns, sizeof(int64_t) * nb, hipMemcpyHostToDevice, s));
  rc = llsr_scan2scan_reserve(h, o.B, mMs > 1 ? mMs : 1, mF, mNc > 1 ? mNc : 1, mNs > 1 ? mNs : 1);
  if (rc != LLSR_OK) return rc;
  OdoArgs a{};
  a.B = B;
  a.HW = h->dc.HW;
  a.counts = h->d.counts;
  a.loam = h->d.loam;
  a.sharp_ind = h->d.sharp;
  a.flat_ind = h->d.flat;
  a.less_sharp = h->d.less_sharp;
  a.lflat = h->d.lflat;
  a.shadow = o.shadow;
  a.sharp_off = o.off; a.sharp = o.sharp;
  a.flat_off = o.off + nb; a.flat = o.flat;
  a.nlast_c_off = o.off + (2 + nxt) * nb; a.nlast_c = o.last_c[nxt];
  a.nlast_s_off = o.off + (4 + nxt) * nb; a.nlast_s = o.last_s[nxt];
  a.scan_c = o.scan_c; a.scan_s = o.scan_s;
  a.tcur = o.tcur; a.tsum = o.tsum; a.inited = o.inited; a.frames = o.frames;
  if (samples) { a.guess = o.guess; a.flags = o.flags; a.tlm = o.tlm; }
  const bool imu = h->imu_undistortion;
  // host-evaluated updateInitialGuess of the flagged slots (the same value before and after the LM:
  // the sample and transformSum do not change in between)
  auto upload_guesses = [&]() -> int32_t {
    for (int b = 0; b < B; ++b) {
      o.h_flags[b] = overwrite ? (overwrite[b] != 0) : 1;
      if (o.h_flags[b]) llsr_odom::update_initial_guess(samples[b], o.h_tsum + 6 * b, o.h_guess + 6 * b);
      else std::memset(o.h_guess + 6 * b, 0, sizeof(float) * 6);
    }
    HIP_OK(h, hipMemcpyAsync(o.guess, o.h_guess, sizeof(float) * 6 * B, hipMemcpyHostToDevice, s));
    HIP_OK(h, hipMemcpyAsync(o.flags, o.h_flags, B, hipMemcpyHostToDevice, s));
    return LLSR_OK;
  };
  if (imu) {
    if (samples && (rc = upload_guesses()) != LLSR_OK) return rc;
    k_odo_inputs_imu<<<B, 256, 0, s>>>(a);
  } else {
    k_odo_inputs<<<B, 256, 0, s>>>(a);
  }
  HIP_OK(h, hipGetLastError());
  llsr_s2s_batch sb{};
  sb.n_problems = B;
  sb.sharp = (const float*)o.sharp; sb.sharp_off = o.off;
  sb.flat = (const float*)o.flat; sb.flat_off = o.off + nb;
  sb.corner_last = (const float*)o.last_c[cur]; sb.corner_last_off = o.off + (2 + cur) * nb;
  sb.surf_last = (const float*)o.last_s[cur]; sb.surf_last_off = o.off + (4 + cur) * nb;
  sb.transform_cur = o.tcur;
  sb.is_degenerate = o.deg;
  sb.report = o.report;
  // the LM instantiation follows this batch's clouds, not the (high-water) reserve
  rc = s2s_launch(h, &sb, s, std::max(std::max(mMs, mF), 1), std::max(mNc, 1));
  if (rc != LLSR_OK) return rc;
  // evaluated while the LM runs: only k_odo_finish reads the guesses
  if (samples && !imu && (rc = upload_guesses()) != LLSR_OK) return rc;
  if (imu) k_odo_finish_imu<<<B, 256, 0, s>>>(a, h->imu.d_carry);
  else k_odo_finish<<<B, 256, 0, s>>>(a);
  HIP_OK(h, hipGetLastError());
  HIP_OK(h, hipEventRecord(h->last_done, s));
  h->last_rec = true;
  o.cur = nxt;
  h->last_stream = s;
  return LLSR_OK;
}

extern "C" int32_t llsr_odometry_batch(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets, int32_t B,
                                       void* hip_stream) {
  if (!h) return LLSR_EINVAL;
  if (h->cfg.mode != LLSR_MODE_LM_APPLIED)
    return fail(h, LLSR_ENOSYS, "odometry needs LLSR_MODE_LM_APPLIED: faithful mode overwrites transformCur "
                                "from the /odom2 topic (updateInitialGuess, FA:2790), which has no input here "
                                "(llsr_odometry_batch_odom takes it)");
  return odo_batch(h, d_xyzi, d_offsets, B, nullptr, nullptr, hip_stream);
}

extern "C" int32_t llsr_odometry_batch_odom(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets, int32_t B,
                                            const llsr_odom_sample* samples, const uint8_t* overwrite,
                                            void* hip_stream) {
  if (!h) return LLSR_EINVAL;
  if (!samples) return fail(h, LLSR_EINVAL, "llsr_odometry_batch_odom: samples is NULL");
  return odo_batch(h, d_xyzi, d_offsets, B, samples, overwrite, hip_stream);
}

extern "C" int32_t llsr_odometry_fetch_lm(llsr_handle* h, int32_t b, float* transform_lm) {
  if (!h || !transform_lm) return LLSR_EINVAL;
  auto& o = h->odo;
  if (!o.pool) return fail(h, LLSR_EINVAL, "llsr_odometry_batch not called");
  if (b < 0 || b >= o.B) return fail(h, LLSR_ERANGE, "slot outside [0, max_batch)");
  int32_t rc = sync_last(h);
  if (rc) return rc;
  HIP_OK(h, d2h(transform_lm, o.tlm + 6 * b, 6));
  return LLSR_OK;
}

extern "C" int32_t llsr_odometry_fetch(llsr_handle* h, int32_t b, llsr_odom_slot* out, float* corner_last,
                                       float* surf_last, float* corner_scan, float* surf_scan) {
  if (!h || !out) return LLSR_EINVAL;
  auto& o = h->odo;
  if (!o.pool) return fail(h, LLSR_EINVAL, "llsr_odometry_batch not called");
  if (b < 0 || b >= o.B) return fail(h, LLSR_ERANGE, "slot outside [0, max_batch)");
  int32_t rc = sync_last(h);
  if (rc) return rc;
  rc = llsr_scan2scan_check(h);
  if (rc) return rc;
  const int nb = o.B + 1;
  const int cur = o.cur;
  const int64_t* hlc = o.h_off + (2 + cur) * nb;
  const int64_t* hls = o.h_off + (4 + cur) * nb;
  std::memset(out, 0, sizeof *out);
  HIP_OK(h, d2h(&out->frames, o.frames + b, 1));
  HIP_OK(h, d2h(out->transform_cur, o.tcur + 6 * b, 6));
  HIP_OK(h, d2h(out->transform_sum, o.tsum + 6 * b, 6));
  HIP_OK(h, d2h(&out->lm, o.report + b, 1));
  out->n_corner_last = (int)(hlc[b + 1] - hlc[b]);
  out->n_surf_last = (int)(hls[b + 1] - hls[b]);
  const bool scans = out->frames > 1;  // the first scan of a slot publishes no scan clouds
  out->n_corner_scan = scans ? (int)(o.h_off[b + 1] - o.h_off[b]) : 0;
  out->n_surf_scan = scans ? (int)(o.h_off[nb + b + 1] - o.h_off[nb + b]) : 0;
  HIP_OK(h, d2h(corner_last, (const float*)(o.last_c[cur] + hlc[b]), 4 * (size_t)out->n_corner_last));
  HIP_OK(h, d2h(surf_last, (const float*)(o.last_s[cur] + hls[b]), 4 * (size_t)out->n_surf_last));
  HIP_OK(h, d2h(corner_scan, (const float*)(o.scan_c + o.h_off[b]), 4 * (size_t)out->n_corner_scan));
  HIP_OK(h, d2h(surf_scan, (const float*)(o.scan_s + o.h_off[nb + b]), 4 * (size_t)out->n_surf_scan));
  return LLSR_OK;
}
