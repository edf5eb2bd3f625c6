// llsr_capi_s2s.hip — C-ABI host side of scan-to-scan (FeatureAssociation::updateTransformation,
// FA:2505-2535; kernels in llsr_fa_lm.hip): the shadow points, reserve, the batch launch, the
// deferred capacity check and the single-problem call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "llsr_handle.h"

using namespace llsr;

extern "C" int32_t llsr_shadow_points(float* out) {
  // GenerateShadowPoint (FA:412-439) with lidar_to_body_centor = (0.008, 0, -0.035) (FA:300),
  // row_size 16, col_size 10 (FA:301); computed on the host with the same libm as the reference.
  if (!out) return LLSR_EINVAL;
  const double c0 = 0.008, c1 = 0.0, c2 = -0.035;
  const int row_size = 16, col_size = 10;
  const double row_angle = (std::atan2(0.120, 0.05) * 2) / (row_size - 1);
  const double col_angle = (std::atan2(0.077, 0.05) * 2) / (col_size - 1);
  int k = 0;
  for (int row = 0; row < row_size; row++) {
    const float row_x = (float)(0.05 * std::tan((((row_size - 1.0) / 2.0) * row_angle) - (row * row_angle)));
    for (int col = 0; col < col_size; col++) {
      const float col_y = (float)(0.05 * std::tan((((col_size - 1.0) / 2.0) * col_angle) - (col * col_angle)));
      out[4 * k + 0] = (float)(col_y + c1);
      out[4 * k + 1] = (float)(-(0.035f + 0.05f) + c2);
      out[4 * k + 2] = (float)(row_x + c0);
      out[4 * k + 3] = (float)((double)((float)row + (float)17) + (double)(float)col / 10000.0);
      ++k;
    }
  }
  return LLSR_OK;
}

extern "C" int32_t llsr_scan2scan_reserve(llsr_handle* h, int32_t P, int32_t ms, int32_t f, int32_t nc, int32_t ns) {
  if (!h) return LLSR_EINVAL;
  if (P < 1 || ms < 0 || f < 0 || nc < 0 || ns < 0 || ms > (1 << 24) || f > (1 << 24) || nc > (1 << 24) || ns > (1 << 24))
    return fail(h, LLSR_EINVAL, "scan2scan capacities out of range");
  HIP_OK(h, hipSetDevice(h->device));
  if (h->s2s.pool && P <= h->s2s.P && ms <= h->s2s.ms && f <= h->s2s.f && nc <= h->s2s.nc && ns <= h->s2s.ns)
    return LLSR_OK;
  if (h->s2s.pool) HIP_OK(h, sync_handle_streams(h));
  return llsr_host::rebuild(h->s2s, [&](llsr_handle::S2S& m) -> int32_t {
    m.P = P; m.ms = ms; m.f = f; m.nc = nc; m.ns = ns;
    int32_t rc = lm_aux(h, h->s2s_aux);
    if (rc != LLSR_OK) return rc;
    S2SArgs& a = m.a;
    const llsr_host::S2SDims dims{P, ms, f, nc, ns, grid_log2_table(nc), grid_log2_table(ns)};
    if (llsr_host::alloc_pool(m.pool, 64, [&](llsr_host::Carver& c) { llsr_host::s2s_layout(c, a, dims); }) !=
        hipSuccess)
      return fail(h, LLSR_ENOMEM, "scan2scan buffers");
    a.cap_sharp = ms;
    a.cap_flat = f;
    HIP_OK(h, hipMemset(a.error, 0, sizeof(int)));
    return LLSR_OK;
  });
}

int32_t s2s_launch(llsr_handle* h, const llsr_s2s_batch* b, void* hip_stream, int hint_q, int hint_nc) {
  if (!h || !b) return fail(h, LLSR_EINVAL, "null argument");
  auto& m = h->s2s;
  const LmAux& x = h->s2s_aux;
  if (!m.pool) return fail(h, LLSR_EINVAL, "llsr_scan2scan_reserve not called");
  const int P = b->n_problems;
  if (P < 1 || P > m.P) return fail(h, LLSR_ERANGE, "n_problems outside [1, reserved]");
  if (!b->sharp_off || !b->flat_off || !b->corner_last_off || !b->surf_last_off || !b->transform_cur ||
      !b->is_degenerate || !b->report)
    return fail(h, LLSR_EINVAL, "null batch array");
  hipStream_t s;
  HIP_OK(h, enter(h, hip_stream, &s));
  S2SArgs a = m.a;
  a.P = P;
  a.dist_sqr = h->cfg.nearest_feature_search_distance * h->cfg.nearest_feature_search_distance;  // FA:152
  a.sharp = reinterpret_cast<const float4*>(b->sharp); a.sharp_off = b->sharp_off;
  a.flat = reinterpret_cast<const float4*>(b->flat); a.flat_off = b->flat_off;
  a.grids.P = P;
  a.grids.g[0].src = reinterpret_cast<const float4*>(b->corner_last);
  a.grids.g[0].off = b->corner_last_off;
  a.grids.g[1].src = reinterpret_cast<const float4*>(b->surf_last);
  a.grids.g[1].off = b->surf_last_off;
  a.tcur = b->transform_cur;
  a.degen = b->is_degenerate;
  a.report = b->report;
  if (h->s2s_rec) HIP_OK(h, hipStreamWaitEvent(s, h->s2s_done, 0));  // shared buffers: after the last batch
  if (h->profiling) HIP_OK(h, hipEventRecord(x.p0, s));
  grid_build(a.grids, s);
  {
    const int nb = (m.ns + 7) / 8;
    if (nb > 0) k_s2s_boxes<<<dim3((nb + 255) / 256, P), 256, 0, s>>>(a);
  }
  if (h->profiling) HIP_OK(h, hipEventRecord(x.p1, s));
  // the small-LDS instantiation (4 workgroups per CU instead of 2) when every problem's queries
  // and corner-last cloud fit it (reserved capacities are the batch maxima)
  // bounds: this launch's largest clouds when the caller knows them (the odometry chain), else
  // the reserved capacities
  const int bq = hint_q > 0 ? hint_q : std::max(m.ms, m.f);
  const int bnc = hint_nc > 0 ? hint_nc : m.nc;
  if (bq <= 1024 && bnc <= 1024) {
    s2s_lm_launch<1024, 1024, 256>(P, s, a);
    h->s2s_last_variant = 1024;
  } else if (bq <= 2560 && bnc <= 1536) {
    s2s_lm_launch<2560, 1536, 512>(P, s, a);
    h->s2s_last_variant = 2560;
  } else {
    s2s_lm_launch<2048, 2048, 512>(P, s, a);
    h->s2s_last_variant = 2048;
  }
  HIP_OK(h, hipGetLastError());
  HIP_OK(h, hipEventRecord(h->s2s_done, s));
  h->s2s_rec = true;
  if (h->profiling) {
    float g = 0.f, lm = 0.f;
    HIP_OK(h, hipEventRecord(x.p2, s));
    HIP_OK(h, hipEventSynchronize(x.p2));
    HIP_OK(h, hipEventElapsedTime(&g, x.p0, x.p1));
    HIP_OK(h, hipEventElapsedTime(&lm, x.p1, x.p2));
    h->s2s_stats.batches += 1;
    h->s2s_stats.grid_ms += g;
    h->s2s_stats.lm_ms += lm;
  }
  return LLSR_OK;
}

extern "C" int32_t llsr_scan2scan_batch(llsr_handle* h, const llsr_s2s_batch* b, void* hip_stream) {
  return s2s_launch(h, b, hip_stream, 0, 0);
}

// Diagnostics (not part of the ABI header): the LDS rows (1024, 2560 or 2048) of the k_s2s_lm
// instantiation the last scan-to-scan launch of this handle used, 0 before any; the two large ones
// run the whole-wave surf walks (tests/test_gpu_fa_lm.py asserts which one a test exercised).
extern "C" int32_t llsr_debug_s2s_variant(llsr_handle* h) { return h ? h->s2s_last_variant : -1; }

// Diagnostics (not part of the ABI header): the diagnostics build's per-problem phase ticks of the
// last scan-to-scan launch (k_s2s_lm, LLSR_S2S_PROF: knn surf / corner, A rows, B sums, C solve,
// corner / surf walks, whole kernel, 100 MHz; [7] the shell fallback queries), [P][8] into out.
// Synchronises. The product build leaves the buffer unwritten.
extern "C" int32_t llsr_debug_s2s_prof(llsr_handle* h, float* out, int32_t cap) {
  if (!h || !out || cap < 0) return LLSR_EINVAL;
  auto& m = h->s2s;
  if (!m.pool) return fail(h, LLSR_EINVAL, "no scan-to-scan batch");
  HIP_OK(h, hipSetDevice(h->device));
  HIP_OK(h, sync_handle_streams(h));
  const int n = cap < m.P ? cap : m.P;
  HIP_OK(h, hipMemcpy(out, m.a.prof, sizeof(float) * 8 * (size_t)n, hipMemcpyDeviceToHost));
  return n;
}

extern "C" int32_t llsr_scan2scan_stats(llsr_handle* h, llsr_s2s_stats* out) {
  if (!h || !out) return LLSR_EINVAL;
  *out = h->s2s_stats;
  return LLSR_OK;
}

extern "C" int32_t llsr_scan2scan_check(llsr_handle* h) {
  if (!h) return LLSR_EINVAL;
  auto& m = h->s2s;
  const LmAux& x = h->s2s_aux;
  if (!m.pool) return LLSR_OK;
  HIP_OK(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;  // the handle's stream, after the last scan-to-scan batch
  if (h->s2s_rec) HIP_OK(h, hipStreamWaitEvent(s, h->s2s_done, 0));
  HIP_OK(h, hipMemcpyAsync(x.flags, m.a.error, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipStreamSynchronize(s));
  if (*x.flags) {
    HIP_OK(h, hipMemsetAsync(m.a.error, 0, sizeof(int), s));
    HIP_OK(h, hipStreamSynchronize(s));
    return fail(h, LLSR_ERANGE, "a scan2scan cloud exceeds the reserved capacity or has bad offsets");
  }
  return LLSR_OK;
}

extern "C" int32_t llsr_scan2scan(llsr_handle* h, const float* sharp, int32_t Ms, const float* flat, int32_t F,
                                  const float* cl, int32_t Nc, const float* sl, int32_t Ns, float* tcur,
                                  int32_t* degen, llsr_s2s_report* rep) {
  if (!h || !tcur || !degen || !rep || Ms < 0 || F < 0 || Nc < 0 || Ns < 0) return fail(h, LLSR_EINVAL, "bad argument");
  if ((Ms && !sharp) || (F && !flat) || (Nc && !cl) || (Ns && !sl)) return fail(h, LLSR_EINVAL, "null cloud");
  auto& m = h->s2s;
  const int P = m.pool ? m.P : 1;
  int32_t rc = llsr_scan2scan_reserve(h, P, Ms > m.ms ? Ms : m.ms, F > m.f ? F : m.f, Nc > m.nc ? Nc : m.nc,
                                      Ns > m.ns ? Ns : m.ns);
  if (rc != LLSR_OK) return rc;
  OneShotStage& st = h->s2s_stage;
  const float* const src[4] = {sharp, flat, cl, sl};
  const int32_t n[4] = {Ms, F, Nc, Ns};
  rc = stage_oneshot(h, st, src, n, tcur, true, sizeof(llsr_s2s_report));
  if (rc != LLSR_OK) return rc;
  llsr_s2s_report* d_rep = reinterpret_cast<llsr_s2s_report*>(st.rep);
  hipStream_t s = h->stream;
  HIP_OK(h, hipMemcpyAsync(st.deg, degen, sizeof(int), hipMemcpyHostToDevice, s));
  llsr_s2s_batch b{};
  b.n_problems = 1;
  b.sharp = (const float*)st.cloud[0]; b.sharp_off = st.off;
  b.flat = (const float*)st.cloud[1]; b.flat_off = st.off + 2;
  b.corner_last = (const float*)st.cloud[2]; b.corner_last_off = st.off + 4;
  b.surf_last = (const float*)st.cloud[3]; b.surf_last_off = st.off + 6;
  b.transform_cur = st.pose;
  b.is_degenerate = st.deg;
  b.report = d_rep;
  const LmAux& x = h->s2s_aux;
  HIP_OK(h, hipEventRecord(x.e0, s));
  rc = llsr_scan2scan_batch(h, &b, s);
  if (rc != LLSR_OK) return rc;
  HIP_OK(h, hipEventRecord(x.e1, s));
  HIP_OK(h, hipMemcpyAsync(rep, d_rep, sizeof *rep, hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipMemcpyAsync(tcur, st.pose, 6 * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipMemcpyAsync(degen, st.deg, sizeof(int), hipMemcpyDeviceToHost, s));
  rc = llsr_scan2scan_check(h);
  if (rc != LLSR_OK) return rc;
  float ms_ = 0.f;
  HIP_OK(h, hipEventElapsedTime(&ms_, x.e0, x.e1));
  rep->ms = ms_;
  return LLSR_OK;
}
