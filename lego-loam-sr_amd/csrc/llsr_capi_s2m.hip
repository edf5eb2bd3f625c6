// llsr_capi_s2m.hip — C-ABI host side of scan-to-map (MapOptimization::scan2MapOptimization,
// MO:1572-1610; kernels in llsr_mo.hip): reserve, the batch, the split-correspondence batch and the
// single-problem call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "llsr_handle.h"

using namespace llsr;

extern "C" int32_t llsr_scan2map_reserve(llsr_handle* h, int32_t P, int32_t mc, int32_t ms, int32_t qc,
                                         int32_t qs) {
  if (!h) return LLSR_EINVAL;
  if (P < 1 || mc < 0 || ms < 0 || qc < 0 || qs < 0 || mc > (1 << 26) || ms > (1 << 26) ||
      qc > (1 << 20) || qs > (1 << 20))  // the solving block keeps the per-block row prefix in LDS
    return fail(h, LLSR_EINVAL, "scan2map capacities out of range");
  HIP_OK(h, hipSetDevice(h->device));
  if (h->mo.pool && P <= h->mo.P && mc <= h->mo.mc && ms <= h->mo.ms && qc <= h->mo.qc && qs <= h->mo.qs)
    return LLSR_OK;
  if (h->mo.pool) HIP_OK(h, sync_handle_streams(h));
  return llsr_host::rebuild(h->mo, [&](llsr_handle::S2M& m) -> int32_t {
    m.P = P; m.mc = mc; m.ms = ms; m.qc = qc; m.qs = qs;
    m.log2T_c = grid_log2_table(mc);
    m.log2T_s = grid_log2_table(ms);
    m.blocks_c = (qc + 255) / 256;
    m.blocks = m.blocks_c + (qs + 255) / 256;
    if (m.blocks == 0) m.blocks = 1;  // one (empty) block still runs each iteration's solve
    // Eigen's GEMM depth blocks of up to qc + qs rows: kc >= 344 once k exceeds max_kc = 680
    // (llsr_eigen::gemm_kc), so at most ceil(N / 344) blocks; k_s2m_solve keeps 64 in LDS
    const long long n_rows = (long long)qc + qs;
    const int spill_cap = std::max(0, (int)((n_rows + 343) / 344) - 64);
    S2MArgs& a = m.a;
    a.solve_rows = (kSolveLds - 4 * ((m.blocks + 4) & ~3)) / 32;
    if (a.solve_rows < 256)
      return fail(h, LLSR_EINVAL, "scan2map: too many query blocks for the solve kernel's LDS");
    if (hipFuncSetAttribute((const void*)k_s2m_solve, hipFuncAttributeMaxDynamicSharedMemorySize, kSolveLds) !=
        hipSuccess)
      return fail(h, LLSR_ENODEV, "k_s2m_solve LDS attribute");
    int32_t rc = lm_aux(h, h->mo_aux);
    if (rc != LLSR_OK) return rc;
    const llsr_host::S2MDims dims{P, mc, ms, m.log2T_c, m.log2T_s, m.blocks, spill_cap};
    if (llsr_host::alloc_pool(m.pool, 4096, [&](llsr_host::Carver& c) { llsr_host::s2m_layout(c, a, dims); }) !=
        hipSuccess)
      return fail(h, LLSR_ENOMEM, "scan2map buffers");
    a.error = a.n_active + 1;
    a.spill_cap = spill_cap;
    a.cap_qc = qc; a.cap_qs = qs; a.cap_mc = mc; a.cap_ms = ms;
    a.blocks_c = m.blocks_c;
    a.blocks = m.blocks;
    return LLSR_OK;
  });
}

// Validate a scan-to-map batch and enqueue the per-problem setup and both cell-grid builds.
static int32_t s2m_prepare(llsr_handle* h, const llsr_s2m_batch* b, hipStream_t s, S2MArgs& a,
                           const S2MOpts& opt = S2MOpts{}) {
  auto& m = h->mo;
  if (!m.pool) return fail(h, LLSR_EINVAL, "llsr_scan2map_reserve not called");
  const int P = b->n_problems;
  if (P < 1 || P > m.P) return fail(h, LLSR_ERANGE, "n_problems outside [1, reserved]");
  if (!b->corner_q_off || !b->surf_q_off || !b->corner_map_off || !b->surf_map_off || !b->pose || !b->report)
    return fail(h, LLSR_EINVAL, "null batch array");
  a = m.a;
  a.P = P;
  a.applied = (opt.mode >= 0 ? opt.mode : h->cfg.mode) == LLSR_MODE_LM_APPLIED;
  a.deg_in = opt.deg_in; a.matP_in = opt.matP_in;
  a.deg_out = opt.deg_out; a.matP_out = opt.matP_out;
  a.iter_max = h->cfg.iterCountThres;
#ifdef LLSR_S2S_PROF
  {  // diagnostics build only: k_s2m_solve stops after stage LLSR_S2M_DBG (scripts/)
    const char* dbg = std::getenv("LLSR_S2M_DBG");
    a.dbg = dbg ? std::atoi(dbg) : 0;
  }
#else
  a.dbg = 0;
#endif
  a.step_size = h->cfg.step_size;
  a.stop_thres = h->cfg.stop_thres;
  a.cq = b->corner_q; a.cq_off = b->corner_q_off;
  a.sq = b->surf_q; a.sq_off = b->surf_q_off;
  a.cm = b->corner_map; a.cm_off = b->corner_map_off;
  a.sm = b->surf_map; a.sm_off = b->surf_map_off;
  a.pose = b->pose;
  a.report = b->report;
  a.rank = 0;
  a.world = 1;
  a.ne = nullptr;
  HIP_OK(h, hipMemsetAsync(a.n_active, 0, 2 * sizeof(int), s));
  a.grids.P = P;
  a.grids.g[0].src = reinterpret_cast<const float4*>(b->corner_map);
  a.grids.g[0].off = b->corner_map_off;
  a.grids.g[1].src = reinterpret_cast<const float4*>(b->surf_map);
  a.grids.g[1].off = b->surf_map_off;
  k_s2m_setup<<<(P + 63) / 64, 64, 0, s>>>(a);
  grid_build(a.grids, s);
  HIP_OK(h, hipGetLastError());
  return LLSR_OK;
}

int32_t s2m_batch(llsr_handle* h, const llsr_s2m_batch* b, hipStream_t s, const S2MOpts& opt) {
  auto& m = h->mo;
  const LmAux& x = h->mo_aux;
  if (h->profiling && m.pool) HIP_OK(h, hipEventRecord(x.p0, s));
  S2MArgs a{};
  m.sh_live = false;  // one scan-to-map batch per handle at a time: this one replaces a shard batch
  // the scan-to-map buffers are the handle's: start after its previous scan-to-map work (any stream)
  if (h->mo_rec) HIP_OK(h, hipStreamWaitEvent(s, h->mo_done, 0));
  int32_t rc = s2m_prepare(h, b, s, a, opt);
  h->mo_rec = true;
  HIP_OK(h, hipEventRecord(h->mo_done, s));
  if (rc != LLSR_OK) return rc;
  const int P = a.P;
  if (h->profiling) HIP_OK(h, hipEventRecord(x.p1, s));
  // LM iterations; the host reads the active count every `poll` launch pairs (converged problems
  // leave their workgroups at the first instruction, so launches past convergence cost little):
  // 4 for lm_applied's few iterations, 16 for faithful's 200 (13 host round trips instead of 50)
  const int poll = a.iter_max >= 64 ? 16 : 4;
  int launches = 0;
  for (int it = 0; it < a.iter_max;) {
    const int n = (a.iter_max - it) < poll ? (a.iter_max - it) : poll;
    for (int k = 0; k < n; ++k) {
      k_s2m_iter<<<8 * ((P + 7) / 8) * m.blocks, 256, 0, s>>>(a);  // XCD-aware (llsr_mo.hip)
      k_s2m_solve<<<P, 256, kSolveLds, s>>>(a);
    }
    it += n;
    launches += n;
    HIP_OK(h, hipGetLastError());
    HIP_OK(h, hipMemcpyAsync(x.flags, a.n_active, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_OK(h, hipStreamSynchronize(s));
    if (x.flags[1]) return fail(h, LLSR_ERANGE, "a scan2map cloud exceeds the reserved capacity or has bad offsets");
    if (x.flags[0] == 0) break;
  }
  if (h->profiling) HIP_OK(h, hipEventRecord(x.p2, s));
  k_s2m_finish<<<(P + 63) / 64, 64, 0, s>>>(a);
  HIP_OK(h, hipGetLastError());
  HIP_OK(h, hipEventRecord(h->mo_done, s));
  if (h->profiling) {
    float g = 0.f, it = 0.f;
    HIP_OK(h, hipEventSynchronize(x.p2));
    HIP_OK(h, hipEventElapsedTime(&g, x.p0, x.p1));
    HIP_OK(h, hipEventElapsedTime(&it, x.p1, x.p2));
    h->mo_stats.batches += 1;
    h->mo_stats.iteration_launches += launches;
    h->mo_stats.grid_ms += g;
    h->mo_stats.iterate_ms += it;
  }
  return LLSR_OK;
}

extern "C" int32_t llsr_scan2map_batch(llsr_handle* h, const llsr_s2m_batch* b, void* hip_stream) {
  if (!h || !b) return fail(h, LLSR_EINVAL, "null argument");
  hipStream_t s;
  HIP_OK(h, enter(h, hip_stream, &s));
  return s2m_batch(h, b, s, S2MOpts{});
}

// ---- split-correspondence scan-to-map (llsr_scan2map_shard_*): the LM loop is the caller's,
// so the per-problem normal equations can be all-reduced across GPUs between the Jacobian build
// (llsr_scan2map_shard_partial) and the solve (llsr_scan2map_shard_step).

extern "C" int32_t llsr_scan2map_shard_begin(llsr_handle* h, const llsr_s2m_batch* b, void* hip_stream) {
  if (!h || !b) return fail(h, LLSR_EINVAL, "null argument");
  hipStream_t s;
  HIP_OK(h, enter(h, hip_stream, &s));
  auto& m = h->mo;
  m.sh_live = false;
  if (h->mo_rec) HIP_OK(h, hipStreamWaitEvent(s, h->mo_done, 0));
  int32_t rc = s2m_prepare(h, b, s, m.sh);
  h->mo_rec = true;
  HIP_OK(h, hipEventRecord(h->mo_done, s));
  if (rc != LLSR_OK) return rc;
  m.sh_live = true;
  return LLSR_OK;
}

extern "C" int32_t llsr_scan2map_shard_partial(llsr_handle* h, int32_t rank, int32_t world, int64_t* d_ne,
                                               void* hip_stream) {
  if (!h || !d_ne) return fail(h, LLSR_EINVAL, "null argument");
  auto& m = h->mo;
  if (!m.sh_live) return fail(h, LLSR_EINVAL, "llsr_scan2map_shard_begin not called");
  if (world < 1 || rank < 0 || rank >= world) return fail(h, LLSR_EINVAL, "rank outside [0, world)");
  hipStream_t s;
  HIP_OK(h, enter(h, hip_stream, &s));
  S2MArgs a = m.sh;
  a.rank = rank;
  a.world = world;
  a.ne = reinterpret_cast<long long*>(d_ne);
  HIP_OK(h, hipStreamWaitEvent(s, h->mo_done, 0));
  HIP_OK(h, hipMemsetAsync(d_ne, 0, sizeof(int64_t) * LLSR_NE_WORDS * (size_t)a.P, s));
  const int bs = m.blocks - m.blocks_c;
  const int nb = (m.blocks_c + world - 1) / world + (bs + world - 1) / world;
  if (nb > 0) k_s2m_iter_fx<<<8 * ((a.P + 7) / 8) * nb, 256, 0, s>>>(a, nb);  // XCD-aware (llsr_mo.hip)
  HIP_OK(h, hipGetLastError());
  HIP_OK(h, hipEventRecord(h->mo_done, s));
  return LLSR_OK;
}

extern "C" int32_t llsr_scan2map_shard_step(llsr_handle* h, const int64_t* d_ne, int32_t* n_active,
                                            void* hip_stream) {
  if (!h || !d_ne) return fail(h, LLSR_EINVAL, "null argument");
  auto& m = h->mo;
  const LmAux& x = h->mo_aux;
  if (!m.sh_live) return fail(h, LLSR_EINVAL, "llsr_scan2map_shard_begin not called");
  hipStream_t s;
  HIP_OK(h, enter(h, hip_stream, &s));
  S2MArgs a = m.sh;
  a.ne = const_cast<long long*>(reinterpret_cast<const long long*>(d_ne));
  HIP_OK(h, hipStreamWaitEvent(s, h->mo_done, 0));
  k_s2m_solve_fx<<<(a.P + 63) / 64, 64, 0, s>>>(a);
  HIP_OK(h, hipGetLastError());
  HIP_OK(h, hipEventRecord(h->mo_done, s));
  if (n_active) {
    HIP_OK(h, hipMemcpyAsync(x.flags, a.n_active, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_OK(h, hipStreamSynchronize(s));
    if (x.flags[1] & 1) return fail(h, LLSR_ERANGE, "a scan2map cloud exceeds the reserved capacity or has bad offsets");
    if (x.flags[1] & 2)
      return fail(h, LLSR_ERANGE, "a normal-equation term is non-finite or outside the fixed-point range (|v| >= 2^32)");
    *n_active = x.flags[0];
  }
  return LLSR_OK;
}

extern "C" int32_t llsr_scan2map_shard_end(llsr_handle* h, void* hip_stream) {
  if (!h) return LLSR_EINVAL;
  auto& m = h->mo;
  if (!m.sh_live) return fail(h, LLSR_EINVAL, "llsr_scan2map_shard_begin not called");
  hipStream_t s;
  HIP_OK(h, enter(h, hip_stream, &s));
  HIP_OK(h, hipStreamWaitEvent(s, h->mo_done, 0));
  k_s2m_finish<<<(m.sh.P + 63) / 64, 64, 0, s>>>(m.sh);
  HIP_OK(h, hipGetLastError());
  HIP_OK(h, hipEventRecord(h->mo_done, s));
  m.sh_live = false;
  return LLSR_OK;
}

extern "C" int32_t llsr_scan2map_stats(llsr_handle* h, llsr_s2m_stats* out) {
  if (!h || !out) return LLSR_EINVAL;
  *out = h->mo_stats;
  return LLSR_OK;
}

extern "C" int32_t llsr_scan2map(llsr_handle* h, const float* cq, int32_t Qc, const float* sq, int32_t Qs,
                                 const float* cm, int32_t Mc, const float* sm, int32_t Ms, float* pose,
                                 llsr_lm_report* rep) {
  if (!h || !pose || !rep || Qc < 0 || Qs < 0 || Mc < 0 || Ms < 0) return fail(h, LLSR_EINVAL, "bad argument");
  if ((Qc && !cq) || (Qs && !sq) || (Mc && !cm) || (Ms && !sm)) return fail(h, LLSR_EINVAL, "null cloud");
  auto& m = h->mo;
  const int P = m.pool ? m.P : 1;
  int32_t rc = llsr_scan2map_reserve(h, P, Mc > m.mc ? Mc : m.mc, Ms > m.ms ? Ms : m.ms,
                                     Qc > m.qc ? Qc : m.qc, Qs > m.qs ? Qs : m.qs);
  if (rc != LLSR_OK) return rc;
  OneShotStage& st = h->mo_stage;
  const float* const src[4] = {cq, sq, cm, sm};
  const int32_t n[4] = {Qc, Qs, Mc, Ms};
  rc = stage_oneshot(h, st, src, n, pose, false, sizeof(llsr_lm_report));
  if (rc != LLSR_OK) return rc;
  llsr_lm_report* d_rep = reinterpret_cast<llsr_lm_report*>(st.rep);
  hipStream_t s = h->stream;
  llsr_s2m_batch b{};
  b.n_problems = 1;
  b.corner_q = (const float*)st.cloud[0]; b.corner_q_off = st.off;
  b.surf_q = (const float*)st.cloud[1]; b.surf_q_off = st.off + 2;
  b.corner_map = (const float*)st.cloud[2]; b.corner_map_off = st.off + 4;
  b.surf_map = (const float*)st.cloud[3]; b.surf_map_off = st.off + 6;
  b.pose = st.pose;
  b.report = d_rep;
  const LmAux& x = h->mo_aux;
  HIP_OK(h, hipEventRecord(x.e0, s));
  rc = llsr_scan2map_batch(h, &b, s);
  if (rc != LLSR_OK) return rc;
  HIP_OK(h, hipEventRecord(x.e1, s));
  HIP_OK(h, hipMemcpyAsync(rep, d_rep, sizeof *rep, hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipMemcpyAsync(pose, st.pose, 6 * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipStreamSynchronize(s));
  float ms_ = 0.f;
  HIP_OK(h, hipEventElapsedTime(&ms_, x.e0, x.e1));
  rep->ms = ms_;
  return LLSR_OK;
}
