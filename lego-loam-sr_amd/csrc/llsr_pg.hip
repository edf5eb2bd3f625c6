// llsr_pg.hip — the batched pose-graph optimiser's kernels and host driver (bodies in
// llsr_pg.h). The graphs are built on the host (append, add_loop: a few dozen double operations per
// pose through the same LLSR_HD bodies the device runs); llsr_pg_optimize copies the problems that
// have a new loop factor into the workspace, runs the Gauss-Newton loop there — five launches per pass
// covering every problem, the host reading one word per pass — and copies the poses that moved back.
// With hip_device == LLSR_PG_HOST the workspace is heap memory of the same sizes and every launch is
// pg_pass_host's loops.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/llsr.h"
#include "llsr_pg.h"

namespace llsr_pgo {
__global__ __launch_bounds__(kBlock) void k_pg_linearize(PgArgs a) {
  pg_linearize_thread(a, blockIdx.x, blockIdx.y, threadIdx.x);
}
__global__ __launch_bounds__(kBlock) void k_pg_error(PgArgs a) { pg_error_thread(a, blockIdx.x, threadIdx.x); }
__global__ __launch_bounds__(kBlock) void k_pg_assemble(PgArgs a) {
  pg_assemble_thread(a, blockIdx.x, blockIdx.y, threadIdx.x);
}
__global__ __launch_bounds__(kBlock) void k_pg_update(PgArgs a) {
  pg_update_thread(a, blockIdx.x, blockIdx.y, threadIdx.x);
}
// One wave per problem, sequential over the scalar columns of its block rows; the barrier orders the
// wave's global writes of one phase before the reads of the next (pg_solve_host is the same sequence).
__global__ __launch_bounds__(kBlock) void k_pg_solve(PgArgs a) {
  const int p = blockIdx.x, lane = threadIdx.x;
  if (!pg_running(a, p)) return;
  const int n = 6 * a.prob[p].K;
  for (int j = 0; j < n; ++j) {
    pg_solve_diag_lane(a, p, j, lane);
    __syncthreads();
    if (a.st[p].state != kRun) return;  // a broken pivot: the same word for every lane
    pg_solve_col_lane(a, p, j, lane);
    __syncthreads();
  }
  for (int k = n - 1; k >= 0; --k) {
    pg_back_diag_lane(a, p, k, lane);
    __syncthreads();
    pg_back_col_lane(a, p, k, lane);
    __syncthreads();
  }
}
}  // namespace llsr_pgo

using namespace llsr_pgo;

struct llsr_pg {
  int device = LLSR_PG_HOST;
  int P = 0, maxK = 0, maxL = 0;
  int64_t maxE = 0;
  std::string err;
  // the graphs (host): counts, the estimate in the store's layout and as matrices, the measurements
  // of the prior / odometry factors by pose and of the loop factors, the loops' 1 / sigma
  std::vector<int32_t> K, L;
  std::vector<char> dirty;  // a loop factor since the last optimise
  std::vector<float> p6;    // [P maxK 6]
  std::vector<double> X;    // [P maxK 12]
  std::vector<double> Zk;   // [P maxK 12]
  std::vector<double> Zl;   // [P maxL 12]
  std::vector<double> wl;   // [P maxL]
  std::vector<int32_t> loops;  // [P maxL 2]
  // staging in the workspace's layout, rebuilt per optimise for the problems that run
  std::vector<double> sZ, sw;
  std::vector<int32_t> c0, longrow;
  std::vector<int64_t> rowoff;
  std::vector<PgProblem> prob;
  std::vector<PgState> st;
  std::vector<float> out6;
  // the workspace: device memory, or heap memory of the same sizes
  PgArgs a{};
  std::vector<void*> mem;
  int* hlive = nullptr;  // pinned (device) or heap
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
};

static int32_t pfail(llsr_pg* w, int32_t code, const std::string& msg) {
  if (w) w->err = msg;
  return code;
}
#define PG_OK(w, expr)                                                           \
  do {                                                                           \
    hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess)                                                        \
      return pfail(w, LLSR_EIO, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

template <class T>
static bool pg_alloc(llsr_pg* w, T** out, size_t n) {
  void* p = nullptr;
  const size_t bytes = (n ? n : 1) * sizeof(T);
  if (w->device == LLSR_PG_HOST) {
    p = std::malloc(bytes);
    if (p) std::memset(p, 0, bytes);
  } else if (hipMalloc(&p, bytes) != hipSuccess || hipMemset(p, 0, bytes) != hipSuccess) {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  if (!p) return false;
  w->mem.push_back(p);
  *out = static_cast<T*>(p);
  return true;
}

extern "C" void llsr_pg_destroy(llsr_pg* w) {
  if (!w) return;
  if (w->device == LLSR_PG_HOST) {
    for (void* p : w->mem) std::free(p);
    std::free(w->hlive);
  } else {
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    for (void* p : w->mem) (void)hipFree(p);
    if (w->hlive) (void)hipHostFree(w->hlive);
    for (hipEvent_t e : w->ev)
      if (e) (void)hipEventDestroy(e);
    if (w->stream) (void)hipStreamDestroy(w->stream);
  }
  delete w;
}

extern "C" llsr_pg* llsr_pg_create(int32_t dev, int32_t P, int32_t max_poses, int32_t max_loops,
                                   int64_t max_envelope_blocks) {
  // (factor and scalar indices are ints: 6 max_poses and max_poses + max_loops must fit)
  if (P < 1 || P > 65535 || max_poses < 1 || max_poses > (1 << 24) || max_loops < 0 || max_loops > (1 << 24) ||
      max_envelope_blocks < 1)
    return nullptr;
  if (dev != LLSR_PG_HOST) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || dev < 0 || dev >= count) return nullptr;
    if (hipSetDevice(dev) != hipSuccess) return nullptr;
  }
  llsr_pg* w = new (std::nothrow) llsr_pg;
  if (!w) return nullptr;
  w->device = dev;
  w->P = P; w->maxK = max_poses; w->maxL = max_loops; w->maxE = max_envelope_blocks;
  const PgSizes z = pg_sizes(P, max_poses, max_loops, max_envelope_blocks);
  try {
    w->K.assign(P, 0); w->L.assign(P, 0); w->dirty.assign(P, 0);
    w->p6.assign(z.out6, 0.0f); w->out6.assign(z.out6, 0.0f);
    w->X.assign(z.X, 0.0); w->Zk.assign(z.X, 0.0);
    w->Zl.assign(12 * z.longrow + 1, 0.0); w->wl.assign(z.longrow + 1, 0.0);
    w->loops.assign(z.loops + 1, 0);
    w->sZ.assign(z.Z, 0.0); w->sw.assign(z.winv, 0.0);
    w->c0.assign(z.c0, 0); w->longrow.assign(z.longrow + 1, 0); w->rowoff.assign(z.rowoff, 0);
    w->prob.assign(P, PgProblem{}); w->st.assign(P, PgState{});
  } catch (const std::bad_alloc&) {
    delete w;
    return nullptr;
  }
  PgArgs& a = w->a;
  a.P = P; a.maxK = max_poses; a.maxL = max_loops; a.maxE = max_envelope_blocks;
  PgProblem* prob = nullptr;
  double *Zb = nullptr, *wb = nullptr;
  int32_t *lb = nullptr, *cb = nullptr, *gb = nullptr;
  int64_t* rb = nullptr;
  bool ok = pg_alloc(w, &prob, z.prob) && pg_alloc(w, &a.st, z.st) && pg_alloc(w, &a.live, 1) &&
            pg_alloc(w, &a.X, z.X) && pg_alloc(w, &a.Xprev, z.X) && pg_alloc(w, &Zb, z.Z) &&
            pg_alloc(w, &wb, z.winv) && pg_alloc(w, &lb, z.loops) && pg_alloc(w, &cb, z.c0) &&
            pg_alloc(w, &rb, z.rowoff) && pg_alloc(w, &gb, z.longrow) && pg_alloc(w, &a.res, z.res) &&
            pg_alloc(w, &a.J, z.J) && pg_alloc(w, &a.eterm, z.eterm) && pg_alloc(w, &a.H, z.H) &&
            pg_alloc(w, &a.d, z.d) && pg_alloc(w, &a.out6, z.out6);
  a.prob = prob; a.Z = Zb; a.winv = wb; a.loops = lb; a.c0 = cb; a.rowoff = rb; a.longrow = gb;
  if (dev == LLSR_PG_HOST) {
    w->hlive = static_cast<int*>(std::malloc(sizeof(int)));
    ok = ok && w->hlive;
  } else {
    ok = ok && hipStreamCreate(&w->stream) == hipSuccess && hipHostMalloc((void**)&w->hlive, sizeof(int)) == hipSuccess;
    for (hipEvent_t& e : w->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  }
  if (!ok) {
    llsr_pg_destroy(w);
    return nullptr;
  }
  return w;
}

extern "C" const char* llsr_pg_last_error(const llsr_pg* w) { return w ? w->err.c_str() : "null graph"; }

extern "C" int32_t llsr_pg_config_default(llsr_pg_config* cfg) {
  if (!cfg) return LLSR_EINVAL;
  cfg->max_iterations = 100;  // NonlinearOptimizerParams' defaults
  cfg->pad = 0;
  cfg->relative_error_tol = 1e-5;
  cfg->absolute_error_tol = 1e-5;
  return LLSR_OK;
}

extern "C" int32_t llsr_pg_reset(llsr_pg* w, int32_t p) {
  if (!w) return LLSR_EINVAL;
  if (p < -1 || p >= w->P) return pfail(w, LLSR_EINVAL, "pg reset: problem outside [-1, P)");
  for (int q = p < 0 ? 0 : p; q < (p < 0 ? w->P : p + 1); ++q) w->K[q] = w->L[q] = w->dirty[q] = 0;
  return LLSR_OK;
}

static bool all_finite(const double* v, int n) {
  for (int k = 0; k < n; ++k)
    if (!finited(v[k])) return false;
  return true;
}
static size_t pose_at(const llsr_pg* w, int p, int k) { return (size_t)p * (size_t)w->maxK + (size_t)k; }
static size_t loop_at(const llsr_pg* w, int p, int l) { return (size_t)p * (size_t)w->maxL + (size_t)l; }

static int32_t pg_append(llsr_pg* w, int32_t p, const float* poses6, int32_t n) {
  if (p < 0 || p >= w->P || n < 0 || (n > 0 && !poses6)) return pfail(w, LLSR_EINVAL, "pg append: bad arguments");
  const int K0 = w->K[p];
  if ((int64_t)K0 + n > w->maxK) return pfail(w, LLSR_ERANGE, "pg append: more than max_poses poses");
  // every refusal comes before the first write
  std::vector<double> T(12 * (size_t)n + 1);
  for (int k = 0; k < n; ++k) {
    pose_from_store6(poses6 + 6 * (size_t)k, &T[12 * (size_t)k]);
    if (!all_finite(&T[12 * (size_t)k], 12)) return pfail(w, LLSR_EINVAL, "pg append: a pose is not finite");
  }
  if (n > 0) {
    std::vector<int32_t> c0((size_t)K0 + n);
    if (pg_envelope(K0 + n, w->L[p], &w->loops[2 * loop_at(w, p, 0)], c0.data(), nullptr, nullptr, nullptr) > w->maxE)
      return pfail(w, LLSR_ERANGE, "pg append: more than max_envelope_blocks envelope blocks");
  }
  for (int k = 0; k < n; ++k) {
    const size_t R = pose_at(w, p, K0 + k);
    const double* Tk = &T[12 * (size_t)k];
    // the prior on pose 0 is the pose itself (MO:1641-1651); a later keyframe's odometry measurement
    // is between(the estimate of the one before it now, the appended pose) (MO:1654-1664)
    if (K0 + k == 0) std::memcpy(&w->Zk[12 * R], Tk, 12 * sizeof(double));
    else pose_between(&w->X[12 * (R - 1)], Tk, &w->Zk[12 * R]);
    std::memcpy(&w->X[12 * R], Tk, 12 * sizeof(double));
    std::memcpy(&w->p6[6 * R], poses6 + 6 * (size_t)k, 6 * sizeof(float));
  }
  w->K[p] = K0 + n;
  return LLSR_OK;
}

// (the entry points' temporaries: no exception crosses the C boundary)
extern "C" int32_t llsr_pg_append(llsr_pg* w, int32_t p, const float* poses6, int32_t n) {
  if (!w) return LLSR_EINVAL;
  try {
    return pg_append(w, p, poses6, n);
  } catch (const std::bad_alloc&) {
    return pfail(w, LLSR_ENOMEM, "pg append: no memory");  // thrown before the first write
  }
}

static int32_t pg_add_loop(llsr_pg* w, int32_t p, int32_t from_id, int32_t to_id, const float* pose_from6,
                           const float* pose_to6, float variance) {
  if (p < 0 || p >= w->P || !pose_from6 || !pose_to6) return pfail(w, LLSR_EINVAL, "pg add_loop: bad arguments");
  const int K = w->K[p], L = w->L[p];
  if (from_id < 0 || from_id >= K || to_id < 0 || to_id >= K || from_id == to_id)
    return pfail(w, LLSR_EINVAL, "pg add_loop: ids must be two different poses of the graph");
  const double var = (double)variance;
  if (!(finited(var) && var > 0.0)) return pfail(w, LLSR_EINVAL, "pg add_loop: the variance must be finite and positive");
  double Tf[12], Tt[12], Z[12];
  pose_from_gtsam6(pose_from6, Tf);
  pose_from_gtsam6(pose_to6, Tt);
  if (!all_finite(Tf, 12) || !all_finite(Tt, 12)) return pfail(w, LLSR_EINVAL, "pg add_loop: a pose is not finite");
  if (L >= w->maxL) return pfail(w, LLSR_ERANGE, "pg add_loop: more than max_loops loop factors");
  int32_t* lp = &w->loops[2 * loop_at(w, p, 0)];
  {  // the envelope with the new loop, on a copy of the table
    std::vector<int32_t> all(lp, lp + 2 * (size_t)L), c0((size_t)K);
    all.push_back(from_id);
    all.push_back(to_id);
    if (pg_envelope(K, L + 1, all.data(), c0.data(), nullptr, nullptr, nullptr) > w->maxE)
      return pfail(w, LLSR_ERANGE, "pg add_loop: more than max_envelope_blocks envelope blocks");
  }
  pose_between(Tf, Tt, Z);
  lp[2 * L] = from_id;
  lp[2 * L + 1] = to_id;
  std::memcpy(&w->Zl[12 * loop_at(w, p, L)], Z, sizeof Z);
  w->wl[loop_at(w, p, L)] = 1.0 / sqrtd(var);
  w->L[p] = L + 1;
  w->dirty[p] = 1;
  return LLSR_OK;
}

extern "C" int32_t llsr_pg_add_loop(llsr_pg* w, int32_t p, int32_t from_id, int32_t to_id, const float* pose_from6,
                                    const float* pose_to6, float variance) {
  if (!w) return LLSR_EINVAL;
  try {
    return pg_add_loop(w, p, from_id, to_id, pose_from6, pose_to6, variance);
  } catch (const std::bad_alloc&) {
    return pfail(w, LLSR_ENOMEM, "pg add_loop: no memory");  // thrown before the first write
  }
}

extern "C" int32_t llsr_pg_poses(const llsr_pg* w, int32_t p, float* out6, int32_t cap) {
  if (!w || p < 0 || p >= w->P) return LLSR_EINVAL;
  const int n = w->K[p];
  if (out6 && cap > 0) std::memcpy(out6, &w->p6[6 * pose_at(w, p, 0)], sizeof(float) * 6 * (size_t)(n < cap ? n : cap));
  return n;
}

// host -> workspace / workspace -> host (ordered on s; the heap workspace copies at once)
template <class T>
static hipError_t pg_in(llsr_pg* w, const T* dst, const T* src, size_t n, hipStream_t s) {
  if (!n) return hipSuccess;
  if (w->device == LLSR_PG_HOST) {
    std::memcpy(const_cast<T*>(dst), src, n * sizeof(T));
    return hipSuccess;
  }
  return hipMemcpyAsync(const_cast<T*>(dst), src, n * sizeof(T), hipMemcpyHostToDevice, s);
}
template <class T>
static hipError_t pg_out(llsr_pg* w, T* dst, const T* src, size_t n, hipStream_t s) {
  if (!n) return hipSuccess;
  if (w->device == LLSR_PG_HOST) {
    std::memcpy(dst, src, n * sizeof(T));
    return hipSuccess;
  }
  return hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, s);
}

extern "C" int32_t llsr_pg_optimize(llsr_pg* w, const llsr_pg_config* cfg, llsr_pg_report* reps, void* hip_stream) {
  if (!w) return LLSR_EINVAL;
  llsr_pg_config own;
  if (!cfg) {
    llsr_pg_config_default(&own);
    cfg = &own;
  }
  if (!(cfg->relative_error_tol >= 0.0) || !(cfg->absolute_error_tol >= 0.0))
    return pfail(w, LLSR_EINVAL, "pg optimize: a tolerance is negative or no number");
  const bool dev = w->device != LLSR_PG_HOST;
  const auto t0 = std::chrono::steady_clock::now();
  hipStream_t s = nullptr;
  if (dev) {
    PG_OK(w, hipSetDevice(w->device));
    s = hip_stream ? static_cast<hipStream_t>(hip_stream) : w->stream;
    PG_OK(w, hipStreamSynchronize(s));  // an earlier failure may have left work queued
  }
  const int P = w->P;
  PgArgs a = w->a;
  a.max_iterations = cfg->max_iterations;
  a.rel_tol = cfg->relative_error_tol;
  a.abs_tol = cfg->absolute_error_tol;
  // 1. the tables of the problems that run
  const double wk[6] = {1.0 / sqrtd(1e-6), 1.0 / sqrtd(1e-6), 1.0 / sqrtd(1e-6),
                        1.0 / sqrtd(1e-8), 1.0 / sqrtd(1e-8), 1.0 / sqrtd(1e-6)};  // MO:1618
  int live = 0;
  for (int p = 0; p < P; ++p) {
    const int K = w->K[p], L = w->L[p];
    PgProblem& pr = w->prob[p];
    pr.K = K; pr.L = L; pr.nlong = 0;
    pr.run = w->dirty[p] ? 1 : 0;
    w->st[p] = PgState{};
    if (!pr.run) continue;
    ++live;
    w->st[p].state = kRun;
    const size_t R0 = pose_at(w, p, 0), F0 = (size_t)p * ((size_t)w->maxK + (size_t)w->maxL), L0 = loop_at(w, p, 0);
    pg_envelope(K, L, &w->loops[2 * L0], &w->c0[R0], &w->rowoff[R0], &w->longrow[L0], &pr.nlong);
    std::memcpy(&w->sZ[12 * F0], &w->Zk[12 * R0], 12 * (size_t)K * sizeof(double));
    std::memcpy(&w->sZ[12 * (F0 + K)], &w->Zl[12 * L0], 12 * (size_t)L * sizeof(double));
    for (int f = 0; f < K; ++f)
      for (int c = 0; c < 6; ++c) w->sw[6 * (F0 + f) + c] = wk[c];
    for (int l = 0; l < L; ++l)
      for (int c = 0; c < 6; ++c) w->sw[6 * (F0 + K + l) + c] = w->wl[L0 + l];
  }
  if (reps)
    for (int p = 0; p < P; ++p) {
      reps[p] = llsr_pg_report{};
      reps[p].poses = w->K[p];
      reps[p].loops = w->L[p];
    }
  if (live == 0) return LLSR_OK;
  // 2. into the workspace
  if (dev) PG_OK(w, hipEventRecord(w->ev[0], s));
  *w->hlive = live;
  PG_OK(w, pg_in(w, a.prob, w->prob.data(), (size_t)P, s));
  PG_OK(w, pg_in(w, a.st, w->st.data(), (size_t)P, s));
  PG_OK(w, pg_in(w, a.live, w->hlive, 1, s));
  for (int p = 0; p < P; ++p) {
    if (!w->prob[p].run) continue;
    const size_t K = (size_t)w->K[p], L = (size_t)w->L[p];
    const size_t R0 = pose_at(w, p, 0), F0 = (size_t)p * ((size_t)w->maxK + (size_t)w->maxL), L0 = loop_at(w, p, 0);
    PG_OK(w, pg_in(w, a.X + 12 * R0, &w->X[12 * R0], 12 * K, s));
    PG_OK(w, pg_in(w, a.Z + 12 * F0, &w->sZ[12 * F0], 12 * (K + L), s));
    PG_OK(w, pg_in(w, a.winv + 6 * F0, &w->sw[6 * F0], 6 * (K + L), s));
    PG_OK(w, pg_in(w, a.loops + 2 * L0, &w->loops[2 * L0], 2 * L, s));
    PG_OK(w, pg_in(w, a.c0 + R0, &w->c0[R0], K, s));
    PG_OK(w, pg_in(w, a.rowoff + R0, &w->rowoff[R0], K, s));
    PG_OK(w, pg_in(w, a.longrow + L0, &w->longrow[L0], (size_t)w->prob[p].nlong, s));
  }
  // 3. the loop: the host reads the count of unfinished problems, one word per pass
  const PgDims d = pg_dims(w->prob.data(), P);
  const int max_passes = (cfg->max_iterations > 0 ? cfg->max_iterations : 0) + 1;
  for (a.pass = 0;; ++a.pass) {
    if (a.pass >= max_passes) return pfail(w, LLSR_EIO, "pg optimize: a problem is unfinished after max_iterations");
    if (dev) {
      k_pg_linearize<<<dim3(d.fac_blocks, P), kBlock, 0, s>>>(a);
      k_pg_error<<<d.prob_blocks, kBlock, 0, s>>>(a);
      k_pg_assemble<<<dim3(d.rows, P), kBlock, 0, s>>>(a);
      k_pg_solve<<<P, kBlock, 0, s>>>(a);
      k_pg_update<<<dim3(d.pose_blocks, P), kBlock, 0, s>>>(a);
      PG_OK(w, hipGetLastError());
      PG_OK(w, hipMemcpyAsync(w->hlive, a.live, sizeof(int), hipMemcpyDeviceToHost, s));
      PG_OK(w, hipStreamSynchronize(s));
    } else {
      pg_pass_host(a, d);
      *w->hlive = *a.live;
    }
    if (*w->hlive <= 0) break;
  }
  // 4. the reports, and the poses of the problems that moved
  PG_OK(w, pg_out(w, w->st.data(), a.st, (size_t)P, s));
  if (dev) PG_OK(w, hipStreamSynchronize(s));
  for (int p = 0; p < P; ++p) {
    if (!w->prob[p].run) continue;
    const PgState& st = w->st[p];
    if (!pg_moved(st)) continue;
    const size_t R0 = pose_at(w, p, 0), K = (size_t)w->K[p];
    PG_OK(w, pg_out(w, &w->X[12 * R0], a.X + 12 * R0, 12 * K, s));
    PG_OK(w, pg_out(w, &w->out6[6 * R0], a.out6 + 6 * R0, 6 * K, s));
  }
  float ms = 0;
  if (dev) {
    PG_OK(w, hipEventRecord(w->ev[1], s));
    PG_OK(w, hipStreamSynchronize(s));
    PG_OK(w, hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
  }
  for (int p = 0; p < P; ++p) {
    if (!w->prob[p].run) continue;
    const PgState& st = w->st[p];
    if (pg_moved(st)) {
      const size_t R0 = pose_at(w, p, 0);
      std::memcpy(&w->p6[6 * R0], &w->out6[6 * R0], 6 * (size_t)w->K[p] * sizeof(float));
    }
    w->dirty[p] = 0;
  }
  if (!dev) ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (reps)
    for (int p = 0; p < P; ++p) {
      if (!w->prob[p].run) continue;
      reps[p].state = w->st[p].state;
      reps[p].iterations = w->st[p].iterations;
      reps[p].error_before = w->st[p].err0;
      reps[p].error_after = w->st[p].err;
      reps[p].moved = pg_moved(w->st[p]) ? 1 : 0;
      reps[p].ms = ms;
    }
  return LLSR_OK;
}

// ---- library-internal -----------------------------------------------------------------------------------
llsr_pg* llsr_pg_grown(const llsr_pg* g, int32_t max_poses, int32_t max_loops, int64_t max_envelope_blocks) {
  if (!g || max_poses < g->maxK || max_loops < g->maxL || max_envelope_blocks < g->maxE) return nullptr;
  llsr_pg* w = llsr_pg_create(g->device, g->P, max_poses, max_loops, max_envelope_blocks);
  if (!w) return nullptr;
  for (int p = 0; p < g->P; ++p) {
    const size_t K = (size_t)g->K[p], L = (size_t)g->L[p];
    w->K[p] = g->K[p]; w->L[p] = g->L[p]; w->dirty[p] = g->dirty[p];
    if (K) {
      std::memcpy(&w->p6[6 * pose_at(w, p, 0)], &g->p6[6 * pose_at(g, p, 0)], 6 * K * sizeof(float));
      std::memcpy(&w->X[12 * pose_at(w, p, 0)], &g->X[12 * pose_at(g, p, 0)], 12 * K * sizeof(double));
      std::memcpy(&w->Zk[12 * pose_at(w, p, 0)], &g->Zk[12 * pose_at(g, p, 0)], 12 * K * sizeof(double));
    }
    if (L) {
      std::memcpy(&w->Zl[12 * loop_at(w, p, 0)], &g->Zl[12 * loop_at(g, p, 0)], 12 * L * sizeof(double));
      std::memcpy(&w->wl[loop_at(w, p, 0)], &g->wl[loop_at(g, p, 0)], L * sizeof(double));
      std::memcpy(&w->loops[2 * loop_at(w, p, 0)], &g->loops[2 * loop_at(g, p, 0)], 2 * L * sizeof(int32_t));
    }
  }
  return w;
}

int32_t llsr_pg_truncate(llsr_pg* w, int32_t p, int32_t keep) {
  if (!w || p < 0 || p >= w->P || keep < 0 || keep > w->K[p]) return LLSR_EINVAL;
  const int32_t* lp = &w->loops[2 * loop_at(w, p, 0)];
  for (int l = 0; l < w->L[p]; ++l)
    if (lp[2 * l] >= keep || lp[2 * l + 1] >= keep) return pfail(w, LLSR_EINVAL, "pg truncate: a loop factor holds the pose");
  w->K[p] = keep;
  return LLSR_OK;
}

void llsr_pg_capacity(const llsr_pg* w, int32_t* max_poses, int32_t* max_loops, int64_t* max_envelope_blocks) {
  *max_poses = w->maxK;
  *max_loops = w->maxL;
  *max_envelope_blocks = w->maxE;
}
