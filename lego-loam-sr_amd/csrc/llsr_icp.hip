// llsr_icp.hip — the host-only entry points of the loop closure (detectLoopClosure /
// performLoopClosure, mapOptmization.cpp:894-1094): the configuration blocks, the candidate selection,
// one ICP iteration's rigid estimate and the pose constraint, as DESIGN.md §16 specifies them
// (llsr_icp.h), and the alignment itself: llsr_icp_align_host, the serial loop over heap buffers, and
// llsr_icp_align, the same loop bodies as kernels on device clouds, and llsr_icp_align_batch, P
// alignments in one set of launches over a table of their arguments. Every kernel of the alignment is
// in this translation unit and calls only force-inlined functions of llsr_icp.h (no cross-TU device
// call); the target's cell grid is built by the k_grid_* kernels of llsr_grid.hip, launched from here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/llsr.h"
#include "llsr_grid.h"
#include "llsr_icp.h"

// ---- host-only entry points ---------------------------------------------------------------------
extern "C" int32_t llsr_loop_config_lidar(llsr_loop_config* c, int32_t lidar) {
  if (!c) return LLSR_EINVAL;
  std::memset(c, 0, sizeof *c);
  if (lidar == LLSR_LIDAR_VLP16) { c->search_radius = 15.0f; c->search_num = 50; c->fitness_score = 0.5f; }        // CFG:29-31
  else if (lidar == LLSR_LIDAR_VLP32C) { c->search_radius = 50.0f; c->search_num = 40; c->fitness_score = 1.5f; }  // CFG:97-99
  else if (lidar == LLSR_LIDAR_HDL64E) { c->search_radius = 30.0f; c->search_num = 30; c->fitness_score = 0.8f; }  // CFG:165-167
  else return LLSR_EINVAL;
  c->leaf = 0.2f;                               // MO:97
  c->min_time_gap = 30.0;                       // MO:912
  c->icp_max_iterations = 100;                  // MO:1001
  c->icp_transformation_epsilon = 1e-6;         // MO:1002
  c->icp_fitness_epsilon = 1e-6;                // MO:1008
  c->icp_max_correspondence_distance = 100.0;   // MO:1007
  return LLSR_OK;
}

// MO:902-919: the first key pose of the sorted radius search that is old (or new) enough. The
// reference writes an unqualified abs(); fabs in double is this library's reading of it.
extern "C" int32_t llsr_loop_candidate(const float* poses4, const double* times, int32_t K, const float pos[3],
                                       double now, float radius, double gap) {
  if (K < 0 || !pos || (K > 0 && (!poses4 || !times))) return LLSR_EINVAL;
  if (K == 0) return -1;
  std::vector<int32_t> near((size_t)K);
  const int n = llsr_keypose_radius_sorted(poses4, K, pos, radius, near.data());
  for (int i = 0; i < n; ++i)
    if (std::fabs(times[near[i]] - now) > gap) return near[i];
  return -1;
}

extern "C" int32_t llsr_umeyama3(const float* src_xyz, const float* dst_xyz, int32_t n, float* T16) {
  if (!src_xyz || !dst_xyz || !T16 || n < 1) return LLSR_EINVAL;
  llsr_loop::umeyama3_host(src_xyz, dst_xyz, n, T16);
  return LLSR_OK;
}

namespace {

// The result of a finished loop from its state
void icp_result(const llsr_loop::IcpState& st, llsr_icp_result* res) {
  res->converged = st.converged;
  res->state = st.state;
  res->iterations = st.iterations;
  res->n_pairs_last = st.n_pairs;
  res->fitness = st.n_fit > 0 ? st.fit_sum / (double)st.n_fit : llsr_loop::kDblMax;
  std::memcpy(res->T, st.fin, sizeof res->T);
}

void icp_params(const llsr_loop_config* cfg, llsr_loop::IcpArgs* a) {
  a->max_iterations = cfg->icp_max_iterations;
  a->eps_t = cfg->icp_transformation_epsilon;
  a->eps_f = cfg->icp_fitness_epsilon;
  a->mcd2 = cfg->icp_max_correspondence_distance * cfg->icp_max_correspondence_distance;
}

bool icp_bad_args(const float* src4, int32_t n_src, const float* tgt4, int32_t n_tgt, const llsr_loop_config* cfg,
                  const llsr_icp_result* res) {
  return !cfg || !res || n_src < 0 || n_tgt < 0 || (n_src > 0 && !src4) || (n_tgt > 0 && !tgt4) ||
         n_src > LLSR_ICP_MAX_POINTS || n_tgt > LLSR_ICP_MAX_POINTS;
}

}  // namespace

// The serial statement of the alignment: heap buffers of exactly icp_sizes, the problem's own table
// size, the one serial driver of llsr_icp.h on a table of that one entry.
extern "C" int32_t llsr_icp_align_host(const float* src4, int32_t n_src, const float* tgt4, int32_t n_tgt,
                                       const llsr_loop_config* cfg, llsr_icp_result* res, float* aligned4) {
  if (icp_bad_args(src4, n_src, tgt4, n_tgt, cfg, res)) return LLSR_EINVAL;
  using namespace llsr_loop;
  const IcpSizes z = icp_sizes(n_src, n_tgt);
  const int log2T = z.log2T;
  std::vector<llsr::CellSlot> tab(z.tab);
  std::vector<float> cells(z.cells4), work(z.work4), d2(z.d2), ps(z.ps4), pd(z.pd4), al(z.aligned4), part(z.part);
  std::vector<int> match(z.match);
  int box[6];
  IcpState st;
  grid_build_host(tgt4, n_tgt, log2T, tab.data(), cells.data(), box);
  IcpArgs a{};
  a.src4 = src4; a.tgt4 = tgt4; a.tab = tab.data(); a.cells4 = cells.data(); a.box = box;
  a.work4 = work.data(); a.match = match.data(); a.d2 = d2.data(); a.ps4 = ps.data(); a.pd4 = pd.data();
  a.part = part.data(); a.st = &st; a.aligned4 = aligned4 ? aligned4 : al.data();
  a.n_src = n_src; a.n_tgt = n_tgt; a.log2T = log2T;
  icp_params(cfg, &a);
  if (icp_run_host(&a, 1) < 1) return LLSR_EIO;
  icp_result(st, res);
  return LLSR_OK;
}

extern "C" int32_t llsr_loop_constraint(const float* T16, const float* pose_latest6, const float* pose_closest6,
                                        double fitness, float* pose_from6, float* pose_to6, float* variance) {
  if (!T16 || !pose_latest6 || !pose_closest6 || !pose_from6 || !pose_to6 || !variance) return LLSR_EINVAL;
  llsr_loop::loop_constraint(T16, pose_latest6, pose_closest6, fitness, pose_from6, pose_to6, variance);
  return LLSR_OK;
}

// ---- the device alignment ---------------------------------------------------------------------------
// One kernel per step of §16's loop, each a wrapper that maps (block, thread) to an index and calls
// the body of llsr_icp.h; the bodies are the ones llsr_icp_align_host runs. The argument struct holds
// device pointers only; the host sees the state through copies into pinned memory.
namespace {

using namespace llsr_loop;

__global__ __launch_bounds__(kLaneBlock) void k_icp_init(IcpArgs a) {
  if (threadIdx.x != 0) return;
  state_init(a.st);
  a.box[0] = a.box[1] = a.box[2] = kBoxEmptyLo;
  a.box[3] = a.box[4] = a.box[5] = kBoxEmptyHi;
}

// The occupied cell box of the target: integer min / max (order independent, so exact)
__global__ __launch_bounds__(kCorrBlock) void k_icp_box(IcpArgs a) {
  int c[3];
  if (!box_cell(a, point_of(blockIdx.x, threadIdx.x, kCorrBlock), c)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    atomicMin(&a.box[k], c[k]);
    atomicMax(&a.box[3 + k], c[k]);
  }
}

__global__ __launch_bounds__(kCorrBlock) void k_icp_corr(IcpArgs a) {
  corr_body(a, point_of(blockIdx.x, threadIdx.x, kCorrBlock));
}

// The kept pairs in source order: one block walks the source in tiles of kPackBlock, a ballot scan
// inside each wave, the wave totals through LDS, the running base in a register of every thread.
__global__ __launch_bounds__(kPackBlock) void k_icp_pack(IcpArgs a) {
  constexpr int kWaves = kPackBlock / 64;
  __shared__ int wtot[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, w = (tid >> 6) & (kWaves - 1);
  const int tiles = blocks_for(a.n_src, kPackBlock);
  int base = 0;
  for (int tile = 0; tile < tiles; ++tile) {
    const int i = point_of(tile, tid, kPackBlock);
    const int keep = pack_keep(a, i);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wtot[w] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int c = wtot[k];
      before += k < w ? c : 0;
      total += c;
    }
    if (keep) pack_write(a, i, base + before + __popcll(m & ((1ull << lane) - 1ull)));
    base += total;
    __syncthreads();
  }
  if (tid == 0) a.st->n_pairs = base;
}

__global__ __launch_bounds__(kLaneBlock) void k_icp_means(IcpArgs a) { means_body(a, threadIdx.x); }

__global__ __launch_bounds__(kCorrBlock) void k_icp_sigma(IcpArgs a) {
  sigma_body(a, point_of(blockIdx.x, threadIdx.x, kCorrBlock));
}

__global__ __launch_bounds__(kLaneBlock) void k_icp_finish(IcpArgs a) {
  if (threadIdx.x == 0) finish_body(a);
}

__global__ __launch_bounds__(kCorrBlock) void k_icp_fit(IcpArgs a) {
  fit_body(a, point_of(blockIdx.x, threadIdx.x, kCorrBlock));
}

__global__ __launch_bounds__(kLaneBlock) void k_icp_fitsum(IcpArgs a) {
  if (threadIdx.x == 0) fitsum_body(a);
}

// ---- the batch kernels (llsr_icp_align_batch): blockIdx.y = problem, tab[blockIdx.y] its arguments ----
// Each is the kernel above on one entry of the table. A block past its problem's extent returns at
// once; the loop kernels also return for a problem that has left kStateNone. `live` counts the
// problems still in the loop: k_icp_finish_b takes a problem off it with an integer atomic, and the
// host reads that one word per pass.
__global__ __launch_bounds__(kLaneBlock) void k_icp_init_b(const IcpArgs* __restrict__ tab, int P, int* live) {
  const int p = point_of(blockIdx.x, threadIdx.x, kLaneBlock);
  if (p == 0) *live = P;
  if (p < P) init_body(tab[p]);
}

__global__ __launch_bounds__(kCorrBlock) void k_icp_box_b(const IcpArgs* __restrict__ tab) {
  const IcpArgs& a = tab[blockIdx.y];
  if (!batch_block(blockIdx.x, a.n_tgt, kCorrBlock)) return;
  int c[3];
  if (!box_cell(a, point_of(blockIdx.x, threadIdx.x, kCorrBlock), c)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    atomicMin(&a.box[k], c[k]);
    atomicMax(&a.box[3 + k], c[k]);
  }
}

__global__ __launch_bounds__(kCorrBlock) void k_icp_corr_b(const IcpArgs* __restrict__ tab) {
  const IcpArgs& a = tab[blockIdx.y];
  if (!batch_live(a) || !batch_block(blockIdx.x, a.n_src, kCorrBlock)) return;
  corr_body(a, point_of(blockIdx.x, threadIdx.x, kCorrBlock));
}

// k_icp_pack's scan, one block per problem (the single call's kernel stays as it is, so the scan is
// written out a second time here)
__global__ __launch_bounds__(kPackBlock) void k_icp_pack_b(const IcpArgs* __restrict__ tab) {
  constexpr int kWaves = kPackBlock / 64;
  __shared__ int wtot[kWaves];
  const IcpArgs& a = tab[blockIdx.x];
  if (!batch_live(a)) return;  // block-uniform
  const int tid = threadIdx.x, lane = tid & 63, w = (tid >> 6) & (kWaves - 1);
  const int tiles = blocks_for(a.n_src, kPackBlock);
  int base = 0;
  for (int tile = 0; tile < tiles; ++tile) {
    const int i = point_of(tile, tid, kPackBlock);
    const int keep = pack_keep(a, i);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wtot[w] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int c = wtot[k];
      before += k < w ? c : 0;
      total += c;
    }
    if (keep) pack_write(a, i, base + before + __popcll(m & ((1ull << lane) - 1ull)));
    base += total;
    __syncthreads();
  }
  if (tid == 0) a.st->n_pairs = base;
}

__global__ __launch_bounds__(kLaneBlock) void k_icp_means_b(const IcpArgs* __restrict__ tab) {
  const IcpArgs& a = tab[blockIdx.x];
  if (batch_live(a)) means_body(a, threadIdx.x);
}

__global__ __launch_bounds__(kCorrBlock) void k_icp_sigma_b(const IcpArgs* __restrict__ tab) {
  const IcpArgs& a = tab[blockIdx.y];
  if (!batch_live(a) || !batch_block(blockIdx.x, 9 * sigma_blocks_max(a.n_src), kCorrBlock)) return;
  sigma_body(a, point_of(blockIdx.x, threadIdx.x, kCorrBlock));
}

__global__ __launch_bounds__(kLaneBlock) void k_icp_finish_b(const IcpArgs* __restrict__ tab, int* live) {
  if (threadIdx.x == 0 && finish_batch_body(tab[blockIdx.x])) atomicSub(live, 1);
}

__global__ __launch_bounds__(kCorrBlock) void k_icp_fit_b(const IcpArgs* __restrict__ tab) {
  const IcpArgs& a = tab[blockIdx.y];
  if (!batch_block(blockIdx.x, a.n_src, kCorrBlock)) return;
  fit_body(a, point_of(blockIdx.x, threadIdx.x, kCorrBlock));
}

__global__ __launch_bounds__(kLaneBlock) void k_icp_fitsum_b(const IcpArgs* __restrict__ tab) {
  if (threadIdx.x == 0) fitsum_body(tab[blockIdx.x]);
}

template <class T>
hipError_t icp_grow(T*& p, size_t& cap, size_t need) {
  if (need <= cap) return hipSuccess;
  size_t n = cap ? cap : 256;
  while (n < need) n += n / 2 + 1;
  if (p) {
    hipError_t e = hipFree(p);
    if (e != hipSuccess) return e;
    p = nullptr;
  }
  cap = 0;
  hipError_t e = hipMalloc(&p, n * sizeof(T));
  if (e == hipSuccess) cap = n;
  return e;
}

}  // namespace

struct llsr_icp {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // the target's grid
  llsr::CellSlot* tab = nullptr;
  float4* sorted = nullptr;
  int2* where = nullptr;
  size_t cap_tab = 0, cap_sorted = 0, cap_where = 0;
  int* cursor = nullptr;      // [1]
  int64_t* off = nullptr;     // [2] = 0, n_tgt
  // the loop's buffers (llsr_loop::IcpArgs)
  float *work = nullptr, *d2 = nullptr, *ps = nullptr, *pd = nullptr, *part = nullptr;
  int* match = nullptr;
  size_t cap_work = 0, cap_d2 = 0, cap_ps = 0, cap_pd = 0, cap_part = 0, cap_match = 0;
  int* box = nullptr;                  // [6]
  llsr_loop::IcpState* st = nullptr;    // device
  llsr_loop::IcpState* hst = nullptr;   // pinned copy
  int64_t* hoff = nullptr;             // pinned [2]
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  float corr_ms = 0, solve_ms = 0, total_ms = 0;
  // llsr_icp_align_batch: the per-problem words ([P] states, [6 P] box words, [P] grid cursors,
  // [P + 1] target offsets), the argument table, the count of unfinished problems, and one pinned
  // staging block (table, offsets, states, the count); the buffers above serve both forms
  llsr_loop::IcpState* bst = nullptr;
  int *bbox = nullptr, *bcursor = nullptr;
  int64_t* boff = nullptr;
  llsr_loop::IcpArgs* btab = nullptr;
  size_t cap_bst = 0, cap_bbox = 0, cap_bcursor = 0, cap_boff = 0, cap_btab = 0;
  int* live = nullptr;   // [1]
  char* hb = nullptr;    // pinned
  size_t cap_hb = 0;
  int passes = 0;        // passes of the last batch call's loop (llsr_icp_last_passes)
};

static int32_t ifail(llsr_icp* w, int32_t code, const std::string& msg) {
  if (w) w->err = msg;
  return code;
}

#define ICP_OK(w, expr)                                                          \
  do {                                                                           \
    hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess)                                                        \
      return ifail(w, LLSR_EIO, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

extern "C" void llsr_icp_destroy(llsr_icp* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  if (w->stream) (void)hipStreamSynchronize(w->stream);
  void* dev[] = {w->tab, w->sorted, w->where, w->cursor, w->off, w->work, w->d2, w->ps, w->pd, w->part, w->match,
                 w->box, w->st, w->bst, w->bbox, w->bcursor, w->boff, w->btab, w->live};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  if (w->hb) (void)hipHostFree(w->hb);
  if (w->hst) (void)hipHostFree(w->hst);
  if (w->hoff) (void)hipHostFree(w->hoff);
  for (hipEvent_t e : w->ev)
    if (e) (void)hipEventDestroy(e);
  if (w->stream) (void)hipStreamDestroy(w->stream);
  delete w;
}

extern "C" llsr_icp* llsr_icp_create(int32_t dev) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || dev < 0 || dev >= count) return nullptr;
  if (hipSetDevice(dev) != hipSuccess) return nullptr;
  llsr_icp* w = new (std::nothrow) llsr_icp;
  if (!w) return nullptr;
  w->device = dev;
  bool ok = hipStreamCreate(&w->stream) == hipSuccess && hipMalloc(&w->cursor, sizeof(int)) == hipSuccess &&
            hipMalloc(&w->off, 2 * sizeof(int64_t)) == hipSuccess && hipMalloc(&w->box, 6 * sizeof(int)) == hipSuccess &&
            hipMalloc(&w->st, sizeof(llsr_loop::IcpState)) == hipSuccess &&
            hipHostMalloc((void**)&w->hst, sizeof(llsr_loop::IcpState)) == hipSuccess &&
            hipHostMalloc((void**)&w->hoff, 2 * sizeof(int64_t)) == hipSuccess;
  for (hipEvent_t& e : w->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  if (!ok) {
    llsr_icp_destroy(w);
    return nullptr;
  }
  return w;
}

extern "C" const char* llsr_icp_last_error(const llsr_icp* w) { return w ? w->err.c_str() : "null workspace"; }

extern "C" int32_t llsr_icp_last_times(const llsr_icp* w, float* corr_ms, float* solve_ms, float* total_ms) {
  if (!w) return LLSR_EINVAL;
  if (corr_ms) *corr_ms = w->corr_ms;
  if (solve_ms) *solve_ms = w->solve_ms;
  if (total_ms) *total_ms = w->total_ms;
  return LLSR_OK;
}

extern "C" int32_t llsr_icp_align(llsr_icp* w, const float* d_src4, int32_t n_src, const float* d_tgt4, int32_t n_tgt,
                                  const llsr_loop_config* cfg, llsr_icp_result* res, float* d_aligned4,
                                  void* hip_stream) {
  if (!w) return LLSR_EINVAL;
  if (icp_bad_args(d_src4, n_src, d_tgt4, n_tgt, cfg, res))
    return ifail(w, LLSR_EINVAL, "icp align: bad arguments");
  if (((uintptr_t)d_src4 | (uintptr_t)d_tgt4 | (uintptr_t)d_aligned4) & 15)
    return ifail(w, LLSR_EINVAL, "icp align: clouds must be 16-byte aligned");
  ICP_OK(w, hipSetDevice(w->device));
  const hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : w->stream;
  // 1. size and grow every buffer of the call; nothing is queued on behalf of this call yet, and the
  //    previous call synchronised before it returned (an earlier failure may not have: wait first)
  const IcpSizes z = icp_sizes(n_src, n_tgt);
  ICP_OK(w, hipStreamSynchronize(s));
  ICP_OK(w, icp_grow(w->tab, w->cap_tab, z.tab));
  ICP_OK(w, icp_grow(w->sorted, w->cap_sorted, z.cells4 / 4));
  ICP_OK(w, icp_grow(w->where, w->cap_where, z.cells4 / 4));
  ICP_OK(w, icp_grow(w->work, w->cap_work, z.work4));
  ICP_OK(w, icp_grow(w->d2, w->cap_d2, z.d2));
  ICP_OK(w, icp_grow(w->match, w->cap_match, z.match));
  ICP_OK(w, icp_grow(w->ps, w->cap_ps, z.ps4));
  ICP_OK(w, icp_grow(w->pd, w->cap_pd, z.pd4));
  ICP_OK(w, icp_grow(w->part, w->cap_part, z.part));
  // 2. only now the pointers go into the argument structs (an empty cloud is given one of the
  //    workspace's own buffers, never a null pointer)
  llsr::CellGrid g;
  g.src = n_tgt > 0 ? reinterpret_cast<const float4*>(d_tgt4) : w->sorted;
  g.off = w->off;
  g.cap = n_tgt;
  g.log2T = z.log2T;
  g.tab = w->tab;
  g.sorted = w->sorted;
  g.where = w->where;
  g.cursor = w->cursor;
  IcpArgs a{};
  a.src4 = n_src > 0 ? d_src4 : w->work;
  a.tgt4 = n_tgt > 0 ? d_tgt4 : reinterpret_cast<const float*>(w->sorted);
  a.tab = w->tab;
  a.cells4 = reinterpret_cast<const float*>(w->sorted);
  a.box = w->box;
  a.work4 = w->work;
  a.match = w->match;
  a.d2 = w->d2;
  a.ps4 = w->ps;
  a.pd4 = w->pd;
  a.part = w->part;
  a.st = w->st;
  a.aligned4 = d_aligned4 ? d_aligned4 : w->work;  // the working cloud is done with when the fit runs
  a.n_src = n_src;
  a.n_tgt = n_tgt;
  a.log2T = z.log2T;
  icp_params(cfg, &a);
  // 3. the grid, the box, the working cloud
  ICP_OK(w, hipEventRecord(w->ev[0], s));
  w->hoff[0] = 0;
  w->hoff[1] = n_tgt;
  ICP_OK(w, hipMemcpyAsync(w->off, w->hoff, 2 * sizeof(int64_t), hipMemcpyHostToDevice, s));
  llsr::grid_build_one(g, 1, s);
  k_icp_init<<<1, kLaneBlock, 0, s>>>(a);
  k_icp_box<<<blocks_for(n_tgt, kCorrBlock), kCorrBlock, 0, s>>>(a);
  ICP_OK(w, hipGetLastError());
  if (n_src > 0)
    ICP_OK(w, hipMemcpyAsync(w->work, d_src4, 4 * (size_t)n_src * sizeof(float), hipMemcpyDeviceToDevice, s));
  ICP_OK(w, hipEventRecord(w->ev[1], s));
  ICP_OK(w, hipStreamSynchronize(s));
  float ms = 0;
  ICP_OK(w, hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
  w->total_ms = ms;
  w->corr_ms = w->solve_ms = 0;
  // 4. the loop: the host reads one state word per iteration
  const int corr_blocks = blocks_for(n_src, kCorrBlock);
  const int sigma_blocks = blocks_for(9 * sigma_blocks_max(n_src), kCorrBlock);
  for (;;) {
    ICP_OK(w, hipEventRecord(w->ev[0], s));
    k_icp_corr<<<corr_blocks, kCorrBlock, 0, s>>>(a);
    ICP_OK(w, hipEventRecord(w->ev[1], s));
    k_icp_pack<<<1, kPackBlock, 0, s>>>(a);
    k_icp_means<<<1, kLaneBlock, 0, s>>>(a);
    k_icp_sigma<<<sigma_blocks, kCorrBlock, 0, s>>>(a);
    k_icp_finish<<<1, kLaneBlock, 0, s>>>(a);
    ICP_OK(w, hipGetLastError());
    ICP_OK(w, hipEventRecord(w->ev[2], s));
    ICP_OK(w, hipMemcpyAsync(&w->hst->state, &w->st->state, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ICP_OK(w, hipStreamSynchronize(s));
    float c = 0, v = 0;
    ICP_OK(w, hipEventElapsedTime(&c, w->ev[0], w->ev[1]));
    ICP_OK(w, hipEventElapsedTime(&v, w->ev[1], w->ev[2]));
    w->corr_ms += c;
    w->solve_ms += v;
    if (w->hst->state != kStateNone) break;
  }
  // 5. the aligned cloud and the fitness
  ICP_OK(w, hipEventRecord(w->ev[0], s));
  k_icp_fit<<<corr_blocks, kCorrBlock, 0, s>>>(a);
  k_icp_fitsum<<<1, kLaneBlock, 0, s>>>(a);
  ICP_OK(w, hipGetLastError());
  ICP_OK(w, hipMemcpyAsync(w->hst, w->st, sizeof(IcpState), hipMemcpyDeviceToHost, s));
  ICP_OK(w, hipEventRecord(w->ev[1], s));
  ICP_OK(w, hipStreamSynchronize(s));
  ICP_OK(w, hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
  w->total_ms += ms + w->corr_ms + w->solve_ms;
  icp_result(*w->hst, res);
  return LLSR_OK;
}

// ---- the batch form -----------------------------------------------------------------------------------
extern "C" int32_t llsr_icp_align_batch(llsr_icp* w, int32_t P, const float* d_src4, const int64_t* src_off,
                                        const float* d_tgt4, const int64_t* tgt_off, const llsr_loop_config* cfgs,
                                        int32_t n_cfgs, llsr_icp_result* res, float* d_aligned4, void* hip_stream) {
  if (!w) return LLSR_EINVAL;
  if (P < 1 || !src_off || !tgt_off || !cfgs || !res || (n_cfgs != 1 && n_cfgs != P) || src_off[0] < 0 ||
      tgt_off[0] < 0)
    return ifail(w, LLSR_EINVAL, "icp align batch: bad arguments");
  if (P > 65535) return ifail(w, LLSR_ERANGE, "icp align batch: more than 65535 problems");
  for (int p = 0; p < P; ++p) {
    const int64_t ns = src_off[p + 1] - src_off[p], nt = tgt_off[p + 1] - tgt_off[p];
    if (ns < 0 || nt < 0) return ifail(w, LLSR_EINVAL, "icp align batch: decreasing offsets");
    if (ns > LLSR_ICP_MAX_POINTS || nt > LLSR_ICP_MAX_POINTS)
      return ifail(w, LLSR_ERANGE, "icp align batch: a problem exceeds LLSR_ICP_MAX_POINTS");
  }
  const int64_t S = src_off[P] - src_off[0], Tn = tgt_off[P] - tgt_off[0];
  if ((S > 0 && !d_src4) || (Tn > 0 && !d_tgt4)) return ifail(w, LLSR_EINVAL, "icp align batch: bad arguments");
  if (((uintptr_t)d_src4 | (uintptr_t)d_tgt4 | (uintptr_t)d_aligned4) & 15)
    return ifail(w, LLSR_EINVAL, "icp align batch: clouds must be 16-byte aligned");
  ICP_OK(w, hipSetDevice(w->device));
  const hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : w->stream;
  // 1. size and grow every buffer of the call before any pointer enters the table (as llsr_icp_align)
  const IcpBatchLayout L = icp_batch_layout(P, src_off, tgt_off);
  const size_t nP = (size_t)P;
  ICP_OK(w, hipStreamSynchronize(s));
  ICP_OK(w, icp_grow(w->tab, w->cap_tab, L.tab));
  ICP_OK(w, icp_grow(w->sorted, w->cap_sorted, L.cells));
  ICP_OK(w, icp_grow(w->where, w->cap_where, L.cells));
  ICP_OK(w, icp_grow(w->work, w->cap_work, 4 * L.points));
  ICP_OK(w, icp_grow(w->d2, w->cap_d2, L.points));
  ICP_OK(w, icp_grow(w->match, w->cap_match, L.points));
  ICP_OK(w, icp_grow(w->ps, w->cap_ps, 4 * L.points));
  ICP_OK(w, icp_grow(w->pd, w->cap_pd, 4 * L.points));
  ICP_OK(w, icp_grow(w->part, w->cap_part, L.part));
  ICP_OK(w, icp_grow(w->bst, w->cap_bst, nP));
  ICP_OK(w, icp_grow(w->bbox, w->cap_bbox, 6 * nP));
  ICP_OK(w, icp_grow(w->bcursor, w->cap_bcursor, nP));
  ICP_OK(w, icp_grow(w->boff, w->cap_boff, nP + 1));
  ICP_OK(w, icp_grow(w->btab, w->cap_btab, nP));
  if (!w->live) ICP_OK(w, hipMalloc((void**)&w->live, sizeof(int)));
  // pinned staging: [P] IcpArgs, [P + 1] offsets, [P] IcpState, the count (8-byte aligned pieces)
  const size_t at_off = nP * sizeof(IcpArgs), at_st = at_off + (nP + 1) * sizeof(int64_t),
               at_live = at_st + nP * sizeof(IcpState), need_hb = at_live + sizeof(int64_t);
  if (need_hb > w->cap_hb) {
    if (w->hb) ICP_OK(w, hipHostFree(w->hb));
    w->hb = nullptr;
    w->cap_hb = 0;
    ICP_OK(w, hipHostMalloc((void**)&w->hb, need_hb + need_hb / 2));
    w->cap_hb = need_hb + need_hb / 2;
  }
  IcpArgs* htab = reinterpret_cast<IcpArgs*>(w->hb);
  int64_t* hoff = reinterpret_cast<int64_t*>(w->hb + at_off);
  IcpState* hst = reinterpret_cast<IcpState*>(w->hb + at_st);
  int* hlive = reinterpret_cast<int*>(w->hb + at_live);
  // 2. the table
  IcpBatchBuffers b{};
  b.src4 = S > 0 ? d_src4 + 4 * (size_t)src_off[0] : w->work;
  b.tgt4 = Tn > 0 ? d_tgt4 + 4 * (size_t)tgt_off[0] : reinterpret_cast<const float*>(w->sorted);
  b.tab = w->tab;
  b.cells4 = reinterpret_cast<float*>(w->sorted);
  b.box = w->bbox;
  b.work4 = w->work; b.ps4 = w->ps; b.pd4 = w->pd;
  b.match = w->match;
  b.d2 = w->d2;
  b.part = w->part;
  b.st = w->bst;
  b.aligned4 = d_aligned4 ? d_aligned4 : w->work;  // the working cloud is done with when the fit runs
  size_t part_at = 0;
  for (int p = 0; p < P; ++p) {
    htab[p] = IcpArgs{};
    icp_batch_entry(L, b, src_off, tgt_off, p, &part_at, &htab[p]);
    icp_params(&cfgs[n_cfgs == 1 ? 0 : p], &htab[p]);
    hoff[p] = tgt_off[p];
  }
  hoff[P] = tgt_off[P];
  const IcpBatchDims dims = icp_batch_dims(htab, P);
  llsr::CellGrid g;
  g.src = Tn > 0 ? reinterpret_cast<const float4*>(d_tgt4) : w->sorted;
  g.off = w->boff;
  g.cap = L.cap;
  g.log2T = L.log2T;
  g.tab = w->tab;
  g.sorted = w->sorted;
  g.where = w->where;
  g.cursor = w->bcursor;
  // 3. the grids, the boxes, the working clouds
  ICP_OK(w, hipEventRecord(w->ev[0], s));
  ICP_OK(w, hipMemcpyAsync(w->btab, htab, nP * sizeof(IcpArgs), hipMemcpyHostToDevice, s));
  ICP_OK(w, hipMemcpyAsync(w->boff, hoff, (nP + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  llsr::grid_build_one(g, P, s);
  k_icp_init_b<<<blocks_for(P, kLaneBlock), kLaneBlock, 0, s>>>(w->btab, P, w->live);
  k_icp_box_b<<<dim3(dims.box_blocks, P), kCorrBlock, 0, s>>>(w->btab);
  ICP_OK(w, hipGetLastError());
  if (S > 0) ICP_OK(w, hipMemcpyAsync(w->work, b.src4, 4 * (size_t)S * sizeof(float), hipMemcpyDeviceToDevice, s));
  ICP_OK(w, hipEventRecord(w->ev[1], s));
  ICP_OK(w, hipStreamSynchronize(s));
  float ms = 0;
  ICP_OK(w, hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
  w->total_ms = ms;
  w->corr_ms = w->solve_ms = 0;
  w->passes = 0;
  // 4. the loop: the host reads the count of unfinished problems, one word per pass
  for (;;) {
    if (w->passes >= dims.max_passes)
      return ifail(w, LLSR_EIO, "icp align batch: a problem is unfinished after the largest icp_max_iterations");
    ++w->passes;
    ICP_OK(w, hipEventRecord(w->ev[0], s));
    k_icp_corr_b<<<dim3(dims.corr_blocks, P), kCorrBlock, 0, s>>>(w->btab);
    ICP_OK(w, hipEventRecord(w->ev[1], s));
    k_icp_pack_b<<<P, kPackBlock, 0, s>>>(w->btab);
    k_icp_means_b<<<P, kLaneBlock, 0, s>>>(w->btab);
    k_icp_sigma_b<<<dim3(dims.sigma_blocks, P), kCorrBlock, 0, s>>>(w->btab);
    k_icp_finish_b<<<P, kLaneBlock, 0, s>>>(w->btab, w->live);
    ICP_OK(w, hipGetLastError());
    ICP_OK(w, hipEventRecord(w->ev[2], s));
    ICP_OK(w, hipMemcpyAsync(hlive, w->live, sizeof(int), hipMemcpyDeviceToHost, s));
    ICP_OK(w, hipStreamSynchronize(s));
    float c = 0, v = 0;
    ICP_OK(w, hipEventElapsedTime(&c, w->ev[0], w->ev[1]));
    ICP_OK(w, hipEventElapsedTime(&v, w->ev[1], w->ev[2]));
    w->corr_ms += c;
    w->solve_ms += v;
    if (*hlive <= 0) break;
  }
  // 5. the aligned clouds and the fitness of every problem
  ICP_OK(w, hipEventRecord(w->ev[0], s));
  k_icp_fit_b<<<dim3(dims.corr_blocks, P), kCorrBlock, 0, s>>>(w->btab);
  k_icp_fitsum_b<<<P, kLaneBlock, 0, s>>>(w->btab);
  ICP_OK(w, hipGetLastError());
  ICP_OK(w, hipMemcpyAsync(hst, w->bst, nP * sizeof(IcpState), hipMemcpyDeviceToHost, s));
  ICP_OK(w, hipEventRecord(w->ev[1], s));
  ICP_OK(w, hipStreamSynchronize(s));
  ICP_OK(w, hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
  w->total_ms += ms + w->corr_ms + w->solve_ms;
  for (int p = 0; p < P; ++p) icp_result(hst[p], &res[p]);
  return LLSR_OK;
}

extern "C" int32_t llsr_icp_last_passes(const llsr_icp* w) { return w ? w->passes : LLSR_EINVAL; }
