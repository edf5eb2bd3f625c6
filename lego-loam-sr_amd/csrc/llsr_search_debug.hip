// llsr_search_debug.hip — diagnostics (not part of the ABI header) that run the cell-grid build
// (llsr_grid.hip) and this translation unit's own copies of the searches (llsr_search.h) on clouds
// and queries given by the caller, for tests/test_gpu_grid_build.py and tests/test_gpu_search.py.
// The kernels here only map a thread or a block to a query; the searches are the header's text.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/llsr.h"
#include "llsr_grid.h"
#include "llsr_host.h"
#include "llsr_search.h"

namespace llsr {
namespace {

constexpr int kDbgMaxP = 64;
constexpr int kDbgMaxPts = 1 << 20;  // per cloud, per query set and per `cap`

// One grid's device memory. `grid` reads the cloud from `src` / `off`, both owned here too.
struct GridMem {
  llsr_host::DevMem src, off, tab, sorted, where, cursor;
  CellGrid grid{};
  size_t tab_bytes = 0, sorted_bytes = 0;
};

// off[0..P] is a non-decreasing list from 0 with a total within the diagnostics' bound
bool offsets_ok(const int64_t* off, int P) {
  if (!off || off[0] != 0) return false;
  for (int p = 0; p < P; ++p)
    if (off[p + 1] < off[p]) return false;
  return off[P] <= kDbgMaxPts;
}

// Allocate and fill the inputs of one grid of P problems (the table and the copy start as 0xff bytes,
// so what the build did not write is recognisable); LLSR_OK, LLSR_ENODEV or LLSR_EIO.
int32_t grid_mem(GridMem& m, const float* xyzw, const int64_t* off, int cap, int P) {
  const size_t n = (size_t)off[P];
  CellGrid& g = m.grid;
  g.cap = cap;
  g.log2T = grid_log2_table(cap);
  m.tab_bytes = sizeof(CellSlot) * ((size_t)P << g.log2T);
  m.sorted_bytes = sizeof(float4) * (size_t)P * cap;
  if (llsr_host::alloc(m.src, sizeof(float4) * (n ? n : 1)) != hipSuccess ||
      llsr_host::alloc(m.off, sizeof(int64_t) * (P + 1)) != hipSuccess ||
      llsr_host::alloc(m.tab, m.tab_bytes) != hipSuccess ||
      llsr_host::alloc(m.sorted, m.sorted_bytes) != hipSuccess ||
      llsr_host::alloc(m.where, sizeof(int2) * (size_t)P * cap) != hipSuccess ||
      llsr_host::alloc(m.cursor, sizeof(int) * P) != hipSuccess)
    return LLSR_ENODEV;
  if ((n && hipMemcpy(m.src, xyzw, sizeof(float4) * n, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(m.off, off, sizeof(int64_t) * (P + 1), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(m.tab, 0xff, m.tab_bytes) != hipSuccess ||
      hipMemset(m.sorted, 0xff, m.sorted_bytes) != hipSuccess)
    return LLSR_EIO;
  g.src = static_cast<const float4*>(m.src.get());
  g.off = static_cast<const int64_t*>(m.off.get());
  g.tab = static_cast<CellSlot*>(m.tab.get());
  g.sorted = static_cast<float4*>(m.sorted.get());
  g.where = static_cast<int2*>(m.where.get());
  g.cursor = static_cast<int*>(m.cursor.get());
  return LLSR_OK;
}

// One cloud as grid 0 of one problem next to an empty grid 1, built by the production grid_build.
int32_t one_grid(GridMem& m, GridMem& none, const float* xyzw, int n) {
  const int64_t off[2] = {0, n}, off0[2] = {0, 0};
  int32_t rc = grid_mem(m, xyzw, off, n > 1 ? n : 1, 1);
  if (rc == LLSR_OK) rc = grid_mem(none, nullptr, off0, 1, 1);
  if (rc != LLSR_OK) return rc;
  CellGrids2 gg;
  gg.g[0] = m.grid;
  gg.g[1] = none.grid;
  gg.P = 1;
  grid_build(gg, nullptr);
  return hipGetLastError() == hipSuccess ? LLSR_OK : LLSR_EIO;
}

template <class T>
bool dev_alloc(llsr_host::DevMem& m, size_t n) {
  return llsr_host::alloc(m, sizeof(T) * (n ? n : 1)) == hipSuccess;
}
template <class T>
bool to_host(T* dst, const llsr_host::DevMem& m, size_t n) {
  return n == 0 || hipMemcpy(dst, m.get(), sizeof(T) * n, hipMemcpyDeviceToHost) == hipSuccess;
}

__global__ void k_debug_knn5(CellGrid g, const float4* q, int Q, int* idx, float* d2, uint8_t* found) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= Q) return;
  Best5 b;
  found[k] = knn5(g.table(0), g.log2T, g.cells(0), q[k].x, q[k].y, q[k].z, b) ? 1 : 0;
  for (int j = 0; j < 5; ++j) { idx[5 * k + j] = b.i[j]; d2[5 * k + j] = b.d[j]; }
}

// nn1_shells (seeded as the surf pass seeds it) and nn1_scan, one query per thread
__global__ void k_debug_nn1(CellGrid g, const float4* q, int Q, float dist_sqr, const int* seed, uint8_t* settled,
                            int* sh_bi, float* sh_bd, int* sc_bi, float* sc_bd) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= Q) return;
  const float4* cloud = g.src;
  const int n = g.count(0);
  int nn = INT_MAX;
  float nd = INFINITY;
  if (seed[k] >= 0) { nn = seed[k]; nd = l2(q[k], cloud[nn]); }
  settled[k] = nn1_shells(g, 0, q[k], dist_sqr, nn, nd) ? 1 : 0;
  sh_bi[k] = nn;
  sh_bd[k] = nd;
  nn1_scan(cloud, n, q[k], nn, nd);
  sc_bi[k] = nn;
  sc_bd[k] = nd;
}

// nn1_block_multi: one block takes the queries kMulti at a time, the last group partial
template <int kNT>
__global__ __launch_bounds__(kNT) void k_debug_nn1_multi(const float4* cloud, int n, const float4* q, int Q, int* bi,
                                                         float* bd) {
  __shared__ float red_d[kMulti][kNT / 64];
  __shared__ int red_i[kMulti][kNT / 64];
  for (int k0 = 0; k0 < Q; k0 += kMulti) {
    const int m = Q - k0 < kMulti ? Q - k0 : kMulti;
    float4 qs[kMulti];
    for (int j = 0; j < kMulti; ++j) qs[j] = j < m ? q[k0 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
    int nn[kMulti];
    float nd[kMulti];
    nn1_block_multi<kNT>(cloud, n, qs, m, nn, nd, red_d, red_i);
    for (int j = 0; j < kMulti; ++j)
      if (j < m && (int)threadIdx.x == j) { bi[k0 + j] = nn[j]; bd[k0 + j] = nd[j]; }
  }
}

}  // namespace
}  // namespace llsr

using namespace llsr;

// The production grid_build over two clouds a, b of P problems each (float x, y, z, w per point,
// off[P + 1] from 0, at most `cap` points of a problem are used). log2T[2]; per grid the table
// CellSlot[P][1 << log2T] (16 bytes a slot: uint64 key, int32 start, int32 count) and the
// cell-contiguous copy float4[P][cap] (w = the original index's bits); what the build leaves
// unwritten reads as 0xff bytes.
extern "C" int32_t llsr_debug_grid_build(const float* a_xyzw, const int64_t* a_off, int32_t a_cap,
                                         const float* b_xyzw, const int64_t* b_off, int32_t b_cap, int32_t P,
                                         int32_t* log2T, void* a_tab, float* a_sorted, void* b_tab, float* b_sorted) {
  if (P < 1 || P > kDbgMaxP || a_cap < 1 || b_cap < 1 || a_cap > kDbgMaxPts || b_cap > kDbgMaxPts || !log2T ||
      !a_tab || !a_sorted || !b_tab || !b_sorted || !offsets_ok(a_off, P) || !offsets_ok(b_off, P) ||
      (a_off[P] && !a_xyzw) || (b_off[P] && !b_xyzw))
    return LLSR_EINVAL;
  GridMem a, b;
  int32_t rc = grid_mem(a, a_xyzw, a_off, a_cap, P);
  if (rc == LLSR_OK) rc = grid_mem(b, b_xyzw, b_off, b_cap, P);
  if (rc != LLSR_OK) return rc;
  CellGrids2 gg;
  gg.g[0] = a.grid;
  gg.g[1] = b.grid;
  gg.P = P;
  grid_build(gg, nullptr);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(a_tab, a.tab, a.tab_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(a_sorted, a.sorted, a.sorted_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(b_tab, b.tab, b.tab_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(b_sorted, b.sorted, b.sorted_bytes, hipMemcpyDeviceToHost) != hipSuccess)
    return LLSR_EIO;
  log2T[0] = a.grid.log2T;
  log2T[1] = b.grid.log2T;
  return LLSR_OK;
}

// knn5 of Q queries (x, y, z, w) in the grid of one map of M points: idx[Q][5], d2[Q][5] as Best5
// holds them (INT_MAX / INF in the places not filled) and found[Q] = knn5's result.
extern "C" int32_t llsr_debug_knn5(const float* map_xyzw, int32_t M, const float* q_xyzw, int32_t Q, int32_t* idx,
                                   float* d2, uint8_t* found) {
  if (M < 0 || M > kDbgMaxPts || Q < 1 || Q > kDbgMaxPts || (M && !map_xyzw) || !q_xyzw || !idx || !d2 || !found)
    return LLSR_EINVAL;
  GridMem m, none;
  llsr_host::DevMem dq, di, dd, df;
  if (!dev_alloc<float4>(dq, Q) || !dev_alloc<int>(di, 5 * (size_t)Q) || !dev_alloc<float>(dd, 5 * (size_t)Q) ||
      !dev_alloc<uint8_t>(df, Q))
    return LLSR_ENODEV;
  if (hipMemcpy(dq, q_xyzw, sizeof(float4) * Q, hipMemcpyHostToDevice) != hipSuccess) return LLSR_EIO;
  const int32_t rc = one_grid(m, none, map_xyzw, M);
  if (rc != LLSR_OK) return rc;
  k_debug_knn5<<<(Q + 255) / 256, 256>>>(m.grid, (const float4*)dq.get(), Q, (int*)di.get(), (float*)dd.get(),
                                         (uint8_t*)df.get());
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess || !to_host(idx, di, 5 * (size_t)Q) ||
      !to_host(d2, dd, 5 * (size_t)Q) || !to_host(found, df, Q))
    return LLSR_EIO;
  return LLSR_OK;
}

// The scan-to-scan kNN-1 of Q queries in one cloud of N points: nn1_shells with dist_sqr from
// (seed[k], its distance) or from (INT_MAX, INF) when seed[k] is -1 -> settled, sh_bi, sh_bd;
// nn1_scan -> sc_bi, sc_bd; nn1_block_multi<256> -> m256_bi, m256_bd; <512> -> m512_bi, m512_bd.
extern "C" int32_t llsr_debug_nn1(const float* cloud_xyzw, int32_t N, const float* q_xyzw, int32_t Q, float dist_sqr,
                                  const int32_t* seed, uint8_t* settled, int32_t* sh_bi, float* sh_bd, int32_t* sc_bi,
                                  float* sc_bd, int32_t* m256_bi, float* m256_bd, int32_t* m512_bi, float* m512_bd) {
  if (N < 0 || N > kDbgMaxPts || Q < 1 || Q > kDbgMaxPts || (N && !cloud_xyzw) || !q_xyzw || !seed || !settled ||
      !sh_bi || !sh_bd || !sc_bi || !sc_bd || !m256_bi || !m256_bd || !m512_bi || !m512_bd || dist_sqr != dist_sqr)
    return LLSR_EINVAL;
  for (int32_t k = 0; k < Q; ++k)
    if (seed[k] < -1 || seed[k] >= N) return LLSR_EINVAL;
  GridMem m, none;
  llsr_host::DevMem dq, ds, dset, di[4], dd[4];
  if (!dev_alloc<float4>(dq, Q) || !dev_alloc<int>(ds, Q) || !dev_alloc<uint8_t>(dset, Q)) return LLSR_ENODEV;
  for (int k = 0; k < 4; ++k)
    if (!dev_alloc<int>(di[k], Q) || !dev_alloc<float>(dd[k], Q)) return LLSR_ENODEV;
  if (hipMemcpy(dq, q_xyzw, sizeof(float4) * Q, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(ds, seed, sizeof(int) * Q, hipMemcpyHostToDevice) != hipSuccess)
    return LLSR_EIO;
  const int32_t rc = one_grid(m, none, cloud_xyzw, N);
  if (rc != LLSR_OK) return rc;
  const float4* q = (const float4*)dq.get();
  k_debug_nn1<<<(Q + 255) / 256, 256>>>(m.grid, q, Q, dist_sqr, (const int*)ds.get(), (uint8_t*)dset.get(),
                                        (int*)di[0].get(), (float*)dd[0].get(), (int*)di[1].get(), (float*)dd[1].get());
  k_debug_nn1_multi<256><<<1, 256>>>(m.grid.src, N, q, Q, (int*)di[2].get(), (float*)dd[2].get());
  k_debug_nn1_multi<512><<<1, 512>>>(m.grid.src, N, q, Q, (int*)di[3].get(), (float*)dd[3].get());
  int32_t* const oi[4] = {sh_bi, sc_bi, m256_bi, m512_bi};
  float* const od[4] = {sh_bd, sc_bd, m256_bd, m512_bd};
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess || !to_host(settled, dset, Q))
    return LLSR_EIO;
  for (int k = 0; k < 4; ++k)
    if (!to_host(oi[k], di[k], Q) || !to_host(od[k], dd[k], Q)) return LLSR_EIO;
  return LLSR_OK;
}
