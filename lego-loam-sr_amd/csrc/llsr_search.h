// llsr_search.h — the device searches over the 1 m cell grids (llsr_grid.h): kNN-5 of the
// scan-to-map LM (llsr_mo.hip) and the kNN-1 of the scan-to-scan LM (llsr_fa_lm.hip) with its two
// exact scans. Everything here has internal linkage: each translation unit that includes the header
// compiles its own copy, so the diagnostic wrappers of llsr_search_debug.hip run this text without
// the device link seeing a second caller of the production kernels' copies.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "llsr_device.h"
#include "llsr_grid.h"

// a translation unit uses the kNN-5 or the kNN-1 half, rarely both
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunused-variable"

namespace llsr {

using llsr_libm::fbits;

namespace {

struct Best5 {
  float d[5];
  int i[5];
};

// The 27 neighbour cells in the order kNN-5 visits them: the query's own cell, the 6 face
// neighbours, the 12 edge and the 8 corner neighbours (packed as (dx+1) | (dy+1) << 2 | (dz+1) << 4),
// so the 5th-best distance tightens early and prunes the farther cells.
__constant__ unsigned char kCellOrder[27] = {
    21,                                          // (0, 0, 0)
    20, 22, 17, 25, 5, 37,                       // faces
    16, 18, 24, 26, 4, 6, 36, 38, 1, 9, 33, 41,  // edges
    0, 2, 8, 10, 32, 34, 40, 42};                // corners

// kNN-5 with d^2 < 1.0 around q in one map; returns true when five were found.
// The result is the five smallest (d^2, index) pairs of the cells' points with d^2 < 1.0, in any
// visiting order. A cell is skipped when no point in it can enter that set: its box lies at squared
// distance LB from q, every point's float d^2 (three rounded differences, squares and sums) is at
// least LB (1 - 5 eps) minus the rounding of the box gaps (< 1e-7 absolute), so a cell with
// LB > lim (1 + 1e-5) + 4e-6 holds only points with d^2 > lim, where lim = 1.0, or the current 5th
// distance once five are held (a tie at lim would need d^2 == lim). Exact, therefore, and typically
// 7 of the 27 cells are probed (the center, the faces and a few edges; tests/test_gpu_mo.py).
__device__ bool knn5(const CellSlot* __restrict__ tab, int log2T, const float4* __restrict__ pts,
                     float qx, float qy, float qz, Best5& b) {
#pragma unroll
  for (int k = 0; k < 5; ++k) { b.d[k] = INFINITY; b.i[k] = INT_MAX; }
  const int cx = cell_coord(qx), cy = cell_coord(qy), cz = cell_coord(qz);
  // distances from q to its cell's lower / upper faces per axis (cell_coord's sentinel cell for
  // NaN / huge coordinates: gaps become NaN / huge, no cell is skipped wrongly since LB > lim fails
  // for NaN and a huge q finds nothing anyway)
  const float lx = qx - floorf(qx), ly = qy - floorf(qy), lz = qz - floorf(qz);
  const float ux = 1.0f - lx, uy = 1.0f - ly, uz = 1.0f - lz;
  // cells visited one at a time (not unrolled): keeps the kernel's VGPRs low, which beat issuing
  // all probes up front on MI355X (latency-bound gathers, 8 waves per SIMD)
#pragma unroll 1
  for (int c = 0; c < 27; ++c) {
    const int o = kCellOrder[c];
    const int ox = (o & 3) - 1, oy = ((o >> 2) & 3) - 1, oz = (o >> 4) - 1;
    const float gx = ox < 0 ? lx : (ox > 0 ? ux : 0.0f);
    const float gy = oy < 0 ? ly : (oy > 0 ? uy : 0.0f);
    const float gz = oz < 0 ? lz : (oz > 0 ? uz : 0.0f);
    const float lb = gx * gx + gy * gy + gz * gz;
    const float lim = b.d[4] < 1.0f ? b.d[4] : 1.0f;
    if (lb > lim * 1.00001f + 4e-6f) continue;
    const int s = grid_find(tab, log2T, cell_key(cx + ox, cy + oy, cz + oz));
    if (s < 0) continue;
    const int st = tab[s].start, n = tab[s].count;
    float4 pn = n > 0 ? pts[st] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = st; j < st + n; ++j) {
      const float4 p = pn;  // the next point's load is in flight while this one is tested
      if (j + 1 < st + n) pn = pts[j + 1];
      float d = 0.0f;
      float t = qx - p.x; d += t * t;  // nanoflann L2 accumulation order
      t = qy - p.y; d += t * t;
      t = qz - p.z; d += t * t;
      const int id = (int)fbits(p.w);
      if (!(d < 1.0f) || !nn_before(d, id, b.d[4], b.i[4])) continue;
      b.d[4] = d; b.i[4] = id;
#pragma unroll
      for (int k = 4; k > 0; --k)
        if (nn_before(b.d[k], b.i[k], b.d[k - 1], b.i[k - 1])) {
          const float td = b.d[k]; b.d[k] = b.d[k - 1]; b.d[k - 1] = td;
          const int ti = b.i[k]; b.i[k] = b.i[k - 1]; b.i[k - 1] = ti;
        }
    }
  }
  return b.d[4] < 1.0f;
}

constexpr int kMaxShell = 2;  // grid shells searched before the exact block-wide scan (queries in sparse regions)

// nanoflann L2_Simple (query - point), accumulated from 0
__device__ __forceinline__ float l2(float4 q, float4 p) {
  float d = 0.0f, t;
  t = q.x - p.x; d += t * t;
  t = q.y - p.y; d += t * t;
  t = q.z - p.z; d += t * t;
  return d;
}

// Nearest neighbour of q in grid g of problem p (KdTreeFLANN::nearestKSearch, k = 1; ties ->
// lower index) over growing shells of 1 m cells. Returns true once the searched shells provably
// contain the nearest point or nothing nearer than dist_sqr can remain outside them; false when
// kMaxShell shells do not settle it (the caller then scans the whole cloud, nn1_block).
// (bi, bd) may start from a known point of the cloud (the previous kNN pass's answer: a real
// candidate, so the lexicographic minimum is unchanged) — cells farther than it are not probed.
__device__ bool nn1_shells(const CellGrid& g, int p, float4 q, float dist_sqr, int& bi, float& bd) {
  const CellSlot* tab = g.table(p);
  const float4* pts = g.cells(p);
  const int cx = cell_coord(q.x), cy = cell_coord(q.y), cz = cell_coord(q.z);
  // squared gap of q to the cell slab at offset dd along one axis, rounded as l2 rounds: a point
  // of that slab has |fl(q - p)| >= this gap (rounding is monotone and symmetric)
  auto gap2 = [](float v, int c, int dd) {
    const float g = dd < 0 ? v - (float)(c + dd + 1) : dd > 0 ? (float)(c + dd) - v : 0.0f;
    return g * g;
  };
  for (int h = 0; h <= kMaxShell; ++h) {
    for (int dx = -h; dx <= h; ++dx)
      for (int dy = -h; dy <= h; ++dy) {
        const int step = (h == 0 || dx == -h || dx == h || dy == -h || dy == h) ? 1 : 2 * h;
        const float lxy = gap2(q.x, cx, dx) + gap2(q.y, cy, dy);
        for (int dz = -h; dz <= h; dz += step) {
          // a cell whose every point is farther than bd cannot change the (d, index) minimum, and
          // one with none nearer than dist_sqr cannot give a correspondence (finish rejects nd >= it)
          const float lb = lxy + gap2(q.z, cz, dz);
          if (lb > bd || lb >= dist_sqr) continue;
          const int s = grid_find(tab, g.log2T, cell_key(cx + dx, cy + dy, cz + dz));
          if (s < 0) continue;
          const int st = tab[s].start, n = tab[s].count;
          for (int j = st; j < st + n; ++j) {
            const float4 c = pts[j];
            const float d = l2(q, c);
            const int id = (int)fbits(c.w);
            if (nn_before(d, id, bd, bi)) { bd = d; bi = id; }
          }
        }
      }
    // every point outside the searched block is at least r away (float slack 1e-5)
    float r = q.x - (float)(cx - h);
    r = fminf(r, (float)(cx + h + 1) - q.x);
    r = fminf(r, q.y - (float)(cy - h));
    r = fminf(r, (float)(cy + h + 1) - q.y);
    r = fminf(r, q.z - (float)(cz - h));
    r = fminf(r, (float)(cz + h + 1) - q.z);
    const float r2 = r * r * (1.0f - 1e-5f);
    if (bd < r2 || r2 >= dist_sqr) return true;
  }
  return false;
}

// Exact nearest neighbour by a scan in index order with strict '<' (ties -> lower index, as the
// shells).
__device__ __forceinline__ void nn1_scan(const float4* pts, int n, float4 q, int& bi, float& bd) {
  bd = INFINITY;
  bi = INT_MAX;
  for (int k = 0; k < n; ++k) {
    const float d = l2(q, pts[k]);
    if (d < bd) { bd = d; bi = k; }
  }
}

// nn1_scan for up to kMulti queries at once by the whole block: each thread scans an interleaved
// slice of the cloud in index order against every query, then each query's (d, index) minima are
// reduced with the index tie-break — equal to nn1_scan per query, with one pass over the cloud
// for kMulti queries. Contains barriers: every thread of the block must call it.
constexpr int kMulti = 2;  // 2 (from 4): 113 instead of 166 spilled VGPRs at the 4-waves bound
template <int kNT>
__device__ void nn1_block_multi(const float4* pts, int n, const float4* qs, int nq, int* bi, float* bd,
                                float (*red_d)[kNT / 64], int (*red_i)[kNT / 64]) {
  float d[kMulti];
  int id[kMulti];
#pragma unroll
  for (int j = 0; j < kMulti; ++j) { d[j] = INFINITY; id[j] = INT_MAX; }
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    const float4 p = pts[k];
#pragma unroll
    for (int j = 0; j < kMulti; ++j)
      if (j < nq) {
        const float dd = l2(qs[j], p);
        if (dd < d[j]) { d[j] = dd; id[j] = k; }
      }
  }
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int j = 0; j < kMulti; ++j) {
    for (int off = 32; off; off >>= 1) {
      const float od = __shfl_xor(d[j], off, 64);
      const int oi = __shfl_xor(id[j], off, 64);
      if (nn_before(od, oi, d[j], id[j])) { d[j] = od; id[j] = oi; }
    }
    if (lane_id() == 0) { red_d[j][w] = d[j]; red_i[j][w] = id[j]; }
  }
  __syncthreads();
  for (int j = 0; j < nq; ++j) {
    float bdj = red_d[j][0];
    int bij = red_i[j][0];
    for (int k = 1; k < nw; ++k)
      if (nn_before(red_d[j][k], red_i[j][k], bdj, bij)) { bdj = red_d[j][k]; bij = red_i[j][k]; }
    bd[j] = bdj;
    bi[j] = bij;
  }
  __syncthreads();
}

}  // namespace

}  // namespace llsr

#pragma clang diagnostic pop
