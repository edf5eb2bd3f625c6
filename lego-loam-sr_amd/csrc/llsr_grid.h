// llsr_grid.h — 1 m cell grids over per-problem point clouds, the device replacement for the
// reference's per-scan nanoflann kd-trees (KdTreeFLANN::setInputCloud; MO:1575-1576 for the
// local maps, FA:2714-2717 for the last corner / surf clouds).
//
// A grid is an open-addressing table of occupied cells (packed floor(x), floor(y), floor(z))
// plus a cell-contiguous copy of the cloud storing (x, y, z, original index bits). Searches
// break distance ties by the original index, so the order of points inside the copy (filled
// with atomics) never changes a result. Built by k_grid_{clear, insert, alloc, scatter} for
// two clouds per problem at once (blockIdx.z).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "llsr_cell.h"  // CellSlot, cell_coord, cell_key, cell_hash, grid_find, nn_before, grid_log2_table

namespace llsr {

struct CellGrid {
  const float4* src;    // the clouds, concatenated over the batch
  const int64_t* off;   // [P+1]
  int cap;              // points per problem reserved
  int log2T;            // table slots per problem = 1 << log2T (> cap, grid_log2_table)
  CellSlot* tab;        // [P][1 << log2T]
  float4* sorted;       // [P][cap]
  int2* where;          // [P][cap] (slot, rank) of each point
  int* cursor;          // [P]
  __device__ __forceinline__ int count(int p) const {
    const int64_t n = off[p + 1] - off[p];
    return n < 0 ? 0 : (n > cap ? cap : (int)n);
  }
  __device__ __forceinline__ const CellSlot* table(int p) const { return tab + ((size_t)p << log2T); }
  __device__ __forceinline__ const float4* cells(int p) const { return sorted + (size_t)p * cap; }
};

struct CellGrids2 {
  CellGrid g[2];
  int P;
};

__global__ void k_grid_clear(CellGrids2 g);
__global__ void k_grid_insert(CellGrids2 g);
__global__ void k_grid_alloc(CellGrids2 g);
__global__ void k_grid_scatter(CellGrids2 g);

// Enqueue the four build kernels for both grids of P problems.
inline void grid_build(const CellGrids2& g, hipStream_t s) {
  const int T = 1 << (g.g[0].log2T > g.g[1].log2T ? g.g[0].log2T : g.g[1].log2T);
  const int M = g.g[0].cap > g.g[1].cap ? g.g[0].cap : g.g[1].cap;
  k_grid_clear<<<dim3((T + 255) / 256, g.P, 2), 256, 0, s>>>(g);
  if (M > 0) k_grid_insert<<<dim3((M + 1023) / 1024, g.P, 2), 256, 0, s>>>(g);  // kInsChunk
  k_grid_alloc<<<dim3((T + 4095) / 4096, g.P, 2), 256, 0, s>>>(g);                // 256 * kAllocPer
  if (M > 0) k_grid_scatter<<<dim3((M + 255) / 256, g.P, 2), 256, 0, s>>>(g);
}

// The same four kernels for one grid of P problems (z extent 1: only g[0] is read). The second entry
// of the argument is a copy of the first, so no launch ever carries a pointer that is not a live
// allocation of the caller's.
inline void grid_build_one(const CellGrid& one, int P, hipStream_t s) {
  CellGrids2 g;
  g.g[0] = one;
  g.g[1] = one;
  g.P = P;
  const int T = 1 << one.log2T;
  const int M = one.cap;
  k_grid_clear<<<dim3((T + 255) / 256, P, 1), 256, 0, s>>>(g);
  if (M > 0) k_grid_insert<<<dim3((M + 1023) / 1024, P, 1), 256, 0, s>>>(g);  // kInsChunk
  k_grid_alloc<<<dim3((T + 4095) / 4096, P, 1), 256, 0, s>>>(g);                // 256 * kAllocPer
  if (M > 0) k_grid_scatter<<<dim3((M + 255) / 256, P, 1), 256, 0, s>>>(g);
}

}  // namespace llsr
