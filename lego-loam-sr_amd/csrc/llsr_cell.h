// llsr_cell.h — the cell arithmetic of the 1 m cell grids (llsr_grid.h), written for host and
// device: the table slot, the cell of a coordinate, the packed key, the hash, the probe and the
// (distance, index) order of the searches. Plain C++ (no HIP types), so the loop-closure ICP's host
// driver and its stand-alone check build from the same text as the kernels.
#pragma once
#include <math.h>
#include <stdint.h>

#include "llsr_libm.h"  // LLSR_HD

namespace llsr {

struct CellSlot {
  uint64_t key;  // packed cell or kCellEmpty
  int start;     // first point of the cell in `sorted`
  int count;
};

constexpr uint64_t kCellEmpty = ~0ull;
constexpr int kCellSentinel = 1048500;  // cell_coord of a NaN / huge coordinate

LLSR_HD int cell_coord(float v) {
  // floor() to a cell index; NaN / huge coordinates land in a far sentinel cell (their distance
  // tests fail anyway, so where they are bucketed cannot change a result)
  const float f = floorf(v);
  return (f > -1048000.0f && f < 1048000.0f) ? (int)f : kCellSentinel;
}

LLSR_HD uint64_t cell_key(int a, int b, int c) {
  return ((uint64_t)(uint32_t)(a + 1048576) << 42) | ((uint64_t)(uint32_t)(b + 1048576) << 21) |
         (uint64_t)(uint32_t)(c + 1048576);
}

LLSR_HD uint32_t cell_hash(uint64_t k, int log2T) {
  return (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> (64 - log2T));
}

// Probe for `key`; returns the slot or -1 (the table is never full: more slots than points).
LLSR_HD int grid_find(const CellSlot* __restrict__ tab, int log2T, uint64_t key) {
  const uint32_t mask = (1u << log2T) - 1u;
  uint32_t s = cell_hash(key, log2T);
  for (;;) {
    const uint64_t k = tab[s].key;
    if (k == key) return (int)s;
    if (k == kCellEmpty) return -1;
    s = (s + 1) & mask;
  }
}

// (d, index) lexicographic order: the result of inserting candidates in index order with
// nanoflann's strict '<' (KNNResultSet::addPoint).
LLSR_HD bool nn_before(float da, int ia, float db, int ib) {
  return da < db || (da == db && ia < ib);
}

// Table size for `cap` points per problem.
// Table slots: the smallest power of two ABOVE the point capacity, so at least one slot stays
// empty even if every point had its own cell (grid_find and the insert probes end at an empty
// slot). Clouds hold several points per 1 m cell, so the load is low in practice; k_grid_clear and
// k_grid_alloc sweep the whole table, so a 2x margin doubled their cost (measured: scan-to-map grid
// build 3.7 ms per 256-problem step with 2x).
inline int grid_log2_table(int cap) {
  int l = 4;
  while ((1ll << l) <= (long long)(cap > 1 ? cap : 1)) ++l;
  return l;
}

}  // namespace llsr
