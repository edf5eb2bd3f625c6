// llsr_pools.h — the layout function of every buffer pool of the C-ABI layer: which pieces a pool
// holds, in which order, and how many elements each has. A layout names no element type (take()
// reads it off the member it fills), so this header needs no device declarations and
// tests/native/host_pool_check.cpp instantiates the same functions on the CPU. The order of the
// take() calls is the order in memory.
#pragma once
#include "llsr_host.h"

namespace llsr_host __attribute__((visibility("hidden"))) {

// The feature pipeline's per-slot buffers (DevBufs): B slots of H rings, HW cells; cnt counter
// words per slot, adj DBSCAN adjacency words per slot.
template <class D>
void feature_layout(Carver& c, D& d, size_t B, size_t H, size_t HW, size_t cnt, size_t adj) {
  const size_t n = B * HW;
  c.take(d.counts, B * cnt);
  c.take(d.orient, B * 4);
  c.take(d.cell_pt, n);
  c.take(d.range, n);
  c.take(d.full, n);
  c.take(d.ground, n);
  c.take(d.label, n);
  c.take(d.near_pts, n);
  c.take(d.shuf, n);
  c.take(d.ccl_a, n);
  c.take(d.ccl_b, n);
  c.take(d.start_ring, B * H);
  c.take(d.end_ring, B * H);
  c.take(d.seg, n);
  c.take(d.seg_ground, n);
  c.take(d.seg_col, n);
  c.take(d.seg_range, n);
  c.take(d.seg_int, n);
  c.take(d.outl, n);
  c.take(d.outl_int, n);
  c.take(d.loam, n);
  c.take(d.curv, n);
  c.take(d.picked, n);
  c.take(d.clabel, n);
  c.take(d.ring_cnt, B * 3 * H);
  c.take(d.edge_tmp, n);
  c.take(d.flat_tmp, n);
  c.take(d.lflat_tmp, n);
  c.take(d.less_sharp, n);
  c.take(d.cluster, n);
  c.take(d.sharp, n);
  c.take(d.flat, n);
  c.take(d.lflat, n);
  c.take(d.db_pts, n);
  c.take(d.db_kz, n);
  c.take(d.db_adj, B * adj);
  c.take(d.mt0, 624);
  c.take(d.phantom, B);
  c.take(d.seg_zero, B);
}

// The staged IMU windows (llsr_stage_imu): B slots of at most `win` samples, and the slots' carry;
// ... and the pinned host staging behind them.
template <class I>
void imu_layout(Carver& c, I& m, size_t B, size_t win) {
  c.take(m.d_samples, B * win);
  c.take(m.d_off, B + 1);
  c.take(m.d_time, B);
  c.take(m.d_carry, B);
}
template <class I>
void imu_host_layout(Carver& c, I& m, size_t B, size_t win) {
  c.take(m.h_samples, B * win);
  c.take(m.h_off, B + 1);
  c.take(m.h_time, B);
}

// The two cell grids (CellGrids2) of P problems: cap_[k] points and 1 << log2T[k] slots each.
template <class G>
void grids_layout(Carver& c, G& g, size_t P, const int cap[2], const int log2T[2]) {
  for (int k = 0; k < 2; ++k) c.take(g.g[k].tab, P << log2T[k]);
  for (int k = 0; k < 2; ++k) c.take(g.g[k].sorted, P * cap[k]);
  for (int k = 0; k < 2; ++k) c.take(g.g[k].where, P * cap[k]);
  for (int k = 0; k < 2; ++k) {
    c.take(g.g[k].cursor, P);
    g.g[k].cap = cap[k];
    g.g[k].log2T = log2T[k];
  }
}

// Scan-to-map (S2MArgs): P problems, map capacities mc / ms, `blocks` query blocks per problem,
// spill_cap Eigen depth blocks per problem beyond the ones the solve keeps in LDS.
struct S2MDims {
  int P, mc, ms, log2T_c, log2T_s, blocks, spill_cap;
};
template <class A>
void s2m_layout(Carver& c, A& a, const S2MDims& d) {
  const size_t P = d.P;
  const int cap[2] = {d.mc, d.ms}, log2T[2] = {d.log2T_c, d.log2T_s};
  c.take(a.prob, P);
  grids_layout(c, a.grids, P, cap, log2T);
  c.take(a.rows, 2 * 256 * P * d.blocks);
  c.take(a.bcnt, P * d.blocks);
  c.take(a.blk_spill, 29 * P * d.spill_cap);
  c.take(a.n_active, 2);  // n_active, error
}

// Scan-to-scan (S2SArgs): P problems, query capacities ms / f, last-cloud capacities nc / ns.
struct S2SDims {
  int P, ms, f, nc, ns, log2T_c, log2T_s;
};
template <class A>
void s2s_layout(Carver& c, A& a, const S2SDims& d) {
  const size_t P = d.P, ns = d.ns, capq = (size_t)(d.ms > d.f ? d.ms : d.f) + 1;
  const int cap[2] = {d.nc, d.ns}, log2T[2] = {d.log2T_c, d.log2T_s};
  grids_layout(c, a.grids, P, cap, log2T);
  c.take(a.idx, 5 * P * capq);  // kIx ints per query (llsr_fa_lm.hip)
  c.take(a.rows, P * capq);
  c.take(a.valid, P * capq);
  c.take(a.error, 1);
  c.take(a.sbox, 2 * P * ((ns + 7) / 8));
  c.take(a.sbox2, 2 * P * ((ns + 63) / 64));
  c.take(a.prof, 8 * P);
}

// A run of pieces llsr_odometry_reset zeroes with one memset (padding included).
struct Span {
  size_t off = 0, bytes = 0;
};

// End-to-end odometry, device side: B slots, `cap` points per packed cloud, `shadow` shadow points.
// o.zero[0] and o.zero[1] receive the two runs of per-slot state that a reset clears.
template <class O>
void odo_layout(Carver& c, O& o, size_t B, size_t cap, size_t shadow) {
  o.zero[0].off = c.off;
  c.take(o.tcur, 6 * B);
  c.take(o.tsum, 6 * B);
  c.take(o.deg, B);
  c.take(o.inited, B);
  c.take(o.frames, B);
  o.zero[0].bytes = c.off - o.zero[0].off;
  c.take(o.shadow, shadow);
  c.take(o.sharp, cap);
  c.take(o.flat, cap);
  c.take(o.scan_c, cap);
  c.take(o.scan_s, cap);
  for (int k = 0; k < 2; ++k) {
    c.take(o.last_c[k], cap);
    c.take(o.last_s[k], cap);
  }
  o.zero[1].off = c.off;
  c.take(o.off, 6 * (B + 1));
  c.take(o.report, B);
  c.take(o.guess, 6 * B);
  c.take(o.tlm, 6 * B);
  c.take(o.flags, B);
  o.zero[1].bytes = c.off - o.zero[1].off;
}
// ... and its pinned host staging (cnt counter words per slot)
template <class O>
void odo_host_layout(Carver& c, O& o, size_t B, size_t cnt) {
  c.take(o.h_off, 6 * (B + 1));
  c.take(o.h_counts, cnt * B);
  c.take(o.h_tsum, 6 * B);
  c.take(o.h_guess, 6 * B);
  c.take(o.h_flags, B);
}

// Mapping chain: the per-slot LM state on the device and its pinned host mirror.
template <class M>
void mapping_layout(Carver& c, M& m, size_t B) {
  c.take(m.d_pose, 6 * B);
  c.take(m.d_rep, B);
  c.take(m.d_deg, B);
  c.take(m.d_matP, 36 * B);
  c.take(m.d_off, 5 * (B + 1));
  c.take(m.d_deg_bak, B);
  c.take(m.d_matP_bak, 36 * B);
}
template <class M>
void mapping_host_layout(Carver& c, M& m, size_t B) {
  c.take(m.h_pose, 6 * B);
  c.take(m.h_rep, B);
  c.take(m.h_off, 5 * (B + 1));
  c.take(m.h_frames, B);
  c.take(m.h_tsum, 6 * B);
}

// Device staging of a single-problem call (llsr_scan2map, llsr_scan2scan): four clouds of n[k]
// points, their four offset pairs, the 6-float pose, the degenerate flag (scan-to-scan only) and
// rep_bytes of report.
template <class S>
void oneshot_layout(Carver& c, S& s, const int32_t n[4], bool with_deg, size_t rep_bytes) {
  for (int k = 0; k < 4; ++k) c.take(s.cloud[k], (size_t)n[k]);
  c.take(s.off, 8);
  c.take(s.pose, 6);
  if (with_deg) c.take(s.deg, 1);
  c.take(s.rep, rep_bytes);
}

}  // namespace llsr_host
