// llsr_icp.h — the loop-closure ICP, written once for host and device: the rigid
// estimate of one iteration (Eigen::umeyama without scaling, in float, with this project's own 3x3
// two-sided Jacobi SVD), the loop itself (the shell search over the target's cell grid, the point
// transform, the sequential sums, the stop rule) as bodies that llsr_icp.hip's kernels and the serial
// host driver both call, and the pose constraint of performLoopClosure (MO:1056-1081).
//
// PCL 1.10 and Eigen 3.3.7 are not available to check against, so every order of evaluation below
// is this project's statement (DESIGN.md §16 marks the choices); tests/_loop_closure.py and
// tests/_icp_loop.py restate the same specification independently and the two sides are compared bit
// for bit. No expression here may contract into an FMA (-ffp-contract=off on both sides).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/llsr.h"
#include "llsr_cell.h"
#include "llsr_eigen.h"
#include "llsr_libm.h"

namespace llsr_loop {

using llsr_libm::fabs_;
using llsr_libm::sqrt_;

constexpr float kFltMin = 1.17549435082228751e-38f;  // numeric_limits<float>::min()
constexpr float kFltEps = 1.1920928955078125e-07f;   // numeric_limits<float>::epsilon()
constexpr int kSvdSweeps = 30;  // bound on the Jacobi sweeps (never reached by a finite matrix)

// rows p, q of a row-major 3x3 by [[c, s], [-s, c]] from the left
LLSR_HD void rot_rows(float* M, int p, int q, float c, float s) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float x = M[3 * p + k], y = M[3 * q + k];
    M[3 * p + k] = c * x + s * y;
    M[3 * q + k] = c * y - s * x;
  }
}
// columns p, q by [[c, s], [-s, c]] from the right
LLSR_HD void rot_cols(float* M, int p, int q, float c, float s) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float x = M[3 * k + p], y = M[3 * k + q];
    M[3 * k + p] = c * x - s * y;
    M[3 * k + q] = s * x + c * y;
  }
}

LLSR_HD float det3(const float* m) {
  return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) +
         m[2] * (m[3] * m[7] - m[4] * m[6]);
}

LLSR_HD void swap_cols(float* M, int a, int b) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float t = M[3 * k + a];
    M[3 * k + a] = M[3 * k + b];
    M[3 * k + b] = t;
  }
}

// A = U diag(sv) V^T, row-major 3x3, sv descending and non-negative. Two-sided Jacobi: for each
// pair (p, q) whose off-diagonal entries exceed the threshold, a rotation from the left makes the
// 2x2 block symmetric, then a symmetric Jacobi rotation diagonalises it.
LLSR_HD void svd3(const float* A, float* U, float* sv, float* V) {
  float M[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    M[k] = A[k];
    U[k] = V[k] = (k % 4 == 0) ? 1.0f : 0.0f;
  }
  const float precision = 2.0f * kFltEps;
  float maxd = fabs_(M[0]);
  if (fabs_(M[4]) > maxd) maxd = fabs_(M[4]);
  if (fabs_(M[8]) > maxd) maxd = fabs_(M[8]);
  for (int sweep = 0; sweep < kSvdSweeps; ++sweep) {
    bool finished = true;
#pragma unroll
    for (int pair = 0; pair < 3; ++pair) {
      const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
      float thr = precision * maxd;
      if (kFltMin > thr) thr = kFltMin;
      const float b = M[3 * p + q], c = M[3 * q + p];
      const float off = fabs_(b) > fabs_(c) ? fabs_(b) : fabs_(c);
      if (!(off > thr)) continue;
      finished = false;
      // the left rotation that makes the block symmetric
      const float t = M[3 * p + p] + M[3 * q + q], d = c - b;
      float c1 = 1.0f, s1 = 0.0f;
      if (!(fabs_(d) < kFltMin)) {
        const float u = t / d, w = sqrt_(1.0f + u * u);
        s1 = 1.0f / w;
        c1 = u / w;
      }
      rot_rows(M, p, q, c1, s1);
      rot_cols(U, p, q, c1, -s1);
      // the symmetric Jacobi rotation of [[x, y], [y, z]]
      const float x = M[3 * p + p], y = M[3 * p + q], z = M[3 * q + q];
      const float deno = 2.0f * fabs_(y);
      float c2 = 1.0f, s2 = 0.0f;
      if (!(deno < kFltMin)) {
        const float tau = (x - z) / deno, w = sqrt_(tau * tau + 1.0f);
        const float tt = tau > 0.0f ? 1.0f / (tau + w) : 1.0f / (tau - w);
        const float n = 1.0f / sqrt_(tt * tt + 1.0f);
        const float sg = (tt > 0.0f ? 1.0f : -1.0f) * (y > 0.0f ? 1.0f : -1.0f);
        s2 = -sg * fabs_(tt) * n;
        c2 = n;
      }
      rot_rows(M, p, q, c2, -s2);
      rot_cols(M, p, q, c2, s2);
      rot_cols(U, p, q, c2, s2);
      rot_cols(V, p, q, c2, s2);
      if (fabs_(M[3 * p + p]) > maxd) maxd = fabs_(M[3 * p + p]);
      if (fabs_(M[3 * q + q]) > maxd) maxd = fabs_(M[3 * q + q]);
    }
    if (finished) break;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    sv[k] = M[4 * k];
    if (sv[k] < 0.0f) {
      sv[k] = -sv[k];
#pragma unroll
      for (int r = 0; r < 3; ++r) U[3 * r + k] = -U[3 * r + k];
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {  // selection sort, descending, the first maximum wins
    int best = i;
#pragma unroll
    for (int j = i + 1; j < 3; ++j)
      if (sv[j] > sv[best]) best = j;
    if (best != i) {
      const float t = sv[i];
      sv[i] = sv[best];
      sv[best] = t;
      swap_cols(U, i, best);
      swap_cols(V, i, best);
    }
  }
}

// The rigid transformation from the means and the cross-covariance sigma (row-major, sigma[3i + j]
// = sum dst_demean_i * src_demean_j / n): R = U S V^T with S = (1, 1, det(U) det(V) < 0 ? -1 : 1),
// t = dst_mean - R src_mean. T row-major 4x4.
LLSR_HD void rigid_from_sigma(const float* sigma, const float* src_mean, const float* dst_mean, float* T) {
  float U[9], sv[3], V[9];
  svd3(sigma, U, sv, V);
  const float s2 = det3(U) * det3(V) < 0.0f ? -1.0f : 1.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      T[4 * i + j] = (U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1]) + (U[3 * i + 2] * s2) * V[3 * j + 2];
    T[4 * i + 3] = dst_mean[i] - ((T[4 * i] * src_mean[0] + T[4 * i + 1] * src_mean[1]) + T[4 * i + 2] * src_mean[2]);
  }
  T[12] = T[13] = T[14] = 0.0f;
  T[15] = 1.0f;
}

// gemm_kc(n, 3, 3): the depth block of sigma's sums
LLSR_HD int sigma_block(int n) { return llsr_eigen::gemm_kc(n, 3, 3); }

// Eigen::umeyama (no scaling) of n correspondences (llsr_umeyama3), in the order DESIGN.md §16 fixes:
// sequential means, sigma by depth blocks from zero, each block times 1 / n added in block order.
inline void umeyama3_host(const float* src, const float* dst, int n, float* T) {
  const float inv_n = 1.0f / (float)n;
  float sm[3], dm[3];
  for (int a = 0; a < 3; ++a) {
    float s = 0.0f, d = 0.0f;
    for (int k = 0; k < n; ++k) {
      s = s + src[3 * (size_t)k + a];
      d = d + dst[3 * (size_t)k + a];
    }
    sm[a] = s * inv_n;
    dm[a] = d * inv_n;
  }
  float sigma[9] = {0};
  const int kc = sigma_block(n);
  for (int k0 = 0; k0 < n; k0 += kc) {
    const int k1 = k0 + kc < n ? k0 + kc : n;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        float acc = 0.0f;
        for (int k = k0; k < k1; ++k)
          acc = acc + (dst[3 * (size_t)k + i] - dm[i]) * (src[3 * (size_t)k + j] - sm[j]);
        sigma[3 * i + j] = sigma[3 * i + j] + inv_n * acc;
      }
  }
  rigid_from_sigma(sigma, sm, dm, T);
}

// ---- the alignment loop (DESIGN.md §16 "ICP loop"), one statement for host and device --------------
// Everything below works on plain pointers and integer indices. The kernels of llsr_icp.hip are
// wrappers that map (block, thread) to an index and call a *_body; the host driver icp_run_host calls
// the same bodies in loops over the same (block, thread) ranges, so the two sides share every line
// that touches memory.

constexpr int kStateNone = 0, kStateIterations = 1, kStateTransform = 2, kStateAbsMse = 3, kStateRelMse = 4,
              kStateNoCorrespondences = 5;
constexpr double kDblMax = 1.7976931348623157e308;
constexpr int kBatch = 8;        // independent loads issued ahead of a chain's dependent adds
constexpr int kCorrBlock = 256;  // threads per block of k_icp_corr / k_icp_fit / k_icp_box / k_icp_sigma
constexpr int kPackBlock = 1024; // threads of the one block of k_icp_pack
constexpr int kLaneBlock = 64;   // threads of the one block of k_icp_means / k_icp_finish / k_icp_fitsum
constexpr int kBoxEmptyLo = 0x7fffffff, kBoxEmptyHi = -0x7fffffff - 1;

// Nearest target of (qx, qy, qz) in the cell grid (tab, log2T, cells4 = the cell-contiguous copy,
// [n][4] = x, y, z, original index bits) whose occupied cells lie in box = {lo x, y, z, hi x, y, z}:
// shells of growing Chebyshev radius around the query's cell, each clamped to the box, from the first
// shell that touches it; candidates ordered by nn_before; the walk ends once the best d^2 is strictly
// below r^2. A query or target in the sentinel cell never matches. Returns false when nothing matched.
LLSR_HD bool nn_search(const llsr::CellSlot* tab, int log2T, const float* cells4, const int* box, float qx, float qy,
                       float qz, int* idx, float* d2) {
  const int c[3] = {llsr::cell_coord(qx), llsr::cell_coord(qy), llsr::cell_coord(qz)};
  if (c[0] == llsr::kCellSentinel || c[1] == llsr::kCellSentinel || c[2] == llsr::kCellSentinel) return false;
  int r0 = 0, r1 = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int lo = box[a], hi = box[3 + a];
    if (lo > hi) return false;  // no target cell
    const int below = lo - c[a], above = c[a] - hi;  // > 0: the query's cell is outside on that side
    const int out = below > above ? below : above;
    if (out > r0) r0 = out;
    const int far = -below > -above ? -below : -above;  // the farthest box cell along this axis
    if (far > r1) r1 = far;
  }
  bool have = false;
  float bd = 0.0f;
  int bi = 0;
  for (int r = r0; r <= r1; ++r) {
    const int x0 = c[0] - r > box[0] ? c[0] - r : box[0], x1 = c[0] + r < box[3] ? c[0] + r : box[3];
    const int y0 = c[1] - r > box[1] ? c[1] - r : box[1], y1 = c[1] + r < box[4] ? c[1] + r : box[4];
    const int z0 = c[2] - r > box[2] ? c[2] - r : box[2], z1 = c[2] + r < box[5] ? c[2] + r : box[5];
    for (int x = x0; x <= x1; ++x) {
      const int ax = x > c[0] ? x - c[0] : c[0] - x;
      for (int y = y0; y <= y1; ++y) {
        const int ay = y > c[1] ? y - c[1] : c[1] - y;
        const bool face = ax == r || ay == r;  // the whole z range lies on the shell
        // off the x / y faces only z = c - r and z = c + r are on the shell (one cell when r = 0)
        const int zstep = face ? 1 : (r > 0 ? 2 * r : 1);
        int z = face ? z0 : c[2] - r;
        for (; z <= z1; z += zstep) {
          if (z < z0) continue;
          const int s = llsr::grid_find(tab, log2T, llsr::cell_key(x, y, z));
          if (s < 0) continue;
          const int b = tab[s].start, e = b + tab[s].count;
          for (int k = b; k < e; ++k) {
            const float* p = cells4 + 4 * (size_t)k;
            const float dx = p[0] - qx, dy = p[1] - qy, dz = p[2] - qz;
            const float d = (dx * dx + dy * dy) + dz * dz;
            const int i = (int)llsr_libm::fbits(p[3]);
            if (!have ? d == d : llsr::nn_before(d, i, bd, bi)) {
              have = true;
              bd = d;
              bi = i;
            }
          }
        }
      }
    }
    if (have && bd < (float)r * (float)r) break;
  }
  if (!have) return false;
  *idx = bi;
  *d2 = bd;
  return true;
}

// ((m00 x + m01 y) + m02 z) + m03 per row of the row-major 4x4 M; q[3] passes through
LLSR_HD void xf_rows(const float* M, const float* p, float* q) {
  const float x = p[0], y = p[1], z = p[2], w = p[3];
  q[0] = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  q[1] = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  q[2] = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
  q[3] = w;
}

// F = T * F, each coefficient summed left to right over k
LLSR_HD void mul4_left(const float* T, float* F) {
  float R[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      R[4 * i + j] = ((T[4 * i] * F[j] + T[4 * i + 1] * F[4 + j]) + T[4 * i + 2] * F[8 + j]) + T[4 * i + 3] * F[12 + j];
#pragma unroll
  for (int k = 0; k < 16; ++k) F[k] = R[k];
}

// The sequential sums. Each is one dependent chain of adds over elements first .. last - 1 of an
// array with a stride of 4 floats (base points at the component); the loads of a batch are issued
// together ahead of its adds, which changes nothing about the order of the adds.
LLSR_HD float mean_chain(const float* base, int first, int last) {
  float acc = 0.0f;
  int k = first;
  for (; k + kBatch <= last; k += kBatch) {
    float v[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) v[u] = base[4 * (size_t)(k + u)];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) acc = acc + v[u];
  }
  for (; k < last; ++k) acc = acc + base[4 * (size_t)k];
  return acc;
}
// entry (i, j) of one depth block: sum of (dst_i - dm) * (src_j - sm) from zero
LLSR_HD float sigma_chain(const float* dst, float dm, const float* src, float sm, int first, int last) {
  float acc = 0.0f;
  int k = first;
  for (; k + kBatch <= last; k += kBatch) {
    float a[kBatch], b[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      a[u] = dst[4 * (size_t)(k + u)];
      b[u] = src[4 * (size_t)(k + u)];
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) acc = acc + (a[u] - dm) * (b[u] - sm);
  }
  for (; k < last; ++k) acc = acc + (dst[4 * (size_t)k] - dm) * (src[4 * (size_t)k] - sm);
  return acc;
}
// the double sum of the float d^2 of the kept pairs
LLSR_HD double mse_chain(const float* base, int first, int last) {
  double acc = 0.0;
  int k = first;
  for (; k + kBatch <= last; k += kBatch) {
    float v[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) v[u] = base[4 * (size_t)(k + u)];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) acc = acc + (double)v[u];
  }
  for (; k < last; ++k) acc = acc + (double)base[4 * (size_t)k];
  return acc;
}
// the fitness sum over d2[first .. last) (stride 1); a negative entry marks a point without a
// target and is neither added nor counted
LLSR_HD double fitness_chain(const float* d2, int first, int last, int* count) {
  double acc = 0.0;
  int n = 0, k = first;
  for (; k + kBatch <= last; k += kBatch) {
    float v[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) v[u] = d2[(size_t)(k + u)];
#pragma unroll
    for (int u = 0; u < kBatch; ++u)
      if (v[u] >= 0.0f) {
        acc = acc + (double)v[u];
        ++n;
      }
  }
  for (; k < last; ++k) {
    const float v = d2[(size_t)k];
    if (v >= 0.0f) {
      acc = acc + (double)v;
      ++n;
    }
  }
  *count = n;
  return acc;
}

// The loop's resident state (device memory on the device side; the host reads `state` only).
struct IcpState {
  int32_t state;       // kState*
  int32_t iterations;
  int32_t converged;
  int32_t n_pairs;     // kept pairs of the last correspondence step
  int32_t apply;       // T holds a transformation the working cloud has not yet been moved by
  int32_t n_fit;
  double prev;         // the stop rule's previous mse
  double mse_sum;
  double fit_sum;
  float sm[3], dm[3];  // this iteration's means
  float T[16];         // this iteration's estimate
  float fin[16];       // final
};

LLSR_HD void state_init(IcpState* st) {
  st->state = kStateNone;
  st->iterations = st->converged = st->n_pairs = st->apply = st->n_fit = 0;
  st->prev = kDblMax;
  st->mse_sum = st->fit_sum = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) st->sm[k] = st->dm[k] = 0.0f;
#pragma unroll
  for (int k = 0; k < 16; ++k) st->T[k] = st->fin[k] = (k % 5 == 0) ? 1.0f : 0.0f;
}

// DefaultConvergenceCriteria after the count was incremented (§16's six steps), in double
LLSR_HD void stop_rule(IcpState* st, int max_iterations, double eps_t, double eps_f) {
  if (st->iterations >= max_iterations) {
    st->state = kStateIterations;
    st->converged = 1;
    return;
  }
  const float* T = st->T;
  const double cosv = 0.5 * ((((double)T[0] + (double)T[5]) + (double)T[10]) - 1.0);
  const double tx = (double)T[3], ty = (double)T[7], tz = (double)T[11];
  const double t2 = (tx * tx + ty * ty) + tz * tz;
  if (cosv >= 1.0 - eps_t && t2 <= eps_t) {
    st->state = kStateTransform;
    st->converged = 1;
    return;
  }
  const double mse = st->mse_sum / (double)st->n_pairs;
  const double diff = mse - st->prev, adiff = diff < 0.0 ? -diff : diff;
  if (adiff < 1e-12) {
    st->state = kStateAbsMse;
    st->converged = 1;
    return;
  }
  if (adiff / st->prev < eps_f) {
    st->state = kStateRelMse;
    st->converged = 1;
    return;
  }
  st->prev = mse;
}

// One alignment's buffers and parameters; every pointer is a live allocation of at least the size
// noted (icp_sizes), on the device for the kernels and on the heap for the host driver.
struct IcpArgs {
  const float* src4;          // [n_src][4] the source cloud
  const float* tgt4;          // [n_tgt][4] the target cloud
  const llsr::CellSlot* tab;  // [1 << log2T]
  const float* cells4;        // [max(n_tgt, 1)][4]
  int* box;                   // [6] occupied cell box, lo then hi
  float* work4;               // [max(n_src, 1)][4] the working cloud
  int* match;                 // [max(n_src, 1)] target index or -1
  float* d2;                  // [max(n_src, 1)] its d^2 (the fit pass: -1 without a target)
  float* ps4;                 // [max(n_src, 1)][4] packed source points, w = d^2
  float* pd4;                 // [max(n_src, 1)][4] packed target points
  float* part;                // [9 * sigma_blocks_max(n_src)] block sums of sigma
  IcpState* st;
  float* aligned4;            // [max(n_src, 1)][4] the fit pass's cloud
  int32_t n_src, n_tgt, log2T, max_iterations;
  double eps_t, eps_f, mcd2;  // mcd2 = max correspondence distance, squared in double
};

// ceil(n / sigma_block(n)) <= n / 680 + 1 for every n (checked by the stand-alone program)
LLSR_HD int sigma_blocks_max(int n) { return n / 680 + 1; }

// Element counts of the buffers of one alignment (IcpArgs): what the host driver allocates exactly
// and the device workspace at least.
struct IcpSizes {
  int log2T;
  size_t tab, cells4, work4, match, d2, ps4, pd4, part, aligned4;
};
inline IcpSizes icp_sizes(int n_src, int n_tgt) {
  const size_t ns = (size_t)(n_src > 0 ? n_src : 1), nt = (size_t)(n_tgt > 0 ? n_tgt : 1);
  IcpSizes z;
  z.log2T = llsr::grid_log2_table(n_tgt);
  z.tab = (size_t)1 << z.log2T;
  z.cells4 = 4 * nt;
  z.work4 = z.ps4 = z.pd4 = z.aligned4 = 4 * ns;
  z.match = z.d2 = ns;
  z.part = 9 * (size_t)sigma_blocks_max(n_src);
  return z;
}

// ---- thread index -> work: the only arithmetic the kernels add ---------------------------------
LLSR_HD int point_of(int block, int thread, int block_size) { return block * block_size + thread; }
LLSR_HD int blocks_for(int n, int block_size) { return n > 0 ? (n + block_size - 1) / block_size : 1; }
// lane t of the sigma launch: entry (i, j) of depth block b over pairs first .. last - 1
LLSR_HD bool sigma_lane(int t, int n, int* b, int* i, int* j, int* first, int* last) {
  if (n < 3) return false;
  const int kc = sigma_block(n);
  *b = t / 9;
  const int e = t - 9 * *b;
  *i = e / 3;
  *j = e - 3 * *i;
  if ((long long)*b * kc >= (long long)n) return false;
  *first = *b * kc;
  *last = *first + kc < n ? *first + kc : n;
  return true;
}

// k_icp_box: thread per target point, integer min / max of its cell (atomics on the device)
LLSR_HD bool box_cell(const IcpArgs& a, int i, int* c) {
  if (i >= a.n_tgt) return false;
  const float* p = a.tgt4 + 4 * (size_t)i;
  c[0] = llsr::cell_coord(p[0]);
  c[1] = llsr::cell_coord(p[1]);
  c[2] = llsr::cell_coord(p[2]);
  return c[0] != llsr::kCellSentinel && c[1] != llsr::kCellSentinel && c[2] != llsr::kCellSentinel;
}

// k_icp_corr: thread per source point. Moves the point by the previous iteration's T, then searches.
LLSR_HD void corr_body(const IcpArgs& a, int i) {
  if (i >= a.n_src) return;
  float* w = a.work4 + 4 * (size_t)i;
  float q[4] = {w[0], w[1], w[2], w[3]};
  if (a.st->apply) {
    xf_rows(a.st->T, q, q);
    w[0] = q[0];
    w[1] = q[1];
    w[2] = q[2];
  }
  int idx = -1;
  float d = 0.0f;
  const bool found = nn_search(a.tab, a.log2T, a.cells4, a.box, q[0], q[1], q[2], &idx, &d);
  a.match[i] = found ? idx : -1;
  a.d2[i] = found ? d : 0.0f;
}
// a pair is kept when a target was found and double(d^2) <= mcd^2
LLSR_HD int pack_keep(const IcpArgs& a, int i) {
  return i < a.n_src && a.match[i] >= 0 && !((double)a.d2[i] > a.mcd2);
}
// the kept pair of source point i goes to packed position pos
LLSR_HD void pack_write(const IcpArgs& a, int i, int pos) {
  const float* w = a.work4 + 4 * (size_t)i;
  const float* t = a.tgt4 + 4 * (size_t)a.match[i];
  float* s = a.ps4 + 4 * (size_t)pos;
  float* d = a.pd4 + 4 * (size_t)pos;
  s[0] = w[0]; s[1] = w[1]; s[2] = w[2]; s[3] = a.d2[i];
  d[0] = t[0]; d[1] = t[1]; d[2] = t[2]; d[3] = 0.0f;
}
// k_icp_means: lanes 0-2 the source means, 3-5 the target means, 6 the MSE sum
LLSR_HD void means_body(const IcpArgs& a, int lane) {
  const int n = a.st->n_pairs;
  if (n < 3 || lane > 6) return;
  const float inv_n = 1.0f / (float)n;
  if (lane < 3) a.st->sm[lane] = mean_chain(a.ps4 + lane, 0, n) * inv_n;
  else if (lane < 6) a.st->dm[lane - 3] = mean_chain(a.pd4 + (lane - 3), 0, n) * inv_n;
  else a.st->mse_sum = mse_chain(a.ps4 + 3, 0, n);
}
// k_icp_sigma: one lane per (depth block, entry)
LLSR_HD void sigma_body(const IcpArgs& a, int t) {
  if (t >= 9 * sigma_blocks_max(a.n_src)) return;
  int b, i, j, first, last;
  if (!sigma_lane(t, a.st->n_pairs, &b, &i, &j, &first, &last)) return;
  a.part[t] = sigma_chain(a.pd4 + i, a.st->dm[i], a.ps4 + j, a.st->sm[j], first, last);
}
// k_icp_finish, one lane: sigma from its blocks in order, the estimate, final, the count, the stop rule
LLSR_HD void finish_body(const IcpArgs& a) {
  IcpState* st = a.st;
  const int n = st->n_pairs;
  if (n < 3) {
    st->state = kStateNoCorrespondences;
    st->converged = 0;
    st->apply = 0;
    return;
  }
  const float inv_n = 1.0f / (float)n;
  const int kc = sigma_block(n);
  float sigma[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) sigma[e] = 0.0f;
  int b = 0;
  for (int k0 = 0; k0 < n; k0 += kc, ++b)
#pragma unroll
    for (int e = 0; e < 9; ++e) sigma[e] = sigma[e] + inv_n * a.part[9 * b + e];
  rigid_from_sigma(sigma, st->sm, st->dm, st->T);
  mul4_left(st->T, st->fin);
  st->apply = 1;
  ++st->iterations;
  stop_rule(st, a.max_iterations, a.eps_t, a.eps_f);
}
// k_icp_fit: thread per source point: the source moved by final in one step, its nearest d^2
LLSR_HD void fit_body(const IcpArgs& a, int i) {
  if (i >= a.n_src) return;
  float q[4];
  xf_rows(a.st->fin, a.src4 + 4 * (size_t)i, q);
  float* o = a.aligned4 + 4 * (size_t)i;
  o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
  int idx;
  float d;
  a.d2[i] = nn_search(a.tab, a.log2T, a.cells4, a.box, q[0], q[1], q[2], &idx, &d) ? d : -1.0f;
}
// k_icp_fitsum, one lane
LLSR_HD void fitsum_body(const IcpArgs& a) {
  int n = 0;
  a.st->fit_sum = fitness_chain(a.d2, 0, a.n_src, &n);
  a.st->n_fit = n;
}

// ---- the serial host side ---------------------------------------------------------------------------
// The target's grid in the layout of llsr_grid.h, built serially: cells claim table slots in point
// order, ranges are laid out in slot order, points are placed in point order (the order inside a
// cell never changes a result: ties go by the original index).
inline void grid_build_host(const float* tgt4, int n, int log2T, llsr::CellSlot* tab, float* cells4, int* box) {
  const uint32_t T = 1u << log2T, mask = T - 1u;
  for (uint32_t s = 0; s < T; ++s) tab[s] = {llsr::kCellEmpty, 0, 0};
  int* slot = n > 0 ? new int[n] : nullptr;
  for (int k = 0; k < n; ++k) {
    const float* p = tgt4 + 4 * (size_t)k;
    const uint64_t key = llsr::cell_key(llsr::cell_coord(p[0]), llsr::cell_coord(p[1]), llsr::cell_coord(p[2]));
    uint32_t h = llsr::cell_hash(key, log2T);
    while (tab[h].key != llsr::kCellEmpty && tab[h].key != key) h = (h + 1) & mask;
    tab[h].key = key;
    ++tab[h].count;
    slot[k] = (int)h;
  }
  int cursor = 0;
  for (uint32_t s = 0; s < T; ++s) {
    tab[s].start = tab[s].count > 0 ? cursor : 0;
    cursor += tab[s].count;
    tab[s].count = 0;
  }
  for (int k = 0; k < n; ++k) {
    llsr::CellSlot& c = tab[slot[k]];
    float* q = cells4 + 4 * (size_t)(c.start + c.count++);
    q[0] = tgt4[4 * (size_t)k];
    q[1] = tgt4[4 * (size_t)k + 1];
    q[2] = tgt4[4 * (size_t)k + 2];
    q[3] = llsr_libm::bitsf((uint32_t)k);
  }
  delete[] slot;
  box[0] = box[1] = box[2] = kBoxEmptyLo;
  box[3] = box[4] = box[5] = kBoxEmptyHi;
}

// ---- the batch form (DESIGN.md §16 "Batch form"): P alignments in one set of launches --------------
// Problem p has its own IcpArgs in a table; a batch kernel finds its problem from blockIdx.y and
// calls the body above on that entry, so a problem's sums, ties, stop rule and fitness are the single
// call's. What the batch adds is below: which blocks of a launch sized for the largest problem belong
// to a problem, which problems still take part in the loop, and where problem p's slices of the shared
// buffers lie.

// a block past the problem's own extent returns at once
LLSR_HD bool batch_block(int block, int n, int block_size) { return block < blocks_for(n, block_size); }
// a problem whose state has left kStateNone takes no further part in the loop kernels: its state,
// final and working cloud stay as the pass that finished it left them
LLSR_HD bool batch_live(const IcpArgs& a) { return a.st->state == kStateNone; }
// k_icp_init_b, one lane per problem
LLSR_HD void init_body(const IcpArgs& a) {
  state_init(a.st);
  a.box[0] = a.box[1] = a.box[2] = kBoxEmptyLo;
  a.box[3] = a.box[4] = a.box[5] = kBoxEmptyHi;
}
// k_icp_finish_b, one lane per problem: true when this pass ended the problem's loop (the caller
// takes it off the count of unfinished problems, an integer atomic on the device)
LLSR_HD bool finish_batch_body(const IcpArgs& a) {
  if (!batch_live(a)) return false;
  finish_body(a);
  return !batch_live(a);
}

// Launch extents of a batch: each sized for the largest problem
struct IcpBatchDims {
  int box_blocks, corr_blocks, sigma_blocks;
  int max_passes;  // max(1, largest max_iterations): the stop rule ends every problem by then
};
inline IcpBatchDims icp_batch_dims(const IcpArgs* tab, int P) {
  int ns = 0, nt = 0, it = 1;
  for (int p = 0; p < P; ++p) {
    if (tab[p].n_src > ns) ns = tab[p].n_src;
    if (tab[p].n_tgt > nt) nt = tab[p].n_tgt;
    if (tab[p].max_iterations > it) it = tab[p].max_iterations;
  }
  return {blocks_for(nt, kCorrBlock), blocks_for(ns, kCorrBlock), blocks_for(9 * sigma_blocks_max(ns), kCorrBlock), it};
}

// Element counts of the shared buffers of a batch and problem p's slices of them. The per-point
// buffers are laid out like the concatenated source (problem p at point src_off[p] - src_off[0]) with
// one point more at the end, so an empty problem's slice is still a live address; every problem's
// grid has the table size and the capacity of the largest target.
struct IcpBatchLayout {
  int P = 0, log2T = 0, cap = 0;         // cap = the largest target, log2T = grid_log2_table(cap)
  size_t tab = 0, cells = 0, points = 0, part = 0;  // slots, target points, source points, floats of `part`
};
inline IcpBatchLayout icp_batch_layout(int P, const int64_t* src_off, const int64_t* tgt_off) {
  IcpBatchLayout L;
  L.P = P;
  for (int p = 0; p < P; ++p) {
    const int nt = (int)(tgt_off[p + 1] - tgt_off[p]);
    if (nt > L.cap) L.cap = nt;
    L.part += 9 * (size_t)sigma_blocks_max((int)(src_off[p + 1] - src_off[p]));
  }
  L.log2T = llsr::grid_log2_table(L.cap);
  L.tab = (size_t)P << L.log2T;
  L.cells = (size_t)P * (size_t)(L.cap > 0 ? L.cap : 1);
  L.points = (size_t)(src_off[P] - src_off[0]) + 1;
  return L;
}
// The base pointers of the shared buffers (sizes in elements, from the layout)
struct IcpBatchBuffers {
  const float* src4;      // the concatenated sources from point src_off[0] on (unused when all are empty)
  const float* tgt4;      // the same for the targets
  llsr::CellSlot* tab;    // [L.tab]
  float* cells4;          // [L.cells][4]
  int* box;               // [6 P]
  float *work4, *ps4, *pd4;  // [L.points][4]
  int* match;             // [L.points]
  float* d2;              // [L.points]
  float* part;            // [L.part]
  IcpState* st;           // [P]
  float* aligned4;        // [L.points][4]; the working cloud serves when the caller wants no aligned cloud
};
// Fill entry p of the table (the parameters max_iterations, eps_*, mcd2 are the caller's); part_at is
// the running offset into `part`, advanced by the problem's share
inline void icp_batch_entry(const IcpBatchLayout& L, const IcpBatchBuffers& b, const int64_t* src_off,
                            const int64_t* tgt_off, int p, size_t* part_at, IcpArgs* a) {
  const size_t so = (size_t)(src_off[p] - src_off[0]), to = (size_t)(tgt_off[p] - tgt_off[0]);
  a->n_src = (int32_t)(src_off[p + 1] - src_off[p]);
  a->n_tgt = (int32_t)(tgt_off[p + 1] - tgt_off[p]);
  a->log2T = L.log2T;
  a->tab = b.tab + ((size_t)p << L.log2T);
  a->cells4 = b.cells4 + 4 * (size_t)p * (size_t)L.cap;
  a->box = b.box + 6 * (size_t)p;
  a->work4 = b.work4 + 4 * so;
  // an empty cloud is given the problem's own slice of the workspace, never a null or outside pointer
  a->src4 = a->n_src > 0 ? b.src4 + 4 * so : a->work4;
  a->tgt4 = a->n_tgt > 0 ? b.tgt4 + 4 * to : a->cells4;
  a->match = b.match + so;
  a->d2 = b.d2 + so;
  a->ps4 = b.ps4 + 4 * so;
  a->pd4 = b.pd4 + 4 * so;
  a->part = b.part + *part_at;
  *part_at += 9 * (size_t)sigma_blocks_max(a->n_src);
  a->st = b.st + p;
  a->aligned4 = b.aligned4 + 4 * so;
}

// The one serial driver: the batch launches of llsr_icp_align_batch as loops over their (block.x,
// block.y, thread) ranges calling the same bodies, over a table whose grids were built with
// grid_build_host at each entry's log2T. A single alignment is a table of one (llsr_icp_align_host),
// and that is also the serial statement of llsr_icp_align's launches: at P = 1 every extent is the
// problem's own and the problem is live until the loop ends. Returns the number of passes of the loop,
// or -1 when a problem is still unfinished after max_passes (which the stop rule excludes).
inline int icp_run_host(const IcpArgs* tab, int P) {
  const IcpBatchDims dims = icp_batch_dims(tab, P);
  int live = P;
  for (int p = 0; p < P; ++p) init_body(tab[p]);
  for (int p = 0; p < P; ++p)
    for (int blk = 0; blk < dims.box_blocks; ++blk) {
      const IcpArgs& a = tab[p];
      if (!batch_block(blk, a.n_tgt, kCorrBlock)) continue;
      for (int t = 0; t < kCorrBlock; ++t) {
        int c[3];
        if (!box_cell(a, point_of(blk, t, kCorrBlock), c)) continue;
        for (int k = 0; k < 3; ++k) {
          if (c[k] < a.box[k]) a.box[k] = c[k];
          if (c[k] > a.box[3 + k]) a.box[3 + k] = c[k];
        }
      }
    }
  for (int p = 0; p < P; ++p)
    for (size_t k = 0; k < 4 * (size_t)tab[p].n_src; ++k) tab[p].work4[k] = tab[p].src4[k];
  int passes = 0;
  while (live > 0) {
    if (passes >= dims.max_passes) return -1;
    ++passes;
    for (int p = 0; p < P; ++p)
      for (int blk = 0; blk < dims.corr_blocks; ++blk) {
        const IcpArgs& a = tab[p];
        if (!batch_live(a) || !batch_block(blk, a.n_src, kCorrBlock)) continue;
        for (int t = 0; t < kCorrBlock; ++t) corr_body(a, point_of(blk, t, kCorrBlock));
      }
    for (int p = 0; p < P; ++p) {
      const IcpArgs& a = tab[p];
      if (!batch_live(a)) continue;
      int pos = 0;  // the scan of k_icp_pack_b, serially
      for (int tile = 0; tile < blocks_for(a.n_src, kPackBlock); ++tile)
        for (int t = 0; t < kPackBlock; ++t) {
          const int i = point_of(tile, t, kPackBlock);
          if (pack_keep(a, i)) pack_write(a, i, pos++);
        }
      a.st->n_pairs = pos;
    }
    for (int p = 0; p < P; ++p)
      if (batch_live(tab[p]))
        for (int lane = 0; lane < kLaneBlock; ++lane) means_body(tab[p], lane);
    for (int p = 0; p < P; ++p)
      for (int blk = 0; blk < dims.sigma_blocks; ++blk) {
        const IcpArgs& a = tab[p];
        if (!batch_live(a) || !batch_block(blk, 9 * sigma_blocks_max(a.n_src), kCorrBlock)) continue;
        for (int t = 0; t < kCorrBlock; ++t) sigma_body(a, point_of(blk, t, kCorrBlock));
      }
    for (int p = 0; p < P; ++p)
      if (finish_batch_body(tab[p])) --live;
  }
  for (int p = 0; p < P; ++p)
    for (int blk = 0; blk < dims.corr_blocks; ++blk) {
      const IcpArgs& a = tab[p];
      if (!batch_block(blk, a.n_src, kCorrBlock)) continue;
      for (int t = 0; t < kCorrBlock; ++t) fit_body(a, point_of(blk, t, kCorrBlock));
    }
  for (int p = 0; p < P; ++p) fitsum_body(tab[p]);
  return passes;
}

// pcl::getTransformation(x, y, z, roll, pitch, yaw) as a row-major 3x4 (glibc float libm)
inline void get_transformation(float x, float y, float z, float roll, float pitch, float yaw, float* t) {
  const float A = cosf(yaw), B = sinf(yaw), C = cosf(pitch), D = sinf(pitch), E = cosf(roll), F = sinf(roll);
  const float DE = D * E, DF = D * F;
  t[0] = A * C; t[1] = A * DF - B * E; t[2] = B * F + A * DE; t[3] = x;
  t[4] = B * C; t[5] = A * E + B * DF; t[6] = B * DE - A * F; t[7] = y;
  t[8] = -D;    t[9] = C * F;          t[10] = C * E;         t[11] = z;
}
// pcl::getTranslationAndEulerAngles of a row-major matrix with row stride `ld`
inline void get_translation_and_euler(const float* t, int ld, float* o) {
  o[0] = t[3];
  o[1] = t[ld + 3];
  o[2] = t[2 * ld + 3];
  o[3] = atan2f(t[2 * ld + 1], t[2 * ld + 2]);
  o[4] = asinf(-t[2 * ld]);
  o[5] = atan2f(t[ld], t[0]);
}
// MO:1056-1081: pose_from = x, y, z, roll, pitch, yaw of tCorrect = correctionLidarFrame * tWrong;
// pose_to = z, x, y, yaw, roll, pitch of the closest key pose (pclPointTogtsamPose3's arguments)
inline void loop_constraint(const float* T16, const float* latest, const float* closest, double fitness,
                            float* pose_from, float* pose_to, float* variance) {
  float c[6];
  get_translation_and_euler(T16, 4, c);
  float L[12], W[12], R[12];
  get_transformation(c[2], c[0], c[1], c[5], c[3], c[4], L);
  get_transformation(latest[2], latest[0], latest[1], latest[5], latest[3], latest[4], W);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      R[4 * i + j] = (L[4 * i] * W[j] + L[4 * i + 1] * W[4 + j]) + L[4 * i + 2] * W[8 + j];
    R[4 * i + 3] = ((L[4 * i] * W[3] + L[4 * i + 1] * W[7]) + L[4 * i + 2] * W[11]) + L[4 * i + 3];
  }
  get_translation_and_euler(R, 4, pose_from);
  pose_to[0] = closest[2]; pose_to[1] = closest[0]; pose_to[2] = closest[1];
  pose_to[3] = closest[5]; pose_to[4] = closest[3]; pose_to[5] = closest[4];
  *variance = (float)fitness;
}
// MO:1038-1040 on rep->icp, and the constraint of an accepted alignment between the latest and the
// closest key pose (x, y, z, roll, pitch, yaw each)
inline void loop_accept(const llsr_loop_config* cfg, const float* latest6, const float* closest6,
                        llsr_loop_report* rep) {
  rep->accepted = rep->icp.converged && !(rep->icp.fitness > (double)cfg->fitness_score);
  if (rep->accepted)
    loop_constraint(rep->icp.T, latest6, closest6, rep->icp.fitness, rep->pose_from, rep->pose_to, &rep->variance);
}
}  // namespace llsr_loop
