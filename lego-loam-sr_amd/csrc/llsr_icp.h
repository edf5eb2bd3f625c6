// llsr_icp.h — the scalar side of the loop-closure ICP, written for host and device:
// the rigid estimate of one iteration (Eigen::umeyama without scaling, in float, with this project's
// own 3x3 two-sided Jacobi SVD) and the pose constraint of performLoopClosure (MO:1056-1081).
//
// PCL 1.10 and Eigen 3.3.7 are not available to check against, so every order of evaluation below
// is this project's statement (DESIGN.md §16 marks the choices); tests/_loop_closure.py restates
// the same specification independently and the two are compared bit for bit. No expression here
// may contract into an FMA (-ffp-contract=off on both sides).
#pragma once
#include <math.h>
#include <stdint.h>

#include "llsr_eigen.h"
#include "llsr_libm.h"

namespace llsr_icp {

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
}  // namespace llsr_icp
