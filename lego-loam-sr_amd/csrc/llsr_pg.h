// llsr_pg.h — the batched pose-graph optimiser, written once for host and device:
// P independent SE(3) graphs (a prior on pose 0, the odometry chain, loop factors), a batch
// Gauss-Newton in double over a block row-envelope Cholesky. Every line that touches the workspace is
// one LLSR_HD body below; llsr_pg.hip's kernels only map (block, thread) to the arguments of the
// *_thread functions, and pg_pass_host runs the same functions serially over the same ranges (the
// LLSR_PG_HOST graph and tests/native/pg_host_check.cpp).
//
// GTSAM is not available to check against, so every order of evaluation here is this project's
// statement (DESIGN.md §19 marks the choices); tests/_pose_graph.py restates the specification
// independently. No expression may contract into an FMA (-ffp-contract=off on both sides); the only
// library-like calls are IEEE sqrt and divide, correctly rounded on both sides.
//
// The double sin / cos / atan2 / acos below follow fdlibm (k_sin.c, k_cos.c, e_rem_pio2.c's medium
// path, s_atan.c, e_atan2.c, e_acos.c), whose notice is preserved as its licence requires:
//
//   ====================================================
//   Copyright (C) 1993 by Sun Microsystems, Inc. All rights reserved.
//
//   Developed at SunPro, a Sun Microsystems, Inc. business.
//   Permission to use, copy, modify, and distribute this
//   software is freely granted, provided that this notice
//   is preserved.
//   ====================================================
#pragma once
#include <stdint.h>
#include <string.h>

#include "llsr_libm.h"

namespace llsr_pgo {

// ---- double-precision elementary functions ---------------------------------------------------------
LLSR_HD uint64_t dbits(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint64_t)__double_as_longlong(x);
#else
  uint64_t u; memcpy(&u, &x, 8); return u;
#endif
}
LLSR_HD double bitsd(uint64_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double((long long)u);
#else
  double x; memcpy(&x, &u, 8); return x;
#endif
}
LLSR_HD int32_t hi32(double x) { return (int32_t)(dbits(x) >> 32); }
LLSR_HD double fabsd(double x) { return bitsd(dbits(x) & 0x7fffffffffffffffull); }
LLSR_HD double sqrtd(double x) { return __builtin_sqrt(x); }  // IEEE, correctly rounded on both sides
LLSR_HD bool finited(double x) { return (dbits(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
LLSR_HD double nand() { return bitsd(0x7ff8000000000000ull); }

// k_sin.c: sin(x + y) on |x| <= pi/4, y the tail of x (iy = 0: y is 0)
LLSR_HD double ksin(double x, double y, int iy) {
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
               S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const int32_t ix = hi32(x) & 0x7fffffff;
  if (ix < 0x3e400000) {  // |x| < 2^-27
    if ((int)x == 0) return x;
  }
  const double z = x * x;
  const double v = z * x;
  const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
  if (iy == 0) return x + v * (S1 + z * r);
  return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
// k_cos.c
LLSR_HD double kcos(double x, double y) {
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
               C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const int32_t ix = hi32(x) & 0x7fffffff;
  if (ix < 0x3e400000) {
    if ((int)x == 0) return 1.0;
  }
  const double z = x * x;
  const double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
  if (ix < 0x3FD33333) return 1.0 - (0.5 * z - (z * r - x * y));
  const double qx = ix > 0x3fe90000 ? 0.28125 : bitsd((uint64_t)(uint32_t)(ix - 0x00200000) << 32);
  const double hz = 0.5 * z - qx;
  const double a = 1.0 - qx;
  return a - (hz - (z * r - x * y));
}
// e_rem_pio2.c, the medium path (|x| < 2^20 pi/2) without its table short cut: x = n pi/2 + y0 + y1.
// Larger arguments are outside the optimiser's range (angles are bounded by a few pi): they give NaN.
LLSR_HD int rem_pio2(double x, double* y0, double* y1) {
  const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00,
               pio2_1t = 6.07710050650619224932e-11, pio2_2 = 6.07710050630396597660e-11,
               pio2_2t = 2.02226624879595063154e-21, pio2_3 = 2.02226624871116645580e-21,
               pio2_3t = 8.47842766036889956997e-32;
  const int32_t hx = hi32(x), ix = hx & 0x7fffffff;
  if (ix > 0x413921fb) {
    *y0 = *y1 = nand();
    return 0;
  }
  const double t0 = fabsd(x);
  const int n = (int)(t0 * invpio2 + 0.5);
  const double fn = (double)n;
  double r = t0 - fn * pio2_1;
  double w = fn * pio2_1t;
  const int j = ix >> 20;
  double y = r - w;
  int i = j - ((hi32(y) >> 20) & 0x7ff);
  if (i > 16) {  // the second iteration, good to 118 bits
    double t = r;
    w = fn * pio2_2;
    r = t - w;
    w = fn * pio2_2t - ((t - r) - w);
    y = r - w;
    i = j - ((hi32(y) >> 20) & 0x7ff);
    if (i > 49) {  // the third, 151 bits
      t = r;
      w = fn * pio2_3;
      r = t - w;
      w = fn * pio2_3t - ((t - r) - w);
      y = r - w;
    }
  }
  const double yt = (r - y) - w;
  if (hx < 0) {
    *y0 = -y;
    *y1 = -yt;
    return -n;
  }
  *y0 = y;
  *y1 = yt;
  return n;
}
LLSR_HD double sind(double x) {
  const int32_t ix = hi32(x) & 0x7fffffff;
  if (ix <= 0x3fe921fb) return ksin(x, 0.0, 0);
  if (ix >= 0x7ff00000) return x - x;
  double y0, y1;
  const int n = rem_pio2(x, &y0, &y1) & 3;
  return n == 0 ? ksin(y0, y1, 1) : n == 1 ? kcos(y0, y1) : n == 2 ? -ksin(y0, y1, 1) : -kcos(y0, y1);
}
LLSR_HD double cosd(double x) {
  const int32_t ix = hi32(x) & 0x7fffffff;
  if (ix <= 0x3fe921fb) return kcos(x, 0.0);
  if (ix >= 0x7ff00000) return x - x;
  double y0, y1;
  const int n = rem_pio2(x, &y0, &y1) & 3;
  return n == 0 ? kcos(y0, y1) : n == 1 ? -ksin(y0, y1, 1) : n == 2 ? -kcos(y0, y1) : ksin(y0, y1, 1);
}
// s_atan.c
LLSR_HD double atand(double x) {
  const double aT0 = 3.33333333333329318027e-01, aT1 = -1.99999999998764832476e-01, aT2 = 1.42857142725034663711e-01,
               aT3 = -1.11111104054623557880e-01, aT4 = 9.09088713343650656196e-02, aT5 = -7.69187620504482999495e-02,
               aT6 = 6.66107313738753120669e-02, aT7 = -5.83357013379057348645e-02, aT8 = 4.97687799461593236017e-02,
               aT9 = -3.65315727442169155270e-02, aT10 = 1.62858201153657823623e-02;
  const int32_t hx = hi32(x), ix = hx & 0x7fffffff;
  if (ix >= 0x44100000) {  // |x| >= 2^66
    if (!finited(x) && (dbits(x) & 0x000fffffffffffffull)) return x + x;
    const double z = 1.57079632679489655800e+00 + 6.12323399573676603587e-17;
    return hx > 0 ? z : -z;
  }
  int id;
  if (ix < 0x3fdc0000) {  // |x| < 0.4375
    if (ix < 0x3e200000) return x;  // |x| < 2^-29
    id = -1;
  } else {
    x = fabsd(x);
    if (ix < 0x3ff30000) {  // |x| < 1.1875
      if (ix < 0x3fe60000) {
        id = 0;
        x = (2.0 * x - 1.0) / (2.0 + x);
      } else {
        id = 1;
        x = (x - 1.0) / (x + 1.0);
      }
    } else if (ix < 0x40038000) {  // |x| < 2.4375
      id = 2;
      x = (x - 1.5) / (1.0 + 1.5 * x);
    } else {
      id = 3;
      x = -1.0 / x;
    }
  }
  const double z = x * x;
  const double w = z * z;
  const double s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
  const double s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
  if (id < 0) return x - x * (s1 + s2);
  const double hi = id == 0   ? 4.63647609000806093515e-01
                    : id == 1 ? 7.85398163397448278999e-01
                    : id == 2 ? 9.82793723247329054082e-01
                              : 1.57079632679489655800e+00;
  const double lo = id == 0   ? 2.26987774529616870924e-17
                    : id == 1 ? 3.06161699786838301793e-17
                    : id == 2 ? 1.39033110312309984516e-17
                              : 6.12323399573676603587e-17;
  const double r = hi - ((x * (s1 + s2) - lo) - x);
  return hx < 0 ? -r : r;
}
// e_atan2.c
LLSR_HD double atan2d(double y, double x) {
  const double tiny = 1.0e-300, pi_o_4 = 7.8539816339744827900E-01, pi_o_2 = 1.5707963267948965580E+00,
               pi = 3.1415926535897931160E+00, pi_lo = 1.2246467991473531772E-16;
  if (x != x || y != y) return x + y;
  const int32_t hx = hi32(x), hy = hi32(y), ix = hx & 0x7fffffff, iy = hy & 0x7fffffff;
  if (x == 1.0) return atand(y);
  const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);  // 2 * sign(x) + sign(y)
  if (y == 0.0) return m == 0 || m == 1 ? y : m == 2 ? pi + tiny : -pi - tiny;
  if (x == 0.0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
  if (!finited(x)) {
    if (!finited(y)) return m == 0 ? pi_o_4 + tiny : m == 1 ? -pi_o_4 - tiny : m == 2 ? 3.0 * pi_o_4 + tiny : -3.0 * pi_o_4 - tiny;
    return m == 0 ? 0.0 : m == 1 ? -0.0 : m == 2 ? pi + tiny : -pi - tiny;
  }
  if (!finited(y)) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
  const int k = (iy - ix) >> 20;
  double z;
  if (k > 60) z = pi_o_2 + 0.5 * pi_lo;
  else if (hx < 0 && k < -60) z = 0.0;
  else z = atand(fabsd(y / x));
  return m == 0 ? z : m == 1 ? -z : m == 2 ? pi - (z - pi_lo) : (z - pi_lo) - pi;
}
// e_acos.c
LLSR_HD double acosd(double x) {
  const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17,
               pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
               pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
               qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
               qS4 = 7.70381505559019352791e-02;
  const int32_t hx = hi32(x), ix = hx & 0x7fffffff;
  if (ix >= 0x3ff00000) {  // |x| >= 1
    if (x == 1.0) return 0.0;
    if (x == -1.0) return 3.14159265358979311600e+00 + 2.0 * pio2_lo;
    return nand();
  }
  if (ix < 0x3fe00000) {  // |x| < 0.5
    if (ix <= 0x3c600000) return pio2_hi + pio2_lo;
    const double z = x * x;
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double r = p / q;
    return pio2_hi - (x - (pio2_lo - x * r));
  }
  if (hx < 0) {  // x < -0.5
    const double z = (1.0 + x) * 0.5;
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double s = sqrtd(z);
    const double r = p / q;
    const double w = r * s - pio2_lo;
    return 3.14159265358979311600e+00 - 2.0 * (s + w);
  }
  const double z = (1.0 - x) * 0.5;  // x > 0.5
  const double s = sqrtd(z);
  const double df = bitsd(dbits(s) & 0xffffffff00000000ull);
  const double c = (z - df * df) / (s + df);
  const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
  const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
  const double r = p / q;
  const double w = r * s + c;
  return 2.0 * (df + w);
}

// ---- SO(3) / SE(3) ------------------------------------------------------------------------------------
// A pose is 12 doubles: R row-major (9), then t (3).
LLSR_HD void mat_mul(const double* A, const double* B, double* C) {  // C = A B
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
LLSR_HD void mat_tmul(const double* A, const double* B, double* C) {  // C = A^T B
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[r] * B[c] + A[3 + r] * B[3 + c]) + A[6 + r] * B[6 + c];
}
LLSR_HD void mat_tvec(const double* A, const double* v, double* o) {  // o = A^T v
  for (int r = 0; r < 3; ++r) o[r] = (A[r] * v[0] + A[3 + r] * v[1]) + A[6 + r] * v[2];
}
LLSR_HD void mat_vec(const double* A, const double* v, double* o) {  // o = A v
  for (int r = 0; r < 3; ++r) o[r] = (A[3 * r] * v[0] + A[3 * r + 1] * v[1]) + A[3 * r + 2] * v[2];
}
// Rot3::RzRyRx(a, b, c) = Rz(c) Ry(b) Rx(a)
LLSR_HD void rot_rzryrx(double a, double b, double c, double* R) {
  const double sx = sind(a), cx = cosd(a), sy = sind(b), cy = cosd(b), sz = sind(c), cz = cosd(c);
  R[0] = cy * cz; R[1] = sx * sy * cz - cx * sz; R[2] = sx * sz + cx * sy * cz;
  R[3] = cy * sz; R[4] = cx * cz + sx * sy * sz; R[5] = cx * sy * sz - sx * cz;
  R[6] = -sy;     R[7] = sx * cy;                R[8] = cx * cy;
}
// the angles of RzRyRx back from the matrix (a choice)
LLSR_HD void rot_angles(const double* R, double* a, double* b, double* c) {
  *a = atan2d(R[7], R[8]);
  *b = atan2d(-R[6], sqrtd(R[7] * R[7] + R[8] * R[8]));
  *c = atan2d(R[3], R[0]);
}
// GTSAM order g = (tx, ty, tz, a, b, c) -> Pose3(RzRyRx(a, b, c), Point3(tx, ty, tz)), floats widened
LLSR_HD void pose_from_gtsam6(const float* g, double* T) {
  rot_rzryrx((double)g[3], (double)g[4], (double)g[5], T);
  T[9] = (double)g[0]; T[10] = (double)g[1]; T[11] = (double)g[2];
}
// a store pose s = (x, y, z, roll, pitch, yaw) -> Pose3(RzRyRx(yaw, roll, pitch), Point3(z, x, y))
LLSR_HD void pose_from_store6(const float* s, double* T) {
  const float g[6] = {s[2], s[0], s[1], s[5], s[3], s[4]};
  pose_from_gtsam6(g, T);
}
// MO:1692-1705 / 1765-1780, narrowed to float
LLSR_HD void pose_to_store6(const double* T, float* s) {
  double a, b, c;
  rot_angles(T, &a, &b, &c);
  s[0] = (float)T[10]; s[1] = (float)T[11]; s[2] = (float)T[9];
  s[3] = (float)b; s[4] = (float)c; s[5] = (float)a;
}
LLSR_HD void pose_between(const double* Ti, const double* Tj, double* H) {  // Ti^-1 Tj
  mat_tmul(Ti, Tj, H);
  const double d[3] = {Tj[9] - Ti[9], Tj[10] - Ti[10], Tj[11] - Ti[11]};
  mat_tvec(Ti, d, H + 9);
}
LLSR_HD void skew(const double* w, double* S) {
  S[0] = 0.0; S[1] = -w[2]; S[2] = w[1];
  S[3] = w[2]; S[4] = 0.0; S[5] = -w[0];
  S[6] = -w[1]; S[7] = w[0]; S[8] = 0.0;
}
// I + A [w]x + B [w]x^2
LLSR_HD void rodrigues(const double* w, double A, double B, double* R) {
  double S[9], S2[9];
  skew(w, S);
  mat_mul(S, S, S2);
  for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + A * S[k]) + B * S2[k];
}
LLSR_HD void so3_exp(const double* w, double* R) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  double A, B;
  if (t2 < 1e-6) {
    A = 1.0 - t2 * (1.0 / 6.0 - t2 * (1.0 / 120.0));
    B = 0.5 - t2 * (1.0 / 24.0 - t2 * (1.0 / 720.0));
  } else {
    const double t = sqrtd(t2);
    A = sind(t) / t;
    B = (1.0 - cosd(t)) / t2;
  }
  rodrigues(w, A, B, R);
}
// theta = atan2(|v| / 2, (tr - 1) / 2) with v = (R - R^T)^vee, w = v theta / |v|; within 1e-6 of pi the
// axis comes from the diagonal
LLSR_HD void so3_log(const double* R, double* w) {
  const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double s2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];  // 4 sin^2
  const double s = 0.5 * sqrtd(s2);
  if (s < 1e-6 && c < 0.0) {
    const double t = atan2d(s, c);
    // (written without a run-time index into R, which would put the matrix into LDS or scratch)
    const int k = R[0] >= R[4] ? (R[0] >= R[8] ? 0 : 2) : (R[4] >= R[8] ? 1 : 2);
    const double rkk = k == 0 ? R[0] : k == 1 ? R[4] : R[8];
    const double s01 = 0.5 * (R[1] + R[3]), s02 = 0.5 * (R[2] + R[6]), s12 = 0.5 * (R[5] + R[7]);
    const double d = sqrtd(fabsd((rkk - c) / (1.0 - c))), q = (1.0 - c) * d;
    const double ax[3] = {k == 0 ? d : (k == 1 ? s01 : s02) / q, k == 1 ? d : (k == 0 ? s01 : s12) / q,
                          k == 2 ? d : (k == 0 ? s02 : s12) / q};
    const double sg = (v[0] * ax[0] + v[1] * ax[1]) + v[2] * ax[2] < 0.0 ? -1.0 : 1.0;
    for (int m = 0; m < 3; ++m) w[m] = sg * t * ax[m];
    return;
  }
  double f;
  if (s2 < 4e-6 && c > 0.0) {
    const double t2 = s * s;  // sin^2 ~ theta^2: theta / sin = 1 + s^2/6 + 3 s^4/40
    f = 0.5 * (1.0 + t2 * (1.0 / 6.0 + t2 * (3.0 / 40.0)));
  } else {
    f = atan2d(s, c) / (2.0 * s);
  }
  for (int m = 0; m < 3; ++m) w[m] = f * v[m];
}
// the inverse of SO(3)'s right Jacobian: I + [w]x / 2 + g(theta) [w]x^2,
// g = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta) -> 1/12 + theta^2/720 + theta^4/30240
LLSR_HD void so3_jr_inv(const double* w, double* J) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  double g;
  if (t2 < 1e-4) {
    g = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0));
  } else {
    const double t = sqrtd(t2);
    g = 1.0 / t2 - (1.0 + cosd(t)) / ((2.0 * t) * sind(t));
  }
  rodrigues(w, 0.5, g, J);
}
LLSR_HD void pose_retract(const double* T, const double* d, double* O) {  // R Exp(d[0..2]), t + R d[3..5]
  double E[9], Rv[3];
  so3_exp(d, E);
  mat_vec(T, d + 3, Rv);
  const double t[3] = {T[9] + Rv[0], T[10] + Rv[1], T[11] + Rv[2]};
  double Rn[9];
  mat_mul(T, E, Rn);
  for (int k = 0; k < 9; ++k) O[k] = Rn[k];
  O[9] = t[0]; O[10] = t[1]; O[11] = t[2];
}
// The error of measurement Z against h and what the Jacobians share: e = [Log(Zr^T hr), Zr^T (ht - Zt)],
// E = Zr^T hr.
LLSR_HD void pose_error(const double* Z, const double* H, double* e, double* E) {
  mat_tmul(Z, H, E);
  so3_log(E, e);
  const double d[3] = {H[9] - Z[9], H[10] - Z[10], H[11] - Z[11]};
  mat_tvec(Z, d, e + 3);
}

// ---- the workspace -------------------------------------------------------------------------------------
constexpr int kBlock = 64;        // threads per block of every kernel; k_pg_solve's one wave
constexpr int kRun = -1;          // PgState::state while the problem iterates
constexpr int kStateClean = 0, kStateAbs = 1, kStateRel = 2, kStateIter = 3, kStateRose = 4, kStateFailed = 5;

struct PgProblem {  // one per problem, rebuilt by the host before every optimise
  int32_t K, L;     // poses, loop factors
  int32_t nlong;    // block rows whose envelope starts before their left neighbour
  int32_t run;      // this optimise works on the problem (it has a loop factor since the last one)
};
struct PgState {
  int32_t state, iterations, stop_pass, pad;
  double err0, err;  // the error at the start, at the iterate kept
};
// Capacities per problem: maxK poses, maxL loops, maxE envelope blocks; factor f of problem p is
// p (maxK + maxL) + f with f = 0 the prior, 1 .. K - 1 the odometry (f - 1 -> f), K + l loop l.
struct PgArgs {
  int32_t P, maxK, maxL, pass;
  int64_t maxE;
  int32_t max_iterations, pad;
  double rel_tol, abs_tol;
  const PgProblem* prob;  // [P]
  PgState* st;            // [P]
  int32_t* live;          // [1] problems still iterating
  double* X;              // [P maxK 12] the iterate
  double* Xprev;          // [P maxK 12] the iterate before the last step
  const double* Z;        // [P (maxK + maxL) 12] measurements
  const double* winv;     // [P (maxK + maxL) 6] 1 / sigma
  const int32_t* loops;   // [P maxL 2] from, to
  const int32_t* c0;      // [P maxK] first block column of block row r
  const int64_t* rowoff;  // [P maxK] blocks before block row r in the problem's envelope
  const int32_t* longrow; // [P maxL] the long block rows, ascending
  double* res;            // [P (maxK + maxL) 6] whitened residuals
  double* J;              // [P (maxK + maxL) 72] whitened Jacobians: wrt the first pose, wrt the second
  double* eterm;          // [P (maxK + maxL)] half the squared whitened residual
  double* H;              // [P maxE 36] the envelope: block row r is 6 scalar rows of 6 (r - c0 + 1) each
  double* d;              // [P maxK 6] the right-hand side, then the step
  float* out6;            // [P maxK 6] the iterate in the store's layout
};
struct PgSizes {  // elements of each buffer above
  size_t prob, st, X, Z, winv, loops, c0, rowoff, longrow, res, J, eterm, H, d, out6;
};
inline PgSizes pg_sizes(int P, int maxK, int maxL, int64_t maxE) {
  const size_t nP = (size_t)P, F = nP * ((size_t)maxK + (size_t)maxL), Kt = nP * (size_t)maxK, Lt = nP * (size_t)maxL;
  PgSizes z;
  z.prob = z.st = nP;
  z.X = 12 * Kt; z.Z = 12 * F; z.winv = 6 * F; z.loops = 2 * Lt; z.c0 = z.rowoff = Kt; z.longrow = Lt;
  z.res = 6 * F; z.J = 72 * F; z.eterm = F; z.H = 36 * nP * (size_t)maxE; z.d = 6 * Kt; z.out6 = 6 * Kt;
  return z;
}

// The iterate differs from the start once a step was kept: one iteration, two when the last one was
// taken back.
LLSR_HD bool pg_moved(const PgState& s) { return s.iterations >= (s.state == kStateRose ? 2 : 1); }
LLSR_HD bool pg_running(const PgArgs& a, int p) { return a.prob[p].run && a.st[p].state == kRun; }
LLSR_HD size_t pg_fac(const PgArgs& a, int p, int f) { return (size_t)p * ((size_t)a.maxK + (size_t)a.maxL) + (size_t)f; }
LLSR_HD size_t pg_pose(const PgArgs& a, int p, int k) { return (size_t)p * (size_t)a.maxK + (size_t)k; }
LLSR_HD void pg_stop(const PgArgs& a, int p, int state) {
  a.st[p].state = state;
  a.st[p].stop_pass = a.pass;
#if defined(__HIP_DEVICE_COMPILE__)
  atomicSub(a.live, 1);
#else
  *a.live -= 1;
#endif
}
// the poses of factor f: i = -1 for the prior
LLSR_HD void pg_factor_poses(const PgArgs& a, int p, int f, int* i, int* j) {
  const int K = a.prob[p].K;
  if (f == 0) { *i = -1; *j = 0; }
  else if (f < K) { *i = f - 1; *j = f; }
  else { const int32_t* l = a.loops + 2 * ((size_t)p * (size_t)a.maxL + (size_t)(f - K)); *i = l[0]; *j = l[1]; }
}

// k_pg_linearize: factor f of problem p at the iterate
LLSR_HD void pg_linearize(const PgArgs& a, int p, int f) {
  int i, j;
  pg_factor_poses(a, p, f, &i, &j);
  const size_t F = pg_fac(a, p, f);
  const double* Z = a.Z + 12 * F;
  const double* Tj = a.X + 12 * pg_pose(a, p, j);
  double Hm[12], e[6], E[9], Jri[9];
  if (i < 0) for (int k = 0; k < 12; ++k) Hm[k] = Tj[k];
  else pose_between(a.X + 12 * pg_pose(a, p, i), Tj, Hm);
  pose_error(Z, Hm, e, E);
  so3_jr_inv(e, Jri);
  const double* wi = a.winv + 6 * F;
  double* J1 = a.J + 72 * F;  // [6][6] row-major, wrt pose i
  double* J2 = J1 + 36;       // wrt pose j
  double half = 0.0;
  for (int r = 0; r < 6; ++r) {
    const double er = e[r] * wi[r];
    a.res[6 * F + r] = er;
    half = half + er * er;
  }
  a.eterm[F] = 0.5 * half;
  // wrt j: [[Jr^-1, 0], [0, E]]
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      J2[6 * r + c] = Jri[3 * r + c] * wi[r];
      J2[6 * r + 3 + c] = 0.0;
      J2[6 * (3 + r) + c] = 0.0;
      J2[6 * (3 + r) + 3 + c] = E[3 * r + c] * wi[3 + r];
    }
  if (i < 0) {
    for (int k = 0; k < 36; ++k) J1[k] = 0.0;
    return;
  }
  // wrt i: [[-Jr^-1 hr^T, 0], [Zr^T [ht]x, -Zr^T]]
  double A[9], S[9], B[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)  // Jri hr^T
      A[3 * r + c] = (Jri[3 * r] * Hm[3 * c] + Jri[3 * r + 1] * Hm[3 * c + 1]) + Jri[3 * r + 2] * Hm[3 * c + 2];
  skew(Hm + 9, S);
  mat_tmul(Z, S, B);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      J1[6 * r + c] = -A[3 * r + c] * wi[r];
      J1[6 * r + 3 + c] = 0.0;
      J1[6 * (3 + r) + c] = B[3 * r + c] * wi[3 + r];
      J1[6 * (3 + r) + 3 + c] = -Z[3 * c + r] * wi[3 + r];
    }
}

// column ca of Ja . column cb of Jb (whitened 6x6 blocks), rows ascending
LLSR_HD double pg_col_dot(const double* Ja, int ca, const double* Jb, int cb) {
  double s = Ja[ca] * Jb[cb];
  for (int k = 1; k < 6; ++k) s = s + Ja[6 * k + ca] * Jb[6 * k + cb];
  return s;
}
LLSR_HD double pg_col_res(const double* Ja, int ca, const double* r) {
  double s = Ja[ca] * r[0];
  for (int k = 1; k < 6; ++k) s = s + Ja[6 * k + ca] * r[k];
  return s;
}
// k_pg_assemble: entry e of block row r. e < 36 nb: scalar row e / w, column e % w of the envelope
// (w = 6 nb, nb = r - c0 + 1); the last 6: the right-hand side -A^T e. Factors in the order prior,
// odometry in, odometry out, loops by insertion.
LLSR_HD void pg_assemble(const PgArgs& a, int p, int r, int e) {
  const int K = a.prob[p].K, L = a.prob[p].L;
  const size_t R = pg_pose(a, p, r);
  const int c0 = a.c0[R], nb = r - c0 + 1, w = 6 * nb;
  const double* J = a.J + 72 * pg_fac(a, p, 0);
  const int32_t* lp = a.loops + 2 * (size_t)p * (size_t)a.maxL;
  double acc = 0.0;
  if (e >= 36 * nb) {
    const int k = e - 36 * nb;
    const double* res = a.res + 6 * pg_fac(a, p, 0);
    if (r == 0) acc = acc + pg_col_res(J + 36, k, res);
    if (r >= 1) acc = acc + pg_col_res(J + 72 * (size_t)r + 36, k, res + 6 * (size_t)r);
    if (r + 1 < K) acc = acc + pg_col_res(J + 72 * (size_t)(r + 1), k, res + 6 * (size_t)(r + 1));
    for (int l = 0; l < L; ++l) {
      const size_t f = (size_t)(K + l);
      if (lp[2 * l] == r) acc = acc + pg_col_res(J + 72 * f, k, res + 6 * f);
      if (lp[2 * l + 1] == r) acc = acc + pg_col_res(J + 72 * f + 36, k, res + 6 * f);
    }
    a.d[6 * R + k] = -acc;
    return;
  }
  const int k = e / w, m = e % w, c = c0 + m / 6, b = m % 6;
  if (c == r) {
    if (r == 0) acc = acc + pg_col_dot(J + 36, k, J + 36, b);
    if (r >= 1) acc = acc + pg_col_dot(J + 72 * (size_t)r + 36, k, J + 72 * (size_t)r + 36, b);
    if (r + 1 < K) acc = acc + pg_col_dot(J + 72 * (size_t)(r + 1), k, J + 72 * (size_t)(r + 1), b);
    for (int l = 0; l < L; ++l) {
      const double* Jl = J + 72 * (size_t)(K + l);
      if (lp[2 * l] == r) acc = acc + pg_col_dot(Jl, k, Jl, b);
      if (lp[2 * l + 1] == r) acc = acc + pg_col_dot(Jl + 36, k, Jl + 36, b);
    }
  } else {
    if (c == r - 1) acc = acc + pg_col_dot(J + 72 * (size_t)r + 36, k, J + 72 * (size_t)r, b);
    for (int l = 0; l < L; ++l) {
      const double* Jl = J + 72 * (size_t)(K + l);
      if (lp[2 * l] == r && lp[2 * l + 1] == c) acc = acc + pg_col_dot(Jl, k, Jl + 36, b);
      if (lp[2 * l + 1] == r && lp[2 * l] == c) acc = acc + pg_col_dot(Jl + 36, k, Jl, b);
    }
  }
  a.H[36 * ((size_t)p * (size_t)a.maxE + (size_t)a.rowoff[R]) + (size_t)k * (size_t)w + (size_t)m] = acc;
}

// ---- the envelope Cholesky, in scalar rows and columns -----------------------------------------------
// Scalar row i lives in block row i / 6 and starts at column first(i) = 6 c0. L overwrites the lower
// triangle of H. Every inner product starts from the entry of H and subtracts its products in
// ascending column order.
struct PgRow {
  double* at;  // at[j] is entry (i, j) for first <= j <= 6 (i / 6) + 5
  int first;
};
LLSR_HD PgRow pg_row(const PgArgs& a, int p, int i) {
  const int r = i / 6, k = i % 6;
  const size_t R = pg_pose(a, p, r);
  const int c0 = a.c0[R], w = 6 * (r - c0 + 1);
  PgRow o;
  o.first = 6 * c0;
  o.at = a.H + 36 * ((size_t)p * (size_t)a.maxE + (size_t)a.rowoff[R]) + (size_t)k * (size_t)w - (size_t)o.first;
  return o;
}
// lane 0 of column j: the pivot, and the forward substitution's y[j]
LLSR_HD void pg_chol_diag(const PgArgs& a, int p, int j) {
  const PgRow rj = pg_row(a, p, j);
  double acc = rj.at[j];
  for (int k = rj.first; k < j; ++k) acc = acc - rj.at[k] * rj.at[k];
  if (!(finited(acc) && acc > 0.0)) {
    pg_stop(a, p, kStateFailed);
    return;
  }
  const double l = sqrtd(acc);
  rj.at[j] = l;
  double* d = a.d + 6 * pg_pose(a, p, 0);
  d[j] = d[j] / l;
}
// The rows below the pivot of column j that hold it, by slot: 0 .. 10 the rest of the block row and
// the next block row, 11 + 6 q + k scalar row k of long row q (when it is further down and reaches
// back to the column's block). -1: no row.
LLSR_HD int pg_col_slots(const PgArgs& a, int p) { return 11 + 6 * a.prob[p].nlong; }
LLSR_HD int pg_col_row(const PgArgs& a, int p, int j, int slot) {
  const int K = a.prob[p].K, bj = j / 6;
  if (slot < 11) {
    const int i = j + 1 + slot, end = 6 * (bj + 2 < K ? bj + 2 : K);
    return i < end ? i : -1;
  }
  const int q = (slot - 11) / 6, k = (slot - 11) % 6;
  const int r = a.longrow[(size_t)p * (size_t)a.maxL + (size_t)q];
  if (r <= bj + 1 || a.c0[pg_pose(a, p, r)] > bj) return -1;
  return 6 * r + k;
}
// entry (i, j) of L, i > j, and row i's share of the forward substitution
LLSR_HD void pg_chol_col(const PgArgs& a, int p, int j, int i) {
  const PgRow ri = pg_row(a, p, i), rj = pg_row(a, p, j);
  double acc = ri.at[j];
  for (int k = ri.first > rj.first ? ri.first : rj.first; k < j; ++k) acc = acc - ri.at[k] * rj.at[k];
  const double l = acc / rj.at[j];
  ri.at[j] = l;
  double* d = a.d + 6 * pg_pose(a, p, 0);
  d[i] = d[i] - l * d[j];
}
// the back substitution L^T x = y by rows of L from the bottom
LLSR_HD void pg_back_diag(const PgArgs& a, int p, int k) {
  const PgRow rk = pg_row(a, p, k);
  double* d = a.d + 6 * pg_pose(a, p, 0);
  d[k] = d[k] / rk.at[k];
}
LLSR_HD void pg_back_col(const PgArgs& a, int p, int k, int i) {
  const PgRow rk = pg_row(a, p, k);
  double* d = a.d + 6 * pg_pose(a, p, 0);
  d[i] = d[i] - rk.at[i] * d[k];
}

// k_pg_update: pose k. A running problem keeps the iterate and steps; a problem whose error rose in
// this pass takes the kept iterate back.
LLSR_HD void pg_update(const PgArgs& a, int p, int k) {
  const size_t R = pg_pose(a, p, k);
  double* X = a.X + 12 * R;
  double* Xp = a.Xprev + 12 * R;
  if (a.st[p].state == kRun) {
    double O[12];
    pose_retract(X, a.d + 6 * R, O);
    for (int m = 0; m < 12; ++m) { Xp[m] = X[m]; X[m] = O[m]; }
  } else if (a.st[p].state == kStateRose && a.st[p].stop_pass == a.pass) {
    for (int m = 0; m < 12; ++m) X[m] = Xp[m];
  } else {
    return;
  }
  pose_to_store6(X, a.out6 + 6 * R);
}

// k_pg_error: the error of problem p at the iterate and the stop rule
LLSR_HD void pg_error(const PgArgs& a, int p) {
  const int nf = a.prob[p].K + a.prob[p].L;
  const double* t = a.eterm + pg_fac(a, p, 0);
  double sum = 0.0;
  for (int f = 0; f < nf; ++f) sum = sum + t[f];
  PgState& s = a.st[p];
  s.iterations = a.pass;
  if (a.pass == 0) {
    s.err0 = s.err = sum;
    if (a.max_iterations <= 0) pg_stop(a, p, kStateIter);
    return;
  }
  const double old = s.err;
  if (!(sum <= old)) {  // the error rose (or is no number): the iterate before stays
    pg_stop(a, p, kStateRose);
    return;
  }
  s.err = sum;
  const double dec = old - sum;
  if (dec < a.abs_tol) pg_stop(a, p, kStateAbs);
  else if (dec / old < a.rel_tol) pg_stop(a, p, kStateRel);
  else if (a.pass >= a.max_iterations) pg_stop(a, p, kStateIter);
}

// ---- what a thread does: the whole of every kernel but its built-in indices --------------------------
LLSR_HD void pg_linearize_thread(const PgArgs& a, int bx, int by, int tid) {
  const int p = by, f = bx * kBlock + tid;
  if (p >= a.P || !pg_running(a, p) || f >= a.prob[p].K + a.prob[p].L) return;
  pg_linearize(a, p, f);
}
LLSR_HD void pg_error_thread(const PgArgs& a, int bx, int tid) {
  const int p = bx * kBlock + tid;
  if (p >= a.P || !pg_running(a, p)) return;
  pg_error(a, p);
}
LLSR_HD void pg_assemble_thread(const PgArgs& a, int bx, int by, int tid) {
  const int p = by, r = bx;
  if (p >= a.P || !pg_running(a, p) || r >= a.prob[p].K) return;
  const int n = 36 * (r - a.c0[pg_pose(a, p, r)] + 1) + 6;
  for (int e = tid; e < n; e += kBlock) pg_assemble(a, p, r, e);
}
LLSR_HD void pg_update_thread(const PgArgs& a, int bx, int by, int tid) {
  const int p = by, k = bx * kBlock + tid;
  if (p >= a.P || !a.prob[p].run || k >= a.prob[p].K) return;
  pg_update(a, p, k);
}
// k_pg_solve's four phases; a barrier of the wave stands between two of them
LLSR_HD void pg_solve_diag_lane(const PgArgs& a, int p, int j, int lane) {
  if (lane == 0) pg_chol_diag(a, p, j);
}
LLSR_HD void pg_solve_col_lane(const PgArgs& a, int p, int j, int lane) {
  const int n = pg_col_slots(a, p);
  for (int s = lane; s < n; s += kBlock) {
    const int i = pg_col_row(a, p, j, s);
    if (i >= 0) pg_chol_col(a, p, j, i);
  }
}
LLSR_HD void pg_back_diag_lane(const PgArgs& a, int p, int k, int lane) {
  if (lane == 0) pg_back_diag(a, p, k);
}
LLSR_HD void pg_back_col_lane(const PgArgs& a, int p, int k, int lane) {
  for (int i = pg_row(a, p, k).first + lane; i < k; i += kBlock) pg_back_col(a, p, k, i);
}

// ---- the launches ---------------------------------------------------------------------------------------
struct PgDims {
  int fac_blocks, rows, pose_blocks, prob_blocks;
};
inline PgDims pg_dims(const PgProblem* prob, int P) {
  int mf = 1, mk = 1;
  for (int p = 0; p < P; ++p)
    if (prob[p].run) {
      mf = prob[p].K + prob[p].L > mf ? prob[p].K + prob[p].L : mf;
      mk = prob[p].K > mk ? prob[p].K : mk;
    }
  PgDims d;
  d.fac_blocks = (mf + kBlock - 1) / kBlock;
  d.rows = mk;
  d.pose_blocks = (mk + kBlock - 1) / kBlock;
  d.prob_blocks = (P + kBlock - 1) / kBlock;
  return d;
}
// k_pg_solve's block p over heap buffers, its lanes one after the other between two barriers
inline void pg_solve_host(const PgArgs& a, int p) {
  if (!pg_running(a, p)) return;
  const int n = 6 * a.prob[p].K;
  for (int j = 0; j < n; ++j) {
    for (int lane = 0; lane < kBlock; ++lane) pg_solve_diag_lane(a, p, j, lane);
    if (a.st[p].state != kRun) return;
    for (int lane = 0; lane < kBlock; ++lane) pg_solve_col_lane(a, p, j, lane);
  }
  for (int k = n - 1; k >= 0; --k) {
    for (int lane = 0; lane < kBlock; ++lane) pg_back_diag_lane(a, p, k, lane);
    for (int lane = 0; lane < kBlock; ++lane) pg_back_col_lane(a, p, k, lane);
  }
}
// one pass of the loop as the device runs it: every launch as loops over its (block.x, block.y, thread)
inline void pg_pass_host(const PgArgs& a, const PgDims& d) {
  for (int by = 0; by < a.P; ++by)
    for (int bx = 0; bx < d.fac_blocks; ++bx)
      for (int t = 0; t < kBlock; ++t) pg_linearize_thread(a, bx, by, t);
  for (int bx = 0; bx < d.prob_blocks; ++bx)
    for (int t = 0; t < kBlock; ++t) pg_error_thread(a, bx, t);
  for (int by = 0; by < a.P; ++by)
    for (int bx = 0; bx < d.rows; ++bx)
      for (int t = 0; t < kBlock; ++t) pg_assemble_thread(a, bx, by, t);
  for (int p = 0; p < a.P; ++p) pg_solve_host(a, p);
  for (int by = 0; by < a.P; ++by)
    for (int bx = 0; bx < d.pose_blocks; ++bx)
      for (int t = 0; t < kBlock; ++t) pg_update_thread(a, bx, by, t);
}

// ---- the graph's tables, built on the host ------------------------------------------------------------
// c0[r], the first block column of block row r: its left neighbour, or the smallest partner of a loop
// that ends on the row.
inline void pg_first_columns(int K, int L, const int32_t* loops, int32_t* c0) {
  for (int r = 0; r < K; ++r) c0[r] = r > 0 ? r - 1 : 0;
  for (int l = 0; l < L; ++l) {
    const int hi = loops[2 * l] > loops[2 * l + 1] ? loops[2 * l] : loops[2 * l + 1];
    const int lo = loops[2 * l] + loops[2 * l + 1] - hi;
    if (lo < c0[hi]) c0[hi] = lo;
  }
}
// c0 / rowoff / longrow of a problem from its K and loops; returns the envelope's blocks. rowoff and
// longrow may be NULL (append / add_loop only ask for the count).
inline int64_t pg_envelope(int K, int L, const int32_t* loops, int32_t* c0, int64_t* rowoff, int32_t* longrow,
                           int32_t* nlong) {
  pg_first_columns(K, L, loops, c0);
  int64_t at = 0;
  int nl = 0;
  for (int r = 0; r < K; ++r) {
    if (rowoff) rowoff[r] = at;
    at += r - c0[r] + 1;
    if (longrow && r > 0 && c0[r] < r - 1) longrow[nl++] = r;
  }
  if (nlong) *nlong = nl;
  return at;
}

}  // namespace llsr_pgo

// Library-internal (not part of the C-ABI; the mapping chain's use of its slots' graphs): the same
// graphs in a new object of larger capacities (NULL without memory; g stays valid), and dropping the
// newest poses of graph p down to `keep` (no loop factor may touch a dropped pose), and the capacities.
struct llsr_pg;
llsr_pg* llsr_pg_grown(const llsr_pg* g, int32_t max_poses, int32_t max_loops, int64_t max_envelope_blocks);
int32_t llsr_pg_truncate(llsr_pg* g, int32_t p, int32_t keep);
void llsr_pg_capacity(const llsr_pg* g, int32_t* max_poses, int32_t* max_loops, int64_t* max_envelope_blocks);
