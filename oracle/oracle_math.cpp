// oracle_math.cpp — TEST INFRASTRUCTURE ONLY (see oracle.h).
//
// Batch references for the numeric headers of the product (tests/test_math_cases_host.py,
// tests/test_gpu_math_headers.py): plain loops over glibc's float and double elementary functions
// and over the oracle's own Eigen 3.3.7 restatement (oracle_eigen.h), so 10^5 cases cost one call.
// Nothing here includes a product header. The selectors and the packing of `in` / `out` are those of
// llsr_debug_libm / llsr_debug_pg_math / llsr_debug_eigen (tests/_math_cases.py names them).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "oracle.h"
#include "oracle_eigen.h"

// fn: 0 asinf, 1 acosf, 2 atanf, 3 atan2f(y, x), 4 tanf, 5 sinf, 6 cosf,
// 7 sqrtf, 8 the ground angle in degrees as IP:559 writes it. y is read by atan2f only.
extern "C" int32_t oracle_libm_f32(int32_t fn, int64_t n, const float* x, const float* y, float* out) {
  if (fn < 0 || fn > 8) return -22;
  const double deg = M_PI / 180.0;  // utility.h:49
  for (int64_t k = 0; k < n; ++k) {
    const float a = x[k];
    float r;
    switch (fn) {
      case 0: r = asinf(a); break;
      case 1: r = acosf(a); break;
      case 2: r = atanf(a); break;
      case 3: r = atan2f(y[k], a); break;
      case 4: r = tanf(a); break;
      case 5: r = sinf(a); break;
      case 6: r = cosf(a); break;
      case 7: r = sqrtf(a); break;
      default: r = (float)((double)acosf(a) / deg); break;
    }
    out[k] = r;
  }
  return 0;
}

// fn: 0 sin, 1 cos, 2 atan, 3 atan2(y, x), 4 acos
extern "C" int32_t oracle_libm_f64(int32_t fn, int64_t n, const double* x, const double* y, double* out) {
  if (fn < 0 || fn > 4) return -22;
  for (int64_t k = 0; k < n; ++k) {
    const double a = x[k];
    double r;
    switch (fn) {
      case 0: r = sin(a); break;
      case 1: r = cos(a); break;
      case 2: r = atan(a); break;
      case 3: r = atan2(y[k], a); break;
      default: r = acos(a); break;
    }
    out[k] = r;
  }
  return 0;
}

namespace {

// the floats one case reads and writes, per op
const int kEigIn[11] = {12, 42, 20, 9, 36, 9, 36, 13, 43, 2, 2};
const int kEigOut[11] = {3, 6, 3, 12, 42, 9, 36, 45, 162, 1, 2};

// The degeneracy chain of FA:1956-1989 / MO:1505-1536 as tests/native/eigen_cross.cpp runs it:
// solve, eig, the rows of V2 below `thr` zeroed from the last one down, inverse, matP, matX.
// out = x[N], evals[N], V[N*N], V2[N*N], inverse[N*N], P[N*N], X[N]; returns eig's code.
template <int N>
int proj(const float* in, float* out) {
  const float *A = in, *b = in + N * N, thr = in[N * N + N];
  float *x = out, *E = x + N, *V = E + N, *V2 = V + N * N, *I = V2 + N * N, *P = I + N * N, *X = P + N * N;
  oeig::colpiv_qr_solve(A, N, N, b, x);
  const int info = N == 3 ? oeig::eig_sym3(A, E, V) : oeig::eig_sym_n(A, N, E, V);
  std::memcpy(V2, V, sizeof(float) * N * N);
  for (int i = N - 1; i >= 0; --i) {
    if (E[i] < thr) { for (int j = 0; j < N; ++j) V2[i + N * j] = 0.0f; }
    else break;
  }
  if (N == 3) {
    oeig::inverse3(V, I);
    oeig::prod33(I, V2, P);
    oeig::prod31(P, x, X);
  } else {
    oeig::inverse_lu(V, N, I);
    oeig::prod66(I, V2, P);
    oeig::prod61(P, x, X);
  }
  return info;
}

}  // namespace

// op: 0 qr33, 1 qr66, 2 qr53 (A, b -> x); 3 eig3, 4 eig6 (A -> values, vectors; info = the code);
// 5 inv3, 6 inv6; 7 proj3, 8 proj6 (A, b, thr -> the chain above); 9 hypot (x, y); 10 givens
// (p, q -> c, s). Matrices column-major; case k reads in[k * kEigIn[op]..] and writes
// out[k * kEigOut[op]..]; info[k] is 0 for the ops without a return code.
extern "C" int32_t oracle_eigen_batch(int32_t op, int64_t n, const float* in, float* out, int32_t* info) {
  if (op < 0 || op > 10) return -22;
  for (int64_t k = 0; k < n; ++k) {
    const float* a = in + k * kEigIn[op];
    float* o = out + k * kEigOut[op];
    int rc = 0;
    switch (op) {
      case 0: oeig::colpiv_qr_solve(a, 3, 3, a + 9, o); break;
      case 1: oeig::colpiv_qr_solve(a, 6, 6, a + 36, o); break;
      case 2: oeig::colpiv_qr_solve(a, 5, 3, a + 15, o); break;
      case 3: rc = oeig::eig_sym3(a, o, o + 3); break;
      case 4: rc = oeig::eig_sym_n(a, 6, o, o + 6); break;
      case 5: oeig::inverse3(a, o); break;
      case 6: oeig::inverse_lu(a, 6, o); break;
      case 7: rc = proj<3>(a, o); break;
      case 8: rc = proj<6>(a, o); break;
      case 9: o[0] = oeig::hypot_impl(a[0], a[1]); break;
      default: { const oeig::Givens g = oeig::make_givens(a[0], a[1]); o[0] = g.c; o[1] = g.s; }
    }
    info[k] = rc;
  }
  return 0;
}
