// llsr_math_debug.hip — diagnostics (not part of the ABI header) that run the shared numeric headers
// call by call on inputs given by the caller: the float libm ports (llsr_libm.h), the Eigen 3.3.7
// restatement (llsr_eigen.h), the double trigonometry and SO(3) charts of llsr_pg.h, and the RANSAC
// iteration bound (llsr_device.h ransac_k), for tests/test_math_cases_host.py and
// tests/test_gpu_math_headers.py. Every entry takes `where`: 0 runs the header's text as this
// translation unit's host compile has it, without touching a device; 1 runs it in a kernel, one
// thread per case. The kernel only maps a thread to a case; the arithmetic is the header's. This file
// is built by the same rule and flags as the production objects, so it sees what they see.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/llsr.h"
#include "llsr_device.h"
#include "llsr_eigen.h"
#include "llsr_host.h"
#include "llsr_libm.h"
#include "llsr_pg.h"

namespace llsr {
namespace {

constexpr int kDbgMaxCases = 1 << 22;  // per call
constexpr int kDbgBlock = 256;
constexpr int kDbgMaxBlocks = 4096;  // 2^20 threads at most; the grid-stride loop takes the rest

// ---- one case of each family ---------------------------------------------------------------------
// A case type names its element types (In, Out), the elements one case reads from `a` and `b` and
// writes to `out` (kA, kB, kOut), whether it writes info[k], and maps case k in operator().

constexpr int kLibmFns = 9;
template <int FN>
struct LibmCase {
  using In = float;
  using Out = uint32_t;
  static constexpr int kA = 1, kB = FN == 3 ? 1 : 0, kOut = 1;
  static constexpr bool kInfo = false;
  const float* a;  // x
  const float* b;  // y, atan2f_ only
  uint32_t* out;
  int32_t* info;
  LLSR_HD void operator()(int k) const {
    using namespace llsr_libm;
    const float x = a[k];
    float r;
    if constexpr (FN == 0) r = asinf_(x);
    else if constexpr (FN == 1) r = acosf_(x);
    else if constexpr (FN == 2) r = atanf_(x);
    else if constexpr (FN == 3) r = atan2f_(b[k], x);
    else if constexpr (FN == 4) r = tanf_(x);
    else if constexpr (FN == 5) r = sinf_(x);
    else if constexpr (FN == 6) r = cosf_(x);
    else if constexpr (FN == 7) r = sqrt_(x);
    else r = ground_angle_deg(x);
    out[k] = fbits(r);
  }
};

constexpr int kEigenOps = 11;
constexpr int kEigIn[kEigenOps] = {12, 42, 20, 9, 36, 9, 36, 13, 43, 2, 2};
constexpr int kEigOut[kEigenOps] = {3, 6, 3, 12, 42, 9, 36, 45, 162, 1, 2};

// The degeneracy chain of FA:1956-1989 / MO:1505-1536 in the order tests/native/eigen_cross.cpp runs
// it: solve, eig, the rows of V2 below `thr` zeroed from the last one down until one is not, inverse,
// matP = inverse * V2, matX = matP * x. in = A[N*N], b[N], thr; out = x[N], evals[N], V[N*N],
// V2[N*N], inverse[N*N], P[N*N], X[N]; returns eig's code.
template <int N>
LLSR_HD int proj_chain(const float* in, float* out) {
  using namespace llsr_eigen;
  const float* A = in;
  const float* b = in + N * N;
  const float thr = in[N * N + N];
  float *x = out, *E = x + N, *V = E + N, *V2 = V + N * N, *I = V2 + N * N, *P = I + N * N, *X = P + N * N;
  colpiv_qr_solve<N, N>(A, b, x);
  int info;
  if constexpr (N == 3) info = eig3(A, E, V);
  else info = eig_sym<N>(A, E, V);
  bool zeroing = true;
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    zeroing = zeroing && E[i] < thr;
#pragma unroll
    for (int j = 0; j < N; ++j) V2[i + N * j] = zeroing ? 0.0f : V[i + N * j];
  }
  if constexpr (N == 3) {
    inverse3(V, I);
    prod33(I, V2, P);
    prod31(P, x, X);
  } else {
    inverse_lu<N>(V, I);
    prod66(I, V2, P);
    prod61(P, x, X);
  }
  return info;
}

template <int OP>
struct EigenCase {
  using In = float;
  using Out = float;
  static constexpr int kA = kEigIn[OP], kB = 0, kOut = kEigOut[OP];
  static constexpr bool kInfo = true;
  const float* a;
  const float* b;  // unused
  float* out;
  int32_t* info;
  LLSR_HD void operator()(int k) const {
    using namespace llsr_eigen;
    float i[kA], o[kOut];
#pragma unroll
    for (int q = 0; q < kA; ++q) i[q] = a[(size_t)k * kA + q];
    int rc = 0;
    if constexpr (OP == 0) colpiv_qr_solve<3, 3>(i, i + 9, o);
    else if constexpr (OP == 1) colpiv_qr_solve<6, 6>(i, i + 36, o);
    else if constexpr (OP == 2) colpiv_qr_solve<5, 3>(i, i + 15, o);
    else if constexpr (OP == 3) rc = eig3(i, o, o + 3);
    else if constexpr (OP == 4) rc = eig_sym<6>(i, o, o + 6);
    else if constexpr (OP == 5) inverse3(i, o);
    else if constexpr (OP == 6) inverse_lu<6>(i, o);
    else if constexpr (OP == 7) rc = proj_chain<3>(i, o);
    else if constexpr (OP == 8) rc = proj_chain<6>(i, o);
    else if constexpr (OP == 9) o[0] = hypot_(i[0], i[1]);
    else make_givens(i[0], i[1], o[0], o[1]);
#pragma unroll
    for (int q = 0; q < kOut; ++q) out[(size_t)k * kOut + q] = o[q];
    info[k] = rc;
  }
};

constexpr int kPgFns = 10;
constexpr int kPgIn[kPgFns] = {1, 1, 1, 2, 1, 3, 9, 3, 3, 9};
constexpr int kPgOut[kPgFns] = {1, 1, 1, 1, 1, 9, 3, 3, 9, 3};

template <int FN>
struct PgCase {
  using In = double;
  using Out = uint64_t;
  static constexpr int kA = kPgIn[FN], kB = 0, kOut = kPgOut[FN];
  static constexpr bool kInfo = false;
  const double* a;
  const double* b;  // unused
  uint64_t* out;
  int32_t* info;
  LLSR_HD void operator()(int k) const {
    using namespace llsr_pgo;
    double i[kA], o[kOut];
#pragma unroll
    for (int q = 0; q < kA; ++q) i[q] = a[(size_t)k * kA + q];
    if constexpr (FN == 0) o[0] = sind(i[0]);
    else if constexpr (FN == 1) o[0] = cosd(i[0]);
    else if constexpr (FN == 2) o[0] = atand(i[0]);
    else if constexpr (FN == 3) o[0] = atan2d(i[0], i[1]);
    else if constexpr (FN == 4) o[0] = acosd(i[0]);
    else if constexpr (FN == 5) so3_exp(i, o);
    else if constexpr (FN == 6) so3_log(i, o);
    else if constexpr (FN == 7) {
      double R[9];
      so3_exp(i, R);
      so3_log(R, o);
    } else if constexpr (FN == 8) rot_rzryrx(i[0], i[1], i[2], o);
    else rot_angles(i, &o[0], &o[1], &o[2]);
#pragma unroll
    for (int q = 0; q < kOut; ++q) out[(size_t)k * kOut + q] = dbits(o[q]);
  }
};

// the bound k_ground_elev_ransac computes after a best model of b[k] inliers among a[k] points, with
// the kernel's own hoisted terms
struct RansacCase {
  using In = int32_t;
  using Out = uint64_t;
  static constexpr int kA = 1, kB = 1, kOut = 1;
  static constexpr bool kInfo = false;
  const int32_t* a;  // K
  const int32_t* b;  // cnt
  uint64_t* out;
  int32_t* info;
  LLSR_HD void operator()(int k) const {
    const int K = a[k];
    const double log_probability = log(1.0 - 0.99);
    const double one_over = K > 0 ? 1.0 / (double)K : 0.0;
    out[k] = llsr_pgo::dbits(ransac_k(b[k], one_over, log_probability));
  }
};

template <class Case>
__global__ __launch_bounds__(kDbgBlock) void k_debug_math(Case c, int n) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) c(k);
}

template <class T>
bool dev_in(llsr_host::DevMem& m, const T* host, size_t n, int32_t& rc) {
  if (n == 0) return true;
  if (llsr_host::alloc(m, sizeof(T) * n) != hipSuccess) { rc = LLSR_ENODEV; return false; }
  if (host && hipMemcpy(m, host, sizeof(T) * n, hipMemcpyHostToDevice) != hipSuccess) { rc = LLSR_EIO; return false; }
  return true;
}

// n cases of one type on the host (where 0) or in one launch (where 1)
template <class Case>
int32_t run_cases(int32_t where, int32_t n, const typename Case::In* a, const typename Case::In* b,
                  typename Case::Out* out, int32_t* info) {
  using In = typename Case::In;
  using Out = typename Case::Out;
  if (n == 0) return LLSR_OK;
  if (where == 0) {
    const Case c{a, b, out, info};
    for (int k = 0; k < n; ++k) c(k);
    return LLSR_OK;
  }
  const size_t N = (size_t)n;
  llsr_host::DevMem da, db, dout, dinfo;
  int32_t rc = LLSR_OK;
  if (!dev_in<In>(da, a, N * Case::kA, rc) || !dev_in<In>(db, b, N * Case::kB, rc) ||
      !dev_in<Out>(dout, nullptr, N * Case::kOut, rc) || !dev_in<int32_t>(dinfo, nullptr, Case::kInfo ? N : 0, rc))
    return rc;
  const Case c{static_cast<const In*>(da.get()), static_cast<const In*>(db.get()), static_cast<Out*>(dout.get()),
               static_cast<int32_t*>(dinfo.get())};
  const int blocks = (n + kDbgBlock - 1) / kDbgBlock;
  k_debug_math<Case><<<blocks < kDbgMaxBlocks ? blocks : kDbgMaxBlocks, kDbgBlock>>>(c, n);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(out, dout, sizeof(Out) * N * Case::kOut, hipMemcpyDeviceToHost) != hipSuccess ||
      (Case::kInfo && hipMemcpy(info, dinfo, sizeof(int32_t) * N, hipMemcpyDeviceToHost) != hipSuccess))
    return LLSR_EIO;
  return LLSR_OK;
}

bool args_ok(int32_t where, int32_t n) { return (where == 0 || where == 1) && n >= 0 && n <= kDbgMaxCases; }

}  // namespace
}  // namespace llsr

using namespace llsr;

#define LLSR_DBG_CASE(T, k, ...) \
  case k: return run_cases<T<k>>(where, n, __VA_ARGS__)

// llsr_libm.h on n floats x (and y for atan2f_(y, x), read by no other fn): the result's bits.
// fn: 0 asinf_, 1 acosf_, 2 atanf_, 3 atan2f_, 4 tanf_, 5 sinf_, 6 cosf_, 7 sqrt_, 8 ground_angle_deg.
extern "C" int32_t llsr_debug_libm(int32_t fn, int32_t where, int32_t n, const float* x, const float* y,
                                   uint32_t* out_bits) {
  if (!args_ok(where, n) || fn < 0 || fn >= kLibmFns || !x || !out_bits || (fn == 3 && !y)) return LLSR_EINVAL;
  switch (fn) {
    LLSR_DBG_CASE(LibmCase, 0, x, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(LibmCase, 1, x, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(LibmCase, 2, x, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(LibmCase, 3, x, y, out_bits, nullptr);
    LLSR_DBG_CASE(LibmCase, 4, x, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(LibmCase, 5, x, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(LibmCase, 6, x, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(LibmCase, 7, x, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(LibmCase, 8, x, nullptr, out_bits, nullptr);
  }
  return LLSR_EINVAL;
}

// llsr_eigen.h on n packed cases of column-major floats; info[k] is the return code of the ops that
// have one (eig3, eig6, proj3, proj6), else 0. Floats read / written per case:
//   0 qr33  A[9] b[3] -> x[3]       1 qr66  A[36] b[6] -> x[6]     2 qr53  A[15] b[5] -> x[3]
//   3 eig3  A[9] -> evals[3] V[9]   4 eig6  A[36] -> evals[6] V[36]
//   5 inv3  A[9] -> inverse[9]      6 inv6  A[36] -> inverse[36]
//   7 proj3 A[9] b[3] thr -> 45     8 proj6 A[36] b[6] thr -> 162  (proj_chain above)
//   9 hypot x y -> hypot_           10 givens p q -> c s
extern "C" int32_t llsr_debug_eigen(int32_t op, int32_t where, int32_t n, const float* in, float* out, int32_t* info) {
  if (!args_ok(where, n) || op < 0 || op >= kEigenOps || !in || !out || !info) return LLSR_EINVAL;
  switch (op) {
    LLSR_DBG_CASE(EigenCase, 0, in, nullptr, out, info);
    LLSR_DBG_CASE(EigenCase, 1, in, nullptr, out, info);
    LLSR_DBG_CASE(EigenCase, 2, in, nullptr, out, info);
    LLSR_DBG_CASE(EigenCase, 3, in, nullptr, out, info);
    LLSR_DBG_CASE(EigenCase, 4, in, nullptr, out, info);
    LLSR_DBG_CASE(EigenCase, 5, in, nullptr, out, info);
    LLSR_DBG_CASE(EigenCase, 6, in, nullptr, out, info);
    LLSR_DBG_CASE(EigenCase, 7, in, nullptr, out, info);
    LLSR_DBG_CASE(EigenCase, 8, in, nullptr, out, info);
    LLSR_DBG_CASE(EigenCase, 9, in, nullptr, out, info);
    LLSR_DBG_CASE(EigenCase, 10, in, nullptr, out, info);
  }
  return LLSR_EINVAL;
}

// llsr_pg.h's double functions on n packed cases: the results' bits. Doubles read -> written per case:
//   0 sind, 1 cosd, 2 atand, 4 acosd: 1 -> 1      3 atan2d: (y, x) -> 1
//   5 so3_exp: w[3] -> R[9] row-major             6 so3_log: R[9] -> w[3]
//   7 exp_then_log: w[3] -> so3_log(so3_exp(w))   8 rot_rzryrx: (a, b, c) -> R[9]
//   9 rot_angles: R[9] -> (a, b, c)
extern "C" int32_t llsr_debug_pg_math(int32_t fn, int32_t where, int32_t n, const double* in, uint64_t* out_bits) {
  if (!args_ok(where, n) || fn < 0 || fn >= kPgFns || !in || !out_bits) return LLSR_EINVAL;
  switch (fn) {
    LLSR_DBG_CASE(PgCase, 0, in, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(PgCase, 1, in, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(PgCase, 2, in, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(PgCase, 3, in, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(PgCase, 4, in, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(PgCase, 5, in, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(PgCase, 6, in, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(PgCase, 7, in, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(PgCase, 8, in, nullptr, out_bits, nullptr);
    LLSR_DBG_CASE(PgCase, 9, in, nullptr, out_bits, nullptr);
  }
  return LLSR_EINVAL;
}
#undef LLSR_DBG_CASE

// ransac_k (llsr_device.h) as k_ground_elev_ransac calls it, for n pairs of K >= 1 points and a best
// model of 0 <= cnt <= K inliers: the double's bits. where 0 evaluates the same expression with the
// host's log and pow.
extern "C" int32_t llsr_debug_ransac_k(int32_t where, int32_t n, const int32_t* K, const int32_t* cnt,
                                       uint64_t* out_bits) {
  if (!args_ok(where, n) || !K || !cnt || !out_bits) return LLSR_EINVAL;
  for (int32_t k = 0; k < n; ++k)
    if (K[k] < 1 || cnt[k] < 0 || cnt[k] > K[k]) return LLSR_EINVAL;
  return run_cases<RansacCase>(where, n, K, cnt, out_bits, nullptr);
}
