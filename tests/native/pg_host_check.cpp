// pg_host_check.cpp — CPU check of the pose-graph optimiser's shared host / device bodies
// (csrc/llsr_pg.h), run by tests/test_pg_native.py under AddressSanitizer / UBSan:
//   * the double sin / cos / atan2 / acos against the C library on 10^6 arguments in [-2 pi, 2 pi]
//     (acos also on the same arguments scaled into [-1, 1]); the bounds asserted are the ones measured
//     with this program (DESIGN.md §19 quotes them);
//   * every analytic Jacobian against central differences of the error under the retract, 1000 random
//     poses with error rotations near 0, of ordinary size and near pi - 0.1, step 1e-6; every entry
//     within 1e-6 of max(1, |entry|): relative for the entries above 1 (the [h_t]x block reaches 60),
//     absolute 1e-6 for the others, the rotation blocks and the zeros among them;
//   * the envelope Cholesky and both substitutions against a dense Cholesky written here, on graphs with
//     nested, crossing and same-row loops: the same sums in the same order, so bit for bit;
//   * every launch's (block, thread) mapping — pg_pass_host, the loops the device's launches are — over
//     heap buffers of exactly pg_sizes' elements, on a batch of K = 1, 2, 12 and 70 next to each problem
//     alone.
// `pg_host_check measure` prints the measured trig errors instead of asserting them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "llsr_pg.h"

using namespace llsr_pgo;

static int g_bad = 0;
#define REQUIRE(c)                                               \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_bad;                                                   \
    }                                                            \
  } while (0)

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static double uni() {  // [0, 1)
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_rng >> 11) / 9007199254740992.0;
}
static double ud(double lo, double hi) { return lo + (hi - lo) * uni(); }

template <class T>
struct Heap {  // exactly n elements on the heap: one past the end is a sanitizer report
  T* p;
  size_t n;
  explicit Heap(size_t n_) : p(static_cast<T*>(std::malloc((n_ ? n_ : 1) * sizeof(T)))), n(n_) {
    std::memset(p, 0, (n_ ? n_ : 1) * sizeof(T));
  }
  ~Heap() { std::free(p); }
  Heap(const Heap&) = delete;
  Heap& operator=(const Heap&) = delete;
};

// ---- trig ----------------------------------------------------------------------------------------------
static double ulps(double got, double want) {
  if (got != got && want != want) return 0.0;
  if (got != got || want != want) return 1e300;
  if (got == want) return 0.0;
  int e;
  std::frexp(want, &e);
  return std::fabs(got - want) / std::ldexp(1.0, e - 53);
}
// Measured with this program (`measure`) against glibc on x86-64; both are faithful to well under
// 1 ulp of the true value, so they differ by at most one unit in the last place.
static const double kSinUlp = 1.0, kCosUlp = 1.0, kAtan2Ulp = 1.0, kAcosUlp = 1.0;

static void check_trig(bool measure) {
  const double two_pi = 6.283185307179586;
  double ms = 0, mc = 0, mt = 0, ma = 0;
  for (int k = 0; k < 1000000; ++k) {
    const double x = ud(-two_pi, two_pi), y = ud(-two_pi, two_pi);
    const double es = ulps(sind(x), std::sin(x)), ec = ulps(cosd(x), std::cos(x));
    const double et = ulps(atan2d(y, x), std::atan2(y, x));
    const double ea = std::fmax(ulps(acosd(x), std::acos(x)), ulps(acosd(x / two_pi), std::acos(x / two_pi)));
    ms = std::fmax(ms, es); mc = std::fmax(mc, ec); mt = std::fmax(mt, et); ma = std::fmax(ma, ea);
  }
  if (measure) std::printf("max ulp: sin %.3f cos %.3f atan2 %.3f acos %.3f\n", ms, mc, mt, ma);
  REQUIRE(ms <= kSinUlp);
  REQUIRE(mc <= kCosUlp);
  REQUIRE(mt <= kAtan2Ulp);
  REQUIRE(ma <= kAcosUlp);
  // the special values the conversions meet
  REQUIRE(sind(0.0) == 0.0 && cosd(0.0) == 1.0 && atan2d(0.0, 1.0) == 0.0 && acosd(1.0) == 0.0);
  REQUIRE(atan2d(0.0, -1.0) == std::atan2(0.0, -1.0) && atan2d(1.0, 0.0) == std::atan2(1.0, 0.0));
  REQUIRE(sind(1e9) != sind(1e9));  // outside the reduction's range: no number, never a wrong one
}

// ---- a workspace on the heap ---------------------------------------------------------------------------
struct Graph {
  std::vector<float> poses;  // store layout, 6 per pose
  std::vector<int> loops;    // from, to
  std::vector<double> loopZ; // 12 per loop
  std::vector<double> loopW; // 1 / sigma
};
struct Ws {
  int P, maxK, maxL;
  int64_t maxE;
  PgSizes z;
  Heap<PgProblem> prob;
  Heap<PgState> st;
  Heap<int32_t> live, loops, c0, longrow;
  Heap<int64_t> rowoff;
  Heap<double> X, Xprev, Z, winv, res, J, eterm, H, d;
  Heap<float> out6;
  PgArgs a;
  Ws(int P_, int maxK_, int maxL_, int64_t maxE_)
      : P(P_), maxK(maxK_), maxL(maxL_), maxE(maxE_), z(pg_sizes(P_, maxK_, maxL_, maxE_)), prob(z.prob), st(z.st),
        live(1), loops(z.loops), c0(z.c0), longrow(z.longrow), rowoff(z.rowoff), X(z.X), Xprev(z.X), Z(z.Z),
        winv(z.winv), res(z.res), J(z.J), eterm(z.eterm), H(z.H), d(z.d), out6(z.out6) {
    a = PgArgs{};
    a.P = P; a.maxK = maxK; a.maxL = maxL; a.maxE = maxE;
    a.max_iterations = 100; a.rel_tol = 1e-5; a.abs_tol = 1e-5;
    a.prob = prob.p; a.st = st.p; a.live = live.p; a.X = X.p; a.Xprev = Xprev.p; a.Z = Z.p; a.winv = winv.p;
    a.loops = loops.p; a.c0 = c0.p; a.rowoff = rowoff.p; a.longrow = longrow.p; a.res = res.p; a.J = J.p;
    a.eterm = eterm.p; a.H = H.p; a.d = d.p; a.out6 = out6.p;
  }
  // graph g into slot p as llsr_pg_append / llsr_pg_add_loop / llsr_pg_optimize's staging do
  void load(int p, const Graph& g) {
    const int K = (int)g.poses.size() / 6, L = (int)g.loops.size() / 2;
    REQUIRE(K <= maxK && L <= maxL);
    const size_t R0 = (size_t)p * maxK, F0 = (size_t)p * ((size_t)maxK + maxL), L0 = (size_t)p * maxL;
    const double var[6] = {1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6};
    for (int k = 0; k < K; ++k) {
      double* T = X.p + 12 * (R0 + k);
      pose_from_store6(&g.poses[6 * (size_t)k], T);
      if (k == 0) std::memcpy(Z.p + 12 * F0, T, 12 * sizeof(double));
      else pose_between(T - 12, T, Z.p + 12 * (F0 + k));
      for (int c = 0; c < 6; ++c) winv.p[6 * (F0 + k) + c] = 1.0 / std::sqrt(var[c]);
    }
    for (int l = 0; l < L; ++l) {
      loops.p[2 * (L0 + l)] = g.loops[2 * l];
      loops.p[2 * (L0 + l) + 1] = g.loops[2 * l + 1];
      std::memcpy(Z.p + 12 * (F0 + K + l), &g.loopZ[12 * (size_t)l], 12 * sizeof(double));
      for (int c = 0; c < 6; ++c) winv.p[6 * (F0 + K + l) + c] = g.loopW[l];
    }
    PgProblem& pr = prob.p[p];
    pr.K = K; pr.L = L; pr.run = L > 0;
    const int64_t blocks = pg_envelope(K, L, loops.p + 2 * L0, c0.p + R0, rowoff.p + R0, longrow.p + L0, &pr.nlong);
    REQUIRE(blocks <= maxE);
    st.p[p] = PgState{};
    st.p[p].state = pr.run ? kRun : kStateClean;
  }
  int run() {  // llsr_pg_optimize's loop
    int n = 0;
    for (int p = 0; p < P; ++p) n += prob.p[p].run;
    *live.p = n;
    const PgDims dm = pg_dims(prob.p, P);
    int passes = 0;
    for (a.pass = 0; *live.p > 0 && a.pass <= a.max_iterations; ++a.pass, ++passes) pg_pass_host(a, dm);
    return passes;
  }
};

// poses around a 4 x 4 m square with yaw turning and small roll / pitch, drifting
static Graph square(int K, double drift) {
  Graph g;
  for (int k = 0; k < K; ++k) {
    const double s = 16.0 * k / K, side = std::floor(s / 4.0), u = s - 4.0 * side;
    const double x = side == 0 ? u : side == 1 ? 4 : side == 2 ? 4 - u : 0;
    const double y = side == 0 ? 0 : side == 1 ? u : side == 2 ? 4 : 4 - u;
    // store layout: x, y, z, roll, pitch, yaw; the ground plane of the store is (z, x), pitch turns in it
    const float p[6] = {(float)(y + drift * k), (float)(0.02 * std::sin(0.7 * k)), (float)(x + 0.5 * drift * k),
                        (float)(0.035 * std::sin(1.3 * k)), (float)(6.283185307179586 * k / K + 0.2 * drift * k),
                        (float)(0.035 * std::cos(0.9 * k))};
    g.poses.insert(g.poses.end(), p, p + 6);
  }
  return g;
}
// a loop factor from -> to holding the relative pose of the drift-free square, moved a little
static void add_loop(Graph& g, const Graph& truth, int from, int to, double variance) {
  double Tf[12], Tt[12], Z[12];
  pose_from_store6(&truth.poses[6 * (size_t)from], Tf);
  pose_from_store6(&truth.poses[6 * (size_t)to], Tt);
  pose_between(Tf, Tt, Z);
  g.loops.push_back(from);
  g.loops.push_back(to);
  g.loopZ.insert(g.loopZ.end(), Z, Z + 12);
  g.loopW.push_back(1.0 / std::sqrt(variance));
}
static Graph drifting(int K, const std::vector<int>& loops, double variance = 0.3) {
  Graph g = square(K, 0.01), truth = square(K, 0.0);
  for (size_t l = 0; l + 1 < loops.size(); l += 2) add_loop(g, truth, loops[l], loops[l + 1], variance * (1.0 + 0.3 * (double)l));
  return g;
}

// ---- Jacobians -------------------------------------------------------------------------------------------
static void random_rot(double scale, double* w) {
  double n;
  do {
    for (int k = 0; k < 3; ++k) w[k] = ud(-1, 1);
    n = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  } while (n < 1e-3 || n > 1.0);
  for (int k = 0; k < 3; ++k) w[k] *= scale / n;
}
static void random_pose(double* T) {
  double w[3];
  random_rot(ud(0.0, 3.0), w);
  so3_exp(w, T);
  for (int k = 0; k < 3; ++k) T[9 + k] = ud(-20, 20);
}
static void check_jacobians() {
  Ws ws(1, 2, 1, 4);
  PgArgs& a = ws.a;
  ws.prob.p[0].K = 2; ws.prob.p[0].L = 1; ws.prob.p[0].run = 1;
  ws.loops.p[0] = 1; ws.loops.p[1] = 0;  // the loop factor's first pose is the later one, as MO:1086 has it
  for (size_t k = 0; k < ws.winv.n; ++k) ws.winv.p[k] = 1.0;
  const double h = 1e-6;
  double worst = 0;
  for (int trial = 0; trial < 1000; ++trial) {
    random_pose(a.X);
    random_pose(a.X + 12);
    // the size of the error rotation: near 0, ordinary, near pi - 0.1
    const double size = trial % 3 == 0 ? std::pow(10.0, ud(-9, -2)) : trial % 3 == 1 ? ud(0.01, 2.5) : 3.141592653589793 - 0.1 - ud(0, 0.01);
    for (int f = 0; f < 3; ++f) {
      int i, j;
      pg_factor_poses(a, 0, f, &i, &j);
      // Z = h moved by the error: Zr = hr Exp(-w), Zt = ht + small
      double Hm[12], w[3], E[9];
      if (i < 0) std::memcpy(Hm, a.X + 12 * j, sizeof Hm);
      else pose_between(a.X + 12 * i, a.X + 12 * j, Hm);
      random_rot(size, w);
      for (int k = 0; k < 3; ++k) w[k] = -w[k];
      so3_exp(w, E);
      double* Z = ws.Z.p + 12 * f;
      mat_mul(Hm, E, Z);
      for (int k = 0; k < 3; ++k) Z[9 + k] = Hm[9 + k] + ud(-0.5, 0.5);
      pg_linearize(a, 0, f);
      double Ja[72], X0[24];
      std::memcpy(Ja, a.J + 72 * f, sizeof Ja);
      std::memcpy(X0, a.X, sizeof X0);
      for (int side = 0; side < 2; ++side) {
        const int pose = side == 0 ? i : j;
        if (pose < 0) continue;
        for (int c = 0; c < 6; ++c) {
          double dl[6] = {0, 0, 0, 0, 0, 0}, ep[6], em[6];
          dl[c] = h;
          pose_retract(X0 + 12 * pose, dl, a.X + 12 * pose);
          pg_linearize(a, 0, f);
          std::memcpy(ep, a.res + 6 * f, sizeof ep);
          dl[c] = -h;
          pose_retract(X0 + 12 * pose, dl, a.X + 12 * pose);
          pg_linearize(a, 0, f);
          std::memcpy(em, a.res + 6 * f, sizeof em);
          std::memcpy(a.X, X0, sizeof X0);
          for (int r = 0; r < 6; ++r) {
            const double an = Ja[36 * side + 6 * r + c], num = (ep[r] - em[r]) / (2 * h);
            const double err = std::fabs(num - an) / std::fmax(1.0, std::fabs(an));
            worst = std::fmax(worst, err);
          }
        }
      }
    }
  }
  std::fprintf(stderr, "Jacobians: worst difference / max(1, |entry|) %.3g\n", worst);
  REQUIRE(worst <= 1e-6);
  // Log at the angles the chart's branches meet, pi included
  const double angles[] = {0.0, 1e-12, 9.9e-4, 1.1e-3, 1.0, 3.0, 3.141592, 3.141592653589793};
  for (double t : angles) {
    double w[3] = {0.6 * t, -0.48 * t, 0.64 * t}, R[9], back[3];
    so3_exp(w, R);
    so3_log(R, back);
    for (int k = 0; k < 3; ++k) REQUIRE(std::fabs(back[k] - w[k]) <= 1e-9 * (1 + t) || std::fabs(back[k] + w[k]) <= 1e-7);
  }
}

// ---- the envelope Cholesky against a dense one ------------------------------------------------------------
static void check_cholesky(const std::vector<int>& loops) {
  const int K = 12, n = 6 * K;
  Graph g = drifting(K, loops);
  Ws ws(1, K, (int)loops.size() / 2, 400);
  ws.load(0, g);
  PgArgs& a = ws.a;
  *ws.live.p = 1;
  a.pass = 0;
  const PgDims dm = pg_dims(ws.prob.p, 1);
  for (int bx = 0; bx < dm.fac_blocks; ++bx)
    for (int t = 0; t < kBlock; ++t) pg_linearize_thread(a, bx, 0, t);
  for (int t = 0; t < kBlock; ++t) pg_error_thread(a, 0, t);
  for (int bx = 0; bx < dm.rows; ++bx)
    for (int t = 0; t < kBlock; ++t) pg_assemble_thread(a, bx, 0, t);
  // the dense system from the envelope (its lower triangle mirrored), zero outside
  std::vector<double> A((size_t)n * n, 0.0), b(n), inside((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) {
    const PgRow r = pg_row(a, 0, i);
    for (int j = r.first; j <= i; ++j) {
      A[(size_t)i * n + j] = A[(size_t)j * n + i] = r.at[j];
      inside[(size_t)i * n + j] = 1.0;
    }
    // the upper part of the diagonal block holds the mirrored entries
    for (int j = i + 1; j < 6 * (i / 6) + 6; ++j) REQUIRE(r.at[j] == pg_row(a, 0, j).at[i]);
    b[i] = a.d[i];
  }
  pg_solve_host(a, 0);
  REQUIRE(ws.st.p[0].state == kRun);
  // dense LL^T, forward and back substitution with the sums in the envelope code's order
  std::vector<double> Ld((size_t)n * n, 0.0), y(b);
  for (int j = 0; j < n; ++j) {
    double acc = A[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) acc = acc - Ld[(size_t)j * n + k] * Ld[(size_t)j * n + k];
    REQUIRE(acc > 0);
    Ld[(size_t)j * n + j] = std::sqrt(acc);
    for (int i = j + 1; i < n; ++i) {
      double s = A[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s = s - Ld[(size_t)i * n + k] * Ld[(size_t)j * n + k];
      Ld[(size_t)i * n + j] = s / Ld[(size_t)j * n + j];
    }
  }
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < i; ++k) y[i] = y[i] - Ld[(size_t)i * n + k] * y[k];
    y[i] = y[i] / Ld[(size_t)i * n + i];
  }
  for (int k = n - 1; k >= 0; --k) {
    y[k] = y[k] / Ld[(size_t)k * n + k];
    for (int i = 0; i < k; ++i) y[i] = y[i] - Ld[(size_t)k * n + i] * y[k];
  }
  int diff = 0, fill = 0;
  for (int i = 0; i < n; ++i) {
    const PgRow r = pg_row(a, 0, i);
    for (int j = 0; j <= i; ++j) {
      if (inside[(size_t)i * n + j]) diff += r.at[j] != Ld[(size_t)i * n + j];
      else fill += Ld[(size_t)i * n + j] != 0.0;  // the factor's fill stays inside the envelope
    }
    diff += a.d[i] != y[i];
  }
  REQUIRE(diff == 0);
  REQUIRE(fill == 0);
  // and it solves the system: the residual against the size of the right-hand side
  double worst = 0, bmax = 0;
  for (int i = 0; i < n; ++i) {
    double s = 0;
    for (int j = 0; j < n; ++j) s += A[(size_t)i * n + j] * a.d[j];
    worst = std::fmax(worst, std::fabs(s - b[i]));
    bmax = std::fmax(bmax, std::fabs(b[i]));
  }
  REQUIRE(worst <= 1e-6 * bmax);
}

// ---- the launches over exact-size buffers: a batch next to each problem alone ----------------------------
static void check_batch() {
  std::vector<Graph> gs;
  gs.push_back(drifting(1, {}));
  gs.push_back(drifting(2, {1, 0}));
  gs.push_back(drifting(12, {11, 0, 11, 4, 8, 1}));
  gs.push_back(drifting(70, {69, 3}, 0.01));  // a stiffer loop: one more iteration than the others
  const int P = (int)gs.size();
  // capacities exactly the largest problem's: nothing to spare in any buffer
  Ws batch(P, 70, 3, 2 * 70 - 1 + 65);
  for (int p = 0; p < P; ++p) batch.load(p, gs[p]);
  const int passes = batch.run();
  REQUIRE(*batch.live.p == 0);
  int seen[8] = {0};
  for (int p = 0; p < P; ++p) {
    const int K = (int)gs[p].poses.size() / 6, L = (int)gs[p].loops.size() / 2;
    Ws one(1, K, L > 0 ? L : 1, batch.rowoff.p[(size_t)p * 70 + K - 1] + (K - batch.c0.p[(size_t)p * 70 + K - 1]));
    one.load(0, gs[p]);
    one.run();
    const PgState &sb = batch.st.p[p], &so = one.st.p[0];
    REQUIRE(sb.state == so.state && sb.iterations == so.iterations);
    REQUIRE(std::memcmp(&sb.err0, &so.err0, 8) == 0 && std::memcmp(&sb.err, &so.err, 8) == 0);
    REQUIRE(std::memcmp(batch.X.p + 12 * (size_t)p * 70, one.X.p, 12 * (size_t)K * sizeof(double)) == 0);
    if (sb.iterations > 0)
      REQUIRE(std::memcmp(batch.out6.p + 6 * (size_t)p * 70, one.out6.p, 6 * (size_t)K * sizeof(float)) == 0);
    if (L == 0) REQUIRE(sb.state == kStateClean && sb.iterations == 0);
    else {
      REQUIRE(sb.state == kStateAbs || sb.state == kStateRel);
      REQUIRE(sb.err < sb.err0);
      REQUIRE(sb.iterations < 8 && !seen[sb.iterations]);  // every problem stops after its own count
      seen[sb.iterations] = 1;
    }
  }
  REQUIRE(passes >= 2);
  // a loop variance of 1e-300: the whitened system's pivots overflow or cancel; the state is "failed"
  // or the problem converges — either way nothing may be out of bounds or not finite in the poses
  Graph g = drifting(12, {11, 0});
  g.loopW[0] = 1.0 / std::sqrt(1e-300);
  Ws w2(1, 12, 1, 40);
  w2.load(0, g);
  w2.run();
  REQUIRE(w2.st.p[0].state != kRun);
  for (int k = 0; k < 12 * 12; ++k) REQUIRE(finited(w2.X.p[k]));
}

int main(int argc, char** argv) {
  const bool measure = argc > 1 && std::strcmp(argv[1], "measure") == 0;
  check_trig(measure);
  check_jacobians();
  check_cholesky({11, 0, 9, 2});          // nested
  check_cholesky({8, 1, 11, 5});          // crossing
  check_cholesky({11, 0, 11, 4, 3, 11});  // the same row three times, one of them given the other way round
  check_cholesky({1, 0, 5, 4, 11, 10});   // loops on top of odometry factors
  check_batch();
  if (g_bad) return 1;
  std::printf("OK\n");
  return 0;
}
