// icp_host_check.cpp — CPU check of the loop-closure ICP's shared bodies (csrc/llsr_icp.h), run by
// tests/test_icp_native.py under AddressSanitizer / UBSan. Everything here runs the library's own
// text over heap buffers of exactly the sizes icp_sizes() gives the device workspace:
//   1. nn_search over the serially built cell grid against a brute-force loop (§16's d^2, the lowest
//      index among equal d^2), on lattice ties, a best d^2 equal to the finished shell's r^2, queries
//      far outside the box, in empty cells, a one-cell target, a sparse box, NaN / huge coordinates;
//   2. the chains: means_body / sigma_body / finish_body over their launch shapes against
//      umeyama3_host on the same pairs, at the depth-block edges of sigma;
//   3. the index mappings: sigma_blocks_max bounds the block count for every n, sigma_lane's ranges
//      tile [0, n) once per entry, and the whole driver (every launch's (block, thread) loop, on a
//      table of one entry) runs over exact-size buffers for the launch shapes the tests use.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "llsr_icp.h"

using namespace llsr_loop;

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
static float uf(double lo, double hi) { return (float)(lo + (hi - lo) * uni()); }

template <class T>
struct Heap {  // exactly n elements on the heap: one past the end is a sanitizer report
  T* p;
  explicit Heap(size_t n) : p(static_cast<T*>(std::malloc(n * sizeof(T)))) { std::memset(p, 0, n * sizeof(T)); }
  ~Heap() { std::free(p); }
  Heap(const Heap&) = delete;
  Heap& operator=(const Heap&) = delete;
};

struct Run {  // one alignment's buffers at their exact sizes
  IcpSizes z;
  Heap<llsr::CellSlot> tab;
  Heap<float> cells, work, d2, ps, pd, part, al;
  Heap<int> match, box;
  Heap<IcpState> st;
  IcpArgs a;
  Run(const std::vector<float>& src, const std::vector<float>& tgt)
      : z(icp_sizes((int)src.size() / 4, (int)tgt.size() / 4)), tab(z.tab), cells(z.cells4), work(z.work4), d2(z.d2),
        ps(z.ps4), pd(z.pd4), part(z.part), al(z.aligned4), match(z.match), box(6), st(1), a{} {
    a.src4 = src.data(); a.tgt4 = tgt.data(); a.tab = tab.p; a.cells4 = cells.p; a.box = box.p;
    a.work4 = work.p; a.match = match.p; a.d2 = d2.p; a.ps4 = ps.p; a.pd4 = pd.p; a.part = part.p;
    a.st = st.p; a.aligned4 = al.p;
    a.n_src = (int)src.size() / 4; a.n_tgt = (int)tgt.size() / 4; a.log2T = z.log2T;
    a.max_iterations = 100; a.eps_t = 1e-6; a.eps_f = 1e-6; a.mcd2 = 100.0 * 100.0;
    grid_build_host(a.tgt4, a.n_tgt, a.log2T, tab.p, cells.p, box.p);
  }
};

static bool in_grid(const float* p) {
  for (int a = 0; a < 3; ++a) {
    const float f = std::floor(p[a]);
    if (!(f > -1048000.0f && f < 1048000.0f)) return false;
  }
  return true;
}

static bool brute(const std::vector<float>& tgt, const float* q, int* idx, float* d2) {
  if (!in_grid(q)) return false;
  bool have = false;
  for (size_t k = 0; k < tgt.size() / 4; ++k) {
    const float* p = &tgt[4 * k];
    if (!in_grid(p)) continue;
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    const float d = (dx * dx + dy * dy) + dz * dz;
    if (!have || d < *d2) {  // strict: the lowest index among equal d^2
      have = true;
      *d2 = d;
      *idx = (int)k;
    }
  }
  return have;
}

static void push(std::vector<float>& v, float x, float y, float z) {
  v.push_back(x); v.push_back(y); v.push_back(z); v.push_back(1.0f);
}

static void check_search(const std::vector<float>& tgt, const std::vector<float>& queries, int* ties) {
  std::vector<float> none;
  Run r(none, tgt);
  // the box the driver computes (icp_run_host's first loop), here for the search alone
  for (int i = 0; i < r.a.n_tgt; ++i) {
    int c[3];
    if (!box_cell(r.a, i, c)) continue;
    for (int k = 0; k < 3; ++k) {
      if (c[k] < r.box.p[k]) r.box.p[k] = c[k];
      if (c[k] > r.box.p[3 + k]) r.box.p[3 + k] = c[k];
    }
  }
  for (size_t k = 0; k < queries.size() / 4; ++k) {
    const float* q = &queries[4 * k];
    int gi = -1, wi = -1;
    float gd = 0, wd = 0;
    const bool g = nn_search(r.a.tab, r.a.log2T, r.a.cells4, r.a.box, q[0], q[1], q[2], &gi, &gd);
    const bool w = brute(tgt, q, &wi, &wd);
    REQUIRE(g == w);
    if (g && w) {
      REQUIRE(gi == wi);
      REQUIRE(std::memcmp(&gd, &wd, 4) == 0);
      if (ties) {  // count queries with a second target at the same d^2
        for (size_t j = 0; j < tgt.size() / 4; ++j) {
          const float* p = &tgt[4 * j];
          const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
          if ((int)j != wi && (dx * dx + dy * dy) + dz * dz == wd) { ++*ties; break; }
        }
      }
    }
  }
}

static void search_cases() {
  // lattice with holes, present twice; queries midway and on the holes (best d^2 = 1 = r^2 of shell 1)
  std::vector<float> lat, q;
  for (int rep = 0; rep < 2; ++rep)
    for (int x = -3; x <= 3; ++x)
      for (int y = -3; y <= 3; ++y)
        for (int z = 0; z <= 3; ++z)
          if (!((x == 0 && y == 0 && z == 1) || (x == 2 && y == -1 && z == 2))) push(lat, (float)x, (float)y, (float)z);
  push(q, 0, 0, 1); push(q, 2, -1, 2); push(q, 0.5f, 1, 1); push(q, 1, -1.5f, 2); push(q, 0.5f, 0.5f, 1.5f);
  push(q, -2, 0, 1.5f); push(q, 80.0f, 0, 0); push(q, -3.5f, -3.5f, -0.5f); push(q, 0, 0, 90.0f);
  push(q, NAN, 0, 0); push(q, 0, 2.0e6f, 0); push(q, 0, 0, -1.1e6f);
  for (int k = 0; k < 300; ++k) push(q, uf(-6, 6), uf(-6, 6), uf(-3, 7));
  int ties = 0;
  check_search(lat, q, &ties);
  REQUIRE(ties >= 6);
  // a gappy structure, queries 80 m outside, in empty cells, NaN / sentinel targets present
  std::vector<float> t2, q2;
  for (int k = 0; k < 500; ++k) push(t2, uf(-20, 20), uf(-20, 20), k % 3 ? -1.5f : uf(-1.5, 6));
  push(t2, NAN, 1, 1); push(t2, 1, -3.0e6f, 1);
  push(q2, 100.5f, 0.5f, 0.5f); push(q2, 0.5f, -97.0f, 2.0f); push(q2, 0.5f, 0.5f, 4.5f); push(q2, 170.0f, 3.0f, 1.0f);
  for (int k = 0; k < 300; ++k) push(q2, uf(-30, 30), uf(-30, 30), uf(-5, 10));
  check_search(t2, q2, nullptr);
  // one cell; one point; a sparse box; an empty target; only unusable targets
  std::vector<float> t3, t4, t5, t6, t7;
  for (int k = 0; k < 7; ++k) push(t3, uf(4.1, 4.9), uf(-2.9, -2.1), uf(1.1, 1.9));
  push(t4, -0.5f, 0.25f, 3.0f);
  for (int k = 0; k < 40; ++k) push(t5, uf(-30, 30), uf(-30, 30), uf(-2, 10));
  push(t7, NAN, NAN, NAN); push(t7, 2.0e6f, 0, 0);
  check_search(t3, q2, nullptr);
  check_search(t4, q2, nullptr);
  check_search(t5, q2, nullptr);
  check_search(t6, q2, nullptr);
  check_search(t7, q2, nullptr);
}

// the solve step of one iteration over its launch shapes against umeyama3_host
static void chain_cases() {
  const int sizes[] = {3, 5, 13, 14, 47, 48, 679, 680, 681, 1360, 1361, 2041};
  for (int n : sizes) {
    std::vector<float> src, tgt;
    for (int k = 0; k < n; ++k) push(src, uf(-30, 30), uf(-30, 30), uf(-3, 8));
    push(tgt, 0, 0, 0);
    Run r(src, tgt);
    std::vector<float> s3(3 * (size_t)n), d3(3 * (size_t)n);
    const float c = std::cos(0.3f), s = std::sin(0.3f);
    for (int k = 0; k < n; ++k) {
      const float* p = &src[4 * (size_t)k];
      const float d[3] = {c * p[0] - s * p[1] + 4.0f + uf(-0.05, 0.05), s * p[0] + c * p[1] - 2.0f + uf(-0.05, 0.05),
                          p[2] + 0.5f + uf(-0.05, 0.05)};
      for (int a = 0; a < 3; ++a) {
        r.ps.p[4 * (size_t)k + a] = s3[3 * (size_t)k + a] = p[a];
        r.pd.p[4 * (size_t)k + a] = d3[3 * (size_t)k + a] = d[a];
      }
      r.ps.p[4 * (size_t)k + 3] = uf(0, 2);
    }
    state_init(r.a.st);
    r.a.st->n_pairs = n;
    for (int lane = 0; lane < kLaneBlock; ++lane) means_body(r.a, lane);
    for (int blk = 0; blk < blocks_for(9 * sigma_blocks_max(n), kCorrBlock); ++blk)
      for (int t = 0; t < kCorrBlock; ++t) sigma_body(r.a, point_of(blk, t, kCorrBlock));
    finish_body(r.a);
    float T[16];
    umeyama3_host(s3.data(), d3.data(), n, T);
    REQUIRE(std::memcmp(T, r.a.st->T, sizeof T) == 0);
    REQUIRE(std::memcmp(T, r.a.st->fin, sizeof T) == 0);  // final = T * I
    double mse = 0.0;
    for (int k = 0; k < n; ++k) mse = mse + (double)r.ps.p[4 * (size_t)k + 3];
    REQUIRE(mse == r.a.st->mse_sum);
    REQUIRE(r.a.st->iterations == 1);
  }
}

static void mapping_cases() {
  for (int n = 0; n <= 300000; ++n) {
    const int kc = n > 0 ? sigma_block(n) : 1;
    REQUIRE(kc >= 1);
    const int blocks = (n + kc - 1) / kc;
    if (blocks > sigma_blocks_max(n)) {
      REQUIRE(blocks <= sigma_blocks_max(n));
      break;
    }
  }
  const int sizes[] = {3, 14, 680, 681, 1360, 1361, 1474, 5000};
  for (int n : sizes) {
    std::vector<int> seen(9 * (size_t)n, 0);
    const int lanes = blocks_for(9 * sigma_blocks_max(n), kCorrBlock) * kCorrBlock;
    for (int t = 0; t < lanes; ++t) {
      int b, i, j, first, last;
      if (!sigma_lane(t, n, &b, &i, &j, &first, &last)) continue;
      REQUIRE(t < 9 * sigma_blocks_max(n) && first >= 0 && first < last && last <= n && last - first <= sigma_block(n));
      for (int k = first; k < last; ++k) ++seen[(size_t)(3 * i + j) * n + k];
    }
    bool once = true;
    for (int v : seen) once = once && v == 1;
    REQUIRE(once);
  }
  int b, i, j, first, last;
  REQUIRE(!sigma_lane(0, 2, &b, &i, &j, &first, &last));
  REQUIRE(blocks_for(0, 256) == 1 && blocks_for(256, 256) == 1 && blocks_for(257, 256) == 2);
  // the whole driver over the launch shapes of the tests, buffers at their exact sizes
  const int shapes[][2] = {{3, 3}, {0, 5}, {5, 0}, {1, 1}, {7, 16}, {255, 300}, {256, 1024}, {257, 1025},
                           {1024, 2048}, {1025, 4095}, {1474, 3000}, {1500, 6000}};
  for (const auto& sh : shapes) {
    std::vector<float> tgt, src;
    for (int k = 0; k < sh[1]; ++k) push(tgt, uf(-20, 20), uf(-20, 20), k % 2 ? -1.5f : uf(-1.5, 6));
    for (int k = 0; k < sh[0]; ++k) {
      if (sh[1] > 0 && k % 13 != 5) {
        const float* p = &tgt[4 * (size_t)((k * 7) % sh[1])];
        push(src, p[0] + 0.05f, p[1] - 0.04f, p[2] + 0.03f);
      } else {
        push(src, uf(170, 175), uf(-5, 5), uf(0, 2));
      }
    }
    Run r(src, tgt);
    REQUIRE(icp_run_host(&r.a, 1) >= 1);
    REQUIRE(r.a.st->state != kStateNone);
    REQUIRE(r.a.st->n_pairs <= sh[0]);
    if (sh[0] >= 3 && sh[1] >= 3) REQUIRE(r.a.st->iterations >= 1);
  }
}

int main() {
  search_cases();
  chain_cases();
  mapping_cases();
  if (g_bad) return 1;
  std::printf("OK\n");
  return 0;
}
