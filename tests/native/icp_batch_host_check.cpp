// icp_batch_host_check.cpp — CPU check of the loop-closure ICP's host driver on a table of many
// problems (csrc/llsr_icp.h, DESIGN.md §16 "Batch form"), run by tests/test_icp_batch_native.py under
// AddressSanitizer / UBSan. icp_run_host — the batch launches of llsr_icp.hip as loops over their
// (block.x, block.y, thread) ranges — runs over one table built by icp_batch_layout / icp_batch_entry, the
// functions the device call builds its table with, over heap buffers of exactly the sizes the layout
// gives. The batch mixes an empty source, an empty target, 2, 3 and 681 kept pairs, and a 7-point
// target next to 3000-point ones, in both orders; every problem's state, final, fitness and aligned
// cloud must equal the same driver on that problem as a hand-filled table of one (exact icp_sizes
// buffers, its own table size), bit for bit: no result depends on log2T, the slices or the order.
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

static uint64_t g_rng = 0x13198A2E03707344ull;
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

static void push(std::vector<float>& v, float x, float y, float z) {
  v.push_back(x); v.push_back(y); v.push_back(z); v.push_back(1.0f);
}

struct Problem {
  std::vector<float> src, tgt;
  int max_iterations = 100;
};

// n_tgt structure points; `kept` source points a small motion away from targets, interleaved with
// points 150 m outside (never a pair), so the packed order differs from the source order
static Problem make(int n_tgt, int kept, int n_far) {
  Problem pr;
  for (int k = 0; k < n_tgt; ++k) push(pr.tgt, uf(-20, 20), uf(-20, 20), k % 2 ? -1.5f : uf(-1.5, 6));
  int far_left = n_far, near_left = kept, k = 0;
  while (far_left + near_left > 0) {
    const bool far = near_left == 0 || (far_left > 0 && k % 5 == 2);
    if (far) {
      push(pr.src, uf(170, 175), uf(-5, 5), uf(0, 2));
      --far_left;
    } else {
      const float* p = &pr.tgt[4 * (size_t)((near_left * 11) % n_tgt)];  // distinct targets (11 is coprime to n_tgt)
      push(pr.src, p[0] + 0.05f, p[1] - 0.04f, p[2] + 0.03f);
      --near_left;
    }
    ++k;
  }
  return pr;
}

struct Alone {  // one problem as a table of one through icp_run_host, buffers at icp_sizes
  IcpSizes z;
  Heap<llsr::CellSlot> tab;
  Heap<float> cells, work, d2, ps, pd, part, al;
  Heap<int> match, box;
  Heap<IcpState> st;
  explicit Alone(const Problem& pr)
      : z(icp_sizes((int)pr.src.size() / 4, (int)pr.tgt.size() / 4)), tab(z.tab), cells(z.cells4), work(z.work4),
        d2(z.d2), ps(z.ps4), pd(z.pd4), part(z.part), al(z.aligned4), match(z.match), box(6), st(1) {
    IcpArgs a{};
    a.src4 = pr.src.data(); a.tgt4 = pr.tgt.data(); a.tab = tab.p; a.cells4 = cells.p; a.box = box.p;
    a.work4 = work.p; a.match = match.p; a.d2 = d2.p; a.ps4 = ps.p; a.pd4 = pd.p; a.part = part.p;
    a.st = st.p; a.aligned4 = al.p;
    a.n_src = (int)pr.src.size() / 4; a.n_tgt = (int)pr.tgt.size() / 4; a.log2T = z.log2T;
    a.max_iterations = pr.max_iterations; a.eps_t = 1e-6; a.eps_f = 1e-6; a.mcd2 = 100.0 * 100.0;
    grid_build_host(a.tgt4, a.n_tgt, a.log2T, tab.p, cells.p, box.p);
    REQUIRE(icp_run_host(&a, 1) >= 1);
  }
};

// the batch over `order` (indices into all), checked against the single runs; returns the passes
static int run_batch(const std::vector<Problem>& all, const std::vector<Alone*>& alone, const std::vector<int>& order) {
  const int P = (int)order.size();
  std::vector<int64_t> so(P + 1, 0), to(P + 1, 0);
  for (int p = 0; p < P; ++p) {
    so[p + 1] = so[p] + (int64_t)all[order[p]].src.size() / 4;
    to[p + 1] = to[p] + (int64_t)all[order[p]].tgt.size() / 4;
  }
  const IcpBatchLayout L = icp_batch_layout(P, so.data(), to.data());
  Heap<float> src(4 * (size_t)so[P]), tgt(4 * (size_t)to[P]);
  for (int p = 0; p < P; ++p) {
    const Problem& pr = all[order[p]];
    if (!pr.src.empty()) std::memcpy(src.p + 4 * so[p], pr.src.data(), pr.src.size() * sizeof(float));
    if (!pr.tgt.empty()) std::memcpy(tgt.p + 4 * to[p], pr.tgt.data(), pr.tgt.size() * sizeof(float));
  }
  Heap<llsr::CellSlot> tab(L.tab);
  Heap<float> cells(4 * L.cells), work(4 * L.points), ps(4 * L.points), pd(4 * L.points), al(4 * L.points),
      d2(L.points), part(L.part);
  Heap<int> match(L.points), box(6 * (size_t)P);
  Heap<IcpState> st((size_t)P);
  Heap<IcpArgs> args((size_t)P);
  IcpBatchBuffers b{};
  b.src4 = src.p; b.tgt4 = tgt.p; b.tab = tab.p; b.cells4 = cells.p; b.box = box.p;
  b.work4 = work.p; b.ps4 = ps.p; b.pd4 = pd.p; b.match = match.p; b.d2 = d2.p; b.part = part.p;
  b.st = st.p; b.aligned4 = al.p;
  size_t part_at = 0;
  for (int p = 0; p < P; ++p) {
    IcpArgs* a = &args.p[p];
    icp_batch_entry(L, b, so.data(), to.data(), p, &part_at, a);
    a->max_iterations = all[order[p]].max_iterations; a->eps_t = 1e-6; a->eps_f = 1e-6; a->mcd2 = 100.0 * 100.0;
    grid_build_host(a->tgt4, a->n_tgt, a->log2T, const_cast<llsr::CellSlot*>(a->tab), const_cast<float*>(a->cells4),
                    a->box);
  }
  REQUIRE(part_at == L.part);
  const int passes = icp_run_host(args.p, P);
  REQUIRE(passes >= 1);
  for (int p = 0; p < P; ++p) {
    const IcpState& g = st.p[p];
    const IcpState& w = *alone[order[p]]->st.p;
    const size_t n = all[order[p]].src.size() / 4;
    REQUIRE(g.state == w.state && g.state != kStateNone);
    REQUIRE(g.iterations == w.iterations && g.converged == w.converged && g.n_pairs == w.n_pairs);
    REQUIRE(std::memcmp(g.fin, w.fin, sizeof g.fin) == 0);
    REQUIRE(g.n_fit == w.n_fit && std::memcmp(&g.fit_sum, &w.fit_sum, sizeof g.fit_sum) == 0);
    REQUIRE(n == 0 || std::memcmp(args.p[p].aligned4, alone[order[p]]->al.p, 4 * n * sizeof(float)) == 0);
    REQUIRE(passes >= g.iterations);
  }
  return passes;
}

int main() {
  std::vector<Problem> all;
  all.push_back(make(3000, 0, 0));     // 0: an empty source
  all.push_back(make(3000, 5, 4));     // 1: an empty target (cleared below)
  all[1].tgt.clear();
  all.push_back(make(3000, 2, 4));     // 2: 2 pairs: no correspondences
  all.push_back(make(3000, 3, 4));     // 3: 3 pairs
  all.push_back(make(3000, 681, 56));  // 4: 681 pairs: two depth blocks of sigma
  all.push_back(make(7, 7, 9));        // 5: a 7-point target in a table sized for 3000
  all.push_back(make(3000, 200, 16));  // 6: stopped by a cap of 1 iteration while others go on
  all[6].max_iterations = 1;
  std::vector<Alone*> alone;
  for (const Problem& pr : all) alone.push_back(new Alone(pr));
  REQUIRE(alone[0]->st.p->state == kStateNoCorrespondences && alone[1]->st.p->state == kStateNoCorrespondences);
  REQUIRE(alone[2]->st.p->n_pairs == 2 && alone[2]->st.p->state == kStateNoCorrespondences);
  REQUIRE(alone[3]->st.p->n_pairs == 3 && alone[3]->st.p->iterations >= 1);
  REQUIRE(alone[4]->st.p->n_pairs == 681 && alone[4]->st.p->iterations >= 2);
  REQUIRE(alone[6]->st.p->state == kStateIterations && alone[6]->st.p->iterations == 1);
  int most = 0;
  for (const Alone* a : alone) most = a->st.p->iterations > most ? a->st.p->iterations : most;
  // the whole mix, its reverse (the small target first, the empty source last), and single-problem batches
  REQUIRE(run_batch(all, alone, {0, 1, 2, 3, 4, 5, 6}) == most);
  REQUIRE(run_batch(all, alone, {6, 5, 4, 3, 2, 1, 0}) == most);
  for (int k = 0; k < (int)all.size(); ++k) run_batch(all, alone, {k});
  // only problems that stop in the first pass: one pass
  REQUIRE(run_batch(all, alone, {0, 1, 2}) == 1);
  for (Alone* a : alone) delete a;
  if (g_bad) return 1;
  std::printf("OK\n");
  return 0;
}
