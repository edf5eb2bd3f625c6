// host_pool_check.cpp — CPU check of csrc/llsr_host.h and csrc/llsr_pools.h (run by
// tests/test_host_pools.py under AddressSanitizer / UBSan). This file defines the handful of HIP
// calls those headers use, over malloc, counting what is live and failing the k-th acquisition on
// request; the pools are laid out into mirrors of the library's argument structs (same member
// names and element sizes), so the layout functions exercised are the library's own.
//   1. every pool layout: measured size == end of the last placed piece, pieces 256-aligned,
//      back to back in call order, members in the order listed, every byte writable;
//   2. a failure at the k-th acquisition of a build, for every k it reaches: nothing stays live,
//      the target sub-state reads as never built; the old generation is freed before the new one;
//   3. owners release exactly once through move construction, move assignment, reset and scope exit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "llsr_pools.h"

// ---- the fake runtime ---------------------------------------------------------------------
static std::set<void*> g_live;
static size_t g_peak = 0;
static int g_calls = 0, g_fail_at = 0, g_bad = 0;

#define REQUIRE(c)                                                     \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      ++g_bad;                                                         \
    }                                                                  \
  } while (0)

static hipError_t acquire(void** out, size_t bytes) {
  if (++g_calls == g_fail_at) return hipErrorOutOfMemory;
  *out = std::aligned_alloc(256, bytes ? (bytes + 255) & ~size_t(255) : 256);
  g_live.insert(*out);
  if (g_live.size() > g_peak) g_peak = g_live.size();
  return hipSuccess;
}
static hipError_t release(void* p) {
  REQUIRE(g_live.erase(p) == 1);  // known and not yet released
  std::free(p);
  return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return acquire(p, n); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return acquire(p, n); }
hipError_t hipFree(void* p) { return release(p); }
hipError_t hipHostFree(void* p) { return release(p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return acquire((void**)e, 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return release(e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return acquire((void**)s, 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return release(s); }
}

using namespace llsr_host;

namespace {  // (internal linkage: the mirrors hold the hidden owner types)

// ---- mirrors of the library's structs (llsr_device.h, llsr_grid.h, llsr_mo.h, llsr_s2s.h, llsr_handle.h)
struct f4 { float x, y, z, w; };
struct i2 { int x, y; };
struct DevBufs {
  int *counts; float* orient; int* cell_pt; float* range; f4* full; int8_t* ground; int* label; f4* near_pts;
  int *shuf, *ccl_a; unsigned long long* ccl_b; int *start_ring, *end_ring; f4* seg; uint8_t* seg_ground;
  uint32_t* seg_col; float *seg_range, *seg_int; f4* outl; float* outl_int; f4* loam; float* curv;
  uint8_t* picked; int8_t* clabel; int *ring_cnt, *edge_tmp, *flat_tmp; f4* lflat_tmp;
  int *less_sharp, *cluster, *sharp, *flat; f4 *lflat, *db_pts; float* db_kz; uint32_t *db_adj, *mt0;
  int *phantom, *seg_zero;
};
struct CellSlot { uint64_t key; int start, count; };
struct CellGrid { int cap, log2T; CellSlot* tab; f4* sorted; i2* where; int* cursor; };
struct CellGrids2 { CellGrid g[2]; };
struct S2MProb { char bytes[256]; };
struct S2MArgs { S2MProb* prob; CellGrids2 grids; f4* rows; int* bcnt; float* blk_spill; int* n_active; };
struct S2SArgs { CellGrids2 grids; int* idx; f4* rows; uint8_t* valid; int* error; f4 *sbox, *sbox2; float* prof; };
struct Report { float v[9]; };
struct Odo {
  DevMem pool; PinnedMem host; Span zero[2]; int B = 0;
  float *tcur = nullptr, *tsum = nullptr; int *deg = nullptr, *inited = nullptr, *frames = nullptr;
  f4 *shadow = nullptr, *sharp = nullptr, *flat = nullptr, *scan_c = nullptr, *scan_s = nullptr;
  f4 *last_c[2] = {}, *last_s[2] = {}; int64_t* off = nullptr; Report* report = nullptr;
  float *guess = nullptr, *tlm = nullptr; unsigned char* flags = nullptr;
  int64_t* h_off = nullptr; int* h_counts = nullptr; float *h_tsum = nullptr, *h_guess = nullptr;
  unsigned char* h_flags = nullptr;
};
struct MapSmall {
  float* d_pose; Report* d_rep; int* d_deg; float* d_matP; int64_t* d_off; int* d_deg_bak; float* d_matP_bak;
  float* h_pose; Report* h_rep; int64_t* h_off; int* h_frames; float* h_tsum;
};
struct Stage { f4* cloud[4]; int64_t* off; float* pose; int* deg; char* rep; };

// ---- 1. layouts ---------------------------------------------------------------------------
// `members` (after placing): the struct's pointers in the order the layout lists them
template <class Layout, class Members>
static void check_layout(const char* name, Layout layout, Members members) {
  Carver measure;
  layout(measure);
  void* base = std::aligned_alloc(256, measure.off ? measure.off : 256);  // exactly the measured size
  std::vector<std::pair<size_t, size_t>> log;
  Carver place(base);
  place.log = &log;
  layout(place);
  REQUIRE(place.off == measure.off);
  size_t end = 0;
  for (const auto& piece : log) {
    REQUIRE(piece.first % 256 == 0);
    REQUIRE(piece.first == ((end + 255) & ~size_t(255)));  // after the previous piece, no gap beyond its pad
    end = piece.first + piece.second;
    std::memset((char*)base + piece.first, 0xA5, piece.second);  // in bounds (ASan)
  }
  REQUIRE(measure.off == ((end + 255) & ~size_t(255)));
  const std::vector<const void*> m = members();
  REQUIRE(m.size() == log.size());
  for (size_t k = 0; k < m.size() && k < log.size(); ++k) REQUIRE(m[k] == (const char*)base + log[k].first);
  if (g_bad) std::printf("  in layout %s\n", name);
  std::free(base);
}

static int log2_table(int cap) {
  int l = 4;
  while ((1ll << l) <= (long long)(cap > 1 ? cap : 1)) ++l;
  return l;
}

static void check_layouts() {
  const int caps[4] = {0, 1, 255, 257};
  for (int B : {1, 3}) {
    const size_t H = 16, HW = 16 * 16;
    DevBufs d{};
    check_layout("feature", [&](Carver& c) { feature_layout(c, d, B, H, HW, 16, 2048 * 64); }, [&] {
      return std::vector<const void*>{d.counts, d.orient, d.cell_pt, d.range, d.full, d.ground, d.label, d.near_pts,
          d.shuf, d.ccl_a, d.ccl_b, d.start_ring, d.end_ring, d.seg, d.seg_ground, d.seg_col, d.seg_range, d.seg_int,
          d.outl, d.outl_int, d.loam, d.curv, d.picked, d.clabel, d.ring_cnt, d.edge_tmp, d.flat_tmp, d.lflat_tmp,
          d.less_sharp, d.cluster, d.sharp, d.flat, d.lflat, d.db_pts, d.db_kz, d.db_adj, d.mt0, d.phantom, d.seg_zero};
    });
    Odo o;
    check_layout("odometry", [&](Carver& c) { odo_layout(c, o, B, B * (HW + 160), 160); }, [&] {
      return std::vector<const void*>{o.tcur, o.tsum, o.deg, o.inited, o.frames, o.shadow, o.sharp, o.flat, o.scan_c,
          o.scan_s, o.last_c[0], o.last_s[0], o.last_c[1], o.last_s[1], o.off, o.report, o.guess, o.tlm, o.flags};
    });
    // the reset spans: tcur .. frames and off .. flags, pads included, nothing else
    REQUIRE(o.zero[0].off == 0 && o.zero[0].off + o.zero[0].bytes == (size_t)((char*)o.shadow - (char*)o.tcur));
    REQUIRE(o.zero[1].off == (size_t)((char*)o.off - (char*)o.tcur));
    {
      Carver total;
      odo_layout(total, o, B, B * (HW + 160), 160);
      REQUIRE(o.zero[1].off + o.zero[1].bytes == total.off);
    }
    check_layout("odometry host", [&](Carver& c) { odo_host_layout(c, o, B, 16); }, [&] {
      return std::vector<const void*>{o.h_off, o.h_counts, o.h_tsum, o.h_guess, o.h_flags};
    });
    MapSmall m{};
    check_layout("mapping", [&](Carver& c) { mapping_layout(c, m, B); }, [&] {
      return std::vector<const void*>{m.d_pose, m.d_rep, m.d_deg, m.d_matP, m.d_off, m.d_deg_bak, m.d_matP_bak};
    });
    check_layout("mapping host", [&](Carver& c) { mapping_host_layout(c, m, B); }, [&] {
      return std::vector<const void*>{m.h_pose, m.h_rep, m.h_off, m.h_frames, m.h_tsum};
    });
    for (int ca : caps)
      for (int cb : caps) {
        const int blocks = (ca + 255) / 256 + (cb + 255) / 256;
        const S2MDims md{B, cb, ca, log2_table(cb), log2_table(ca), blocks ? blocks : 1, ca == 257 ? 3 : 0};
        S2MArgs a{};
        check_layout("scan2map", [&](Carver& c) { s2m_layout(c, a, md); }, [&] {
          const CellGrid* g = a.grids.g;
          return std::vector<const void*>{a.prob, g[0].tab, g[1].tab, g[0].sorted, g[1].sorted, g[0].where, g[1].where,
              g[0].cursor, g[1].cursor, a.rows, a.bcnt, a.blk_spill, a.n_active};
        });
        REQUIRE(a.grids.g[0].cap == cb && a.grids.g[1].cap == ca && a.grids.g[1].log2T == log2_table(ca));
        const S2SDims sd{B, ca, cb, cb, ca, log2_table(cb), log2_table(ca)};
        S2SArgs s{};
        check_layout("scan2scan", [&](Carver& c) { s2s_layout(c, s, sd); }, [&] {
          const CellGrid* g = s.grids.g;
          return std::vector<const void*>{g[0].tab, g[1].tab, g[0].sorted, g[1].sorted, g[0].where, g[1].where,
              g[0].cursor, g[1].cursor, s.idx, s.rows, s.valid, s.error, s.sbox, s.sbox2, s.prof};
        });
        const int32_t n[4] = {ca, cb, cb, ca};
        for (bool with_deg : {false, true}) {
          Stage st{};
          check_layout("one-shot stage", [&](Carver& c) { oneshot_layout(c, st, n, with_deg, sizeof(Report)); }, [&] {
            std::vector<const void*> v{st.cloud[0], st.cloud[1], st.cloud[2], st.cloud[3], st.off, st.pose};
            if (with_deg) v.push_back(st.deg);
            v.push_back(st.rep);
            return v;
          });
        }
      }
  }
}

// ---- 2. failure at the k-th acquisition -----------------------------------------------------
// The odometry state as odo_alloc builds it (two pools), then an LM stage's reserve: a pool, and
// the pinned flags and five events of its first use.
struct Lm {
  DevMem pool; PinnedMem flags; Event e[5]; int P = 0; S2SArgs a{};
};
static int32_t build_odo(Odo& o, int B) {
  o.B = B;
  if (alloc_pool(o.pool, 0, [&](Carver& c) { odo_layout(c, o, B, B * 416, 160); }) != hipSuccess) return -1;
  if (alloc_pool(o.host, 0, [&](Carver& c) { odo_host_layout(c, o, B, 16); }) != hipSuccess) return -2;
  return 0;
}
static int32_t build_lm(Lm& m, int P) {
  m.P = P;
  if (alloc(m.flags, 8) != hipSuccess) return -1;
  for (Event& e : m.e)
    if (create(e) != hipSuccess) return -2;
  const S2SDims sd{P, 3, 3, 257, 255, 9, 8};
  if (alloc_pool(m.pool, 64, [&](Carver& c) { s2s_layout(c, m.a, sd); }) != hipSuccess) return -3;
  return 0;
}

template <class S, class Build>
static void check_failures(int acquisitions, Build build) {
  for (int regrow = 0; regrow < 2; ++regrow)
    for (int k = 1; k <= acquisitions + 1; ++k) {
      S dst;
      g_fail_at = 0;
      if (regrow) REQUIRE(rebuild(dst, [&](S& n) { return build(n, 1); }) == 0 && (int)g_live.size() == acquisitions);
      g_calls = 0;
      g_fail_at = k;
      g_peak = 0;
      const int32_t rc = rebuild(dst, [&](S& n) { return build(n, 3); });
      REQUIRE((int)g_peak <= acquisitions);  // the old generation went before the new one came
      if (k <= acquisitions) {
        REQUIRE(rc != 0 && g_live.empty());
        REQUIRE(!dst.pool && dst.pool.get() == nullptr);
        REQUIRE(dst.B_or_P() == 0);
      } else {
        REQUIRE(rc == 0 && (int)g_live.size() == acquisitions && dst.pool && dst.B_or_P() == 3);
        REQUIRE(g_calls == acquisitions);  // every k the build reaches was injected
      }
      dst = S{};
      REQUIRE(g_live.empty());
    }
  g_fail_at = 0;
}
struct OdoState : Odo { int B_or_P() const { return B; } };
struct LmState : Lm { int B_or_P() const { return P; } };

// ---- 3. owners ----------------------------------------------------------------------------
static void check_owners() {
  {
    DevMem a, b;
    REQUIRE(alloc(a, 100) == hipSuccess && alloc(b, 100) == hipSuccess && g_live.size() == 2);
    void* pa = a.get();
    DevMem c(std::move(a));  // move construction: a gives up, nothing released
    REQUIRE(!a && c.get() == pa && g_live.size() == 2);
    b = std::move(c);  // move assignment: b's old buffer released, c gives up
    REQUIRE(!c && b.get() == pa && g_live.size() == 1);
    DevMem& self = b;
    b = std::move(self);  // self-move keeps the buffer
    REQUIRE(b.get() == pa && g_live.size() == 1);
    REQUIRE(alloc(b, 50) == hipSuccess && g_live.size() == 1 && g_live.count(pa) == 0);  // re-acquire releases
    g_fail_at = g_calls + 1;
    void* pb = b.get();
    REQUIRE(alloc(b, 50) != hipSuccess && b.get() == pb && g_live.size() == 1);  // a failure keeps what it held
    g_fail_at = 0;
    void* raw = b.release();  // release() hands the buffer out
    REQUIRE(!b && g_live.size() == 1);
    b.reset(raw);
    b.reset();
    REQUIRE(g_live.empty());
    PinnedMem p;
    Event e;
    Stream s;
    REQUIRE(alloc(p, 8) == hipSuccess && create(e) == hipSuccess && create(s, 0) == hipSuccess && g_live.size() == 3);
    Event ring[4][3];
    for (auto& set : ring)
      for (auto& ev : set) REQUIRE(create(ev) == hipSuccess);
    REQUIRE(g_live.size() == 15);
  }  // scope exit releases each once (release() asserts it)
  REQUIRE(g_live.empty());
}

}  // namespace

int main() {
  check_layouts();
  check_failures<OdoState>(2, [](OdoState& o, int B) { return build_odo(o, B); });
  check_failures<LmState>(7, [](LmState& m, int P) { return build_lm(m, P); });
  check_owners();
  std::printf("%s\n", g_bad ? "FAILED" : "OK");
  return g_bad ? 1 : 0;
}
