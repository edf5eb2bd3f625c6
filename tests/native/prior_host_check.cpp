// prior_host_check.cpp — CPU check of the prior map's host path (csrc/llsr_prior.h), run
// by tests/test_prior_native.py under AddressSanitizer / UBSan: the index build and the serial crop — the
// bodies the device kernels share — against a brute-force statement written here, with the output on
// the heap at exactly the size the crop reports (one point past the end is a sanitizer report):
//   * the hand-built edge clouds: d2 == r2 exactly, a sphere tangent to a tile face with points on the
//     face, points on and either side of tile boundaries at negative coordinates and -0.0, a sphere
//     that misses the map, one that contains it, a non-finite position, an empty kind;
//   * random clouds at random tiles, radii and positions, also far from the origin where a tile is a
//     few float32 ulps wide;
//   * the refusals and the capacity protocol.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "llsr_prior.h"

using namespace llsr_prior_ns;

static int g_bad = 0;
#define REQUIRE(c)                                               \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_bad;                                                   \
    }                                                            \
  } while (0)

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static double uni() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_rng >> 11) / 9007199254740992.0;
}
static float uf(double lo, double hi) { return (float)(lo + (hi - lo) * uni()); }

typedef std::vector<float> Cloud;  // [n][4]
static bool same_bits(const float* a, const Cloud& b) { return b.empty() || !memcmp(a, b.data(), b.size() * 4); }
static void push(Cloud& c, float x, float y, float z) {
  const float w = (float)(c.size() / 4);
  c.push_back(x); c.push_back(y); c.push_back(z); c.push_back(w);
}

// The specification, without tiles: keys by floorf(c / tile), a stable sort, the predicate per point.
static void brute_stored(const Cloud& in, float tile, Cloud* out, std::vector<uint32_t>* start) {
  const size_t n = in.size() / 4;
  out->clear();
  start->assign(1, 0u);
  if (!n) return;
  long lo[3], hi[3];
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const long t = (long)floorf(in[4 * i + a] / tile);
      if (!i || t < lo[a]) lo[a] = t;
      if (!i || t > hi[a]) hi[a] = t;
    }
  const long nx = hi[0] - lo[0] + 1, ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
  std::vector<long> key(n);
  for (size_t i = 0; i < n; ++i) {
    const long ix = (long)floorf(in[4 * i] / tile) - lo[0], iy = (long)floorf(in[4 * i + 1] / tile) - lo[1],
               iz = (long)floorf(in[4 * i + 2] / tile) - lo[2];
    key[i] = (iz * ny + iy) * nx + ix;
  }
  start->assign((size_t)(nx * ny * nz) + 1, 0u);
  for (long k = 0; k < nx * ny * nz; ++k) {  // (quadratic, small clouds only: the plainest stable sort)
    for (size_t i = 0; i < n; ++i)
      if (key[i] == k) out->insert(out->end(), in.begin() + 4 * i, in.begin() + 4 * i + 4);
    (*start)[(size_t)k + 1] = (uint32_t)(out->size() / 4);
  }
}
static void brute_crop(const Cloud& stored, const float* p, float r, Cloud* out) {
  const float r2 = (float)((double)r * (double)r);
  for (size_t i = 0; i < stored.size() / 4; ++i) {
    const float dx = stored[4 * i] - p[0], dy = stored[4 * i + 1] - p[1], dz = stored[4 * i + 2] - p[2];
    float d = 0.0f + dx * dx;
    d = d + dy * dy;
    d = d + dz * dz;
    if (d < r2) out->insert(out->end(), stored.begin() + 4 * i, stored.begin() + 4 * i + 4);
  }
}

// Build, crop with the capacity protocol on exact-size heap memory, compare bit for bit.
static void check(const Cloud& corner, const Cloud& surf, float radius, float tile, const std::vector<float>& pos) {
  Kind k[2];
  std::string err;
  REQUIRE(build_kind(corner.data(), (int64_t)(corner.size() / 4), tile, &k[0], &err) == 0);
  REQUIRE(build_kind(surf.data(), (int64_t)(surf.size() / 4), tile, &k[1], &err) == 0);
  Cloud st[2];
  std::vector<uint32_t> start;
  const Cloud* src[2] = {&corner, &surf};
  for (int a = 0; a < 2; ++a) {
    brute_stored(*src[a], tile, &st[a], &start);
    REQUIRE(st[a].size() == k[a].pts.size() && same_bits(k[a].pts.data(), st[a]));
    REQUIRE(start == k[a].tile_start);
  }
  const int P = (int)(pos.size() / 3);
  Cloud want;
  std::vector<int64_t> woc(P + 1, 0), wos(P + 1, 0);
  for (int a = 0; a < 2; ++a)
    for (int p = 0; p < P; ++p) {
      brute_crop(st[a], &pos[3 * p], radius, &want);
      (a ? wos : woc)[p + 1] = (int64_t)(want.size() / 4);
    }
  wos[0] = woc[P];
  std::vector<int64_t> oc(P + 1, -1), os(P + 1, -1);
  int64_t tested = -1;
  REQUIRE(crop_host(k, radius, tile, pos.data(), P, nullptr, 0, oc.data(), os.data(), &tested) == 0);
  REQUIRE(oc == woc && os == wos);
  const int64_t total = os[P];
  REQUIRE(tested >= total && tested <= (int64_t)((corner.size() + surf.size()) / 4) * P);
  if (total > 0) {  // one point short: refused, the sizes set, nothing written
    float* small = (float*)std::malloc((size_t)(total - 1) * 16 + 1);
    std::memset(small, 0x5a, (size_t)(total - 1) * 16 + 1);
    std::fill(oc.begin(), oc.end(), -1);
    REQUIRE(crop_host(k, radius, tile, pos.data(), P, small, total - 1, oc.data(), os.data(), nullptr) == -34);
    REQUIRE(oc == woc && os == wos);
    for (size_t b = 0; b < (size_t)(total - 1) * 16; ++b) REQUIRE(((unsigned char*)small)[b] == 0x5a);
    std::free(small);
  }
  float* out = (float*)std::malloc((size_t)total * 16 + 1);
  REQUIRE(crop_host(k, radius, tile, pos.data(), P, out, total, oc.data(), os.data(), nullptr) == 0);
  REQUIRE(oc == woc && os == wos);
  REQUIRE((size_t)total * 4 == want.size() && same_bits(out, want));
  std::free(out);
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  auto dn = [](float v, float to) { return nextafterf(v, to); };
  {  // d2 == r2 exactly
    Cloud c;
    push(c, 3, 4, 0); push(c, 3, dn(4, 0), 0); push(c, dn(3, 0), 4, 0); push(c, -3, -4, 0); push(c, -3, dn(-4, 0), 0);
    push(c, 0, 0, 5); push(c, 0, 0, dn(5, 0)); push(c, 0, 0, dn(5, 9)); push(c, 0, 0, 0);
    check(c, Cloud(), 5.0f, 1.0f, {0, 0, 0});
    Kind k[2];
    std::string err;
    build_kind(c.data(), 9, 1.0f, &k[0], &err);
    build_kind(nullptr, 0, 1.0f, &k[1], &err);
    const float p[3] = {0, 0, 0};
    int64_t oc[2], os[2];
    float out[9 * 4];
    REQUIRE(crop_host(k, 5.0f, 1.0f, p, 1, out, 9, oc, os, nullptr) == 0);
    bool has0 = false, has1 = false;
    for (int64_t i = 0; i < oc[1]; ++i) { has0 |= out[4 * i + 3] == 0.0f; has1 |= out[4 * i + 3] == 1.0f; }
    REQUIRE(!has0 && has1);  // (3, 4, 0) is out, its float32 neighbour inside is in
  }
  {  // tangent to the tile faces x, y, z = +-5, points on the faces; tile 1 and tile 5
    Cloud c;
    for (int a = 0; a < 3; ++a)
      for (float s : {5.0f, -5.0f}) {
        float v[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        v[0][a] = s; v[1][a] = dn(s, 0); v[2][a] = dn(s, 9 * s);
        for (auto& q : v) push(c, q[0], q[1], q[2]);
      }
    check(c, c, 5.0f, 1.0f, {0, 0, 0});
    check(c, Cloud(), 5.0f, 5.0f, {0, 0, 0, 0.5f, 0, 0});
  }
  {  // tile boundaries, negative coordinates, -0.0; misses, contains, non-finite positions
    Cloud c;
    std::vector<float> g;
    for (float v : {-3.0f, -2.0f, -1.0f, -0.0f, 0.0f, 1.0f, 2.0f}) { g.push_back(dn(v, -9)); g.push_back(v); g.push_back(dn(v, 9)); }
    for (float x : g)
      for (float y : g)
        for (float z : {-1.0f, dn(0, -9), 0.0f, 0.5f}) push(c, x, y, z);
    Cloud half(c.begin(), c.begin() + c.size() / 8 * 4);
    const std::vector<float> pos = {0, 0, 0, -1, -1, 0, -2.5f, 1.5f, -0.5f, 1, -3, 0.25f, 0.3f, 0.3f, 0.3f};
    check(c, half, 2.0f, 1.0f, pos);
    check(c, half, 1.0f, 0.5f, pos);
    check(c, half, 3.0f, 1.0f, {1000, 0, 0, 0, -1000, 0, 0, 0, 1e30f, nan, 0, 0, 0, inf, 0});
    check(c, half, 100.0f, 1.0f, {0, 0, 0, 3, 3, 3});
    check(Cloud(), Cloud(), 2.0f, 1.0f, {0, 0, 0});
  }
  for (int it = 0; it < 60; ++it) {  // random clouds; every third far from the origin
    const float tile = uf(0.3, 3.0), radius = uf(0.2, 6.0);
    const double off = it % 3 == 2 ? 2.0e5 * (uni() - 0.5) * 2 : 0.0, ext = uf(2.0, 12.0);
    Cloud c, s;
    const int nc = (int)(uni() * 600), ns = (int)(uni() * 600);
    for (int i = 0; i < nc; ++i) push(c, (float)(off + uf(-ext, ext)), (float)(off + uf(-ext, ext)), uf(-2, 2));
    for (int i = 0; i < ns; ++i) push(s, (float)(off + uf(-ext, ext)), (float)(off + uf(-ext, ext)), uf(-2, 2));
    std::vector<float> pos;
    for (int p = 0; p < 4; ++p) {
      pos.push_back((float)(off + uf(-ext - 2, ext + 2))); pos.push_back((float)(off + uf(-ext - 2, ext + 2))); pos.push_back(uf(-3, 3));
    }
    if (nc) { pos.push_back(c[0]); pos.push_back(c[1]); pos.push_back(c[2]); }  // on a point
    check(c, s, radius, tile, pos);
  }
  {  // refusals
    Kind k;
    std::string err;
    float bad[8] = {0, 0, 0, 0, 1, nan, 0, 1};
    REQUIRE(build_kind(bad, 2, 1.0f, &k, &err) == -22 && err.find("non-finite") != std::string::npos);
    bad[5] = -inf;
    REQUIRE(build_kind(bad, 2, 1.0f, &k, &err) == -22);
    float far[8] = {0, 0, 0, 0, 1000, 1000, 1000, 1};
    REQUIRE(build_kind(far, 2, 1.0f, &k, &err) == -34 && err.find("a tile of 4 fits") != std::string::npos);
    REQUIRE(build_kind(far, 2, 4.0f, &k, &err) == 0 && k.tiles() == 251 * 251 * 251 && k.used == 2);
    float huge[8] = {3e38f, 0, 0, 0, -3e38f, 0, 0, 1};
    REQUIRE(build_kind(huge, 2, 1e-3f, &k, &err) == -34);
    float out_of_index[4] = {3e9f, 0, 0, 0};  // one tile, but its index leaves +-2^30
    REQUIRE(build_kind(out_of_index, 1, 1.0f, &k, &err) == -34 && err.find("fits") != std::string::npos);
    REQUIRE(!positive_finite(0.0f) && !positive_finite(-1.0f) && !positive_finite(nan) && !positive_finite(inf) &&
            positive_finite(1e-30f));
  }
  if (g_bad) return 1;
  std::printf("OK\n");
  return 0;
}
