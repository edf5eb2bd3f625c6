// llsr_prior.h — the prior map: a static corner and a static surf cloud, each stably
// sorted by the key of a tile grid, with a CSR over the tiles, and the crop of both around P positions.
// The reference has no such mode; every order of evaluation here is this project's statement.
//
// This header is the whole host side of the object — the index build, the tile geometry and the
// serial crop — and compiles without HIP (tests/native/prior_host_check.cpp). llsr_prior.hip adds the
// device copy of the index and the kernels; they share the LLSR_HD bodies below, so the device tests
// the same points against the same predicate in the same order.
//
//   stored order   tile coordinate i = (int)floorf(c / tile) - min over the cloud, per axis, the
//                  division one correctly rounded float32 divide; key = (iz ny + iy) nx + ix; the
//                  cloud stably sorted by key; tile_start[ntiles + 1].
//   predicate      d2 = ((0 + dx^2) + dy^2) + dz^2 in float32, no contraction; d2 < float(double(r)
//                  double(r)) (llsr_keypose_radius_sorted's).
//   rows           with x fastest in the key, the tiles (ix0 .. ix1, iy, iz) are one contiguous range
//                  of the stored cloud. A crop walks the rows of a (y, z) box of tiles in key order and
//                  tests every point of each row's x range: stored order within a row by
//                  construction, across rows by their order.
//   shortcuts      tiles are only ever skipped, never copied untested. Which tiles a row may skip is
//                  decided in double with explicit slack (tile_lo / tile_hi / tile_span below): a
//                  tile is skipped only when no float32 coordinate that floorf(c / tile) can send to
//                  it passes the float32 predicate. The per-point predicate alone decides the result.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "llsr_libm.h"

namespace llsr_prior_ns {

constexpr int64_t kMaxTiles = (int64_t)1 << 24;   // per kind
constexpr int64_t kMaxPoints = 2147483646;        // per kind (2^31 - 2)
constexpr int32_t kMaxTileIndex = 1 << 30;        // |floorf(c / tile)| beyond this is refused
constexpr int kWaves = 4;                         // parts a row is split into (one wave each on the device)
constexpr int kLoads = 4;                         // float4 loads a lane keeps in flight
constexpr int kChunk = 64 * kLoads;               // points a wave tests per step
constexpr double kSlack = 9.5367431640625e-07;    // 2^-20: 16 float32 ulps, 2^33 double ulps

// One kind's index. Host memory; llsr_prior.hip mirrors pts / tile_start on the device.
struct Kind {
  std::vector<float> pts;             // [n][4] in stored order
  std::vector<uint32_t> tile_start;   // [ntiles + 1]
  int32_t o[3] = {0, 0, 0};           // min floorf(c / tile) per axis
  int32_t n[3] = {0, 0, 0};           // nx, ny, nz
  int64_t used = 0;                   // tiles with at least one point
  int64_t size() const { return (int64_t)(pts.size() / 4); }
  int64_t tiles() const { return (int64_t)n[0] * n[1] * n[2]; }
};

// The (y, z) box of tiles a crop walks for one position and kind; ny * nz rows, possibly none.
struct Box {
  int32_t y0, ny, z0, nz;
};

// What a row's geometry needs of a kind (the device copy of Kind's scalars)
struct Grid {
  int32_t ox, oy, oz, nx, ny, nz;
};

LLSR_HD bool in_sphere(float x, float y, float z, float px, float py, float pz, float r2) {
  const float dx = x - px, dy = y - py, dz = z - pz;
  float d = 0.0f + dx * dx;
  d = d + dy * dy;
  d = d + dz * dz;
  return d < r2;
}

// ---- tile geometry in double, conservative by construction -------------------------------------------
// A float32 coordinate c lands in tile t = floorf(q), q = fl(c / tile), |q - c / tile| <= 2^-24 |c /
// tile| + 2^-149. All three bounds below widen by (|.| + 2) 2^-20 tile widths, 16 times that error or
// more, and the double operations that form them err by 2^-53 relative: no rounding on either side can
// move a coordinate across them.
//   tile_lo(x): a lower bound of the tile of every coordinate c >= x;
//   tile_hi(x): an upper bound of the tile of every coordinate c <= x;
//   tile_span(t): every coordinate of tile t lies in [lo, hi].
LLSR_HD double tile_lo(double x, double tile) {
  const double u = x / tile;
  return floor(u - (fabs(u) + 2.0) * kSlack);
}
LLSR_HD double tile_hi(double x, double tile) {
  const double u = x / tile;
  return floor(u + (fabs(u) + 2.0) * kSlack);
}
LLSR_HD void tile_span(double t, double tile, double* lo, double* hi) {
  const double s = (fabs(t) + 2.0) * kSlack;
  *lo = (t - s) * tile;
  *hi = (t + 1.0 + s) * tile;
}
// Clamp the absolute tile range [a, b] to a grid axis (origin o, n tiles): relative [*i0, *i1], empty
// when *i1 < *i0. A NaN bound keeps the whole axis.
LLSR_HD void clamp_axis(double a, double b, int32_t o, int32_t n, int32_t* i0, int32_t* i1) {
  double lo = a - (double)o, hi = b - (double)o;
  lo = lo > 0.0 ? lo : 0.0;                         // NaN -> 0
  hi = hi < (double)(n - 1) ? hi : (double)(n - 1); // NaN -> n - 1
  if (!(lo <= hi)) {
    *i0 = 0;
    *i1 = -1;
    return;
  }
  *i0 = (int32_t)lo;
  *i1 = (int32_t)hi;
}
// The squared radius the real-number squared distance of a passing point stays below. Along any one
// term of the float32 predicate lie at most five roundings (its difference, taken twice by the square,
// the square, two sums), each within 2^-24 and sums of non-negative floats monotone, so that distance
// is below r2 (1 + 2^-24)^5 < r2 (1 + 2^-21); 2^-20 leaves a factor two for the double arithmetic
// here, and a square that underflows loses less than 2^-126.
LLSR_HD double reach2(float r2) { return (double)r2 * (1.0 + kSlack) + 7.5231638452626401e-37; /* 2^-120 */ }

// The distance from p to the coordinates of tile t, from below (0 when p may lie inside)
LLSR_HD double tile_gap(double p, double t, double tile) {
  double lo, hi;
  tile_span(t, tile, &lo, &hi);
  const double a = lo - p, b = p - hi;
  const double g = a > b ? a : b;
  return g > 0.0 ? g * (1.0 - kSlack) : 0.0;  // (fl(c - p) may fall short of c - p by 2^-24)
}

// Row r of `bx` (iy fastest): the relative x tile range a passing point can lie in; false: none.
LLSR_HD bool row_x_range(const Grid& g, const Box& bx, int32_t r, const float* pos, float r2, float tile,
                         int32_t* iy, int32_t* iz, int32_t* x0, int32_t* x1) {
  *iy = bx.y0 + r % bx.ny;
  *iz = bx.z0 + r / bx.ny;
  const double t = (double)tile;
  const double gy = tile_gap((double)pos[1], (double)g.oy + (double)*iy, t);
  const double gz = tile_gap((double)pos[2], (double)g.oz + (double)*iz, t);
  const double rem = (reach2(r2) - gy * gy) - gz * gz;
  if (rem < 0.0) return false;
  const double hw = sqrt(rem) * (1.0 + kSlack);
  clamp_axis(tile_lo((double)pos[0] - hw, t), tile_hi((double)pos[0] + hw, t), g.ox, g.nx, x0, x1);
  return *x1 >= *x0;
}

// Points [*s, *e) of the stored cloud: row r's x range (empty when the row can hold no passing point)
LLSR_HD void row_points(const Grid& g, const uint32_t* tile_start, const Box& bx, int32_t r, const float* pos, float r2,
                        float tile, uint32_t* s, uint32_t* e) {
  int32_t iy, iz, x0, x1;
  if (!row_x_range(g, bx, r, pos, r2, tile, &iy, &iz, &x0, &x1)) {
    *s = *e = 0;
    return;
  }
  const int64_t key = ((int64_t)iz * g.ny + iy) * g.nx;
  *s = tile_start[key + x0];
  *e = tile_start[key + x1 + 1];
}

// Part w of kWaves of the row [s, e): whole chunks of 64 points, in order
LLSR_HD void row_part(uint32_t s, uint32_t e, int w, uint32_t* ps, uint32_t* pe) {
  const uint64_t len = e - s;
  const uint64_t per = (((len + kWaves - 1) / kWaves) + 63) & ~(uint64_t)63;
  const uint64_t a = (uint64_t)w * per, b = a + per;
  *ps = s + (uint32_t)(a < len ? a : len);
  *pe = s + (uint32_t)(b < len ? b : len);
}

// ---- host only ------------------------------------------------------------------------------------
inline float r_squared(float r) { return (float)((double)r * (double)r); }
inline bool positive_finite(float v) { return v > 0.0f && v <= 3.4028234663852886e+38f; }

// The (y, z) box for one position: every tile a passing point can lie in (the rows then narrow x).
inline Box make_box(const Kind& k, const float* pos, float r2, float tile) {
  Box b{0, 0, 0, 0};
  if (k.size() == 0) return b;
  for (int a = 0; a < 3; ++a)
    if (!(fabsf(pos[a]) <= 3.4028234663852886e+38f)) return b;  // NaN / inf: the predicate passes nothing
  const double t = (double)tile, R = sqrt(reach2(r2)) * (1.0 + kSlack);
  int32_t y0, y1, z0, z1;
  clamp_axis(tile_lo((double)pos[1] - R, t), tile_hi((double)pos[1] + R, t), k.o[1], k.n[1], &y0, &y1);
  clamp_axis(tile_lo((double)pos[2] - R, t), tile_hi((double)pos[2] + R, t), k.o[2], k.n[2], &z0, &z1);
  if (y1 < y0 || z1 < z0) return b;
  b.y0 = y0; b.ny = y1 - y0 + 1; b.z0 = z0; b.nz = z1 - z0 + 1;
  return b;
}
inline Grid grid_of(const Kind& k) { return Grid{k.o[0], k.o[1], k.o[2], k.n[0], k.n[1], k.n[2]}; }

// Build one kind's index from n float4 points. LLSR_EINVAL (-22): a non-finite coordinate;
// LLSR_ERANGE (-34): too many points or tiles, the text naming a tile size that fits.
inline int32_t build_kind(const float* in, int64_t n, float tile, Kind* out, std::string* err) {
  Kind k;
  if (n < 0 || (n > 0 && !in)) { *err = "prior load: bad arguments"; return -22; }
  if (n > kMaxPoints) { *err = "prior load: more than 2^31 - 2 points of one kind"; return -34; }
  if (n == 0) {
    k.tile_start.assign(1, 0u);
    *out = std::move(k);
    return 0;
  }
  float lo[3], hi[3], clo[3], chi[3];
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const float c = in[4 * i + a];
      if (!(fabsf(c) <= 3.4028234663852886e+38f)) {
        char msg[96];
        snprintf(msg, sizeof msg, "prior load: point %lld has a non-finite coordinate", (long long)i);
        *err = msg;
        return -22;
      }
      const float t = floorf(c / tile);
      if (i == 0 || t < lo[a]) lo[a] = t;
      if (i == 0 || t > hi[a]) hi[a] = t;
      if (i == 0 || c < clo[a]) clo[a] = c;
      if (i == 0 || c > chi[a]) chi[a] = c;
    }
  double tiles = 1.0;
  bool far = false;
  for (int a = 0; a < 3; ++a) {
    tiles *= (double)hi[a] - (double)lo[a] + 1.0;
    far |= !(fabsf(lo[a]) <= (float)kMaxTileIndex) || !(fabsf(hi[a]) <= (float)kMaxTileIndex);
  }
  if (far || tiles > (double)kMaxTiles) {
    // the smallest tile * 2^j under which the extent needs at most kMaxTiles tiles and no index
    // leaves +-2^30 (two spare tiles per axis for where the grid falls)
    double fit = (double)tile;
    for (int j = 0; j < 400; ++j, fit *= 2.0) {
      double need = 1.0, idx = 0.0;
      for (int a = 0; a < 3; ++a) {
        need *= floor(((double)chi[a] - (double)clo[a]) / fit) + 2.0;
        idx = fmax(idx, fmax(fabs((double)clo[a]), fabs((double)chi[a])) / fit + 1.0);
      }
      if (need <= (double)kMaxTiles && idx <= (double)kMaxTileIndex) break;
    }
    char msg[200];
    if (far)
      snprintf(msg, sizeof msg, "prior load: coordinates lie beyond 2^30 tiles of %g from zero; a tile of %g fits",
               (double)tile, fit);
    else
      snprintf(msg, sizeof msg, "prior load: %.0f tiles of %g for one kind, more than 2^24; a tile of %g fits", tiles,
               (double)tile, fit);
    *err = msg;
    return -34;
  }
  for (int a = 0; a < 3; ++a) {
    k.o[a] = (int32_t)lo[a];
    k.n[a] = (int32_t)hi[a] - (int32_t)lo[a] + 1;
  }
  const int64_t nt = k.tiles();
  // stable counting sort by key
  std::vector<uint32_t> key((size_t)n);
  k.tile_start.assign((size_t)nt + 1, 0u);
  for (int64_t i = 0; i < n; ++i) {
    int32_t t[3];
    for (int a = 0; a < 3; ++a) t[a] = (int32_t)floorf(in[4 * i + a] / tile) - k.o[a];
    key[(size_t)i] = (uint32_t)(((int64_t)t[2] * k.n[1] + t[1]) * k.n[0] + t[0]);
    k.tile_start[(size_t)key[(size_t)i] + 1] += 1;
  }
  for (int64_t t = 0; t < nt; ++t) {
    k.used += k.tile_start[(size_t)t + 1] != 0;
    k.tile_start[(size_t)t + 1] += k.tile_start[(size_t)t];
  }
  std::vector<uint32_t> at(k.tile_start.begin(), k.tile_start.end() - 1);
  k.pts.resize((size_t)n * 4);
  for (int64_t i = 0; i < n; ++i) memcpy(&k.pts[4 * (size_t)at[key[(size_t)i]]++], in + 4 * i, 16);
  *out = std::move(k);
  return 0;
}

// Segment q of a crop over P positions: kind q / P at position q % P, so that the packed output is
// all corner crops, then all surf crops.
// The serial crop: sizes into off_c / off_s ([P + 1] each, in points into out), then — when out is
// given and cap holds them — the points. Returns 0, or -34 with the sizes set and nothing written.
// `tested` (may be NULL) receives the points the predicate ran on.
inline int32_t crop_host(const Kind* kinds, float radius, float tile, const float* pos, int32_t P, float* out,
                         int64_t cap, int64_t* off_c, int64_t* off_s, int64_t* tested) {
  const float r2 = r_squared(radius);
  std::vector<Box> box((size_t)2 * P);
  std::vector<int64_t> tot((size_t)2 * P, 0);
  int64_t seen = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int q = 0; q < 2 * P; ++q) {
      const Kind& k = kinds[q / P];
      const Grid g = grid_of(k);
      const float* p = pos + 3 * (q % P);
      if (pass == 0) box[(size_t)q] = make_box(k, p, r2, tile);
      const Box& bx = box[(size_t)q];
      int64_t at = pass ? (q < P ? off_c[q] : off_s[q - P]) : 0;
      for (int32_t r = 0; r < bx.ny * bx.nz; ++r) {
        uint32_t s, e;
        row_points(g, k.tile_start.data(), bx, r, p, r2, tile, &s, &e);
        for (int w = 0; w < kWaves; ++w) {  // (the device's partition; any partition gives this order)
          uint32_t ps, pe;
          row_part(s, e, w, &ps, &pe);
          for (uint32_t i = ps; i < pe; ++i) {
            const float* c = &k.pts[4 * (size_t)i];
            if (!in_sphere(c[0], c[1], c[2], p[0], p[1], p[2], r2)) continue;
            if (pass) memcpy(out + 4 * at, c, 16);
            ++at;
          }
          if (!pass) seen += pe - ps;
        }
      }
      if (!pass) tot[(size_t)q] = at;
    }
    if (pass) break;
    off_c[0] = 0;
    for (int p = 0; p < P; ++p) off_c[p + 1] = off_c[p] + tot[(size_t)p];
    off_s[0] = off_c[P];
    for (int p = 0; p < P; ++p) off_s[p + 1] = off_s[p] + tot[(size_t)P + p];
    if (tested) *tested = seen;
    if (!out && cap == 0) return 0;
    if (off_s[P] > cap) return -34;
  }
  return 0;
}

}  // namespace llsr_prior_ns
