// llsr_prior.hip — the prior map's C API, its device copy and the crop kernels (bodies in
// llsr_prior.h). The index is built on the host once per load and copied; a crop is three launches:
//   k_prior_count  grid (row, segment): one block per row of tiles of a segment's (y, z) box, the
//                  row's point range read from the device CSR, split into kWaves parts of whole
//                  64-point chunks; each wave counts its part with one ballot per 64 points, kLoads
//                  float4 loads in flight per lane, and stores its total;
//   k_prior_scan   one block per segment: the exclusive scan of its rows' wave totals, in place, and
//                  the segment's total;
//   k_prior_write  the counting kernel's walk again, each passing point stored at the segment's base
//                  + its wave's scanned offset + the points the wave kept so far + its mbcnt rank.
// Between the scan and the writer the host reads the 2 P totals, forms the offsets and checks the
// capacity. A segment is (kind, position): kind * P + position, so the packed output is the P corner
// crops, then the P surf crops. The loads of a row form the chain box -> tile_start -> points, the
// first two uniform per block; a wave's point addresses depend on nothing it loaded before them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/llsr.h"
#include "llsr_prior.h"
#include "llsr_prior_internal.h"

namespace llsr_prior_ns {

struct KindDev {
  const float4* pts;
  const uint32_t* tile_start;
  Grid g;
};
struct CropArgs {
  KindDev k[2];
  const Box* box;           // [2 P]
  const float* pos;         // [P][3]
  const int64_t* rowbase;   // [2 P + 1]: rows of the segments before
  uint32_t* cnt;            // [rows][kWaves]: wave totals, then their exclusive scan per segment
  int64_t* tot;             // [2 P]
  const int64_t* base;      // [2 P]: the segments' offsets into out
  float4* out;
  float r2, tile;
  int32_t P;
};

// The part of its row this wave walks; false: the block has no row
__device__ __forceinline__ bool wave_part(const CropArgs& a, int seg, int r, int wave, const float4** pts, float* p,
                                          uint32_t* ps, uint32_t* pe) {
  const Box bx = a.box[seg];
  if (r >= bx.ny * bx.nz) return false;
  const KindDev& k = a.k[seg >= a.P];
  const float* q = a.pos + 3 * (seg >= a.P ? seg - a.P : seg);
  p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
  uint32_t s, e;
  row_points(k.g, k.tile_start, bx, r, p, a.r2, a.tile, &s, &e);
  row_part(s, e, wave, ps, pe);
  *pts = k.pts;
  return true;
}

// One step of a wave: kLoads chunks of 64 points from i on, all loads issued before the first test;
// in[u] = lane's point of chunk u passes.
__device__ __forceinline__ void wave_step(const float4* pts, uint32_t i, uint32_t pe, int lane, const float* p, float r2,
                                          float4* q, bool* in) {
#pragma unroll
  for (int u = 0; u < kLoads; ++u) {
    const uint64_t j = (uint64_t)i + (uint32_t)(u * 64 + lane);
    q[u] = j < pe ? pts[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    in[u] = j < pe;
  }
#pragma unroll
  for (int u = 0; u < kLoads; ++u) in[u] = in[u] && in_sphere(q[u].x, q[u].y, q[u].z, p[0], p[1], p[2], r2);
}

__global__ __launch_bounds__(64 * kWaves) void k_prior_count(CropArgs a) {
  const int seg = blockIdx.y, r = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float4* pts;
  float p[3];
  uint32_t ps, pe;
  if (!wave_part(a, seg, r, wave, &pts, p, &ps, &pe)) return;
  uint32_t c = 0;
  for (uint64_t i = ps; i < pe; i += kChunk) {
    float4 q[kLoads];
    bool in[kLoads];
    wave_step(pts, (uint32_t)i, pe, lane, p, a.r2, q, in);
#pragma unroll
    for (int u = 0; u < kLoads; ++u) c += (uint32_t)__popcll(__ballot(in[u]));
  }
  if (lane == 0) a.cnt[(a.rowbase[seg] + r) * kWaves + wave] = c;
}

__global__ __launch_bounds__(64 * kWaves) void k_prior_scan(CropArgs a) {
  const int seg = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const Box bx = a.box[seg];
  const int64_t n = (int64_t)bx.ny * bx.nz * kWaves;
  uint32_t* c = a.cnt + a.rowbase[seg] * kWaves;
  __shared__ uint32_t wsum[kWaves];
  uint32_t carry = 0;
  for (int64_t base = 0; base < n; base += 64 * kWaves) {
    const int64_t i = base + tid;
    const uint32_t v = i < n ? c[i] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      before += w < wave ? wsum[w] : 0u;
      all += wsum[w];
    }
    if (i < n) c[i] = carry + before + (x - v);
    carry += all;
    __syncthreads();
  }
  if (tid == 0) a.tot[seg] = (int64_t)carry;
}

__global__ __launch_bounds__(64 * kWaves) void k_prior_write(CropArgs a) {
  const int seg = blockIdx.y, r = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float4* pts;
  float p[3];
  uint32_t ps, pe;
  if (!wave_part(a, seg, r, wave, &pts, p, &ps, &pe)) return;
  if (ps >= pe) return;
  float4* out = a.out + a.base[seg] + a.cnt[(a.rowbase[seg] + r) * kWaves + wave];
  uint32_t kept = 0;
  for (uint64_t i = ps; i < pe; i += kChunk) {
    float4 q[kLoads];
    bool in[kLoads];
    wave_step(pts, (uint32_t)i, pe, lane, p, a.r2, q, in);
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const unsigned long long m = __ballot(in[u]);
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (in[u]) out[kept + rank] = q[u];
      kept += (uint32_t)__popcll(m);
    }
  }
}

}  // namespace llsr_prior_ns

using namespace llsr_prior_ns;

struct llsr_prior {
  int device = LLSR_PRIOR_HOST;
  llsr_prior_config cfg{};
  std::string err;
  Kind kind[2];
  // the device copy of the index
  float4* d_pts[2] = {nullptr, nullptr};
  uint32_t* d_ts[2] = {nullptr, nullptr};
  // the crop's workspace: per segment box / rowbase / tot / base and the positions (device, and one
  // pinned block of the same layout), the rows' wave totals
  int capP = 0;
  char* d_small = nullptr;
  char* h_small = nullptr;
  uint32_t* d_cnt = nullptr;
  int64_t cap_rows = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // the crop begun by crop_begin, finished by crop_write
  int P = 0;
  int64_t rows = 0, max_rows = 0, total = 0;
  std::vector<float> pos;
  float last_ms = 0.f;
  int64_t last_written = 0, last_tested_host = 0;
};

// The small arrays' layout for P positions (each piece 16-byte aligned)
struct Small {
  size_t box, pos, rowbase, tot, base, bytes;
  explicit Small(int P) {
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    box = 0;
    pos = up(box + sizeof(Box) * 2 * (size_t)P);
    rowbase = up(pos + sizeof(float) * 3 * (size_t)P);
    tot = up(rowbase + sizeof(int64_t) * (2 * (size_t)P + 1));
    base = up(tot + sizeof(int64_t) * 2 * (size_t)P);
    bytes = up(base + sizeof(int64_t) * 2 * (size_t)P);
  }
};

static int32_t prfail(llsr_prior* w, int32_t code, const std::string& msg) {
  if (w) w->err = msg;
  return code;
}
#define PR_OK(w, expr)                                                            \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess)                                                         \
      return prfail(w, LLSR_EIO, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

extern "C" int32_t llsr_prior_config_default(llsr_prior_config* cfg) {
  if (!cfg) return LLSR_EINVAL;
  cfg->radius = 50.0f;  // surrounding_keyframe_search_radius (CFG:26)
  cfg->tile = 10.0f;
  return LLSR_OK;
}

extern "C" void llsr_prior_destroy(llsr_prior* w) {
  if (!w) return;
  if (w->device != LLSR_PRIOR_HOST) {
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    for (int k = 0; k < 2; ++k) {
      if (w->d_pts[k]) (void)hipFree(w->d_pts[k]);
      if (w->d_ts[k]) (void)hipFree(w->d_ts[k]);
    }
    if (w->d_small) (void)hipFree(w->d_small);
    if (w->h_small) (void)hipHostFree(w->h_small);
    if (w->d_cnt) (void)hipFree(w->d_cnt);
    for (hipEvent_t e : w->ev)
      if (e) (void)hipEventDestroy(e);
    if (w->stream) (void)hipStreamDestroy(w->stream);
  }
  delete w;
}

extern "C" llsr_prior* llsr_prior_create(const llsr_prior_config* cfg, int32_t dev) {
  llsr_prior_config c;
  llsr_prior_config_default(&c);
  if (cfg) c = *cfg;
  if (!positive_finite(c.radius) || !positive_finite(c.tile)) return nullptr;
  if (dev != LLSR_PRIOR_HOST) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || dev < 0 || dev >= count) return nullptr;
    if (hipSetDevice(dev) != hipSuccess) return nullptr;
  }
  llsr_prior* w = new (std::nothrow) llsr_prior;
  if (!w) return nullptr;
  w->device = dev;
  w->cfg = c;
  w->kind[0].tile_start.assign(1, 0u);
  w->kind[1].tile_start.assign(1, 0u);
  if (dev != LLSR_PRIOR_HOST) {
    bool ok = hipStreamCreate(&w->stream) == hipSuccess;
    for (hipEvent_t& e : w->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok) {
      llsr_prior_destroy(w);
      return nullptr;
    }
  }
  return w;
}

extern "C" const char* llsr_prior_last_error(const llsr_prior* w) { return w ? w->err.c_str() : "null prior map"; }

extern "C" int32_t llsr_prior_load(llsr_prior* w, const float* corner, int64_t n_corner, const float* surf,
                                   int64_t n_surf, void* hip_stream) {
  if (!w) return LLSR_EINVAL;
  Kind k[2];
  const float* src[2] = {corner, surf};
  const int64_t n[2] = {n_corner, n_surf};
  try {
    for (int a = 0; a < 2; ++a) {
      std::string msg;
      const int32_t rc = build_kind(src[a], n[a], w->cfg.tile, &k[a], &msg);
      if (rc != LLSR_OK) return prfail(w, rc, (a ? "surf: " : "corner: ") + msg);
    }
  } catch (const std::bad_alloc&) {
    return prfail(w, LLSR_ENOMEM, "prior load: no host memory for the index");
  }
  if (w->device != LLSR_PRIOR_HOST) {
    PR_OK(w, hipSetDevice(w->device));
    const hipStream_t s = hip_stream ? (hipStream_t)hip_stream : w->stream;
    float4* dp[2] = {nullptr, nullptr};
    uint32_t* dt[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int a = 0; a < 2 && e == hipSuccess; ++a) {
      const size_t pb = std::max<size_t>(k[a].pts.size() * sizeof(float), 16), tb = k[a].tile_start.size() * sizeof(uint32_t);
      e = hipMalloc(&dp[a], pb);
      if (e == hipSuccess) e = hipMalloc(&dt[a], tb);
      if (e == hipSuccess && !k[a].pts.empty())
        e = hipMemcpyAsync(dp[a], k[a].pts.data(), k[a].pts.size() * sizeof(float), hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(dt[a], k[a].tile_start.data(), tb, hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipStreamSynchronize(w->stream);  // a crop of the old index still running
    if (e != hipSuccess) {
      for (int a = 0; a < 2; ++a) {
        if (dp[a]) (void)hipFree(dp[a]);
        if (dt[a]) (void)hipFree(dt[a]);
      }
      return prfail(w, e == hipErrorOutOfMemory ? LLSR_ENOMEM : LLSR_EIO,
                    std::string("prior load: ") + hipGetErrorString(e));
    }
    for (int a = 0; a < 2; ++a) {
      if (w->d_pts[a]) (void)hipFree(w->d_pts[a]);
      if (w->d_ts[a]) (void)hipFree(w->d_ts[a]);
      w->d_pts[a] = dp[a];
      w->d_ts[a] = dt[a];
    }
  }
  w->kind[0] = std::move(k[0]);
  w->kind[1] = std::move(k[1]);
  w->P = 0;
  return LLSR_OK;
}

extern "C" int32_t llsr_prior_info(const llsr_prior* w, llsr_prior_report* out) {
  if (!w || !out) return LLSR_EINVAL;
  std::memset(out, 0, sizeof *out);
  for (int a = 0; a < 2; ++a) {
    const Kind& k = w->kind[a];
    out->n_points[a] = k.size();
    out->n_tiles[a] = k.tiles();
    out->n_tiles_used[a] = k.used;
    for (int j = 0; j < 3; ++j) {
      out->dims[a][j] = k.n[j];
      out->origin[a][j] = k.o[j];
    }
  }
  out->radius = w->cfg.radius;
  out->tile = w->cfg.tile;
  out->device = w->device;
  return LLSR_OK;
}

extern "C" int64_t llsr_prior_points(const llsr_prior* w, int32_t kind, float* out, int64_t cap) {
  if (!w || kind < 0 || kind > 1 || cap < 0 || (cap > 0 && !out)) return LLSR_EINVAL;
  const Kind& k = w->kind[kind];
  const int64_t n = k.size();
  if (cap > 0 && n > 0) std::memcpy(out, k.pts.data(), sizeof(float) * 4 * (size_t)std::min(n, cap));
  return n;
}

extern "C" int64_t llsr_prior_tile_starts(const llsr_prior* w, int32_t kind, uint32_t* out, int64_t cap) {
  if (!w || kind < 0 || kind > 1 || cap < 0 || (cap > 0 && !out)) return LLSR_EINVAL;
  const Kind& k = w->kind[kind];
  const int64_t n = (int64_t)k.tile_start.size();
  if (cap > 0) std::memcpy(out, k.tile_start.data(), sizeof(uint32_t) * (size_t)std::min(n, cap));
  return n;
}

static CropArgs crop_args(llsr_prior* w, const Small& z) {
  CropArgs a{};
  for (int k = 0; k < 2; ++k) {
    a.k[k].pts = w->d_pts[k];
    a.k[k].tile_start = w->d_ts[k];
    a.k[k].g = grid_of(w->kind[k]);
  }
  a.box = (const Box*)(w->d_small + z.box);
  a.pos = (const float*)(w->d_small + z.pos);
  a.rowbase = (const int64_t*)(w->d_small + z.rowbase);
  a.tot = (int64_t*)(w->d_small + z.tot);
  a.base = (const int64_t*)(w->d_small + z.base);
  a.cnt = w->d_cnt;
  a.r2 = r_squared(w->cfg.radius);
  a.tile = w->cfg.tile;
  a.P = w->P;
  return a;
}

int32_t llsr_prior_ns::crop_begin(llsr_prior* w, const float* pos, int32_t P, int64_t* off_c, int64_t* off_s,
                                  void* hip_stream) {
  if (!w || !pos || !off_c || !off_s) return prfail(w, LLSR_EINVAL, "prior crop: bad arguments");
  if (P < 1 || P > 32767) return prfail(w, LLSR_ERANGE, "prior crop: P outside [1, 32767]");
  if (w->device == LLSR_PRIOR_HOST) return prfail(w, LLSR_EINVAL, "prior crop: a host object");
  w->P = 0;
  PR_OK(w, hipSetDevice(w->device));
  const hipStream_t s = hip_stream ? (hipStream_t)hip_stream : w->stream;
  if (P > w->capP) {
    int n = w->capP ? w->capP : 64;
    while (n < P) n *= 2;
    n = std::min(n, 32767);
    PR_OK(w, hipStreamSynchronize(w->stream));
    if (w->d_small) (void)hipFree(w->d_small);
    if (w->h_small) (void)hipHostFree(w->h_small);
    w->d_small = w->h_small = nullptr;
    w->capP = 0;
    const Small zc(n);
    PR_OK(w, hipMalloc((void**)&w->d_small, zc.bytes));
    PR_OK(w, hipHostMalloc((void**)&w->h_small, zc.bytes));
    w->capP = n;
  }
  const Small z(P);
  Box* box = (Box*)(w->h_small + z.box);
  int64_t* rowbase = (int64_t*)(w->h_small + z.rowbase);
  const float r2 = r_squared(w->cfg.radius);
  std::memcpy(w->h_small + z.pos, pos, sizeof(float) * 3 * (size_t)P);
  rowbase[0] = 0;
  int64_t max_rows = 0;
  for (int q = 0; q < 2 * P; ++q) {
    box[q] = make_box(w->kind[q / P], pos + 3 * (q % P), r2, w->cfg.tile);
    const int64_t rows = (int64_t)box[q].ny * box[q].nz;
    rowbase[q + 1] = rowbase[q] + rows;
    max_rows = std::max(max_rows, rows);
  }
  const int64_t rows = rowbase[2 * P];
  if (rows > w->cap_rows) {
    int64_t n = w->cap_rows ? w->cap_rows : (int64_t)1 << 14;
    while (n < rows) n *= 2;
    PR_OK(w, hipStreamSynchronize(w->stream));
    if (w->d_cnt) (void)hipFree(w->d_cnt);
    w->d_cnt = nullptr;
    w->cap_rows = 0;
    if (hipMalloc((void**)&w->d_cnt, sizeof(uint32_t) * kWaves * (size_t)n) != hipSuccess)
      return prfail(w, LLSR_ENOMEM, "prior crop: no device memory for the rows' counts");
    w->cap_rows = n;
  }
  w->pos.assign(pos, pos + 3 * (size_t)P);
  w->P = P;
  w->rows = rows;
  w->max_rows = max_rows;
  int64_t* tot = (int64_t*)(w->h_small + z.tot);
  std::memset(tot, 0, sizeof(int64_t) * 2 * (size_t)P);
  PR_OK(w, hipEventRecord(w->ev[0], s));
  if (max_rows > 0) {
    // box, pos, rowbase: one copy (tot and base follow them in the layout)
    PR_OK(w, hipMemcpyAsync(w->d_small, w->h_small, z.tot, hipMemcpyHostToDevice, s));
    const CropArgs a = crop_args(w, z);
    k_prior_count<<<dim3((unsigned)max_rows, 2 * P), 64 * kWaves, 0, s>>>(a);
    k_prior_scan<<<2 * P, 64 * kWaves, 0, s>>>(a);
    PR_OK(w, hipGetLastError());
    PR_OK(w, hipMemcpyAsync(tot, w->d_small + z.tot, sizeof(int64_t) * 2 * (size_t)P, hipMemcpyDeviceToHost, s));
  }
  PR_OK(w, hipEventRecord(w->ev[1], s));
  PR_OK(w, hipStreamSynchronize(s));
  int64_t* base = (int64_t*)(w->h_small + z.base);
  off_c[0] = 0;
  for (int p = 0; p < P; ++p) {
    base[p] = off_c[p];
    off_c[p + 1] = off_c[p] + tot[p];
  }
  off_s[0] = off_c[P];
  for (int p = 0; p < P; ++p) {
    base[P + p] = off_s[p];
    off_s[p + 1] = off_s[p] + tot[P + p];
  }
  w->total = off_s[P];
  w->last_written = 0;
  w->last_tested_host = -1;
  PR_OK(w, hipEventElapsedTime(&w->last_ms, w->ev[0], w->ev[1]));
  return LLSR_OK;
}

int32_t llsr_prior_ns::crop_write(llsr_prior* w, float* out, int64_t cap, void* hip_stream) {
  if (!w || w->P < 1) return prfail(w, LLSR_EINVAL, "prior crop: no crop begun");
  if (w->total > cap) return prfail(w, LLSR_ERANGE, "prior crop: the output holds fewer points than the crops");
  if (w->total > 0 && (!out || ((uintptr_t)out & 15))) return prfail(w, LLSR_EINVAL, "prior crop: out is NULL or misaligned");
  PR_OK(w, hipSetDevice(w->device));
  const hipStream_t s = hip_stream ? (hipStream_t)hip_stream : w->stream;
  if (w->total > 0) {
    const Small z(w->P);
    CropArgs a = crop_args(w, z);
    a.out = (float4*)out;
    PR_OK(w, hipEventRecord(w->ev[2], s));
    PR_OK(w, hipMemcpyAsync(w->d_small + z.base, w->h_small + z.base, sizeof(int64_t) * 2 * (size_t)w->P,
                            hipMemcpyHostToDevice, s));
    k_prior_write<<<dim3((unsigned)w->max_rows, 2 * w->P), 64 * kWaves, 0, s>>>(a);
    PR_OK(w, hipGetLastError());
    PR_OK(w, hipEventRecord(w->ev[3], s));
    PR_OK(w, hipStreamSynchronize(s));
    float ms = 0.f;
    PR_OK(w, hipEventElapsedTime(&ms, w->ev[2], w->ev[3]));
    w->last_ms += ms;
  }
  w->last_written = w->total;
  return LLSR_OK;
}

extern "C" int32_t llsr_prior_crop_batch(llsr_prior* w, const float* pos, int32_t P, float* out, int64_t cap,
                                         int64_t* off_c, int64_t* off_s, void* hip_stream) {
  if (!w || !pos || !off_c || !off_s || cap < 0 || (!out && cap != 0))
    return prfail(w, LLSR_EINVAL, "prior crop: bad arguments");
  if (P < 1 || P > 32767) return prfail(w, LLSR_ERANGE, "prior crop: P outside [1, 32767]");
  if (w->device == LLSR_PRIOR_HOST) {
    const auto t0 = std::chrono::steady_clock::now();
    int32_t rc;
    try {
      rc = crop_host(w->kind, w->cfg.radius, w->cfg.tile, pos, P, out, cap, off_c, off_s, &w->last_tested_host);
    } catch (const std::bad_alloc&) {
      return prfail(w, LLSR_ENOMEM, "prior crop: no host memory");
    }
    w->last_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    w->last_written = (rc == LLSR_OK && out) ? off_s[P] : 0;
    w->pos.assign(pos, pos + 3 * (size_t)P);
    w->P = P;
    return rc == LLSR_OK ? rc : prfail(w, rc, "prior crop: the output holds fewer points than the crops");
  }
  int32_t rc = crop_begin(w, pos, P, off_c, off_s, hip_stream);
  if (rc != LLSR_OK) return rc;
  if (!out && cap == 0) return LLSR_OK;
  return crop_write(w, out, cap, hip_stream);
}

extern "C" int32_t llsr_prior_last_crop(const llsr_prior* w, float* ms, int64_t* tested, int64_t* written) {
  if (!w) return LLSR_EINVAL;
  if (ms) *ms = w->last_ms;
  if (written) *written = w->last_written;
  if (tested) {  // the rows' lengths, from the host's copy of the index
    int64_t n = 0;
    if (w->device == LLSR_PRIOR_HOST && w->last_tested_host >= 0) {
      n = w->last_tested_host;
    } else {
      const float r2 = r_squared(w->cfg.radius);
      for (int q = 0; q < 2 * w->P; ++q) {
        const Kind& k = w->kind[q / w->P];
        const float* p = w->pos.data() + 3 * (size_t)(q % w->P);
        const Box bx = make_box(k, p, r2, w->cfg.tile);
        const Grid g = grid_of(k);
        for (int32_t r = 0; r < bx.ny * bx.nz; ++r) {
          uint32_t s, e;
          row_points(g, k.tile_start.data(), bx, r, p, r2, w->cfg.tile, &s, &e);
          n += e - s;
        }
      }
    }
    *tested = n;
  }
  return LLSR_OK;
}

int llsr_prior_ns::device_of(const llsr_prior* w) { return w ? w->device : LLSR_PRIOR_HOST; }
const char* llsr_prior_ns::error_of(const llsr_prior* w) { return llsr_prior_last_error(w); }
