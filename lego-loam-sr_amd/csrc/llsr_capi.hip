// llsr_capi.hip — host side of the C-ABI (include/llsr.h): handle lifetime, the HBM buffer
// pool, the per-batch launch sequence and result fetch. No C++ exception crosses the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "llsr_handle.h"
#include "llsr_isort.h"
#include "llsr_libm.h"

namespace llsr {
template <bool kRanked> __global__ void k_project(DevCfg, const float4*, const int64_t*, DevBufs, const uint32_t*);
__global__ void k_row_bins(DevCfg, const float4*, const int64_t*, uint32_t*);
__global__ void k_gather_column(DevCfg, const float4*, const int64_t*, DevBufs);
__global__ void k_project_fused(DevCfg, const float4*, const int64_t*, DevBufs);
__global__ void k_ground_add(DevCfg, DevBufs);
__global__ void k_ground_elev_ransac(DevCfg, DevBufs);
template <bool kLds> __global__ void k_label(DevCfg, DevBufs);
__global__ void k_segment(DevCfg, const float4*, const int64_t*, DevBufs);
void launch_fa_points(const DevCfg&, const DevBufs&, int, hipStream_t);
void launch_fa_points_imu(const DevCfg&, const DevBufs&, const ImuDev&, int, hipStream_t);
__global__ void k_select_ring(DevCfg, DevBufs);
__global__ void k_vox_top(DevCfg, DevBufs, VoxRanges);
__global__ void k_vox_leaf(DevCfg, DevBufs, VoxRanges);
__global__ void k_vox_sum(DevCfg, DevBufs);
__global__ void k_debug_exact_sort(const float*, int, int*);
__global__ void k_debug_vox_keys(const float4*, int, int, uint32_t*, int*);
__global__ void k_debug_half_passed(const float*, int, uint8_t*);
__global__ void k_fa_concat(DevCfg, DevBufs);
__global__ void k_dbscan_adj(DevCfg, DevBufs, const float4* __restrict__);
__global__ void k_vis_clouds(DevCfg, DevBufs, int, float4*, int*);
template <int kDbL> __global__ void k_dbscan_merge(DevCfg, DevBufs);

__global__ void k_init_counts(int* counts, int B, int* vox_count) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < kVoxSub) vox_count[b * kVoxCntStride] = 0;  // (the grid has at least 256 threads)
  if (b >= B) return;
  int* c = counts + b * kCnt;
  for (int k = 0; k < kCnt; ++k) c[k] = 0;
  c[C_FIRST] = INT_MAX;
  c[C_LAST] = -1;
}
}  // namespace llsr

using namespace llsr;

namespace {
const char* kKernelNames[] = {"init",          "k_project",    "k_gather_column", "k_ground_add",
                              "k_ground_elev_ransac", "k_label", "k_segment",      "k_fa_points",
                              "k_select_ring", "k_vox_pcl", "k_fa_concat", "k_dbscan_adj", "k_dbscan_merge",
                              "k_row_bins"};
static_assert(sizeof kKernelNames / sizeof *kKernelNames == kNumKernels, "one name per timed kernel");
}  // namespace

// use_vlp32c: one more than the largest elevation bin a point can fall into (IP:356 with asinf's
// largest value, float pi / 2), in the reference's arithmetic; NaN-safe (a bad angle gives INT_MIN)
static int row_bin_bound(const DevCfg& c) {
  const int top = trunc_i32((double)(1.57079637050628662109375f + c.ip_angBottom) / (0.335 * (M_PI / 180.0)));
  return top < 0 ? top : top + 1;
}

// The fused projection keeps the winning raw index per cell in LDS (k_project_fused).
static int fused_lds(const DevCfg& c) { return c.HW * (int)sizeof(int); }
// k_label<true>'s dynamic LDS: the parent word of every cell, the right-edge row mask of every
// column (16 bits, an even count of them) and a queue of 128 cells for each of the 16 waves
// (HW <= 32000, W <= 2048: <= 136192 B)
static int label_lds(const DevCfg& c) {
  return c.HW * (int)sizeof(int) + (((c.W + 1) & ~1) + 16 * 128) * (int)sizeof(unsigned short);
}

static int label_band_lds(const DevCfg& c) { return c.lbl_band * c.W * (int)sizeof(int); }
// (a use_vlp32c handle ranks its rows first: always k_row_bins -> k_project<true> -> k_gather_column)
static bool use_fused(const llsr_handle* h) { return h->dc.ccl_lds != 0 && !h->dc.use_vlp32c; }

// k_segment / k_ground_elev_ransac (any multiple of 64 up to 1024 threads): 512 for range images
// that fit LDS (VLP-16: three / two scans per CU instead of one; r06_v40, 0.289 -> 0.282 and
// 0.180 -> 0.167 ms per 1024 scans), 1024 for the larger ones (HDL-64E: 512 was slower)
static int per_scan_threads(const DevCfg& c) { return c.ccl_lds ? 512 : 1024; }

// the PCL-order less-flat VoxelGrid of every pending ring (the profiling ring's k_vox_pcl slot):
// block-wide partitions, the listed ranges as one pool of one-wave items, the centroids. vr's
// counters are zero before (k_init_counts). `waves`: k_vox_leaf's largest grid (vox_leaf_waves); a
// ring lists ~6 ranges, so small batches launch a smaller one. Diagnostics: dbg_phase 100 stops after k_vox_top, 101 and 102
// after k_vox_leaf.
static void launch_vox_pcl(const DevCfg& c, const DevBufs& d, const VoxRanges& vr, int waves, int B, hipStream_t s) {
  k_vox_top<<<dim3(c.H, B), 256, 0, s>>>(c, d, vr);
  if (c.dbg_phase <= 100) return;
  k_vox_leaf<<<std::min(waves, (8 * c.H * B + kVoxSub - 1) / kVoxSub * kVoxSub), 64, 0, s>>>(c, d, vr);
  if (c.dbg_phase <= 102) return;
  k_vox_sum<<<dim3(c.H, B), 256, 0, s>>>(c, d);
}
// k_vox_leaf's largest grid, a multiple of kVoxSub: 16 times the device's wave slots (32 per CU at
// the kernel's 8 waves per SIMD). The items' costs differ widely; with one wave per slot each
// keeps its fixed share of them and the kernel waits for the unluckiest (0.77 ms per 1024 VLP-16
// scans at 8 times the slots against 1.09 at one; 16 and 32 times are equal within noise), with
// more workgroups than slots the dispatcher hands the next few items to whichever slot is free.
static int vox_leaf_waves(int device) {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
  return std::max(kVoxSub, 16 * 32 * cus / kVoxSub * kVoxSub);
}
static const size_t kVoxCntBytes = sizeof(int) * kVoxSub * kVoxCntStride;

extern "C" int32_t llsr_abi_version(void) { return LLSR_ABI_VERSION; }

extern "C" int32_t llsr_config_default(llsr_config* c, int32_t lidar) {
  if (!c) return LLSR_EINVAL;
  std::memset(c, 0, sizeof *c);
  if (lidar == LLSR_LIDAR_VLP16) {  // loam_config.yaml:1-67
    c->num_vertical_scans = 16; c->num_horizontal_scans = 1800;
    c->vertical_angle_bottom = -15.0f; c->vertical_angle_top = 15.0f;
    c->ground_scan_index = 7; c->use_kitti = 0;
    c->DBFr = 5.0f; c->RatioXY = 0.5f; c->RatioZ = 2.5f;
    c->edge_threshold = 0.03f; c->surf_threshold = 0.03f; c->nearest_feature_search_distance = 5.0f;
  } else if (lidar == LLSR_LIDAR_VLP32C) {  // loam_config.yaml:69-135
    c->num_vertical_scans = 32; c->num_horizontal_scans = 1800;
    c->vertical_angle_bottom = -25.0f; c->vertical_angle_top = 15.0f;
    c->ground_scan_index = 7; c->use_kitti = 0;
    c->DBFr = 5.0f; c->RatioXY = 0.5f; c->RatioZ = 2.5f;
    c->edge_threshold = 0.005f; c->surf_threshold = 0.005f; c->nearest_feature_search_distance = 5.0f;
  } else if (lidar == LLSR_LIDAR_HDL64E) {  // loam_config.yaml:137-203
    c->num_vertical_scans = 64; c->num_horizontal_scans = 1800;
    c->vertical_angle_bottom = -24.8f; c->vertical_angle_top = 2.0f;
    c->ground_scan_index = 50; c->use_kitti = 1;
    c->DBFr = 7.5f; c->RatioXY = 0.3f; c->RatioZ = 5.0f;
    c->edge_threshold = 0.005f; c->surf_threshold = 0.005f; c->nearest_feature_search_distance = 25.0f;
  } else {
    return LLSR_EINVAL;
  }
  c->sensor_mount_angle = 0.0f;
  c->use_vlp32c = lidar == LLSR_LIDAR_VLP32C ? 1 : 0;
  c->segment_theta = 60.0f; c->segment_valid_point_num = 5; c->segment_valid_line_num = 3;
  c->scan_period = 0.1f;
  c->mapping_frequency_divider = 1;
  c->iterCountThres = lidar == LLSR_LIDAR_VLP32C ? 50 : 200;  // CFG:98
  c->step_size = 1.0f; c->stop_thres = 0.05f;
  c->mode = LLSR_MODE_FAITHFUL;
  return LLSR_OK;
}

// Host-side constants with the reference's exact conversions (IP:117-121, 849; FA:152-154).
static void make_devcfg(const llsr_config& c, DevCfg& d) {
  const double kDegToRad = M_PI / 180.0;
  d.H = c.num_vertical_scans;
  d.W = c.num_horizontal_scans;
  d.HW = d.H * d.W;
  d.ip_resX = (float)((M_PI * 2) / d.W);
  d.ip_resY = (float)(kDegToRad * (c.vertical_angle_top - c.vertical_angle_bottom) / float(d.H - 1));
  d.ip_angBottom = (float)(-(c.vertical_angle_bottom - 0.1) * kDegToRad);
  const float segTheta = (float)(c.segment_theta * kDegToRad);
  d.segThr = std::tan(segTheta);
  d.sinX = std::sin(d.ip_resX); d.cosX = std::cos(d.ip_resX);
  d.sinY = std::sin(d.ip_resY); d.cosY = std::cos(d.ip_resY);
  d.use_kitti = c.use_kitti;
  d.gsi = c.ground_scan_index;
  d.pointNum = c.segment_valid_point_num;
  d.lineNum = c.segment_valid_line_num;
  d.scan_period = c.scan_period;
  d.edge_thr = c.edge_threshold;
  d.surf_thr = c.surf_threshold;
  const float fa_resX = (float)((M_PI * 2) / d.W);
  d.fa_resY = (float)(kDegToRad * (c.vertical_angle_top - c.vertical_angle_bottom) / float(d.H - 1));
  d.sinResX = std::sin(fa_resX);
  d.RatioXY = c.RatioXY;
  d.RatioZ = c.RatioZ;
  d.DBFr = c.DBFr;
  d.gnd_cos[0] = llsr_libm::ground_cos_threshold(12.5f);
  d.gnd_cos[1] = llsr_libm::ground_cos_threshold(60.0f);
  d.gnd_cos[2] = llsr_libm::ground_cos_threshold(25.0f);
  d.use_vlp32c = c.use_vlp32c ? 1 : 0;
  d.ccl_lds = (d.H <= 16 && d.HW <= 32000) ? 1 : 0;
  // 72 KB bands: two labelling workgroups per CU (a 512-scan HDL-64E batch runs in one round)
  // (at most 16 rows: a band root's LDS word keeps its members' rows in 16 bits)
  d.lbl_band = std::max(1, std::min(std::min(d.H, 16), 18432 / std::max(1, d.W)));
  d.exact_vg = 1;  // LLSR_VOXEL_ORDER_PCL: the reference's summation order
  d.dbg_phase = 1 << 30;
}

// boost::mt19937 seeded with 12345 (PCL 1.10 SampleConsensusModel's rng_alg_, IP:716-721), state
// after the seeding recurrence and the first twist: every scan's RANSAC starts its draws here, so
// the device loads 624 words instead of running 1248 serial steps on one lane per scan.
static void mt_first_state(uint32_t* m) {
  m[0] = 12345u;
  for (int k = 1; k < 624; ++k) m[k] = 1812433253u * (m[k - 1] ^ (m[k - 1] >> 30)) + (uint32_t)k;
  for (int k = 0; k < 624; ++k) {
    const uint32_t y = (m[k] & 0x80000000u) | (m[(k + 1) % 624] & 0x7fffffffu);
    m[k] = m[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
  }
}

// The configurations the reference's arithmetic defines no result for (include/llsr.h, next to
// llsr_config): host-only, so llsr_create refuses them before it looks for a device.
static bool config_defined(const llsr_config& c) {
  if (c.num_vertical_scans < 2 || c.num_vertical_scans > 64 || c.num_horizontal_scans < 16 ||
      c.num_horizontal_scans > 2048)
    return false;
  const float f[] = {c.vertical_angle_bottom, c.vertical_angle_top, c.sensor_mount_angle, c.segment_theta,
                     c.scan_period, c.edge_threshold, c.surf_threshold, c.nearest_feature_search_distance,
                     c.DBFr, c.RatioXY, c.RatioZ, c.step_size, c.stop_thres};
  for (float v : f)
    if (!std::isfinite(v)) return false;
  if (!(c.vertical_angle_top > c.vertical_angle_bottom)) return false;  // resolution 0: IP:313-316 divides by it
  if (!(c.scan_period > 0.0f)) return false;
  if (!(c.segment_theta > 0.0f && c.segment_theta < 90.0f)) return false;  // tan() of it: IP:849
  return true;
}

extern "C" int32_t llsr_create(const llsr_config* cfg, int32_t hip_device, int32_t max_batch,
                               int32_t max_points, llsr_handle** out) {
  if (!cfg || !out || max_batch < 1 || max_points < 1) return LLSR_EINVAL;
  *out = nullptr;
  if (!config_defined(*cfg)) return LLSR_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= hip_device || hip_device < 0) return LLSR_ENODEV;
  // every error exit below releases what was acquired so far with the handle (its members own it)
  std::unique_ptr<llsr_handle> h(new (std::nothrow) llsr_handle());
  if (!h) return LLSR_ENOMEM;
  h->cfg = *cfg;
  h->device = hip_device;
  h->max_batch = max_batch;
  h->max_points = max_points;
  make_devcfg(*cfg, h->dc);
  const DevCfg& c = h->dc;
  if (c.use_vlp32c && (row_bin_bound(c) < 1 || row_bin_bound(c) > kBinWords * 32)) return LLSR_EINVAL;
  if (hipSetDevice(hip_device) != hipSuccess) return LLSR_ENODEV;
  if (c.use_vlp32c && llsr_host::alloc(h->row_bm, sizeof(uint32_t) * kBinWords * (size_t)max_batch) != hipSuccess)
    return LLSR_ENOMEM;
  if (llsr_host::alloc_pool(h->pool, 4096, [&](llsr_host::Carver& cv) {
        llsr_host::feature_layout(cv, h->d, max_batch, c.H, c.HW, kCnt, kAdjCap * kAdjWords);
      }) != hipSuccess)
    return LLSR_ENOMEM;
  {  // the VoxelGrid sort's range list (llsr_device.h VoxRanges) and, behind it, its counters
    const size_t subcap = ((size_t)max_batch * c.H + kVoxSub - 1) / kVoxSub * kBsList;
    if (subcap > (size_t)INT_MAX ||
        llsr_host::alloc(h->vox_mem, sizeof(int2) * subcap * kVoxSub + kVoxCntBytes) != hipSuccess)
      return LLSR_ENOMEM;
    h->vox.item = static_cast<int2*>(h->vox_mem.get());
    h->vox.count = reinterpret_cast<int*>(h->vox.item + subcap * kVoxSub);
    h->vox.subcap = (int)subcap;
    h->vox_waves = vox_leaf_waves(hip_device);
  }
  {
    uint32_t mt0[624];
    mt_first_state(mt0);
    if (hipMemcpy(h->d.mt0, mt0, sizeof(mt0), hipMemcpyHostToDevice) != hipSuccess) return LLSR_ENODEV;
  }
  if (llsr_host::alloc(h->d_in, sizeof(float4) * (size_t)max_points) != hipSuccess ||
      llsr_host::alloc(h->d_off, sizeof(int64_t) * 2) != hipSuccess ||
      llsr_host::create(h->stream, hipStreamNonBlocking) != hipSuccess)
    return LLSR_ENOMEM;
  {
    const char* ds = std::getenv("LLSR_DEBUG_SYNC");
    h->debug_sync = ds && ds[0] == '1';
  }
  for (auto& set : h->ev)
    for (auto& e : set)
      if (llsr_host::create(e) != hipSuccess) return LLSR_ENODEV;
  if (llsr_host::create(h->last_done, hipEventDisableTiming) != hipSuccess ||
      llsr_host::create(h->s2s_done, hipEventDisableTiming) != hipSuccess ||
      llsr_host::create(h->mo_done, hipEventDisableTiming) != hipSuccess)
    return LLSR_ENODEV;
  const auto set_lds = [](const void* kernel, int bytes) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
  };
  const bool lds_ok = c.ccl_lds ? set_lds((const void*)k_label<true>, label_lds(c)) &&
                                      set_lds((const void*)k_project_fused, fused_lds(c))
                                : set_lds((const void*)k_label<false>, label_band_lds(c));
  if (!lds_ok) return LLSR_ENODEV;
  const int32_t rc = llsr_reset_state(h.get());
  if (rc != LLSR_OK) return rc;
  *out = h.release();
  return LLSR_OK;
}

extern "C" void llsr_destroy(llsr_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)sync_handle_streams(h);
  mapping_free(h);
  delete h;
}

hipError_t sync_handle_streams(llsr_handle* h) {
  if (h->stream) {
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return e;
  }
  const std::pair<hipEvent_t, bool> evs[] = {{h->last_done, h->last_rec}, {h->s2s_done, h->s2s_rec},
                                             {h->mo_done, h->mo_rec}};
  for (const auto& ev : evs) {
    if (!ev.first || !ev.second) continue;
    const hipError_t e = hipEventSynchronize(ev.first);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int32_t lm_aux(llsr_handle* h, LmAux& x) {
  if (x.flags) return LLSR_OK;
  LmAux n;
  if (llsr_host::alloc(n.flags_mem, 2 * sizeof(int)) != hipSuccess) return fail(h, LLSR_ENOMEM, "pinned flags");
  for (llsr_host::Event* e : {&n.e0, &n.e1, &n.p0, &n.p1, &n.p2})
    if (llsr_host::create(*e) != hipSuccess) return fail(h, LLSR_ENODEV, "events");
  n.flags = static_cast<int*>(n.flags_mem.get());
  x = std::move(n);
  return LLSR_OK;
}

int32_t stage_oneshot(llsr_handle* h, OneShotStage& st, const float* const src[4], const int32_t n[4],
                      const float* pose, bool with_deg, size_t rep_bytes) {
  hipStream_t s;
  HIP_OK(h, enter(h, nullptr, &s));
  llsr_host::Carver measure;
  llsr_host::oneshot_layout(measure, st, n, with_deg, rep_bytes);
  if (measure.off > st.bytes) {
    st = OneShotStage{};  // the old buffer goes first; a failed allocation leaves the stage empty
    if (llsr_host::alloc(st.mem, measure.off) != hipSuccess) return fail(h, LLSR_ENOMEM, "staging");
    st.bytes = measure.off;
  }
  llsr_host::Carver place(st.mem.get());
  llsr_host::oneshot_layout(place, st, n, with_deg, rep_bytes);
  for (int k = 0; k < 4; ++k)
    if (n[k]) HIP_OK(h, hipMemcpyAsync(st.cloud[k], src[k], sizeof(float4) * n[k], hipMemcpyHostToDevice, s));
  const int64_t offs[8] = {0, n[0], 0, n[1], 0, n[2], 0, n[3]};
  HIP_OK(h, hipMemcpyAsync(st.off, offs, sizeof offs, hipMemcpyHostToDevice, s));
  HIP_OK(h, hipMemcpyAsync(st.pose, pose, 6 * sizeof(float), hipMemcpyHostToDevice, s));
  return LLSR_OK;
}

extern "C" int32_t llsr_get_config(const llsr_handle* h, llsr_config* cfg) {
  if (!h || !cfg) return LLSR_EINVAL;
  *cfg = h->cfg;
  return LLSR_OK;
}

extern "C" const char* llsr_last_error(const llsr_handle* h) { return h ? h->err.c_str() : "null handle"; }

extern "C" int32_t llsr_query_sizes(const llsr_handle* h, llsr_sizes* s) {
  if (!h || !s) return LLSR_EINVAL;
  s->cells = h->dc.HW;
  s->rings = h->dc.H;
  s->max_points = h->max_points;
  s->shadow_points = 160;
  return LLSR_OK;
}

extern "C" int32_t llsr_set_voxel_order(llsr_handle* h, int32_t order) {
  if (!h) return LLSR_EINVAL;
  if (order != LLSR_VOXEL_ORDER_INPUT && order != LLSR_VOXEL_ORDER_PCL) return fail(h, LLSR_EINVAL, "voxel order");
  h->dc.exact_vg = order == LLSR_VOXEL_ORDER_PCL ? 1 : 0;
  return LLSR_OK;
}

extern "C" int32_t llsr_set_imu_undistortion(llsr_handle* h, int32_t on) {
  if (!h) return LLSR_EINVAL;
  h->imu_undistortion = on != 0;
  return LLSR_OK;
}

extern "C" int32_t llsr_reset_state(llsr_handle* h) {
  if (!h) return LLSR_EINVAL;
  HIP_OK(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->max_batch * h->dc.HW;
  HIP_OK(h, hipMemsetAsync(h->d.picked, 0, n, h->stream));
  HIP_OK(h, hipMemsetAsync(h->d.clabel, 0, n, h->stream));
  HIP_OK(h, hipMemsetAsync(h->d.phantom, 0, sizeof(int) * (size_t)h->max_batch, h->stream));
  HIP_OK(h, hipMemsetD32Async(h->d.seg_zero, h->dc.HW, (size_t)h->max_batch, h->stream));
  if (h->imu.d_carry)  // the IMU members carried from scan to scan (FA:255-257)
    HIP_OK(h, hipMemsetAsync(h->imu.d_carry, 0, sizeof(llsr_imu_carry) * (size_t)h->max_batch, h->stream));
  HIP_OK(h, hipStreamSynchronize(h->stream));
  return LLSR_OK;
}

// ---- IMU de-skew staging (include/llsr.h; the kernel side is k_fa_points_imu, llsr_fa.hip) ----
static int32_t imu_alloc(llsr_handle* h) {
  auto& m = h->imu;
  if (m.dev) return LLSR_OK;
  llsr_handle::Imu n;
  const size_t B = (size_t)h->max_batch;
  if (llsr_host::alloc_pool(n.dev, 0, [&](llsr_host::Carver& cv) {
        llsr_host::imu_layout(cv, n, B, LLSR_IMU_WINDOW_MAX);
      }) != hipSuccess ||
      llsr_host::alloc_pool(n.host, 0, [&](llsr_host::Carver& cv) {
        llsr_host::imu_host_layout(cv, n, B, LLSR_IMU_WINDOW_MAX);
      }) != hipSuccess)
    return fail(h, LLSR_ENOMEM, "IMU staging");
  HIP_OK(h, hipMemset(n.d_carry, 0, sizeof(llsr_imu_carry) * B));
  m = std::move(n);
  return LLSR_OK;
}

extern "C" int32_t llsr_stage_imu(llsr_handle* h, const int32_t* scan_sec, const uint32_t* scan_nanosec,
                                  const llsr_imu_sample* samples, const int64_t* offsets, int32_t B) {
  if (!h) return LLSR_EINVAL;
  if (!scan_sec || !scan_nanosec || !offsets) return fail(h, LLSR_EINVAL, "llsr_stage_imu: null argument");
  if (B < 1 || B > h->max_batch) return fail(h, LLSR_ERANGE, "batch size outside [1, max_batch]");
  if (offsets[0] != 0) return fail(h, LLSR_EINVAL, "llsr_stage_imu: offsets[0] != 0");
  for (int b = 0; b < B; ++b) {
    const int64_t n = offsets[b + 1] - offsets[b];  // none, or the back entry + 1 .. 200 candidates
    if (n != 0 && (n < 2 || n > LLSR_IMU_WINDOW_MAX)) return fail(h, LLSR_EINVAL, "llsr_stage_imu: window length");
  }
  if (offsets[B] > 0 && !samples) return fail(h, LLSR_EINVAL, "llsr_stage_imu: samples is NULL");
  HIP_OK(h, hipSetDevice(h->device));
  const int32_t rc = imu_alloc(h);
  if (rc != LLSR_OK) return rc;
  // the pinned arrays may still feed the previous batch's upload
  const int32_t rs = sync_last(h);
  if (rs != LLSR_OK) return rs;
  auto& m = h->imu;
  for (int b = 0; b <= B; ++b) m.h_off[b] = (int)offsets[b];
  for (int b = 0; b < B; ++b) m.h_time[b] = scan_sec[b] + scan_nanosec[b] / 1e9;  // FA:2761
  if (offsets[B] > 0) std::memcpy(m.h_samples, samples, sizeof(llsr_imu_sample) * (size_t)offsets[B]);
  m.B = B;
  m.any = offsets[B] > 0;
  m.armed = true;
  return LLSR_OK;
}

extern "C" int32_t llsr_fetch_imu_report(llsr_handle* h, int32_t b, llsr_imu_report* report) {
  if (!h || !report) return fail(h, LLSR_EINVAL, "null argument");
  if (b < 0 || b >= h->max_batch) return fail(h, LLSR_ERANGE, "slot index outside the handle's slots");
  *report = llsr_imu_report{};
  if (!h->imu.d_carry) return LLSR_OK;  // never staged: the constructor's zeros
  const int32_t rc = sync_last(h);
  if (rc != LLSR_OK) return rc;
  llsr_imu_carry c;
  HIP_OK(h, hipMemcpy(&c, h->imu.d_carry + b, sizeof c, hipMemcpyDeviceToHost));
  *report = c.report;
  return LLSR_OK;
}

// Retire the oldest profiled batch: wait for its last event and add its kernel intervals.
static void retire_oldest(llsr_handle* h) {
  const int slot = (h->ring_head - h->ring_used + llsr_handle::kRing) % llsr_handle::kRing;
  (void)hipEventSynchronize(h->ev[slot][kSeqKernels]);
  for (int k = 0; k < kSeqKernels; ++k) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev[slot][k], h->ev[slot][k + 1]) == hipSuccess) h->ksum[k] += ms;
  }
  if (h->dc.use_vlp32c) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev[slot][kSeqKernels + 1], h->ev[slot][kSeqKernels + 2]) == hipSuccess)
      h->ksum[kRowBins] += ms;
  }
  h->kbatches += 1;
  h->ring_used -= 1;
}

extern "C" int32_t llsr_set_profiling(llsr_handle* h, int32_t enable) {
  if (!h) return LLSR_EINVAL;
  while (h->ring_used > 0) retire_oldest(h);
  for (double& v : h->ksum) v = 0.0;
  h->kbatches = 0;
  h->mo_stats = llsr_s2m_stats{};
  h->s2s_stats = llsr_s2s_stats{};
  h->profiling = enable != 0;
  return LLSR_OK;
}

extern "C" int32_t llsr_process_batch(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets,
                                      int32_t B, void* hip_stream) {
  if (!h || !d_xyzi || !d_offsets) return fail(h, LLSR_EINVAL, "null argument");
  if (B < 1 || B > h->max_batch) return fail(h, LLSR_ERANGE, "batch size outside [1, max_batch]");
  if (h->imu.armed && h->imu.B != B) return fail(h, LLSR_EINVAL, "llsr_stage_imu staged another batch size");
  hipStream_t s;
  HIP_OK(h, enter(h, hip_stream, &s));
  // the slot buffers and the FA carry-over state are shared by every batch of this handle: a
  // batch on another stream than the previous one starts after it
  if (h->last_stream && h->last_stream != s) HIP_OK(h, hipStreamWaitEvent(s, h->last_done, 0));
  const DevCfg& c = h->dc;
  const float4* pts = reinterpret_cast<const float4*>(d_xyzi);
  int k = 0;
  if (h->profiling && h->ring_used == llsr_handle::kRing) retire_oldest(h);
  const llsr_host::Event* evs = h->ev[h->ring_head];
  auto mark = [&]() {
    if (h->profiling) (void)hipEventRecord(evs[k], s);
    if (h->debug_sync) {  // diagnostics: the kernel that faults is the last one named
      const hipError_t e = hipStreamSynchronize(s);
      std::fprintf(stderr, "llsr debug: after %s: %s\n", k < kNumKernels ? kKernelNames[k] : "?", hipGetErrorString(e));
    }
    ++k;
  };
  // grid-stride kernels: ~16k workgroups in all, at least 4 per scan
  const int gx = std::max(1, std::min((h->max_points + 255) / 256, std::max(4, 16384 / B)));
  uint32_t* row_bm = static_cast<uint32_t*>(h->row_bm.get());
  if (c.use_vlp32c) {  // the slots' observed elevation bins, ahead of the kernels every handle runs
    HIP_OK(h, hipMemsetAsync(row_bm, 0, sizeof(uint32_t) * kBinWords * (size_t)B, s));
    if (h->profiling) (void)hipEventRecord(evs[kSeqKernels + 1], s);
    k_row_bins<<<dim3(gx, B), 256, 0, s>>>(c, pts, d_offsets, row_bm);
    if (h->profiling) (void)hipEventRecord(evs[kSeqKernels + 2], s);
  }
  mark();
  const bool fused = use_fused(h);
  if (!fused) HIP_OK(h, hipMemsetAsync(h->d.ccl_a, 0xFF, sizeof(int) * (size_t)B * c.HW, s));
  k_init_counts<<<(B + 255) / 256, 256, 0, s>>>(h->d.counts, B, h->vox.count);
  mark();
  if (fused) {  // fused projection + column ground pass with the cell table in LDS
    k_project_fused<<<B, 1024, fused_lds(c), s>>>(c, pts, d_offsets, h->d);
    mark();
    mark();
  } else {
    if (c.use_vlp32c) k_project<true><<<dim3(gx, B), 256, 0, s>>>(c, pts, d_offsets, h->d, row_bm);
    else k_project<false><<<dim3(gx, B), 256, 0, s>>>(c, pts, d_offsets, h->d, nullptr);
    mark();
    k_gather_column<<<dim3((c.W + 63) / 64, B), 64, sizeof(int) * 64 * (c.H + 1), s>>>(c, pts, d_offsets, h->d);
    mark();
  }
  k_ground_add<<<dim3((c.H + 3) / 4, B), 256, 0, s>>>(c, h->d);
  mark();
  k_ground_elev_ransac<<<B, per_scan_threads(c), 0, s>>>(c, h->d);
  mark();
  if (c.ccl_lds)
    k_label<true><<<B, 1024, label_lds(c), s>>>(c, h->d);
  else
    k_label<false><<<B, 1024, label_band_lds(c), s>>>(c, h->d);
  mark();
  k_segment<<<B, per_scan_threads(c), 0, s>>>(c, pts, d_offsets, h->d);
  mark();
  if (h->imu.armed && h->imu.any) {  // staged windows: uploaded on this stream, ahead of their reader
    auto& m = h->imu;
    HIP_OK(h, hipMemcpyAsync(m.d_samples, m.h_samples, sizeof(llsr_imu_sample) * (size_t)m.h_off[B],
                             hipMemcpyHostToDevice, s));
    HIP_OK(h, hipMemcpyAsync(m.d_off, m.h_off, sizeof(int) * (size_t)(B + 1), hipMemcpyHostToDevice, s));
    HIP_OK(h, hipMemcpyAsync(m.d_time, m.h_time, sizeof(double) * (size_t)B, hipMemcpyHostToDevice, s));
    launch_fa_points_imu(c, h->d, ImuDev{m.d_samples, m.d_off, m.d_time, m.d_carry}, B, s);
  } else {
    launch_fa_points(c, h->d, B, s);
  }
  mark();
  k_select_ring<<<dim3(c.H, B), 256, 0, s>>>(c, h->d);
  mark();
  if (c.exact_vg) launch_vox_pcl(c, h->d, h->vox, h->vox_waves, B, s);
  mark();
  k_fa_concat<<<B, 256, 0, s>>>(c, h->d);
  mark();
  k_dbscan_adj<<<dim3(32, B), 256, 0, s>>>(c, h->d, h->d.db_pts);
  mark();
  if (c.HW <= 32768) k_dbscan_merge<1024><<<B, 64, 0, s>>>(c, h->d);
  else k_dbscan_merge<2048><<<B, 64, 0, s>>>(c, h->d);
  mark();
  HIP_OK(h, hipGetLastError());
  HIP_OK(h, hipEventRecord(h->last_done, s));
  h->last_rec = true;
  if (h->profiling) {
    h->ring_head = (h->ring_head + 1) % llsr_handle::kRing;
    h->ring_used += 1;
  }
  h->imu.armed = false;  // consumed: the slots' carry advanced with this feature stage
  h->last_stream = s;
  h->last_B = B;
  h->last_pts = pts;
  h->last_off = d_offsets;
  return LLSR_OK;
}

int32_t sync_last(llsr_handle* h) {
  HIP_OK(h, hipSetDevice(h->device));
  if (h->last_rec) HIP_OK(h, hipEventSynchronize(h->last_done));
  else HIP_OK(h, hipStreamSynchronize(h->stream));
  return LLSR_OK;
}

extern "C" int32_t llsr_kernel_times_ms(llsr_handle* h, float* out, int32_t cap) {
  if (!h || !out) return LLSR_EINVAL;
  HIP_OK(h, hipSetDevice(h->device));
  while (h->ring_used > 0) retire_oldest(h);
  if (h->kbatches == 0) return 0;
  int n = 0;
  // k_row_bins, the table's last entry, only where it runs
  const int nk = h->dc.use_vlp32c ? kNumKernels : kSeqKernels;
  for (int k = 0; k < nk && n < cap; ++k, ++n) out[n] = (float)(h->ksum[k] / (double)h->kbatches);
  return n;
}

extern "C" int32_t llsr_row_bins(llsr_handle* h, int32_t b, int32_t* n_bins, int32_t* bins, int32_t cap) {
  if (!h || !n_bins || cap < 0 || (cap > 0 && !bins)) return LLSR_EINVAL;
  if (!h->dc.use_vlp32c) return fail(h, LLSR_EINVAL, "llsr_row_bins needs a use_vlp32c handle");
  if (b < 0 || b >= h->last_B) return fail(h, LLSR_ERANGE, "slot outside last batch");
  int32_t rc = sync_last(h);
  if (rc) return rc;
  uint32_t bm[kBinWords];
  HIP_OK(h, d2h(bm, static_cast<const uint32_t*>(h->row_bm.get()) + (size_t)b * kBinWords, kBinWords));
  int n = 0;
  for (int bin = 0; bin < kBinWords * 32; ++bin) {
    if (!((bm[bin >> 5] >> (bin & 31)) & 1u)) continue;
    if (n < cap) bins[n] = bin;
    ++n;
  }
  *n_bins = n;
  return LLSR_OK;
}

// Diagnostics (not part of the ABI header): the device's exact libstdc++ std::sort as k_select_ring
// runs it on a ring's curvatures (llsr_isort.h block_introsort, one 256-thread workgroup) on
// n <= 2048 host values; out[k] = the input position at sorted position k. For
// tests/test_gpu_features_ties.py.
extern "C" int32_t llsr_debug_exact_sort(const float* vals, int32_t n, int32_t* out) {
  if (!vals || !out || n < 0 || n > 2048) return LLSR_EINVAL;
  if (n == 0) return LLSR_OK;
  llsr_host::DevMem dv, di;
  if (llsr_host::alloc(dv, sizeof(float) * n) != hipSuccess || llsr_host::alloc(di, sizeof(int) * n) != hipSuccess)
    return LLSR_ENODEV;
  if (hipMemcpy(dv, vals, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess) return LLSR_EIO;
  k_debug_exact_sort<<<1, 256>>>((const float*)dv.get(), n, (int*)di.get());
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(out, di, sizeof(int) * n, hipMemcpyDeviceToHost) != hipSuccess)
    return LLSR_EIO;
  return LLSR_OK;
}

// Diagnostics (not part of the ABI header): the PCL-order VoxelGrid's exact sort of 32-bit keys
// (VoxLess32: voxel rank << 11 | position) on n <= 2048 host ranks < 2^21, by the kernels a batch
// runs (k_vox_top, k_vox_leaf) on a one-ring scan made of the keys; out[k] = the input position at
// sorted position k. For tests/test_gpu_features_ties.py and tests/test_gpu_vox_split.py.
extern "C" int32_t llsr_debug_exact_sort32(const uint32_t* ranks, int32_t n, int32_t* out) {
  if (!ranks || !out || n < 0 || n > 2048) return LLSR_EINVAL;
  for (int32_t t = 0; t < n; ++t)
    if (ranks[t] >= (1u << 21)) return LLSR_EINVAL;
  if (n == 0) return LLSR_OK;
  std::vector<uint32_t> key(n);
  for (int32_t t = 0; t < n; ++t) key[t] = (ranks[t] << 11) | (uint32_t)t;
  // ring_cnt [3] (the ring pending with n candidates), start_ring [1]; the list (one ring per
  // sub-list at most) and its counters
  const int head[4] = {0, 0, -1 - n, 0};
  int device = 0;
  llsr_host::DevMem dk, dh, di;
  if (hipGetDevice(&device) != hipSuccess || llsr_host::alloc(dk, sizeof(uint32_t) * n) != hipSuccess ||
      llsr_host::alloc(dh, sizeof head) != hipSuccess ||
      llsr_host::alloc(di, sizeof(int2) * kBsList * kVoxSub + kVoxCntBytes) != hipSuccess)
    return LLSR_ENODEV;
  int2* items = static_cast<int2*>(di.get());
  if (hipMemcpy(dk, key.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dh, head, sizeof head, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(items + kBsList * kVoxSub, 0, kVoxCntBytes) != hipSuccess)
    return LLSR_EIO;
  DevCfg c{};
  c.H = 1;
  c.W = c.HW = n;
  c.dbg_phase = 102;  // the sort without the centroids
  DevBufs d{};
  d.ccl_a = static_cast<int*>(dk.get());
  d.ring_cnt = static_cast<int*>(dh.get());
  d.start_ring = d.ring_cnt + 3;
  const VoxRanges vr{items, reinterpret_cast<int*>(items + kBsList * kVoxSub), kBsList};
  launch_vox_pcl(c, d, vr, vox_leaf_waves(device), 1, nullptr);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(key.data(), dk, sizeof(uint32_t) * n, hipMemcpyDeviceToHost) != hipSuccess)
    return LLSR_EIO;
  for (int32_t t = 0; t < n; ++t) out[t] = (int32_t)(key[t] & 0x7ffu);
  return LLSR_OK;
}

// Diagnostics (not part of the ABI header): the PCL-order VoxelGrid's sort keys of one ring's worth
// of candidate points, points[L][4] (x, y, z, intensity) with 1 <= L <= 2048, by the code
// k_select_ring runs on a ring (vox_pcl_keys, in a kernel of its own): keys_out[t] = order << 11 | t
// with `order` strictly increasing in the PCL voxel id of point t. *path_out = 0 where the keys came
// from the row bitmap, 1 from the sorted runs (force_runs != 0 takes that path whatever the grid),
// -1 where PCL's grid overflows and no keys are made. For tests/test_gpu_vox_keys.py.
extern "C" int32_t llsr_debug_vox_keys(const float* points, int32_t L, int32_t force_runs, uint32_t* keys_out,
                                       int32_t* path_out) {
  if (!points || !keys_out || !path_out || L < 1 || L > 2048) return LLSR_EINVAL;
  llsr_host::DevMem dp, dk, dq;
  if (llsr_host::alloc(dp, sizeof(float4) * L) != hipSuccess || llsr_host::alloc(dk, sizeof(uint32_t) * L) != hipSuccess ||
      llsr_host::alloc(dq, sizeof(int)) != hipSuccess)
    return LLSR_ENODEV;
  if (hipMemcpy(dp, points, sizeof(float4) * L, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dk, 0, sizeof(uint32_t) * L) != hipSuccess)
    return LLSR_EIO;
  k_debug_vox_keys<<<1, 256>>>((const float4*)dp.get(), L, force_runs, (uint32_t*)dk.get(), (int*)dq.get());
  int path = 0;
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(keys_out, dk, sizeof(uint32_t) * L, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&path, dq, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    return LLSR_EIO;
  *path_out = path;
  return LLSR_OK;
}

// Diagnostics (not part of the ABI header): out[b] = C_VOXRUNS of slot b of the last batch, the
// number of its rings whose PCL-order keys came from the sorted runs (grid beyond the row bitmap).
extern "C" int32_t llsr_debug_vox_runs(llsr_handle* h, int32_t* out) {
  if (!h || !out) return LLSR_EINVAL;
  int32_t rc = sync_last(h);
  if (rc) return rc;
  std::vector<int> cnt((size_t)h->last_B * kCnt);
  HIP_OK(h, hipMemcpy(cnt.data(), h->d.counts, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int b = 0; b < h->last_B; ++b) out[b] = cnt[(size_t)b * kCnt + C_VOXRUNS];
  return LLSR_OK;
}

// Diagnostics (not part of the ABI header): the DBSCAN merge and its run-length filter as a batch
// runs them (k_dbscan_merge<kDbL>, kDbL 1024 or 2048) over n independent neighbourhood relations
// given as host bit rows adj[n][kAdjCap][kAdjWords] (row i, bit j: j is a neighbour of i; only rows
// below M[k] and the two words of every 64-point chunk below M[k] are read, as k_dbscan_adj writes
// them), M[k] <= kDbL. less_sharp[a] = a, so sharp[n][kAdjCap] returns positions; cluster is
// [n][kAdjCap] too, entries past M[k] / n_sharp[k] are -1. For tests/test_gpu_dbscan_merge.py.
extern "C" int32_t llsr_debug_dbscan_merge(const uint32_t* adj, const int32_t* M, int32_t n, int32_t kDbL,
                                           int32_t* cluster, int32_t* sharp, int32_t* n_sharp) {
  if (!adj || !M || !cluster || !sharp || !n_sharp || n < 1 || n > 1024 || (kDbL != 1024 && kDbL != 2048))
    return LLSR_EINVAL;
  for (int32_t k = 0; k < n; ++k)
    if (M[k] < 0 || M[k] > kDbL) return LLSR_EINVAL;
  const size_t HW = kAdjCap, nadj = (size_t)n * kAdjCap * kAdjWords;
  std::vector<int> cnt((size_t)n * kCnt, 0), pos((size_t)n * HW);
  for (int32_t k = 0; k < n; ++k) {
    cnt[(size_t)k * kCnt + C_M] = M[k];
    for (size_t a = 0; a < HW; ++a) pos[k * HW + a] = (int)a;
  }
  llsr_host::DevMem dadj, dcnt, dpos, dcl, dsh;
  if (llsr_host::alloc(dadj, sizeof(uint32_t) * nadj) != hipSuccess ||
      llsr_host::alloc(dcnt, sizeof(int) * cnt.size()) != hipSuccess ||
      llsr_host::alloc(dpos, sizeof(int) * n * HW) != hipSuccess ||
      llsr_host::alloc(dcl, sizeof(int) * n * HW) != hipSuccess ||
      llsr_host::alloc(dsh, sizeof(int) * n * HW) != hipSuccess)
    return LLSR_ENODEV;
  if (hipMemcpy(dadj, adj, sizeof(uint32_t) * nadj, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dcnt, cnt.data(), sizeof(int) * cnt.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dpos, pos.data(), sizeof(int) * n * HW, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dcl, 0xff, sizeof(int) * n * HW) != hipSuccess ||
      hipMemset(dsh, 0xff, sizeof(int) * n * HW) != hipSuccess)
    return LLSR_EIO;
  DevCfg c{};
  c.HW = (int)HW;
  DevBufs d{};  // the fields the kernel reads at M <= kDbL
  d.counts = static_cast<int*>(dcnt.get());
  d.db_adj = static_cast<uint32_t*>(dadj.get());
  d.less_sharp = static_cast<int*>(dpos.get());
  d.cluster = static_cast<int*>(dcl.get());
  d.sharp = static_cast<int*>(dsh.get());
  if (kDbL == 1024) k_dbscan_merge<1024><<<n, 64>>>(c, d);
  else k_dbscan_merge<2048><<<n, 64>>>(c, d);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(cluster, dcl, sizeof(int) * n * HW, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(sharp, dsh, sizeof(int) * n * HW, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(cnt.data(), dcnt, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return LLSR_EIO;
  for (int32_t k = 0; k < n; ++k) n_sharp[k] = cnt[(size_t)k * kCnt + C_SHARP];
  return LLSR_OK;
}

// Diagnostics (not part of the ABI header): adjustDistortion's halfPassed test (FA:578-586) as
// k_segment evaluates it, for n (y, x, start) triples: out[3 i] = the certified fast test's code
// (0 fails, 1 passes, 2 undecided), out[3 i + 1] = its decision with the exact fallback, out[3 i + 2] =
// the exact libm test.
extern "C" int32_t llsr_debug_half_passed(const float* yxs, int32_t n, uint8_t* out) {
  if (!yxs || !out || n < 0 || n > (1 << 24)) return LLSR_EINVAL;
  if (n == 0) return LLSR_OK;
  llsr_host::DevMem dv, dout;
  if (llsr_host::alloc(dv, sizeof(float) * 3 * (size_t)n) != hipSuccess ||
      llsr_host::alloc(dout, 3 * (size_t)n) != hipSuccess)
    return LLSR_ENODEV;
  if (hipMemcpy(dv, yxs, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) return LLSR_EIO;
  k_debug_half_passed<<<(n + 255) / 256, 256>>>((const float*)dv.get(), n, (uint8_t*)dout.get());
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(out, dout, 3 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
    return LLSR_EIO;
  return LLSR_OK;
}

// Diagnostics (not part of the ABI header): mean device ms of one block_introsort of vals[0, n)
// by one 256-thread workgroup (k_debug_exact_sort), over `reps` launches.
extern "C" float llsr_debug_exact_sort_ms(const float* vals, int32_t n, int32_t reps) {
  if (!vals || n < 1 || n > 2048 || reps < 1) return -1.f;
  llsr_host::DevMem dv, di;
  llsr_host::Event e0, e1;
  float ms = -1.f;
  if (llsr_host::alloc(dv, sizeof(float) * n) == hipSuccess && llsr_host::alloc(di, sizeof(int) * n) == hipSuccess &&
      llsr_host::create(e0) == hipSuccess && llsr_host::create(e1) == hipSuccess &&
      hipMemcpy(dv, vals, sizeof(float) * n, hipMemcpyHostToDevice) == hipSuccess) {
    k_debug_exact_sort<<<1, 256>>>((const float*)dv.get(), n, (int*)di.get());
    (void)hipEventRecord(e0, nullptr);
    for (int r = 0; r < reps; ++r) k_debug_exact_sort<<<1, 256>>>((const float*)dv.get(), n, (int*)di.get());
    (void)hipEventRecord(e1, nullptr);
    if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ms /= reps;
  }
  return ms;
}

// After diagnostic launches of the selection stage that stop early: the whole stage once more with
// the handle's configuration, so every ring's less-flat count is final again (k_select_ring leaves
// a pending ring's count negative until the PCL-order VoxelGrid writes it; a later k_fa_concat
// builds its ring offsets from these counts).
static void restore_selection(llsr_handle* h, int B, hipStream_t s) {
  const DevCfg& c = h->dc;
  launch_fa_points(c, h->d, B, s);
  // (the diagnostic launches counted their run-path rings too: C_VOXRUNS starts over)
  (void)hipMemset2DAsync(h->d.counts + C_VOXRUNS, sizeof(int) * kCnt, 0, sizeof(int), B, s);
  k_select_ring<<<dim3(c.H, B), 256, 0, s>>>(c, h->d);
  if (c.exact_vg) {
    (void)hipMemsetAsync(h->vox.count, 0, kVoxCntBytes, s);
    launch_vox_pcl(c, h->d, h->vox, h->vox_waves, B, s);
  }
  (void)hipStreamSynchronize(s);
}

// Diagnostics (not part of the ABI header): re-launch kernel k on the last batch's buffers with
// an early exit at `phase`, `reps` times; returns the mean device ms per launch (< 0 on error).
// Used to attribute a kernel's time to its phases; results of such launches are meaningless.
extern "C" float llsr_debug_phase_ms(llsr_handle* h, int32_t k, int32_t phase, int32_t reps) {
  if (!h || h->last_B < 1 || reps < 1) return -1.f;
  if (hipSetDevice(h->device) != hipSuccess) return -1.f;
  hipStream_t s = h->stream;
  DevCfg c = h->dc;
  c.dbg_phase = phase;
  const int B = h->last_B;
  hipEvent_t e0 = h->ev[0][0], e1 = h->ev[0][1];
  if (sync_last(h) != LLSR_OK) return -1.f;
  if (k == 9) {  // the PCL-order VoxelGrid needs the keys k_select_ring leaves and an empty range
    float tot = 0.f;  // list: both redone before each launch
    for (int r = 0; r < reps; ++r) {
      launch_fa_points(h->dc, h->d, B, s);
      k_select_ring<<<dim3(c.H, B), 256, 0, s>>>(h->dc, h->d);
      (void)hipMemsetAsync(h->vox.count, 0, kVoxCntBytes, s);
      (void)hipEventRecord(e0, s);
      launch_vox_pcl(c, h->d, h->vox, h->vox_waves, B, s);
      (void)hipEventRecord(e1, s);
      float ms = 0.f;
      if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1.f;
      tot += ms;
    }
    restore_selection(h, B, s);
    return tot / reps;
  }
  if (k == 8) {
    // k_select_ring consumes the picked / label state k_fa_points leaves (and overwrites it):
    // k_fa_points restores it before every timed launch, so each phase sees the batch's real work
    float tot = 0.f;
    for (int r = 0; r < reps; ++r) {
      launch_fa_points(h->dc, h->d, B, s);
      (void)hipEventRecord(e0, s);
      k_select_ring<<<dim3(c.H, B), 256, 0, s>>>(c, h->d);
      (void)hipEventRecord(e1, s);
      float ms = 0.f;
      if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1.f;
      tot += ms;
    }
    restore_selection(h, B, s);
    return tot / reps;
  }
  (void)hipEventRecord(e0, s);
  for (int r = 0; r < reps; ++r) {
    switch (k) {
      case 8: k_select_ring<<<dim3(c.H, B), 256, 0, s>>>(c, h->d); break;
      case 10: k_fa_concat<<<B, 256, 0, s>>>(c, h->d); break;
      case 11: k_dbscan_adj<<<dim3(32, B), 256, 0, s>>>(c, h->d, h->d.db_pts); break;
      case 12:
        if (c.HW <= 32768) k_dbscan_merge<1024><<<B, 64, 0, s>>>(c, h->d);
        else k_dbscan_merge<2048><<<B, 64, 0, s>>>(c, h->d);
        break;
      case 7: launch_fa_points(c, h->d, B, s); break;
      case 6: k_segment<<<B, per_scan_threads(c), 0, s>>>(c, h->last_pts, h->last_off, h->d); break;
      case 5:
        if (c.ccl_lds) k_label<true><<<B, 1024, label_lds(c), s>>>(c, h->d);
        else k_label<false><<<B, 1024, label_band_lds(c), s>>>(c, h->d);
        break;
      case 4: k_ground_elev_ransac<<<B, per_scan_threads(c), 0, s>>>(c, h->d); break;
      case 3: k_ground_add<<<dim3((c.H + 3) / 4, B), 256, 0, s>>>(c, h->d); break;
      case 1:
        if (!use_fused(h)) return -2.f;
        k_project_fused<<<B, 1024, fused_lds(c), s>>>(c, h->last_pts, h->last_off, h->d);
        break;
      default: return -2.f;
    }
  }
  (void)hipEventRecord(e1, s);
  if (hipEventSynchronize(e1) != hipSuccess) return -1.f;
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  return ms / reps;
}

extern "C" const char* llsr_kernel_name(int32_t k) {
  return (k >= 0 && k < kNumKernels) ? kKernelNames[k] : "";
}

extern "C" int32_t llsr_batch_counts(llsr_handle* h, int32_t* out) {
  if (!h || !out) return LLSR_EINVAL;
  int32_t rc = sync_last(h);
  if (rc) return rc;
  std::vector<int> cnt((size_t)h->last_B * kCnt);
  HIP_OK(h, hipMemcpy(cnt.data(), h->d.counts, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
  const int idx[8] = {C_NPTS, C_S, C_O, C_M, C_SHARP, C_F, C_L, C_K};
  for (int b = 0; b < h->last_B; ++b)
    for (int q = 0; q < 8; ++q) out[b * 8 + q] = cnt[(size_t)b * kCnt + idx[q]];
  return LLSR_OK;
}

extern "C" int32_t llsr_fetch_scan(llsr_handle* h, int32_t b, llsr_scan_out* o) {
  if (!h || !o) return LLSR_EINVAL;
  if (b < 0 || b >= h->last_B) return fail(h, LLSR_ERANGE, "slot outside last batch");
  int32_t rc = sync_last(h);
  if (rc) return rc;
  const DevCfg& c = h->dc;
  const size_t base = (size_t)b * c.HW;
  int cnt[kCnt];
  HIP_OK(h, d2h(cnt, h->d.counts + b * kCnt, kCnt));
  float ori[4];
  HIP_OK(h, d2h(ori, h->d.orient + b * 4, 4));
  o->n_points = cnt[C_NPTS];
  std::memcpy(o->orientation, ori, sizeof(float) * 3);
  const int S = cnt[C_S], O = cnt[C_O], M = cnt[C_M];
  o->n_segmented = S;
  o->n_outlier = O;
  o->n_near = cnt[C_K];
  o->n_ransac_inliers = cnt[C_INL];
  o->ransac_iterations = cnt[C_RIT];
  o->n_less_sharp = M;
  o->n_sharp = cnt[C_SHARP];
  o->n_flat = cnt[C_F];
  o->n_less_flat = cnt[C_L];
  HIP_OK(h, d2h(o->range_image, h->d.range + base, c.HW));
  HIP_OK(h, d2h(o->cell_point, h->d.cell_pt + base, c.HW));
  HIP_OK(h, d2h(o->ground_image, h->d.ground + base, c.HW));
  HIP_OK(h, d2h(o->label_image, h->d.label + base, c.HW));
  HIP_OK(h, d2h(o->start_ring_index, h->d.start_ring + (size_t)b * c.H, c.H));
  HIP_OK(h, d2h(o->end_ring_index, h->d.end_ring + (size_t)b * c.H, c.H));
  HIP_OK(h, d2h(o->seg_xyzi, (const float*)(h->d.seg + base), 4 * (size_t)S));
  HIP_OK(h, d2h(o->seg_ground_flag, h->d.seg_ground + base, S));
  HIP_OK(h, d2h(o->seg_col_ind, h->d.seg_col + base, S));
  HIP_OK(h, d2h(o->seg_range, h->d.seg_range + base, S));
  HIP_OK(h, d2h(o->seg_intensity, h->d.seg_int + base, S));
  HIP_OK(h, d2h(o->outlier_xyzi, (const float*)(h->d.outl + base), 4 * (size_t)O));
  HIP_OK(h, d2h(o->outlier_intensity, h->d.outl_int + base, O));
  HIP_OK(h, d2h(o->loam_xyzi, (const float*)(h->d.loam + base), 4 * (size_t)S));
  HIP_OK(h, d2h(o->curvature, h->d.curv + base, S));
  HIP_OK(h, d2h(o->picked, h->d.picked + base, S));
  HIP_OK(h, d2h(o->label, h->d.clabel + base, S));
  HIP_OK(h, d2h(o->less_sharp_ind, h->d.less_sharp + base, M));
  HIP_OK(h, d2h(o->dbscan_cluster, h->d.cluster + base, M));
  HIP_OK(h, d2h(o->sharp_ind, h->d.sharp + base, o->n_sharp));
  HIP_OK(h, d2h(o->flat_ind, h->d.flat + base, o->n_flat));
  HIP_OK(h, d2h(o->less_flat_xyzi, (const float*)(h->d.lflat + base), 4 * (size_t)o->n_less_flat));
  return LLSR_OK;
}

extern "C" int32_t llsr_fetch_vis_clouds(llsr_handle* h, int32_t b, llsr_vis_out* o) {
  if (!h || !o) return LLSR_EINVAL;
  if (b < 0 || b >= h->last_B) return fail(h, LLSR_ERANGE, "slot outside last batch");
  int32_t rc = sync_last(h);
  if (rc) return rc;
  const DevCfg& c = h->dc;
  const size_t HW = (size_t)c.HW;
  if (!h->d_vis) HIP_OK(h, llsr_host::alloc(h->d_vis, sizeof(float4) * (6 * HW + 1)));
  float4* d_vis = static_cast<float4*>(h->d_vis.get());
  int* d_cnt = reinterpret_cast<int*>(d_vis + 6 * HW);
  k_vis_clouds<<<1, 1024, 0, h->stream>>>(c, h->d, b, d_vis, d_cnt);
  HIP_OK(h, hipGetLastError());
  HIP_OK(h, hipStreamSynchronize(h->stream));
  int cnt[4];
  HIP_OK(h, d2h(cnt, d_cnt, 4));
  o->n_ground = cnt[0];
  o->n_nonground = cnt[1];
  o->n_unknownground = cnt[2];
  o->n_segmented_pure = cnt[3];
  float* dst[6] = {o->full_cloud, o->full_info_cloud, o->ground_cloud, o->nonground_cloud, o->unknownground_cloud,
                   o->segmented_cloud_pure};
  const size_t n[6] = {HW, HW, (size_t)cnt[0], (size_t)cnt[1], (size_t)cnt[2], (size_t)cnt[3]};
  for (int k = 0; k < 6; ++k)
    if (dst[k] && n[k]) HIP_OK(h, d2h(dst[k], (const float*)(d_vis + k * HW), 4 * n[k]));
  return LLSR_OK;
}

extern "C" int32_t llsr_process_scan(llsr_handle* h, const float* xyzi, int32_t n, llsr_scan_out* out) {
  if (!h || !out || n < 0 || (n > 0 && !xyzi)) return fail(h, LLSR_EINVAL, "bad argument");
  if (n > h->max_points) return fail(h, LLSR_ERANGE, "scan larger than max_points");
  HIP_OK(h, hipSetDevice(h->device));
  const int64_t off[2] = {0, n};
  HIP_OK(h, hipStreamSynchronize(h->stream));
  if (n > 0) HIP_OK(h, hipMemcpy(h->d_in, xyzi, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice));
  HIP_OK(h, hipMemcpy(h->d_off, off, sizeof off, hipMemcpyHostToDevice));
  int32_t rc = llsr_process_batch(h, (const float*)h->d_in.get(), (const int64_t*)h->d_off.get(), 1, h->stream);
  if (rc) return rc;
  return llsr_fetch_scan(h, 0, out);
}
