// llsr_handle.h — private to the C-ABI host layer (llsr_capi*.hip): the handle, error reporting,
// and the helpers that cross its translation units (hidden: the library exports only the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/llsr.h"
#include "llsr_device.h"
#include "llsr_mapping.h"
#include "llsr_mo.h"
#include "llsr_pools.h"
#include "llsr_s2s.h"

#define LLSR_HIDDEN __attribute__((visibility("hidden")))

constexpr int kSeqKernels = 13;  // feature-batch kernels every handle runs back to back
// ... and, at the table's end, k_row_bins: a use_vlp32c handle runs it ahead of them, between two
// events of its own
constexpr int kNumKernels = kSeqKernels + 1;
constexpr int kRowBins = kSeqKernels;

// Pinned flag words and timing events of an LM stage (scan-to-map, scan-to-scan), made once.
struct LLSR_HIDDEN LmAux {
  llsr_host::PinnedMem flags_mem;
  int* flags = nullptr;        // scan-to-map: n_active, error; scan-to-scan: error
  llsr_host::Event e0, e1;     // the one-shot's report.ms
  llsr_host::Event p0, p1, p2;  // profiling: start, grid(s) built, LM done
};

// Device staging of a one-shot call, regrown to the largest problem seen.
struct LLSR_HIDDEN OneShotStage {
  llsr_host::DevMem mem;
  size_t bytes = 0;
  float4* cloud[4] = {};
  int64_t* off = nullptr;
  float* pose = nullptr;
  int* deg = nullptr;
  char* rep = nullptr;
};

// A device point buffer that doubles on demand (mp_grow).
struct LLSR_HIDDEN GrowBuf {
  llsr_host::DevMem mem;
  size_t cap = 0;
  float4* p() const { return static_cast<float4*>(mem.get()); }
};

// Members are destroyed last to first: the stream and the completion events come first, so they
// outlive every buffer work on them may touch.
struct LLSR_HIDDEN llsr_handle {
  llsr_config cfg;
  llsr::DevCfg dc;
  int device = 0;
  int max_batch = 0, max_points = 0;
  llsr_host::Stream stream;
  hipStream_t last_stream = nullptr;  // compared, never used: the caller may destroy its streams
  llsr_host::Event last_done;  // recorded after each batch: the next one (any stream) waits on it
  // Handle-owned completion events of the last work enqueued on a caller's stream, per kind
  // (feature batches / odometry / mapping, scan-to-scan, scan-to-map): buffer re-allocation and
  // llsr_destroy wait on these, so a stream the caller destroyed since is never touched.
  llsr_host::Event s2s_done, mo_done;
  bool last_rec = false, s2s_rec = false, mo_rec = false;
  llsr::DevBufs d{};
  llsr_host::DevMem pool;
  llsr_host::DevMem vox_mem;   // vox's items, then its counters
  llsr::VoxRanges vox{};       // the PCL-order VoxelGrid's range list, sized for max_batch (llsr_device.h)
  int vox_waves = 0;           // k_vox_leaf's largest grid (vox_leaf_waves)
  llsr_host::DevMem d_in;      // float4 [max_points]: single-scan staging
  llsr_host::DevMem d_vis;     // llsr_fetch_vis_clouds: 6 x HW points + 4 counts (on first use)
  llsr_host::DevMem d_off;     // int64 [2]
  llsr_host::DevMem row_bm;    // use_vlp32c: uint32 [max_batch][kBinWords] observed elevation bins
  int last_B = 0;
  const float4* last_pts = nullptr;  // inputs of the last batch (diagnostic re-launches only)
  const int64_t* last_off = nullptr;
  bool profiling = false;
  bool debug_sync = false;  // LLSR_DEBUG_SYNC=1: wait after every feature-batch kernel, name a failing one
  // Event sets for up to kRing in-flight profiled batches; retired sets are summed into ksum.
  static constexpr int kRing = 64;
  llsr_host::Event ev[kRing][kSeqKernels + 3];  // kSeqKernels + 1 boundaries, then k_row_bins' pair
  int ring_head = 0, ring_used = 0;
  double ksum[kNumKernels] = {};
  long long kbatches = 0;
  // scan-to-map (llsr_scan2map_*): what llsr_scan2map_reserve builds; pool null = not reserved
  struct S2M {
    int P = 0, qc = 0, qs = 0, mc = 0, ms = 0, log2T_c = 0, log2T_s = 0, blocks_c = 0, blocks = 0;
    llsr_host::DevMem pool;
    llsr::S2MArgs a{};
    llsr::S2MArgs sh{};          // the open split-correspondence batch (llsr_scan2map_shard_*)
    bool sh_live = false;
  } mo;
  LmAux mo_aux;
  OneShotStage mo_stage;       // llsr_scan2map
  llsr_s2m_stats mo_stats{};
  // scan-to-scan (llsr_scan2scan_*): what llsr_scan2scan_reserve builds
  struct S2S {
    int P = 0, ms = 0, f = 0, nc = 0, ns = 0;
    llsr_host::DevMem pool;
    llsr::S2SArgs a{};
  } s2s;
  LmAux s2s_aux;
  OneShotStage s2s_stage;      // llsr_scan2scan
  llsr_s2s_stats s2s_stats{};
  int s2s_last_variant = 0;  // kLdsRows of the last k_s2s_lm instantiation launched (diagnostics)
  // end-to-end odometry (llsr_odometry_*): per-slot FA state + packed clouds, allocated lazily
  // (odo_alloc); the pieces in llsr_pools.h's order
  struct Odo {
    llsr_host::DevMem pool;
    llsr_host::PinnedMem host;
    llsr_host::Span zero[2];      // what llsr_odometry_reset clears in the pool
    int B = 0;                    // slots
    size_t cap = 0;               // points per packed buffer (B * (H*W + 160))
    float* tcur = nullptr;        // [B][6]
    float* tsum = nullptr;        // [B][6]
    int* deg = nullptr;           // [B] isDegenerate
    int* inited = nullptr;        // [B]
    int* frames = nullptr;        // [B]
    float4* shadow = nullptr;     // [160]
    float4 *sharp = nullptr, *flat = nullptr, *scan_c = nullptr, *scan_s = nullptr;
    float4 *last_c[2] = {nullptr, nullptr}, *last_s[2] = {nullptr, nullptr};
    int64_t* off = nullptr;       // device [6][B+1]: sharp, flat, last_c[0], last_c[1], last_s[0], last_s[1]
    llsr_s2s_report* report = nullptr;  // [B]
    // llsr_odometry_batch_odom: updateInitialGuess's transformCur per slot, the slots it replaces
    // the LM's in, and the LM's own result of those slots
    float* guess = nullptr;       // [B][6]
    float* tlm = nullptr;         // [B][6]
    unsigned char* flags = nullptr;  // [B]
    int64_t* h_off = nullptr;     // pinned copy of off
    int* h_counts = nullptr;      // pinned [B][kCnt]
    float* h_tsum = nullptr;      // pinned [B][6] transformSum
    float* h_guess = nullptr;     // pinned [B][6]
    unsigned char* h_flags = nullptr;  // pinned [B]
    int cur = 0;                  // last_c/s[cur] hold the current last clouds
  } odo;
  // use_imu_undistortion (llsr_set_imu_undistortion): the odometry launches k_odo_*_imu; a handle
  // setting like dc.exact_vg, untouched by the reset calls
  bool imu_undistortion = false;
  // mapping chain (llsr_mapping_*): MapOptimization's members per slot + the batch buffers
  struct MapSlot {
    llsr_mapping::MoPoses pose;
    llsr_map* map = nullptr;           // keyframe store (cornerCloudKeyFrames etc., cloudKeyPoses6D)
    float robot[3] = {0, 0, 0};        // currentRobotPosPoint
    int frames = 0, mo_frames = 0, lm_ran = 0, n_cq = 0, n_sq = 0;
    int cycle = 0;                     // FeatureAssociation's _cycle_count (FA:2818-2821)
    llsr_lm_report lm{};
    llsr_map_report mrep{};
    std::vector<float> keyposes;       // [keyframes][6]
    double now = NAN;                  // timeLaserOdometry.seconds() of the last staged scan MapOptimization ran
  };
  // device: pose [B][6], report [B], deg [B], matP [B][36], off [5][B+1], and the deg / matP of
  // the frame before (rollback); pinned host mirror
  struct MapSmall {
    llsr_host::DevMem dev;
    llsr_host::PinnedMem host;
    float* d_pose = nullptr; llsr_lm_report* d_rep = nullptr; int* d_deg = nullptr; float* d_matP = nullptr;
    int* d_deg_bak = nullptr; float* d_matP_bak = nullptr;
    int64_t* d_off = nullptr;
    float* h_pose = nullptr; llsr_lm_report* h_rep = nullptr; int64_t* h_off = nullptr; int* h_frames = nullptr;
    float* h_tsum = nullptr;
  };
  struct {
    bool live = false;
    int mode = LLSR_MODE_LM_APPLIED;   // MapOptimization's LM mode
    llsr_map_config mcfg{};
    llsr_map* vg = nullptr;            // VoxelGrid engine of the batched downsample
    std::vector<MapSlot> slot;
    GrowBuf outl, ds, tot, cmap;       // cmap: empty-map base
    MapSmall sm;
    // loop closure of the slots (llsr_mapping_stage_times / llsr_mapping_loop_closure): the scan times
    // staged for the next batch call, the gathered raw clouds of the slots with a candidate, and the
    // chain's own ICP workspace (created on first use)
    std::vector<double> times;
    bool times_staged = false;
    GrowBuf lsrc, ltgt;
    llsr_icp* icp = nullptr;
    // the slots' pose graphs (llsr_mapping_enable_pose_graph): one object, graph b = slot b; NULL = off
    llsr_pg* pg = nullptr;
    // localisation mode (llsr_mapping_set_prior): the attached prior map, not owned; NULL = mapping.
    // `fresh`: no frame since llsr_mapping_init / llsr_mapping_reset (when attaching is allowed)
    llsr_prior* prior = nullptr;
    bool fresh = false;
  } mp;
  // IMU de-skew (llsr_stage_imu): device windows + per-slot carry and their pinned staging, allocated
  // on the first staging call; `armed` until a batch's feature stage consumes it
  struct Imu {
    llsr_host::DevMem dev;
    llsr_host::PinnedMem host;
    llsr_imu_sample* d_samples = nullptr;  // packed windows of the batch
    int* d_off = nullptr;                  // [max_batch + 1]
    double* d_time = nullptr;              // [max_batch] timeScanCur
    llsr_imu_carry* d_carry = nullptr;     // [max_batch]
    llsr_imu_sample* h_samples = nullptr;
    int* h_off = nullptr;
    double* h_time = nullptr;
    bool armed = false;
    bool any = false;  // at least one slot of the staged batch has a window
    int B = 0;
  } imu;
  std::string err;
};

static inline int32_t fail(llsr_handle* h, int32_t code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

#define HIP_OK(h, expr)                                                                  \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
      return fail(h, LLSR_EIO, std::string(#expr ": ") + hipGetErrorString(e_));         \
  } while (0)

// Entry-point preamble: make the handle's device current; *s = the caller's stream, or the handle's.
static inline hipError_t enter(llsr_handle* h, void* hip_stream, hipStream_t* s) {
  *s = hip_stream ? (hipStream_t)hip_stream : h->stream.get();
  return hipSetDevice(h->device);
}

template <class T>
static hipError_t d2h(void* dst, const T* src, size_t n) {
  if (!dst || n == 0) return hipSuccess;
  return hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost);
}

// Wait for every stream this handle has launched work on (before its buffers are re-allocated):
// stream-scoped, so other handles' streams on the device keep running.
LLSR_HIDDEN hipError_t sync_handle_streams(llsr_handle* h);
// Wait for the last feature / odometry / mapping batch.
LLSR_HIDDEN int32_t sync_last(llsr_handle* h);
// The pinned flags and events of an LM stage, on first use.
LLSR_HIDDEN int32_t lm_aux(llsr_handle* h, LmAux& x);
// Stage a one-shot's four host clouds (n[k] points each), offset pairs and pose on h->stream.
LLSR_HIDDEN int32_t stage_oneshot(llsr_handle* h, OneShotStage& st, const float* const src[4], const int32_t n[4],
                                  const float* pose, bool with_deg, size_t rep_bytes);

// Options of the internal scan-to-map entry (the mapping chain): the MO mode and the optimiser's
// cross-frame members; the public entries use the handle's mode and a fresh optimiser.
struct S2MOpts {
  int mode = -1;  // -1: h->cfg.mode
  const int* deg_in = nullptr;
  const float* matP_in = nullptr;
  int* deg_out = nullptr;
  float* matP_out = nullptr;
};
LLSR_HIDDEN int32_t s2m_batch(llsr_handle* h, const llsr_s2m_batch* b, hipStream_t s, const S2MOpts& opt);
// hint_q / hint_nc: this launch's largest query count and corner-last cloud when the caller knows
// them (the odometry chain), else 0 = the reserved capacities; they pick the LM instantiation only
LLSR_HIDDEN int32_t s2s_launch(llsr_handle* h, const llsr_s2s_batch* b, void* hip_stream, int hint_q, int hint_nc);
LLSR_HIDDEN int32_t odo_alloc(llsr_handle* h);
// llsr_odometry_batch (samples == nullptr) and llsr_odometry_batch_odom
LLSR_HIDDEN int32_t odo_batch(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets, int32_t B,
                              const llsr_odom_sample* samples, const uint8_t* overwrite, void* hip_stream);
// Release every mapping-chain allocation (slot stores, engine, state); mp.live becomes false.
LLSR_HIDDEN void mapping_free(llsr_handle* h);
