/* llsr.h — C-ABI of the MI355X-native LeGO-LOAM-SR per-scan hot path.
 *
 * Drop-in boundary for the reference's ImageProjection → FeatureAssociation handoff
 * (LeGO-LOAM/src/imageProjection.cpp:189-222 cloudHandler, featureAssociation.cpp:2742-2778
 * runFeatureAssociation feature stage; stage types utility.h:63-83, cloud_msgs/msg/CloudInfo.msg).
 * The reference has no FFI of its own; these entry points replace the arithmetic behind the
 * node callbacks so a ROS2 shim keeps every topic and the Channel semantics.
 *
 * Conventions: plain C types only; int status codes (0 = OK, negative errno-style);
 * llsr_last_error() gives text; no C++ exception crosses the ABI. A handle is single-threaded
 * (one per pipeline/stream), matching the reference's one-thread-per-node layout.
 * Caller owns every host buffer; device buffers live in the handle.
 */
#ifndef LLSR_H_
#define LLSR_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on every change of a struct layout or entry-point signature. Version 2: llsr_map_config
 * gained enable_loop_closure and surrounding_keyframe_search_num (5 floats -> 5 floats + 2 int32),
 * so a caller built against version 1 would pass a struct the library reads past. A consumer checks
 * llsr_abi_version() == LLSR_ABI_VERSION once after loading the library. */
#define LLSR_ABI_VERSION 2

/* LLSR_ABI_VERSION as compiled into the loaded library. */
int32_t llsr_abi_version(void);
/* 16 hex digits identifying the kernel sources the library was built from (a hash of them): the
 * performance records under profiles/ name the build they measured. */
const char* llsr_build_id(void);

#define LLSR_OK 0
#define LLSR_EINVAL (-22)
#define LLSR_ENOMEM (-12)
#define LLSR_ENODEV (-19)
#define LLSR_ERANGE (-34)
#define LLSR_ENOSYS (-38)
#define LLSR_EIO (-5)

#define LLSR_LIDAR_VLP16 0
#define LLSR_LIDAR_VLP32C 1
#define LLSR_LIDAR_HDL64E 2

#define LLSR_MODE_FAITHFUL 0
#define LLSR_MODE_LM_APPLIED 1

/* Mirrors the ROS2 parameters of the three nodes (loam_config.yaml:1-67 / 69-135 / 137-203;
 * read at imageProjection.cpp:80-121, featureAssociation.cpp:112-154). Angles in degrees,
 * exactly as in the YAML; the library applies the reference's conversions. */
typedef struct llsr_config {
  int32_t num_vertical_scans;      /* laser.num_vertical_scans   (H)          */
  int32_t num_horizontal_scans;    /* laser.num_horizontal_scans (W)          */
  float vertical_angle_bottom;     /* deg */
  float vertical_angle_top;        /* deg */
  float sensor_mount_angle;        /* deg (read but unused by groundRemovalOurs) */
  int32_t ground_scan_index;
  int32_t use_kitti;               /* ground angle D = 60/25 deg by row (IP:561-566) */
  int32_t use_vlp32c;              /* rows by observed-elevation rank (IP:349-427), see below */
  float segment_theta;             /* deg */
  int32_t segment_valid_point_num;
  int32_t segment_valid_line_num;
  float scan_period;               /* s */
  float edge_threshold;
  float surf_threshold;
  float nearest_feature_search_distance;
  float DBFr;
  float RatioXY;
  float RatioZ;
  int32_t mapping_frequency_divider;
  int32_t iterCountThres;          /* map_optimization.mapping.iterCountThres */
  float step_size;
  float stop_thres;
  int32_t mode;                    /* LLSR_MODE_* */
} llsr_config;

/* Configurations llsr_create refuses with LLSR_EINVAL, before it looks for a device: those for
 * which the reference's arithmetic defines no result.
 *  - num_vertical_scans outside 2..64 or num_horizontal_scans outside 16..2048;
 *  - a float field that is not finite (NaN or +-Inf), whichever field it is;
 *  - vertical_angle_top <= vertical_angle_bottom: the vertical resolution is 0 or negative, and the
 *    row formula divides by it (IP:117-121, 313-316);
 *  - scan_period <= 0;
 *  - segment_theta outside the open interval (0, 90) deg: tan() of it is the segmentation
 *    threshold (IP:849);
 *  - use_vlp32c with more than 512 elevation bins (below).
 * Every other value is accepted and computes what the reference's code computes with it:
 * ground_scan_index >= num_vertical_scans (no row lies above it: no outlier), thresholds of 0 or
 * below, segment_valid_point_num above 30 (the line test is then dead), use_kitti on any H. */

/* use_vlp32c (IP:349-427, 567-568). A point's row is not computed from its elevation: every
 * finite point of the scan falls into the 0.335 deg elevation bin
 *   temp = int((asinf(z / range) + ang_bottom) / (0.335 * DEG_TO_RAD)),
 * before any column or range test, and the row of a point with temp >= 0 is the RANK of its bin
 * among the distinct non-negative bins observed in this scan (vertical_raw2, llsr_row_bins). Points
 * with temp < 0 are skipped; the column and range < 0.1 tests follow as in the plain branch. The
 * ground column test takes D = 25 deg on every row unless use_kitti is set too, which is tested
 * first (D = 60 / 25 deg by row). Two cases the reference leaves undefined are defined here:
 *  1. Overflow. The reference has no row < num_vertical_scans test and writes out of bounds when a
 *     scan shows more than H distinct bins. Here a point whose rank is >= H is dropped and claims
 *     no cell; llsr_row_bins reports n_bins > H for that scan.
 *  2. range == 0. z / range is NaN and its conversion to int is undefined; temp is defined as
 *     negative (what x86-64's cvttsd2si gives): the point sets no bin and is skipped.
 * The bin count is bounded by the configuration (344 for the shipped block); llsr_create returns
 * LLSR_EINVAL when the bound exceeds 512. The reference's std::cout per point (IP:400) is not
 * reproduced. */

/* Fill *cfg with the YAML block for `lidar` (LLSR_LIDAR_VLP16 / LLSR_LIDAR_VLP32C /
 * LLSR_LIDAR_HDL64E). */
int32_t llsr_config_default(llsr_config* cfg, int32_t lidar);

/* The less-flat VoxelGrid of the feature stage (surfPointsLessFlatScan, FA:1268-1270) averages
 * each 0.2 m voxel's points. PCL sums them in the order std::sort leaves its index_vector (equal
 * voxel ids in libstdc++ introsort's order); the default, LLSR_VOXEL_ORDER_PCL, reproduces that
 * exactly (each ring's workgroup runs the introsort, partitions level by level). The opt-in
 * LLSR_VOXEL_ORDER_INPUT sums each voxel in ring order instead (a centroid may differ from PCL's in
 * the last bits when its voxel holds three or more points; voxel set, count and order are the
 * same), and the difference reaches the next scan's laserCloudSurfLast and so every later pose.
 * MapOptimization's VoxelGrids (llsr_map_*, llsr_mapping_*) always follow PCL's order. */
#define LLSR_VOXEL_ORDER_INPUT 0
#define LLSR_VOXEL_ORDER_PCL 1

/* Per-scan outputs of projection+segmentation (IP) and feature extraction (FA), in the
 * reference's own order. Host buffers, caller-allocated; capacities from llsr_query_sizes().
 * Any pointer may be NULL to skip that output. Counts are always written. */
typedef struct llsr_scan_out {
  /* ---- ImageProjection (IP) ---- */
  int32_t n_points;            /* finite input points (after removeNaNFromPointCloud, IP:198) */
  float orientation[3];        /* start, end, diff (CloudInfo.msg:6-8; IP:430-445) */
  float* range_image;          /* [H*W] _range_mat, FLT_MAX where empty (IP:337)          */
  int32_t* cell_point;         /* [H*W] raw-input index of the point kept in the cell, -1  */
  int8_t* ground_image;        /* [H*W] _ground_mat after groundRemovalOurs (IP:522-774)  */
  int32_t* label_image;        /* [H*W] _label_mat after cloudSegmentation (IP:776-931)   */
  int32_t* start_ring_index;   /* [H] CloudInfo.start_ring_index (IP:794)                 */
  int32_t* end_ring_index;     /* [H] CloudInfo.end_ring_index   (IP:831)                 */
  int32_t n_segmented;         /* S */
  float* seg_xyzi;             /* [4*S] _segmented_cloud (intensity = row + col/1e4)      */
  uint8_t* seg_ground_flag;    /* [S] CloudInfo.segmented_cloud_ground_flag               */
  uint32_t* seg_col_ind;       /* [S] CloudInfo.segmented_cloud_col_ind                   */
  float* seg_range;            /* [S] CloudInfo.segmented_cloud_range                     */
  float* seg_intensity;        /* [S] ProjectionOut.segmentedCloud_Intensity              */
  int32_t n_outlier;           /* O */
  float* outlier_xyzi;         /* [4*O] _outlier_cloud                                    */
  float* outlier_intensity;    /* [O] ProjectionOut.outlierCloud_Intensity                */
  int32_t n_near;              /* nearground_cloud size K (IP:700-715)                    */
  int32_t n_ransac_inliers;    /* RANSAC inliers (IP:716-721)                             */
  int32_t ransac_iterations;   /* PCL iterations_ after computeModel                      */
  /* ---- FeatureAssociation feature stage (FA:2766-2775) ---- */
  float* loam_xyzi;            /* [4*S] segmentedCloud after adjustDistortion (FA:565-789) */
  float* curvature;            /* [S] cloudCurvature, defined on [5, S-5) (FA:817-848)     */
  uint8_t* picked;             /* [S] cloudNeighborPicked after extractFeaturesOurs         */
  int8_t* label;               /* [S] cloudLabel after extractFeaturesOurs                  */
  int32_t n_less_sharp;        /* M */
  int32_t* less_sharp_ind;     /* [M] cornerPointsLessSharp as segmented indices           */
  int32_t* dbscan_cluster;     /* [M] DBSCAN_EdgeFeature cluster labels (FA:1318-1387)      */
  int32_t n_sharp;
  int32_t* sharp_ind;          /* cornerPointsSharp as segmented indices (FA:1299-1305)     */
  int32_t n_flat;              /* surfPointsFlat WITHOUT the 160 shadow points               */
  int32_t* flat_ind;           /* segmented indices; shadow points follow implicitly         */
  int32_t n_less_flat;
  float* less_flat_xyzi;       /* [4*L] surfPointsLessFlat (per-ring VoxelGrid 0.2, FA:1268) */
} llsr_scan_out;

/* Result of one scan-to-map optimisation (MapOptimization::scan2MapOptimization, MO:1572-1610). */
typedef struct llsr_lm_report {
  int32_t iterations;     /* iter_num (MO:1581): 200 in faithful mode unless iteration 0 converges */
  int32_t converged;      /* LMOptimization returned true */
  int32_t degenerate;     /* isDegenerate (MO:1518-1529) */
  float min_lambda;       /* smallest eigenvalue of J^T J at iteration 0 (MO:1515) */
  float cf_mean;          /* mean |residual| of the last evaluated iteration (MO:1560/1568) */
  int32_t n_corner_corr;  /* corner / surf correspondences kept at the last iteration */
  int32_t n_surf_corr;
  float matX0[6];         /* the iteration-0 step matX (faithful-mode parity target) */
  float pose[6];          /* final transformTobeMapped */
  float ms;               /* wall/device time of the optimisation, ms */
} llsr_lm_report;

typedef struct llsr_sizes {
  int32_t cells;               /* H*W: bound for every per-point array */
  int32_t rings;               /* H */
  int32_t max_points;          /* input points per scan accepted by the handle */
  int32_t shadow_points;       /* 160 virtual points (FA:412-450) */
} llsr_sizes;

typedef struct llsr_handle llsr_handle;
/* The configuration a handle was created with (e.g. iterCountThres for a host loop that drives
 * the llsr_scan2map_shard_* steps itself). */
int32_t llsr_get_config(const llsr_handle* h, llsr_config* cfg);

/* Create a handle on HIP device `hip_device` able to process batches of up to `max_batch`
 * scans of up to `max_points` raw points each. Fails with LLSR_ENODEV when no device or the
 * HIP kernels are unavailable — there is no CPU fallback behind this ABI. */
int32_t llsr_create(const llsr_config* cfg, int32_t hip_device, int32_t max_batch,
                    int32_t max_points, llsr_handle** out);
void llsr_destroy(llsr_handle* h);
const char* llsr_last_error(const llsr_handle* h);
int32_t llsr_query_sizes(const llsr_handle* h, llsr_sizes* out);
/* Reset the per-slot FeatureAssociation carry-over state (FA:167-198: the H*W arrays that the
 * reference sizes once and never clears). */
int32_t llsr_reset_state(llsr_handle* h);
/* LLSR_VOXEL_ORDER_PCL (default) or LLSR_VOXEL_ORDER_INPUT for the less-flat VoxelGrid; takes
 * effect from the next batch. */
int32_t llsr_set_voxel_order(llsr_handle* h, int32_t order);

/* One scan, host buffers in/out: the ImageProjection::cloudHandler + FeatureAssociation
 * feature-stage replacement. `xyzi` holds n raw points (x,y,z,intensity, NaN allowed). */
int32_t llsr_process_scan(llsr_handle* h, const float* xyzi, int32_t n, llsr_scan_out* out);

/* Batched, device-resident: scans b = 0..B-1 are d_xyzi[d_offsets[b] .. d_offsets[b+1]),
 * float4 records in HBM (B+1 int64 offsets, also in device memory). Slot b uses FA carry-over
 * state b. Enqueued on `hip_stream` (hipStream_t); NULL selects the handle's own stream, which is
 * created non-blocking — it does NOT synchronise with the legacy default stream, so a caller that
 * filled d_xyzi on the default stream must pass that stream (or synchronise) itself. Returns after
 * enqueue. Batches of one handle are ordered even across streams (each waits for the previous
 * one's completion event), because they share the slot buffers and the FA carry-over state.
 * d_xyzi and d_offsets must stay valid and unchanged until the batch has completed: the kernels
 * read them while they run.
 * Results stay in the handle until the next call. */
int32_t llsr_process_batch(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets,
                           int32_t B, void* hip_stream);

/* Copy slot b's results of the last batch into host buffers (synchronises the stream). */
int32_t llsr_fetch_scan(llsr_handle* h, int32_t b, llsr_scan_out* out);

/* ImageProjection's visualization topics for slot b of the last batch (publishClouds,
 * imageProjection.cpp:933-967), built on the device from the slot's range image, kept points,
 * ground and label images, then copied to the caller's host buffers (each may be NULL: skipped):
 *   full_cloud / full_info_cloud  [H*W][4]  /full_cloud (IP:54), /full_cloud_info: per cell
 *       x, y, z with intensity row + col / 1e4 resp. the range (IP:337-347); resetParameters'
 *       nanPoint (NaN x, y, z, intensity 0) where no point landed (IP:170-179)
 *   ground / nonground / unknownground_cloud  [<= H*W][4]  the full-cloud points of the cells
 *       whose final ground_mat is 1 / 0 / 2, row-major (IP:760-769)
 *   segmented_cloud_pure  [<= H*W][4]  cells with 0 < label != 999999, intensity = label,
 *       row-major (IP:833-842)
 * The n_* fields receive the four clouds' sizes. Synchronises. */
typedef struct llsr_vis_out {
  float* full_cloud;
  float* full_info_cloud;
  float* ground_cloud;
  float* nonground_cloud;
  float* unknownground_cloud;
  float* segmented_cloud_pure;
  int32_t n_ground;
  int32_t n_nonground;
  int32_t n_unknownground;
  int32_t n_segmented_pure;
} llsr_vis_out;
int32_t llsr_fetch_vis_clouds(llsr_handle* h, int32_t b, llsr_vis_out* out);

/* Device-side counters of the last batch: per slot {n_points, S, O, M, n_sharp, F, L, K}.
 * `out` must hold 8*B int32 (host). Synchronises. */
int32_t llsr_batch_counts(llsr_handle* h, int32_t* out);

/* use_vlp32c handles: slot b's vertical_raw2 of the last batch (IP:366-369), the ascending
 * distinct elevation bins its finite points fell into. *n_bins receives their number (more than
 * num_vertical_scans: the scan overflowed, see use_vlp32c above) and bins[0 .. min(cap, *n_bins))
 * the bin numbers; bins may be NULL when cap is 0. LLSR_EINVAL on a handle without use_vlp32c.
 * Synchronises. */
int32_t llsr_row_bins(llsr_handle* h, int32_t b, int32_t* n_bins, int32_t* bins, int32_t cap);

/* Per-kernel device time (ms per batch, averaged over every batch enqueued since profiling was
 * enabled) from HIP events recorded on each batch's launch stream between its kernels, in the
 * order of llsr_kernel_name(k); k_row_bins, the last name, is written by use_vlp32c handles only.
 * Synchronises. Returns the number of kernels written (<= cap). */
int32_t llsr_kernel_times_ms(llsr_handle* h, float* out, int32_t cap);
const char* llsr_kernel_name(int32_t k);
/* Enable/disable per-kernel event timing; (re)enabling clears the accumulated averages. */
int32_t llsr_set_profiling(llsr_handle* h, int32_t enable);

/* ---- FeatureAssociation scan-to-scan LM (updateTransformation, featureAssociation.cpp:2505-2535) ----
 * Two-step LM between consecutive scans: surf phase (rx, rz, ty; FA:1699-2010) then corner
 * phase (ry, tx, tz; FA:1580-1697, 2013-2143), each <= 100 iterations, kNN-1 + ring-constrained
 * neighbour search every 5th iteration. Inputs per scan (float4 x, y, z, intensity, LOAM frame):
 * cornerPointsSharp and surfPointsFlat (with the 160 shadow points, FA:1310-1314) of the
 * current scan; laserCloudCornerLast / laserCloudSurfLast of the previous one (after
 * TransformToEnd + shadow points, FA:2660-2712). */
typedef struct llsr_s2s_report {
  int32_t surf_iterations;    /* iterCount1 when the surf loop ended (index of the converged step, or 100) */
  int32_t corner_iterations;  /* iterCount2 likewise (the reference's odometry_itertimes, FA:2800) */
  int32_t n_surf_corr;        /* correspondences at the last evaluated iteration of each phase */
  int32_t n_corner_corr;
  int32_t degenerate;         /* isDegenerate after the call (member state, FA:1975-1980) */
  int32_t skipped;            /* 1: last clouds too small, transformCur untouched (FA:2506) */
  float transform_cur[6];     /* rx, ry, rz, tx, ty, tz after updateTransformation */
  float ms;
} llsr_s2s_report;

/* The 160 virtual shadow points of GenerateShadowPoint (FA:412-439), float4 [160]. */
int32_t llsr_shadow_points(float* out_xyzi);

typedef struct llsr_s2s_batch {
  int32_t n_problems;
  const float* sharp;       const int64_t* sharp_off;        /* cornerPointsSharp */
  const float* flat;        const int64_t* flat_off;         /* surfPointsFlat + shadow points */
  const float* corner_last; const int64_t* corner_last_off;  /* laserCloudCornerLast */
  const float* surf_last;   const int64_t* surf_last_off;    /* laserCloudSurfLast */
  float* transform_cur;     /* [P][6] in/out */
  int32_t* is_degenerate;   /* [P] in/out (member state) */
  llsr_s2s_report* report;  /* [P] out (device memory) */
} llsr_s2s_batch;

/* Size the scan-to-scan buffers (problems per batch, points per cloud). */
int32_t llsr_scan2scan_reserve(llsr_handle* h, int32_t max_problems, int32_t max_sharp, int32_t max_flat,
                               int32_t max_corner_last, int32_t max_surf_last);
/* Enqueue a batch on `hip_stream` (NULL: the handle's own non-blocking stream); fully asynchronous: every
 * iteration runs inside one kernel. LLSR_ERANGE is reported by a later call's check of the
 * device error flag (llsr_scan2scan_check) when a cloud exceeded the reservation. */
int32_t llsr_scan2scan_batch(llsr_handle* h, const llsr_s2s_batch* batch, void* hip_stream);
/* Synchronise the last scan-to-scan batch and report capacity violations (LLSR_ERANGE). */
int32_t llsr_scan2scan_check(llsr_handle* h);
/* One scan from host buffers; reserves as needed; transform_cur / is_degenerate in/out. */
int32_t llsr_scan2scan(llsr_handle* h, const float* sharp, int32_t n_sharp, const float* flat, int32_t n_flat,
                       const float* corner_last, int32_t n_corner_last, const float* surf_last,
                       int32_t n_surf_last, float* transform_cur, int32_t* is_degenerate,
                       llsr_s2s_report* rep);


/* ---- MapOptimization scan-to-map (scan2MapOptimization, mapOptmization.cpp:1572-1610) ----
 * A batch of independent problems, one per scan: the scan's corner queries
 * (laserCloudCornerScanDS, MO:1244-1247) and surf queries (laserCloudSurfTotalLastDS,
 * MO:1259-1266), the corner / surf local maps (laserCloud{Corner,Surf}FromMapDS, MO:1225-1231)
 * and transformTobeMapped. Clouds are float4 rows (x, y, z, intensity) concatenated over the
 * batch with int64 offsets [P+1], all device-resident. The handle's config supplies
 * iterCountThres, step_size, stop_thres and mode (LLSR_MODE_FAITHFUL keeps the reference's
 * commented-out pose update, MO:1539-1545; LLSR_MODE_LM_APPLIED applies it). */
typedef struct llsr_s2m_batch {
  int32_t n_problems;
  const float* corner_q;   const int64_t* corner_q_off;
  const float* surf_q;     const int64_t* surf_q_off;
  const float* corner_map; const int64_t* corner_map_off;
  const float* surf_map;   const int64_t* surf_map_off;
  float* pose;               /* [P][6] in/out: roll, pitch, yaw, x, y, z (LOAM frame) */
  llsr_lm_report* report;    /* [P] out (device memory); report.ms is 0 in batch mode */
} llsr_s2m_batch;

/* Size the scan-to-map buffers: up to `max_problems` problems per batch with at most the given
 * points per cloud. Replaces MO's per-scan kd-tree allocation (MO:1575-1576). */
int32_t llsr_scan2map_reserve(llsr_handle* h, int32_t max_problems, int32_t max_corner_map,
                              int32_t max_surf_map, int32_t max_corner_q, int32_t max_surf_q);
/* Run the batch on `hip_stream` (NULL: the handle's own non-blocking stream). The LM's iteration count is data
 * dependent, so the call waits on the stream every few iterations to stop once every problem
 * has converged or reached iterCountThres; it returns when the batch is complete.
 * LLSR_ERANGE: a cloud exceeds the reserved capacity (nothing written for that problem). */
int32_t llsr_scan2map_batch(llsr_handle* h, const llsr_s2m_batch* batch, void* hip_stream);
/* Device time of the scan-to-map batches run since profiling was (re)enabled
 * (llsr_set_profiling), from HIP events on the launch stream. */
typedef struct llsr_s2m_stats {
  int32_t batches;
  int32_t iteration_launches;  /* k_s2m_iter launches, summed over batches */
  float grid_ms;               /* setup + cell-table build, summed */
  float iterate_ms;            /* first to last LM launch incl. the host's convergence polls, summed */
} llsr_s2m_stats;
int32_t llsr_scan2map_stats(llsr_handle* h, llsr_s2m_stats* out);
/* Device time of the scan-to-scan batches (llsr_scan2scan_batch, and the LM inside
 * llsr_odometry_batch) run since profiling was (re)enabled, from HIP events on the launch stream.
 * Profiling syncs the stream after each batch. */
typedef struct llsr_s2s_stats {
  int32_t batches;
  int32_t reserved;
  float grid_ms; /* cell grids of the last clouds (kd-tree build, FA:2313-2314), summed */
  float lm_ms;   /* k_s2s_lm: both LM phases of every problem (FA:2505-2535), summed */
} llsr_s2s_stats;
int32_t llsr_scan2scan_stats(llsr_handle* h, llsr_s2s_stats* out);
/* ---- Split-correspondence scan-to-map for multi-GPU (BASELINE.json configs[4]) ----
 * The optimisation of llsr_scan2map_batch driven one LM iteration at a time, so that the
 * per-problem normal equations can be summed across GPUs between the Jacobian build and the
 * solve. Rank r of W evaluates only its share of every problem's queries (256-query blocks b of
 * each kind with b % W == r) and writes int64 fixed-point partial sums, LLSR_NE_WORDS per
 * problem: AtA upper triangle (21, row-major), AtB (6), sum |coeff.intensity|, #corner, #surf
 * correspondences, 2 spare; every term is rounded once to a multiple of 2^-30 before it is
 * added. Range: a term must satisfy |v| < 2^32 and the sums stay exact while sum |term| < 2^33 per
 * word (e.g. 20k correspondences with |J|^2 up to 4e5, points ~600 m away); a non-finite or
 * out-of-range term contributes 0, is counted, and the step returns LLSR_ERANGE. Integer sums are associative, so the summed words, and therefore every pose, are
 * bit-identical for any W and any all-reduce order (they differ from llsr_scan2map_batch's float
 * sums only by that rounding: well inside the 1e-4 pose tolerance). Per batch:
 *   llsr_scan2map_shard_begin(h, batch, stream)              (reserve as for llsr_scan2map_batch)
 *   up to iterCountThres times:
 *     llsr_scan2map_shard_partial(h, r, W, d_ne, stream)     d_ne: int64 [P][LLSR_NE_WORDS], device
 *     the caller sums d_ne over the W ranks in place (e.g. an RCCL all-reduce on `stream`)
 *     llsr_scan2map_shard_step(h, d_ne, &n_active, stream)   n_active NULL: no host sync
 *     stop once n_active == 0 (every rank sees the same count: no extra collective)
 *   llsr_scan2map_shard_end(h, stream)                        pose + report into the batch arrays
 * A handle holds one scan-to-map batch at a time (llsr_scan2map_batch / llsr_scan2map close an
 * open shard batch). */
#define LLSR_NE_WORDS 32
int32_t llsr_scan2map_shard_begin(llsr_handle* h, const llsr_s2m_batch* batch, void* hip_stream);
int32_t llsr_scan2map_shard_partial(llsr_handle* h, int32_t rank, int32_t world, int64_t* d_ne, void* hip_stream);
int32_t llsr_scan2map_shard_step(llsr_handle* h, const int64_t* d_ne, int32_t* n_active, void* hip_stream);
int32_t llsr_scan2map_shard_end(llsr_handle* h, void* hip_stream);

/* One problem from host buffers (the reference's call shape: scan2MapOptimization on the
 * member clouds); reserves as needed; `pose` in/out; rep->ms = device time. */
int32_t llsr_scan2map(llsr_handle* h, const float* corner_q, int32_t n_corner_q, const float* surf_q,
                      int32_t n_surf_q, const float* corner_map, int32_t n_corner_map,
                      const float* surf_map, int32_t n_surf_map, float* pose, llsr_lm_report* rep);


/* ---- End-to-end odometry (runFeatureAssociation, featureAssociation.cpp:2742-2853) ----
 * B independent sequences (slots). Each call consumes one device-resident scan per slot (as
 * llsr_process_batch) and runs, without leaving the device: the ImageProjection + feature stage,
 * then updateTransformation against the slot's last clouds (FA:2505-2535), integrateTransformation
 * (FA:2537-2568, transformSum) and publishCloudsLast (FA:2660-2717): TransformToEnd of the
 * less-sharp / less-flat clouds, which become the slot's last clouds (+ the 160 shadow points on
 * the surf side), and of the sharp / flat clouds (MapOptimization's scan inputs). A slot's first
 * scan runs checkSystemInitialization (FA:2291-2315) instead. transformCur carries over to the
 * next scan as the LM's initial guess. Requires LLSR_MODE_LM_APPLIED (LLSR_ENOSYS otherwise): in
 * the faithful mode updateInitialGuess (FA:2790) overwrites transformCur from the /odom2 topic,
 * which has no input here (llsr_odometry_batch_odom below takes it). One host sync per call (the
 * feature counts size the packed clouds). */
typedef struct llsr_odom_slot {
  int32_t frames;            /* scans this slot has consumed */
  int32_t n_corner_last;     /* laserCloudCornerLastNum after the last scan */
  int32_t n_surf_last;       /* laserCloudSurfLastNum (incl. the 160 shadow points) */
  int32_t n_corner_scan;     /* laserCloudCornerScan = TransformToEnd(cornerPointsSharp); 0 on frame 1 */
  int32_t n_surf_scan;       /* laserCloudSurfScan = TransformToEnd(surfPointsFlat + shadow); 0 on frame 1 */
  float transform_cur[6];    /* transformCur after updateTransformation */
  float transform_sum[6];    /* transformSum after integrateTransformation */
  llsr_s2s_report lm;        /* the last scan's updateTransformation (skipped = 1 on frame 1) */
} llsr_odom_slot;
int32_t llsr_odometry_batch(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets, int32_t B,
                            void* hip_stream);
/* Slot b's state after the last call; the float4 cloud buffers (host, may be NULL) receive the
 * last clouds and the scan clouds (capacity H*W + 160 points each). Synchronises. */
int32_t llsr_odometry_fetch(llsr_handle* h, int32_t b, llsr_odom_slot* out, float* corner_last, float* surf_last,
                            float* corner_scan, float* surf_scan);
/* Start every slot over: transformCur / transformSum = 0, no last clouds, FA carry-over reset. */
int32_t llsr_odometry_reset(llsr_handle* h);

/* ---- MapOptimization local map (llsr_map.hip) ----
 * The keyframe store of saveKeyFramesAndFactor (MO:1686-1752) kept in HBM, the local-map assembly
 * of extractSurroundingKeyFrames (MO:1096-1231, both branches: the key-pose radius search of the
 * VLP-16 block, enable_loop_closure false at CFG:23, and the recent-keyframe queue of the VLP-32c /
 * HDL-64E blocks, enable_loop_closure true at CFG:91, 159) and the downSizeFilter* VoxelGrids
 * (MO:92-104; downsampleCurrentScan MO:1234-1267), on the device. A llsr_map is independent of any
 * llsr_handle, one per mapped sequence; it owns a non-blocking stream used when hip_stream is NULL.
 * Point clouds are float4 x, y, z, intensity. VoxelGrid = pcl::VoxelGrid<PointXYZI>::filter
 * (downsample_all_data, 0 min points): same voxel set and output order (ascending voxel index) as
 * PCL, each centroid summed in the order libstdc++'s std::sort leaves PCL's index_vector. */
typedef struct llsr_map llsr_map;
typedef struct llsr_map_config {
  float surrounding_radius;  /* surrounding_keyframe_search_radius, 50 m (CFG:26) */
  float keypose_leaf;        /* downSizeFilterSurroundingKeyPoses, 1.0 (MO:99) */
  float corner_leaf;         /* downSizeFilterCorner, 0.2 (MO:92) */
  float surf_leaf;           /* downSizeFilterSurf, 0.4 (MO:93) */
  float outlier_leaf;        /* downSizeFilterOutlier, 0.4 (MO:94) */
  /* mapping.enable_loop_closure (CFG:23 / 91 / 159). Non-zero selects the branch of
   * extractSurroundingKeyFrames at MO:1099-1151: the local map is the last
   * surrounding_keyframe_search_num keyframes, refilled from the newest backwards while the queue
   * is short, then one pop-oldest / push-newest per call whenever the newest keyframe index changed
   * (latestFrameID, MO:1126-1134). The loop-closure ICP thread itself is commented out in the
   * reference (MO:174), so this flag changes only the local map. */
  int32_t enable_loop_closure;
  int32_t surrounding_keyframe_search_num;  /* 50 (CFG:27 / 95 / 163) */
} llsr_map_config;
/* VLP-16 block: radius branch (enable_loop_closure 0), search num 50, the leaves above. */
int32_t llsr_map_config_default(llsr_map_config* cfg);
/* The block of loam_config.yaml for `lidar` (LLSR_LIDAR_VLP16: CFG:20-27; LLSR_LIDAR_VLP32C:
 * CFG:88-95 and LLSR_LIDAR_HDL64E: CFG:156-163, both enable_loop_closure 1). */
int32_t llsr_map_config_lidar(llsr_map_config* cfg, int32_t lidar);
llsr_map* llsr_map_create(const llsr_map_config* cfg, int32_t hip_device);
void llsr_map_destroy(llsr_map* m);
const char* llsr_map_last_error(const llsr_map* m);
/* Drop every keyframe and the surrounding-keyframe list. */
int32_t llsr_map_reset(llsr_map* m);
/* VoxelGrid of S independent clouds packed in d_in (device float4); off[S+1] and leaf[S] are host
 * arrays; d_out (device, capacity off[S] points) receives the S results packed, out_off[S+1]
 * (host) their offsets. Synchronises hip_stream. */
int32_t llsr_map_voxel_grid(llsr_map* m, const float* d_in, const int64_t* off, int32_t S, const float* leaf,
                            float* d_out, int64_t* out_off, void* hip_stream);
/* downsampleCurrentScan (MO:1234-1267). Inputs (device float4): laserCloudCornerLast, SurfLast,
 * OutlierLast, CornerScan, SurfScan. d_out (capacity n_cl + n_sl + n_ol + n_cs + n_ss + n_sl +
 * n_ol points) receives, packed in this order: CornerLastDS (corner leaf), SurfLastDS (surf leaf),
 * OutlierLastDS (outlier leaf), CornerScanDS, SurfScanDS, SurfTotalLastDS (= surf leaf over
 * SurfLastDS + OutlierLastDS); out_off[7] (host) their offsets. Synchronises. */
int32_t llsr_map_downsample_scan(llsr_map* m, const float* corner_last, int32_t n_cl, const float* surf_last,
                                 int32_t n_sl, const float* outlier_last, int32_t n_ol, const float* corner_scan,
                                 int32_t n_cs, const float* surf_scan, int32_t n_ss, float* d_out, int64_t* out_off,
                                 void* hip_stream);
/* saveKeyFramesAndFactor's store (MO:1686-1752): key pose x, y, z, roll, pitch, yaw (PointTypePose;
 * cloudKeyPoses3D = x, y, z with intensity = the returned keyframe index) and the keyframe's corner
 * (laserCloudCornerScan), surf (SurfLastDS) and outlier (OutlierLastDS) clouds, copied into the
 * store (device or host pointers). Returns the index (>= 0) or an error. */
int32_t llsr_map_add_keyframe(llsr_map* m, const float pose[6], const float* corner, int32_t n_corner,
                              const float* surf, int32_t n_surf, const float* outlier, int32_t n_outlier,
                              void* hip_stream);
int32_t llsr_map_num_keyframes(const llsr_map* m);
typedef struct llsr_map_report {
  int32_t n_in_radius;     /* key poses within surrounding_radius (MO:1157-1164); 0 with loop closure */
  int32_t n_poses_ds;      /* surroundingKeyPosesDS size (MO:1166-1167); 0 with loop closure */
  int32_t n_keyframes;     /* surroundingExistingKeyPosesID size after the update (loop closure:
                              recentCornerCloudKeyFrames size) */
  int32_t n_transformed;   /* keyframes newly added to the list this call (MO:1205-1220; loop
                              closure: pushed onto the queue, MO:1115-1120 / 1138-1143) */
  int64_t n_corner_map;    /* laserCloudCornerFromMap before / after VoxelGrid */
  int64_t n_surf_map;      /* laserCloudSurfFromMap (surf + outlier keyframe clouds) */
  int64_t n_corner_ds;
  int64_t n_surf_ds;
  float ms;                /* wall time of the call */
} llsr_map_report;
/* extractSurroundingKeyFrames (MO:1096-1232) around robot_pos (currentRobotPosPoint = x, y, z of
 * transformAftMapped; unused with loop closure): the corner / surf local maps (…FromMapDS) into
 * d_corner / d_surf (device, capacities in points; LLSR_ERANGE with the sizes in rep when they do
 * not fit). Synchronises. */
int32_t llsr_map_extract(llsr_map* m, const float robot_pos[3], float* d_corner, int64_t cap_corner, float* d_surf,
                         int64_t cap_surf, llsr_map_report* rep, void* hip_stream);
/* surroundingExistingKeyPosesID (loop closure: the queue's keyframe indices, oldest first) after the
 * last extract; returns its length. */
int32_t llsr_map_keyframe_ids(const llsr_map* m, int32_t* out, int32_t cap);

/* ---- The global map: publishGlobalMap (MO:775-892) and saveMapService (MO:344-434) ----
 * MapOptimization's third thread (publishGlobalMapThread, MO:305-315) and its end-of-run product, on
 * the map's keyframe store. publishGlobalMap, in program order:
 *  1. nothing happens without key poses (MO:780);
 *  2. kdtreeGlobalMap.radiusSearch around the robot with sorted results (nanoflann_pcl.h:113-116,
 *     165-167): key poses with d^2 = ((0 + dx^2) + dy^2) + dz^2 < float(double(r) * double(r)), in
 *     ascending d^2. Tie divergence (as for the kNN): among exactly equal d^2 the
 *     reference's order follows its kd-tree traversal and std::sort; here it is ascending key index;
 *  3. unless high_dense, VoxelGrid keypose_leaf of those poses (x, y, z, intensity = key index) —
 *     but `globalMapKeyPosesDS = globalMapKeyPoses` (MO:807) re-points the shared pointer, so the
 *     first call's filter output lands in an orphaned cloud and the raw sorted list is used; from
 *     the second call on both names are one cloud, pcl::Filter::filter works in place, and the
 *     downsampled poses are used;
 *  4. for every pose of that list, keyframe (int)intensity (after the filter: the voxel's mean key
 *     index, truncated; two voxels may name one keyframe, which is then appended twice):
 *     edge += corner, planar += surf, global += corner, surf, outlier (transformPointCloud);
 *  5. unless high_dense, VoxelGrid cloud_leaf of the global cloud, with the same pointer behaviour
 *     (MO:836): raw on the first call, downsampled later; PCL returns its input unchanged when the
 *     voxel-extent product exceeds INT32_MAX (`passthrough`), which a 5000 m radius at a 0.4 m
 *     leaf makes realistic;
 *  6. the published clouds are global, edge and planar; the latter two are never downsampled.
 * The call-to-call state is one counter per llsr_map: calls that returned LLSR_OK on a non-empty
 * store since llsr_map_create / llsr_map_reset (an empty store returns before the pointers move,
 * MO:780, and counts nothing). */
typedef struct llsr_global_map_config {
  float search_radius;    /* global_map_visualization_search_radius, 5000 (CFG:37) */
  float keypose_leaf;     /* downSizeFilterGlobalMapKeyPoses, 1.0 (MO:102) */
  float cloud_leaf;       /* downSizeFilterGlobalMapKeyFrames, 0.4 (MO:104) */
  int32_t high_dense;     /* HighDenseMapping (CFG:40): no VoxelGrid at all */
  int32_t first_call_raw; /* 1 = the reference's pointer behaviour (steps 3, 5);
                             0 = downsample on every call */
} llsr_global_map_config;
typedef struct llsr_global_map_report {
  int32_t call;           /* 1-based count of successful calls since create / reset (a refused or
                             empty-store call reports the count so far) */
  int32_t n_in_radius, n_poses_used;   /* used = list length of step 4, duplicates counted */
  int32_t downsampled_poses, downsampled_cloud, passthrough;  /* what steps 3 / 5 did; PCL overflow */
  int64_t n_edge, n_planar, n_global_raw, n_global;
  float ms;               /* wall time of the call */
} llsr_global_map_report;
/* The largest cloud the VoxelGrid engine takes (its point indices are 32-bit); a larger global or
 * surface cloud to downsample returns LLSR_ERANGE. */
#define LLSR_VOXEL_GRID_MAX_POINTS 2147483646
int32_t llsr_global_map_config_default(llsr_global_map_config* cfg);
/* Steps 1-6 around robot_pos (currentRobotPosPoint, MO:1613-1615); cfg NULL = the defaults. Outputs
 * are device float4 clouds, capacities in points; a NULL output with capacity 0 skips that cloud,
 * its count is still reported (for a downsampled global cloud the VoxelGrid then runs in the map's
 * scratch). When a requested capacity is too small the call returns LLSR_ERANGE with the sizes in
 * rep (n_global is the upper bound n_global_raw when the refusal came before the VoxelGrid ran),
 * leaves the outputs unspecified and does not advance the call counter, so a retry with larger
 * buffers gives the identical result. cap_global >= n_global_raw lets the VoxelGrid write straight
 * into d_global. Synchronises hip_stream. Uses the map's VoxelGrid scratch and assembly buffers:
 * must not overlap llsr_map_add_keyframe, llsr_map_extract or any other call on the same map. */
int32_t llsr_map_global(llsr_map* m, const llsr_global_map_config* cfg, const float robot_pos[3], float* d_global,
                        int64_t cap_global, float* d_edge, int64_t cap_edge, float* d_planar, int64_t cap_planar,
                        llsr_global_map_report* rep, void* hip_stream);
/* saveMapService's clouds in the save_key_feature_pcd == false branch every config block uses
 * (MO:382-395), over all keyframes in index order: cornerMap = the transformed corner clouds (raw,
 * as written); surfaceMap = per keyframe the transformed surf cloud then the outlier cloud, through
 * downSizeFilterSurf (the map's surf_leaf). Same output, capacity, LLSR_ERANGE (*n_surf then an
 * upper bound or the exact size) and overlap rules as llsr_map_global; no call-to-call state. */
int32_t llsr_map_save(llsr_map* m, float* d_corner, int64_t cap_corner, float* d_surf, int64_t cap_surf,
                      int64_t* n_corner, int64_t* n_surf, void* hip_stream);
/* Host-only (no device): the selection of step 2 over K poses (x, y, z, anything) into out_idx[K];
 * returns the count. */
int32_t llsr_keypose_radius_sorted(const float* poses4, int32_t K, const float pos[3], float radius,
                                   int32_t* out_idx);

/* ---- Loop closure: detectLoopClosure / performLoopClosure (MO:894-1094), correctPoses (MO:1757-1785) ----
 * The reference's loop-closure thread (started at the commented-out MO:174) up to the factor graph:
 * keyframe times, the candidate selection, the two submaps on the keyframe store, the ICP alignment on
 * the device (llsr_icp_align) and on the host (llsr_icp_align_host), the acceptance test, the pose
 * constraint, and the corrected poses coming back. llsr_map_loop_closure runs all of it in one call;
 * the pieces are entry points of their own. DESIGN.md §16 is the specification of the whole path (PCL
 * and Eigen are restated, not linked). The BetweenFactor and iSAM2 stay in the node, or the llsr_pg_*
 * calls below take their place. */
typedef struct llsr_loop_config {
  float search_radius;     /* history_keyframe_search_radius (CFG:29 / 97 / 165) */
  int32_t search_num;      /* history_keyframe_search_num (CFG:30 / 98 / 166) */
  float fitness_score;     /* history_keyframe_fitness_score (CFG:31 / 99 / 167) */
  float leaf;              /* downSizeFilterHistoryKeyFrames (MO:97) */
  double min_time_gap;     /* 30.0 s (MO:912) */
  int32_t icp_max_iterations;               /* 100 (MO:1001) */
  int32_t pad;
  double icp_transformation_epsilon;        /* 1e-6 (MO:1002) */
  double icp_fitness_epsilon;               /* 1e-6 (MO:1008) */
  double icp_max_correspondence_distance;   /* 100 (MO:1007) */
} llsr_loop_config;
/* The block of loam_config.yaml for `lidar` (VLP-16: 15 m, 50, 0.5; VLP-32c: 50 m, 40, 1.5;
 * HDL-64E: 30 m, 30, 0.8) and the constants of MO:97, 912, 1001-1008. */
int32_t llsr_loop_config_lidar(llsr_loop_config* cfg, int32_t lidar);
/* cloudKeyPoses6D[index].time in seconds (timeLaserOdometry of the keyframe's scan, MO:1709). A
 * keyframe whose time was never set holds NaN: fabs(NaN - now) > gap is false, so it is never a loop
 * candidate. llsr_map_keyframe_times copies the times of keyframes 0 .. min(cap, K) - 1 and returns K. */
int32_t llsr_map_set_keyframe_time(llsr_map* m, int32_t index, double seconds);
int32_t llsr_map_keyframe_times(const llsr_map* m, double* out, int32_t cap);
/* correctPoses (MO:1757-1785): overwrite the first n key poses (x, y, z, roll, pitch, yaw each, the
 * store's layout; the node applies the GTSAM axis remap of MO:1765-1780) and clear the recent-
 * keyframe queue (MO:1759-1761) and the radius branch's keyframe list, so the next llsr_map_extract
 * with enable_loop_closure refills from the newest keyframe backwards with the new poses; the global
 * map and llsr_map_save read the new poses too. LLSR_ERANGE when n exceeds the keyframe count. */
int32_t llsr_map_set_key_poses(llsr_map* m, const float* poses6, int32_t n);
/* Host-only (no device). The candidate of detectLoopClosure (MO:902-919) over K poses (x, y, z,
 * anything) and times[K]: the sorted radius search of llsr_keypose_radius_sorted, then the first hit
 * with fabs(times[k] - now) > gap in double; the keyframe index or -1. */
int32_t llsr_loop_candidate(const float* poses4, const double* times, int32_t K, const float pos[3], double now,
                            float radius, double gap);
/* Eigen::umeyama without scaling of n >= 1 correspondences src_xyz[3n] -> dst_xyz[3n]
 * into the row-major 4x4 T16: what one ICP iteration estimates. */
int32_t llsr_umeyama3(const float* src_xyz, const float* dst_xyz, int32_t n, float* T16);
/* The pose constraint of MO:1056-1081 from the ICP transformation, the latest and the closest key
 * pose (x, y, z, roll, pitch, yaw each) and the fitness score: pose_from = x, y, z, roll, pitch, yaw
 * of tCorrect (MO:1072), pose_to = z, x, y, yaw, roll, pitch of the closest key pose (MO:1076),
 * *variance = (float)fitness for all six variances (MO:1078-1081). */
int32_t llsr_loop_constraint(const float* T16, const float* pose_latest6, const float* pose_closest6, double fitness,
                             float* pose_from6, float* pose_to6, float* variance);
/* The alignment itself: pcl::IterativeClosestPoint with an identity guess (MO:1000-1017) as DESIGN.md
 * §16 specifies it. Clouds are [n][4] floats (x, y, z, intensity). `state` is the convergence state:
 * 0 none, 1 iterations, 2 transform, 3 absolute MSE, 4 relative MSE, 5 no correspondences (fewer
 * than 3 pairs: converged 0, T keeps its value). A point that finds no target (a NaN or beyond
 * +-1 048 000 m coordinate, an empty target) is in no pair and is not counted in the fitness mean;
 * fitness is DBL_MAX when no point counts. */
typedef struct llsr_icp_result {
  int32_t converged;      /* hasConverged() */
  int32_t state;          /* see above */
  int32_t iterations;     /* completed iterations */
  int32_t n_pairs_last;   /* correspondences kept in the last correspondence step */
  double fitness;         /* getFitnessScore() of the source moved by T */
  float T[16];            /* getFinalTransformation(), row-major 4x4 */
} llsr_icp_result;
#define LLSR_ICP_MAX_POINTS 100000000
/* Host-only (no device), serial: the same loop bodies the device alignment runs, over heap buffers.
 * aligned4 ([n_src][4], may be NULL) receives the source moved by T in one step (the pubIcpKeyFrames
 * cloud); it must not overlap the inputs. Uses cfg's icp_* fields. */
int32_t llsr_icp_align_host(const float* src4, int32_t n_src, const float* tgt4, int32_t n_tgt,
                            const llsr_loop_config* cfg, llsr_icp_result* res, float* aligned4);
/* The same alignment on device clouds (16-byte aligned, [n][4] floats). The workspace owns the
 * target's cell grid and the loop's buffers and grows them on demand; one call at a time per
 * workspace. d_aligned4 (device, [n_src][4], may be NULL) as above. The loop's state lives in device
 * memory; the host reads one state word per iteration and the result at the end. Synchronises
 * hip_stream (NULL: the workspace's own stream). llsr_icp_create returns NULL without a HIP device. */
typedef struct llsr_icp llsr_icp;
llsr_icp* llsr_icp_create(int32_t hip_device);
void llsr_icp_destroy(llsr_icp* w);
const char* llsr_icp_last_error(const llsr_icp* w);
int32_t llsr_icp_align(llsr_icp* w, const float* d_src4, int32_t n_src, const float* d_tgt4, int32_t n_tgt,
                       const llsr_loop_config* cfg, llsr_icp_result* res, float* d_aligned4, void* hip_stream);
/* P alignments in one set of launches (DESIGN.md §16 "Batch form"). The clouds are concatenated over
 * the batch as [n][4] float rows: problem p's source is points src_off[p] .. src_off[p + 1] - 1 of
 * d_src4, its target points tgt_off[p] .. tgt_off[p + 1] - 1 of d_tgt4. The clouds are on the device;
 * the offsets ([P + 1], in points, non-decreasing) are on the HOST, because the host sizes the
 * workspace from them. cfgs holds n_cfgs = 1 configuration shared by all problems or n_cfgs = P, one
 * per problem. res[p], and problem p's rows of d_aligned4 (laid out like d_src4 from src_off[0] on;
 * may be NULL), are bit for bit what llsr_icp_align gives for that problem alone. A problem that has
 * finished stays as it is while the others go on; the host reads one word per pass of the loop, and
 * the call makes at most max(1, largest icp_max_iterations) passes. LLSR_EINVAL: P < 1, decreasing
 * or negative offsets, n_cfgs not 1 or P, misaligned clouds; LLSR_ERANGE: a problem larger than
 * LLSR_ICP_MAX_POINTS, or more than 65535 problems. Every problem's grid is sized for the largest
 * target, so the workspace holds P times that. One call at a time per workspace; synchronises
 * hip_stream. */
int32_t llsr_icp_align_batch(llsr_icp* w, int32_t P, const float* d_src4, const int64_t* src_off,
                             const float* d_tgt4, const int64_t* tgt_off, const llsr_loop_config* cfgs, int32_t n_cfgs,
                             llsr_icp_result* res, float* d_aligned4, void* hip_stream);
/* Diagnostic: HIP-event times of the last llsr_icp_align or llsr_icp_align_batch on w, in ms: the
 * correspondence kernels and the solve kernels summed over the iterations (the batch: over the
 * passes, all problems together), and the whole call's device time. */
int32_t llsr_icp_last_times(const llsr_icp* w, float* corr_ms, float* solve_ms, float* total_ms);
/* Diagnostic: passes of the loop in the last llsr_icp_align_batch on w (0 before the first). */
int32_t llsr_icp_last_passes(const llsr_icp* w);
/* One detectLoopClosure + performLoopClosure on the keyframe store. */
typedef struct llsr_loop_report {
  int32_t found;            /* a candidate exists (0: an empty store or no candidate; nothing else is set) */
  int32_t closest_id;       /* closestHistoryFrameID, -1 without a candidate */
  int32_t latest_id;        /* latestFrameIDLoopCloure = the newest keyframe */
  int32_t accepted;         /* converged && fitness <= fitness_score (MO:1038-1040) */
  int64_t n_source;         /* latestSurfKeyFrameCloud after the intensity filter */
  int64_t n_target;         /* nearHistorySurfKeyFrameCloud before the VoxelGrid */
  int64_t n_source_ds;      /* both through downSizeFilterHistoryKeyFrames */
  int64_t n_target_ds;
  llsr_icp_result icp;      /* the alignment of the raw clouds (llsr_map_loop_closure only) */
  float pose_from[6];       /* the constraint of llsr_loop_constraint, when accepted */
  float pose_to[6];
  float variance;
  float ms;                 /* wall time of the call */
} llsr_loop_report;
/* The candidate (llsr_loop_candidate over the store's poses and times, robot_pos = currentRobotPosPoint,
 * now = timeLaserOdometry) and the two submaps (MO:920-981): source = the newest keyframe's corner
 * then surf cloud in the map frame, the points with (int)intensity >= 0 in order; target = keyframes
 * closest - search_num .. closest + search_num inside the store, corner then surf each; both also
 * through a VoxelGrid of cfg->leaf. Outputs are device float4 clouds with capacities in points, with
 * the rules of llsr_map_global: a NULL output with capacity 0 is skipped and its size still reported;
 * LLSR_ERANGE with the sizes in rep when a capacity is too small, nothing written, and a retry with
 * larger buffers gives the identical result. Changes no map state. Synchronises hip_stream; uses the
 * map's scratch, so it must not overlap another call on the same map. */
int32_t llsr_map_loop_submaps(llsr_map* m, const llsr_loop_config* cfg, const float robot_pos[3], double now,
                              llsr_loop_report* rep, float* d_source, int64_t cap_source, float* d_target,
                              int64_t cap_target, float* d_source_ds, int64_t cap_sds, float* d_target_ds, int64_t cap_tds,
                              void* hip_stream);
/* llsr_map_loop_submaps, then llsr_icp_align of the raw source onto the raw target (MO:1011-1012) in
 * the workspace w (NULL: one the map owns), the acceptance test and, when accepted, the constraint.
 * d_aligned receives the source moved by the final transformation (pubIcpKeyFrames /
 * pubIcpKeyFramesFalse) whether or not the result is accepted; d_target_ds the downsampled target
 * (pubHistoryKeyFrames). The node adds the BetweenFactor, runs iSAM2 and hands the corrected poses
 * back through llsr_map_set_key_poses. Same output, capacity, state and overlap rules as above. */
int32_t llsr_map_loop_closure(llsr_map* m, llsr_icp* w, const llsr_loop_config* cfg, const float robot_pos[3],
                              double now, llsr_loop_report* rep, float* d_aligned, int64_t cap_aligned,
                              float* d_target_ds, int64_t cap_tds, void* hip_stream);

/* ---- Mapping chain: ImageProjection -> FeatureAssociation -> MapOptimization::run ----
 * (mapOptmization.cpp:1854-1896.) Each llsr_mapping_batch call runs llsr_odometry_batch on the B
 * slots and then, for every slot that sends an AssociationOut this frame — FA counts the frames
 * after the first (the first scan sends nothing, FA:2781-2784) and sends on every
 * mapping_frequency_divider-th of them (FA:2818-2821; llsr_config.mapping_frequency_divider, 1 in
 * every config block; a value < 1 never sends, as in the reference) — OdometryToTransform of the published odometry
 * (tf2 round trip, FA:2612-2625 / utility.h:99-113), transformAssociateToMap (MO:458-581),
 * extractSurroundingKeyFrames on the slot's keyframe store (MO:1096-1232), downsampleCurrentScan
 * of the AssociationOut clouds (corner / surf last, the adjustOutlierCloud'ed IP outliers
 * FA:2600-2610, corner / surf scan; MO:1234-1267), scan2MapOptimization (MO:1572-1610: all slots
 * in one device batch, isDegenerate / matP carried per slot), transformUpdate (MO:583-589) and
 * saveKeyFramesAndFactor (MO:1612-1755; every frame is a keyframe there, saveThisKeyFrame is forced
 * true at MO:1629; the prior / between factors with the initial values as measurements leave
 * iSAM2's estimate at the initial values, so the key pose is transformTobeMapped for the first
 * keyframe and transformAftMapped after). llsr_mapping_batch requires the handle's mode
 * LLSR_MODE_LM_APPLIED (the odometry's; llsr_mapping_batch_odom runs either); `mo_mode` selects MapOptimization's own LM mode (LLSR_MODE_FAITHFUL: the pose
 * update at MO:1539-1545 stays commented out, as in the reference). map_cfg NULL selects the
 * config block of the handle's lidar (llsr_map_config_lidar: HDL-64E when num_vertical_scans is
 * 64, else VLP-16), which decides the local-map branch (enable_loop_closure). Synchronises per
 * call. An error from the MapOptimization part of a call (after the odometry advanced) leaves every
 * slot's MapOptimization members (poses, keyframes, local-map queue, LM members) as before the call. */
typedef struct llsr_mapping_slot {
  int32_t frames;               /* scans consumed by the slot (odometry frames) */
  int32_t mo_frames;            /* MapOptimization::run iterations = frames - 1 once frames >= 2 */
  int32_t keyframes;            /* cloudKeyPoses3D size */
  int32_t lm_ran;               /* the last frame's map passed MO:1573 (corner > 10, surf > 100) */
  float transform_sum[6];       /* OdometryToTransform of the last published odometry */
  float transform_tobe_mapped[6];
  float transform_bef_mapped[6];
  float transform_aft_mapped[6];
  int32_t n_corner_q;           /* laserCloudCornerScanDSNum (the corner queries) */
  int32_t n_surf_q;             /* laserCloudSurfTotalLastDSNum (the surf queries) */
  llsr_lm_report lm;            /* the last frame's scan2MapOptimization (iterations 0 when skipped) */
  llsr_map_report map;          /* the last frame's extractSurroundingKeyFrames */
} llsr_mapping_slot;
/* Allocate the per-slot MapOptimization state (max_batch slots, map_cfg NULL = the reference's
 * leaves and radius) and start every slot over (also resets the odometry). */
int32_t llsr_mapping_init(llsr_handle* h, int32_t mo_mode, const llsr_map_config* map_cfg);
int32_t llsr_mapping_batch(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets, int32_t B,
                           void* hip_stream);
int32_t llsr_mapping_fetch(llsr_handle* h, int32_t b, llsr_mapping_slot* out);
/* cloudKeyPoses6D of slot b: x, y, z, roll, pitch, yaw per keyframe into out[6*cap]; returns the
 * keyframe count (may exceed cap). */
int32_t llsr_mapping_keyposes(llsr_handle* h, int32_t b, float* out, int32_t cap);
/* Start every slot over: odometry, poses, keyframe stores, the global map's call counters. */
int32_t llsr_mapping_reset(llsr_handle* h);
/* llsr_map_global / llsr_map_save on slot b's keyframe store, after the handle's pending work;
 * robot_pos is the slot's transform_aft_mapped[3..5]. One call counter per slot. */
int32_t llsr_mapping_global_map(llsr_handle* h, int32_t b, const llsr_global_map_config* cfg, float* d_global,
                                int64_t cap_global, float* d_edge, int64_t cap_edge, float* d_planar,
                                int64_t cap_planar, llsr_global_map_report* rep, void* hip_stream);
int32_t llsr_mapping_save_map(llsr_handle* h, int32_t b, float* d_corner, int64_t cap_corner, float* d_surf,
                              int64_t cap_surf, int64_t* n_corner, int64_t* n_surf, void* hip_stream);
/* Loop closure of the slots (DESIGN.md §16 "Batch form"; the loop-closure thread of the reference,
 * per slot). llsr_mapping_stage_times arms the next llsr_mapping_batch / _batch_odom call of the same
 * B with seconds[b] = timeLaserOdometry.seconds() of slot b's scan (host array, copied): the keyframe
 * that call saves for slot b is stamped with it (MO:1706), and a slot whose MapOptimization runs in
 * that call keeps it as its `now`. The staging is consumed by that call once its odometry has
 * advanced (a batch of another B returns LLSR_EINVAL and leaves it staged); a call without staging
 * leaves its keyframe's time NaN and the slot's `now` as it was. The rollback of a failed
 * MapOptimization part restores `now`; llsr_mapping_reset clears it and any staging. */
int32_t llsr_mapping_stage_times(llsr_handle* h, const double* seconds, int32_t B);
/* llsr_map_keyframe_times of slot b's store. */
int32_t llsr_mapping_keyframe_times(llsr_handle* h, int32_t b, double* out, int32_t cap);
/* detectLoopClosure + performLoopClosure of slots 0 .. B - 1 in one call, after the handle's pending
 * work: per slot the candidate and the submaps on its store (llsr_map_loop_submaps with robot_pos =
 * the slot's currentRobotPosPoint and now = its staged time; a slot that never got a time holds NaN
 * and finds no candidate), then ONE llsr_icp_align_batch over the raw clouds of every slot that found
 * a candidate, on a workspace the handle owns, then per slot the acceptance test and, when accepted,
 * the constraint. reps[b] is what llsr_map_loop_closure reports for that slot alone (ms: the whole
 * call's wall time). cfg NULL: llsr_loop_config_lidar of the handle's lidar. Changes no map state;
 * the aligned and history clouds are not exported. Synchronises hip_stream (NULL: the handle's). */
int32_t llsr_mapping_loop_closure(llsr_handle* h, const llsr_loop_config* cfg, int32_t B, llsr_loop_report* reps,
                                  void* hip_stream);
/* correctPoses (MO:1757-1785) on slot b: llsr_map_set_key_poses on its store, and the same n poses
 * into the slot's own cloudKeyPoses6D (llsr_mapping_keyposes). latest_estimate6 (may be NULL), in the
 * layout of transform_aft_mapped, is iSAM2's latestEstimate after the loop factor: transformAftMapped,
 * transformLast and transformTobeMapped are set to it (MO:1722-1733) and currentRobotPosPoint from it. */
int32_t llsr_mapping_set_key_poses(llsr_handle* h, int32_t b, const float* poses6, int32_t n,
                                   const float* latest_estimate6);
/* ---- Pose graph: the factor graph of MO:1086-1090 / 1612-1690, batched ----
 * P independent graphs in one object: per graph K poses, a prior on pose 0, K - 1 odometry factors and
 * the loop factors in insertion order; llsr_pg_optimize runs a Gauss-Newton in double over every
 * graph that received a loop factor since its last optimisation, all of them in one set of launches
 * per pass. GTSAM is restated, not linked; §19 marks the choices. Poses are the store's floats (x, y,
 * z, roll, pitch, yaw: llsr_mapping_keyposes, llsr_map_set_key_poses); a loop factor takes
 * llsr_loop_constraint's outputs as they are. A node that keeps GTSAM ignores these calls.
 * hip_device == LLSR_PG_HOST: no device; the same loop bodies run serially over heap buffers of the
 * device workspace's sizes, and every result is bit for bit the device's. */
#define LLSR_PG_HOST (-1)
typedef struct llsr_pg llsr_pg;
typedef struct llsr_pg_config {
  int32_t max_iterations;      /* 100 (NonlinearOptimizerParams) */
  int32_t pad;
  double relative_error_tol;   /* 1e-5 */
  double absolute_error_tol;   /* 1e-5 */
} llsr_pg_config;
/* state: 0 clean (no loop factor since the last optimisation: skipped, nothing else set but poses /
 * loops), 1 stopped by the absolute tolerance, 2 by the relative tolerance, 3 by max_iterations, 4 the
 * error rose (the iterate before is kept; `iterations` counts the step taken back), 5 failed (a pivot
 * of the factorisation was not finite and positive; the poses stay at the iterate it was reached
 * with). error_before / error_after: half the sum of squared whitened residuals at the start and at
 * the iterate kept. */
typedef struct llsr_pg_report {
  int32_t state;
  int32_t iterations;
  double error_before;
  double error_after;
  int32_t poses;
  int32_t loops;
  float ms;          /* the whole call (HIP events on a device, wall time on the host), all graphs */
  int32_t moved;     /* the estimate differs from the one before the call (a step was kept) */
} llsr_pg_report;
/* Capacities are per graph: poses, loop factors, 6x6 blocks of the normal equations' row envelope (a
 * graph needs 2 K - 1 blocks plus max(from, to) - min(from, to) - 1 for the longest loop ending on
 * each row). NULL: P < 1 or P > 65535, a capacity < 1 (max_loops < 0), no such device, no memory. */
llsr_pg* llsr_pg_create(int32_t hip_device, int32_t P, int32_t max_poses, int32_t max_loops,
                        int64_t max_envelope_blocks);
void llsr_pg_destroy(llsr_pg* g);
const char* llsr_pg_last_error(const llsr_pg* g);
int32_t llsr_pg_config_default(llsr_pg_config* cfg);
/* Empty graph p (-1: all). */
int32_t llsr_pg_reset(llsr_pg* g, int32_t p);
/* Append n keyframes to graph p: pose 0 gets the prior at its own value, keyframe k the odometry
 * factor between(estimate of k - 1 now, poses6[k]) (MO:1641-1664). Never optimises: the new factor has
 * no error at the new pose, and the estimate of the others stays. */
int32_t llsr_pg_append(llsr_pg* g, int32_t p, const float* poses6, int32_t n);
/* The loop factor of MO:1086-1088 between from_id (latest) and to_id (closest):
 * pose_from.between(pose_to) of llsr_loop_constraint's outputs, one variance for all six components. */
int32_t llsr_pg_add_loop(llsr_pg* g, int32_t p, int32_t from_id, int32_t to_id, const float pose_from6[6],
                         const float pose_to6[6], float variance);
/* Optimise every graph with a loop factor since its last optimisation; reps[P] (may be NULL). cfg NULL:
 * the defaults. Synchronises hip_stream (NULL: the object's own; ignored on the host). */
int32_t llsr_pg_optimize(llsr_pg* g, const llsr_pg_config* cfg, llsr_pg_report* reps, void* hip_stream);
/* Graph p's estimate, x, y, z, roll, pitch, yaw per pose into out6[6 * cap]; returns K (may exceed
 * cap). A pose no optimisation moved is the appended floats bit for bit. */
int32_t llsr_pg_poses(const llsr_pg* g, int32_t p, float* out6, int32_t cap);
/* LLSR_EINVAL: ids out of range, from_id == to_id, a variance that is not finite and positive, a pose
 * that is not finite, a problem index outside [0, P); LLSR_ERANGE: the pose, loop or envelope capacity
 * is exceeded. A refused call leaves the graph unchanged.
 *
 * The mapping chain's graphs, opt-in: after llsr_mapping_enable_pose_graph(h, 1, max_loops) every
 * keyframe a slot saves is appended to the slot's graph (inside the rollback of a failed
 * MapOptimization part), llsr_mapping_reset empties the graphs, and llsr_mapping_close_loops runs
 * llsr_mapping_loop_closure, adds the loop factor of every accepted slot, runs ONE llsr_pg_optimize
 * over all slots and, for every slot whose graph moved, llsr_mapping_set_key_poses with the new poses
 * and the newest pose as latest_estimate6 (MO:1722-1733). A slot without an accepted loop is
 * untouched. Enabling starts the graphs from the slots' current key poses; on == 0 drops them.
 * pg_reps[B] may be NULL. The graphs live on the handle's device.
 * When llsr_mapping_close_loops fails after the loop closure itself (a graph's loop capacity is full,
 * the optimisation fails), the loop factors it already added stay in their graphs and no key pose has
 * changed: those graphs are optimised, with whatever is added then, by the next call. The graphs
 * follow the slots only through these calls: key poses set from outside (llsr_mapping_set_key_poses)
 * do not reach a slot's graph, so a caller that corrects poses itself should not enable them, or
 * should enable them again afterwards (which starts the graphs from the key poses as they are then).
 * Memory: one object holds all max_batch graphs at the capacity of the fullest, K poses (256 at
 * first, doubled when a slot fills it) and E envelope blocks (4 K at first, at most (2 + max_loops) K)
 * each: about 264 K + 776 (K + max_loops) + 288 E bytes per slot on the device, 0.6 MB at first for
 * max_loops = 64 (0.6 GB for 1024 slots), and about 250 K + 144 (K + max_loops) on the host (0.1 MB). */
int32_t llsr_mapping_enable_pose_graph(llsr_handle* h, int32_t on, int32_t max_loops);
int32_t llsr_mapping_close_loops(llsr_handle* h, const llsr_loop_config* loop_cfg, const llsr_pg_config* pg_cfg,
                                 int32_t B, llsr_loop_report* loop_reps, llsr_pg_report* pg_reps, void* hip_stream);
/* Graph b's poses (llsr_pg_poses of the slot's graph). */
int32_t llsr_mapping_pose_graph_poses(llsr_handle* h, int32_t b, float* out6, int32_t cap);
/* Host-only (no device): the pose glue llsr_mapping_batch applies per frame — OdometryToTransform
 * of FA's transformSum (tf2 round trip) into transform_sum, then transformAssociateToMap with the
 * given transformBefMapped / transformAftMapped into transform_tobe_mapped (and transform_incre,
 * may be NULL). */
int32_t llsr_mapping_associate(const float transform_sum_fa[6], const float transform_bef_mapped[6],
                               const float transform_aft_mapped[6], float transform_sum[6],
                               float transform_tobe_mapped[6], float transform_incre[6]);

/* ---- Prior map: localising in a saved map ----
 * The reference saves cornerMap / surfaceMap (saveMapService) and has no way to take them back: its
 * /initialpose subscriber's body is commented out (MO:437-456). A prior map holds one static corner
 * and one static surf cloud (float4 x, y, z, intensity in the map frame, as the save calls above write
 * them; never downsampled here) and crops both around P positions in one call; attached to a mapping
 * handle, the crop takes the place of extractSurroundingKeyFrames for every slot.
 * Stored order, per kind: tile coordinate i = (int)floorf(c / tile) - min over the cloud, per axis
 * (one correctly rounded float32 divide); key = (iz ny + iy) nx + ix; the cloud stably sorted by key,
 * with tile_start[ntiles + 1] over the keys. The crop of a kind at a position is exactly the stored
 * points with d^2 = ((0 + dx^2) + dy^2) + dz^2 < float(double(radius) * double(radius)) in float32, in
 * stored order (the predicate of the global map's step 2). Tiles that cannot hold such a point are
 * skipped; no point is copied untested.
 * hip_device == LLSR_PRIOR_HOST: no device; the same index and the same crop run serially over heap
 * buffers, `out` is host memory, and every result is bit for bit the device's. One call at a time per
 * object. */
#define LLSR_PRIOR_HOST (-1)
#define LLSR_PRIOR_CORNER 0
#define LLSR_PRIOR_SURF 1
typedef struct llsr_prior llsr_prior;
typedef struct llsr_prior_config {
  float radius;   /* surrounding_keyframe_search_radius, 50 (CFG:26) */
  float tile;     /* tile edge, 10 m */
} llsr_prior_config;
typedef struct llsr_prior_report {
  int64_t n_points[2];      /* [kind]: corner, surf */
  int64_t n_tiles[2];       /* nx ny nz */
  int64_t n_tiles_used[2];  /* tiles that hold a point */
  int32_t dims[2][3];       /* nx, ny, nz */
  int32_t origin[2][3];     /* min over the cloud of floorf(c / tile), per axis */
  float radius, tile;
  int32_t device;           /* LLSR_PRIOR_HOST or the HIP device */
  int32_t pad;
} llsr_prior_report;
int32_t llsr_prior_config_default(llsr_prior_config* cfg);
/* cfg NULL: the defaults. NULL: a radius or tile that is not finite and positive, no such device, no
 * memory. */
llsr_prior* llsr_prior_create(const llsr_prior_config* cfg, int32_t hip_device);
void llsr_prior_destroy(llsr_prior* p);
const char* llsr_prior_last_error(const llsr_prior* p);
/* Replace both clouds (host arrays, [n][4] floats; an empty kind is allowed). The index is built on the
 * host, once per map. LLSR_EINVAL: a non-finite coordinate; LLSR_ERANGE: more than 2^24 tiles or 2^31 - 2
 * points of one kind, or a tile index beyond +-2^30 (the error text names a tile size that fits). A
 * refused call leaves the object as it was. Synchronises hip_stream (NULL: the object's own). */
int32_t llsr_prior_load(llsr_prior* p, const float* corner, int64_t n_corner, const float* surf, int64_t n_surf,
                        void* hip_stream);
int32_t llsr_prior_info(const llsr_prior* p, llsr_prior_report* out);
/* Kind `kind`'s cloud in stored order into out_host[4 * cap] / its tile_start into out_host[cap];
 * they return the point count / ntiles + 1 (may exceed cap; negative: an error). */
int64_t llsr_prior_points(const llsr_prior* p, int32_t kind, float* out_host, int64_t cap);
int64_t llsr_prior_tile_starts(const llsr_prior* p, int32_t kind, uint32_t* out_host, int64_t cap);
/* The crops around positions3 (host, [P][3]): `out` (device float4, 16-byte aligned; host memory on
 * a host object; capacity `cap` points) receives the P corner crops packed, then the P surf crops;
 * corner_off / surf_off (host, [P + 1] each) are offsets in points into `out`: position p's corner
 * crop is points corner_off[p] .. corner_off[p + 1] - 1, corner_off[0] = 0, surf_off[0] =
 * corner_off[P]. This is the map side of llsr_s2m_batch: one buffer, two offset rows. A position with
 * a non-finite coordinate gets empty crops. out NULL with cap 0 only counts. When cap is too small the
 * call returns LLSR_ERANGE with the sizes in the offsets and nothing written, and a retry with a
 * larger buffer gives the identical result. LLSR_ERANGE also for P outside [1, 32767]. On the device:
 * a counting kernel over (row of tiles, position, kind), a scan per position, one copy of the 2 P
 * totals to the host, a writing kernel. Synchronises hip_stream (NULL: the object's own). */
int32_t llsr_prior_crop_batch(llsr_prior* p, const float* positions3, int32_t P, float* out, int64_t cap,
                              int64_t* corner_off, int64_t* surf_off, void* hip_stream);
/* Diagnostic: the last crop on p — its device time in ms (HIP events around both kernels; wall time
 * on the host), the points the predicate ran on and the points written. */
int32_t llsr_prior_last_crop(const llsr_prior* p, float* ms, int64_t* tested, int64_t* written);
/* The mapping chain in localisation mode. llsr_mapping_set_prior attaches p (on the handle's device;
 * not owned: it must outlive the attachment; NULL detaches) to every slot. Allowed only directly after
 * llsr_mapping_init or llsr_mapping_reset, before any frame, else LLSR_EINVAL; the reset keeps the
 * attachment, the init drops it. With a prior attached MapOptimization::run differs in three things:
 * extractSurroundingKeyFrames is one crop over all stepping slots at their currentRobotPosPoint,
 * handed straight to the scan-to-map batch (the empty-store return of MO:1097 does not apply: a slot
 * has a local map from its first MapOptimization frame); saveKeyFramesAndFactor records the key pose,
 * its time and the pose-graph factor but no clouds; and the first-keyframe distinction counts key
 * poses. llsr_mapping_slot.map then reports the crop sizes in n_corner_map = n_corner_ds and
 * n_surf_map = n_surf_ds, its other fields zero. The calls that need keyframe clouds — the global map
 * and save calls and both loop-closure calls of the chain — return LLSR_ENOSYS.
 * llsr_mapping_set_pose is the /initialpose handler the reference left commented out: between batches,
 * slot b's transformAftMapped, transformTobeMapped and transformLast become pose6 (transform_aft_mapped's
 * layout) and currentRobotPosPoint its position; transformBefMapped stays, so the next
 * transformAssociateToMap carries the pose forward by the odometry since the last mapped frame. With
 * or without a prior. */
int32_t llsr_mapping_set_prior(llsr_handle* h, llsr_prior* p);
int32_t llsr_mapping_set_pose(llsr_handle* h, int32_t b, const float pose6[6]);


/* ---- FA end of scan on the FA node's thread (host side, no handle) ----
 * For a node whose FeatureAssociation thread owns its own clouds and calls llsr_scan2scan on its
 * own handle: integrateTransformation (FA:2537-2568, no IMU) updates
 * transform_sum in place from transformCur; TransformToEnd (FA:1414-1490, the
 * use_imu_undistortion == false branch) moves n float4 rows (x, y, z, intensity; intensity =
 * ring + relTime / 10 as adjustDistortion leaves it) to the scan's end with transformCur, as
 * publishCloudsLast does for the less-sharp / less-flat and sharp / flat clouds (FA:2666-2707).
 * out_xyzi may equal in_xyzi. Bit-identical to the device odometry path (llsr_odometry_batch). */
int32_t llsr_integrate_transformation(float transform_sum[6], const float transform_cur[6]);
int32_t llsr_transform_to_end(const float transform_cur[6], const float* in_xyzi, int32_t n, float* out_xyzi);

/* ---- TransformFusion (transformFusion.cpp) ----
 * The fourth node of the reference fuses the 10 Hz scan-to-scan odometry with the slower mapped
 * pose. It is scalar host work per message, so these entry points run on the host side of the
 * library (no device, no handle), with the reference's float / double typing: tf2's
 * Quaternion::setRPY / Matrix3x3::getRPY in double, transformAssociateToMap on floats (the same
 * routine as MO:458-581, TF:65-186). The odometry messages carry the nav_msgs/Odometry fields the
 * nodes read and write. */
typedef struct llsr_odometry_msg {
  double orientation[4];    /* pose.pose.orientation x, y, z, w */
  double position[3];       /* pose.pose.position */
  double twist_angular[3];  /* twist.twist.angular (MO's transformBefMapped[0..2]) */
  double twist_linear[3];   /* twist.twist.linear (MO's transformBefMapped[3..5]) */
} llsr_odometry_msg;
typedef struct llsr_fusion_state {  /* TransformFusion's members (transformFusion.h) */
  float transform_sum[6];
  float transform_incre[6];
  float transform_mapped[6];
  float transform_bef_mapped[6];
  float transform_aft_mapped[6];
} llsr_fusion_state;
/* The constructor's zeros (TF:51-57). */
int32_t llsr_fusion_init(llsr_fusion_state* st);
/* How the publishers encode a pose: orientation = (-q.y, -q.z, q.x, q.w) of
 * setRPY(pose[2], -pose[0], -pose[1]), position = pose[3..5]; twist = twist6 (NULL: zeros).
 * FeatureAssociation::publishOdometry (FA:2612-2625: transformSum, no twist),
 * MapOptimization::publishTF (MO:704-723: transformAftMapped, twist = transformBefMapped),
 * TransformFusion's /integrated_to_init (TF:193-206: transformMapped, no twist). */
int32_t llsr_pose_to_odometry(const float pose[6], const float twist6[6], llsr_odometry_msg* out);
/* OdometryToTransform (UT:99-113): getRPY of Quaternion(o.z, -o.x, -o.y, o.w) -> (-pitch, -yaw,
 * roll), position. */
int32_t llsr_odometry_to_transform(const llsr_odometry_msg* in, float transform[6]);
/* TransformFusion::laserOdometryHandler (TF:188-280): transform_sum from /laser_odom_to_init,
 * transformAssociateToMap, and the /integrated_to_init message (also the camera_init -> camera tf,
 * same rotation and translation). */
int32_t llsr_fusion_laser_odometry(llsr_fusion_state* st, const llsr_odometry_msg* laser_odometry,
                                   llsr_odometry_msg* integrated);
/* TransformFusion::odomAftMappedHandler (TF:282-304): transform_aft_mapped from the pose (getRPY
 * of Quaternion(o.z, -o.x, -o.y, o.w) -> -pitch, -yaw, roll), transform_bef_mapped from the twist. */
int32_t llsr_fusion_aft_mapped(llsr_fusion_state* st, const llsr_odometry_msg* odom_aft_mapped);

/* ---- /odom2 and updateInitialGuess (featureAssociation.cpp:354-383, 2337-2402) ----
 * After every scan-to-scan LM the reference runs updateInitialGuess (FA:2790), which rebuilds all
 * six entries of transformCur from the latest /odom2 sample and the previous transformSum; the
 * rebuilt value is what integrateTransformation, publishCloudsLast and the next LM's initial guess
 * see. Host side of the library (no device, no handle), double arithmetic in the order the
 * reference's x86-64 build evaluates Eigen 3.3.7's expressions (glibc sincos /
 * atan2 / sqrt in double).
 * llsr_odom_sample holds odomRoll / Pitch / Yaw / PosX / PosY / PosZ[odomPointerLast]; llsr_odom_state
 * holds odomCallback's members: odomInitialIter, the number of messages seen, x/y/z_initial and the
 * latest sample (the reference's 200-entry ring is only read at odomPointerLast). */
typedef struct llsr_odom_sample { float roll, pitch, yaw, x, y, z; } llsr_odom_sample;
typedef struct llsr_odom_state {
  int32_t initial_iter;
  int32_t n_msgs;
  double origin[3];
  llsr_odom_sample last;
} llsr_odom_state;
/* The constructor's zeros (FA:277-287). `last` is the zero sample: this library's definition of "no
 * /odom2 message yet", where the reference reads its arrays at index -1. */
int32_t llsr_odom_init(llsr_odom_state* st);
/* odomCallback (FA:354-383): tf2 getRPY of the orientation (x, y, z, w as they come) in double,
 * narrowed to float; the first message latches the origin; position = (double)position - origin,
 * narrowed to float. Reads orientation and position of the message only. */
int32_t llsr_odom_callback(llsr_odom_state* st, const llsr_odometry_msg* msg);
/* updateInitialGuess (FA:2370-2402): reads transform_sum, overwrites all six entries of
 * transform_cur. */
int32_t llsr_update_initial_guess(const llsr_odom_sample* sample, const float transform_sum[6],
                                  float transform_cur[6]);

/* llsr_odometry_batch with updateInitialGuess in program order (FA:2789-2796), accepted in both
 * handle modes (the FA LM is always applied; llsr_config.mode only ever meant MapOptimization's
 * update). samples: host [B], the slots' latest /odom2 samples (llsr_odom_state.last); overwrite:
 * host [B] flags, NULL = every slot. For a slot with overwrite[b] != 0, on every scan after its
 * first: the LM starts from the slot's carried transformCur; transformCur is then replaced by
 * llsr_update_initial_guess(samples[b], transformSum); integrateTransformation and the four
 * TransformToEnd use the replaced value, and it carries over as the next LM's initial guess. The
 * slot's first scan runs checkSystemInitialization only (the `continue` at FA:2781-2784). A slot
 * with overwrite[b] == 0 behaves exactly as under llsr_odometry_batch. llsr_odometry_fetch then
 * reports the replaced transformCur (as the reference's member would read) and `lm` the LM that ran;
 * llsr_odometry_fetch_lm returns the LM's own transformCur of slot b's last scan (zeros before the
 * slot's second scan or when the slot was not flagged). Same single host sync as
 * llsr_odometry_batch: transformSum rides on the feature-count copy, the guesses are evaluated on
 * the host and uploaded asynchronously. */
int32_t llsr_odometry_batch_odom(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets, int32_t B,
                                 const llsr_odom_sample* samples, const uint8_t* overwrite, void* hip_stream);
int32_t llsr_odometry_fetch_lm(llsr_handle* h, int32_t b, float transform_lm[6]);
/* llsr_mapping_batch over llsr_odometry_batch_odom: same trailing arguments, accepted in both handle
 * modes (llsr_mapping_init likewise), same rollback contract. */
int32_t llsr_mapping_batch_odom(llsr_handle* h, const float* d_xyzi, const int64_t* d_offsets, int32_t B,
                                const llsr_odom_sample* samples, const uint8_t* overwrite, void* hip_stream);

/* ---- /imu_type and adjustDistortion's IMU de-skew (featureAssociation.cpp:315-351, 452-563, 600-690, 788) ----
 * Once one /imu_type message has arrived (imuPointerLast >= 0; use_imu_undistortion is not read on
 * this path) adjustDistortion interpolates the IMU queue at every segmented point's time and rotates
 * the point into the scan-start frame. The queue lives on the host side of the library (no device, no
 * handle), like /odom2 above; a scan takes a linear window of it, and the feature stage de-skews on
 * the device from that window (llsr_stage_imu) or on the host (llsr_imu_deskew_host); both run the
 * same per-point body (csrc/llsr_imu.h). DESIGN.md §17. */
#define LLSR_IMU_QUEUE 200
#define LLSR_IMU_WINDOW_MAX (LLSR_IMU_QUEUE + 1)
typedef struct llsr_imu_msg {  /* the sensor_msgs/Imu fields imuHandler reads */
  int32_t sec;                 /* header.stamp */
  uint32_t nanosec;
  double orientation[4];       /* x, y, z, w */
  double angular_velocity[3];
  double linear_acceleration[3];
} llsr_imu_msg;
typedef struct llsr_imu_state {  /* FeatureAssociation's IMU queue members (featureAssociation.h:68-119) */
  int32_t pointer_last;            /* imuPointerLast: -1 until the first message */
  int32_t pointer_last_iteration;  /* imuPointerLastIteration */
  double time[LLSR_IMU_QUEUE];
  float roll[LLSR_IMU_QUEUE], pitch[LLSR_IMU_QUEUE], yaw[LLSR_IMU_QUEUE];
  float acc[3][LLSR_IMU_QUEUE];               /* imuAccX / Y / Z */
  float velo[3][LLSR_IMU_QUEUE];              /* imuVeloX / Y / Z */
  float shift[3][LLSR_IMU_QUEUE];             /* imuShiftX / Y / Z */
  float angular_velo[3][LLSR_IMU_QUEUE];      /* imuAngularVeloX / Y / Z */
  float angular_rotation[3][LLSR_IMU_QUEUE];  /* imuAngularRotationX / Y / Z */
} llsr_imu_state;
/* The constructor's values (FA:237-239, 261-270): zeros, pointer_last = -1. */
int32_t llsr_imu_init(llsr_imu_state* st);
/* imuHandler + AccumulateIMUShiftAndRotation (FA:315-351, 452-489): tf2 getRPY of the orientation in
 * double; the gravity-compensated acceleration from double sin / cos, narrowed to float; the ring
 * advances; the accumulate step rotates the acceleration with float sin / cos and, when the gap to the
 * entry before is below scan_period, writes shift / velocity / angular rotation (each update in
 * double, narrowed on the store). A gap >= scan_period leaves those nine entries as the ring held
 * them 200 messages earlier (or zero). */
int32_t llsr_imu_callback(llsr_imu_state* st, const llsr_imu_msg* msg, float scan_period);
typedef struct llsr_imu_sample {  /* one ring entry as the de-skew reads it */
  double time;
  float roll, pitch, yaw;
  float velo[3], shift[3], angular_rotation[3];
} llsr_imu_sample;
/* The ring entries one adjustDistortion call can read, in walk order, then FA:788
 * (pointer_last_iteration = pointer_last). *n = 0 when no message ever arrived (pointer_last < 0: no
 * de-skew; pointer_last_iteration becomes -1 as in the reference, whose next walk would then start
 * outside the array: here -1 is read as entry 0, the first message); otherwise *n = ((pointer_last - pointer_last_iteration) mod 200) + 1
 * candidates and out[k], k = 0 .. *n, is ring entry (pointer_last_iteration - 1 + k) mod 200 copied as
 * it stands: out[0] is the "back" of the first candidate, the search walks k = 1 .. *n and stops at
 * k = *n (= pointer_last) at the latest. The ring walk starts at pointer_last_iteration and steps
 * (front + 1) mod 200 until it meets pointer_last, so it visits exactly these entries in this order,
 * also across the wrap, and every "back" (front + 199) mod 200 it reads is out[k - 1]. With no new
 * message since the previous scan, or exactly 200 of them, the pointers are equal: the walk does not
 * advance and *n = 1 (one candidate); that is not "no IMU", which only pointer_last < 0 means. */
int32_t llsr_imu_scan_window(llsr_imu_state* st, llsr_imu_sample out[LLSR_IMU_WINDOW_MAX], int32_t* n);
typedef struct llsr_imu_report {   /* FeatureAssociation's members after adjustDistortion */
  float start[3];                  /* imuRollStart, imuPitchStart, imuYawStart */
  float angular_from_start[3];     /* imuAngularFromStartX / Y / Z */
  float cur[3];                    /* imuRollCur, imuPitchCur, imuYawCur of the last point */
  float velo_from_start[3];        /* imuVeloFromStartX / Y / ZCur of the last point */
} llsr_imu_report;
typedef struct llsr_imu_carry {    /* what one scan hands to the next; zeros before the first */
  float angular_rotation_last[3];  /* imuAngularRotationX / Y / ZLast */
  llsr_imu_report report;          /* members a scan does not write keep their value */
} llsr_imu_carry;
/* adjustDistortion (FA:565-690) of one scan on the host, serially. scan_time_*: the segmented cloud's
 * header stamp (timeScanCur); window / n: llsr_imu_scan_window's (n = 0: no IMU, the plain LOAM swap);
 * seg_xyzi: S segmented points (IP frame, intensity = ring + col / 1e4); orientation: segInfo's
 * start_orientation, end_orientation, orientation_diff; carry: updated in place; loam_xyzi_out: S
 * points; report (may be NULL): carry->report after the scan. Point 0 latches the start state and is
 * not rotated; a scan that writes no member (n = 0, S = 0; S = 1 for velo_from_start) reports the
 * carried one. */
int32_t llsr_imu_deskew_host(const llsr_config* cfg, int32_t scan_time_sec, uint32_t scan_time_nanosec,
                             const llsr_imu_sample* window, int32_t n, const float* seg_xyzi, int32_t S,
                             const float orientation[3], llsr_imu_carry* carry, float* loam_xyzi_out,
                             llsr_imu_report* report);
/* Arm the next batch call of this handle (llsr_process_scan / llsr_process_batch, llsr_odometry_batch /
 * _batch_odom, llsr_mapping_batch / _batch_odom) with the slots' windows: host arrays scan_sec[B],
 * scan_nanosec[B], offsets[B + 1] and the packed samples; slot b's window is
 * samples[offsets[b] .. offsets[b + 1]) = llsr_imu_scan_window's out[0 .. n] (n + 1 entries), or empty
 * for a slot without IMU (plain path, carry untouched). The arrays are copied to handle-owned pinned
 * memory here and uploaded asynchronously on that batch's stream. The batch must have the same B
 * (else it returns LLSR_EINVAL and the staging stays). The staging is consumed when the call's
 * feature stage has been enqueued; a call that fails before that leaves it staged. A failure later in
 * the call (the LM or MapOptimization part) finds the carry advanced together with the odometry, as
 * the mapping batch's rollback contract states for the odometry, and the staging consumed. Waits for
 * the handle's previous batch (it may still read the pinned arrays). Each slot carries its
 * llsr_imu_carry on the device, zeroed by llsr_reset_state, llsr_odometry_reset and
 * llsr_mapping_reset. */
int32_t llsr_stage_imu(llsr_handle* h, const int32_t* scan_sec, const uint32_t* scan_nanosec,
                       const llsr_imu_sample* samples, const int64_t* offsets, int32_t B);
/* Slot b's report (its carried members) after the last batch; synchronises with it. */
int32_t llsr_fetch_imu_report(llsr_handle* h, int32_t b, llsr_imu_report* report);

/* ---- use_imu_undistortion == true (featureAssociation.cpp:1456-1483, 1492-1550, 2329-2332,
 * 2339-2349, 2557-2560, 2662-2663, 2786-2788) ----
 * The switch of the reference's YAML (false in its three shipped blocks). on != 0: from the next
 * batch call on, every odometry of this handle (llsr_odometry_batch / _batch_odom, llsr_mapping_batch /
 * _batch_odom) runs the reference's branches under the switch; the default is off, and
 * llsr_reset_state / llsr_odometry_reset / llsr_mapping_reset leave it as it is. Of a slot's
 * llsr_imu_report after the scan's feature stage (llsr_fetch_imu_report) the branches read `start`
 * (imuRoll / Pitch / YawStart) and `cur` (imuRoll / Pitch / YawCur of the last point, which the pre-LM
 * updateInitialGuess copies to imuRoll / Pitch / YawLast); angular_from_start and velo_from_start are
 * not read (their uses at FA:2351-2361 are commented out), and imuShiftFromStartX / Y / Z is always 0
 * (ShiftToStartIMU is never called). A slot that was never staged reads the constructor's zeros. Per
 * scan of a slot:
 *   first scan: checkSystemInitialization adds imuPitchStart to transformSum[0] and imuRollStart to
 *     transformSum[2] (FA:2329-2332);
 *   later scans: under llsr_odometry_batch_odom / llsr_mapping_batch_odom, for a slot with
 *     overwrite[b] != 0, the LM starts from llsr_update_initial_guess(samples[b], transformSum) instead
 *     of the carried transformCur (the updateInitialGuess before updateTransformation, FA:2786-2788;
 *     llsr_odometry_fetch_lm still returns the LM's own result); elsewhere the LM starts from the carried
 *     transformCur as with the switch off. integrateTransformation ends in PluginIMURotation
 *     (FA:2557-2560) and TransformToEnd runs its IMU tail (FA:1456-1483) on the four clouds (the shadow
 *     points appended to the surf last cloud stay raw).
 * Same single host sync per batch. DESIGN.md §18. */
int32_t llsr_set_imu_undistortion(llsr_handle* h, int32_t on);
/* The host twins of llsr_integrate_transformation / llsr_transform_to_end with the switch on, for the
 * FA node's thread (no device, no handle); they read report->start and report->cur only and are
 * bit-identical to the device path. out_xyzi may equal in_xyzi. llsr_first_scan_imu is
 * checkSystemInitialization's add on a slot's first scan. */
int32_t llsr_integrate_transformation_imu(float transform_sum[6], const float transform_cur[6],
                                          const llsr_imu_report* report);
int32_t llsr_transform_to_end_imu(const float transform_cur[6], const llsr_imu_report* report, const float* in_xyzi,
                                  int32_t n, float* out_xyzi);
int32_t llsr_first_scan_imu(float transform_sum[6], const llsr_imu_report* report);

/* ---- Input wire formats (llsr_input.hip) ----
 * sensor_msgs/PointCloud2 (PointField datatype codes, sensor_msgs/msg/PointField.msg) decoded as
 * pcl::fromROSMsg<PointXYZI> (IP:196): x, y, z, intensity are taken from the fields of that name
 * whose datatype is FLOAT32 and count 1; any other field is ignored and an unmatched PointXYZI
 * field reads 0 (its default). Byte order is taken as-is (PCL ignores is_bigendian). */
#define LLSR_PC2_FLOAT32 7
#define LLSR_PC2_MAX_FIELDS 16
typedef struct llsr_pc2_field {
  char name[16];
  int32_t offset;    /* byte offset in the point */
  int32_t datatype;  /* PointField.datatype */
  int32_t count;
} llsr_pc2_field;
typedef struct llsr_pc2_layout {  /* the message's fields + point_step (constant per sensor) */
  int32_t point_step;
  int32_t num_fields;
  llsr_pc2_field fields[LLSR_PC2_MAX_FIELDS];
} llsr_pc2_layout;
typedef struct llsr_pc2_msg {     /* one message of the batch */
  int64_t data_offset;            /* first byte of its `data` in the packed device buffer */
  int32_t width, height;          /* points = width * height */
  int32_t row_step;               /* bytes per row (organized clouds, height > 1) */
  int32_t pad;
} llsr_pc2_msg;
/* Decode B messages whose data bytes are packed in d_data (device) into float4 x, y, z, intensity
 * points packed in d_out (device, capacity sum(width * height)), in row-major point order; writes
 * the point offsets to out_off[B+1] (host) and, if not NULL, to d_out_off[B+1] (device) — the
 * inputs llsr_process_batch / llsr_odometry_batch take. NaN points are kept (those calls remove
 * them, IP:198). Synchronises hip_stream. */
int32_t llsr_decode_pointcloud2(const llsr_pc2_layout* layout, const uint8_t* d_data, const llsr_pc2_msg* msgs,
                                int32_t B, float* d_out, int64_t* out_off, int64_t* d_out_off, void* hip_stream);
/* KITTI velodyne sequences (offlineKittiService IP:224-248, KittiLoader imageProjection.h:127-200):
 * a frame file holds float32 x, y, z, reflectance records; like the reference, at most
 * LLSR_KITTI_MAX_FLOATS floats are read and floor(floats / 4) points kept. */
#define LLSR_KITTI_MAX_FLOATS 1000000
/* Number of consecutive frames <dir>/%06d.bin starting at 0. */
int32_t llsr_kitti_count(const char* velodyne_dir);
/* One frame into a host buffer (capacity cap points); *n = points (LLSR_ERANGE if > cap). */
int32_t llsr_kitti_read(const char* path, float* xyzi, int32_t cap, int32_t* n);
/* Frames first .. first+B-1 of <dir> into d_xyzi (device, capacity cap_points) with one pinned
 * upload; point offsets to off[B+1] (host) and, if not NULL, d_off[B+1] (device). Synchronises. */
int32_t llsr_kitti_load(const char* velodyne_dir, int32_t first, int32_t B, float* d_xyzi, int64_t cap_points,
                        int64_t* off, int64_t* d_off, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* LLSR_H_ */
