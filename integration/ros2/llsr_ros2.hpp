// llsr_ros2.hpp — the node-side half of the drop-in: what the reference's ROS2 nodes call in place
// of their per-scan arithmetic, over the C-ABI of include/llsr.h. Header-only C++11, templated on
// the message and cloud types so the same code builds against ROS2 + PCL (cloud_msgs::msg::CloudInfo,
// pcl::PointCloud<pcl::PointXYZI>) and, in tests/test_ros2_adapter.py, against plain structs with
// the same field names (no ROS here). INTEGRATION.md §2 shows the four member bodies that call it.
//
// Seams (reference file:line):
//   ImageProjection::cloudHandler            imageProjection.cpp:189-222 -> Projection::run
//   FeatureAssociation feature stage         featureAssociation.cpp:2769-2775 (+ 1310-1314 shadow points)
//                                            -> Projection::handoff (on the IP thread, into ProjectionOut)
//   runFeatureAssociation after the features featureAssociation.cpp:2777-2796, 2291-2315, 2660-2712
//                                            -> Odometry::solve / OdomInput::apply / Odometry::finish
//                                               (on the FA thread, its own handle; step = solve + finish)
//   FeatureAssociation::odomCallback         featureAssociation.cpp:354-383 -> OdomInput::on_message
//   FeatureAssociation::updateInitialGuess   featureAssociation.cpp:2337-2402 -> OdomInput::apply
//   use_imu_undistortion == true            featureAssociation.cpp:1456-1483, 2329-2332, 2557-2560,
//                                            2786-2788 -> Odometry's constructor switch, FeatureClouds::imu
//   FeatureAssociation::updateTransformation featureAssociation.cpp:2505-2535 -> update_transformation
//   MapOptimization::scan2MapOptimization    mapOptmization.cpp:1572-1610 -> scan2map_optimization
//   MapOptimization::publishGlobalMapThread  mapOptmization.cpp:305-315, 775-892 -> GlobalMap (opt-in)
//
// Threads. The reference runs IP, FA and MO on their own executor threads joined by one-slot
// Channels (main.cpp:10-11, channel.h:24-54); IP's blocking send waits only until FA has *taken*
// the previous scan, so IP's next cloudHandler overlaps FA's work on the last one. A handle is
// single-threaded and its host buffers are overwritten by the next scan, so nothing that FA uses
// may point into the IP node's Projection: the feature stage keeps FA's carry-over state
// (FA:167-198) in the IP handle and runs with the rest of the scan on the IP thread, and
// Projection::handoff copies its clouds into the ProjectionOut that crosses the channel
// (FeatureClouds below). FA's Odometry and MO's scan-to-map each own another handle.
#pragma once
#include <stdint.h>

#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "llsr.h"
#ifdef LLSR_ROS2_GLOBAL_MAP
#include <hip/hip_runtime_api.h>
#endif

namespace llsr_ros2 {

inline void check(int32_t rc, llsr_handle* h, const char* what) {
  if (rc != LLSR_OK)
    throw std::runtime_error(std::string("llsr: ") + what + ": " + (h ? llsr_last_error(h) : "no handle"));
}

// PCL PointXYZI is 32 bytes (x, y, z, pad, intensity, pad...): the ABI takes packed float4 rows.
template <class Cloud>
void repack_xyzi(const Cloud& c, std::vector<float>& out) {
  const size_t n = c.points.size();
  out.resize(4 * n);
  for (size_t i = 0; i < n; ++i) {
    const auto& p = c.points[i];
    out[4 * i] = p.x;
    out[4 * i + 1] = p.y;
    out[4 * i + 2] = p.z;
    out[4 * i + 3] = p.intensity;
  }
}

template <class Cloud>
void unpack_xyzi(const float* xyzi, int32_t n, Cloud& c) {
  c.points.resize((size_t)n);
  for (int32_t i = 0; i < n; ++i) {
    auto& p = c.points[(size_t)i];
    p.x = xyzi[4 * i];
    p.y = xyzi[4 * i + 1];
    p.z = xyzi[4 * i + 2];
    p.intensity = xyzi[4 * i + 3];
  }
  c.width = (uint32_t)n;
  c.height = 1;
}

// rows `ind` of a float4 array, in list order (cornerPointsSharp / LessSharp, surfPointsFlat)
template <class Cloud>
void gather_xyzi(const float* xyzi, const int32_t* ind, int32_t n, Cloud& c) {
  c.points.resize((size_t)n);
  for (int32_t k = 0; k < n; ++k) {
    const float* r = xyzi + 4 * (size_t)ind[k];
    auto& p = c.points[(size_t)k];
    p.x = r[0];
    p.y = r[1];
    p.z = r[2];
    p.intensity = r[3];
  }
  c.width = (uint32_t)n;
  c.height = 1;
}

// CloudInfo as IP:791-832 fills _seg_msg (header left to the caller: IP:199)
template <class CloudInfo>
void cloud_info(const llsr_scan_out& o, int32_t rings, CloudInfo& msg) {
  const size_t S = (size_t)o.n_segmented;
  msg.start_ring_index.assign(o.start_ring_index, o.start_ring_index + rings);
  msg.end_ring_index.assign(o.end_ring_index, o.end_ring_index + rings);
  msg.start_orientation = o.orientation[0];
  msg.end_orientation = o.orientation[1];
  msg.orientation_diff = o.orientation[2];
  msg.segmented_cloud_ground_flag.resize(S);
  msg.segmented_cloud_col_ind.resize(S);
  msg.segmented_cloud_range.resize(S);
  for (size_t k = 0; k < S; ++k) {
    msg.segmented_cloud_ground_flag[k] = o.seg_ground_flag[k] != 0;
    msg.segmented_cloud_col_ind[k] = o.seg_col_ind[k];
    msg.segmented_cloud_range[k] = o.seg_range[k];
  }
}

// ProjectionOut (UT:63-72) as publishClouds hands it to the FA channel (IP:933-1000): the
// segmented and outlier clouds, seg_msg, and the two intensity vectors (double, as declared)
template <class ProjOut, class Cloud>
void projection_out(const llsr_scan_out& o, int32_t rings, ProjOut& po, Cloud& segmented_cloud, Cloud& outlier_cloud) {
  unpack_xyzi(o.seg_xyzi, o.n_segmented, segmented_cloud);
  unpack_xyzi(o.outlier_xyzi, o.n_outlier, outlier_cloud);
  cloud_info(o, rings, po.seg_msg);
  po.segmentedCloud_Intensity.assign(o.seg_intensity, o.seg_intensity + o.n_segmented);
  po.outlierCloud_Intensity.assign(o.outlier_intensity, o.outlier_intensity + o.n_outlier);
}

// The FA feature stage's clouds (FA:2769-2775): segmentedCloud after adjustDistortion (LOAM
// frame), cornerPointsSharp / LessSharp and surfPointsFlat as gathers of it, the `ns` shadow points
// (GenerateShadowPoint, FA:412-450) appended to surfPointsFlat as FA:1310-1314 does, and
// surfPointsLessFlat as the per-ring VoxelGrid output
template <class Cloud>
void features(const llsr_scan_out& o, const float* shadow, int32_t ns, Cloud& segmented_cloud, Cloud& corner_sharp,
              Cloud& corner_less_sharp, Cloud& surf_flat, Cloud& surf_less_flat) {
  unpack_xyzi(o.loam_xyzi, o.n_segmented, segmented_cloud);
  gather_xyzi(o.loam_xyzi, o.sharp_ind, o.n_sharp, corner_sharp);
  gather_xyzi(o.loam_xyzi, o.less_sharp_ind, o.n_less_sharp, corner_less_sharp);
  gather_xyzi(o.loam_xyzi, o.flat_ind, o.n_flat, surf_flat);
  const size_t f = surf_flat.points.size();
  surf_flat.points.resize(f + (size_t)ns);
  for (int32_t k = 0; k < ns; ++k) {
    auto& p = surf_flat.points[f + (size_t)k];
    p.x = shadow[4 * k];
    p.y = shadow[4 * k + 1];
    p.z = shadow[4 * k + 2];
    p.intensity = shadow[4 * k + 3];
  }
  surf_flat.width = (uint32_t)surf_flat.points.size();
  surf_flat.height = 1;
  unpack_xyzi(o.less_flat_xyzi, o.n_less_flat, surf_less_flat);
}

// The feature clouds of one scan as runFeatureAssociation holds them after extractFeaturesOurs
// (FA:2769-2775): computed on the IP thread and carried to FA inside ProjectionOut. A maintainer
// adds the member `llsr_ros2::FeatureClouds<pcl::PointCloud<PointType>> features;` to ProjectionOut
// (UT:63-72). Values, not pointers into a handle's buffers: the IP thread's next scan cannot touch
// them once they are in the channel.
template <class Cloud>
struct FeatureClouds {
  Cloud segmented;          // segmentedCloud after adjustDistortion (LOAM frame)
  Cloud corner_sharp;       // cornerPointsSharp
  Cloud corner_less_sharp;  // cornerPointsLessSharp
  Cloud surf_flat;          // surfPointsFlat + the shadow points (FA:1310-1314)
  Cloud surf_less_flat;     // surfPointsLessFlat (per-ring VoxelGrid)
  // the scan's IMU members after adjustDistortion (Projection::imu_report; zeros without IMU): what
  // Odometry reads when use_imu_undistortion is on
  llsr_imu_report imu = llsr_imu_report();
};

// TransformToEnd (FA:1414-1490) of every point of `in` into `out` (may be the same cloud)
template <class Cloud>
void transform_to_end(const float transform_cur[6], const Cloud& in, Cloud& out) {
  std::vector<float> a;
  repack_xyzi(in, a);
  const int32_t n = (int32_t)(a.size() / 4);
  check(llsr_transform_to_end(transform_cur, a.data(), n, a.data()), nullptr, "llsr_transform_to_end");
  unpack_xyzi(a.data(), n, out);
}

// ... with use_imu_undistortion: the tail at FA:1456-1483 from the scan's IMU report
template <class Cloud>
void transform_to_end_imu(const float transform_cur[6], const llsr_imu_report& imu, const Cloud& in, Cloud& out) {
  std::vector<float> a;
  repack_xyzi(in, a);
  const int32_t n = (int32_t)(a.size() / 4);
  check(llsr_transform_to_end_imu(transform_cur, &imu, a.data(), n, a.data()), nullptr, "llsr_transform_to_end_imu");
  unpack_xyzi(a.data(), n, out);
}

template <class Cloud>
void append_xyzi(const float* xyzi, int32_t n, Cloud& c) {
  const size_t f = c.points.size();
  c.points.resize(f + (size_t)n);
  for (int32_t k = 0; k < n; ++k) {
    auto& p = c.points[f + (size_t)k];
    p.x = xyzi[4 * k];
    p.y = xyzi[4 * k + 1];
    p.z = xyzi[4 * k + 2];
    p.intensity = xyzi[4 * k + 3];
  }
  c.width = (uint32_t)c.points.size();
  c.height = 1;
}

// `lidar` everywhere below is the launch file's lidar_type: VLP-16 -> LLSR_LIDAR_VLP16, VLP-32c ->
// LLSR_LIDAR_VLP32C (use_vlp32c: rows by observed-elevation rank, ground D = 25 deg), HDL-64E ->
// LLSR_LIDAR_HDL64E; llsr_config_default fills that block of loam_config.yaml.
//
// An llsr handle owned by one node thread (FA's scan-to-scan, MO's scan-to-map): one scan slot,
// the LMs' buffers grow on first use. mode: LLSR_MODE_FAITHFUL / LLSR_MODE_LM_APPLIED (MO:1539-1545)
class Handle {
 public:
  explicit Handle(int32_t lidar, int32_t device = 0, int32_t mode = LLSR_MODE_LM_APPLIED) {
    llsr_config cfg;
    check(llsr_config_default(&cfg, lidar), nullptr, "llsr_config_default");
    if (llsr_abi_version() != LLSR_ABI_VERSION) throw std::runtime_error("llsr: library ABI version differs from llsr.h");
    cfg.mode = mode;
    llsr_handle* h = nullptr;
    const int32_t rc = llsr_create(&cfg, device, 1, cfg.num_vertical_scans * cfg.num_horizontal_scans, &h);
    if (rc != LLSR_OK || !h) throw std::runtime_error("llsr: llsr_create failed (no HIP device?)");
    h_ = h;
  }
  ~Handle() {
    if (h_) llsr_destroy(h_);
  }
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  llsr_handle* get() const { return h_; }

 private:
  llsr_handle* h_ = nullptr;
};

// FeatureAssociation's IMU queue (FA:237-239, 261-270) behind a mutex. Thread layout: on_message is
// imuHandler (FA:315-351, 452-489) and runs on the /imu_type subscription's thread; window() is taken
// once per scan by Projection::run on the projection thread, where this library runs the feature
// stage (adjustDistortion included) right after the segmentation. The reference reads the queue
// unsynchronised from runFeatureAssociation's thread while the handler writes it, so which messages
// a scan sees there depends on timing; here a scan sees the snapshot taken under the mutex at
// window(): every message whose callback returned before it, none after (and FA:788 happens in the
// same critical section). on_message accepts any message type with sensor_msgs/Imu's header.stamp,
// orientation, angular_velocity and linear_acceleration fields.
class ImuInput {
 public:
  struct Window {
    llsr_imu_sample samples[LLSR_IMU_WINDOW_MAX];
    int32_t n = 0;  // candidates; 0: no /imu_type message yet
  };
  explicit ImuInput(float scan_period) : scan_period_(scan_period) {
    check(llsr_imu_init(&st_), nullptr, "llsr_imu_init");
  }
  template <class Msg>
  void on_message(const Msg& msg) {
    llsr_imu_msg m = llsr_imu_msg();
    m.sec = msg.header.stamp.sec;
    m.nanosec = msg.header.stamp.nanosec;
    m.orientation[0] = msg.orientation.x;
    m.orientation[1] = msg.orientation.y;
    m.orientation[2] = msg.orientation.z;
    m.orientation[3] = msg.orientation.w;
    m.angular_velocity[0] = msg.angular_velocity.x;
    m.angular_velocity[1] = msg.angular_velocity.y;
    m.angular_velocity[2] = msg.angular_velocity.z;
    m.linear_acceleration[0] = msg.linear_acceleration.x;
    m.linear_acceleration[1] = msg.linear_acceleration.y;
    m.linear_acceleration[2] = msg.linear_acceleration.z;
    std::lock_guard<std::mutex> lk(m_);
    check(llsr_imu_callback(&st_, &m, scan_period_), nullptr, "llsr_imu_callback");
    ++messages_;
  }
  // the entries the scan that starts now can read; advances imuPointerLastIteration (FA:788)
  void window(Window& w) {
    std::lock_guard<std::mutex> lk(m_);
    check(llsr_imu_scan_window(&st_, w.samples, &w.n), nullptr, "llsr_imu_scan_window");
  }
  int64_t messages() const {
    std::lock_guard<std::mutex> lk(m_);
    return messages_;
  }

 private:
  mutable std::mutex m_;
  llsr_imu_state st_;
  float scan_period_;
  int64_t messages_ = 0;
};

// One handle and its host output buffers (capacity H*W per array, llsr_query_sizes), for the
// single-scan call shape the nodes use; one per pipeline thread, as the reference runs one thread
// per node.
class Projection {
 public:
  // max_points: raw points per scan the handle accepts (0: twice the range image)
  explicit Projection(int32_t lidar, int32_t device = 0, int32_t max_points = 0) {
    llsr_config cfg;
    check(llsr_config_default(&cfg, lidar), nullptr, "llsr_config_default");
    if (llsr_abi_version() != LLSR_ABI_VERSION) throw std::runtime_error("llsr: library ABI version differs from llsr.h");
    if (max_points < 1) max_points = 2 * cfg.num_vertical_scans * cfg.num_horizontal_scans;
    llsr_handle* h = nullptr;
    const int32_t rc = llsr_create(&cfg, device, 1, max_points, &h);
    if (rc != LLSR_OK || !h) throw std::runtime_error("llsr: llsr_create failed (no HIP device?)");
    h_ = h;
    llsr_sizes sz;
    check(llsr_query_sizes(h_, &sz), h_, "llsr_query_sizes");
    rings_ = sz.rings;
    cells_ = (size_t)sz.cells;
    start_.resize((size_t)rings_);
    end_.resize((size_t)rings_);
    seg_.resize(4 * cells_);
    loam_.resize(4 * cells_);
    lflat_.resize(4 * cells_);
    out_.resize(4 * cells_);
    gflag_.resize(cells_);
    col_.resize(cells_);
    rng_.resize(cells_);
    sint_.resize(cells_);
    oint_.resize(cells_);
    edge_.resize(cells_);
    sharp_.resize(cells_);
    flat_.resize(cells_);
    shadow_.resize(4 * (size_t)sz.shadow_points);
    check(llsr_shadow_points(shadow_.data()), h_, "llsr_shadow_points");
  }
  ~Projection() {
    if (h_) llsr_destroy(h_);
  }
  Projection(const Projection&) = delete;
  Projection& operator=(const Projection&) = delete;

  llsr_handle* handle() const { return h_; }
  const llsr_scan_out& out() const { return o_; }

  // cloudHandler from fromROSMsg on (IP:196-207): NaN removal, findStartEndAngle,
  // projectPointCloud, groundRemovalOurs, cloudSegmentation, then the FA feature stage of the
  // same scan (the handle keeps FA's carry-over arrays, FA:167-198)
  template <class Cloud>
  void run(const Cloud& laser_cloud_in) {
    repack_xyzi(laser_cloud_in, xyzi_);
    o_ = llsr_scan_out();
    o_.start_ring_index = start_.data();
    o_.end_ring_index = end_.data();
    o_.seg_xyzi = seg_.data();
    o_.seg_ground_flag = gflag_.data();
    o_.seg_col_ind = col_.data();
    o_.seg_range = rng_.data();
    o_.seg_intensity = sint_.data();
    o_.outlier_xyzi = out_.data();
    o_.outlier_intensity = oint_.data();
    o_.loam_xyzi = loam_.data();
    o_.less_sharp_ind = edge_.data();
    o_.sharp_ind = sharp_.data();
    o_.flat_ind = flat_.data();
    o_.less_flat_xyzi = lflat_.data();
    check(llsr_process_scan(h_, xyzi_.data(), (int32_t)(xyzi_.size() / 4), &o_), h_, "llsr_process_scan");
  }

  // ... with the IMU de-skew of adjustDistortion (FA:600-690): stamp = the cloud's header stamp
  // (timeScanCur, FA:2761); takes the scan's window from `imu` here, on this thread
  template <class Cloud>
  void run(const Cloud& laser_cloud_in, int32_t stamp_sec, uint32_t stamp_nanosec, ImuInput& imu) {
    imu.window(imu_window_);
    const int64_t off[2] = {0, imu_window_.n > 0 ? imu_window_.n + 1 : 0};
    check(llsr_stage_imu(h_, &stamp_sec, &stamp_nanosec, imu_window_.samples, off, 1), h_, "llsr_stage_imu");
    run(laser_cloud_in);
  }
  // FeatureAssociation's IMU members after the last scan
  llsr_imu_report imu_report() const {
    llsr_imu_report r;
    check(llsr_fetch_imu_report(h_, 0, &r), h_, "llsr_fetch_imu_report");
    return r;
  }

  // the marshalling below, on this handle's last scan
  template <class CloudInfo>
  void cloud_info(CloudInfo& msg) const { llsr_ros2::cloud_info(o_, rings_, msg); }
  template <class ProjOut, class Cloud>
  void projection_out(ProjOut& po, Cloud& segmented_cloud, Cloud& outlier_cloud) const {
    llsr_ros2::projection_out(o_, rings_, po, segmented_cloud, outlier_cloud);
  }
  template <class Cloud>
  void features(Cloud& segmented_cloud, Cloud& corner_sharp, Cloud& corner_less_sharp, Cloud& surf_flat,
                Cloud& surf_less_flat) const {
    llsr_ros2::features(o_, shadow_.data(), (int32_t)(shadow_.size() / 4), segmented_cloud, corner_sharp,
                        corner_less_sharp, surf_flat, surf_less_flat);
  }
  // publishClouds' ProjectionOut (IP:933-1000) with this scan's feature clouds in po.features, built
  // on the IP thread before Channel::send; po.segmented_cloud / outlier_cloud must be allocated
  template <class ProjOut>
  void handoff(ProjOut& po) const {
    projection_out(po, *po.segmented_cloud, *po.outlier_cloud);
    features(po.features.segmented, po.features.corner_sharp, po.features.corner_less_sharp, po.features.surf_flat,
             po.features.surf_less_flat);
    po.features.imu = imu_report();
  }

 private:
  llsr_handle* h_ = nullptr;
  int32_t rings_ = 0;
  size_t cells_ = 0;
  llsr_scan_out o_ = llsr_scan_out();
  std::vector<float> xyzi_, seg_, loam_, lflat_, out_, rng_, sint_, oint_, shadow_;
  ImuInput::Window imu_window_;
  std::vector<int32_t> start_, end_, edge_, sharp_, flat_;
  std::vector<uint8_t> gflag_;
  std::vector<uint32_t> col_;
};

// updateTransformation (FA:2505-2535) with its member state: transformCur[6] and isDegenerate in
// and out; returns the report (corner_iterations = iterCount2, the odometry_itertimes entry)
template <class Cloud>
llsr_s2s_report update_transformation(llsr_handle* h, const Cloud& corner_sharp, const Cloud& surf_flat,
                                      const Cloud& corner_last, const Cloud& surf_last, float transform_cur[6],
                                      bool& is_degenerate) {
  std::vector<float> a, b, c, d;
  repack_xyzi(corner_sharp, a);
  repack_xyzi(surf_flat, b);
  repack_xyzi(corner_last, c);
  repack_xyzi(surf_last, d);
  int32_t deg = is_degenerate ? 1 : 0;
  llsr_s2s_report rep;
  check(llsr_scan2scan(h, a.data(), (int32_t)(a.size() / 4), b.data(), (int32_t)(b.size() / 4), c.data(),
                       (int32_t)(c.size() / 4), d.data(), (int32_t)(d.size() / 4), transform_cur, &deg, &rep),
        h, "llsr_scan2scan");
  is_degenerate = deg != 0;
  return rep;
}

// runFeatureAssociation from `if (!systemInitedLM)` on (FA:2777-2796) for the FA node's thread, on
// its own handle and its own clouds: checkSystemInitialization (FA:2291-2315) on the first scan,
// then updateTransformation (FA:2505-2535), integrateTransformation (FA:2537-2568) and
// publishCloudsLast (FA:2660-2712: TransformToEnd of the less-sharp / less-flat clouds, which
// become the last clouds + the shadow points, and of the sharp / flat clouds, MO's scan clouds).
// The reference's order (FA:2781-2796) is solve(f), then OdomInput::apply(transform_sum,
// transform_cur) for updateInitialGuess (FA:2790), then finish(f), then the node's publishOdometry;
// step(f) = solve + finish leaves the LM's transformCur in place (LLSR_MODE_LM_APPLIED semantics).
// Either way transform_cur carries over as the next LM's initial guess.
// With use_imu_undistortion (the YAML switch, the constructor's argument) the order is
// OdomInput::apply before solve(f) as well (the updateInitialGuess at FA:2786-2788: the LM starts
// from the guess), solve(f), apply, finish(f); the scan's IMU report rides in f.imu
// (Projection::handoff). checkSystemInitialization then adds imuPitchStart / imuRollStart to
// transform_sum (FA:2329-2332), integrateTransformation ends in PluginIMURotation (FA:2557-2560) and
// TransformToEnd runs its IMU tail (FA:1456-1483).
template <class Cloud>
class Odometry {
 public:
  explicit Odometry(int32_t lidar, int32_t device = 0, bool use_imu_undistortion = false)
      : use_imu_undistortion(use_imu_undistortion), h_(lidar, device) {
    shadow_.resize(4 * 160);
    check(llsr_shadow_points(shadow_.data()), nullptr, "llsr_shadow_points");
  }
  llsr_handle* handle() const { return h_.get(); }
  bool initialised() const { return inited_; }

  // one scan's features (moved from the channel's ProjectionOut): checkSystemInitialization on the
  // first scan (returns false: the `continue` at FA:2781-2784, finish must not follow), else
  // updateTransformation (FA:2789)
  bool solve(FeatureClouds<Cloud>& f) {
    if (!inited_) {
      corner_last = std::move(f.corner_less_sharp);
      surf_last = std::move(f.surf_less_flat);
      append_xyzi(shadow_.data(), (int32_t)(shadow_.size() / 4), surf_last);
      if (use_imu_undistortion) check(llsr_first_scan_imu(transform_sum, &f.imu), nullptr, "llsr_first_scan_imu");
      inited_ = true;
      return false;
    }
    report = update_transformation(h_.get(), f.corner_sharp, f.surf_flat, corner_last, surf_last, transform_cur,
                                   is_degenerate);
    return true;
  }
  // integrateTransformation and publishCloudsLast's four TransformToEnd (FA:2792-2796) with whatever
  // transform_cur then holds
  void finish(FeatureClouds<Cloud>& f) {
    if (use_imu_undistortion) {
      check(llsr_integrate_transformation_imu(transform_sum, transform_cur, &f.imu), nullptr,
            "llsr_integrate_transformation_imu");
      transform_to_end_imu(transform_cur, f.imu, f.corner_less_sharp, corner_last);
      transform_to_end_imu(transform_cur, f.imu, f.surf_less_flat, surf_last);
      append_xyzi(shadow_.data(), (int32_t)(shadow_.size() / 4), surf_last);
      transform_to_end_imu(transform_cur, f.imu, f.corner_sharp, corner_scan);
      transform_to_end_imu(transform_cur, f.imu, f.surf_flat, surf_scan);
      return;
    }
    check(llsr_integrate_transformation(transform_sum, transform_cur), nullptr, "llsr_integrate_transformation");
    transform_to_end(transform_cur, f.corner_less_sharp, corner_last);
    transform_to_end(transform_cur, f.surf_less_flat, surf_last);
    append_xyzi(shadow_.data(), (int32_t)(shadow_.size() / 4), surf_last);
    transform_to_end(transform_cur, f.corner_sharp, corner_scan);
    transform_to_end(transform_cur, f.surf_flat, surf_scan);
  }
  // solve then finish; false on the initialisation scan
  bool step(FeatureClouds<Cloud>& f) {
    if (!solve(f)) return false;
    finish(f);
    return true;
  }

  const bool use_imu_undistortion;
  // FA's member state after the last step
  float transform_cur[6] = {0, 0, 0, 0, 0, 0};
  float transform_sum[6] = {0, 0, 0, 0, 0, 0};
  bool is_degenerate = false;
  llsr_s2s_report report = llsr_s2s_report();
  Cloud corner_last, surf_last;   // laserCloudCornerLast / laserCloudSurfLast
  Cloud corner_scan, surf_scan;   // laserCloudCornerScan / laserCloudSurfScan (AssociationOut)

 private:
  Handle h_;
  bool inited_ = false;
  std::vector<float> shadow_;
};

// FeatureAssociation's /odom2 members (FA:277-287) behind a mutex: the subscription's callback runs
// on another thread than runFeatureAssociation. on_message is odomCallback (FA:354-383) for any
// message type with nav_msgs/Odometry's pose.pose.orientation / position fields; apply is
// updateInitialGuess (FA:2370-2402) with the latest sample (the zero sample before any message).
class OdomInput {
 public:
  OdomInput() { check(llsr_odom_init(&st_), nullptr, "llsr_odom_init"); }
  template <class Msg>
  void on_message(const Msg& msg) {
    llsr_odometry_msg m = llsr_odometry_msg();
    m.orientation[0] = msg.pose.pose.orientation.x;
    m.orientation[1] = msg.pose.pose.orientation.y;
    m.orientation[2] = msg.pose.pose.orientation.z;
    m.orientation[3] = msg.pose.pose.orientation.w;
    m.position[0] = msg.pose.pose.position.x;
    m.position[1] = msg.pose.pose.position.y;
    m.position[2] = msg.pose.pose.position.z;
    std::lock_guard<std::mutex> lk(m_);
    check(llsr_odom_callback(&st_, &m), nullptr, "llsr_odom_callback");
  }
  llsr_odom_sample sample() const {
    std::lock_guard<std::mutex> lk(m_);
    return st_.last;
  }
  int32_t messages() const {
    std::lock_guard<std::mutex> lk(m_);
    return st_.n_msgs;
  }
  void apply(const float transform_sum[6], float transform_cur[6]) const {
    const llsr_odom_sample s = sample();
    check(llsr_update_initial_guess(&s, transform_sum, transform_cur), nullptr, "llsr_update_initial_guess");
  }

 private:
  mutable std::mutex m_;
  llsr_odom_state st_;
};

// scan2MapOptimization (MO:1572-1610) once its guard (MO:1573: corner map > 10, surf map > 100)
// holds: kd-tree builds, corner / surf optimisation and LMOptimization on transformTobeMapped;
// the report's iterations feed MapIterTimes (MO:1587-1588), min_lambda / cf_mean localInfo
template <class Cloud>
llsr_lm_report scan2map_optimization(llsr_handle* h, const Cloud& corner_scan_ds, const Cloud& surf_total_last_ds,
                                     const Cloud& corner_from_map_ds, const Cloud& surf_from_map_ds,
                                     float transform_tobe_mapped[6]) {
  std::vector<float> a, b, c, d;
  repack_xyzi(corner_scan_ds, a);
  repack_xyzi(surf_total_last_ds, b);
  repack_xyzi(corner_from_map_ds, c);
  repack_xyzi(surf_from_map_ds, d);
  llsr_lm_report rep;
  check(llsr_scan2map(h, a.data(), (int32_t)(a.size() / 4), b.data(), (int32_t)(b.size() / 4), c.data(),
                      (int32_t)(c.size() / 4), d.data(), (int32_t)(d.size() / 4), transform_tobe_mapped, &rep),
        h, "llsr_scan2map");
  return rep;
}

#ifdef LLSR_ROS2_GLOBAL_MAP
// publishGlobalMapThread (MO:305-315) over llsr_map_global. Opt-in (define LLSR_ROS2_GLOBAL_MAP
// before including this header and link the HIP runtime): the helper owns the three device output
// buffers, which the rest of this header has no need for. run() counts its iterations and signals
// the thread on every fifth (MO:1913-1921): on_cycle() once per run() iteration, publish() when it
// returns true. The call counter that makes the first publish raw lives in the llsr_map.
template <class Cloud>
class GlobalMap {
 public:
  explicit GlobalMap(const llsr_global_map_config* cfg = nullptr) {
    if (cfg) cfg_ = *cfg;
    else check(llsr_global_map_config_default(&cfg_), nullptr, "llsr_global_map_config_default");
  }
  ~GlobalMap() {
    for (int k = 0; k < 3; ++k)
      if (dev_[k]) (void)hipFree(dev_[k]);
  }
  GlobalMap(const GlobalMap&) = delete;
  GlobalMap& operator=(const GlobalMap&) = delete;

  bool on_cycle() { return ++cycle_count_ % 5 == 0; }

  // publishGlobalMap (MO:775-892) around robot_pos (currentRobotPosPoint): the clouds of
  // /laser_cloud_surround, the edge feature map and the planar feature map. Must not overlap
  // another call on `m` (the reference takes mtx around its own use of the key poses, MO:785-790).
  void publish(llsr_map* m, const float robot_pos[3]) {
    for (int k = 0; k < 3; ++k) reserve(k, 1);  // a NULL output would be skipped
    int32_t rc = LLSR_ERANGE;
    for (int attempt = 0; attempt < 2 && rc == LLSR_ERANGE; ++attempt) {
      rc = llsr_map_global(m, &cfg_, robot_pos, dev_[0], cap_[0], dev_[1], cap_[1], dev_[2], cap_[2], &report, nullptr);
      if (rc != LLSR_ERANGE) break;
      const int64_t need[3] = {report.n_global, report.n_edge, report.n_planar};
      for (int k = 0; k < 3; ++k) reserve(k, need[k]);
    }
    if (rc != LLSR_OK) throw std::runtime_error(std::string("llsr: llsr_map_global: ") + llsr_map_last_error(m));
    fetch(0, report.n_global, global);
    fetch(1, report.n_edge, edge);
    fetch(2, report.n_planar, planar);
  }

  Cloud global, edge, planar;  // globalMapKeyFrames, edgeMapKeyFrames, planarMapKeyFrames
  llsr_global_map_report report = llsr_global_map_report();

 private:
  void reserve(int k, int64_t need) {
    if (need <= cap_[k]) return;
    if (dev_[k] && hipFree(dev_[k]) != hipSuccess) throw std::runtime_error("llsr: hipFree");
    dev_[k] = nullptr;
    cap_[k] = 0;
    void* p = nullptr;
    if (hipMalloc(&p, (size_t)need * 4 * sizeof(float)) != hipSuccess) throw std::runtime_error("llsr: hipMalloc");
    dev_[k] = static_cast<float*>(p);
    cap_[k] = need;
  }
  void fetch(int k, int64_t n, Cloud& c) {
    host_[k].resize(4 * (size_t)n);
    if (n && hipMemcpy(host_[k].data(), dev_[k], (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("llsr: hipMemcpy");
    unpack_xyzi(host_[k].data(), (int32_t)n, c);
  }
  llsr_global_map_config cfg_;
  int cycle_count_ = 0;
  float* dev_[3] = {nullptr, nullptr, nullptr};  // global, edge, planar
  int64_t cap_[3] = {0, 0, 0};
  std::vector<float> host_[3];
};
#endif  // LLSR_ROS2_GLOBAL_MAP

}  // namespace llsr_ros2
