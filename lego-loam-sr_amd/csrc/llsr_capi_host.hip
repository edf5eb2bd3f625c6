// llsr_capi_host.hip — the C ABI's pure host functions (no handle, no device work): the pose glue
// of MapOptimization and TransformFusion, FeatureAssociation's end of scan, and the /odom2 input.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/llsr.h"
#include "llsr_mapping.h"
#include "llsr_odo.h"
#include "llsr_imu.h"
#include "llsr_odom_guess.h"

extern "C" int32_t llsr_mapping_associate(const float* ts_fa, const float* bef, const float* aft, float* ts,
                                          float* tobe, float* incre) {
  if (!ts_fa || !bef || !aft || !ts || !tobe) return LLSR_EINVAL;
  llsr_mapping::MoPoses P;
  for (int k = 0; k < 6; ++k) {
    P.transformBefMapped[k] = bef[k];
    P.transformAftMapped[k] = aft[k];
  }
  llsr_mapping::odometry_roundtrip(ts_fa, P.transformSum);
  llsr_mapping::transform_associate_to_map(P);
  for (int k = 0; k < 6; ++k) {
    ts[k] = P.transformSum[k];
    tobe[k] = P.transformTobeMapped[k];
    if (incre) incre[k] = P.transformIncre[k];
  }
  return LLSR_OK;
}

// ---- TransformFusion (transformFusion.cpp, TF:65-304): host-side scalar glue ----------------
extern "C" int32_t llsr_fusion_init(llsr_fusion_state* st) {
  if (!st) return LLSR_EINVAL;
  std::memset(st, 0, sizeof *st);
  return LLSR_OK;
}

extern "C" int32_t llsr_pose_to_odometry(const float* pose, const float* twist6, llsr_odometry_msg* out) {
  if (!pose || !out) return LLSR_EINVAL;
  llsr_mapping::pose_to_odometry(pose, twist6, *out);
  return LLSR_OK;
}

extern "C" int32_t llsr_odometry_to_transform(const llsr_odometry_msg* in, float* transform) {
  if (!in || !transform) return LLSR_EINVAL;
  llsr_mapping::odometry_to_transform(*in, transform);
  return LLSR_OK;
}

extern "C" int32_t llsr_fusion_laser_odometry(llsr_fusion_state* st, const llsr_odometry_msg* laser_odometry,
                                              llsr_odometry_msg* integrated) {
  if (!st || !laser_odometry || !integrated) return LLSR_EINVAL;
  // TF:190-192: OdometryToTransform, then transformAssociateToMap (TF:65-186 = MO:458-581 with
  // transformMapped in place of transformTobeMapped)
  llsr_mapping::MoPoses P;
  llsr_mapping::odometry_to_transform(*laser_odometry, P.transformSum);
  for (int k = 0; k < 6; ++k) {
    P.transformBefMapped[k] = st->transform_bef_mapped[k];
    P.transformAftMapped[k] = st->transform_aft_mapped[k];
    P.transformIncre[k] = st->transform_incre[k];
  }
  llsr_mapping::transform_associate_to_map(P);
  for (int k = 0; k < 6; ++k) {
    st->transform_sum[k] = P.transformSum[k];
    st->transform_incre[k] = P.transformIncre[k];
    st->transform_mapped[k] = P.transformTobeMapped[k];
  }
  // TF:194-206: q.setRPY(mapped[2], -mapped[0], -mapped[1]); /integrated_to_init
  llsr_mapping::pose_to_odometry(st->transform_mapped, nullptr, *integrated);
  return LLSR_OK;
}

extern "C" int32_t llsr_fusion_aft_mapped(llsr_fusion_state* st, const llsr_odometry_msg* m) {
  if (!st || !m) return LLSR_EINVAL;
  llsr_mapping::odometry_to_transform(*m, st->transform_aft_mapped);  // TF:284-297: -pitch, -yaw, roll, position
  for (int k = 0; k < 3; ++k) {                                       // TF:299-304
    st->transform_bef_mapped[k] = (float)m->twist_angular[k];
    st->transform_bef_mapped[3 + k] = (float)m->twist_linear[k];
  }
  return LLSR_OK;
}

// ---- FA end of scan on the FA node's own thread (host side, no handle) ------------------------
// integrateTransformation (FA:2537-2568) and TransformToEnd (FA:1414-1490) as k_odo_finish runs
// them, for a node whose FA thread owns its clouds: the same functions
// (llsr_odo.h) compiled for the host, with the same glibc-exact sin / cos / asin / atan2 ports.
extern "C" int32_t llsr_integrate_transformation(float* transform_sum, const float* transform_cur) {
  if (!transform_sum || !transform_cur) return LLSR_EINVAL;
  float ts[6], tc[6];
  for (int k = 0; k < 6; ++k) {
    ts[k] = transform_sum[k];
    tc[k] = transform_cur[k];
  }
  llsr::odo_integrate(ts, tc);
  for (int k = 0; k < 6; ++k) transform_sum[k] = ts[k];
  return LLSR_OK;
}

extern "C" int32_t llsr_transform_to_end(const float* transform_cur, const float* in_xyzi, int32_t n,
                                         float* out_xyzi) {
  if (!transform_cur || n < 0 || (n > 0 && (!in_xyzi || !out_xyzi))) return LLSR_EINVAL;
  float tc[6];
  for (int k = 0; k < 6; ++k) tc[k] = transform_cur[k];
  for (int32_t i = 0; i < n; ++i) {  // in place allowed: each row is read before it is written
    const float* r = in_xyzi + 4 * (size_t)i;
    const float4 q = llsr::odo_to_end(tc, make_float4(r[0], r[1], r[2], r[3]));
    float* o = out_xyzi + 4 * (size_t)i;
    o[0] = q.x;
    o[1] = q.y;
    o[2] = q.z;
    o[3] = q.w;
  }
  return LLSR_OK;
}

// ---- the same with use_imu_undistortion == true: the functions k_odo_finish_imu runs (llsr_odo.h)
extern "C" int32_t llsr_integrate_transformation_imu(float* transform_sum, const float* transform_cur,
                                                     const llsr_imu_report* report) {
  if (!transform_sum || !transform_cur || !report) return LLSR_EINVAL;
  float ts[6], tc[6];
  for (int k = 0; k < 6; ++k) { ts[k] = transform_sum[k]; tc[k] = transform_cur[k]; }
  llsr::odo_integrate_imu(ts, tc, report->start, report->cur);
  for (int k = 0; k < 6; ++k) transform_sum[k] = ts[k];
  return LLSR_OK;
}

extern "C" int32_t llsr_first_scan_imu(float* transform_sum, const llsr_imu_report* report) {
  if (!transform_sum || !report) return LLSR_EINVAL;
  llsr::odo_first_scan_imu(transform_sum, report->start);
  return LLSR_OK;
}

extern "C" int32_t llsr_transform_to_end_imu(const float* transform_cur, const llsr_imu_report* report,
                                             const float* in_xyzi, int32_t n, float* out_xyzi) {
  if (!transform_cur || !report || n < 0 || (n > 0 && (!in_xyzi || !out_xyzi))) return LLSR_EINVAL;
  float tc[6];
  for (int k = 0; k < 6; ++k) tc[k] = transform_cur[k];
  llsr::OdoImuTail tail;
  llsr::odo_imu_tail_set(tail, report->start, report->cur);
  for (int32_t i = 0; i < n; ++i) {  // in place allowed: each row is read before it is written
    const float* r = in_xyzi + 4 * (size_t)i;
    const float4 q = llsr::odo_imu_tail(tail, llsr::odo_to_end(tc, make_float4(r[0], r[1], r[2], r[3])));
    float* o = out_xyzi + 4 * (size_t)i;
    o[0] = q.x;
    o[1] = q.y;
    o[2] = q.z;
    o[3] = q.w;
  }
  return LLSR_OK;
}

// ---- /odom2 and updateInitialGuess (FA:354-383, 2337-2402): host-side scalar glue, llsr_odom_guess.h
extern "C" int32_t llsr_odom_init(llsr_odom_state* st) {
  if (!st) return LLSR_EINVAL;
  std::memset(st, 0, sizeof *st);  // FA:277-287; `last` = the zero sample ("no message yet")
  return LLSR_OK;
}

extern "C" int32_t llsr_odom_callback(llsr_odom_state* st, const llsr_odometry_msg* msg) {
  if (!st || !msg) return LLSR_EINVAL;
  llsr_odom::callback(*st, *msg);
  return LLSR_OK;
}

extern "C" int32_t llsr_update_initial_guess(const llsr_odom_sample* sample, const float* transform_sum,
                                             float* transform_cur) {
  if (!sample || !transform_sum || !transform_cur) return LLSR_EINVAL;
  float ts[6];
  for (int k = 0; k < 6; ++k) ts[k] = transform_sum[k];  // transform_cur may alias transform_sum
  llsr_odom::update_initial_guess(*sample, ts, transform_cur);
  return LLSR_OK;
}

// ---- /imu_type and adjustDistortion's IMU de-skew (FA:315-351, 452-563, 600-690, 788): llsr_imu.h
extern "C" int32_t llsr_imu_init(llsr_imu_state* st) {
  if (!st) return LLSR_EINVAL;
  llsr_imu::init(*st);
  return LLSR_OK;
}

extern "C" int32_t llsr_imu_callback(llsr_imu_state* st, const llsr_imu_msg* msg, float scan_period) {
  if (!st || !msg || st->pointer_last < -1 || st->pointer_last >= LLSR_IMU_QUEUE) return LLSR_EINVAL;
  double roll, pitch, yaw;
  llsr_mapping::tf2_get_rpy(msg->orientation, roll, pitch, yaw);  // tf2::convert copies x, y, z, w
  llsr_imu::callback_rpy(*st, *msg, roll, pitch, yaw, scan_period);
  return LLSR_OK;
}

extern "C" int32_t llsr_imu_scan_window(llsr_imu_state* st, llsr_imu_sample* out, int32_t* n) {
  if (!st || !out || !n || st->pointer_last < -1 || st->pointer_last >= LLSR_IMU_QUEUE ||
      st->pointer_last_iteration < -1 || st->pointer_last_iteration >= LLSR_IMU_QUEUE)
    return LLSR_EINVAL;
  *n = llsr_imu::scan_window(*st, out);
  return LLSR_OK;
}

extern "C" int32_t llsr_imu_deskew_host(const llsr_config* cfg, int32_t scan_time_sec, uint32_t scan_time_nanosec,
                                        const llsr_imu_sample* window, int32_t n, const float* seg_xyzi, int32_t S,
                                        const float* orientation, llsr_imu_carry* carry, float* loam_xyzi_out,
                                        llsr_imu_report* report) {
  if (!cfg || !orientation || !carry || n < 0 || n > LLSR_IMU_QUEUE || (n > 0 && !window) || S < 0 ||
      (S > 0 && (!seg_xyzi || !loam_xyzi_out)))
    return LLSR_EINVAL;
  const double scan_time = scan_time_sec + scan_time_nanosec / 1e9;  // FA:2761
  llsr_imu::deskew_host(cfg->scan_period, scan_time, window, n, seg_xyzi, S, orientation, carry, loam_xyzi_out);
  if (report) *report = carry->report;
  return LLSR_OK;
}
