// llsr_odom_guess.h — the /odom2 input of FeatureAssociation and the updateInitialGuess that runs
// after every scan-to-scan LM (featureAssociation.cpp:2790): host-side scalar glue like
// llsr_mapping.h, evaluated the way the reference's x86-64 GCC -O3 build (SSE2, no -march, Eigen
// 3.3.7, no FMA contraction) evaluates it. The transcendental calls are the host glibc's double
// sincos / atan2 / sqrt, the functions the reference itself calls.
//   * odomCallback (FA:354-383): tf2 getRPY of the message orientation, position relative to the
//     first message;
//   * updateInitialGuess (FA:2370-2402): transformCur rebuilt from the latest /odom2 sample and
//     transformSum. Its IMU member copies (FA:2339-2349) need no state here: with
//     use_imu_undistortion on, k_odo_finish_imu reads the scan's imu*Cur as imu*Last.
// Evaluation order restated here (unpinned: neither Eigen nor tf2 is available to
// check against):
//   * AngleAxisd * AngleAxisd * AngleAxisd is (Quaterniond(a) * Quaterniond(b)) * Quaterniond(c)
//     (AngleAxis::operator* returns a quaternion product), assigned to a Matrix3d through
//     Quaternion::toRotationMatrix;
//   * Quaterniond(AngleAxisd) is w = cos(angle / 2), vec = sin(angle / 2) * axis; GCC merges the
//     cos / sin pair of one argument into one glibc sincos call (as in tf2_set_rpy, llsr_mapping.h);
//   * the quaternion product is Eigen's SSE2 specialisation for double (Geometry_SSE.h): two
//     packets of two products each, combined as t1 -/+ swap(t2);
//   * a 3-term dot product of the fixed-size matrix products is Eigen's redux: with both operands
//     contiguous (the row of a transposed Matrix3d against a column) the first two products are
//     summed as one packet and the third added, (p0 + p1) + p2; with a strided operand (the row of a
//     Matrix3d against a vector) the unrolled scalar redux halves the range, p0 + (p1 + p2).
#pragma once
#include <cmath>

#include "../../include/llsr.h"
#include "llsr_mapping.h"

namespace llsr_odom {

struct Quat { double x, y, z, w; };

// Eigen::Quaterniond(Eigen::AngleAxisd(angle, unit axis `axis`))
inline Quat quat_axis(double angle, int axis) {
  const double ha = 0.5 * angle;
  double s, c;
  ::sincos(ha, &s, &c);
  Quat q;
  q.w = c;
  q.x = s * (axis == 0 ? 1.0 : 0.0);
  q.y = s * (axis == 1 ? 1.0 : 0.0);
  q.z = s * (axis == 2 ? 1.0 : 0.0);
  return q;
}

// quat_product<Architecture::SSE, ..., double> (Eigen 3.3.7 Geometry_SSE.h)
inline Quat quat_mul(const Quat& a, const Quat& b) {
  Quat r;
  double t1x = a.w * b.x + a.y * b.z, t1y = a.w * b.y + a.y * b.w;
  double t2x = a.z * b.x - a.x * b.z, t2y = a.z * b.y - a.x * b.w;
  r.x = t1x - t2y;
  r.y = t1y + t2x;
  t1x = a.w * b.z - a.y * b.x; t1y = a.w * b.w - a.y * b.y;
  t2x = a.z * b.z + a.x * b.x; t2y = a.z * b.w + a.x * b.y;
  r.w = t1y - t2x;
  r.z = t1x + t2y;
  return r;
}

// QuaternionBase::toRotationMatrix, m[row][col]
inline void quat_matrix(const Quat& q, double m[3][3]) {
  const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  m[0][0] = 1.0 - (tyy + tzz); m[0][1] = txy - twz; m[0][2] = txz + twy;
  m[1][0] = txy + twz; m[1][1] = 1.0 - (txx + tzz); m[1][2] = tyz - twx;
  m[2][0] = txz - twy; m[2][1] = tyz + twx; m[2][2] = 1.0 - (txx + tyy);
}

// AngleAxisd(a, axis a_ax) * AngleAxisd(b, b_ax) * AngleAxisd(c, c_ax) assigned to a Matrix3d
inline void euler_matrix(double a, int a_ax, double b, int b_ax, double c, int c_ax, double m[3][3]) {
  quat_matrix(quat_mul(quat_mul(quat_axis(a, a_ax), quat_axis(b, b_ax)), quat_axis(c, c_ax)), m);
}

// odomCallback (FA:354-383). The reference's 200-entry ring is only ever read at odomPointerLast,
// so keeping the latest sample is equivalent.
inline void callback(llsr_odom_state& st, const llsr_odometry_msg& msg) {
  double roll, pitch, yaw;
  llsr_mapping::tf2_get_rpy(msg.orientation, roll, pitch, yaw);  // tf2::convert copies x, y, z, w
  if (st.initial_iter == 0) {
    for (int k = 0; k < 3; ++k) st.origin[k] = msg.position[k];
    st.initial_iter += 1;
  }
  st.n_msgs += 1;
  st.last.roll = (float)roll;
  st.last.pitch = (float)pitch;
  st.last.yaw = (float)yaw;
  st.last.x = (float)(msg.position[0] - st.origin[0]);
  st.last.y = (float)(msg.position[1] - st.origin[1]);
  st.last.z = (float)(msg.position[2] - st.origin[2]);
}

// updateInitialGuess (FA:2370-2402): reads transformSum, overwrites all of transformCur
inline void update_initial_guess(const llsr_odom_sample& o, const float ts[6], float tc[6]) {
  double now[3][3], last[3][3];
  euler_matrix((double)o.yaw, 2, (double)o.pitch, 1, (double)o.roll, 0, now);     // FA:2372-2374
  euler_matrix((double)ts[1], 2, (double)ts[0], 1, (double)ts[2], 0, last);       // FA:2378-2380
  // rotationFromStartToEnd = (last^T * now)^T (FA:2381-2382): r[i][j] = sum_k last[k][j] * now[k][i]
  double r[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      r[i][j] = (last[0][j] * now[0][i] + last[1][j] * now[1][i]) + last[2][j] * now[2][i];
  const float odomX = (float)std::atan2(r[2][1], r[2][2]);                                        // FA:2386
  const float odomY = (float)std::atan2(-r[2][0], std::sqrt(r[2][1] * r[2][1] + r[2][2] * r[2][2]));  // FA:2387
  const float odomZ = (float)std::atan2(r[1][0], r[0][0]);                                        // FA:2388
  tc[0] = odomY;
  tc[1] = odomZ;
  tc[2] = odomX;
  const double body[3] = {0.08, 0.0, 0.0377};  // outer_param_body
  double global[3];                            // rotation_matrix_now * outer_param_body
  for (int i = 0; i < 3; ++i) global[i] = now[i][0] * body[0] + (now[i][1] * body[1] + now[i][2] * body[2]);
  // the lever arm enters twice, as written (FA:2398)
  const double tv[3] = {(double)ts[5] - (((double)o.x + body[0]) + global[0]),
                        (double)ts[3] - (((double)o.y + body[1]) + global[1]),
                        (double)ts[4] - (((double)o.z + body[2]) + global[2])};
  double tb[3];  // rotation_matrix_last.transpose() * transVector
  for (int i = 0; i < 3; ++i) tb[i] = (last[0][i] * tv[0] + last[1][i] * tv[1]) + last[2][i] * tv[2];
  tc[5] = (float)tb[0];
  tc[3] = (float)tb[1];
  tc[4] = (float)tb[2];
}

}  // namespace llsr_odom
