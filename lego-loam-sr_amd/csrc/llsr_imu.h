// llsr_imu.h — the /imu_type input of FeatureAssociation and adjustDistortion's IMU de-skew
// (featureAssociation.cpp = FA, lines 315-351, 452-563, 600-690, 788).
//   * host only: imuHandler + AccumulateIMUShiftAndRotation on the 200-entry ring (callback), the
//     linear window one scan can read (scan_window), adjustDistortion of one scan serially
//     (deskew_host);
//   * host and device: the per-point body (deskew_point: the queue search, the blend, the rotation
//     into the scan-start frame) and the point-0 / last-point member updates. k_fa_points<true> and
//     deskew_host call the same functions; the float libm is glibc's on the host (the functions the
//     reference calls) and the llsr_libm.h ports on the device.
// Typing follows the reference's members: imuTime and timeScanCur are double, everything else float;
// built with -ffp-contract=off (a * rf + b * rb is two multiplies and an add).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/llsr.h"
#include "llsr_libm.h"

namespace llsr_imu {

constexpr int kQueue = LLSR_IMU_QUEUE;
constexpr double kPi = 3.14159265358979323846;

LLSR_HD float sin_f(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return llsr_libm::sinf_(x);
#else
  return ::sinf(x);
#endif
}
LLSR_HD float cos_f(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return llsr_libm::cosf_(x);
#else
  return ::cosf(x);
#endif
}

// A scan's window as the body reads it: entry 0 is the back of the first candidate, the candidates
// are 1 .. n (llsr_imu_scan_window). Times and angles only: every point needs them; the velocity
// and angular-rotation entries are read by point 0 and the last point alone (blend3 below).
struct Window {
  const double* time;
  const float *roll, *pitch, *yaw;
  int n;
};

// Where a point's time falls in the window (FA:603-628): the candidate the walk stops at, and either
// "newer than it: take its entries" or the two float ratios, each narrowed from a double quotient
// (a zero or negative divisor is plain IEEE: inf / NaN / extrapolation).
struct Sel {
  int front;
  int take;
  float rf, rb;
};

LLSR_HD Sel select(const Window& w, double scan_time, float point_time) {
  Sel s;
  int front = 1;  // imuPointerLastIteration: every point restarts there
  while (front != w.n) {
    if (scan_time + point_time < w.time[front]) break;
    ++front;
  }
  s.front = front;
  s.take = scan_time + point_time > w.time[front] ? 1 : 0;
  s.rf = 0.0f;
  s.rb = 0.0f;
  if (!s.take) {
    const double tf = w.time[front], tb = w.time[front - 1];
    s.rf = (float)((scan_time + point_time - tb) / (tf - tb));
    s.rb = (float)((tf - scan_time - point_time) / (tf - tb));
  }
  return s;
}

// front * ratioFront + back * ratioBack in float (FA:630-646), or front's entry
LLSR_HD float blend(const Sel& s, float front, float back) { return s.take ? front : front * s.rf + back * s.rb; }

// imuYawCur (FA:632-638): the +-pi wrap branches promote the blend to double
LLSR_HD float blend_yaw(const Sel& s, float front, float back) {
  if (s.take) return front;
  if (front - back > kPi) return (float)(front * s.rf + (back + 2 * kPi) * s.rb);
  if (front - back < -kPi) return (float)(front * s.rf + (back - 2 * kPi) * s.rb);
  return front * s.rf + back * s.rb;
}

// a three-float member of the window's samples (velo, angular_rotation) at the point's time
LLSR_HD void blend3(const Sel& s, const llsr_imu_sample* win, int member_offset, float out[3]) {
  const float* f = reinterpret_cast<const float*>(reinterpret_cast<const char*>(&win[s.front]) + member_offset);
  const float* b = reinterpret_cast<const float*>(reinterpret_cast<const char*>(&win[s.front - 1]) + member_offset);
  for (int k = 0; k < 3; ++k) out[k] = blend(s, f[k], b[k]);
}
constexpr int kVeloOffset = offsetof(llsr_imu_sample, velo), kAngularOffset = offsetof(llsr_imu_sample, angular_rotation);
static_assert(sizeof(llsr_imu_sample) == 56, "llsr_imu_sample: double time, twelve floats");

// The start state point 0 latches (FA:650-652, 685; updateImuRollPitchYawStartSinCos FA:491-498) and
// where its time fell (the last point's VeloToStartIMU needs imuVelo*Start from the same blend).
struct Start {
  float roll, pitch, yaw;
  float cr, cp, cy, sr, sp, sy;
  Sel sel;
};

LLSR_HD void latch_start(const float cur[3], const Sel& sel, Start* st) {
  st->roll = cur[0];
  st->pitch = cur[1];
  st->yaw = cur[2];
  st->cr = cos_f(cur[0]);
  st->cp = cos_f(cur[1]);
  st->cy = cos_f(cur[2]);
  st->sr = sin_f(cur[0]);
  st->sp = sin_f(cur[1]);
  st->sy = sin_f(cur[2]);
  st->sel = sel;
}

// TransformToStartIMU (FA:538-563): six float sin / cos of the point's own angles, five plane
// rotations, + imuShiftFromStart*Cur. ShiftToStartIMU is never called, so that member stays at the
// constructor's 0; the add stays in the expression (-0.0f becomes +0.0f).
LLSR_HD void transform_to_start(const Start& st, const float cur[3], float* px, float* py, float* pz) {
  const float shift_from_start = 0.0f;
  const float cr = cos_f(cur[0]), sr = sin_f(cur[0]);
  const float cp = cos_f(cur[1]), sp = sin_f(cur[1]);
  const float cy = cos_f(cur[2]), sy = sin_f(cur[2]);
  const float x1 = cr * *px - sr * *py;
  const float y1 = sr * *px + cr * *py;
  const float z1 = *pz;
  const float x2 = x1;
  const float y2 = cp * y1 - sp * z1;
  const float z2 = sp * y1 + cp * z1;
  const float x3 = cy * x2 + sy * z2;
  const float y3 = y2;
  const float z3 = -sy * x2 + cy * z2;
  const float x4 = st.cy * x3 - st.sy * z3;
  const float y4 = y3;
  const float z4 = st.sy * x3 + st.cy * z3;
  const float x5 = x4;
  const float y5 = st.cp * y4 + st.sp * z4;
  const float z5 = -st.sp * y4 + st.cp * z4;
  *px = st.cr * x5 + st.sr * y5 + shift_from_start;
  *py = -st.sr * x5 + st.cr * y5 + shift_from_start;
  *pz = z5 + shift_from_start;
}

// The per-point body (FA:602-647, 686-689): pointTime, the search, the blend of the three angles
// into cur[] and, for every point but the scan's first, the rotation of (x, y, z) into the start
// frame. rel_time is adjustDistortion's relTime of the point; *sel receives where its time fell.
LLSR_HD void deskew_point(const Window& w, double scan_time, float scan_period, float rel_time, bool first,
                          const Start& st, float cur[3], Sel* sel, float* px, float* py, float* pz) {
  const float point_time = rel_time * scan_period;
  const Sel s = select(w, scan_time, point_time);
  const int f = s.front, b = s.front - 1;
  cur[0] = blend(s, w.roll[f], w.roll[b]);
  cur[1] = blend(s, w.pitch[f], w.pitch[b]);
  cur[2] = blend_yaw(s, w.yaw[f], w.yaw[b]);
  *sel = s;
  if (!first) transform_to_start(st, cur, px, py, pz);
}

// Point 0's member updates beyond the start latch (FA:662-683): imuAngularRotation*Cur from the same
// blend, imuAngularFromStart = Cur - Last, Last = Cur; and the report's start angles.
LLSR_HD void first_point_members(const Start& st, const llsr_imu_sample* win, llsr_imu_carry* c) {
  float ar[3];
  blend3(st.sel, win, kAngularOffset, ar);
  for (int k = 0; k < 3; ++k) {
    c->report.angular_from_start[k] = ar[k] - c->angular_rotation_last[k];
    c->angular_rotation_last[k] = ar[k];
  }
  c->report.start[0] = st.roll;
  c->report.start[1] = st.pitch;
  c->report.start[2] = st.yaw;
}

// The last point's members: imuRoll/Pitch/YawCur and, when it is not point 0, VeloToStartIMU
// (FA:519-536) of its imuVelo*Cur against point 0's imuVelo*Start.
LLSR_HD void last_point_members(const Start& st, const Sel& sel, const float cur[3], bool is_first,
                                const llsr_imu_sample* win, llsr_imu_report* r) {
  for (int k = 0; k < 3; ++k) r->cur[k] = cur[k];
  if (is_first) return;
  float vs[3], vc[3];
  blend3(st.sel, win, kVeloOffset, vs);
  blend3(sel, win, kVeloOffset, vc);
  const float fx = vc[0] - vs[0], fy = vc[1] - vs[1], fz = vc[2] - vs[2];
  const float x1 = st.cy * fx - st.sy * fz;
  const float y1 = fy;
  const float z1 = st.sy * fx + st.cy * fz;
  const float x2 = x1;
  const float y2 = st.cp * y1 + st.sp * z1;
  const float z2 = -st.sp * y1 + st.cp * z1;
  r->velo_from_start[0] = st.cr * x2 + st.sr * y2;
  r->velo_from_start[1] = -st.sr * x2 + st.cr * y2;
  r->velo_from_start[2] = z2;
}

// ---- host side ------------------------------------------------------------------------------

inline void init(llsr_imu_state& st) {
  st = llsr_imu_state{};
  st.pointer_last = -1;
  st.pointer_last_iteration = 0;
}

// imuHandler (FA:315-351) with the roll / pitch / yaw of the message (tf2 getRPY, double), then
// AccumulateIMUShiftAndRotation (FA:452-489)
inline void callback_rpy(llsr_imu_state& st, const llsr_imu_msg& m, double roll, double pitch, double yaw,
                         float scan_period) {
  const float accX0 = (float)(m.linear_acceleration[1] - ::sin(roll) * ::cos(pitch) * 9.81);
  const float accY0 = (float)(m.linear_acceleration[2] - ::cos(roll) * ::cos(pitch) * 9.81);
  const float accZ0 = (float)(m.linear_acceleration[0] + ::sin(pitch) * 9.81);
  const int last = (st.pointer_last + 1) % kQueue;
  st.pointer_last = last;
  st.time[last] = m.sec + m.nanosec / 1e9;
  st.roll[last] = (float)roll;
  st.pitch[last] = (float)pitch;
  st.yaw[last] = (float)yaw;
  st.acc[0][last] = accX0;
  st.acc[1][last] = accY0;
  st.acc[2][last] = accZ0;
  for (int k = 0; k < 3; ++k) st.angular_velo[k][last] = (float)m.angular_velocity[k];
  // the accumulate step: float sin / cos of the float angles
  const float r = st.roll[last], p = st.pitch[last], y = st.yaw[last];
  float accX = accX0, accY = accY0, accZ = accZ0;
  const float x1 = ::cosf(r) * accX - ::sinf(r) * accY;
  const float y1 = ::sinf(r) * accX + ::cosf(r) * accY;
  const float z1 = accZ;
  const float x2 = x1;
  const float y2 = ::cosf(p) * y1 - ::sinf(p) * z1;
  const float z2 = ::sinf(p) * y1 + ::cosf(p) * z1;
  accX = ::cosf(y) * x2 + ::sinf(y) * z2;
  accY = y2;
  accZ = -::sinf(y) * x2 + ::cosf(y) * z2;
  const float acc[3] = {accX, accY, accZ};
  const int back = (last + kQueue - 1) % kQueue;
  const double dt = st.time[last] - st.time[back];
  if (dt < scan_period) {  // each update in double (dt is), narrowed on the store
    for (int k = 0; k < 3; ++k) {
      st.shift[k][last] = (float)(st.shift[k][back] + st.velo[k][back] * dt + acc[k] * dt * dt / 2);
      st.velo[k][last] = (float)(st.velo[k][back] + acc[k] * dt);
      st.angular_rotation[k][last] = (float)(st.angular_rotation[k][back] + st.angular_velo[k][back] * dt);
    }
  }
}

inline llsr_imu_sample sample_at(const llsr_imu_state& st, int i) {
  llsr_imu_sample s;
  s.time = st.time[i];
  s.roll = st.roll[i];
  s.pitch = st.pitch[i];
  s.yaw = st.yaw[i];
  for (int k = 0; k < 3; ++k) {
    s.velo[k] = st.velo[k][i];
    s.shift[k] = st.shift[k][i];
    s.angular_rotation[k] = st.angular_rotation[k][i];
  }
  return s;
}

// the window of the scan that starts now, then FA:788 (include/llsr.h states the linearisation)
inline int scan_window(llsr_imu_state& st, llsr_imu_sample* out) {
  if (st.pointer_last < 0) {  // no message yet: FA:788 copies the -1
    st.pointer_last_iteration = -1;
    return 0;
  }
  // after such a scan the reference's walk starts at imuTime[-1], outside the array; here it starts at
  // entry 0, the first message
  const int first = st.pointer_last_iteration < 0 ? 0 : st.pointer_last_iteration;
  const int n = (st.pointer_last - first + kQueue) % kQueue + 1;
  for (int k = 0; k <= n; ++k) out[k] = sample_at(st, (first + kQueue - 1 + k) % kQueue);
  st.pointer_last_iteration = st.pointer_last;
  return n;
}

// adjustDistortion's LOAM swap and relative time of one point (FA:573-596), host libm; *half_passed is
// the loop's latch
inline float loam_swap(const float p[4], const float ori3[3], float scan_period, bool* half_passed, float out[4]) {
  const float start = ori3[0], endo = ori3[1], diff = ori3[2];
  const float x = p[1], y = p[2], z = p[0];
  float ori = -::atan2f(x, z);
  if (!*half_passed) {
    if (ori < start - kPi / 2) ori = (float)(ori + 2 * kPi);
    else if (ori > start + kPi * 3 / 2) ori = (float)(ori - 2 * kPi);
    if (ori - start > kPi) *half_passed = true;
  } else {
    ori = (float)(ori + 2 * kPi);
    if (ori < endo - kPi * 3 / 2) ori = (float)(ori + 2 * kPi);
    else if (ori > endo + kPi / 2) ori = (float)(ori - 2 * kPi);
  }
  const float rel = (ori - start) / diff;
  out[0] = x;
  out[1] = y;
  out[2] = z;
  out[3] = (float)(int)p[3] + scan_period * rel;
  return rel;
}

// FA:565-690 of one scan. win: n + 1 samples (n = 0: no IMU). The SoA copies are exactly n + 1 long.
inline void deskew_host(float scan_period, double scan_time, const llsr_imu_sample* win, int n, const float* seg, int S,
                        const float ori3[3], llsr_imu_carry* carry, float* out) {
  double* wt = nullptr;
  float* wa = nullptr;
  Window w{nullptr, nullptr, nullptr, nullptr, n};
  if (n > 0) {
    wt = new double[n + 1];
    wa = new float[3 * (size_t)(n + 1)];
    for (int k = 0; k <= n; ++k) {
      wt[k] = win[k].time;
      wa[k] = win[k].roll;
      wa[(n + 1) + k] = win[k].pitch;
      wa[2 * (n + 1) + k] = win[k].yaw;
    }
    w = Window{wt, wa, wa + (n + 1), wa + 2 * (n + 1), n};
  }
  bool half = false;
  Start st{};
  for (int i = 0; i < S; ++i) {
    float* o = out + 4 * (size_t)i;
    const float rel = loam_swap(seg + 4 * (size_t)i, ori3, scan_period, &half, o);
    if (n <= 0) continue;
    float cur[3];
    Sel sel;
    deskew_point(w, scan_time, scan_period, rel, i == 0, st, cur, &sel, &o[0], &o[1], &o[2]);
    if (i == 0) {
      latch_start(cur, sel, &st);
      first_point_members(st, win, carry);
    }
    if (i == S - 1) last_point_members(st, sel, cur, i == 0, win, &carry->report);
  }
  delete[] wt;
  delete[] wa;
}
}  // namespace llsr_imu
