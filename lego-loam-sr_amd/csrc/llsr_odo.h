// llsr_odo.h — device data of the end-to-end odometry batch (llsr_odo.hip, llsr_odometry_*).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "llsr_device.h"
#include "llsr_libm.h"

namespace llsr {

constexpr int kShadow = 160;  // GenerateShadowPoint: 16 x 10 virtual points (FA:412-450)

struct OdoArgs {
  int B, HW;
  const int* counts;                       // [B][kCnt] of the feature batch
  const float4* loam;                      // [B][HW] segmented cloud in the LOAM frame
  const int* sharp_ind;                    // [B][HW] cornerPointsSharp as segmented indices
  const int* flat_ind;                     // [B][HW] surfPointsFlat (without shadow points)
  const int* less_sharp;                   // [B][HW] cornerPointsLessSharp
  const float4* lflat;                     // [B][HW] surfPointsLessFlat points
  const float4* shadow;                    // [160]
  const int64_t* sharp_off; float4* sharp; // LM queries of this batch, packed [B+1]
  const int64_t* flat_off; float4* flat;
  const int64_t* nlast_c_off; float4* nlast_c;  // the next last clouds, packed [B+1]
  const int64_t* nlast_s_off; float4* nlast_s;
  float4* scan_c; float4* scan_s;          // TransformToEnd'd sharp / flat (offsets of sharp / flat)
  float* tcur;                             // [B][6] transformCur (after the LM)
  float* tsum;                             // [B][6] transformSum
  int* inited;                             // [B] systemInitedLM
  int* frames;                             // [B]
  // updateInitialGuess after the LM (FA:2790, llsr_odometry_batch_odom); all nullptr otherwise
  const float* guess;                      // [B][6] the transformCur it builds (host-evaluated)
  const unsigned char* flags;              // [B] slots whose transformCur it replaces
  float* tlm;                              // [B][6] the LM's own transformCur of those slots
};

__global__ void k_odo_inputs(OdoArgs a);
__global__ void k_odo_finish(OdoArgs a);
// use_imu_undistortion == true (llsr_set_imu_undistortion); carry: [max_batch] or nullptr
__global__ void k_odo_inputs_imu(OdoArgs a);
__global__ void k_odo_finish_imu(OdoArgs a, const llsr_imu_carry* carry);

// The per-scan pose arithmetic of FA's end of scan, shared by k_odo_finish and the host entry points
// llsr_transform_to_end / llsr_integrate_transformation (the FA node's thread calls those on its own
// clouds). Float typing and operation order follow the reference lines; sin / cos / asin / atan2 are
// the glibc ports of llsr_libm.h on both sides. The use_imu_undistortion == true branches (false in
// the shipped config blocks, CFG:59/127/195; llsr_set_imu_undistortion) are the *_imu functions
// below: k_odo_finish_imu and the llsr_*_imu host entry points.
using llsr_libm::asinf_;
using llsr_libm::atan2f_;
using llsr_libm::cosf_;
using llsr_libm::sinf_;

// TransformToEnd (FA:1414-1490) up to (x6, y6, z6): all of it when use_imu_undistortion is false,
// followed by odo_imu_tail when it is true.
__host__ __device__ __forceinline__ float4 odo_to_end(const float* tc, float4 pi) {
  const float s = 10 * (pi.w - (float)trunc_i32(pi.w));
  float rx = s * tc[0], ry = s * tc[1], rz = s * tc[2];
  float tx = s * tc[3], ty = s * tc[4], tz = s * tc[5];
  const float x1 = cosf_(rz) * (pi.x - tx) + sinf_(rz) * (pi.y - ty);
  const float y1 = -sinf_(rz) * (pi.x - tx) + cosf_(rz) * (pi.y - ty);
  const float z1 = (pi.z - tz);
  const float x2 = x1;
  const float y2 = cosf_(rx) * y1 + sinf_(rx) * z1;
  const float z2 = -sinf_(rx) * y1 + cosf_(rx) * z1;
  const float x3 = cosf_(ry) * x2 - sinf_(ry) * z2;
  const float y3 = y2;
  const float z3 = sinf_(ry) * x2 + cosf_(ry) * z2;
  rx = tc[0]; ry = tc[1]; rz = tc[2];
  tx = tc[3]; ty = tc[4]; tz = tc[5];
  const float x4 = cosf_(ry) * x3 + sinf_(ry) * z3;
  const float y4 = y3;
  const float z4 = -sinf_(ry) * x3 + cosf_(ry) * z3;
  const float x5 = x4;
  const float y5 = cosf_(rx) * y4 - sinf_(rx) * z4;
  const float z5 = sinf_(rx) * y4 + cosf_(rx) * z4;
  return make_float4(cosf_(rz) * x5 - sinf_(rz) * y5 + tx, sinf_(rz) * x5 + cosf_(rz) * y5 + ty, z5 + tz,
                     (float)trunc_i32(pi.w));
}

// AccumulateRotation (FA:1552-1578)
__host__ __device__ __forceinline__ void odo_accumulate_rotation(float cx, float cy, float cz, float lx, float ly, float lz,
                                                            float& ox, float& oy, float& oz) {
  const float srx = cosf_(lx) * cosf_(cx) * sinf_(ly) * sinf_(cz) - cosf_(cx) * cosf_(cz) * sinf_(lx) -
                    cosf_(lx) * cosf_(ly) * sinf_(cx);
  ox = -asinf_(srx);
  const float srycrx = sinf_(lx) * (cosf_(cy) * sinf_(cz) - cosf_(cz) * sinf_(cx) * sinf_(cy)) +
                       cosf_(lx) * sinf_(ly) * (cosf_(cy) * cosf_(cz) + sinf_(cx) * sinf_(cy) * sinf_(cz)) +
                       cosf_(lx) * cosf_(ly) * cosf_(cx) * sinf_(cy);
  const float crycrx = cosf_(lx) * cosf_(ly) * cosf_(cx) * cosf_(cy) -
                       cosf_(lx) * sinf_(ly) * (cosf_(cz) * sinf_(cy) - cosf_(cy) * sinf_(cx) * sinf_(cz)) -
                       sinf_(lx) * (sinf_(cy) * sinf_(cz) + cosf_(cy) * cosf_(cz) * sinf_(cx));
  oy = atan2f_(srycrx / cosf_(ox), crycrx / cosf_(ox));
  const float srzcrx = sinf_(cx) * (cosf_(lz) * sinf_(ly) - cosf_(ly) * sinf_(lx) * sinf_(lz)) +
                       cosf_(cx) * sinf_(cz) * (cosf_(ly) * cosf_(lz) + sinf_(lx) * sinf_(ly) * sinf_(lz)) +
                       cosf_(lx) * cosf_(cx) * cosf_(cz) * sinf_(lz);
  const float crzcrx = cosf_(lx) * cosf_(lz) * cosf_(cx) * cosf_(cz) -
                       cosf_(cx) * sinf_(cz) * (cosf_(ly) * sinf_(lz) - cosf_(lz) * sinf_(lx) * sinf_(ly)) -
                       sinf_(cx) * (sinf_(ly) * sinf_(lz) + cosf_(ly) * cosf_(lz) * sinf_(lx));
  oz = atan2f_(srzcrx / cosf_(ox), crzcrx / cosf_(ox));
}

// integrateTransformation (FA:2537-2568), no IMU.
__host__ __device__ __forceinline__ void odo_integrate(float* ts, const float* tc) {
  float rx, ry, rz;
  odo_accumulate_rotation(ts[0], ts[1], ts[2], -tc[0], -tc[1], -tc[2], rx, ry, rz);
  const float x1 = cosf_(rz) * (tc[3]) - sinf_(rz) * (tc[4]);
  const float y1 = sinf_(rz) * (tc[3]) + cosf_(rz) * (tc[4]);
  const float z1 = tc[5];
  const float x2 = x1;
  const float y2 = cosf_(rx) * y1 - sinf_(rx) * z1;
  const float z2 = sinf_(rx) * y1 + cosf_(rx) * z1;
  const float tx = ts[3] - (cosf_(ry) * x2 + sinf_(ry) * z2);
  const float ty = ts[4] - y2;
  const float tz = ts[5] - (-sinf_(ry) * x2 + cosf_(ry) * z2);
  ts[0] = rx; ts[1] = ry; ts[2] = rz;
  ts[3] = tx; ts[4] = ty; ts[5] = tz;
}

// ---- use_imu_undistortion == true ----
// What TransformToEnd's tail reads, once per scan: updateImuRollPitchYawStartSinCos (FA:491-498), the
// cos / sin of imuYaw / Pitch / RollLast the reference evaluates per point (FA:1472-1481; the same
// value for every point of the scan) and imuShiftFromStartX / Y / Z (always 0: ShiftToStartIMU is
// never called).
struct OdoImuTail {
  float cos_start[3], sin_start[3];  // roll, pitch, yaw (imuRoll / Pitch / YawStart)
  float cos_last[3], sin_last[3];    // roll, pitch, yaw (imuRoll / Pitch / YawLast)
  float shift[3];                    // imuShiftFromStartX / Y / Z
};

// Entry k of the twelve: k < 6 the start cos (0..2) and sin (3..5), else the last cos (6..8) and sin
// (9..11); start / last are llsr_imu_report's start / cur (roll, pitch, yaw).
__host__ __device__ __forceinline__ float odo_imu_tail_entry(const float* start, const float* last, int k) {
  const int j = k % 3;  // selects, not indexing: the callers' arrays stay in registers
  const float a0 = k < 6 ? start[0] : last[0], a1 = k < 6 ? start[1] : last[1], a2 = k < 6 ? start[2] : last[2];
  const float a = j == 0 ? a0 : (j == 1 ? a1 : a2);
  return (k / 3) % 2 == 0 ? cosf_(a) : sinf_(a);
}

__host__ __device__ __forceinline__ void odo_imu_tail_set(OdoImuTail& t, const float* start, const float* last) {
  for (int k = 0; k < 3; ++k) {
    t.cos_start[k] = odo_imu_tail_entry(start, last, k);
    t.sin_start[k] = odo_imu_tail_entry(start, last, 3 + k);
    t.cos_last[k] = odo_imu_tail_entry(start, last, 6 + k);
    t.sin_last[k] = odo_imu_tail_entry(start, last, 9 + k);
    t.shift[k] = 0.f;
  }
}

// TransformToEnd's tail (FA:1458-1483) of p = (x6, y6, z6, int(intensity)).
__host__ __device__ __forceinline__ float4 odo_imu_tail(const OdoImuTail& t, float4 p) {
  const float x7 = t.cos_start[0] * (p.x - t.shift[0]) - t.sin_start[0] * (p.y - t.shift[1]);
  const float y7 = t.sin_start[0] * (p.x - t.shift[0]) + t.cos_start[0] * (p.y - t.shift[1]);
  const float z7 = p.z - t.shift[2];
  const float x8 = x7;
  const float y8 = t.cos_start[1] * y7 - t.sin_start[1] * z7;
  const float z8 = t.sin_start[1] * y7 + t.cos_start[1] * z7;
  const float x9 = t.cos_start[2] * x8 + t.sin_start[2] * z8;
  const float y9 = y8;
  const float z9 = -t.sin_start[2] * x8 + t.cos_start[2] * z8;
  const float x10 = t.cos_last[2] * x9 - t.sin_last[2] * z9;
  const float y10 = y9;
  const float z10 = t.sin_last[2] * x9 + t.cos_last[2] * z9;
  const float x11 = x10;
  const float y11 = t.cos_last[1] * y10 + t.sin_last[1] * z10;
  const float z11 = -t.sin_last[1] * y10 + t.cos_last[1] * z10;
  return make_float4(t.cos_last[0] * x11 + t.sin_last[0] * y11, -t.sin_last[0] * x11 + t.cos_last[0] * y11, z11,
                     p.w);
}

// PluginIMURotation (FA:1492-1550); ac* may alias bc* (the sines and cosines are taken first).
__host__ __device__ inline void odo_plugin_imu_rotation(float bcx, float bcy, float bcz, float blx, float bly,
                                                        float blz, float alx, float aly, float alz, float& acx,
                                                        float& acy, float& acz) {
  const float sbcx = sinf_(bcx), cbcx = cosf_(bcx), sbcy = sinf_(bcy), cbcy = cosf_(bcy);
  const float sbcz = sinf_(bcz), cbcz = cosf_(bcz);
  const float sblx = sinf_(blx), cblx = cosf_(blx), sbly = sinf_(bly), cbly = cosf_(bly);
  const float sblz = sinf_(blz), cblz = cosf_(blz);
  const float salx = sinf_(alx), calx = cosf_(alx), saly = sinf_(aly), caly = cosf_(aly);
  const float salz = sinf_(alz), calz = cosf_(alz);

  const float srx = -sbcx*(salx*sblx + calx*caly*cblx*cbly + calx*cblx*saly*sbly)
                  - cbcx*cbcz*(calx*saly*(cbly*sblz - cblz*sblx*sbly)
                  - calx*caly*(sbly*sblz + cbly*cblz*sblx) + cblx*cblz*salx)
                  - cbcx*sbcz*(calx*caly*(cblz*sbly - cbly*sblx*sblz)
                  - calx*saly*(cbly*cblz + sblx*sbly*sblz) + cblx*salx*sblz);
  acx = -asinf_(srx);

  const float srycrx = (cbcy*sbcz - cbcz*sbcx*sbcy)*(calx*saly*(cbly*sblz - cblz*sblx*sbly)
                     - calx*caly*(sbly*sblz + cbly*cblz*sblx) + cblx*cblz*salx)
                     - (cbcy*cbcz + sbcx*sbcy*sbcz)*(calx*caly*(cblz*sbly - cbly*sblx*sblz)
                     - calx*saly*(cbly*cblz + sblx*sbly*sblz) + cblx*salx*sblz)
                     + cbcx*sbcy*(salx*sblx + calx*caly*cblx*cbly + calx*cblx*saly*sbly);
  const float crycrx = (cbcz*sbcy - cbcy*sbcx*sbcz)*(calx*caly*(cblz*sbly - cbly*sblx*sblz)
                     - calx*saly*(cbly*cblz + sblx*sbly*sblz) + cblx*salx*sblz)
                     - (sbcy*sbcz + cbcy*cbcz*sbcx)*(calx*saly*(cbly*sblz - cblz*sblx*sbly)
                     - calx*caly*(sbly*sblz + cbly*cblz*sblx) + cblx*cblz*salx)
                     + cbcx*cbcy*(salx*sblx + calx*caly*cblx*cbly + calx*cblx*saly*sbly);
  acy = atan2f_(srycrx / cosf_(acx), crycrx / cosf_(acx));

  const float srzcrx = sbcx*(cblx*cbly*(calz*saly - caly*salx*salz)
                     - cblx*sbly*(caly*calz + salx*saly*salz) + calx*salz*sblx)
                     - cbcx*cbcz*((caly*calz + salx*saly*salz)*(cbly*sblz - cblz*sblx*sbly)
                     + (calz*saly - caly*salx*salz)*(sbly*sblz + cbly*cblz*sblx)
                     - calx*cblx*cblz*salz) + cbcx*sbcz*((caly*calz + salx*saly*salz)*(cbly*cblz
                     + sblx*sbly*sblz) + (calz*saly - caly*salx*salz)*(cblz*sbly - cbly*sblx*sblz)
                     + calx*cblx*salz*sblz);
  const float crzcrx = sbcx*(cblx*sbly*(caly*salz - calz*salx*saly)
                     - cblx*cbly*(saly*salz + caly*calz*salx) + calx*calz*sblx)
                     + cbcx*cbcz*((saly*salz + caly*calz*salx)*(sbly*sblz + cbly*cblz*sblx)
                     + (caly*salz - calz*salx*saly)*(cbly*sblz - cblz*sblx*sbly)
                     + calx*calz*cblx*cblz) - cbcx*sbcz*((saly*salz + caly*calz*salx)*(cblz*sbly
                     - cbly*sblx*sblz) + (caly*salz - calz*salx*saly)*(cbly*cblz + sblx*sbly*sblz)
                     - calx*calz*cblx*sblz);
  acz = atan2f_(srzcrx / cosf_(acx), crzcrx / cosf_(acx));
}

// integrateTransformation (FA:2537-2568) with use_imu_undistortion: the translation comes from the
// un-plugged rotation, then PluginIMURotation(rx, ry, rz, imuPitch / Yaw / RollStart,
// imuPitch / Yaw / RollLast). start / last: roll, pitch, yaw.
__host__ __device__ inline void odo_integrate_imu(float* ts, const float* tc, const float* start, const float* last) {
  odo_integrate(ts, tc);
  float rx, ry, rz;
  odo_plugin_imu_rotation(ts[0], ts[1], ts[2], start[1], start[2], start[0], last[1], last[2], last[0], rx, ry, rz);
  ts[0] = rx; ts[1] = ry; ts[2] = rz;
}

// checkSystemInitialization's add on a slot's first scan (FA:2329-2332).
__host__ __device__ __forceinline__ void odo_first_scan_imu(float* ts, const float* start) {
  ts[0] += start[1];
  ts[2] += start[0];
}

}  // namespace llsr
