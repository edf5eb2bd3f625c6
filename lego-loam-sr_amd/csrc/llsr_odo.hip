// llsr_odo.hip — the device glue of FeatureAssociation's per-scan loop around the scan-to-scan LM
// (runFeatureAssociation, featureAssociation.cpp:2742-2853), for a batch of independent
// sequences (one slot each), so IP -> features -> LM -> last clouds never leaves HBM:
//
//   k_odo_inputs   cornerPointsSharp / surfPointsFlat (+ the 160 GenerateShadowPoint points,
//                  FA:1310-1314) gathered from the feature stage into the LM's packed inputs
//   (k_grid_* + k_s2s_lm: updateTransformation against the slot's last clouds, llsr_fa_lm.hip)
//   k_odo_finish   first scan of a slot: checkSystemInitialization (FA:2291-2315);
//                  afterwards integrateTransformation (FA:2537-2568 with AccumulateRotation
//                  FA:1552-1578) and publishCloudsLast (FA:2660-2712): TransformToEnd
//                  (FA:1414-1490) of the less-sharp / less-flat clouds, which become the next
//                  last clouds (+ shadow points on the surf side), and of the sharp / flat
//                  clouds, which are the MapOptimization scan inputs (AssociationOut). With
//                  llsr_odometry_batch_odom, updateInitialGuess (FA:2790, evaluated on the host,
//                  llsr_odom_guess.h) replaces the LM's transformCur first, per flagged slot.
//   k_odo_inputs_imu / k_odo_finish_imu   the same two with use_imu_undistortion == true
//                  (llsr_set_imu_undistortion; false in the shipped config blocks, CFG:59/127/195):
//                  the pre-LM updateInitialGuess (FA:2786-2788) stores the guess as the LM's start,
//                  TransformToEnd runs its IMU tail (FA:1456-1483), integrateTransformation ends in
//                  PluginIMURotation (FA:2557-2560) and a slot's first scan adds imuPitch / RollStart
//                  to transformSum (FA:2329-2332). DESIGN.md §18.
// Float typing and operation order follow the reference lines; sin/cos/asin/atan2 are the glibc
// ports of llsr_libm.h.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "llsr_device.h"
#include "llsr_libm.h"
#include "llsr_odo.h"

namespace llsr {

// grid B, block 256: the LM's query clouds of slot b, packed at the host-computed offsets. kImu: the
// pre-LM updateInitialGuess (FA:2786-2788) of a flagged, initialised slot overwrites transformCur, so
// the LM starts from the odometry guess (its member copies need no store: k_odo_finish_imu reads
// this scan's imu*Cur as imu*Last).
template <bool kImu>
__device__ __forceinline__ void odo_inputs_body(OdoArgs a) {
  const int b = blockIdx.x;
  const int* cnt = a.counts + b * kCnt;
  const size_t base = (size_t)b * a.HW;
  const int Ms = cnt[C_SHARP], F = cnt[C_F];
  float4* sharp = a.sharp + a.sharp_off[b];
  float4* flat = a.flat + a.flat_off[b];
  for (int k = threadIdx.x; k < Ms; k += blockDim.x) sharp[k] = a.loam[base + a.sharp_ind[base + k]];
  for (int k = threadIdx.x; k < F + kShadow; k += blockDim.x)
    flat[k] = k < F ? a.loam[base + a.flat_ind[base + k]] : a.shadow[k - F];
  if constexpr (kImu) {
    if (threadIdx.x < 6 && a.flags != nullptr && a.flags[b] != 0 && a.inited[b] != 0)
      a.tcur[6 * b + threadIdx.x] = a.guess[6 * b + threadIdx.x];
  }
}

__global__ __launch_bounds__(256) void k_odo_inputs(OdoArgs a) { odo_inputs_body<false>(a); }
__global__ __launch_bounds__(256) void k_odo_inputs_imu(OdoArgs a) { odo_inputs_body<true>(a); }

// What the kImu instantiation of odo_finish_body keeps per thread; the plain one keeps nothing.
struct OdoImuCtx {
  OdoImuTail tail;
  float start[3], last[3];  // imuRoll / Pitch / YawStart, imuRoll / Pitch / YawLast
};
struct OdoNoImu {};

__device__ __forceinline__ float4 odo_point(const float* tc, const OdoNoImu&, float4 p) { return odo_to_end(tc, p); }
__device__ __forceinline__ float4 odo_point(const float* tc, const OdoImuCtx& c, float4 p) {
  return odo_imu_tail(c.tail, odo_to_end(tc, p));
}

// grid B, block 256: after the LM of slot b (transformCur in a.tcur). kImu: `carry` is the slots'
// IMU carry after this scan's feature stage (nullptr: never staged, the constructor's zeros). The
// arguments stay by value: by reference the plain instantiation's frame comes out different.
template <bool kImu>
__device__ __forceinline__ void odo_finish_body(OdoArgs a,const llsr_imu_carry* carry) {
  const int b = blockIdx.x;
  const int* cnt = a.counts + b * kCnt;
  const size_t base = (size_t)b * a.HW;
  const int M = cnt[C_M], L = cnt[C_L], Ms = cnt[C_SHARP], F = cnt[C_F];
  const bool inited = a.inited[b] != 0;
  // updateInitialGuess (FA:2790) replaces the LM's transformCur before integrateTransformation and
  // publishCloudsLast; not on the initialisation scan (the `continue` at FA:2781-2784). Every thread
  // takes the replaced value from a.guess, so thread 0's store to a.tcur below races with no read.
  const bool ow = inited && a.flags != nullptr && a.flags[b] != 0;
  const float* src = ow ? a.guess : a.tcur;
  float tc[6];
  for (int k = 0; k < 6; ++k) tc[k] = src[6 * b + k];
  // the slot's imuRoll / Pitch / YawStart and, after updateInitialGuess's member copy, imu*Last = this
  // scan's imu*Cur; the twelve sines and cosines of the tail once per slot, by twelve lanes
  typename std::conditional<kImu, OdoImuCtx, OdoNoImu>::type ctx;
  if constexpr (kImu) {
    __shared__ float s_imu[12];
    for (int k = 0; k < 3; ++k) {
      ctx.start[k] = carry != nullptr ? carry[b].report.start[k] : 0.f;
      ctx.last[k] = carry != nullptr ? carry[b].report.cur[k] : 0.f;
    }
    if (inited) {
      if (threadIdx.x < 12) s_imu[threadIdx.x] = odo_imu_tail_entry(ctx.start, ctx.last, threadIdx.x);
      __syncthreads();
      // the same value in every lane: kept in scalar registers (the vector budget stays at
      // k_odo_finish's 4 waves per SIMD)
      auto uniform = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
      for (int k = 0; k < 3; ++k) {
        ctx.tail.cos_start[k] = uniform(s_imu[k]);
        ctx.tail.sin_start[k] = uniform(s_imu[3 + k]);
        ctx.tail.cos_last[k] = uniform(s_imu[6 + k]);
        ctx.tail.sin_last[k] = uniform(s_imu[9 + k]);
        ctx.tail.shift[k] = 0.f;  // imuShiftFromStartX / Y / Z: ShiftToStartIMU is never called
      }
    }
  }
  float4* cl = a.nlast_c + a.nlast_c_off[b];
  float4* sl = a.nlast_s + a.nlast_s_off[b];
  if (!inited) {  // checkSystemInitialization (FA:2291-2315): the clouds as they are
    for (int k = threadIdx.x; k < M; k += blockDim.x) cl[k] = a.loam[base + a.less_sharp[base + k]];
    for (int k = threadIdx.x; k < L + kShadow; k += blockDim.x) sl[k] = k < L ? a.lflat[base + k] : a.shadow[k - L];
  } else {  // publishCloudsLast (FA:2666-2707)
    for (int k = threadIdx.x; k < M; k += blockDim.x) cl[k] = odo_point(tc, ctx, a.loam[base + a.less_sharp[base + k]]);
    for (int k = threadIdx.x; k < L + kShadow; k += blockDim.x)
      sl[k] = k < L ? odo_point(tc, ctx, a.lflat[base + k]) : a.shadow[k - L];
    float4* sc = a.scan_c + a.sharp_off[b];
    float4* ss = a.scan_s + a.flat_off[b];
    for (int k = threadIdx.x; k < Ms; k += blockDim.x) sc[k] = odo_point(tc, ctx, a.sharp[a.sharp_off[b] + k]);
    for (int k = threadIdx.x; k < F + kShadow; k += blockDim.x) ss[k] = odo_point(tc, ctx, a.flat[a.flat_off[b] + k]);
  }
  // every wave has read a.inited[b] (and, unflagged, a.tcur) before thread 0 stores to them
  __syncthreads();
  if (threadIdx.x == 0) {
    if (a.tlm != nullptr)
      for (int k = 0; k < 6; ++k) {
        a.tlm[6 * b + k] = ow ? a.tcur[6 * b + k] : 0.f;
        if (ow) a.tcur[6 * b + k] = tc[k];
      }
    if (inited) {
      float ts[6];
      for (int k = 0; k < 6; ++k) ts[k] = a.tsum[6 * b + k];
      if constexpr (kImu) odo_integrate_imu(ts, tc, ctx.start, ctx.last);
      else odo_integrate(ts, tc);
      for (int k = 0; k < 6; ++k) a.tsum[6 * b + k] = ts[k];
    } else if constexpr (kImu) {  // checkSystemInitialization's add (FA:2329-2332)
      float ts[6];
      for (int k = 0; k < 6; ++k) ts[k] = a.tsum[6 * b + k];
      odo_first_scan_imu(ts, ctx.start);
      a.tsum[6 * b] = ts[0];
      a.tsum[6 * b + 2] = ts[2];
    }
    a.inited[b] = 1;
    a.frames[b] += 1;
  }
}

__global__ __launch_bounds__(256) void k_odo_finish(OdoArgs a) { odo_finish_body<false>(a, nullptr); }
__global__ __launch_bounds__(256) void k_odo_finish_imu(OdoArgs a, const llsr_imu_carry* carry) {
  odo_finish_body<true>(a, carry);
}

}  // namespace llsr
