// llsr_prior_internal.h — what the mapping chain (llsr_capi_mapping.hip) uses of a device prior map
// beyond include/llsr.h: the crop in its two halves, so that the chain sizes its local-map buffer from
// the counts without counting twice.
#pragma once
#include <stdint.h>

struct llsr_prior;

namespace llsr_prior_ns {
// The counting half of llsr_prior_crop_batch on a device object: the offsets (host, [P + 1] each) of
// the crops around pos[P][3]. Synchronises the stream.
int32_t crop_begin(llsr_prior* w, const float* pos, int32_t P, int64_t* off_c, int64_t* off_s, void* hip_stream);
// The writing half, for the crop crop_begin counted last: `out` (device float4) of `cap` points.
// LLSR_ERANGE when it does not fit (nothing written). Synchronises the stream.
int32_t crop_write(llsr_prior* w, float* out, int64_t cap, void* hip_stream);
int device_of(const llsr_prior* w);
const char* error_of(const llsr_prior* w);
}  // namespace llsr_prior_ns
