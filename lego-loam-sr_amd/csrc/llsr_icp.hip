// llsr_icp.hip — the host-only entry points of the loop closure (detectLoopClosure /
// performLoopClosure, mapOptmization.cpp:894-1094): the configuration blocks, the candidate selection,
// one ICP iteration's rigid estimate and the pose constraint, as DESIGN.md §16 specifies them
// (llsr_icp.h). No device code: the device alignment is not part of the library yet (§16).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/llsr.h"
#include "llsr_icp.h"

// ---- host-only entry points ---------------------------------------------------------------------
extern "C" int32_t llsr_loop_config_lidar(llsr_loop_config* c, int32_t lidar) {
  if (!c) return LLSR_EINVAL;
  std::memset(c, 0, sizeof *c);
  if (lidar == LLSR_LIDAR_VLP16) { c->search_radius = 15.0f; c->search_num = 50; c->fitness_score = 0.5f; }        // CFG:29-31
  else if (lidar == LLSR_LIDAR_VLP32C) { c->search_radius = 50.0f; c->search_num = 40; c->fitness_score = 1.5f; }  // CFG:97-99
  else if (lidar == LLSR_LIDAR_HDL64E) { c->search_radius = 30.0f; c->search_num = 30; c->fitness_score = 0.8f; }  // CFG:165-167
  else return LLSR_EINVAL;
  c->leaf = 0.2f;                               // MO:97
  c->min_time_gap = 30.0;                       // MO:912
  c->icp_max_iterations = 100;                  // MO:1001
  c->icp_transformation_epsilon = 1e-6;         // MO:1002
  c->icp_fitness_epsilon = 1e-6;                // MO:1008
  c->icp_max_correspondence_distance = 100.0;   // MO:1007
  return LLSR_OK;
}

// MO:902-919: the first key pose of the sorted radius search that is old (or new) enough. The
// reference writes an unqualified abs(); fabs in double is this library's reading of it.
extern "C" int32_t llsr_loop_candidate(const float* poses4, const double* times, int32_t K, const float pos[3],
                                       double now, float radius, double gap) {
  if (K < 0 || !pos || (K > 0 && (!poses4 || !times))) return LLSR_EINVAL;
  if (K == 0) return -1;
  std::vector<int32_t> near((size_t)K);
  const int n = llsr_keypose_radius_sorted(poses4, K, pos, radius, near.data());
  for (int i = 0; i < n; ++i)
    if (std::fabs(times[near[i]] - now) > gap) return near[i];
  return -1;
}

extern "C" int32_t llsr_umeyama3(const float* src_xyz, const float* dst_xyz, int32_t n, float* T16) {
  if (!src_xyz || !dst_xyz || !T16 || n < 1) return LLSR_EINVAL;
  llsr_icp::umeyama3_host(src_xyz, dst_xyz, n, T16);
  return LLSR_OK;
}

extern "C" int32_t llsr_loop_constraint(const float* T16, const float* pose_latest6, const float* pose_closest6,
                                        double fitness, float* pose_from6, float* pose_to6, float* variance) {
  if (!T16 || !pose_latest6 || !pose_closest6 || !pose_from6 || !pose_to6 || !variance) return LLSR_EINVAL;
  llsr_icp::loop_constraint(T16, pose_latest6, pose_closest6, fitness, pose_from6, pose_to6, variance);
  return LLSR_OK;
}
