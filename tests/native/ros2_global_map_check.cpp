// publishGlobalMapThread (mapOptmization.cpp:305-315) through llsr_ros2::GlobalMap
// (integration/ros2/llsr_ros2.hpp) next to the C API it wraps. Plain structs stand in for the PCL
// cloud type, as in ros2_adapter_check.cpp (no ROS in this image).
//
//   llsr_ros2_global_map <frames.bin> <out.bin>  (GPU)
//     frames.bin  int32 K, then K keyframes: float pose[6] (x, y, z, roll, pitch, yaw) and the
//                 corner, surf, outlier clouds (int32 n, n float4 rows each)
//   One run() iteration per keyframe (MO:1854-1925): the keyframe is stored in two maps, then the
//   cycle is counted; when GlobalMap::on_cycle() says so the helper publishes from the first map
//   around the newest key position, and llsr_map_global is called directly on the second with
//   buffers of its own. Exit status 1 when the two disagree in any byte or count.
//   out.bin: int32 publishes, then per publish int32 cycle, call, then the global, edge and planar
//   clouds as the helper returned them (int32 n, n float4 rows each).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define LLSR_ROS2_GLOBAL_MAP
#include "../../integration/ros2/llsr_ros2.hpp"

namespace mock {
struct PointXYZI {
  float x, y, z, pad0, intensity, pad1, pad2, pad3;  // PCL's 32-byte layout
};
struct Cloud {
  std::vector<PointXYZI> points;
  uint32_t width = 0, height = 0;
};
}  // namespace mock

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

static void write_cloud(FILE* f, const mock::Cloud& c) {
  std::vector<float> a;
  llsr_ros2::repack_xyzi(c, a);
  const int32_t n = (int32_t)(a.size() / 4);
  fwrite(&n, sizeof n, 1, f);
  fwrite(a.data(), sizeof(float), a.size(), f);
}

// the helper's cloud against n rows downloaded from the direct call's device buffer
static bool same(const mock::Cloud& c, const float* d_rows, int64_t n) {
  std::vector<float> a, b(4 * (size_t)n);
  llsr_ros2::repack_xyzi(c, a);
  if (a.size() != b.size()) return false;
  if (n && hipMemcpy(b.data(), d_rows, b.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return false;
  return memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s frames.bin out.bin\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  int32_t K = 0;
  if (!in || !out || !read_exact(in, &K, sizeof K) || K < 1) {
    fprintf(stderr, "cannot read %s / write %s\n", argv[1], argv[2]);
    return 2;
  }
  llsr_map* helper_map = llsr_map_create(nullptr, 0);
  llsr_map* direct_map = llsr_map_create(nullptr, 0);
  if (!helper_map || !direct_map) {
    fprintf(stderr, "llsr_map_create failed (no HIP device?)\n");
    return 2;
  }
  int status = 0;
  try {
    llsr_ros2::GlobalMap<mock::Cloud> gm;
    std::vector<int32_t> head;
    std::vector<mock::Cloud> clouds;
    int64_t total = 0;
    for (int32_t cycle = 1; cycle <= K; ++cycle) {
      float pose[6];
      std::vector<float> cl[3];
      int32_t n[3];
      if (!read_exact(in, pose, sizeof pose)) throw std::runtime_error("frames.bin: short pose");
      for (int a = 0; a < 3; ++a) {
        if (!read_exact(in, &n[a], sizeof n[a]) || n[a] < 0) throw std::runtime_error("frames.bin: short count");
        cl[a].resize(4 * (size_t)n[a]);
        if (!read_exact(in, cl[a].data(), cl[a].size() * sizeof(float))) throw std::runtime_error("frames.bin: short cloud");
        total += n[a];
      }
      for (llsr_map* m : {helper_map, direct_map})
        if (llsr_map_add_keyframe(m, pose, cl[0].data(), n[0], cl[1].data(), n[1], cl[2].data(), n[2], nullptr) != cycle - 1)
          throw std::runtime_error(std::string("llsr_map_add_keyframe: ") + llsr_map_last_error(m));
      if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("hipDeviceSynchronize");
      if (!gm.on_cycle()) continue;
      gm.publish(helper_map, pose);
      // the same call on the other map, every output sized for the raw clouds
      float* d[3] = {nullptr, nullptr, nullptr};
      for (int k = 0; k < 3; ++k)
        if (hipMalloc((void**)&d[k], (size_t)(total + 1) * 4 * sizeof(float)) != hipSuccess)
          throw std::runtime_error("hipMalloc");
      llsr_global_map_report rep;
      const int32_t rc = llsr_map_global(direct_map, nullptr, pose, d[0], total, d[1], total, d[2], total, &rep, nullptr);
      if (rc != LLSR_OK) throw std::runtime_error(std::string("llsr_map_global: ") + llsr_map_last_error(direct_map));
      const llsr_global_map_report& g = gm.report;
      if (g.call != rep.call || g.n_global != rep.n_global || g.n_edge != rep.n_edge || g.n_planar != rep.n_planar ||
          g.n_poses_used != rep.n_poses_used || g.downsampled_cloud != rep.downsampled_cloud ||
          !same(gm.global, d[0], rep.n_global) || !same(gm.edge, d[1], rep.n_edge) ||
          !same(gm.planar, d[2], rep.n_planar)) {
        fprintf(stderr, "cycle %d: the helper's clouds differ from llsr_map_global's\n", cycle);
        status = 1;
      }
      for (int k = 0; k < 3; ++k) (void)hipFree(d[k]);
      head.push_back(cycle);
      head.push_back(g.call);
      clouds.push_back(gm.global);
      clouds.push_back(gm.edge);
      clouds.push_back(gm.planar);
    }
    const int32_t np = (int32_t)(head.size() / 2);
    fwrite(&np, sizeof np, 1, out);
    for (int32_t p = 0; p < np; ++p) {
      fwrite(&head[2 * p], sizeof(int32_t), 2, out);
      for (int k = 0; k < 3; ++k) write_cloud(out, clouds[3 * p + k]);
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    status = 2;
  }
  llsr_map_destroy(helper_map);
  llsr_map_destroy(direct_map);
  fclose(in);
  fclose(out);
  return status;
}
