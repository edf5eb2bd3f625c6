// The node adapter's IMU input (integration/ros2/llsr_ros2.hpp: ImuInput, Projection::run with a
// stamp) over stand-in message structs with sensor_msgs/Imu's field names.
//   ros2_imu_check cpu                       ImuInput against the C entry points, fed from a second
//                                            thread (no device): prints OK
//   ros2_imu_check drive LIDAR FRAMES IMU OUT a drive in the adapter's thread layout: an /imu_type
//                                            thread feeds a frame's messages, then the projection
//                                            thread runs the scan (tests/test_gpu_ros2_imu.py)
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "llsr_ros2.hpp"

struct PointXYZI {
  float x, y, z, intensity;
};
struct Cloud {
  std::vector<PointXYZI> points;
  uint32_t width = 0, height = 1;
  bool is_dense = true;
};
struct Stamp {
  int32_t sec;
  uint32_t nanosec;
};
struct Header {
  Stamp stamp;
};
struct Vector3 {
  double x, y, z;
};
struct Quaternion {
  double x, y, z, w;
};
struct ImuMsg {  // sensor_msgs/msg/Imu.msg
  Header header;
  Quaternion orientation;
  Vector3 angular_velocity, linear_acceleration;
};

static ImuMsg message(int i) {
  ImuMsg m;
  m.header.stamp.sec = 100 + i / 100;
  m.header.stamp.nanosec = (uint32_t)(i % 100) * 10000000u;
  const double a = 0.01 * i;
  m.orientation = Quaternion{0.0, std::sin(a / 2), 0.0, std::cos(a / 2)};
  m.angular_velocity = Vector3{0.1, -0.2, 0.05 * i};
  m.linear_acceleration = Vector3{0.3, 0.1 * (i % 7), 9.81};
  return m;
}

static int cpu_check() {
  llsr_ros2::ImuInput in(0.1f);
  llsr_imu_state st;
  if (llsr_imu_init(&st) != LLSR_OK) return 1;
  llsr_ros2::ImuInput::Window w;
  in.window(w);
  if (w.n != 0 || in.messages() != 0) return 2;
  int fed = 0;
  for (int scan = 0; scan < 5; ++scan) {
    const int count = scan == 2 ? 230 : 12;  // one window across the ring's wrap
    std::thread t([&] { for (int i = 0; i < count; ++i) in.on_message(message(fed + i)); });
    t.join();
    for (int i = 0; i < count; ++i) {
      const ImuMsg s = message(fed + i);
      llsr_imu_msg m = llsr_imu_msg();
      m.sec = s.header.stamp.sec;
      m.nanosec = s.header.stamp.nanosec;
      const double q[4] = {s.orientation.x, s.orientation.y, s.orientation.z, s.orientation.w};
      const double av[3] = {s.angular_velocity.x, s.angular_velocity.y, s.angular_velocity.z};
      const double la[3] = {s.linear_acceleration.x, s.linear_acceleration.y, s.linear_acceleration.z};
      std::memcpy(m.orientation, q, sizeof q);
      std::memcpy(m.angular_velocity, av, sizeof av);
      std::memcpy(m.linear_acceleration, la, sizeof la);
      if (llsr_imu_callback(&st, &m, 0.1f) != LLSR_OK) return 3;
    }
    fed += count;
    llsr_imu_sample ref[LLSR_IMU_WINDOW_MAX];
    int32_t n = 0;
    if (llsr_imu_scan_window(&st, ref, &n) != LLSR_OK) return 4;
    in.window(w);
    if (w.n != n || n < 1 || std::memcmp(w.samples, ref, sizeof(llsr_imu_sample) * (size_t)(n + 1)) != 0) return 5;
    if (in.messages() != fed) return 6;
  }
  std::printf("OK\n");
  return 0;
}

template <class T>
static bool rd(FILE* f, T* v, size_t n = 1) {
  return std::fread(v, sizeof(T), n, f) == n;
}

static int drive(int lidar, const char* frames_path, const char* imu_path, const char* out_path) {
  FILE* ff = std::fopen(frames_path, "rb");
  FILE* fi = std::fopen(imu_path, "rb");
  FILE* fo = std::fopen(out_path, "wb");
  if (!ff || !fi || !fo) return 2;
  int32_t frames = 0;
  if (!rd(ff, &frames)) return 3;
  std::vector<Cloud> clouds((size_t)frames);
  std::vector<Stamp> stamps((size_t)frames);
  std::vector<std::vector<ImuMsg>> msgs((size_t)frames);
  for (int k = 0; k < frames; ++k) {
    int32_t n = 0, cnt = 0;
    if (!rd(ff, &stamps[k].sec) || !rd(ff, &stamps[k].nanosec) || !rd(ff, &n)) return 3;
    clouds[k].points.resize((size_t)n);
    if (n && !rd(ff, clouds[k].points.data(), (size_t)n)) return 3;
    clouds[k].width = (uint32_t)n;
    if (!rd(fi, &cnt)) return 3;
    msgs[k].resize((size_t)cnt);
    for (int i = 0; i < cnt; ++i) {
      double d[10];
      if (!rd(fi, &msgs[k][i].header.stamp.sec) || !rd(fi, &msgs[k][i].header.stamp.nanosec) || !rd(fi, d, 10)) return 3;
      msgs[k][i].orientation = Quaternion{d[0], d[1], d[2], d[3]};
      msgs[k][i].angular_velocity = Vector3{d[4], d[5], d[6]};
      msgs[k][i].linear_acceleration = Vector3{d[7], d[8], d[9]};
    }
  }
  llsr_config cfg;
  if (llsr_config_default(&cfg, lidar) != LLSR_OK) return 4;
  llsr_ros2::ImuInput imu(cfg.scan_period);
  llsr_ros2::Projection proj(lidar);
  // the /imu_type thread delivers frame k's messages when the projection thread asks for them, so
  // the snapshot each scan takes is the one the test restates
  std::mutex m;
  std::condition_variable cv;
  int want = -1, done = -1;
  std::thread imu_thread([&] {
    for (int k = 0; k < frames; ++k) {
      std::unique_lock<std::mutex> lk(m);
      cv.wait(lk, [&] { return want >= k; });
      lk.unlock();
      for (const ImuMsg& msg : msgs[k]) imu.on_message(msg);
      lk.lock();
      done = k;
      cv.notify_all();
    }
  });
  int rc = 0;
  for (int k = 0; k < frames && rc == 0; ++k) {
    {
      std::unique_lock<std::mutex> lk(m);
      want = k;
      cv.notify_all();
      cv.wait(lk, [&] { return done >= k; });
    }
    try {
      proj.run(clouds[k], stamps[k].sec, stamps[k].nanosec, imu);
      const llsr_scan_out& o = proj.out();
      const llsr_imu_report rep = proj.imu_report();
      const int32_t S = o.n_segmented;
      const int64_t seen = imu.messages();
      std::fwrite(&S, sizeof S, 1, fo);
      std::fwrite(o.seg_xyzi, sizeof(float), 4 * (size_t)S, fo);
      std::fwrite(o.loam_xyzi, sizeof(float), 4 * (size_t)S, fo);
      std::fwrite(o.orientation, sizeof(float), 3, fo);
      std::fwrite(&rep, sizeof rep, 1, fo);
      std::fwrite(&seen, sizeof seen, 1, fo);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "frame %d: %s\n", k, e.what());
      rc = 5;
      std::unique_lock<std::mutex> lk(m);
      want = frames;  // let the other thread run out
      cv.notify_all();
    }
  }
  imu_thread.join();
  std::fclose(ff);
  std::fclose(fi);
  std::fclose(fo);
  return rc;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "cpu")) return cpu_check();
  if (argc == 6 && !std::strcmp(argv[1], "drive")) return drive(std::atoi(argv[2]), argv[3], argv[4], argv[5]);
  std::fprintf(stderr, "usage: %s cpu | drive LIDAR FRAMES IMU OUT\n", argv[0]);
  return 64;
}
