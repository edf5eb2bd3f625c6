// The node adapter with use_imu_undistortion on (integration/ros2/llsr_ros2.hpp: Odometry's switch,
// FeatureClouds::imu, Projection::handoff), over stand-in message structs, in the node's thread
// layout (tests/test_gpu_ros2_imu_undistortion.py):
//   ros2_imu_undistortion_check LIDAR FRAMES IMU ODOM OUT
// an input thread delivers a frame's /imu_type messages and its /odom2 message, the projection thread
// runs the scan with the IMU window and hands the feature clouds and the IMU report to the FA thread
// through the one-slot channel, and the FA thread runs runFeatureAssociation's order with the switch
// on: apply, solve, apply, finish.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../integration/ros2/llsr_ros2.hpp"

namespace mock {
struct PointXYZI {
  float x, y, z, pad0, intensity, pad1, pad2, pad3;  // PCL's 32-byte layout
};
struct Cloud {
  std::vector<PointXYZI> points;
  uint32_t width = 0, height = 0;
};
struct CloudInfo {  // cloud_msgs/msg/CloudInfo.msg
  std::vector<int32_t> start_ring_index, end_ring_index;
  float start_orientation = 0, end_orientation = 0, orientation_diff = 0;
  std::vector<bool> segmented_cloud_ground_flag;
  std::vector<uint32_t> segmented_cloud_col_ind;
  std::vector<float> segmented_cloud_range;
};
struct ProjectionOut {  // utility.h:63-72, with the member INTEGRATION.md §2 adds
  std::shared_ptr<Cloud> segmented_cloud, outlier_cloud;
  CloudInfo seg_msg;
  std::vector<double> outlierCloud_Intensity, segmentedCloud_Intensity;
  llsr_ros2::FeatureClouds<Cloud> features;
  int32_t seq = -1;
};
struct Odometry {  // nav_msgs/msg/Odometry: the fields odomCallback reads
  struct {
    struct {
      struct { double x, y, z, w; } orientation;
      struct { double x, y, z; } position;
    } pose;
  } pose;
};
struct Imu {  // sensor_msgs/msg/Imu
  struct { struct { int32_t sec; uint32_t nanosec; } stamp; } header;
  struct { double x, y, z, w; } orientation;
  struct { double x, y, z; } angular_velocity, linear_acceleration;
};

// one writer, one reader, one slot (channel.h:24-54), blocking send
template <class T>
class Channel {
 public:
  void send(T&& v) {
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [this] { return !full_; });
    slot_ = std::move(v);
    full_ = true;
    cv_.notify_all();
  }
  void receive(T& v) {
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [this] { return full_; });
    v = std::move(slot_);
    full_ = false;
    cv_.notify_all();
  }

 private:
  bool full_ = false;
  T slot_;
  std::mutex m_;
  std::condition_variable cv_;
};
}  // namespace mock

template <class T>
static bool rd(FILE* f, T* v, size_t n = 1) {
  return fread(v, sizeof(T), n, f) == n;
}

template <class T>
static void put(std::vector<char>& b, const T* v, size_t n = 1) {
  const char* p = reinterpret_cast<const char*>(v);
  b.insert(b.end(), p, p + sizeof(T) * n);
}

static void put_cloud(std::vector<char>& b, const mock::Cloud& c) {
  const int32_t n = (int32_t)c.points.size();
  put(b, &n);
  for (const auto& p : c.points) {
    const float r[4] = {p.x, p.y, p.z, p.intensity};
    put(b, r, 4);
  }
}

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s LIDAR FRAMES IMU ODOM OUT\n", argv[0]);
    return 64;
  }
  const int lidar = atoi(argv[1]);
  FILE* ff = fopen(argv[2], "rb");
  FILE* fi = fopen(argv[3], "rb");
  FILE* fd = fopen(argv[4], "rb");
  if (!ff || !fi || !fd) return 2;
  int32_t frames = 0;
  if (!rd(ff, &frames) || frames < 1) return 3;
  std::vector<mock::Cloud> clouds((size_t)frames);
  std::vector<int32_t> sec((size_t)frames);
  std::vector<uint32_t> nsec((size_t)frames);
  std::vector<std::vector<mock::Imu>> imu_msgs((size_t)frames);
  std::vector<mock::Odometry> odom_msgs((size_t)frames);
  for (int k = 0; k < frames; ++k) {
    int32_t n = 0, cnt = 0;
    if (!rd(ff, &sec[k]) || !rd(ff, &nsec[k]) || !rd(ff, &n) || n < 0) return 3;
    std::vector<float> rows(4 * (size_t)n);
    if (n && !rd(ff, rows.data(), rows.size())) return 3;
    llsr_ros2::unpack_xyzi(rows.data(), n, clouds[k]);
    if (!rd(fi, &cnt) || cnt < 0) return 3;
    imu_msgs[k].resize((size_t)cnt);
    for (int i = 0; i < cnt; ++i) {
      mock::Imu& m = imu_msgs[k][i];
      double d[10];
      if (!rd(fi, &m.header.stamp.sec) || !rd(fi, &m.header.stamp.nanosec) || !rd(fi, d, 10)) return 3;
      m.orientation = {d[0], d[1], d[2], d[3]};
      m.angular_velocity = {d[4], d[5], d[6]};
      m.linear_acceleration = {d[7], d[8], d[9]};
    }
    double v[7];
    if (!rd(fd, v, 7)) return 3;
    odom_msgs[k].pose.pose.orientation = {v[0], v[1], v[2], v[3]};
    odom_msgs[k].pose.pose.position = {v[4], v[5], v[6]};
  }
  fclose(ff);
  fclose(fi);
  fclose(fd);
  llsr_config cfg;
  if (llsr_config_default(&cfg, lidar) != LLSR_OK) return 4;

  llsr_ros2::ImuInput imu_in(cfg.scan_period);
  llsr_ros2::OdomInput odom_in;
  mock::Channel<mock::ProjectionOut> ip_to_fa;
  std::mutex m;
  std::condition_variable cv;
  // frame k's /imu_type messages arrive when the projection thread asks for them and its /odom2 message
  // when the FA thread does, so the snapshots each thread takes are the ones the test restates
  int want_imu = -1, done_imu = -1, want_odom = -1, done_odom = -1;
  bool stop = false;
  std::vector<std::vector<char>> ip_rec((size_t)frames), fa_rec((size_t)frames);
  int rc_ip = 0, rc_fa = 0;

  // the subscriptions' thread
  std::thread input_thread([&] {
    std::unique_lock<std::mutex> lk(m);
    while (done_imu < frames - 1 || done_odom < frames - 1) {
      cv.wait(lk, [&] { return stop || want_imu > done_imu || want_odom > done_odom; });
      if (stop) return;
      if (want_imu > done_imu) {
        const int k = done_imu + 1;
        lk.unlock();
        for (const mock::Imu& msg : imu_msgs[k]) imu_in.on_message(msg);
        lk.lock();
        done_imu = k;
      } else {
        const int k = done_odom + 1;
        lk.unlock();
        odom_in.on_message(odom_msgs[k]);
        lk.lock();
        done_odom = k;
      }
      cv.notify_all();
    }
  });
  auto give_up = [&] {
    std::unique_lock<std::mutex> lk(m);
    stop = true;
    cv.notify_all();
  };

  // FeatureAssociation's thread
  std::thread fa_thread([&] {
    try {
      llsr_ros2::Odometry<mock::Cloud> odo(lidar, 0, true);
      for (int k = 0; k < frames; ++k) {
        mock::ProjectionOut po;
        ip_to_fa.receive(po);
        if (po.seq < 0) return;  // the projection thread gave up
        llsr_ros2::FeatureClouds<mock::Cloud>& f = po.features;
        {
          std::unique_lock<std::mutex> lk(m);
          want_odom = k;
          cv.notify_all();
          cv.wait(lk, [&] { return stop || done_odom >= k; });
        }
        const llsr_odom_sample smp = odom_in.sample();
        float tlm[6] = {0, 0, 0, 0, 0, 0};
        int32_t lm = 0;
        if (odo.initialised()) odom_in.apply(odo.transform_sum, odo.transform_cur);  // FA:2786-2788
        if (odo.solve(f)) {                                                          // FA:2789
          lm = 1;
          for (int i = 0; i < 6; ++i) tlm[i] = odo.transform_cur[i];
          odom_in.apply(odo.transform_sum, odo.transform_cur);                       // FA:2790
          odo.finish(f);                                                             // FA:2792-2796
        }
        std::vector<char>& b = fa_rec[(size_t)k];
        put(b, &smp);
        put(b, &lm);
        put(b, &odo.report, 1);
        put(b, tlm, 6);
        put(b, odo.transform_cur, 6);
        put(b, odo.transform_sum, 6);
        put_cloud(b, odo.corner_last);
        put_cloud(b, odo.surf_last);
        put_cloud(b, lm ? odo.corner_scan : mock::Cloud());
        put_cloud(b, lm ? odo.surf_scan : mock::Cloud());
      }
    } catch (const std::exception& e) {
      fprintf(stderr, "FA thread: %s\n", e.what());
      rc_fa = 6;
      give_up();
      // keep draining so that the projection thread's blocking send returns
      for (;;) {
        mock::ProjectionOut po;
        ip_to_fa.receive(po);
        if (po.seq < 0 || po.seq == frames - 1) return;
      }
    }
  });

  // ImageProjection's thread (this one)
  try {
    llsr_ros2::Projection proj(lidar);
    for (int k = 0; k < frames; ++k) {
      {
        std::unique_lock<std::mutex> lk(m);
        want_imu = k;
        cv.notify_all();
        cv.wait(lk, [&] { return stop || done_imu >= k; });
      }
      proj.run(clouds[k], sec[k], nsec[k], imu_in);
      const llsr_scan_out& o = proj.out();
      std::vector<char>& b = ip_rec[(size_t)k];
      put(b, &o.n_segmented);
      put(b, o.loam_xyzi, 4 * (size_t)o.n_segmented);
      put(b, &o.n_sharp);
      put(b, o.sharp_ind, (size_t)o.n_sharp);
      put(b, &o.n_flat);
      put(b, o.flat_ind, (size_t)o.n_flat);
      put(b, &o.n_less_sharp);
      put(b, o.less_sharp_ind, (size_t)o.n_less_sharp);
      put(b, &o.n_less_flat);
      put(b, o.less_flat_xyzi, 4 * (size_t)o.n_less_flat);
      const llsr_imu_report rep = proj.imu_report();
      put(b, &rep);
      mock::ProjectionOut po;
      po.segmented_cloud.reset(new mock::Cloud());
      po.outlier_cloud.reset(new mock::Cloud());
      proj.handoff(po);
      po.seq = k;
      ip_to_fa.send(std::move(po));
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "projection thread: %s\n", e.what());
    rc_ip = 5;
    give_up();
    mock::ProjectionOut last;
    ip_to_fa.send(std::move(last));
  }
  input_thread.join();
  fa_thread.join();
  if (rc_ip || rc_fa) return rc_ip ? rc_ip : rc_fa;
  FILE* fo = fopen(argv[5], "wb");
  if (!fo) return 2;
  for (int k = 0; k < frames; ++k) {
    fwrite(ip_rec[(size_t)k].data(), 1, ip_rec[(size_t)k].size(), fo);
    fwrite(fa_rec[(size_t)k].data(), 1, fa_rec[(size_t)k].size(), fo);
  }
  fclose(fo);
  return 0;
}
