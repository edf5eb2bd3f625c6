// runFeatureAssociation in the reference's program order (featureAssociation.cpp:2781-2796) through
// integration/ros2/llsr_ros2.hpp: Odometry::solve, OdomInput::apply (updateInitialGuess),
// Odometry::finish, with /odom2 arriving on its own thread. Plain structs stand in for the ROS2 /
// PCL message types, as in ros2_adapter_check.cpp (no ROS in this image).
//
//   drive <lidar> <frames.bin> <odom.bin> <out.bin>  (GPU)
//     frames.bin  int32 F, then F clouds (int32 n, n float4 rows)
//     odom.bin    F records: int32 has_message, 7 doubles (orientation x, y, z, w, position)
//   Two drives over the same frames, each with the thread layout of main.cpp:10-11 (an IP thread:
//   Projection::run + handoff, blocking one-slot send; an FA thread on its own handle; an MO thread
//   taking the AssociationOut, non-blocking send) plus a fourth thread that feeds OdomInput: frame
//   k's message, when it has one, is delivered after FA received frame k and before its solve (the
//   FA thread asks for it and waits, so the run is deterministic). The first drive delivers
//   odom.bin's messages, the second none at all (OdomInput stays at the zero sample).
//   out.bin: per drive int32 frames, then per frame int32 seq, lm, messages seen; float[6] the LM's
//   transformCur, transformCur after apply, transformSum; the clouds corner_last, surf_last,
//   corner_scan, surf_scan; then int32 count and the seq + transformSum[6] of what MO received.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
struct Header {
  int32_t sec = 0;
};
struct CloudInfo {  // cloud_msgs/msg/CloudInfo.msg
  Header header;
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
};
struct AssociationOut {  // utility.h:75-83
  Header header;
  float transform_sum[6];
};
struct Odometry {  // nav_msgs/msg/Odometry: the fields odomCallback reads
  struct {
    struct {
      struct { double x, y, z, w; } orientation;
      struct { double x, y, z; } position;
    } pose;
  } pose;
};

// one writer, one reader, one slot (channel.h:24-54)
template <class T>
class Channel {
 public:
  explicit Channel(bool blocking_send) : blocking_(blocking_send) {}
  void send(T&& v) {
    std::unique_lock<std::mutex> lk(m_);
    if (blocking_) cv_.wait(lk, [this] { return !full_; });
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
  bool blocking_;
  bool full_ = false;
  T slot_;
  std::mutex m_;
  std::condition_variable cv_;
};
}  // namespace mock

struct OdomRecord {
  int32_t has = 0;
  double v[7];
};

static bool read_cloud(FILE* f, mock::Cloud& c) {
  int32_t n = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 0) return false;
  std::vector<float> rows(4 * (size_t)n);
  if (n && fread(rows.data(), 4, rows.size(), f) != rows.size()) return false;
  llsr_ros2::unpack_xyzi(rows.data(), n, c);
  return true;
}

static void put_cloud(FILE* g, const mock::Cloud& c) {
  const int32_t n = (int32_t)c.points.size();
  fwrite(&n, 4, 1, g);
  for (const auto& p : c.points) {
    const float r[4] = {p.x, p.y, p.z, p.intensity};
    fwrite(r, 4, 4, g);
  }
}

struct FaRecord {
  int32_t seq = -1, lm = 0, messages = 0;
  float tlm[6], tcur[6], tsum[6];
  mock::Cloud corner_last, surf_last, corner_scan, surf_scan;
};
struct MoRecord {
  int32_t seq = -1;
  float tsum[6];
};

// The FA thread asks for frame k's message and waits until the /odom2 thread has delivered it.
struct Handoff {
  std::mutex m;
  std::condition_variable cv;
  int32_t wanted = -1, delivered = -1;
  bool stop = false;
};

static int drive(int lidar, const std::vector<mock::Cloud>& frames, const std::vector<OdomRecord>& odom,
                 bool deliver, FILE* g) {
  const int32_t F = (int32_t)frames.size();
  mock::Channel<mock::ProjectionOut> ip_to_fa(true);    // projection_out_channel(true)
  mock::Channel<mock::AssociationOut> fa_to_mo(false);  // association_out_channel(false)
  llsr_ros2::OdomInput odom_in;
  Handoff ho;
  std::vector<FaRecord> fa_rec;
  std::vector<MoRecord> mo_rec;
  std::string err;
  std::mutex err_m;
  auto guard = [&](const char* who, const std::exception& e) {
    std::lock_guard<std::mutex> lk(err_m);
    err += std::string(who) + ": " + e.what() + "\n";
  };

  std::thread od([&] {  // the /odom2 subscription's thread
    try {
      while (true) {
        int32_t k;
        {
          std::unique_lock<std::mutex> lk(ho.m);
          ho.cv.wait(lk, [&] { return ho.stop || ho.wanted > ho.delivered; });
          if (ho.stop) break;
          k = ho.wanted;
        }
        if (deliver && odom[(size_t)k].has) {
          mock::Odometry msg;
          const double* v = odom[(size_t)k].v;
          msg.pose.pose.orientation.x = v[0]; msg.pose.pose.orientation.y = v[1];
          msg.pose.pose.orientation.z = v[2]; msg.pose.pose.orientation.w = v[3];
          msg.pose.pose.position.x = v[4]; msg.pose.pose.position.y = v[5]; msg.pose.pose.position.z = v[6];
          odom_in.on_message(msg);
        }
        std::lock_guard<std::mutex> lk(ho.m);
        ho.delivered = k;
        ho.cv.notify_all();
      }
    } catch (const std::exception& e) {
      guard("odom", e);
      std::lock_guard<std::mutex> lk(ho.m);
      ho.delivered = F;  // release the FA thread
      ho.cv.notify_all();
    }
  });
  std::thread ip([&] {  // ImageProjection::cloudHandler per message, then publishClouds' send
    try {
      llsr_ros2::Projection proj(lidar, 0);
      for (int32_t k = 0; k < F; ++k) {
        mock::ProjectionOut po;
        proj.run(frames[(size_t)k]);
        po.segmented_cloud = std::make_shared<mock::Cloud>();
        po.outlier_cloud = std::make_shared<mock::Cloud>();
        proj.handoff(po);
        po.seg_msg.header.sec = k;
        ip_to_fa.send(std::move(po));
      }
    } catch (const std::exception& e) {
      guard("ip", e);
    }
    mock::ProjectionOut end;
    end.seg_msg.header.sec = -1;  // end of the drive
    ip_to_fa.send(std::move(end));
  });
  std::thread fa([&] {  // runFeatureAssociation's loop (FA:2742-2853) on its own handle
    try {
      llsr_ros2::Odometry<mock::Cloud> odo(lidar, 0);
      while (true) {
        mock::ProjectionOut po;
        ip_to_fa.receive(po);
        if (po.seg_msg.header.sec < 0) break;
        FaRecord r;
        r.seq = po.seg_msg.header.sec;
        {
          std::unique_lock<std::mutex> lk(ho.m);
          ho.wanted = r.seq;
          ho.cv.notify_all();
          ho.cv.wait(lk, [&] { return ho.delivered >= r.seq; });
        }
        r.messages = odom_in.messages();
        r.lm = odo.solve(po.features) ? 1 : 0;  // checkSystemInitialization + continue, or updateTransformation
        for (int i = 0; i < 6; ++i) r.tlm[i] = odo.transform_cur[i];
        if (r.lm) {
          odom_in.apply(odo.transform_sum, odo.transform_cur);  // updateInitialGuess (FA:2790)
          odo.finish(po.features);  // integrateTransformation, publishCloudsLast
        }
        for (int i = 0; i < 6; ++i) {
          r.tcur[i] = odo.transform_cur[i];
          r.tsum[i] = odo.transform_sum[i];
        }
        r.corner_last = odo.corner_last;
        r.surf_last = odo.surf_last;
        if (r.lm) {
          r.corner_scan = odo.corner_scan;
          r.surf_scan = odo.surf_scan;
          mock::AssociationOut ao;  // _output_channel.send (FA:2822-2852), mapping_frequency_divider 1
          ao.header.sec = r.seq;
          for (int i = 0; i < 6; ++i) ao.transform_sum[i] = odo.transform_sum[i];
          fa_to_mo.send(std::move(ao));
        }
        fa_rec.push_back(std::move(r));
      }
    } catch (const std::exception& e) {
      guard("fa", e);
      mock::ProjectionOut po;  // drain so that IP's blocking send returns
      do ip_to_fa.receive(po); while (po.seg_msg.header.sec >= 0);
    }
    {
      std::lock_guard<std::mutex> lk(ho.m);
      ho.stop = true;
      ho.cv.notify_all();
    }
    mock::AssociationOut end;
    end.header.sec = -1;
    fa_to_mo.send(std::move(end));
  });
  std::thread mo([&] {  // MapOptimization's loop: what it received (latest wins, as the channel)
    while (true) {
      mock::AssociationOut ao;
      fa_to_mo.receive(ao);
      if (ao.header.sec < 0) break;
      MoRecord r;
      r.seq = ao.header.sec;
      memcpy(r.tsum, ao.transform_sum, sizeof r.tsum);
      mo_rec.push_back(r);
    }
  });
  ip.join();
  fa.join();
  mo.join();
  od.join();
  if (!err.empty()) {
    fprintf(stderr, "%s", err.c_str());
    return 1;
  }
  const int32_t nf = (int32_t)fa_rec.size(), nm = (int32_t)mo_rec.size();
  fwrite(&nf, 4, 1, g);
  for (const auto& r : fa_rec) {
    const int32_t hdr[3] = {r.seq, r.lm, r.messages};
    fwrite(hdr, 4, 3, g);
    fwrite(r.tlm, 4, 6, g);
    fwrite(r.tcur, 4, 6, g);
    fwrite(r.tsum, 4, 6, g);
    for (const mock::Cloud* c : {&r.corner_last, &r.surf_last, &r.corner_scan, &r.surf_scan}) put_cloud(g, *c);
  }
  fwrite(&nm, 4, 1, g);
  for (const auto& r : mo_rec) {
    fwrite(&r.seq, 4, 1, g);
    fwrite(r.tsum, 4, 6, g);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 6 || strcmp(argv[1], "drive")) {
    fprintf(stderr, "usage: %s drive <lidar> <frames.bin> <odom.bin> <out.bin>\n", argv[0]);
    return 2;
  }
  const int lidar = atoi(argv[2]);
  FILE* f = fopen(argv[3], "rb");
  if (!f) return 2;
  int32_t F = 0;
  if (fread(&F, 4, 1, f) != 1 || F < 1) return 2;
  std::vector<mock::Cloud> frames((size_t)F);
  for (auto& c : frames)
    if (!read_cloud(f, c)) return 2;
  fclose(f);
  std::vector<OdomRecord> odom((size_t)F);
  FILE* o = fopen(argv[4], "rb");
  if (!o) return 2;
  for (auto& r : odom)
    if (fread(&r.has, 4, 1, o) != 1 || fread(r.v, 8, 7, o) != 7) return 2;
  fclose(o);
  FILE* g = fopen(argv[5], "wb");
  if (!g) return 2;
  int rc = drive(lidar, frames, odom, true, g);
  if (rc == 0) rc = drive(lidar, frames, odom, false, g);
  fclose(g);
  return rc;
}
