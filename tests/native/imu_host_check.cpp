// The IMU de-skew's shared host / device body (csrc/llsr_imu.h) as a stand-alone program for
// AddressSanitizer / UBSan (tests/test_imu_native.py): the per-point body over heap buffers of
// exactly the window's and the cloud's sizes, for every window length the ring can produce and the
// edge windows (all samples older, all newer, equal stamps, one candidate); the ring callback across
// two wraps and the window copy at every pointer distance. Prints OK.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "llsr_imu.h"

static int g_fail = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);   \
      ++g_fail;                                                 \
    }                                                           \
  } while (0)

static llsr_imu_msg message(double t, double yaw) {
  llsr_imu_msg m = llsr_imu_msg();
  m.sec = (int32_t)t;
  m.nanosec = (uint32_t)((t - (double)m.sec) * 1e9);
  m.orientation[2] = std::sin(yaw / 2);
  m.orientation[3] = std::cos(yaw / 2);
  m.angular_velocity[0] = 0.1;
  m.angular_velocity[2] = -0.2;
  m.linear_acceleration[0] = 0.3;
  m.linear_acceleration[2] = 9.81;
  return m;
}

// one scan of S points over a window of n candidates whose stamps start at t0 and step by dt
static void one_scan(int n, int S, double t0, double dt, double scan_time, llsr_imu_carry* carry) {
  llsr_imu_sample* win = n > 0 ? new llsr_imu_sample[n + 1] : nullptr;  // exactly n + 1 entries
  for (int k = 0; k <= n && n > 0; ++k) {
    win[k] = llsr_imu_sample();
    win[k].time = t0 + dt * k;
    win[k].roll = 0.01f * (float)k;
    win[k].pitch = -0.02f * (float)(k % 7);
    win[k].yaw = 3.0f - 6.1f * (float)(k & 1);  // jumps by more than pi between neighbours
    for (int a = 0; a < 3; ++a) {
      win[k].velo[a] = 0.1f * (float)(k + a);
      win[k].angular_rotation[a] = 0.05f * (float)(k - a);
    }
  }
  float* seg = S > 0 ? new float[4 * (size_t)S] : nullptr;  // exactly S points
  float* out = S > 0 ? new float[4 * (size_t)S] : nullptr;
  for (int i = 0; i < S; ++i) {
    const double az = 3.13 - 6.26 * (double)i / (double)(S > 1 ? S - 1 : 1);
    seg[4 * i + 0] = (float)(10.0 * std::cos(az));
    seg[4 * i + 1] = (float)(10.0 * std::sin(az));
    seg[4 * i + 2] = (float)(0.1 * (i % 5));
    seg[4 * i + 3] = (float)(i % 16) + 0.0123f;
  }
  const float ori3[3] = {-3.13f, 3.13f + 6.2831855f - 6.26f, 6.2831855f};
  llsr_imu::deskew_host(0.1f, scan_time, win, n, seg, S, ori3, carry, out);
  for (int i = 0; i < S; ++i) CHECK(n > 0 || (out[4 * i] == seg[4 * i + 1] && out[4 * i + 2] == seg[4 * i]));
  if (n > 0 && S > 0) {
    CHECK(out[0] == seg[1] && out[1] == seg[2] && out[2] == seg[0]);  // point 0 is not rotated
    // the search alone, over exactly n + 1 times: stays inside [1, n] for any point time
    std::vector<double> t(n + 1);
    std::vector<float> z(n + 1, 0.f);
    for (int k = 0; k <= n; ++k) t[k] = win[k].time;
    const llsr_imu::Window w{t.data(), z.data(), z.data(), z.data(), n};
    const float probes[] = {-1e9f, -0.05f, 0.f, 0.05f, 0.0999f, 0.1f, 1e9f, NAN};
    for (float pt : probes) {
      const llsr_imu::Sel s = llsr_imu::select(w, scan_time, pt);
      CHECK(s.front >= 1 && s.front <= n);
    }
  }
  delete[] win;
  delete[] seg;
  delete[] out;
}

int main() {
  // ---- the ring: 450 messages (two wraps), two gaps that skip the accumulate step ----
  llsr_imu_state st;
  llsr_imu::init(st);
  CHECK(st.pointer_last == -1 && st.pointer_last_iteration == 0);
  llsr_imu_sample* win = new llsr_imu_sample[LLSR_IMU_WINDOW_MAX];
  CHECK(llsr_imu::scan_window(st, win) == 0 && st.pointer_last_iteration == -1);
  double t = 100.0;
  for (int i = 0; i < 450; ++i) {
    t += (i == 120 || i == 333) ? 0.4 : 0.01;
    const llsr_imu_msg m = message(t, 3.0 + 0.01 * i);
    const double yaw = std::atan2(std::sin(3.0 + 0.01 * i), std::cos(3.0 + 0.01 * i));
    llsr_imu::callback_rpy(st, m, 0.0, 0.0, yaw, 0.1f);
    CHECK(st.pointer_last == i % LLSR_IMU_QUEUE);
    if (i % 37 == 0 || i == 449) {  // windows at many pointer distances, across both wraps
      const int before = st.pointer_last_iteration < 0 ? 0 : st.pointer_last_iteration;
      const int n = llsr_imu::scan_window(st, win);
      CHECK(n == (st.pointer_last - before + LLSR_IMU_QUEUE) % LLSR_IMU_QUEUE + 1);
      CHECK(n >= 1 && n <= LLSR_IMU_QUEUE);
      CHECK(win[n].time == st.time[st.pointer_last]);
      CHECK(st.pointer_last_iteration == st.pointer_last);
    }
  }
  delete[] win;
  // ---- the per-point body: every window length, cloud sizes around the edge cases ----
  llsr_imu_carry carry = llsr_imu_carry();
  const int sizes[] = {0, 1, 2, 11, 1013};
  for (int n = 0; n <= LLSR_IMU_QUEUE; n += (n < 4 || n > 196) ? 1 : 13)
    for (int S : sizes) one_scan(n, S, 99.95, 0.01, 100.0, &carry);
  one_scan(10, 300, 50.0, 0.01, 100.0, &carry);    // every sample older than the scan
  one_scan(10, 300, 150.0, 0.01, 100.0, &carry);   // every sample newer: extrapolates
  one_scan(10, 300, 100.02, 0.0, 100.0, &carry);   // equal stamps: a zero divisor
  one_scan(1, 300, 100.05, 0.01, 100.0, &carry);   // one candidate
  llsr_imu_carry fresh = llsr_imu_carry();
  one_scan(0, 300, 0.0, 0.0, 100.0, &fresh);       // no IMU: the carry stays
  llsr_imu_carry zero = llsr_imu_carry();
  CHECK(std::memcmp(&fresh, &zero, sizeof zero) == 0);
  if (g_fail) return 1;
  std::printf("OK\n");
  return 0;
}
