// CPU checker of the sensor-cloud entries (include/topay.h: topay_sense_*): a plain sequential restatement of rog_map's ProbMap in
// the reference's order -- the cloud loop, then the ray loop, then the flush of the update queue.
//   ProbMap::updateProbMap            src/rog_map/src/rog_map/prob_map.cpp:302-373
//   raycastProcess                    prob_map.cpp:666-779
//   insertUpdateCandidate             prob_map.cpp:781-790
//   updateLocalBox                    prob_map.cpp:792-822
//   probabilisticMapFromCache         prob_map.cpp:544-568
//   hitPointUpdate / missPointUpdate  prob_map.cpp:570-664 (the counter maps they feed are out of scope)
//   RayCaster::setInput / step        src/rog_map/include/utils/raycaster.cpp:65-192 (ORIGIN_AT_CORNER, CMakeLists.txt:14)
//   lineBoxIntersectPoint             src/rog_map/include/utils/common_lib.hpp:148-170
//   logit                             src/rog_map/include/rog_map/rog_map_core/config.hpp:229-235
//   SlidingMap::mapSliding            src/rog_map/src/rog_map/sliding_map.cpp:113-166, clearMemoryOutOfMap 96-111
//   the two triggers of a slide       prob_map.cpp:306-311, 324-328
// Configuration: raycasting on, no ESDF, no frontiers, no inflation.  The sliding window is a step of its own (slide): the local map
// is the grid given to reset until then.  As in the reference the buffers are addressed as a ring (getLocalIndexHash of the index
// modulo the size, sliding_map.cpp:168-173, 205-): a slide clears the slabs that leave and moves the origin, no voxel is copied.
// Every position is moved into the grid's frame first (u = p - origin) and the reference's code runs on u.  The first-frame clearing
// of a sphere of raycast_range_min (356-372) is not restated: range_min is 0.
// This is the checker only; nothing on the product path includes it.  Its parity with rog_map itself is not pinned (rog_map needs
// Eigen, PCL and ROS).  The range sensor at the end is not a restatement; its sin / cos are the library's deterministic ones
// (FreeBSD msun k_sin / k_cos with a two-step Cody-Waite reduction), restated so that a ray's direction has the library's bits.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <queue>
#include <vector>

namespace prob_map {

struct Params {   // == topay_sense_params_t
  float p_min, p_miss, p_free, p_occ, p_hit, p_max;
  double ray_range[2];
  int point_filt_num, batch_update_size, intensity_thresh, reserved;
  double virtual_ceil_height, virtual_ground_height;
  double local_update_box[3];
  double chassis_height;
};

inline float logit(float x) { return (float)std::log((double)(x / (1.0f - x))); }

struct Vec3 { double v[3]; double& operator[](int i) { return v[i]; } double operator[](int i) const { return v[i]; } };
struct Idx3 { int v[3]; int& operator[](int i) { return v[i]; } int operator[](int i) const { return v[i]; } };

struct RayCaster {
  double res = 0.1;
  int cur[3] = {0, 0, 0}, end[3] = {0, 0, 0}, dir[3] = {0, 0, 0};
  double t_to_bound[3] = {0, 0, 0}, t_when_step[3] = {0, 0, 0};
  static int signum(int x) { return x == 0 ? 0 : (x < 0 ? -1 : 1); }
  int posToIndex(double d) const { return (int)std::floor(d / res); }
  double indexToPos(int id) const { return (id + 0.5) * res; }
  bool setInput(const Vec3& start, const Vec3& e) {
    for (int a = 0; a < 3; a++) {
      cur[a] = posToIndex(start[a]);
      end[a] = posToIndex(e[a]);
      dir[a] = signum(end[a] - cur[a]);
    }
    if (dir[0] == 0 && dir[1] == 0 && dir[2] == 0) return false;
    double dis[3];
    for (int a = 0; a < 3; a++) dis[a] = std::abs(e[a] - start[a]);
    const double t_max = std::sqrt(dis[0] * dis[0] + dis[1] * dis[1] + dis[2] * dis[2]);
    for (int a = 0; a < 3; a++) dis[a] /= t_max;
    for (int a = 0; a < 3; a++) {
      t_when_step[a] = dir[a] == 0 ? std::numeric_limits<double>::max() : std::abs(res / dis[a]);
      const double next_bound = indexToPos(cur[a]) + dir[a] * res * 0.5;
      t_to_bound[a] = dir[a] == 0 ? std::numeric_limits<double>::max() : std::fabs(next_bound - start[a]) / dis[a];
    }
    return true;
  }
  bool step(Idx3& id) {
    for (int a = 0; a < 3; a++) id[a] = cur[a];
    if (cur[0] == end[0] && cur[1] == end[1] && cur[2] == end[2]) return false;
    if (t_to_bound[0] < t_to_bound[1]) {
      if (t_to_bound[0] < t_to_bound[2]) { cur[0] += dir[0]; t_to_bound[0] += t_when_step[0]; }
      else { cur[2] += dir[2]; t_to_bound[2] += t_when_step[2]; }
    } else {
      if (t_to_bound[1] < t_to_bound[2]) { cur[1] += dir[1]; t_to_bound[1] += t_when_step[1]; }
      else { cur[2] += dir[2]; t_to_bound[2] += t_when_step[2]; }
    }
    return true;
  }
};

inline Vec3 normalized(const Vec3& d) {   // Eigen's: v / sqrt(squaredNorm) when that is positive
  const double n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  if (!(n2 > 0.0)) return d;
  const double n = std::sqrt(n2);
  return Vec3{{d[0] / n, d[1] / n, d[2] / n}};
}

struct ProbMap {
  double origin[3] = {0, 0, 0}, res = 0.1, res_inv = 10.0;
  int dims[3] = {0, 0, 0};
  int ring[3] = {0, 0, 0};   // ring address of local voxel 0, per axis
  std::vector<float> occupancy_buffer;
  std::vector<int> operation_cnt, hit_cnt;
  std::queue<Idx3> update_cache;
  int batch_update_counter = 0;
  float l_hit = 0, l_miss = 0, l_min = 0, l_max = 0, l_occ = 0, l_free = 0;

  void reset(const double* origin_, double res_, const int* dims_) {
    for (int a = 0; a < 3; a++) { origin[a] = origin_[a]; dims[a] = dims_[a]; ring[a] = 0; }
    res = res_;
    res_inv = 1.0 / res_;
    const size_t n3 = (size_t)dims[0] * dims[1] * dims[2];
    occupancy_buffer.assign(n3, 0.0f);   // prob_map.cpp:78
    operation_cnt.assign(n3, 0);
    hit_cnt.assign(n3, 0);
    update_cache = std::queue<Idx3>();
    batch_update_counter = 0;
  }
  size_t address(const Idx3& id) const {
    const int r[3] = {(id[0] + ring[0]) % dims[0], (id[1] + ring[1]) % dims[1], (id[2] + ring[2]) % dims[2]};
    return ((size_t)r[0] * dims[1] + r[1]) * dims[2] + r[2];
  }
  bool insideLocalMap(const Idx3& id) const {
    for (int a = 0; a < 3; a++)
      if (id[a] < 0 || id[a] >= dims[a]) return false;
    return true;
  }
  Idx3 posToGlobalIndex(const Vec3& p) const {
    return Idx3{{(int)std::floor(p[0] * res_inv), (int)std::floor(p[1] * res_inv), (int)std::floor(p[2] * res_inv)}};
  }
  void insertUpdateCandidate(const Idx3& id, bool is_hit) {
    const size_t h = address(id);
    operation_cnt[h]++;
    if (operation_cnt[h] == 1) update_cache.push(id);
    if (is_hit) hit_cnt[h]++;
  }
  void setParams(const Params& P) {
    l_hit = logit(P.p_hit); l_miss = logit(P.p_miss); l_min = logit(P.p_min);
    l_max = logit(P.p_max); l_occ = logit(P.p_occ); l_free = logit(P.p_free);
  }

  // updateProbMap.  xyzi: n points of four floats; sensor: world frame.  Returns 1 flushed, 0 batch open, -1 / -2 above the
  // ceiling / below the ground.
  int update(const float* xyzi, int n, const double* sensor, const Params& P) {
    if (sensor[2] > P.virtual_ceil_height) return -1;
    if (sensor[2] < P.virtual_ground_height) return -2;
    setParams(P);
    const Vec3 cur_odom{{sensor[0] - origin[0], sensor[1] - origin[1], sensor[2] - origin[2]}};
    const double ceil_u = P.virtual_ceil_height - origin[2], ground_u = P.virtual_ground_height - origin[2];
    const int filt = P.point_filt_num > 0 ? P.point_filt_num : 1, batch = P.batch_update_size > 0 ? P.batch_update_size : 1;
    // updateLocalBox
    Vec3 box_min, box_max;
    const Idx3 odom_i = posToGlobalIndex(cur_odom);
    for (int a = 0; a < 3; a++) {
      const int half = (int)(P.local_update_box[a] / 2 / res);
      box_max[a] = std::fmin(((double)(odom_i[a] + half) + 0.5) * res, ((double)(dims[a] - 1) + 0.5) * res);
      box_min[a] = std::fmax(((double)(odom_i[a] - half) + 0.5) * res, 0.5 * res);
    }
    // raycastProcess, the cloud loop
    const double range_max = P.ray_range[1], range_min = P.ray_range[0], sqr_range_max = range_max * range_max;
    std::vector<Vec3> raycasting_cloud;
    int temperol_cnt = 0;
    for (int i = 0; i < n; i++) {
      const float* q = xyzi + 4 * (size_t)i;
      if (P.intensity_thresh > 0 && q[3] < (float)P.intensity_thresh) continue;   // 1.1
      if (temperol_cnt++ % filt) continue;                                        // 1.2
      Vec3 p{{(double)q[0] - origin[0], (double)q[1] - origin[1], (double)q[2] - origin[2]}};
      if (!(std::fabs(p[0]) < 1e300 && std::fabs(p[1]) < 1e300 && std::fabs(p[2]) < 1e300)) continue;   // (not a position: no ray)
      bool update_hit = true;
      if (p[2] > ceil_u || p[2] < ground_u) {   // 1.3
        update_hit = false;
        const double dz = p[2] - cur_odom[2], pc = (p[2] > ceil_u ? ceil_u : ground_u) - cur_odom[2];
        const Vec3 nn = normalized(Vec3{{p[0] - cur_odom[0], p[1] - cur_odom[1], p[2] - cur_odom[2]}});
        for (int a = 0; a < 3; a++) p[a] = cur_odom[a] + nn[a] * pc / dz;
      }
      const Vec3 d{{p[0] - cur_odom[0], p[1] - cur_odom[1], p[2] - cur_odom[2]}};
      const double sqr_dis = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      if (sqr_dis > sqr_range_max) {   // 1.4
        const double k = range_max / std::sqrt(sqr_dis);
        for (int a = 0; a < 3; a++) p[a] = k * d[a] + cur_odom[a];
        update_hit = false;
      }
      const double mn = std::fmin(std::fmin(p[0] - box_min[0], p[1] - box_min[1]), p[2] - box_min[2]);
      const double mx = std::fmax(std::fmax(p[0] - box_max[0], p[1] - box_max[1]), p[2] - box_max[2]);
      if (mn < 0 || mx > 0) {   // lineBoxIntersectPoint(p, cur_odom, box_min, box_max)
        const Vec3 diff{{p[0] - cur_odom[0], p[1] - cur_odom[1], p[2] - cur_odom[2]}};
        double min_t = 1000000;
        for (int a = 0; a < 3; a++)
          if (std::fabs(diff[a]) > 0) {
            const double t1 = (box_max[a] - cur_odom[a]) / diff[a];
            if (t1 > 0 && t1 < min_t) min_t = t1;
            const double t2 = (box_min[a] - cur_odom[a]) / diff[a];
            if (t2 > 0 && t2 < min_t) min_t = t2;
          }
        for (int a = 0; a < 3; a++) p[a] = cur_odom[a] + (min_t - 1e-3) * diff[a];
        update_hit = false;
      }
      raycasting_cloud.push_back(p);
      if (update_hit) {
        const Idx3 id = posToGlobalIndex(p);
        if (insideLocalMap(id)) insertUpdateCandidate(id, true);   // (always inside: the update box is)
      }
    }
    // the ray loop
    RayCaster rc;
    rc.res = res;
    for (const Vec3& p : raycasting_cloud) {
      const Vec3 nn = normalized(Vec3{{p[0] - cur_odom[0], p[1] - cur_odom[1], p[2] - cur_odom[2]}});
      const Vec3 start{{nn[0] * range_min + cur_odom[0], nn[1] * range_min + cur_odom[1], nn[2] * range_min + cur_odom[2]}};
      rc.setInput(start, p);
      Idx3 id;
      while (rc.step(id)) {
        if (!insideLocalMap(id)) break;
        insertUpdateCandidate(id, false);
      }
    }
    batch_update_counter++;
    if (batch_update_counter < batch) return 0;
    batch_update_counter = 0;
    // probabilisticMapFromCache
    while (!update_cache.empty()) {
      const Idx3 id = update_cache.front();
      update_cache.pop();
      const size_t h = address(id);
      float& ret = occupancy_buffer[h];
      if (hit_cnt[h] > 0) {
        ret += l_hit * hit_cnt[h];
        if (ret > l_max) ret = l_max;
      } else {
        ret += l_miss * (operation_cnt[h] - hit_cnt[h]);
        if (ret < l_min) ret = l_min;
      }
      hit_cnt[h] = 0;
      operation_cnt[h] = 0;
    }
    return 1;
  }

  void resetCell(size_t h) { occupancy_buffer[h] = 0.0f; }   // prob_map.cpp:511- (the counter maps it feeds are out of scope)
  void resetLocalMap() {                                     // prob_map.cpp:823-831
    std::fill(occupancy_buffer.begin(), occupancy_buffer.end(), 0.0f);
    update_cache = std::queue<Idx3>();
    batch_update_counter = 0;
    std::fill(operation_cnt.begin(), operation_cnt.end(), 0);
    std::fill(hit_cnt.begin(), hit_cnt.end(), 0);
  }
  // The slide of updateProbMap for one sensor position.  Returns 0 within the threshold, 1 slid, 2 slid because the sensor was
  // outside the local map (the reference then drops the cloud), -1 a batch is open; shift: the voxels the window moved by.
  // slide_z false: z takes no part (the deviation of include/topay.h).
  int slide(const double* sensor, double threshold, bool slide_z, int* shift) {
    shift[0] = shift[1] = shift[2] = 0;
    if (batch_update_counter != 0) return -1;   // the condition of both slides (prob_map.cpp:306, 324)
    const int axes = slide_z ? 3 : 2;
    const Vec3 pos{{sensor[0] - origin[0], sensor[1] - origin[1], sensor[2] - origin[2]}};
    const Idx3 new_origin_i = posToGlobalIndex(pos);
    int local_map_origin_i[3];                   // the centre voxel of the window, in the grid's frame
    double local_map_origin_d[3];                // origin_i * resolution: its low corner (sliding_map.cpp:118)
    for (int a = 0; a < 3; a++) { local_map_origin_i[a] = dims[a] / 2; local_map_origin_d[a] = (double)local_map_origin_i[a] * res; }
    bool inside = true;                          // insideLocalMap(pos), on the sliding axes
    for (int a = 0; a < axes; a++) inside = inside && new_origin_i[a] >= 0 && new_origin_i[a] < dims[a];
    int status;
    if (!inside) status = 2;                     // prob_map.cpp:306-311
    else {
      double n2 = 0.0;                           // (pos - local_map_origin_d_).norm(), prob_map.cpp:326
      for (int a = 0; a < axes; a++) { const double d = pos[a] - local_map_origin_d[a]; n2 = a == 0 ? d * d : n2 + d * d; }
      if (!(std::sqrt(n2) > threshold)) return 0;
      status = 1;
    }
    // mapSliding
    int shift_num[3] = {0, 0, 0};
    for (int a = 0; a < axes; a++) shift_num[a] = new_origin_i[a] - local_map_origin_i[a];
    bool all = false;
    for (int a = 0; a < 3; a++) all = all || std::abs(shift_num[a]) > dims[a];
    if (all) resetLocalMap();                    // sliding_map.cpp:121-128
    else
      for (int i = 0; i < 3; i++) {              // the slabs that leave, axis by axis (130-163, clearMemoryOutOfMap)
        if (shift_num[i] == 0) continue;
        std::vector<int> clear_id;               // local indices on axis i before the slide
        if (shift_num[i] > 0) for (int k = 0; k < shift_num[i]; k++) clear_id.push_back(k % dims[i]);
        else for (int k = -1; k >= shift_num[i]; k--) clear_id.push_back(((dims[i] + k) % dims[i] + dims[i]) % dims[i]);
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        for (int idd : clear_id)
          for (int x = 0; x < dims[i1]; x++)
            for (int y = 0; y < dims[i2]; y++) {
              Idx3 id;
              id[i] = idd; id[i1] = x; id[i2] = y;
              resetCell(address(id));
            }
      }
    // updateLocalMapOriginAndBound: local voxel l is now what was l + shift, the frame moves by whole voxels
    for (int a = 0; a < 3; a++) {
      ring[a] = ((ring[a] + shift_num[a]) % dims[a] + dims[a]) % dims[a];
      origin[a] = origin[a] + (double)shift_num[a] * res;
      shift[a] = shift_num[a];
    }
    return status;
  }
  // a buffer in local order [nx][ny][nz]
  template <typename T> void unring(const std::vector<T>& buf, T* out) const {
    Idx3 id;
    size_t k = 0;
    for (id[0] = 0; id[0] < dims[0]; id[0]++)
      for (id[1] = 0; id[1] < dims[1]; id[1]++)
        for (id[2] = 0; id[2] < dims[2]; id[2]++) out[k++] = buf[address(id)];
  }

  // isOccupied per voxel, its projection, and the cells with an occupied voxel whose centre is below the chassis height
  void occupancy(float l_occ_, double chassis_height, int8_t* occ2d, int8_t* occ2d_critical, int8_t* occ3d) const {
    const size_t n2 = (size_t)dims[0] * dims[1];
    for (size_t c = 0; c < n2; c++) {
      bool any = false, low = false;
      for (int z = 0; z < dims[2]; z++) {
        const bool occ = occupancy_buffer[address(Idx3{{(int)(c / dims[1]), (int)(c % dims[1]), z}})] >= l_occ_;
        occ3d[c * dims[2] + z] = occ ? 1 : 0;
        any = any || occ;
        low = low || (occ && origin[2] + ((double)z + 0.5) * res < chassis_height);
      }
      occ2d_critical[c] = any ? 1 : 0;
      occ2d[c] = low ? 1 : 0;
    }
  }
};

// ---- the library's deterministic sin / cos (topay_amd/csrc/topay_math.h), operation by operation -------------------------
inline double k_sin(double x, double y) {
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
               S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double z = x * x, w = z * z;
  const double r = S2 + z * (S3 + z * S4) + z * w * (S5 + z * S6);
  const double v = z * x;
  return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
inline double k_cos(double x, double y) {
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
               C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double z = x * x, w0 = z * z;
  const double r = z * (C1 + z * (C2 + z * C3)) + (w0 * w0) * (C4 + z * (C5 + z * C6));
  const double hz = 0.5 * z, w = 1.0 - hz;
  return w + (((1.0 - w) - hz) + (z * r - x * y));
}
inline void det_sincos(double x, double* sn, double* cs) {
  const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00, pio2_2 = 6.07710050630396597660e-11,
               pio2_2t = 2.02226624879595063154e-21;
  const double fn = std::rint(x * invpio2);
  const double t = x - fn * pio2_1;
  double w = fn * pio2_2;
  const double r = t - w;
  w = fn * pio2_2t - ((t - r) - w);
  const double y0 = r - w, y1 = (r - y0) - w;
  const double s = k_sin(y0, y1), c = k_cos(y0, y1);
  const int n = (int)((long long)fn & 3);
  *sn = n == 0 ? s : n == 1 ? c : n == 2 ? -s : -c;
  *cs = n == 0 ? c : n == 1 ? -s : n == 2 ? -c : s;
}

// The range sensor of topay_sense_scan for one pose (x, y, z, yaw), ray by ray: out[n_az * n_el][4].
inline void scan(const int8_t* occ3d, const double* origin, double res, const int* dims, const double* pose, int n_az, int n_el, double fov,
                 double range, float* out) {
  RayCaster rc;
  rc.res = res;
  for (int i = 0; i < n_az; i++)
    for (int j = 0; j < n_el; j++) {
      const double az = 6.283185307179586 * (double)i / (double)n_az + pose[3], el = fov * (((double)j + 0.5) / (double)n_el - 0.5);
      double sa, ca, se, ce;
      det_sincos(az, &sa, &ca);
      det_sincos(el, &se, &ce);
      const double dir[3] = {ce * ca, ce * sa, se};
      Vec3 s, e;
      for (int a = 0; a < 3; a++) { s[a] = pose[a] - origin[a]; e[a] = s[a] + dir[a] * range; }
      rc.setInput(s, e);
      Idx3 id;
      bool found = false;
      for (;;) {
        const bool more = rc.step(id);
        if (id[0] < 0 || id[1] < 0 || id[2] < 0 || id[0] >= dims[0] || id[1] >= dims[1] || id[2] >= dims[2]) break;
        if (occ3d[((size_t)id[0] * dims[1] + id[1]) * dims[2] + id[2]]) { found = true; break; }
        if (!more) break;
      }
      float* q = out + 4 * ((size_t)i * n_el + j);
      for (int a = 0; a < 3; a++) q[a] = found ? (float)(origin[a] + ((double)id[a] + 0.5) * res) : (float)(pose[a] + dir[a] * (1.5 * range));
      q[3] = 0.0f;
    }
}

}  // namespace prob_map
