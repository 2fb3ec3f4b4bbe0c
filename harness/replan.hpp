// CPU restatement (checker, not product) of what runs around planMomaParallel while the robot moves:
//   MomaTraj::setTraj / init / getState / getDState   planner/include/planner/moma_traj_opt.h:40-158
//   Planner::safeCallback                            planner/src/planner.cpp:597-638
//   the endpoints of Planner::replanCallback          planner/src/planner.cpp:708-731
// With the reference's structure: serial loops, running sums, a break at the first hit, libm's sin / cos.  The map
// queries and the collision spheres are the oracle's restatements (GridMap::getDistance2d / 3d, MomaParam::getColliPts).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <vector>

#include "../oracle/topay_oracle.hpp"

namespace topay_wl {

struct ReplanTraj {   // MomaTraj
  double start_state[3] = {0, 0, 0};
  std::vector<double> T;                        // durations
  std::vector<double> C;                        // [piece][9][6], coefficient of t^5 first (CoefficientMat)
  std::vector<std::array<double, 4>> car_seq;   // (x, y, theta, t) every 0.1 s

  int pieces() const { return (int)T.size(); }
  double totalDuration() const {                // minco.hpp:304-313
    double s = 0.0;
    for (double d : T) s += d;
    return s;
  }
  int locatePieceIdx(double& t) const {         // minco.hpp:356-374
    const int N = pieces();
    int idx;
    double dur;
    for (idx = 0; idx < N && t > (dur = T[idx]); idx++) t -= dur;
    if (idx == N) { idx--; t += T[idx]; }
    return idx;
  }
  double ck(int i, int d, int k) const { return C[(size_t)i * 54 + d * 6 + 5 - k]; }
  void getPos(double t, double out[9]) const {  // minco.hpp:103-117
    const int i = locatePieceIdx(t);
    for (int d = 0; d < 9; d++) {
      double v = 0.0, tn = 1.0;
      for (int k = 0; k <= 5; k++) { v += tn * ck(i, d, k); tn *= t; }
      out[d] = v;
    }
  }
  void getVel(double t, double out[9]) const {  // minco.hpp:119-133
    const int i = locatePieceIdx(t);
    for (int d = 0; d < 9; d++) {
      double v = 0.0, tn = 1.0;
      int n = 1;
      for (int k = 1; k <= 5; k++) { v += n * tn * ck(i, d, k); tn *= t; n++; }
      out[d] = v;
    }
  }
  void init() {                                 // moma_traj_opt.h:71-94
    const double seq_res = 0.1;
    const int approx_res = 4;
    const double h = seq_res / approx_res, hh = h / 2.0, h6 = h / 6.0;
    car_seq.clear();
    double cx = start_state[0], cy = start_state[1];
    car_seq.push_back({cx, cy, start_state[2], 0.0});
    const int num = (int)std::floor(totalDuration() / h);
    double p1[9], p2[9], p3[9], v1[9], v2[9], v3[9];
    getPos(0.0, p3);
    getVel(0.0, v3);
    for (int i = 0; i < num; i++) {
      for (int d = 0; d < 2; d++) { p1[d] = p3[d]; v1[d] = v3[d]; }
      getPos(i * h + hh, p2); getVel(i * h + hh, v2);
      getPos(i * h + h, p3);  getVel(i * h + h, v3);
      cx += h6 * (v1[1] * std::cos(p1[0]) + 4.0 * v2[1] * std::cos(p2[0]) + v3[1] * std::cos(p3[0]));
      cy += h6 * (v1[1] * std::sin(p1[0]) + 4.0 * v2[1] * std::sin(p2[0]) + v3[1] * std::sin(p3[0]));
      if (i % approx_res == approx_res - 1) car_seq.push_back({cx, cy, p3[0], (i + 1) * h});
    }
  }
  void getState(double t, double state[10]) const {   // moma_traj_opt.h:113-137
    const double seq_res = 0.1;
    t = std::min(std::max(t, 0.0), totalDuration());
    const int index = (int)std::floor(t / seq_res);
    const double floor_t = index * seq_res, diff_t = t - floor_t;
    double cx = car_seq[index][0], cy = car_seq[index][1];
    double p1[9], p2[9], p3[9], v1[9], v2[9], v3[9];
    getPos(floor_t, p1); getVel(floor_t, v1);
    getPos(floor_t + diff_t / 2.0, p2); getVel(floor_t + diff_t / 2.0, v2);
    getPos(t, p3); getVel(t, v3);
    cx += diff_t / 6.0 * (v1[1] * std::cos(p1[0]) + 4.0 * v2[1] * std::cos(p2[0]) + v3[1] * std::cos(p3[0]));
    cy += diff_t / 6.0 * (v1[1] * std::sin(p1[0]) + 4.0 * v2[1] * std::sin(p2[0]) + v3[1] * std::sin(p3[0]));
    state[0] = cx; state[1] = cy; state[2] = p3[0];
    for (int q = 0; q < 7; q++) state[3 + q] = p3[2 + q];
  }
  void getDState(double t, double state[10]) const {  // moma_traj_opt.h:149-158
    for (int a = 0; a < 10; a++) state[a] = 0.0;
    t = std::min(std::max(t, 0.0), totalDuration());
    double v[9];
    getVel(t, v);
    state[0] = v[1];
    state[1] = v[0];
    for (int q = 0; q < 7; q++) state[3 + q] = v[2 + q];
  }
};

struct ReplanSafe {
  bool is_safe = true;
  int sample = -1, body = -1;          // first hit: sample index, body (0 chassis, 1..12 spheres)
  double t = 0.0 / 0.0, d = 0.0 / 0.0; // its time and distance
  // smallest |d - 0.99 r| over every body of every sample up to and including the first hit: how far the verdict, the sample
  // and the body are from depending on rounding
  double min_margin = 1.0e+300;
};

// Planner::safeCallback, planner.cpp:597-638
inline ReplanSafe replan_safe(const ReplanTraj& end_traj, const topay_oracle::Map& grid_map, const topay_oracle::Robot& moma_param) {
  ReplanSafe out;
  double temp_state[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const std::vector<topay_oracle::Sphere> min_dist_mani = moma_param.getColliPts(temp_state);
  const double res = 0.01;
  int k = 0;
  for (double t = 0.0; t < end_traj.totalDuration(); t += res, k++) {
    double state[10];
    end_traj.getState(t, state);
    const std::vector<topay_oracle::Sphere> mani_pts = moma_param.getColliPts(state);
    {   // (the margin of every body of this sample, whether or not the loop below gets to it)
      out.min_margin = std::min(out.min_margin, std::fabs(grid_map.getDistance2d(state) - moma_param.chassis_colli_radius * 0.99));
      for (size_t i = 0; i < mani_pts.size(); i++) {
        const double pc[3] = {mani_pts[i].p.x, mani_pts[i].p.y, mani_pts[i].p.z};
        out.min_margin = std::min(out.min_margin, std::fabs(grid_map.getDistance3d(pc) - min_dist_mani[i].r * 0.99));
      }
    }
    double d = grid_map.getDistance2d(state);
    if (d < moma_param.chassis_colli_radius * 0.99) {
      out.is_safe = false; out.sample = k; out.body = 0; out.t = t; out.d = d;
      break;
    }
    for (size_t i = 0; i < mani_pts.size(); i++) {
      const double pc[3] = {mani_pts[i].p.x, mani_pts[i].p.y, mani_pts[i].p.z};
      const double d3 = grid_map.getDistance3d(pc);
      if (d3 < min_dist_mani[i].r * 0.99) {
        out.is_safe = false; out.sample = k; out.body = (int)i + 1; out.t = t; out.d = d3;
        break;
      }
    }
    if (!out.is_safe) break;
  }
  return out;
}

// Planner::replanCallback, planner.cpp:708-731.  global_traj may be null (no trajectory: the goal is global_goal).
// Returns the index of the step that gave local_goal, -1 for global_goal.
inline int replan_endpoints(const ReplanTraj& end_traj, const ReplanTraj* global_traj, double since_last_replan, double since_begin,
                            const double global_goal[10], double planning_budget, double planning_horizon, double local_start[10],
                            double local_v[10], double local_goal[10]) {
  {
    const double t = since_last_replan + planning_budget;
    end_traj.getState(t, local_start);
    end_traj.getDState(t, local_v);
  }
  double t = since_begin;
  int k = 0;
  if (global_traj)
    for (; t < global_traj->totalDuration(); t += 0.1, k++) {
      double state[10];
      global_traj->getState(t, state);
      const double dx = state[0] - local_start[0], dy = state[1] - local_start[1];
      if (std::sqrt(dx * dx + dy * dy) > planning_horizon) {
        for (int a = 0; a < 10; a++) local_goal[a] = state[a];
        return k;
      }
    }
  for (int a = 0; a < 10; a++) local_goal[a] = global_goal[a];
  return -1;
}

}  // namespace topay_wl
