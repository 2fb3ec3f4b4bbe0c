// TEST INFRASTRUCTURE: serial CPU restatement (libm) of the end-effector goal solve, the checker of topay_ee_*.
//   MomaParam::getFKPose       simulator/fake_moma/include/fake_moma/moma_param.h:339-373
//   MomaParam::getEEGrads      moma_param.h:375-468, in the reference's own triple-loop structure
//   MomaTrajOpt::eeCostCallback planner/src/moma_traj_opt.cpp:48-140, with the gradient ASSIGNED (the reference adds into a
//                              vector lbfgs_optimize never clears: lines 135-137, lbfgs.hpp:504, 523, 318)
//   MomaTrajOpt::optimizeEE    moma_traj_opt.cpp:5-46, driven by the oracle's restatement of lbfgs.hpp
// The reference ships no vectors for any of this; tests/test_ee_goal.py pins the gradient by central differences.
#pragma once
#include <cmath>
#include <vector>

#include "../oracle/topay_oracle.hpp"

namespace ee_goal {
using topay_oracle::M3;
using topay_oracle::Map;
using topay_oracle::Robot;
using topay_oracle::V3;

struct Weights {   // moma_traj_opt.cpp:68-70, 78
  double cost_scale = 10.0, mani_colli_weight = 100.0, self_colli_weight = 100.0, clearance = 1.1;
};

inline void getFKPose(const Robot& mp, const double* moma_pos, double* fk_pose) {
  V3 now_p{moma_pos[0], moma_pos[1], mp.chassis_height};
  M3 now_R = Robot::rotZ(moma_pos[2]);
  now_p = now_p + now_R * mp.relative_t;
  now_R = now_R * mp.relative_R;
  for (int i = 0; i < Robot::dof; i++) {
    now_p = now_p + now_R.col(2) * mp.colli_length[i];
    const M3 dof_R = (i % 2 == 0) ? Robot::rotZ(moma_pos[3 + i]) : Robot::rotY(moma_pos[3 + i]);
    now_R = now_R * dof_R;
  }
  fk_pose[0] = now_p.x; fk_pose[1] = now_p.y; fk_pose[2] = now_p.z;
  for (int b = 0; b < 3; b++) { fk_pose[3 + b] = now_R.m[0][b]; fk_pose[6 + b] = now_R.m[1][b]; }
}

inline void getEEGrads(const Robot& mp, const double* moma_pos, const double* ee_grad, double* moma_grads) {
  const int dof = Robot::dof;
  for (int i = 0; i < 10; i++) moma_grads[i] = 0.0;
  V3 grad_p_list[8], grad_R_list[8];
  std::vector<M3> now_R_list, R_list, dR_list;
  M3 now_R = Robot::rotZ(moma_pos[2]);
  now_R = now_R * mp.relative_R;
  R_list.push_back(now_R);
  M3 dR = Robot::drotZ(moma_pos[2]);
  dR = dR * mp.relative_R;
  dR_list.push_back(dR);
  for (int i = 0; i < dof; i++) {   // 399-426
    now_R_list.push_back(now_R);
    M3 dof_R;
    if (i % 2 == 0) { dof_R = Robot::rotZ(moma_pos[3 + i]); dR = Robot::drotZ(moma_pos[3 + i]); }
    else { dof_R = Robot::rotY(moma_pos[3 + i]); dR = Robot::drotY(moma_pos[3 + i]); }
    now_R = now_R * dof_R;
    R_list.push_back(dof_R);
    dR_list.push_back(dR);
  }
  grad_p_list[dof] = V3{ee_grad[0], ee_grad[1], ee_grad[2]};   // 428
  for (int i = dof; i > 0; i--) {   // 429-445
    moma_grads[2 + i] += dot(now_R_list[i - 1] * dR_list[i].col(2), grad_R_list[i]);
    for (int j = 0; j < i; j++) {
      M3 R1 = M3::identity();
      for (int k = 0; k < j; k++) R1 = R1 * R_list[k];
      R1 = R1 * dR_list[j];
      for (int k = j + 1; k <= i; k++) R1 = R1 * R_list[k];
      moma_grads[2 + j] += dot(R1.col(2), grad_R_list[i]);
    }
    grad_R_list[i - 1] = grad_R_list[i - 1] + grad_p_list[i] * mp.colli_length[i - 1];
    grad_p_list[i - 1] = grad_p_list[i - 1] + grad_p_list[i];
  }
  moma_grads[2] += dot(dR_list[0].col(2), grad_R_list[0]);   // 446-451
  const M3 dR0 = Robot::drotZ(moma_pos[2]);
  moma_grads[2] += dot(dR0 * mp.relative_t, grad_p_list[0]);
  moma_grads[0] = grad_p_list[0].x;
  moma_grads[1] = grad_p_list[0].y;
  for (int j = 0; j < dof + 1; j++) {   // grad Ree, 454-465
    M3 R1 = M3::identity();
    for (int k = 0; k < j; k++) R1 = R1 * R_list[k];
    R1 = R1 * dR_list[j];
    for (int k = j + 1; k <= dof; k++) R1 = R1 * R_list[k];
    for (int b = 0; b < 3; b++) moma_grads[2 + j] += R1.m[0][b] * ee_grad[3 + b];
    for (int b = 0; b < 3; b++) moma_grads[2 + j] += R1.m[1][b] * ee_grad[6 + b];
  }
}

// smoothL1Penalty, moma_traj_opt.h:810-830
inline void smoothL1Penalty(double pe, double xx, double& f, double& df) {
  const double half = 0.5 * pe, f3c = 1.0 / (pe * pe), f4c = -0.5 * f3c / pe, d2c = 3.0 * f3c, d3c = 4.0 * f4c;
  if (xx < pe) { f = (f4c * xx + f3c) * xx * xx * xx; df = (d3c * xx + d2c) * xx * xx; }
  else { f = xx - half; df = 1.0; }
}

// What the tests assert about a case: the cost by term, how many terms of each kind are active, spheres outside the map,
// and the distance of the point from everything across which the cost is not smooth.
struct Breakdown {
  double ee = 0, mani = 0, chassis = 0, pairs = 0;
  int n_mani = 0, n_chassis = 0, n_pairs = 0, n_outside = 0;
  double kink_penalty = 1e300;   // min |v|, |v - relu_mu| over every penalty argument v (environment, chassis top, pairs)
  double kink_cell = 1e300;      // min distance [m] of a sphere centre inside the map from a face of the interpolation cells or of the
                                 // in-map test (trilinear interpolation: the gradient jumps across cell faces)
  double kink_sigmoid = 1e300;   // min |Vq_i| (expC2 changes branch at 0)
};

struct Problem {
  const Map* grid_map = nullptr;
  Robot moma_param;
  Weights w;
  double relu_mu = 1.0e-3;
  double ee_pose[9];

  double cost(const double* Vq, double* gradVq, Breakdown* bd = nullptr) const {
    using T = topay_oracle::TrajOpt;
    const int dof = Robot::dof;
    double now_pos[10];
    for (int i = 0; i < 3; i++) now_pos[i] = Vq[i];
    for (int i = 0; i < dof; i++) now_pos[i + 3] = T::sigmoidC2(Vq[i + 3], moma_param.joint_pos_limit_max[i]);
    double ee_pose_now[9], grad_ee[9], moma_grad[10];
    getFKPose(moma_param, now_pos, ee_pose_now);
    double sq = 0.0;
    for (int a = 0; a < 9; a++) { grad_ee[a] = ee_pose_now[a] - ee_pose[a]; sq += grad_ee[a] * grad_ee[a]; }
    const double ee_cost = 0.5 * sq;
    getEEGrads(moma_param, now_pos, grad_ee, moma_grad);
    double sdf_cost = 0.0;
    const std::vector<topay_oracle::Sphere> colli_pts = moma_param.getColliPts(now_pos);
    std::vector<V3> pos_grads;
    Breakdown B;
    B.ee = ee_cost;
    auto kink = [&](double v) { B.kink_penalty = std::min(B.kink_penalty, std::min(std::fabs(v), std::fabs(v - relu_mu))); };
    for (int i = 0; i < dof; i++) B.kink_sigmoid = std::min(B.kink_sigmoid, std::fabs(Vq[i + 3]));
    for (size_t cidx = 0; cidx < colli_pts.size(); cidx++) {   // 73-88
      const double pc[3] = {colli_pts[cidx].p.x, colli_pts[cidx].p.y, colli_pts[cidx].p.z};
      double sdf_value, grad_pc[3];
      grid_map->getDisWithGradI3d(pc, sdf_value, grad_pc);
      bool inside = true;
      for (int a = 0; a < 3; a++) {
        if (pc[a] < grid_map->min_b[a] + 1e-4 || pc[a] > grid_map->max_b[a] - 1e-4) inside = false;
      }
      if (!inside) B.n_outside++;
      for (int a = 0; a < 3; a++) {
        B.kink_cell = std::min(B.kink_cell, std::min(std::fabs(pc[a] - (grid_map->min_b[a] + 1e-4)), std::fabs(pc[a] - (grid_map->max_b[a] - 1e-4))));
        if (inside) {
          const double u = (pc[a] - 0.5 * grid_map->res - grid_map->origin[a]) * grid_map->res_inv;
          B.kink_cell = std::min(B.kink_cell, std::fabs(u - std::round(u)) * grid_map->res);
        }
      }
      const double violaPos = colli_pts[cidx].r * w.cost_scale * w.clearance - sdf_value * w.cost_scale;
      kink(violaPos);
      V3 grad_to_pos;
      if (violaPos > 0) {
        double pena, penaD;
        smoothL1Penalty(relu_mu, violaPos, pena, penaD);
        const double s = -w.mani_colli_weight * penaD;
        grad_to_pos = V3{s * grad_pc[0] * w.cost_scale, s * grad_pc[1] * w.cost_scale, s * grad_pc[2] * w.cost_scale};
        sdf_cost += w.mani_colli_weight * pena;
        B.mani += w.mani_colli_weight * pena;
        B.n_mani++;
      }
      pos_grads.push_back(grad_to_pos);
    }
    for (size_t cidx = 0; cidx < colli_pts.size(); cidx++) {   // 90-131
      if (cidx > 2) {
        const double height = moma_param.chassis_height + moma_param.relative_t.z + colli_pts[cidx].r - colli_pts[cidx].p.z;
        kink(height);
        if (height > 0) {
          double pena, penaD;
          smoothL1Penalty(relu_mu, height, pena, penaD);
          sdf_cost += w.self_colli_weight * pena;
          pos_grads[cidx].z += -w.self_colli_weight * penaD;
          B.chassis += w.self_colli_weight * pena;
          B.n_chassis++;
        }
      }
      for (size_t cj = cidx + 1; cj < colli_pts.size(); cj++) {
        if (moma_param.collision_matrix[cidx][cj] != -1) continue;
        const V3 diff = colli_pts[cidx].p - colli_pts[cj].p;
        const double rr = colli_pts[cidx].r + colli_pts[cj].r;
        const double dist = rr * rr - dot(diff, diff);
        kink(dist);
        if (dist > 0) {
          double pena, penaD;
          smoothL1Penalty(relu_mu, dist, pena, penaD);
          const V3 grad1 = diff * (-w.self_colli_weight * penaD * 2.0);
          sdf_cost += w.self_colli_weight * pena;
          pos_grads[cidx] = pos_grads[cidx] + grad1;
          pos_grads[cj] = pos_grads[cj] - grad1;
          B.pairs += w.self_colli_weight * pena;
          B.n_pairs++;
        }
      }
    }
    double colli_grads[10];
    moma_param.getColliGrads(now_pos, pos_grads, colli_grads);
    for (int i = 0; i < 10; i++) moma_grad[i] += colli_grads[i];
    for (int i = 0; i < 3; i++) gradVq[i] = moma_grad[i];   // assigned: the documented deviation from 135-137
    for (int j = 0; j < dof; j++) gradVq[j + 3] = moma_grad[j + 3] * T::getQtoVqGrad(Vq[j + 3], moma_param.joint_pos_limit_max[j]);
    if (bd) *bd = B;
    return ee_cost + sdf_cost;
  }

  // optimizeEE.  Returns the L-BFGS code; moma_pos is rewritten for the reference's success codes only.
  int optimize(double* moma_pos, const topay_oracle::LbfgsParam& lbfgs_param, double* cost_out, int* iters, int* evals) const {
    using T = topay_oracle::TrajOpt;
    std::vector<double> x(10);
    for (int i = 0; i < 3; i++) x[i] = moma_pos[i];
    for (int i = 0; i < Robot::dof; i++) x[i + 3] = T::invSigmoidC2(moma_pos[i + 3], moma_param.joint_pos_limit_max[i]);
    double c = 0.0;
    topay_oracle::LbfgsStats st;
    const int result = topay_oracle::lbfgs_optimize(
        x, c, [&](const std::vector<double>& xx, std::vector<double>& gg) { return cost(xx.data(), gg.data()); }, nullptr, lbfgs_param, &st);
    if (result == topay_oracle::LBFGS_CONVERGENCE || result == topay_oracle::LBFGS_CANCELED || result == topay_oracle::LBFGS_STOP ||
        result == topay_oracle::LBFGSERR_MAXIMUMITERATION) {
      for (int i = 0; i < 3; i++) moma_pos[i] = x[i];
      for (int i = 0; i < Robot::dof; i++) moma_pos[i + 3] = T::sigmoidC2(x[i + 3], moma_param.joint_pos_limit_max[i]);
    }
    *cost_out = c; *iters = st.iterations; *evals = st.evaluations;
    return result;
  }
};

}  // namespace ee_goal
