// Host side of the C-ABI, part 10: end-effector goals (topay_ee.h; MomaTrajOpt::optimizeEE, MomaParam::getFKPose).

#pragma once

static topay::EeWeights ee_weights(const topay_ee_params_t& p) {
  topay::EeWeights w;
  w.cost_scale = p.cost_scale; w.mani_colli_weight = p.mani_colli_weight; w.self_colli_weight = p.self_colli_weight; w.clearance = p.clearance_factor;
  return w;
}

static topay_status ee_params_ok(const topay_ee_params_t& p) {
  const topay_lbfgs_params_t& l = p.lbfgs;
  if (l.mem_size < 1 || l.mem_size > topay::kEeMaxMem) { set_err("topay_ee: lbfgs.mem_size must be in 1..64"); return TOPAY_ERR_INVALID_ARG; }
  if (l.past < 0 || l.past > topay::kEeMaxPast) { set_err("topay_ee: lbfgs.past must be in 0..8"); return TOPAY_ERR_INVALID_ARG; }
  // lbfgs.hpp:452-495: what lbfgs_optimize refuses
  if (l.g_epsilon < 0.0 || l.delta < 0.0 || l.min_step < 0.0 || l.max_step < l.min_step || !(l.f_dec_coeff > 0.0 && l.f_dec_coeff < 1.0) ||
      !(l.s_curv_coeff < 1.0 && l.s_curv_coeff > l.f_dec_coeff) || !(l.machine_prec > 0.0) || l.max_linesearch <= 0 || l.max_iterations < 0) {
    set_err("topay_ee: an lbfgs parameter is outside what lbfgs_optimize accepts");
    return TOPAY_ERR_INVALID_ARG;
  }
  if (!(p.cost_scale > 0.0) || !(p.mani_colli_weight >= 0.0) || !(p.self_colli_weight >= 0.0) || !(p.clearance_factor > 0.0) || !(p.pose_tol >= 0.0)) {
    set_err("topay_ee: weights must not be negative, cost_scale and clearance_factor positive");
    return TOPAY_ERR_INVALID_ARG;
  }
  return TOPAY_OK;
}

extern "C" {

void topay_ee_default_params(topay_ee_params_t* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  // moma_traj_opt.cpp:16-21 over lbfgs_parameter_t's defaults (lbfgs.hpp:15-129)
  p->lbfgs.mem_size = 64; p->lbfgs.past = 3; p->lbfgs.g_epsilon = 1.0e-5; p->lbfgs.delta = 1.0e-4; p->lbfgs.max_iterations = 10000;
  p->lbfgs.max_linesearch = 64; p->lbfgs.min_step = 1.0e-20; p->lbfgs.max_step = 1.0e+20; p->lbfgs.f_dec_coeff = 1.0e-4;
  p->lbfgs.s_curv_coeff = 0.9; p->lbfgs.cautious_factor = 1.0e-6; p->lbfgs.machine_prec = 1.0e-16;
  p->cost_scale = 10.0; p->mani_colli_weight = 100.0; p->self_colli_weight = 100.0; p->clearance_factor = 1.1;   // 68-70, 78
  p->pose_tol = 1.0e-2;
  p->require_collision_free = 1;
}

topay_status topay_ee_pose(topay_ctx* c, int n, const double* states, double* pose) {
  if (!c || n < 0 || (n > 0 && (!states || !pose))) return TOPAY_ERR_INVALID_ARG;
  if (n == 0) return TOPAY_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t N = (size_t)n;
  double *d_st, *d_po;
  topay_status s;
  if ((s = c->ee.io.carve([&](Carver& k) { d_st = k.take<double>(10 * N); d_po = k.take<double>(9 * N); })) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_st, states, 10 * N));
  if ((s = push_params(c)) != TOPAY_OK) return s;
  hipLaunchKernelGGL(topay::k_ee_pose, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, n, (const double*)d_st, d_po);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(c, pose, d_po, 9 * N));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

topay_status topay_ee_eval(topay_ctx* c, int n, const int* map_ids, const double* x, const double* ee_ref, double* f, double* g) {
  if (!c || n <= 0 || !x || !ee_ref || !f || !g) return TOPAY_ERR_INVALID_ARG;
  topay_status s;
  if ((s = check_map_slots(c, n, map_ids, kMapResident | kMap3d, "topay_ee_eval")) != TOPAY_OK) return s;
  HIPCHK(hipSetDevice(c->device));
  topay_ee_params_t prm;
  topay_ee_default_params(&prm);
  const size_t N = (size_t)n;
  double *d_x, *d_ref, *d_f, *d_g; int* d_mid;
  auto lay = [&](Carver& k) { d_x = k.take<double>(10 * N); d_ref = k.take<double>(9 * N); d_f = k.take<double>(N); d_g = k.take<double>(10 * N); d_mid = k.take<int>(N); };
  if ((s = c->ee.io.carve(lay)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_x, x, 10 * N));
  HIPCHK(h2d(c, d_ref, ee_ref, 9 * N));
  if (map_ids) HIPCHK(h2d(c, d_mid, map_ids, N));
  if ((s = push_params(c)) != TOPAY_OK) return s;
  hipLaunchKernelGGL(topay::k_ee_eval, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, n, (const DevMap*)c->dmaps.p,
                     (const int*)(map_ids ? d_mid : nullptr), ee_weights(prm), (const double*)d_x, (const double*)d_ref, d_f, d_g);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(c, f, d_f, N));
  HIPCHK(d2h(c, g, d_g, 10 * N));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

topay_status topay_ee_goals(topay_ctx* c, int n, const int* map_ids, const double* seed_states, const double* ee_ref, const topay_ee_params_t* params,
                            double* states, double* cost, int* code, int* iters, int* evals) {
  if (!c || n <= 0 || !seed_states || !ee_ref || !states) return TOPAY_ERR_INVALID_ARG;
  topay_ee_params_t prm;
  if (params) prm = *params; else topay_ee_default_params(&prm);
  topay_status s;
  if ((s = ee_params_ok(prm)) != TOPAY_OK) return s;
  if ((s = check_map_slots(c, n, map_ids, kMapResident | kMap3d, "topay_ee_goals")) != TOPAY_OK) return s;
  for (int k = 0; k < n; k++)
    for (int q = 0; q < 7; q++) {
      const double v = seed_states[10 * (size_t)k + 3 + q];
      if (!(std::fabs(v) < c->hp.joint_pos_limit_max[q])) {   // (a NaN too) invSigmoidC2 has no image there
        set_err("topay_ee_goals: seed " + std::to_string(k) + ", joint " + std::to_string(q + 1) + " is at or beyond its limit");
        return TOPAY_ERR_INVALID_ARG;
      }
    }
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  const size_t N = (size_t)n, waves = (N + 63) / 64;
  // the history of this call, sized from n and mem_size, kept until the next call
  if ((s = c->ee.hist.ensure(waves * (size_t)prm.lbfgs.mem_size * topay::kEeHistRows * 64 * sizeof(double))) != TOPAY_OK) return s;
  double *d_seed, *d_ref, *d_st, *d_cost; int *d_mid, *d_code, *d_it, *d_ev;
  auto lay = [&](Carver& k) {
    d_seed = k.take<double>(10 * N); d_ref = k.take<double>(9 * N); d_st = k.take<double>(10 * N); d_cost = k.take<double>(N);
    d_mid = k.take<int>(N); d_code = k.take<int>(N); d_it = k.take<int>(N); d_ev = k.take<int>(N);
  };
  if ((s = c->ee.io.carve(lay)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_seed, seed_states, 10 * N));
  HIPCHK(h2d(c, d_ref, ee_ref, 9 * N));
  if (map_ids) HIPCHK(h2d(c, d_mid, map_ids, N));
  if ((s = push_params(c)) != TOPAY_OK) return s;
  topay::EeGoalArgs A;
  A.n = n; A.map_ids = map_ids ? d_mid : nullptr; A.seed = d_seed; A.ee_ref = d_ref; A.W = ee_weights(prm);
  A.L = to_dev_lbfgs(prm.lbfgs);
  A.hist = c->ee.hist.as<double>(); A.states = d_st; A.cost = d_cost; A.code = d_code; A.iters = d_it; A.evals = d_ev;
  HIPCHK(c->ee.timer.start(c->stream));
  hipLaunchKernelGGL(topay::k_ee_goals, dim3((unsigned)waves), dim3(64), 0, c->stream, A, (const DevMap*)c->dmaps.p);
  HIPCHK(hipGetLastError());
  HIPCHK(c->ee.timer.stop(c->stream));
  HIPCHK(d2h(c, states, d_st, 10 * N));
  if (cost) HIPCHK(d2h(c, cost, d_cost, N));
  if (code) HIPCHK(d2h(c, code, d_code, N));
  if (iters) HIPCHK(d2h(c, iters, d_it, N));
  if (evals) HIPCHK(d2h(c, evals, d_ev, N));
  HIPCHK(hipStreamSynchronize(c->stream));
  (void)c->ee.timer.read(&c->ee.ms);
  return TOPAY_OK;
}

topay_status topay_ee_ms(topay_ctx* c, double* ms) {
  if (!c || !ms) return TOPAY_ERR_INVALID_ARG;
  *ms = c->ee.ms;
  return TOPAY_OK;
}

topay_status topay_ee_select(topay_ctx* c, int n, const int* map_ids, const int* group_of, int n_groups, const double* states, const double* cost,
                             const int* code, const double* ee_ref, const topay_ee_params_t* params, int* winner, double* goal) {
  if (!c || n <= 0 || n_groups <= 0 || !group_of || !states || !cost || !code || !ee_ref || !winner || !goal) return TOPAY_ERR_INVALID_ARG;
  topay_ee_params_t prm;
  if (params) prm = *params; else topay_ee_default_params(&prm);
  topay_status s;
  if ((s = ee_params_ok(prm)) != TOPAY_OK) return s;
  const bool cf = prm.require_collision_free != 0;
  if (cf && (s = check_map_slots(c, n, map_ids, kMapResident | kMap2d | kMap3d, "topay_ee_select")) != TOPAY_OK) return s;
  HIPCHK(hipSetDevice(c->device));
  const size_t N = (size_t)n, G = (size_t)n_groups;
  double *d_st, *d_cost, *d_ref, *d_goal; int *d_mid, *d_grp, *d_code, *d_q, *d_win;
  auto lay = [&](Carver& k) {
    d_st = k.take<double>(10 * N); d_cost = k.take<double>(N); d_ref = k.take<double>(9 * N); d_goal = k.take<double>(10 * G);
    d_mid = k.take<int>(N); d_grp = k.take<int>(N); d_code = k.take<int>(N); d_q = k.take<int>(N); d_win = k.take<int>(G);
  };
  if ((s = c->ee.io.carve(lay)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_st, states, 10 * N));
  HIPCHK(h2d(c, d_cost, cost, N));
  HIPCHK(h2d(c, d_ref, ee_ref, 9 * N));
  HIPCHK(h2d(c, d_goal, goal, 10 * G));   // (a group without a winner keeps what the caller had)
  HIPCHK(h2d(c, d_grp, group_of, N));
  HIPCHK(h2d(c, d_code, code, N));
  if (map_ids) HIPCHK(h2d(c, d_mid, map_ids, N));
  if ((s = push_params(c)) != TOPAY_OK) return s;
  hipLaunchKernelGGL(topay::k_ee_qualify, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, n, (const DevMap*)c->dmaps.p,
                     (const int*)(map_ids ? d_mid : nullptr), (const double*)d_st, (const int*)d_code, (const double*)d_ref, prm.pose_tol, cf ? 1 : 0, d_q);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(topay::k_ee_select, dim3((unsigned)((n_groups + 63) / 64)), dim3(64), 0, c->stream, n, n_groups, (const int*)d_grp, (const int*)d_q,
                     (const double*)d_cost, (const double*)d_st, d_win, d_goal);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(c, winner, d_win, G));
  HIPCHK(d2h(c, goal, d_goal, 10 * G));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

}  // extern "C"
