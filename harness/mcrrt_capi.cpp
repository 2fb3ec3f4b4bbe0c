// C entry points of the MCRRT / Reeds-Shepp restatement (harness/mcrrt.hpp) for the Python tests.  A library of its own,
// built with -ffp-contract=off: the search compares costs computed with a*b+c expressions, and a fused multiply-add
// on the host would differ from the device (built with contraction off) in the last bit.
#include "mcrrt.hpp"
#include "jps.hpp"
#include "topo_prm.hpp"
#include "replan.hpp"
#include "ee_goal.hpp"
#include "prob_map.hpp"

using namespace topay_wl;

extern "C" {

// One planning instance on `world` (a World* of libtopay_workload.so: same header, same layout).  car_path: L x (x, y,
// theta, dt) as getDensePath returns it.  wb: up to L x 10.  stats[8]: status (1 path, 0 none, -1 node pool full), nodes,
// iterations, tree count, anti-tree count, index of path_node_1, of path_node_2, whole-body checks.  nodes: up to
// nodes_cap rows in creation order (may be null).
int wl_mcrrt_plan(void* world, const double* start, const double* end, int L, const double* car_path, const McrrtParams* prm,
                  unsigned long long inst, int track_slack, double* wb, int* wb_len, int* stats, double* cmax, double* min_slack,
                  int nodes_cap, McrrtNodeRec* nodes) {
  const World& w = *(const World*)world;
  MCRRTs m(w, *prm, inst);
  m.track_slack = track_slack != 0;
  std::vector<std::array<double, 4>> path(L);
  for (int i = 0; i < L; i++) for (int a = 0; a < 4; a++) path[i][a] = car_path[4 * i + a];
  std::vector<std::array<double, 10>> out;
  const int st = m.plan(start, end, path, out);
  *wb_len = (int)out.size();
  for (size_t i = 0; i < out.size(); i++) std::memcpy(wb + 10 * i, out[i].data(), 10 * sizeof(double));
  stats[0] = st;
  stats[1] = (int)m.by_index.size();
  stats[2] = m.iterations;
  stats[3] = m.tree_count_;
  stats[4] = m.anti_tree_count_;
  stats[5] = m.path_node_1 ? m.path_node_1->index : -1;
  stats[6] = m.path_node_2 ? m.path_node_2->index : -1;
  stats[7] = (int)(m.n_checks & 0x7fffffff);
  *cmax = m.c_max;
  *min_slack = m.min_slack;
  if (nodes)
    for (int i = 0; i < (int)m.by_index.size() && i < nodes_cap; i++) {
      const MCRRTs::Node* n = m.by_index[i];
      nodes[i].layer = n->layer;
      nodes[i].state = (int)n->node_state;
      nodes[i].parent = n->parent ? n->parent->index : -1;
      nodes[i].cost = n->cost;
      std::memcpy(nodes[i].q, n->q, sizeof(n->q));
    }
  return st;
}

// ReedsSheppStateSpace(rho): the shortest path's word (0..17), its five signed segment lengths (units of rho) and
// distance(); interpolate(from, to, t).
double wl_rs_path(double rho, const double* from, const double* to, int* type, double* lengths) {
  ReedsShepp rs(rho);
  ReedsShepp::Path p = rs.reedsShepp(from, to);
  *type = p.type;
  for (int i = 0; i < 5; i++) lengths[i] = p.length[i];
  return rho * p.total;
}
void wl_rs_interpolate(double rho, const double* from, const double* to, double t, double* out) { ReedsShepp(rho).interpolate(from, to, t, out); }

// GraphSearch::plan2dJPS on `world`'s 2-D distance field: returns the number of path points (0 = no path), writes at most
// cap of them; stats[0] = expanded nodes, stats[1] = jump points of the raw path (before the zigzag cut).
int wl_plan2d_jps(void* world, const double* start, const double* end, double threshold, int cap, double* out_xy, int* stats) {
  const World& w = *(const World*)world;
  GraphSearch gs(w.gm, threshold);
  auto path = gs.plan2dJPS(start, end, threshold);
  stats[0] = gs.expand_iteration;
  stats[1] = (int)gs.path_.size();
  for (size_t i = 0; i < path.size() && (int)i < cap; i++) { out_xy[2 * i] = path[i][0]; out_xy[2 * i + 1] = path[i][1]; }
  return (int)path.size();
}

double wl_mcrrt_u01(unsigned long long seed, unsigned long long inst, unsigned long long iter, unsigned long long slot) {
  return mcrrt_u01(seed, inst, iter, slot);
}

// TopologyPRM::findTopoPaths restated (harness/topo_prm.hpp) on `world` with the two front-end fields given by the caller
// (wl_edt_front_end_fields).  Returns a handle that keeps every intermediate result; stats[8] as topay_topo_paths,
// counters[2] = connector moves (topo_prm.cpp:254), collision-point pushes (543-549).
void* wl_topo_run(void* world, const double* inflate, const double* critical, const double* start_xy, const double* end_xy,
                  const TopoParams* prm, unsigned long long inst, int use_critical, int track_slack, int* stats, int* counters,
                  double* min_slack) {
  const World& w = *(const World*)world;
  TopologyPRM* t = new TopologyPRM(w.gm, inflate, critical, *prm, inst);
  t->track_slack = track_slack != 0;
  const int st = t->findTopoPaths({start_xy[0], start_xy[1], 0.0}, {end_xy[0], end_xy[1], 0.0}, use_critical != 0);
  for (int i = 0; i < 8; i++) stats[i] = 0;
  stats[0] = st;
  if (st >= 0) {
    stats[1] = t->samples_drawn; stats[2] = t->samples_passed; stats[3] = t->nodes_before; stats[4] = t->nodes_after;
    stats[5] = t->raw_found; stats[6] = t->n_filtered; stats[7] = (int)t->select_paths.size();
  }
  counters[0] = t->n_moves; counters[1] = t->n_pushes;
  *min_slack = t->min_slack;
  return t;
}
void wl_topo_free(void* h) { delete (TopologyPRM*)h; }
int wl_topo_graph_size(void* h) { return (int)((TopologyPRM*)h)->graph_.size(); }
// graph in list order: id, type, position, neighbour ids (WL_TOPO_MAX_NB per node)
void wl_topo_graph(void* h, int* id, int* type, double* pos_xy, int* n_nb, int* nb) {
  int k = 0;
  for (auto& n : ((TopologyPRM*)h)->graph_) {
    id[k] = n->id_; type[k] = n->type_; pos_xy[2 * k] = n->pos_[0]; pos_xy[2 * k + 1] = n->pos_[1];
    n_nb[k] = (int)n->neighbors_.size();
    for (int j = 0; j < n_nb[k] && j < WL_TOPO_MAX_NB; j++) nb[k * WL_TOPO_MAX_NB + j] = n->neighbors_[j]->id_;
    k++;
  }
}
// which: 0 raw paths kept by searchPaths, 1 their shortcut versions, 2 the selected paths.  lens == NULL: returns the
// number of paths; else fills lens and, when xy != NULL, the points back to back.
int wl_topo_get_paths(void* h, int which, int* lens, double* xy) {
  TopologyPRM* t = (TopologyPRM*)h;
  const std::vector<TopologyPRM::Path>& ps = which == 0 ? t->raw_paths_ : (which == 1 ? t->short_paths_first_ : t->select_paths);
  if (!lens) return (int)ps.size();
  size_t o = 0;
  for (size_t i = 0; i < ps.size(); i++) {
    lens[i] = (int)ps[i].size();
    if (xy) for (auto& p : ps[i]) { xy[o++] = p[0]; xy[o++] = p[1]; }
  }
  return (int)ps.size();
}
// the cells lineVisib tests for the ray p1 -> p2 (before boundIndex2d): returns their number, writes at most cap
int wl_topo_ray_cells(void* world, const double* inflate, const double* p1, const double* p2, int cap, int* cells) {
  const World& w = *(const World*)world;
  TopoParams prm{};
  TopologyPRM t(w.gm, inflate, inflate, prm, 0);
  t.record_cells = true;
  V3 pc;
  t.lineVisib({p1[0], p1[1], 0.0}, {p2[0], p2[1], 0.0}, -1.0e300, pc);
  for (size_t i = 0; i < t.visited_cells.size() && (int)i < cap; i++) { cells[2 * i] = t.visited_cells[i][0]; cells[2 * i + 1] = t.visited_cells[i][1]; }
  return (int)t.visited_cells.size();
}
// samples createGraph draws in `seconds` of accumulated loop time (the reference's max_sample_time rule, for the budget measurement)
int wl_topo_samples_in(void* world, const double* inflate, const double* critical, const double* start_xy, const double* end_xy,
                       const TopoParams* prm, unsigned long long inst, double seconds) {
  const World& w = *(const World*)world;
  // doubling search on the count: the loop body is deterministic, so the time of the first k samples is measured directly
  int lo = 64;
  for (;;) {
    TopoParams q = *prm;
    q.max_sample_num = lo;
    TopologyPRM t(w.gm, inflate, critical, q, inst);
    const auto t0 = std::chrono::steady_clock::now();
    try { t.use_critical = false; t.createGraph({start_xy[0], start_xy[1], 0.0}, {end_xy[0], end_xy[1], 0.0}); } catch (const TopoAbort&) { return lo; }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (dt >= seconds || lo >= (1 << 20)) return (int)((double)lo * std::min(1.0, seconds / dt));
    lo *= 2;
  }
}
}

extern "C" {

// ---- the replanning cycle's restatement (harness/replan.hpp) ----------------------------------------------------------
// A MomaTraj from setTraj's arguments: start (x, y, theta), durations [n], coefficients [n][9][6], highest order first.
void* wl_replan_traj_create(const double* start3, int n, const double* durations, const double* coeffs) {
  ReplanTraj* t = new ReplanTraj();
  for (int a = 0; a < 3; a++) t->start_state[a] = start3[a];
  t->T.assign(durations, durations + n);
  t->C.assign(coeffs, coeffs + (size_t)n * 54);
  t->init();
  return t;
}
void wl_replan_traj_destroy(void* h) { delete (ReplanTraj*)h; }
int wl_replan_car_seq_len(void* h) { return (int)((ReplanTraj*)h)->car_seq.size(); }
void wl_replan_state(void* h, double t, double* state10, double* dstate10) {
  ((ReplanTraj*)h)->getState(t, state10);
  ((ReplanTraj*)h)->getDState(t, dstate10);
}
// safeCallback against the given fields.  first_hit[2] = sample, body; hit[2] = time, distance; returns is_safe.
int wl_replan_safe(void* h, const double* origin, double res, const int* dims, const double* min_b, const double* max_b, const double* esdf2d,
                   const double* esdf3d, int* first_hit, double* hit, double* min_margin) {
  topay_oracle::Map m;
  m.set(origin, res, dims, esdf2d, esdf3d);
  m.setBounds(min_b, max_b);
  const topay_oracle::Robot robot;
  const ReplanSafe r = replan_safe(*(ReplanTraj*)h, m, robot);
  first_hit[0] = r.sample; first_hit[1] = r.body;
  hit[0] = r.t; hit[1] = r.d;
  *min_margin = r.min_margin;
  return r.is_safe ? 1 : 0;
}
int wl_replan_endpoints(void* end_traj, void* global_traj, double since_last_replan, double since_begin, const double* global_goal,
                        double planning_budget, double planning_horizon, double* start, double* start_v, double* goal) {
  return replan_endpoints(*(ReplanTraj*)end_traj, (const ReplanTraj*)global_traj, since_last_replan, since_begin, global_goal, planning_budget,
                          planning_horizon, start, start_v, goal);
}

// ---- end-effector goals' restatement (harness/ee_goal.hpp) ------------------------------------------------------------
void wl_ee_pose(int n, const double* states, double* pose) {
  const topay_oracle::Robot robot;
  for (int k = 0; k < n; k++) ee_goal::getFKPose(robot, states + 10 * (size_t)k, pose + 9 * (size_t)k);
}
static void ee_problem(ee_goal::Problem& p, topay_oracle::Map& m, const double* origin, double res, const int* dims, const double* min_b,
                       const double* max_b, const double* esdf2d, const double* esdf3d, const double* ee_ref) {
  m.set(origin, res, dims, esdf2d, esdf3d);
  m.setBounds(min_b, max_b);
  p.grid_map = &m;
  p.relu_mu = topay_oracle::Params().relu_mu;
  for (int a = 0; a < 9; a++) p.ee_pose[a] = ee_ref[a];
}
// eeCostCallback at the unconstrained x.  terms[4] = ee, environment, chassis top, pairs; counts[4] = active terms of the
// last three kinds, spheres outside the map; kinks[3] = Breakdown's kink distances.  Returns f.
double wl_ee_eval(const double* origin, double res, const int* dims, const double* min_b, const double* max_b, const double* esdf2d,
                  const double* esdf3d, const double* x, const double* ee_ref, double* g, double* terms, int* counts, double* kinks) {
  topay_oracle::Map m;
  ee_goal::Problem p;
  ee_problem(p, m, origin, res, dims, min_b, max_b, esdf2d, esdf3d, ee_ref);
  ee_goal::Breakdown b;
  const double f = p.cost(x, g, &b);
  if (terms) { terms[0] = b.ee; terms[1] = b.mani; terms[2] = b.chassis; terms[3] = b.pairs; }
  if (counts) { counts[0] = b.n_mani; counts[1] = b.n_chassis; counts[2] = b.n_pairs; counts[3] = b.n_outside; }
  if (kinks) { kinks[0] = b.kink_penalty; kinks[1] = b.kink_cell; kinks[2] = b.kink_sigmoid; }
  return f;
}
// optimizeEE of one problem; state10 in / out.  lbfgs[4] = mem_size, past, max_iterations, max_linesearch; g_epsilon, delta as given,
// the other fields lbfgs_parameter_t's defaults.  out_int[2] = iterations, evaluations.  Returns the L-BFGS code.
int wl_ee_optimize(const double* origin, double res, const int* dims, const double* min_b, const double* max_b, const double* esdf2d,
                   const double* esdf3d, double* state10, const double* ee_ref, const int* lbfgs, double g_epsilon, double delta, double* cost,
                   int* out_int) {
  topay_oracle::Map m;
  ee_goal::Problem p;
  ee_problem(p, m, origin, res, dims, min_b, max_b, esdf2d, esdf3d, ee_ref);
  topay_oracle::LbfgsParam lp;
  lp.mem_size = lbfgs[0]; lp.past = lbfgs[1]; lp.max_iterations = lbfgs[2]; lp.max_linesearch = lbfgs[3];
  lp.g_epsilon = g_epsilon; lp.delta = delta;
  return p.optimize(state10, lp, cost, out_int, out_int + 1);
}

// ---- sensor clouds' restatement (harness/prob_map.hpp) ----------------------------------------------------------------
void* wl_pm_create(const double* origin, double res, const int* dims) {
  prob_map::ProbMap* m = new prob_map::ProbMap();
  m->reset(origin, res, dims);
  return m;
}
void wl_pm_destroy(void* h) { delete (prob_map::ProbMap*)h; }
// updateProbMap of one cloud (n points of x, y, z, intensity); returns 1 flushed, 0 batch open, -1 / -2 sensor above the ceiling / below the ground
int wl_pm_update(void* h, int n, const float* xyzi, const double* sensor3, const prob_map::Params* params) {
  return ((prob_map::ProbMap*)h)->update(xyzi, n, sensor3, *params);
}
void wl_pm_get(void* h, float* logodds, int* op_cnt, int* hit_cnt, int* batch_counter) {
  const prob_map::ProbMap& m = *(prob_map::ProbMap*)h;
  if (logodds) m.unring(m.occupancy_buffer, logodds);
  if (op_cnt) m.unring(m.operation_cnt, op_cnt);
  if (hit_cnt) m.unring(m.hit_cnt, hit_cnt);
  if (batch_counter) *batch_counter = m.batch_update_counter;
}
// the slide of one sensor position (ProbMap::slide); shift3 receives the voxels the window moved by, origin3 the grid's origin after it
int wl_pm_slide(void* h, const double* sensor3, double threshold, int slide_z, int* shift3, double* origin3) {
  prob_map::ProbMap& m = *(prob_map::ProbMap*)h;
  const int st = m.slide(sensor3, threshold, slide_z != 0, shift3);
  for (int a = 0; a < 3; a++) origin3[a] = m.origin[a];
  return st;
}
void wl_pm_occupancy(void* h, const prob_map::Params* params, int8_t* occ2d, int8_t* occ2d_critical, int8_t* occ3d) {
  ((prob_map::ProbMap*)h)->occupancy(prob_map::logit(params->p_occ), params->chassis_height, occ2d, occ2d_critical, occ3d);
}
void wl_pm_logodds(const prob_map::Params* p, float* l6) {
  l6[0] = prob_map::logit(p->p_hit); l6[1] = prob_map::logit(p->p_miss); l6[2] = prob_map::logit(p->p_min);
  l6[3] = prob_map::logit(p->p_max); l6[4] = prob_map::logit(p->p_occ); l6[5] = prob_map::logit(p->p_free);
}
void wl_pm_scan(const int8_t* occ3d, const double* origin, double res, const int* dims, const double* pose4, int n_az, int n_el, double fov,
                double range, float* out) {
  prob_map::scan(occ3d, origin, res, dims, pose4, n_az, n_el, fov, range, out);
}

}  // extern "C"

#include "ompc.hpp"

extern "C" {

// ---- the tracking controller's and the fake robot's restatement (harness/ompc.hpp) -------------------------------------
void* wl_ompc_create(const ompc::Params* p) { return new ompc::OMPC(*p); }
void wl_ompc_destroy(void* h) { delete (ompc::OMPC*)h; }
void wl_ompc_set_direct(void* h, int on, const double* pos3) {
  ompc::OMPC* m = (ompc::OMPC*)h;
  m->control_state = on ? 1 : 0;
  for (int a = 0; a < 3; a++) m->direct_pos[a] = on ? pos3[a] : 0.0;
}
// getCmd; rows [T][3], arm_q / arm_dq [7] from the caller's trajectory; xopt [(T + 1)][3] may be null
void wl_ompc_cmd(void* h, int has_traj, double t_cur, double T_total, const double* now10, const double* rows, const double* arm_q, const double* arm_dq,
                 double* cmd16, int* status4, double* xopt) {
  ((ompc::OMPC*)h)->getCmd(has_traj != 0, t_cur, T_total, now10, rows, arm_q, arm_dq, cmd16, status4, xopt);
}
// output [2][T], output_buff [maxd][2]
void wl_ompc_get(void* h, double* output, double* fifo) {
  const ompc::OMPC& m = *(ompc::OMPC*)h;
  if (output) memcpy(output, m.output.data(), m.output.size() * sizeof(double));
  if (fifo) memcpy(fifo, m.output_buff.data(), m.output_buff.size() * sizeof(double));
}
// The first QP of getCmd, the controller's state untouched: solveMPCDiff's matrices as the reference fills them, and the
// solution of the stage-order solver in that order.  info[2] = steps, solved.  Returns 0 when getCmd does not reach the QP.
int wl_ompc_probe(void* h, int has_traj, double t_cur, double T_total, const double* now10, const double* rows, double* P, double* q, double* A,
                  double* l, double* u, double* x, double* y, double* z, int* info) {
  ompc::OMPC* m = (ompc::OMPC*)h;
  ompc::Dense D;
  double cmd[16], arm[7] = {0, 0, 0, 0, 0, 0, 0};
  int st[4];
  m->getCmd(has_traj != 0, t_cur, T_total, now10, rows, arm, arm, cmd, st, nullptr, &D);
  if (D.nx == 0) return 0;
  memcpy(P, D.P.data(), D.P.size() * 8); memcpy(q, D.q.data(), D.q.size() * 8); memcpy(A, D.A.data(), D.A.size() * 8);
  memcpy(l, D.l.data(), D.l.size() * 8); memcpy(u, D.u.data(), D.u.size() * 8);
  memcpy(x, D.x.data(), D.x.size() * 8); memcpy(y, D.y.data(), D.y.size() * 8); memcpy(z, D.z.data(), D.z.size() * 8);
  info[0] = D.iters; info[1] = D.solved;
  return 1;
}
void* wl_sim_create(const double* state10, int delay_cmds) { return new ompc::Sim(state10, delay_cmds); }
void wl_sim_destroy(void* h) { delete (ompc::Sim*)h; }
void wl_sim_step(void* h, const double* cmd16, int ticks, double* state10) {
  ompc::Sim* s = (ompc::Sim*)h;
  s->step(cmd16, ticks);
  for (int a = 0; a < 10; a++) state10[a] = s->st[a];
}

}  // extern "C"
