// Host side of the C-ABI, part 5: the front-end stages -- whole-body collision, dense paths, edge checks, JPS, the
// topological roadmap, the joint-space search, Reeds-Shepp.

#pragma once

// getDensePath for n_paths raw paths that are on the device, results left there (the public entry and topay_plan_calls).
static topay_status dense_launch(topay_ctx* c, int n_paths, const double* d_raw, const long long* d_off, const int* d_len, double step_size,
                                 const double* d_syaw, const double* d_eyaw, double v_max, double w_max, int cap_per_path, double* d_out, int* d_olen) {
  hipLaunchKernelGGL(k_dense_path, dim3((n_paths + 63) / 64), dim3(64), 0, c->stream, n_paths, d_raw, d_off, d_len, step_size, d_syaw, d_eyaw, v_max,
                     w_max, cap_per_path, d_out, d_olen);
  HIPCHK(hipGetLastError());
  return TOPAY_OK;
}

// Device results of a stage launcher: where the launch left them (valid until the buffers are sized again).
struct JpsDev { int* len; double* out; int* stats; };

// plan2dJPS for n host-side (start, goal) pairs; the results stay on the device in `io` (the public entry copies them
// back, topay_plan_calls hands them on).  out_ext: write the paths there (n x cap_points x 2) instead of into `io`.  tm (optional):
// started and stopped around the kernels alone.
static topay_status jps_impl(topay_ctx* c, int n, const int* map_ids, const double* start_xy, const double* end_xy, double threshold, int cap_points,
                             DevBuf& io, double* out_ext, JpsDev* dev, const char* who, DevTimer* tm = nullptr) {
  if (topay_status cs = check_map_slots(c, n, map_ids, kMapResident, who)) return cs;
  std::vector<int> mid((size_t)n, 0);
  if (map_ids) mid.assign(map_ids, map_ids + n);
  long long ncell = 0;
  for (int m : mid) ncell = std::max(ncell, (long long)c->hmaps[m].dims[0] * c->hmaps[m].dims[1]);
  HIPCHK(hipSetDevice(c->device));
  // search state per instance: g (8) + parent, heap position, heap (3 x 4) + flags (1) bytes per cell; searches run in
  // chunks of at most 2 GB of it
  const size_t per = (size_t)ncell * 21;   // (sizes the chunks; the block itself is laid out below)
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)2 << 30) / std::max<size_t>(per, 1)));
  const size_t N = (size_t)n, cells = (size_t)chunk * ncell;
  topay::JpsBatch B;
  auto lay_ws = [&](Carver& k) {
    B.g = k.take<double>(cells); B.parent = k.take<int>(cells); B.hpos = k.take<int>(cells); B.heap = k.take<int>(cells);
    B.flag = k.take<unsigned char>(cells + 64);   // (64 bytes of slack behind the flags, as ever)
  };
  double *d_start, *d_end, *d_own; int *d_mid, *d_len, *d_stats;
  auto lay_io = [&](Carver& k) {
    d_start = k.take<double>(2 * N); d_end = k.take<double>(2 * N); d_own = k.take<double>(out_ext ? 0 : 2 * N * cap_points);
    d_mid = k.take<int>(N); d_len = k.take<int>(N); d_stats = k.take<int>(2 * N);
  };
  DevBuf ws;
  topay_status s;
  if ((s = ws.carve(lay_ws)) != TOPAY_OK || (s = io.carve(lay_io)) != TOPAY_OK) return s;
  double* d_out = out_ext ? out_ext : d_own;
  HIPCHK(h2d(c, d_start, start_xy, 2 * N));
  HIPCHK(h2d(c, d_end, end_xy, 2 * N));
  HIPCHK(h2d(c, d_mid, mid.data(), N));
  B.cap = cap_points; B.ncell_max = ncell; B.map_id = d_mid; B.start = d_start; B.end = d_end; B.threshold = threshold;
  B.out_len = d_len; B.out_xy = d_out; B.stats = d_stats;
  if (tm) HIPCHK(tm->start(c->stream));
  for (int i0 = 0; i0 < n; i0 += chunk) {
    B.inst0 = i0;
    B.n = std::min(chunk, n - i0);
    HIPCHK(hipMemsetAsync(B.flag, 0, (size_t)B.n * ncell, c->stream));
    hipLaunchKernelGGL(topay::k_jps, dim3((unsigned)B.n), dim3(64), 0, c->stream, (const DevMap*)c->dmaps.p, B);   // one wave per search
    HIPCHK(hipGetLastError());
  }
  if (tm) HIPCHK(tm->stop(c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));   // (the search state is released on the way out)
  dev->len = d_len; dev->out = d_out; dev->stats = d_stats;
  return TOPAY_OK;
}

// Points a discretised / shortened path may have: one point per cell along twice the map's diagonal, and 512 for the
// extra point of every segment.  (A raw path zigzags inside the sampling region, whose length is at most the diagonal
// + 2 sample_inflate_x; a path that needs more gives status -1.)  The cap of a query is that of its own map (the kernel
// forms it again from the map's dimensions); the buffers of a call are strided by the largest.  harness/topo_prm.hpp: topo_pt_cap.
static int topo_pt_cap(int nx, int ny) { return 2 * (int)std::ceil(std::sqrt((double)nx * nx + (double)ny * ny)) + 512; }

// Layout of the integer scratch of a topay_topo_paths call (FrontState::tp_i), in ints from its start: per node type,
// neighbour count, guard list, neighbour ids; per query raw-path lengths, kept raw paths, point-buffer lengths, meta.
struct TopoLayout {
  size_t type, nnb, guards, nb, raw_len, keep, pts_len, meta, total;
  TopoLayout(size_t N, const topay_topo_params_t& P, int nbuf) {
    const size_t nn = N * (size_t)P.node_cap;
    type = 0; nnb = nn; guards = 2 * nn; nb = 3 * nn;
    raw_len = nb + nn * TOPAY_TOPO_MAX_NB;
    keep = raw_len + N * (size_t)P.max_raw_path;
    pts_len = keep + N * (size_t)P.max_raw_path2;
    meta = pts_len + N * (size_t)nbuf;
    total = meta + N * 8;
  }
};

struct TopoDev { int* n_paths; int* path_len; double* path_xy; int* stats; };

// findTopoPaths for n host-side queries; the results stay on the device (in the context's tp_io, or the paths at out_ext:
// n x cap_paths x cap_points x 2).  inst (optional, host): the instance number of every query instead of first_instance +
// query.  The public entry copies the results back and clears the unwritten part of the paths first (clear_out).  tm: started and
// stopped around the kernel alone (null: the roadmap's own stopwatch).
static topay_status topo_impl(topay_ctx* c, int n, const int* map_ids, const double* start_xy, const double* end_xy, const int* critical,
                              const topay_topo_params_t* prm, unsigned long long first_instance, const unsigned long long* inst, int cap_paths,
                              int cap_points, double* out_ext, bool clear_out, TopoDev* dev, DevTimer* tm = nullptr) {
  if (!c || n <= 0 || !start_xy || !end_xy || cap_points < 2) return TOPAY_ERR_INVALID_ARG;
  topay_topo_params_t P;
  if (prm) P = *prm;
  else topay_topo_default_params(&P);
  if (P.max_sample_num < 0 || P.max_raw_path < 1 || P.max_raw_path > 4096 || P.max_raw_path2 < 1 || P.max_raw_path2 > 64 || P.reserve_num < 1 ||
      P.reserve_num > 16 || P.node_cap < 2 || P.node_cap > 65535 || !(P.sample_inflate_x >= 0.0) || !(P.sample_inflate_y >= 0.0)) {
    set_err("topay_topo_paths: parameters out of range (max_raw_path 1..4096, max_raw_path2 1..64, reserve_num 1..16, node_cap 2..65535)");
    return TOPAY_ERR_INVALID_ARG;
  }
  if (cap_paths < P.reserve_num) { set_err("topay_topo_paths: cap_paths is smaller than reserve_num"); return TOPAY_ERR_INVALID_ARG; }
  if (topay_status cs = check_map_slots(c, n, map_ids, kMapResident | kMapFront, "topay_topo_paths")) return cs;
  std::vector<int> mid((size_t)n, 0);
  if (map_ids) mid.assign(map_ids, map_ids + n);
  int pt_cap = 0;
  for (int m : mid) pt_cap = std::max(pt_cap, topo_pt_cap(c->hmaps[m].dims[0], c->hmaps[m].dims[1]));
  HIPCHK(hipSetDevice(c->device));
  const size_t N = (size_t)n, nn = N * P.node_cap;
  const int nbuf = 2 * P.max_raw_path2 + 2 * P.reserve_num;
  topay_status s;
  const TopoLayout lay(N, P, nbuf);
  if ((s = c->front.tp_i.ensure(lay.total * 4)) != TOPAY_OK || (s = c->front.tp_d.ensure(nn * 2 * 8)) != TOPAY_OK ||
      (s = c->front.tp_raw.ensure(N * P.max_raw_path * TOPAY_TOPO_RAWLEN * 2)) != TOPAY_OK ||
      (s = c->front.tp_pts.ensure(N * (size_t)nbuf * (size_t)pt_cap * 16)) != TOPAY_OK)
    return s;
  const size_t out_pts = N * (size_t)cap_paths * cap_points;
  double *d_start, *d_end, *d_own; unsigned long long* d_inst; int *d_mid, *d_crit, *d_np, *d_len, *d_stats;
  auto lay_io = [&](Carver& k) {
    d_start = k.take<double>(2 * N); d_end = k.take<double>(2 * N); d_inst = k.take<unsigned long long>(N);
    d_own = k.take<double>(out_ext ? 0 : 2 * out_pts);
    d_mid = k.take<int>(N); d_crit = k.take<int>(N); d_np = k.take<int>(N); d_len = k.take<int>(N * cap_paths); d_stats = k.take<int>(8 * N);
  };
  if ((s = c->front.tp_io.carve(lay_io)) != TOPAY_OK) return s;
  double* d_out = out_ext ? out_ext : d_own;
  HIPCHK(h2d(c, d_start, start_xy, 2 * N));
  HIPCHK(h2d(c, d_end, end_xy, 2 * N));
  HIPCHK(h2d(c, d_mid, mid.data(), N));
  if (critical) HIPCHK(h2d(c, d_crit, critical, N));
  if (inst) HIPCHK(h2d(c, d_inst, inst, N));
  if (clear_out) HIPCHK(hipMemsetAsync(d_out, 0, 2 * out_pts * sizeof(double), c->stream));
  topay::TopoBatch B;
  B.n = n; B.cap_paths = cap_paths; B.cap_points = cap_points; B.pt_cap = pt_cap; B.nbuf = nbuf; B.inst_base = first_instance;
  B.inst = inst ? d_inst : nullptr;
  B.map_id = d_mid; B.start = d_start; B.end = d_end; B.critical = critical ? d_crit : nullptr;
  B.P.sample_inflate_x = P.sample_inflate_x; B.P.sample_inflate_y = P.sample_inflate_y; B.P.clearance = P.clearance;
  B.P.ratio_to_short = P.ratio_to_short; B.P.max_sample_num = P.max_sample_num; B.P.max_raw_path = P.max_raw_path;
  B.P.max_raw_path2 = P.max_raw_path2; B.P.reserve_num = P.reserve_num; B.P.node_cap = P.node_cap; B.P.reserved = 0; B.P.seed = P.seed;
  int* ti = c->front.tp_i.as<int>();
  B.nd_type = ti + lay.type; B.nd_nnb = ti + lay.nnb; B.guards = ti + lay.guards; B.nd_nb = ti + lay.nb;
  B.raw_len = ti + lay.raw_len; B.keep = ti + lay.keep; B.pts_len = ti + lay.pts_len; B.meta = ti + lay.meta;
  B.nd_pos = c->front.tp_d.as<double>();
  B.raw = c->front.tp_raw.as<unsigned short>();
  B.pts = c->front.tp_pts.as<double>();
  B.n_paths = d_np; B.path_len = d_len; B.path_xy = d_out; B.stats = d_stats;
  c->front.tp_n = 0;
  if (!tm) tm = &c->front.tp_timer;
  HIPCHK(tm->start(c->stream));
  hipLaunchKernelGGL(topay::k_topo, dim3((unsigned)n), dim3(64), 0, c->stream, (const DevMap*)c->dmaps.p, B);   // one wave per query
  HIPCHK(hipGetLastError());
  HIPCHK(tm->stop(c->stream));
  dev->n_paths = d_np; dev->path_len = d_len; dev->path_xy = d_out; dev->stats = d_stats;
  c->front.tp_n = n; c->front.tp_pt_cap = pt_cap; c->front.tp_nbuf = nbuf; c->front.tp_P = P;   // (valid once the stream has been waited for)
  return TOPAY_OK;
}

// Inputs and results of one launch of the joint-space search, all on the device.
struct McIo {
  const long long* off; const int* len; const double* car; const double* start; const double* end; const int* mid;
  const unsigned long long* inst;   // instance numbers, or null: first_instance + search
  int* wb_len; double* wb; int* stats; double* cmax;
};

// MCRRTs::plan for n searches whose inputs are on the device; sizes the node tables, leaves the results on the device.
static topay_status mcrrt_launch(topay_ctx* c, int n, const topay_mcrrt_params_t& P, unsigned long long first_instance, int cap_per_path, const McIo& io) {
  const size_t nn = (size_t)n * P.node_cap;
  topay_status s;
  if ((s = c->front.mc_i.ensure(nn * 5 * 4)) != TOPAY_OK || (s = c->front.mc_d.ensure(nn * 8 * 8)) != TOPAY_OK ||
      (s = c->front.mc_k.ensure(nn * TOPAY_MC_KEYW * 8)) != TOPAY_OK || (s = c->front.mc_rs.ensure((size_t)n * 2 * cap_per_path * sizeof(topay::RsPath))) != TOPAY_OK)
    return s;
  HIPCHK(hipMemsetAsync(io.wb, 0, (size_t)n * cap_per_path * 10 * 8, c->stream));
  HIPCHK(hipMemsetAsync(io.cmax, 0, (size_t)n * 8, c->stream));
  topay_status ps = push_params(c);
  if (ps != TOPAY_OK) return ps;
  topay::McrrtBatch B;
  B.n = n; B.layer_cap = cap_per_path; B.inst_base = first_instance; B.inst = io.inst;
  B.map_id = io.mid; B.car_off = io.off; B.car_len = io.len; B.car = io.car; B.start = io.start; B.end = io.end;
  B.P.goal_sample_rate = P.goal_sample_rate; B.P.check_colli_res = P.check_colli_res; B.P.rs_rho = P.rs_turning_radius;
  B.P.max_iter = P.max_iter; B.P.max_sample_tries = P.max_sample_tries; B.P.node_cap = P.node_cap; B.P.reserved = 0; B.P.seed = P.seed;
  int* ni = c->front.mc_i.as<int>();
  B.nd_layer = ni; B.nd_state = ni + nn; B.nd_parent = ni + 2 * nn; B.nd_nchild = ni + 3 * nn; B.nd_mark = ni + 4 * nn;
  B.nd_cost = c->front.mc_d.as<double>(); B.nd_q = B.nd_cost + nn; B.nd_key = c->front.mc_k.as<unsigned long long>();
  B.rs = (topay::RsPath*)c->front.mc_rs.p;
  B.wb_len = io.wb_len; B.wb = io.wb; B.stats = io.stats; B.cmax = io.cmax;
  c->front.mc_n = 0;
  hipLaunchKernelGGL(topay::k_mcrrt, dim3((unsigned)n), dim3(64), 0, c->stream, (const DevMap*)c->dmaps.p, B);
  HIPCHK(hipGetLastError());
  c->front.mc_n = n;
  c->front.mc_node_cap = P.node_cap;
  return TOPAY_OK;
}

static bool mcrrt_params_ok(const topay_mcrrt_params_t& P) {
  return !(P.max_iter < 0 || P.max_sample_tries < 1 || P.node_cap < 2 || !(P.check_colli_res > 0.0) || !(P.rs_turning_radius > 0.0));
}

extern "C" {

// GridMap::isWholeBodyCollision (grid_map.h:613-650) of n states (x, y, theta, q1..q7) against map slot map_id:
// collide[i] = 1 when the state violates a joint limit, leaves the map or collides (front-end building block).
topay_status topay_whole_body_collision(topay_ctx* c, int map_id, int n, const double* states, int* collide) {
  if (!c || !states || !collide || n < 0) return TOPAY_ERR_INVALID_ARG;
  if (topay_status cs = check_map_slots(c, 1, &map_id, kMapResident, "topay_whole_body_collision")) return cs;
  if (n == 0) return TOPAY_OK;
  HIPCHK(hipSetDevice(c->device));
  topay_status s;
  double* d_st; int* d_out;
  if ((s = c->pb_io.carve([&](Carver& k) { d_st = k.take<double>((size_t)n * 10); d_out = k.take<int>((size_t)n); })) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_st, states, (size_t)n * 10));
  topay_status ps = push_params(c);
  if (ps != TOPAY_OK) return ps;
  hipLaunchKernelGGL(k_whole_body, dim3((n + 63) / 64), dim3(64), 0, c->stream, (const DevMap*)c->dmaps.p, map_id, n,
                     (const double*)d_st, d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(c, collide, d_out, (size_t)n));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

// GraphSearch::getDensePath (graph_search.cpp:119-176) for n_paths raw 2-D paths at once.
topay_status topay_dense_path(topay_ctx* c, int n_paths, const int* raw_len, const double* raw_xy, double step_size, const double* start_yaw,
                              const double* end_yaw, double v_max, double w_max, int cap_per_path, int* out_len, double* out) {
  if (!c || n_paths <= 0 || !raw_len || !raw_xy || !start_yaw || !end_yaw || !out_len || !out || cap_per_path <= 0 || !(step_size > 0.0))
    return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  std::vector<long long> off((size_t)n_paths + 1, 0);
  for (int p = 0; p < n_paths; p++) {
    if (raw_len[p] < 1) return TOPAY_ERR_INVALID_ARG;
    off[p + 1] = off[p] + raw_len[p];
  }
  const size_t tot = (size_t)off[n_paths];
  DevBuf d_raw, d_off, d_len, d_yaw, d_out, d_olen;
  topay_status s;
  if ((s = d_raw.ensure(tot * 16)) != TOPAY_OK || (s = d_off.ensure(((size_t)n_paths + 1) * 8)) != TOPAY_OK ||
      (s = d_len.ensure((size_t)n_paths * 4)) != TOPAY_OK || (s = d_yaw.ensure((size_t)n_paths * 16)) != TOPAY_OK ||
      (s = d_out.ensure((size_t)n_paths * cap_per_path * 32)) != TOPAY_OK || (s = d_olen.ensure((size_t)n_paths * 4)) != TOPAY_OK)
    return s;
  HIPCHK(h2d(c, d_raw.as<double>(), raw_xy, 2 * tot));
  HIPCHK(h2d(c, d_off.as<long long>(), off.data(), (size_t)n_paths + 1));
  HIPCHK(h2d(c, d_len.as<int>(), raw_len, (size_t)n_paths));
  HIPCHK(h2d(c, d_yaw.as<double>(), start_yaw, (size_t)n_paths));
  HIPCHK(h2d(c, d_yaw.as<double>() + n_paths, end_yaw, (size_t)n_paths));
  if ((s = dense_launch(c, n_paths, d_raw.as<double>(), d_off.as<long long>(), d_len.as<int>(), step_size, d_yaw.as<double>(),
                        d_yaw.as<double>() + n_paths, v_max, w_max, cap_per_path, d_out.as<double>(), d_olen.as<int>())) != TOPAY_OK)
    return s;
  HIPCHK(d2h(c, out_len, d_olen.as<int>(), (size_t)n_paths));
  HIPCHK(d2h(c, out, d_out.as<double>(), (size_t)n_paths * cap_per_path * 4));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

// MCRRTs::connectCollision (mcrrts.h:310-348): number of checks of every edge (lines 321-328; host arithmetic) ...
topay_status topay_connect_check_num(int n_edges, const double* rs_distance, const double* q_from, const double* q_to, double check_res,
                                     int* piece_num) {
  if (n_edges < 0 || !rs_distance || !q_from || !q_to || !piece_num || !(check_res > 0.0)) return TOPAY_ERR_INVALID_ARG;
  for (int e = 0; e < n_edges; e++) {
    const int check_num_car = (int)std::ceil(rs_distance[e] / check_res);
    double dmax = 0.0;
    for (int q = 0; q < 7; q++) dmax = std::max(dmax, std::fabs(q_to[7 * e + q] - q_from[7 * e + q]));
    const int check_num_theta = (int)std::ceil(dmax / check_res);
    piece_num[e] = std::max(std::max(check_num_car, check_num_theta), 3);
  }
  return TOPAY_OK;
}

// ... and the checks themselves (lines 330-345), every interpolated state of every edge in one launch.
topay_status topay_connect_collision(topay_ctx* c, int map_id, int n_edges, const int* piece_num, const double* car_poses, const double* q_from,
                                     const double* q_to, int* collide) {
  if (!c || n_edges < 0 || (n_edges > 0 && (!piece_num || !car_poses || !q_from || !q_to || !collide))) return TOPAY_ERR_INVALID_ARG;
  if (topay_status cs = check_map_slots(c, 1, &map_id, kMapResident, "topay_connect_collision")) return cs;
  if (n_edges == 0) return TOPAY_OK;
  HIPCHK(hipSetDevice(c->device));
  std::vector<int> edge_of, idx;
  for (int e = 0; e < n_edges; e++) {
    if (piece_num[e] <= 0) return TOPAY_ERR_INVALID_ARG;
    for (int i = 0; i < piece_num[e]; i++) { edge_of.push_back(e); idx.push_back(i); }
  }
  const size_t nc = edge_of.size();
  DevBuf d_i, d_d;
  topay_status s;
  const size_t ne = (size_t)n_edges;
  int *d_edge, *d_idx, *d_pn, *d_col; double *d_car, *d_qf, *d_qt;
  auto lay_i = [&](Carver& k) { d_edge = k.take<int>(nc); d_idx = k.take<int>(nc); d_pn = k.take<int>(ne); d_col = k.take<int>(ne); };
  auto lay_d = [&](Carver& k) { d_car = k.take<double>(3 * nc); d_qf = k.take<double>(7 * ne); d_qt = k.take<double>(7 * ne); };
  if ((s = d_i.carve(lay_i)) != TOPAY_OK || (s = d_d.carve(lay_d)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_edge, edge_of.data(), nc));
  HIPCHK(h2d(c, d_idx, idx.data(), nc));
  HIPCHK(h2d(c, d_pn, piece_num, ne));
  HIPCHK(hipMemsetAsync(d_col, 0, ne * sizeof(int), c->stream));
  HIPCHK(h2d(c, d_car, car_poses, 3 * nc));
  HIPCHK(h2d(c, d_qf, q_from, 7 * ne));
  HIPCHK(h2d(c, d_qt, q_to, 7 * ne));
  topay_status ps = push_params(c);
  if (ps != TOPAY_OK) return ps;
  hipLaunchKernelGGL(k_connect, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, c->stream, (const DevMap*)c->dmaps.p, map_id, (long long)nc,
                     (const int*)d_edge, (const int*)d_idx, (const int*)d_pn, (const double*)d_car, (const double*)d_qf, (const double*)d_qt, d_col);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(c, collide, d_col, ne));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

topay_status topay_plan2d_jps(topay_ctx* c, int n, const int* map_ids, const double* start_xy, const double* end_xy, double threshold,
                              int cap_points, int* out_len, double* out_xy, int* stats) {
  if (!c || n < 0 || cap_points < 2 || (n > 0 && (!start_xy || !end_xy || !out_len || !out_xy))) return TOPAY_ERR_INVALID_ARG;
  if (n == 0) return TOPAY_OK;
  DevBuf io;
  JpsDev d;
  topay_status s = jps_impl(c, n, map_ids, start_xy, end_xy, threshold, cap_points, io, nullptr, &d, "topay_plan2d_jps");
  if (s != TOPAY_OK) return s;
  HIPCHK(d2h(c, out_len, d.len, (size_t)n));
  HIPCHK(d2h(c, out_xy, d.out, (size_t)n * cap_points * 2));
  if (stats) HIPCHK(d2h(c, stats, d.stats, (size_t)n * 2));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

void topay_topo_default_params(topay_topo_params_t* p) {
  if (!p) return;
  p->sample_inflate_x = 1.5;     // planner/params/topo_prm.yaml
  p->sample_inflate_y = 4.0;
  p->clearance = 0.1;
  p->ratio_to_short = 2.0;
  p->max_sample_num = 2368;      // the reference's 0.01 s of sampling as a count (include/topay.h; docs/EXPERIMENTS.md)
  p->max_raw_path = 300;
  p->max_raw_path2 = 25;
  p->reserve_num = 6;
  p->node_cap = 512;
  p->reserved = 0;
  p->seed = 42;
}

topay_status topay_topo_paths(topay_ctx* c, int n, const int* map_ids, const double* start_xy, const double* end_xy, const int* critical,
                              const topay_topo_params_t* prm, unsigned long long first_instance, int cap_paths, int cap_points, int* n_paths,
                              int* path_len, double* path_xy, int* stats) {
  if (!c || n <= 0 || !start_xy || !end_xy || !n_paths || !path_len || !path_xy || cap_points < 2) return TOPAY_ERR_INVALID_ARG;
  TopoDev d;
  const size_t N = (size_t)n;
  topay_status s = topo_impl(c, n, map_ids, start_xy, end_xy, critical, prm, first_instance, nullptr, cap_paths, cap_points, nullptr, true, &d);
  if (s != TOPAY_OK) return s;
  const int keep_n = c->front.tp_n;
  c->front.tp_n = 0;   // (the graphs are readable once the results have arrived)
  HIPCHK(d2h(c, n_paths, d.n_paths, N));
  HIPCHK(d2h(c, path_len, d.path_len, N * cap_paths));
  HIPCHK(d2h(c, path_xy, d.path_xy, N * (size_t)cap_paths * cap_points * 2));
  if (stats) HIPCHK(d2h(c, stats, d.stats, N * 8));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(c->front.tp_timer.read(&c->last_ms));
  c->last_launches = 1;
  c->front.tp_n = keep_n;
  return TOPAY_OK;
}

topay_status topay_topo_graph(topay_ctx* c, int instance, int cap, int* id, int* type, double* pos_xy, int* n_neighbors, int* neighbors,
                              int* n_nodes) {
  if (!c || instance < 0 || instance >= c->front.tp_n || cap < 0) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  const topay_topo_params_t& P = c->front.tp_P;
  const size_t N = (size_t)c->front.tp_n, o = (size_t)instance * P.node_cap;
  const TopoLayout lay(N, P, c->front.tp_nbuf);
  const int* ti = c->front.tp_i.as<int>();
  const int* d_meta = ti + lay.meta + 8 * (size_t)instance;
  int meta[8];
  HIPCHK(memcpy_sync(c, meta, d_meta, sizeof(meta), hipMemcpyDeviceToHost));
  const int created = std::min(std::max(meta[0], 0), P.node_cap);
  std::vector<int> t((size_t)created), k((size_t)created), nb((size_t)created * TOPAY_TOPO_MAX_NB);
  std::vector<double> pos((size_t)created * 2);
  if (created > 0) {
    HIPCHK(d2h_sync(c, t.data(), ti + lay.type + o, (size_t)created));
    HIPCHK(d2h_sync(c, k.data(), ti + lay.nnb + o, (size_t)created));
    HIPCHK(d2h_sync(c, nb.data(), ti + lay.nb + o * TOPAY_TOPO_MAX_NB, (size_t)created * TOPAY_TOPO_MAX_NB));
    HIPCHK(d2h_sync(c, pos.data(), c->front.tp_d.as<double>() + 2 * o, (size_t)created * 2));
  }
  int m = 0;
  for (int i = 0; i < created; i++) {
    if (t[i] == 0) continue;   // erased by pruneGraph
    if (m < cap) {
      if (id) id[m] = i;
      if (type) type[m] = t[i];
      if (pos_xy) { pos_xy[2 * m] = pos[2 * (size_t)i]; pos_xy[2 * m + 1] = pos[2 * (size_t)i + 1]; }
      if (n_neighbors) n_neighbors[m] = k[i];
      if (neighbors)
        for (int j = 0; j < TOPAY_TOPO_MAX_NB; j++) neighbors[(size_t)m * TOPAY_TOPO_MAX_NB + j] = j < k[i] ? nb[(size_t)i * TOPAY_TOPO_MAX_NB + j] : 0;
    }
    m++;
  }
  if (n_nodes) *n_nodes = m;
  return TOPAY_OK;
}

topay_status topay_topo_raw_paths(topay_ctx* c, int instance, int which, int cap_paths, int cap_points, int* n_paths, int* path_len,
                                  double* path_xy) {
  if (!c || instance < 0 || instance >= c->front.tp_n || which < 0 || which > 1 || cap_paths < 0 || cap_points < 0 || !n_paths || !path_len || !path_xy)
    return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  const topay_topo_params_t& P = c->front.tp_P;
  const size_t N = (size_t)c->front.tp_n, q = (size_t)instance;
  const TopoLayout lay(N, P, c->front.tp_nbuf);
  const int* ti = c->front.tp_i.as<int>();
  const int* d_rawlen = ti + lay.raw_len;
  const int* d_keep = ti + lay.keep;
  const int* d_ptslen = ti + lay.pts_len;
  const int* d_meta = ti + lay.meta;
  int meta[8];
  HIPCHK(memcpy_sync(c, meta, d_meta + 8 * q, sizeof(meta), hipMemcpyDeviceToHost));
  const int n_keep = meta[3] == 0 ? std::min(std::max(meta[1], 0), P.max_raw_path2) : 0;
  *n_paths = n_keep;
  if (n_keep == 0) return TOPAY_OK;
  std::vector<int> keep((size_t)n_keep);
  HIPCHK(d2h_sync(c, keep.data(), d_keep + q * P.max_raw_path2, (size_t)n_keep));
  if (which == 0) {
    const int created = std::min(std::max(meta[0], 0), P.node_cap);
    std::vector<double> pos((size_t)created * 2);
    HIPCHK(d2h_sync(c, pos.data(), c->front.tp_d.as<double>() + 2 * q * P.node_cap, (size_t)created * 2));
    std::vector<int> rl((size_t)P.max_raw_path);
    HIPCHK(d2h_sync(c, rl.data(), d_rawlen + q * P.max_raw_path, rl.size()));
    std::vector<unsigned short> ids(TOPAY_TOPO_RAWLEN);
    for (int k = 0; k < n_keep && k < cap_paths; k++) {
      const int r = keep[k], len = std::min(std::max(rl[r], 0), TOPAY_TOPO_RAWLEN);
      HIPCHK(d2h_sync(c, ids.data(), c->front.tp_raw.as<unsigned short>() + (q * P.max_raw_path + r) * TOPAY_TOPO_RAWLEN, (size_t)len));
      path_len[k] = len;
      for (int j = 0; j < len && j < cap_points; j++) {
        const int nd = std::min((int)ids[j], created - 1);
        path_xy[((size_t)k * cap_points + j) * 2] = pos[2 * (size_t)nd];
        path_xy[((size_t)k * cap_points + j) * 2 + 1] = pos[2 * (size_t)nd + 1];
      }
    }
  } else {
    std::vector<int> pl((size_t)n_keep);
    HIPCHK(d2h_sync(c, pl.data(), d_ptslen + q * c->front.tp_nbuf, (size_t)n_keep));
    for (int k = 0; k < n_keep && k < cap_paths; k++) {
      const int len = std::min(std::max(pl[k], 0), c->front.tp_pt_cap);
      path_len[k] = len;
      const int w = std::min(len, cap_points);
      if (w > 0)
        HIPCHK(d2h_sync(c, path_xy + (size_t)k * cap_points * 2, c->front.tp_pts.as<double>() + (q * c->front.tp_nbuf + k) * (size_t)c->front.tp_pt_cap * 2, (size_t)w * 2));
    }
  }
  return TOPAY_OK;
}

void topay_mcrrt_default_params(topay_mcrrt_params_t* p) {
  if (!p) return;
  p->goal_sample_rate = 0.4;      // planner/params/mcrrts.yaml
  p->check_colli_res = 0.01;
  p->rs_turning_radius = 1.0e-2;  // mcrrts.h:134
  p->max_iter = 1000;
  p->max_sample_tries = 64;
  p->node_cap = 2048;
  p->reserved = 0;
  p->seed = 42;
}

topay_status topay_mcrrt_plan(topay_ctx* c, int n, const int* map_ids, const int* path_len, const double* car_paths, const double* start,
                              const double* end, const topay_mcrrt_params_t* prm, unsigned long long first_instance, int cap_per_path,
                              int* wb_len, double* wb_path, int* stats, double* c_max) {
  if (!c || n < 0 || cap_per_path < 2 || (n > 0 && (!path_len || !car_paths || !start || !end || !wb_len || !wb_path))) return TOPAY_ERR_INVALID_ARG;
  topay_mcrrt_params_t P;
  if (prm) P = *prm;
  else topay_mcrrt_default_params(&P);
  if (!mcrrt_params_ok(P)) return TOPAY_ERR_INVALID_ARG;
  if (n == 0) return TOPAY_OK;
  std::vector<long long> off((size_t)n + 1, 0);
  std::vector<int> mid((size_t)n, 0);
  if (map_ids) mid.assign(map_ids, map_ids + n);
  for (int p = 0; p < n; p++) {
    if (path_len[p] < 2 || path_len[p] > cap_per_path || path_len[p] > 255) {
      set_err("topay_mcrrt_plan: chassis path " + std::to_string(p) + " has " + std::to_string(path_len[p]) + " layers (2.." +
              std::to_string(std::min(cap_per_path, 255)) + " supported: the reference's node key holds the layer in one character)");
      return TOPAY_ERR_INVALID_ARG;
    }
    off[p + 1] = off[p] + path_len[p];
  }
  if (topay_status cs = check_map_slots(c, n, map_ids, kMapResident, "topay_mcrrt_plan")) return cs;
  HIPCHK(hipSetDevice(c->device));
  const size_t tot = (size_t)off[n];
  topay_status s;
  // inputs: offsets (i64), chassis paths, start, end (f64), map ids, lengths (int); outputs: wb, c_max (f64), wb_len, stats (int)
  const size_t N = (size_t)n;
  long long* d_off; double *d_car, *d_start, *d_end, *d_wb, *d_cmax; int *d_mid, *d_len, *d_wlen, *d_stats;
  auto lay = [&](Carver& k) {
    d_off = k.take<long long>(N + 1); d_car = k.take<double>(4 * tot); d_start = k.take<double>(10 * N); d_end = k.take<double>(10 * N);
    d_wb = k.take<double>(N * cap_per_path * 10); d_cmax = k.take<double>(N);
    d_mid = k.take<int>(N); d_len = k.take<int>(N); d_wlen = k.take<int>(N); d_stats = k.take<int>(8 * N);
  };
  if ((s = c->front.mc_in.carve(lay)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_off, off.data(), N + 1));
  HIPCHK(h2d(c, d_car, car_paths, 4 * tot));
  HIPCHK(h2d(c, d_start, start, 10 * N));
  HIPCHK(h2d(c, d_end, end, 10 * N));
  HIPCHK(h2d(c, d_mid, mid.data(), N));
  HIPCHK(h2d(c, d_len, path_len, N));
  McIo io;
  io.off = d_off; io.len = d_len; io.car = d_car; io.start = d_start; io.end = d_end; io.mid = d_mid; io.inst = nullptr;
  io.wb_len = d_wlen; io.wb = d_wb; io.stats = d_stats; io.cmax = d_cmax;
  if ((s = mcrrt_launch(c, n, P, first_instance, cap_per_path, io)) != TOPAY_OK) return s;
  HIPCHK(d2h(c, wb_len, d_wlen, N));
  HIPCHK(d2h(c, wb_path, d_wb, N * cap_per_path * 10));
  if (stats) HIPCHK(d2h(c, stats, d_stats, 8 * N));
  if (c_max) HIPCHK(d2h(c, c_max, d_cmax, N));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TOPAY_OK;
}

topay_status topay_mcrrt_nodes(topay_ctx* c, int instance, int cap, int* layer, int* state, int* parent, double* cost, double* q) {
  if (!c || instance < 0 || instance >= c->front.mc_n || cap < 0) return TOPAY_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(c->device));
  const size_t nn = (size_t)c->front.mc_n * c->front.mc_node_cap, o = (size_t)instance * c->front.mc_node_cap;
  const size_t m = (size_t)std::min(cap, c->front.mc_node_cap);
  const int* ni = c->front.mc_i.as<int>();
  const double* nd = c->front.mc_d.as<double>();
  if (layer) HIPCHK(d2h_sync(c, layer, ni + o, m));
  if (state) HIPCHK(d2h_sync(c, state, ni + nn + o, m));
  if (parent) HIPCHK(d2h_sync(c, parent, ni + 2 * nn + o, m));
  if (cost) HIPCHK(d2h_sync(c, cost, nd + o, m));
  if (q) HIPCHK(d2h_sync(c, q, nd + nn + 7 * o, m * 7));
  return TOPAY_OK;
}

// ompl::base::ReedsSheppStateSpace(rho): distance and interpolate as the search uses them, for n pose pairs (one thread each)
topay_status topay_reeds_shepp(topay_ctx* c, int n, const double* from, const double* to, const double* t, double rho, double* distance,
                               int* word, double* lengths, double* pose) {
  if (!c || n < 0 || !(rho > 0.0) || (n > 0 && (!from || !to))) return TOPAY_ERR_INVALID_ARG;
  if (n == 0) return TOPAY_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t N = (size_t)n;
  double *d_from, *d_to, *d_t, *d_dist, *d_len, *d_pose; int* d_word;
  auto lay = [&](Carver& k) {
    d_from = k.take<double>(3 * N); d_to = k.take<double>(3 * N); d_t = k.take<double>(N); d_dist = k.take<double>(N);
    d_len = k.take<double>(5 * N); d_pose = k.take<double>(3 * N); d_word = k.take<int>(N);
  };
  DevBuf d;
  if (topay_status s = d.carve(lay); s != TOPAY_OK) return s;
  HIPCHK(h2d_sync(c, d_from, from, (size_t)n * 3));
  HIPCHK(h2d_sync(c, d_to, to, (size_t)n * 3));
  if (t) HIPCHK(h2d_sync(c, d_t, t, (size_t)n));
  hipLaunchKernelGGL(topay::k_reeds_shepp, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, (const double*)d_from, (const double*)d_to,
                     t ? (const double*)d_t : (const double*)nullptr, rho, d_dist, d_word, d_len, d_pose);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  if (distance) HIPCHK(d2h_sync(c, distance, d_dist, (size_t)n));
  if (word) HIPCHK(d2h_sync(c, word, d_word, (size_t)n));
  if (lengths) HIPCHK(d2h_sync(c, lengths, d_len, (size_t)n * 5));
  if (pose && t) HIPCHK(d2h_sync(c, pose, d_pose, (size_t)n * 3));
  return TOPAY_OK;
}

}  // extern "C"
