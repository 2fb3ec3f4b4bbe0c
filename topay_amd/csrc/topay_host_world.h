// Host side of the C-ABI, part 8: benchmark episodes on the device -- world generator, rasteriser, scenario samplers
// (topay_world.h) and their hand-over to the field construction (topay_host_maps.h).

#pragma once

static topay_status world_check_params(const topay_world_params_t* p) {
  if (!p || (p->kind != 0 && p->kind != 1)) return TOPAY_ERR_INVALID_ARG;
  if (!(p->size_xy > 0.0) || !(p->size_z > 0.0) || !(p->resolution > 0.0) || !(p->cloud_resolution > 0.0)) return TOPAY_ERR_INVALID_ARG;
  if (p->obs_num[0] < 0 || p->obs_num[1] < 0) return TOPAY_ERR_INVALID_ARG;
  if (p->desk_arrangement_range[0] < 1 || p->desk_arrangement_range[1] < p->desk_arrangement_range[0] || p->desk_arrangement_range[1] > 8)
    return TOPAY_ERR_INVALID_ARG;
  if ((long long)p->obs_num[0] + p->obs_num[1] + 2 > TOPAY_WORLD_MAX_BOXES) {
    set_err("world generator: more than " + std::to_string(TOPAY_WORLD_MAX_BOXES) + " obstacle boxes per map (obs_num[0] + obs_num[1] + 2 keep-outs)");
    return TOPAY_ERR_INVALID_ARG;
  }
  return TOPAY_OK;
}
// GridMap::init (workload.hpp:264-275)
static void world_map_desc(const topay_world_params_t* p, topay_map_desc_t* d) {
  const double size[3] = {p->size_xy, p->size_xy, p->size_z};
  for (int i = 0; i < 3; i++) {
    d->min_boundary[i] = -size[i] / 2.0;
    d->max_boundary[i] = size[i] / 2.0;
  }
  d->min_boundary[2] = 0.0;
  d->max_boundary[2] = size[2];
  for (int i = 0; i < 3; i++) {
    d->origin[i] = d->min_boundary[i];
    d->dims[i] = (int)std::ceil(size[i] / p->resolution);
  }
  d->resolution = p->resolution;
}
// a start / goal pair 3 m apart has to fit the square the ends are drawn from (the harness would draw for ever)
static bool world_fits_start_goal(double size_xy) { return (size_xy - 4.0) * 1.4142135623730951 > 3.0; }

// generation, rasterisation and the fields of n maps; the seeds and keep-outs are host arrays
static topay_status world_generate(topay_ctx* c, int n, int first_map_id, const topay_world_params_t* p, const unsigned long long* seed,
                                   const double* keepouts_xy, int* status, const char* who) {
  topay_status s;
  if ((s = world_check_params(p)) != TOPAY_OK) return s;
  if (!c || !seed) return TOPAY_ERR_INVALID_ARG;
  if ((s = check_map_range(first_map_id, n, who)) != TOPAY_OK) return s;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  WorldState& W = c->world;
  topay_map_desc_t desc;
  world_map_desc(p, &desc);
  const int nx = desc.dims[0], ny = desc.dims[1], nz = desc.dims[2];
  const size_t n2 = (size_t)nx * ny, n3 = n2 * nz, M = (size_t)n;
  if (n2 == 0 || n3 == 0) return TOPAY_ERR_INVALID_ARG;
  if (n3 >= (1ull << 31)) { set_err("world generator: map of 2^31 cells or more"); return TOPAY_ERR_UNSUPPORTED; }
  const bool keep = p->kind == 0 && keepouts_xy;
  WorldGenP G;
  memset(&G, 0, sizeof(G));
  G.kind = p->kind; G.obs0 = p->obs_num[0]; G.obs1 = p->obs_num[1];
  G.arr_lo = p->desk_arrangement_range[0]; G.arr_hi = p->desk_arrangement_range[1];
  G.box_cap = p->obs_num[0] + p->obs_num[1] + 2;
  // primitives of a map: 4 walls, 5 per desk of a group of up to arr_hi x arr_hi, 1 per box
  const long long prim_cap = p->kind == 0 ? 4 + 5LL * p->obs_num[0] * G.arr_hi * G.arr_hi + p->obs_num[1] : 4 + (long long)p->obs_num[0] + p->obs_num[1];
  if (prim_cap * (long long)n >= (1ll << 31)) { set_err("world generator: too many primitive boxes in one call"); return TOPAY_ERR_INVALID_ARG; }
  G.prim_cap = (int)prim_cap;
  G.size_xy = p->size_xy; G.cres = p->cloud_resolution;
  for (int i = 0; i < 2; i++) {
    G.wall_size[i] = p->wall_size_range[i]; G.wall_h[i] = p->wall_height_range[i]; G.float_size[i] = p->float_size_range[i];
    G.float_h[i] = p->float_height_range[i]; G.desk_len[i] = p->desk_length_range[i]; G.desk_wid[i] = p->desk_width_range[i];
    G.desk_h[i] = p->desk_height_range[i];
  }
  WorldGrid R;
  memset(&R, 0, sizeof(R));
  for (int i = 0; i < 3; i++) { R.origin[i] = desc.origin[i]; R.dims[i] = desc.dims[i]; }
  R.res_inv = 1.0 / p->resolution;   // grid_map.cpp:41
  R.chassis_height = c->hp.chassis_height;
  R.cres = p->cloud_resolution;
  R.prim_cap = G.prim_cap;

  unsigned long long* d_seed; double* d_keep; int *d_count, *d_status;
  auto lay_io = [&](Carver& k) { d_seed = k.take<unsigned long long>(M); d_keep = k.take<double>(M * 4); d_count = k.take<int>(M); d_status = k.take<int>(M); };
  if ((s = c->world.io.carve(lay_io)) != TOPAY_OK) return s;
  if ((s = c->world.prims.ensure(M * (size_t)G.prim_cap * sizeof(WorldPrim))) != TOPAY_OK) return s;
  signed char *d_occ3, *d_occ2, *d_occ2c;
  // (each grid starts on a 16-byte boundary: the first path stores 16 bytes at a time)
  const size_t b3 = WorldState::pad16(M * n3), b2 = WorldState::pad16(M * n2);
  c->sense.forget(first_map_id, n);   // (topay_sense_commit's grids)
  c->world.n = 0;
  if ((s = c->world.occ.ensure(b3 + 2 * b2)) != TOPAY_OK) return s;
  d_occ3 = c->world.occ.as<signed char>();
  d_occ2 = d_occ3 + b3;
  d_occ2c = d_occ2 + b2;
  WorldPrim* d_prims = c->world.prims.as<WorldPrim>();
  HIPCHK(h2d(c, d_seed, seed, M));
  if (keep) HIPCHK(h2d(c, d_keep, keepouts_xy, M * 4));

  HIPCHK(W.timer[WorldState::kGen].start(c->stream));
  {
    const size_t lb = (size_t)(312 + 6 * G.box_cap + 16) * sizeof(double);
    HIPCHK(hipFuncSetAttribute((const void*)k_world_generate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb));
    hipLaunchKernelGGL(k_world_generate, dim3((unsigned)n), dim3(TOPAY_WAVE), lb, c->stream, G, n, (const unsigned long long*)d_seed,
                       keep ? (const double*)d_keep : (const double*)nullptr, d_prims, d_count, d_status);
  }
  HIPCHK(W.timer[WorldState::kGen].stop(c->stream));
  HIPCHK(W.timer[WorldState::kRaster].start(c->stream));
  // The rule that picks the path: masks in LDS when the map has at most 32 layers, a multiple of 16 columns (whole 16-byte
  // stores, every map of the batch aligned) and masks of at most 150 KB; byte stores otherwise.
  const size_t lb = world_lds_bytes(nx, ny, nz);
  const bool lds_path = c->world.force_path != 2 && nz <= 32 && n2 % 16 == 0 && lb <= 150 * 1024;
  if (lds_path) {
    auto kern = nz <= 16 ? k_world_raster_lds<16> : k_world_raster_lds<32>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb));
    hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(256), lb, c->stream, R, (const WorldPrim*)d_prims, (const int*)d_count, d_occ3, d_occ2, d_occ2c);
  } else {
    HIPCHK(hipMemsetAsync(d_occ3, 0, b3 + 2 * b2, c->stream));
    hipLaunchKernelGGL(k_world_raster_bytes, dim3((unsigned)(M * (size_t)G.prim_cap)), dim3(TOPAY_WAVE), 0, c->stream, R, (const WorldPrim*)d_prims,
                       (const int*)d_count, d_occ3, d_occ2, d_occ2c);
  }
  c->world.path = lds_path ? 1 : 2;
  HIPCHK(hipGetLastError());
  HIPCHK(W.timer[WorldState::kRaster].stop(c->stream));
  HIPCHK(W.timer[WorldState::kFields].start(c->stream));
  if ((s = build_fields_from_device(c, n, first_map_id, &desc, d_occ3, d_occ2, d_occ2c, false)) != TOPAY_OK) return s;
  HIPCHK(W.timer[WorldState::kFields].stop(c->stream));
  if (status) HIPCHK(d2h(c, status, (const int*)d_status, M));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int k = WorldState::kGen; k <= WorldState::kFields; k++) HIPCHK(W.timer[k].read(&W.ms[k]));
  W.ms[WorldState::kSample] = 0.0;
  c->world.first = first_map_id;
  c->world.n = n;
  for (int i = 0; i < 3; i++) c->world.dims[i] = desc.dims[i];
  c->world.prims.release();
  return TOPAY_OK;
}

// The samplers' bodies: host arrays in and out, the slots checked by the caller.  timed: the sampling stopwatch runs around the
// launch alone (not the copies) and its time is kept.
static topay_status world_sample_arm(topay_ctx* c, int n, const int* map_ids, const unsigned long long* seed, int max_tries, double* states, int* ok,
                                     int* tries, bool timed) {
  topay_status s;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  const size_t N = (size_t)n;
  unsigned long long* d_seed; double* d_st; int *d_mid, *d_ok, *d_tr;
  auto lay = [&](Carver& k) { d_seed = k.take<unsigned long long>(N); d_st = k.take<double>(N * 10); d_mid = k.take<int>(N); d_ok = k.take<int>(N); d_tr = k.take<int>(N); };
  if ((s = c->world.io.carve(lay)) != TOPAY_OK) return s;
  std::vector<int> mid(N, 0);
  if (map_ids) mid.assign(map_ids, map_ids + n);
  HIPCHK(h2d(c, d_seed, seed, N));
  HIPCHK(h2d(c, d_st, (const double*)states, N * 10));
  HIPCHK(h2d(c, d_mid, (const int*)mid.data(), N));
  if ((s = push_params(c)) != TOPAY_OK) return s;
  const int bs = TOPAY_WORLD_SAMPLER_LANES;
  if (timed) HIPCHK(c->world.timer[WorldState::kSample].start(c->stream));
  hipLaunchKernelGGL(k_world_sample_arm, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), (size_t)bs * 312 * 8, c->stream, (const DevMap*)c->dmaps.p, n,
                     (const int*)d_mid, (const unsigned long long*)d_seed, max_tries > 0 ? max_tries : 2000, d_st, d_ok, d_tr);
  HIPCHK(hipGetLastError());
  if (timed) HIPCHK(c->world.timer[WorldState::kSample].stop(c->stream));
  HIPCHK(d2h(c, states, (const double*)d_st, N * 10));
  HIPCHK(d2h(c, ok, (const int*)d_ok, N));
  if (tries) HIPCHK(d2h(c, tries, (const int*)d_tr, N));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) HIPCHK(c->world.timer[WorldState::kSample].read(&c->world.ms[WorldState::kSample]));
  return TOPAY_OK;
}
static topay_status world_sample_scenarios(topay_ctx* c, int n, const int* map_ids, const unsigned long long* seed, double* start, double* goal, int* ok,
                                           bool timed) {
  topay_status s;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  const size_t N = (size_t)n;
  unsigned long long* d_seed; double *d_s, *d_g; int *d_mid, *d_ok;
  auto lay = [&](Carver& k) { d_seed = k.take<unsigned long long>(N); d_s = k.take<double>(N * 10); d_g = k.take<double>(N * 10); d_mid = k.take<int>(N); d_ok = k.take<int>(N); };
  if ((s = c->world.io.carve(lay)) != TOPAY_OK) return s;
  std::vector<int> mid(N, 0);
  if (map_ids) mid.assign(map_ids, map_ids + n);
  HIPCHK(h2d(c, d_seed, seed, N));
  HIPCHK(h2d(c, d_mid, (const int*)mid.data(), N));
  if ((s = push_params(c)) != TOPAY_OK) return s;
  const int bs = TOPAY_WORLD_SAMPLER_LANES;
  if (timed) HIPCHK(c->world.timer[WorldState::kSample].start(c->stream));
  hipLaunchKernelGGL(k_world_sample_scenario, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), (size_t)bs * 312 * 8, c->stream, (const DevMap*)c->dmaps.p, n,
                     (const int*)d_mid, (const unsigned long long*)d_seed, d_s, d_g, d_ok);
  HIPCHK(hipGetLastError());
  if (timed) HIPCHK(c->world.timer[WorldState::kSample].stop(c->stream));
  HIPCHK(d2h(c, start, (const double*)d_s, N * 10));
  HIPCHK(d2h(c, goal, (const double*)d_g, N * 10));
  HIPCHK(d2h(c, ok, (const int*)d_ok, N));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (timed) HIPCHK(c->world.timer[WorldState::kSample].read(&c->world.ms[WorldState::kSample]));
  return TOPAY_OK;
}

extern "C" {

topay_status topay_world_default_params(int kind, topay_world_params_t* p) {
  if (!p || (kind != 0 && kind != 1)) return TOPAY_ERR_INVALID_ARG;
  memset(p, 0, sizeof(*p));
  p->kind = kind;
  // params/map_tables.yaml, map_cuboids.yaml (harness/workload.hpp:80-92, 690-691)
  p->obs_num[0] = kind == 0 ? 40 : 80; p->obs_num[1] = 80;
  p->size_xy = 20.0; p->size_z = 1.6; p->resolution = 0.1; p->cloud_resolution = 0.05;
  p->wall_size_range[0] = 0.2; p->wall_size_range[1] = 0.8;
  p->wall_height_range[0] = 0.4; p->wall_height_range[1] = 1.5;
  p->float_size_range[0] = 0.3; p->float_size_range[1] = 0.6;
  p->float_height_range[0] = 0.4; p->float_height_range[1] = 0.8;
  p->desk_length_range[0] = 0.75; p->desk_length_range[1] = 1.25;
  p->desk_width_range[0] = 0.75; p->desk_width_range[1] = 1.25;
  p->desk_height_range[0] = 0.5; p->desk_height_range[1] = 1.0;
  p->desk_arrangement_range[0] = 1; p->desk_arrangement_range[1] = 2;
  return TOPAY_OK;
}

topay_status topay_generate_worlds(topay_ctx* c, int n, int first_map_id, const topay_world_params_t* params, const unsigned long long* seed,
                                   const double* keepouts_xy, int* status) {
  if (!c) return TOPAY_ERR_INVALID_ARG;
  return world_generate(c, n, first_map_id, params, seed, keepouts_xy, status, "topay_generate_worlds");
}

topay_status topay_get_occupancy(topay_ctx* c, int map_id, signed char* occ2d, signed char* occ2d_critical, signed char* occ3d) {
  if (!c) return TOPAY_ERR_INVALID_ARG;
  // a slot of the last topay_sense_commit, or of the last world generation
  int dims[3];
  const bool sensed = c->sense.has_occ(map_id);
  const signed char* o3 = sensed ? c->sense.occ3_of(map_id, dims) : c->world.occ3_of(map_id, dims);
  if (!o3) { set_err("topay_get_occupancy: map slot " + std::to_string(map_id) + " has no resident occupancy grids"); return TOPAY_ERR_NO_MAP; }
  HIPCHK(hipSetDevice(c->device));
  const size_t n2 = (size_t)dims[0] * dims[1], n3 = n2 * dims[2];
  if (occ3d) HIPCHK(d2h_sync(c, occ3d, o3, n3));
  if (occ2d) HIPCHK(d2h_sync(c, occ2d, sensed ? c->sense.occ2_of(map_id, false) : c->world.occ2_of(map_id, false), n2));
  if (occ2d_critical) HIPCHK(d2h_sync(c, occ2d_critical, sensed ? c->sense.occ2_of(map_id, true) : c->world.occ2_of(map_id, true), n2));
  return TOPAY_OK;
}

topay_status topay_world_last_path(topay_ctx* c, int* path) {
  if (!c || !path) return TOPAY_ERR_INVALID_ARG;
  *path = c->world.path;
  return TOPAY_OK;
}
topay_status topay_world_test_path(topay_ctx* c, int path) {
  if (!c || (path != 0 && path != 2)) return TOPAY_ERR_INVALID_ARG;
  c->world.force_path = path;
  return TOPAY_OK;
}
topay_status topay_world_test_max_tries(topay_ctx* c, int max_tries) {
  if (!c || max_tries < 0) return TOPAY_ERR_INVALID_ARG;
  c->world.max_tries = max_tries;
  return TOPAY_OK;
}
topay_status topay_world_stage_ms(topay_ctx* c, double ms[4]) {
  if (!c || !ms) return TOPAY_ERR_INVALID_ARG;
  for (int k = 0; k < 4; k++) ms[k] = c->world.ms[k];
  return TOPAY_OK;
}

topay_status topay_sample_start_goal_xy(int n, const unsigned long long* seed, double size_xy, double* start3, double* goal3) {
  if (n <= 0 || !seed || !start3 || !goal3 || !world_fits_start_goal(size_xy)) return TOPAY_ERR_INVALID_ARG;
  const double min_b[2] = {-size_xy / 2.0, -size_xy / 2.0}, max_b[2] = {size_xy / 2.0, size_xy / 2.0};
  std::vector<unsigned long long> state(312);
  for (int i = 0; i < n; i++) {
    Mt64<unsigned long long*> rng{state.data(), 1, 312};
    rng.seed(seed[i]);
    if (!world_start_goal_xy(rng, min_b, max_b, start3 + 3 * (size_t)i, goal3 + 3 * (size_t)i)) { set_err("topay_sample_start_goal_xy: no pair accepted"); return TOPAY_ERR_INVALID_ARG; }
  }
  return TOPAY_OK;
}

topay_status topay_sample_arm(topay_ctx* c, int n, const int* map_ids, const unsigned long long* seed, int max_tries, double* states, int* ok,
                              int* tries) {
  if (!c || n <= 0 || !seed || !states || !ok) return TOPAY_ERR_INVALID_ARG;
  topay_status s;
  if ((s = check_map_slots(c, n, map_ids, kMapResident, "topay_sample_arm")) != TOPAY_OK) return s;
  return world_sample_arm(c, n, map_ids, seed, max_tries, states, ok, tries, false);
}

topay_status topay_sample_scenarios(topay_ctx* c, int n, const int* map_ids, const unsigned long long* seed, double* start, double* goal, int* ok) {
  if (!c || n <= 0 || !seed || !start || !goal || !ok) return TOPAY_ERR_INVALID_ARG;
  topay_status s;
  if ((s = check_map_slots(c, n, map_ids, kMapResident, "topay_sample_scenarios")) != TOPAY_OK) return s;
  for (int i = 0; i < n; i++) {
    const DevMap& m = c->hmaps[map_ids ? map_ids[i] : 0];
    if (!world_fits_start_goal(m.max_b[0] - m.min_b[0]) || !world_fits_start_goal(m.max_b[1] - m.min_b[1])) {
      set_err("topay_sample_scenarios: the map is too small for a start and a goal 3 m apart");
      return TOPAY_ERR_INVALID_ARG;
    }
  }
  return world_sample_scenarios(c, n, map_ids, seed, start, goal, ok, false);
}

topay_status topay_generate_episodes(topay_ctx* c, int n, int first_map_id, const topay_world_params_t* params, const unsigned long long* seed,
                                     const int* attempt, double* start, double* goal, int* status) {
  if (!c || !params || !seed || !start || !goal || !status) return TOPAY_ERR_INVALID_ARG;
  topay_status s;
  if ((s = check_map_range(first_map_id, n, "topay_generate_episodes")) != TOPAY_OK) return s;
  if ((s = world_check_params(params)) != TOPAY_OK) return s;
  if (!world_fits_start_goal(params->size_xy)) { set_err("topay_generate_episodes: the map is too small for a start and a goal 3 m apart"); return TOPAY_ERR_INVALID_ARG; }
  const size_t N = (size_t)n;
  std::vector<unsigned long long> sd(N), arm_seed(2 * N);
  std::vector<double> keep, s3(3 * N), g3(3 * N);
  std::vector<int> mid(N);
  for (int i = 0; i < n; i++) {
    const unsigned long long at = (unsigned long long)(attempt ? attempt[i] : 0);
    sd[i] = params->kind == 0 ? seed[i] * 1000ULL + at : seed[i];
    arm_seed[i] = seed[i] * 7919ULL + 2ULL * at;           // the goal arm
    arm_seed[N + i] = seed[i] * 7919ULL + 2ULL * at + 1ULL; // the start arm
    mid[i] = first_map_id + i;
  }
  if (params->kind == 0) {
    if ((s = topay_sample_start_goal_xy(n, sd.data(), params->size_xy, s3.data(), g3.data())) != TOPAY_OK) return s;
    keep.resize(4 * N);
    for (size_t i = 0; i < N; i++) { keep[4 * i] = s3[3 * i]; keep[4 * i + 1] = s3[3 * i + 1]; keep[4 * i + 2] = g3[3 * i]; keep[4 * i + 3] = g3[3 * i + 1]; }
  }
  if ((s = world_generate(c, n, first_map_id, params, sd.data(), params->kind == 0 ? keep.data() : nullptr, nullptr, "topay_generate_episodes")) != TOPAY_OK) return s;
  if (params->kind == 1) return world_sample_scenarios(c, n, mid.data(), sd.data(), start, goal, status, true);
  // tables: both arms in one launch, goal states first (instances i and n + i share map i)
  std::vector<double> st(20 * N, 0.0);
  std::vector<int> mid2(2 * N), ok(2 * N);
  for (size_t i = 0; i < N; i++) {
    for (int k = 0; k < 3; k++) { st[10 * i + k] = g3[3 * i + k]; st[10 * (N + i) + k] = s3[3 * i + k]; }
    mid2[i] = mid2[N + i] = mid[i];
  }
  if ((s = world_sample_arm(c, 2 * n, mid2.data(), arm_seed.data(), c->world.max_tries, st.data(), ok.data(), nullptr, true)) != TOPAY_OK) return s;
  for (size_t i = 0; i < N; i++) {
    for (int k = 0; k < 10; k++) { goal[10 * i + k] = st[10 * i + k]; start[10 * i + k] = st[10 * (N + i) + k]; }
    status[i] = ok[i] && ok[N + i] ? 1 : 0;
  }
  return TOPAY_OK;
}

topay_status topay_test_mt64(unsigned long long seed, int skip, int n, unsigned long long* out) {
  if (skip < 0 || n <= 0 || !out) return TOPAY_ERR_INVALID_ARG;
  DevBuf d;
  topay_status s;
  if ((s = d.ensure((size_t)n * 8)) != TOPAY_OK) return s;
  hipLaunchKernelGGL(k_world_mt64, dim3(1), dim3(TOPAY_WAVE), 312 * 8, (hipStream_t) nullptr, seed, skip, n, d.as<unsigned long long>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, d.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return TOPAY_OK;
}

}  // extern "C"
