// Host side of the C-ABI, part 11: sensor clouds into the map (topay_sense.h) -- the beliefs of the map slots, insertion, the
// hand-over of the derived occupancy grids to the field construction (topay_host_maps.h), the range sensor.

#pragma once

// logit of config.hpp:229: the quotient in float, its logarithm in double, rounded to float
static float sense_logit(float x) { return (float)std::log((double)(x / (1.0f - x))); }

static topay_status sense_make_params(const topay_sense_params_t* p, SenseP& P) {
  const float pr[6] = {p->p_hit, p->p_miss, p->p_min, p->p_max, p->p_occ, p->p_free};
  for (float v : pr)
    if (!(v > 0.0f && v < 1.0f)) { set_err("topay_sense: a probability outside (0, 1)"); return TOPAY_ERR_INVALID_ARG; }
  if (!(p->ray_range[0] >= 0.0) || !(p->ray_range[1] > 0.0) || !(p->ray_range[1] <= 1.0e6) || !(p->ray_range[0] <= p->ray_range[1])) {
    set_err("topay_sense: ray_range must be 0 <= min <= max, 0 < max <= 1e6");
    return TOPAY_ERR_INVALID_ARG;
  }
  if (p->ray_range[0] > 0.0) {
    set_err("topay_sense: ray_range[0] > 0 needs the first-frame clearing of prob_map.cpp:356-372, which is not restated");
    return TOPAY_ERR_UNSUPPORTED;
  }
  if (!(p->virtual_ground_height <= p->virtual_ceil_height) || !(p->chassis_height == p->chassis_height)) return TOPAY_ERR_INVALID_ARG;
  memset(&P, 0, sizeof(P));
  P.l_hit = sense_logit(p->p_hit); P.l_miss = sense_logit(p->p_miss); P.l_min = sense_logit(p->p_min);
  P.l_max = sense_logit(p->p_max); P.l_occ = sense_logit(p->p_occ); P.l_free = sense_logit(p->p_free);
  P.range_min = p->ray_range[0]; P.range_max = p->ray_range[1];
  P.sqr_range_max = P.range_max * P.range_max;   // config.hpp:212
  P.ceil_height = p->virtual_ceil_height; P.ground_height = p->virtual_ground_height;
  P.filt = p->point_filt_num > 0 ? p->point_filt_num : 1;   // config.hpp:180-184
  P.thresh = p->intensity_thresh;
  return TOPAY_OK;
}
// half_local_update_box_i = (local_update_box_d / 2 / resolution).cast<int>() (config.hpp:378-379)
static topay_status sense_half_box(const topay_sense_params_t* p, double res, SenseP& P) {
  for (int a = 0; a < 3; a++) {
    const double h = p->local_update_box[a] / 2 / res;
    if (!(h >= 0.0) || !(h < 1.0e9)) { set_err("topay_sense: local_update_box out of range"); return TOPAY_ERR_INVALID_ARG; }
    P.half_box[a] = (int)h;
  }
  return TOPAY_OK;
}
// every slot of a call has a belief (the slots are in range: check_map_slots)
static topay_status sense_check_beliefs(topay_ctx* c, int n, const int* map_ids, const char* who) {
  for (int k = 0; k < n; k++)
    if (!c->sense.has_belief(map_ids[k])) { set_err(std::string(who) + ": slot " + std::to_string(map_ids[k]) + " without a belief (topay_sense_reset)"); return TOPAY_ERR_NO_MAP; }
  return TOPAY_OK;
}

// What topay_sense_slide does to one slot, from its descriptor and the sensor (include/topay.h, "Sliding sensor map"): the sensor's
// voxel v with the inserter's expression, the centre voxel c = dims / 2, the shift v - c on the sliding axes, and the trigger of
// prob_map.cpp:324-326 with local_map_origin_d_ the LOW CORNER of the centre voxel (sliding_map.cpp:118).  A sensor whose voxel is
// outside the window slides whatever the threshold (prob_map.cpp:306-311).  false: a voxel index beyond an int.
struct SenseSlide { int status, shift[3]; };
static bool sense_slide_decide(const topay_map_desc_t& g, const double* sensor, double threshold, bool slide_z, bool batch_open, SenseSlide& D) {
  D.status = 0;
  D.shift[0] = D.shift[1] = D.shift[2] = 0;
  const double res_inv = 1.0 / g.resolution;
  const int axes = slide_z ? 3 : 2;
  double sq = 0.0;
  bool outside = false;
  for (int a = 0; a < axes; a++) {
    const double u = sensor[a] - g.origin[a];
    const double vf = floor(u * res_inv);
    if (!(std::fabs(vf) <= 1.0e9)) return false;
    const int v = (int)vf, cv = g.dims[a] / 2;
    D.shift[a] = v - cv;
    outside = outside || v < 0 || v >= g.dims[a];
    const double d = u - (double)cv * g.resolution;
    sq = a == 0 ? d * d : sq + d * d;
  }
  if (batch_open) D.status = -1;   // batch_update_counter == 0 is the condition of both slides
  else if (outside) D.status = 2;
  else if (sqrt(sq) > threshold) D.status = 1;
  return true;
}

extern "C" {

topay_status topay_sense_default_params(topay_sense_params_t* p) {
  if (!p) return TOPAY_ERR_INVALID_ARG;
  memset(p, 0, sizeof(*p));
  // src/planner/params/rog_map.yaml
  p->p_min = 0.12f; p->p_miss = 0.49f; p->p_free = 0.499f; p->p_occ = 0.85f; p->p_hit = 0.9f; p->p_max = 0.98f;
  p->ray_range[0] = 0.0; p->ray_range[1] = 5.0;
  p->point_filt_num = 15; p->batch_update_size = 1; p->intensity_thresh = -10;
  p->virtual_ceil_height = 9999.0; p->virtual_ground_height = -9999.0;
  p->local_update_box[0] = 50.0; p->local_update_box[1] = 50.0; p->local_update_box[2] = 5.0;
  p->chassis_height = 0.155;   // moma_param.h
  return TOPAY_OK;
}

topay_status topay_sense_logodds(const topay_sense_params_t* p, float* l6) {
  if (!p || !l6) return TOPAY_ERR_INVALID_ARG;
  SenseP P;
  if (topay_status s = sense_make_params(p, P)) return s;
  l6[0] = P.l_hit; l6[1] = P.l_miss; l6[2] = P.l_min; l6[3] = P.l_max; l6[4] = P.l_occ; l6[5] = P.l_free;
  return TOPAY_OK;
}

topay_status topay_sense_reset(topay_ctx* c, int n, const int* map_ids, const topay_map_desc_t* desc) {
  if (!c || n <= 0 || !map_ids || !desc || !(desc->resolution > 0.0)) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_map_slots(c, n, map_ids, kMapOnce, "topay_sense_reset")) return s;
  if (topay_status s = map_dims_check(desc)) return s;
  HIPCHK(hipSetDevice(c->device));
  if (c->sense.slot.empty()) c->sense.slot.resize(TOPAY_MAX_MAPS);
  const size_t n3 = (size_t)desc->dims[0] * desc->dims[1] * desc->dims[2];
  const int empty_box[6] = {0x7f7f7f7f, 0x7f7f7f7f, 0x7f7f7f7f, 0x7f7f7f7f, 0x7f7f7f7f, 0x7f7f7f7f};
  for (int k = 0; k < n; k++) {
    SenseBelief& b = c->sense.slot[map_ids[k]];
    b.have = false;
    auto lay = [&](Carver& q) { b.logodds = q.take<float>(n3); b.cnt = q.take<int>(n3); b.box = q.take<int>(8); };
    if (topay_status s = b.buf.carve(lay)) return s;
    HIPCHK(hipMemsetAsync(b.logodds, 0, n3 * 8, c->stream));   // log-odds 0 (prob_map.cpp:78) and the counts behind them
    HIPCHK(h2d(c, b.box, empty_box, 6));
    b.desc = *desc;
    topay_sense_default_params(&b.prm);
    b.prm.chassis_height = c->hp.chassis_height;
    b.batch_counter = 0; b.pending_rays = 0;
    b.have = true;
  }
  HIPCHK(hipStreamSynchronize(c->stream));   // (empty_box is on this stack)
  return TOPAY_OK;
}

topay_status topay_sense_insert(topay_ctx* c, int n, const int* map_ids, const int* cloud_off, const float* points_xyzi, const double* sensor_pos,
                                const topay_sense_params_t* params, int* status) {
  if (!c || n <= 0 || !map_ids || !cloud_off || !sensor_pos || !params) return TOPAY_ERR_INVALID_ARG;
  topay_status s;
  if ((s = check_map_slots(c, n, map_ids, kMapOnce, "topay_sense_insert")) != TOPAY_OK) return s;
  SenseP P;
  if ((s = sense_make_params(params, P)) != TOPAY_OK) return s;
  const int batch_size = params->batch_update_size > 0 ? params->batch_update_size : 1;   // config.hpp:190-194
  const bool from_scan = points_xyzi == TOPAY_SENSE_LAST_SCAN;
  if (cloud_off[0] < 0) return TOPAY_ERR_INVALID_ARG;
  for (int k = 0; k < n; k++)
    if (cloud_off[k + 1] < cloud_off[k]) return TOPAY_ERR_INVALID_ARG;
  const size_t total = (size_t)cloud_off[n];
  if (total > 0 && !points_xyzi) return TOPAY_ERR_INVALID_ARG;
  if (from_scan && total > c->sense.scan_points) { set_err("topay_sense_insert: offsets beyond the points of the last topay_sense_scan"); return TOPAY_ERR_INVALID_ARG; }
  if ((s = sense_check_beliefs(c, n, map_ids, "topay_sense_insert")) != TOPAY_OK) return s;
  // per slot: the descriptor, the rays this cloud can add to the batch, the voxel box a flush has to cover
  std::vector<SenseSlot> hs((size_t)n);
  std::vector<int> h_nsurv((size_t)n), st((size_t)n, 0);
  int max_rays = 0, max_len = 0;
  long long max_fvol = 0;
  bool any_flush = false;
  for (int k = 0; k < n; k++) {
    SenseBelief& b = c->sense.slot[map_ids[k]];
    SenseSlot& S = hs[(size_t)k];
    memset(&S, 0, sizeof(S));
    if (k == 0) { if ((s = sense_half_box(params, b.desc.resolution, P)) != TOPAY_OK) return s; }
    else if (b.desc.resolution != c->sense.slot[map_ids[0]].desc.resolution) { set_err("topay_sense_insert: the slots of a call share one resolution"); return TOPAY_ERR_INVALID_ARG; }
    const double* sp = sensor_pos + 3 * (size_t)k;
    for (int a = 0; a < 3; a++) {
      if (!(std::fabs(sp[a] - b.desc.origin[a]) <= 1.0e6)) { set_err("topay_sense_insert: sensor position not finite or more than 1e6 m from the map"); return TOPAY_ERR_INVALID_ARG; }
      S.origin[a] = b.desc.origin[a]; S.dims[a] = b.desc.dims[a]; S.sensor[a] = sp[a];
    }
    S.res = b.desc.resolution; S.res_inv = 1.0 / b.desc.resolution;
    S.logodds = b.logodds; S.cnt = b.cnt; S.box = b.box;
    S.cloud_begin = cloud_off[k]; S.cloud_len = cloud_off[k + 1] - cloud_off[k];
    if (sp[2] > params->virtual_ceil_height) st[(size_t)k] = -1;
    else if (sp[2] < params->virtual_ground_height) st[(size_t)k] = -2;
    S.skip = st[(size_t)k] < 0;
    const int rays = S.skip ? 0 : (S.cloud_len + P.filt - 1) / P.filt;
    if (b.pending_rays + rays > TOPAY_SENSE_MAX_BATCH_RAYS) {
      set_err("topay_sense_insert: slot " + std::to_string(map_ids[k]) + " would count more than " + std::to_string(TOPAY_SENSE_MAX_BATCH_RAYS) +
              " rays in one batch (16-bit counts per voxel)");
      return TOPAY_ERR_INVALID_ARG;
    }
    h_nsurv[(size_t)k] = rays;
    max_rays = std::max(max_rays, rays);
    max_len = std::max(max_len, S.skip ? 0 : S.cloud_len);
  }
  // What the call does to each slot's host state, worked out beside it: nothing of a slot moves before every check, allocation
  // and upload of the call has succeeded.
  struct Next { int batch_counter, pending_rays; };
  std::vector<Next> nx((size_t)n);
  long long max_vol = 0;   // the largest grid of the call: no cache box is larger
  for (int k = 0; k < n; k++) {
    const SenseBelief& b = c->sense.slot[map_ids[k]];
    SenseSlot& S = hs[(size_t)k];
    Next& N = nx[(size_t)k];
    N.batch_counter = b.batch_counter; N.pending_rays = b.pending_rays;
    if (S.skip) continue;
    N.pending_rays += h_nsurv[(size_t)k];
    N.batch_counter++;
    if (N.batch_counter >= batch_size) {   // prob_map.cpp:340-341
      N.batch_counter = 0;
      N.pending_rays = 0;
      S.flush = 1;
      st[(size_t)k] = 1;
      max_vol = std::max(max_vol, (long long)S.dims[0] * S.dims[1] * S.dims[2]);
      any_flush = true;
    }
  }
  if ((long long)n * ((max_vol + TOPAY_SENSE_BLOCK - 1) / TOPAY_SENSE_BLOCK) >= (1ll << 31)) { set_err("topay_sense_insert: flush launch too large"); return TOPAY_ERR_UNSUPPORTED; }
  HIPCHK(hipSetDevice(c->device));
  DevTimer* tm = c->sense.timer;
  const bool select = P.thresh > 0 && max_len > 0;
  SenseSlot* d_slots; int *d_nsurv, *d_surv, *d_boxes;
  auto lay = [&](Carver& q) {
    d_slots = q.take<SenseSlot>((size_t)n); d_nsurv = q.take<int>((size_t)n); d_boxes = q.take<int>(6 * (size_t)n); d_surv = q.take<int>(select ? total : 1);
  };
  if ((s = c->sense.io.carve(lay)) != TOPAY_OK) return s;
  const SensePoint* d_pts = nullptr;
  if (from_scan) d_pts = c->sense.scan.as<SensePoint>();
  else if (total > 0) {
    if ((s = c->sense.pts.ensure(total * sizeof(SensePoint))) != TOPAY_OK) return s;
    HIPCHK(h2d(c, c->sense.pts.as<float>(), points_xyzi, total * 4));
    d_pts = c->sense.pts.as<SensePoint>();
  }
  HIPCHK(h2d(c, d_slots, (const SenseSlot*)hs.data(), (size_t)n));
  HIPCHK(h2d(c, d_nsurv, (const int*)h_nsurv.data(), (size_t)n));
  HIPCHK(tm[SenseState::kInsert].start(c->stream));
  for (int k = 0; k < n; k++) {   // the launches follow: the slots' host state moves with them
    if (hs[(size_t)k].skip) continue;
    SenseBelief& b = c->sense.slot[map_ids[k]];
    const Next& N = nx[(size_t)k];
    b.prm = *params;
    b.batch_counter = N.batch_counter; b.pending_rays = N.pending_rays;
  }
  if (max_rays > 0) {
    if (select) hipLaunchKernelGGL(k_sense_select, dim3((unsigned)n), dim3(TOPAY_SENSE_BLOCK), 0, c->stream, P, (const SenseSlot*)d_slots, d_pts, d_surv, d_nsurv);
    const int bps = (max_rays + TOPAY_SENSE_BLOCK - 1) / TOPAY_SENSE_BLOCK;
    hipLaunchKernelGGL(k_sense_rays, dim3((unsigned)((size_t)n * bps)), dim3(TOPAY_SENSE_BLOCK), 0, c->stream, P, (const SenseSlot*)d_slots, bps, d_pts,
                       select ? (const int*)d_surv : (const int*)nullptr, (const int*)d_nsurv);
  }
  // The voxels a flush has to cover are the batch's cache box, which the rays of this and the batch's earlier calls have reduced on
  // the device: whatever path a ray took (a traversal that steps past its end voxel on a tie runs on to the map's edge, as the
  // reference's does), a voxel with a count lies in it.  The boxes come back with the wait that ends the insert stage.
  std::vector<int> h_boxes(6 * (size_t)n, 0x7f7f7f7f);
  if (any_flush) {
    hipLaunchKernelGGL(k_sense_box_gather, dim3((unsigned)((n * 6 + 255) / 256)), dim3(256), 0, c->stream, (const SenseSlot*)d_slots, n, d_boxes);
    HIPCHK(d2h(c, h_boxes.data(), (const int*)d_boxes, 6 * (size_t)n));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(tm[SenseState::kInsert].stop(c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(tm[SenseState::kInsert].read(&c->sense.ms[SenseState::kInsert]));
  for (int k = 0; k < n; k++) {
    const int* bx = h_boxes.data() + 6 * (size_t)k;
    if (!hs[(size_t)k].flush || bx[0] == 0x7f7f7f7f) continue;
    long long vol = 1;
    for (int a = 0; a < 3; a++) vol *= (long long)(-bx[3 + a]) - bx[a] + 1;
    max_fvol = std::max(max_fvol, vol);
  }
  max_fvol = std::min(max_fvol, max_vol);   // (a box lies inside its grid: the launch size checked above holds)
  const long long fbps = (max_fvol + TOPAY_SENSE_BLOCK - 1) / TOPAY_SENSE_BLOCK;
  HIPCHK(tm[SenseState::kFlush].start(c->stream));
  if (any_flush) {
    if (max_fvol > 0) {
      hipLaunchKernelGGL(k_sense_flush, dim3((unsigned)((long long)n * fbps)), dim3(TOPAY_SENSE_BLOCK), 0, c->stream, P, (const SenseSlot*)d_slots, (int)fbps);
    }
    hipLaunchKernelGGL(k_sense_box_reset, dim3((unsigned)((n * 6 + 255) / 256)), dim3(256), 0, c->stream, (const SenseSlot*)d_slots, n);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(tm[SenseState::kFlush].stop(c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(tm[SenseState::kFlush].read(&c->sense.ms[SenseState::kFlush]));
  if (status) memcpy(status, st.data(), sizeof(int) * (size_t)n);
  return TOPAY_OK;
}

topay_status topay_sense_commit(topay_ctx* c, int n, const int* map_ids) {
  if (!c || n <= 0 || !map_ids) return TOPAY_ERR_INVALID_ARG;
  topay_status s;
  if ((s = check_map_slots(c, n, map_ids, kMapOnce, "topay_sense_commit")) != TOPAY_OK) return s;
  if ((s = sense_check_beliefs(c, n, map_ids, "topay_sense_commit")) != TOPAY_OK) return s;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;   // inputs of a solve in flight stay untouched
  DevTimer& tm = c->sense.timer[SenseState::kCommit];
  // Runs of consecutive slots on one grid go through the field construction together (its launches take a batch of maps).  Under
  // the lane emulator a run stays one slot: an emulator that walks the blocks of a launch along x only (blockIdx.y = map stays 0)
  // would build the first map of a run alone.  The batched construction is checked in tests/test_edt_exact.py.
#ifdef TOPAY_CPU_EMU
  const int max_run = 1;
#else
  const int max_run = TOPAY_MAX_MAPS;
#endif
  std::vector<int> ids(map_ids, map_ids + n);
  std::sort(ids.begin(), ids.end());
  struct Run { int first, n; size_t o3, o2, o2c; };
  std::vector<Run> runs;
  size_t bytes = 0;
  auto same_grid = [](const topay_map_desc_t& a, const topay_map_desc_t& b) {
    bool eq = a.resolution == b.resolution;
    for (int i = 0; i < 3; i++)
      eq = eq && a.origin[i] == b.origin[i] && a.dims[i] == b.dims[i] && a.min_boundary[i] == b.min_boundary[i] && a.max_boundary[i] == b.max_boundary[i];
    return eq;
  };
  for (int k = 0; k < n;) {
    int e = k + 1;
    while (e < n && e - k < max_run && ids[e] == ids[e - 1] + 1 && same_grid(c->sense.slot[ids[e]].desc, c->sense.slot[ids[k]].desc)) e++;
    const topay_map_desc_t& d = c->sense.slot[ids[k]].desc;
    const size_t n2 = (size_t)d.dims[0] * d.dims[1], n3 = n2 * d.dims[2], R = (size_t)(e - k);
    Run r{ids[k], e - k, bytes, 0, 0};
    bytes += (R * n3 + 15) & ~(size_t)15;   // (each grid starts on a 16-byte boundary: k_sense_occupancy's 16-byte stores)
    r.o2 = bytes; bytes += (R * n2 + 15) & ~(size_t)15;
    r.o2c = bytes; bytes += (R * n2 + 15) & ~(size_t)15;
    runs.push_back(r);
    k = e;
  }
  c->sense.forget(0, TOPAY_MAX_MAPS);   // the grids of the last commit are overwritten
  if ((s = c->sense.occ.ensure(bytes)) != TOPAY_OK) return s;
  signed char* base = c->sense.occ.as<signed char>();
  std::vector<SenseOccSlot> ho((size_t)n);
  int max_cols = 0, at = 0;
  for (const Run& r : runs)
    for (int i = 0; i < r.n; i++, at++) {
      SenseBelief& b = c->sense.slot[r.first + i];
      const size_t n2 = (size_t)b.desc.dims[0] * b.desc.dims[1], n3 = n2 * b.desc.dims[2];
      SenseP P;
      if ((s = sense_make_params(&b.prm, P)) != TOPAY_OK) return s;
      b.occ3_off = r.o3 + (size_t)i * n3; b.occ2_off = r.o2 + (size_t)i * n2; b.occ2c_off = r.o2c + (size_t)i * n2;
      SenseOccSlot& S = ho[(size_t)at];
      S.logodds = b.logodds; S.occ3 = base + b.occ3_off; S.occ2 = base + b.occ2_off; S.occ2c = base + b.occ2c_off;
      S.z0 = b.desc.origin[2]; S.res = b.desc.resolution; S.chassis_height = b.prm.chassis_height; S.l_occ = P.l_occ;
      for (int a = 0; a < 3; a++) S.dims[a] = b.desc.dims[a];
      max_cols = std::max(max_cols, (int)n2);
    }
  if ((s = c->sense.io.ensure(sizeof(SenseOccSlot) * (size_t)n)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, c->sense.io.as<SenseOccSlot>(), (const SenseOccSlot*)ho.data(), (size_t)n));
  HIPCHK(tm.start(c->stream));
  const int bps = (max_cols + TOPAY_SENSE_BLOCK - 1) / TOPAY_SENSE_BLOCK;
  hipLaunchKernelGGL(k_sense_occupancy, dim3((unsigned)((size_t)n * bps)), dim3(TOPAY_SENSE_BLOCK), 0, c->stream, (const SenseOccSlot*)c->sense.io.as<SenseOccSlot>(), bps);
  HIPCHK(hipGetLastError());
  for (const Run& r : runs) {
    forget_occupancy(c, r.first, r.n);
    if ((s = build_fields_from_device(c, r.n, r.first, &c->sense.slot[r.first].desc, base + r.o3, base + r.o2, base + r.o2c, false)) != TOPAY_OK) return s;
    for (int i = 0; i < r.n; i++) c->sense.slot[r.first + i].have_occ = true;
  }
  HIPCHK(tm.stop(c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(tm.read(&c->sense.ms[SenseState::kCommit]));
  return TOPAY_OK;
}

topay_status topay_sense_get(topay_ctx* c, int map_id, float* logodds, int* op_cnt, int* hit_cnt, int* batch_counter) {
  if (!c) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_map_slots(c, 1, &map_id, 0, "topay_sense_get")) return s;
  if (topay_status s = sense_check_beliefs(c, 1, &map_id, "topay_sense_get")) return s;
  HIPCHK(hipSetDevice(c->device));
  const SenseBelief& b = c->sense.slot[map_id];
  const size_t n3 = (size_t)b.desc.dims[0] * b.desc.dims[1] * b.desc.dims[2];
  if (logodds) HIPCHK(d2h_sync(c, logodds, (const float*)b.logodds, n3));
  if (op_cnt || hit_cnt) {
    std::vector<int> packed(n3);
    HIPCHK(d2h_sync(c, packed.data(), (const int*)b.cnt, n3));
    for (size_t i = 0; i < n3; i++) {
      if (op_cnt) op_cnt[i] = (int)((unsigned)packed[i] & 0xffffu);
      if (hit_cnt) hit_cnt[i] = (int)((unsigned)packed[i] >> 16);
    }
  }
  if (batch_counter) *batch_counter = b.batch_counter;
  return TOPAY_OK;
}

topay_status topay_sense_scan(topay_ctx* c, int n, const int* truth_map_ids, const double* poses, int n_az, int n_el, double fov, double range,
                              int cloud_cap, int* cloud_off, float* points) {
  if (!c || n <= 0 || !truth_map_ids || !poses || n_az <= 0 || n_el <= 0 || !(range > 0.0) || !(range <= 1.0e6) || !(std::fabs(fov) <= 3.2))
    return TOPAY_ERR_INVALID_ARG;
  const long long rays = (long long)n_az * n_el, total = rays * n;
  if (rays > (1 << 24) || total >= (1ll << 31) / 16) { set_err("topay_sense_scan: too many rays"); return TOPAY_ERR_INVALID_ARG; }
  if (points && (long long)cloud_cap < total) { set_err("topay_sense_scan: cloud_cap below n * n_az * n_el"); return TOPAY_ERR_INVALID_ARG; }
  if (topay_status cs = check_map_slots(c, n, truth_map_ids, kMapResident, "topay_sense_scan")) return cs;
  std::vector<SenseScanSlot> hs((size_t)n);
  for (int k = 0; k < n; k++) {
    const int m = truth_map_ids[k];
    SenseScanSlot& S = hs[(size_t)k];
    memset(&S, 0, sizeof(S));
    S.occ3 = c->sense.has_occ(m) ? c->sense.occ3_of(m, S.dims) : c->world.occ3_of(m, S.dims);   // the last commit's grid, or the world generator's
    if (!S.occ3) { set_err("topay_sense_scan: slot " + std::to_string(m) + " has no resident occupancy (topay_get_occupancy)"); return TOPAY_ERR_NO_MAP; }
    const DevMap& M = c->hmaps[m];
    for (int a = 0; a < 3; a++) S.origin[a] = M.origin[a];
    S.res = M.res;
    for (int a = 0; a < 4; a++) {
      S.pose[a] = poses[4 * (size_t)k + a];
      if (!(std::fabs(S.pose[a] - (a < 3 ? S.origin[a] : 0.0)) <= 1.0e6)) { set_err("topay_sense_scan: pose not finite or more than 1e6 m from the map"); return TOPAY_ERR_INVALID_ARG; }
    }
  }
  HIPCHK(hipSetDevice(c->device));
  topay_status s;
  DevTimer& tm = c->sense.timer[SenseState::kScan];
  c->sense.scan_points = 0;
  if ((s = c->sense.scan.ensure((size_t)total * sizeof(SensePoint))) != TOPAY_OK) return s;
  if ((s = c->sense.io.ensure(sizeof(SenseScanSlot) * (size_t)n)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, c->sense.io.as<SenseScanSlot>(), (const SenseScanSlot*)hs.data(), (size_t)n));
  HIPCHK(tm.start(c->stream));
  const int bps = (int)((rays + TOPAY_SENSE_BLOCK - 1) / TOPAY_SENSE_BLOCK);
  hipLaunchKernelGGL(k_sense_scan, dim3((unsigned)((size_t)n * bps)), dim3(TOPAY_SENSE_BLOCK), 0, c->stream, (const SenseScanSlot*)c->sense.io.as<SenseScanSlot>(), bps,
                     n_az, n_el, fov, range, c->sense.scan.as<SensePoint>());
  HIPCHK(hipGetLastError());
  HIPCHK(tm.stop(c->stream));
  if (points) HIPCHK(d2h(c, points, (const float*)c->sense.scan.as<float>(), (size_t)total * 4));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->sense.scan_points = (size_t)total;
  if (cloud_off)
    for (int k = 0; k <= n; k++) cloud_off[k] = (int)(rays * k);
  HIPCHK(tm.read(&c->sense.ms[SenseState::kScan]));
  return TOPAY_OK;
}

topay_status topay_sense_ms(topay_ctx* c, double ms[4]) {
  if (!c || !ms) return TOPAY_ERR_INVALID_ARG;
  for (int k = 0; k < 4; k++) ms[k] = c->sense.ms[k];
  return TOPAY_OK;
}

topay_status topay_sense_slide_default_params(topay_sense_slide_params_t* p) {
  if (!p) return TOPAY_ERR_INVALID_ARG;
  memset(p, 0, sizeof(*p));
  p->threshold = 0.3;   // params/rog_map.yaml map_sliding/threshold
  p->slide_z = 0;
  return TOPAY_OK;
}

topay_status topay_sense_slide(topay_ctx* c, int n, const int* map_ids, const double* sensor_pos, const topay_sense_slide_params_t* params, int* status,
                               int* shift) {
  if (!c || n <= 0 || !map_ids || !sensor_pos) return TOPAY_ERR_INVALID_ARG;
  topay_status s;
  if ((s = check_map_slots(c, n, map_ids, kMapOnce, "topay_sense_slide")) != TOPAY_OK) return s;
  topay_sense_slide_params_t prm;
  topay_sense_slide_default_params(&prm);
  if (params) prm = *params;
  if (!(prm.threshold >= 0.0) || !(prm.threshold <= 1.7976931348623157e308)) { set_err("topay_sense_slide: threshold negative or not finite"); return TOPAY_ERR_INVALID_ARG; }
  if ((s = sense_check_beliefs(c, n, map_ids, "topay_sense_slide")) != TOPAY_OK) return s;
  // the decisions, slot by slot; nothing of a slot moves before every check, allocation and upload of the call has succeeded
  std::vector<SenseSlide> dec((size_t)n);
  std::vector<SenseSlideSlot> rows;
  std::vector<int> row_slot;
  size_t floats = 0;
  int max_cols = 0;
  for (int k = 0; k < n; k++) {
    const SenseBelief& b = c->sense.slot[map_ids[k]];
    const double* sp = sensor_pos + 3 * (size_t)k;
    for (int a = 0; a < 3; a++)
      if (!(std::fabs(sp[a] - b.desc.origin[a]) <= 1.0e6)) { set_err("topay_sense_slide: sensor position not finite or more than 1e6 m from the map"); return TOPAY_ERR_INVALID_ARG; }
    SenseSlide& D = dec[(size_t)k];
    if (!sense_slide_decide(b.desc, sp, prm.threshold, prm.slide_z != 0, b.batch_counter != 0, D)) {
      set_err("topay_sense_slide: the sensor's voxel index does not fit an int at this resolution");
      return TOPAY_ERR_INVALID_ARG;
    }
    if (D.status <= 0 || (D.shift[0] == 0 && D.shift[1] == 0 && D.shift[2] == 0)) continue;   // nothing to move
    SenseSlideSlot R;
    memset(&R, 0, sizeof(R));
    R.src = b.logodds;
    for (int a = 0; a < 3; a++) {   // (a shift of dims or more clears everything, and so does one of exactly dims)
      R.dims[a] = b.desc.dims[a];
      R.shift[a] = std::max(-b.desc.dims[a], std::min(b.desc.dims[a], D.shift[a]));
    }
    rows.push_back(R);
    row_slot.push_back(k);
    floats += ((size_t)R.dims[0] * R.dims[1] * R.dims[2] + 3) & ~(size_t)3;   // (each image starts on a 16-byte boundary)
    max_cols = std::max(max_cols, R.dims[0] * R.dims[1]);
  }
  const size_t nr = rows.size();
  const int bps = (max_cols + TOPAY_SENSE_BLOCK - 1) / TOPAY_SENSE_BLOCK;
  if ((long long)nr * bps >= (1ll << 31)) { set_err("topay_sense_slide: launch too large"); return TOPAY_ERR_UNSUPPORTED; }
  HIPCHK(hipSetDevice(c->device));
  DevTimer& tm = c->sense.slide_timer;
  if (nr > 0) {
    if ((s = c->sense.slide.ensure(floats * sizeof(float))) != TOPAY_OK) return s;
    if ((s = c->sense.io.ensure(sizeof(SenseSlideSlot) * nr)) != TOPAY_OK) return s;
    float* at = c->sense.slide.as<float>();
    for (SenseSlideSlot& R : rows) { R.dst = at; at += ((size_t)R.dims[0] * R.dims[1] * R.dims[2] + 3) & ~(size_t)3; }
    HIPCHK(h2d(c, c->sense.io.as<SenseSlideSlot>(), (const SenseSlideSlot*)rows.data(), nr));
  }
  HIPCHK(tm.start(c->stream));
  if (nr > 0) {
    hipLaunchKernelGGL(k_sense_slide, dim3((unsigned)(nr * bps)), dim3(TOPAY_SENSE_BLOCK), 0, c->stream, (const SenseSlideSlot*)c->sense.io.as<SenseSlideSlot>(), bps);
    HIPCHK(hipGetLastError());
    for (const SenseSlideSlot& R : rows)   // the image back into the belief, on the same stream
      HIPCHK(hipMemcpyAsync((void*)R.src, R.dst, sizeof(float) * (size_t)R.dims[0] * R.dims[1] * R.dims[2], hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(tm.stop(c->stream));
  for (int k = 0; k < n; k++) {   // the descriptor is the one statement of the grid: it moves with the launches
    const SenseSlide& D = dec[(size_t)k];
    if (D.status <= 0) continue;
    topay_map_desc_t& d = c->sense.slot[map_ids[k]].desc;
    for (int a = 0; a < 3; a++) {
      const double by = (double)D.shift[a] * d.resolution;
      d.origin[a] = d.origin[a] + by;
      d.min_boundary[a] = d.min_boundary[a] + by;
      d.max_boundary[a] = d.max_boundary[a] + by;
    }
  }
  HIPCHK(hipStreamSynchronize(c->stream));   // (rows is on this stack)
  HIPCHK(tm.read(&c->sense.slide_ms));
  for (int k = 0; k < n; k++) {
    if (status) status[k] = dec[(size_t)k].status;
    if (shift)
      for (int a = 0; a < 3; a++) shift[3 * (size_t)k + a] = dec[(size_t)k].status > 0 ? dec[(size_t)k].shift[a] : 0;
  }
  return TOPAY_OK;
}

topay_status topay_sense_slide_ms(topay_ctx* c, double* ms) {
  if (!c || !ms) return TOPAY_ERR_INVALID_ARG;
  *ms = c->sense.slide_ms;
  return TOPAY_OK;
}

topay_status topay_sense_get_desc(topay_ctx* c, int map_id, topay_map_desc_t* desc) {
  if (!c || !desc) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_map_slots(c, 1, &map_id, 0, "topay_sense_get_desc")) return s;
  if (topay_status s = sense_check_beliefs(c, 1, &map_id, "topay_sense_get_desc")) return s;
  *desc = c->sense.slot[map_id].desc;
  return TOPAY_OK;
}

}  // extern "C"
