// Host side of the C-ABI, part 2: the map slots -- the one check of the slots an entry names, upload, sharing between contexts,
// ESDF construction on the device.

#pragma once

// what every entry that fills a slot asks of a map's dimensions
static topay_status map_dims_check(const topay_map_desc_t* desc) {
  const size_t n2 = (size_t)desc->dims[0] * desc->dims[1], n3 = n2 * desc->dims[2];
  if (n2 == 0 || n3 == 0) return TOPAY_ERR_INVALID_ARG;
  if (n3 >= (1ull << 32)) { set_err("map of 2^32 cells or more (the lookups index a field with 32 bits)"); return TOPAY_ERR_UNSUPPORTED; }
  if (desc->dims[2] < 2) { set_err("3-D field with a single layer (the lookups fetch z-neighbours in pairs)"); return TOPAY_ERR_UNSUPPORTED; }
  return TOPAY_OK;
}

// What an entry asks of the map slots it names (check_map_slots).
enum : unsigned {
  kMapResident = 1,   // the slot is filled
  kMap2d = 2,         // ... and has the 2-D field
  kMap3d = 4,         // ... the 3-D field
  kMapFront = 8,      // ... the front-end's inflate and critical fields (a slot filled by topay_build_esdf*, not topay_set_map)
  kMapOnce = 16       // every slot is named once
};
// The one check of map slots: map_ids[0 .. n) (null: slot 0).  A slot out of range or named twice is TOPAY_ERR_INVALID_ARG, an
// empty one or one without a field TOPAY_ERR_NO_MAP; the error text names the entry (`who`) and the slot.
static topay_status check_map_slots(topay_ctx* c, int n, const int* map_ids, unsigned need, const char* who) {
  std::vector<char> seen(need & kMapOnce ? TOPAY_MAX_MAPS : 0, 0);
  for (int k = 0; k < (map_ids ? n : 1); k++) {
    const int m = map_ids ? map_ids[k] : 0;
    const std::string slot = std::string(who) + ": map slot " + std::to_string(m);
    if (m < 0 || m >= TOPAY_MAX_MAPS) { set_err(slot + " out of range"); return TOPAY_ERR_INVALID_ARG; }
    if (need & kMapOnce) {
      if (seen[m]) { set_err(slot + " named twice in one call"); return TOPAY_ERR_INVALID_ARG; }
      seen[m] = 1;
    }
    const DevMap& d = c->hmaps[m];
    const bool fields = ((need & kMap2d) && !d.esdf2d) || ((need & kMap3d) && !d.esdf3d);
    if (fields || ((need & kMapResident) && !c->have_map[m])) { set_err(slot + (need & (kMap2d | kMap3d) ? " has no fields" : " is not set")); return TOPAY_ERR_NO_MAP; }
    if ((need & kMapFront) && (!d.esdf2d_inflate || !d.esdf2d_critical)) {
      set_err(slot + " has no front-end fields (esdf_buffer_2d_inflate / _critical): fill it with topay_build_esdf_fields (or topay_build_esdf / _batch), "
              "not topay_set_map");
      return TOPAY_ERR_NO_MAP;
    }
  }
  return TOPAY_OK;
}
// ... and of a range of slots that an entry fills or takes over
static topay_status check_map_range(int first_map_id, int n_maps, const char* who) {
  if (n_maps > 0 && first_map_id >= 0 && first_map_id + n_maps <= TOPAY_MAX_MAPS) return TOPAY_OK;
  set_err(std::string(who) + ": map slots [" + std::to_string(first_map_id) + ", " + std::to_string(first_map_id) + " + " + std::to_string(n_maps) + ") out of range");
  return TOPAY_ERR_INVALID_ARG;
}

extern "C" {

topay_status topay_set_map(topay_ctx* c, int map_id, const topay_map_desc_t* desc, const double* esdf2d, const double* esdf3d) {
  if (!c || !desc || !esdf2d || !esdf3d) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_map_slots(c, 1, &map_id, 0, "topay_set_map")) return s;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;   // inputs of a solve in flight stay untouched
  const size_t n2 = (size_t)desc->dims[0] * desc->dims[1], n3 = n2 * desc->dims[2];
  if (topay_status ds = map_dims_check(desc)) return ds;
  invalidate_sharers(c, map_id, 1);
  drop_shared_slots(c, map_id, 1);
  forget_occupancy(c, map_id, 1);
  topay_status s;
  if ((s = c->map2d[map_id].ensure(n2 * 8)) != TOPAY_OK) return s;
  if ((s = c->map3d[map_id].ensure(n3 * 8)) != TOPAY_OK) return s;
  HIPCHK(h2d_sync(c, c->map2d[map_id].as<double>(), esdf2d, n2));
  HIPCHK(h2d_sync(c, c->map3d[map_id].as<double>(), esdf3d, n3));
  DevMap& m = c->hmaps[map_id];
  for (int i = 0; i < 3; i++) {
    m.origin[i] = desc->origin[i]; m.dims[i] = desc->dims[i];
    m.min_b[i] = desc->min_boundary[i]; m.max_b[i] = desc->max_boundary[i];
  }
  m.res = desc->resolution;
  m.res_inv = 1.0 / desc->resolution;  // grid_map.cpp:41
  m.esdf2d = (glb_cdp)c->map2d[map_id].as<double>();
  m.esdf3d = (glb_cdp)c->map3d[map_id].as<double>();
  m.esdf2d_inflate = nullptr;
  m.esdf2d_critical = nullptr;
  c->map2d_inf[map_id].release();
  c->map2d_crit[map_id].release();
  c->have_map[map_id] = 1;
  HIPCHK(memcpy_sync(c, (char*)c->dmaps.p + sizeof(DevMap) * map_id, &c->hmaps[map_id], sizeof(DevMap), hipMemcpyHostToDevice));
  return TOPAY_OK;
}

// Read-only map slots shared between the contexts of a device: `c` takes over the descriptors (device pointers) of the
// slots `owner` holds, without a copy of the fields.  The batches in flight of a pipelined planner (one context each)
// then keep one copy of the maps instead of one per context.
topay_status topay_share_maps(topay_ctx* c, topay_ctx* owner, int first_map_id, int n_maps) {
  if (!c || !owner || c == owner) return TOPAY_ERR_INVALID_ARG;
  if (topay_status s = check_map_range(first_map_id, n_maps, "topay_share_maps")) return s;
  if (c->device != owner->device) { set_err("topay_share_maps: the contexts are on different devices"); return TOPAY_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;
  for (int m = first_map_id; m < first_map_id + n_maps; m++)
    if (topay_status s = check_map_slots(owner, 1, &m, kMapResident, "topay_share_maps (the owner)")) return s;
  invalidate_sharers(c, first_map_id, n_maps);   // (contexts that shared c's own copies of these slots)
  drop_shared_slots(c, first_map_id, n_maps);
  forget_occupancy(c, first_map_id, n_maps);
  for (int m = first_map_id; m < first_map_id + n_maps; m++) {
    c->map2d[m].release(); c->map3d[m].release(); c->map2d_inf[m].release(); c->map2d_crit[m].release();   // own copies of these slots, if any
    c->hmaps[m] = owner->hmaps[m];
    c->have_map[m] = 1;
    // A slot that `owner` itself only shares is registered with the context that holds the fields (the root): it is the
    // root's refill / destroy that frees them, and its list of sharers is the one invalidate_sharers walks.
    topay_ctx* root = owner->map_owner[m] ? owner->map_owner[m] : owner;
    c->map_owner[m] = root;
    std::lock_guard<std::mutex> lk(g_registry_mutex);
    if (std::find(root->map_sharers.begin(), root->map_sharers.end(), c) == root->map_sharers.end()) root->map_sharers.push_back(c);
  }
  for (size_t i = 0; i < c->map_arenas.size();) {   // arenas of own builds that only held these slots
    topay_ctx::MapArena& a = c->map_arenas[i];
    if (a.first >= first_map_id && a.first + a.n <= first_map_id + n_maps) {
      a.buf.release();
      c->map_arenas.erase(c->map_arenas.begin() + (long)i);
    } else {
      i++;
    }
  }
  HIPCHK(memcpy_sync(c, (char*)c->dmaps.p + sizeof(DevMap) * first_map_id, &c->hmaps[first_map_id], sizeof(DevMap) * n_maps, hipMemcpyHostToDevice));
  return TOPAY_OK;
}

// ESDF construction on the device (GridMap::updateESDF, grid_map.cpp:125-521) from occupancy grids that already lie in device
// memory: d_occ3 [n_maps][nx*ny*nz], d_occ2 [n_maps][nx*ny] (points below the chassis height), d_occ2c [n_maps][nx*ny] (the
// critical grid; written here as the projection of d_occ3 when project_critical).  The body of topay_build_esdf_fields, which
// uploads the grids first, and of topay_generate_worlds (topay_host_world.h), whose rasteriser wrote them.  The grids are read
// only (d_occ2c apart) and stay the caller's.
static topay_status build_fields_from_device(topay_ctx* c, int n_maps, int first_map_id, const topay_map_desc_t* desc, signed char* d_occ3,
                                             signed char* d_occ2, signed char* d_occ2c, bool project_critical) {
  const int nx = desc->dims[0], ny = desc->dims[1], nz = desc->dims[2];
  const size_t n2 = (size_t)nx * ny, n3 = n2 * nz, M = (size_t)n_maps;
  if (topay_status ds = map_dims_check(desc)) return ds;
  invalidate_sharers(c, first_map_id, n_maps);
  drop_shared_slots(c, first_map_id, n_maps);
  topay_status s;
  if ((s = c->edt.thr.ensure(M * n2)) != TOPAY_OK) return s;
  signed char* d_occ2t = c->edt.thr.as<signed char>();   // 2-D scratch: the thresholded fields
  if ((s = c->edt.tmp1.ensure(M * n3 * 8)) != TOPAY_OK) return s;
  if ((s = c->edt.tmp2.ensure(M * n3 * 8)) != TOPAY_OK) return s;
  // results: e3 | e2 | e2 inflate | e2 critical in a new arena (they stay there); the plain critical field is scratch
  // (a rebuild of the same range of slots -- a new episode's maps -- takes the arena of the previous build over)
  // arenas of earlier builds whose slots this build overwrites completely are released (a caller that varies the slot
  // ranges would otherwise accumulate full-size arenas until topay_destroy)
  for (size_t i = 0; i < c->map_arenas.size();) {
    topay_ctx::MapArena& a = c->map_arenas[i];
    const bool same = a.first == first_map_id && a.n == n_maps;
    if (!same && a.first >= first_map_id && a.first + a.n <= first_map_id + n_maps) {
      a.buf.release();
      c->map_arenas.erase(c->map_arenas.begin() + (long)i);
    } else {
      i++;
    }
  }
  topay_ctx::MapArena* ar = nullptr;
  for (auto& a : c->map_arenas)
    if (a.first == first_map_id && a.n == n_maps) ar = &a;
  if (!ar) {
    c->map_arenas.emplace_back();
    ar = &c->map_arenas.back();
    ar->first = first_map_id;
    ar->n = n_maps;
  }
  DevBuf& arena = ar->buf;
  double *e3, *e2, *e2i, *e2c;   // e2i: inflate; e2c: critical (holds the critical-inflate field at the end, as the reference's buffer does)
  auto lay_arena = [&](Carver& k) {
    e3 = k.take<double>(M * n3); e2 = k.take<double>(M * n2); e2i = k.take<double>(M * n2); e2c = k.take<double>(M * n2);
  };
  if ((s = arena.carve(lay_arena)) != TOPAY_OK) return s;
  if ((s = c->edt.out2.ensure(M * n2 * 8)) != TOPAY_OK) return s;
  // workspace for the envelope stacks of the pass with the most (lines x cells), per map
  const size_t ws_elems = std::max(std::max((size_t)nx * ny * (nz + 2), (size_t)nx * nz * (ny + 2)), (size_t)ny * nz * (nx + 2));
  if ((s = c->edt.v.ensure(M * ws_elems * 4)) != TOPAY_OK) return s;
  if ((s = c->edt.z.ensure(M * ws_elems * 8)) != TOPAY_OK) return s;
  HIPCHK(c->edt.timer.start(c->stream));
  double* t1 = c->edt.tmp1.as<double>();
  double* t2 = c->edt.tmp2.as<double>();
  double* e2s = c->edt.out2.as<double>();   // scratch: the plain critical field
  int* vws = c->edt.v.as<int>();
  double* zws = c->edt.z.as<double>();
  const double res = desc->resolution;
  // envelope stacks in LDS when a 64-line block fits ((n + 2) x 64 x (8 + 2) B <= 150 KB, i.e. lines up to ~238 cells)
  // and the launch is small, else in the HBM workspace
  auto lds_bytes = [](int n) { return (size_t)(n + 2) * 64 * 10; };
  auto launch = [&](auto kern_g, auto kern_l, EdtPass P, long long map_stride, const signed char* occ, const double* src,
                    double* dst, int pass) -> topay_status {
    const int bs = 64;
    P.map_stride = map_stride;
    P.ws_stride = (long long)ws_elems;
    const dim3 grid((unsigned)((P.nlines + bs - 1) / bs), (unsigned)n_maps);
    const size_t lb = lds_bytes(P.n);
    // LDS stacks cut the latency of every envelope step but leave one wave per CU resident (129 KB per 64-line block
    // at n = 200): they win while the launch cannot fill the device anyway (a single benchmark-size map: 2.7 vs 3.8 ms)
    // and lose when there are lines enough to hide the HBM latency instead (1024 maps: 191 vs 142 ms).
    if (lb <= 56 * 1024 || (lb <= 150 * 1024 && (long long)n_maps * P.nlines <= 65536)) {  // short lines: several blocks per CU still fit
      HIPCHK(hipFuncSetAttribute((const void*)kern_l, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb));
      hipLaunchKernelGGL(kern_l, grid, dim3(bs), lb, c->stream, P, occ, src, dst, vws, zws, pass, res);
    } else {
      hipLaunchKernelGGL(kern_g, grid, dim3(bs), 0, c->stream, P, occ, src, dst, vws, zws, pass, res);
    }
    return TOPAY_OK;
  };
  // Lines of up to 512 cells (every benchmark map: 200 x 200 x 16) take the exhaustive-search passes (topay_edt.h:
  // k_edt_direct / k_edt_tile, 32-bit squared distances between the passes); longer lines the serial envelope passes.
  const bool small_lines = std::max(nx, std::max(ny, nz)) <= 512;
  auto pick_w = [](long long lines) { int w = 1; for (int d = 1; d <= 64; d++) if (lines % d == 0) w = d; return w; };
  int* i1 = (int*)t1;
  int* i2 = (int*)t2;
  auto direct = [&](auto kern, long long n_elems, int n, const signed char* occ, const int* src, int* dst_i, double* dst_d, int pass) {
    hipLaunchKernelGGL(kern, dim3((unsigned)((n_elems + 255) / 256), (unsigned)n_maps), dim3(256), 0, c->stream, n_elems, n, n_elems, occ, src,
                       dst_i, dst_d, pass, res);
  };
  auto tile = [&](auto kern, long long n_elems, int n, int W, long long step, long long inner_tiles, long long outer_stride, long long tiles,
                  const int* src, int* dst_i, double* dst_d, int pass) -> topay_status {
    const size_t lb = (size_t)n * W * sizeof(int);
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)n_maps), dim3(256), lb, c->stream, n, W, step, inner_tiles, outer_stride, n_elems,
                       (const signed char*)nullptr, src, dst_i, dst_d, pass, res);
    return TOPAY_OK;
  };
  // final pass of a signed field, both signs at once (k_edt_tile_signed: two tiles of W <= 32 lines in LDS)
  auto pick_w32 = [](long long lines) { int w = 1; for (int d = 1; d <= 32; d++) if (lines % d == 0) w = d; return w; };
  auto signed_x = [&](long long n_elems, int n, int W, long long step, long long inner_tiles, long long outer_stride, long long tiles,
                      const int* sp, const int* sn, double* dst_d) {
    const size_t lb = (size_t)n * W * sizeof(int) * 2;
    hipLaunchKernelGGL(k_edt_tile_signed, dim3((unsigned)tiles, (unsigned)n_maps), dim3(256), lb, c->stream, n, W, step, inner_tiles, outer_stride,
                       n_elems, sp, sn, dst_d, res);
  };
  if (small_lines) {
    // (tiles of up to 512 x 64 cells x 4 B = 128 KB of LDS: above the 64 KB default; set once, not per launch)
    static std::once_flag edt_attr_once[16];
    std::call_once(edt_attr_once[c->device % 16], [] {
      (void)hipFuncSetAttribute((const void*)k_edt_tile<1, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 512 * 64 * 4);
      (void)hipFuncSetAttribute((const void*)k_edt_tile<1, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 512 * 64 * 4);
      (void)hipFuncSetAttribute((const void*)k_edt_tile_signed, hipFuncAttributeMaxDynamicSharedMemorySize, 512 * 32 * 4 * 2);
    });
    const int wy = pick_w(nz), wx = pick_w32((long long)ny * nz);
    int* i2n = i2 + M * n3;   // second half of the workspace volume: the negative part's squared distances after the y pass
    for (int pass = 0; pass < 2; pass++) {   // 3-D: along z and y per sign, then along x for both — grid_map.cpp:425-521
      const dim3 g1((unsigned)((n3 + 255) / 256), (unsigned)n_maps);
      if (nz == 16) hipLaunchKernelGGL(k_edt_first_ballot<16>, g1, dim3(256), 0, c->stream, (long long)n3, (long long)n3, (const signed char*)d_occ3, i1, pass);
      else if (nz == 32) hipLaunchKernelGGL(k_edt_first_ballot<32>, g1, dim3(256), 0, c->stream, (long long)n3, (long long)n3, (const signed char*)d_occ3, i1, pass);
      else if (nz == 64) hipLaunchKernelGGL(k_edt_first_ballot<64>, g1, dim3(256), 0, c->stream, (long long)n3, (long long)n3, (const signed char*)d_occ3, i1, pass);
      else direct(k_edt_direct<0, 0>, (long long)n3, nz, d_occ3, nullptr, i1, nullptr, pass);
      if ((s = tile(k_edt_tile<1, 0>, (long long)n3, ny, wy, nz, nz / wy, (long long)ny * nz, (long long)nx * (nz / wy), i1, pass == 0 ? i2 : i2n, nullptr, pass)) != TOPAY_OK) return s;
    }
    signed_x((long long)n3, nx, wx, (long long)ny * nz, ((long long)ny * nz) / wx, 0, ((long long)ny * nz) / wx, i2, i2n, e3);
  }
  for (int pass = 0; pass < 2 && !small_lines; pass++) {
    // 3-D: along z (lines (x, y)), along y (lines (x, z)), along x (lines (y, z)) — grid_map.cpp:425-521
    EdtPass pz{(long long)nx * ny, nz, (long long)nx * ny, 0, (long long)nz, 1, 0, 0};
    EdtPass py{(long long)nx * nz, ny, (long long)nz, (long long)ny * nz, 1, (long long)nz, 0, 0};
    EdtPass px{(long long)ny * nz, nx, (long long)ny * nz, 0, 1, (long long)ny * nz, 0, 0};
    if ((s = launch(k_edt_pass<0, 0, 0>, k_edt_pass<0, 0, 1>, pz, (long long)n3, d_occ3, nullptr, t1, pass)) != TOPAY_OK) return s;
    if ((s = launch(k_edt_pass<1, 0, 0>, k_edt_pass<1, 0, 1>, py, (long long)n3, nullptr, t1, t2, pass)) != TOPAY_OK) return s;
    if ((s = launch(k_edt_pass<1, 1, 0>, k_edt_pass<1, 1, 1>, px, (long long)n3, nullptr, t2, e3, pass)) != TOPAY_OK) return s;
  }
  // One signed 2-D field from an occupancy grid: along y (lines x), along x (lines y), positive then negative part —
  // grid_map.cpp:125-207 and, with other seeds, 211-279, 283-351, 355-423
  auto field2d = [&](const signed char* occ, double* out) -> topay_status {
    if (small_lines) {
      const int w2 = pick_w32(ny);
      int* i1n = i1 + M * n2;
      direct(k_edt_direct<0, 0>, (long long)n2, ny, occ, nullptr, i1, nullptr, 0);
      direct(k_edt_direct<0, 0>, (long long)n2, ny, occ, nullptr, i1n, nullptr, 1);
      signed_x((long long)n2, nx, w2, ny, ny / w2, 0, ny / w2, i1, i1n, out);
      return TOPAY_OK;
    }
    EdtPass qy{(long long)nx, ny, (long long)nx, 0, (long long)ny, 1, 0, 0};
    EdtPass qx{(long long)ny, nx, (long long)ny, 0, 1, (long long)ny, 0, 0};
    for (int pass = 0; pass < 2; pass++) {
      topay_status s2;
      if ((s2 = launch(k_edt_pass<0, 0, 0>, k_edt_pass<0, 0, 1>, qy, (long long)n2, occ, nullptr, t1, pass)) != TOPAY_OK) return s2;
      if ((s2 = launch(k_edt_pass<1, 1, 0>, k_edt_pass<1, 1, 1>, qx, (long long)n2, nullptr, t1, out, pass)) != TOPAY_OK) return s2;
    }
    return TOPAY_OK;
  };
  auto threshold = [&](const double* field, signed char* occ) {
    const long long n = (long long)(M * n2);
    hipLaunchKernelGGL(k_edt_threshold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, field, c->dp.chassis_colli_radius, occ, n);
  };
  if ((s = field2d(d_occ2, e2)) != TOPAY_OK) return s;              // esdf_buffer_2d
  threshold(e2, d_occ2t);
  if ((s = field2d(d_occ2t, e2i)) != TOPAY_OK) return s;            // esdf_buffer_2d_inflate (355-423)
  if (project_critical) {
    const long long n = (long long)(M * n2);
    hipLaunchKernelGGL(k_edt_project, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const signed char*)d_occ3, d_occ2c,
                       (long long)n2, nz, (long long)M);
  }
  if ((s = field2d(d_occ2c, e2s)) != TOPAY_OK) return s;            // 2-D critical (211-279)
  threshold(e2s, d_occ2t);
  if ((s = field2d(d_occ2t, e2c)) != TOPAY_OK) return s;            // critical inflate, stored in esdf_buffer_2d_critical (283-351)
  HIPCHK(hipGetLastError());
  HIPCHK(c->edt.timer.stop(c->stream));
  // the map slots point into the arena; descriptors as topay_set_map
  for (int k = 0; k < n_maps; k++) {
    const int map_id = first_map_id + k;
    c->map2d[map_id].release(); c->map3d[map_id].release(); c->map2d_inf[map_id].release(); c->map2d_crit[map_id].release();
    DevMap& m = c->hmaps[map_id];
    for (int i = 0; i < 3; i++) {
      m.origin[i] = desc->origin[i]; m.dims[i] = desc->dims[i];
      m.min_b[i] = desc->min_boundary[i]; m.max_b[i] = desc->max_boundary[i];
    }
    m.res = desc->resolution;
    m.res_inv = 1.0 / desc->resolution;
    m.esdf2d = (glb_cdp)(e2 + (size_t)k * n2);
    m.esdf3d = (glb_cdp)(e3 + (size_t)k * n3);
    m.esdf2d_inflate = (glb_cdp)(e2i + (size_t)k * n2);
    m.esdf2d_critical = (glb_cdp)(e2c + (size_t)k * n2);
    c->have_map[map_id] = 1;
  }
  HIPCHK(hipMemcpyAsync((char*)c->dmaps.p + sizeof(DevMap) * first_map_id, &c->hmaps[first_map_id], sizeof(DevMap) * n_maps,
                        hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(c->edt.timer.read(&c->edt.ms));
  // the construction's workspace (occupancy, two intermediate volumes, the envelope stacks, the staged results: about
  // five times the maps themselves) is not needed once the fields sit in their map slots
  c->edt.thr.release(); c->edt.tmp1.release(); c->edt.tmp2.release(); c->edt.v.release(); c->edt.z.release(); c->edt.out2.release();
  return TOPAY_OK;
}

// ESDF construction on the device from the occupancy grids the reference fills from its point cloud (grid_map.cpp:733-747):
// occ2d[x*ny + y] (points below the chassis height), occ3d[x*ny*nz + y*nz + z].  The map slots then hold the result exactly as
// topay_set_map would.  A batch of maps of equal dimensions (the benchmark loop: one map per scenario) is built by the same
// launches, blockIdx.y = map: a single 200 x 200 x 16 map has too few lines to fill the device.
topay_status topay_build_esdf_fields(topay_ctx* c, int n_maps, int first_map_id, const topay_map_desc_t* desc,
                                     const signed char* occ2d, const signed char* occ2d_critical, const signed char* occ3d) {
  if (!c || !desc || !occ2d || !occ3d) return TOPAY_ERR_INVALID_ARG;
  if (topay_status rs = check_map_range(first_map_id, n_maps, "topay_build_esdf_fields")) return rs;
  HIPCHK(hipSetDevice(c->device));
  if (topay_status ws = wait_pending(c)) return ws;   // inputs of a solve in flight stay untouched
  const size_t n2 = (size_t)desc->dims[0] * desc->dims[1], n3 = n2 * desc->dims[2], M = (size_t)n_maps;
  if (topay_status ds = map_dims_check(desc)) return ds;
  forget_occupancy(c, first_map_id, n_maps);
  topay_status s;
  signed char *d_occ3, *d_occ2, *d_occ2c;   // 3-D, 2-D, 2-D critical
  auto lay_occ = [&](Carver& k) { d_occ3 = k.take<signed char>(M * n3); d_occ2 = k.take<signed char>(M * n2); d_occ2c = k.take<signed char>(M * n2); };
  if ((s = c->edt.occ.carve(lay_occ)) != TOPAY_OK) return s;
  HIPCHK(h2d(c, d_occ3, occ3d, M * n3));
  HIPCHK(h2d(c, d_occ2, occ2d, M * n2));
  if (occ2d_critical) HIPCHK(h2d(c, d_occ2c, occ2d_critical, M * n2));
  s = build_fields_from_device(c, n_maps, first_map_id, desc, d_occ3, d_occ2, d_occ2c, occ2d_critical == nullptr);
  c->edt.occ.release();
  return s;
}

topay_status topay_build_esdf_batch(topay_ctx* c, int n_maps, int first_map_id, const topay_map_desc_t* desc,
                                    const signed char* occ2d, const signed char* occ3d) {
  return topay_build_esdf_fields(c, n_maps, first_map_id, desc, occ2d, nullptr, occ3d);
}

topay_status topay_build_esdf(topay_ctx* c, int map_id, const topay_map_desc_t* desc, const signed char* occ2d,
                              const signed char* occ3d) {
  return topay_build_esdf_fields(c, 1, map_id, desc, occ2d, nullptr, occ3d);
}

// The two front-end fields of a map built on the device (GridMap::esdf_buffer_2d_inflate, esdf_buffer_2d_critical).
topay_status topay_get_map_fields(topay_ctx* c, int map_id, double* esdf2d_inflate, double* esdf2d_critical) {
  if (!c || check_map_slots(c, 1, &map_id, kMapResident | kMapFront, "topay_get_map_fields") != TOPAY_OK) return TOPAY_ERR_NO_MAP;   // (out of range too)
  const DevMap& m = c->hmaps[map_id];
  HIPCHK(hipSetDevice(c->device));
  const size_t n2 = (size_t)m.dims[0] * m.dims[1];
  if (esdf2d_inflate) HIPCHK(d2h_sync(c, esdf2d_inflate, (const double*)m.esdf2d_inflate, n2));
  if (esdf2d_critical) HIPCHK(d2h_sync(c, esdf2d_critical, (const double*)m.esdf2d_critical, n2));
  return TOPAY_OK;
}

// Copy a resident map back (tests, or a caller that wants the GPU-built ESDF on the host); milliseconds of the last build.
topay_status topay_get_map(topay_ctx* c, int map_id, double* esdf2d, double* esdf3d, double* build_ms) {
  if (!c || check_map_slots(c, 1, &map_id, kMapResident, "topay_get_map") != TOPAY_OK) return TOPAY_ERR_NO_MAP;   // (out of range too)
  HIPCHK(hipSetDevice(c->device));
  const DevMap& m = c->hmaps[map_id];
  const size_t n2 = (size_t)m.dims[0] * m.dims[1], n3 = n2 * m.dims[2];
  if (esdf2d) HIPCHK(d2h_sync(c, esdf2d, (const double*)m.esdf2d, n2));
  if (esdf3d) HIPCHK(d2h_sync(c, esdf3d, (const double*)m.esdf3d, n3));
  if (build_ms) *build_ms = c->edt.ms;
  return TOPAY_OK;
}

}  // extern "C"
