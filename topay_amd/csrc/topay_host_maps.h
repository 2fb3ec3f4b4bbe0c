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

// ESDF construction on the device (GridMap::updateESDF, grid_map.cpp:125-521): one batch of n_maps maps of equal dimensions.  What
// the shape decides -- kernel family, first pass, tile widths, LDS sizes, where the envelope stacks live -- is edt_plan's
// (topay_edt.h); the launchers here read it.  Three jobs: setup (arena and workspace), construct (the launches), publish (the slots).
struct EdtBuild {
  topay_ctx* c;
  const int n_maps, nx, ny, nz;
  const size_t n2, n3, M;
  const double res;
  const EdtPlan plan;
  double *e3, *e2, *e2i, *e2c;   // results; e2i: inflate; e2c: critical (holds the critical-inflate field at the end, as the reference's buffer does)
  double *t1, *t2, *e2s;         // workspace: two intermediate volumes; the plain critical field
  signed char* occ_thr;          // 2-D scratch: the thresholded fields
  int* vws;                      // envelope stacks in HBM
  double* zws;

  EdtBuild(topay_ctx* ctx, int maps, const topay_map_desc_t* desc)
      : c(ctx), n_maps(maps), nx(desc->dims[0]), ny(desc->dims[1]), nz(desc->dims[2]), n2((size_t)nx * ny), n3(n2 * nz), M((size_t)maps),
        res(desc->resolution), plan(edt_plan(nx, ny, nz, maps)) {}

  topay_status setup(int first_map_id) {
    topay_status s;
    EdtState& w = c->edt;
    if ((s = w.thr.ensure(M * n2)) != TOPAY_OK) return s;
    if ((s = w.tmp1.ensure(M * n3 * 8)) != TOPAY_OK) return s;
    if ((s = w.tmp2.ensure(M * n3 * 8)) != TOPAY_OK) return s;
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
    auto lay_arena = [&](Carver& k) {
      e3 = k.take<double>(M * n3); e2 = k.take<double>(M * n2); e2i = k.take<double>(M * n2); e2c = k.take<double>(M * n2);
    };
    if ((s = ar->buf.carve(lay_arena)) != TOPAY_OK) return s;
    if ((s = w.out2.ensure(M * n2 * 8)) != TOPAY_OK) return s;
    if ((s = w.v.ensure(M * plan.ws_elems * 4)) != TOPAY_OK) return s;
    if ((s = w.z.ensure(M * plan.ws_elems * 8)) != TOPAY_OK) return s;
    occ_thr = w.thr.as<signed char>();
    t1 = w.tmp1.as<double>();
    t2 = w.tmp2.as<double>();
    e2s = w.out2.as<double>();
    vws = w.v.as<int>();
    zws = w.z.as<double>();
    return TOPAY_OK;
  }

  // One launcher per kernel family.  Only the envelope launcher can fail (its per-launch LDS attribute).
  dim3 cells(long long n_elems) const { return dim3((unsigned)((n_elems + 255) / 256), (unsigned)n_maps); }
  // first pass, along the contiguous axis: lines of n cells, n_elems cells per map; ballot 16 / 32 / 64 = n, or 0
  void first_pass(long long n_elems, int n, int ballot, const signed char* occ, int* dst_i, int pass) const {
    const long long map_stride = n_elems;   // the maps of a batch lie back to back
    if (ballot == 16) hipLaunchKernelGGL(k_edt_first_ballot<16>, cells(n_elems), dim3(256), 0, c->stream, n_elems, map_stride, occ, dst_i, pass);
    else if (ballot == 32) hipLaunchKernelGGL(k_edt_first_ballot<32>, cells(n_elems), dim3(256), 0, c->stream, n_elems, map_stride, occ, dst_i, pass);
    else if (ballot == 64) hipLaunchKernelGGL(k_edt_first_ballot<64>, cells(n_elems), dim3(256), 0, c->stream, n_elems, map_stride, occ, dst_i, pass);
    else hipLaunchKernelGGL(k_edt_direct, cells(n_elems), dim3(256), 0, c->stream, n_elems, n, map_stride, occ, dst_i, pass);
  }
  // strided pass over tiles of W lines x n cells (geometry: topay_edt.h), int32 to int32
  void tile(long long map_stride, int n, int W, size_t lds, long long step, long long inner_tiles, long long outer_stride, long long tiles,
            const int* src, int* dst_i) const {
    hipLaunchKernelGGL(k_edt_tile, dim3((unsigned)tiles, (unsigned)n_maps), dim3(256), lds, c->stream, n, W, step, inner_tiles, outer_stride,
                       map_stride, src, dst_i);
  }
  // final pass of a signed field, both signs at once (two tiles of W <= 32 lines in LDS)
  void tile_signed(long long map_stride, int n, int W, size_t lds, long long step, long long inner_tiles, long long outer_stride, long long tiles,
                   const int* src_pos, const int* src_neg, double* dst_d) const {
    hipLaunchKernelGGL(k_edt_tile_signed, dim3((unsigned)tiles, (unsigned)n_maps), dim3(256), lds, c->stream, n, W, step, inner_tiles,
                       outer_stride, map_stride, src_pos, src_neg, dst_d, res);
  }
  // envelope pass k of the plan: kern_l with the stacks in LDS, kern_g with the stacks in the HBM workspace
  using EnvelopeKernel = void (*)(EdtPass, const signed char*, const double*, double*, int*, double*, int, double);
  topay_status envelope(EnvelopeKernel kern_g, EnvelopeKernel kern_l, int k, const signed char* occ, const double* src, double* dst, int pass) const {
    const EdtPass& P = plan.pass[k];
    const dim3 grid((unsigned)((P.nlines + 63) / 64), (unsigned)n_maps);
    if (plan.stack_lds[k]) {
      HIPCHK(hipFuncSetAttribute((const void*)kern_l, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.stack_bytes[k]));
      hipLaunchKernelGGL(kern_l, grid, dim3(64), plan.stack_bytes[k], c->stream, P, occ, src, dst, vws, zws, pass, res);
    } else {
      hipLaunchKernelGGL(kern_g, grid, dim3(64), 0, c->stream, P, occ, src, dst, vws, zws, pass, res);
    }
    return TOPAY_OK;
  }
  void threshold(const double* field, signed char* occ) const {
    const long long n = (long long)(M * n2);
    hipLaunchKernelGGL(k_edt_threshold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, field, c->dp.chassis_colli_radius, occ, n);
  }
  void project(const signed char* occ3, signed char* occ2) const {
    const long long n = (long long)(M * n2);
    hipLaunchKernelGGL(k_edt_project, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, occ3, occ2, (long long)n2, nz, (long long)M);
  }

  // The 3-D field: along z and y per sign, then along x (small family: both signs in one launch) -- grid_map.cpp:425-521
  topay_status field3d(const signed char* occ, double* out) const {
    const long long yz = (long long)ny * nz;
    if (plan.small) {
      // (tiles of up to 512 x 64 cells x 4 B = 128 KB of LDS: above the 64 KB default; set once, not per launch)
      static std::once_flag edt_attr_once[16];
      std::call_once(edt_attr_once[c->device % 16], [] {
        (void)hipFuncSetAttribute((const void*)k_edt_tile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEdtTileLdsMax);
        (void)hipFuncSetAttribute((const void*)k_edt_tile_signed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEdtSignedLdsMax);
      });
      const int wy = plan.wy, wx = plan.wx;
      int *i1 = (int*)t1, *i2 = (int*)t2;
      int* i2n = i2 + M * n3;   // second half of the workspace volume: the negative part's squared distances after the y pass
      for (int pass = 0; pass < 2; pass++) {
        first_pass((long long)n3, nz, plan.first, occ, i1, pass);
        tile((long long)n3, ny, wy, plan.lds_y, nz, nz / wy, yz, (long long)nx * (nz / wy), i1, pass == 0 ? i2 : i2n);
      }
      tile_signed((long long)n3, nx, wx, plan.lds_x, yz, yz / wx, 0, yz / wx, i2, i2n, out);
      return TOPAY_OK;
    }
    for (int pass = 0; pass < 2; pass++) {
      topay_status s;
      if ((s = envelope(k_edt_pass<0, 0, 0>, k_edt_pass<0, 0, 1>, kEdtZ, occ, nullptr, t1, pass)) != TOPAY_OK) return s;
      if ((s = envelope(k_edt_pass<1, 0, 0>, k_edt_pass<1, 0, 1>, kEdtY, nullptr, t1, t2, pass)) != TOPAY_OK) return s;
      if ((s = envelope(k_edt_pass<1, 1, 0>, k_edt_pass<1, 1, 1>, kEdtX, nullptr, t2, out, pass)) != TOPAY_OK) return s;
    }
    return TOPAY_OK;
  }
  // One signed 2-D field from an occupancy grid: along y (lines x), along x (lines y), positive then negative part --
  // grid_map.cpp:125-207 and, with other seeds, 211-279, 283-351, 355-423
  topay_status field2d(const signed char* occ, double* out) const {
    if (plan.small) {
      const int w2 = plan.w2;
      int* i1 = (int*)t1;
      int* i1n = i1 + M * n2;
      first_pass((long long)n2, ny, 0, occ, i1, 0);
      first_pass((long long)n2, ny, 0, occ, i1n, 1);
      tile_signed((long long)n2, nx, w2, plan.lds_2, ny, ny / w2, 0, ny / w2, i1, i1n, out);
      return TOPAY_OK;
    }
    for (int pass = 0; pass < 2; pass++) {
      topay_status s;
      if ((s = envelope(k_edt_pass<0, 0, 0>, k_edt_pass<0, 0, 1>, kEdtY2, occ, nullptr, t1, pass)) != TOPAY_OK) return s;
      if ((s = envelope(k_edt_pass<1, 1, 0>, k_edt_pass<1, 1, 1>, kEdtX2, nullptr, t1, out, pass)) != TOPAY_OK) return s;
    }
    return TOPAY_OK;
  }

  // The five fields in the order of updateESDF.  occ2c is written here, as the projection of occ3, when project_critical.
  topay_status construct(const signed char* occ3, const signed char* occ2, signed char* occ2c, bool project_critical) const {
    topay_status s;
    if ((s = field3d(occ3, e3)) != TOPAY_OK) return s;               // esdf_buffer_3d (425-521)
    if ((s = field2d(occ2, e2)) != TOPAY_OK) return s;               // esdf_buffer_2d
    threshold(e2, occ_thr);
    if ((s = field2d(occ_thr, e2i)) != TOPAY_OK) return s;           // esdf_buffer_2d_inflate (355-423)
    if (project_critical) project(occ3, occ2c);
    if ((s = field2d(occ2c, e2s)) != TOPAY_OK) return s;             // 2-D critical (211-279)
    threshold(e2s, occ_thr);
    return field2d(occ_thr, e2c);                                    // critical inflate, stored in esdf_buffer_2d_critical (283-351)
  }

  // the map slots point into the arena; descriptors as topay_set_map
  topay_status publish(int first_map_id, const topay_map_desc_t* desc) const {
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
    return TOPAY_OK;
  }
};

// The construction from occupancy grids that already lie in device memory: d_occ3 [n_maps][nx*ny*nz], d_occ2 [n_maps][nx*ny] (points
// below the chassis height), d_occ2c [n_maps][nx*ny] (the critical grid; written here as the projection of d_occ3 when
// project_critical).  The body of topay_build_esdf_fields, which uploads the grids first, and of topay_generate_worlds
// (topay_host_world.h), whose rasteriser wrote them.  The grids are read only (d_occ2c apart) and stay the caller's.
static topay_status build_fields_from_device(topay_ctx* c, int n_maps, int first_map_id, const topay_map_desc_t* desc, signed char* d_occ3,
                                             signed char* d_occ2, signed char* d_occ2c, bool project_critical) {
  if (topay_status ds = map_dims_check(desc)) return ds;
  invalidate_sharers(c, first_map_id, n_maps);
  drop_shared_slots(c, first_map_id, n_maps);
  EdtBuild b(c, n_maps, desc);
  topay_status s;
  if ((s = b.setup(first_map_id)) != TOPAY_OK) return s;
  HIPCHK(c->edt.timer.start(c->stream));
  if ((s = b.construct(d_occ3, d_occ2, d_occ2c, project_critical)) != TOPAY_OK) return s;
  HIPCHK(hipGetLastError());
  HIPCHK(c->edt.timer.stop(c->stream));
  if ((s = b.publish(first_map_id, desc)) != TOPAY_OK) return s;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(c->edt.timer.read(&c->edt.ms));
  // the construction's workspace (occupancy, two intermediate volumes, the envelope stacks, the staged results: about
  // five times the maps themselves) is not needed once the fields sit in their map slots
  c->edt.thr.release(); c->edt.tmp1.release(); c->edt.tmp2.release(); c->edt.v.release(); c->edt.z.release(); c->edt.out2.release();
  return TOPAY_OK;
}

// Test hook: the plan of n_maps maps of dims, as 19 numbers: small (0 / 1); first (16 / 32 / 64 = ballot width, 0 = direct); wy, wx,
// w2; lds_y, lds_x, lds_2; then per envelope pass in the order 3-D z, y, x, 2-D y, x: five times stacks in LDS (0 / 1), five times
// the stacks' LDS bytes; the workspace elements per map.  No context, no device.
topay_status topay_edt_test_plan(const int dims[3], int n_maps, long long* out) {
  if (!dims || !out || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 || n_maps <= 0) return TOPAY_ERR_INVALID_ARG;
  const EdtPlan p = edt_plan(dims[0], dims[1], dims[2], n_maps);
  const long long head[8] = {p.small, p.first, p.wy, p.wx, p.w2, (long long)p.lds_y, (long long)p.lds_x, (long long)p.lds_2};
  std::copy(head, head + 8, out);
  for (int k = 0; k < kEdtPasses; k++) {
    out[8 + k] = p.stack_lds[k];
    out[13 + k] = (long long)p.stack_bytes[k];
  }
  out[18] = (long long)p.ws_elems;
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
