// lbm_host_live.inc -- part of lbm_api.hip (included there, behind the observer calls): the live inputs of a context,
// lbm_set_obstacles and lbm_write_state.  DESIGN.md 3.18.
//
// Both calls leave the context what lbm_create would have made of (map, lattice) on the same slabs: options, acceleration,
// probe set, engine choice, tiling and the mailbox tag sequence are not touched.  Neither communicates; every run starts by
// trading the halos (ghost bands, mail) of the lattice as it stands, so no engine trusts a ghost row from an earlier run and
// nothing beyond the slabs' own rows is refreshed here.
//
// What follows the map, all of it replaced by lbm_set_obstacles:
//   Slab::blocked                          lbm_swap_blocked (lbm_live.hip.h), which also refills and counts
//   blocked_gs / gn, band_blk_s / n        upload_ghost_masks, from the global map
//   lbm_ctx::obst_keep, tot_fluid          rebuilt as finish_create / lbm_create build them
//   fcells, fcells_host, tforces, fmap, fidx, fcontrib, fpmap, nbodies     lbm_set_bodies(ctx, NULL, 0)
//   pmap, pidx                             wave_probe_free: obstacle bytes with marks, rebuilt by wave_probe_ready
// What does not: the probe lists and the tiles' probe and window tables (cells and their places in the output: whether a
// cell is blocked is read from the bytes when a value is taken), march_slabs_setup's answer (peer access and shapes), the
// neighbours' nb_blocked (aliases of their bytes: hence the ordering rule of the header).
namespace {

int live_guard(const lbm_ctx* c) {
  if (int refused = refuse_failed(c)) return refused;
  return LBM_OK;
}

}  // namespace

extern "C" int lbm_set_obstacles(lbm_ctx* c, const int* obstacles, int refill) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (!obstacles) return fail(LBM_EINVAL, "obstacles is NULL");
  if (refill != LBM_REFILL_KEEP && refill != LBM_REFILL_REST)
    return fail(LBM_EINVAL, "refill must be LBM_REFILL_KEEP (0) or LBM_REFILL_REST (1) (got %d)", refill);
  int rc;
  if ((rc = live_guard(c))) return rc;
  const int nx = c->p.nx, ny = c->p.ny;
  const size_t ns = c->slabs.size();
  // ---- the staging of every slab first: no room, nothing queued
  std::vector<DeviceTemp> d_ob(ns), d_cnt(ns);
  std::vector<int> grid(ns);
  for (size_t i = 0; i < ns; ++i) {
    Slab& s = c->slabs[i];
    const long ncell = (long)s.nyl * nx;
    grid[i] = std::min(cdiv(ncell, lbm::kBlock), lbm::kSwapBlocksMax);
    HIPC(hipSetDevice(s.dev));
    if (hipMalloc(&d_ob[i].p, sizeof(int) * (size_t)ncell) != hipSuccess || hipMalloc(&d_cnt[i].p, sizeof(int) * (size_t)grid[i]) != hipSuccess) {
      (void)hipGetLastError();
      return fail(LBM_ENOMEM, "no room on device %d to stage %ld cells of the new map", s.dev, ncell);
    }
  }
  // ---- every slab: its rows of the new map to the device, the swap on its compute stream, the rows either side
  // (the same constants, by the same expressions, as slab_upload hands lbm_fill_equilibrium)
  const float w0 = c->p.density * 4.f / 9.f, w1 = c->p.density / 9.f, w2 = c->p.density / 36.f;
  std::vector<std::vector<int>> counts(ns);
  for (size_t i = 0; i < ns; ++i) {
    Slab& s = c->slabs[i];
    const long ncell = (long)s.nyl * nx;
    HIPC(hipSetDevice(s.dev));
    HIPC(hipMemcpyAsync(d_ob[i].p, obstacles + (long)s.row0 * nx, sizeof(int) * (size_t)ncell, hipMemcpyHostToDevice, s.sc));
    hipLaunchKernelGGL(lbm::lbm_swap_blocked, dim3(grid[i]), dim3(lbm::kBlock), 0, s.sc, (const int*)d_ob[i].p, s.blocked, s.lat[c->cur],
                       s.plane, s.pitch, nx, ncell, refill, w0, w1, w2, (int*)d_cnt[i].p);
    HIPC(hipGetLastError());
    if (s.blocked_gs && (rc = upload_ghost_masks(c, s, obstacles))) return rc;
    HIPC(hipStreamSynchronize(s.sc));
    counts[i].resize((size_t)grid[i]);
    HIPC(hipMemcpy(counts[i].data(), d_cnt[i].p, sizeof(int) * (size_t)grid[i], hipMemcpyDeviceToHost));
  }
  long refilled = 0;
  for (auto& v : counts) for (int n : v) refilled += n;
  // ---- the host's copies
  for (int i = 0; i < c->keep_rows; ++i) {
    const long gy = ((long)(c->keep_row0 + i) % ny + ny) % ny;
    for (int x = 0; x < nx; ++x) c->obst_keep[(size_t)i * nx + x] = obstacles[gy * nx + x] ? 1 : 0;
  }
  c->tot_fluid = count_fluid(obstacles, (long)nx * ny);
  // ---- the labelling goes (the library keeps no label array to validate against the new map), and lbm_wave's probe maps
  if ((rc = lbm_set_bodies(c, nullptr, 0))) return rc;
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    wave_probe_free(s, true);
  }
  c->obstacle_updates += 1;
  c->refilled_cells = refilled;
  return LBM_OK;
}

extern "C" int lbm_write_state(lbm_ctx* c, const float* cells) {
  if (!c || !cells) return fail(LBM_EINVAL, "NULL argument");
  int rc;
  if ((rc = live_guard(c))) return rc;
  bool on_dev = false;
  if ((rc = output_on_device(c, cells, "cells", &on_dev))) return rc;
  const int nx = c->p.nx;
  const int base_row = c->rank_mode ? c->slabs[0].row0 : 0;
  const size_t ns = c->slabs.size();
  // ---- host memory: the staging of every slab first (no room: nothing queued); device memory needs none
  std::vector<DeviceTemp> stage(ns);
  for (size_t i = 0; i < ns && !on_dev; ++i) {
    Slab& s = c->slabs[i];
    const long ncell = (long)s.nyl * nx;
    HIPC(hipSetDevice(s.dev));
    if (hipMalloc(&stage[i].p, sizeof(float) * 9 * (size_t)ncell) != hipSuccess) {
      (void)hipGetLastError();
      stage[i].p = nullptr;
      return fail(LBM_ENOMEM, "no room on device %d to stage %ld cells of the new lattice", s.dev, ncell);
    }
  }
  // ---- AoS to SoA into the lattice that holds the current state: whichever of the two it is, the next run reads it and
  // overwrites the other in full
  for (size_t i = 0; i < ns; ++i) {
    Slab& s = c->slabs[i];
    const long ncell = (long)s.nyl * nx;
    const float* rows = cells + 9L * (s.row0 - base_row) * nx;
    HIPC(hipSetDevice(s.dev));
    if (!on_dev) HIPC(hipMemcpyAsync(stage[i].p, rows, sizeof(float) * 9 * (size_t)ncell, hipMemcpyHostToDevice, s.sc));
    hipLaunchKernelGGL(lbm::lbm_aos_to_soa, dim3(cdiv(ncell, 256)), dim3(256), 0, s.sc, on_dev ? rows : (const float*)stage[i].p,
                       s.lat[c->cur], s.plane, s.pitch, nx, ncell);
    HIPC(hipGetLastError());
  }
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    HIPC(hipStreamSynchronize(s.sc));
  }
  return LBM_OK;
}
