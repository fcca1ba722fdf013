// lbm_host_run.inc -- part of lbm_api.hip (included there): the kind of a run (RunKind: one flavour field for the register
// tiles), the end of a run (sums, agreement), the tiles' tables (ONE upload, tile_table_set, of the layout lbm_tile_table.h
// builds: forces, probes, windows, the empty table), the register-tile engine (one driver for a lattice alone and for
// slabs; run_regtile turns the flavour into kernel, LDS and tables in one switch).  (The step loop of every halo transport
// is run_steps, lbm_api.hip; its launch groups are in lbm_host_march.inc.)
namespace {

// Where a register-tile run puts its snapshots (lbm_run_sampled): per local slab, the slab's region of snapshot 0 on its
// device and the floats from one snapshot to the next; every = 0: none.
struct SnapPlan {
  int every = 0;
  std::vector<float*> at;
  std::vector<long> stride;
};

// The kind of a run, handed from lbm_run and the observer calls (lbm_host_observe.inc) through run_steps to the engine that runs it
// (a plain lbm_run: the defaults).  `flavour` says what the register tiles would run, one line each with the other fields it
// reads; every flavour but plain and forces tries ONLY the tiles (they did not run: nothing has been stepped):
//   plain      lbm_run, lbm_run_driven: the plain kernel -- kRegDrive under a schedule (drive)
//   snapshots  lbm_run_sampled: kRegSnap.  snap: per slab, where snapshot 0 goes and the floats to the next one
//   forces     lbm_run_forces: kRegForce.  nb, nval; the slabs' force tables and partials are in place (force_tables)
//   mean       lbm_run_mean: kRegMean.  snap: at[i] is where slab i's means go, the strides unused
//   probes     lbm_run_probes: kRegProbe.  snap: at[i] is row 0 of the output slab i stores into, stride[i] the floats from one
//              sample's row to the next (4 x the probes of the whole set); the slabs' probe tables are in place (probe_tables)
//   window     lbm_run_window: as probes, fed the slabs' window tables (window_tables) in place of the probe set's
//   piece      lbm_run_observed, lbm_run_driven_observed: a piece of a longer call, in the kRegForce | kRegProbe flavour
//              (| kRegDrive under a schedule: drive, drive_at), which alone keeps the probes' phase and stores the last step's
//              speed sums folded like any other step's (piece_mid, not the last piece of the call: those are the ones used).
//              Forces are wanted when nb > 0 (nb, nval, as forces), probes when snap (as probes; pfirst: the first sample
//              that many steps into the piece, 1 .. every); an observer that is not wanted gets the table of -1s
//              (Slab::tnone: no tile counts or stores anything).  *ran tells the caller whether the tiles ran the piece
//              (false with LBM_OK: nothing stepped, nothing of the piece's output is valid).  win_table
//              (lbm_run_window_stats): the probes are a window's cells -- the piece is fed the slabs' window tables
//              (window_tables) where it would be fed the probe set's, which stays untouched.
// nb > 0 on every path: nb bodies; the run's forces are nval = 2 nb nsteps doubles at sums + nsteps + 1 of every slab (behind
// the per-step sums and the spare word of the register tiles' "somebody gave up"), reduced and fetched with them.
// no_tiles: the register tiles are not tried (the flavour is then read by nobody).
enum class RegFlavour { plain, snapshots, forces, mean, probes, window, piece };
struct RunKind {
  RegFlavour flavour = RegFlavour::plain;
  const SnapPlan* snap = nullptr;
  int nb = 0;
  long nval = 0;
  bool piece_mid = false, no_tiles = false, win_table = false;
  int pfirst = 0;
  bool* ran = nullptr;
  // what the run wants from its groups of K steps inside lbm_wave launches (lbm_wave_pick.h; a lattice alone that wave_admit said
  // yes to, the register tiles kept off): nothing, probes (with pfirst) or fields
  WaveWants wave;
  // drive (lbm_run_driven): drive[2 t], drive[2 t + 1] = (a1, a2) of the accelerate phase of step t (0-based) of this run, host
  // memory, in place of the context's pair.  The register tiles run their kRegDrive flavour (the slabs' device tables,
  // Slab::dtab, have room: the caller asked); off them, a lattice alone that wave_admit said yes to runs its groups of K
  // steps in lbm_wave's driven flavour; every other step goes through the one-step kernel with its own pair.
  const float* drive = nullptr;
  // drive with the piece flavour (lbm_run_driven_observed): the register tiles run kRegForce | kRegProbe | kRegDrive.  The
  // table of the WHOLE call is on the slabs' devices already (uploaded once, before the first piece); drive_at is the call's
  // step this piece starts at: the launch is handed Slab::dtab advanced by that many pairs, and uploads nothing.  drive
  // itself is the host table advanced likewise, for every path off the tiles.
  long drive_at = 0;
};

// End of a run: reduce across ranks (if there is a communicator), fetch the per-step sums and the
// peer-to-peer error word through pinned staging with async copies queued behind the step loop,
// then ONE wait per slab (s.sc has joined the edge and exchange streams by then).
int collect_sums(lbm_ctx* c, int nsteps, float* av_vels, std::chrono::steady_clock::time_point wall0, RunKind k, int extra = 0) {
  // (extra: doubles behind the per-step sums that are reduced and fetched with them -- the register tiles' "somebody gave up";
  // during lbm_run_forces that word and the forces behind it, on every path: every rank issues the same count)
  if (k.nb > 0) extra = 1 + (int)k.nval;
  if (c->rank_mode && c->slabs[0].comm != nullptr) {   // (a ring of one rank has a communicator too: identity)
    Slab& s = c->slabs[0];
    NCCLC(rccl::AllReduce(s.sums, s.sums, (size_t)(nsteps + extra), rccl::kFloat64, rccl::kSum, s.comm, s.sc));
  }
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    if ((av_vels || extra) && !s.sums_direct) HIPC(hipMemcpyAsync(s.sums_host, s.sums, sizeof(double) * (nsteps + extra), hipMemcpyDeviceToHost, s.sc));
    if (s.counters) HIPC(hipMemcpyAsync(s.err_host, s.counters + 32, sizeof(uint32_t), hipMemcpyDeviceToHost, s.sc));
  }
  double gpu_ms = 0.0;
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    if (c->exchange != 0) {
      HIPC(hipStreamSynchronize(s.sx));
      HIPC(hipStreamSynchronize(s.se));
    }
    HIPC(hipStreamSynchronize(s.sc));
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, s.ev_t0, s.ev_t1));
    if (ms > gpu_ms) gpu_ms = ms;
  }
  c->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  c->gpu_ms = gpu_ms;
  for (auto& s : c->slabs)
    if (s.counters && *s.err_host) {
      c->p2p_failed = true;
      return fail(LBM_EHIP, "peer-to-peer halo wait timed out (a neighbouring slab stopped)");
    }
  if (av_vels) {
    const double nf = (double)c->tot_fluid;
    const size_t ns = c->slabs.size();
    for (int i = 0; i < nsteps; ++i) {
      double acc = 0.0;
      for (size_t k = 0; k < ns; ++k) acc += c->slabs[k].sums_host[i];
      av_vels[i] = (float)(acc / nf);  // d2q9-bgk.c:1811
    }
  }
  return LBM_OK;
}

// ----------------------------------------------------------------- the register tiles' tables (lbm_tile_table.h)
void tile_table_free(TileTable& t) {
  if (t.slot) (void)hipFree(t.slot);
  if (t.words) (void)hipFree(t.words);
  t = TileTable();
}

// Table t of a slab for tiles of ty rows and ntx columns of tiles, built from `cells` and uploaded: both arrays or neither.
// LBM_ENOMEM (`kind`: the table's word in the message): nothing queued, the table left empty.
int tile_table_set(Slab& s, TileTable& t, int ty, int ntx, const std::vector<TileCell>& cells, const char* kind) {
  HIPC(hipSetDevice(s.dev));
  std::vector<int> slot;
  std::vector<uint32_t> words;
  const int n = tile_table_build(ty, ntx, s.nyl / ty, cells, slot, words);
  tile_table_free(t);
  if (hipMalloc((void**)&t.slot, sizeof(int) * slot.size()) != hipSuccess ||
      (n > 0 && hipMalloc((void**)&t.words, sizeof(uint32_t) * words.size()) != hipSuccess)) {
    (void)hipGetLastError();
    tile_table_free(t);
    return fail(LBM_ENOMEM, "no room on device %d for the %s tables (%d tiles)", s.dev, kind, n);
  }
  HIPC(hipMemcpy(t.slot, slot.data(), sizeof(int) * slot.size(), hipMemcpyHostToDevice));
  if (n > 0) HIPC(hipMemcpy(t.words, words.data(), sizeof(uint32_t) * words.size(), hipMemcpyHostToDevice));
  t.nslots = n; t.ty = ty;
  return LBM_OK;
}

// A slab's body cells / probes as the tables take them: the word is mask | label << 8 / the probe's index + 1
std::vector<TileCell> tile_cells(const std::vector<int4>& cells, uint32_t add) {
  std::vector<TileCell> v;
  for (const int4& q : cells) v.push_back({q.x, q.y, (uint32_t)q.z + add});
  return v;
}

// The force table of a slab for tiles of ty rows (kept until lbm_set_bodies or another tiling), and room for the partials of
// nsteps steps.  LBM_ENOMEM: nothing queued.
int force_tables(Slab& s, int ty, int ntx, int nsteps) {
  int rc;
  if (s.tforces.ty != ty && (rc = tile_table_set(s, s.tforces, ty, ntx, tile_cells(s.fcells_host, 0u), "force"))) return rc;
  if (!grown_room(s, s.fpart, (long)nsteps * s.tforces.nslots * 8, 1, false))
    return fail(LBM_ENOMEM, "no room on device %d for the force partials (%d steps x %d tiles)", s.dev, nsteps, s.tforces.nslots);
  return LBM_OK;
}

// The probe table of a slab likewise (kept until lbm_set_probes or another tiling; a slab without probes gets the table of
// -1s alone), and the table of -1s for an observer that a piece does not want.
int probe_tables(Slab& s, int ty, int ntx) {
  return s.tprobes.ty == ty ? LBM_OK : tile_table_set(s, s.tprobes, ty, ntx, tile_cells(s.pcells_host, 1u), "probe");
}
int empty_table(Slab& s, int ty, int ntx) {
  if (s.tnone.ty == ty) return LBM_OK;
  const int rc = tile_table_set(s, s.tnone, ty, ntx, {}, "empty");
  return rc == LBM_ENOMEM ? fail(rc, "no room on device %d for the empty force table (%d tiles)", s.dev, ntx * (s.nyl / ty)) : rc;
}

// Every engine but the register tiles: the forces of step tt (0-based) from the lattice just stored, on the compute stream
// behind the step (and behind its edge rows, where they run on a stream of their own); launch parity q.
int launch_forces(lbm_ctx* c, int tt, int q, int nsteps, RunKind k) {
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    if (c->exchange != 0 && c->exchange != LBM_EXCHANGE_P2P && split_edge_stream(c, s)) HIPC(hipStreamWaitEvent(s.sc, s.ev_bnd[q], 0));
    hipLaunchKernelGGL(lbm::lbm_body_forces, dim3(1), dim3(lbm::kBlock), 0, s.sc, s.lat[c->cur], s.plane, s.fcells, s.fcells_n,
                       k.nb, s.sums + nsteps + 1 + (long)tt * 2 * k.nb);
    HIPC(hipGetLastError());
  }
  return LBM_OK;
}

// ----------------------------------------------------------------- register tiles (lbm_regtile.hip.h)
// The resident engine cannot be used on this context (any more): remember why, say so ONCE on stderr (a run that quietly
// takes twice as long is worse than a line of text), carry on with the streaming kernels.
void resident_give_up(lbm_ctx* c, const char* why) {
  c->resident_broken = true;
  snprintf(c->resident_why, sizeof(c->resident_why), "%s", why);
  static bool said = false;
  if (!said || getenv("LBM_VERBOSE")) fprintf(stderr, "lbm: register-tile engine not used (%s); running the streaming kernels instead\n", why);
  said = true;
}

// ---- a lattice alone on its GPU: 64-column tiles of nw x r rows, one per CU
bool regtile_ok(const lbm_ctx* c, int ty, int r) {
  if (c->p.nx % 64 != 0 || ty < 1 || ty > c->p.ny || c->p.ny % ty != 0) return false;
  if (!(r == 1 || r == 2 || r == 4) || ty % r != 0 || ty / r > 16) return false;
  // every tile must be resident at once: a CU takes 16 waves of this kernel (128 VGPRs) and 160 KB of its blocks' LDS
  const int nw = ty / r;
  const int per_cu = std::min({3, 16 / nw, (160 * 1024) / lbm::regtile_lds_bytes(nw, r)});
  return (long)(c->p.nx / 64) * (c->p.ny / ty) <= (long)c->ncu * per_cu;
}
// The tiling of every slab (of the lattice alone): tiles of ty rows, nty tile rows per slab; its residency not asked yet
void regtile_set(lbm_ctx* c, int ty, int r, int nty) {
  c->tplan.ty = ty; c->tplan.r = r; c->tplan.nw = ty / r; c->tplan.ntx = c->p.nx / 64; c->tplan.nty = nty;
  c->tplan.bpc = 0;
}
// Default tiling (of a lattice alone and of equal slabs alike; `per_dev` = slabs sharing a device, `rows` = rows per slab).
// Measured with the mailboxes in uncached memory (profiles/r03_regtile_tilings.log), us per step: the SHORTEST tiles that
// still fit one per CU win -- 1024x512: 32 rows 2.26, 64 rows 2.94; 1024x256: 16 rows 1.94, 32 rows 2.20; 1024x128: 8 rows
// 1.58, 16 rows 1.87; 256x256: 4 rows 1.34, 8 rows 1.38 -- but not one-row tiles (128x128: 2 rows 1.26, 1 row 1.31); and
// within a tile height, as few rows per wave as leave at most EIGHT waves (they meet at a barrier every step; 1024x256,
// 16-row tiles: 16 x 1 rows 2.00, 8 x 2 1.94, 4 x 4 1.98; 1024x128, 8-row tiles: 8 x 1 1.58, 4 x 2 1.76, 2 x 4 1.93),
// sixteen where the lattice leaves no choice (1024x1024: 16 waves x 4 rows, 2.94).
bool regtile_tiling_rule(int nx, int rows, int per_dev, int ncu, int* ty_out, int* r_out) {
  if (nx < 64 || nx % 64 != 0 || rows < 1 || per_dev < 1 || ncu < 1) return false;
  const long ntx = nx / 64;
  for (int ty = (rows >= 2 ? 2 : 1); ty <= std::min(rows, 64); ++ty) {
    if (rows % ty != 0 || (long)per_dev * ntx * (rows / ty) > (long)ncu) continue;
    for (int waves : {8, 16})
      for (int r : {1, 2, 4}) {
        if (ty % r != 0 || ty / r > waves) continue;
        if ((160 * 1024) / lbm::regtile_lds_bytes(ty / r, r) < 1) continue;
        *ty_out = ty; *r_out = r;
        return true;
      }
  }
  return false;
}
bool regtile_default_tiling(const lbm_ctx* c, int rows, int per_dev, int* ty_out, int* r_out) {
  return regtile_tiling_rule(c->p.nx, rows, per_dev, c->ncu, ty_out, r_out);
}
bool plan_regtile(lbm_ctx* c) {
  c->tplan.ty = 0;
  int ty = 0, r = 0;
  if (!regtile_default_tiling(c, c->p.ny, 1, &ty, &r) || !regtile_ok(c, ty, r)) return false;
  regtile_set(c, ty, r, c->p.ny / ty);
  return true;
}

// ---- register tiles ACROSS SLABS (SURVEY 8 f1, the multi-GPU half): every slab keeps its rows in the registers of its
// own GPU for the whole run, and the granules that leave a slab through its bottom / top edge go straight into the
// neighbouring slab's mailboxes (lbm_regtile.hip.h, kRegSlab) -- over xGMI when that slab lives on another GPU.  Same
// tiling on every slab (equal slabs, 64-column tiles of ty rows); the slabs of one device go in ONE launch (their tiles
// wait for each other, so they must be resident together).  Contexts whose neighbours can store into each other's
// memory: slabs of one process (copy and peer-to-peer contexts: pointers, peer access across devices), and one process
// per GPU with peer-to-peer halos (hipIpc mappings, handles in the halo block; needs the communicator, through which the
// ranks agree after every run whether anybody gave up).
int regtile_slab_count(const lbm_ctx* c) { return c->rank_mode ? c->nranks : (int)c->slabs.size(); }

bool regtile_slabs_possible(const lbm_ctx* c) {
  if (c->exchange != LBM_EXCHANGE_P2P && c->exchange != LBM_EXCHANGE_COPY) return false;
  // (ranks without a communicator cannot agree on whether anybody gave up: the streaming kernels, unless a test that adds up
  // the ranks' results itself says otherwise)
  static const bool trust = getenv("LBM_REGTILE_SLABS_NO_AGREEMENT") && atoi(getenv("LBM_REGTILE_SLABS_NO_AGREEMENT"));
  if (c->rank_mode && c->nranks > 1 && ((c->no_comm && !trust) || c->exchange != LBM_EXCHANGE_P2P)) return false;
  const int n = regtile_slab_count(c);
  return c->p.nx % 64 == 0 && n >= 1 && c->p.ny % n == 0;
}

// Tiling: as for a lattice alone (as few rows per wave as fit, on at most half the CUs where possible), counted per device.
bool plan_regtile_slabs(lbm_ctx* c) {
  c->tplan.ty = 0;
  if (!regtile_slabs_possible(c)) return false;
  const char* off = getenv("LBM_REGTILE_SLABS");
  if (off && atoi(off) == 0) return false;
  const int nyl = c->p.ny / regtile_slab_count(c);
  int per_dev = 1;
  for (auto& a : c->slabs) {
    int n = 0;
    for (auto& b : c->slabs) n += (b.dev == a.dev) ? 1 : 0;
    per_dev = std::max(per_dev, n);
  }
  // (development: LBM_REGTILE_SLAB_TILING = rows per tile x 10 + rows per wave, as the `regtile` option of a lone lattice)
  const int forced = getenv("LBM_REGTILE_SLAB_TILING") ? atoi(getenv("LBM_REGTILE_SLAB_TILING")) : 0;
  int ty = 0, r = 0;
  if (forced > 0) {
    ty = forced / 10; r = forced % 10;
    if (!(r == 1 || r == 2 || r == 4) || ty < r || ty % r != 0 || ty / r > 16 || nyl % ty != 0 ||
        (long)per_dev * (c->p.nx / 64) * (nyl / ty) > (long)c->ncu) return false;
  } else if (!regtile_default_tiling(c, nyl, per_dev, &ty, &r)) return false;
  regtile_set(c, ty, r, nyl / ty);
  return true;
}

// Will the next run try the register tiles first?  (info "engine_next")
bool regtile_is_next(const lbm_ctx* c) {
  if (c->tplan.ty <= 0 || c->resident_broken || (c->variant & 8) != 0 || !(c->engine == 0 || c->engine == 3)) return false;
  if (c->exchange == 0) return c->slabs.size() == 1;
  if (!regtile_slabs_possible(c)) return false;
  if (c->rank_mode && c->nranks > 1) {
    if (!c->p2p_connected) return false;
    for (int side = 0; side < 2; ++side) if (!c->slabs[0].tmail_nb[side]) return false;
  }
  return true;
}

// The instantiation of the register tiles for a tiling and a flavour (0, kRegSnap, kRegForce, kRegMean, kRegProbe): lbm_regtile, its arguments
// by value (a lattice alone), or lbm_regtile_slabs, a table of them (SLAB)
template <bool SLAB, int R, int MODE>
constexpr auto regtile_instance() {
  if constexpr (SLAB) return lbm::lbm_regtile_slabs<R, MODE | lbm::kRegSlab>;
  else return lbm::lbm_regtile<R, MODE>;
}
template <bool SLAB, int FLAVOUR>
auto regtile_flavour(int r, bool fast, bool async) {
  constexpr int AS = lbm::kRegAsync | FLAVOUR;     // (R = 1 has no asynchronous loop)
  if (async && r == 4) return fast ? regtile_instance<SLAB, 4, AS | 1>() : regtile_instance<SLAB, 4, AS>();
  if (async && r == 2) return fast ? regtile_instance<SLAB, 2, AS | 1>() : regtile_instance<SLAB, 2, AS>();
  switch (r) {
    case 4: return fast ? regtile_instance<SLAB, 4, FLAVOUR | 1>() : regtile_instance<SLAB, 4, FLAVOUR>();
    case 2: return fast ? regtile_instance<SLAB, 2, FLAVOUR | 1>() : regtile_instance<SLAB, 2, FLAVOUR>();
    default: return fast ? regtile_instance<SLAB, 1, FLAVOUR | 1>() : regtile_instance<SLAB, 1, FLAVOUR>();
  }
}
template <bool SLAB>
auto regtile_kernel(int r, bool fast, bool async, int flavour) {
  if (flavour == lbm::kRegSnap) return regtile_flavour<SLAB, lbm::kRegSnap>(r, fast, async);
  if (flavour == lbm::kRegForce) return regtile_flavour<SLAB, lbm::kRegForce>(r, fast, async);
  if (flavour == lbm::kRegMean) return regtile_flavour<SLAB, lbm::kRegMean>(r, fast, async);
  if (flavour == lbm::kRegProbe) return regtile_flavour<SLAB, lbm::kRegProbe>(r, fast, async);
  if (flavour == lbm::kRegDrive) return regtile_flavour<SLAB, lbm::kRegDrive>(r, fast, async);
  if (flavour == (lbm::kRegForce | lbm::kRegProbe)) return regtile_flavour<SLAB, lbm::kRegForce | lbm::kRegProbe>(r, fast, async);
  if (flavour == (lbm::kRegForce | lbm::kRegProbe | lbm::kRegDrive)) return regtile_flavour<SLAB, lbm::kRegForce | lbm::kRegProbe | lbm::kRegDrive>(r, fast, async);
  return regtile_flavour<SLAB, 0>(r, fast, async);
}

// Before the first launch of a tiling on a device: let the kernel have its dynamic LDS (beyond the 64 KB a kernel gets
// without asking) and ASK the runtime how many of its blocks a CU takes.  The tiles wait on each other, so all of them must
// be resident at once: blocks per CU x CUs >= tiles, or the launch would stall until its waits time out.  Returns the
// blocks per CU, or -1 with the reason in lbm_last_error.
int regtile_prepare(const lbm_ctx* c, const void* fn, int dev, int threads, unsigned shm) {
  struct Seen { const void* fn; int dev; };
  static std::mutex mu;
  static std::vector<Seen> raised;
  {
    std::lock_guard<std::mutex> g(mu);
    bool have = false;
    for (auto& e : raised) have = have || (e.fn == fn && e.dev == dev);
    if (!have) {
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        if (shm > 64u * 1024u) { fail(LBM_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed: %s", hipGetErrorString(e)); return -1; }
      } else raised.push_back({fn, dev});
    }
  }
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, shm);
  if (e != hipSuccess) { (void)hipGetLastError(); fail(LBM_EHIP, "occupancy query failed: %s", hipGetErrorString(e)); return -1; }
  (void)c;
  return n;
}

size_t regtile_mail_bytes(const lbm_ctx* c) {
  return (size_t)c->tplan.ntx * c->tplan.nty * 2 * (size_t)lbm::regtile_box(c->tplan.ty);
}

// A slab's mail area.  Uncached device memory: the granules are written once and read once, by another CU, and every
// access is sc1 anyway -- without the L2 allocation a hand-off is shorter (1024x1024: 4.14 -> 3.48 us per step, found when
// the slabs' mail areas, uncached for the sake of stores from other GPUs, ran faster than a lone lattice's); a slab's
// neighbour on another GPU stores into it behind this GPU's L2.  A lattice alone takes ordinary device memory where the
// device refuses uncached memory; slabs do not (LBM_REGTILE_MAIL_CACHED=1: ordinary device memory, to measure what that costs).
int regtile_mail_alloc(lbm_ctx* c, Slab& s) {
  if (s.tmail) return LBM_OK;
  HIPC(hipSetDevice(s.dev));
  const size_t bytes = regtile_mail_bytes(c);
  static const bool cached = getenv("LBM_REGTILE_MAIL_CACHED") && atoi(getenv("LBM_REGTILE_MAIL_CACHED"));
  hipError_t e = cached ? hipMalloc((void**)&s.tmail, bytes) : hipExtMallocWithFlags((void**)&s.tmail, bytes, hipDeviceMallocUncached);
  if (e != hipSuccess && c->exchange == 0) {
    (void)hipGetLastError();
    e = hipMalloc((void**)&s.tmail, bytes);
  }
  if (e != hipSuccess) { (void)hipGetLastError(); s.tmail = nullptr; return fail(LBM_EHIP, "cannot allocate the mail area of a slab: %s", hipGetErrorString(e)); }
  HIPC(hipMemset(s.tmail, 0, bytes));
  HIPC(hipDeviceSynchronize());
  s.tmail_bytes = bytes;
  return LBM_OK;
}

// Every buffer of the register tiles: a new tiling (option "regtile") starts without them.
void regtile_free(lbm_ctx* c) {
  for (auto& s : c->slabs) {
    (void)hipSetDevice(s.dev);
    for (int side = 0; side < 2; ++side) {
      if (s.tmail_nb_ipc[side] && s.tmail_nb[side] && (side == 0 || s.tmail_nb[1] != s.tmail_nb[0])) (void)hipIpcCloseMemHandle(s.tmail_nb[side]);
      s.tmail_nb[side] = nullptr; s.tmail_nb_ipc[side] = false;
    }
    if (s.tmail) (void)hipFree(s.tmail);
    grown_free(s.rpartials);
    if (s.rabort) (void)hipFree(s.rabort);
    if (s.ev_rt) (void)hipEventDestroy(s.ev_rt);
    s.tmail = nullptr; s.rabort = nullptr; s.ev_rt = nullptr;
  }
  if (c->rtable) (void)hipHostFree(c->rtable);
  c->rtable = c->rtable_dev = nullptr;
}

// A run of the register tiles, a lattice alone (one device group of one slab) or the slabs of a context.  *done: the steps
// ran; false with LBM_OK: nothing was queued or the tiles gave up with the lattice untouched -- the caller runs the streaming
// kernels.
int run_regtile(lbm_ctx* c, int nsteps, float* av_vels, bool* done, RunKind k) {
  *done = false;
  const bool lone = c->exchange == 0;
  const auto& t = c->tplan;
  const int ns = (int)c->slabs.size(), ntiles = t.ntx * t.nty;
  const bool fast = (c->variant & lbm::kFastMath) != 0, async = c->regtile_async != 0;
  const dim3 block(64 * t.nw);
  const unsigned shm = (unsigned)lbm::regtile_lds_bytes(t.nw, t.r);
  // What RunKind::flavour means to a launch, all of it here: the kernel's flavour and its LDS, and the two tables of a slab it
  // is handed -- `counted` through RegTileArgs::fslot / fwords (the probe flavour reads its probes or window there), `sampled`
  // through pslot / pwords (the force-and-probe flavour alone).  A table nobody reads: the table of -1s, built or not.
  const bool fpk = k.flavour == RegFlavour::piece;
  const bool fk = k.flavour == RegFlavour::forces || (fpk && k.nb > 0);   // forces are counted: partials, and their fold behind the launch
  const bool dk = k.drive != nullptr && (fpk || k.flavour == RegFlavour::plain);
  int flavour = dk ? lbm::kRegDrive : 0;
  unsigned shm_run = shm;
  TileTable Slab::*counted = &Slab::tnone, Slab::*sampled = &Slab::tnone;
  switch (k.flavour) {
    case RegFlavour::plain: break;
    case RegFlavour::snapshots: flavour = lbm::kRegSnap; break;
    case RegFlavour::forces: flavour = lbm::kRegForce; shm_run = (unsigned)lbm::regtile_lds_bytes_force(t.nw, t.r); counted = &Slab::tforces; break;
    case RegFlavour::mean: flavour = lbm::kRegMean; shm_run = (unsigned)lbm::regtile_lds_bytes_mean(t.nw, t.r); break;
    case RegFlavour::probes: flavour = lbm::kRegProbe; shm_run = (unsigned)lbm::regtile_lds_bytes_probe(t.nw, t.r); counted = &Slab::tprobes; break;
    case RegFlavour::window: flavour = lbm::kRegProbe; shm_run = (unsigned)lbm::regtile_lds_bytes_probe(t.nw, t.r); counted = &Slab::twindow; break;
    case RegFlavour::piece:
      flavour |= lbm::kRegForce | lbm::kRegProbe; shm_run = (unsigned)lbm::regtile_lds_bytes_force_probe(t.nw, t.r);
      if (fk) counted = &Slab::tforces;
      if (k.snap) sampled = k.win_table ? &Slab::twindow : &Slab::tprobes;
      break;
  }
  auto kernel = [&](int fl) {
    return lone ? reinterpret_cast<const void*>(regtile_kernel<false>(t.r, fast, async, fl))
                : reinterpret_cast<const void*>(regtile_kernel<true>(t.r, fast, async, fl));
  };
  static const bool want_stats = getenv("LBM_REGTILE_STATS") != nullptr;   // development: missed polls per run
  const bool stats = lone && want_stats;
  int rc;
  // device groups: the local slabs in the order of their devices' first appearance (found once)
  auto& order = c->tplan.order;            // order[k] = slab index; gstart[g] = first k of group g (+ end)
  auto& gstart = c->tplan.gstart;
  if (gstart.empty()) {
    std::vector<bool> taken(ns, false);
    for (int i = 0; i < ns; ++i) {
      if (taken[i]) continue;
      gstart.push_back((int)order.size());
      for (int j = i; j < ns; ++j) if (!taken[j] && c->slabs[j].dev == c->slabs[i].dev) { taken[j] = true; order.push_back(j); }
    }
    gstart.push_back((int)order.size());
  }
  const int ngroups = (int)gstart.size() - 1;
  auto lead = [&](int g) -> Slab& { return c->slabs[order[gstart[g]]]; };
  if (t.bpc == 0) {                     // first run of this tiling: is every tile of every device resident at once?
    int worst = 1 << 30, most = 1;
    for (int g = 0; g < ngroups; ++g) {
      HIPC(hipSetDevice(lead(g).dev));
      const int n = regtile_prepare(c, kernel(0), lead(g).dev, (int)block.x, shm);
      if (n < 0) { c->tplan.bpc = -1; snprintf(c->resident_why, sizeof(c->resident_why), "%s", lbm_last_error()); break; }
      worst = std::min(worst, n); most = std::max(most, gstart[g + 1] - gstart[g]);
    }
    if (t.bpc == 0) {
      c->tplan.bpc = worst;
      if ((long)worst * std::max(c->ncu, 1) < (long)ntiles * most) {
        c->tplan.bpc = -1;
        snprintf(c->resident_why, sizeof(c->resident_why), "%d slab(s) x %d tiles of %d waves on one device, but it takes %d block(s) per CU on %d CUs at once", most, ntiles, t.nw, worst, c->ncu);
      }
    }
  }
  if (t.bpc < 0) return fail(LBM_EINVAL, "register tiling%s not usable: %s", lone ? "" : " across slabs", c->resident_why);
  if (flavour != 0)                                     // the snapshot / force / mean / probe flavour must be resident at once too (else: the split
    for (int g = 0; g < ngroups; ++g) {                 // run / the force kernel; lbm_run_forces has asked every rank already)
      HIPC(hipSetDevice(lead(g).dev));
      const int n = regtile_prepare(c, kernel(flavour), lead(g).dev, (int)block.x, shm_run);
      if (n < 0 || (long)n * std::max(c->ncu, 1) < (long)ntiles * (gstart[g + 1] - gstart[g])) { (void)hipGetLastError(); return LBM_OK; }
    }
  // peer access between the devices of neighbouring slabs (one process; asked once)
  if (!c->rank_mode && !c->regtile_peers)
    for (int i = 0; i < ns; ++i)
      for (int d : {(i + ns - 1) % ns, (i + 1) % ns}) {
        const int a = c->slabs[i].dev, b = c->slabs[d].dev;
        if (a == b) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) { (void)hipGetLastError(); return fail(LBM_EHIP, "device %d cannot store into device %d", a, b); }
        HIPC(hipSetDevice(a));
        const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
        (void)hipGetLastError();
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(LBM_EHIP, "hipDeviceEnablePeerAccess(%d -> %d): %s", a, b, hipGetErrorString(e));
      }
  c->regtile_peers = true;
  // buffers: the mail areas, the per-step tile sums, the groups' abort words, the table of arguments
  for (auto& s : c->slabs) {
    if ((rc = regtile_mail_alloc(c, s))) return rc;
    if (!grown_room(s, s.rpartials, nsteps + (fpk ? 1 : 0), ntiles, true))   // (the force + probe flavour: one row more, see RegTileArgs::pfirst)
      return fail(LBM_EHIP, "no room on device %d for the tile sums of %d steps", s.dev, nsteps);
    if ((rc = ensure_sums(s, nsteps + 1))) return rc;
  }
  for (int g = 0; g < ngroups; ++g) {
    Slab& l = lead(g);
    if (!l.rabort) {
      HIPC(hipSetDevice(l.dev));
      HIPC(hipMalloc((void**)&l.rabort, 64));
      HIPC(hipMemsetAsync(l.rabort, 0, 64, l.sc));   // (in front of the group's launch on this stream)
    }
    if (!l.ev_rt && gstart[g + 1] - gstart[g] > 1) {
      HIPC(hipSetDevice(l.dev));
      HIPC(hipEventCreateWithFlags(&l.ev_rt, hipEventDisableTiming));
    }
  }
  if (!c->rtable) {
    HIPC(hipHostMalloc((void**)&c->rtable, sizeof(lbm::RegTileArgs) * ns, hipHostMallocPortable | hipHostMallocMapped));
    HIPC(hipHostGetDevicePointer((void**)&c->rtable_dev, c->rtable, 0));
  }
  // Tags only ever grow (a freshly zeroed mailbox is valid for any tag >= 1); every slab (every rank) counts the same runs,
  // so all hold the same tag0.  Before the 31-bit tags would wrap the mail areas are cleared and the count starts over.  A
  // lattice alone clears them in front of the run that would wrap them.  Slabs clear at the END of the run that passes
  // 0x60000000 (below), behind the slab's own launch and in front of the all-reduce that closes the run: no rank is past
  // that all-reduce before every rank has cleared, so no early mail of the next run can be wiped (late mail of THIS run
  // that lands after the clearing carries a tag of the old count: never asked for again)
  const bool wraps = (unsigned long long)c->rtag + (unsigned long long)nsteps >= 0x7fffff00ull;
  if (wraps && !lone) return fail(LBM_EINVAL, "a run of %d steps does not fit the mailbox tags left (split it)", nsteps);
  if (wraps) {
    HIPC(hipSetDevice(c->slabs[0].dev));
    HIPC(hipMemsetAsync(c->slabs[0].tmail, 0, c->slabs[0].tmail_bytes, c->slabs[0].sc));
    c->rtag = 1;
  }
  const bool restart_tags = !lone && (unsigned long long)c->rtag + (unsigned long long)nsteps >= 0x60000000ull;
  for (int g = 0; g < ngroups; ++g)
    for (int q = gstart[g]; q < gstart[g + 1]; ++q) {
      const int i = order[q];
      Slab& s = c->slabs[i];
      lbm::RegTileArgs& a = c->rtable[q];
      a.src = s.lat[c->cur]; a.dst = s.lat[c->cur ^ 1];
      a.plane = s.plane; a.pitch = s.pitch; a.nx = c->p.nx; a.ny = s.nyl;
      a.blocked = s.blocked; a.omega = c->p.omega;
      a.accel_row = s.accel_row;
      a.a1 = accel_pair(c).a1; a.a2 = accel_pair(c).a2;
      a.ty = t.ty; a.ntx = t.ntx; a.nty = t.nty;
      a.nsteps = nsteps; a.tag0 = c->rtag;
      a.mail = s.tmail; a.mail_bytes = (unsigned)s.tmail_bytes;
      a.partials = s.rpartials.p; a.abort_word = lead(g).rabort;
      a.fault = (getenv("LBM_REGTILE_FAULT") && i == 0) ? 1 : 0;   // (tests: a tile that never starts)
      a.stats = nullptr;
      a.snap = k.snap ? k.snap->at[i] : nullptr; a.snap_stride = k.snap ? k.snap->stride[i] : 0; a.every = k.snap ? k.snap->every : 0;
      a.density = c->p.density;
      a.fslot = (s.*counted).slot; a.fwords = (s.*counted).words;
      a.fpart = fk ? s.fpart.p : nullptr; a.nslots = fk ? s.tforces.nslots : 0;
      a.pslot = (s.*sampled).slot; a.pwords = (s.*sampled).words;
      a.pfirst = (fpk && !k.snap) ? 0x7fffffff : k.pfirst;   // (a piece with no probe wanted: no step is a sample step)
      if (c->rank_mode && c->nranks > 1) {
        a.mail_s = s.tmail_nb[0]; a.mail_n = s.tmail_nb[1];
        a.mail_bytes_s = (unsigned)s.tmail_nb_bytes[0]; a.mail_bytes_n = (unsigned)s.tmail_nb_bytes[1];
      } else {                        // (one process, or a ring of one rank: the neighbours are local slabs)
        Slab& so = c->slabs[(i + ns - 1) % ns];
        Slab& no = c->slabs[(i + 1) % ns];
        a.mail_s = so.tmail; a.mail_n = no.tmail;
        a.mail_bytes_s = (unsigned)so.tmail_bytes; a.mail_bytes_n = (unsigned)no.tmail_bytes;
      }
      a.nty_s = t.nty; a.nty_n = t.nty;
      a.drive = nullptr;
      if (dk && fpk) a.drive = s.dtab.p + 2 * k.drive_at;   // (a piece: the whole call's table is there, uploaded once)
      else if (dk) {                  // the schedule, in front of the slab's launch on its stream: 8 bytes per step
        HIPC(hipSetDevice(s.dev));
        HIPC(hipMemcpyAsync(s.dtab.p, k.drive, sizeof(float) * 2 * (size_t)nsteps, hipMemcpyHostToDevice, s.sc));
        a.drive = s.dtab.p;
      }
    }
  static unsigned long long* stats_buf = nullptr;
  constexpr size_t kStatsWords = 1028 + 72;   // [0], [1]: the counts; [1028 ..]: the first wave to give up (lbm_regtile.hip.h, await)
  if (stats) {
    HIPC(hipSetDevice(c->slabs[0].dev));
    if (!stats_buf) HIPC(hipMalloc((void**)&stats_buf, kStatsWords * 8));
    HIPC(hipMemsetAsync(stats_buf, 0, kStatsWords * 8, c->slabs[0].sc));
    c->rtable[0].stats = stats_buf;
  }
  c->rtag += (uint32_t)nsteps + 1u;   // (the last step's mail is sent too, and must never be taken for the next run's state 0)
  const auto wall0 = std::chrono::steady_clock::now();
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    s.err_host[1] = 0;                // lbm_fold_steps stores the abort word here
    HIPC(hipEventRecord(s.ev_t0, s.sc));
  }
  for (int g = 0; g < ngroups; ++g) {
    Slab& l = lead(g);
    const int n = gstart[g + 1] - gstart[g];
    HIPC(hipSetDevice(l.dev));
    for (int q = gstart[g] + 1; q < gstart[g + 1]; ++q) HIPC(hipStreamWaitEvent(l.sc, c->slabs[order[q]].ev_t0, 0));
    if (lone) hipLaunchKernelGGL(regtile_kernel<false>(t.r, fast, async, flavour), dim3(ntiles), block, shm_run, l.sc, c->rtable[0]);
    else hipLaunchKernelGGL(regtile_kernel<true>(t.r, fast, async, flavour), dim3(ntiles, n), block, shm_run, l.sc, c->rtable_dev + gstart[g]);
    HIPC(hipGetLastError());
    if (n > 1) HIPC(hipEventRecord(l.ev_rt, l.sc));
    for (int q = gstart[g]; q < gstart[g + 1]; ++q) {
      Slab& s = c->slabs[order[q]];
      if (q > gstart[g]) HIPC(hipStreamWaitEvent(s.sc, l.ev_rt, 0));
      if (fpk && k.piece_mid)           // a piece, not the call's last: its last step's tile sums as the loop folds them
        HIPC(hipMemcpyAsync(s.rpartials.p + (size_t)(nsteps - 1) * ntiles, s.rpartials.p + (size_t)nsteps * ntiles, sizeof(float) * ntiles,
                            hipMemcpyDeviceToDevice, s.sc));
      hipLaunchKernelGGL(lbm::lbm_fold_steps, dim3(cdiv(nsteps, lbm::kBlock / 64)), dim3(lbm::kBlock), 0, s.sc,
                         s.rpartials.p, ntiles, nsteps, s.sums, l.rabort, s.err_host + 1);
      HIPC(hipGetLastError());
      if (fk) {
        hipLaunchKernelGGL(lbm::lbm_fold_forces, dim3(cdiv(k.nval, lbm::kBlock)), dim3(lbm::kBlock), 0, s.sc,
                           s.fpart.p, s.tforces.nslots, nsteps, k.nb, s.sums + nsteps + 1);
        HIPC(hipGetLastError());
      }
      HIPC(hipEventRecord(s.ev_t1, s.sc));
    }
  }
  if (restart_tags)
    for (auto& s : c->slabs) {
      HIPC(hipSetDevice(s.dev));
      HIPC(hipMemsetAsync(s.tmail, 0, s.tmail_bytes, s.sc));
    }
  // did anybody give up?  One process: the abort words are all here.  One process per GPU: the ranks must agree (a rank whose
  // neighbour stopped notices a second later; one far away in a short run might not at all), so the word rides as one more
  // double behind the per-step sums through the all-reduce that ends the run.
  const bool agree = c->rank_mode && c->slabs[0].comm != nullptr;
  if (agree) {
    Slab& s = c->slabs[0];
    hipLaunchKernelGGL(lbm::lbm_abort_to_sum, dim3(1), dim3(64), 0, s.sc, s.rabort, s.sums + nsteps);
    HIPC(hipGetLastError());
  }
  if ((rc = collect_sums(c, nsteps, av_vels, wall0, k, agree ? 1 : 0))) return rc;
  if (stats) {
    std::vector<unsigned long long> st(kStatsWords);
    HIPC(hipMemcpy(st.data(), stats_buf, kStatsWords * 8, hipMemcpyDeviceToHost));
    fprintf(stderr, "lbm_regtile: %d steps, %d waves: %llu waits found their mail missing (%.3f per wave and step), %llu extra fetches\n",
            nsteps, ntiles * t.nw, st[0], (double)st[0] / ((double)nsteps * ntiles * t.nw), st[1]);
    if (st[1028] != 0) {
      fprintf(stderr, "lbm_regtile: the first wave to give up: tile %llu (of %d x %d) wave %llu row %llu, waiting for tag %llu (run's tag0 %u); tags it holds, lane: couriers / edge row\n",
              st[1028] - 1, t.ntx, t.nty, st[1029], st[1030], st[1031], c->rtable[0].tag0);
      for (int l : {0, 1, 2, 3, 31, 60, 61, 62, 63}) fprintf(stderr, "   lane %2d: %llu / %llu\n", l, st[1032 + l] >> 32, st[1032 + l] & 0xffffffffull);
    }
  }
  bool gave_up = false;
  for (auto& s : c->slabs) gave_up = gave_up || s.err_host[1] != 0;
  if (agree) gave_up = gave_up || c->slabs[0].sums_host[nsteps] != 0.0;
  if (gave_up) {
    for (int g = 0; g < ngroups; ++g) {
      Slab& l = lead(g);
      HIPC(hipSetDevice(l.dev));
      HIPC(hipMemsetAsync(l.rabort, 0, 64, l.sc));
      HIPC(hipStreamSynchronize(l.sc));
    }
    resident_give_up(c, lone ? "a tile waited 1 s for a neighbour: not every tile was running at once"
                             : "a tile waited 1 s for a neighbour (register tiles across slabs): not every tile was running at once");
    return LBM_OK;
  }
  if (restart_tags) c->rtag = 1;
  c->cur ^= 1;
  *done = true;
  return LBM_OK;
}

// The two-step kernel's peer-to-peer kind (declared in lbm_host_slabs.inc, launched by launch_pair): its instantiations are
// asked for HERE, behind everything above, which is where the code object has them.
void launch_sweep2_p2p(const lbm_ctx* c, const lbm::Sweep2Args& a, int grid, hipStream_t st) { launch_sweep2_k<lbm::kSweep2P2P>(c, a, grid, st); }

}  // namespace
