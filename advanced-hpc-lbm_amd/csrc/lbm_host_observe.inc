// lbm_host_observe.inc -- part of lbm_api.hip (included there, in front of run_steps): the observer calls -- lbm_run_sampled,
// lbm_run_forces, lbm_run_mean, lbm_run_stats, lbm_run_probes with lbm_set_bodies / lbm_set_probes, lbm_run_observed, and
// lbm_run_window with lbm_window_rows (WindowOut, window_tables: in front of it), lbm_run_window_stats behind it -- and the
// one copy of what they share:
//   output_on_device, ranks_agree          where an output lies; a rank context's ranks take the same path and fail together
//   device_room, wait_slabs, zero_output   an allocation whose refusal the caller words; every slab's stream waited for; an
//                                          output of which other ranks hold rows, zeroed first
//   launch_probe_gather, launch_cell_add (lbm_mean_add / lbm_stats_add), launch_window (lbm_derive_window /
//   lbm_window_stats_add), launch_mean_div the one launch site of each small kernel (run_steps' pgather uses them too);
//                                          lbm_window_stats_fold is launched by CellSums::fold alone
//   fetch_forces                           a run's forces from behind its per-step sums
//   SlabRows                               which rows of an output each slab owns: of the lattice, or of a window (the one
//                                          caller of lbm_window_rows)
//   ProbeOut, WindowOut                    where one call's probe values / windows go: device output in place, host output
//                                          through per-slab staging (snapshots keep derive_all and their two staging shapes)
//   CellSums                               a record of 4 or 8 floats per cell and slab, over the lattice or a window, divided
//                                          at the end: lbm_run_mean, lbm_run_stats, lbm_run_window_stats, lbm_run_observed
//   run_split, TilePieces                  the step loop cut at the sample steps (the single calls): plain run_steps pieces,
//                                          or register-tile pieces of `chunk` samples first, with the give-up rule, the
//                                          times and the piece count
//   observers_free                         everything a slab holds for these calls, released in one place (slab_free)
// Each call keeps its own refusals, the order in which it decides things before anything is queued, and its choice of path; it
// names what the register tiles would run in RunKind::flavour, and hands its cells to the one table builder (tile_table_set).
//
// lbm_run_observed, one run with any subset of the four observers (forces, probes, means, snapshots).  DESIGN.md 3.11.
//
// One observer alone IS its own call.  Two or more: the step loop is cut into pieces at the sample steps of the observers that
// are not taken inside a launch -- means and snapshots always; probes where the register tiles do not run -- and each piece is
// one run_steps with a RunKind that carries the observers taken inside it.
//   register tiles   EVERY piece runs the kRegForce | kRegProbe flavour (RegFlavour::piece), whichever of the two is wanted: it
//            alone knows a first-sample phase (pfirst), and it alone folds the last step's speed sum of a piece that is not the
//            call's last as the loop folds every other step's (piece_mid) -- a whole-run launch folds its last step in
//            another order of additions, so pieces of the other flavours would move the last bit of av_vels at the cuts.
//            An observer that is not wanted gets the table of -1s (empty_table).  A piece of n steps leaves its forces behind its per-step
//            sums (sums + n + 1), reduced and fetched with them.
//   elsewhere        forces as lbm_run_forces there (one-step kernel, lbm_body_forces behind each step), lbm_probe_gather
//            behind the piece that ends on a probe sample step.
// Behind a piece, on the slabs' streams: lbm_mean_add into the per-slab sums, lbm_final_state's derive into the snapshot's
// slot.  lbm_mean_div and the copies of staged output to the host after the last piece.
// A register-tile piece that gives up (or whose flavour is not resident) has stepped nothing: run_steps says so (RunKind::ran),
// and the loop repeats THAT piece from the same `done` off the tiles (RunKind::no_tiles, for the rest of the call) -- cut at
// the probes' sample steps, every row of the piece gathered again, the forces of its steps stored again.

// Output of lbm_run_sampled / lbm_run_mean (`what`: the argument's name): host memory, or device memory -- then of the device
// that holds every slab, written in place.
static int output_on_device(const lbm_ctx* c, const void* out, const char* what, bool* on_dev) {
  *on_dev = false;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, out) == hipSuccess && attr.type == hipMemoryTypeDevice) {
    *on_dev = true;
    for (auto& s : c->slabs)
      if (s.dev != attr.device)
        return fail(LBM_EINVAL, "%s is memory of device %d: device output needs every slab on that device (slab on %d)", what, attr.device, s.dev);
  }
  (void)hipGetLastError();      // (host memory unknown to HIP: an error the runtime remembers)
  return LBM_OK;
}

// Before lbm_run_forces / lbm_run_mean queue anything: a rank context's ranks take the same path and fail together.  rc: this
// rank's allocation result (`what` it was for); *in_kernel: would this rank use the register tiles -- on return, would every rank.
// Returns what the call must return now, or LBM_OK.
static int ranks_agree(lbm_ctx* c, int rc, bool* in_kernel, const char* what) {
  if (!(c->rank_mode && c->slabs[0].comm != nullptr)) return rc;
  // [0] ranks short of room, [1] ranks that would not use the tiles
  Slab& s = c->slabs[0];
  double v[2] = {rc ? 1.0 : 0.0, *in_kernel ? 0.0 : 1.0};
  HIPC(hipSetDevice(s.dev));
  HIPC(hipMemcpy(s.scratch_d, v, sizeof(v), hipMemcpyHostToDevice));
  NCCLC(rccl::AllReduce(s.scratch_d, s.scratch_d, 2, rccl::kFloat64, rccl::kSum, s.comm, s.sc));
  HIPC(hipStreamSynchronize(s.sc));
  HIPC(hipMemcpy(v, s.scratch_d, sizeof(v), hipMemcpyDeviceToHost));
  if (v[0] > 0.0) return rc ? rc : fail(LBM_ENOMEM, "another rank has no room for %s", what);
  *in_kernel = *in_kernel && v[1] == 0.0;
  return LBM_OK;
}

namespace {

// room for `bytes` on the current device; false: none -- the HIP error cleared, *p NULL (the caller words the refusal)
bool device_room(void** p, size_t bytes) {
  if (hipMalloc(p, bytes) == hipSuccess) return true;
  (void)hipGetLastError();
  *p = nullptr;
  return false;
}

// every slab's stream waited for
int wait_slabs(lbm_ctx* c) {
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    HIPC(hipStreamSynchronize(s.sc));
  }
  return LBM_OK;
}

// an output of which this context's slabs hold only a part: what other ranks' rows hold reads +0.0f
int zero_output(lbm_ctx* c, float* out, size_t bytes, bool on_dev) {
  if (on_dev) {
    Slab& s = c->slabs[0];
    HIPC(hipSetDevice(s.dev));
    HIPC(hipMemsetAsync(out, 0, bytes, s.sc));
    HIPC(hipStreamSynchronize(s.sc));
  } else memset(out, 0, bytes);
  return LBM_OK;
}

// ---- the small kernels behind a stored lattice, each launched from here alone (on the slab's stream)

// the slab's probes' cells of the stored lattice into their places of out_row, one sample's row of 4 x nprobes floats
int launch_probe_gather(const lbm_ctx* c, Slab& s, float* out_row) {
  const int n_here = (int)s.pcells_host.size();
  HIPC(hipSetDevice(s.dev));
  hipLaunchKernelGGL(lbm::lbm_probe_gather, dim3(cdiv(n_here, lbm::kBlock)), dim3(lbm::kBlock), 0, s.sc, s.lat[c->cur], s.plane,
                     s.pcells, n_here, s.blocked, c->p.density, out_row);
  HIPC(hipGetLastError());
  return LBM_OK;
}

// the fields of the slab's stored lattice added to its sums, one record per cell: of 4 floats (lbm_mean_add), or of 8 with
// their products beside them (lbm_stats_add)
int launch_cell_add(const lbm_ctx* c, Slab& s, int width, float* acc) {
  const int nx = c->p.nx;
  const long ncell = (long)s.nyl * nx;
  HIPC(hipSetDevice(s.dev));
  hipLaunchKernelGGL(width == 8 ? lbm::lbm_stats_add : lbm::lbm_mean_add, dim3(cdiv(ncell, lbm::kBlock)), dim3(lbm::kBlock), 0, s.sc,
                     s.lat[c->cur], s.plane, s.pitch, nx, ncell, s.blocked, c->p.density, acc);
  HIPC(hipGetLastError());
  return LBM_OK;
}

// the slab's sums of m samples, nf4 float4s, divided into out (which may be the sums themselves)
int launch_mean_div(Slab& s, const float* acc, long nf4, int m, float* out) {
  HIPC(hipSetDevice(s.dev));
  hipLaunchKernelGGL(lbm::lbm_mean_div, dim3(cdiv(nf4, lbm::kBlock)), dim3(lbm::kBlock), 0, s.sc, acc, nf4, (float)m, out);
  HIPC(hipGetLastError());
  return LBM_OK;
}

// the window cells of a slab's stored lattice, the slab's window rows first .. first + count - 1: into out = float[count][w.nx][4]
// (lbm_derive_window), or -- stats -- added with their products to out = float[count][w.nx][8], the sums of those rows
// (lbm_window_stats_add)
int launch_window(const lbm_ctx* c, Slab& s, const lbm_window& w, int first, int count, float* out, bool stats) {
  if (count <= 0) return LBM_OK;
  const long ncell = (long)count * w.nx;
  const long yl0 = (long)w.y0 + (long)first * w.sy - s.row0;
  HIPC(hipSetDevice(s.dev));
  hipLaunchKernelGGL(stats ? lbm::lbm_window_stats_add : lbm::lbm_derive_window, dim3(cdiv(ncell, lbm::kBlock)), dim3(lbm::kBlock), 0, s.sc,
                     s.lat[c->cur], s.plane, s.pitch, w.x0, w.nx > 1 ? w.sx : 1, w.nx, (int)yl0, count > 1 ? w.sy : 1, ncell, s.blocked,
                     c->p.density, out);
  HIPC(hipGetLastError());
  return LBM_OK;
}

// a run's forces: the local slabs' sums behind its n per-step sums (a rank: everybody's, through the all-reduce that ended it)
void fetch_forces(const lbm_ctx* c, int n, long nval, float* out) {
  for (long k = 0; k < nval; ++k) {
    double acc = 0.0;
    for (auto& s : c->slabs) acc += s.sums_host[n + 1 + k];
    out[k] = (float)acc;
  }
}

// Where one call's probe values go, [m][nprobes][4] floats.  Device output is written in place; host output goes through one
// staging buffer of that shape per slab that holds a probe (a slab stores into its probes' places only), copied out by to_host.
struct ProbeOut {
  lbm_ctx* c;
  float* out = nullptr;
  bool on_dev = false;
  int m = 0, np = 0;
  size_t nfloat = 0, local = 0;            // floats of the output; probes that the slabs of this context hold
  std::vector<DeviceTemp> stage;

  explicit ProbeOut(lbm_ctx* ctx) : c(ctx) {}
  int locate(float* o, const char* what) { out = o; return output_on_device(c, o, what, &on_dev); }
  // the staging of m_ samples (LBM_ENOMEM: nothing queued; the caller hands it to ranks_agree)
  int prepare(int m_) {
    m = m_; np = c->nprobes; nfloat = 4 * (size_t)m * (size_t)np;
    stage.resize(c->slabs.size());
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      Slab& s = c->slabs[i];
      local += s.pcells_host.size();
      if (on_dev || s.pcells_host.empty()) continue;
      HIPC(hipSetDevice(s.dev));
      if (!device_room(&stage[i].p, sizeof(float) * nfloat))
        return fail(LBM_ENOMEM, "no room on device %d for %d sample(s) of %d probe(s) of slab %zu (%zu bytes)", s.dev, m, np, i, sizeof(float) * nfloat);
    }
    return LBM_OK;
  }
  // the probes of other ranks' rows read +0.0f
  int zero_foreign() { return local >= (size_t)np ? LBM_OK : zero_output(c, out, sizeof(float) * nfloat, on_dev); }
  // row `row` of what slab i stores into (a slab without a probe stores nothing: NULL)
  float* at(size_t i, int row) const {
    float* base = on_dev ? out : (float*)stage[i].p;
    return base ? base + 4 * (size_t)row * (size_t)np : nullptr;
  }
  // the probes' cells of the stored lattice into row `row`, on every slab that holds a probe
  int gather(int row) {
    int rc;
    for (size_t i = 0; i < c->slabs.size(); ++i)
      if (!c->slabs[i].pcells_host.empty() && (rc = launch_probe_gather(c, c->slabs[i], at(i, row)))) return rc;
    return LBM_OK;
  }
  // what was staged, into the caller's array (the slabs' streams have been waited for)
  int to_host() {
    if (on_dev) return LBM_OK;
    std::vector<float> tmp;
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      Slab& s = c->slabs[i];
      if (s.pcells_host.empty()) continue;
      HIPC(hipSetDevice(s.dev));
      if (s.pcells_host.size() == (size_t)np) {          // (every probe is this slab's)
        HIPC(hipMemcpy(out, stage[i].p, sizeof(float) * nfloat, hipMemcpyDeviceToHost));
        continue;
      }
      tmp.resize(nfloat);
      HIPC(hipMemcpy(tmp.data(), stage[i].p, sizeof(float) * nfloat, hipMemcpyDeviceToHost));
      for (int j = 0; j < m; ++j)
        for (const int4& q : s.pcells_host) {
          const size_t o = 4 * ((size_t)j * np + (size_t)q.z);
          memcpy(out + o, tmp.data() + o, 4 * sizeof(float));
        }
    }
    return LBM_OK;
  }
};

// The staging bound of lbm_run_window_stats' register-tile path: the most bytes of staged samples one slab holds at a time.  Scratch-memory
// policy, not a tuned number (DESIGN.md 3.20): 64 MiB is four samples of the largest window a register-tile lattice has
// (1024 x 1024 cells, 16 MiB a sample) and thousands of a wake window's.
constexpr size_t kWindowStatsStageBytes = 64u << 20;

// Which rows of an output each slab of the context owns: slab i the rows first[i] .. first[i] + count[i] - 1 of `nx` cells,
// `local` rows between them.  Of a window: its window rows (lbm_window_rows) of w.nx cells; of the whole lattice: the
// slab's nyl rows of nx cells, counted from the context's first row.
struct SlabRows {
  std::vector<int> first, count;
  long local = 0;
  int nx;

  SlabRows(const lbm_ctx* c, const lbm_window* w) : nx(w ? w->nx : c->p.nx) {
    for (auto& s : c->slabs) {
      int f = s.row0 - (c->rank_mode ? c->slabs[0].row0 : 0), n = s.nyl;
      if (w) (void)lbm_window_rows(w, c->p.nx, c->p.ny, s.row0, s.row0 + s.nyl, &f, &n);
      first.push_back(f); count.push_back(n); local += n;
    }
  }
};

// Where one call's sums live and its means go, [rows][nx][width] floats: one record per cell and slab, of 4 floats
// (lbm_run_mean: the fields) or 8 (lbm_run_stats, lbm_run_window_stats: the fields and their products), over the whole
// lattice or over a window's cells (win) -- the sums of every path but the register tiles' mean flavour, and the staging of
// host output on every path.  A slab that owns no row allocates nothing and launches nothing.  Device output is written in
// place by the divide, host output is the sums divided in place and copied out.  lbm_run_window_stats on the register
// tiles has, beside the sums, the staging of one piece's samples, float[chunk][count][w.nx][4] per slab (stage_room, fold).
struct CellSums : SlabRows {
  lbm_ctx* c;
  int width;
  const lbm_window* win;
  float* out = nullptr;
  bool on_dev = false;
  std::vector<DeviceTemp> acc, stage;

  CellSums(lbm_ctx* ctx, int w, const lbm_window* window = nullptr) : SlabRows(ctx, window), c(ctx), width(w), win(window) {}
  int locate(float* o, const char* what) { out = o; return output_on_device(c, o, what, &on_dev); }
  long cells(size_t i) const { return (long)count[i] * nx; }
  size_t bytes(size_t i) const { return sizeof(float) * (size_t)width * (size_t)cells(i); }
  float* sums(size_t i) const { return (float*)acc[i].p; }
  float* out_rows(size_t i) const { return out + (size_t)width * (size_t)first[i] * (size_t)nx; }
  // where slab i's means go
  float* at(size_t i) const { return on_dev ? out_rows(i) : sums(i); }
  // the slabs' sums (LBM_ENOMEM: nothing queued; the caller hands it to ranks_agree)
  int prepare() {
    acc.resize(c->slabs.size());
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      Slab& s = c->slabs[i];
      if (count[i] == 0) continue;
      HIPC(hipSetDevice(s.dev));
      if (!device_room(&acc[i].p, bytes(i)))
        return fail(LBM_ENOMEM, "no room on device %d for the %s of slab %zu (%zu bytes)", s.dev, win ? "window sums" : "sums", i, bytes(i));
    }
    return LBM_OK;
  }
  int clear() {
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      Slab& s = c->slabs[i];
      if (count[i] == 0) continue;
      HIPC(hipSetDevice(s.dev));
      HIPC(hipMemsetAsync(acc[i].p, 0, bytes(i), s.sc));
    }
    return LBM_OK;
  }
  // the window rows of other ranks' lattice rows read +0.0f (the whole lattice: a context's output is its own rows, none is foreign)
  int zero_foreign() {
    if (!win || local >= win->ny) return LBM_OK;
    return zero_output(c, out, sizeof(float) * (size_t)width * (size_t)nx * (size_t)win->ny, on_dev);
  }
  // the fields of the stored lattice (and their products) added to the sums, on every slab that owns a row
  int add() {
    int rc;
    for (size_t i = 0; i < c->slabs.size(); ++i)
      if ((rc = win ? launch_window(c, c->slabs[i], *win, first[i], count[i], sums(i), true) : launch_cell_add(c, c->slabs[i], width, sums(i))))
        return rc;
    return LBM_OK;
  }
  int to_host() {
    if (on_dev) return LBM_OK;
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      Slab& s = c->slabs[i];
      if (count[i] == 0) continue;
      HIPC(hipSetDevice(s.dev));
      HIPC(hipMemcpy(out_rows(i), acc[i].p, bytes(i), hipMemcpyDeviceToHost));
    }
    return LBM_OK;
  }
  // the sums of m samples divided into their place (lbm_mean_div: IEEE division), every slab's stream waited for, host
  // output copied out
  int finish(int m) {
    int rc;
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      Slab& s = c->slabs[i];
      if (count[i] > 0 && (rc = launch_mean_div(s, sums(i), cells(i) * (width / 4), m, at(i)))) return rc;
      HIPC(hipSetDevice(s.dev));
      HIPC(hipStreamSynchronize(s.sc));
    }
    return to_host();
  }
  // ---- lbm_run_window_stats on the register tiles
  // the most samples a piece may stage under the bound: at least 1, at most m
  int auto_chunk(int m) const {
    size_t per = 0;                          // bytes of one sample of the slab with the most window cells
    for (size_t i = 0; i < c->slabs.size(); ++i) per = std::max(per, sizeof(float) * 4 * (size_t)cells(i));
    const size_t fit = per ? kWindowStatsStageBytes / per : (size_t)m;
    return (int)std::min<size_t>((size_t)m, std::max<size_t>(1, fit));
  }
  // the staging of `chunk` samples on every slab that holds a window row; false: no room, nothing kept, nothing queued
  bool stage_room(int chunk) {
    stage.clear(); stage.resize(c->slabs.size());
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      Slab& s = c->slabs[i];
      if (count[i] == 0) continue;
      if (hipSetDevice(s.dev) != hipSuccess || !device_room(&stage[i].p, sizeof(float) * 4 * (size_t)cells(i) * (size_t)chunk)) {
        (void)hipGetLastError();
        stage.clear();
        return false;
      }
    }
    return true;
  }
  float* staged(size_t i) const { return stage.empty() ? nullptr : (float*)stage[i].p; }
  // the n samples a register-tile piece staged, added to the sums in step order, behind the piece on every slab's stream
  int fold(int n) {
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      Slab& s = c->slabs[i];
      if (count[i] == 0) continue;
      HIPC(hipSetDevice(s.dev));
      hipLaunchKernelGGL(lbm::lbm_window_stats_fold, dim3(cdiv(cells(i), lbm::kBlock)), dim3(lbm::kBlock), 0, s.sc, staged(i), cells(i), n,
                         c->p.density, sums(i));
      HIPC(hipGetLastError());
    }
    return LBM_OK;
  }
};

// The tile pieces of run_split, for a call that tries each piece on the register tiles first, in the piece flavour
// (RegFlavour::piece, which alone folds the last step's speed sum of a piece that is not the call's last as a whole run
// folds it there, piece_mid -- av_vels is lbm_run's bits wherever the call is cut): a piece takes `chunk` samples, cc of
// them where fewer are left (0: the tail).
struct TilePieces {
  bool on = false;                                 // would the tiles run the pieces (decided with ranks_agree)
  int chunk = 1;
  std::function<void(int cc, RunKind& k)> fill;    // completes the RunKind of a piece of cc samples (none: nothing to add)
  std::function<int(int cc)> behind;               // behind a piece of cc > 0 samples that ran (none: after_sample, chunk 1)
  int pieces = 0;                                  // on return: the pieces that ran, on the tiles or off them
};

// The step loop split at the sample steps every, 2 every, ... m every, then the tail: each piece a complete plain run_steps
// (the register tiles may run it) with after_sample(j) behind piece j < m on the stored lattice.  Correct, not fast.
// With tile pieces (tp) each piece is tried on the tiles first; one that gives up, or whose flavour is not resident, has
// stepped nothing: the plain piece from the same `done`, and plain pieces for the rest of the call.
template <class After>
int run_split(lbm_ctx* c, int nsteps, float* av_vels, int every, int m, After after_sample, TilePieces* tp = nullptr) {
  double gpu_ms = 0.0, wall_ms = 0.0;
  int done = 0, taken = 0, pieces = 0, rc;
  bool tiles = tp && tp->on;
  while (done < nsteps) {
    float* av = av_vels ? av_vels + done : nullptr;
    bool ran = false;
    if (tiles && regtile_is_next(c)) {
      const int cc = std::min(tp->chunk, m - taken);
      const int n = cc > 0 ? cc * every : nsteps - done;
      RunKind k;
      k.flavour = RegFlavour::piece; k.piece_mid = done + n < nsteps; k.ran = &ran;
      if (tp->fill) tp->fill(cc, k);
      if ((rc = run_steps(c, n, av, k))) return rc;
      tiles = ran;
      if (ran && cc > 0 && (rc = tp->behind ? tp->behind(cc) : after_sample(taken))) return rc;
      if (ran) { taken += cc; done += n; }
    }
    if (!ran) {
      const int n = taken < m ? every : nsteps - done;
      if ((rc = run_steps(c, n, av))) return rc;
      done += n;
      if (taken < m && (rc = after_sample(taken++))) return rc;
    }
    gpu_ms += c->gpu_ms; wall_ms += c->wall_ms;
    ++pieces;
  }
  c->gpu_ms = gpu_ms; c->wall_ms = wall_ms;
  if (tp) tp->pieces = pieces;
  return LBM_OK;
}

// Everything a slab holds for the observer calls (slab_free): the cell lists, the four tables, the four grown buffers, lbm_wave's maps
void observers_free(Slab& s) {
  if (s.fcells) (void)hipFree(s.fcells);
  if (s.pcells) (void)hipFree(s.pcells);
  s.fcells = nullptr; s.pcells = nullptr; s.fcells_n = 0;
  for (TileTable* t : {&s.tforces, &s.tprobes, &s.twindow, &s.tnone}) tile_table_free(*t);
  for (GrownBuf* b : {&s.rpartials, &s.fpart, &s.dtab, &s.fcontrib}) grown_free(*b);
  wave_force_free(s);
  wave_probe_free(s, true);
}

// room on a slab's device for the (a1, a2) pairs of a schedule of nsteps steps (Slab::dtab; lbm_run_driven and
// lbm_run_driven_observed on the register tiles).  false: no room, nothing queued -- the caller keeps off the tiles
bool drive_table_room(Slab& s, int nsteps) { return grown_room(s, s.dtab, nsteps, 2, true); }

}  // namespace

extern "C" int lbm_run_sampled(lbm_ctx* c, int nsteps, float* av_vels, int every, float* fields_out) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (nsteps < 0) return fail(LBM_EINVAL, "nsteps < 0");
  if (every < 0) return fail(LBM_EINVAL, "every < 0");
  const int m = every > 0 ? nsteps / every : 0;
  if (m > 0 && !fields_out) return fail(LBM_EINVAL, "fields_out is NULL but %d snapshot(s) are due", m);
  c->samples_in_kernel = 0; c->samples_in_wave = 0;
  if (m == 0) return run_steps(c, nsteps, av_vels);
  if (int refused = refuse_failed(c)) return refused;
  // ---- everything that can fail for want of room or a wrong pointer is decided here, before anything is queued
  const int nx = c->p.nx;
  const int base_row = c->rank_mode ? c->slabs[0].row0 : 0;
  long rows = 0;
  for (auto& s : c->slabs) rows += s.nyl;
  const long slot = rows * nx * 4;                          // floats per snapshot
  if ((unsigned long long)m > (unsigned long long)(PTRDIFF_MAX / 4) / (unsigned long long)slot)
    return fail(LBM_EINVAL, "%d snapshots of %ld floats do not fit the address space", m, slot);
  bool on_dev = false;
  int rc;
  if ((rc = output_on_device(c, fields_out, "fields_out", &on_dev))) return rc;
  if (regtile_is_next(c)) {
    // ---- in the kernel: straight into device output, or into one staging buffer per slab copied out after the run
    SnapPlan sp;
    sp.every = every;
    std::vector<DeviceTemp> stage(c->slabs.size());
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      Slab& s = c->slabs[i];
      if (on_dev) { sp.at.push_back(fields_out + 4L * (s.row0 - base_row) * nx); sp.stride.push_back(slot); continue; }
      HIPC(hipSetDevice(s.dev));
      const size_t bytes = sizeof(float) * 4 * (size_t)m * (size_t)s.nyl * (size_t)nx;
      if (!device_room(&stage[i].p, bytes)) return fail(LBM_ENOMEM, "no room on device %d for %d snapshot(s) of slab %zu (%zu bytes)", s.dev, m, i, bytes);
      sp.at.push_back((float*)stage[i].p); sp.stride.push_back((long)s.nyl * nx * 4);
    }
    RunKind k;
    k.flavour = RegFlavour::snapshots; k.snap = &sp;
    if ((rc = run_steps(c, nsteps, av_vels, k))) return rc;
    if (c->samples_in_kernel) {
      if (!on_dev)
        for (size_t i = 0; i < c->slabs.size(); ++i) {
          Slab& s = c->slabs[i];
          HIPC(hipSetDevice(s.dev));
          const size_t w = sizeof(float) * 4 * (size_t)s.nyl * (size_t)nx;
          HIPC(hipMemcpy2D(fields_out + 4L * (s.row0 - base_row) * nx, sizeof(float) * (size_t)slot, stage[i].p, w, w, (size_t)m,
                           hipMemcpyDeviceToHost));
        }
      return LBM_OK;
    }
    // (the register tiles did not run, or gave up with the lattice untouched: the pieces below repeat the run)
  }
  // ---- where lbm_run would run lbm_wave (a lattice alone): ONE run, the groups of K steps that hold a sample step in
  // lbm_wave's field flavour, which stores every delivered cell's fields at the sample levels of a pass; lbm_derive behind
  // the left-over steps that are sample steps.  Device output is written in place, host output goes through one staging of
  // the m snapshots.  Decided here, before anything is queued; a staging that does not fit: the pieces below, the same bits.
  if (nsteps >= c->time_block && wave_admit(c, false)) {
    Slab& s = c->slabs[0];
    HIPC(hipSetDevice(s.dev));
    DeviceTemp stage, part;
    bool room = true;
    if (!on_dev && !device_room(&stage.p, sizeof(float) * (size_t)m * (size_t)slot)) room = false;
    // (lbm_derive leaves a float and a double per block, unused here; the partial-sum buffers are busy during a run)
    const size_t nblk = (size_t)cdiv((long)s.nyl * nx, lbm::kBlock);
    if (room && !device_room(&part.p, (sizeof(double) + sizeof(float)) * nblk)) room = false;
    if (room) {
      RunKind k;
      k.no_tiles = true; k.wave.fout = on_dev ? fields_out : (float*)stage.p; k.wave.fevery = every; k.wave.fstride = slot;
      k.wave.fmass = (double*)part.p; k.wave.fpart = (float*)(k.wave.fmass + nblk);
      if ((rc = run_steps(c, nsteps, av_vels, k))) return rc;
      if (!on_dev) HIPC(hipMemcpy(fields_out, stage.p, sizeof(float) * (size_t)m * (size_t)slot, hipMemcpyDeviceToHost));
      return LBM_OK;
    }
  }
  // ---- the step loop split at the sample steps: each piece a complete run, then lbm_final_state's derive into its slot
  return run_split(c, nsteps, av_vels, every, m,
                   [&](int j) { return derive_all(c, fields_out + (size_t)j * (size_t)slot, nullptr, nullptr, on_dev); });
}

extern "C" int lbm_set_bodies(lbm_ctx* c, const int* body, int nbodies) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (nbodies < 0 || nbodies > LBM_MAX_BODIES) return fail(LBM_EINVAL, "nbodies must be in [0, %d] (got %d)", LBM_MAX_BODIES, nbodies);
  if (nbodies > 0 && !body) return fail(LBM_EINVAL, "body is NULL");
  const int nx = c->p.nx, ny = c->p.ny;
  // c_i of directions 1..8 (E N W S NE NW SW SE)
  static const int cx[9] = {0, 1, 0, -1, 0, 1, -1, -1, 1}, cy[9] = {0, 0, 1, 0, -1, 1, 1, -1, -1};
  std::vector<std::vector<int4>> lists(c->slabs.size());
  for (size_t k = 0; k < c->slabs.size() && nbodies > 0; ++k) {
    const Slab& s = c->slabs[k];
    for (int y = 0; y < s.nyl; ++y) {
      const int gy = s.row0 + y, ky = gy - c->keep_row0;       // (row of obst_keep)
      for (int x = 0; x < nx; ++x) {
        if (!c->obst_keep[(size_t)ky * nx + x]) continue;       // (labels on fluid cells are ignored)
        const int lab = body[(long)gy * nx + x];
        if (lab < 0 || lab > nbodies) return fail(LBM_EINVAL, "label %d of blocked cell (%d, %d) is outside [0, %d]", lab, x, gy, nbodies);
        if (lab == 0) continue;
        unsigned m = 0u;
        for (int i = 1; i <= 8; ++i) {
          const int sx = ((x - cx[i]) % nx + nx) % nx, sy = ky - cy[i];   // the source cell B - c_i (wraps in x; rows: kept)
          if (!c->obst_keep[(size_t)sy * nx + sx]) m |= 1u << (i - 1);
        }
        if (m) lists[k].push_back(int4{x, y, (int)(m | ((unsigned)lab << 8)), 0});
      }
    }
  }
  (void)ny;
  for (size_t k = 0; k < c->slabs.size(); ++k) {
    Slab& s = c->slabs[k];
    HIPC(hipSetDevice(s.dev));
    if (s.fcells) HIPC(hipFree(s.fcells));
    s.fcells = nullptr; s.fcells_n = 0;
    tile_table_free(s.tforces);         // (the register tiles' table: rebuilt by the next run that counts forces)
    wave_force_free(s);                 // (lbm_wave's force maps follow the list: rebuilt by the next forces run that wants them)
    wave_probe_free(s, false);          // (... and so does the force-and-probe map)
    s.fcells_host.swap(lists[k]);
    if (s.fcells_host.empty()) continue;
    std::vector<int2> dev(s.fcells_host.size());
    for (size_t j = 0; j < dev.size(); ++j)
      dev[j] = int2{s.fcells_host[j].y * s.pitch + s.fcells_host[j].x, s.fcells_host[j].z};
    if (!device_room((void**)&s.fcells, sizeof(int2) * dev.size())) {
      s.fcells_host.clear(); c->nbodies = 0;
      return fail(LBM_ENOMEM, "no room on device %d for %zu body cells", s.dev, dev.size());
    }
    HIPC(hipMemcpy(s.fcells, dev.data(), sizeof(int2) * dev.size(), hipMemcpyHostToDevice));
    s.fcells_n = (int)dev.size();
  }
  c->nbodies = nbodies;
  return LBM_OK;
}

extern "C" int lbm_run_forces(lbm_ctx* c, int nsteps, float* av_vels, float* forces) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (nsteps < 0) return fail(LBM_EINVAL, "nsteps < 0");
  if (c->nbodies == 0) return fail(LBM_EINVAL, "no bodies are set (lbm_set_bodies)");
  if (nsteps > 0 && !forces) return fail(LBM_EINVAL, "forces is NULL");
  c->forces_in_kernel = 0; c->forces_in_wave = 0;
  if (nsteps == 0) return run_steps(c, 0, av_vels);
  if (int refused = refuse_failed(c)) return refused;
  const int nb = c->nbodies;
  const long nval = 2L * nb * nsteps;
  if (nval + nsteps + 1 > (1L << 30)) return fail(LBM_EINVAL, "a forces run of %d steps is too long (split it)", nsteps);
  // ---- everything that can fail for want of room is decided here, before anything is queued
  int rc = LBM_OK;
  for (auto& s : c->slabs)
    if (ensure_sums(s, (int)(nsteps + 1 + nval))) { (void)hipGetLastError(); return fail(LBM_ENOMEM, "no room for the sums of %d steps and their forces", nsteps); }
  bool in_kernel = regtile_is_next(c);
  if (in_kernel) {
    for (auto& s : c->slabs)
      if ((rc = force_tables(s, c->tplan.ty, c->tplan.ntx, nsteps))) break;
  }
  if ((rc = ranks_agree(c, rc, &in_kernel, "the force partials"))) return rc;
  RunKind k;
  k.flavour = RegFlavour::forces; k.nb = nb; k.nval = nval; k.no_tiles = !in_kernel;
  if ((rc = run_steps(c, nsteps, av_vels, k))) return rc;
  fetch_forces(c, nsteps, nval, forces);
  return LBM_OK;
}

extern "C" int lbm_run_mean(lbm_ctx* c, int nsteps, float* av_vels, int every, float* mean_out) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (nsteps < 0) return fail(LBM_EINVAL, "nsteps < 0");
  if (every <= 0) return fail(LBM_EINVAL, "every must be positive (got %d)", every);
  const int m = nsteps / every;
  if (m == 0) return fail(LBM_EINVAL, "nothing to average: no sample step in %d step(s) at every = %d", nsteps, every);
  if (!mean_out) return fail(LBM_EINVAL, "mean_out is NULL");
  c->mean_in_kernel = 0; c->mean_in_wave = 0;
  if (int refused = refuse_failed(c)) return refused;
  // ---- everything that can fail for want of room or a wrong pointer is decided here, before anything is queued
  CellSums mo(c, 4);
  int rc;
  if ((rc = mo.locate(mean_out, "mean_out"))) return rc;
  rc = mo.prepare();
  bool in_kernel = regtile_is_next(c);
  if ((rc = ranks_agree(c, rc, &in_kernel, "the sums"))) return rc;
  if (in_kernel) {
    // ---- in the kernel: the means straight into device output, or into the slab's buffer copied out after the run
    SnapPlan sp;
    sp.every = every;
    for (size_t i = 0; i < c->slabs.size(); ++i) { sp.at.push_back(mo.at(i)); sp.stride.push_back(0); }
    RunKind k;
    k.flavour = RegFlavour::mean; k.snap = &sp;
    if ((rc = run_steps(c, nsteps, av_vels, k))) return rc;
    if (c->mean_in_kernel) return mo.to_host();
    // (the register tiles did not run, or gave up with the lattice untouched and nothing stored: the pieces below repeat the run)
  }
  if ((rc = mo.clear())) return rc;
  // ---- where lbm_run would run lbm_wave (a lattice alone): ONE run, the groups of K steps that hold a sample step in
  // lbm_wave's field flavour, which adds every delivered cell's fields to the slab's sums at the sample levels of a pass, in
  // the order of the steps; lbm_mean_add behind the left-over steps that are sample steps.  The same adds in the same order
  // as below.
  if (nsteps >= c->time_block && wave_admit(c, false)) {
    RunKind k;
    k.no_tiles = true; k.wave.fout = mo.sums(0); k.wave.fevery = every; k.wave.fstride = 0; k.wave.fadd = true;
    if ((rc = run_steps(c, nsteps, av_vels, k))) return rc;
    return mo.finish(m);
  }
  // ---- the step loop split at the sample steps: each piece a complete run, then the fields of the stored lattice added to
  // the slab's sums (no snapshot, no host round trip per sample); the same adds in the same order as in the register tiles.
  if ((rc = run_split(c, nsteps, av_vels, every, m, [&](int) { return mo.add(); }))) return rc;
  return mo.finish(m);
}

extern "C" int lbm_run_stats(lbm_ctx* c, int nsteps, float* av_vels, int every, float* stats_out) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (nsteps < 0) return fail(LBM_EINVAL, "nsteps < 0");
  if (every <= 0) return fail(LBM_EINVAL, "every must be positive (got %d)", every);
  const int m = nsteps / every;
  if (m == 0) return fail(LBM_EINVAL, "nothing to average: no sample step in %d step(s) at every = %d", nsteps, every);
  if (!stats_out) return fail(LBM_EINVAL, "stats_out is NULL");
  c->stats_in_wave = 0;
  if (int refused = refuse_failed(c)) return refused;
  // ---- everything that can fail for want of room or a wrong pointer is decided here, before anything is queued
  CellSums mo(c, 8);
  int rc;
  if ((rc = mo.locate(stats_out, "stats_out"))) return rc;
  rc = mo.prepare();
  // (no sums inside the register tiles; their pieces below run in the piece flavour, with the table of -1s for both of its
  // observers -- no room for that table: plain pieces, nobody fails.  The ranks agree on the room for the sums and on the flavour.)
  bool tiles = regtile_is_next(c);
  for (size_t i = 0; i < c->slabs.size() && tiles; ++i)
    if (empty_table(c->slabs[i], c->tplan.ty, c->tplan.ntx)) tiles = false;
  if ((rc = ranks_agree(c, rc, &tiles, "the sums"))) return rc;
  if ((rc = mo.clear())) return rc;
  // ---- where lbm_run would run lbm_wave (a lattice alone; admission as lbm_run_mean's): ONE run, the groups of K steps that
  // hold a sample step in lbm_wave's stats flavour, lbm_stats_add behind the left-over steps that are sample steps.  The
  // same adds in the same order as below.  (Where lbm_run_mean would keep its sums inside the register tiles, the tiles run
  // the pieces below.)
  if (!regtile_is_next(c) && nsteps >= c->time_block && wave_admit(c, false)) {
    RunKind k;
    k.no_tiles = true; k.wave.fout = mo.sums(0); k.wave.fevery = every; k.wave.fstride = 0; k.wave.fadd = true; k.wave.fstats = true;
    if ((rc = run_steps(c, nsteps, av_vels, k))) return rc;
    return mo.finish(m);
  }
  // ---- the step loop split at the sample steps: each piece a complete run, then the fields of the stored lattice and their
  // products added to the slab's sums.  On a register-tile context the pieces run on the tiles, as lbm_run_observed's do
  // and for its reason: the piece flavour with neither observer wanted (RegFlavour::piece), which alone folds the last
  // step's speed sums of a piece that is not the call's last as a whole run folds them there (piece_mid) -- plain launches
  // would move the last bit of av_vels at every cut.  A flavour that cannot be resident: plain pieces from there on.
  TilePieces tp;
  tp.on = tiles;
  if ((rc = run_split(c, nsteps, av_vels, every, m, [&](int) { return mo.add(); }, &tp))) return rc;
  return mo.finish(m);
}

extern "C" int lbm_set_probes(lbm_ctx* c, const int* xy, int nprobes) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (nprobes < 0 || nprobes > LBM_MAX_PROBES) return fail(LBM_EINVAL, "nprobes must be in [0, %d] (got %d)", LBM_MAX_PROBES, nprobes);
  if (nprobes > 0 && !xy) return fail(LBM_EINVAL, "xy is NULL");
  const int nx = c->p.nx, ny = c->p.ny;
  // ---- the whole set is checked, and the slabs' new lists are on their devices, before anything of the earlier set goes
  std::vector<std::pair<long, int>> seen((size_t)nprobes);
  for (int i = 0; i < nprobes; ++i) {
    const int x = xy[2 * i], y = xy[2 * i + 1];
    if (x < 0 || x >= nx || y < 0 || y >= ny)
      return fail(LBM_EINVAL, "xy[%d] = (%d, %d) is outside the %d x %d lattice", i, x, y, nx, ny);
    seen[i] = {(long)y * nx + x, i};
  }
  std::sort(seen.begin(), seen.end());
  for (int i = 1; i < nprobes; ++i)
    if (seen[i].first == seen[i - 1].first)
      return fail(LBM_EINVAL, "xy[%d] and xy[%d] are the same cell (%d, %d)", seen[i - 1].second, seen[i].second,
                  (int)(seen[i].first % nx), (int)(seen[i].first / nx));
  const size_t ns = c->slabs.size();
  std::vector<std::vector<int4>> lists(ns);
  std::vector<DeviceTemp> fresh(ns);
  for (size_t k = 0; k < ns; ++k) {
    Slab& s = c->slabs[k];
    for (int i = 0; i < nprobes; ++i) {
      const int y = xy[2 * i + 1] - s.row0;
      if (y >= 0 && y < s.nyl) lists[k].push_back(int4{xy[2 * i], y, i, 0});
    }
    if (lists[k].empty()) continue;
    std::vector<int2> dev(lists[k].size());
    for (size_t j = 0; j < dev.size(); ++j) dev[j] = int2{lists[k][j].y * s.pitch + lists[k][j].x, lists[k][j].z};
    HIPC(hipSetDevice(s.dev));
    if (!device_room(&fresh[k].p, sizeof(int2) * dev.size())) return fail(LBM_ENOMEM, "no room on device %d for %zu probe cells", s.dev, dev.size());
    HIPC(hipMemcpy(fresh[k].p, dev.data(), sizeof(int2) * dev.size(), hipMemcpyHostToDevice));
  }
  for (size_t k = 0; k < ns; ++k) {
    Slab& s = c->slabs[k];
    HIPC(hipSetDevice(s.dev));
    if (s.pcells) HIPC(hipFree(s.pcells));
    s.pcells = (int2*)fresh[k].p; fresh[k].p = nullptr;
    s.pcells_host.swap(lists[k]);
    tile_table_free(s.tprobes);     // (the register tiles' table: rebuilt by the next run that takes probes)
    wave_probe_free(s, true);       // (lbm_wave's probe maps likewise)
  }
  c->nprobes = nprobes;
  return LBM_OK;
}

extern "C" int lbm_run_probes(lbm_ctx* c, int nsteps, float* av_vels, int every, float* probes_out) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (c->nprobes == 0) return fail(LBM_EINVAL, "no probes are set (lbm_set_probes)");
  if (nsteps < 0) return fail(LBM_EINVAL, "nsteps < 0");
  if (every <= 0) return fail(LBM_EINVAL, "every must be positive (got %d)", every);
  const int m = nsteps / every;
  if (m == 0) return fail(LBM_EINVAL, "nothing to record: no sample step in nsteps = %d step(s) at every = %d", nsteps, every);
  if (!probes_out) return fail(LBM_EINVAL, "probes_out is NULL");
  c->probes_in_kernel = 0; c->probes_in_wave = 0;
  if (int refused = refuse_failed(c)) return refused;
  // ---- everything that can fail for want of room or a wrong pointer is decided here, before anything is queued
  ProbeOut po(c);
  int rc;
  if ((rc = po.locate(probes_out, "probes_out"))) return rc;
  bool in_kernel = regtile_is_next(c);
  rc = po.prepare(m);
  for (size_t i = 0; i < c->slabs.size() && !rc && in_kernel; ++i) rc = probe_tables(c->slabs[i], c->tplan.ty, c->tplan.ntx);
  if ((rc = ranks_agree(c, rc, &in_kernel, "the probes"))) return rc;
  if ((rc = po.zero_foreign())) return rc;
  if (in_kernel) {
    // ---- in the kernel: every slab's tiles store their probes straight into their places of device output / of the slab's staging
    SnapPlan sp;
    sp.every = every;
    for (size_t i = 0; i < c->slabs.size(); ++i) { sp.at.push_back(po.at(i, 0)); sp.stride.push_back(4L * po.np); }
    RunKind k;
    k.flavour = RegFlavour::probes; k.snap = &sp;
    if ((rc = run_steps(c, nsteps, av_vels, k))) return rc;
    if (c->probes_in_kernel) return po.to_host();
    // (the register tiles did not run, or gave up with the lattice untouched: the pieces below repeat the run and store every value again)
  }
  // ---- where lbm_run would run lbm_wave (a lattice alone): ONE run, the groups of K steps in lbm_wave's probe flavour, which
  // stores the probes of every sample step of a pass; lbm_probe_gather behind the left-over steps that are sample steps.
  // Decided here, before anything is queued; maps or partials that do not fit: the pieces below, the same bits.
  if (nsteps >= c->time_block && wave_probes_admit(c, false)) {
    RunKind k;
    k.no_tiles = true; k.wave.pout = po.at(0, 0); k.wave.pevery = every; k.pfirst = every;
    if ((rc = run_steps(c, nsteps, av_vels, k))) return rc;
    return po.to_host();
  }
  // ---- the step loop split at the sample steps: each piece a complete run, then the probes' cells of the stored lattice
  // gathered into row j
  if ((rc = run_split(c, nsteps, av_vels, every, m, [&](int j) { return po.gather(j); }))) return rc;
  if ((rc = wait_slabs(c))) return rc;
  return po.to_host();
}

// ----------------------------------------------------------------- windows (lbm_run_window)
static_assert(sizeof(lbm_window) == 24 && offsetof(lbm_window, x0) == 0 && offsetof(lbm_window, y0) == 4 && offsetof(lbm_window, nx) == 8 &&
              offsetof(lbm_window, ny) == 12 && offsetof(lbm_window, sx) == 16 && offsetof(lbm_window, sy) == 20, "the layout lbm_mi355x.h states");

// Is w a window of an nx x ny lattice?  64-bit arithmetic: coordinates near INT_MAX must not wrap.
static int window_check(const lbm_window* w, int nx, int ny) {
  if (!w) return fail(LBM_EINVAL, "win is NULL");
  if (nx < 1 || ny < 1) return fail(LBM_EINVAL, "a %d x %d lattice holds no window", nx, ny);
  if (w->nx < 1 || w->ny < 1 || w->sx < 1 || w->sy < 1)
    return fail(LBM_EINVAL, "a window needs nx, ny, sx, sy >= 1 (got %d x %d cells at strides %d, %d)", w->nx, w->ny, w->sx, w->sy);
  if (w->x0 < 0 || w->y0 < 0) return fail(LBM_EINVAL, "a window starts inside the lattice (got x0 = %d, y0 = %d)", w->x0, w->y0);
  const long long xl = (long long)w->x0 + ((long long)w->nx - 1) * (long long)w->sx, yl = (long long)w->y0 + ((long long)w->ny - 1) * (long long)w->sy;
  if (xl >= nx || yl >= ny)
    return fail(LBM_EINVAL, "the window's last cell (%lld, %lld) is outside the %d x %d lattice (windows do not wrap)", xl, yl, nx, ny);
  return LBM_OK;
}

extern "C" int lbm_window_rows(const lbm_window* w, int nx, int ny, int row_begin, int row_end, int* first, int* count) {
  int rc;
  if ((rc = window_check(w, nx, ny))) return rc;
  if (row_begin > row_end) return fail(LBM_EINVAL, "row_begin %d > row_end %d", row_begin, row_end);
  // window row r lies at lattice row y0 + r sy: the r with row_begin <= y0 + r sy < row_end
  auto rows_below = [&](long long row) -> long long {    // window rows whose lattice row is < row
    const long long d = row - (long long)w->y0;
    if (d <= 0) return 0;
    return std::min<long long>(w->ny, (d + w->sy - 1) / w->sy);
  };
  const long long a = rows_below(row_begin), b = rows_below(row_end);
  if (first) *first = (int)a;
  if (count) *count = (int)(b - a);
  return LBM_OK;
}

namespace {

// The window table of a slab for tiles of ty rows, fed to the probe flavour as the probe set's is: a cell's word is its place
// among the SLAB's window rows + 1, (r - first) w.nx + c + 1 -- the slab's output pointer is its first window row's.  Kept by
// (window, tiling); the probe set's table is not touched.  LBM_ENOMEM: nothing queued.  The key names a window only once its
// table stands: tile_table_set can return before it has touched the old table (its hipSetDevice), which would otherwise be
// left under the new window's key and the old tiling -- a hit for the next call with this window.
int window_tables(Slab& s, int ty, int ntx, const lbm_window& w, int first, int count) {
  if (s.twindow.ty == ty && memcmp(&s.wkey, &w, sizeof(w)) == 0) return LBM_OK;
  std::vector<TileCell> cells;
  for (int r = 0; r < count; ++r)
    for (int cc = 0; cc < w.nx; ++cc)
      cells.push_back({(int)((long)w.x0 + (long)cc * w.sx), (int)((long)w.y0 + (long)(first + r) * w.sy - s.row0), (uint32_t)((long)r * w.nx + cc) + 1u});
  const int rc = tile_table_set(s, s.twindow, ty, ntx, cells, "window");
  if (rc) return rc;
  s.wkey = w;
  return LBM_OK;
}

// Where one call's windows go, [m][w.ny][w.nx][4] floats.  Device output is written in place; host output goes through one
// staging buffer per slab that holds a window row, of the slab's own window rows only -- [m][count][w.nx][4], copied out by
// to_host -- or, where that does not fit, of ONE sample (`single`: the split path alone, copied out behind each sample).
struct WindowOut : SlabRows {             // (per slab: its window rows)
  lbm_ctx* c;
  lbm_window w;
  float* out = nullptr;
  bool on_dev = false, single = false;
  int m = 0;
  size_t wfloats;                          // floats of one window
  std::vector<DeviceTemp> stage;

  WindowOut(lbm_ctx* ctx, const lbm_window& win) : SlabRows(ctx, &win), c(ctx), w(win), wfloats(4 * (size_t)win.nx * (size_t)win.ny) {}
  int locate(float* o, const char* what) { out = o; return output_on_device(c, o, what, &on_dev); }
  size_t slab_floats(size_t i) const { return 4 * (size_t)w.nx * (size_t)count[i]; }
  // the staging of m_ samples, or of one (LBM_ENOMEM: nothing queued, nothing kept)
  int prepare(int m_, bool one) {
    m = m_; single = one;
    stage.clear(); stage.resize(c->slabs.size());
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      Slab& s = c->slabs[i];
      if (on_dev || count[i] == 0) continue;
      const size_t bytes = sizeof(float) * slab_floats(i) * (size_t)(one ? 1 : m);
      HIPC(hipSetDevice(s.dev));
      if (!device_room(&stage[i].p, bytes)) return fail(LBM_ENOMEM, "no room on device %d for %d window(s) of slab %zu (%zu bytes)", s.dev, one ? 1 : m, i, bytes);
    }
    return LBM_OK;
  }
  // the window rows of other ranks' lattice rows read +0.0f
  int zero_foreign() { return local >= w.ny ? LBM_OK : zero_output(c, out, sizeof(float) * wfloats * (size_t)m, on_dev); }
  // where slab i's first window row of sample j goes (a slab without a window row stores nothing: NULL), and the floats
  // from one sample to the next there
  long stride(size_t i) const { return on_dev ? (long)wfloats : (long)slab_floats(i); }
  float* at(size_t i, int j) const {
    if (count[i] == 0) return nullptr;
    if (on_dev) return out + (size_t)j * wfloats + 4 * (size_t)first[i] * (size_t)w.nx;
    return (float*)stage[i].p + (single ? 0 : (size_t)j * slab_floats(i));
  }
  float* host_at(size_t i, int j) const { return out + (size_t)j * wfloats + 4 * (size_t)first[i] * (size_t)w.nx; }
  // the window cells of the stored lattice into sample j, on every slab that holds a window row
  int derive(int j) {
    int rc;
    for (size_t i = 0; i < c->slabs.size(); ++i)
      if ((rc = launch_window(c, c->slabs[i], w, first[i], count[i], at(i, j), false))) return rc;
    if (!single || on_dev) return LBM_OK;
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      Slab& s = c->slabs[i];
      if (count[i] == 0) continue;
      HIPC(hipSetDevice(s.dev));
      HIPC(hipStreamSynchronize(s.sc));
      HIPC(hipMemcpy(host_at(i, j), stage[i].p, sizeof(float) * slab_floats(i), hipMemcpyDeviceToHost));
    }
    return LBM_OK;
  }
  // every slab's stream waited for, and what was staged into the caller's array
  int finish() {
    int rc;
    if ((rc = wait_slabs(c))) return rc;
    for (size_t i = 0; i < c->slabs.size(); ++i) {
      if (on_dev || single || count[i] == 0) continue;
      HIPC(hipSetDevice(c->slabs[i].dev));
      const size_t wbytes = sizeof(float) * slab_floats(i);
      if (count[i] == w.ny) HIPC(hipMemcpy(out, stage[i].p, wbytes * (size_t)m, hipMemcpyDeviceToHost));
      else HIPC(hipMemcpy2D(host_at(i, 0), sizeof(float) * wfloats, stage[i].p, wbytes, wbytes, (size_t)m, hipMemcpyDeviceToHost));
    }
    return LBM_OK;
  }
};

// the window as lbm_wave's window flavour tests it; false: a multiply-high would not be exact (extent x stride >= 2^32)
bool window_for_wave(const lbm_window& w, lbm::WaveWin* out) {
  const unsigned long long sx = w.nx > 1 ? (unsigned)w.sx : 1u, sy = w.ny > 1 ? (unsigned)w.sy : 1u;
  const unsigned long long xl = (unsigned long long)(w.nx - 1) * sx, yl = (unsigned long long)(w.ny - 1) * sy;
  if (xl * sx >= (1ull << 32) || yl * sy >= (1ull << 32)) return false;
  out->x0 = w.x0; out->y0 = w.y0; out->nx = w.nx;
  out->sx = (unsigned)sx; out->sy = (unsigned)sy; out->xlast = (unsigned)xl; out->ylast = (unsigned)yl;
  out->mx = sx > 1 ? (unsigned)((1ull << 32) / sx + 1ull) : 0u;
  out->my = sy > 1 ? (unsigned)((1ull << 32) / sy + 1ull) : 0u;
  return true;
}

}  // namespace

extern "C" int lbm_run_window(lbm_ctx* c, int nsteps, float* av_vels, int every, const lbm_window* win, float* window_out) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  int rc;
  if ((rc = window_check(win, c->p.nx, c->p.ny))) return rc;
  if (nsteps < 0) return fail(LBM_EINVAL, "nsteps < 0");
  if (every < 0) return fail(LBM_EINVAL, "every < 0");
  const int m = every > 0 ? nsteps / every : 0;
  if (m > 0 && !window_out) return fail(LBM_EINVAL, "window_out is NULL but %d window(s) are due", m);
  const unsigned long long wfl = 4ull * (unsigned long long)win->nx * (unsigned long long)win->ny;
  if ((unsigned long long)m > (unsigned long long)(PTRDIFF_MAX / 4) / wfl)
    return fail(LBM_EINVAL, "%d windows of %llu floats do not fit the address space", m, wfl);
  WinPlan plan;
  plan.w = *win;
  const bool wave_exact = window_for_wave(plan.w, &plan.wave);
  WindowOut wo(c, plan.w);
  if (m > 0 && (rc = wo.locate(window_out, "window_out"))) return rc;
  c->window_in_kernel = 0; c->window_in_wave = 0;
  if (m == 0) return run_steps(c, nsteps, av_vels);
  if (int refused = refuse_failed(c)) return refused;
  // ---- everything that can fail for want of room is decided here, before anything is queued.  The staging of m windows, or
  // the register tiles' tables, that do not fit: the split path with the staging of one window, the same bits.
  bool in_kernel = regtile_is_next(c);
  bool staged = wo.prepare(m, false) == LBM_OK;
  for (size_t i = 0; i < c->slabs.size() && staged && in_kernel; ++i)
    in_kernel = window_tables(c->slabs[i], c->tplan.ty, c->tplan.ntx, plan.w, wo.first[i], wo.count[i]) == LBM_OK;
  rc = staged ? LBM_OK : wo.prepare(m, true);
  in_kernel = in_kernel && staged;
  if ((rc = ranks_agree(c, rc, &in_kernel, "the window"))) return rc;
  if ((rc = wo.zero_foreign())) return rc;
  if (in_kernel) {
    // ---- in the kernel: the probe flavour of the register tiles, every slab's tiles store their window cells straight
    // into their places of device output / of the slab's staging
    SnapPlan sp;
    sp.every = every;
    for (size_t i = 0; i < c->slabs.size(); ++i) { sp.at.push_back(wo.at(i, 0)); sp.stride.push_back(wo.stride(i)); }
    RunKind k;
    k.flavour = RegFlavour::window; k.snap = &sp;
    if ((rc = run_steps(c, nsteps, av_vels, k))) return rc;
    if (c->window_in_kernel) return wo.finish();
    // (the register tiles did not run, or gave up with the lattice untouched: the paths below repeat the run and store every cell again)
  }
  // ---- where lbm_run would run lbm_wave (a lattice alone; admission as lbm_run_sampled's): ONE run, the groups of K steps
  // that hold a sample step in lbm_wave's window flavour, lbm_derive_window behind the left-over steps that are sample steps.
  // Device output is written in place, host output goes through the one staging of the m windows.
  if (staged && wave_exact && nsteps >= c->time_block && wave_admit(c, false)) {
    RunKind k;
    k.no_tiles = true; k.wave.fout = wo.at(0, 0); k.wave.fevery = every; k.wave.fstride = wo.stride(0); k.wave.win = &plan;
    if ((rc = run_steps(c, nsteps, av_vels, k))) return rc;
    return wo.finish();
  }
  // ---- the step loop split at the sample steps: each piece a complete run, then the window cells of the stored lattice
  // derived into sample j on every local slab
  if ((rc = run_split(c, nsteps, av_vels, every, m, [&](int j) { return wo.derive(j); }))) return rc;
  return wo.finish();
}

// ----------------------------------------------------------------- stats over a window (lbm_run_window_stats; DESIGN.md 3.20)
extern "C" int lbm_run_window_stats(lbm_ctx* c, int nsteps, float* av_vels, int every, const lbm_window* win, float* stats_out) {
  // (the three pointers first, each on its own: none of them is optional, whatever the other arguments say)
  if (!win) return fail(LBM_EINVAL, "win is NULL");
  if (!stats_out) return fail(LBM_EINVAL, "stats_out is NULL");
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  int rc;
  if ((rc = window_check(win, c->p.nx, c->p.ny))) return rc;
  if (nsteps < 0) return fail(LBM_EINVAL, "nsteps < 0");
  if (every <= 0) return fail(LBM_EINVAL, "every must be positive (got %d)", every);
  const int m = nsteps / every;
  if (m == 0) return fail(LBM_EINVAL, "nothing to average: no sample step in %d step(s) at every = %d", nsteps, every);
  WinPlan plan;
  plan.w = *win;
  const bool wave_exact = window_for_wave(plan.w, &plan.wave);
  CellSums ws(c, 8, &plan.w);
  if ((rc = ws.locate(stats_out, "stats_out"))) return rc;
  c->window_stats_in_wave = 0; c->window_stats_in_kernel = 0; c->window_stats_pieces = 0;
  if (int refused = refuse_failed(c)) return refused;
  // ---- everything that can fail for want of room is decided here, before anything is queued.  The sums must fit; the
  // register tiles' tables or staging that do not: the split path, the same bits, nobody fails.
  rc = ws.prepare();
  bool tiles = regtile_is_next(c);
  const int chunk = c->window_stats_chunk > 0 ? std::min(c->window_stats_chunk, m) : ws.auto_chunk(m);
  for (size_t i = 0; i < c->slabs.size() && !rc && tiles; ++i)
    tiles = window_tables(c->slabs[i], c->tplan.ty, c->tplan.ntx, plan.w, ws.first[i], ws.count[i]) == LBM_OK &&
            empty_table(c->slabs[i], c->tplan.ty, c->tplan.ntx) == LBM_OK;
  if (!rc && tiles) tiles = ws.stage_room(chunk);
  if ((rc = ranks_agree(c, rc, &tiles, "the window sums"))) return rc;
  if ((rc = ws.zero_foreign())) return rc;
  if ((rc = ws.clear())) return rc;
  // ---- where lbm_run would run lbm_wave (a lattice alone; admission as lbm_run_stats'): ONE run, the groups of K steps that
  // hold a sample step in lbm_wave's window-stats flavour, lbm_window_stats_add behind the left-over steps that are sample
  // steps.  A window whose multiply-high would not be exact: the pieces below, the same bits.
  if (!regtile_is_next(c) && wave_exact && nsteps >= c->time_block && wave_admit(c, false)) {
    RunKind k;
    k.no_tiles = true; k.wave.fout = ws.sums(0); k.wave.fevery = every; k.wave.fstride = 0; k.wave.fadd = true; k.wave.fstats = true;
    k.wave.win = &plan;
    if ((rc = run_steps(c, nsteps, av_vels, k))) return rc;
    c->window_stats_pieces = 1;
    return ws.finish(m);
  }
  // ---- the pieces.  On the register tiles: `chunk` sample steps a piece, in the piece flavour (RegFlavour::piece, which
  // alone knows a first-sample phase and folds a cut piece's last step sum as a whole run folds it, piece_mid: av_vels is
  // lbm_run's bits wherever the call is cut) fed the window tables as its probe tables and the table of -1s for forces; it
  // stores the piece's samples into the slab's staging, lbm_window_stats_fold adds them to the sums behind it; the steps
  // past m every run as one more piece without samples.  A piece that gives up, or whose flavour is not resident, has
  // stepped nothing: from the same step on, and everywhere else, pieces of `every` steps with lbm_window_stats_add behind each.
  SnapPlan sp;
  sp.every = every;
  for (size_t i = 0; i < c->slabs.size(); ++i) { sp.at.push_back(ws.staged(i)); sp.stride.push_back(4 * ws.cells(i)); }
  TilePieces tp;
  tp.on = tiles; tp.chunk = chunk;
  tp.fill = [&](int cc, RunKind& k) { if (cc > 0) { k.snap = &sp; k.pfirst = every; k.win_table = true; } };
  tp.behind = [&](int cc) { const int r = ws.fold(cc); if (!r) c->window_stats_in_kernel = 1; return r; };
  if ((rc = run_split(c, nsteps, av_vels, every, m, [&](int) { return ws.add(); }, &tp))) return rc;
  c->window_stats_pieces = tp.pieces;
  return ws.finish(m);
}

static_assert(sizeof(lbm_observe) == 48 && offsetof(lbm_observe, forces) == 0 && offsetof(lbm_observe, probes_out) == 8 &&
              offsetof(lbm_observe, mean_out) == 16 && offsetof(lbm_observe, fields_out) == 24 && offsetof(lbm_observe, probes_every) == 32 &&
              offsetof(lbm_observe, mean_every) == 36 && offsetof(lbm_observe, fields_every) == 40, "the layout lbm_mi355x.h states");

// lbm_run_observed and lbm_run_driven_observed (driven; accel: the schedule, float[nsteps] of host memory, checked by the
// caller): one body, one copy of the cutting logic.  Under a schedule (DESIGN.md 3.17):
//   - every piece is handed its part of the schedule: RunKind::drive is the host table of (a1, a2) pairs advanced by `done`
//     pairs; the register tiles run kRegForce | kRegProbe | kRegDrive on the device table (Slab::dtab: the whole call's,
//     uploaded once in front of the first piece; RunKind::drive_at = done);
//   - there are no driven single calls: one observer alone goes through the pieces too (none wanted: lbm_run_driven itself);
//   - forces ride in lbm_wave launches where run_steps finds both the force and the driven flavour admitted, probes where
//     wave_probes_admit says yes -- one flavour with all three, an observer that is not wanted marks nothing in its map;
//   - the keys are "driven_observed_in_kernel", "driven_observed_in_wave", "driven_observed_pieces".
static int run_observed(lbm_ctx* c, int nsteps, float* av_vels, const lbm_observe* what, bool driven, const float* accel) {
  int& key_kernel = driven ? c->driven_observed_in_kernel : c->observed_in_kernel;
  int& key_wave = driven ? c->driven_observed_in_wave : c->observed_in_wave;
  int& key_pieces = driven ? c->driven_observed_pieces : c->observed_pieces;
  const bool wf = what && what->forces, wp = what && what->probes_out, wm = what && what->mean_out;
  bool ws = what && what->fields_out;
  const int pe = wp ? what->probes_every : 0, me = wm ? what->mean_every : 0, se = ws ? what->fields_every : 0;
  // ---- refusals: nothing queued, the lattice untouched
  if (wf && c->nbodies == 0) return fail(LBM_EINVAL, "forces are wanted but no bodies are set (lbm_set_bodies)");
  if (wp && c->nprobes == 0) return fail(LBM_EINVAL, "probes are wanted but no probes are set (lbm_set_probes)");
  if (wp && pe <= 0) return fail(LBM_EINVAL, "probes_every must be positive (got %d)", pe);
  if (wp && nsteps / pe == 0) return fail(LBM_EINVAL, "nothing to record: no sample step in nsteps = %d step(s) at probes_every = %d", nsteps, pe);
  if (wm && me <= 0) return fail(LBM_EINVAL, "mean_every must be positive (got %d)", me);
  if (wm && nsteps / me == 0) return fail(LBM_EINVAL, "nothing to average: no sample step in %d step(s) at mean_every = %d", nsteps, me);
  if (ws && se < 0) return fail(LBM_EINVAL, "fields_every < 0");
  const int mp = wp ? nsteps / pe : 0, mm = wm ? nsteps / me : 0, msn = (ws && se > 0) ? nsteps / se : 0;
  if (msn == 0) ws = false;                               // (no snapshot is due: legal, nothing written, as lbm_run_sampled)
  if (int refused = refuse_failed(c)) return refused;
  ProbeOut po(c);
  CellSums mo(c, 4);
  bool s_dev = false;
  int rc;
  if (wp && (rc = po.locate(what->probes_out, "probes_out"))) return rc;
  if (wm && (rc = mo.locate(what->mean_out, "mean_out"))) return rc;
  if (ws && (rc = output_on_device(c, what->fields_out, "fields_out", &s_dev))) return rc;
  key_kernel = 0; key_wave = 0; key_pieces = 0;
  if (wf) c->forces_in_wave = 0;                          // (set by any piece whose forces rode in lbm_wave launches)
  // ---- none, or one alone: the call itself (under a schedule: none is lbm_run_driven, one alone goes through the pieces)
  const int wanted = (wf ? 1 : 0) + (wp ? 1 : 0) + (wm ? 1 : 0) + (ws ? 1 : 0);
  if (driven && nsteps == 0) return run_steps(c, 0, av_vels);   // (success, nothing runs)
  if (driven && wanted == 0) {
    const int r = lbm_run_driven(c, nsteps, av_vels, accel);
    if (!r && nsteps > 0 && (c->driven_in_kernel || c->driven_in_wave)) key_pieces = 1;
    return r;
  }
  if (!driven && wanted <= 1) {
    if (wf) { rc = lbm_run_forces(c, nsteps, av_vels, what->forces); if (!rc && c->forces_in_kernel) c->observed_in_kernel = 1; if (!rc && c->forces_in_wave) c->observed_in_wave = 1; }
    else if (wp) { rc = lbm_run_probes(c, nsteps, av_vels, pe, what->probes_out); if (!rc && c->probes_in_kernel) c->observed_in_kernel = 2; if (!rc && c->probes_in_wave) c->observed_in_wave = 2; }
    else if (wm) { rc = lbm_run_mean(c, nsteps, av_vels, me, what->mean_out); if (!rc && c->mean_in_kernel) c->observed_in_kernel = 4; }
    else if (ws) { rc = lbm_run_sampled(c, nsteps, av_vels, se, what->fields_out); if (!rc && c->samples_in_kernel) c->observed_in_kernel = 8; }
    else rc = lbm_run(c, nsteps, av_vels);
    if (!rc) {
      const int m = wp ? mp : wm ? mm : ws ? msn : 0, ev = wp ? pe : wm ? me : se;
      // (a lone mean or snapshot series that rode in lbm_wave launches ran in one piece too; observed_in_wave keeps its two bits)
      const bool fields_in_wave = (wm && c->mean_in_wave) || (ws && c->samples_in_wave);
      c->observed_pieces = (wanted == 0 || wf || c->observed_in_kernel != 0 || c->observed_in_wave != 0 || fields_in_wave) ? 1 : m + (nsteps > m * ev ? 1 : 0);
    }
    return rc;
  }
  // ---- two or more.  Everything that can fail for want of room is decided here, before anything is queued.
  const int nx = c->p.nx, nb = c->nbodies, np = c->nprobes;
  const size_t ns = c->slabs.size();
  long rows = 0;
  for (auto& s : c->slabs) rows += s.nyl;
  const long slot = rows * nx * 4;                        // floats per snapshot
  if (ws && (unsigned long long)msn > (unsigned long long)(PTRDIFF_MAX / 4) / (unsigned long long)slot)
    return fail(LBM_EINVAL, "%d snapshots of %ld floats do not fit the address space", msn, slot);
  if (wf && 2L * nb * nsteps + nsteps + 1 > (1L << 30)) return fail(LBM_EINVAL, "a forces run of %d steps is too long (split it)", nsteps);
  bool tiles = regtile_is_next(c);
  rc = LBM_OK;
  for (size_t i = 0; i < ns && !rc; ++i) {
    Slab& s = c->slabs[i];
    HIPC(hipSetDevice(s.dev));
    if (wf && ensure_sums(s, (int)(nsteps + 1 + 2L * nb * nsteps))) {
      (void)hipGetLastError();
      rc = fail(LBM_ENOMEM, "no room for the sums of %d steps and their forces", nsteps);
    }
    if (!rc && tiles && !(wf && wp)) rc = empty_table(s, c->tplan.ty, c->tplan.ntx);
    if (!rc && wf && tiles) rc = force_tables(s, c->tplan.ty, c->tplan.ntx, nsteps);
    if (!rc && wp && tiles) rc = probe_tables(s, c->tplan.ty, c->tplan.ntx);
  }
  if (!rc && wp) rc = po.prepare(mp);
  if (!rc && wm) rc = mo.prepare();
  // the schedule: the pairs made on the host by run_steps' own expression, as lbm_run_driven makes them; room for the whole
  // call's table on every slab's device where the tiles would run -- no room: the call keeps off the tiles, nobody fails
  std::vector<float> pairs;
  if (driven) {
    pairs = accel_pairs(c, accel, nsteps);
    for (size_t i = 0; i < ns && !rc && tiles; ++i)
      if (!drive_table_room(c->slabs[i], nsteps)) tiles = false;
  }
  if ((rc = ranks_agree(c, rc, &tiles, "the observers' buffers"))) return rc;
  if (driven && tiles)
    for (auto& s : c->slabs) {
      HIPC(hipSetDevice(s.dev));
      HIPC(hipMemcpyAsync(s.dtab.p, pairs.data(), sizeof(float) * 2 * (size_t)nsteps, hipMemcpyHostToDevice, s.sc));
    }
  // probes where lbm_run would run lbm_wave (a lattice alone): they ride in its launches, beside the forces if those are
  // wanted, and cut no piece; decided here, before anything is queued (no: lbm_probe_gather behind pieces cut at their steps)
  const bool pwave = wp && !rc && !tiles && wave_probes_admit(c, wf);
  int wbits = 0;
  if (wp && (rc = po.zero_foreign())) return rc;
  if (wm && (rc = mo.clear())) return rc;
  // ---- the pieces
  double gpu_ms = 0.0, wall_ms = 0.0;
  int done = 0, pieces = 0, bits = 0, jsnap = 0;
  bool in_launches = false;                               // (under a schedule) a piece ran on the tiles, or its groups of K steps in lbm_wave
  while (done < nsteps) {
    const bool on_tiles = tiles && regtile_is_next(c);
    int next = nsteps;
    if (wm) next = std::min<long>(next, ((long)done / me + 1) * me);
    if (ws) next = std::min<long>(next, ((long)done / se + 1) * se);
    if (wp && !on_tiles && !pwave) next = std::min<long>(next, ((long)done / pe + 1) * pe);
    const int n = next - done;
    const long nval = wf ? 2L * nb * n : 0;
    const int jp = wp ? done / pe : 0;                    // the probes' samples taken before this piece
    float* av = av_vels ? av_vels + done : nullptr;
    RunKind k;
    if (wf) { k.nb = nb; k.nval = nval; }
    if (driven) { k.drive = pairs.data() + 2 * (size_t)done; k.drive_at = done; }
    if (on_tiles) {
      SnapPlan sp;
      sp.every = pe;
      for (size_t i = 0; wp && i < ns; ++i) { sp.at.push_back(po.at(i, jp)); sp.stride.push_back(4L * np); }
      bool ran = false;
      if (wp) { k.snap = &sp; k.pfirst = pe - done % pe; }
      k.flavour = RegFlavour::piece; k.piece_mid = next < nsteps; k.ran = &ran;
      if ((rc = run_steps(c, n, av, k))) return rc;
      if (!ran) { tiles = false; continue; }              // (nothing stepped: this piece again, off the tiles)
      bits |= (wf ? 1 : 0) | (wp ? 2 : 0);
      in_launches = true;
    } else {
      k.no_tiles = true;
      if (pwave) {
        // (the probes' phase runs on from the start of the call: the first sample of this piece, and its row of the output)
        k.wave.pevery = pe; k.pfirst = pe - done % pe; k.wave.pout = po.at(0, jp);
        c->probes_in_wave = 0;
      }
      if (driven) c->driven_in_wave = 0;
      if ((rc = run_steps(c, n, av, k))) return rc;
      if (driven && c->driven_in_wave) in_launches = true;
      if (pwave && c->probes_in_wave) wbits |= 2;
      if (wf && c->forces_in_wave) wbits |= 1;
      if (wp && !pwave && (done + n) % pe == 0 && (rc = po.gather(jp))) return rc;
    }
    if (wf) fetch_forces(c, n, nval, what->forces + 2L * nb * done);
    gpu_ms += c->gpu_ms; wall_ms += c->wall_ms;
    done += n;
    ++pieces;
    if (wm && done % me == 0 && (rc = mo.add())) return rc;
    if (ws && done % se == 0) {
      if ((rc = derive_all(c, what->fields_out + (size_t)jsnap * (size_t)slot, nullptr, nullptr, s_dev))) return rc;
      ++jsnap;
    }
  }
  // ---- the means, and what was staged for the host
  if ((rc = wm ? mo.finish(mm) : wait_slabs(c))) return rc;
  if (wp && (rc = po.to_host())) return rc;
  c->gpu_ms = gpu_ms; c->wall_ms = wall_ms;
  // (under a schedule the three keys read 0 where the whole call took the one-step path)
  key_kernel = bits; key_wave = wbits; key_pieces = (!driven || in_launches) ? pieces : 0;
  return LBM_OK;
}

extern "C" int lbm_run_observed(lbm_ctx* c, int nsteps, float* av_vels, const lbm_observe* what) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (nsteps < 0) return fail(LBM_EINVAL, "nsteps < 0");
  return run_observed(c, nsteps, av_vels, what, false, nullptr);
}

extern "C" int lbm_run_driven_observed(lbm_ctx* c, int nsteps, float* av_vels, const float* accel, const lbm_observe* what) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (nsteps < 0) return fail(LBM_EINVAL, "nsteps < 0");
  if (nsteps > 0 && !accel) return fail(LBM_EINVAL, "accel is NULL");
  for (int t = 0; t < nsteps; ++t)
    if (!std::isfinite(accel[t])) return fail(LBM_EINVAL, "accel[%d] is not finite", t);
  return run_observed(c, nsteps, av_vels, what, true, accel);
}
