// lbm_host_march.inc -- part of lbm_api.hip (included there): the launch groups of the step loop (run_steps), each with a
// branch per halo transport -- the parts they share (sweep_args, sweep2_args, launch_accelerate, launch_fold), single steps and
// pairs, and the marching kernels on the host side: lbm_march and lbm_wave on a lattice alone and across slabs (neighbours'
// rows read in place, under copies and peer-to-peer; ghost bands under RCCL), the wave-slot model that picks chunk heights and
// columns per lane.
namespace {

// Edge launches run on their own high-priority stream, concurrent with the interior launch, only
// when the interior is long enough to pay for the extra cross-stream events (measured on one GPU,
// RCCL self-ring: 8192^2 577 -> 537 us/step, but 1024^2 24 -> 33 us/step): big slabs only.
inline bool split_edge_stream(const lbm_ctx* c, const Slab& s) { return (long)s.nyl * c->p.nx >= (1L << 22); }
inline hipStream_t edge_stream(const lbm_ctx* c, const Slab& s) { return split_edge_stream(c, s) ? s.se : s.sc; }

// ---- the parts of the step loop (run_steps), one copy each
// The accelerate phase of the current lattice, by a launch of its own: the first step of a run, and behind a gather.
int launch_accelerate(const lbm_ctx* c, Slab& s, float a1, float a2) {
  if (s.accel_row < 0) return LBM_OK;
  hipLaunchKernelGGL(lbm::lbm_accelerate_row, dim3(cdiv(c->p.nx, 256)), dim3(256), 0, s.sc,
                     s.lat[c->cur], s.plane, s.pitch, c->p.nx, s.accel_row, s.blocked, a1, a2);
  HIPC(hipGetLastError());
  return LBM_OK;
}

// Folds `steps` steps of the launch of parity q, nb blocks' partials each, into sums + t: behind the last launch of its kind,
// which no next launch folds.
int launch_fold(Slab& s, int q, int steps, int nb, int t) {
  hipLaunchKernelGGL(lbm::lbm_fold_partials, dim3(steps), dim3(lbm::kBlock), 0, s.sc, s.partials[q], nb, s.sums + t, steps > 1 ? nb : 0);
  HIPC(hipGetLastError());
  return LBM_OK;
}

// Partial sums (blocks) of one single-step launch group of a slab: edge rows and interior rows where they are two launches.
int single_partial_count(const lbm_ctx* c, const Slab& s) {
  if (c->exchange == 0 || c->exchange == LBM_EXCHANGE_P2P) return sweep_blocks(c, s.nyl);
  return sweep_blocks(c, s.nyl >= 2 ? 2 : 1) + (s.nyl > 2 ? sweep_blocks(c, s.nyl - 2) : 0);
}

// The arguments of a one-step launch of slab s, launch parity q, as every launch sets them: lattices, geometry, omega, the
// accelerate row (last: none) and pair, the partials of parity q and -- fold_prev -- the fold of the group before, step
// tt - 1.  The caller sets the rows, the ghost rows and the send buffers (value-initialised: none).
lbm::SweepArgs sweep_args(const lbm_ctx* c, const Slab& s, int q, int tt, bool last, bool fold_prev, float a1, float a2) {
  lbm::SweepArgs a{};
  a.src = s.lat[c->cur]; a.dst = s.lat[c->cur ^ 1];
  a.plane = s.plane; a.pitch = s.pitch; a.nx = c->p.nx; a.nyl = s.nyl;
  a.blocked = s.blocked; a.omega = c->p.omega;
  a.accel_row = last ? -1 : s.accel_row;
  a.a1 = a1; a.a2 = a2;
  a.partials = s.partials[q];
  if (fold_prev) { a.prev_partials = s.partials[q ^ 1]; a.prev_count = single_partial_count(c, s); a.prev_sum = s.sums + (tt - 1); }
  return a;
}
// ... and of a two-step launch (steps tt, tt + 1; the fold: of the pair before).  The caller sets the tile rows and, on an
// edge or peer-to-peer launch, the ghost rows, their obstacle bytes, the send buffers and the hand-off.
lbm::Sweep2Args sweep2_args(const lbm_ctx* c, const Slab& s, int q, int tt, bool accel_out, bool fold_prev, float a1, float a2) {
  const int nbtot = t2_tiles(c, s.nyl);
  lbm::Sweep2Args a{};
  a.src = s.lat[c->cur]; a.dst = s.lat[c->cur ^ 1];
  a.plane = s.plane; a.pitch = s.pitch; a.nx = c->p.nx; a.ny = s.nyl;
  a.blocked = s.blocked; a.omega = c->p.omega;
  a.accel_row = s.accel_row >= 0 ? s.accel_row : lbm::kNoRow;
  a.accel_out = accel_out ? 1 : 0;
  a.a1 = a1; a.a2 = a2;
  a.partials1 = s.partials[q]; a.partials2 = s.partials[q] + nbtot;
  if (fold_prev) { a.prev1 = s.partials[q ^ 1]; a.prev2 = s.partials[q ^ 1] + nbtot; a.prev_count = nbtot; a.prev_sum = s.sums + (tt - 2); }
  return a;
}

// One single-step launch group (all local slabs) for step tt, launch index li, by the context's transport: a slab alone;
// slabs that trade halos through events (RCCL, copies): the edge rows, the exchange, the interior rows; peer-to-peer: group
// ++c->seq -- a wait launch, the rows on the halos of the group before, a push launch.
int launch_single(lbm_ctx* c, int li, int tt, bool last, bool fold_prev, float a1, float a2) {
  const int nx = c->p.nx;
  const int q = li & 1, qp = q ^ 1;
  const bool p2p = c->exchange == LBM_EXCHANGE_P2P, ex = c->exchange != 0 && !p2p;
  const uint32_t seq = p2p ? ++c->seq : 0;
  const long h3 = 3L * nx;  // one-step halos live in slots 3..5 of the nine-slot buffers
  int rc;
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    lbm::SweepArgs a = sweep_args(c, s, q, tt, last, fold_prev, a1, a2);
    a.y_begin = 0; a.y_count = s.nyl; a.y_stride = 1;
    if (c->exchange == 0) {
      // one slab, periodic self-wrap: the halo rows are the slab's own edge rows
      const long top = (long)(s.nyl - 1) * s.pitch;
      a.south2 = a.src + 2 * s.plane + top; a.south5 = a.src + 5 * s.plane + top; a.south6 = a.src + 6 * s.plane + top;
      a.north4 = a.src + 4 * s.plane; a.north7 = a.src + 7 * s.plane; a.north8 = a.src + 8 * s.plane;
      launch_sweep(c, a, s.sc);
      HIPC(hipGetLastError());
      continue;
    }
    const int qg = p2p ? (seq - 1) & 1 : qp;
    const float* gs = s.ghost_s[qg] + h3;
    const float* gn = s.ghost_n[qg] + h3;
    a.south2 = gs; a.south5 = gs + nx; a.south6 = gs + 2 * nx;
    a.north4 = gn; a.north7 = gn + nx; a.north8 = gn + 2 * nx;
    if (p2p) {
      if ((rc = p2p_push(c, s, nullptr, seq))) return rc;
      launch_sweep(c, a, s.sc);
      HIPC(hipGetLastError());
      if ((rc = p2p_push(c, s, a.dst, seq))) return rc;   // the new edge rows
    } else {
      a.send_south = s.send_s[q] + h3; a.send_north = s.send_n[q] + h3;
      // boundary rows first: they feed the exchange
      a.y_count = s.nyl >= 2 ? 2 : 1; a.y_stride = s.nyl >= 2 ? s.nyl - 1 : 1;
      // edge stream: after the halos of the previous launch arrived and its interior finished
      hipStream_t es = edge_stream(c, s);
      HIPC(hipStreamWaitEvent(es, s.ev_recv[qp], 0));
      if (es != s.sc) HIPC(hipStreamWaitEvent(es, s.ev_int[qp], 0));
      launch_sweep(c, a, es);
      HIPC(hipGetLastError());
      HIPC(hipEventRecord(s.ev_bnd[q], es));
    }
  }
  if (ex) {
    if ((rc = exchange_halos(c, q, 3, 3))) return rc;
    for (auto& s : c->slabs) {
      HIPC(hipSetDevice(s.dev));
      // interior stream: after the previous launch's edge rows are in place (ev_bnd of launch li-1)
      const bool split = split_edge_stream(c, s);
      if (split) HIPC(hipStreamWaitEvent(s.sc, s.ev_bnd[qp], 0));
      if (s.nyl <= 2) { if (split) HIPC(hipEventRecord(s.ev_int[q], s.sc)); continue; }
      lbm::SweepArgs a = sweep_args(c, s, q, tt, last, false, a1, a2);   // (interior rows never touch halos)
      a.y_begin = 1; a.y_count = s.nyl - 2; a.y_stride = 1;
      a.partials += sweep_blocks(c, 2);
      launch_sweep(c, a, s.sc);
      HIPC(hipGetLastError());
      if (split) HIPC(hipEventRecord(s.ev_int[q], s.sc));
    }
  }
  c->cur ^= 1;
  return LBM_OK;
}

// One two-step launch group (all local slabs) for steps tt, tt+1, launch index li.  Peer-to-peer: ONE launch per slab, whose
// edge tiles go first and carry the hand-off themselves (lbm::kSweep2P2P).
int launch_pair(lbm_ctx* c, int li, int tt, bool accel_out, bool fold_prev, float a1, float a2) {
  const int q = li & 1, qp = q ^ 1;
  const bool p2p = c->exchange == LBM_EXCHANGE_P2P, ex = c->exchange != 0 && !p2p;
  const uint32_t seq = p2p ? ++c->seq : 0;
  const int ntx = cdiv(c->p.nx, kT2X);   // (partial tiles only when the slab is alone)
  int rc;
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    lbm::Sweep2Args a = sweep2_args(c, s, q, tt, accel_out, fold_prev, a1, a2);
    const int nty = cdiv(s.nyl, kT2Y);
    a.by_begin = 0; a.by_count = nty; a.by_stride = 1;
    if (c->exchange == 0) {
      launch_sweep2(c, a, ntx * nty, s.sc, false);
      HIPC(hipGetLastError());
      continue;
    }
    const int qg = p2p ? (seq - 1) & 1 : qp;
    a.ghost_s = s.ghost_s[qg]; a.ghost_n = s.ghost_n[qg];
    a.blocked_gs = s.blocked_gs; a.blocked_gn = s.blocked_gn;
    if (p2p) {
      a.send_s = p2p_remote_s(s, seq); a.send_n = p2p_remote_n(s, seq);
      a.sync = p2p_sync(s, seq, ntx, ntx);
      launch_sweep2_p2p(c, a, ntx * nty, s.sc);
      HIPC(hipGetLastError());
    } else {
      // edge tile rows first: they consume the halos of the previous pair and pack the next ones
      a.by_count = nty >= 2 ? 2 : 1; a.by_stride = nty >= 2 ? nty - 1 : 1;
      a.send_s = s.send_s[q]; a.send_n = s.send_n[q];
      hipStream_t es = edge_stream(c, s);
      HIPC(hipStreamWaitEvent(es, s.ev_recv[qp], 0));
      if (es != s.sc) HIPC(hipStreamWaitEvent(es, s.ev_int[qp], 0));
      launch_sweep2(c, a, ntx * a.by_count, es, true);
      HIPC(hipGetLastError());
      HIPC(hipEventRecord(s.ev_bnd[q], es));
    }
  }
  if (ex) {
    if ((rc = exchange_halos(c, q, 0, lbm::kHaloSlots))) return rc;
    for (auto& s : c->slabs) {
      const int nty = cdiv(s.nyl, kT2Y);
      HIPC(hipSetDevice(s.dev));
      const bool split = split_edge_stream(c, s);
      if (split) HIPC(hipStreamWaitEvent(s.sc, s.ev_bnd[qp], 0));
      if (nty <= 2) { if (split) HIPC(hipEventRecord(s.ev_int[q], s.sc)); continue; }
      lbm::Sweep2Args a = sweep2_args(c, s, q, tt, accel_out, false, a1, a2);
      a.by_begin = 1; a.by_count = nty - 2; a.by_stride = 1;
      a.partials1 += 2 * ntx; a.partials2 += 2 * ntx;   // after the two edge tile rows
      launch_sweep2(c, a, ntx * (nty - 2), s.sc, false);
      HIPC(hipGetLastError());
      if (split) HIPC(hipEventRecord(s.ev_int[q], s.sc));
    }
  }
  c->cur ^= 1;
  return LBM_OK;
}

// One marching launch: steps tt .. tt+K-1 of the lone slab, launch index li.
int launch_march(lbm_ctx* c, int li, int tt, bool accel_out, bool fold_prev) {
  using Cfg = lbm::MarchCfg<kMarchK>;
  Slab& s = c->slabs[0];
  HIPC(hipSetDevice(s.dev));
  if (c->march_rows <= 0) c->march_rows = march_pick_rows(c);
  const int q = li & 1, qp = q ^ 1;
  lbm::MarchArgs a;
  a.src = s.lat[c->cur]; a.dst = s.lat[c->cur ^ 1];
  a.plane = s.plane; a.pitch = s.pitch; a.nx = c->p.nx; a.ny = c->p.ny;
  a.blocked = s.blocked; a.omega = c->p.omega;
  a.accel_row = c->p.ny - 2; a.accel_out = accel_out ? 1 : 0;
  a.a1 = accel_pair(c).a1; a.a2 = accel_pair(c).a2;
  a.H = c->march_rows;
  a.nstrips = cdiv(c->p.nx, Cfg::WOUT); a.nchunks = cdiv(c->p.ny, a.H);
  const int nb = a.nstrips * a.nchunks;
  if ((long)kMarchK * nb > s.partial_cap) return fail(LBM_EINVAL, "marching kernel: %d blocks exceed the partial-sum buffer", nb);
  a.partials = s.partials[q];
  a.prev = nullptr; a.prev_count = 0; a.prev_sum = nullptr;
  if (fold_prev) { a.prev = s.partials[qp]; a.prev_count = nb; a.prev_sum = s.sums + (tt - kMarchK); }
  switch ((int)(c->variant & (lbm::kFastMath | lbm::kNtStore))) {
    case 0: hipLaunchKernelGGL((lbm::lbm_march<kMarchK, 0>), dim3(nb), dim3(kMarchK * 256), 0, s.sc, a); break;
    case 1: hipLaunchKernelGGL((lbm::lbm_march<kMarchK, 1>), dim3(nb), dim3(kMarchK * 256), 0, s.sc, a); break;
    case 2: hipLaunchKernelGGL((lbm::lbm_march<kMarchK, 2>), dim3(nb), dim3(kMarchK * 256), 0, s.sc, a); break;
    default: hipLaunchKernelGGL((lbm::lbm_march<kMarchK, 3>), dim3(nb), dim3(kMarchK * 256), 0, s.sc, a); break;
  }
  HIPC(hipGetLastError());
  c->cur ^= 1;
  return LBM_OK;
}

// ---- lbm_march across the slabs of ONE process.  A slab's K ghost rows on either side are not copied anywhere: the
// kernel reads them out of the neighbouring slab's lattice (same device, or a peer device over xGMI once peer
// access is on).  Launch n+1 of a slab waits for launch n of both neighbours: that orders the rows it reads and
// the rows of its own source lattice (next launch's destination) the neighbours were reading.
bool march_slabs_setup(lbm_ctx* c) {
  if (c->march_slabs >= 0) return c->march_slabs == 1;
  c->march_slabs = 0;
  if (c->rank_mode || c->exchange != LBM_EXCHANGE_COPY) return false;   // (peer-to-peer contexts march by p2p_march_on's rule)
  const int K = (c->time_block == 8) ? 8 : kMarchK;
  if (K != kMarchK ? c->p.nx < 64 : (c->p.nx % 4 != 0 || c->p.nx < lbm::MarchCfg<kMarchK>::W)) return false;
  const int ns = (int)c->slabs.size();
  for (auto& s : c->slabs)
    if (s.nyl < 4 * K || (double)s.nyl * s.pitch * 4.0 >= 4.0e9) return false;
  for (int i = 0; i < ns; ++i)
    for (int d : {(i + ns - 1) % ns, (i + 1) % ns}) {
      const int a = c->slabs[i].dev, b = c->slabs[d].dev;
      if (a == b) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) { (void)hipGetLastError(); return false; }
      if (hipSetDevice(a) != hipSuccess) return false;
      const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
      (void)hipGetLastError();
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return false;
    }
  c->march_slabs = 1;
  return true;
}
// Steps per marching pass of a context whose slabs trade rows: 8 = lbm_wave<8>, 4 = lbm_march, 0 = no marching.
inline int slab_K(const lbm_ctx* c) {
  if (c->exchange == 0 || (c->variant & 8)) return 0;
  if (c->time_block == 8) return (c->p.nx >= 64) ? 8 : 0;
  if (c->time_block == kMarchK) return (c->p.nx % 4 == 0 && c->p.nx >= lbm::MarchCfg<kMarchK>::W) ? kMarchK : 0;
  return 0;
}
inline bool march_slabs_on(lbm_ctx* c) { return slab_K(c) != 0 && march_slabs_setup(c); }

int march_rows_for(const lbm_ctx* c, int ny_rows) {
  const int ns = cdiv(c->p.nx, lbm::MarchCfg<kMarchK>::WOUT), ncu = std::max(c->ncu, 1);
  int best_h = std::min(ny_rows, 256);
  double best = -1.0;
  for (int h = std::min(ny_rows, 32); h <= std::min(ny_rows, 1024); ++h) {
    const long blocks = (long)ns * cdiv(ny_rows, h);
    const long rounds = (blocks + ncu - 1) / ncu;
    const double eff = (double)ny_rows * ns / ((double)rounds * ncu * (h + 3 * (kMarchK - 1)));
    if (eff > best + 1e-9) { best = eff; best_h = h; }
  }
  return best_h;
}
// Rows per chunk of lbm_wave<8> on a slab of ny_rows rows, and the share of the chip's wave-slot time that is useful
// work with it: a chunk costs 2K fill iterations, and waves that do not fill the last round leave slots idle.
inline bool slab_is_wave(int K) { return K == 8; }
// wave slots of the chip for lbm_wave<K> with the context's columns per lane
int wave_slots(const lbm_ctx* c, int K) { return std::max(c->ncu, 1) * std::max(wave_blocks_per_cu(K, wave_C(c, K)), 1) * (lbm::kWaveBlock / 64); }
// The share of the chip's wave-slot time that is useful work with chunks of h rows: a chunk costs its 2K fill
// iterations on top of its h, and the waves come in rounds of `slots`: up to three rounds a partial round costs a whole
// one (4096^2: 118-row chunks = 0.98 rounds 285 GLUPS, 114-row chunks = 1.008 rounds 231; 5120^2: 91 rows = 1.99 rounds
// 310, 87 rows = 2.06 rounds 282), beyond that the rounds blur into each other.  A single round, in which every wave
// fills at the same time, runs ~0.87 of what this predicts, several rounds ~0.94 (371 GLUPS x this figure against the
// measured rates of 2048^2 ... 8192^2 and of the 8192-wide slabs).
double slab_wave_efficiency(const lbm_ctx* c, int ny_rows, int h, int K, int extra_waves) {
  const int nwc = cdiv(c->p.nx, wave_out_cols(c, K));
  const long waves = (long)nwc * cdiv(ny_rows, h) + extra_waves, slots = wave_slots(c, K);
  const double r = (double)waves / slots;
  const double rounds = r <= 3.0 ? std::ceil(r) : r;
  // (two columns per lane: 0.91 - 0.96 measured for one round and for two alike)
  const double shape = wave_C(c, K) == 2 ? 0.93 : rounds <= 1.0 ? 0.87 : 0.94;
  // (a level's fill rows are half empty on average: K of the 2K fill iterations' worth of work)
  return shape * (double)nwc * ny_rows / (rounds * slots * (h + 2.0 * K));
}
int slab_wave_rows(const lbm_ctx* c, int ny_rows, int K, int extra_waves) {
  if (c->wave_rows > 0) return std::min(c->wave_rows, ny_rows);
  const int hmax = wave_C(c, K) == 2 ? 320 : 128;
  int best_h = std::min(ny_rows, 128);
  double best = -1.0;
  for (int h = std::min(ny_rows, 32); h <= std::min(ny_rows, hmax); ++h) {        // (beyond 128 rows the one-column chunks get slower: measured)
    const double e = slab_wave_efficiency(c, ny_rows, h, K, extra_waves);
    if (e > best + 1e-9) { best = e; best_h = h; }
  }
  return best_h;
}
// partial-sum slots (blocks) of one marching launch on a slab
inline int march_slab_blocks(const lbm_ctx* c, const Slab& s) {
  const int K = slab_K(c);
  if (slab_is_wave(K)) return cdiv((long)cdiv(c->p.nx, wave_out_cols(c, K)) * cdiv(s.nyl, slab_wave_rows(c, s.nyl, K)), lbm::kWaveBlock / 64);
  return cdiv(c->p.nx, lbm::MarchCfg<kMarchK>::WOUT) * cdiv(s.nyl, march_rows_for(c, s.nyl));
}

// The neighbours of a slab as a marching launch sees them.
struct SlabNb { const float* src_s; const float* src_n; long plane_s, plane_n; int ny_s, ny_n; const uint8_t* blk_s; const uint8_t* blk_n; };

// One marching launch on one slab: steps tt .. tt+K-1, partial sums into buffer q (folding the previous launch's).
int launch_slab_pass(lbm_ctx* c, Slab& s, const SlabNb& nbr, int K, int q, int tt, bool accel_out, bool fold_prev) {
  const auto [a1, a2] = accel_pair(c);
  const int nb = march_slab_blocks(c, s), qp = q ^ 1;
  if ((long)K * nb > s.partial_cap) return fail(LBM_EINVAL, "marching kernel: %d blocks exceed the partial-sum buffer", nb);
  // the lattice's accelerate row (ny-2) in this slab's row numbers, and its periodic images: one of them may fall
  // into the K rows this slab recomputes on a neighbour's behalf
  const int ar = (c->p.ny - 2) - s.row0;
  const int flavour = (int)(c->variant & (lbm::kFastMath | lbm::kNtStore));
  if (slab_is_wave(K)) {
    lbm::WaveArgs a;
    a.src = s.lat[c->cur]; a.dst = s.lat[c->cur ^ 1];
    a.plane = s.plane; a.pitch = s.pitch; a.nx = c->p.nx; a.ny = s.nyl;
    a.blocked = s.blocked; a.omega = c->p.omega;
    a.accel_row = lbm::kNoRow; a.accel_out = accel_out ? 1 : 0; a.a1 = a1; a.a2 = a2;
    a.H = slab_wave_rows(c, s.nyl, K);
    a.y_begin = 0; a.y_end = s.nyl;
    a.nwc = cdiv(c->p.nx, wave_out_cols(c, K)); a.nchunks = cdiv(s.nyl, a.H);
    a.nchunks_a = a.nchunks; a.yb_begin = a.yb_end = 0;
    a.partials = s.partials[q]; a.pstride = nb; a.pbase = 0;
    a.prev = nullptr; a.prev_count = 0; a.prev_sum = nullptr;
    if (fold_prev) { a.prev = s.partials[qp]; a.prev_count = nb; a.prev_sum = s.sums + (tt - K); }
    a.src_s = nbr.src_s; a.src_n = nbr.src_n; a.plane_s = nbr.plane_s; a.plane_n = nbr.plane_n;
    a.ny_s = nbr.ny_s; a.ny_n = nbr.ny_n; a.blocked_s = nbr.blk_s; a.blocked_n = nbr.blk_n;
    a.acc_rows[0] = ar; a.acc_rows[1] = ar - c->p.ny; a.acc_rows[2] = ar + c->p.ny;
    hipLaunchKernelGGL(wave_kernel(K, true, wave_C(c, K), flavour, WaveFlavour::plain), dim3(nb), dim3(lbm::kWaveBlock), 0, s.sc, a);
  } else {
    using Cfg = lbm::MarchCfg<kMarchK>;
    lbm::MarchArgs a;
    a.src = s.lat[c->cur]; a.dst = s.lat[c->cur ^ 1];
    a.plane = s.plane; a.pitch = s.pitch; a.nx = c->p.nx; a.ny = s.nyl;
    a.blocked = s.blocked; a.omega = c->p.omega;
    a.accel_row = lbm::kNoRow; a.accel_out = accel_out ? 1 : 0; a.a1 = a1; a.a2 = a2;
    a.H = march_rows_for(c, s.nyl);
    a.nstrips = cdiv(c->p.nx, Cfg::WOUT); a.nchunks = cdiv(s.nyl, a.H);
    a.partials = s.partials[q];
    a.prev = nullptr; a.prev_count = 0; a.prev_sum = nullptr;
    if (fold_prev) { a.prev = s.partials[qp]; a.prev_count = nb; a.prev_sum = s.sums + (tt - K); }
    a.src_s = nbr.src_s; a.src_n = nbr.src_n; a.plane_s = nbr.plane_s; a.plane_n = nbr.plane_n;
    a.ny_s = nbr.ny_s; a.ny_n = nbr.ny_n; a.blocked_s = nbr.blk_s; a.blocked_n = nbr.blk_n;
    a.acc_rows[0] = ar; a.acc_rows[1] = ar - c->p.ny; a.acc_rows[2] = ar + c->p.ny;
    switch (flavour) {
      case 0: hipLaunchKernelGGL((lbm::lbm_march<kMarchK, 0, true>), dim3(nb), dim3(kMarchK * 256), 0, s.sc, a); break;
      case 1: hipLaunchKernelGGL((lbm::lbm_march<kMarchK, 1, true>), dim3(nb), dim3(kMarchK * 256), 0, s.sc, a); break;
      case 2: hipLaunchKernelGGL((lbm::lbm_march<kMarchK, 2, true>), dim3(nb), dim3(kMarchK * 256), 0, s.sc, a); break;
      default: hipLaunchKernelGGL((lbm::lbm_march<kMarchK, 3, true>), dim3(nb), dim3(kMarchK * 256), 0, s.sc, a); break;
    }
  }
  HIPC(hipGetLastError());
  return LBM_OK;
}

// One marching launch group over all slabs: steps tt .. tt+K-1, launch index li.
int launch_march_slabs(lbm_ctx* c, int li, int tt, bool accel_out, bool fold_prev) {
  const int ns = (int)c->slabs.size(), q = li & 1, qp = q ^ 1, K = slab_K(c);
  for (int i = 0; i < ns; ++i) {
    Slab& s = c->slabs[i];
    Slab& so = c->slabs[(i + ns - 1) % ns];
    Slab& no = c->slabs[(i + 1) % ns];
    HIPC(hipSetDevice(s.dev));
    HIPC(hipStreamWaitEvent(s.sc, so.ev_march[qp], 0));
    HIPC(hipStreamWaitEvent(s.sc, no.ev_march[qp], 0));
    const SlabNb nbr{so.lat[c->cur], no.lat[c->cur], so.plane, no.plane, so.nyl, no.nyl, so.blocked, no.blocked};
    const int rc = launch_slab_pass(c, s, nbr, K, q, tt, accel_out, fold_prev);
    if (rc) return rc;
    HIPC(hipEventRecord(s.ev_march[q], s.sc));
  }
  c->cur ^= 1;
  return LBM_OK;
}

// ---- ... and across slabs with peer-to-peer halos, one process or one per GPU: the K ghost rows either side are read
// straight out of the neighbours' lattices (Slab::nb_lat, over xGMI), where every slab fills the chip.  The decision uses
// the lattice, the number of slabs and the options only -- every rank must come to the same answer, the two protocols
// do not mix.
bool p2p_march_on(const lbm_ctx* c) {
  const int K = slab_K(c);
  if (K == 0 || c->exchange != LBM_EXCHANGE_P2P) return false;
  const int rows = c->p.ny / c->nranks;                     // the smallest slab
  if (rows < 4 * K || (double)(rows + 1) * c->slabs[0].pitch * 4.0 >= 4.0e9) return false;
  for (auto& s : c->slabs) if (!s.nb_lat[0][0] || !s.nb_lat[1][0]) return false;   // (connect failed: an error everywhere)
  return true;
}
bool p2p_march_pays(const lbm_ctx* c) {                      // same estimate as for a lone lattice, on the smallest slab
  const int rows = c->p.ny / c->nranks, h = march_rows_for(c, rows), ns = cdiv(c->p.nx, lbm::MarchCfg<kMarchK>::WOUT), ncu = std::max(c->ncu, 1);
  const long blocks = (long)ns * cdiv(rows, h), rounds = (blocks + ncu - 1) / ncu;
  return (double)rows * ns / ((double)rounds * ncu * (h + 3 * (kMarchK - 1))) >= 0.65;
}
// lbm_wave<8> instead of lbm_march on slabs of `rows` rows?  When its waves fill at least most of one round of the
// chip's wave slots.  Measured on one GPU (tools/strong_scaling_proxy.py, us per step, lbm_wave<8> against lbm_march):
// 8192 x 4096 126 / 135, 8192 x 2048 69.3 / 70.3, 8192 x 1024 38.7 / 39.4 -- a little ahead everywhere, with half as
// many launches (and flag hand-offs over xGMI) per step; 1024-wide slabs (22 wave columns) are far too narrow: 12.4 / 5.4.
bool slab_wave_pays(const lbm_ctx* c, int rows, int K) {
  if (c->p.nx < 64 || rows < 32 || c->march_kernel == 0) return false;
  const int h = slab_wave_rows(c, rows, K);
  return (double)cdiv(c->p.nx, wave_out_cols(c, K)) * cdiv(rows, h) >= 0.85 * wave_slots(c, K);
}
// Launch group seq of a slab starts once both neighbours have raised seq - 1 ("my group seq - 1 is over": their rows are
// final, and they no longer read the lattice this launch overwrites) and raises seq when it is over.  In front of a run's
// first group, "the starting lattice is in place": a group of its own that launches nothing.
int p2p_march_open(lbm_ctx* c) {
  const uint32_t seq = ++c->seq;
  int rc;
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    if ((rc = p2p_push(c, s, nullptr, seq))) return rc;   // (the neighbours are through with the previous run)
    if ((rc = p2p_raise(s, seq))) return rc;
  }
  return LBM_OK;
}
// One marching launch group over all local slabs: steps tt .. tt+K-1, launch index li.
int launch_march_p2p(lbm_ctx* c, int li, int tt, bool accel_out, bool fold_prev) {
  const uint32_t seq = ++c->seq;
  int rc;
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    if ((rc = p2p_push(c, s, nullptr, seq))) return rc;   // wait for both neighbours' seq-1
    const SlabNb nbr{s.nb_lat[0][c->cur], s.nb_lat[1][c->cur], s.nb_plane[0], s.nb_plane[1], s.nb_nyl[0], s.nb_nyl[1],
                     s.nb_blocked[0], s.nb_blocked[1]};
    if ((rc = launch_slab_pass(c, s, nbr, slab_K(c), li & 1, tt, accel_out, fold_prev))) return rc;
    if ((rc = p2p_raise(s, seq))) return rc;
  }
  c->cur ^= 1;
  return LBM_OK;
}

// ---- lbm_wave across slabs under the RCCL transport (LBM_EXCHANGE_RCCL, one process per GPU or one process with one
// slab per GPU): GHOST BANDS.  The K rows below and above a slab are kept as the neighbours hold them in two bands per
// lattice ([9 planes][K rows][pitch], contiguous) and travel once per K steps: after the slab's two EDGE launches (a
// short chunk of rows at the bottom and one at the top, which produce the K rows each neighbour needs) the rows are
// packed and sent with ncclSend / ncclRecv on the exchange stream, overlapped with the INTERIOR launch, which touches
// no ghost row (reference rows: d2q9-bgk.c:971-998 names the planes that cross a row boundary; K steps need all nine
// planes of K rows).  The kernel is the SLAB flavour that also reads neighbours' rows in place: a band looks to it
// like a neighbour's lattice of K rows.  Message protocol: tests/test_slab_gloo.py::test_k_row_ghost_zone_of_the_marching_kernels.
struct BandPlan { int K, he, H, nwc, nb_e, nb_i; };   // edge chunk rows, interior chunk rows, blocks of the edge launch (both edge chunks) and of the interior launch

bool march_bands_on(const lbm_ctx* c) {
  const int K = slab_K(c);
  if (c->exchange != LBM_EXCHANGE_RCCL || !slab_is_wave(K)) return false;
  const int rows = c->p.ny / c->nranks;                     // the smallest slab: every rank decides alike
  if (rows < 4 * K || (double)(rows + 1) * c->slabs[0].pitch * 4.0 >= 4.0e9) return false;
  for (auto& s : c->slabs) if (!s.band_blk_s) return false;
  return true;
}

// Edge chunks about half the height of the interior's, so that an edge launch plus the exchange it feeds is over before
// the interior launch is; interior chunks such that all three launches fit the chip's wave slots in whole rounds.
BandPlan band_plan(const lbm_ctx* c, const Slab& s) {
  BandPlan b;
  b.K = slab_K(c);
  b.nwc = cdiv(c->p.nx, wave_out_cols(c, b.K));
  // (an edge chunk is one wave per strip marching alone on its SIMD: ~2.2 us per row at K = 8, against ~3.7 for the rows of the
  // interior launch's three waves per SIMD; LBM_BAND_EDGE_ROWS overrides)
  static const int edge_rows_env = getenv("LBM_BAND_EDGE_ROWS") ? atoi(getenv("LBM_BAND_EDGE_ROWS")) : 0;
  const int hu = slab_wave_rows(c, s.nyl, b.K);
  b.he = std::max(b.K, std::min(edge_rows_env > 0 ? edge_rows_env : hu / 3, s.nyl / 4));
  b.H = slab_wave_rows(c, s.nyl - 2 * b.he, b.K, 2 * b.nwc);
  const int per = lbm::kWaveBlock / 64;
  b.nb_e = cdiv(2 * b.nwc, per);
  b.nb_i = cdiv((long)b.nwc * cdiv(s.nyl - 2 * b.he, b.H), per);
  return b;
}

int bands_setup(lbm_ctx* c, int K) {
  for (auto& s : c->slabs) {
    if (s.band_K == K) continue;
    HIPC(hipSetDevice(s.dev));
    const size_t bytes = sizeof(float) * 9 * (size_t)K * s.pitch;
    for (int i = 0; i < 2; ++i) {
      if (s.band_s[i]) HIPC(hipFree(s.band_s[i]));
      if (s.band_n[i]) HIPC(hipFree(s.band_n[i]));
      s.band_s[i] = s.band_n[i] = nullptr;
      HIPC(hipMalloc((void**)&s.band_s[i], bytes));
      HIPC(hipMalloc((void**)&s.band_n[i], bytes));
    }
    if (s.band_send_s) HIPC(hipFree(s.band_send_s));
    if (s.band_send_n) HIPC(hipFree(s.band_send_n));
    s.band_send_s = s.band_send_n = nullptr;
    HIPC(hipMalloc((void**)&s.band_send_s, bytes));
    HIPC(hipMalloc((void**)&s.band_send_n, bytes));
    s.band_K = K;
  }
  return LBM_OK;
}

// The K edge rows of lattice `par` of every local slab to the neighbours' bands of the same parity: on the exchange
// streams, behind event ev_bnd[q] ("the launches that wrote those rows are over"); ev_recv[q] says the bands have arrived.
int exchange_bands(lbm_ctx* c, int q, int par, int K) {
  const int ns = (int)c->slabs.size();
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    HIPC(hipStreamWaitEvent(s.sx, s.ev_bnd[q], 0));
    hipLaunchKernelGGL(lbm::lbm_pack_band_rows, dim3(cdiv((long)K * s.pitch, 256)), dim3(256), 0, s.sx,
                       s.lat[par], s.plane, s.pitch, s.nyl, K, s.band_send_s, s.band_send_n);
    HIPC(hipGetLastError());
  }
  NCCLC(rccl::GroupStart());
  for (int i = 0; i < ns; ++i) {
    Slab& s = c->slabs[i];
    const size_t n = 9 * (size_t)K * s.pitch;
    const int me = c->rank_mode ? c->rank : i;
    const int south = (me + c->nranks - 1) % c->nranks, north = (me + 1) % c->nranks;
    // order matters when south == north (1 or 2 ranks): sends S then N, receives N then S
    NCCLC(rccl::Send(s.band_send_s, n, rccl::kFloat32, south, s.comm, s.sx));
    NCCLC(rccl::Send(s.band_send_n, n, rccl::kFloat32, north, s.comm, s.sx));
    NCCLC(rccl::Recv(s.band_n[par], n, rccl::kFloat32, north, s.comm, s.sx));
    NCCLC(rccl::Recv(s.band_s[par], n, rccl::kFloat32, south, s.comm, s.sx));
  }
  NCCLC(rccl::GroupEnd());
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    HIPC(hipEventRecord(s.ev_recv[q], s.sx));
  }
  return LBM_OK;
}

// One launch of lbm_wave<K, ., SLAB> on a slab whose ghost rows live in bands: the interior rows [he, nyl - he) in chunks of
// H, or (edge) the two edge chunks [0, he) and [nyl - he, nyl) together.
int launch_band_rows(lbm_ctx* c, Slab& s, const BandPlan& b, bool edge, int q, int tt, bool accel_out, bool fold_prev, hipStream_t st) {
  const int K = b.K, qp = q ^ 1, ntot = b.nb_e + b.nb_i;
  const int nblocks = edge ? b.nb_e : b.nb_i, pbase = edge ? 0 : b.nb_e;
  lbm::WaveArgs a;
  a.src = s.lat[c->cur]; a.dst = s.lat[c->cur ^ 1];
  a.plane = s.plane; a.pitch = s.pitch; a.nx = c->p.nx; a.ny = s.nyl;
  a.blocked = s.blocked; a.omega = c->p.omega;
  a.accel_row = lbm::kNoRow; a.accel_out = accel_out ? 1 : 0;
  a.a1 = accel_pair(c).a1; a.a2 = accel_pair(c).a2;
  if (edge) {
    a.H = b.he; a.y_begin = 0; a.y_end = b.he; a.nchunks_a = 1; a.yb_begin = s.nyl - b.he; a.yb_end = s.nyl; a.nchunks = 2;
  } else {
    a.H = b.H; a.y_begin = b.he; a.y_end = s.nyl - b.he; a.nchunks = cdiv(a.y_end - a.y_begin, b.H); a.nchunks_a = a.nchunks;
    a.yb_begin = a.yb_end = 0;
  }
  a.nwc = b.nwc;
  a.partials = s.partials[q]; a.pstride = ntot; a.pbase = pbase;
  a.prev = nullptr; a.prev_count = 0; a.prev_sum = nullptr;
  if (fold_prev) { a.prev = s.partials[qp]; a.prev_count = ntot; a.prev_sum = s.sums + (tt - K); }
  const long bplane = (long)K * s.pitch;
  a.src_s = s.band_s[c->cur]; a.src_n = s.band_n[c->cur]; a.plane_s = bplane; a.plane_n = bplane;
  a.ny_s = K; a.ny_n = K;
  a.blocked_s = s.band_blk_s + (size_t)(kBandRows - K) * s.pitch; a.blocked_n = s.band_blk_n;
  const int ar = (c->p.ny - 2) - s.row0;
  a.acc_rows[0] = ar; a.acc_rows[1] = ar - c->p.ny; a.acc_rows[2] = ar + c->p.ny;
  hipLaunchKernelGGL(wave_kernel(K, true, wave_C(c, K), (int)(c->variant & (lbm::kFastMath | lbm::kNtStore)), WaveFlavour::plain),
                     dim3(nblocks), dim3(lbm::kWaveBlock), 0, st, a);
  HIPC(hipGetLastError());
  return LBM_OK;
}

// One marching group (K steps) of every local slab: edge launches, exchange of the new edge rows, interior launch.
int launch_band_group(lbm_ctx* c, int li, int tt, bool accel_out, bool fold_prev) {
  const int q = li & 1, qp = q ^ 1, K = slab_K(c);
  int rc;
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    const BandPlan b = band_plan(c, s);
    hipStream_t es = edge_stream(c, s);
    HIPC(hipStreamWaitEvent(es, s.ev_recv[qp], 0));                       // the bands of the source lattice have arrived
    if (es != s.sc) HIPC(hipStreamWaitEvent(es, s.ev_int[qp], 0));        // the previous interior launch is over
    if ((rc = launch_band_rows(c, s, b, true, q, tt, accel_out, fold_prev, es))) return rc;
    HIPC(hipEventRecord(s.ev_bnd[q], es));
  }
  if ((rc = exchange_bands(c, q, c->cur ^ 1, K))) return rc;
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    const BandPlan b = band_plan(c, s);
    const bool split = split_edge_stream(c, s);
    if (split) HIPC(hipStreamWaitEvent(s.sc, s.ev_bnd[qp], 0));           // the previous edge launches are over
    if ((rc = launch_band_rows(c, s, b, false, q, tt, accel_out, false, s.sc))) return rc;
    if (split) HIPC(hipEventRecord(s.ev_int[q], s.sc));
  }
  c->cur ^= 1;
  return LBM_OK;
}

// ---- lbm_wave: K steps per pass, one wave per strip of 64 (or 128) columns
// The instantiations: a lattice alone (K = 4, 6, 8 with one column per lane, K = 8 with two) in every flavour, and a slab with
// neighbours (K = 8, one or two columns) in the plain one; math = IEEE or fast rcp / sqrt (bit 0) x nontemporal stores (bit 1).
// What a flavour (lbm_wave_pick.h) switches on in the kernel, by lbm_wave's template parameters:
struct WaveTraits { bool FORCE, PROBE, FIELD, WINDOW, DRIVEN, STATS; };
constexpr WaveTraits kWaveTraits[10] = {
    /* plain           */ {false, false, false, false, false, false},
    /* force           */ {true, false, false, false, false, false},    // lbm_run_forces
    /* probe           */ {false, true, false, false, false, false},    // lbm_run_probes
    /* force_probe     */ {true, true, false, false, false, false},     // lbm_run_observed's forces and probes
    /* field           */ {false, false, true, false, false, false},    // lbm_run_sampled, lbm_run_mean
    /* window          */ {false, false, false, true, false, false},    // lbm_run_window
    /* driven          */ {false, false, false, false, true, false},    // lbm_run_driven
    /* driven_observed */ {true, true, false, false, true, false},      // lbm_run_driven_observed
    /* stats           */ {false, false, false, false, false, true},    // lbm_run_stats
    /* window_stats    */ {false, false, false, true, false, true},     // lbm_run_window_stats
};
template <int K, bool SLAB, int C, WaveFlavour F>
wave_fn wave_kernel_m(int math) {
  constexpr WaveTraits t = kWaveTraits[(int)F];
  switch (math & 3) {
    case 0: return lbm::lbm_wave<K, 0, SLAB, C, t.FORCE, t.PROBE, t.FIELD, t.WINDOW, t.DRIVEN, t.STATS>;
    case 1: return lbm::lbm_wave<K, 1, SLAB, C, t.FORCE, t.PROBE, t.FIELD, t.WINDOW, t.DRIVEN, t.STATS>;
    case 2: return lbm::lbm_wave<K, 2, SLAB, C, t.FORCE, t.PROBE, t.FIELD, t.WINDOW, t.DRIVEN, t.STATS>;
    default: return lbm::lbm_wave<K, 3, SLAB, C, t.FORCE, t.PROBE, t.FIELD, t.WINDOW, t.DRIVEN, t.STATS>;
  }
}
template <WaveFlavour F>
wave_fn wave_kernel_kc(int K, bool slab, int C, int math) {
  if constexpr (F == WaveFlavour::plain)
    if (slab) return C == 2 ? wave_kernel_m<8, true, 2, F>(math) : wave_kernel_m<8, true, 1, F>(math);     // (K = 8 only)
  if (K == 8) return C == 2 ? wave_kernel_m<8, false, 2, F>(math) : wave_kernel_m<8, false, 1, F>(math);
  if (K == 6) return wave_kernel_m<6, false, 1, F>(math);
  return wave_kernel_m<4, false, 1, F>(math);
}
// (the cases in the order in which the flavours came to the code object: it keeps its kernels in that order)
wave_fn wave_kernel(int K, bool slab, int C, int math, WaveFlavour f) {
  switch (f) {
    case WaveFlavour::plain: return wave_kernel_kc<WaveFlavour::plain>(K, slab, C, math);
    case WaveFlavour::force: return wave_kernel_kc<WaveFlavour::force>(K, slab, C, math);
    case WaveFlavour::field: return wave_kernel_kc<WaveFlavour::field>(K, slab, C, math);
    case WaveFlavour::driven: return wave_kernel_kc<WaveFlavour::driven>(K, slab, C, math);
    case WaveFlavour::driven_observed: return wave_kernel_kc<WaveFlavour::driven_observed>(K, slab, C, math);
    case WaveFlavour::window: return wave_kernel_kc<WaveFlavour::window>(K, slab, C, math);
    case WaveFlavour::force_probe: return wave_kernel_kc<WaveFlavour::force_probe>(K, slab, C, math);
    case WaveFlavour::probe: return wave_kernel_kc<WaveFlavour::probe>(K, slab, C, math);
    case WaveFlavour::stats: return wave_kernel_kc<WaveFlavour::stats>(K, slab, C, math);
    case WaveFlavour::window_stats: return wave_kernel_kc<WaveFlavour::window_stats>(K, slab, C, math);
  }
  return nullptr;
}

int wave_blocks_per_cu(int K, int C) {
  static int cache[16][3] = {};                 // (the answer does not change; lbm_set_option asks often)
  if (K < 16 && C < 3 && cache[K][C] > 0) return cache[K][C];
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(wave_kernel(K, false, C, 1, WaveFlavour::plain)), lbm::kWaveBlock, 0) != hipSuccess) { (void)hipGetLastError(); n = 0; }
  if (K < 16 && C < 3) cache[K][C] = n;
  return n;
}

// Waves the device holds at once (occupancy query), and the rows per chunk.  Short chunks win although each
// pays 2K fill iterations: many more waves than the device holds keep every SIMD's wave slots full from the
// first row to the last (measured at 8192^2, GLUPS for 24 / 32 / 48 / 64 / 96 rows: K = 4: 193 219 191 204 179;
// K = 6: 229 237 244 246 237; K = 8: 198 212 224 227 228; one resident round of 511-row chunks: 153 at K = 4).
void wave_plan(lbm_ctx* c) {
  const int K = c->time_block;
  int bpc = wave_blocks_per_cu(K, wave_C(c, K));
  if (bpc < 1) bpc = 4;
  c->wave_capacity = std::max(c->ncu, 1) * bpc * (lbm::kWaveBlock / 64);
  if (c->wave_rows > 0) return;
  c->wave_rows = (K == 8) ? slab_wave_rows(c, c->p.ny, 8) : std::min(c->p.ny, K >= 6 ? 64 : 32);   // (K = 8: whole rounds of the chip's wave slots)
}
// The blocks of one lbm_wave launch on the lone slab (the chunk heights chosen first, where they are not yet), and the bound
// admission, launch_wave and check_march_partials ask about: their partial sums, K floats per block, fit the slab's buffer.
inline int wave_blocks(lbm_ctx* c) {
  if (c->wave_rows <= 0 || c->wave_capacity <= 0) wave_plan(c);
  return cdiv((long)cdiv(c->p.nx, wave_out_cols(c, c->time_block)) * cdiv(c->p.ny, c->wave_rows), lbm::kWaveBlock / 64);
}
inline bool wave_partials_fit(lbm_ctx* c) { return (long)c->time_block * wave_blocks(c) <= c->slabs[0].partial_cap; }

// The force flavour's buffers of the lone slab: the force map and the index map (built at the first forces run that wants
// them, freed with fcells by lbm_set_bodies) and the contributions of one group of K steps (the stream orders the fold of
// group g before launch g + 1: one buffer).  false: no room -- the run takes the one-step path, nothing has been queued.
void wave_force_free(Slab& s) {
  if (s.fmap) (void)hipFree(s.fmap);
  if (s.fidx) (void)hipFree(s.fidx);
  grown_free(s.fcontrib);
  s.fmap = nullptr; s.fidx = nullptr;
}
bool wave_force_ready(lbm_ctx* c, int K) {
  Slab& s = c->slabs[0];
  const int n = s.fcells_n;
  if (n == 0) return true;                       // (no counted cell: the plain kernel, and the fold writes the zeros)
  if (hipSetDevice(s.dev) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (!s.fmap) {
    bool ok = hipMalloc((void**)&s.fmap, (size_t)s.plane) == hipSuccess &&
              hipMalloc((void**)&s.fidx, sizeof(int) * (size_t)s.nyl * s.pitch) == hipSuccess &&
              hipMemcpyAsync(s.fmap, s.blocked, (size_t)s.plane, hipMemcpyDeviceToDevice, s.sc) == hipSuccess;
    if (ok) {
      hipLaunchKernelGGL(lbm::lbm_mark_counted, dim3(cdiv(n, 256)), dim3(256), 0, s.sc, s.fcells, n, s.fmap, s.fidx);
      ok = hipGetLastError() == hipSuccess;
    }
    if (!ok) { (void)hipGetLastError(); (void)hipStreamSynchronize(s.sc); wave_force_free(s); return false; }
  }
  return grown_room(s, s.fcontrib, 2L * K * n, 1, false);
}

// The probe flavours' maps of the lone slab, built at the first probe run that wants them: the probe map and the index map
// (freed by lbm_set_probes), and -- with_forces, where a cell is counted -- the force-and-probe map from the force map
// (freed by lbm_set_probes and by lbm_set_bodies: it follows both sets).  false: no room, nothing has been queued.
void wave_probe_free(Slab& s, bool all) {
  if (s.fpmap) (void)hipFree(s.fpmap);
  s.fpmap = nullptr;
  if (!all) return;
  if (s.pmap) (void)hipFree(s.pmap);
  if (s.pidx) (void)hipFree(s.pidx);
  s.pmap = nullptr; s.pidx = nullptr;
}
bool wave_probe_ready(lbm_ctx* c, bool with_forces) {
  Slab& s = c->slabs[0];
  const int n = (int)s.pcells_host.size();
  if (n == 0 || !s.pcells) return false;
  if (hipSetDevice(s.dev) != hipSuccess) { (void)hipGetLastError(); return false; }
  auto build = [&](uint8_t*& map, const uint8_t* from) {
    bool ok = hipMalloc((void**)&map, (size_t)s.plane) == hipSuccess &&
              (s.pidx || hipMalloc((void**)&s.pidx, sizeof(int) * (size_t)s.nyl * s.pitch) == hipSuccess) &&
              hipMemcpyAsync(map, from, (size_t)s.plane, hipMemcpyDeviceToDevice, s.sc) == hipSuccess;
    if (ok) {
      hipLaunchKernelGGL(lbm::lbm_mark_probes, dim3(cdiv(n, 256)), dim3(256), 0, s.sc, s.pcells, n, map, s.pidx);
      ok = hipGetLastError() == hipSuccess;
    }
    if (!ok) { (void)hipGetLastError(); (void)hipStreamSynchronize(s.sc); wave_probe_free(s, true); }
    return ok;
  };
  if (with_forces && s.fcells_n > 0) {           // (no counted cell: the probe flavour alone, and the fold writes the zeros)
    if (!s.fmap) return false;                   // (wave_force_ready comes first)
    return s.fpmap || build(s.fpmap, s.fmap);
  }
  return s.pmap || build(s.pmap, s.blocked);
}

// One lbm_wave launch: steps tt .. tt+K-1 of the lone slab, launch index li; w: what the run wants from its groups, g: what
// this one is told (lbm_wave_pick.h).  Which flavour runs on which obstacle map is wave_pick's answer; here its arguments
// are filled.  nb_bodies > 0 (lbm_run_forces, wave_force_ready said yes): behind the launch, the fold of the group's forces
// into the run's sums (of nsteps steps).  Probes and fields: wave_probe_ready / wave_admit said yes.
int launch_wave(lbm_ctx* c, int li, int tt, bool accel_out, bool fold_prev, int nb_bodies, int nsteps, const WaveWants& w, const WaveGroup& g) {
  Slab& s = c->slabs[0];
  HIPC(hipSetDevice(s.dev));
  const int K = c->time_block;
  const int nb = wave_blocks(c);
  const int q = li & 1, qp = q ^ 1;
  lbm::WaveArgs a;
  a.src = s.lat[c->cur]; a.dst = s.lat[c->cur ^ 1];
  a.plane = s.plane; a.pitch = s.pitch; a.nx = c->p.nx; a.ny = c->p.ny;
  a.omega = c->p.omega;
  a.accel_row = c->p.ny - 2; a.accel_out = accel_out ? 1 : 0;
  a.a1 = accel_pair(c).a1; a.a2 = accel_pair(c).a2;
  a.H = c->wave_rows;
  a.y_begin = 0; a.y_end = c->p.ny;
  a.nwc = cdiv(c->p.nx, wave_out_cols(c, K)); a.nchunks = cdiv(c->p.ny, a.H);
  a.nchunks_a = a.nchunks; a.yb_begin = a.yb_end = 0;
  if (!wave_partials_fit(c)) return fail(LBM_EINVAL, "lbm_wave: %d blocks exceed the partial-sum buffer (raise wave_rows)", nb);
  a.partials = s.partials[q]; a.pstride = nb; a.pbase = 0;
  a.prev = nullptr; a.prev_count = 0; a.prev_sum = nullptr;
  if (fold_prev) { a.prev = s.partials[qp]; a.prev_count = nb; a.prev_sum = s.sums + (tt - K); }
  // (development: LBM_WAVE_PAD_LDS = bytes of unused dynamic LDS per block, to hold fewer blocks on a CU than the registers
  // allow -- how the rate depends on the waves per SIMD: profiles/r03_wave_occupancy.log)
  static const int pad_lds = getenv("LBM_WAVE_PAD_LDS") ? atoi(getenv("LBM_WAVE_PAD_LDS")) : 0;
  const WavePick p = wave_pick(g.driven, nb_bodies > 0, s.fcells_n > 0, w.pout != nullptr, g.pmask != 0u, w.fout != nullptr, g.fmask != 0u, w.win != nullptr,
                                   w.fstats);
  if (p.refused) return fail(LBM_EINVAL, g.driven ? "lbm_wave: the driven flavour runs beside no fields" : "lbm_wave: the field flavour runs beside neither forces nor probes");
  a.blocked = p.map == WaveMap::fpmap ? s.fpmap : p.map == WaveMap::pmap ? s.pmap : p.map == WaveMap::fmap ? s.fmap : s.blocked;
  a.fidx = nullptr; a.fcells = nullptr; a.contrib = nullptr; a.fcells_n = 0;
  if (p.forces) { a.fidx = s.fidx; a.fcells = s.fcells; a.contrib = s.fcontrib.p; a.fcells_n = s.fcells_n; }
  a.pidx = nullptr; a.pout = nullptr; a.nprobes = 0; a.pmask = 0u; a.prow = 0; a.density = c->p.density;
  if (g.pmask != 0u) { a.pidx = s.pidx; a.pout = w.pout; a.nprobes = c->nprobes; a.pmask = g.pmask; a.prow = g.prow; }
  a.fmask = 0u; a.fout = nullptr; a.fstride = 0; a.fadd = 0;
  a.win = lbm::WaveWin{0, 0, 0, 1u, 1u, 0u, 0u, 0u, 0u};
  if (g.fmask != 0u) {
    a.fmask = g.fmask; a.fout = g.fout; a.fstride = w.fstride; a.fadd = (w.fadd && !w.win) ? 1 : 0;
    if (w.win) a.win = w.win->wave;
  }
  for (int i = 0; i < 16; ++i) a.drv[i] = g.drv[i];
  // (every launch of a wave kernel on a lattice alone goes through here and is counted: info "wave_launches", one per group of K steps)
  hipLaunchKernelGGL(wave_kernel(K, false, wave_C(c, K), (int)(c->variant & (lbm::kFastMath | lbm::kNtStore)), p.flavour),
                     dim3(nb), dim3(lbm::kWaveBlock), pad_lds, s.sc, a);
  ++c->wave_launches;
  HIPC(hipGetLastError());
  if (nb_bodies > 0) {
    hipLaunchKernelGGL(lbm::lbm_fold_wave_forces, dim3(K), dim3(lbm::kBlock), 0, s.sc, s.fcontrib.p, s.fcells, s.fcells_n, nb_bodies,
                       s.sums + nsteps + 1 + (long)tt * 2 * nb_bodies);
    HIPC(hipGetLastError());
  }
  c->cur ^= 1;
  return LBM_OK;
}

// The blocks of one marching launch must fit the per-block partial sums (K floats per block).  Asked BEFORE anything
// of a run is queued -- behind the prologue the lattice would already carry the accelerate phase of a step that is
// then never taken -- and when the chunk heights are set.
int check_march_partials(lbm_ctx* c, bool slabs_march) {
  if (slabs_march) {
    const int K = slab_K(c);
    for (auto& s : c->slabs) {
      const long nb = march_slab_blocks(c, s);
      if ((long)K * nb > s.partial_cap) return fail(LBM_EINVAL, "marching kernel: %ld blocks exceed the partial-sum buffer (raise wave_rows / march_rows)", nb);
    }
  } else if (march_eligible(c)) {
    long nb;
    bool fit;
    if (use_wave_kernel(c)) { nb = wave_blocks(c); fit = wave_partials_fit(c); }
    else {
      if (c->march_rows <= 0) c->march_rows = march_pick_rows(c);
      nb = (long)cdiv(c->p.nx, lbm::MarchCfg<kMarchK>::WOUT) * cdiv(c->p.ny, c->march_rows);
      fit = c->time_block * nb <= c->slabs[0].partial_cap;
    }
    if (!fit)
      return fail(LBM_EINVAL, "marching kernel: %ld blocks exceed the partial-sum buffer (raise wave_rows / march_rows)", nb);
  }
  return LBM_OK;
}

}  // namespace
