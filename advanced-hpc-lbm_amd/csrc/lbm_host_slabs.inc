// lbm_host_slabs.inc -- part of lbm_api.hip (included there, not a translation unit of its own): the layout rules (row
// partition, plane padding, the peer-to-peer halo block: slab_rows, slab_plane, CommLayout), slab allocation and upload, halo
// buffers, the launch helpers of the one- and two-step kernels, the halo exchange and the peer-to-peer hand-off launches, the
// per-step sums, the kernel defaults of a new context (finish_create).
namespace {

int pick_vector_width(int nx) {
  const char* e = getenv("LBM_VECTOR_WIDTH");
  int want = e ? atoi(e) : 4;
  if (want >= 4 && nx % 4 == 0 && nx >= 8) return 4;
  if (want >= 2 && nx % 2 == 0 && nx >= 4) return 2;
  return 1;
}

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- the layout rules, each in ONE place: every slab, and every rank about its neighbours, must come to the same numbers
// The row partition: slab (or rank) i of n holds the global rows [row0, row0 + nyl).
struct RowRange { int row0, nyl; };
inline RowRange slab_rows(int ny, int n, int i) {
  auto first = [=](long j) { return (int)(j * ny / n); };
  return {first(i), first(i + 1) - first(i)};
}
// Floats per plane of a slab of nyl rows: the rows + 20.25 KiB (why: slab_alloc).
inline long slab_plane(int nyl, int pitch) { return (long)nyl * pitch + 5184; }
// The peer-to-peer halo block of a slab (Slab::comm_block), as byte offsets: the four nine-slot halo buffers (halo_bytes
// each, a multiple of 256), the flag line the southern neighbour raises and the one the northern raises, the hipIpc handles
// of lattice 0, lattice 1 and the obstacle map (a neighbouring PROCESS reads the slab's rows in place) and of the mail area
// of the register tiles (zero: none).
struct CommLayout {
  size_t halo_bytes;
  static constexpr size_t kFlagLine = 256, kHandle = sizeof(hipIpcMemHandle_t);
  size_t ghost_s(int par) const { return (size_t)par * halo_bytes; }
  size_t ghost_n(int par) const { return (size_t)(2 + par) * halo_bytes; }
  size_t flag_s() const { return 4 * halo_bytes; }
  size_t flag_n() const { return flag_s() + kFlagLine; }
  size_t lattice_handles() const { return flag_n() + kFlagLine; }
  size_t mail_handle() const { return lattice_handles() + 3 * kHandle; }
  size_t total() const { return mail_handle() + kHandle; }
};
inline CommLayout comm_layout(int nx) { return {(sizeof(float) * lbm::kHaloSlots * (size_t)nx + 255) / 256 * 256}; }
inline CommLayout comm_layout(const Slab& s) { return {s.halo_bytes}; }

// Halo buffers of a slab for the context's exchange mode (callable again after a fallback from
// peer-to-peer to RCCL: slab_free_halos first).
void slab_free_halos(Slab& s) {
  (void)hipSetDevice(s.dev);
  for (int i = 0; i < 2; ++i) {
    if (s.ghost_s[i] && !s.comm_block) (void)hipFree(s.ghost_s[i]);
    if (s.ghost_n[i] && !s.comm_block) (void)hipFree(s.ghost_n[i]);
    if (s.send_s[i]) (void)hipFree(s.send_s[i]);
    if (s.send_n[i]) (void)hipFree(s.send_n[i]);
    s.ghost_s[i] = s.ghost_n[i] = s.send_s[i] = s.send_n[i] = nullptr;
  }
  if (s.blocked_gs) (void)hipFree(s.blocked_gs);
  if (s.blocked_gn) (void)hipFree(s.blocked_gn);
  s.blocked_gs = s.blocked_gn = nullptr;
  for (int i = 0; i < 2; ++i) {
    if (s.band_s[i]) (void)hipFree(s.band_s[i]);
    if (s.band_n[i]) (void)hipFree(s.band_n[i]);
    s.band_s[i] = s.band_n[i] = nullptr;
  }
  if (s.band_send_s) (void)hipFree(s.band_send_s);
  if (s.band_send_n) (void)hipFree(s.band_send_n);
  if (s.band_blk_s) (void)hipFree(s.band_blk_s);
  if (s.band_blk_n) (void)hipFree(s.band_blk_n);
  s.band_send_s = s.band_send_n = nullptr; s.band_blk_s = s.band_blk_n = nullptr; s.band_K = 0;
  for (int side = 0; side < 2; ++side)
    for (int i = 0; i < 3; ++i) {
      if (s.nb_ipc[side][i] && (side == 0 || s.nb_ipc[1][i] != s.nb_ipc[0][i])) (void)hipIpcCloseMemHandle(s.nb_ipc[side][i]);
    }
  for (int side = 0; side < 2; ++side) {
    for (int i = 0; i < 3; ++i) s.nb_ipc[side][i] = nullptr;
    s.nb_lat[side][0] = s.nb_lat[side][1] = nullptr; s.nb_blocked[side] = nullptr;
  }
  if (s.peer_s_ipc && s.peer_s) (void)hipIpcCloseMemHandle(s.peer_s);
  if (s.peer_n_ipc && s.peer_n && s.peer_n != s.peer_s) (void)hipIpcCloseMemHandle(s.peer_n);
  s.peer_s = s.peer_n = nullptr; s.peer_s_ipc = s.peer_n_ipc = false;
  if (s.comm_block) (void)hipFree(s.comm_block);
  if (s.counters) (void)hipFree(s.counters);
  s.comm_block = nullptr; s.counters = nullptr;
}

int slab_alloc_halos(lbm_ctx* c, Slab& s) {
  HIPC(hipSetDevice(s.dev));
  const int nx = c->p.nx;
  if (c->exchange == LBM_EXCHANGE_P2P) {
    HIPC(hipMalloc((void**)&s.blocked_gs, (size_t)nx));
    HIPC(hipMalloc((void**)&s.blocked_gn, (size_t)nx));
    const CommLayout lay = comm_layout(nx);
    const size_t total = lay.total();
    s.halo_bytes = lay.halo_bytes;
    // uncached: the neighbours write it over xGMI behind this GPU's L2.  Fine-grained memory is NOT
    // accepted as a substitute (the local L2 may keep ghost rows a neighbour has since rewritten):
    // without uncached memory peer-to-peer halos count as unavailable and the caller uses RCCL.
    hipError_t e = hipExtMallocWithFlags((void**)&s.comm_block, total, hipDeviceMallocUncached);
    if (e != hipSuccess) { (void)hipGetLastError(); s.comm_block = nullptr; return fail(LBM_EHIP, "cannot allocate uncached halo memory: %s", hipGetErrorString(e)); }
    HIPC(hipMemset(s.comm_block, 0, total));
    HIPC(hipMalloc((void**)&s.counters, 64 * sizeof(uint32_t)));
    HIPC(hipMemset(s.counters, 0, 64 * sizeof(uint32_t)));
    HIPC(hipDeviceSynchronize());
    for (int i = 0; i < 2; ++i) {
      s.ghost_s[i] = (float*)(s.comm_block + lay.ghost_s(i));
      s.ghost_n[i] = (float*)(s.comm_block + lay.ghost_n(i));
    }
    if (c->rank_mode && c->nranks > 1) {
      // a neighbouring PROCESS reads this slab's rows in place (marching launches): it finds the handles here
      hipIpcMemHandle_t h[3];
      HIPC(hipIpcGetMemHandle(&h[0], s.lat[0]));
      HIPC(hipIpcGetMemHandle(&h[1], s.lat[1]));
      HIPC(hipIpcGetMemHandle(&h[2], s.blocked));
      static_assert(sizeof(hipIpcMemHandle_t) == 64, "three handles in 192 bytes");
      HIPC(hipMemcpy(s.comm_block + lay.lattice_handles(), h, sizeof(h), hipMemcpyHostToDevice));
    }
  } else {
    const size_t hb = sizeof(float) * lbm::kHaloSlots * (size_t)nx;
    HIPC(hipMalloc((void**)&s.blocked_gs, (size_t)nx));
    HIPC(hipMalloc((void**)&s.blocked_gn, (size_t)nx));
    HIPC(hipMalloc((void**)&s.band_blk_s, (size_t)kBandRows * s.pitch));
    HIPC(hipMalloc((void**)&s.band_blk_n, (size_t)kBandRows * s.pitch));
    for (int i = 0; i < 2; ++i) {
      HIPC(hipMalloc((void**)&s.ghost_s[i], hb));
      HIPC(hipMalloc((void**)&s.ghost_n[i], hb));
      HIPC(hipMalloc((void**)&s.send_s[i], hb));
      HIPC(hipMalloc((void**)&s.send_n[i], hb));
    }
  }
  return LBM_OK;
}

int slab_alloc(lbm_ctx* c, Slab& s, bool exchanging) {
  HIPC(hipSetDevice(s.dev));
  const int nx = c->p.nx;
  s.pitch = (nx + 63) / 64 * 64;
  // Plane stride: rows + 20.25 KiB.  A power-of-two stride (8192^2: exactly 256 MiB) puts the
  // same cell of all nine planes on the same HBM channel; a few KiB of padding spread the 18
  // concurrent streams (kbench: plain 9-plane copy 4.9 -> 5.4 TB/s, sweep 5.35 -> 5.6 TB/s with
  // 4 KiB; a sweep over pads on two boxes put 5 x 4 KiB + 256 B at or next to the best for the
  // copy, the one-step and the two-step kernels, 2-8 % ahead of 4 KiB).
  s.plane = slab_plane(s.nyl, s.pitch);
  const size_t lat_bytes = sizeof(float) * 9 * (size_t)s.plane;
  for (int i = 0; i < 2; ++i) HIPC(hipMalloc((void**)&s.lat[i], lat_bytes));
  HIPC(hipMalloc((void**)&s.blocked, (size_t)s.plane));
  // one partial per block; worst case V = 1, one launch covering all rows (+2 for split launches)
  s.partial_cap = std::max({cdiv((long)s.nyl * nx, lbm::kBlock), 2 * cdiv(nx, kT2X) * cdiv(s.nyl, kT2Y),
                            4 * cdiv(nx, 224) * s.nyl,
                            8 * cdiv((long)cdiv(nx, 48) * cdiv(s.nyl, 16), 4)}) + 8;   // (last two: the marching kernels with small chunks)
  for (int i = 0; i < 2; ++i) HIPC(hipMalloc((void**)&s.partials[i], sizeof(float) * s.partial_cap));
  s.scratch_cap = s.partial_cap;
  HIPC(hipMalloc((void**)&s.scratch_d, sizeof(double) * (s.scratch_cap + 8)));
  if (exchanging) { int rc = slab_alloc_halos(c, s); if (rc) return rc; }
  HIPC(hipStreamCreateWithFlags(&s.sc, hipStreamNonBlocking));
  {
    int lo = 0, hi = 0;  // numerically lower = higher priority
    HIPC(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPC(hipStreamCreateWithPriority(&s.se, hipStreamNonBlocking, hi));
    HIPC(hipStreamCreateWithPriority(&s.sx, hipStreamNonBlocking, hi));
  }
  // everything that touches slab memory is ordered on s.sc (the streams are
  // non-blocking: a null-stream memset would race with the first kernels)
  HIPC(hipMemsetAsync(s.blocked, 0, (size_t)s.plane, s.sc));
  for (int i = 0; i < 2; ++i) {
    HIPC(hipEventCreateWithFlags(&s.ev_bnd[i], hipEventDisableTiming));
    HIPC(hipEventCreateWithFlags(&s.ev_recv[i], hipEventDisableTiming));
    HIPC(hipEventCreateWithFlags(&s.ev_int[i], hipEventDisableTiming));
  }
  HIPC(hipEventCreate(&s.ev_t0));
  HIPC(hipEventCreate(&s.ev_t1));
  for (int i = 0; i < 2; ++i) HIPC(hipEventCreateWithFlags(&s.ev_march[i], hipEventDisableTiming));
  return LBM_OK;
}

// Blocked maps of the two rows just outside the slab (periodic in the global lattice): the ring
// rows of the two-step kernel.
int upload_ghost_masks(lbm_ctx* c, Slab& s, const int* obstacles) {
  HIPC(hipSetDevice(s.dev));
  const int nx = c->p.nx, ny = c->p.ny;
  const int rs = (s.row0 + ny - 1) % ny, rn = (s.row0 + s.nyl) % ny;
  std::vector<uint8_t> gs(nx), gn(nx);
  for (int x = 0; x < nx; ++x) { gs[x] = obstacles[(long)rs * nx + x] ? 1 : 0; gn[x] = obstacles[(long)rn * nx + x] ? 1 : 0; }
  HIPC(hipMemcpyAsync(s.blocked_gs, gs.data(), nx, hipMemcpyHostToDevice, s.sc));
  HIPC(hipMemcpyAsync(s.blocked_gn, gn.data(), nx, hipMemcpyHostToDevice, s.sc));
  std::vector<uint8_t> bs, bn;
  if (s.band_blk_s) {
    // the kBandRows rows below and above the slab (periodic in the global lattice), for the ghost bands
    bs.assign((size_t)kBandRows * s.pitch, 0); bn.assign((size_t)kBandRows * s.pitch, 0);
    for (int i = 0; i < kBandRows; ++i) {
      const int gs_row = ((s.row0 - kBandRows + i) % ny + ny) % ny, gn_row = (s.row0 + s.nyl + i) % ny;
      for (int x = 0; x < nx; ++x) {
        bs[(size_t)i * s.pitch + x] = obstacles[(long)gs_row * nx + x] ? 1 : 0;
        bn[(size_t)i * s.pitch + x] = obstacles[(long)gn_row * nx + x] ? 1 : 0;
      }
    }
    HIPC(hipMemcpyAsync(s.band_blk_s, bs.data(), bs.size(), hipMemcpyHostToDevice, s.sc));
    HIPC(hipMemcpyAsync(s.band_blk_n, bn.data(), bn.size(), hipMemcpyHostToDevice, s.sc));
  }
  HIPC(hipStreamSynchronize(s.sc));
  return LBM_OK;
}

// A device staging buffer that is released on every path out of its scope.
struct DeviceTemp {
  void* p = nullptr;
  ~DeviceTemp() { if (p) (void)hipFree(p); }
};

// A grow-only device buffer of a slab: room for at least `need` units of `per` floats, old contents not kept.  Grows to
// exactly `need`, or (geometric) by doubling from a floor of 1024.  false: no room -- the HIP error cleared, the buffer empty.
void grown_free(GrownBuf& b) { if (b.p) (void)hipFree(b.p); b = GrownBuf(); }
bool grown_room(const Slab& s, GrownBuf& b, long need, size_t per, bool geometric) {
  if (b.cap >= need) return true;
  long cap = geometric ? std::max(1024L, b.cap) : need;
  while (cap < need) cap *= 2;
  if (hipSetDevice(s.dev) != hipSuccess) { (void)hipGetLastError(); return false; }
  grown_free(b);
  if (hipMalloc((void**)&b.p, sizeof(float) * per * (size_t)cap) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return false; }
  b.cap = cap;
  return true;
}
void observers_free(Slab& s);   // everything a slab holds for the observer calls (lbm_host_observe.inc)

// Uploads the slab's rows of the global host arrays and converts to the device layout.
int slab_upload(lbm_ctx* c, Slab& s, const int* obstacles, const float* cells) {
  HIPC(hipSetDevice(s.dev));
  const int nx = c->p.nx;
  const long ncell = (long)s.nyl * nx;
  const int grid = cdiv(ncell, 256);
  {
    DeviceTemp t;
    HIPC(hipMalloc(&t.p, sizeof(int) * ncell));
    int* d_ob = (int*)t.p;
    HIPC(hipMemcpyAsync(d_ob, obstacles + (long)s.row0 * nx, sizeof(int) * ncell, hipMemcpyHostToDevice, s.sc));
    hipLaunchKernelGGL(lbm::lbm_pack_blocked, dim3(grid), dim3(256), 0, s.sc, d_ob, s.blocked, s.pitch, nx, ncell);
    HIPC(hipGetLastError());
    if (s.blocked_gs) { int rc2 = upload_ghost_masks(c, s, obstacles); if (rc2) return rc2; }
    HIPC(hipStreamSynchronize(s.sc));
  }
  if (cells != nullptr) {
    DeviceTemp t;
    HIPC(hipMalloc(&t.p, sizeof(float) * 9 * ncell));
    float* d_aos = (float*)t.p;
    HIPC(hipMemcpyAsync(d_aos, cells + 9L * s.row0 * nx, sizeof(float) * 9 * ncell, hipMemcpyHostToDevice, s.sc));
    hipLaunchKernelGGL(lbm::lbm_aos_to_soa, dim3(grid), dim3(256), 0, s.sc, d_aos, s.lat[c->cur], s.plane, s.pitch, nx, ncell);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s.sc));
  } else {
    // rest equilibrium, every cell (d2q9-bgk.c:2802-2823); padding columns get it too
    const float w0 = c->p.density * 4.f / 9.f, w1 = c->p.density / 9.f, w2 = c->p.density / 36.f;
    hipLaunchKernelGGL(lbm::lbm_fill_equilibrium, dim3(cdiv(s.plane, 256)), dim3(256), 0, s.sc, s.lat[c->cur], s.plane, w0, w1, w2);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s.sc));
  }
  // the other lattice is fully overwritten by the first step (padding columns never read)
  return LBM_OK;
}

// Default kernel flavour for a context (overridable: LBM_VECTOR_WIDTH / LBM_KERNEL_VARIANT
// env, or lbm_set_option).  Measured on MI355X (tools/kbench, profiles/):
//   * lattices that stay resident in the 256 MiB Infinity Cache (both lattices of 1024^2
//     are 75 MB): 4 cells per thread, default cache policy -- nontemporal accesses bypass
//     the cache the next step would hit (12.9 us vs 15-19 us per step);
//   * lattices streamed from HBM (8192^2: 4.8 GB): 2 cells per thread (8 waves per SIMD)
//     with nontemporal loads and stores (862 us vs 887-940 us per step).
// v_rcp_f32 / v_sqrt_f32 (1 ulp) replace the IEEE divide and sqrt sequences in both.
void pick_defaults(lbm_ctx* c) {
  double bytes = 0;
  for (auto& s : c->slabs) bytes += 2.0 * 9 * sizeof(float) * (double)s.plane;
  const bool cache_resident = bytes / (double)c->slabs.size() <= 160.0 * 1024 * 1024;
  const int nx = c->p.nx;
  if (cache_resident) {
    c->V = pick_vector_width(nx);
    c->variant = lbm::kFastMath;
  } else {
    c->V = (nx % 2 == 0 && nx >= 4) ? 2 : 1;
    c->variant = lbm::kFastMath | lbm::kNtLoad | lbm::kNtStore;
  }
  // Two steps per pass through LDS: 1.4x (1024^2) to 1.65x (8192^2) over the single-step
  // sweep (kbench); nontemporal stores only pay off when the lattice streams from HBM.
  c->time_block = 2;
  // Threads per 64 x 16 tile of the two-step kernel (tools/t2_threads_check.py,
  // tools/strong_scaling_proxy.py): 512 (2 cells per thread and phase, 62 VGPRs, 32 waves per CU)
  // beats 256 on every lattice alone on a GPU -- 1024^2 8.7 -> 7.6 us/step, 128^2/256^2 4.1 -> 3.3,
  // 8192^2 equal -- and on slabs; a slab with at most one tile per CU (1024 x 128 on one of 8
  // GPUs) is bound by a single block's serial chain and does best with 1024 (4.6 -> 4.3 us/step).
  c->t2_threads = 512;
  if (c->exchange != 0) {
    long tiles = 0;
    for (auto& s : c->slabs) tiles = std::max(tiles, (long)(nx / kT2X) * (s.nyl / kT2Y));
    if (tiles <= 256) c->t2_threads = 1024;
  }
  const char* e;
  if ((e = getenv("LBM_VECTOR_WIDTH"))) c->V = pick_vector_width(nx);
  if ((e = getenv("LBM_KERNEL_VARIANT"))) c->variant = atol(e) & 15;
  if ((e = getenv("LBM_TIME_BLOCK"))) { const int v = atoi(e); c->time_block = (v == 8 || v == 6 || v == 4 || v == 2) ? v : 1; }
  if ((e = getenv("LBM_MARCH_KERNEL"))) c->march_kernel = atoi(e) == 0 ? 0 : atoi(e) == 1 ? 1 : -1;
  if ((e = getenv("LBM_WAVE_ROWS")) && atoi(e) > 0) c->wave_rows = std::min(atoi(e), c->p.ny);
  if ((e = getenv("LBM_WAVE_COLS"))) c->wave_cols = atoi(e) == 2 ? 2 : 1;
  if ((e = getenv("LBM_MARCH_ROWS")) && atoi(e) > 0) c->march_rows = std::min(atoi(e), c->p.ny);
  if ((e = getenv("LBM_T2_THREADS"))) { const int t = atoi(e); if (t == 256 || t == 512 || t == 1024) c->t2_threads = t; }
}

// The two-step kernel covers whole 64 x 16 tiles.  With neighbours every slab must tile too,
// and every rank must come to the same answer (the halo message size depends on it).
bool t2_eligible(const lbm_ctx* c) {
  if (c->time_block < 2 || (c->variant & 8)) return false;   // (variant bit 3: the reference's speed sum, one-step kernel only)
  // a slab alone: any lattice of at least one tile (partial tiles at the east / north end)
  if (c->exchange == 0) return c->slabs.size() == 1 && c->p.nx >= kT2X && c->p.ny >= kT2Y;
  return c->p.nx % kT2X == 0 && c->p.ny % (c->nranks * kT2Y) == 0;
}

// Steps per pass of the marching kernel (lbm_march.hip.h).
constexpr int kMarchK = 4;
// lbm_wave: columns per lane actually used (two need an even width of at least one 128-column strip and K = 8),
// and the columns a wave delivers
inline int wave_C(const lbm_ctx* c, int K) { return (c->wave_cols == 2 && K == 8 && c->p.nx % 2 == 0 && c->p.nx >= 128) ? 2 : 1; }
inline int wave_out_cols(const lbm_ctx* c, int K) { return 64 * wave_C(c, K) - 2 * K; }

// The marching kernel runs on a lattice alone on its GPU (periodic wrap inside the kernel); its row
// fetches are 16-byte LDS-DMA pieces, so columns must come in fours, and a strip is 256 columns wide.
inline bool march_block_ok(const lbm_ctx* c) {   // lbm_march's own requirements
  return c->time_block == kMarchK && c->p.nx % 4 == 0 && c->p.nx >= lbm::MarchCfg<kMarchK>::W && c->p.ny >= 2 * kMarchK;
}
inline bool use_wave_kernel(const lbm_ctx* c) { return c->march_kernel == 1 || (c->march_kernel < 0 && !march_block_ok(c)); }
bool march_eligible(const lbm_ctx* c) {
  if (c->time_block < 4 || c->exchange != 0 || c->slabs.size() != 1 || (c->variant & 8)) return false;
  if ((double)c->p.ny * c->slabs[0].pitch * 4.0 >= 4.0e9) return false;   // 32-bit byte offsets inside a plane
  // lbm_wave: any width of at least one wave; ny >= 2K because the kernel applies the accelerate phase at two
  // periodic images of row ny-2 per chunk (lbm_wave.hip.h: jacc, jacc2) and a chunk plus its 2K fill rows spans
  // up to ny + 2K rows: on a shorter lattice a third image would fall among them
  if (use_wave_kernel(c)) return c->p.nx >= 64 && c->p.ny >= 2 * c->time_block;
  return march_block_ok(c);
}

// Useful rows over rows of time for chunks of h rows: `rounds` rounds of full-height blocks on every CU,
// each paying its fill iterations.
double march_efficiency(const lbm_ctx* c, int h) {
  const int ns = cdiv(c->p.nx, lbm::MarchCfg<kMarchK>::WOUT), ncu = std::max(c->ncu, 1), ny = c->p.ny;
  const long blocks = (long)ns * cdiv(ny, h);
  const long rounds = (blocks + ncu - 1) / ncu;
  return (double)ny * ns / ((double)rounds * ncu * (h + 3 * (kMarchK - 1)));
}

int march_pick_rows(const lbm_ctx* c) {
  const int ny = c->p.ny;
  int best_h = std::min(ny, 256);
  double best = -1.0;
  for (int h = std::min(ny, 32); h <= std::min(ny, 1024); ++h) {
    const double eff = march_efficiency(c, h);
    if (eff > best + 1e-9) { best = eff; best_h = h; }
  }
  return best_h;
}

// Tiles of a lone slab (partial ones included).
inline int t2_tiles(const lbm_ctx* c, int nyl) { return cdiv(c->p.nx, kT2X) * cdiv(nyl, kT2Y); }

template <int MODE, int KIND, int NT>
void launch_sweep2_mkn(const lbm::Sweep2Args& a, int grid, hipStream_t st) {
  if constexpr (KIND == lbm::kSweep2Plain) {
    if (a.nx % kT2X != 0 || a.ny % kT2Y != 0) {   // lone slab that does not tile exactly
      hipLaunchKernelGGL((lbm::lbm_sweep2<kT2X, kT2Y, MODE, KIND, NT, true>), dim3(grid), dim3(NT), 0, st, a);
      return;
    }
  }
  hipLaunchKernelGGL((lbm::lbm_sweep2<kT2X, kT2Y, MODE, KIND, NT, false>), dim3(grid), dim3(NT), 0, st, a);
}

template <int MODE, int KIND>
void launch_sweep2_mk(const lbm_ctx* c, const lbm::Sweep2Args& a, int grid, hipStream_t st) {
  int nt = c->t2_threads;                      // threads per tile: see lbm_sweep2
  if (a.nx % (1024 / nt) != 0) nt = 1024;      // phase B moves 1024/nt cells per thread as one vector
  switch (nt) {
    case 1024: launch_sweep2_mkn<MODE, KIND, 1024>(a, grid, st); break;
    case 512: launch_sweep2_mkn<MODE, KIND, 512>(a, grid, st); break;
    default: launch_sweep2_mkn<MODE, KIND, 256>(a, grid, st); break;
  }
}

template <int KIND>
void launch_sweep2_k(const lbm_ctx* c, const lbm::Sweep2Args& a, int grid, hipStream_t st) {
  // cache-resident lattices: default policy; streamed lattices: nontemporal stores (kbench)
  switch ((int)(c->variant & (lbm::kFastMath | lbm::kNtStore))) {
    case 0: launch_sweep2_mk<0, KIND>(c, a, grid, st); break;
    case 1: launch_sweep2_mk<1, KIND>(c, a, grid, st); break;
    case 2: launch_sweep2_mk<2, KIND>(c, a, grid, st); break;
    default: launch_sweep2_mk<3, KIND>(c, a, grid, st); break;
  }
}

void launch_sweep2(const lbm_ctx* c, const lbm::Sweep2Args& a, int grid, hipStream_t st, bool edge) {
  if (edge) launch_sweep2_k<lbm::kSweep2Edge>(c, a, grid, st);
  else launch_sweep2_k<lbm::kSweep2Plain>(c, a, grid, st);
}
// ... and of its peer-to-peer kind (defined at the end of lbm_host_run.inc: the code object keeps its kernels in the order
// in which the source first asks for them, and these come last)
void launch_sweep2_p2p(const lbm_ctx* c, const lbm::Sweep2Args& a, int grid, hipStream_t st);

void slab_free(Slab& s) {
  slab_free_halos(s);
  (void)hipSetDevice(s.dev);
  for (int i = 0; i < 2; ++i) {
    if (s.lat[i]) (void)hipFree(s.lat[i]);
    if (s.partials[i]) (void)hipFree(s.partials[i]);
    if (s.ev_bnd[i]) (void)hipEventDestroy(s.ev_bnd[i]);
    if (s.ev_recv[i]) (void)hipEventDestroy(s.ev_recv[i]);
    if (s.ev_int[i]) (void)hipEventDestroy(s.ev_int[i]);
  }
  if (s.blocked) (void)hipFree(s.blocked);
  observers_free(s);
  if (s.sums && !s.sums_direct) (void)hipFree(s.sums);
  if (s.sums_host) (void)hipHostFree(s.sums_host);
  if (s.err_host) (void)hipHostFree(s.err_host);
  if (s.scratch_d) (void)hipFree(s.scratch_d);
  for (int i = 0; i < 2; ++i) if (s.ev_march[i]) (void)hipEventDestroy(s.ev_march[i]);
  if (s.ev_t0) (void)hipEventDestroy(s.ev_t0);
  if (s.ev_t1) (void)hipEventDestroy(s.ev_t1);
  if (s.comm) (void)rccl::CommDestroy(s.comm);
  if (s.sc) (void)hipStreamDestroy(s.sc);
  if (s.se) (void)hipStreamDestroy(s.se);
  if (s.sx) (void)hipStreamDestroy(s.sx);
}

int check_params(const lbm_param* p) {
  if (!p) return fail(LBM_EINVAL, "params is NULL");
  if (p->nx < 1 || p->ny < 2) return fail(LBM_EINVAL, "lattice must be at least 1 x 2 (got %d x %d)", p->nx, p->ny);
  if ((long)p->nx * p->ny > (1L << 31) - 1) return fail(LBM_EINVAL, "lattice too large for int cell indices");
  return LBM_OK;
}

long count_fluid(const int* obstacles, long n) {
  long f = 0;
  for (long i = 0; i < n; ++i) f += obstacles[i] ? 0 : 1;
  return f;
}

// Launches one sweep over rows y_begin + i*y_stride of slab s.
template <int V, int MODE>
void launch_sweep_vm(const lbm::SweepArgs& a, hipStream_t st) {
  const long threads = (long)a.y_count * (a.nx / V);
  const int grid = cdiv(threads, lbm::kBlock);
  hipLaunchKernelGGL((lbm::lbm_sweep<V, MODE>), dim3(grid), dim3(lbm::kBlock), 0, st, a);
}

// variant = lbm::kFastMath | kNtStore | kNtLoad bits (option "kernel_variant"); bit 3 (value 8) = the step's average
// speed re-summed from the stored populations, the reference's form (lbm::kSpeedFromStored; one-step kernel only)
template <int V>
void launch_sweep_v(const lbm::SweepArgs& a, hipStream_t st, long variant) {
  constexpr int S = lbm::kSpeedFromStored;
  switch (variant & 15) {
    case 0: launch_sweep_vm<V, 0>(a, st); break;
    case 1: launch_sweep_vm<V, 1>(a, st); break;
    case 2: launch_sweep_vm<V, 2>(a, st); break;
    case 3: launch_sweep_vm<V, 3>(a, st); break;
    case 4: launch_sweep_vm<V, 4>(a, st); break;
    case 5: launch_sweep_vm<V, 5>(a, st); break;
    case 6: launch_sweep_vm<V, 6>(a, st); break;
    case 7: launch_sweep_vm<V, 7>(a, st); break;
    case 8: launch_sweep_vm<V, S | 0>(a, st); break;
    case 9: launch_sweep_vm<V, S | 1>(a, st); break;
    case 10: launch_sweep_vm<V, S | 2>(a, st); break;
    case 11: launch_sweep_vm<V, S | 3>(a, st); break;
    case 12: launch_sweep_vm<V, S | 4>(a, st); break;
    case 13: launch_sweep_vm<V, S | 5>(a, st); break;
    case 14: launch_sweep_vm<V, S | 6>(a, st); break;
    default: launch_sweep_vm<V, S | 7>(a, st); break;
  }
}

int sweep_blocks(const lbm_ctx* c, int y_count) {
  return cdiv((long)y_count * (c->p.nx / c->V), lbm::kBlock);
}

void launch_sweep(const lbm_ctx* c, const lbm::SweepArgs& a, hipStream_t st) {
  switch (c->V) {
    case 4: launch_sweep_v<4>(a, st, c->variant); break;
    case 2: launch_sweep_v<2>(a, st, c->variant); break;
    default: launch_sweep_v<1>(a, st, c->variant); break;
  }
}

// Halo exchange for parity q on the exchange streams (all local slabs): slots
// [slot0, slot0 + nslots) of the nine-slot halo buffers (lbm_kernels.hip.h, kHaloSlots).
int exchange_halos(lbm_ctx* c, int q, int slot0, int nslots) {
  const size_t off = (size_t)slot0 * c->p.nx;
  const size_t n = (size_t)nslots * c->p.nx;
  const int ns = (int)c->slabs.size();
  if (c->exchange == LBM_EXCHANGE_RCCL) {
    for (auto& s : c->slabs) {
      HIPC(hipSetDevice(s.dev));
      HIPC(hipStreamWaitEvent(s.sx, s.ev_bnd[q], 0));
    }
    NCCLC(rccl::GroupStart());
    for (int i = 0; i < ns; ++i) {
      Slab& s = c->slabs[i];
      const int me = c->rank_mode ? c->rank : i;
      const int south = (me + c->nranks - 1) % c->nranks, north = (me + 1) % c->nranks;
      // order matters when south == north (2 ranks): sends S then N, receives N then S
      NCCLC(rccl::Send(s.send_s[q] + off, n, rccl::kFloat32, south, s.comm, s.sx));
      NCCLC(rccl::Send(s.send_n[q] + off, n, rccl::kFloat32, north, s.comm, s.sx));
      NCCLC(rccl::Recv(s.ghost_n[q] + off, n, rccl::kFloat32, north, s.comm, s.sx));
      NCCLC(rccl::Recv(s.ghost_s[q] + off, n, rccl::kFloat32, south, s.comm, s.sx));
    }
    NCCLC(rccl::GroupEnd());
    for (auto& s : c->slabs) {
      HIPC(hipSetDevice(s.dev));
      HIPC(hipEventRecord(s.ev_recv[q], s.sx));
    }
  } else {  // LBM_EXCHANGE_COPY: the receiver pulls from its neighbours' send buffers
    for (int i = 0; i < ns; ++i) {
      Slab& s = c->slabs[i];
      Slab& so = c->slabs[(i + ns - 1) % ns];
      Slab& no = c->slabs[(i + 1) % ns];
      HIPC(hipSetDevice(s.dev));
      HIPC(hipStreamWaitEvent(s.sx, s.ev_bnd[q], 0));
      HIPC(hipStreamWaitEvent(s.sx, so.ev_bnd[q], 0));
      HIPC(hipStreamWaitEvent(s.sx, no.ev_bnd[q], 0));
      HIPC(hipMemcpyAsync(s.ghost_s[q] + off, so.send_n[q] + off, sizeof(float) * n, hipMemcpyDeviceToDevice, s.sx));
      HIPC(hipMemcpyAsync(s.ghost_n[q] + off, no.send_s[q] + off, sizeof(float) * n, hipMemcpyDeviceToDevice, s.sx));
      HIPC(hipEventRecord(s.ev_recv[q], s.sx));
    }
  }
  return LBM_OK;
}

// ---- peer-to-peer halos (LBM_EXCHANGE_P2P): no events, no host-side exchange -- launch group `seq` of a slab hands off
// through the flags in the halo blocks (lbm::P2PSync).
// The pointers of a slab for launch group `seq`; bumps the completion targets by the number of blocks that will count
// themselves done on each side.
lbm::P2PSync p2p_sync(Slab& s, uint32_t seq, int blocks_s, int blocks_n) {
  lbm::P2PSync y;
  const CommLayout lay = comm_layout(s);
  y.flag_s = (const uint32_t*)(s.comm_block + lay.flag_s());
  y.flag_n = (const uint32_t*)(s.comm_block + lay.flag_n());
  y.rem_flag_s = (uint32_t*)(s.peer_s + lay.flag_n());   // I am the south neighbour's NORTH side
  y.rem_flag_n = (uint32_t*)(s.peer_n + lay.flag_s());
  y.cnt_s = s.counters; y.cnt_n = s.counters + 16; y.err = s.counters + 32;
  s.cnt_s_total += (uint32_t)blocks_s; s.cnt_n_total += (uint32_t)blocks_n;
  y.cnt_target_s = s.cnt_s_total; y.cnt_target_n = s.cnt_n_total;
  y.seq = seq;
  return y;
}
inline float* p2p_remote_s(const Slab& s, uint32_t seq) { return (float*)(s.peer_s + comm_layout(s).ghost_n(seq & 1)); }  // its ghost_n
inline float* p2p_remote_n(const Slab& s, uint32_t seq) { return (float*)(s.peer_n + comm_layout(s).ghost_s(seq & 1)); }  // its ghost_s
// One launch of lbm_p2p_push for group seq: waits for both neighbours' seq - 1; then, given a lattice, packs its edge rows
// and pushes them into the neighbours' blocks as seq (lat == nullptr: the wait alone, one block).
int p2p_push(const lbm_ctx* c, Slab& s, const float* lat, uint32_t seq) {
  const int push = lat ? 1 : 0, grid = push ? cdiv(c->p.nx, lbm::kBlock) : 1;
  const lbm::P2PSync y = p2p_sync(s, seq, push * grid, push * grid);
  hipLaunchKernelGGL(lbm::lbm_p2p_push, dim3(grid), dim3(lbm::kBlock), 0, s.sc, lat, s.plane, s.pitch, c->p.nx, s.nyl,
                     p2p_remote_s(s, seq), p2p_remote_n(s, seq), y, push);
  HIPC(hipGetLastError());
  return LBM_OK;
}
// ... and of lbm_p2p_raise: "my launch group seq is over", into both neighbours' flags (the marching launches, which push nothing)
int p2p_raise(Slab& s, uint32_t seq) {
  const CommLayout lay = comm_layout(s);
  hipLaunchKernelGGL(lbm::lbm_p2p_raise, dim3(1), dim3(64), 0, s.sc, (uint32_t*)(s.peer_s + lay.flag_n()), (uint32_t*)(s.peer_n + lay.flag_s()), seq);
  HIPC(hipGetLastError());
  return LBM_OK;
}

// Per-step sums of a run.  Sized once at lbm_create for the deck's own maxIters and grown
// geometrically, so that a run never allocates unless it is longer than anything before it (an
// allocation inside lbm_run costs more than a 20-step run of 1024^2).  Where no collective reduces
// them on the device (every context but a rank of a process-per-GPU job), the folding blocks store
// each step's double straight into pinned host memory -- one posted 8-byte write per step -- and a
// run ends without a device-to-host copy (two queued copies cost ~10 us of a 150-us 20-step run);
// a rank keeps a device array (RCCL reduces it) and a pinned staging copy.
int ensure_sums(Slab& s, int nsteps) {
  if (s.sums_cap >= nsteps) return LBM_OK;
  HIPC(hipSetDevice(s.dev));
  int cap = std::max(1024, s.sums_cap);
  while (cap < nsteps) cap = (cap > (1 << 29)) ? nsteps : cap * 2;
  if (s.sums && !s.sums_direct) HIPC(hipFree(s.sums));
  if (s.sums_host) HIPC(hipHostFree(s.sums_host));
  s.sums = nullptr; s.sums_host = nullptr; s.sums_cap = 0;
  HIPC(hipHostMalloc((void**)&s.sums_host, sizeof(double) * cap, hipHostMallocPortable | hipHostMallocMapped));
  if (s.sums_direct) HIPC(hipHostGetDevicePointer((void**)&s.sums, s.sums_host, 0));
  else HIPC(hipMalloc((void**)&s.sums, sizeof(double) * cap));
  if (!s.err_host) {
    HIPC(hipHostMalloc((void**)&s.err_host, 64, hipHostMallocPortable | hipHostMallocMapped));
    memset(s.err_host, 0, 64);
  }
  s.sums_cap = cap;
  return LBM_OK;
}

bool plan_regtile(lbm_ctx* c);    // resident engine, below
bool plan_regtile_slabs(lbm_ctx* c);
bool regtile_tiling_rule(int nx, int rows, int per_dev, int ncu, int* ty_out, int* r_out);
struct Slab;
int regtile_mail_alloc(lbm_ctx* c, Slab& s);
size_t regtile_mail_bytes(const lbm_ctx* c);
typedef void (*wave_fn)(const lbm::WaveArgs);
wave_fn wave_kernel(int K, bool slab, int C, int math, WaveFlavour f);   // the lbm_wave instantiations, below
bool march_slabs_setup(lbm_ctx* c);   // marching kernel across slabs, below
int wave_blocks_per_cu(int K, int C);        // occupancy of lbm_wave<K, ., ., C>, below
bool p2p_march_pays(const lbm_ctx* c);
bool slab_wave_pays(const lbm_ctx* c, int rows, int K = 8);
int slab_wave_rows(const lbm_ctx* c, int ny_rows, int K = 8, int extra_waves = 0);
double slab_wave_efficiency(const lbm_ctx* c, int ny_rows, int h, int K = 8, int extra_waves = 0);
int march_rows_for(const lbm_ctx* c, int ny_rows);
int wave_slots(const lbm_ctx* c, int K);

// lbm_wave<8>: one or two columns per lane?  Each form is priced by what it does with a full chip -- 394 GLUPS with one
// column (three waves per SIMD, 48 of 64 lanes delivered), 456 with two (two waves per SIMD, 112 of 128 delivered, the two
// cells of a lane issued statement by statement; both figures rose by 6 / 11 % with the 70-instruction collision, the
// measurements quoted below are from before it) -- times the useful share of its wave-slot time with its best chunk
// height on `rows` rows.  Measured in one call (profiles/r03_wave_two_columns.log): 8192^2 348 against 320 GLUPS (149-row
// chunks: 4070 waves for 2 x 2048 slots), 6144^2 324 against 314, 4096^2 219 against 274 (too few waves for two rounds);
// 8192-wide slabs of N = 2 / 4 / 8: 113 / 62.8 / 35.5 us per step against 119 / 66.7 / 37.4.  What the two-column form wants
// is a chunk height that fills WHOLE rounds of its 2048 wave slots -- one round is as good as two: 4096^2 with 75-row chunks
// (2035 waves) 321 GLUPS, with 74-row chunks (2072 waves: a second round for 24 of them) 208; lbm_march there: 278.
// Sets c->wave_cols (unless the caller fixed it) and returns the predicted rate of the form chosen.
double wave_pick_cols(lbm_ctx* c, int rows, int* rows_per_chunk) {
  const bool fixed = getenv("LBM_WAVE_COLS") != nullptr;
  double best = -1.0;
  int best_c = c->wave_cols, best_h = 0;
  for (int cols : {1, 2}) {
    if (fixed && cols != c->wave_cols) continue;
    if (cols == 2 && !(c->p.nx % 2 == 0 && c->p.nx >= 128)) continue;
    const int was = c->wave_cols;
    c->wave_cols = cols;
    const int h = slab_wave_rows(c, rows, 8);
    const double rate = (cols == 2 ? 456.0 : 394.0) * slab_wave_efficiency(c, rows, h, 8);
    c->wave_cols = was;
    if (rate > best) { best = rate; best_c = cols; best_h = h; }
  }
  c->wave_cols = best_c;
  if (rows_per_chunk) *rows_per_chunk = best_h;
  return best;
}

int finish_create(lbm_ctx* c, const int* obstacles, const float* cells) {
  const bool exchanging = c->exchange != 0;
  const int ay = c->p.ny - 2;  // the accelerate row of the global lattice (d2q9-bgk.c:240)
  {
    const int nx = c->p.nx, ny = c->p.ny;
    c->keep_row0 = c->slabs.front().row0 - 1;
    c->keep_rows = c->slabs.back().row0 + c->slabs.back().nyl + 1 - c->keep_row0;
    c->obst_keep.resize((size_t)c->keep_rows * nx);
    for (int i = 0; i < c->keep_rows; ++i) {
      const long gy = ((long)(c->keep_row0 + i) % ny + ny) % ny;
      for (int x = 0; x < nx; ++x) c->obst_keep[(size_t)i * nx + x] = obstacles[gy * nx + x] ? 1 : 0;
    }
  }
  for (auto& s : c->slabs) {
    s.accel_row = (ay >= s.row0 && ay < s.row0 + s.nyl) ? ay - s.row0 : -1;
    int rc = slab_alloc(c, s, exchanging);
    if (rc) return rc;
    rc = slab_upload(c, s, obstacles, cells);
    if (rc) return rc;
    s.sums_direct = !c->rank_mode;
    rc = ensure_sums(s, std::max(c->p.maxIters, 1));
    if (rc) return rc;
  }
  pick_defaults(c);
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->slabs[0].dev) == hipSuccess) c->ncu = prop.multiProcessorCount;
    else (void)hipGetLastError();
    const char* e = getenv("LBM_ENGINE");
    if (e) c->engine = (atoi(e) == 0 || atoi(e) == 1 || atoi(e) == 3) ? atoi(e) : 0;
    if ((e = getenv("LBM_REGTILE_ASYNC"))) c->regtile_async = atoi(e) ? 1 : 0;
    if (!exchanging && c->slabs.size() == 1) plan_regtile(c);
    if (exchanging && plan_regtile_slabs(c) && c->rank_mode && c->nranks > 1) {
      // one process per GPU: the neighbours find this slab's mail area through a hipIpc handle in its halo block
      Slab& s0 = c->slabs[0];
      int rc = regtile_mail_alloc(c, s0);
      if (rc) { (void)hipGetLastError(); c->tplan.ty = 0; }
      else {
        hipIpcMemHandle_t h;
        if (hipIpcGetMemHandle(&h, s0.tmail) != hipSuccess) { (void)hipGetLastError(); c->tplan.ty = 0; }
        else HIPC(hipMemcpy(s0.comm_block + comm_layout(s0).mail_handle(), &h, sizeof(h), hipMemcpyHostToDevice));
      }
    }
    // Four steps per pass (lbm_march) where its strips and chunks fill the chip: measured 1.5-1.6x
    // lbm_sweep2 from 2048^2 up (194 / 226 / 238 GLUPS at 2048^2 / 4096^2 / 8192^2 against 129 / 146 /
    // 150), 0.8x at 1024^2, where 5 strips x 32-row chunks leave the CUs 49 % busy by the estimate
    // below (2048^2: 88 %).
    if (!getenv("LBM_TIME_BLOCK") && c->time_block == 2 && exchanging && c->exchange == LBM_EXCHANGE_P2P) {
      // peer-to-peer halos (one process or one process per GPU): lbm_march where the smallest slab fills the chip
      // (a function of the lattice and the number of slabs only: every rank decides alike)
      if (c->p.nx % 4 == 0 && c->p.nx >= lbm::MarchCfg<kMarchK>::W && c->p.ny / c->nranks >= 4 * kMarchK && p2p_march_pays(c)) c->time_block = 4;
      if (c->time_block == 4 && c->march_kernel != 0 && !getenv("LBM_MARCH_KERNEL")) {
        // lbm_wave<8> (one or two columns per lane, whichever the model prices higher) where its waves fill a round of the chip
        const int rows = c->p.ny / c->nranks;
        wave_pick_cols(c, rows, nullptr);
        if (slab_wave_pays(c, rows, 8)) c->time_block = 8; else c->wave_cols = 1;
      }
    } else
    if (!getenv("LBM_TIME_BLOCK") && c->time_block == 2 && exchanging && c->exchange == LBM_EXCHANGE_RCCL) {
      // RCCL halos (one process per GPU, or one process with a slab per GPU): lbm_wave<8> with ghost bands -- K rows of all
      // nine planes per direction per K steps -- where the smallest slab fills the chip's wave slots (every rank decides alike)
      // (one column per lane: with the slab cut into an edge launch and an interior launch the two-column form's fewer, fatter
      // waves measured behind -- ring of one, 8192-wide slabs of N = 1 / 2 / 4 / 8: 256 / 134 / 71.0 / 40.4 us per step against
      // 219 / 122 / 68.3 / 39.1)
      if (c->march_kernel != 0 && slab_wave_pays(c, c->p.ny / c->nranks)) c->time_block = 8;
    } else
    if (!getenv("LBM_TIME_BLOCK") && c->time_block == 2 && exchanging) {
      // slabs of one process: lbm_march with the neighbours' rows read in place, where every slab fills the chip
      c->time_block = 4;
      bool ok = c->march_kernel != 1 && march_slabs_setup(c);
      for (auto& s : c->slabs) {
        if (!ok) break;
        const int h = march_rows_for(c, s.nyl), ns = cdiv(c->p.nx, lbm::MarchCfg<kMarchK>::WOUT);
        const long blocks = (long)ns * cdiv(s.nyl, h), rounds = (blocks + c->ncu - 1) / std::max(c->ncu, 1);
        if ((double)s.nyl * ns / ((double)rounds * std::max(c->ncu, 1) * (h + 3 * (kMarchK - 1))) < 0.65) ok = false;
      }
      if (!ok) { c->time_block = 2; c->march_slabs = -1; }
      else if (c->march_kernel != 0 && !getenv("LBM_MARCH_KERNEL")) {
        int smallest = c->p.ny;
        for (auto& s : c->slabs) smallest = std::min(smallest, s.nyl);
        wave_pick_cols(c, smallest, nullptr);
        bool w8 = true;
        for (auto& s : c->slabs) w8 = w8 && slab_wave_pays(c, s.nyl);
        if (w8) c->time_block = 8; else c->wave_cols = 1;
      }
    } else
    if (!getenv("LBM_TIME_BLOCK") && c->time_block == 2) {
      c->time_block = 4;
      if (!march_eligible(c)) c->time_block = 2;
      else if (!use_wave_kernel(c)) { if (march_efficiency(c, march_pick_rows(c)) < 0.65) c->time_block = 2; }
      else if ((long)c->p.nx * c->p.ny < (3L << 20)) c->time_block = 2;   // lbm_wave needs a few thousand waves: from about 2048^2
      else c->time_block = 6;
      // Eight steps per pass in registers (lbm_wave<8>, 10.5 B per update, bound by its arithmetic) against lbm_march
      // (19.4 B, bound by HBM): each priced by what it does with a full chip -- 371 and 300 GLUPS -- times the share of
      // its slot-iterations that are useful with the best chunk height.  Measured in one call, lbm_wave<8> with the
      // chunk height of the model / lbm_march: 8192^2 328 / 284, 7168^2 329 / 299, 6144^2 325 / 302, 5120^2 310 / 294
      // (91-row chunks = 1.99 rounds; 87 rows = 2.06 rounds: 282), 4608^2 308 / 295, 4096^2 287 / 280, 3072^2 265 / 259,
      // 2048^2 201 / 230.
      if (c->time_block == 4 && c->march_kernel < 0 && !getenv("LBM_MARCH_KERNEL") && c->p.nx >= 64 && c->p.ny >= 32 &&
          (double)c->p.ny * c->slabs[0].pitch * 4.0 < 4.0e9) {
        int h = 0;
        const int cols_was = c->wave_cols;
        // (x 0.88: for a single short round the wave-slot model is about a tenth too pessimistic -- 2048^2 predicted 205, measured
        // 247, lbm_march 231; 2560^2 254 / 277-281 / 254 -- profiles/r03_default_kernel_by_size.log)
        if (wave_pick_cols(c, c->p.ny, &h) >= 0.88 * 300.0 * march_efficiency(c, march_pick_rows(c))) {
          c->time_block = 8; c->march_kernel = 1;
          if (c->wave_rows <= 0) c->wave_rows = h;
        } else c->wave_cols = cols_was;
      }
    }
  }
  return LBM_OK;
}

}  // namespace
