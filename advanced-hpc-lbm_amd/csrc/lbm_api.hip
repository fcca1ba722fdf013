// lbm_api.hip -- the C ABI of include/lbm_mi355x.h on top of the HIP kernels.
//
// Host-side structure (MI355X-first, nothing here mirrors the reference's
// serial layout):
//   * a context owns one or more ROW SLABS; each slab lives on one GPU with
//     both lattices resident in HBM as 9 SoA planes, a byte mask and nine-slot
//     halo buffers per launch parity;
//   * a launch group advances the lattice by two steps (lbm_sweep2, wherever
//     the lattice tiles) or by one (lbm_sweep);
//   * slabs with neighbours trade halos once per launch group, by one of three
//     transports: RCCL send/recv on a second stream between an edge launch and
//     the interior launch it overlaps (events join the streams); peer copies
//     inside one process; or peer-to-peer -- the edge tiles of ONE launch per
//     group store straight into the neighbour's halo block over xGMI and hand
//     off through flags polled in-kernel (no events, no host-side exchange,
//     no collective in the loop);
//   * ONE step loop, run_steps, for all of them: prologue, groups of K steps,
//     pairs, single steps, the fold of the last launch's sums.  The transport
//     is a branch inside each launch group (lbm_host_march.inc), and the parts
//     every group needs -- kernel arguments, the accelerate and fold launches,
//     the layout of slabs and halo blocks -- stand once (lbm_host_slabs.inc,
//     lbm_host_march.inc);
//   * no host synchronisation inside the step loop; per-step speed sums stay
//     on the device (one double per step and slab, folded from per-block
//     partials by block 0 of the NEXT launch) and are reduced once at the end
//     of the run.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <chrono>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lbm_mi355x.h"
#include "lbm_kernels.hip.h"
#include "lbm_march.hip.h"
#include "lbm_wave.hip.h"
#include "lbm_regtile.hip.h"
#include "lbm_live.hip.h"
#include "lbm_tile_table.h"
#include "lbm_wave_pick.h"

// ----------------------------------------------------------------- errors
static thread_local char g_err[1024] = "";

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIPC(call)                                                                         \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(LBM_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

extern "C" const char* lbm_last_error(void) { return g_err; }

// ----------------------------------------------------------------- RCCL (loaded on demand)
// Minimal declarations of the RCCL entry points used (rccl.h: ncclGetUniqueId,
// ncclCommInitRank, ncclCommInitAll, ncclSend/ncclRecv, ncclGroupStart/End,
// ncclAllReduce, ncclCommDestroy).  dlopen by SONAME so that inside a process
// that already carries RCCL (PyTorch) the same instance is shared.
namespace rccl {
typedef struct ncclComm* comm_t;
struct unique_id { char internal[128]; };
enum { kInt8 = 0, kFloat32 = 7, kFloat64 = 8, kSum = 0 };
static int (*GetUniqueId)(unique_id*);
static int (*CommInitRank)(comm_t*, int, unique_id, int);
static int (*CommInitAll)(comm_t*, int, const int*);
static int (*CommDestroy)(comm_t);
static int (*Send)(const void*, size_t, int, int, comm_t, hipStream_t);
static int (*Recv)(void*, size_t, int, int, comm_t, hipStream_t);
static int (*GroupStart)();
static int (*GroupEnd)();
static int (*AllReduce)(const void*, void*, size_t, int, int, comm_t, hipStream_t);
static int (*AllGather)(const void*, void*, size_t, int, comm_t, hipStream_t);
static const char* (*GetErrorString)(int);
static void* handle = nullptr;

static std::mutex load_mutex;

static int load() {
  std::lock_guard<std::mutex> guard(load_mutex);
  if (handle) return LBM_OK;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char* n : names) {
    handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (handle) break;
  }
  if (!handle) return fail(LBM_ERCCL, "cannot load librccl: %s", dlerror());
#define SYM(var, name)                                                       \
  *(void**)(&var) = dlsym(handle, name);                                     \
  if (!var) return fail(LBM_ERCCL, "librccl lacks symbol %s", name);
  SYM(GetUniqueId, "ncclGetUniqueId");
  SYM(CommInitRank, "ncclCommInitRank");
  SYM(CommInitAll, "ncclCommInitAll");
  SYM(CommDestroy, "ncclCommDestroy");
  SYM(Send, "ncclSend");
  SYM(Recv, "ncclRecv");
  SYM(GroupStart, "ncclGroupStart");
  SYM(GroupEnd, "ncclGroupEnd");
  SYM(AllReduce, "ncclAllReduce");
  SYM(AllGather, "ncclAllGather");
  SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
  return LBM_OK;
}
}  // namespace rccl

#define NCCLC(call)                                                                        \
  do {                                                                                     \
    int r_ = (call);                                                                       \
    if (r_ != 0)                                                                           \
      return fail(LBM_ERCCL, "%s failed: %s (%s:%d)", #call, rccl::GetErrorString(r_), __FILE__, __LINE__); \
  } while (0)

// ----------------------------------------------------------------- context
namespace {

// A grow-only device buffer of floats (grown_room, lbm_host_slabs.inc); cap in the units of its call site
struct GrownBuf { float* p = nullptr; long cap = 0; };

struct Slab {
  int dev = 0;
  int row0 = 0, nyl = 0;       // global rows [row0, row0+nyl)
  int pitch = 0;               // floats per row
  long plane = 0;              // floats per plane
  float* lat[2] = {nullptr, nullptr};
  uint8_t* blocked = nullptr;
  uint8_t* blocked_gs = nullptr;   // blocked map of the row below the slab (global row0-1) ...
  uint8_t* blocked_gn = nullptr;   // ... and of the row above it (two-step kernel ring rows)
  // Halo buffers, nine slots of nx floats each (layout: lbm_kernels.hip.h, kHaloSlots), one pair
  // per launch parity.  One-step launches move slots 3..5 only.
  float* ghost_s[2] = {nullptr, nullptr};  // received from the south neighbour (its top rows)
  float* ghost_n[2] = {nullptr, nullptr};  // received from the north neighbour (its bottom rows)
  float* send_s[2] = {nullptr, nullptr};   // own rows 0, 1 packed for the south neighbour (RCCL / copy transports)
  float* send_n[2] = {nullptr, nullptr};   // own rows nyl-1, nyl-2 packed for the north neighbour
  float* partials[2] = {nullptr, nullptr};
  int partial_cap = 0;
  double* sums = nullptr;      // one double per step of the current run
  double* sums_host = nullptr; // pinned host copy of the same
  bool sums_direct = false;    // the kernels write the sums straight into sums_host (sums aliases it): no copy at the end of a run
  int sums_cap = 0;
  uint32_t* err_host = nullptr;  // pinned: copy of the peer-to-peer error word, fetched with the sums
  double* scratch_d = nullptr; // small double scratch (derive / reductions)
  int scratch_cap = 0;
  // sc: interior launches (and everything outside the step loop); se: edge launches, higher
  // priority, concurrent with the interior launch of the same step; sx: halo exchange
  hipStream_t sc = nullptr, se = nullptr, sx = nullptr;
  hipEvent_t ev_bnd[2] = {nullptr, nullptr}, ev_recv[2] = {nullptr, nullptr}, ev_int[2] = {nullptr, nullptr};
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
  hipEvent_t ev_march[2] = {nullptr, nullptr};   // "marching launch n of this slab has finished" (by launch parity)
  int accel_row = -1;          // local index of global row ny-2, or -1
  // Ghost bands (marching kernels under the RCCL transport): the K rows below / above the slab as the neighbours hold
  // them, received once per K steps.  band_*[i] accompanies lat[i]: [9 planes][K rows][pitch]; the obstacle bytes of
  // kBandRows rows either side are uploaded at create (row i of band_blk_s = global row row0 - kBandRows + i).
  float* band_s[2] = {nullptr, nullptr};
  float* band_n[2] = {nullptr, nullptr};
  float* band_send_s = nullptr;    // own bottom / top K rows, packed for the neighbours
  float* band_send_n = nullptr;
  uint8_t* band_blk_s = nullptr;
  uint8_t* band_blk_n = nullptr;
  int band_K = 0;              // K the float bands are sized for (0: none yet)
  rccl::comm_t comm = nullptr;
  // peer-to-peer halos (LBM_EXCHANGE_P2P): one uncached block holds ghost_s[2], ghost_n[2] and the
  // two flags the neighbours raise; the neighbours' blocks are mapped here (peer access or hipIpc)
  char* comm_block = nullptr;
  size_t halo_bytes = 0;       // one nine-slot halo buffer, rounded up to 256 B
  char* peer_s = nullptr;      // south / north neighbour's comm block as seen from this device
  char* peer_n = nullptr;
  bool peer_s_ipc = false, peer_n_ipc = false;
  uint32_t* counters = nullptr;  // device: [0] cnt_s, [16] cnt_n, [32] err (separate 64-B lines)
  // peer-to-peer marching launches read the neighbours' lattices in place: [0] = southern, [1] = northern neighbour
  const float* nb_lat[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [side][lattice 0 / 1]
  const uint8_t* nb_blocked[2] = {nullptr, nullptr};
  long nb_plane[2] = {0, 0};
  int nb_nyl[2] = {0, 0};
  void* nb_ipc[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};   // hipIpc mappings to close (rank mode)
  uint32_t cnt_s_total = 0, cnt_n_total = 0;
  // register tiles across slabs (lbm_regtile_slabs): this slab's mailboxes (uncached: the neighbours may store into them
  // over xGMI), its per-step tile sums, and the neighbours' mail areas as this device sees them ([0] south, [1] north)
  char* tmail = nullptr;
  size_t tmail_bytes = 0;
  GrownBuf rpartials;              // (cap in steps, ntiles floats each)
  char* tmail_nb[2] = {nullptr, nullptr};
  size_t tmail_nb_bytes[2] = {0, 0};
  bool tmail_nb_ipc[2] = {false, false};
  uint32_t* rabort = nullptr;      // abort word of this slab's device group (owned by the group's first slab)
  hipEvent_t ev_rt = nullptr;      // "the group's launch is over" (recorded on the first slab's stream)
  // bodies (lbm_set_bodies): the slab's blocked labelled cells with a fluid source, {column, local row, mask | label << 8};
  // on the device as {offset in a plane, word} for lbm_body_forces; the register tiles' table (lbm_regtile.hip.h, kRegForce)
  // and their per-step partials
  std::vector<int4> fcells_host;
  int2* fcells = nullptr;
  int fcells_n = 0;
  TileTable tforces;
  GrownBuf fpart;                  // (cap in floats)
  // lbm_wave's force flavour (a lattice alone; lbm_host_march.inc, wave_force_ready): the obstacle bytes with 2 on the cells
  // of fcells, those cells' indices in fcells (dense, read at counted cells only), one group's contributions [K][fcells_n][2]
  uint8_t* fmap = nullptr;
  int* fidx = nullptr;
  GrownBuf fcontrib;               // (cap in floats)
  // probes (lbm_set_probes): the slab's probes, {column, local row, index in the set}; on the device as {offset in a plane,
  // index} for lbm_probe_gather; the register tiles' table (lbm_regtile.hip.h, kRegProbe)
  std::vector<int4> pcells_host;
  int2* pcells = nullptr;
  TileTable tprobes;
  // windows (lbm_run_window): the register tiles' table of the last window this slab ran, the window wkey, laid out and fed
  // as the probes'; the probe set and its table are not touched
  TileTable twindow;
  lbm_window wkey = {0, 0, 0, 0, 0, 0};
  // the table of -1s, no words: what the kRegForce | kRegProbe flavour is handed for an observer that is not wanted
  TileTable tnone;
  // lbm_wave's probe flavours (a lattice alone; lbm_host_march.inc, wave_probe_ready): the obstacle bytes with 4 added on the
  // probes' cells (probes alone), the force map with the same (forces and probes: follows both sets), the probes' indices in
  // the set (dense, read at probe cells only)
  uint8_t* pmap = nullptr;
  uint8_t* fpmap = nullptr;
  int* pidx = nullptr;
  // lbm_run_driven on the register tiles: the schedule's (a1, a2) pairs on the device
  GrownBuf dtab;                   // (cap in steps, 2 floats each)
};

}  // namespace

struct lbm_ctx {
  lbm_param p;
  std::vector<Slab> slabs;     // slabs owned by THIS process
  int exchange = LBM_EXCHANGE_AUTO;  // resolved: 0 = none
  int cur = 0;                 // which lattice holds the current state
  bool rank_mode = false;
  int rank = 0, nranks = 1;    // position in the global ring (rank mode); else 0 / nslabs
  long tot_fluid = 0;          // non-blocked cells of the GLOBAL lattice
  int V = 1;                   // cells per thread
  long variant = 0;
  int time_block = 1;          // 2: fuse pairs of steps through LDS (lbm_sweep2) where eligible;
                               // 4: four steps per pass, row-marching (lbm_march), where eligible, then 2, then 1
  int t2_threads = 256;        // threads per tile of the two-step kernel (256 / 512 / 1024)
  int march_rows = 0;          // rows per chunk of the marching kernel (lbm_march, time_block = 4); 0 = not chosen yet
  int march_kernel = -1;       // which marching kernel runs time_block >= 4: 0 = lbm_march (one block per strip, LDS rings,
                               // K = 4, widths that are multiples of 4 from 256 up), 1 = lbm_wave (one wave per strip,
                               // register pipeline, K = 4 / 6 / 8, any width from 64 up), -1 = lbm_march where it can run
                               // (269 GLUPS at 8192^2 against 262 for lbm_wave<8>), lbm_wave elsewhere
  int wave_rows = 0;           // rows per chunk of lbm_wave; 0 = not chosen yet
  int wave_cols = 1;           // columns per lane of lbm_wave: 1 (a wave delivers 64 - 2K columns) or 2 (128 - 2K; K = 8; even widths from 128)
  int wave_capacity = 0;       // waves of lbm_wave<time_block> the device holds at once (occupancy query)
  uint32_t seq = 0;            // peer-to-peer: sequence number of the last launch group (same on all slabs)
  bool p2p_connected = false;
  bool no_comm = false;        // rank mode without RCCL: results are this rank's contribution
  bool p2p_failed = false;     // a peer-to-peer halo wait timed out: the lattice is no longer defined
  int march_slabs = -1;        // slabs of one process march too (neighbour rows read in place): -1 not decided, 0 no, 1 yes
  // engine: which kernel family lbm_run uses for a lattice alone on its GPU
  //   0 auto = the register-resident kernel (lbm_regtile) where the lattice tiles onto the CUs (the four
  //   shipped decks: 1.5-2x the streaming kernels), the streaming kernels elsewhere,
  //   1 streaming only (lbm_sweep2 / lbm_sweep / the marching kernels),
  //   3 resident in registers (lbm_regtile) or fail   (2 was the LDS-resident engine, removed in round 3)
  int engine = 0;
  int engine_last = 0;         // what the last lbm_run used: 1 streaming, 3 resident in registers
  int samples_in_kernel = 0;   // 1: the snapshots of the last lbm_run_sampled came from the register tiles
  int forces_in_kernel = 0;    // 1: the last lbm_run_forces took its sums inside the register tiles
  int forces_in_wave = 0;      // 1: the last lbm_run_forces took its per-cell contributions inside lbm_wave launches
  int mean_in_kernel = 0;      // 1: the last lbm_run_mean took its sums inside the register tiles
  int samples_in_wave = 0;     // 1: the last lbm_run_sampled took its snapshots inside lbm_wave launches
  int mean_in_wave = 0;        // 1: the last lbm_run_mean took its sums inside lbm_wave launches
  int stats_in_wave = 0;       // 1: the last lbm_run_stats took its sums inside lbm_wave launches
  long wave_launches = 0;      // lbm_wave kernels this context has launched so far, every flavour (launch_wave counts them)
  int probes_in_kernel = 0;    // 1: the last lbm_run_probes took its values inside the register tiles
  int probes_in_wave = 0;      // 1: the last lbm_run_probes took its values inside lbm_wave launches
  int window_in_kernel = 0;    // 1: the last lbm_run_window took its window inside the register tiles
  int window_in_wave = 0;      // 1: the last lbm_run_window took its window inside lbm_wave launches
  int window_stats_in_wave = 0;    // 1: the last lbm_run_window_stats took its sums inside lbm_wave launches
  int window_stats_in_kernel = 0;  // 1: ... its samples inside the register tiles (staged there, folded into the sums behind each piece)
  int window_stats_pieces = 0;     // ... and the step-loop pieces it ran (1: the whole call in one)
  int window_stats_chunk = 0;      // option: the most sample steps one register-tile piece of lbm_run_window_stats holds (0: automatic)
  int driven_in_kernel = 0;    // 1: the last lbm_run_driven ran inside the register tiles (their kRegDrive flavour)
  int driven_in_wave = 0;      // 1: the last lbm_run_driven ran its groups of K steps inside lbm_wave launches (the driven flavour)
  int driven_observed_in_kernel = 0;  // the last lbm_run_driven_observed: bits 1 forces, 2 probes, 4 means, 8 snapshots taken inside register-tile launches
  int driven_observed_in_wave = 0;    // ... bits 1 forces, 2 probes taken inside lbm_wave launches
  int driven_observed_pieces = 0;     // ... and the step-loop pieces it ran
  int observed_in_wave = 0;    // the last lbm_run_observed: bits 1 forces, 2 probes taken inside lbm_wave launches
  int observed_in_kernel = 0;  // the last lbm_run_observed: bits 1 forces, 2 probes, 4 means, 8 snapshots taken inside register-tile launches
  int observed_pieces = 0;     // ... and the step-loop pieces it ran (1: the whole call in one)
  int nbodies = 0;             // lbm_set_bodies (0: none)
  int nprobes = 0;             // lbm_set_probes (0: none)
  long obstacle_updates = 0;   // successful lbm_set_obstacles calls on this context
  long refilled_cells = 0;     // cells the last of them refilled in this process's rows (0 under LBM_REFILL_KEEP)
  // obstacle map of the local rows and one row either side (global rows keep_row0 .. keep_row0 + keep_rows - 1, taken
  // modulo ny), for the bodies' direction masks
  std::vector<uint8_t> obst_keep;
  int keep_row0 = 0, keep_rows = 0;
  // register-tile engine (engine 3), a lattice alone or the same tiling on every slab: 64 x ty tiles, nw waves of r rows
  // (ty == 0: none), nty tile rows per slab; bpc = blocks of this tiling a CU takes by the occupancy query (0 = not asked yet,
  // -1 = the query failed or the grid does not fit); the local slabs grouped by device (order[gstart[g]] .. : the slabs of
  // device group g, found at the first run).  The buffers are the slabs'.
  struct { int ty = 0, r = 0, nw = 0, ntx = 0, nty = 0, bpc = 0; std::vector<int> order, gstart; } tplan;
  int regtile_async = 1;       // lbm_regtile, R > 1: the loop's mail issued and waited for by hand (counted vmcnt), granules sent at once
                               // (0: the round-2 loop, compiler-scheduled loads and stores; R = 1 always runs that one)
  uint32_t rtag = 1;           // next unused mailbox tag (0 = never written); never goes back except when the mailboxes are cleared
  bool resident_broken = false;   // the resident kernel cannot run here (not every tile resident, set-up failed, or a run
                                  // gave up): stay with the streaming kernels
  char resident_why[160] = "";    // ... and why (lbm_last_error does not carry it: the run itself succeeds)
  bool regtile_peers = false;           // peer access between the neighbouring slabs' devices has been switched on
  lbm::RegTileArgs* rtable = nullptr;   // pinned, device-mapped: one entry per local slab, grouped by device
  lbm::RegTileArgs* rtable_dev = nullptr;
  int ncu = 0;                 // CUs of slab 0's device
  double gpu_ms = 0.0, wall_ms = 0.0;
};

// tile of the two-step kernel
constexpr int kT2X = 64, kT2Y = 16;
// rows of obstacle bytes kept either side of a slab for the ghost bands of the marching kernels (the largest K)
constexpr int kBandRows = 8;
// The window of one lbm_run_window call (WaveWants::win): as given (validated), and as lbm_wave's window flavour tests it.
struct WinPlan {
  lbm_window w;
  lbm::WaveWin wave;
};
// The constants of a step's accelerate phase (d2q9-bgk.c:230-231), the context's and a schedule's alike: the ONE expression,
// which is why a schedule of equal entries leaves lbm_run's bits.
struct AccelPair { float a1, a2; };
static inline AccelPair accel_pair(float density, float accel) { return {density * accel / 9.f, density * accel / 36.f}; }
static inline AccelPair accel_pair(const lbm_ctx* c) { return accel_pair(c->p.density, c->p.accel); }
// a schedule's pairs, (a1, a2) of step t at [2 t], [2 t + 1] (RunKind::drive)
static std::vector<float> accel_pairs(const lbm_ctx* c, const float* accel, int nsteps) {
  std::vector<float> pairs(2 * (size_t)nsteps);
  for (int t = 0; t < nsteps; ++t) {
    const AccelPair p = accel_pair(c->p.density, accel[t]);
    pairs[2 * (size_t)t] = p.a1; pairs[2 * (size_t)t + 1] = p.a2;
  }
  return pairs;
}
// The accelerate constants of one run of the step loop: the context's pair, or under a schedule (RunKind::drive; nullptr:
// none) every step's own.
struct AccelRun {
  AccelPair ctx;
  const float* drive;
  AccelPair pair(int t) const { return drive ? AccelPair{drive[2 * t], drive[2 * t + 1]} : ctx; }   // of step t (0-based) of the run
  // what the launch of step t hands its kernel: the rows a step writes carry the NEXT step's accelerate phase; behind the
  // run's last step there is none (and no entry: the context's pair, which the kernel does not apply)
  AccelPair after(int t, int nsteps) const { return t == nsteps - 1 ? ctx : pair(t + 1); }
};

// A context whose peer-to-peer halo wait timed out holds no defined lattice: every call that would step, read or write it
// refuses through here.
static int refuse_failed(const lbm_ctx* c) {
  return c->p2p_failed ? fail(LBM_EHIP, "a peer-to-peer halo wait timed out earlier: this lattice is no longer defined") : LBM_OK;
}

#include "lbm_host_slabs.inc"

// ----------------------------------------------------------------- C ABI
// The tiling lbm_regtile would use: host arithmetic only (no device is touched), so that the rule can be tested where there
// is no GPU (tests/test_abi.py).
extern "C" int lbm_plan_tiles(int nx, int rows, int slabs_per_device, int compute_units, int* tile_rows, int* rows_per_wave) {
  if (!tile_rows || !rows_per_wave) return fail(LBM_EINVAL, "NULL argument");
  int ty = 0, r = 0;
  if (!regtile_tiling_rule(nx, rows, slabs_per_device, compute_units, &ty, &r))
    return fail(LBM_EINVAL, "no register tiling: %d columns x %d rows, %d slab(s) per device, %d compute units", nx, rows, slabs_per_device, compute_units);
  *tile_rows = ty; *rows_per_wave = r;
  return LBM_OK;
}

extern "C" int lbm_device_count(int* count) {
  if (!count) return fail(LBM_EINVAL, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { (void)hipGetLastError(); n = 0; }
  *count = n;
  return LBM_OK;
}

extern "C" int lbm_rccl_unique_id(void* id128) {
  if (!id128) return fail(LBM_EINVAL, "id buffer is NULL");
  int rc = rccl::load();
  if (rc) return rc;
  rccl::unique_id id;
  NCCLC(rccl::GetUniqueId(&id));
  memcpy(id128, &id, sizeof(id));
  return LBM_OK;
}

namespace {

// Peer-to-peer: neighbour comm blocks of slabs that live in THIS process.
int p2p_connect_local(lbm_ctx* c) {
  const int ns = (int)c->slabs.size();
  for (int i = 0; i < ns; ++i) {
    Slab& s = c->slabs[i];
    Slab& so = c->slabs[(i + ns - 1) % ns];
    Slab& no = c->slabs[(i + 1) % ns];
    for (Slab* o : {&so, &no}) {
      if (o->dev == s.dev) continue;
      int can = 0;
      HIPC(hipDeviceCanAccessPeer(&can, s.dev, o->dev));
      if (!can) return fail(LBM_EHIP, "device %d cannot access device %d peer-to-peer", s.dev, o->dev);
      HIPC(hipSetDevice(s.dev));
      hipError_t e = hipDeviceEnablePeerAccess(o->dev, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
        return fail(LBM_EHIP, "hipDeviceEnablePeerAccess(%d -> %d): %s", s.dev, o->dev, hipGetErrorString(e));
      (void)hipGetLastError();
    }
    s.peer_s = so.comm_block;
    s.peer_n = no.comm_block;
    Slab* nb[2] = {&so, &no};
    for (int side = 0; side < 2; ++side) {
      s.nb_lat[side][0] = nb[side]->lat[0]; s.nb_lat[side][1] = nb[side]->lat[1];
      s.nb_blocked[side] = nb[side]->blocked; s.nb_plane[side] = nb[side]->plane; s.nb_nyl[side] = nb[side]->nyl;
    }
  }
  c->p2p_connected = true;
  return LBM_OK;
}

// Peer-to-peer, one process per GPU: map the two neighbours' comm blocks from their hipIpc handles.
int p2p_connect_ipc(lbm_ctx* c, const char* handles, int nranks) {
  if (nranks != c->nranks) return fail(LBM_EINVAL, "expected %d handles, got %d", c->nranks, nranks);
  Slab& s = c->slabs[0];
  HIPC(hipSetDevice(s.dev));
  const int south = (c->rank + nranks - 1) % nranks, north = (c->rank + 1) % nranks;
  auto open = [&](int r, char** out, bool* ipc) -> int {
    if (r == c->rank) { *out = s.comm_block; *ipc = false; return LBM_OK; }
    hipIpcMemHandle_t h;
    memcpy(&h, handles + (size_t)r * LBM_P2P_HANDLE_BYTES, sizeof(h));
    void* ptr = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(LBM_EHIP, "hipIpcOpenMemHandle(rank %d): %s", r, hipGetErrorString(e)); }
    *out = (char*)ptr; *ipc = true;
    return LBM_OK;
  };
  int rc = open(south, &s.peer_s, &s.peer_s_ipc);
  if (rc) return rc;
  if (north == south) { s.peer_n = s.peer_s; s.peer_n_ipc = false; }
  else if ((rc = open(north, &s.peer_n, &s.peer_n_ipc))) return rc;
  // the neighbours' lattices and obstacle maps, for the marching launches (their handles sit in their halo blocks)
  const int nbr[2] = {south, north};
  char* blocks[2] = {s.peer_s, s.peer_n};
  for (int side = 0; side < 2; ++side) {
    const int r = nbr[side];
    s.nb_nyl[side] = slab_rows(c->p.ny, nranks, r).nyl;
    s.nb_plane[side] = slab_plane(s.nb_nyl[side], s.pitch);
    if (r == c->rank) {
      s.nb_lat[side][0] = s.lat[0]; s.nb_lat[side][1] = s.lat[1]; s.nb_blocked[side] = s.blocked;
    } else if (side == 1 && north == south) {
      for (int i = 0; i < 3; ++i) s.nb_ipc[1][i] = s.nb_ipc[0][i];
      s.nb_lat[1][0] = s.nb_lat[0][0]; s.nb_lat[1][1] = s.nb_lat[0][1]; s.nb_blocked[1] = s.nb_blocked[0];
    } else {
      hipIpcMemHandle_t h[3];
      HIPC(hipMemcpy(h, blocks[side] + comm_layout(s).lattice_handles(), sizeof(h), hipMemcpyDeviceToHost));
      for (int i = 0; i < 3; ++i) {
        void* ptr = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&ptr, h[i], hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(LBM_EHIP, "hipIpcOpenMemHandle(lattice of rank %d): %s", r, hipGetErrorString(e)); }
        s.nb_ipc[side][i] = ptr;
      }
      s.nb_lat[side][0] = (const float*)s.nb_ipc[side][0]; s.nb_lat[side][1] = (const float*)s.nb_ipc[side][1];
      s.nb_blocked[side] = (const uint8_t*)s.nb_ipc[side][2];
    }
    // the neighbour's mail area (register tiles across slabs): a fourth handle behind the three, zero if it has none
    if (c->tplan.ty > 0 && r != c->rank) {
      if (side == 1 && north == south) { s.tmail_nb[1] = s.tmail_nb[0]; s.tmail_nb_bytes[1] = s.tmail_nb_bytes[0]; s.tmail_nb_ipc[1] = false; }
      else {
        hipIpcMemHandle_t h, zero;
        memset(&zero, 0, sizeof(zero));
        HIPC(hipMemcpy(&h, blocks[side] + comm_layout(s).mail_handle(), sizeof(h), hipMemcpyDeviceToHost));
        void* ptr = nullptr;
        if (memcmp(&h, &zero, sizeof(h)) != 0 && hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess) == hipSuccess) {
          s.tmail_nb[side] = (char*)ptr; s.tmail_nb_bytes[side] = regtile_mail_bytes(c); s.tmail_nb_ipc[side] = true;
        } else { (void)hipGetLastError(); c->tplan.ty = 0; }      // (no mail area over there, or not mappable: the streaming kernels)
      }
    }
  }
  c->p2p_connected = true;
  return LBM_OK;
}

int p2p_export(lbm_ctx* c, char* handle64) {
  Slab& s = c->slabs[0];
  if (!s.comm_block) return fail(LBM_EINVAL, "context has no peer-to-peer halo block");
  HIPC(hipSetDevice(s.dev));
  hipIpcMemHandle_t h;
  HIPC(hipIpcGetMemHandle(&h, s.comm_block));
  memcpy(handle64, &h, LBM_P2P_HANDLE_BYTES);
  return LBM_OK;
}

// What lbm_create and lbm_create_rank_ex ask alike, in the order in which they ask: the arguments every context needs ...
int create_args(const lbm_param* params, const int* obstacles, lbm_ctx** out) {
  if (!out) return fail(LBM_EINVAL, "out is NULL");
  *out = nullptr;
  const int rc = check_params(params);
  if (rc) return rc;
  if (!obstacles) return fail(LBM_EINVAL, "obstacles is NULL");
  return LBM_OK;
}
// ... behind their own checks of slabs, ranks and transport: a device at all ...
int visible_devices(int* ndev) {
  lbm_device_count(ndev);
  if (*ndev < 1) return fail(LBM_ENODEV, "no HIP device visible; this library has no CPU path");
  return LBM_OK;
}
// ... whether a ring of one trades halos with itself (tests) ...
bool exchange_forced() {
  const char* force = getenv("LBM_FORCE_EXCHANGE");
  return force && atoi(force);
}
// ... and, of a peer-to-peer context of n slabs: the rows its halo pushes need
int p2p_rows_check(const lbm_param* params, int n) {
  return params->ny / n < 2 ? fail(LBM_EINVAL, "peer-to-peer halos need at least 2 rows per slab") : LBM_OK;
}

// Every failure of a create call once the context exists: the context freed, the failure's text kept.
int create_fail(lbm_ctx* c, int rc) {
  std::string keep = g_err;
  lbm_destroy(c);
  snprintf(g_err, sizeof(g_err), "%s", keep.c_str());
  return rc;
}

}  // namespace

extern "C" int lbm_create(const lbm_param* params, const int* obstacles, const float* cells,
                          int nslabs, const int* devices, int exchange, lbm_ctx** out) {
  int rc = create_args(params, obstacles, out);
  if (rc) return rc;
  if (nslabs < 1 || nslabs > params->ny) return fail(LBM_EINVAL, "nslabs must be in [1, ny] (got %d)", nslabs);
  if (exchange < 0 || exchange > LBM_EXCHANGE_P2P) return fail(LBM_EINVAL, "unknown exchange mode %d", exchange);
  int ndev = 0;
  if ((rc = visible_devices(&ndev))) return rc;
  auto dev_of = [&](int i) { return devices ? devices[i] : i; };
  if (nslabs == 1 && !exchange_forced())
    exchange = 0;
  else if (exchange == LBM_EXCHANGE_AUTO) {
    // RCCL wants one rank per device (ncclCommInitAll rejects a repeated device): several slabs
    // on one GPU trade their halos with peer copies instead
    bool repeated = false;
    for (int i = 0; i < nslabs && !repeated; ++i)
      for (int j = 0; j < i; ++j)
        if (dev_of(i) == dev_of(j)) { repeated = true; break; }
    exchange = repeated ? LBM_EXCHANGE_COPY : LBM_EXCHANGE_RCCL;
  }
  if (exchange == LBM_EXCHANGE_P2P && (rc = p2p_rows_check(params, nslabs))) return rc;
  for (int i = 0; i < nslabs; ++i)
    if (dev_of(i) < 0 || dev_of(i) >= ndev) return fail(LBM_ENODEV, "slab %d wants HIP device %d but only %d visible", i, dev_of(i), ndev);

  lbm_ctx* c = new lbm_ctx();   // (from here on every failure goes through create_fail)
  c->p = *params;
  c->nranks = nslabs;
  c->exchange = exchange;
  c->tot_fluid = count_fluid(obstacles, (long)params->nx * params->ny);
  c->slabs.resize(nslabs);
  std::vector<int> devs(nslabs);
  for (int i = 0; i < nslabs; ++i) {
    Slab& s = c->slabs[i];
    s.dev = devs[i] = dev_of(i);
    const RowRange r = slab_rows(params->ny, nslabs, i);
    s.row0 = r.row0; s.nyl = r.nyl;
  }
  rc = finish_create(c, obstacles, cells);
  if (!rc && c->exchange == LBM_EXCHANGE_RCCL) {
    rc = rccl::load();
    if (!rc) {
      std::vector<rccl::comm_t> comms(nslabs);
      int r = rccl::CommInitAll(comms.data(), nslabs, devs.data());
      if (r != 0) rc = fail(LBM_ERCCL, "ncclCommInitAll failed: %s", rccl::GetErrorString(r));
      else for (int i = 0; i < nslabs; ++i) c->slabs[i].comm = comms[i];
    }
  }
  if (!rc && c->exchange == LBM_EXCHANGE_P2P) rc = p2p_connect_local(c);
  if (rc) return create_fail(c, rc);
  *out = c;
  return LBM_OK;
}

extern "C" int lbm_create_rank_ex(const lbm_param* params, const int* obstacles, const float* cells,
                                  int rank, int nranks, int device, const void* unique_id, int exchange,
                                  lbm_ctx** out) {
  int rc = create_args(params, obstacles, out);
  if (rc) return rc;
  if (nranks < 1 || nranks > params->ny || rank < 0 || rank >= nranks)
    return fail(LBM_EINVAL, "bad rank %d of %d (ny = %d)", rank, nranks, params->ny);
  if (exchange != LBM_EXCHANGE_RCCL && exchange != LBM_EXCHANGE_P2P)
    return fail(LBM_EINVAL, "rank contexts trade halos by RCCL or peer-to-peer (got mode %d)", exchange);
  int ndev = 0;
  if ((rc = visible_devices(&ndev))) return rc;
  if (device < 0 || device >= ndev) return fail(LBM_ENODEV, "HIP device %d not visible (%d devices)", device, ndev);
  const bool exchanging = nranks > 1 || exchange_forced();
  const bool want_p2p = exchanging && exchange == LBM_EXCHANGE_P2P;
  if (exchanging && !unique_id && !want_p2p) return fail(LBM_EINVAL, "unique_id is NULL");
  if (want_p2p && (rc = p2p_rows_check(params, nranks))) return rc;

  lbm_ctx* c = new lbm_ctx();
  c->p = *params;
  c->rank_mode = true;
  c->rank = rank;
  c->nranks = nranks;
  c->exchange = exchanging ? (want_p2p ? LBM_EXCHANGE_P2P : LBM_EXCHANGE_RCCL) : 0;
  c->no_comm = (unique_id == nullptr) && nranks > 1;
  c->tot_fluid = count_fluid(obstacles, (long)params->nx * params->ny);
  c->slabs.resize(1);
  Slab& s = c->slabs[0];
  s.dev = device;
  const RowRange rows = slab_rows(params->ny, nranks, rank);
  s.row0 = rows.row0; s.nyl = rows.nyl;
  int p2p_rc = LBM_OK;   // a failed peer-to-peer set-up is survivable when RCCL is there to fall back on
  if (want_p2p && unique_id) {
    // probe the uncached allocation first, so that a refusal does not abort the slab set-up half way
    void* probe = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipExtMallocWithFlags(&probe, 4096, hipDeviceMallocUncached) != hipSuccess) {
      (void)hipGetLastError();
      p2p_rc = fail(LBM_EHIP, "uncached device memory not available");
      c->exchange = LBM_EXCHANGE_RCCL;
    }
    if (probe) (void)hipFree(probe);
  }
  rc = finish_create(c, obstacles, cells);
  if (!rc && unique_id && (exchanging || nranks > 1)) {
    rc = rccl::load();
    if (!rc) {
      rccl::unique_id id;
      memcpy(&id, unique_id, sizeof(id));
      if (hipSetDevice(device) != hipSuccess) rc = fail(LBM_EHIP, "hipSetDevice(%d) failed", device);
      if (!rc) {
        int r = rccl::CommInitRank(&s.comm, nranks, id, rank);
        if (r != 0) rc = fail(LBM_ERCCL, "ncclCommInitRank failed: %s", rccl::GetErrorString(r));
      }
    }
  }
  if (!rc && want_p2p && unique_id) {
    // trade the hipIpc handles through the communicator; every rank learns whether ALL succeeded
    const size_t hb = LBM_P2P_HANDLE_BYTES;
    std::vector<char> all((size_t)nranks * hb, 0), mine(hb, 0);
    if (!p2p_rc && nranks > 1) p2p_rc = p2p_export(c, mine.data());
    char* d_buf = nullptr;
    if (hipMalloc((void**)&d_buf, (size_t)(nranks + 1) * hb) != hipSuccess) rc = fail(LBM_EHIP, "hipMalloc failed");
    if (!rc) {
      (void)hipMemcpy(d_buf + (size_t)nranks * hb, mine.data(), hb, hipMemcpyHostToDevice);
      int r = rccl::AllGather(d_buf + (size_t)nranks * hb, d_buf, hb, rccl::kInt8, s.comm, s.sc);
      if (r != 0) rc = fail(LBM_ERCCL, "ncclAllGather failed: %s", rccl::GetErrorString(r));
      if (!rc && hipStreamSynchronize(s.sc) != hipSuccess) rc = fail(LBM_EHIP, "handle all-gather failed");
      if (!rc) (void)hipMemcpy(all.data(), d_buf, (size_t)nranks * hb, hipMemcpyDeviceToHost);
    }
    if (!rc && !p2p_rc) p2p_rc = (nranks > 1) ? p2p_connect_ipc(c, all.data(), nranks) : p2p_connect_local(c);
    if (!rc) {  // agreement: sum of failures over all ranks -- [0] the halo blocks, [1] the mail areas of the register tiles
      // (a rank whose mail area could not be allocated or mapped must not be the only one to know: the others would launch
      // tiles that wait for its mail)
      bool tiles_ok = c->tplan.ty > 0;
      if (tiles_ok && nranks > 1) for (int side = 0; side < 2; ++side) tiles_ok = tiles_ok && s.tmail_nb[side] != nullptr;
      double both[2] = {p2p_rc ? 1.0 : 0.0, tiles_ok ? 0.0 : 1.0}, *d_f = (double*)d_buf;
      (void)hipMemcpy(d_f, both, sizeof(both), hipMemcpyHostToDevice);
      int r = rccl::AllReduce(d_f, d_f, 2, rccl::kFloat64, rccl::kSum, s.comm, s.sc);
      if (r != 0 || hipStreamSynchronize(s.sc) != hipSuccess) rc = fail(LBM_ERCCL, "peer-to-peer agreement failed");
      else (void)hipMemcpy(both, d_f, sizeof(both), hipMemcpyDeviceToHost);
      const double fails = both[0];
      if (!rc && both[1] > 0.0) c->tplan.ty = 0;       // somebody has no register tiling: nobody uses it
      if (!rc && fails > 0.0) {
        // somebody could not map a neighbour: everyone trades halos by RCCL instead
        if (getenv("LBM_VERBOSE")) fprintf(stderr, "lbm: peer-to-peer halos unavailable (%s); using RCCL\n", p2p_rc ? g_err : "another rank failed");
        slab_free_halos(s);
        c->exchange = LBM_EXCHANGE_RCCL;
        c->p2p_connected = false;
        rc = slab_alloc_halos(c, s);
        if (!rc) rc = upload_ghost_masks(c, s, obstacles);
      }
    }
    if (d_buf) (void)hipFree(d_buf);
  } else if (!rc && want_p2p && nranks == 1) {
    rc = p2p_connect_local(c);   // ring of one (LBM_FORCE_EXCHANGE)
  }
  if (rc) return create_fail(c, rc);
  *out = c;
  return LBM_OK;
}

extern "C" int lbm_create_rank(const lbm_param* params, const int* obstacles, const float* cells,
                               int rank, int nranks, int device, const void* unique_id, lbm_ctx** out) {
  const char* e = getenv("LBM_RANK_EXCHANGE");
  const int mode = (e && !strcmp(e, "p2p")) ? LBM_EXCHANGE_P2P : LBM_EXCHANGE_RCCL;
  return lbm_create_rank_ex(params, obstacles, cells, rank, nranks, device, unique_id, mode, out);
}

extern "C" int lbm_p2p_handle(lbm_ctx* c, void* handle64) {
  if (!c || !handle64) return fail(LBM_EINVAL, "NULL argument");
  if (!c->rank_mode || c->exchange != LBM_EXCHANGE_P2P) return fail(LBM_EINVAL, "not a peer-to-peer rank context");
  return p2p_export(c, (char*)handle64);
}

extern "C" int lbm_p2p_connect(lbm_ctx* c, const void* handles, int nranks) {
  if (!c || !handles) return fail(LBM_EINVAL, "NULL argument");
  if (!c->rank_mode || c->exchange != LBM_EXCHANGE_P2P) return fail(LBM_EINVAL, "not a peer-to-peer rank context");
  if (c->p2p_connected) return fail(LBM_EINVAL, "already connected");
  return p2p_connect_ipc(c, (const char*)handles, nranks);
}

extern "C" int lbm_num_slabs(const lbm_ctx* ctx) { return ctx ? (int)ctx->slabs.size() : 0; }

extern "C" int lbm_slab_rows(const lbm_ctx* ctx, int slab, int* row_begin, int* row_end) {
  if (!ctx || slab < 0 || slab >= (int)ctx->slabs.size()) return fail(LBM_EINVAL, "bad slab index");
  if (row_begin) *row_begin = ctx->slabs[slab].row0;
  if (row_end) *row_end = ctx->slabs[slab].row0 + ctx->slabs[slab].nyl;
  return LBM_OK;
}

#include "lbm_host_march.inc"

#include "lbm_host_run.inc"

static int derive_all(lbm_ctx* c, float* out4, double* speed_sum, double* mass, bool out_on_device);
static int run_steps(lbm_ctx* c, int nsteps, float* av_vels, RunKind k = RunKind());

// May a run of this context take what it wants inside lbm_wave launches?  A lattice alone, no ranks, no exchange, lbm_wave the
// engine of the groups of K steps, their partial sums fit.  Asked before anything is queued; no: the caller keeps the split
// (a forces run: the one-step) path.  (Whether a run is long enough for a group is the caller's question.)  Snapshots and
// means need no more: the field flavour reads the plain obstacle bytes.  forces_run: lbm_run_forces' own admission -- a rank
// context of one rank that trades no halos takes its forces inside lbm_wave, and keeps doing so.
static bool wave_admit(lbm_ctx* c, bool forces_run) {
  if ((c->rank_mode && !forces_run) || c->exchange != 0 || !march_eligible(c) || !use_wave_kernel(c)) return false;
  return wave_partials_fit(c);
}

// ... and probes (with_forces: forces beside them): the maps in place as well.
static bool wave_probes_admit(lbm_ctx* c, bool with_forces) {
  return wave_admit(c, false) && (!with_forces || wave_force_ready(c, c->time_block)) && wave_probe_ready(c, with_forces);
}

#include "lbm_host_observe.inc"

// The step loop of lbm_run.  k.snap (the snapshots, mean, probes and window flavours of RunKind): ONLY the register tiles
// are tried, with the snapshots (the sums, the probes, the window) in the kernel; if they did not run (the flavour's
// *_in_kernel key stays 0), nothing has been stepped and the caller runs the steps in pieces.
static int run_steps(lbm_ctx* c, int nsteps, float* av_vels, RunKind k) {
  if (nsteps == 0) { c->gpu_ms = c->wall_ms = 0.0; return LBM_OK; }
  if (int refused = refuse_failed(c)) return refused;
  const int nx = c->p.nx;
  const AccelRun acc{accel_pair(c), k.drive};
  const float a1 = acc.ctx.a1, a2 = acc.ctx.a2;
  const bool fo = k.nb > 0;   // lbm_run_forces: the register tiles only in their force flavour; lbm_wave in its force flavour where lbm_run would
                              // run it (fwave, below); else the one-step kernel, lbm_body_forces behind each step
  const bool dr = k.drive != nullptr;   // lbm_run_driven: the register tiles in their kRegDrive flavour; lbm_wave in its driven flavour on a
                                        // lattice alone (dwave, below); else the one-step kernel, each step with its own constants
                                        // (with forces or probes beside it, lbm_run_driven_observed: the driven force-and-probe flavours)
  if (!k.no_tiles && regtile_is_next(c)) {   // (a forces run that may not use the tiles says no_tiles)
    bool done = false;
    int rr = run_regtile(c, nsteps, av_vels, &done, k);
    if (rr && c->engine == 0) {
      // automatic engine: a set-up or launch failure of the register tiles (LDS attribute refused, tiles not all resident,
      // allocation failed) is not the caller's problem -- the source lattice is untouched, the streaming kernels run
      (void)hipGetLastError();
      resident_give_up(c, lbm_last_error());
      rr = LBM_OK;
    }
    if (rr) return rr;
    if (done) {
      c->engine_last = 3;
      if (k.flavour == RegFlavour::window) c->window_in_kernel = 1;
      else if (k.flavour == RegFlavour::probes || (k.flavour == RegFlavour::piece && k.snap && !k.win_table)) c->probes_in_kernel = 1;
      else if (k.flavour == RegFlavour::mean) c->mean_in_kernel = 1;
      else if (k.flavour == RegFlavour::snapshots) c->samples_in_kernel = 1;
      if (fo) c->forces_in_kernel = 1;
      if (dr) c->driven_in_kernel = 1;
      if (k.ran) *k.ran = true;
      return LBM_OK;
    }
  }
  if (k.flavour == RegFlavour::piece) return LBM_OK;   // (lbm_run_observed: nothing stepped; it runs the piece again off the tiles)
  if (c->engine >= 2 && !fo && !dr) return fail(LBM_EINVAL, "the register tiles cannot run here (%s), or this lattice has no register tiling (engine = %d)",
                                         c->resident_why[0] ? c->resident_why : "no tiling", c->engine);
  if (k.snap) return LBM_OK;
  c->engine_last = 1;
  // The halo transport: none (a lattice alone); events -- RCCL or peer copies on the exchange stream between an edge launch and
  // the interior launch, ev_bnd / ev_int / ev_recv joining the streams; or peer-to-peer -- one stream per slab, no events, no
  // host-side exchange, the hand-off in the kernels (launch group c->seq).  The launch groups below take their branch by it.
  const bool p2p = c->exchange == LBM_EXCHANGE_P2P, ev = c->exchange != 0 && !p2p;
  if (p2p && !c->p2p_connected) return fail(LBM_EINVAL, "peer-to-peer halos are not connected (lbm_p2p_connect)");
  int rc;
  // lbm_run_forces where lbm_run would run lbm_wave (a lattice alone): the groups of K steps in lbm_wave's force flavour.
  // Decided before anything is queued; maps, contributions or partials that do not fit: the one-step path, the same bits.
  const bool fwave = fo && nsteps >= c->time_block && wave_admit(c, true) && wave_force_ready(c, c->time_block);
  // lbm_run_driven likewise: the groups of K steps in lbm_wave's driven flavour on a lattice alone
  const bool dwave = dr && nsteps >= c->time_block && wave_admit(c, false);
  // (behind those groups the left-over steps go as lbm_run's do, in pairs where it takes pairs: av_vels is lbm_run's bits;
  // a driven run takes no pairs -- lbm_sweep2 has one pair of constants for its two steps)
  const bool pairs = (!fo || fwave) && !dr && t2_eligible(c) && nsteps >= 2;
  // probes and fields on an admitted context (RunKind::wave; wave_admit: a lattice alone, so under no exchange): is step s
  // (1-based) of this run a sample step of theirs
  const WaveWants& w = k.wave;
  const bool pw = w.pout != nullptr, fw = w.fout != nullptr;
  // (the field flavour is a flavour of its own: refused before anything is queued, launch_wave would refuse it mid-run)
  if (fw && (pw || fo)) return fail(LBM_EINVAL, "run_steps: fields inside lbm_wave run beside neither probes nor forces");
  if (fw && dr) return fail(LBM_EINVAL, "run_steps: fields inside lbm_wave run under no schedule");
  auto psample = [&](int s) { return w.psample(k.pfirst, s); };
  auto fsample = [&](int s) { return w.fsample(s); };
  // ... a left-over step that is a sample step: the probes' cells of the lattice just stored (stored WITHOUT the next step's
  // accelerate phase, which `then_accelerate` applies behind the gather as the prologue does, to the same bits); for fields
  // likewise, the stored lattice through the kernels of the split path, lbm_derive into the sample's slot or lbm_mean_add
  // into the sums
  auto pgather = [&](int s, bool then_accelerate) -> int {
    Slab& sl = c->slabs[0];
    HIPC(hipSetDevice(sl.dev));
    int rc;
    if (psample(s) && (rc = launch_probe_gather(c, sl, w.pout + 4 * (size_t)w.prow(k.pfirst, s) * (size_t)c->nprobes))) return rc;
    // (a window: into the sample's slot, or -- lbm_run_window_stats, one slot -- the sums over the window's cells)
    if (fsample(s) && w.win && (rc = launch_window(c, sl, w.win->w, 0, w.win->w.ny, w.fslot(s), w.fstats))) return rc;
    if (fsample(s) && w.fadd && !w.win && (rc = launch_cell_add(c, sl, w.fstats ? 8 : 4, w.fout))) return rc;
    if (fsample(s) && !w.fadd && !w.win) {
      const long ncell = (long)sl.nyl * nx;
      hipLaunchKernelGGL(lbm::lbm_derive, dim3(cdiv(ncell, lbm::kBlock)), dim3(lbm::kBlock), 0, sl.sc, sl.lat[c->cur], sl.plane, sl.pitch,
                         nx, ncell, sl.blocked, c->p.density, w.fslot(s), w.fpart, w.fmass);
      HIPC(hipGetLastError());
    }
    return then_accelerate ? launch_accelerate(c, sl, acc.pair(s).a1, acc.pair(s).a2) : LBM_OK;   // (step s + 1's phase: entry s)
  };

  for (auto& s : c->slabs)
    if ((rc = ensure_sums(s, nsteps))) return rc;

  // groups of K steps across slabs: the neighbours' rows read in place (slabs of one process under copies; peer-to-peer
  // contexts by their own rule, the same on every rank), or ghost bands under RCCL
  const bool slabs_march = !fo && !dr && ev && march_slabs_on(c) && nsteps >= slab_K(c);
  const bool p2p_march = !fo && !dr && p2p && p2p_march_on(c) && nsteps >= slab_K(c);
  const bool nb_march = slabs_march || p2p_march;
  const bool bands = !fo && !dr && ev && !slabs_march && march_bands_on(c) && nsteps >= slab_K(c);
  if (!fo && (!dr || dwave) && (nb_march || nsteps >= c->time_block) && (rc = check_march_partials(c, nb_march))) return rc;   // (before anything is queued)
  if (bands) {
    if ((rc = bands_setup(c, slab_K(c)))) return rc;
    for (auto& s : c->slabs) {
      const BandPlan b = band_plan(c, s);
      if ((long)b.K * (b.nb_e + b.nb_i) > s.partial_cap)
        return fail(LBM_EINVAL, "marching kernel: %d blocks exceed the partial-sum buffer (raise wave_rows)", b.nb_e + b.nb_i);
    }
  }

  // ---- prologue: accelerate phase of the first step
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    if ((rc = launch_accelerate(c, s, acc.pair(0).a1, acc.pair(0).a2))) return rc;
    if (slabs_march) HIPC(hipEventRecord(s.ev_march[1], s.sc));   // "launch -1": the starting lattice is in place
  }
  // halo buffers of the launches that trade halos (lbm_sweep2 / lbm_sweep on slabs), filled from the current lattice
  // as "launch par" (the launch before the first one that reads them); peer-to-peer: pushed, as a launch group of its own
  auto prime_halos = [&](int par) -> int {
    const uint32_t seq = p2p ? ++c->seq : 0;
    for (auto& s : c->slabs) {
      HIPC(hipSetDevice(s.dev));
      if (p2p) {
        const int rc = p2p_push(c, s, s.lat[c->cur], seq);
        if (rc) return rc;
        continue;
      }
      if (s.nyl >= 2)
        hipLaunchKernelGGL(lbm::lbm_pack_halos9, dim3(cdiv(nx, 256)), dim3(256), 0, s.sc,
                           s.lat[c->cur], s.plane, s.pitch, nx, s.nyl, s.send_s[par], s.send_n[par]);
      else
        hipLaunchKernelGGL(lbm::lbm_pack_halos, dim3(cdiv(nx, 256)), dim3(256), 0, s.sc,
                           s.lat[c->cur], s.plane, s.pitch, nx, s.nyl, s.send_s[par] + 3L * nx, s.send_n[par] + 3L * nx);
      HIPC(hipGetLastError());
      HIPC(hipEventRecord(s.ev_bnd[par], s.sc));   // "edge rows of launch -1 are in place"
      if (split_edge_stream(c, s)) HIPC(hipEventRecord(s.ev_int[par], s.sc));   // "interior of launch -1 is done"
    }
    if (p2p) return LBM_OK;
    return pairs ? exchange_halos(c, par, 0, lbm::kHaloSlots) : exchange_halos(c, par, 3, 3);
  };
  if (ev && !slabs_march && !bands && (rc = prime_halos(1))) return rc;
  if (bands) {
    // the ghost bands of the starting lattice, as "group -1" (parity 1 of the events)
    for (auto& s : c->slabs) {
      HIPC(hipSetDevice(s.dev));
      HIPC(hipEventRecord(s.ev_bnd[1], s.sc));
      if (split_edge_stream(c, s)) HIPC(hipEventRecord(s.ev_int[1], s.sc));
    }
    if ((rc = exchange_bands(c, 1, c->cur, slab_K(c)))) return rc;
  }

  const auto wall0 = std::chrono::steady_clock::now();
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    HIPC(hipEventRecord(s.ev_t0, s.sc));
  }

  // ---- the step loop (reference d2q9-bgk.c:180-201); no host sync inside.
  // Launch index li numbers the launch groups (K steps, a pair of steps or a single step); its parity
  // selects the halo / partial-sum buffers.
  int li = 0, tt = 0;
  // Every launch folds the partials of the one before it; behind the last group of a kind, here: its `steps` steps,
  // blocks(s) partials each (join: the edge stream first, where the group had an edge launch).
  auto fold_last = [&](int steps, bool join, auto blocks) -> int {
    const int ql = (li - 1) & 1;
    for (auto& s : c->slabs) {
      HIPC(hipSetDevice(s.dev));
      if (join && split_edge_stream(c, s)) HIPC(hipStreamWaitEvent(s.sc, s.ev_bnd[ql], 0));
      const int rc = launch_fold(s, ql, steps, blocks(s), tt - steps);
      if (rc) return rc;
    }
    return LBM_OK;
  };
  if (bands) {                                         // groups of K steps, ghost bands by RCCL once per group
    const int K = slab_K(c), ngroups = nsteps / K;
    for (int g = 0; g < ngroups; ++g, ++li, tt += K)
      if ((rc = launch_band_group(c, li, tt, tt + K < nsteps, g > 0))) return rc;
    if ((rc = fold_last(K, true, [&](const Slab& s) { const BandPlan b = band_plan(c, s); return b.nb_e + b.nb_i; }))) return rc;
  } else
  if (nb_march) {                                      // groups of K steps, row-marching, every slab of this process
    const int K = slab_K(c), ngroups = nsteps / K;
    if (p2p_march && (rc = p2p_march_open(c))) return rc;
    for (int g = 0; g < ngroups; ++g, ++li, tt += K)
      if ((rc = (p2p_march ? launch_march_p2p : launch_march_slabs)(c, li, tt, tt + K < nsteps, g > 0))) return rc;
    if ((rc = fold_last(K, false, [&](const Slab& s) { return march_slab_blocks(c, s); }))) return rc;
  } else
  if ((!fo || fwave) && (!dr || dwave) && march_eligible(c) && nsteps >= c->time_block) {   // groups of K steps, row-marching (lone slab)
    const int K = c->time_block, ngroups = nsteps / K;
    const bool wave = use_wave_kernel(c);
    for (int g = 0; g < ngroups; ++g, ++li, tt += K)
      if ((rc = wave ? launch_wave(c, li, tt, tt + K < nsteps, g > 0, k.nb, nsteps, w, wave_group(w, k.pfirst, k.drive, tt, K, nsteps))
                     : launch_march(c, li, tt, tt + K < nsteps, g > 0))) return rc;
    // what rode in those launches (forces and a schedule: admitted above, and only then do the groups run at all)
    if (fwave) c->forces_in_wave = 1;
    if (dwave) c->driven_in_wave = 1;
    if (pw && wave) c->probes_in_wave = 1;
    if (fw && wave) (w.win && w.fstats ? c->window_stats_in_wave : w.win ? c->window_in_wave : w.fstats ? c->stats_in_wave : w.fadd ? c->mean_in_wave : c->samples_in_wave) = 1;
    const int nb = wave ? wave_blocks(c) : cdiv(nx, lbm::MarchCfg<kMarchK>::WOUT) * cdiv(c->p.ny, c->march_rows);
    if ((rc = fold_last(K, false, [&](const Slab&) { return nb; }))) return rc;
  }
  if (tt < nsteps && (bands || nb_march || p2p)) {
    // the remaining steps trade halos (peer-to-peer: all of them do).  Slabs that marched: every slab's marching launches
    // must be over before a neighbour packs / copies
    if (slabs_march)
      for (auto& s : c->slabs) {
        HIPC(hipSetDevice(s.dev));
        for (auto& o : c->slabs) HIPC(hipStreamWaitEvent(s.sc, o.ev_march[(li - 1) & 1], 0));
      }
    if ((rc = prime_halos((li & 1) ^ 1))) return rc;
  }
  if (pairs && nsteps - tt >= 2) {
    const int npairs = (nsteps - tt) / 2;
    for (int j = 0; j < npairs; ++j, ++li, tt += 2) {
      const bool p1 = psample(tt + 1) || fsample(tt + 1), p2 = psample(tt + 2) || fsample(tt + 2);
      if (fo || p1) {
        // (a forces run behind its lbm_wave groups, a lattice alone; a probe, snapshot or mean run whose sample step this is)
        // the pair's first step alone into the destination lattice, for its forces, probes and fields -- its speed sums go
        // unused -- then the pair from the same source over it
        if ((rc = launch_single(c, li, tt, true, false, a1, a2))) return rc;
        if (fo && (rc = launch_forces(c, tt, li & 1, nsteps, k))) return rc;
        if (p1 && (rc = pgather(tt + 1, false))) return rc;
        c->cur ^= 1;
      }
      if ((rc = launch_pair(c, li, tt, tt + 2 < nsteps && !p2, j > 0, a1, a2))) return rc;
      if (fo && (rc = launch_forces(c, tt + 1, li & 1, nsteps, k))) return rc;
      if (p2 && (rc = pgather(tt + 2, tt + 2 < nsteps))) return rc;
    }
    if ((rc = fold_last(2, ev, [&](const Slab& s) { return t2_tiles(c, s.nyl); }))) return rc;
  }
  const int first_single = tt;
  for (; tt < nsteps; ++tt, ++li) {
    const bool ps = psample(tt + 1) || fsample(tt + 1);
    const AccelPair next = acc.after(tt, nsteps);
    if ((rc = launch_single(c, li, tt, tt == nsteps - 1 || ps, tt > first_single, next.a1, next.a2))) return rc;
    if (fo && (rc = launch_forces(c, tt, li & 1, nsteps, k))) return rc;
    if (ps && (rc = pgather(tt + 1, tt + 1 < nsteps))) return rc;
  }

  // ---- epilogue: fold the last single step's partials, collect the per-step sums
  const int ql = (li - 1) & 1;
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    if (ev && split_edge_stream(c, s)) HIPC(hipStreamWaitEvent(s.sc, s.ev_bnd[ql], 0));     // join the edge stream
    if (first_single < nsteps && (rc = launch_fold(s, ql, 1, single_partial_count(c, s), nsteps - 1))) return rc;
    HIPC(hipEventRecord(s.ev_t1, s.sc));
    if (ev) HIPC(hipStreamWaitEvent(s.sc, s.ev_recv[ql], 0));  // drain the last exchange
  }
  return collect_sums(c, nsteps, av_vels, wall0, k);
}

extern "C" int lbm_run(lbm_ctx* c, int nsteps, float* av_vels) { return lbm_run_sampled(c, nsteps, av_vels, 0, nullptr); }

extern "C" int lbm_set_accel(lbm_ctx* c, float accel) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (!std::isfinite(accel)) return fail(LBM_EINVAL, "accel is not finite");
  c->p.accel = accel;          // (every run makes its accelerate constants from c->p when it starts: nothing else to do)
  return LBM_OK;
}

// lbm_run with a per-step acceleration: the constants of every step made here, on the host, by lbm_run's
// expression; then the register tiles' kRegDrive flavour with the table on the device, lbm_wave's driven flavour on a lattice
// alone, or the one-step kernel -- run_steps decides as it does for lbm_run_forces.
extern "C" int lbm_run_driven(lbm_ctx* c, int nsteps, float* av_vels, const float* accel) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (nsteps < 0) return fail(LBM_EINVAL, "nsteps < 0");
  if (nsteps > 0 && !accel) return fail(LBM_EINVAL, "accel is NULL");
  for (int t = 0; t < nsteps; ++t)
    if (!std::isfinite(accel[t])) return fail(LBM_EINVAL, "accel[%d] is not finite", t);
  c->driven_in_kernel = 0; c->driven_in_wave = 0;
  if (nsteps == 0) return run_steps(c, 0, av_vels);
  if (int refused = refuse_failed(c)) return refused;
  const std::vector<float> pairs = accel_pairs(c, accel, nsteps);
  // ---- the register tiles need the table on the device: decided here, before anything is queued; no room, or a rank that
  // would not use the tiles: every rank takes the one-step path (the same bits), nobody fails
  bool in_kernel = regtile_is_next(c);
  if (in_kernel)
    for (auto& s : c->slabs)
      if (!drive_table_room(s, nsteps)) { in_kernel = false; break; }
  int rc;
  if ((rc = ranks_agree(c, LBM_OK, &in_kernel, "the schedule"))) return rc;
  RunKind k;
  k.drive = pairs.data(); k.no_tiles = !in_kernel;
  return run_steps(c, nsteps, av_vels, k);
}

extern "C" int lbm_last_run_ms(const lbm_ctx* c, double* gpu_ms, double* wall_ms) {
  if (!c) return fail(LBM_EINVAL, "ctx is NULL");
  if (gpu_ms) *gpu_ms = c->gpu_ms;
  if (wall_ms) *wall_ms = c->wall_ms;
  return LBM_OK;
}

extern "C" int lbm_read_state(lbm_ctx* c, float* out) {
  if (!c || !out) return fail(LBM_EINVAL, "NULL argument");
  const int nx = c->p.nx;
  const int base_row = c->rank_mode ? c->slabs[0].row0 : 0;
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    const long ncell = (long)s.nyl * nx;
    DeviceTemp t;
    HIPC(hipMalloc(&t.p, sizeof(float) * 9 * ncell));
    float* d_aos = (float*)t.p;
    hipLaunchKernelGGL(lbm::lbm_soa_to_aos, dim3(cdiv(ncell, 256)), dim3(256), 0, s.sc, s.lat[c->cur], d_aos, s.plane, s.pitch, nx, ncell);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s.sc));
    HIPC(hipMemcpy(out + 9L * (s.row0 - base_row) * nx, d_aos, sizeof(float) * 9 * ncell, hipMemcpyDeviceToHost));
  }
  return LBM_OK;
}

// Runs lbm_derive on every local slab; returns global speed sum and mass.
// out_on_device: out4 is device memory on the slabs' device (written in place, nothing copied).
static int derive_all(lbm_ctx* c, float* out4, double* speed_sum, double* mass, bool out_on_device) {
  const int nx = c->p.nx;
  const int base_row = c->rank_mode ? c->slabs[0].row0 : 0;
  double tot[2] = {0.0, 0.0};
  for (auto& s : c->slabs) {
    HIPC(hipSetDevice(s.dev));
    const long ncell = (long)s.nyl * nx;
    const int grid = cdiv(ncell, lbm::kBlock);
    DeviceTemp t;
    if (out4 && !out_on_device) HIPC(hipMalloc(&t.p, sizeof(float) * 4 * ncell));
    float* d_out = out_on_device ? out4 + 4L * (s.row0 - base_row) * nx : (float*)t.p;
    float* part = s.partials[0];  // idle between runs; capacity >= grid
    double* mpart = s.scratch_d;
    double* res = s.scratch_d + s.scratch_cap;  // 2 doubles: speed, mass
    hipLaunchKernelGGL(lbm::lbm_derive, dim3(grid), dim3(lbm::kBlock), 0, s.sc, s.lat[c->cur], s.plane, s.pitch, nx, ncell,
                       s.blocked, c->p.density, d_out, part, mpart);
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(lbm::lbm_fold_partials, dim3(1), dim3(lbm::kBlock), 0, s.sc, part, grid, res, 0);
    hipLaunchKernelGGL(lbm::lbm_fold_double, dim3(1), dim3(lbm::kBlock), 0, s.sc, mpart, grid, res + 1);
    HIPC(hipGetLastError());
    if (c->rank_mode && s.comm != nullptr)
      NCCLC(rccl::AllReduce(res, res, 2, rccl::kFloat64, rccl::kSum, s.comm, s.sc));
    HIPC(hipStreamSynchronize(s.sc));
    double h[2];
    HIPC(hipMemcpy(h, res, sizeof(h), hipMemcpyDeviceToHost));
    tot[0] += h[0]; tot[1] += h[1];
    if (out4 && !out_on_device) {
      HIPC(hipMemcpy(out4 + 4L * (s.row0 - base_row) * nx, d_out, sizeof(float) * 4 * ncell, hipMemcpyDeviceToHost));
    }
  }
  if (speed_sum) *speed_sum = tot[0];
  if (mass) *mass = tot[1];
  return LBM_OK;
}

extern "C" int lbm_av_velocity(lbm_ctx* c, float* out) {
  if (!c || !out) return fail(LBM_EINVAL, "NULL argument");
  double sp = 0.0;
  int rc = derive_all(c, nullptr, &sp, nullptr, false);
  if (rc) return rc;
  *out = (float)(sp / (double)c->tot_fluid);  // d2q9-bgk.c:2713
  return LBM_OK;
}

extern "C" int lbm_reynolds(lbm_ctx* c, float* out) {
  if (!c || !out) return fail(LBM_EINVAL, "NULL argument");
  float av = 0.f;
  int rc = lbm_av_velocity(c, &av);
  if (rc) return rc;
  const float viscosity = 1.f / 6.f * (2.f / c->p.omega - 1.f);  // d2q9-bgk.c:2895
  *out = av * c->p.reynolds_dim / viscosity;
  return LBM_OK;
}

extern "C" int lbm_total_density(lbm_ctx* c, double* out) {
  if (!c || !out) return fail(LBM_EINVAL, "NULL argument");
  return derive_all(c, nullptr, nullptr, out, false);
}

extern "C" int lbm_final_state(lbm_ctx* c, float* out) {
  if (!c || !out) return fail(LBM_EINVAL, "NULL argument");
  return derive_all(c, out, nullptr, nullptr, false);
}

extern "C" int lbm_destroy(lbm_ctx* c) {
  if (!c) return LBM_OK;
  regtile_free(c);
  for (auto& s : c->slabs) slab_free(s);
  delete c;
  return LBM_OK;
}

#include "lbm_host_live.inc"

extern "C" int lbm_timestep(const lbm_param* params, float* cells, float* tmp_cells,
                            const int* obstacles, float* av_vel) {
  if (!cells || !tmp_cells) return fail(LBM_EINVAL, "NULL lattice");
  lbm_ctx* c = nullptr;
  int rc = lbm_create(params, obstacles, cells, 1, nullptr, LBM_EXCHANGE_AUTO, &c);
  if (rc) return rc;
  float av = 0.f;
  rc = lbm_run(c, 1, &av);
  if (!rc) rc = lbm_read_state(c, tmp_cells);
  lbm_destroy(c);
  if (rc) return rc;
  // the reference mutates `cells` (accelerate, row ny-2, d2q9-bgk.c:230-260): do the same
  // host-side so that callers relying on that side effect see it
  {
    const auto [a1, a2] = accel_pair(params->density, params->accel);
    const int jj = params->ny - 2;
    for (int ii = 0; ii < params->nx; ++ii) {
      float* s = cells + 9L * (ii + (long)jj * params->nx);
      if (!obstacles[ii + jj * params->nx] && (s[3] - a1) > 0.f && (s[6] - a2) > 0.f && (s[7] - a2) > 0.f) {
        s[1] += a1; s[5] += a2; s[8] += a2; s[3] -= a1; s[6] -= a2; s[7] -= a2;
      }
    }
  }
  if (av_vel) *av_vel = av;
  return LBM_OK;
}

extern "C" int lbm_set_option(lbm_ctx* c, const char* key, long value) {
  if (!c || !key) return fail(LBM_EINVAL, "NULL argument");
  if (!strcmp(key, "vector_width")) {
    if (!(value == 1 || (value == 2 && c->p.nx % 2 == 0 && c->p.nx >= 4) || (value == 4 && c->p.nx % 4 == 0 && c->p.nx >= 8)))
      return fail(LBM_EINVAL, "vector_width %ld not usable with nx = %d", value, c->p.nx);
    c->V = (int)value;
    c->engine = 1;   // (choosing among the streaming kernels selects the streaming engine)
    return LBM_OK;
  }
  if (!strcmp(key, "t2_threads")) {
    if (value != 256 && value != 512 && value != 1024) return fail(LBM_EINVAL, "t2_threads must be 256, 512 or 1024");
    c->t2_threads = (int)value;
    c->engine = 1;
    return LBM_OK;
  }
  if (!strcmp(key, "march_rows")) {
    if (value < 1 || value > c->p.ny) return fail(LBM_EINVAL, "march_rows must be in [1, ny]");
    { const int was = c->march_rows; c->march_rows = (int)value;
      if (check_march_partials(c, march_slabs_on(c))) { c->march_rows = was; return LBM_EINVAL; } }
    return LBM_OK;
  }
  if (!strcmp(key, "march_kernel")) {
    if (value < -1 || value > 1) return fail(LBM_EINVAL, "march_kernel must be 0 (lbm_march), 1 (lbm_wave) or -1 (automatic)");
    c->march_kernel = (int)value;
    return LBM_OK;
  }
  if (!strcmp(key, "wave_rows")) {
    if (value < 1 || value > c->p.ny) return fail(LBM_EINVAL, "wave_rows must be in [1, ny]");
    { const int was = c->wave_rows; c->wave_rows = (int)value;
      if (check_march_partials(c, p2p_march_on(c) || march_slabs_on(c))) { c->wave_rows = was; return LBM_EINVAL; } }
    return LBM_OK;
  }
  if (!strcmp(key, "wave_cols")) {
    if (value != 1 && value != 2) return fail(LBM_EINVAL, "wave_cols must be 1 or 2 (columns per lane of lbm_wave)");
    if (value != c->wave_cols) { c->wave_rows = 0; c->wave_capacity = 0; }
    c->wave_cols = (int)value;
    return LBM_OK;
  }
  if (!strcmp(key, "time_block")) {
    if (value != 1 && value != 2 && value != 4 && value != 6 && value != 8) return fail(LBM_EINVAL, "time_block must be 1, 2, 4, 6 or 8");
    // (what the slabs can march depends on K, either way: a yes for K = 4 is no yes for K = 8, whose slabs need 32 rows)
    if (value != c->time_block) { c->wave_rows = 0; c->wave_capacity = 0; c->march_slabs = -1; }
    c->time_block = (int)value;
    c->engine = 1;
    return LBM_OK;
  }
  if (!strcmp(key, "engine")) {
    if (value != 0 && value != 1 && value != 3)
      return fail(LBM_EINVAL, "engine must be 0 (auto), 1 (streaming kernels) or 3 (resident in registers); 2, the LDS-resident engine, was removed");
    if (value == 3 && c->exchange != 0 && c->tplan.ty == 0)
      return fail(LBM_EINVAL, "register tiles across slabs need equal slabs that tile onto the CUs and neighbours that can store into each other's memory");
    if (value == 3 && c->exchange == 0 && (c->slabs.size() != 1 || c->tplan.ty == 0))
      return fail(LBM_EINVAL, "the resident kernel needs a lattice alone on its GPU that tiles onto the CUs");
    c->engine = (int)value;
    if (value == 3) {
      c->resident_broken = false; c->resident_why[0] = 0;
      if (c->tplan.bpc < 0) c->tplan.bpc = 0;
    }
    return LBM_OK;
  }
  if (!strcmp(key, "regtile_tag")) {      // test hook: the next mailbox tag (they only grow: tests reach the restart paths with it)
    if (value < (long)c->rtag || value >= 0x7fffff00L) return fail(LBM_EINVAL, "regtile_tag must not go back (now %u) and must stay below 2^31", c->rtag);
    c->rtag = (uint32_t)value;
    return LBM_OK;
  }
  if (!strcmp(key, "regtile_async")) {
    if (value != 0 && value != 1) return fail(LBM_EINVAL, "regtile_async must be 0 or 1");
    c->regtile_async = (int)value;
    c->tplan.bpc = c->tplan.bpc < 0 ? c->tplan.bpc : 0;     // (another instantiation: ask about its residency again)
    return LBM_OK;
  }
  if (!strcmp(key, "regtile")) {   // rows per tile * 10 + rows per wave
    const int ty = (int)(value / 10), r = (int)(value % 10);
    if (c->exchange != 0 || c->slabs.size() != 1 || !regtile_ok(c, ty, r))
      return fail(LBM_EINVAL, "register tile of %d rows, %d per wave, does not fit this lattice / device", ty, r);
    regtile_free(c);
    regtile_set(c, ty, r, c->p.ny / ty);
    return LBM_OK;
  }
  if (!strcmp(key, "window_stats_chunk")) {   // lbm_run_window_stats on the register tiles: sample steps per piece (0: automatic)
    if (value < 0 || value > 0x7fffffffL) return fail(LBM_EINVAL, "window_stats_chunk must be 0 (automatic) or a positive number of sample steps");
    c->window_stats_chunk = (int)value;
    return LBM_OK;
  }
  if (!strcmp(key, "kernel_variant")) {
    if (value < 0 || value > 15) return fail(LBM_EINVAL, "kernel_variant must be in [0, 15]");
    c->variant = value;      // (bit 3: the one-step kernel with the reference's speed sum; see t2_eligible / march_eligible / lbm_run)
    return LBM_OK;
  }
  return fail(LBM_EINVAL, "unknown option %s", key);
}

extern "C" int lbm_get_info(const lbm_ctx* c, const char* key, double* value) {
  if (!c || !key || !value) return fail(LBM_EINVAL, "NULL argument");
  // the keys that read one int of the context
  static const struct { const char* key; int lbm_ctx::*member; } plain[] = {
      {"vector_width", &lbm_ctx::V}, {"time_block", &lbm_ctx::time_block}, {"t2_threads", &lbm_ctx::t2_threads},
      {"wave_rows", &lbm_ctx::wave_rows}, {"wave_cols", &lbm_ctx::wave_cols}, {"wave_capacity", &lbm_ctx::wave_capacity},
      {"engine", &lbm_ctx::engine}, {"engine_last", &lbm_ctx::engine_last}, {"compute_units", &lbm_ctx::ncu},
      {"regtile_async", &lbm_ctx::regtile_async}, {"exchange", &lbm_ctx::exchange},
      {"samples_in_kernel", &lbm_ctx::samples_in_kernel}, {"samples_in_wave", &lbm_ctx::samples_in_wave},
      {"forces_in_kernel", &lbm_ctx::forces_in_kernel}, {"forces_in_wave", &lbm_ctx::forces_in_wave},
      {"mean_in_kernel", &lbm_ctx::mean_in_kernel}, {"mean_in_wave", &lbm_ctx::mean_in_wave},
      {"stats_in_wave", &lbm_ctx::stats_in_wave},
      {"probes_in_kernel", &lbm_ctx::probes_in_kernel}, {"probes_in_wave", &lbm_ctx::probes_in_wave},
      {"window_in_kernel", &lbm_ctx::window_in_kernel}, {"window_in_wave", &lbm_ctx::window_in_wave},
      {"window_stats_in_wave", &lbm_ctx::window_stats_in_wave}, {"window_stats_in_kernel", &lbm_ctx::window_stats_in_kernel},
      {"window_stats_pieces", &lbm_ctx::window_stats_pieces}, {"window_stats_chunk", &lbm_ctx::window_stats_chunk},
      {"driven_in_kernel", &lbm_ctx::driven_in_kernel}, {"driven_in_wave", &lbm_ctx::driven_in_wave},
      {"driven_observed_in_kernel", &lbm_ctx::driven_observed_in_kernel}, {"driven_observed_in_wave", &lbm_ctx::driven_observed_in_wave},
      {"driven_observed_pieces", &lbm_ctx::driven_observed_pieces},
      {"observed_in_kernel", &lbm_ctx::observed_in_kernel}, {"observed_in_wave", &lbm_ctx::observed_in_wave}, {"observed_pieces", &lbm_ctx::observed_pieces},
  };
  for (const auto& e : plain)
    if (!strcmp(key, e.key)) { *value = c->*e.member; return LBM_OK; }
  if (!strcmp(key, "kernel_variant")) { *value = (double)c->variant; return LBM_OK; }
  if (!strcmp(key, "time_block_active")) {
    *value = (march_eligible(c) || p2p_march_on(c) || march_bands_on(c) || march_slabs_on(const_cast<lbm_ctx*>(c)))
                 ? c->time_block : t2_eligible(c) ? 2 : 1;
    return LBM_OK;
  }
  if (!strcmp(key, "march_kernel")) { *value = ((march_eligible(c) && use_wave_kernel(c)) || (c->exchange != 0 && slab_is_wave(slab_K(c)))) ? 1 : 0; return LBM_OK; }
  if (!strcmp(key, "wave_cols_active")) { *value = wave_C(c, c->time_block); return LBM_OK; }   // what lbm_wave<time_block> would run with
  if (!strcmp(key, "wave_out_cols")) { *value = wave_out_cols(c, c->time_block); return LBM_OK; }
  if (!strcmp(key, "march_rows")) { *value = c->march_rows > 0 ? c->march_rows : march_pick_rows(c); return LBM_OK; }
  if (!strcmp(key, "fluid_cells")) { *value = (double)c->tot_fluid; return LBM_OK; }
  if (!strcmp(key, "obstacle_updates")) { *value = (double)c->obstacle_updates; return LBM_OK; }
  if (!strcmp(key, "refilled_cells")) { *value = (double)c->refilled_cells; return LBM_OK; }
  if (!strcmp(key, "wave_launches")) { *value = (double)c->wave_launches; return LBM_OK; }
  if (!strcmp(key, "accel")) { *value = (double)c->p.accel; return LBM_OK; }
  if (!strcmp(key, "engine_next")) {   // what the next lbm_run will try first
    *value = regtile_is_next(c) ? 3 : 1;
    return LBM_OK;
  }
  if (!strcmp(key, "resident_fallback")) { *value = c->resident_broken ? 1 : 0; return LBM_OK; }   // 1: the resident kernel could not run here
  if (!strcmp(key, "regtile_blocks_per_cu")) { *value = c->tplan.bpc; return LBM_OK; }   // occupancy answer (0: not asked yet)
  if (!strcmp(key, "regtile")) { *value = c->tplan.ty * 10.0 + c->tplan.r; return LBM_OK; }
  if (!strcmp(key, "regtile_tag")) { *value = c->rtag; return LBM_OK; }
  if (!strcmp(key, "pitch")) { *value = c->slabs[0].pitch; return LBM_OK; }
  if (!strcmp(key, "hbm_bytes")) {
    double b = 0;
    for (auto& s : c->slabs) b += 2.0 * 9 * 4 * (double)s.plane + (double)s.plane;
    *value = b; return LBM_OK;
  }
  return fail(LBM_EINVAL, "unknown info key %s", key);
}
