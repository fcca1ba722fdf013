// lbm_wave.hip.h -- K time steps per pass with the time skew held in REGISTERS: every wavefront marches
// up its own 64-column strip of the lattice on its own, no LDS, no barrier, no other wave to wait for
// (reference step: /root/reference/d2q9-bgk.c:228-1813; per-cell arithmetic = collide_cell /
// accelerate_cell, so the lattice is bit-identical to K single steps).
//
// A lane owns one column.  In iteration j the wave
//     loads row  S0 + j          of the source lattice (nine aligned 256-byte row segments, prefetched one
//                                iteration ahead), which plays "level 0", and then for l = 1 .. K
//     computes step t+l on row  S0 + j - l  from what level l-1 produced in this iteration (the row
//                                above: planes 4,7,8), in the previous one (the same row: planes 0,1,3) and
//                                the one before (the row below: planes 2,5,6),
//     and stores level K's row to the destination lattice.
// What a level needs from its producer's older rows is nine registers per lane (three planes one row back,
// three planes one and two rows back); the neighbouring COLUMNS are the neighbouring lanes, one whole-wave
// DPP shift per diagonal / east / west plane (v_mov_b32_dpp wave_shr:1 / wave_shl:1).  A level is valid one
// lane less far out than its producer on either side, so a wave delivers 64 - 2K columns; rows cost 2K
// extra iterations per chunk.  HBM traffic per K updates: 36 B x 64/(64-2K) read + 36 B written = 19.3 B
// per lattice update at K = 4, 13.7 at K = 6, 10.5 at K = 8.  Everything a wave touches while it
// marches is its registers and the two lattices: waves drift apart freely, which is what overlaps one
// wave's loads with another's arithmetic (lbm_march, the LDS form of the same idea, spends a third of
// its time in the barrier that keeps its sixteen waves in step).
#pragma once
#include <type_traits>
#include "lbm_kernels.hip.h"

namespace lbm {

// The window of the window flavour (lbm_run_window), as the kernel tests it: cell (x, y) is window cell (c, r) when
// x - x0 = c sx <= xlast and y - y0 = r sy <= ylast.  c and r come from a multiply-high by mx / my = floor(2^32 / stride) + 1
// (exact while extent x stride < 2^32, which the host checks; stride 1: no multiply).  A window of one column / row is given stride 1.
struct WaveWin {
  int x0, y0, nx;              // first column, first row, cells per window row
  unsigned sx, sy, xlast, ylast, mx, my;
};

// is lattice column x a window column (q: which)?  A column left of the window wraps past xlast.
__device__ __forceinline__ bool window_col(const WaveWin& w, int x, unsigned& q) {
  const unsigned cx = (unsigned)(x - w.x0);
  q = w.sx == 1u ? cx : __umulhi(cx, w.mx);
  return cx <= w.xlast && q * w.sx == cx;
}

struct WaveArgs {
  const float* src;            // lattice at step t (accelerate phase of step t+1 already applied)
  float* dst;                  // lattice at step t+K
  long plane;
  int pitch, nx, ny;
  const uint8_t* blocked;
  Relax omega;
  int accel_row;               // global row ny-2
  int accel_out;               // apply the accelerate phase of step t+K+1 to the outputs
  float a1, a2;
  int H;                       // rows per chunk
  int y_begin, y_end;          // rows this launch covers, in chunks of H from y_begin ([0, ny): the whole lattice / slab)
  int nchunks_a;               // chunks of that range; chunks beyond it (up to nchunks) cover a SECOND range of rows --
  int yb_begin, yb_end;        // the two edge chunks of a slab, bottom and top, in one launch (nchunks_a = nchunks: no second range)
  int nwc, nchunks;            // wave columns (of 64 C - 2K output columns) x chunks = waves with work
  float* partials;             // [K][pstride]: per block, speed sums of steps t+1 .. t+K; this launch's blocks start at pbase
  int pstride, pbase;          // (one launch per group: pstride = gridDim.x, pbase = 0; a group of several launches -- the
                               // edge chunks before the ghost-row exchange, the interior chunks beside it -- shares one array)
  const float* prev;           // the previous launch's partials, folded by block 0 (or nullptr)
  int prev_count;              // its block count
  double* prev_sum;            // K doubles
  // ---- a slab with neighbours (SLAB kernels; the same protocol as lbm_march's, lbm_march.hip.h): `ny` rows are this
  // slab's, the K rows below row 0 and above row ny-1 are read straight from the neighbours' lattices; the host orders
  // the launches (launch n+1 of a slab starts after launch n of both neighbours).
  const float* src_s; const float* src_n;
  long plane_s, plane_n;
  int ny_s, ny_n;
  const uint8_t* blocked_s; const uint8_t* blocked_n;
  int acc_rows[3];             // this slab's row indices of the lattice's accelerate row and of its periodic images
  // ---- the force flavour (FORCE; a lattice alone, lbm_run_forces): `blocked` is then the slab's force map -- 0 fluid,
  // 1 blocked, 2 blocked and counted (a cell of `fcells`: labelled, with a fluid source) -- and a counted cell's lane
  // stores what body_force_cell gives for it at level l to contrib[l - 1][fidx[cell]][2] (lbm_fold_wave_forces adds them up)
  const int* fidx;             // [ny][pitch]: a counted cell's index in fcells (read at counted cells only)
  const int2* fcells;          // {offset in a plane, mask | label << 8}, as lbm_body_forces takes them
  float* contrib;              // [K][fcells_n][2]
  int fcells_n;
  // ---- the probe flavours (PROBE, alone or with FORCE; a lattice alone, lbm_run_probes / lbm_run_observed): `blocked` is
  // then the slab's probe map -- the low two bits as above (0 fluid, 1 blocked, 2 blocked and counted), plus 4 on a probe's
  // cell, blocked or not -- and at the sample levels of the pass a probe's lane stores what derive_cell gives for the cell
  // to pout + 4 * (row * nprobes + pidx[cell]): one 16-byte store, nothing to fold
  const int* pidx;             // [ny][pitch]: a probe cell's index in the set (read at probe cells only)
  float* pout;                 // [samples][nprobes][4]
  int nprobes;
  unsigned pmask;              // bit l - 1: step t + l of this pass is a sample step
  int prow;                    // the output row of the pass's first sample; a later one's: + the sample levels below it
  float density;               // what derive_cell gives a blocked cell's pressure from
  // ---- the field flavour (FIELD; a lattice alone, lbm_run_sampled / lbm_run_mean): `blocked` stays the obstacle bytes, and
  // at the sample levels of the pass EVERY delivered cell's lane takes what derive_cell gives for the cell to its place of a
  // field in lbm_derive's layout, [ny][nx][4] -- nx, not pitch
  unsigned fmask;              // bit l - 1: step t + l of this pass is a sample step
  float* fout;                 // the output base of the pass's first sample
  long fstride;                // floats between consecutive samples' outputs (snapshots: one field; sums: 0)
  int fadd;                    // 0: stored (snapshots); 1: added to what is there (the sums of lbm_run_mean)
                               // (the stats flavour, STATS: fmask as above, fout the run's ONE array of sums, [ny][nx][8]; fstride, fadd unread)
                               // (STATS beside WINDOW: fout the run's ONE array of sums over the window, [win.ny][win.nx][8])
  // ---- the window flavour (WINDOW; a lattice alone, lbm_run_window): fmask, fout and fstride as above, but a sample's
  // output is the window, [win.ny][win.nx][4], and only the window's cells are derived and stored (appended: every earlier
  // member keeps its offset)
  WaveWin win;
  // ---- the driven flavour (DRIVEN; a lattice alone, lbm_run_driven): drv[2 (l - 1)], drv[2 (l - 1) + 1] = (a1, a2) of the
  // accelerate phase that level l applies -- that of step t + l + 1 -- made on the host as a1 and a2 are; a1, a2 unused; level
  // K's pair is read only under accel_out (appended: every earlier member keeps its offset)
  float drv[16];
};

constexpr int kWaveBlock = 256;   // four independent waves per block (they only meet for the final sums)

// lane i <- lane i-1 (the column to the west) / lane i+1 (east); the wave's outermost lanes get 0,
// which only ever reaches columns the wave does not deliver
__device__ __forceinline__ float from_west(float v) {   // wave_shr:1, bound_ctrl: no source lane -> 0, no `old` register to set up
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float from_east(float v) {   // wave_shl:1
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x130, 0xf, 0xf, true));
}

// waves per SIMD the register allocation must leave room for: the loop is a chain of K dependent cell
// updates per iteration, so it is other waves, not instruction-level parallelism, that keep a SIMD busy.
// Two columns per lane (C = 2) double the registers AND the independent work per wave: two waves per SIMD then
// issue what four did (a SIMD needs two waves to issue every cycle pair, MI355X_MICROARCH.md, wave scheduling).
constexpr int wave_min_occupancy(int K, int C = 1) { return C == 2 ? 2 : (K <= 6 ? 4 : 3); }

// C = columns per lane.  C = 1: the wave covers 64 columns and delivers 64 - 2K.  C = 2: a lane owns columns
// 2 lane, 2 lane + 1 of a 128-column strip (one aligned 8-byte access per plane and row), the wave delivers 128 - 2K
// -- 112 of 128 at K = 8 instead of 48 of 64 -- and half of the east / west neighbours are the lane's own other
// column: six DPP shifts per PAIR of cells instead of twelve.  Needs K and nx even (a lane's pair never straddles the
// periodic wrap, and is delivered or dropped as a whole).
// FORCE (lbm_run_forces where lbm_wave runs; a lattice alone): after collide_cell at level l a blocked cell's p[] holds
// the populations the stored lattice of step t + l would hold (accelerate_cell leaves blocked cells alone), so
// body_force_cell on them gives, for EVERY step of the pass, the bits lbm_body_forces gets from the stored lattice.  The
// lane that owns a counted cell (own_row && out_ok: each cell exactly once per step) stores its two floats to the cell's
// slot; no accumulator, no atomic, no LDS.  "Counted" rides down the levels in a second bit field beside mreg, from the
// same byte of the map that says "blocked": no extra traffic, and a row without counted cells costs one scalar branch.
// Not offered, and left on the one-step path with lbm_body_forces behind each step: contexts where lbm_march would run,
// slabs with neighbours (the SLAB kernels, band groups, peer-to-peer marching), runs shorter than K.
// PROBE (lbm_run_probes, with FORCE lbm_run_observed's forces and probes, where lbm_wave runs; a lattice alone): after
// collide_cell at level l and BEFORE accelerate_cell, p[] of any cell, fluid or blocked, holds the populations the stored
// lattice of step t + l would hold at the end of a run -- what lbm_probe_gather hands to derive_cell.  (Behind
// accelerate_cell a fluid cell of row ny - 2 would carry the next step's accelerate phase, which a run's last lattice
// never does.)  At a sample level -- wave-uniform, a bit of pmask: a level that samples nothing costs one scalar test --
// the lane that owns a probe's cell (own_row && out_ok) stores the four floats into the probe's place of the sample's
// output row.  "Probe" rides down the levels in a third bit field, from the same map byte.
// FIELD (lbm_run_sampled / lbm_run_mean where lbm_wave runs; a lattice alone, a flavour of its own): at the same point, at a
// sample level (a bit of fmask, wave-uniform: a level that samples nothing costs one scalar test), every lane that delivers
// cells (own_row && out_ok) hands each of them to derive_cell -- the plain obstacle bit of mreg serves, no map of its own --
// and stores the four floats at 4 * (row * nx + column) of the sample's field: a snapshot (fadd = 0; one 16-byte store per
// cell, a lane's two cells 32 contiguous bytes), or an add into the sums of a mean (fadd = 1; fstride = 0: load the four
// sums, four float adds, store them back -- no contraction, lbm_mean_add's arithmetic).
// WINDOW (lbm_run_window where lbm_wave runs; a lattice alone, a flavour of its own): at the same point and on the same fmask
// levels as FIELD, but the level's row S0 + j - l is tested against the window's rows first -- wave-uniform: a row outside
// the window costs one scalar test and never reaches derive_cell -- and then each of the lane's C cells against the window's
// columns; a cell of the window goes through derive_cell with the plain obstacle bit of mreg and is stored with one 16-byte
// store at 4 * (r * win.nx + c) of the sample's window.  No map, no index array, no division (WaveWin), nothing held across
// the loop: what the test needs is recomputed at the sample level from kernel arguments.  Windows are stored, never summed.
// Why the adds come in the order of the steps, as lbm_mean_add's do: own_row and out_ok do not depend on the level, so ONE
// lane of ONE wave owns a cell at every level of a pass; it reaches levels l and l + 1 of a row in consecutive iterations,
// in program order; so the adds of one pass into a cell's sums are same-thread accesses to one address (plain loads and
// stores, not the nontemporal helpers), and the adds of different passes are ordered by the stream.
// STATS (lbm_run_stats where lbm_wave runs; a lattice alone, a flavour of its own): FIELD's levels, mask, ownership and call
// site, but a cell's record is eight floats at 8 * (row * nx + column) of the run's one array of sums, a lane's two cells 64
// contiguous bytes: the four fields are added to the first four as FIELD's fadd = 1 adds them, their products
// (stats_products: u_x^2, u_y^2, u_x u_y, (p - p0)^2) to the last four -- lbm_stats_add's arithmetic.  The first half's
// load, adds and store come before the second half's: four sums are live at a time, not eight.  The record index is 64-bit
// (2^28 cells pass 2^31 floats).  The existing FIELD kernels are not touched: no third fadd value.
// WINDOW and STATS together (lbm_run_window_stats where lbm_wave runs; a lattice alone, the one product of the two): WINDOW's
// levels, row test (wave-uniform) and per-cell column test from WaveWin -- no map, no division -- and then, for a window cell
// (c, r), what STATS does for a lattice cell, into the record at 8 * ((long)r * win.nx + c) of the run's one array of sums,
// [win.ny][win.nx][8]: load four sums, add, store, then stats_products and the second four; plain same-thread accesses,
// contraction off, the index 64-bit.  The step order holds for FIELD's reason above: one lane of one wave owns a lattice
// cell at every level of a pass, a window cell is one lattice cell, and passes follow each other on one stream.  fstride
// and fadd are unread.  The WINDOW kernels and the STATS kernels are not touched.
// DRIVEN (lbm_run_driven where lbm_wave runs; a lattice alone, a flavour of its own): level l takes its accelerate constants from
// the pass's K pairs in the kernel's arguments (scalar registers, the level is a compile-time constant of the unrolled loop)
// where every other flavour takes a1, a2; both images of the accelerate row that a chunk's fill rows may pass within a level
// take that level's pair.  Nothing else differs from the plain kernel.
// FORCE, PROBE and DRIVEN together (lbm_run_driven_observed; the one product of flavours there is): the force-and-probe flavour
// with the constants taken as DRIVEN takes them.  It serves forces alone, probes alone or both: `blocked` is then whichever
// map marks what is wanted -- the force map (no probe bit: no lane ever stores a probe, pidx is not read), the probe map (no
// counted cell: contrib and fidx are not read), the force-and-probe map, or the plain obstacle bytes, whose values 0 and 1
// are a map that marks nothing.
template <int K, int MODE, bool SLAB = false, int C = 1, bool FORCE = false, bool PROBE = false, bool FIELD = false, bool WINDOW = false,
          bool DRIVEN = false, bool STATS = false>
__global__ __launch_bounds__(kWaveBlock) __attribute__((amdgpu_waves_per_eu(wave_min_occupancy(K, C))))
void lbm_wave(const WaveArgs a) {
  constexpr bool FAST = (MODE & kFastMath) != 0, NTS = (MODE & kNtStore) != 0, NTL = (MODE & kNtLoad) != 0;
  constexpr int VW = 64 * C - 2 * K;
  static_assert(K >= 1 && K <= 12, "a wave must keep some columns");
  static_assert(C == 1 || (C == 2 && K % 2 == 0), "one or two columns per lane; pairs need an even K");
  static_assert(!(FORCE && SLAB), "the force flavour is for a lattice alone");
  static_assert(!(PROBE && SLAB), "the probe flavours are for a lattice alone");
  static_assert(!(FIELD && (SLAB || FORCE || PROBE)), "the field flavour is for a lattice alone, and a flavour of its own");
  static_assert(!(WINDOW && (SLAB || FORCE || PROBE || FIELD)), "the window flavour is for a lattice alone, and a flavour of its own");
  static_assert(!(DRIVEN && (SLAB || FORCE != PROBE || FIELD || WINDOW)), "the driven flavour is for a lattice alone: alone, or with forces and probes");
  static_assert(!DRIVEN || K <= 8, "K pairs of constants in the arguments");
  // (STATS beside WINDOW is the one product there: the window-stats flavour, lbm_run_window_stats)
  static_assert(!(STATS && (SLAB || FORCE || PROBE || FIELD || DRIVEN)), "the stats flavour is for a lattice alone: alone, or with the window");
  using fC = std::conditional_t<C == 1, float, f2a>;     // a lane's columns of one plane and row: one aligned access
  __shared__ double red_d[kWaveBlock / 64];
  __shared__ float red_f[kWaveBlock / 64][K];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

  // block 0 folds the previous launch's per-block sums (K steps) in double, fixed order
  if (blockIdx.x == 0 && a.prev != nullptr) {
    for (int l = 0; l < K; ++l) {
      double s = 0.0;
      for (int i = tid; i < a.prev_count; i += kWaveBlock) s += (double)a.prev[(long)l * a.prev_count + i];
      s = block_sum<double, kWaveBlock / 64>(s, red_d);
      if (tid == 0) a.prev_sum[l] = s;
      __syncthreads();
    }
  }

  // wave -> (wave column, chunk); the four waves of a block are neighbours in x (they share halo columns
  // through L1 / L2); blocks get an XCD-aware order so that neighbouring blocks share an L2 too
  const int nb = gridDim.x;
  int b;
  {
    const int x = blockIdx.x & 7, i = blockIdx.x >> 3, q = nb >> 3, r = nb & 7;
    b = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
  }
  const int g = b * (kWaveBlock / 64) + w;
  float sum[K];
#pragma unroll
  for (int l = 0; l < K; ++l) sum[l] = 0.f;

  if (g < a.nwc * a.nchunks) {
    const int chunk = g / a.nwc, wc = g - chunk * a.nwc;
    // rows [y_begin, y_end) of the lattice / slab in chunks of H rows (y_begin = 0, y_end = ny: all of it)
    const bool second = chunk >= a.nchunks_a;
    const int X0 = wc * VW, Y0 = second ? a.yb_begin + (chunk - a.nchunks_a) * a.H : a.y_begin + chunk * a.H;
    const int wx = min(VW, a.nx - X0), hy = min(a.H, (second ? a.yb_end : a.y_end) - Y0);
    const int S0 = Y0 - K;                      // first source row
    const int niter = hy + 2 * K;
    int gx = X0 - K + C * lane;                 // this lane's (first) column (periodic)
    gx += (gx < 0) ? a.nx : 0; gx -= (gx >= a.nx) ? a.nx : 0;
    const bool out_ok = (C * lane >= K) && (C * lane < K + wx);
    // row walk of the loads: byte offset of (row, column) inside a plane / inside the obstacle map
    int gy = S0 % a.ny; gy += (gy < 0) ? a.ny : 0;
    unsigned ld_off = ((unsigned)gy * (unsigned)a.pitch + (unsigned)gx) * 4u;
    const unsigned ld_step = (unsigned)a.pitch * 4u, ld_back = (unsigned)(a.ny - 1) * (unsigned)a.pitch * 4u;
    // ... of the stores (level K's first row is Y0; its columns never wrap)
    unsigned st_off = ((unsigned)Y0 * (unsigned)a.pitch + (unsigned)(X0 - K + C * lane)) * 4u;
    // iterations (minus the level) in which a level's row is the accelerate row: the chunk plus its fill
    // rows may pass it twice (never three times: the host keeps ny >= 2K)
    int jacc = (a.accel_row - S0) % a.ny; jacc += (jacc < 0) ? a.ny : 0;
    int jacc2 = jacc + a.ny, jacc3 = -1;
    if constexpr (SLAB) {                       // nothing wraps in y: the three images of the accelerate row, as they are
      jacc = a.acc_rows[0] - S0; jacc2 = a.acc_rows[1] - S0; jacc3 = a.acc_rows[2] - S0;
    }
    int srow = S0;                              // SLAB: the source row about to be loaded, in this slab's numbering

    // The source lattice is loaded plane by plane WHERE LEVEL 1 FIRST NEEDS IT, not row by row: for iteration j
    // planes 4,7,8 of row S0+j (pulled from the row above), planes 0,1,3 of row S0+j-1 (the row itself) and planes 2,5,6 of
    // row S0+j-2 (the row below) -- every plane of every row still exactly once, and level 1 needs no history registers
    // (nine fewer per column).  In the first two iterations the two older rows lie outside the chunk's rows: the addresses
    // are valid (periodic wrap; SLAB: clamped) and nothing uses the values (level 1 starts in iteration 2).
    auto load_row = [&](float (&f)[C][9], unsigned& blk) {
      const float *baseA = a.src, *baseB = a.src, *baseC = a.src;
      long plA = a.plane, plB = a.plane, plC = a.plane;
      const uint8_t* bl = a.blocked;
      unsigned offA, offB, offC;
      if constexpr (SLAB) {
        // rows below 0 live at the top of the southern neighbour's lattice (or of the ghost band that mirrors it), rows
        // from ny up at the bottom of the northern one's
        auto where = [&](int r, const float*& base, long& pl, const uint8_t** blp) -> unsigned {
          if (r < 0) { base = a.src_s; pl = a.plane_s; if (blp) *blp = a.blocked_s; r = max(r + a.ny_s, 0); }
          else if (r >= a.ny) { base = a.src_n; pl = a.plane_n; if (blp) *blp = a.blocked_n; r = r - a.ny; }
          return ((unsigned)r * (unsigned)a.pitch + (unsigned)gx) * 4u;
        };
        offA = where(srow, baseA, plA, &bl);
        offB = where(srow - 1, baseB, plB, nullptr);
        offC = where(srow - 2, baseC, plC, nullptr);
        ++srow;
      } else {
        offA = ld_off;
        offB = (gy == 0) ? ld_off + ld_back : ld_off - ld_step;
        offC = (gy == 0) ? ld_off + ld_back - ld_step : (gy == 1) ? ld_off - ld_step + ld_back : ld_off - 2u * ld_step;
      }
      auto ld = [&](int k, const float* base, long pl, unsigned off) {
        const fC v = ldg<NTL>(reinterpret_cast<const fC*>(reinterpret_cast<const char*>(base + k * pl) + off));
        if constexpr (C == 1) { f[0][k] = v; } else { f[0][k] = v.x; f[1][k] = v.y; }
      };
      ld(4, baseA, plA, offA); ld(7, baseA, plA, offA); ld(8, baseA, plA, offA);
      ld(0, baseB, plB, offB); ld(1, baseB, plB, offB); ld(3, baseB, plB, offB);
      ld(2, baseC, plC, offC); ld(5, baseC, plC, offC); ld(6, baseC, plC, offC);
      if constexpr (C == 1) blk = bl[offA >> 2];
      else blk = *reinterpret_cast<const uint16_t*>(bl + (offA >> 2));     // byte c = column c
      if constexpr (!SLAB) {
        ++gy;
        if (gy == a.ny) { gy = 0; ld_off -= ld_back; } else { ld_off += ld_step; }
      }
    };

    {
    // interface l (between level l and level l+1, l >= 1; level 1 pulls from the loads themselves): planes 0,1,3 of
    // the producer's previous row, planes 2,5,6 of its previous two rows  (index 0 of the arrays is never used)
    float Bp[K][C][3], C1[K][C][3], C2[K][C][3];
#pragma unroll
    for (int l = 0; l < K; ++l)
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int i = 0; i < 3; ++i) { Bp[l][c][i] = 1.f; C1[l][c][i] = 1.f; C2[l][c][i] = 1.f; }
    unsigned mreg[C];                            // bit l = obstacle flag of the row level l works on, per column
#pragma unroll
    for (int c = 0; c < C; ++c) mreg[c] = 0u;
    [[maybe_unused]] unsigned creg[C];           // FORCE: bit l = "counted" flag of the same cell
#pragma unroll
    for (int c = 0; c < C; ++c) creg[c] = 0u;
    [[maybe_unused]] unsigned preg[C];           // PROBE: bit l = "a probe sits here" flag of the same cell
#pragma unroll
    for (int c = 0; c < C; ++c) preg[c] = 0u;
    // PROBE, at a sample level behind collide_cell(s): the probes of the level's row, straight to their places
    // (l is a constant once the level loop is unrolled)
    [[maybe_unused]] auto store_probes = [&](int l, int j, const float (&p)[C][9], bool own_row, bool out_ok) {
      if (own_row && ((a.pmask >> (l - 1)) & 1u) != 0u) {       // (wave-uniform)
        bool pr[C], any = false;
#pragma unroll
        for (int c = 0; c < C; ++c) { pr[c] = out_ok && ((preg[c] >> l) & 1u) != 0u; any = any || pr[c]; }
        if (__any(any)) {
          const int cell = (S0 + j - l) * a.pitch + (X0 - K + C * lane);
          const long row = a.prow + __builtin_popcount(a.pmask & ((1u << (l - 1)) - 1u));
#pragma unroll
          for (int c = 0; c < C; ++c)
            if (pr[c]) {
              float rho;
              const f4a v = derive_cell(p[c], ((mreg[c] >> l) & 1u) != 0u, a.density, rho);
              *reinterpret_cast<f4a*>(a.pout + 4 * (row * a.nprobes + a.pidx[cell + c])) = v;
            }
        }
      }
    };
    // FIELD, at a sample level behind collide_cell(s): every delivered cell of the level's row into the sample's field
    [[maybe_unused]] auto store_fields = [&](int l, int j, const float (&p)[C][9], bool own_row, bool out_ok) {
      if (own_row && ((a.fmask >> (l - 1)) & 1u) != 0u) {       // (wave-uniform)
        if (out_ok) {                            // (row S0 + j - l in [Y0, Y0 + hy), columns X0 - K + C lane + c in [X0, X0 + wx))
#pragma clang fp contract(off)
          float* o = a.fout + (long)__builtin_popcount(a.fmask & ((1u << (l - 1)) - 1u)) * a.fstride +
                     4 * ((long)(S0 + j - l) * a.nx + (X0 - K + C * lane));
#pragma unroll
          for (int c = 0; c < C; ++c) {
            float rho;
            const f4a v = derive_cell(p[c], ((mreg[c] >> l) & 1u) != 0u, a.density, rho);
            f4a* at = reinterpret_cast<f4a*>(o + 4 * c);
            if (a.fadd != 0) add4(*at, v);       // (wave-uniform) the sums of a mean: one rounding per add, the order of the steps
            else *at = v;
          }
        }
      }
    };
    // STATS, at a sample level behind collide_cell(s): every delivered cell of the level's row into its record of the sums
    [[maybe_unused]] auto store_stats = [&](int l, int j, const float (&p)[C][9], bool own_row, bool out_ok) {
      if (own_row && ((a.fmask >> (l - 1)) & 1u) != 0u) {       // (wave-uniform)
        if (out_ok) {                            // (as store_fields: the lane's cells lie inside the chunk's rows and columns)
#pragma clang fp contract(off)
          float* o = a.fout + 8 * ((long)(S0 + j - l) * a.nx + (X0 - K + C * lane));
#pragma unroll
          for (int c = 0; c < C; ++c) {
            float rho;
            const f4a v = derive_cell(p[c], ((mreg[c] >> l) & 1u) != 0u, a.density, rho);
            f4a* at = reinterpret_cast<f4a*>(o + 8 * c);
            stats_add8(at[0], at[1], v, a.density);   // (one rounding per add, the order of the steps; plain same-thread accesses)
          }
        }
      }
    };
    // WINDOW, at a sample level behind collide_cell(s): the window's cells of the level's row into the sample's window
    [[maybe_unused]] auto store_window = [&](int l, int j, const float (&p)[C][9], bool own_row, bool out_ok) {
      if (own_row && ((a.fmask >> (l - 1)) & 1u) != 0u) {       // (wave-uniform)
        const unsigned ry = (unsigned)(S0 + j - l - a.win.y0);  // (a row below the window wraps past ylast)
        if (ry <= a.win.ylast) {                                // (wave-uniform, as is the rest of the row test)
          const unsigned r = a.win.sy == 1u ? ry : __umulhi(ry, a.win.my);
          if (r * a.win.sy == ry && out_ok) {
#pragma clang fp contract(off)
            float* o = a.fout + (long)__builtin_popcount(a.fmask & ((1u << (l - 1)) - 1u)) * a.fstride + 4 * (long)r * a.win.nx;
            unsigned q;
#pragma unroll
            for (int c = 0; c < C; ++c)
              if (window_col(a.win, X0 - K + C * lane + c, q)) {
                float rho;
                const f4a v = derive_cell(p[c], ((mreg[c] >> l) & 1u) != 0u, a.density, rho);
                *reinterpret_cast<f4a*>(o + 4 * (long)q) = v;
              }
          }
        }
      }
    };
    // WINDOW and STATS, at a sample level behind collide_cell(s): the window's cells of the level's row into their records of
    // the sums.  (The row test stands here a second time: written once, as a function beside window_col, it moves the
    // instruction text of every window flavour.)
    [[maybe_unused]] auto store_window_stats = [&](int l, int j, const float (&p)[C][9], bool own_row, bool out_ok) {
      if (own_row && ((a.fmask >> (l - 1)) & 1u) != 0u) {       // (wave-uniform)
        const unsigned ry = (unsigned)(S0 + j - l - a.win.y0);  // (a row below the window wraps past ylast)
        if (ry <= a.win.ylast) {                                // (wave-uniform, as is the rest of the row test)
          const unsigned r = a.win.sy == 1u ? ry : __umulhi(ry, a.win.my);
          if (r * a.win.sy == ry && out_ok) {
#pragma clang fp contract(off)
            unsigned q;
#pragma unroll
            for (int c = 0; c < C; ++c)
              if (window_col(a.win, X0 - K + C * lane + c, q)) {
                float rho;
                const f4a v = derive_cell(p[c], ((mreg[c] >> l) & 1u) != 0u, a.density, rho);
                f4a* at = reinterpret_cast<f4a*>(a.fout + 8 * ((long)r * a.win.nx + (long)q));
                stats_add8(at[0], at[1], v, a.density);   // (one rounding per add, the order of the steps; plain same-thread accesses)
              }
          }
        }
      }
    };
    float nxt[C][9]; unsigned nblk;
    load_row(nxt, nblk);
    // One iteration.  STEADY: past the 2K fill iterations of the chunk every level has its history, the "is this level
    // running yet" tests are gone and with them the register copies their merge points force (a quarter of the loop).
    auto iteration = [&](auto steady_c, int j) {
      constexpr bool STEADY = decltype(steady_c)::value;
      float cur[C][9];
#pragma unroll
      for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int k = 0; k < 9; ++k) cur[c][k] = nxt[c][k];
        if constexpr (PROBE) {                   // (the probe map: blocked / counted in the low two bits, 4 = a probe)
          mreg[c] = (mreg[c] << 1) | (((nblk >> (8 * c)) & 3u) != 0u ? 1u : 0u);
          if constexpr (FORCE) creg[c] = (creg[c] << 1) | (((nblk >> (8 * c)) & 3u) == 2u ? 1u : 0u);
          preg[c] = (preg[c] << 1) | ((nblk >> (8 * c + 2)) & 1u);
        } else {
          mreg[c] = (mreg[c] << 1) | (((nblk >> (8 * c)) & 0xffu) != 0u ? 1u : 0u);
          if constexpr (FORCE) creg[c] = (creg[c] << 1) | (((nblk >> (8 * c)) & 0xffu) == 2u ? 1u : 0u);
        }
      }
      if (j + 1 < niter) load_row(nxt, nblk);    // next iteration's source row, in flight behind this one's arithmetic
#pragma unroll
      for (int l = 1; l <= K; ++l) {
        float p[C][9];
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int k = 0; k < 9; ++k) p[c][k] = cur[c][k];
        if (STEADY || j >= 2 * l) {
          // pull (d2q9-bgk.c:2139-2147): row above = cur, same row = Bp, row below = C2 of interface l-1.
          // The column to the west of column c is the lane's own column c-1, or (c = 0) the last column of the lane
          // to the west: one whole-wave DPP shift; likewise to the east.
          const bool acc = ((j - l == jacc) || (j - l == jacc2) || (SLAB && j - l == jacc3)) && (l < K || a.accel_out != 0);
          const bool own_row = (j - l >= K) && (j - l < K + hy);
          const float la1 = DRIVEN ? a.drv[2 * (l - 1)] : a.a1, la2 = DRIVEN ? a.drv[2 * (l - 1) + 1] : a.a2;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const int cw = (c == 0) ? C - 1 : c - 1, ce = (c == C - 1) ? 0 : c + 1;
            // (level 1: all nine come straight from this iteration's loads, each plane from the row it is pulled from)
            const float s0 = (l == 1) ? cur[c][0] : Bp[l - 1][c][0];
            const float s1 = (l == 1) ? cur[cw][1] : Bp[l - 1][cw][1];
            const float s3 = (l == 1) ? cur[ce][3] : Bp[l - 1][ce][2];
            const float s2 = (l == 1) ? cur[c][2] : C2[l - 1][c][0];
            const float s5 = (l == 1) ? cur[cw][5] : C2[l - 1][cw][1];
            const float s6 = (l == 1) ? cur[ce][6] : C2[l - 1][ce][2];
            p[c][0] = s0;
            p[c][1] = (c == 0) ? from_west(s1) : s1;
            p[c][3] = (c == C - 1) ? from_east(s3) : s3;
            p[c][2] = s2;
            p[c][5] = (c == 0) ? from_west(s5) : s5;
            p[c][6] = (c == C - 1) ? from_east(s6) : s6;
            p[c][4] = cur[c][4];
            p[c][7] = (c == C - 1) ? from_east(cur[ce][7]) : cur[ce][7];
            p[c][8] = (c == 0) ? from_west(cur[cw][8]) : cur[cw][8];
          }
          if constexpr (C == 1) {
            const bool blk = ((mreg[0] >> l) & 1u) != 0u;
            const float sp = collide_cell<FAST>(p[0], blk, a.omega);
            if constexpr (PROBE) store_probes(l, j, p, own_row, out_ok);
            if constexpr (FIELD) store_fields(l, j, p, own_row, out_ok);
            if constexpr (WINDOW && !STATS) store_window(l, j, p, own_row, out_ok);
            if constexpr (STATS && !WINDOW) store_stats(l, j, p, own_row, out_ok);
            if constexpr (WINDOW && STATS) store_window_stats(l, j, p, own_row, out_ok);
            if (acc) accelerate_cell(p[0], blk, la1, la2);
            sum[l - 1] += (out_ok && own_row) ? sp : 0.f;
          } else {
            bool blk[C];
            float sp[C];
#pragma unroll
            for (int c = 0; c < C; ++c) blk[c] = ((mreg[c] >> l) & 1u) != 0u;
            collide_cells<FAST, C>(p, blk, a.omega, sp);      // the lane's cells statement by statement: independent chains
            if constexpr (PROBE) store_probes(l, j, p, own_row, out_ok);
            if constexpr (FIELD) store_fields(l, j, p, own_row, out_ok);
            if constexpr (WINDOW && !STATS) store_window(l, j, p, own_row, out_ok);
            if constexpr (STATS && !WINDOW) store_stats(l, j, p, own_row, out_ok);
            if constexpr (WINDOW && STATS) store_window_stats(l, j, p, own_row, out_ok);
#pragma unroll
            for (int c = 0; c < C; ++c)
              if (acc) accelerate_cell(p[c], blk[c], la1, la2);
            // (the K sums stay in registers: as lane-private LDS words -- read, add, write per level -- they cost the two-column
            // kernel 12 % at K = 8 and 18 % at K = 6, more than the eight dwords the K = 8 loop spills without them)
#pragma unroll
            for (int c = 0; c < C; ++c) sum[l - 1] += (out_ok && own_row) ? sp[c] : 0.f;
          }
          if constexpr (FORCE) {
            if (own_row) {                       // (wave-uniform; the row is Y0 + j - l - K, its columns do not wrap)
              bool cnt[C], any = false;
#pragma unroll
              for (int c = 0; c < C; ++c) { cnt[c] = out_ok && ((creg[c] >> l) & 1u) != 0u; any = any || cnt[c]; }
              if (__any(any)) {
                const int cell = (S0 + j - l) * a.pitch + (X0 - K + C * lane);
#pragma unroll
                for (int c = 0; c < C; ++c)
                  if (cnt[c]) {
                    const int jc = a.fidx[cell + c];
                    float fx, fy;
                    body_force_cell(p[c], (uint32_t)a.fcells[jc].y, fx, fy);
                    *reinterpret_cast<float2*>(a.contrib + ((long)(l - 1) * a.fcells_n + jc) * 2) = make_float2(fx, fy);
                  }
              }
            }
          }
        }
        if (l >= 2 && (STEADY || j >= 2 * (l - 1))) {   // the producer's row of this iteration becomes history for the next two
#pragma unroll
          for (int c = 0; c < C; ++c) {
            C2[l - 1][c][0] = C1[l - 1][c][0]; C2[l - 1][c][1] = C1[l - 1][c][1]; C2[l - 1][c][2] = C1[l - 1][c][2];
            C1[l - 1][c][0] = cur[c][2]; C1[l - 1][c][1] = cur[c][5]; C1[l - 1][c][2] = cur[c][6];
            Bp[l - 1][c][0] = cur[c][0]; Bp[l - 1][c][1] = cur[c][1]; Bp[l - 1][c][2] = cur[c][3];
          }
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int k = 0; k < 9; ++k) cur[c][k] = p[c][k];
      }
      if (STEADY || j >= 2 * K) {                // level K's row S0 + j - K = Y0 + (j - 2K)
        if (out_ok) {
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            fC v;
            if constexpr (C == 1) { v = cur[0][k]; } else { v.x = cur[0][k]; v.y = cur[1][k]; }
            stg<NTS>(reinterpret_cast<fC*>(reinterpret_cast<char*>(a.dst + k * a.plane) + st_off), v);
          }
        }
        st_off += ld_step;
      }
    };
    int j = 0;
    for (; j < 2 * K && j < niter; ++j) iteration(std::false_type{}, j);
    for (; j < niter; ++j) iteration(std::true_type{}, j);
    }
  }

  // per level: block sum of the speeds -> partials[level][block]
#pragma unroll
  for (int l = 0; l < K; ++l) {
    const float s = wave_sum(sum[l]);
    if (lane == 0) red_f[w][l] = s;
  }
  __syncthreads();
  if (tid < K) a.partials[(long)tid * a.pstride + a.pbase + blockIdx.x] = red_f[0][tid] + red_f[1][tid] + red_f[2][tid] + red_f[3][tid];
}

}  // namespace lbm
