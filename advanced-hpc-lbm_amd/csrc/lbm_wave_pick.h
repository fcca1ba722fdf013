// lbm_wave_pick.h -- what ONE launch of lbm_wave on a lattice alone runs, decided on the host: the flavour of the kernel and
// the obstacle map it reads (wave_pick), what a run wants from its groups of K steps (WaveWants), and what one group of them is
// told (WaveGroup, wave_group).  Host code only, nothing of HIP: a host compiler builds it alone (tests/wave_pick_check.cpp).
#pragma once
#include <cstddef>

// The flavours lbm_wave is instantiated in beyond SLAB (lbm_host_march.inc, wave_kernel, names each one's template flags).
enum class WaveFlavour { plain, force, probe, force_probe, field, window, driven, driven_observed, stats, window_stats };

// The obstacle bytes a launch reads: the slab's own, or with the counted cells (fmap), the probes' cells (pmap) or both
// (fpmap) marked on them (Slab; wave_force_ready and wave_probe_ready build them).
enum class WaveMap { blocked, fmap, pmap, fpmap };

struct WavePick {
  WaveFlavour flavour = WaveFlavour::plain;
  WaveMap map = WaveMap::blocked;
  bool forces = false;     // the force arguments are filled (the counted cells, their indices, the group's contributions)
  bool refused = false;    // no such launch: fields beside forces or probes, or under a schedule
};

// schedule: a per-step acceleration (lbm_run_driven).  bodies: forces are wanted (nb > 0); counted: a cell of this slab is
// counted (fcells_n > 0) -- with none the kernel that counts nothing runs and the fold writes the zeros.  probes / fields: the
// run wants them; psample / fsample: this group of K steps holds a sample step of theirs (read only beside its want);
// window: the fields are a window's (read only beside fields); stats: the fields are the eight sums of lbm_run_stats (read
// only beside fields; beside window: the eight sums over the window's cells, lbm_run_window_stats).
//   - fields are a flavour of their own: refused beside forces or probes, and under a schedule;
//   - under a schedule with an observer EVERY group runs driven_observed, a sample step in it or not, on the map that marks
//     what is wanted (an observer that is not wanted: nothing marked); under a schedule alone, driven;
//   - else a group without a sample step runs what it would run without probes or fields: field (window) > force_probe >
//     probe > force > plain.
inline WavePick wave_pick(bool schedule, bool bodies, bool counted, bool probes, bool psample, bool fields, bool fsample, bool window,
                          bool stats = false) {
  WavePick p;
  if (fields && (schedule || bodies || probes)) { p.refused = true; return p; }
  const bool f = bodies && counted;
  if (schedule && (bodies || probes)) {
    p.flavour = WaveFlavour::driven_observed;
    p.map = probes ? (f ? WaveMap::fpmap : WaveMap::pmap) : (f ? WaveMap::fmap : WaveMap::blocked);
    p.forces = f;
  } else if (schedule) p.flavour = WaveFlavour::driven;
  else if (fields && fsample) p.flavour = window ? (stats ? WaveFlavour::window_stats : WaveFlavour::window) : stats ? WaveFlavour::stats : WaveFlavour::field;
  else if (probes && psample) {
    p.flavour = f ? WaveFlavour::force_probe : WaveFlavour::probe;
    p.map = f ? WaveMap::fpmap : WaveMap::pmap;
    p.forces = f;
  } else if (f) { p.flavour = WaveFlavour::force; p.map = WaveMap::fmap; p.forces = true; }
  return p;
}

// What a run wants from its lbm_wave groups (RunKind::wave; a lattice alone that wave_admit said yes to, the register tiles
// kept off).  Steps are counted from 1 within the run.
//   probes (pout != nullptr; lbm_run_probes, lbm_run_observed): the sample steps are pfirst, pfirst + pevery, ... (pfirst:
//     RunKind's, shared with the register tiles' piece flavour); pout is the output row of the first of them, rows of
//     4 x nprobes floats.  The groups take them in lbm_wave's probe flavours; behind a left-over step that is a sample step,
//     lbm_probe_gather.
//   fields (fout != nullptr; lbm_run_sampled, lbm_run_mean, lbm_run_window): the sample steps are fevery, 2 fevery, ...; fout
//     is the first sample's field, [ny][nx][4] floats on the slab's device, fstride the floats from one sample's field to the
//     next; fadd: the samples are added into ONE field (fstride = 0), the sums of a mean; win: fout and fstride are of windows
//     and the groups run the window flavour (win->wave).  Behind a left-over step that is a sample step: lbm_derive into the
//     slot (its sums go to fpart / fmass, one float / double per block, unused), lbm_mean_add into the sums, or
//     lbm_derive_window into the slot.  fstats (lbm_run_stats; beside fadd): the ONE field is the run's
//     sums of eight floats per cell, [ny][nx][8]; the groups run the stats flavour, lbm_stats_add behind a left-over step.
//     fstats beside win (lbm_run_window_stats; fadd, fstride = 0): the ONE field is the sums over the window's cells,
//     [win.ny][win.nx][8]; the groups run the window-stats flavour, lbm_window_stats_add behind a left-over step.
struct WaveWants {
  float* pout = nullptr;
  int pevery = 0;
  float* fout = nullptr;
  int fevery = 0;
  long fstride = 0;
  bool fadd = false;
  bool fstats = false;
  float* fpart = nullptr;
  double* fmass = nullptr;
  const struct WinPlan* win = nullptr;

  bool psample(int pfirst, int s) const { return pout != nullptr && s >= pfirst && (s - pfirst) % pevery == 0; }
  int prow(int pfirst, int s) const { return (s - pfirst) / pevery; }
  bool fsample(int s) const { return fout != nullptr && s % fevery == 0; }
  float* fslot(int s) const { return fout + (size_t)(s / fevery - 1) * (size_t)fstride; }
};

// What the launch of one group, steps tt + 1 .. tt + K of the run, is told: the sample levels of its K steps (bit l - 1:
// step tt + l) with the output row / the field of the first of them, and under a schedule (drive[2 t], drive[2 t + 1]: the
// pair of step t, 0-based) the pairs its levels apply -- level l the accelerate phase of step tt + l, the run's last level none.
struct WaveGroup {
  unsigned pmask = 0u, fmask = 0u;
  int prow = 0;
  float* fout = nullptr;
  bool driven = false;
  float drv[16] = {0.f};
};
inline WaveGroup wave_group(const WaveWants& w, int pfirst, const float* drive, int tt, int K, int nsteps) {
  WaveGroup g;
  for (int l = K; l >= 1; --l) {
    if (w.psample(pfirst, tt + l)) { g.pmask |= 1u << (l - 1); g.prow = w.prow(pfirst, tt + l); }
    if (w.fsample(tt + l)) { g.fmask |= 1u << (l - 1); g.fout = w.fslot(tt + l); }
  }
  g.driven = drive != nullptr;
  for (int l = 1; drive && l <= K && tt + l < nsteps; ++l) { g.drv[2 * (l - 1)] = drive[2 * (tt + l)]; g.drv[2 * (l - 1) + 1] = drive[2 * (tt + l) + 1]; }
  return g;
}
