// Stand-alone check program of csrc/lbm_wave_pick.h (tests/test_wave_pick.py builds and runs it; nothing else is included).
//   wave_pick_check pick       one line per combination of wave_pick's eight boolean inputs, 256 in all:
//                              schedule bodies counted probes psample fields fsample window : flavour map forces refused
//   wave_pick_check groups     reads "K nsteps pevery pfirst fevery fstride driven" lines from stdin (pevery / fevery 0: no
//                              probes / fields; driven 0: no schedule); per case one line per group of K steps:
//                              tt pmask prow fmask fslot drv[0] .. drv[2K-1] driven, where fslot is the first field sample's
//                              offset in floats from the output (-1: none) and the schedule is (t + 0.25, -t - 0.5) for step t
#include <cstdio>
#include <cstring>
#include <vector>

#include "lbm_wave_pick.h"

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "pick")) {
    for (int v = 0; v < 256; ++v) {
      bool b[8];
      for (int i = 0; i < 8; ++i) b[i] = ((v >> (7 - i)) & 1) != 0;
      const WavePick p = wave_pick(b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7]);
      for (int i = 0; i < 8; ++i) printf("%d ", b[i] ? 1 : 0);
      printf(": %d %d %d %d\n", (int)p.flavour, (int)p.map, p.forces ? 1 : 0, p.refused ? 1 : 0);
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "groups")) {
    int K, nsteps, pevery, pfirst, fevery, driven;
    long fstride;
    while (scanf("%d %d %d %d %d %ld %d", &K, &nsteps, &pevery, &pfirst, &fevery, &fstride, &driven) == 7) {
      // (the outputs: addresses only, nothing is stored; the fields' as long as its samples)
      std::vector<float> drive(2 * (size_t)nsteps), pout(1), fout(fevery > 0 ? (size_t)(nsteps / fevery) * fstride + 1 : 1);
      for (int t = 0; t < nsteps; ++t) { drive[2 * t] = t + 0.25f; drive[2 * t + 1] = -t - 0.5f; }
      WaveWants w;
      if (pevery > 0) { w.pout = pout.data(); w.pevery = pevery; }
      if (fevery > 0) { w.fout = fout.data(); w.fevery = fevery; w.fstride = fstride; }
      for (int tt = 0; tt + K <= nsteps; tt += K) {
        const WaveGroup g = wave_group(w, pfirst, driven ? drive.data() : nullptr, tt, K, nsteps);
        printf("%d %u %d %u %ld", tt, g.pmask, g.prow, g.fmask, g.fout ? (long)(g.fout - w.fout) : -1L);
        for (int i = 0; i < 2 * K; ++i) printf(" %g", g.drv[i]);
        for (int i = 2 * K; i < 16; ++i) if (g.drv[i] != 0.f) return 2;   // (levels beyond K: never set)
        printf(" %d\n", g.driven ? 1 : 0);
      }
      printf("end\n");
    }
    return 0;
  }
  fprintf(stderr, "usage: wave_pick_check pick | groups\n");
  return 1;
}
