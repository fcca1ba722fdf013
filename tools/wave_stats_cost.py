#!/usr/bin/env python3
"""What means and second moments cost where lbm_wave runs (lbm_run_stats inside lbm_wave launches), and
whether the new flavour left lbm_run and lbm_run_mean where they were: the 8192 x 8192 and 4096 x 4096 lattices of
tools/make_deck.py, default options (what a caller gets: the info keys printed with each size say which kernel that is).

Per size, GPU microseconds per step (lbm_last_run_ms: device events around the step loop -- on the split path around each
piece's, which leaves the add kernels between the pieces out) and wall microseconds per step (the clock around the call,
which returns after the division and a wait for the stream: everything the call does) of
  (a) run            lbm_run                                                    this build and the parent's
  (b) mean /1        lbm_run_mean, every = 1, into a device tensor              this build and the parent's
  (c) stats /1       lbm_run_stats, every = 1, into a device tensor, in lbm_wave
  (d) stats /10      every = 10
  (e) stats /100     every = 100
  (f) split /1       lbm_run_stats, every = 1, forced onto the split path (engine 1, time_block 1: the one-step kernel,
  (g) split /10      lbm_stats_add behind each piece), in a context of its own
  (h) split /100
each the median over every timed run, with min .. max beside it.  Per round three child processes: (a) and (b) on this
build, (a) and (b) on the parent's (--parent-lib: a build of the parent commit's library) -- two processes that differ in
the library alone -- and (c) .. (h) on this build; inside a child a warm-up of each call, then the calls in turn --repeat
times.  Every child runs under a time limit; the first that fails ends the measurement.  (torch is imported first in a child: it holds
the output tensors.)
Exit status 1 unless: the medians of (a) and (b) here lie within the parent's own spread (max - min) of the parent's; both builds give identical bits for the
mean of (b) in every process; (c) and (f), from the same lattice, give identical bits.  The stats figures
carry no threshold: the sums are HBM traffic (derived, not measured: (c) moves about 9.6 + 64 = 74 bytes per cell and
step, (f) about 72 + 36 + 64 = 172).

    python tools/wave_stats_cost.py --parent-lib path [--steps 800] [--repeat 3] [--rounds 2] [--out profiles/wave_stats_cost.txt]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_deck import obstacle_map  # noqa: E402

SIZES = (8192, 4096)
INFO = ("engine_last", "time_block_active", "march_kernel", "wave_cols_active", "wave_rows", "mean_in_kernel", "mean_in_wave",
        "stats_in_wave")
CASES = (("run", "(a) run        "), ("mean1", "(b) mean /1    "), ("stats1", "(c) stats /1   "), ("stats10", "(d) stats /10  "),
         ("stats100", "(e) stats /100 "), ("split1", "(f) split /1   "), ("split10", "(g) split /10  "), ("split100", "(h) split /100 "))
EVERY = {"mean1": 1, "stats1": 1, "stats10": 10, "stats100": 100, "split1": 1, "split10": 10, "split100": 100}
ON_PARENT = ("run", "mean1")
SPLIT = (("engine", 1), ("time_block", 1))


def child(n, steps, repeat, cases):
    import torch
    sys.path.insert(0, ROOT)
    import numpy as np
    import advanced_hpc_lbm_amd as L          # (LBM_MI355X_LIB, set by the parent process, picks the build)
    if "stats1" not in cases:                 # the parent's library has no lbm_run_stats: the binding's set-up must not stop at it
        import ctypes

        class _Absent:
            argtypes = restype = None

        class _ParentLib(ctypes.CDLL):
            def __getattr__(self, name):
                return _Absent() if name == "lbm_run_stats" else super().__getattr__(name)

        L.C.CDLL = _ParentLib
    p = L.Param(n, n, steps, 10, 0.1, 0.01, 1.85)
    ob = obstacle_map(n, n)
    mean_t = torch.empty((n, n, 4), dtype=torch.float32, device="cuda:0")
    stats_t = torch.empty((n, n, 8), dtype=torch.float32, device="cuda:0") if any(c not in ON_PARENT for c in cases) else None
    times, walls, last, info = {c: [] for c in cases}, {c: [] for c in cases}, {}, {}

    def digest(t):
        torch.cuda.synchronize()
        return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()[:16]

    def measure(lat, mine):
        def call(c):
            if c == "run":
                lat.run(steps)
                return None
            if c == "mean1":
                lat.run_mean(steps, EVERY[c], out=mean_t)
                return mean_t
            lat.run_stats(steps, EVERY[c], out=stats_t)
            return stats_t

        # warm-up: every shape the timed window uses.  The calls both builds make come first and in one order, so that
        # they start from the same lattices on both: the output's bits are taken here
        for c in mine:
            t = call(c)
            if t is not None and c in ("mean1", "stats1", "split1"):
                last[c] = digest(t)
        for _ in range(repeat):
            for c in mine:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(c)
                walls[c].append(1e6 * (time.perf_counter() - t0) / steps)
                times[c].append(1e3 * lat.last_run_ms()[0] / steps)
                if c in ("mean1", "stats1", "split1"):
                    for k in INFO:
                        try:
                            info[("split_" if c == "split1" else "") + k] = int(lat.info(k))
                        except L.LbmError:       # (a key the parent's build does not know)
                            info[k] = None

    with L.Lattice(p, ob) as lat:
        measure(lat, [c for c in cases if not c.startswith("split")])
    split = [c for c in cases if c.startswith("split")]
    if split:
        # the split path from the lattice (c) started from: the steps both builds' calls and the stats calls before it took
        with L.Lattice(p, ob) as lat:
            for k, v in SPLIT:
                lat.set_option(k, v)
            lat.run(steps * [c for c in cases].index("stats1"))
            measure(lat, split)
    print(json.dumps({"n": n, "times": times, "walls": walls, "last": last, "info": info}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=800, help="steps per timed run (at least 200)")
    ap.add_argument("--repeat", type=int, default=3, help="timed runs of each call per child")
    ap.add_argument("--rounds", type=int, default=2, help="children per build and size (rounds x repeat >= 5 runs per figure)")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--cases", default=",".join(c for c, _ in CASES), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.repeat, a.cases.split(","))
    if a.steps < 200 or a.rounds * a.repeat < 5:
        ap.error("need at least 200 steps and rounds x repeat >= 5")
    if not a.parent_lib:
        ap.error("--parent-lib is needed: the bars compare this build with the parent commit's")
    lines = [f"{a.steps} steps per run, {a.rounds} processes per build and size (alternating), {a.repeat} timed runs of each call per process; "
             "GPU us/step: median (min .. max, n)"]
    ok = True

    def fig(v):
        return f"{statistics.median(v):10.2f} ({min(v):.2f} .. {max(v):.2f}, n = {len(v)})"

    for n in SIZES:
        got = {b: {"times": {}, "walls": {}, "last": {}, "info": {}} for b in ("this", "parent")}
        for _ in range(a.rounds):
            for b, cases in (("this", list(ON_PARENT)), ("parent", list(ON_PARENT)), ("this", [c for c, _ in CASES if c not in ON_PARENT])):
                env = dict(os.environ)
                if b == "parent":
                    env["LBM_MI355X_LIB"] = os.path.abspath(a.parent_lib)
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--steps", str(a.steps),
                                        "--repeat", str(a.repeat), "--cases", ",".join(cases)],
                                       capture_output=True, text=True, timeout=a.timeout, env=env)
                except subprocess.TimeoutExpired:
                    print(f"{n} ({b}): timed out after {a.timeout} s; stopping", file=sys.stderr)
                    return 1
                if r.returncode != 0:
                    print(f"{n} ({b}): exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                    return 1
                x = json.loads(r.stdout.strip().splitlines()[-1])
                for c, v in x["times"].items():
                    got[b]["times"].setdefault(c, []).extend(v)
                for c, v in x["walls"].items():
                    got[b]["walls"].setdefault(c, []).extend(v)
                for c, h in x["last"].items():
                    got[b]["last"].setdefault(c, set()).add(h)
                got[b]["info"].update(x["info"])
        t, q = got["this"], got["parent"]
        lines += ["", f"{n} x {n}: " + ", ".join(f"{k} = {v}" for k, v in t["info"].items()),
                  f"  {'':16s}{'this build, GPU events':>42s}   {'the parent, GPU events':>42s}   {'this build, wall':>12s}"]
        for c, name in CASES:
            lines.append(f"  {name} {fig(t['times'][c]):>42s}   " + (f"{fig(q['times'][c]):>42s}" if c in q["times"] else f"{'--':>42s}")
                         + f"   {statistics.median(t['walls'][c]):12.2f}")
        med = {b: {c: statistics.median(v) for c, v in got[b]["times"].items()} for b in got}
        same = True
        for c, name in CASES[:2]:
            spread = max(q["times"][c]) - min(q["times"][c])
            s = abs(med["this"][c] - med["parent"][c]) <= spread
            lines.append(f"  {name.split()[0]} here against the parent: medians differ by {abs(med['this'][c] - med['parent'][c]):.2f} us/step, "
                         f"the parent's own spread {spread:.2f}: " + ("inside" if s else "OUTSIDE"))
            same = same and s
        wall = {c: statistics.median(v) for c, v in t["walls"].items()}
        run, mean = wall["run"], wall["mean1"]
        lines.append("  wall against (a) here: " + ", ".join(f"{name.split()[0]} {wall[c] / run:.3f} x" for c, name in CASES[1:]))
        lines.append(f"  wall added to (a): (b) {mean - run:.2f}, (c) {wall['stats1'] - run:.2f} us/step = "
                     f"{(wall['stats1'] - run) / (mean - run) if mean > run else float('nan'):.2f} x (b)'s; "
                     f"(f) / (c) = {wall['split1'] / wall['stats1']:.2f} x, (g) / (d) = {wall['split10'] / wall['stats10']:.2f} x, "
                     f"(h) / (e) = {wall['split100'] / wall['stats100']:.2f} x")
        bits = len(t["last"]["mean1"] | q["last"]["mean1"]) == 1 and len(t["last"]["stats1"] | t["last"]["split1"]) == 1
        lines.append("  the bits: (b) in every process of both builds, (c) against (f) from the same lattice: "
                     + ("identical" if bits else "DIFFERENT"))
        ok = ok and same and bits
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
