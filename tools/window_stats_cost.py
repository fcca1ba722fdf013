#!/usr/bin/env python3
"""What means and second moments over a window cost (lbm_run_window_stats) against the whole-lattice call
and against lbm_run, and whether the new code left lbm_run, lbm_run_stats and lbm_run_window where they were.  Two settings:
  1024   the shipped 1024 x 1024 deck (register tiles), 2000 steps, a 256 x 256 window from (384, 384)
  8192   the 8192 x 8192 lattice of tools/make_deck.py (lbm_wave, default options), 800 steps, a 512 x 512 window from
         (3840, 3840)
Per setting, GPU microseconds per step (lbm_last_run_ms: device events around the step loop -- of a call that runs in
pieces around each piece's, which leaves the add and fold kernels between the pieces out) and wall microseconds per step
(the clock around the call, which returns after the division and a wait for the stream: everything the call does) of
  (a) run          lbm_run                                                       this build and the parent's
  (b) stats /10    lbm_run_stats, every = 10, into a device tensor               this build and the parent's
  (c) window /10   lbm_run_window, every = 10, into a device tensor              this build and the parent's
  (d) stats /1     lbm_run_stats, every = 1 (the only way to a window's stats on the parent: then slice)
  (e) wstats /1    lbm_run_window_stats, every = 1, into a device tensor
  (f) wstats /10   every = 10
each the median over every timed run, with min .. max beside it.  Per round two child processes that differ in the library
alone: (a) .. (f) on this build, (a) .. (c) on the parent's (--parent-lib: a build of the parent commit's library); inside a
child a warm-up of each call, then the calls in turn --repeat times.  Every child runs under a time limit; the first that
fails ends the measurement.  (torch is imported first in a child: it holds the output tensors.)
Exit status 1 unless: the wall medians of (a), (b), (c) here lie within the parent's own spread (max - min) of the parent's;
(e)'s bits are (d)'s in the window's cells, from the same lattice.  The new figures carry no threshold.

    python tools/window_stats_cost.py --parent-lib path [--repeat 3] [--rounds 2] [--out profiles/window_stats_cost.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_deck import obstacle_map  # noqa: E402

SETTINGS = {1024: dict(steps=2000, win=(384, 384, 256, 256)), 8192: dict(steps=800, win=(3840, 3840, 512, 512))}
INFO = ("engine_last", "time_block_active", "stats_in_wave", "window_in_kernel", "window_in_wave", "window_stats_in_kernel",
        "window_stats_in_wave", "window_stats_pieces")
CASES = (("run", "(a) run        "), ("stats10", "(b) stats /10  "), ("window10", "(c) window /10 "), ("stats1", "(d) stats /1   "),
         ("wstats1", "(e) wstats /1  "), ("wstats10", "(f) wstats /10 "))
EVERY = {"stats10": 10, "window10": 10, "stats1": 1, "wstats1": 1, "wstats10": 10}
ON_PARENT = ("run", "stats10", "window10")


def child(n, repeat, cases):
    import torch
    sys.path.insert(0, ROOT)
    import advanced_hpc_lbm_amd as L          # (LBM_MI355X_LIB, set by the parent process, picks the build)
    if "wstats1" not in cases:                # the parent's library has no lbm_run_window_stats: the binding's set-up must not stop at it
        import ctypes

        class _Absent:
            argtypes = restype = None

        class _ParentLib(ctypes.CDLL):
            def __getattr__(self, name):
                return _Absent() if name == "lbm_run_window_stats" else super().__getattr__(name)

        L.C.CDLL = _ParentLib
    steps, win = SETTINGS[n]["steps"], L.Window(*SETTINGS[n]["win"])
    if n == 1024:
        p = L.read_params(os.path.join(ROOT, "input_1024x1024.params"))
        ob = L.read_obstacles(os.path.join(ROOT, "obstacles_1024x1024.dat"), p)
    else:
        p = L.Param(n, n, steps, 10, 0.1, 0.01, 1.85)
        ob = obstacle_map(n, n)
    stats_t = torch.empty((n, n, 8), dtype=torch.float32, device="cuda:0")
    window_t = torch.empty((steps // 10, win.ny, win.nx, 4), dtype=torch.float32, device="cuda:0")
    wstats_t = torch.empty((win.ny, win.nx, 8), dtype=torch.float32, device="cuda:0")
    times, walls, info = {c: [] for c in cases}, {c: [] for c in cases}, {}

    def call(lat, c):
        if c == "run":
            lat.run(steps)
        elif c.startswith("stats"):
            lat.run_stats(steps, EVERY[c], out=stats_t)
        elif c == "window10":
            lat.run_window(steps, 10, win, out=window_t)
        else:
            lat.run_window_stats(steps, EVERY[c], win, out=wstats_t)

    bits = None
    with L.Lattice(p, ob) as lat:
        if "wstats1" in cases:                # the bits: both calls from the lattice at rest
            call(lat, "wstats1")
            torch.cuda.synchronize()
            with L.Lattice(p, ob) as twin:
                call(twin, "stats1")
            torch.cuda.synchronize()
            cut = stats_t[win.y0:win.y0 + win.ny, win.x0:win.x0 + win.nx]
            bits = bool(torch.equal(cut.view(torch.int32), wstats_t.view(torch.int32)))
        for c in cases:                       # warm-up: every shape the timed runs use
            call(lat, c)
        for _ in range(repeat):
            for c in cases:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(lat, c)
                walls[c].append(1e6 * (time.perf_counter() - t0) / steps)
                times[c].append(1e3 * lat.last_run_ms()[0] / steps)
                for k in INFO:
                    try:
                        info[k] = int(lat.info(k))
                    except L.LbmError:        # (a key the parent's build does not know)
                        info[k] = None
    print(json.dumps({"n": n, "times": times, "walls": walls, "bits": bits, "info": info}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3, help="timed runs of each call per child")
    ap.add_argument("--rounds", type=int, default=2, help="children per build and setting (rounds x repeat >= 5 runs per figure)")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library")
    ap.add_argument("--sizes", default="1024,8192", help="the settings to run")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--cases", default=",".join(c for c, _ in CASES), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.repeat, a.cases.split(","))
    if a.rounds * a.repeat < 5:
        ap.error("need rounds x repeat >= 5")
    if not a.parent_lib:
        ap.error("--parent-lib is needed: the bars compare this build with the parent commit's")
    lines = [f"{a.rounds} processes per build and setting (alternating), {a.repeat} timed runs of each call per process; "
             "us/step: median (min .. max, n)"]
    ok = True

    def fig(v):
        return f"{statistics.median(v):10.2f} ({min(v):.2f} .. {max(v):.2f}, n = {len(v)})"

    for n in (int(s) for s in a.sizes.split(",")):
        got = {b: {"times": {}, "walls": {}, "bits": [], "info": {}} for b in ("this", "parent")}
        for _ in range(a.rounds):
            for b, cases in (("this", [c for c, _ in CASES]), ("parent", list(ON_PARENT))):
                env = dict(os.environ)
                if b == "parent":
                    env["LBM_MI355X_LIB"] = os.path.abspath(a.parent_lib)
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--repeat", str(a.repeat),
                                        "--cases", ",".join(cases)], capture_output=True, text=True, timeout=a.timeout, env=env)
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
                if x["bits"] is not None:
                    got[b]["bits"].append(x["bits"])
                got[b]["info"].update(x["info"])
        t, q = got["this"], got["parent"]
        s = SETTINGS[n]
        lines += ["", f"{n} x {n}, {s['steps']} steps, window {s['win'][2]} x {s['win'][3]} from ({s['win'][0]}, {s['win'][1]}): "
                  + ", ".join(f"{k} = {v}" for k, v in t["info"].items()),
                  f"  {'':16s}{'this build, GPU events':>40s}   {'this build, wall':>40s}   {'the parent, wall':>40s}"]
        for c, name in CASES:
            lines.append(f"  {name} {fig(t['times'][c]):>40s}   {fig(t['walls'][c]):>40s}   "
                         + (f"{fig(q['walls'][c]):>40s}" if c in q["walls"] else f"{'--':>40s}"))
        wall = {c: statistics.median(v) for c, v in t["walls"].items()}
        same = True
        for c, name in CASES[:3]:
            pm, spread = statistics.median(q["walls"][c]), max(q["walls"][c]) - min(q["walls"][c])
            inside = abs(wall[c] - pm) <= spread
            lines.append(f"  {name.split()[0]} here against the parent: wall medians differ by {abs(wall[c] - pm):.2f} us/step, "
                         f"the parent's own spread {spread:.2f}: " + ("inside" if inside else "OUTSIDE"))
            same = same and inside
        run = wall["run"]
        lines.append("  wall against (a) here: " + ", ".join(f"{name.split()[0]} {wall[c] / run:.3f} x" for c, name in CASES[1:]))
        lines.append(f"  wall added to (a): (d) {wall['stats1'] - run:.2f}, (e) {wall['wstats1'] - run:.2f}, (b) {wall['stats10'] - run:.2f}, "
                     f"(f) {wall['wstats10'] - run:.2f} us/step; (d) / (e) = {wall['stats1'] / wall['wstats1']:.2f} x, "
                     f"(b) / (f) = {wall['stats10'] / wall['wstats10']:.2f} x")
        bits = bool(t["bits"]) and all(t["bits"])
        lines.append("  the bits: (e) against (d) in the window's cells, from the same lattice: " + ("identical" if bits else "DIFFERENT"))
        ok = ok and same and bits
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
