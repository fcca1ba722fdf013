#!/usr/bin/env python3
"""What a time average or a snapshot series costs where lbm_wave runs (lbm_run_mean / lbm_run_sampled inside lbm_wave
launches): the 8192 x 8192 and 4096 x 4096 lattices of tools/make_deck.py, default options (what a caller
gets: the info keys printed with each size say which kernel that is).

Per size, GPU microseconds per step (lbm_last_run_ms: device events around the step loop, add and derive kernels included) of
  (a) run            lbm_run                                                    this build and the parent's
  (b) mean /1        lbm_run_mean, every = 1, into a device tensor              this build and the parent's
  (c) mean /10       every = 10                                                 this build and the parent's
  (d) mean /100      every = 100                                                this build and the parent's
  (e) sampled /200   lbm_run_sampled, every = 200, into a device tensor (steps // 200 snapshots)
each the median over every timed run, with min .. max beside it.  One child process per build and round, this build and
the parent's (--parent-lib: a build of the parent commit's library) alternating; inside a child a warm-up of each call,
then the calls in turn --repeat times (the calls both builds make first, in one order: the same lattices on both).  Every
child runs under a time limit; the first that fails ends the measurement.  (torch is imported first in a child: it holds
the output tensors.)
Exit status 1 unless: (a) here lies inside its own spread of the parent's (a); the slowest (b) and (c) here are faster than
the parent's fastest; both builds give identical bits for the mean of (b), (c) and (d) in every process.

    python tools/wave_fields_cost.py --parent-lib path [--steps 800] [--repeat 3] [--rounds 2] [--out profiles/wave_fields_cost.txt]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_deck import obstacle_map  # noqa: E402

SIZES = (8192, 4096)
INFO = ("engine_last", "time_block_active", "march_kernel", "wave_cols_active", "wave_rows", "mean_in_kernel", "mean_in_wave",
        "samples_in_kernel", "samples_in_wave")
CASES = (("run", "(a) run          "), ("mean1", "(b) mean /1      "), ("mean10", "(c) mean /10     "),
         ("mean100", "(d) mean /100    "), ("snap200", "(e) sampled /200 "))
EVERY = {"mean1": 1, "mean10": 10, "mean100": 100, "snap200": 200}
ON_PARENT = ("run", "mean1", "mean10", "mean100")


def child(n, steps, repeat, cases):
    import torch
    sys.path.insert(0, ROOT)
    import numpy as np
    import advanced_hpc_lbm_amd as L          # (LBM_MI355X_LIB, set by the parent process, picks the build)
    p = L.Param(n, n, steps, 10, 0.1, 0.01, 1.85)
    ob = obstacle_map(n, n)
    mean_t = torch.empty((n, n, 4), dtype=torch.float32, device="cuda:0")
    snap_t = torch.empty((steps // EVERY["snap200"], n, n, 4), dtype=torch.float32, device="cuda:0") if "snap200" in cases else None
    times, last, info = {c: [] for c in cases}, {}, {}

    def digest(t):
        torch.cuda.synchronize()
        return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()[:16]

    with L.Lattice(p, ob) as lat:
        def call(c):
            if c == "run":
                lat.run(steps)
                return None
            if c == "snap200":
                lat.run_sampled(steps, EVERY[c], out=snap_t)
                return snap_t[-1]
            lat.run_mean(steps, EVERY[c], out=mean_t)
            return mean_t

        # warm-up: every shape the timed window uses.  The calls both builds make come first and in one order, so that
        # they start from the same lattices on both: the output's bits are taken here
        for c in cases:
            t = call(c)
            if t is not None:
                last[c] = digest(t)
        for _ in range(repeat):
            for c in cases:
                call(c)
                times[c].append(1e3 * lat.last_run_ms()[0] / steps)
                if c in ("mean1", "snap200"):
                    for k in INFO:
                        if k.startswith("mean" if c == "snap200" else "samples"):
                            continue
                        try:
                            info[k] = int(lat.info(k))
                        except L.LbmError:       # (a key the parent's build does not know)
                            info[k] = None
    print(json.dumps({"n": n, "times": times, "last": last, "info": info}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=800, help="steps per timed run (at least 200)")
    ap.add_argument("--repeat", type=int, default=3, help="timed runs of each call per child")
    ap.add_argument("--rounds", type=int, default=2, help="children per build and size (rounds x repeat >= 5 runs per figure)")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
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
        got = {b: {"times": {}, "last": {}, "info": {}} for b in ("this", "parent")}
        for _ in range(a.rounds):
            for b in ("this", "parent"):
                env = dict(os.environ)
                cases = list(ON_PARENT) + [c for c, _ in CASES if c not in ON_PARENT]
                if b == "parent":
                    env["LBM_MI355X_LIB"] = os.path.abspath(a.parent_lib)
                    cases = list(ON_PARENT)
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
                for c, h in x["last"].items():
                    got[b]["last"].setdefault(c, set()).add(h)
                got[b]["info"] = x["info"]
        t, q = got["this"], got["parent"]
        lines += ["", f"{n} x {n}: " + ", ".join(f"{k} = {v}" for k, v in t["info"].items()),
                  f"  {'':18s}{'this build':>42s}   {'the parent':>42s}"]
        for c, name in CASES:
            lines.append(f"  {name} {fig(t['times'][c]):>42s}   " + (f"{fig(q['times'][c]):>42s}" if c in q["times"] else f"{'--':>42s}"))
        med = {b: {c: statistics.median(v) for c, v in got[b]["times"].items()} for b in got}
        spread = max(t["times"]["run"]) - min(t["times"]["run"])
        same = abs(med["this"]["run"] - med["parent"]["run"]) <= spread
        lines.append(f"  (a) here against the parent: medians differ by {abs(med['this']['run'] - med['parent']['run']):.2f} us/step, "
                     f"its own spread {spread:.2f}: " + ("inside" if same else "OUTSIDE"))
        faster = True
        for c, name in CASES[1:4]:
            f = max(t["times"][c]) < min(q["times"][c])
            lines.append(f"  {name.split()[0]} parent / here = {med['parent'][c] / med['this'][c]:.2f} x; the slowest run here "
                         f"{max(t['times'][c]):.2f}, the parent's fastest {min(q['times'][c]):.2f}"
                         + ("" if f or c == "mean100" else "  -- NOT FASTER"))
            faster = faster and (f or c == "mean100")
        lines.append("  against (a) here: " + ", ".join(f"{name.split()[0]} {med['this'][c] / med['this']['run']:.3f} x" for c, name in CASES[1:]))
        bits = all(len(t["last"][c] | q["last"][c]) == 1 for c in ("mean1", "mean10", "mean100"))
        lines.append("  the mean's bits, (b), (c) and (d), every process of both builds: " + ("identical" if bits else "DIFFERENT"))
        ok = ok and same and faster and bits
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
