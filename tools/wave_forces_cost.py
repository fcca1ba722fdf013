#!/usr/bin/env python3
"""What drag and lift cost where lbm_wave runs (lbm_run_forces inside lbm_wave launches): the 8192 x 8192 and
4096 x 4096 lattices of tools/make_deck.py, every obstacle cell outside rows 0 and ny - 1 labelled body 1, default options
(what a caller gets: the info keys printed with each size say which kernel that is).

Per size, GPU microseconds per step (lbm_last_run_ms: device events around the step loop, the fold kernels included) of
  (a) forces@parent   lbm_run_forces against another build of the library (--parent-lib: the parent commit's)
  (b) forces          lbm_run_forces, this build
  (c) run             lbm_run, this build
  (d) run@parent      lbm_run, the parent's build
each the median over every timed run, with min .. max beside it.  One child process per build and round, this build and
the parent's alternating; inside a child a warm-up of each call, then lbm_run and lbm_run_forces alternating --repeat times.
Every child runs under a time limit; the first that fails ends the measurement.
The bars: (c) against (d) inside (c)'s own spread; (b) against (a) at least 2 x at 8192^2; (b) over (c) is the observer's price.

    python tools/wave_forces_cost.py [--steps 800] [--repeat 3] [--rounds 2] [--parent-lib path] [--out profiles/wave_forces_cost.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_deck import obstacle_map  # noqa: E402

SIZES = (8192, 4096)
INFO = ("engine_last", "time_block_active", "march_kernel", "wave_cols_active", "wave_rows", "forces_in_kernel", "forces_in_wave")


def child(n, steps, repeat):
    sys.path.insert(0, ROOT)
    import numpy as np
    import advanced_hpc_lbm_amd as L          # (LBM_MI355X_LIB, set by the parent process, picks the build)
    p = L.Param(n, n, steps, 10, 0.1, 0.01, 1.85)
    ob = obstacle_map(n, n)
    body = (ob != 0).astype(np.int32)
    body[0] = body[-1] = 0
    run, forces, info = [], [], {}
    with L.Lattice(p, ob) as lat:
        lat.set_bodies(body, 1)
        lat.run(steps)                           # warm-up: every shape the timed window uses
        lat.run_forces(steps)
        for _ in range(repeat):
            lat.run(steps)
            run.append(1e3 * lat.last_run_ms()[0] / steps)
            _, F = lat.run_forces(steps)
            forces.append(1e3 * lat.last_run_ms()[0] / steps)
        for k in INFO:
            try:
                info[k] = int(lat.info(k))
            except L.LbmError:                   # (a key the parent's build does not know)
                info[k] = None
    print(json.dumps({"n": n, "run": run, "forces": forces, "info": info, "drag_last": float(F[-1, 0, 0])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=800, help="steps per timed run (at least 160)")
    ap.add_argument("--repeat", type=int, default=3, help="timed runs of each call per child")
    ap.add_argument("--rounds", type=int, default=2, help="children per build and size (rounds x repeat >= 5 runs per figure)")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library, for (a) and (d)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.repeat)
    if a.steps < 160 or a.rounds * a.repeat < 5:
        ap.error("need at least 160 steps and rounds x repeat >= 5")
    builds = ["this"] + (["parent"] if a.parent_lib else [])
    lines = [f"{a.steps} steps per run, {a.rounds} processes per build and size (alternating), {a.repeat} timed runs of each call per process; "
             "GPU us/step: median (min .. max, n)"]
    ok = True

    def fig(v):
        return f"{statistics.median(v):10.2f} ({min(v):.2f} .. {max(v):.2f}, n = {len(v)})"

    for n in SIZES:
        got = {b: {"run": [], "forces": [], "info": None, "drag_last": None} for b in builds}
        for _ in range(a.rounds):
            for b in builds:
                env = dict(os.environ)
                if b == "parent":
                    env["LBM_MI355X_LIB"] = os.path.abspath(a.parent_lib)
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--steps", str(a.steps),
                                        "--repeat", str(a.repeat)], capture_output=True, text=True, timeout=a.timeout, env=env)
                except subprocess.TimeoutExpired:
                    print(f"{n} ({b}): timed out after {a.timeout} s; stopping", file=sys.stderr)
                    return 1
                if r.returncode != 0:
                    print(f"{n} ({b}): exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                    return 1
                x = json.loads(r.stdout.strip().splitlines()[-1])
                got[b]["run"] += x["run"]
                got[b]["forces"] += x["forces"]
                got[b]["info"], got[b]["drag_last"] = x["info"], x["drag_last"]
        t = got["this"]
        lines += ["", f"{n} x {n}: " + ", ".join(f"{k} = {v}" for k, v in t["info"].items())]
        if "parent" in got:
            lines.append(f"  (a) forces@parent {fig(got['parent']['forces'])}")
        lines.append(f"  (b) forces        {fig(t['forces'])}")
        lines.append(f"  (c) run           {fig(t['run'])}")
        b_, c_ = statistics.median(t["forces"]), statistics.median(t["run"])
        if "parent" in got:
            q = got["parent"]
            lines.append(f"  (d) run@parent    {fig(q['run'])}")
            a_, d_ = statistics.median(q["forces"]), statistics.median(q["run"])
            spread = max(t["run"]) - min(t["run"])
            same = abs(c_ - d_) <= spread
            lines.append(f"  (c) against (d): medians differ by {abs(c_ - d_):.2f} us/step, (c)'s own spread {spread:.2f}: "
                         + ("inside" if same else "OUTSIDE"))
            lines.append(f"  (a) / (b) = {a_ / b_:.2f} x" + ("" if n != 8192 or a_ >= 2.0 * b_ else "  -- LESS THAN 2 x"))
            lines.append(f"  last step's drag: {t['drag_last']!r} here, {q['drag_last']!r} on the parent"
                         + ("" if t["drag_last"] == q["drag_last"] else "  -- DIFFERENT"))
            ok = ok and same and (n != 8192 or a_ >= 2.0 * b_) and t["drag_last"] == q["drag_last"]
        lines.append(f"  (b) / (c) = {b_ / c_:.3f} x  (the observer's price; the probes' on the register tiles: 1.09 x)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
