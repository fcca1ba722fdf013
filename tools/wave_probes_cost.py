#!/usr/bin/env python3
"""What a time series at chosen cells costs where lbm_wave runs (lbm_run_probes inside lbm_wave launches):
the 8192 x 8192 and 4096 x 4096 lattices of tools/make_deck.py, default options (what a caller gets: the info keys printed
with each size say which kernel that is).

Per size, GPU microseconds per step (lbm_last_run_ms: device events around the step loop, gather kernels included) of
  (a) run                lbm_run                                             this build and the parent's
  (b) probes 8x8 /1      lbm_run_probes, every = 1, 64 probes on an 8 x 8 grid    this build and the parent's
  (c) probes row /1      every = 1, one row of probes (LBM_MAX_PROBES = 4096 of them: a full row at 4096, half of one at 8192)
  (d) probes column /1   every = 1, one column of probes (likewise)
  (e) probes 8x8 /100    every = 100, the 64 probes
  (f) observed f+p /1    lbm_run_observed, forces (every obstacle cell outside rows 0 and ny - 1 is body 1) and the 64 probes
                         at every = 1                                             this build and the parent's
each the median over every timed run, with min .. max beside it.  One child process per build and round, this build and
the parent's (--parent-lib: a build of the parent commit's library) alternating; inside a child a warm-up of each call,
then the calls in turn --repeat times (the calls both builds make first, in one order: the same lattices on both).  Every child runs under a time limit; the first that fails ends the measurement.
Exit status 1 unless: (a) here lies inside its own spread of the parent's (a); at 8192^2 the slowest (b) here is faster than
the parent's fastest (b); both builds give identical bits for the last sample of (b) and of (f).

    python tools/wave_probes_cost.py --parent-lib path [--steps 800] [--repeat 3] [--rounds 2] [--out profiles/wave_probes_cost.txt]
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
MAX_PROBES = 4096
INFO = ("engine_last", "time_block_active", "march_kernel", "wave_cols_active", "wave_rows", "probes_in_kernel", "probes_in_wave",
        "observed_in_wave", "observed_pieces")
CASES = (("run", "(a) run             "), ("grid", "(b) probes 8x8 /1   "), ("row", "(c) probes row /1   "),
         ("col", "(d) probes column /1"), ("grid100", "(e) probes 8x8 /100 "), ("obs", "(f) observed f+p /1 "))
ON_PARENT = ("run", "grid", "obs")


def child(n, steps, repeat, cases):
    sys.path.insert(0, ROOT)
    import numpy as np
    import advanced_hpc_lbm_amd as L          # (LBM_MI355X_LIB, set by the parent process, picks the build)
    p = L.Param(n, n, steps, 10, 0.1, 0.01, 1.85)
    ob = obstacle_map(n, n)
    body = (ob != 0).astype(np.int32)
    body[0] = body[-1] = 0
    g = (np.arange(8) * (n // 8) + n // 16).astype(np.int32)
    line = (np.arange(min(n, MAX_PROBES)) + (n - min(n, MAX_PROBES)) // 2).astype(np.int32)
    sets = {"grid": np.array([(i, j) for j in g for i in g], dtype=np.int32),
            "row": np.stack([line, np.full_like(line, n // 2 + 3)], axis=1),
            "col": np.stack([np.full_like(line, n // 2 + 3), line], axis=1)}
    sets["grid100"] = sets["obs"] = sets["grid"]
    times, last, info = {c: [] for c in cases}, {}, {}
    with L.Lattice(p, ob) as lat:
        lat.set_bodies(body, 1)

        def call(c):
            if c == "run":
                lat.run(steps)
                return None
            lat.set_probes(sets[c])
            if c == "obs":
                return lat.run_observed(steps, forces=True, probes_every=1)["probes"]
            return lat.run_probes(steps, 100 if c == "grid100" else 1)[1]

        # warm-up: every shape the timed window uses.  The calls both builds make come first and in one order, so that
        # they start from the same lattices on both: the last sample's bits are taken here
        for c in cases:
            pr = call(c)
            if pr is not None:
                last[c] = hashlib.sha256(np.ascontiguousarray(pr[-1]).tobytes()).hexdigest()[:16]
        for _ in range(repeat):
            for c in cases:
                call(c)
                times[c].append(1e3 * lat.last_run_ms()[0] / steps)
                if c in ("grid", "obs"):
                    for k in INFO:
                        if c == "grid" and k.startswith("observed"):
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
                  f"  {'':21s}{'this build':>42s}   {'the parent':>42s}"]
        for c, name in CASES:
            lines.append(f"  {name} {fig(t['times'][c]):>42s}   " + (f"{fig(q['times'][c]):>42s}" if c in q["times"] else f"{'--':>42s}"))
        med = {b: {c: statistics.median(v) for c, v in got[b]["times"].items()} for b in got}
        spread = max(t["times"]["run"]) - min(t["times"]["run"])
        same = abs(med["this"]["run"] - med["parent"]["run"]) <= spread
        lines.append(f"  (a) here against the parent: medians differ by {abs(med['this']['run'] - med['parent']['run']):.2f} us/step, "
                     f"its own spread {spread:.2f}: " + ("inside" if same else "OUTSIDE"))
        faster = max(t["times"]["grid"]) < min(q["times"]["grid"])
        lines.append(f"  (b) parent / here = {med['parent']['grid'] / med['this']['grid']:.2f} x; the slowest run here "
                     f"{max(t['times']['grid']):.2f}, the parent's fastest {min(q['times']['grid']):.2f}"
                     + ("" if faster or n != 8192 else "  -- NOT FASTER"))
        lines.append(f"  (f) parent / here = {med['parent']['obs'] / med['this']['obs']:.2f} x")
        lines.append("  against (a) here: " + ", ".join(f"{name.split()[0]} {med['this'][c] / med['this']['run']:.3f} x" for c, name in CASES[1:]))
        bits = all(len(t["last"][c] | q["last"][c]) == 1 for c in ("grid", "obs"))
        lines.append("  the last sample's bits, (b) and (f), every run of both builds: " + ("identical" if bits else "DIFFERENT"))
        ok = ok and same and (faster or n != 8192) and bits
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
