#!/usr/bin/env python3
"""What one run with several observers costs on the 1024 x 1024 deck (lbm_run_observed), next to the single
calls it replaces.

Per case, GPU microseconds per step (lbm_last_run_ms: the sums over the step-loop pieces) and wall microseconds per step (the
whole call):
  run            lbm_run(nsteps)
  run@parent     the same against another build of the library (--parent-lib: the parent commit's), alternating with `run`
                 child by child; the two must agree within the spread `run` shows against itself (tools/probe_run_cost.py's
                 child, which binds only the entry points an older build has)
  groups         one child process per group: the combined call and every single call it replaces, alternating inside the
                 process, so that a group's rows were measured under the same conditions.  64 probes = an 8 x 8 grid over
                 the lattice (64 different tiles); the bodies = the walls and the obstacle (two labels).
                   F+P      forces + 64 probes every step: one launch of the force + probe flavour
                   F+P+M    ... + means every 100: pieces of 100 steps
                   F+P+M+S  ... + snapshots every 500 (host output)
The structural bar: a combined call takes less GPU time than its single calls together.  Every child runs under a time limit,
after a warm-up run of 200 steps and one untimed call of each shape; best of --repeat, all repeats kept for the spread.

    python tools/observed_run_cost.py [--steps 2000] [--repeat 3] [--rounds 3] [--parent-lib path] [--out profiles/observed_run_cost.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from probe_run_cost import child_run, probe_set  # noqa: E402

MEAN_EVERY, FIELDS_EVERY = 100, 500
GROUPS = {"F+P": ("forces", "probes"), "F+P+M": ("forces", "probes", "mean"), "F+P+M+S": ("forces", "probes", "mean", "fields")}


def child_group(group, steps, repeat):
    sys.path.insert(0, ROOT)
    import numpy as np
    import advanced_hpc_lbm_amd as L
    p = L.read_params(os.path.join(ROOT, "input_1024x1024.params"))
    ob = np.ascontiguousarray(L.read_obstacles(os.path.join(ROOT, "obstacles_1024x1024.dat"), p), dtype=np.int32).reshape(p.ny, p.nx)
    walls = np.zeros(ob.shape, bool)
    walls[0], walls[-1] = ob[0] != 0, ob[-1] != 0
    body = np.where(walls, 1, np.where(ob != 0, 2, 0)).astype(np.int32)
    kinds = GROUPS[group]
    want = dict(forces=True, probes_every=1, mean_every=MEAN_EVERY if "mean" in kinds else 0,
                fields_every=FIELDS_EVERY if "fields" in kinds else 0)
    with L.Lattice(p, ob) as lat:
        lat.set_bodies(body, 2)
        lat.set_probes(probe_set(64, p.nx, p.ny))
        lat.run(200)                                             # warm-up (first launch, tiling query)
        calls = {group: lambda: lat.run_observed(steps, **want), "forces": lambda: lat.run_forces(steps),
                 "probes/1:64": lambda: lat.run_probes(steps, 1)}
        if "mean" in kinds:
            calls[f"mean/{MEAN_EVERY}"] = lambda: lat.run_mean(steps, MEAN_EVERY)
        if "fields" in kinds:
            calls[f"sampled/{FIELDS_EVERY}"] = lambda: lat.run_sampled(steps, FIELDS_EVERY)
        vals = {name: [] for name in calls}
        info = {}
        for rep in range(repeat + 1):                            # (the first round: every shape once, untimed)
            for name, call in calls.items():
                t0 = time.perf_counter()
                call()
                wall = (time.perf_counter() - t0) * 1e3
                if rep:
                    vals[name].append((1e3 * lat.last_run_ms()[0] / steps, 1e3 * wall / steps))
                if name == group:
                    info = {k: int(lat.info(k)) for k in ("observed_in_kernel", "observed_pieces", "engine_last")}
    rows = []
    for name, v in vals.items():
        best = min(v)
        rows.append({"case": ("observed " if name == group else "  ") + name, "gpu_us_per_step": round(best[0], 3),
                     "wall_us_per_step": round(best[1], 3), "all_gpu_us_per_step": [round(x[0], 3) for x in v]})
    rows[0].update(info)
    print(json.dumps({"group": group, "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="children of `run` (and of run@parent, alternating)")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library, for run@parent")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        if a.case.startswith("run"):
            return child_run(a.case, a.steps, a.repeat, os.environ.get("LBM_COST_LIB"))
        return child_group(a.case, a.steps, a.repeat)
    cases = []
    for _ in range(a.rounds):
        cases.append("run")
        if a.parent_lib:
            cases.append("run@parent")
    cases += list(GROUPS)
    runs, groups, ok = {}, [], True
    for case in cases:
        env = dict(os.environ)
        if case == "run@parent":
            env["LBM_COST_LIB"] = os.path.abspath(a.parent_lib)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--steps", str(a.steps),
                                "--repeat", str(a.repeat)], capture_output=True, text=True, timeout=a.timeout, env=env)
        except subprocess.TimeoutExpired:
            print(f"{case}: timed out after {a.timeout} s; stopping", file=sys.stderr)
            ok = False
            break
        if r.returncode != 0:
            print(f"{case}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            ok = False
            break
        x = json.loads(r.stdout.strip().splitlines()[-1])
        if "group" in x:
            groups.append(x)
        elif case in runs:                                       # a further round of the same case
            y = runs[case]
            y["all_gpu_us_per_step"] += x["all_gpu_us_per_step"]
            if x["gpu_us_per_step"] < y["gpu_us_per_step"]:
                y["gpu_us_per_step"], y["wall_us_per_step"] = x["gpu_us_per_step"], x["wall_us_per_step"]
        else:
            runs[case] = x
    lines = [f"1024x1024, {a.steps} steps, best of {a.repeat} per process (run, run@parent: {a.rounds} processes each, alternating; "
             "one process per group)",
             f"{'case':28s} {'GPU us/step':>12s} {'wall us/step':>13s}   all GPU us/step (min .. max)"]

    def line(x):
        al = x["all_gpu_us_per_step"]
        return f"{x['case']:28s} {x['gpu_us_per_step']:12.3f} {x['wall_us_per_step']:13.3f}   {min(al):.3f} .. {max(al):.3f} (n = {len(al)})"
    for x in runs.values():
        lines.append(line(x))
    if "run" in runs and "run@parent" in runs:
        al = runs["run"]["all_gpu_us_per_step"]
        spread = max(al) - min(al)
        diff = abs(runs["run"]["gpu_us_per_step"] - runs["run@parent"]["gpu_us_per_step"])
        lines.append(f"run against run@parent: best differs by {diff:.3f} us/step; run's own spread {spread:.3f} us/step: "
                     + ("agree" if diff <= spread else "DO NOT AGREE"))
    for g in groups:
        rows = g["rows"]
        lines.append("")
        for x in rows:
            lines.append(line(x))
        both = rows[0]["gpu_us_per_step"]
        singles = sum(x["gpu_us_per_step"] for x in rows[1:])
        lines.append(f"  {g['group']}: observed_in_kernel = {rows[0].get('observed_in_kernel')}, observed_pieces = {rows[0].get('observed_pieces')}, "
                     f"engine_last = {rows[0].get('engine_last')}; one run {both:.3f} against {singles:.3f} us/step for its single calls together "
                     f"({both / singles:.2f}x): " + ("less" if both < singles else "NOT LESS"))
        ok = ok and both < singles
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
