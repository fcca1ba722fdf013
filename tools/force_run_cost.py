#!/usr/bin/env python3
"""What drag and lift during a run cost on the 1024 x 1024 deck (lbm_run_forces, DESIGN.md "Forces on bodies").

Per case, GPU microseconds per step (lbm_last_run_ms: the step loop with its force sums and their fold) and wall
microseconds per step (the whole call, or the whole per-step loop):
  run            lbm_run(nsteps)
  forces/1       lbm_run_forces(nsteps), one body: the deck's obstacle (the walls, rows 0 and ny-1, unlabelled)
  forces/4       lbm_run_forces(nsteps), four bodies: the obstacle cut in two by its middle column, the bottom wall, the top wall
  loop           nsteps x (lbm_run(1) + lbm_read_state), the loop lbm_run_forces replaces (at most 200 steps of it: per step)
Every case runs in a child process of its own under a time limit; a case that fails or runs out ends the table.

    python tools/force_run_cost.py [--steps 2000] [--repeat 3] [--out profiles/force_run_cost.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["run", "forces/1", "forces/4", "loop"]


def bodies(ob, n):
    ob = ob.reshape(-1, ob.shape[-1]) if ob.ndim == 2 else ob
    blocked = ob != 0
    walls = np.zeros(ob.shape, dtype=bool)
    walls[0], walls[-1] = blocked[0], blocked[-1]
    obstacle = blocked & ~walls
    if n == 1:
        return obstacle.astype(np.int32)
    cols = np.nonzero(obstacle.any(axis=0))[0]
    mid = (cols.min() + cols.max() + 1) // 2 if cols.size else 0
    lab = np.zeros(ob.shape, dtype=np.int32)
    lab[obstacle] = 1
    lab[:, mid:][obstacle[:, mid:]] = 2
    lab[0][walls[0]] = 3
    lab[-1][walls[-1]] = 4
    return lab


def child(case, steps, repeat):
    sys.path.insert(0, ROOT)
    import advanced_hpc_lbm_amd as L
    p = L.read_params(os.path.join(ROOT, "input_1024x1024.params"))
    ob = np.asarray(L.read_obstacles(os.path.join(ROOT, "obstacles_1024x1024.dat"), p)).reshape(p.ny, p.nx)
    kind, _, e = case.partition("/")
    best = None
    with L.Lattice(p, ob) as lat:
        if kind == "forces":
            lat.set_bodies(bodies(ob, int(e)), int(e))
        lat.run(200)                                             # warm-up (first launch, tiling query)
        if kind == "loop":
            steps = min(steps, 200)
        for _ in range(repeat):
            t0 = time.perf_counter()
            if kind == "run":
                lat.run(steps)
                gpu = lat.last_run_ms()[0]
            elif kind == "forces":
                lat.run_forces(steps)
                gpu = lat.last_run_ms()[0]
                assert lat.info("forces_in_kernel") == 1
            else:
                gpu = 0.0
                for _ in range(steps):
                    lat.run(1)
                    gpu += lat.last_run_ms()[0]
                    lat.read_state()
            wall = (time.perf_counter() - t0) * 1e3
            r = (1e3 * gpu / steps, 1e3 * wall / steps)
            best = r if best is None or r[0] < best[0] else best
        engine = int(lat.info("engine_last"))
    print(json.dumps({"case": case, "gpu_us_per_step": round(best[0], 3), "wall_us_per_step": round(best[1], 3),
                      "engine_last": engine}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        return child(a.case, a.steps, a.repeat)
    rows = []
    for case in CASES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--steps", str(a.steps),
                                "--repeat", str(a.repeat)], capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"{case}: timed out after {a.timeout} s; stopping", file=sys.stderr)
            break
        if r.returncode != 0:
            print(f"{case}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            break
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    base = next((x["gpu_us_per_step"] for x in rows if x["case"] == "run"), None)
    print(f"1024x1024, {a.steps} steps, best of {a.repeat}")
    print(f"{'case':14s} {'GPU us/step':>12s} {'wall us/step':>13s} {'GPU vs run':>11s}")
    for x in rows:
        rel = f"{x['gpu_us_per_step'] / base:10.3f}x" if base else ""
        print(f"{x['case']:14s} {x['gpu_us_per_step']:12.3f} {x['wall_us_per_step']:13.3f} {rel}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"deck": "1024x1024", "steps": a.steps, "repeat": a.repeat, "rows": rows}, f, indent=1)
    return 0 if len(rows) == len(CASES) else 1


if __name__ == "__main__":
    sys.exit(main())
