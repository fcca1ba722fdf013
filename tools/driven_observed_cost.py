#!/usr/bin/env python3
"""What observers under an acceleration schedule cost (lbm_run_driven_observed), on the 1024 x 1024 deck
over 2000 steps (the register tiles) and on the 8192 x 8192 synthetic deck of tools/make_deck.py over 800 steps (lbm_wave),
with forces on the deck's obstacle cells (one body) and 64 probes, both every step.

Per deck, GPU microseconds per step (lbm_last_run_ms: the step loop) and wall microseconds per step (the whole call, or the
whole loop of calls):
  run               lbm_run(nsteps)
  observed          lbm_run_observed with those observers: the floor, the same observers without a schedule
  driven            lbm_run_driven with nsteps distinct values from [0.5, 1.5] x the deck's acceleration
  <case>@parent     the three above against another build of the library (--parent-lib: the parent commit's), alternating
                    with this build's process by process; each pair's medians must differ by less than the spread `run` shows
                    against itself -- the existing kernels did not move
  driven_observed   lbm_run_driven_observed, that schedule and those observers
  loop              the parent's only alternative, on this build: nsteps x (lbm_set_accel + lbm_run_observed(1)); wall time
                    (every call has a GPU time of its own; their sum is printed beside it); --loop-decks, default the first
Every case runs in a process of its own under a time limit, one at a time, through the entry points it needs bound here (the
parent's build lacks the new one), after a warm-up run of 200 steps and one untimed call of the case's own shape; medians
with min and max over --repeat calls x --rounds processes.  A case that fails or runs out ends the table.

    python tools/driven_observed_cost.py [--decks 1024,8192] [--repeat 3] [--rounds 2] [--parent-lib path] [--out profiles/driven_observed_cost.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECKS = {"1024": (1024, 1024, 2000), "8192": (8192, 8192, 800)}
PAIRED = ("run", "observed", "driven")


def child(case, deck, repeat, lib_path):
    import ctypes as C
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import advanced_hpc_lbm_amd as L                             # (Param, Observe and the deck readers only: no library loaded)
    from make_deck import obstacle_map
    lib = C.CDLL(lib_path or L.LIB_PATH)
    vp = C.c_void_p
    lib.lbm_create.argtypes = [C.POINTER(L.Param), vp, vp, C.c_int, vp, C.c_int, C.POINTER(vp)]
    lib.lbm_run.argtypes = [vp, C.c_int, vp]
    lib.lbm_set_bodies.argtypes = [vp, vp, C.c_int]
    lib.lbm_set_probes.argtypes = [vp, vp, C.c_int]
    lib.lbm_run_observed.argtypes = [vp, C.c_int, vp, C.POINTER(L.Observe)]
    lib.lbm_set_accel.argtypes = [vp, C.c_float]
    lib.lbm_run_driven.argtypes = [vp, C.c_int, vp, vp]
    lib.lbm_last_run_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.lbm_destroy.argtypes = [vp]
    lib.lbm_get_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double)]
    lib.lbm_last_error.restype = C.c_char_p
    base = case.split("@")[0]
    if base == "driven_observed":
        lib.lbm_run_driven_observed.argtypes = [vp, C.c_int, vp, vp, C.POINTER(L.Observe)]
    nx, ny, steps = DECKS[deck]
    if deck == "1024":
        p = L.read_params(os.path.join(ROOT, "input_1024x1024.params"))
        ob = np.ascontiguousarray(L.read_obstacles(os.path.join(ROOT, "obstacles_1024x1024.dat"), p), dtype=np.int32)
    else:
        p = L.Param(nx, ny, steps, 10, 0.1, 0.01, 1.85)
        ob = np.ascontiguousarray(obstacle_map(nx, ny), dtype=np.int32)
    ob = ob.reshape(ny, nx)

    def ok(rc):
        if rc != 0:
            raise RuntimeError(lib.lbm_last_error().decode())

    def info(key):
        v = C.c_double(0)
        lib.lbm_get_info(ctx, key, C.byref(v))
        return int(v.value)

    def gpu_ms():
        g, w = C.c_double(0), C.c_double(0)
        lib.lbm_last_run_ms(ctx, C.byref(g), C.byref(w))
        return g.value

    ctx = vp()
    ok(lib.lbm_create(C.byref(p), ob.ctypes.data, None, 1, None, 0, C.byref(ctx)))
    body = np.ascontiguousarray((ob != 0).astype(np.int32))
    ok(lib.lbm_set_bodies(ctx, body.ctypes.data, 1))
    xy = np.array([(nx // 16 + i * (nx // 8), ny // 16 + j * (ny // 8)) for j in range(8) for i in range(8)], dtype=np.int32)
    ok(lib.lbm_set_probes(ctx, xy.ctypes.data, len(xy)))
    av = np.empty(steps, dtype=np.float32)
    forces = np.empty((steps, 1, 2), dtype=np.float32)
    probes = np.empty((steps, len(xy), 4), dtype=np.float32)
    what = L.Observe()
    what.forces, what.probes_out, what.probes_every = forces.ctypes.data, probes.ctypes.data, 1
    rng = np.random.default_rng(1)
    sched = (p.accel * (0.5 + rng.permutation(steps) / (steps - 1))).astype(np.float32)

    def once(n):
        t0 = time.perf_counter()
        if base == "run":
            ok(lib.lbm_run(ctx, n, av.ctypes.data))
            g = gpu_ms()
        elif base == "observed":
            ok(lib.lbm_run_observed(ctx, n, av.ctypes.data, C.byref(what)))
            g = gpu_ms()
        elif base == "driven":
            ok(lib.lbm_run_driven(ctx, n, av.ctypes.data, sched.ctypes.data))
            g = gpu_ms()
        elif base == "driven_observed":
            ok(lib.lbm_run_driven_observed(ctx, n, av.ctypes.data, sched.ctypes.data, C.byref(what)))
            g = gpu_ms()
        else:                                                    # loop
            g = 0.0
            for t in range(n):
                ok(lib.lbm_set_accel(ctx, float(sched[t])))
                ok(lib.lbm_run_observed(ctx, 1, av.ctypes.data, C.byref(what)))
                g += gpu_ms()
            ok(lib.lbm_set_accel(ctx, float(p.accel)))
        wall = (time.perf_counter() - t0) * 1e3
        return 1e3 * g / n, 1e3 * wall / n

    ok(lib.lbm_run(ctx, 200, av.ctypes.data))                    # warm-up (first launch, tiling query)
    once(steps)                                                  # the case's own shape, untimed
    vals = [once(steps) for _ in range(repeat)]
    keys = {"engine_last": info(b"engine_last")}
    if base == "observed":
        keys.update(in_kernel=info(b"observed_in_kernel"), in_wave=info(b"observed_in_wave"), pieces=info(b"observed_pieces"))
    if base == "driven":
        keys.update(in_kernel=info(b"driven_in_kernel"), in_wave=info(b"driven_in_wave"))
    if base == "driven_observed":
        keys.update(in_kernel=info(b"driven_observed_in_kernel"), in_wave=info(b"driven_observed_in_wave"),
                    pieces=info(b"driven_observed_pieces"))
    lib.lbm_destroy(ctx)
    print(json.dumps({"case": case, "gpu": [round(v[0], 3) for v in vals], "wall": [round(v[1], 3) for v in vals], "info": keys}))


def mmm(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f}, n = {len(v)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decks", default="1024,8192")
    ap.add_argument("--loop-decks", default=None, help="decks that also run the per-step loop (default: the first of --decks)")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="processes per case (a case and its @parent twin alternate)")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library, for the @parent cases")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--deck", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        return child(a.case, a.deck, a.repeat, os.environ.get("LBM_COST_LIB"))
    decks = a.decks.split(",")
    loop_decks = a.loop_decks.split(",") if a.loop_decks is not None else decks[:1]
    lines, good = [], True
    for deck in decks:
        nx, ny, steps = DECKS[deck]
        cases = []
        for base in PAIRED:
            for _ in range(a.rounds):
                cases.append(base)
                if a.parent_lib:
                    cases.append(base + "@parent")
        cases += ["driven_observed"] * a.rounds
        if deck in loop_decks:
            cases.append("loop")
        rows = {}
        for case in cases:
            env = dict(os.environ)
            if case.endswith("@parent"):
                env["LBM_COST_LIB"] = os.path.abspath(a.parent_lib)
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--deck", deck, "--repeat",
                                    str(1 if case == "loop" else a.repeat)], capture_output=True, text=True, timeout=a.timeout, env=env)
            except subprocess.TimeoutExpired:
                print(f"{deck} {case}: timed out after {a.timeout} s; stopping", file=sys.stderr)
                good = False
                break
            if r.returncode != 0:
                print(f"{deck} {case}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                good = False
                break
            x = json.loads(r.stdout.strip().splitlines()[-1])
            y = rows.setdefault(case, {"gpu": [], "wall": [], "info": x["info"]})
            y["gpu"] += x["gpu"]
            y["wall"] += x["wall"]
        lines.append(f"{nx} x {ny}, {steps} steps, forces on one body and 64 probes every step; us/step: median (min .. max, n); "
                     f"{a.repeat} timed calls per process after a warm-up and one untimed call, {a.rounds} process(es) per case, "
                     f"a case and its @parent twin alternating")
        lines.append(f"  {'case':18s} {'GPU us/step':>44s} {'wall us/step':>48s}   info")
        for case, x in rows.items():
            lines.append(f"  {case:18s} {mmm(x['gpu']):>44s} {mmm(x['wall']):>48s}   {x['info']}")
        med = {case: statistics.median(x["gpu"]) for case, x in rows.items()}
        if "run" in rows:
            spread = max(rows["run"]["gpu"]) - min(rows["run"]["gpu"])
            for base in PAIRED:
                if base in rows and base + "@parent" in rows:
                    diff = abs(med[base] - med[base + "@parent"])
                    lines.append(f"  {base} against {base}@parent: medians differ by {diff:.3f} us/step; run's own spread {spread:.3f} us/step: "
                                 + ("less: the existing kernels did not move" if diff < spread else "NOT LESS"))
        if "driven_observed" in rows:
            for base in ("observed", "driven", "run"):
                if base in rows:
                    lines.append(f"  driven_observed - {base} = {med['driven_observed'] - med[base]:+.3f} us/step of GPU time "
                                 f"({med['driven_observed'] / med[base]:.3f} x)")
            if "loop" in rows:
                lines.append(f"  loop / driven_observed = "
                             f"{statistics.median(rows['loop']['wall']) / statistics.median(rows['driven_observed']['wall']):.1f} x of wall time")
        lines.append("")
        if not good:
            break
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
