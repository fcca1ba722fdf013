#!/usr/bin/env python3
"""What the live inputs cost (lbm_set_obstacles, lbm_write_state) against the only alternative the parent
had, on the 1024 x 1024 deck and on the 8192 x 8192 synthetic deck of tools/make_deck.py.

Per deck, wall milliseconds per call (time.perf_counter around the call: every one of them returns complete):
  set_obstacles/keep   lbm_set_obstacles(LBM_REFILL_KEEP), the map alternating between the deck's and a shifted copy of it
  set_obstacles/rest   the same under LBM_REFILL_REST
  write_state/host     lbm_write_state from a host array (what lbm_read_state returned)
  write_state/device   lbm_write_state from device memory holding the same floats
  recreate             lbm_destroy + lbm_create with the same map and lattice + the first lbm_run(1) behind it: first-run
                       costs (the tiling's residency query, the first launch) are part of what the live inputs save
  first_run/live       lbm_run(1) behind a live input, for comparison with the one inside `recreate`
and GPU microseconds per step of lbm_run:
  run            lbm_run(nsteps) on this build
  run@parent     the same against another build of the library (--parent-lib: the parent commit's), alternating with `run`
                 process by process; the two must agree within the spread the PARENT shows against itself
Every process runs under a time limit; medians with min and max over n >= 5 values.  A case that fails or runs out ends
the table.

    python tools/live_inputs_cost.py [--decks 1024,8192] [--repeat 3] [--rounds 2] [--parent-lib path] [--out profiles/live_inputs_cost.txt]
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
HIP_RUNTIME = ("libamdhip64.so.7", "libamdhip64.so", "/opt/rocm/lib/libamdhip64.so")   # (the library has loaded it already)


def child(case, deck, repeat, lib_path):
    import ctypes as C
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import advanced_hpc_lbm_amd as L                             # (Param and the deck readers only: no library loaded)
    from make_deck import obstacle_map
    lib = C.CDLL(lib_path or L.LIB_PATH)
    vp = C.c_void_p
    lib.lbm_create.argtypes = [C.POINTER(L.Param), vp, vp, C.c_int, vp, C.c_int, C.POINTER(vp)]
    lib.lbm_run.argtypes = [vp, C.c_int, vp]
    lib.lbm_last_run_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.lbm_read_state.argtypes = [vp, vp]
    lib.lbm_destroy.argtypes = [vp]
    lib.lbm_get_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double)]
    lib.lbm_last_error.restype = C.c_char_p
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

    def timed(f):
        t0 = time.perf_counter()
        f()
        return round((time.perf_counter() - t0) * 1e3, 4)

    ctx = vp()
    ok(lib.lbm_create(C.byref(p), ob.ctypes.data, None, 1, None, 0, C.byref(ctx)))
    av = np.empty(steps, dtype=np.float32)
    ok(lib.lbm_run(ctx, 200, av.ctypes.data))                    # warm-up (first launch, tiling query)
    if case.startswith("run"):
        ok(lib.lbm_run(ctx, steps, av.ctypes.data))              # the case's own shape, untimed
        vals = []
        for _ in range(repeat):
            ok(lib.lbm_run(ctx, steps, av.ctypes.data))
            vals.append(round(1e3 * gpu_ms() / steps, 3))
        res = {"lbm_run": vals}
        keys = {"engine_last": info(b"engine_last")}
    else:
        n = max(2 * repeat, 5)
        lib.lbm_set_obstacles.argtypes = [vp, vp, C.c_int]
        lib.lbm_write_state.argtypes = [vp, vp]
        hip = None
        for name in HIP_RUNTIME:
            try:
                hip = C.CDLL(name)
                break
            except OSError:
                continue
        if hip is None:
            raise RuntimeError("cannot load the HIP runtime for the device copy of the lattice")
        hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
        hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [vp]
        maps = (np.ascontiguousarray(np.roll(ob, 3, axis=1)), ob)    # (the body three columns east, and back)
        cells = np.empty((ny, nx, 9), dtype=np.float32)
        ok(lib.lbm_read_state(ctx, cells.ctypes.data))
        d_cells = vp()
        if hip.hipMalloc(C.byref(d_cells), cells.nbytes) != 0 or hip.hipMemcpy(d_cells, cells.ctypes.data, cells.nbytes, 1) != 0:
            raise RuntimeError("no device copy of the lattice")
        res = {}
        for name, refill in (("set_obstacles/keep", 0), ("set_obstacles/rest", 1)):
            ok(lib.lbm_set_obstacles(ctx, maps[1].ctypes.data, refill))                  # untimed
            res[name] = [timed(lambda: ok(lib.lbm_set_obstacles(ctx, maps[i % 2].ctypes.data, refill))) for i in range(n)]
        keys = {"refilled_cells": info(b"refilled_cells"), "obstacle_updates": info(b"obstacle_updates")}
        for name, ptr in (("write_state/host", cells.ctypes.data), ("write_state/device", d_cells)):
            ok(lib.lbm_write_state(ctx, ptr))
            res[name] = [timed(lambda: ok(lib.lbm_write_state(ctx, ptr))) for _ in range(n)]
        res["first_run/live"] = []
        for i in range(n):
            ok(lib.lbm_set_obstacles(ctx, maps[i % 2].ctypes.data, 1))
            ok(lib.lbm_write_state(ctx, d_cells))
            res["first_run/live"].append(timed(lambda: ok(lib.lbm_run(ctx, 1, av.ctypes.data))))
        hip.hipFree(d_cells)

        def recreate():
            lib.lbm_destroy(ctx)
            ok(lib.lbm_create(C.byref(p), ob.ctypes.data, cells.ctypes.data, 1, None, 0, C.byref(ctx)))
            ok(lib.lbm_run(ctx, 1, av.ctypes.data))

        recreate()
        res["recreate"] = [timed(recreate) for _ in range(n)]
        keys["engine_last"] = info(b"engine_last")
    lib.lbm_destroy(ctx)
    print(json.dumps({"case": case, "values": res, "info": keys}))


def mmm(v):
    return f"{statistics.median(v):11.3f} ({min(v):.3f} .. {max(v):.3f}, n = {len(v)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decks", default="1024,8192")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="processes of run (and run@parent, alternating)")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library, for run@parent")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--deck", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        return child(a.case, a.deck, a.repeat, os.environ.get("LBM_COST_LIB"))
    lines, good = [], True
    for deck in a.decks.split(","):
        nx, ny, steps = DECKS[deck]
        cases = ["live"]
        for _ in range(a.rounds):
            cases.append("run")
            if a.parent_lib:
                cases.append("run@parent")
        rows, infos = {}, {}
        for case in cases:
            env = dict(os.environ)
            if case == "run@parent":
                env["LBM_COST_LIB"] = os.path.abspath(a.parent_lib)
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--deck", deck, "--repeat", str(a.repeat)],
                                   capture_output=True, text=True, timeout=a.timeout, env=env)
            except subprocess.TimeoutExpired:
                print(f"{deck} {case}: timed out after {a.timeout} s; stopping", file=sys.stderr)
                good = False
                break
            if r.returncode != 0:
                print(f"{deck} {case}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                good = False
                break
            x = json.loads(r.stdout.strip().splitlines()[-1])
            infos[case] = x["info"]
            for name, v in x["values"].items():
                rows.setdefault(name if case != "run@parent" else name + "@parent", []).extend(v)
        lines.append(f"{nx} x {ny}: median (min .. max, n)")
        lines.append(f"  {'call':22s} {'wall ms per call':>48s}")
        for name in ("set_obstacles/keep", "set_obstacles/rest", "write_state/host", "write_state/device", "first_run/live", "recreate"):
            if name in rows:
                lines.append(f"  {name:22s} {mmm(rows[name]):>48s}")
        if "live" in infos:
            lines.append(f"  info after the live calls: {infos['live']}")
        if "recreate" in rows:
            base = statistics.median(rows["recreate"])
            for name in ("set_obstacles/keep", "set_obstacles/rest", "write_state/host", "write_state/device"):
                if name in rows:
                    lines.append(f"  recreate / {name} = {base / statistics.median(rows[name]):.1f} x")
        lines.append(f"  lbm_run over {steps} steps, GPU us per step; {a.repeat} timed calls per process after a warm-up and one untimed call, "
                     f"{a.rounds} process(es) each, alternating")
        for name in ("lbm_run", "lbm_run@parent"):
            if name in rows:
                lines.append(f"  {name:22s} {mmm(rows[name]):>48s}")
        if "lbm_run" in rows and "lbm_run@parent" in rows:
            g = rows["lbm_run@parent"]
            spread = max(g) - min(g)
            diff = abs(statistics.median(rows["lbm_run"]) - statistics.median(g))
            lines.append(f"  lbm_run against lbm_run@parent: medians differ by {diff:.3f} us/step; the parent's own spread {spread:.3f} us/step: "
                         + ("within it: the existing kernels did not move" if diff <= spread else "NOT WITHIN IT"))
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
