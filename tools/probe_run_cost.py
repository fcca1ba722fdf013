#!/usr/bin/env python3
"""What time series at chosen cells cost on the 1024 x 1024 deck (lbm_run_probes).

Per case, GPU microseconds per step (lbm_last_run_ms: the step loop, the probes' stores included, copies to the host not)
and wall microseconds per step (the whole call, or the whole chunked loop with its torch sums, synchronised):
  run            lbm_run(nsteps)
  run@parent     the same against another build of the library (--parent-lib: the parent commit's), alternating with `run`
                 child by child; the two must agree within the spread `run` shows against itself.  Both go through the five
                 entry points they need (create, run, last_run_ms, get_info, destroy) bound here, not through the package's binding,
                 which asks an older build for symbols it does not have
  probes/E:N     lbm_run_probes(nsteps, every = E) with N probes, host output: N = 1 a wake probe, N = 64 an 8 x 8 grid
                 over the lattice (64 different tiles), N = 1024 one full column (ii = 512: one lane per row storing, 16
                 tiles doing so on every sample step), N = 1024row one full row (jj = 512: the same number of stores, but
                 one row of one wave in each of 16 tiles -- what tells the stores' cost from the cost of derive_cell on
                 every row of a tile)
  mean/1         lbm_run_mean(nsteps, every = 1), for scale
  sampled+sum/1  what probes replace: lbm_run_sampled(every = 1) into a device tensor, in chunks of at most 64 snapshots
                 (1 GiB), and a torch sum over each chunk's snapshots (the cheapest use anybody could make of them)
Every case runs in a child process of its own (torch imported first where it is used) under a time limit, after a warm-up
run of 200 steps and one untimed call of the case's own shape; best of --repeat, all repeats kept for the spread.  A case
that fails or runs out ends the table.

    python tools/probe_run_cost.py [--steps 2000] [--repeat 3] [--rounds 3] [--parent-lib path] [--out profiles/probe_run_cost.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("probes/1:1", "probes/1:64", "probes/1:1024", "probes/1:1024row", "probes/100:64", "mean/1", "sampled+sum/1")
CHUNK_SNAPS = 64


def probe_set(n, nx, ny):
    if n == "1024row":
        return [(ii, ny // 2) for ii in range(nx)]
    n = int(n)
    if n == 1:
        return [(3 * nx // 4, ny // 2)]
    if n == 64:
        return [(nx // 16 + a * (nx // 8), ny // 16 + b * (ny // 8)) for b in range(8) for a in range(8)]
    return [(nx // 2, jj) for jj in range(ny)]


def child_run(case, steps, repeat, lib_path):
    import ctypes as C
    sys.path.insert(0, ROOT)
    import numpy as np
    import advanced_hpc_lbm_amd as L                             # (Param and the deck readers only: no library loaded)
    lib = C.CDLL(lib_path or L.LIB_PATH)
    vp = C.c_void_p
    lib.lbm_create.argtypes = [C.POINTER(L.Param), vp, vp, C.c_int, vp, C.c_int, C.POINTER(vp)]
    lib.lbm_run.argtypes = [vp, C.c_int, vp]
    lib.lbm_last_run_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.lbm_destroy.argtypes = [vp]
    lib.lbm_get_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double)]
    lib.lbm_last_error.restype = C.c_char_p
    p = L.read_params(os.path.join(ROOT, "input_1024x1024.params"))
    ob = np.ascontiguousarray(L.read_obstacles(os.path.join(ROOT, "obstacles_1024x1024.dat"), p), dtype=np.int32)
    ctx = vp()
    if lib.lbm_create(C.byref(p), ob.ctypes.data, None, 1, None, 0, C.byref(ctx)) != 0:
        raise RuntimeError(lib.lbm_last_error().decode())
    av = np.empty(steps, dtype=np.float32)
    vals = []
    for n in (200, steps) + (steps,) * repeat:                   # warm-up, one untimed call of the timed shape, the repeats
        t0 = time.perf_counter()
        if lib.lbm_run(ctx, n, av.ctypes.data) != 0:
            raise RuntimeError(lib.lbm_last_error().decode())
        wall = (time.perf_counter() - t0) * 1e3
        g, w = C.c_double(0), C.c_double(0)
        lib.lbm_last_run_ms(ctx, C.byref(g), C.byref(w))
        vals.append((1e3 * g.value / n, 1e3 * wall / n))
    eng = C.c_double(0)
    lib.lbm_get_info(ctx, b"engine_last", C.byref(eng))
    lib.lbm_destroy(ctx)
    vals = vals[2:]
    best = min(vals)
    print(json.dumps({"case": case, "gpu_us_per_step": round(best[0], 3), "wall_us_per_step": round(best[1], 3),
                      "all_gpu_us_per_step": [round(v[0], 3) for v in vals], "engine_last": int(eng.value)}))


def child(case, steps, repeat):
    if case.startswith("run"):
        return child_run(case, steps, repeat, os.environ.get("LBM_COST_LIB"))
    kind, _, e = case.partition("/")
    e, _, nprobes = e.partition(":")
    every = int(e) if e else 0
    if kind == "sampled+sum":
        import torch
    sys.path.insert(0, ROOT)
    import advanced_hpc_lbm_amd as L
    p = L.read_params(os.path.join(ROOT, "input_1024x1024.params"))
    ob = L.read_obstacles(os.path.join(ROOT, "obstacles_1024x1024.dat"), p)
    vals = []
    with L.Lattice(p, ob) as lat:
        lat.run(200)                                             # warm-up (first launch, tiling query)
        outs = {}
        if kind == "probes":
            lat.set_probes(probe_set(nprobes, p.nx, p.ny))

        def once():
            t0 = time.perf_counter()
            if kind == "probes":
                lat.run_probes(steps, every)
                gpu = lat.last_run_ms()[0]
                assert lat.info("probes_in_kernel") == 1
            elif kind == "mean":
                lat.run_mean(steps, every)
                gpu = lat.last_run_ms()[0]
                assert lat.info("mean_in_kernel") == 1
            else:
                gpu, done = 0.0, 0
                total = torch.zeros((p.ny, p.nx, 4), dtype=torch.float32, device="cuda:0")
                while done < steps:
                    n = min(CHUNK_SNAPS * every, steps - done)
                    m = n // every
                    if m not in outs:
                        outs[m] = torch.empty((m, p.ny, p.nx, 4), dtype=torch.float32, device="cuda:0")
                    lat.run_sampled(n, every, out=outs[m])
                    assert m == 0 or lat.info("samples_in_kernel") == 1
                    gpu += lat.last_run_ms()[0]
                    if m:
                        total += outs[m].sum(dim=0)
                    done += n
                (total / float(steps // every)).cpu()
                torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            return 1e3 * gpu / steps, 1e3 * wall / steps

        once()                                                   # the case's own shape, untimed
        for _ in range(repeat):
            vals.append(once())
        engine = int(lat.info("engine_last"))
    best = min(vals)
    print(json.dumps({"case": case, "gpu_us_per_step": round(best[0], 3), "wall_us_per_step": round(best[1], 3),
                      "all_gpu_us_per_step": [round(v[0], 3) for v in vals], "engine_last": engine}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="children of `run` (and of run@parent, alternating)")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library, for run@parent")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case")
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        return child(a.case, a.steps, a.repeat)
    cases = []
    for _ in range(a.rounds):
        cases.append("run")
        if a.parent_lib:
            cases.append("run@parent")
    cases += list(CASES)
    rows, ok = {}, True
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
        if case in rows:                                         # a further round of the same case
            y = rows[case]
            y["all_gpu_us_per_step"] += x["all_gpu_us_per_step"]
            if x["gpu_us_per_step"] < y["gpu_us_per_step"]:
                y["gpu_us_per_step"], y["wall_us_per_step"] = x["gpu_us_per_step"], x["wall_us_per_step"]
        else:
            rows[case] = x
    base = rows.get("run", {}).get("gpu_us_per_step")
    lines = [f"1024x1024, {a.steps} steps, best of {a.repeat} per process (run, run@parent: {a.rounds} processes each, alternating)",
             f"{'case':16s} {'GPU us/step':>12s} {'wall us/step':>13s} {'GPU vs run':>11s}   all GPU us/step (min .. max)"]
    for case, x in rows.items():
        rel = f"{x['gpu_us_per_step'] / base:10.3f}x" if base else ""
        al = x["all_gpu_us_per_step"]
        lines.append(f"{case:16s} {x['gpu_us_per_step']:12.3f} {x['wall_us_per_step']:13.3f} {rel}   {min(al):.3f} .. {max(al):.3f} (n = {len(al)})")
    if "run" in rows and "run@parent" in rows:
        al = rows["run"]["all_gpu_us_per_step"]
        spread = max(al) - min(al)
        diff = abs(rows["run"]["gpu_us_per_step"] - rows["run@parent"]["gpu_us_per_step"])
        lines.append(f"run against run@parent: best differs by {diff:.3f} us/step; run's own spread {spread:.3f} us/step: "
                     + ("agree" if diff <= spread else "DO NOT AGREE"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
