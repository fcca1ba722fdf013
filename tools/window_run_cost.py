#!/usr/bin/env python3
"""What a window series costs (lbm_run_window) against the only way to get the same data without it:
lbm_run_sampled plus a slice on the host.  Host output on both sides, default options (what a caller gets: the info keys
printed with each case say which kernels took the samples).

Cases
  1024 x 1024 deck, 2000 steps, every = 10 and 100 (the register tiles):
      whole        the whole lattice at stride 1 (the probe flavour fed a dense table against the snapshot flavour)
      256x256      a 256 x 256 window at (384, 384)
      stride4      the whole extent at strides (4, 4)
  8192 x 1024, no obstacles, 800 steps, every = 10 (lbm_wave):
      512x512      a 512 x 512 window at (3840, 256)
      stride8      the whole extent at strides (8, 8)
Per case and side, GPU microseconds per step (lbm_last_run_ms: device events around the step loop, sample stores included,
the copy to the host not) and wall microseconds per step (the whole call; on the sampled side the host slice, made
contiguous, included), each the median over every timed run with min .. max beside it.  One child process per case, side and
round, the two sides alternating; inside a child one warm-up call, then --repeat timed calls from the lattice the call
before left.  Every child runs under a time limit; the first that fails ends the measurement.  Both sides make the same
calls in the same order from the same start, so their last outputs must be the same bits: the table says so per case.
No ratio is asserted: the table is there to show (1) whether a window run's GPU time stays at or below lbm_run_sampled's at
the same period, within the run-to-run spread printed beside it, and (2) how much of the wall time the smaller copy removes.
Exit status 1 only if a child fails or the two sides' bits differ.

    python tools/window_run_cost.py [--repeat 3] [--rounds 2] [--out profiles/window_run_cost.txt]
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
INFO = ("engine_last", "time_block_active", "window_in_kernel", "window_in_wave", "samples_in_kernel", "samples_in_wave")
# name: (lattice, steps, every, (x0, y0, nx, ny, sx, sy))
CASES = {}
for _e in (10, 100):
    CASES[f"1024^2 whole /{_e}"] = ("deck", 2000, _e, (0, 0, 1024, 1024, 1, 1))
    CASES[f"1024^2 256x256 /{_e}"] = ("deck", 2000, _e, (384, 384, 256, 256, 1, 1))
    CASES[f"1024^2 stride4 /{_e}"] = ("deck", 2000, _e, (0, 0, 256, 256, 4, 4))
CASES["8192x1024 512x512 /10"] = ("wave", 800, 10, (3840, 256, 512, 512, 1, 1))
CASES["8192x1024 stride8 /10"] = ("wave", 800, 10, (0, 0, 1024, 128, 8, 8))


def child(case, side, repeat):
    sys.path.insert(0, ROOT)
    import numpy as np
    import advanced_hpc_lbm_amd as L
    lattice, steps, every, win = CASES[case]
    if lattice == "deck":
        p = L.read_params(os.path.join(ROOT, "input_1024x1024.params"))
        ob = L.read_obstacles(os.path.join(ROOT, "obstacles_1024x1024.dat"), p)
    else:
        p = L.Param(8192, 1024, steps, 10, 0.1, 0.005, 1.7)
        ob = np.zeros((p.ny, p.nx), np.int32)
    w = L.Window(*win)
    gpu, wall, out = [], [], None
    with L.Lattice(p, ob) as lat:
        for i in range(repeat + 1):                              # (the first call is the warm-up)
            t0 = time.perf_counter()
            if side == "window":
                _, out = lat.run_window(steps, every, w)
            else:
                _, fields = lat.run_sampled(steps, every)
                out = np.ascontiguousarray(fields[:, w.y0:w.y0 + (w.ny - 1) * w.sy + 1:w.sy, w.x0:w.x0 + (w.nx - 1) * w.sx + 1:w.sx])
                copied = fields.nbytes
                del fields
            t1 = time.perf_counter()
            if i > 0:
                gpu.append(1e3 * lat.last_run_ms()[0] / steps)
                wall.append(1e6 * (t1 - t0) / steps)
        info = {k: int(lat.info(k)) for k in INFO}
    if side == "window":
        copied = out.nbytes
    print(json.dumps({"gpu": gpu, "wall": wall, "info": info, "copied": copied,
                      "bits": hashlib.sha256(out.tobytes()).hexdigest()[:16]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3, help="timed calls per child")
    ap.add_argument("--rounds", type=int, default=2, help="children per case and side")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--only", default=None, help="a substring of the case names to run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--side", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.side, a.repeat)
    lines = [f"{a.rounds} processes per case and side (alternating), {a.repeat} timed calls per process after one warm-up call; "
             "us/step: median (min .. max, n)", "window: lbm_run_window; sampled: lbm_run_sampled + the slice on the host", ""]
    ok = True

    def fig(v):
        return f"{statistics.median(v):9.2f} ({min(v):.2f} .. {max(v):.2f}, n = {len(v)})"

    for case in CASES:
        if a.only and a.only not in case:
            continue
        got = {s: {"gpu": [], "wall": [], "bits": set()} for s in ("window", "sampled")}
        for _ in range(a.rounds):
            for side in ("window", "sampled"):
                print(f"{case}: {side}", file=sys.stderr, flush=True)
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--side", side,
                                        "--repeat", str(a.repeat)], capture_output=True, text=True, timeout=a.timeout)
                except subprocess.TimeoutExpired:
                    print(f"{case} ({side}): timed out after {a.timeout} s; stopping", file=sys.stderr)
                    return 1
                if r.returncode != 0:
                    print(f"{case} ({side}): exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                    return 1
                x = json.loads(r.stdout.strip().splitlines()[-1])
                g = got[side]
                g["gpu"] += x["gpu"]; g["wall"] += x["wall"]; g["bits"].add(x["bits"]); g["info"] = x["info"]; g["copied"] = x["copied"]
        wn, sm = got["window"], got["sampled"]
        _, steps, every, win = CASES[case]
        keys = ", ".join(f"{k} = {v}" for k, v in wn["info"].items() if k.startswith(("engine", "time", "window")))
        keys_s = ", ".join(f"{k} = {v}" for k, v in sm["info"].items() if k.startswith("samples"))
        lines += [f"{case}: {steps} steps, window {win}; window side: {keys}; sampled side: {keys_s}",
                  f"  {'':8s}{'GPU us/step':>40s}   {'wall us/step':>40s}   {'copied to the host':>20s}"]
        for name, g in (("window", wn), ("sampled", sm)):
            lines.append(f"  {name:8s}{fig(g['gpu']):>40s}   {fig(g['wall']):>40s}   {g['copied'] / 2 ** 20:16.1f} MiB")
        mg = {s: statistics.median(got[s]["gpu"]) for s in got}
        mw = {s: statistics.median(got[s]["wall"]) for s in got}
        spread = max(max(g["gpu"]) - min(g["gpu"]) for g in (wn, sm))
        below = mg["window"] <= mg["sampled"] + spread
        lines.append(f"  GPU: window - sampled = {mg['window'] - mg['sampled']:+.2f} us/step, the larger spread {spread:.2f}: "
                     + ("at or below, within the spread" if below else "ABOVE, beyond the spread"))
        lines.append(f"  wall: sampled / window = {mw['sampled'] / mw['window']:.1f} x; the window removes "
                     f"{100 * (1 - mw['window'] / mw['sampled']):.0f} % of the wall time")
        same = len(wn["bits"] | sm["bits"]) == 1
        lines += ["  the last output's bits, every process of both sides: " + ("identical" if same else "DIFFERENT"), ""]
        ok = ok and same
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
