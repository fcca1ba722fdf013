#!/usr/bin/env python3
"""Regenerates the committed fixtures under tests/golden/ (run in the build container).

Two kinds of fixture, both DATA (inputs + expected outputs), never source:

1. `<deck>.final_state.pressure.f64.npz` for the two decks whose golden
   final_state.dat is absent from the reference mount
   (/root/reference/.MISSING_LARGE_BLOBS: 256x256, 1024x1024).  Produced by the
   double-precision oracle, which reproduces every golden file that IS shipped
   digit for digit (tests/test_oracle_golden.py); the arrays are checked here
   against the sha256 fingerprints recorded in BASELINE.md (addendum), which
   were taken from a double build of the reference itself.  Stored values are
   the pressures as printed with %.12E and parsed back (what check.py would
   load), little-endian float64, row-major jj outer / ii inner.

2. `kat_*.npz` known-answer vectors: small lattices (non-square, random
   obstacles, open top/bottom rows so the y-wrap is live, perturbed initial
   state) advanced 1, 2 and 10 steps by THE REFERENCE ITSELF --
   timestep_new2 from /root/reference/d2q9-bgk.c compiled with strict IEEE
   flags by oracle/Makefile into oracle/_ref/libd2q9_ref_strict.so.  They pin
   the oracle (bit-exact, float) on the GPU box, where the reference is absent.

3. `ref_float_<deck>.npz`: av_vels + final pressure written by the reference
   CLI binary as shipped (float, -Ofast; oracle/_ref/d2q9-bgk) on the small
   decks: the expected float-vs-double deviation our own checker must report.

4. `ref_strict_decks.npz` / `ref_strict_random.npz` / `ref_strict_params.npz`: what the strict build of
   the reference (oracle/_ref/libd2q9_ref_strict.so) computes on the shipped
   decks (from rest, a few hundred steps: av_vels per step, sha256 of the final
   lattice, av_velocity, Reynolds number) and on small random lattices (inputs
   and outputs in full; ref_strict_params: the same at every point of
   PARAM_GRID, accelerate refusals included).  They pin the float oracle bit
   for bit where the reference is absent.

5. `check_py_128x128.json`: the stdout and exit status of the reference's
   unchanged check/check.py on the cases check_py_cases() writes (identical
   files, the reference float binary's outputs, out of tolerance, wrong step
   count, wrong coordinates), against the 128x128 golden files.

Usage: python tests/golden/make_golden.py [--pressure 256x256 1024x1024] [--kat] [--ref-float]
                                          [--ref-strict] [--ref-strict-params] [--check-py <reference>/check/check.py]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import lbm_oracle as O  # noqa: E402

# BASELINE.md addendum: sha256 of the float64-LE pressure arrays
PRESSURE_SHA256 = {
    "256x256": "51d1f8f682c6da7a63b43b997e27fce96c910aaaf44c210b5f8fc1572c55cc2d",
    "1024x1024": "e65843180cc9c608c67d63d1b124e73e613cdd78a625845dc7cf41316e69a00d",
}


def printed(a: np.ndarray) -> np.ndarray:
    """Round-trip through the %.12E text form, as a reader of final_state.dat sees it."""
    return np.array([float("%.12E" % v) for v in a.ravel()], dtype="<f8").reshape(a.shape)


def make_pressure(deck: str) -> None:
    orc = O.Oracle()
    prm = O.read_params(os.path.join(ROOT, f"input_{deck}.params"))
    ob = O.read_obstacles(os.path.join(ROOT, f"obstacles_{deck}.dat"), prm.nx, prm.ny)
    cells = orc.init_cells(prm, np.float64)
    t = time.time()
    av = orc.run(prm, cells, ob, prm.maxIters)
    print(f"{deck}: double oracle ran {prm.maxIters} steps in {time.time() - t:.1f} s", flush=True)
    gold_av = open(os.path.join(HERE, f"{deck}.av_vels.dat")).read()
    assert O.format_av_vels(av) == gold_av, "double oracle does not reproduce the shipped av_vels golden"
    fs = orc.final_state(prm, cells, ob)
    pressure = printed(fs[:, :, 3])
    sha = hashlib.sha256(pressure.tobytes()).hexdigest()
    print(f"{deck}: sha256(pressure f64) = {sha}")
    assert sha == PRESSURE_SHA256[deck], "fingerprint differs from BASELINE.md"
    np.savez_compressed(os.path.join(HERE, f"{deck}.final_state.pressure.f64.npz"),
                        pressure=pressure, reynolds=np.float64(orc.reynolds(prm, cells, ob)))


def make_kat() -> None:
    ref = O.ReferenceStrict()
    rng = np.random.default_rng(20260104)
    cases = [("kat_8x6", 8, 6), ("kat_16x12", 16, 12), ("kat_33x20", 33, 20), ("kat_64x40", 64, 40)]
    for name, nx, ny in cases:
        prm = O.OrcParam(nx, ny, 10, 10, 0.1, 0.005, 1.85)
        rp = O.to_ref_param(prm)
        ob = (rng.random((ny, nx)) < 0.12).astype(np.int32)
        ob[0, 1:-1] = 0          # open bottom and top rows: y-wrap is exercised
        ob[ny - 1, 1:-1] = 0
        ob[ny - 2, : nx // 2] = 0  # accelerate row: half guaranteed fluid, rest random
        w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
        cells0 = (0.1 * w * (1.0 + 0.2 * (rng.random((ny, nx, 9)) - 0.5))).astype(np.float32)
        # a few cells so thin that the accelerate guard (f3-w1>0 etc.) must refuse them
        cells0[ny - 2, 1, 3] = 1e-6
        cells0[ny - 2, 2, 6] = 1e-7
        out = {"nx": nx, "ny": ny, "reynolds_dim": 10, "density": 0.1, "accel": 0.005, "omega": 1.85,
               "obstacles": ob, "cells0": cells0}
        a, b = cells0.copy(), np.empty_like(cells0)
        av = []
        for tt in range(1, 11):
            av.append(ref.timestep_new2(rp, a, b, ob))
            a, b = b, a
            if tt in (1, 2, 10):
                out[f"cells_after_{tt}"] = a.copy()
        out["av_vels"] = np.array(av, dtype=np.float32)
        out["reynolds_after_10"] = np.float32(ref.calc_reynolds(rp, a, ob))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print(f"{name}: blocked {int(ob.sum())}/{nx * ny}, av_vels[9] = {av[-1]:.9e}")


def make_ref_float(decks) -> None:
    exe = os.path.join(ROOT, "oracle", "_ref", "d2q9-bgk")
    for deck in decks:
        with tempfile.TemporaryDirectory() as td:
            r = subprocess.run([exe, os.path.join(ROOT, f"input_{deck}.params"),
                                os.path.join(ROOT, f"obstacles_{deck}.dat")],
                               cwd=td, check=True, capture_output=True, text=True)
            av = O.read_av_vels(os.path.join(td, "av_vels.dat")).astype(np.float32)
            fs = O.read_final_state(os.path.join(td, "final_state.dat"))
            reyn = [ln for ln in r.stdout.splitlines() if ln.startswith("Reynolds")][0].split()[-1]
        ny_nx = deck.split("x")
        nx, ny = int(ny_nx[0]), int(ny_nx[1])
        np.savez_compressed(os.path.join(HERE, f"ref_float_{deck}.npz"), av_vels=av,
                            pressure=fs[:, 5].astype(np.float32).reshape(ny, nx),
                            reynolds=np.float64(reyn))
        print(f"ref_float_{deck}: Reynolds {reyn}")


# (deck, steps) and (nx, ny, seed) of the strict-reference fixtures; tests/test_oracle_vs_reference.py runs the same
REF_STRICT_DECKS = (("128x128", 300), ("128x256", 300), ("256x256", 100), ("1024x1024", 8))
REF_STRICT_RANDOM = ((2, 2, 1), (3, 5, 2), (17, 9, 3), (40, 31, 4), (128, 7, 5))
RANDOM_STEPS = 5


def random_param(nx, ny):
    return O.OrcParam(nx, ny, RANDOM_STEPS, 7, 0.13, 0.02, 1.7)


def random_case(nx, ny, seed):
    """(param, obstacles, cells0) of a random lattice: dense random obstacles, perturbed populations."""
    rng = np.random.default_rng(seed)
    prm = random_param(nx, ny)
    ob = (rng.random((ny, nx)) < 0.3).astype(np.int32)
    ob[0, 0] = 0
    a = (0.05 + 0.1 * rng.random((ny, nx, 9))).astype(np.float32)
    return prm, ob, a


def make_ref_strict() -> None:
    ref = O.ReferenceStrict()
    out = {}
    for deck, nsteps in REF_STRICT_DECKS:
        prm = O.read_params(os.path.join(ROOT, f"input_{deck}.params"))
        rp = O.to_ref_param(prm)
        ob = O.read_obstacles(os.path.join(ROOT, f"obstacles_{deck}.dat"), prm.nx, prm.ny)
        a = O.Oracle().init_cells(prm, np.float32)
        b = np.empty_like(a)
        av = []
        for _ in range(nsteps):
            av.append(ref.timestep_new2(rp, a, b, ob))
            a, b = b, a
        out[f"{deck}.av_vels"] = np.array(av, dtype=np.float32)
        out[f"{deck}.state_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())
        out[f"{deck}.av_velocity"] = np.float32(ref.av_velocity(rp, a, ob))
        out[f"{deck}.reynolds"] = np.float32(ref.calc_reynolds(rp, a, ob))
        print(f"ref_strict {deck}: {nsteps} steps, av_vels[-1] = {av[-1]:.9e}")
    np.savez_compressed(os.path.join(HERE, "ref_strict_decks.npz"), **out)
    out = {}
    for nx, ny, seed in REF_STRICT_RANDOM:
        prm, ob, a = random_case(nx, ny, seed)
        rp = O.to_ref_param(prm)
        key = f"{nx}x{ny}_{seed}"
        out[f"{key}.obstacles"], out[f"{key}.cells0"] = ob, a.copy()
        b = np.empty_like(a)
        av = []
        for _ in range(RANDOM_STEPS):
            av.append(ref.timestep_new2(rp, a, b, ob))
            a, b = b, a
        out[f"{key}.av_vels"], out[f"{key}.cells"] = np.array(av, dtype=np.float32), a
    np.savez_compressed(os.path.join(HERE, "ref_strict_random.npz"), **out)
    print(f"ref_strict random lattices: {len(REF_STRICT_RANDOM)}")


# Points of the parameter space that the suite visits, (density, accel, omega); tests/test_param_space.py runs them all.
# "refusal": the accelerate guard (f3 - a1 > 0 && f6 - a2 > 0 && f7 - a2 > 0) refuses part of row ny-2 from step 3 on
# when started from rest (calibrated on the float oracle: tests/test_param_space.py checks that it still does).
PARAM_GRID = {
    "control": (0.1, 0.01, 1.85),          # the shipped decks
    "under_relaxed": (0.1, 0.005, 0.6),    # omega < 1
    "omega_one": (0.1, 0.02, 1.0),         # 1 - omega is exactly 0
    "stability_edge": (0.37, 0.03, 1.99),  # density well away from 0.1
    "light_fluid": (0.02, 0.5, 1.5),       # small density, strong accel
    "refusal": (0.1, 0.3, 1.85),           # guard refuses during the run
}
# (nx, ny, seed, state kind, steps) of ref_strict_params.npz, run at every point of PARAM_GRID
REF_STRICT_PARAMS = ((17, 9, 11, "guard", 6), (33, 20, 12, "rest", 12), (21, 14, 13, "perturbed", 6))
EQ_WEIGHTS = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)


def grid_param(point, nx, ny, steps=100):
    density, accel, omega = PARAM_GRID[point]
    return O.OrcParam(nx, ny, steps, 10, density, accel, omega)


def accel_weights(density, accel):
    """(a1, a2) of the accelerate phase in float, as the reference forms them (d2q9-bgk.c:230-231)."""
    d, a = np.float32(density), np.float32(accel)
    return d * a / np.float32(9), d * a / np.float32(36)


def refused(density, accel, ob, cells):
    """Mask over row ny-2: the fluid cells whose accelerate the guard refuses on the float lattice `cells`."""
    a1, a2 = accel_weights(density, accel)
    row = np.asarray(cells[-2], dtype=np.float32)
    ok = (row[:, 3] - a1 > 0) & (row[:, 6] - a2 > 0) & (row[:, 7] - a2 > 0)
    return (np.asarray(ob[-2]) == 0) & ~ok


def param_state(point, nx, ny, seed, kind, blocked=0.1):
    """(obstacles, cells0) at a point of PARAM_GRID.  kind:
      "rest"      -- the equilibrium at rest (as the reference initialises), random obstacles;
      "perturbed" -- every population within +-10 % of that equilibrium;
      "guard"     -- perturbed, and row ny-2 holds every kind of cell the accelerate guard tells apart: refused by
                     f3 - a1, by f6 - a2 and by f7 - a2 alone, f3 == a1 exactly (refused: 0 > 0 is false), f6 == a2
                     exactly, blocked cells with populations thinner than a1 / a2, and cells that pass."""
    density, accel, _ = PARAM_GRID[point]
    rng = np.random.default_rng(seed)
    ob = (rng.random((ny, nx)) < blocked).astype(np.int32)
    eq = np.float32(density) * EQ_WEIGHTS
    if kind == "rest":
        return ob, np.broadcast_to(eq.astype(np.float32), (ny, nx, 9)).copy()
    cells = (eq * (1.0 + 0.2 * (rng.random((ny, nx, 9)) - 0.5))).astype(np.float32)
    if kind == "guard":
        assert nx >= 10
        a1, a2 = accel_weights(density, accel)
        row = cells[ny - 2]
        ob[ny - 2, :8] = 0
        ob[ny - 2, 8:10] = 1
        row[0, 3] = a1 * np.float32(0.5)      # f3 alone
        row[1, 6] = a2 * np.float32(0.25)     # f6 alone
        row[2, 7] = a2 * np.float32(0.9)      # f7 alone
        row[3, 3] = a1                        # f3 == a1 exactly
        row[4, 6] = a2                        # f6 == a2 exactly
        row[5, 3] = np.nextafter(a1, np.float32(1))   # the smallest f3 that passes
        row[8, 3], row[8, 6], row[8, 7] = a1 * np.float32(0.5), a2 * np.float32(0.5), np.float32(0)   # blocked, thin
        row[9, 3], row[9, 6], row[9, 7] = np.float32(1e-9), np.float32(0), a2                        # blocked, thin
        # cells 6 and 7 (and the random rest of the row) pass
    return ob, cells


def make_ref_strict_params() -> None:
    """ref_strict_params.npz: the strict reference's per-step av_vels and final lattice at every PARAM_GRID point."""
    ref = O.ReferenceStrict()
    out = {}
    for point in PARAM_GRID:
        for nx, ny, seed, kind, nsteps in REF_STRICT_PARAMS:
            prm = grid_param(point, nx, ny, nsteps)
            rp = O.to_ref_param(prm)
            ob, a = param_state(point, nx, ny, seed, kind)
            b = np.empty_like(a)
            av, nref = [], 0
            for _ in range(nsteps):
                nref += int(refused(prm.density, prm.accel, ob, a).sum())
                av.append(ref.timestep_new2(rp, a, b, ob))
                a, b = b, a
            key = f"{point}.{nx}x{ny}_{seed}"
            out[f"{key}.obstacles"], out[f"{key}.cells0"] = ob, param_state(point, nx, ny, seed, kind)[1]
            out[f"{key}.av_vels"], out[f"{key}.cells"] = np.array(av, dtype=np.float32), a
            print(f"ref_strict_params {key} ({kind}): {nsteps} steps, {nref} refusals, av_vels[-1] = {av[-1]:.9e}")
    np.savez_compressed(os.path.join(HERE, "ref_strict_params.npz"), **out)


def check_py_cases(outdir):
    """{case: (av_vels file, final_state file)} written under `outdir`, each to be checked against
    tests/golden/128x128.{av_vels,final_state}.dat."""
    ga = os.path.join(HERE, "128x128.av_vels.dat")
    gf = os.path.join(HERE, "128x128.final_state.dat")
    with np.load(os.path.join(HERE, "ref_float_128x128.npz")) as z:
        av, pr = z["av_vels"].astype(np.float64), z["pressure"].astype(np.float64).ravel()
    fs_lines = open(gf).readlines()

    def write(name, av, pr, lines=fs_lines):
        pa, pf = os.path.join(outdir, f"{name}.av_vels.dat"), os.path.join(outdir, f"{name}.final_state.dat")
        with open(pa, "w") as f:
            f.write(O.format_av_vels(av))
        with open(pf, "w") as f:
            for ln, p in zip(lines, pr):
                t = ln.split(" ")
                t[5] = "%.12E" % p
                f.write(" ".join(t))
        return pa, pf

    off_av, off_pr = av.copy(), pr.copy()
    off_av[30000] *= 1.015
    off_pr[777] *= 0.97
    swapped = list(fs_lines)
    swapped[5], swapped[6] = swapped[6], swapped[5]
    return {
        "identical": (ga, gf),
        "float_binary": write("float_binary", av, pr),
        "out_of_tolerance": write("out_of_tolerance", off_av, off_pr),
        "fewer_steps": write("fewer_steps", av[:-1], pr),
        "coordinates_differ": write("coordinates_differ", av, pr, swapped),
    }


def make_check_py(check_py) -> None:
    ga = os.path.join(HERE, "128x128.av_vels.dat")
    gf = os.path.join(HERE, "128x128.final_state.dat")
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for case, (sa, sf) in check_py_cases(td).items():
            r = subprocess.run([sys.executable, check_py, "--ref-av-vels-file", ga, "--ref-final-state-file", gf,
                                "--av-vels-file", sa, "--final-state-file", sf], capture_output=True, text=True)
            out[case] = {"returncode": r.returncode, "stdout": r.stdout}
            print(f"check.py {case}: exit {r.returncode}")
    with open(os.path.join(HERE, "check_py_128x128.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pressure", nargs="*", default=[])
    ap.add_argument("--kat", action="store_true")
    ap.add_argument("--ref-float", nargs="*", default=[])
    ap.add_argument("--ref-strict", action="store_true")
    ap.add_argument("--check-py", default=None, help="the reference's check/check.py")
    ap.add_argument("--ref-strict-params", action="store_true")
    args = ap.parse_args()
    O.build()
    for d in args.pressure:
        make_pressure(d)
    if args.kat:
        make_kat()
    if args.ref_float:
        make_ref_float(args.ref_float)
    if args.ref_strict:
        make_ref_strict()
    if args.check_py:
        make_check_py(args.check_py)
    if args.ref_strict_params:
        make_ref_strict_params()
