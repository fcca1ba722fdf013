"""The parameter space away from the shipped decks: every engine at every point of PARAM_GRID (tests/golden/make_golden.py),
in the regime where the accelerate guard (f3 - a1 > 0 && f6 - a2 > 0 && f7 - a2 > 0, d2q9-bgk.c:246-258) refuses cells
during the run, and against the double-precision oracle.

  * no GPU: the float oracle equals the strict build of the reference bit for bit at every grid point
    (tests/golden/ref_strict_params.npz), and the states used here do what they claim (refusals, finite lattices);
  * one step from the GPU's own state, shadowed by the oracle in double and in float: u = 2^-24, rho = the cell's
    density; every element |gpu - f64| <= 8 u rho, and the GPU's worst error at most twice the float oracle's + 1 u rho;
    the accelerate phase is the reference's float arithmetic, so a guard decision that differs moves a population by
    a1 (1e-3 rho and more), far outside that bar;
  * every multi-step engine bit for bit against the one-step kernel at grid points and in the refusal regime;
  * whole runs at the smooth points against the double oracle: at most 4 x the float oracle's own deviation + a floor."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, deck_paths

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden import PARAM_GRID, REF_STRICT_PARAMS, accel_weights, param_state, refused  # noqa: E402

U = 2.0 ** -24
# No refusal over 200 steps from rest (asserted).  Not "stability_edge": from rest on a channel it starts refusing near step
# 40 and is no longer finite by step 50, so it is held to the one-step and engine tests (20 steps) only.
SMOOTH = ("control", "under_relaxed", "omega_one")
REFUSING = ("light_fluid", "refusal")
ONE_THIRD = np.float32(1.0 / 3.0)
ENGINE_AV_RTOL = 2e-6               # av_vels of a multi-step engine against the one-step kernel: summation order


def _orc_param(O, point, nx, ny, steps=100):
    """The grid point as the float parameters the reference reads (t_param holds floats), for both oracle flavours."""
    d, a, o = (float(np.float32(v)) for v in PARAM_GRID[point])
    return O.OrcParam(nx, ny, steps, 10, d, a, o)


def _lparam(L, point, nx, ny, steps=100):
    d, a, o = PARAM_GRID[point]
    return L.Param(nx, ny, steps, 10, d, a, o)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _count_refusals(oracle, prm, ob, cells, nsteps):
    """Per step: fluid cells of row ny-2 the guard refuses on the float oracle's run from `cells`."""
    a, b = cells.copy(), np.empty_like(cells)
    counts = []
    for _ in range(nsteps):
        counts.append(int(refused(prm.density, prm.accel, ob, a).sum()))
        oracle.timestep(prm, a, b, ob)
        a, b = b, a
    assert np.all(np.isfinite(a))
    return counts


# ----------------------------------------------------------------------------------------------------------- no GPU
def _params_vectors():
    with np.load(os.path.join(GOLDEN, "ref_strict_params.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("nx,ny,seed,kind,nsteps", REF_STRICT_PARAMS)
@pytest.mark.parametrize("point", list(PARAM_GRID))
def test_oracle_equals_reference_on_the_parameter_grid_bitwise(O, oracle, point, nx, ny, seed, kind, nsteps):
    """Every step's av_vels and the final lattice equal what the strict build of the reference computed at this grid
    point (tests/golden/ref_strict_params.npz); the guard states and the refusing points did refuse."""
    k = _params_vectors()
    key = f"{point}.{nx}x{ny}_{seed}"
    prm = _orc_param(O, point, nx, ny, nsteps)
    ob, a = k[f"{key}.obstacles"], k[f"{key}.cells0"].copy()
    b = np.empty_like(a)
    av, nref = [], 0
    for _ in range(nsteps):
        nref += int(refused(prm.density, prm.accel, ob, a).sum())
        av.append(oracle.timestep(prm, a, b, ob))
        a, b = b, a
    assert np.array_equal(np.array(av, np.float32).view(np.uint32), k[f"{key}.av_vels"].view(np.uint32))
    assert np.array_equal(_bits(a), _bits(k[f"{key}.cells"]))
    assert np.all(np.isfinite(a))
    if kind == "guard" or point in REFUSING:
        assert nref > 0, key


@pytest.mark.parametrize("point", list(PARAM_GRID))
def test_guard_state_holds_every_kind_of_cell(O, oracle, point):
    """Row ny-2 of the guard state: cells 0-4 refused (f3, f6, f7 alone; f3 == a1 and f6 == a2 exactly), 5-7 pass (5 by
    one ulp), 8-9 blocked with populations thinner than a1 / a2.  The float oracle's accelerate leaves exactly the
    refused and blocked cells untouched."""
    nx, ny = 17, 9
    ob, cells = param_state(point, nx, ny, 11, "guard")
    prm = _orc_param(O, point, nx, ny)
    a1, a2 = accel_weights(prm.density, prm.accel)
    row = cells[ny - 2]
    assert row[3, 3] == a1 and row[4, 6] == a2 and row[5, 3] > a1
    assert row[8, 3] < a1 and row[9, 6] < a2 and ob[ny - 2, 8] == 1 and ob[ny - 2, 9] == 1
    ref = refused(prm.density, prm.accel, ob, cells)
    assert ref[:5].all() and not ref[5:10].any()
    # each of the first three is refused by its own condition alone
    assert row[0, 6] > a2 and row[0, 7] > a2 and row[1, 3] > a1 and row[1, 7] > a2 and row[2, 3] > a1 and row[2, 6] > a2
    acc = cells.copy()
    oracle.accelerate(prm, acc, ob)
    moved = np.any(acc[ny - 2] != cells[ny - 2], axis=1)
    assert np.array_equal(moved, (ob[ny - 2] == 0) & ~ref)
    assert np.array_equal(_bits(acc[: ny - 2]), _bits(cells[: ny - 2]))


def test_refusal_regime_is_calibrated(O, oracle):
    """The refusal point from rest on 128 x 64 with 10 % random obstacles: from step 4 on the guard refuses between 5 %
    and 95 % of the fluid cells of row ny-2 at every step, and the lattice stays finite over 40 steps."""
    nx, ny = 128, 64
    ob, cells = param_state("refusal", nx, ny, 1, "rest")
    counts = _count_refusals(oracle, _orc_param(O, "refusal", nx, ny), ob, cells, 40)
    fluid = int((ob[ny - 2] == 0).sum())
    frac = np.array(counts[3:]) / fluid
    assert counts[0] == 0 and np.all(frac >= 0.05) and np.all(frac <= 0.95), np.round(frac, 2)


def test_smooth_points_do_not_refuse(O, oracle):
    """The points held to the double oracle over whole runs refuse nothing over 200 steps from rest (a refusal is a
    threshold: its float and double decisions may differ, and the bar there would be a1, not the float rounding)."""
    for point in SMOOTH:
        prm = _orc_param(O, point, 128, 256)
        of = deck_paths("128x256")[1]
        ob = O.read_obstacles(of, 128, 256)
        cells = oracle.init_cells(prm, np.float32)
        assert sum(_count_refusals(oracle, prm, ob, cells, 200)) == 0, point


# ----------------------------------------------------------------------------------------------------------- GPU: one step
# (nx, ny, seed, state kind at a smooth point, at a refusing point)
SHADOW_CASES = [(64, 40, 31, "guard", "guard"), (33, 20, 32, "perturbed", "rest"), (128, 64, 33, "rest", "rest")]
NSHADOW = 20


def one_step_oracle(oracle, o64, prm, ob, x):
    """One step from the float lattice x by the oracle in double and in float, the accelerate phase in the reference's
    float arithmetic for both: (t64, rho, e32, av32, av64); e32 = the float oracle's worst error in u rho."""
    acc = x.copy()
    oracle.accelerate(prm, acc, ob)
    a64 = acc.astype(np.float64)
    t64 = np.empty_like(a64)
    av64 = o64.sweep(prm, a64, t64, ob)
    t32 = np.empty_like(acc)
    av32 = oracle.sweep(prm, acc.copy(), t32, ob)
    rho = t64.sum(axis=-1, keepdims=True)
    return t64, rho, float(np.max(np.abs(t32 - t64) / (U * rho))), av32, av64


def hold_one_step(st, av, shadow, tag):
    """The one-step bar (module docstring) on a GPU step (st, av) against shadow = one_step_oracle(...) of the state before
    it: (worst |gpu - f64| in u rho, |av - av64|)."""
    t64, rho, e32, av32, av64 = shadow
    e = float(np.max(np.abs(st - t64) / (U * rho)))
    assert e <= 8.0 and e <= 2.0 * e32 + 1.0, (tag, e, e32)
    eav = abs(av - av64)
    assert eav <= 2.0 * abs(av32 - av64) + 4 * U, (tag, av, av32, av64)
    return e, eav


def _one_gpu_step(L, p, ob, x, V=None, variant=None):
    with L.Lattice(p, ob, x) as lat:
        lat.set_option("time_block", 1)
        if V is not None:
            lat.set_option("vector_width", V)
        if variant is not None:
            lat.set_option("kernel_variant", variant)
        av = float(lat.run(1)[0])
        assert lat.info("engine_last") == 1 and lat.info("time_block_active") == 1
        return av, lat.read_state()


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,seed,kind_smooth,kind_refusing", SHADOW_CASES)
@pytest.mark.parametrize("point", list(PARAM_GRID))
def test_one_step_kernel_against_double_oracle(gpu, O, oracle, point, nx, ny, seed, kind_smooth, kind_refusing):
    """20 steps of the one-step kernel, each from the GPU's own previous state, shadowed by the oracle in double and in
    float from that same state (so that no guard decision can flip on earlier rounding).  All 20 steps with the default
    kernel; at steps 1, 2, the first that refuses and 20 also vector widths 1 / 2 / 4, kernel_variant 0 / 1 / 7 (IEEE,
    fast reciprocal and root, nontemporal) and 8 / 9 (the reference's form of the speed sum).  Bars in the module
    docstring; step averages of both speed forms within twice the float oracle's error + 4 u (|u| is O(1) in lattice
    units where rho is not: a speed carries an absolute error of a few u)."""
    L = gpu
    o64 = O.Oracle("strict")
    kind = kind_refusing if point in REFUSING else kind_smooth
    ob, x = param_state(point, nx, ny, seed, kind)
    prm = _orc_param(O, point, nx, ny)
    p = _lparam(L, point, nx, ny)
    combos = [(V, var) for V, var in ((1, 0), (2, 1), (4, 7), (None, 8), (None, 9))
              if V is None or (nx % V == 0 and nx >= 2 * V)]
    worst = {"gpu": 0.0, "f32": 0.0, "av": 0.0}
    first_refusal, nref = None, 0
    for t in range(1, NSHADOW + 1):
        r = int(refused(prm.density, prm.accel, ob, x).sum())
        nref += r
        if r and first_refusal is None:
            first_refusal = t
        shadow = one_step_oracle(oracle, o64, prm, ob, x)  # the reference's float accelerate, for both flavours
        worst["f32"] = max(worst["f32"], shadow[2])
        runs = [(None, None)] + (combos if t in (1, 2, first_refusal, NSHADOW) else [])
        for V, variant in runs:
            av, st = _one_gpu_step(L, p, ob, x, V, variant)
            e, eav = hold_one_step(st, av, shadow, (point, t, V, variant))
            worst["gpu"] = max(worst["gpu"], e)
            worst["av"] = max(worst["av"], eav / U)
            if V is None and variant is None:
                nxt = st
        if t == 1:
            # the reference's call shape: the accelerate side effect on the caller's lattice, bit for bit
            acc = x.copy()
            oracle.accelerate(prm, acc, ob)
            c, tmp = x.copy(), np.empty_like(x)
            L.timestep_new2(p, c, tmp, ob)
            assert np.array_equal(_bits(c), _bits(acc)) and np.array_equal(_bits(tmp), _bits(nxt))
        x = nxt
    print(f"{point} {nx}x{ny} {kind}: refusals {nref} (first at step {first_refusal}); worst |gpu - f64| {worst['gpu']:.2f} u rho,"
          f" float oracle {worst['f32']:.2f} u rho; worst step average {worst['av']:.2f} u")
    if kind == "guard" or point in REFUSING:
        assert nref > 0 and first_refusal is not None
    # the derived quantities on the GPU's final state, against the oracle on that state
    with L.Lattice(p, ob, x) as lat:
        avv, re, fs, mass = lat.av_velocity(), lat.reynolds(), lat.final_state(), lat.total_density()
    x64 = x.astype(np.float64)
    av_o = o64.av_velocity(prm, x64, ob)
    re_o = o64.reynolds(prm, x64, ob)
    assert abs(avv - av_o) <= 1e-5 * av_o + 8 * U, (avv, av_o)
    assert abs(re - re_o) <= (1e-5 + 8 * U / av_o) * re_o, (re, re_o)
    fo = o64.final_state(prm, x64, ob)
    assert np.all(np.abs(fs - fo) <= 2e-6 * np.abs(fo) + 8 * U), float(np.max(np.abs(fs - fo)))
    # a cell's density is summed in float, f0 .. f8 in order, the cells in double (lbm_derive): that sum exactly, up to
    # the order of the double additions; and within the 8 u rho a float sum of nine terms may carry of the exact one
    rho32 = x[..., 0].copy()
    for k in range(1, 9):
        rho32 = rho32 + x[..., k]
    assert abs(mass - float(rho32.astype(np.float64).sum())) <= 1e-12 * mass
    assert abs(mass - float(x64.sum())) <= 8 * U * mass
    blocked = ob.astype(bool)
    assert blocked.any()
    assert np.all(fs[blocked][:, :3] == 0) and np.all(fs[blocked][:, 3] == np.float32(p.density) * ONE_THIRD)


# ----------------------------------------------------------------------------------------------------------- GPU: engines
def _tile(t):
    return ("regtile", t[0] * 10 + t[1])


# (one-row slabs: copy only, peer-to-peer halos need two rows per slab; wave_cols 2: lbm_wave<8> only at these widths)
# id -> (nx, ny, steps per run (the 'K' of split runs [K+1, K, 3]), options, info that must hold after, Lattice kwargs)
ENGINES = {
    "sweep2": (128, 64, 2, [("time_block", 2), ("engine", 1)], {"time_block_active": 2, "engine_last": 1}, {}),
    "march": (256, 64, 4, [("march_kernel", 0), ("time_block", 4)], {"time_block_active": 4, "march_kernel": 0}, {}),
    "wave4": (256, 64, 4, [("march_kernel", 1), ("time_block", 4)], {"time_block_active": 4, "march_kernel": 1}, {}),
    "wave6": (256, 64, 6, [("march_kernel", 1), ("time_block", 6)], {"time_block_active": 6, "march_kernel": 1}, {}),
    "wave8": (256, 64, 8, [("march_kernel", 1), ("time_block", 8)], {"time_block_active": 8, "march_kernel": 1}, {}),
    "wave8_cols2": (256, 64, 8, [("march_kernel", 1), ("time_block", 8), ("wave_cols", 2)],
                    {"time_block_active": 8, "march_kernel": 1, "wave_cols_active": 2}, {}),
    "regtile": (128, 128, 7, [], {"engine_last": 3}, {}),
    "regtile_8x4": (256, 256, 7, [_tile((8, 4)), ("engine", 3)], {"engine_last": 3}, {}),
    "regtile_4x2": (128, 16, 7, [_tile((4, 2)), ("engine", 3)], {"engine_last": 3}, {}),
    "regtile_async_16x2": (256, 256, 7, [_tile((16, 2)), ("regtile_async", 1), ("engine", 3)],
                           {"engine_last": 3, "regtile_async": 1}, {}),
    "regtile_sync_8x2": (128, 16, 7, [_tile((8, 2)), ("regtile_async", 0), ("engine", 3)],
                         {"engine_last": 3, "regtile_async": 0}, {}),
    "regtile_ieee": (128, 128, 7, [("kernel_variant", 0), ("engine", 3)], {"engine_last": 3, "kernel_variant": 0}, {}),
    "slabs_inside_copy": (64, 40, 3, [("engine", 1)], {"engine_last": 1}, {"nslabs": 3, "exchange": "copy"}),
    "slabs_first_row_p2p": (64, 12, 3, [("engine", 1)], {"engine_last": 1}, {"nslabs": 6, "exchange": "p2p"}),
    "slabs_one_row_copy": (64, 8, 3, [("engine", 1)], {"engine_last": 1}, {"nslabs": 8, "exchange": "copy"}),
    "slabs_first_row_copy": (64, 12, 3, [("engine", 1)], {"engine_last": 1}, {"nslabs": 6, "exchange": "copy"}),
    "regtile_slabs_copy": (128, 128, 7, [], {"engine_last": 3, "resident_fallback": 0}, {"nslabs": 2, "exchange": "copy"}),
    "regtile_slabs_p2p": (192, 96, 7, [], {"engine_last": 3, "resident_fallback": 0}, {"nslabs": 3, "exchange": "p2p"}),
    "rccl_ring_of_one": (128, 64, 2, [], {"exchange": "rccl", "time_block_active": 2}, {"rccl": True}),
}
# each engine once in the refusal regime (from rest) and once at another grid point (guard state: every kind of cell at step 1)
_OTHER = [pt for pt in PARAM_GRID if pt != "refusal"]
ENGINE_CASES = ([(e, "refusal", "rest") for e in ENGINES]
                + [(e, _OTHER[i % len(_OTHER)], "guard") for i, e in enumerate(ENGINES)])


@pytest.mark.gpu
@pytest.mark.parametrize("engine,point,kind", ENGINE_CASES)
def test_engine_equals_one_step_kernel_on_the_grid(gpu, O, oracle, monkeypatch, engine, point, kind):
    """Every multi-step engine against the one-step kernel at grid points and while the accelerate guard refuses part of
    row ny-2 at write time (steps >= 2 inside the engines' passes): split runs [K+1, K, 3], bit-identical lattice, av_vels
    within summation order; the info keys say the engine asked for really ran (a fall-back must not pass)."""
    L = gpu
    nx, ny, K, options, want, kw = ENGINES[engine]
    runs = [K + 1, K, 3]
    ob, cells = param_state(point, nx, ny, 40 + len(engine), kind)
    p = _lparam(L, point, nx, ny)
    counts = _count_refusals(oracle, _orc_param(O, point, nx, ny), ob, cells, sum(runs))
    if kind == "guard":
        assert counts[0] >= 5
    if point in REFUSING:
        assert sum(counts[1:]) > 0, counts               # refused at write time, inside the engines' passes
    with L.Lattice(p, ob, cells) as a:
        a.set_option("time_block", 1)
        for key, v in options:
            if key == "kernel_variant":                  # (the same arithmetic on both sides)
                a.set_option(key, v)
        av_a = np.concatenate([a.run(n) for n in runs])
        assert a.info("engine_last") == 1
        st_a = a.read_state()
    if kw.get("rccl"):
        monkeypatch.setenv("LBM_FORCE_EXCHANGE", "1")
        lat_kw = dict(rank=0, nranks=1, device=0, unique_id=L.rccl_unique_id(), exchange=L.EXCHANGE_RCCL)
    elif kw:
        ex = L.EXCHANGE_COPY if kw["exchange"] == "copy" else L.EXCHANGE_P2P
        lat_kw = dict(nslabs=kw["nslabs"], devices=[0] * kw["nslabs"], exchange=ex)
    else:
        lat_kw = {}
    with L.Lattice(p, ob, cells, **lat_kw) as b:
        for key, v in options:
            b.set_option(key, v)
        av_b = np.concatenate([b.run(n) for n in runs])
        for key, v in want.items():
            if key == "exchange":
                v = {"rccl": L.EXCHANGE_RCCL}[v]
            assert b.info(key) == v, (engine, key, b.info(key))
        st_b = b.read_state()
    assert np.array_equal(_bits(st_a), _bits(st_b)), engine
    assert np.allclose(av_a, av_b, rtol=ENGINE_AV_RTOL, atol=0), engine


@pytest.mark.gpu
@pytest.mark.parametrize("point,nslabs", [("stability_edge", 1), ("refusal", 1), ("light_fluid", 2), ("under_relaxed", 2)])
def test_register_tile_snapshots_away_from_the_decks(gpu, point, nslabs):
    """lbm_run_sampled with the register tiles (snapshots written from inside the kernel, the density reaching them
    bit-packed through LDS) at densities other than 0.1: snapshot j equals lbm_final_state after (j+1) every steps of
    separate runs, bit for bit; a blocked cell's pressure is float32(density) x float32(1/3) exactly."""
    L = gpu
    nx, ny, nsteps, every = 128, 128, 12, 4
    ob, cells = param_state(point, nx, ny, 51, "rest" if point in REFUSING else "perturbed")
    p = _lparam(L, point, nx, ny)
    kw = dict(nslabs=nslabs, devices=[0] * nslabs, exchange=L.EXCHANGE_P2P) if nslabs > 1 else {}
    snaps, avs = [], []
    with L.Lattice(p, ob, cells, **kw) as lat:
        for _ in range(nsteps // every):
            avs.append(lat.run(every))
            snaps.append(lat.final_state())
        st0 = lat.read_state()
    with L.Lattice(p, ob, cells, **kw) as lat:
        av, fields = lat.run_sampled(nsteps, every)
        assert lat.info("engine_last") == 3 and lat.info("samples_in_kernel") == 1
        st = lat.read_state()
    assert np.array_equal(_bits(fields), _bits(np.stack(snaps)))
    assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(av), _bits(np.concatenate(avs)))
    blocked = ob.astype(bool)
    assert np.all(fields[:, blocked, 3] == np.float32(p.density) * ONE_THIRD)
    assert np.all(fields[:, blocked, :3] == 0)


# ----------------------------------------------------------------------------------------------------------- GPU: whole runs
# (point, lattice, slabs); lattice: a shipped deck's obstacles, or "random" (256 x 256, 10 % random obstacles)
WHOLE_RUNS = ([(pt, "128x256", 1) for pt in SMOOTH] + [(pt, "random", 2) for pt in SMOOTH]
              + [("under_relaxed", "1024x1024", 4), ("omega_one", "1024x1024", 1)])
# the CLI deck: a dense fluid that stays smooth over a whole run (density 0.37 as at the stability edge, gentler accel and omega)
CLI_PARAMS = (0.37, 0.01, 1.9)
WHOLE_STEPS = 200


def _whole_run_case(O, point, lattice):
    if lattice == "random":
        nx = ny = 256
        ob = (np.random.default_rng(61).random((ny, nx)) < 0.1).astype(np.int32)
    else:
        nx, ny = (int(v) for v in lattice.split("x"))
        ob = O.read_obstacles(deck_paths(lattice)[1], nx, ny)
    return nx, ny, ob


def _double_and_float(O, oracle, prm, ob, cells0, nsteps):
    """(f64 lattice, f64 av_vels, f32 lattice, f32 av_vels) of nsteps from the float lattice cells0."""
    c64 = cells0.astype(np.float64)
    av64 = O.Oracle("strict").run(prm, c64, ob, nsteps)
    c32 = cells0.copy()
    av32 = oracle.run(prm, c32, ob, nsteps)
    return c64, av64, c32, av32


@pytest.mark.gpu
@pytest.mark.parametrize("point,lattice,nslabs", WHOLE_RUNS)
def test_whole_runs_against_double_oracle(gpu, O, oracle, point, lattice, nslabs):
    """200 steps from rest with the default engine (register tiles: across slabs where nslabs > 1) against the double
    oracle from the same float initial lattice: max |gpu - f64| <= 4 x the float oracle's max deviation + 8 u of the
    lattice maximum, the same for av_vels (u of the largest step average)."""
    L = gpu
    nx, ny, ob = _whole_run_case(O, point, lattice)
    prm = _orc_param(O, point, nx, ny, WHOLE_STEPS)
    cells0 = oracle.init_cells(prm, np.float32)
    assert sum(_count_refusals(oracle, prm, ob, cells0, 1)) == 0
    c64, av64, c32, av32 = _double_and_float(O, oracle, prm, ob, cells0, WHOLE_STEPS)
    assert int(refused(prm.density, prm.accel, ob, c32).sum()) == 0
    p = _lparam(L, point, nx, ny, WHOLE_STEPS)
    kw = dict(nslabs=nslabs, devices=[0] * nslabs, exchange=L.EXCHANGE_P2P) if nslabs > 1 else {}
    with L.Lattice(p, ob, cells0, **kw) as lat:
        av = lat.run(WHOLE_STEPS)
        assert lat.info("engine_last") == 3
        st = lat.read_state()
    d32 = float(np.max(np.abs(c32 - c64)))
    dg = float(np.max(np.abs(st - c64)))
    a32 = float(np.max(np.abs(av32 - av64)))
    ag = float(np.max(np.abs(av - av64)))
    print(f"{point} {lattice} x{nslabs}: lattice |gpu - f64| {dg:.3e}, |f32 - f64| {d32:.3e};"
          f" av_vels {ag:.3e}, {a32:.3e}")
    assert dg <= 4 * d32 + 8 * U * float(np.max(np.abs(c64))), (dg, d32)
    assert ag <= 4 * a32 + 8 * U * float(np.max(av64)), (ag, a32)


@pytest.mark.gpu
def test_cli_on_a_generated_deck_away_from_the_decks(gpu, O, oracle, tmp_path):
    """./d2q9-bgk on a deck with non-default density, accel and omega (tools/make_deck.py): the project's checker passes
    it against the double oracle's files, and the pressures and av_vels meet the whole-run bar above.  No refusal on
    the oracle side over the run."""
    import check_results as CR
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_deck
    density, accel, omega = CLI_PARAMS
    nx, ny, nsteps = 256, 128, WHOLE_STEPS
    pf, of, _ = make_deck.write_deck(nx, ny, nsteps, outdir=str(tmp_path), porous=0.05, density=density, accel=accel,
                                     omega=omega)
    r = subprocess.run([os.path.join(ROOT, "d2q9-bgk"), pf, of], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    prm = O.read_params(pf)
    assert (prm.density, prm.accel, prm.omega) == (density, accel, omega)
    prm = O.OrcParam(nx, ny, nsteps, 10, *(float(np.float32(v)) for v in CLI_PARAMS))
    ob = O.read_obstacles(of, nx, ny)
    cells0 = oracle.init_cells(prm, np.float32)
    assert sum(_count_refusals(oracle, prm, ob, cells0, nsteps)) == 0
    c64, av64, c32, av32 = _double_and_float(O, oracle, prm, ob, cells0, nsteps)
    p64 = O.Oracle("strict").final_state(prm, c64, ob)[:, :, 3]
    p32 = oracle.final_state(prm, c32, ob)[:, :, 3]
    ra, rf = tmp_path / "ref_av_vels.dat", tmp_path / "ref_final_state.dat"
    ra.write_text(O.format_av_vels(av64))
    with open(rf, "w") as f:
        for jj in range(ny):
            f.write("".join("%d %d %.12E %.12E %.12E %.12E %d\n" % (ii, jj, 0.0, 0.0, 0.0, p64[jj, ii], ob[jj, ii])
                            for ii in range(nx)))
    ok, a, fdev = CR.compare(str(ra), str(rf), str(tmp_path / "av_vels.dat"), str(tmp_path / "final_state.dat"),
                             out=open(os.devnull, "w"))
    assert ok, (a, fdev)
    av = np.loadtxt(tmp_path / "av_vels.dat", usecols=[1])
    pr = np.loadtxt(tmp_path / "final_state.dat", usecols=[5]).reshape(ny, nx)
    assert av.shape == (nsteps,)
    assert np.max(np.abs(pr - p64)) <= 4 * np.max(np.abs(p32 - p64)) + 8 * U * np.max(p64)
    assert np.max(np.abs(av - av64)) <= 4 * np.max(np.abs(av32 - av64)) + 8 * U * np.max(av64)
