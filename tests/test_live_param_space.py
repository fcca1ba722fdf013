"""lbm_set_obstacles and lbm_write_state away from the shipped decks: at every point of PARAM_GRID
(tests/golden/make_golden.py), on the smallest shapes the parameter-space files use for each engine.

Until this module every live-input test ran at density 0.1, omega 1.85 and accel 0.01: the refill values density * 4.f / 9.f,
density / 9.f and density / 36.f were never read back at another density, and no refilled cell had met the accelerate guard.

  * ENGINES: the one-step kernel and time_block 2 at 33 x 20 (narrower than a two-step tile: the library takes the one-step
    kernel there, asserted), the two-step kernel at 128 x 64 where it does run, one register tiling at 128 x 16, lbm_wave<4>
    and lbm_wave<8> with two columns per lane at 256 x 64 in chunks of 24, 24 and 16 rows.
  * Per case, one LIVE context: run(n1), n1 odd; set_obstacles(B, LBM_REFILL_REST); run_probes(n2, 1); write_state(W);
    run(n3).  B refills cells in rows 0, ny-1 and the accelerate row ny-2, blocks others, and marks blocked cells with 2 and
    -1 as well as 1.  The probe set holds refilled cells, newly blocked cells and cells at random.
  * Behind the refill: read_state is S' = the state before the call with rest_values(density) -- the C expressions in float --
    in the refilled cells, bit for bit; refilled_cells, fluid_cells and obstacle_updates against numpy.
  * LIVE equals FRESH bit for bit: a context lbm_create makes from (B, S') under the same options and probes for the probe
    run, from (B, W) for the last run.
  * The oracle, piecewise: for each piece a one-step context (engine 1, time_block 1) is created from the piece's start --
    (A, S0), (B, S'), (B, W), the map swapped and the refill applied in numpy -- and stepped one step at a time, every step
    from its own previous state against the oracle in double and in strict float at the one-step bar of
    tests/test_param_space.py (hold_one_step: 8 u rho, and twice the float oracle's error + 1 u rho).  LIVE's lattice after
    the piece is that context's bit for bit, its av_vels within ENGINE_AV_RTOL, its probes the bits of final_state.
  * At "refusal" and "light_fluid" the guard refuses cells of row ny-2 in the step right behind the refill (asserted without
    a GPU on the float oracle alone) and no refilled cell is among them: at rest f3 = rho/9 > a1 = rho a/9 and
    f6 = f7 = rho/36 > a2 = rho a/36 whenever a < 1, and a <= 0.5 on the grid.

No GPU: the maps, probe sets and step counts are what they say, every piece stays tame on the float oracle (fluid
rho >= 0.25 rho0, |f| <= rho0) and the refusing points refuse behind the refill."""
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN
from test_live_inputs import REST, _same, refilled, rest_values, s_prime
from test_observer_param_space import EXTRA, _wave_opts
from test_param_space import ENGINE_AV_RTOL, ENGINES as GRID_ENGINES, REFUSING, _lparam, _orc_param, hold_one_step, one_step_oracle

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden import PARAM_GRID, accel_weights, param_state, refused  # noqa: E402

SEED = 71
_ONE = [("engine", 1), ("time_block", 1)]
# id -> (nx, ny, steps per pass, options, info that must hold after the first run)
ENGINES = {
    "tb1": (33, 20, 1, _ONE, {"engine_last": 1, "time_block_active": 1}),
    "tb2_33x20": (33, 20, 1, [("engine", 1), ("time_block", 2)], {"engine_last": 1, "time_block": 2, "time_block_active": 1}),
    "tb2": GRID_ENGINES["sweep2"][:5],
    "regtile_4x2": GRID_ENGINES["regtile_4x2"][:5],
    "wave4_rows24": (256, 64, 4, _wave_opts(4, 1, 24),
                     {"engine_last": 1, "time_block_active": 4, "march_kernel": 1, "wave_cols_active": 1, "wave_rows": 24}),
    "wave8_cols2_rows24": EXTRA["wave8_cols2_ragged"][:5],
}
CASES = [(e, pt) for e in ENGINES for pt in PARAM_GRID]
IN_KERNEL = {"regtile_4x2": "probes_in_kernel", "wave4_rows24": "probes_in_wave", "wave8_cols2_rows24": "probes_in_wave"}


def _steps(K):
    """(n1, n2, n3): n1 odd, every piece at least one full pass and a remainder shorter than a pass where K > 1."""
    return (K + 1 if K % 2 == 0 else K + 2), K + (3 if K == 2 else 2), K + 1


_CASE = {}


def _case(engine, point):
    """dict(A, B, S0, W, xy, steps): A = param_state's map ("guard" kind at "refusal": every kind of guard cell in row
    ny-2, cells 8 and 9 blocked and thinner than a1 / a2) with obstacles dashed into rows 0, ny-1 and ny-2; B = A with 3 %
    of the cells flipped at random, then every other dashed obstacle and guard cell 8 opened, guard cell 6 and cells of rows
    1 and ny-2 blocked, and the blocked cells marked 1, 2 or -1 in turn."""
    nx, ny, K = ENGINES[engine][:3]
    key = (nx, ny, K, point)
    if key not in _CASE:
        kind = "guard" if point == "refusal" else "rest" if point in REFUSING else "perturbed"
        A, S0 = param_state(point, nx, ny, SEED, kind)
        A[0, 2::7] = 1
        A[ny - 1, 3::7] = 1
        A[ny - 2, 12::7] = 1
        rng = np.random.default_rng(SEED + 1)
        B = np.where(rng.random((ny, nx)) < 0.03, 1 - A, A).astype(np.int32)
        B[0, 2::7], B[ny - 1, 3::7], B[ny - 2, 12::7] = A[0, 2::7], A[ny - 1, 3::7], A[ny - 2, 12::7]
        B[0, 2::14] = 0
        B[ny - 1, 3::14] = 0
        B[ny - 2, 12::14] = 0
        B[ny - 2, 8] = 0 if A[ny - 2, 8] else B[ny - 2, 8]
        B[ny - 2, 6] = 1
        B[ny - 2, 15::14] = 1
        B[1, 5::9] = 1
        marks = np.array([1, 2, -1], np.int32)
        B[B != 0] = marks[np.arange(int((B != 0).sum())) % 3]
        W = param_state(point, nx, ny, SEED + 2, "perturbed")[1]
        m = refilled(A, B)
        cells = set()
        for r in (0, ny - 1, ny - 2):
            cells |= {(int(c), r) for c in np.flatnonzero(m[r])[:3]}
        turned = np.argwhere((A == 0) & (B != 0))
        cells |= {(int(c), int(r)) for r, c in turned[:: max(len(turned) // 4, 1)][:4]} | {(6, ny - 2)}
        cells |= {(int(c), int(r)) for c, r in zip(rng.integers(0, nx, 8), rng.integers(0, ny, 8))}
        xy = np.array(sorted(cells), dtype=np.int32)
        xy = xy[rng.permutation(len(xy))]
        for a in (A, B, S0, W, xy):
            a.setflags(write=False)
        _CASE[key] = dict(A=A, B=B, S0=S0, W=W, xy=xy, steps=_steps(K))
    return _CASE[key]


def _tame(x, ob, rho0):
    rho = x.astype(np.float64).sum(axis=-1)[ob == 0]
    return bool(np.all(np.isfinite(x))) and float(rho.min()) >= 0.25 * rho0 and float(np.abs(x).max()) <= rho0


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_the_table_holds_every_engine_at_every_point():
    assert len(PARAM_GRID) == 6 and len(CASES) == len(set(CASES)) == 6 * len(ENGINES)
    shapes = {e: ENGINES[e][:3] for e in ENGINES}
    assert shapes == {"tb1": (33, 20, 1), "tb2_33x20": (33, 20, 1), "tb2": (128, 64, 2), "regtile_4x2": (128, 16, 7),
                      "wave4_rows24": (256, 64, 4), "wave8_cols2_rows24": (256, 64, 8)}
    for e in ("wave4_rows24", "wave8_cols2_rows24"):
        assert dict(ENGINES[e][3])["wave_rows"] == 24 and ENGINES[e][4]["march_kernel"] == 1
    assert dict(ENGINES["wave8_cols2_rows24"][3])["wave_cols"] == 2
    assert dict(ENGINES["regtile_4x2"][3]) == {"regtile": 42, "engine": 3}
    for K in (1, 2, 4, 7, 8):
        n1, n2, n3 = _steps(K)
        assert n1 % 2 == 1 and min(n1, n2, n3) > K and (K == 1 or all(n % K for n in (n1, n2, n3)))


@pytest.mark.parametrize("engine,point", CASES)
def test_case_holds_what_it_claims(O, oracle, engine, point):
    nx, ny, K = ENGINES[engine][:3]
    c = _case(engine, point)
    A, B, S0, W, xy = c["A"], c["B"], c["S0"], c["W"], c["xy"]
    n1, n2, n3 = c["steps"]
    m = refilled(A, B)
    for r in (0, ny - 1, ny - 2):
        assert m[r].sum() >= 2, r
    assert ((A == 0) & (B != 0)).sum() > 0 and set(np.unique(B)) == {-1, 0, 1, 2}
    assert ((A[ny - 2] == 0) & (B[ny - 2] != 0)).any()
    assert (A == 0).sum() != (B == 0).sum()
    probed = np.zeros((ny, nx), bool)
    probed[xy[:, 1], xy[:, 0]] = True
    assert len({tuple(q) for q in xy}) == len(xy)
    for r in (0, ny - 1, ny - 2):
        assert (probed & m)[r].any(), r
    assert (probed & (A == 0) & (B != 0)).any() and (probed & (A == 0) & (B == 0)).any()
    # the float oracle, piecewise: tame, and at the refusing points refusing right behind the refill
    prm = _orc_param(O, point, nx, ny)
    rho0 = float(prm.density)
    Ab, Bb = (A != 0).astype(np.int32), (B != 0).astype(np.int32)
    x = S0.copy()
    oracle.run(prm, x, Ab, n1)
    assert _tame(x, Ab, rho0)
    x = s_prime(x, A, B, REST, prm.density)
    assert np.all(x[m] == rest_values(prm.density))
    ref = refused(prm.density, prm.accel, Bb, x)
    a1, a2 = accel_weights(prm.density, prm.accel)
    w = rest_values(prm.density)
    assert w[3] - a1 > 0 and w[6] - a2 > 0 and w[7] - a2 > 0          # a refilled cell passes the guard, at every point
    assert not (ref & m[ny - 2]).any()
    if point in REFUSING:
        assert ref.sum() > 0 and ((Bb[ny - 2] == 0) & ~ref).any(), (engine, point, int(ref.sum()))
    oracle.run(prm, x, Bb, n2)
    assert _tame(x, Bb, rho0)
    x = W.copy()
    oracle.run(prm, x, Bb, n3)
    assert _tame(x, Bb, rho0)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _open(L, p, ob, cells, options, xy):
    lat = L.Lattice(p, ob, cells)
    for k, v in options:
        lat.set_option(k, v)
    lat.set_probes(xy)
    return lat


def _one_step_piece(L, O, oracle, p, prm, ob, start, n, tag, worst):
    """The piece's reference: a one-step context made from (ob, start), n x run(1), every step held to the oracle from its
    own previous state.  (av_vels[n], final_state per step, the last lattice)"""
    o64 = O.Oracle("strict")
    obb = (np.asarray(ob) != 0).astype(np.int32)
    av, X, x = [], [], start
    with _open(L, p, ob, start, _ONE, None) as lat:
        for t in range(1, n + 1):
            shadow = one_step_oracle(oracle, o64, prm, obb, x)
            a = lat.run(1)
            assert lat.info("engine_last") == 1 and lat.info("time_block_active") == 1
            x = lat.read_state()
            e, _ = hold_one_step(x, float(a[0]), shadow, (tag, t))
            worst[0] = max(worst[0], e / min(8.0, 2.0 * shadow[2] + 1.0))
            av.append(a)
            X.append(lat.final_state())
    return np.concatenate(av), np.stack(X), x


def _engine_keys(lat):
    return {k: int(lat.info(k)) for k in ("engine_last", "time_block_active", "march_kernel", "wave_cols_active", "wave_rows", "regtile")}


@pytest.mark.gpu
@pytest.mark.parametrize("engine,point", CASES)
def test_live_inputs_on_the_grid(gpu, O, oracle, engine, point):
    L = gpu
    t0 = time.time()
    nx, ny, K, options, want = ENGINES[engine]
    c = _case(engine, point)
    A, B, S0, W, xy = c["A"], c["B"], c["S0"], c["W"], c["xy"]
    n1, n2, n3 = c["steps"]
    p, prm = _lparam(L, point, nx, ny), _orc_param(O, point, nx, ny)
    m = refilled(A, B)
    worst = [0.0]
    tag = (engine, point)
    with _open(L, p, A, S0, options, xy) as live:
        # ---- piece 1
        av1 = live.run(n1)
        for k, v in want.items():
            assert live.info(k) == v, (tag, k, live.info(k))
        keys = _engine_keys(live)
        S = live.read_state()
        av_r, _, S_r = _one_step_piece(L, O, oracle, p, prm, A, S0, n1, tag + (1,), worst)
        assert _same(S, S_r) and np.allclose(av1, av_r, rtol=ENGINE_AV_RTOL, atol=0), tag
        # ---- the map, with the refill
        live.set_obstacles(B, REST)
        Sp = s_prime(S, A, B, REST, p.density)
        back = live.read_state()
        assert np.all(back[m] == rest_values(p.density)) and int(m.sum()) > 0, tag
        assert _same(back, Sp), tag
        assert live.info("refilled_cells") == int(m.sum()) and live.info("obstacle_updates") == 1
        assert live.info("fluid_cells") == int((B == 0).sum())
        ref = refused(p.density, p.accel, B, Sp)
        assert not (ref & m[ny - 2]).any(), tag
        if point in REFUSING:
            assert ref.sum() > 0, tag
        # ---- piece 2: probes behind the new map
        av2, pr2 = live.run_probes(n2, 1)
        if engine in IN_KERNEL:
            assert live.info(IN_KERNEL[engine]) == 1, tag
        assert _engine_keys(live) == keys, tag
        S2 = live.read_state()
        with _open(L, p, B, Sp, options, xy) as fresh:
            av_f, pr_f = fresh.run_probes(n2, 1)
            assert _engine_keys(fresh) == keys, tag
            assert _same(av2, av_f) and _same(pr2, pr_f) and _same(S2, fresh.read_state()), tag
        av_r, X_r, S_r = _one_step_piece(L, O, oracle, p, prm, B, Sp, n2, tag + (2,), worst)
        assert _same(S2, S_r) and np.allclose(av2, av_r, rtol=ENGINE_AV_RTOL, atol=0), tag
        assert _same(pr2, X_r[:, xy[:, 1], xy[:, 0], :]), tag
        # ---- piece 3: a written lattice under the new map
        live.write_state(W)
        assert _same(live.read_state(), W), tag
        av3 = live.run(n3)
        assert _engine_keys(live) == keys and live.info("obstacle_updates") == 1, tag
        S3 = live.read_state()
        with _open(L, p, B, W, options, xy) as fresh:
            av_f = fresh.run(n3)
            assert _same(av3, av_f) and _same(S3, fresh.read_state()), tag
        av_r, _, S_r = _one_step_piece(L, O, oracle, p, prm, B, W, n3, tag + (3,), worst)
        assert _same(S3, S_r) and np.allclose(av3, av_r, rtol=ENGINE_AV_RTOL, atol=0), tag
    print(f"{engine} {point}: steps {n1}+{n2}+{n3}, {int(m.sum())} cells refilled, {int(ref.sum())} refused behind the refill;"
          f" one-step pieces at {worst[0]:.2f} of their bar from double; live = fresh = one-step bit for bit; {time.time() - t0:.2f} s")
