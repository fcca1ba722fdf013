"""lbm_run_stats away from the shipped decks: every path of tests/test_observer_param_space.py (PATHS, with the info keys
that say which engine ran) at that file's points -- "refusal", "stability_edge", "light_fluid" and one of "under_relaxed" /
"omega_one" in turn -- and at one point more on every path, "thirds" = (0.3, 0.01, 1.85).

Why "thirds".  A blocked cell's pressure, and the p0 that stats_products subtracts, is density * (1.f / 3.f) in float: the
kernels and the reference (c_sq = 1.f / 3.f) multiply.  At densities 0.1 and 0.37 of PARAM_GRID that float and
float(density) / 3.f are the same float; at 0.02 they are one ulp apart (test_which_grid_densities_can_tell_the_two_forms_of_
p0_apart), but 0.02 is "light_fluid" alone, which runs from rest for 16 steps at most before the lattice blows up.  So no
smooth, perturbed run of the grid can tell a kernel that divides from one that multiplies.  At 0.3 the two differ by one ulp,
which changes the bits of every (p - p0)^2 and makes a blocked cell's float 7 non-zero
(test_thirds_tells_the_two_forms_of_p0_and_the_densities_apart).
The density itself reaches p0 through WaveArgs::density and the argument of launch_cell_add: a site that kept 0.1 passes
every stats test at the control point, and none of the four densities here.  "thirds" is not a point of PARAM_GRID and has
no golden file: its state is param_state's "perturbed" recipe from the local triple (thirds_state; held to param_state bit
for bit at a grid point).  On the strict float oracle, seed 7, it stays far inside the tameness condition over 30 steps
(fluid rho >= 0.91 rho0 -- the least, on 200 x 72, is 0.9147 -- |f| <= 0.50 rho0, nothing refused:
test_case_holds_what_it_claims).

Periods: the mean period `me` of the older file's _periods (a sample step below level K, one at level K, one among the
left-over steps; m = n // me >= 3 and no power of two), and on the lbm_wave paths every = 1 as well, where every level of every
pass is a sample.

The reference is the older file's: the one-step kernel, one step at a time, S_t = read_state and X_t = final_state, X_t held
to the double oracle's final_state of S_t at every step (2e-6 |fo| + 8 x 2^-24).  Per case and period three calls, each on a
fresh context under the path's options: lbm_run, lbm_run_stats, lbm_run_mean.

  bits       stats_out = test_stats_run.stats_of(X[every - 1:n:every], p0), p0 = float32(density) * (float32(1) / float32(3))
  means      floats 0..3 = lbm_run_mean's bits
  blocked    a blocked cell reads exactly (0, 0, 0, p0', 0, 0, 0, 0), p0' the float sum of m copies of p0 over m
             (blocked_record: p0 itself wherever that sum does not round)
  lattice    lbm_run's bits, which are S_n's
  av_vels    lbm_run's bits on the register tiles and on lbm_wave; elsewhere within ENGINE_AV_RTOL (2e-6)
  info       the path's keys; stats_in_wave = 1 on the lbm_wave paths, 0 elsewhere; mean_in_kernel = 0

The second moments against an outside reference.  fo_j = the DOUBLE oracle's fields of S_t at the sample steps, d = fo.p - p0,
Q_j = (x x, y y, x y, d d) in float64, blocked cells 0.  The bound is _oracle_moment_bound's (tests/test_stats_run.py) with
the per-element dx the bar X_t is held to, dx = 2e-6 |fo| + 8 u (u = 2^-24), carried through each product,
    e_j = (2 |x| dx + dx^2, 2 |y| dy + dy^2, |x| dy + |y| dx + dx dy, 2 |d| dp + dp^2),
    |stats[4..7] - mean_j Q_j| <= bQ = mean_j e_j + m u mean_j |Q_j| + u |stats[4..7]|
(m - 1 float additions and the product's own rounding; the division), and exactly 0 in a blocked cell.

The variances.  V = (s4 - s0^2, s5 - s1^2, s6 - s0 s1, s7 - (s3 - p0)^2), formed in double from the eight floats as the header
says, against the population (co)variances of the fo_j: W = (mean xx - mx^2, mean yy - my^2, mean xy - mx my, mean dd - md^2)
with mx = mean_j fo.x and so on.  lbm_run_mean's bound holds s_k to the float64 mean of the X_j,
(m - 1) u sum_j |X_j| + u |s_k|, and X_j lies within dx_j of fo_j, so
    |s_k - m_k| <= bM_k = mean_j dx_j,k + (m - 1) u sum_j |X_j,k| + u |s_k|
and with s = m + (s - m):  |s_a s_b - m_a m_b| <= |m_a| bM_b + |m_b| bM_a + bM_a bM_b, hence
    |V_0 - W_0| <= bQ_4 + 2 |mx| bM_0 + bM_0^2                 (V_1 likewise)
    |V_2 - W_2| <= bQ_6 + |mx| bM_1 + |my| bM_0 + bM_0 bM_1
    |V_3 - W_3| <= bQ_7 + 2 |md| bM_3 + bM_3^2                 (s3 - p0 against md = mean p - p0: the same p0 on both sides)
plus 2^-50 (|s_4| + s_0^2) and its like for the three double operations (never visible).  Nothing in either bound is fitted
to the library: every term is a bar the suite already uses, or a rounding.  A blocked cell's first three variances are
exactly 0; its pressure variance is -(p0' - p0)^2 with p0' of blocked_record, which is 0 only where the float sum of m copies of
p0 does not round (at density 0.3, m = 3, it rounds).

Measured on one MI355X (printed by the tests; DESIGN.md section 4, "Stats on the grid"): the second moments at most 0.058 of
their bound, the variances at most 0.036 of theirs; 27.5 s for the 100 cases, beside tests/test_observer_param_space.py's
34.5 s for 80 in the same visit.  Found here: av_vels of lbm_run_stats one ulp from lbm_run's on the 16 x 2 and 8 x 2 tilings
(plain launches per piece; the pieces now run in lbm_run_observed's piece flavour), and a blocked cell's float 3 one ulp from
p0 where the sum of m copies of p0 rounds."""
import sys

import numpy as np
import pytest

import test_observer_param_space as OBS
from conftest import GOLDEN
from test_mean_run import mean_of
from test_observer_param_space import COMPULSORY, PATHS, ROTATED, U, _bits, _nsteps, _periods, _placement, _power_of_two, _trajectory
from test_param_space import ENGINE_AV_RTOL, REFUSING, _lparam, _orc_param
from test_stats_run import p0_of, stats_of

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden import EQ_WEIGHTS, PARAM_GRID, param_state  # noqa: E402

THIRDS = (0.3, 0.01, 1.85)
THIRDS_SEED = 7
THIRDS_STEPS = 30                        # the steps "thirds" is shown tame over; every run there is shorter
CONTROL_ACCEL = PARAM_GRID["control"][1]
CASES = list(OBS.CASES) + [(path, "thirds") for path in PATHS]


def _triple(point):
    return THIRDS if point == "thirds" else PARAM_GRID[point]


def p0_divided(density):
    """the other form: float(density) / 3.f"""
    return np.float32(density) / np.float32(3)


def blocked_record(p0, m):
    """What a blocked cell reads after m samples: every snapshot there is (0, 0, 0, p0), so floats 0..2 and 4..7 are +0 and
    float 3 is the header's float sum of m copies of p0, divided by m -- p0 itself where that sum does not round (m = 1, 2, 4
    always), else within an ulp or two of it."""
    assert type(p0) is np.float32
    s = np.float32(0)
    for _ in range(m):
        s = s + p0
    return np.array([0, 0, 0, s / np.float32(m), 0, 0, 0, 0], dtype=np.float32)


def thirds_state(triple, nx, ny, seed, blocked=0.1):
    """param_state's "perturbed" recipe (tests/golden/make_golden.py) from a triple of one's own."""
    rng = np.random.default_rng(seed)
    ob = (rng.random((ny, nx)) < blocked).astype(np.int32)
    eq = np.float32(triple[0]) * EQ_WEIGHTS
    return ob, (eq * (1.0 + 0.2 * (rng.random((ny, nx, 9)) - 0.5))).astype(np.float32)


def _lib_param(L, point, nx, ny):
    return _lparam(L, point, nx, ny) if point != "thirds" else L.Param(nx, ny, 100, 10, *THIRDS)


def _oracle_param(O, point, nx, ny):
    if point != "thirds":
        return _orc_param(O, point, nx, ny)
    return O.OrcParam(nx, ny, 100, 10, *(float(np.float32(v)) for v in THIRDS))


_CASE = {}


def _case(path, point):
    """(nx, ny, K, nsteps, the mean period, state kind, obstacles, cells0, bodies, probes): the older file's case, and its like
    at "thirds" (bodies and probes only because that file's _open sets them)."""
    if (path, point) not in _CASE:
        if point != "thirds":
            nx, ny, K, n, periods, kind, ob, cells, body, xy = OBS._case(path, point)
        else:
            nx, ny, K = PATHS[path][:3]
            kind, n = "perturbed", _nsteps(K, point)
            periods = _periods(K, n)
            ob, cells = thirds_state(THIRDS, nx, ny, THIRDS_SEED)
            for a in (ob, cells):
                a.setflags(write=False)
            body, xy = OBS._bodies(ob), OBS._probes(path, ob)
        _CASE[(path, point)] = (nx, ny, K, n, periods[1], kind, ob, cells, body, xy)
    return _CASE[(path, point)]


def _everys(path, point):
    me = _case(path, point)[4]
    return (me, 1) if PATHS[path][6] == "wave" and me != 1 else (me,)


def _steps(O, oracle, path, point, nsteps):
    nx, ny, _, _, _, kind, ob, cells, _, _ = _case(path, point)
    start = (ob, cells, THIRDS) if point == "thirds" else None
    return _trajectory(O, oracle, nx, ny, point, kind, nsteps, start)


def _float_oracle_fields(oracle, prm, ob, cells, n):
    """X_t, t = 1..n, of the strict float oracle: (n, ny, nx, 4) float32"""
    a, b, out = cells.copy(), np.empty_like(cells), []
    for _ in range(n):
        oracle.timestep(prm, a, b, ob)
        a, b = b, a
        out.append(oracle.final_state(prm, a, ob).reshape(prm.ny, prm.nx, 4))
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_the_table_holds_every_path_at_every_compulsory_point_and_at_thirds():
    assert len(PATHS) == 20 and len(CASES) == len(set(CASES)) == 100
    for path in PATHS:
        for point in COMPULSORY + ("thirds",):
            assert (path, point) in CASES
        assert sum((path, point) in CASES for point in ROTATED) == 1
    assert "thirds" not in PARAM_GRID and THIRDS == (0.3, 0.01, 1.85)
    kinds = {PATHS[p][6] for p in PATHS}
    assert kinds == {"split", "wave", "tiles"}
    for path, point in CASES:
        nx, ny, K, n, me, kind, *_ = _case(path, point)
        assert nx <= 256 and ny <= 256 and n <= THIRDS_STEPS
        assert _everys(path, point) == ((me, 1) if PATHS[path][6] == "wave" else (me,))     # (me > 1 on every lbm_wave path)


def test_thirds_state_is_param_states_recipe():
    """thirds_state from a grid point's triple is param_state's "perturbed" state there, bit for bit."""
    for point, (nx, ny, seed) in (("stability_edge", (33, 20, 12)), ("light_fluid", (64, 40, 7))):
        ob, cells = param_state(point, nx, ny, seed, "perturbed")
        ob2, cells2 = thirds_state(PARAM_GRID[point], nx, ny, seed)
        assert np.array_equal(ob, ob2) and ob2.dtype == np.int32 and np.array_equal(_bits(cells), _bits(cells2))


def test_which_grid_densities_can_tell_the_two_forms_of_p0_apart():
    """float(d) * float(1/3) and float(d) / 3.f are one float at 0.1 and at 0.37; at 0.02 they differ by one ulp, but the
    points of that density run from rest for 16 steps at most.  That is why "thirds" exists: one ulp apart, and smooth."""
    assert sorted({v[0] for v in PARAM_GRID.values()}) == [0.02, 0.1, 0.37]
    for d in (0.1, 0.37):
        assert _bits(p0_of(d)) == _bits(p0_divided(d)), d
    assert {pt for pt, v in PARAM_GRID.items() if v[0] == 0.02} == {"light_fluid"} and "light_fluid" in REFUSING
    for d in (0.02, THIRDS[0]):
        a, b = p0_of(d), p0_divided(d)
        assert type(a) is type(b) is np.float32 and int(_bits(a)[0]) - int(_bits(b)[0]) == 1, (d, a, b)


@pytest.mark.parametrize("nx,ny", [(128, 64), (256, 64), (200, 72), (64, 40)])
def test_thirds_tells_the_two_forms_of_p0_and_the_densities_apart(O, oracle, nx, ny):
    """On the strict float oracle's fields at "thirds" over 30 steps: the oracle's blocked pressure is the multiplied p0 and not
    the divided one; every sample's (p - p0)^2 has other bits under density / 3.f, in every cell, and under density 0.1; so
    stats_of's floats 7 -- what the GPU is held to bit for bit -- differ in every blocked cell (from 0) and in 95 % of all
    cells at least (sums of terms that all differ may round alike: measured 0.984 and more)."""
    ob, cells = thirds_state(THIRDS, nx, ny, THIRDS_SEED)
    prm = O.OrcParam(nx, ny, 100, 10, *(float(np.float32(v)) for v in THIRDS))
    X = _float_oracle_fields(oracle, prm, ob, cells, THIRDS_STEPS)
    p0, p0d, p01 = p0_of(THIRDS[0]), p0_divided(THIRDS[0]), p0_of(0.1)
    blocked = ob != 0
    assert blocked.any() and np.all(_bits(X[:, blocked, 3]) == _bits(p0)) and _bits(p0) != _bits(p0d)
    sq = {k: (X[..., 3] - q) * (X[..., 3] - q) for k, q in (("p0", p0), ("divided", p0d), ("0.1", p01))}
    assert np.all(_bits(sq["p0"]) != _bits(sq["divided"])) and np.all(_bits(sq["p0"]) != _bits(sq["0.1"]))
    for every in (1, 7):
        want = stats_of(X[every - 1::every], p0)
        for other in (p0d, p01):
            got = stats_of(X[every - 1::every], other)
            differ = _bits(got[..., 7]) != _bits(want[..., 7])     # (a sum of m terms that all differ may still round alike)
            print(f"{nx}x{ny} every {every}: floats 7 differ in {differ.mean():.4f} of the cells")
            assert np.array_equal(_bits(got[..., :7]), _bits(want[..., :7])) and differ.mean() >= 0.95 and differ[blocked].all()
        assert np.all(_bits(want[blocked]) == _bits(blocked_record(p0, len(X[every - 1::every]))))
        assert np.all(stats_of(X[every - 1::every], p0d)[blocked][:, 7] > 0)


@pytest.mark.parametrize("path,point", CASES)
def test_case_holds_what_it_claims(O, oracle, path, point):
    """Tame over its run on the float oracle (fluid rho >= 0.25 rho0, |f| <= rho0; "thirds" over 30 steps with room to spare:
    rho >= 0.91 rho0, |f| <= 0.50 rho0, nothing refused); refusing where it says so, before a sample step and inside a full
    pass; the period with every kind of sample step and a division that rounds.  At the refusing points the sums feel the
    guard: float 0 of stats_of over the float oracle's fields differs, in a fluid cell of row ny-2 that the guard refused
    before a sample step, from the same run at the control acceleration."""
    nx, ny, K, n, me, kind, ob, cells, _, _ = _case(path, point)
    steps = _steps(O, oracle, path, point, THIRDS_STEPS if point == "thirds" else n)
    if point == "thirds":
        assert len(steps) == THIRDS_STEPS and 2 * K + 5 <= n <= 3 * K + 5
        assert min(s[0] for s in steps) >= 0.91 and max(s[1] for s in steps) <= 0.50, (min(s[0] for s in steps), max(s[1] for s in steps))
        assert not any(s[2].any() for s in steps)
    assert min(s[0] for s in steps) >= 0.25 and max(s[1] for s in steps) <= 1.0
    m = n // me
    assert m >= 3 and not _power_of_two(m) and (K == 1 or all(_placement(K, n, me))), (K, n, me)
    if point in REFUSING:
        full, last = n // K * K, m * me
        assert not steps[0][2].any() and any(steps[t - 1][2].any() for t in range(2, full + 1))
        hit = np.zeros(nx, bool)
        for t in range(2, last + 1):                              # (step t's accelerate shapes the fields of step t)
            hit |= steps[t - 1][2]
        prm = _oracle_param(O, point, nx, ny)
        d, _, w = (float(np.float32(v)) for v in PARAM_GRID[point])
        calm = O.OrcParam(nx, ny, 100, 10, d, float(np.float32(CONTROL_ACCEL)), w)
        p0 = p0_of(PARAM_GRID[point][0])
        got = [stats_of(_float_oracle_fields(oracle, q, ob, cells, n)[me - 1:n:me], p0)[ny - 2, :, 0] for q in (prm, calm)]
        assert hit.any() and np.any(_bits(got[0])[hit] != _bits(got[1])[hit]), (path, point)


# ---------------------------------------------------------------------------------------------------------------- GPU
WORST = {"moments": 0.0, "variances": 0.0}


def _reference(L, O, path, point):
    if point != "thirds":
        return OBS._reference(L, O, path, point)
    nx, ny, _, _, _, kind, ob, cells, body, _ = _case(path, point)
    variant = dict(PATHS[path][3]).get("kernel_variant")
    key = (nx, ny, point, kind, variant)
    if key not in OBS._REF:
        nmax = max(_case(q, pt)[3] for q, pt in CASES
                   if pt == point and PATHS[q][:2] == (nx, ny) and dict(PATHS[q][3]).get("kernel_variant") == variant)
        OBS._REF[key] = OBS._reference_run(L, O, key, ob, cells, body, _lib_param(L, point, nx, ny), _oracle_param(O, point, nx, ny), nmax)
    return OBS._REF[key]


def _outside_bounds(O, prm, ob, S, X, stats, p0):
    """(worst |stats[4..7] - mean Q| / bQ, worst |V - W| / its bound) by the module docstring; S, X: the sampled steps'
    lattices and fields (m, ny, nx, .); asserts both bounds and the exact zeros of the blocked cells."""
    return bounds_from_fields(double_oracle_fields(O, prm, ob, S), ob != 0, X, stats, p0)


def double_oracle_fields(O, prm, ob, S):
    """fo_j: the DOUBLE oracle's fields of the lattices S (m, ny, nx, 9), (m, ny, nx, 4) float64"""
    o64 = O.Oracle("strict")
    ny, nx = ob.shape
    return np.stack([o64.final_state(prm, s.astype(np.float64), ob).reshape(ny, nx, 4) for s in S])


def bounds_from_fields(fo, blocked, X, stats, p0):
    """_outside_bounds from the double oracle's fields fo, on any set of cells: fo, X (m, rows, cols, 4), blocked
    (rows, cols) and stats (rows, cols, 8) of the same cells (tests/test_window_stats_param_space.py hands it a window's)."""
    m = X.shape[0]
    assert fo.shape == X.shape and blocked.shape == X.shape[1:3] and stats.shape == X.shape[1:3] + (8,)
    dx = 2e-6 * np.abs(fo) + 8 * U
    x, y, d = fo[..., 0], fo[..., 1], fo[..., 3] - float(p0)
    ex, ey, ep = dx[..., 0], dx[..., 1], dx[..., 3]
    Q = np.stack([x * x, y * y, x * y, d * d], axis=-1)
    e = np.stack([2 * np.abs(x) * ex + ex * ex, 2 * np.abs(y) * ey + ey * ey, np.abs(x) * ey + np.abs(y) * ex + ex * ey,
                  2 * np.abs(d) * ep + ep * ep], axis=-1)
    Q[:, blocked], e[:, blocked] = 0.0, 0.0
    s = stats.astype(np.float64)
    bQ = e.mean(axis=0) + m * U * np.abs(Q).mean(axis=0) + U * np.abs(s[..., 4:])
    errQ = np.abs(s[..., 4:] - Q.mean(axis=0))
    assert np.all(s[blocked][:, 4:] == 0) and np.all(bQ[blocked] == 0)
    rQ = float(np.max(errQ / np.where(bQ > 0, bQ, 1.0)))
    assert np.all(errQ <= bQ), ("second moments against the double oracle", rQ)
    # the variances
    bM = dx.mean(axis=0) + (m - 1) * U * np.abs(X.astype(np.float64)).sum(axis=0) + U * np.abs(s[..., :4])
    mx, my, md = x.mean(axis=0), y.mean(axis=0), d.mean(axis=0)
    mx[blocked], my[blocked], md[blocked] = 0.0, 0.0, 0.0         # (d there: float(p0) - float(p0))
    sd = s[..., 3] - float(p0)
    V = np.stack([s[..., 4] - s[..., 0] ** 2, s[..., 5] - s[..., 1] ** 2, s[..., 6] - s[..., 0] * s[..., 1], s[..., 7] - sd ** 2], axis=-1)
    Qm = Q.mean(axis=0)
    W = np.stack([Qm[..., 0] - mx ** 2, Qm[..., 1] - my ** 2, Qm[..., 2] - mx * my, Qm[..., 3] - md ** 2], axis=-1)
    bV = np.stack([bQ[..., 0] + 2 * np.abs(mx) * bM[..., 0] + bM[..., 0] ** 2,
                   bQ[..., 1] + 2 * np.abs(my) * bM[..., 1] + bM[..., 1] ** 2,
                   bQ[..., 2] + np.abs(mx) * bM[..., 1] + np.abs(my) * bM[..., 0] + bM[..., 0] * bM[..., 1],
                   bQ[..., 3] + 2 * np.abs(md) * bM[..., 3] + bM[..., 3] ** 2], axis=-1)
    prod = np.stack([s[..., 0] ** 2, s[..., 1] ** 2, np.abs(s[..., 0] * s[..., 1]), sd ** 2], axis=-1)
    bV = bV + 2.0 ** -50 * (np.abs(s[..., 4:]) + prod)
    errV = np.abs(V - W)
    # (a blocked cell: three variances exactly 0; the pressure's is -(p0' - p0)^2 of blocked_record, 0 where the sum of p0 does not round)
    assert np.all(V[blocked][:, :3] == 0) and np.all(np.abs(V[blocked][:, 3]) <= (m * U * float(p0)) ** 2) and np.all(W[blocked] == 0)
    rV = float(np.max(errV / np.where(bV > 0, bV, 1.0)))
    assert np.all(errV <= bV), ("variances against the double oracle", rV)
    return rQ, rV


@pytest.mark.gpu
@pytest.mark.parametrize("path,point", CASES)
def test_stats_on_the_parameter_grid(gpu, O, monkeypatch, path, point):
    L = gpu
    nx, ny, K, n, me, kind, ob, cells, body, xy = _case(path, point)
    _, _, _, options, info_want, kw, pkind = PATHS[path]
    ref = _reference(L, O, path, point)
    p, prm = _lib_param(L, point, nx, ny), _oracle_param(O, point, nx, ny)
    p0 = p0_of(p.density)
    assert _bits(p0) == _bits(p0_of(_triple(point)[0]))
    blocked = ob != 0
    assert blocked.any()

    def call(name, fn, every=0):
        where = (path, point, n, every, name)
        with OBS._open(L, path, p, ob, cells, body, xy, monkeypatch) as lat:
            out = fn(lat)
            if name == "stats":
                got = {k: int(lat.info(k)) for k in ("stats_in_wave", "mean_in_kernel")}
                assert got == {"stats_in_wave": 1 if pkind == "wave" else 0, "mean_in_kernel": 0}, (where, got)
            for key, v in info_want.items():
                if key == "exchange":
                    v = {"rccl": L.EXCHANGE_RCCL}[v]
                assert lat.info(key) == v, (where, key, lat.info(key))
            st = lat.read_state()
        return out, st

    av0, st0 = call("plain", lambda lat: lat.run(n))
    assert np.array_equal(_bits(st0), _bits(ref["S"][n - 1])), (path, point, "the lattice of the one-step kernel")
    for every in _everys(path, point):
        where = (path, point, n, every)
        m = n // every
        (av, stats), st = call("stats", lambda lat: lat.run_stats(n, every), every)
        (_, mean), _ = call("mean", lambda lat: lat.run_mean(n, every), every)
        Xs, Ss = ref["X"][every - 1:n:every][:m], ref["S"][every - 1:n:every][:m]
        want = stats_of(Xs, p0)
        assert stats.shape == want.shape == (ny, nx, 8) and stats.dtype == np.float32, where
        bad = np.argwhere(_bits(stats) != _bits(want))
        assert len(bad) == 0, (where, "stats", len(bad), [tuple(int(v) for v in b) for b in bad[:8]])
        assert np.array_equal(_bits(stats[..., :4]), _bits(mean)), (where, "floats 0..3 against lbm_run_mean")
        assert np.array_equal(_bits(mean), _bits(mean_of(Xs))), (where, "lbm_run_mean")
        const = blocked_record(p0, m)
        assert np.all(_bits(stats[blocked]) == _bits(const)) and abs(float(const[3]) - float(p0)) <= m * U * float(p0), (where, "blocked cells")
        assert np.array_equal(_bits(st), _bits(st0)), (where, "lattice")
        if pkind in ("tiles", "wave"):
            assert np.array_equal(_bits(av), _bits(av0)), (where, "av_vels")
        assert av.shape == (n,) and np.allclose(av, av0, rtol=ENGINE_AV_RTOL, atol=0), (where, "av_vels")
        rQ, rV = _outside_bounds(O, prm, ob, Ss, Xs, stats, p0)
        WORST["moments"], WORST["variances"] = max(WORST["moments"], rQ), max(WORST["variances"], rV)
        print(f"{path} {point}: {n} steps, every {every} (m = {m}); second moments {rQ:.3f} of their bound, variances {rV:.3f} of"
              f" theirs; worst so far: {WORST['moments']:.3f}, {WORST['variances']:.3f}")
