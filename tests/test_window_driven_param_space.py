"""The three newest run calls away from the shipped decks: lbm_run_window, lbm_run_driven and lbm_run_driven_observed on
the 80 (path, point) cases of tests/test_observer_param_space.py -- every observer path at the points of PARAM_GRID whose
density is not 0.1 and where the accelerate guard refuses part of row ny-2 inside a pass.

Until this module every test of these calls ran at density 0.1 and omega 1.85.  The density reaches a window through
launch_window, the window flavour of lbm_wave and the register tiles' probe flavour fed window tables; a schedule
reaches the lattice through accel_pair(density, accel[t]), once per call for the register tiles, per pass for lbm_wave and
per step behind the last pass.  A site that kept 0.1 passes every test at the control point; a flavour that reads pair
t +- 1, or the context's own pair, changes lattice bits only where the guard's decision flips ("refusal", "light_fluid").

  * Shapes, step counts n, obstacles, initial states, bodies, probes and periods: test_observer_param_space._case.
  * Schedules, one pair per group of cases that share a reference (shape, point, maths), cut to a case's n:
      "a"  constant at the point's acceleration;
      "s"  test_driven_run.schedules(...)["b"] -- distinct values in [0.5, 1.5] accel, an index slip changes the constants --
           times a sign pattern at the points that do not refuse (negative at step 2, at every member's last step and at
           steps 3, 7, 11, ...); positive at the refusing points, where a negative acceleration would drive the unguarded
           populations 1, 5 and 8 negative within a few steps.
    No GPU: on the float oracle's driven run every case stays tame under "s" (fluid rho >= 0.25 rho0, |f| <= rho0); at a
    refusing point some step t >= 2 inside a full pass has refused and accepted fluid cells in row ny-2 and a refusal mask
    that differs from the masks of accel[t-1], accel[t+1] and the point's own acceleration on the same state; elsewhere "s"
    holds both signs, at K > 1 a negative entry inside a full pass and another among the left-over steps.
  * The driven reference, once per group: a fresh context under engine 1, time_block 1, `set_accel(accel[t]); run(1)`;
    S_t = read_state(), X_t = final_state().  Every S_t against one step of the oracle in double from S_{t-1} with
    prm.accel = accel[t], the accelerate phase in the reference's float arithmetic (a guard decision cannot flip), at the
    bar of test_param_space.test_one_step_kernel_against_double_oracle: u = 2^-24, rho the cell's density, every element
    within 8 u rho and within twice the float oracle's worst error + 1 u rho.  Every X_t against the double oracle's
    final_state of S_t at 2e-6 |fo| + 8 u.  A second loop, `set_accel(accel[t]); run_forces(1)`, gives the forces' bits of the
    one-step path (F1); the float64 forces and their scale follow from S_t (test_body_forces.forces_from_state).  The loop
    under "a" gives the bits of run(1) at a time without set_accel.
  * Windows (constant acceleration; X of test_observer_param_space._reference): per case the whole extent at strides
    (3, 5), the accelerate row, and 7 x 7 cells across the first column edge and a row edge of the path (the middle of the
    lattice where the path has none) that hold a blocked cell.  window_out = cut(X[se-1:n:se], w) bit for bit; a blocked
    cell reads exactly (0, 0, 0, float32(density) x float32(1/3)); window_in_kernel on the tiles, window_in_wave on lbm_wave;
    av_vels lbm_run's bits there, within rtol 2e-6 on the split paths; the lattice the bits of S_n.
  * lbm_run_driven: under "s" the lattice is the driven reference's S_n, av_vels within rtol 2e-6 of the loop's,
    driven_in_kernel / driven_in_wave 1/0 on the tiles, 0/1 on lbm_wave, 0/0 on the split paths; under "a" the lattice is
    lbm_run's, and av_vels are lbm_run's bits on the tiles.
  * lbm_run_driven_observed under "s", three calls: all four observers at the case's periods, forces with probes, and one
    observer alone (forces, probes, mean, snapshots in turn by case index).  Snapshots, probes and means bit for bit from
    X_t (means also within (m - 1) 2^-24 sum |X_j| + 2^-24 |mean| of the float64 mean); forces the bits of F1 on the paths of
    FORCE_BITS and everywhere _close to the float64 forces; the lattice S_n; av_vels within rtol 2e-6; the three info keys
    by _expected_driven_info.  At the refusing points the forces differ in bits from lbm_run_observed's at constant
    acceleration on some step >= 2: the schedule reached the force flavour.

Measured on one MI355X (printed by the tests): S_t at most 0.70 of its bar, X_t 0.09 of its bar, the forces 8e-9 of their
scale (bar 1e-5), the mean 0.33 of its bound; 51 s for the 240 GPU tests ("Windows and schedules on
the grid")."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from test_body_forces import _close, forces_from_state
from test_driven_run import driven_oracle, schedules
from test_mean_run import mean_of
from test_observer_param_space import (CASES, FORCE_BITS, NBODIES, PATHS, _bits, _case, _edges, _open, _periods,
                                       _reference)
from test_param_space import REFUSING, _lparam, _orc_param
from test_window_run import cut

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden import PARAM_GRID, refused  # noqa: E402

U = 2.0 ** -24
ONE_THIRD = np.float32(1.0 / 3.0)
AV_RTOL = 2e-6                     # the bar of tests/test_driven_run.py and tests/test_window_run.py for the split paths
SEED = 43
ALONE = ("forces", "probes", "mean", "fields")


def _alone(path, point):
    """The observer of a case's one-observer call: in turn by case index, shifted by one from path to path (a path has
    four cases: without the shift a point would always meet the same observer)."""
    i = CASES.index((path, point))
    return ALONE[(i + i // 4) % 4]


# ---------------------------------------------------------------------------------------------------------------- schedules
def _variant(path):
    return dict(PATHS[path][3]).get("kernel_variant")


_GROUP = {}


def _group(path, point):
    """The cases that share a reference -- one shape, one point (hence one state), one maths -- with their schedules over
    the longest run among them: dict(key, nmax, a, s)."""
    nx, ny = PATHS[path][:2]
    key = (nx, ny, point, _variant(path))
    if key not in _GROUP:
        ns = sorted({_case(q, pt)[3] for q, pt in CASES if pt == point and PATHS[q][:2] == (nx, ny) and _variant(q) == _variant(path)})
        nmax = ns[-1]
        accel = PARAM_GRID[point][1]
        s = schedules(accel, nmax, SEED)
        sign = np.ones(nmax, dtype=np.float32)
        if point not in REFUSING:
            t = np.arange(1, nmax + 1)
            sign[(t == 2) | np.isin(t, ns) | (t % 4 == 3)] = -1.0
        sched = dict(a=s["a"], s=s["b"] * sign)
        for v in sched.values():
            assert v.dtype == np.float32 and v.shape == (nmax,)
            v.setflags(write=False)
        _GROUP[key] = dict(key=key, nmax=nmax, **sched)
    return _GROUP[key]


def _schedule(path, point, name):
    return _group(path, point)[name][:_case(path, point)[3]]


# ---------------------------------------------------------------------------------------------------------------- windows
def _blocked_in(ob, w):
    return cut(ob[None, :, :, None], w)[0, :, :, 0] != 0


def _straddle(path):
    """(column c, rows) such that c - 1 | c is the first column edge of the path and r - 1 | r a row edge for every r of
    rows, the middle one first; the middle of the lattice where the path has no edge of that kind."""
    nx, ny = PATHS[path][:2]
    ecols, erows = _edges(path)
    c = next((c for c in ecols if c - 1 in ecols), nx // 2)
    pairs = [r for r in erows if r - 1 in erows] or [ny // 2]
    mid = len(pairs) // 2
    return c, sorted(pairs, key=lambda r: abs(pairs.index(r) - mid))


def windows_of(L, path, ob):
    """The three windows of a case: strided whole extent, accelerate row, 7 x 7 cells across a column edge and the first
    of the row edges that leaves a blocked cell inside (every lattice here is at least 64 x 12).  ob: the case's obstacles
    (tests/test_window_stats_param_space.py builds its windows here too, at "thirds" from that point's own map)."""
    nx, ny = PATHS[path][:2]
    W = L.Window
    c, rows = _straddle(path)
    rects = [W(c - 3, min(max(r - 3, 0), ny - 7), 7, 7) for r in rows]
    rect = next((w for w in rects if _blocked_in(ob, w).any()), rects[0])
    return [W(0, 0, (nx + 2) // 3, (ny + 4) // 5, 3, 5), W(0, ny - 2, nx, 1), rect]


# ---------------------------------------------------------------------------------------------------------------- no GPU
_TRAJECTORY = {}


def _trajectory(O, oracle, path, point):
    """The float oracle's driven run of the group under "s": per step t = 1 .. nmax (min fluid rho / rho0, max |f| / rho0,
    row ny-2 has refused and accepted fluid cells under accel[t], and that step's refusal mask differs on the same state
    from the mask under accel[t-1] / under accel[t+1] (None behind the last step) / under the point's acceleration)."""
    g = _group(path, point)
    if g["key"] not in _TRAJECTORY:
        nx, ny, _, _, _, kind, ob, cells, _, _ = _case(path, point)
        prm = _orc_param(O, point, nx, ny)
        rho0 = float(np.float32(PARAM_GRID[point][0]))
        s, x, out = g["s"], cells.copy(), []
        fluid = ob[ny - 2] == 0
        for t in range(1, g["nmax"] + 1):
            m = refused(prm.density, s[t - 1], ob, x)

            def differs(a):
                return bool(np.any(m != refused(prm.density, a, ob, x)))

            marks = (bool(m.any() and (fluid & ~m).any()), t >= 2 and differs(s[t - 2]),
                     differs(s[t]) if t < g["nmax"] else None, differs(prm.accel))
            driven_oracle(oracle, prm, x, ob, s[t - 1:t])
            assert np.all(np.isfinite(x)), (g["key"], t)
            rho = x.astype(np.float64).sum(axis=-1)[ob == 0]
            out.append((float(rho.min()) / rho0, float(np.abs(x).max()) / rho0) + marks)
        _TRAJECTORY[g["key"]] = out
    return _TRAJECTORY[g["key"]]


def test_groups_and_schedules_are_what_they_say():
    assert len(CASES) == 80
    keys = {_group(path, point)["key"] for path, point in CASES}
    assert len(keys) < len(CASES)                                   # references are shared
    for path, point in CASES:
        g, n = _group(path, point), _case(path, point)[3]
        accel = np.float32(PARAM_GRID[point][1])
        a, s = _schedule(path, point, "a"), _schedule(path, point, "s")
        assert a.shape == s.shape == (n,) and n <= g["nmax"] and np.all(a == accel)
        assert len(set(np.abs(s).tolist())) == n                    # n distinct values: any index slip changes the constants
        assert np.all(np.abs(s) >= 0.5 * accel * (1 - 1e-6)) and np.all(np.abs(s) <= 1.5 * accel * (1 + 1e-6))
        assert np.array_equal(np.abs(g["s"]), schedules(PARAM_GRID[point][1], g["nmax"], SEED)["b"])
        if point in REFUSING:
            assert np.all(s > 0)
    # the one-observer call takes every observer on every kind of path and at a refusing point
    for name in ALONE:
        mine = [case for case in CASES if _alone(*case) == name]
        assert len(mine) == 20
        assert {PATHS[p][6] for p, _ in mine} == {"split", "wave", "tiles"}, name
        assert any(pt in REFUSING for _, pt in mine), name


@pytest.mark.parametrize("path,point", CASES)
def test_schedule_holds_what_it_claims(O, oracle, path, point):
    """The counterpart of test_observer_param_space.test_case_holds_what_it_claims for schedule "s" (module docstring)."""
    nx, ny, K, n, _, kind, ob, cells, _, _ = _case(path, point)
    s = _schedule(path, point, "s")
    steps = _trajectory(O, oracle, path, point)[:n]
    assert min(st[0] for st in steps) >= 0.25 and max(st[1] for st in steps) <= 1.0, [(round(st[0], 2), round(st[1], 2)) for st in steps]
    full = n // K * K
    if point in REFUSING:
        flips = [t for t in range(2, full + 1)
                 if steps[t - 1][2] and steps[t - 1][3] and steps[t - 1][5] and (t == n or steps[t - 1][4])]
        assert flips, ("no step inside a full pass whose refusals differ from those of its neighbours' pairs", [st[2:] for st in steps])
    else:
        assert (s > 0).any() and (s < 0).any()
        if K > 1:
            assert (s[:full] < 0).any() and (s[full:] < 0).any(), (K, n, s)


@pytest.mark.parametrize("path,point", CASES)
def test_windows_hold_what_they_claim(L, path, point):
    """Three legal windows, blocked and fluid cells in each; the rectangle at least 5 x 5 cells with cells on both sides of
    the path's first column edge and of one of its row edges (of the middle of the lattice where it has none)."""
    nx, ny, K, n, (pe, me, se), kind, ob, cells, _, _ = _case(path, point)
    ws = windows_of(L, path, ob)
    assert len(ws) == 3 and n // se >= 1 and (pe, me, se) == _periods(K, n)
    for w in ws:
        assert w.nx >= 1 and w.ny >= 1 and 0 <= w.x0 and 0 <= w.y0
        assert w.x0 + (w.nx - 1) * w.sx < nx and w.y0 + (w.ny - 1) * w.sy < ny, w
        assert L.window_rows(w, nx, ny, 0, ny) == (0, w.ny)
        blocked = _blocked_in(ob, w)
        assert blocked.shape == (w.ny, w.nx) and blocked.any() and not blocked.all(), w
    whole, row, rect = ws
    assert (whole.sx, whole.sy) == (3, 5) and whole.x0 + whole.nx * 3 >= nx and whole.y0 + whole.ny * 5 >= ny
    assert (row.x0, row.y0, row.nx, row.ny) == (0, ny - 2, nx, 1)
    assert rect.nx >= 5 and rect.ny >= 5 and (rect.sx, rect.sy) == (1, 1)
    ecols, erows = _edges(path)
    c = next((c for c in ecols if c - 1 in ecols), nx // 2)
    assert rect.x0 <= c - 1 and c < rect.x0 + rect.nx
    if ecols:
        assert c == ecols[1] and c - 1 == ecols[0]                # the first column edge
    pairs = [r for r in erows if r - 1 in erows] or [ny // 2]
    assert any(rect.y0 <= r - 1 and r < rect.y0 + rect.ny for r in pairs), (rect, pairs)


# ---------------------------------------------------------------------------------------------------------------- GPU
WORST = {"S": 0.0, "X": 0.0, "forces": 0.0, "mean": 0.0}
_DREF = {}


def _driven_reference(L, O, oracle, path, point):
    """Once per group: S_t, X_t and av_vels of the loop set_accel(accel[t]); run(1) under "s" on the one-step kernel, S_t
    and X_t held to the double oracle; the float64 forces of S_t with their scale; F1, the forces of the loop
    set_accel(accel[t]); run_forces(1); and the loop under "a" held to the bits of run(1) at a time."""
    g = _group(path, point)
    if g["key"] in _DREF:
        return _DREF[g["key"]]
    nx, ny, _, _, _, kind, ob, cells, body, _ = _case(path, point)
    nmax, s = g["nmax"], g["s"]
    p = _lparam(L, point, nx, ny)
    prm = _orc_param(O, point, nx, ny)
    keep = prm.accel
    variant = _variant(path)
    opts = [("engine", 1), ("time_block", 1)] + ([("kernel_variant", variant)] if variant is not None else [])

    def fresh(with_bodies=False):
        lat = L.Lattice(p, ob, cells)
        for k, v in opts:
            lat.set_option(k, v)
        if with_bodies:
            lat.set_bodies(body, NBODIES)
        return lat

    S, X, F64, A, av = [], [], [], [], []
    worst_s = worst_x = 0.0
    prev = np.array(cells, dtype=np.float32)
    with fresh() as lat:
        for t in range(1, nmax + 1):
            lat.set_accel(float(s[t - 1]))
            av.append(lat.run(1))
            st, x = lat.read_state(), lat.final_state()
            assert lat.info("engine_last") == 1 and lat.info("time_block_active") == 1
            assert np.float32(lat.info("accel")) == s[t - 1]
            # S_t: one step of the oracle from S_{t-1}, accelerate in the reference's float arithmetic, the sweep in double
            prm.accel = float(s[t - 1])
            acc = prev.copy()
            oracle.accelerate(prm, acc, ob)
            a64 = acc.astype(np.float64)
            t64, t32 = np.empty_like(a64), np.empty_like(acc)
            oracle.sweep(prm, a64, t64, ob)
            oracle.sweep(prm, acc.copy(), t32, ob)
            rho = t64.sum(axis=-1, keepdims=True)
            e32 = float(np.max(np.abs(t32 - t64) / (U * rho)))
            e = float(np.max(np.abs(st - t64) / (U * rho)))
            worst_s = max(worst_s, e / 8.0, e / (2.0 * e32 + 1.0))
            assert e <= 8.0 and e <= 2.0 * e32 + 1.0, (g["key"], t, e, e32)
            # X_t: the double oracle's final_state of S_t
            fo = oracle.final_state(prm, st.astype(np.float64), ob).reshape(ny, nx, 4)
            err, bar = np.abs(x - fo), 2e-6 * np.abs(fo) + 8 * U
            worst_x = max(worst_x, float(np.max(err / bar)))
            assert np.all(err <= bar), (g["key"], t, float(np.max(err / bar)))
            f, a = forces_from_state(st, ob, body, NBODIES)
            S.append(st), X.append(x), F64.append(f), A.append(a)
            prev = st
    prm.accel = keep
    F1, av1 = [], []
    with fresh(True) as lat:
        for t in range(1, nmax + 1):
            lat.set_accel(float(s[t - 1]))
            a1, f1 = lat.run_forces(1)
            assert lat.info("engine_last") == 1 and lat.info("forces_in_kernel") == 0 and lat.info("forces_in_wave") == 0
            av1.append(a1), F1.append(f1[0])
        assert np.array_equal(_bits(lat.read_state()), _bits(S[-1]))
    assert np.array_equal(_bits(np.concatenate(av1)), _bits(np.concatenate(av)))
    # "a": set_accel with the context's own value changes no bit of run(1) at a time
    const = _reference(L, O, path, point)
    with fresh() as lat:
        ava = []
        for a in g["a"]:
            lat.set_accel(float(a))
            ava.append(lat.run(1))
        assert np.array_equal(_bits(lat.read_state()), _bits(const["S"][nmax - 1]))
    assert np.array_equal(_bits(np.concatenate(ava)), _bits(const["av"][:nmax]))
    ref = dict(S=np.stack(S), X=np.stack(X), F64=np.array(F64), A=np.array(A), av=np.concatenate(av), F1=np.array(F1))
    for a in ref.values():
        assert np.all(np.isfinite(a))
        a.setflags(write=False)
    WORST["S"], WORST["X"] = max(WORST["S"], worst_s), max(WORST["X"], worst_x)
    print(f"driven reference {nx}x{ny} {point} {kind}: {nmax} steps, worst S_t {worst_s:.3f} of its bar, X_t {worst_x:.3f} of its bar")
    _DREF[g["key"]] = ref
    return ref


_PLAIN = {}


def _context(L, path, point, monkeypatch):
    nx, ny, _, _, _, _, ob, cells, body, xy = _case(path, point)
    lat = _open(L, path, _lparam(L, point, nx, ny), ob, cells, body, xy, monkeypatch)
    if PATHS[path][5].get("rccl"):
        assert lat.slab_rows(0) == (0, ny)
    return lat


def _check_path(L, lat, path, where):
    for key, v in PATHS[path][4].items():
        if key == "exchange":
            v = {"rccl": L.EXCHANGE_RCCL}[v]
        assert lat.info(key) == v, (where, key, lat.info(key))


def _plain(L, path, point, monkeypatch):
    """(av_vels, lattice) of lbm_run under the path's options, once per case."""
    if (path, point) not in _PLAIN:
        n = _case(path, point)[3]
        with _context(L, path, point, monkeypatch) as lat:
            av, st = lat.run(n), lat.read_state()
            _check_path(L, lat, path, "lbm_run")
        av.setflags(write=False), st.setflags(write=False)
        _PLAIN[(path, point)] = (av, st)
    return _PLAIN[(path, point)]


def _same(got, want, where):
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (where, len(bad), [tuple(int(v) for v in b) for b in bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("path,point", CASES)
def test_windows_on_the_parameter_grid(gpu, O, monkeypatch, path, point):
    L = gpu
    nx, ny, K, n, (pe, me, se), kind, ob, cells, body, xy = _case(path, point)
    pkind = PATHS[path][6]
    ref = _reference(L, O, path, point)
    av0, st0 = _plain(L, path, point, monkeypatch)
    assert np.array_equal(_bits(st0), _bits(ref["S"][n - 1])), (path, point, "the lattice of the one-step kernel")
    fields = ref["X"][se - 1:n:se][:n // se]
    const = np.array([0.0, 0.0, 0.0, np.float32(_lparam(L, point, nx, ny).density) * ONE_THIRD], dtype=np.float32)
    for w in windows_of(L, path, ob):
        where = (path, point, n, se, w)
        with _context(L, path, point, monkeypatch) as lat:
            av, out = lat.run_window(n, se, w)
            got = {k: int(lat.info(k)) for k in ("window_in_kernel", "window_in_wave")}
            assert got == dict(window_in_kernel=int(pkind == "tiles"), window_in_wave=int(pkind == "wave")), (where, got)
            _check_path(L, lat, path, where)
            st = lat.read_state()
        _same(out, cut(fields, w), where)
        blocked = _blocked_in(ob, w)
        assert blocked.any() and np.all(_bits(out[:, blocked]) == _bits(const)), (where, "blocked cells")
        if pkind != "split":
            assert np.array_equal(_bits(av), _bits(av0)), (where, "av_vels")
        assert np.allclose(av, av0, rtol=AV_RTOL, atol=0), (where, "av_vels")
        assert np.array_equal(_bits(st), _bits(ref["S"][n - 1])), (where, "lattice")


@pytest.mark.gpu
@pytest.mark.parametrize("path,point", CASES)
def test_driven_runs_on_the_parameter_grid(gpu, O, oracle, monkeypatch, path, point):
    L = gpu
    nx, ny, K, n, _, kind, ob, cells, body, xy = _case(path, point)
    pkind = PATHS[path][6]
    dref = _driven_reference(L, O, oracle, path, point)
    av0, st0 = _plain(L, path, point, monkeypatch)
    want = dict(driven_in_kernel=int(pkind == "tiles"), driven_in_wave=int(pkind == "wave"))
    for name in ("s", "a"):
        s = _schedule(path, point, name)
        where = (path, point, n, name)
        with _context(L, path, point, monkeypatch) as lat:
            av = lat.run_driven(s)
            got = {k: int(lat.info(k)) for k in want}
            assert got == want, (where, got)
            _check_path(L, lat, path, where)
            assert np.float32(lat.info("accel")) == np.float32(PARAM_GRID[point][1])
            st = lat.read_state()
        assert av.shape == (n,)
        if name == "s":
            assert np.array_equal(_bits(st), _bits(dref["S"][n - 1])), (where, "lattice")
            assert np.allclose(av, dref["av"][:n], rtol=AV_RTOL, atol=0), (where, "av_vels")
        else:
            assert np.array_equal(_bits(st), _bits(st0)), (where, "lattice")
            if pkind == "tiles":
                assert np.array_equal(_bits(av), _bits(av0)), (where, "av_vels")
            assert np.allclose(av, av0, rtol=AV_RTOL, atol=0), (where, "av_vels")


def _expected_driven_info(path, call, K, n, pe, me, se):
    """The three keys after lbm_run_driven_observed: `call` is "all" (the four observers), "pair" (forces and probes) or
    one of ALONE.  Forces and probes cut no piece on the tiles and in lbm_wave; means and snapshots cut at their sample
    steps; lbm_wave takes a piece of K steps or more; pieces reads 0 where the whole call took the one-step path."""
    kind = PATHS[path][6]
    forces, probes = call in ("all", "pair", "forces"), call in ("all", "pair", "probes")
    cuts = {n}
    if call in ("all", "mean"):
        cuts |= set(range(me, n + 1, me))
    if call in ("all", "fields"):
        cuts |= set(range(se, n + 1, se))
    pieces = np.diff([0] + sorted(cuts))
    bits = (1 if forces else 0) | (2 if probes else 0)
    in_launches = kind == "tiles" or (kind == "wave" and pieces.max() >= K)
    return dict(driven_observed_in_kernel=bits if kind == "tiles" else 0,
                driven_observed_in_wave=bits if kind == "wave" and in_launches else 0,
                driven_observed_pieces=len(pieces) if in_launches else 0)


def test_expected_driven_info_is_what_the_other_tests_assert():
    """(tests/test_driven_observed.py: the tiles at n = 23 with a mean every 3 and snapshots every 5 run 11 pieces with
    bits 3; tests/test_wave_driven_observed.py: lbm_wave<K> over 2 K + 5 steps cut by K + 1 and 2 K runs 4 pieces.)"""
    assert _expected_driven_info("regtile", "all", 7, 23, 1, 3, 5) == dict(
        driven_observed_in_kernel=3, driven_observed_in_wave=0, driven_observed_pieces=11)
    assert _expected_driven_info("regtile", "mean", 7, 23, 1, 3, 5) == dict(
        driven_observed_in_kernel=0, driven_observed_in_wave=0, driven_observed_pieces=8)
    assert _expected_driven_info("regtile", "probes", 7, 23, 1, 3, 5)["driven_observed_in_kernel"] == 2
    assert _expected_driven_info("wave8", "all", 8, 21, 1, 9, 16) == dict(
        driven_observed_in_kernel=0, driven_observed_in_wave=3, driven_observed_pieces=4)
    assert _expected_driven_info("wave8", "pair", 8, 21, 1, 9, 16) == dict(
        driven_observed_in_kernel=0, driven_observed_in_wave=3, driven_observed_pieces=1)
    assert _expected_driven_info("wave8", "all", 8, 21, 1, 3, 5) == dict(
        driven_observed_in_kernel=0, driven_observed_in_wave=0, driven_observed_pieces=0)
    assert set(_expected_driven_info("march", "all", 4, 14, 1, 3, 5).values()) == {0}


@pytest.mark.gpu
@pytest.mark.parametrize("path,point", CASES)
def test_driven_observers_on_the_parameter_grid(gpu, O, oracle, monkeypatch, path, point):
    L = gpu
    nx, ny, K, n, (pe, me, se), kind, ob, cells, body, xy = _case(path, point)
    dref = _driven_reference(L, O, oracle, path, point)
    s = _schedule(path, point, "s")
    alone = _alone(path, point)
    blocked = ob[xy[:, 1], xy[:, 0]] != 0
    const = np.array([0.0, 0.0, 0.0, np.float32(_lparam(L, point, nx, ny).density) * ONE_THIRD], dtype=np.float32)
    worst = {"forces": 0.0, "mean": 0.0}

    def call(name, **kw):
        where = (path, point, n, pe, me, se, name)
        with _context(L, path, point, monkeypatch) as lat:
            res = lat.run_driven_observed(s, **kw)
            want = _expected_driven_info(path, name, K, n, pe, me, se)
            got = {k: int(lat.info(k)) for k in want}
            assert got == want, (where, got)
            _check_path(L, lat, path, where)
            assert np.float32(lat.info("accel")) == np.float32(PARAM_GRID[point][1])
            st = lat.read_state()
        assert np.array_equal(_bits(st), _bits(dref["S"][n - 1])), (where, "lattice")
        assert res["av_vels"].shape == (n,) and np.allclose(res["av_vels"], dref["av"][:n], rtol=AV_RTOL, atol=0), (where, "av_vels")
        assert sorted(res) == sorted(["av_vels"] + [k for k, v in (("forces", kw.get("forces")), ("probes", kw.get("probes_every")),
                                                                   ("mean", kw.get("mean_every")), ("fields", kw.get("fields_every"))) if v])
        if "fields" in res:
            _same(res["fields"], dref["X"][se - 1:n:se][:n // se], (where, "snapshots"))
        if "probes" in res:
            want = dref["X"][pe - 1:n:pe][:n // pe][:, xy[:, 1], xy[:, 0]]
            assert res["probes"].shape == want.shape == (n // pe, len(xy), 4)
            bad = np.argwhere(_bits(res["probes"]) != _bits(want))
            assert len(bad) == 0, (where, "probes", len(bad), [(int(j), tuple(xy[i]), int(k)) for j, i, k in bad[:8]])
            assert blocked.any() and np.all(_bits(res["probes"][:, blocked]) == _bits(const)), (where, "blocked probes")
        if "mean" in res:
            Xm = dref["X"][me - 1:n:me][:n // me]
            m = len(Xm)
            _same(res["mean"], mean_of(Xm), (where, "mean"))
            X64 = Xm.astype(np.float64)
            err = np.abs(res["mean"].astype(np.float64) - X64.mean(axis=0))
            lim = (m - 1) * U * np.abs(X64).sum(axis=0) + U * np.abs(res["mean"].astype(np.float64))
            worst["mean"] = max(worst["mean"], float(np.max(err / np.maximum(lim, 1e-300))))
            assert np.all(err <= lim), (where, "mean against float64", worst["mean"])
        if "forces" in res:
            F = res["forces"]
            assert F.shape == (n, NBODIES, 2)
            wf = float(np.max(np.abs(F - dref["F64"][:n]) / np.maximum(dref["A"][:n], 1e-30)))
            worst["forces"] = max(worst["forces"], wf / 1e-5)
            if path in FORCE_BITS:
                assert np.array_equal(_bits(F), _bits(dref["F1"][:n])), (where, "forces", float(np.abs(F - dref["F1"][:n]).max()))
            assert _close(F, dref["F64"][:n], dref["A"][:n]), (where, "forces against float64", wf)
        return res

    res = call("all", forces=True, probes_every=pe, mean_every=me, fields_every=se)
    call("pair", forces=True, probes_every=pe)
    call(alone, **{"forces": dict(forces=True), "probes": dict(probes_every=pe), "mean": dict(mean_every=me),
                   "fields": dict(fields_every=se)}[alone])
    if point in REFUSING:
        with _context(L, path, point, monkeypatch) as lat:
            steady = lat.run_observed(n, forces=True)["forces"]
        assert steady.shape == res["forces"].shape
        assert np.any(_bits(res["forces"][1:]) != _bits(steady[1:])), (path, point, "the schedule did not reach the forces")
    for k in worst:
        WORST[k] = max(WORST[k], worst[k])
    print(f"{path} {point}: {n} steps, periods {pe}/{me}/{se}, alone {alone}; forces {worst['forces']:.4f} of the 1e-5 scale bar,"
          f" mean {worst['mean']:.3f} of its bound; worst so far: S_t {WORST['S']:.3f} of its bar, X_t {WORST['X']:.3f},"
          f" forces {WORST['forces']:.4f}, mean {WORST['mean']:.3f}")
