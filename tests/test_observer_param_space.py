"""The observers away from the shipped decks: lbm_run_forces, lbm_run_probes, lbm_run_mean, lbm_run_sampled and
lbm_run_observed on every observer path at the points of PARAM_GRID (tests/golden/make_golden.py) whose density is not
0.1 and where the accelerate guard refuses part of row ny-2 inside a pass.

A blocked cell's pressure is density x (1/3), and the density reaches derive_cell through about a dozen host sites (the
WaveArgs of the probe, force-and-probe and field flavours of lbm_wave, the arguments of lbm_probe_gather / lbm_mean_add /
lbm_derive, the word the register tiles pack into LDS): a site that kept 0.1 passes every test at the control point.

  * PATHS: the rows of test_param_space.ENGINES that take an observer path of their own, and three more -- the one-step
    kernel at 128 x 64, lbm_wave<6> at 200 x 72 (the last wave column delivers part of its columns) and lbm_wave<8> x2 at
    256 x 64 in chunks of 24, 24 and 16 rows.  Every path carries the info keys that say where its observers ran.
  * CASES: every path at "refusal" and "light_fluid" from rest (at most 16 steps: the lattice blows up soon after),
    at "stability_edge" (density 0.37) and at one of "under_relaxed" / "omega_one" in turn (2 K + 5 steps).
  * The reference, once per (shape, point, state): the one-step kernel (engine 1, time_block 1), run(1) at a time,
    read_state() = S_t and final_state() = X_t after each.  X_t is held to the double oracle's final_state of S_t at every
    step (2e-6 |fo| + 8 x 2^-24, the bar of test_one_step_kernel_against_double_oracle); the float64 forces follow from
    S_t (test_body_forces.forces_from_state).  S_t itself is held to the double oracle by tests/test_param_space.py.
  * Per case six calls, each on a fresh context under the path's options: the four single calls, lbm_run_observed with
    all four observers at those periods, and lbm_run_observed with forces and probes alone (on lbm_wave the all-four call
    is cut into pieces shorter than K by any mean period that meets the placement conditions below, so the
    force-and-probe flavour of lbm_wave runs in this sixth call only).
      snapshots  fields[j] = X at step (j + 1) every, bit for bit
      probes     probes[j][p] = that snapshot in the probe's cell, bit for bit; a blocked probe reads exactly
                 (0, 0, 0, float32(density) x float32(1/3))
      mean       the header's definition in numpy float32 over the X_j, bit for bit; and within
                 (m - 1) 2^-24 sum |X_j| + 2^-24 |mean| of their float64 mean
      forces     the bits of the one-step path where that is defined (lbm_wave, the lone streaming kernels, the rank
                 ring of one); everywhere within 1e-5 of the absolute contributions of the float64 forces; at the
                 refusing points a body's force moves by more than 10 % between step 1 (no refusal) and a later step
      observed   every output the bits of its own call
      lattice    after every call the bits of lbm_run under the same options, which are the bits of S_nsteps
      av_vels    lbm_run's bits on the register tiles, and on lbm_wave for the single calls and forces + probes;
                 elsewhere within rtol 2e-6
  * No GPU: every case stays tame on the float oracle (fluid rho >= 0.25 rho0, |f| <= rho0), refuses where it claims to,
    and its bodies, probes and periods hold every kind of cell and sample step listed in _case().

Periods (K = the path's steps per pass, n = the run): each of the three is the largest `every` that has a sample step
inside a full pass below level K, one at level K and one among the left-over steps (means: with m = n // every >= 3 and no
power of two, so that the division rounds); the probes take the next smaller one where there is one.  At K = 1 every step
is a pass of its own: nothing lies below level K or behind the last pass, and the periods are 2, 1 and 3.

Measured on one MI355X (printed by the tests): X_t at most 0.09 of its bar from double, the forces at most 1e-8 of
their scale (bar 1e-5), the mean at most 0.33 of its bound; 39 s for the 80 cases ("Observers on the
grid")."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from test_body_forces import CX, CY, _close, forces_from_state
from test_mean_run import mean_of
from test_param_space import ENGINES, REFUSING, _lparam, _orc_param

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden import PARAM_GRID, param_state, refused  # noqa: E402

U = 2.0 ** -24
ONE_THIRD = np.float32(1.0 / 3.0)
NBODIES = 4
SEED = 7
SEEDS = {(64, 40): 9}         # (seed 7 leaves row 37 of 64 x 40 three blocked cells with a fluid source: one short of four bodies)


def _seed(nx, ny):
    return SEEDS.get((nx, ny), SEED)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the table
def _wave_opts(K, cols=1, rows=0):
    o = [("engine", 1), ("march_kernel", 1), ("time_block", K), ("wave_cols", cols)]
    if rows:
        o.append(("wave_rows", rows))                 # (after time_block, which forgets the chunk height)
    return o


# as ENGINES: id -> (nx, ny, K, options, info that must hold after, Lattice kwargs)
EXTRA = {
    "one_step": (128, 64, 1, [("engine", 1), ("time_block", 1)], {"engine_last": 1, "time_block_active": 1}, {}),
    "wave6_partial_column": (200, 72, 6, _wave_opts(6), {"engine_last": 1, "time_block_active": 6, "march_kernel": 1}, {}),
    "wave8_cols2_ragged": (256, 64, 8, _wave_opts(8, 2, 24),
                           {"engine_last": 1, "time_block_active": 8, "march_kernel": 1, "wave_cols_active": 2, "wave_rows": 24}, {}),
}
# which observer path a row takes: "split" (small kernels behind pieces / single steps), "wave", "tiles"
FROM_ENGINES = {
    "sweep2": "split", "march": "split",
    "wave4": "wave", "wave6": "wave", "wave8": "wave", "wave8_cols2": "wave",
    "regtile": "tiles", "regtile_8x4": "tiles", "regtile_4x2": "tiles", "regtile_async_16x2": "tiles",
    "regtile_sync_8x2": "tiles", "regtile_ieee": "tiles", "regtile_slabs_copy": "tiles", "regtile_slabs_p2p": "tiles",
    "slabs_inside_copy": "split", "slabs_first_row_p2p": "split", "rccl_ring_of_one": "split",
}
PATHS = {name: ENGINES[name] + (kind,) for name, kind in FROM_ENGINES.items()}
PATHS.update({"one_step": EXTRA["one_step"] + ("split",), "wave6_partial_column": EXTRA["wave6_partial_column"] + ("wave",),
              "wave8_cols2_ragged": EXTRA["wave8_cols2_ragged"] + ("wave",)})
# forces: the one-step path's bits (slabs add their partial sums slab by slab: to rounding there)
FORCE_BITS = {n for n, row in PATHS.items() if row[6] == "wave" or (row[6] == "split" and "nslabs" not in row[5])}

COMPULSORY = ("refusal", "stability_edge", "light_fluid")
ROTATED = ("under_relaxed", "omega_one")
STATE = {"refusal": "rest", "light_fluid": "rest", "stability_edge": "guard", "under_relaxed": "perturbed", "omega_one": "guard"}
CASES = [(path, point) for i, path in enumerate(PATHS) for point in COMPULSORY + (ROTATED[i % 2],)]


def _nsteps(K, point):
    """From K + 5 steps where the guard refuses (at most 16), from 2 K + 5 elsewhere: the shortest run within one more
    pass whose mean can have a period above 1 (K = 4: 14 steps, every second; K = 2: 9 steps, every third), else the
    shortest run that has periods at all (K = 7: 12 steps, every step; K = 3: 11, since at 8 steps m is 4 or 8)."""
    base = K + 5 if point in REFUSING else 2 * K + 5
    runs = [n for n in range(base, base + K + 1) if (n <= 16 or point not in REFUSING) and _periods(K, n) is not None]
    return next((n for n in runs if _periods(K, n)[1] > 1), runs[0])


def _placement(K, n, every):
    """(a sample step inside a full pass below level K, one at level K, one among the left-over steps)"""
    full = n // K * K
    s = range(every, n + 1, every)
    return (any(t <= full and t % K for t in s), any(t <= full and t % K == 0 for t in s), any(t > full for t in s))


def _power_of_two(m):
    return m & (m - 1) == 0


def _periods(K, n):
    """(probes_every, mean_every, fields_every), or None where no mean period meets the conditions"""
    if K == 1:
        return 2, 1, 3
    valid = [e for e in range(1, n + 1) if all(_placement(K, n, e))]
    means = [e for e in valid if n // e >= 3 and not _power_of_two(n // e)]
    if not valid or not means:
        return None
    i = len(valid) - 1
    return valid[max(i - 1, 0)], means[-1], valid[i]


def _fluid_source(ob):
    """blocked cells with a fluid cell at B - c_i for some i: the cells lbm_run_forces counts when labelled"""
    blocked = ob != 0
    src = np.zeros(ob.shape, bool)
    for i in range(1, 9):
        src |= np.roll(~blocked, shift=(CY[i], CX[i]), axis=(0, 1))
    return blocked & src


def _bodies(ob):
    """Labels 0..4 on the blocked cells, at random; in rows ny-3, ny-2 and ny-1 -- the neighbours of the accelerate row --
    the cells with a fluid source take 1, 2, 3, 4, 1, ... in column order, so that every body counts cells there."""
    ny = ob.shape[0]
    rng = np.random.default_rng(SEED + 1)
    body = np.where(ob != 0, rng.integers(0, NBODIES + 1, size=ob.shape), 0).astype(np.int32)
    src = _fluid_source(ob)
    for jj in (ny - 3, ny - 2, ny - 1):
        cols = np.flatnonzero(src[jj])
        body[jj, cols] = 1 + (np.arange(len(cols)) + jj) % NBODIES
    return body


def _edges(path):
    """(columns, rows) either side of every wave-strip, chunk, tile and slab edge of the path"""
    nx, ny, K, options, _, kw, kind = PATHS[path]
    opt = dict(options)
    cols, rows = set(), set()
    if kind == "wave":
        vw = (64 - 2 * K) * opt.get("wave_cols", 1)               # the columns a wave delivers
        cols |= {c for c in range(vw - 1, nx, vw)} | {c for c in range(vw, nx, vw)}
        h = opt.get("wave_rows", 0)
        if h:
            rows |= {r for r in range(h - 1, ny, h)} | {r for r in range(h, ny, h)}
    if kind == "tiles":
        cols |= {63, 64}
        edges = {1, 2, 4, 8, 16, 32, 64}                          # rows per wavefront and per tile of every tiling
        if "regtile" in opt:
            edges |= {opt["regtile"] // 10, opt["regtile"] % 10}
        rows |= {r - 1 for r in edges if r < ny} | {r for r in edges if r < ny}
    for s in range(1, kw.get("nslabs", 1)):
        r = s * ny // kw["nslabs"]
        rows |= {r - 1, r}
    return sorted(c for c in cols if c < nx), sorted(r for r in rows if r < ny)


def _probes(path, ob):
    """About 64 probes: the corners and the middles of rows 0 / ny-1 and columns 0 / nx-1; 16 fluid cells of row ny-2 and
    its blocked cells; blocked cells across the lattice; both sides of every edge of _edges, in rows 1, ny-3, ny-2 and the
    middle (columns) and in columns 0, 63 / 64 or the middle (rows); 20 cells at random; shuffled."""
    nx, ny = PATHS[path][:2]
    cells = {(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (nx // 2, 0), (nx // 2, ny - 1), (0, ny // 2), (nx - 1, ny // 2)}
    fluid = np.flatnonzero(ob[ny - 2] == 0)
    cells |= {(int(c), ny - 2) for c in fluid[np.linspace(0, len(fluid) - 1, 16).astype(int)]}
    cells |= {(int(c), ny - 2) for c in np.flatnonzero(ob[ny - 2] != 0)[:3]}
    blocked = np.argwhere(ob != 0)
    cells |= {(int(c), int(r)) for r, c in blocked[:: max(len(blocked) // 6, 1)][:6]}
    ecols, erows = _edges(path)
    for c in ecols:
        cells |= {(c, 1), (c, ny // 2), (c, ny - 3), (c, ny - 2)}
    for r in erows:
        cells |= {(0, r), (ecols[0] if ecols else nx // 2, r), (ecols[1] if len(ecols) > 1 else nx // 2 + 1, r)}
    rng = np.random.default_rng(5)
    cells |= {(int(c), int(r)) for c, r in zip(rng.integers(0, nx, 20), rng.integers(0, ny, 20))}
    xy = np.array(sorted(cells), dtype=np.int32)
    return xy[rng.permutation(len(xy))]


_CASE = {}


def _case(path, point):
    """(nx, ny, K, nsteps, (probes_every, mean_every, fields_every), state kind, obstacles, cells0, bodies, probes)"""
    if (path, point) not in _CASE:
        nx, ny, K = PATHS[path][:3]
        kind = STATE[point]
        ob, cells = param_state(point, nx, ny, _seed(nx, ny), kind)
        n = _nsteps(K, point)
        for a in (ob, cells):
            a.setflags(write=False)
        _CASE[(path, point)] = (nx, ny, K, n, _periods(K, n), kind, ob, cells, _bodies(ob), _probes(path, ob))
    return _CASE[(path, point)]


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_the_table_holds_every_path_at_every_compulsory_point():
    assert set(FROM_ENGINES) <= set(ENGINES) and len(PATHS) == 20
    for name in ("sweep2", "march", "wave4", "wave6", "wave8", "wave8_cols2", "regtile", "regtile_8x4", "regtile_4x2",
                 "regtile_async_16x2", "regtile_sync_8x2", "regtile_ieee", "regtile_slabs_copy", "regtile_slabs_p2p",
                 "slabs_inside_copy", "slabs_first_row_p2p", "rccl_ring_of_one", "one_step", "wave6_partial_column",
                 "wave8_cols2_ragged"):
        assert name in PATHS
        for point in COMPULSORY:
            assert (name, point) in CASES
    assert PATHS["one_step"][:2] == (128, 64) and PATHS["wave6_partial_column"][:3] == (200, 72, 6)
    assert PATHS["wave8_cols2_ragged"][:3] == (256, 64, 8) and ("wave_rows", 24) in PATHS["wave8_cols2_ragged"][3]
    assert all(nx <= 256 and ny <= 256 for nx, ny, *_ in PATHS.values())
    assert PARAM_GRID["stability_edge"][0] == 0.37 and PARAM_GRID["light_fluid"][0] == 0.02 and PARAM_GRID["refusal"][0] == 0.1
    for point in ROTATED:
        kinds = [PATHS[p][6] for p, pt in CASES if pt == point]
        assert len(kinds) >= 4 and "wave" in kinds and "tiles" in kinds, (point, kinds)
    for point, kind in STATE.items():
        assert kind in (("rest", "guard") if point in REFUSING else ("guard", "perturbed"))
    assert len(CASES) == len(set(CASES)) == 80
    # the register tiles at R = 1, 2, 4, both loops, both maths
    r = {dict(PATHS[p][3]).get("regtile", 0) % 10 for p in PATHS if PATHS[p][6] == "tiles"}
    assert {2, 4} <= r and dict(PATHS["regtile_async_16x2"][3])["regtile_async"] == 1
    assert dict(PATHS["regtile_sync_8x2"][3])["regtile_async"] == 0 and dict(PATHS["regtile_ieee"][3])["kernel_variant"] == 0


_TRAJECTORY = {}


def _trajectory(O, oracle, nx, ny, point, kind, nsteps, start=None):
    """The float oracle's run of the case: per step t = 1..n (min fluid rho / rho0, max |f| / rho0, the fluid cells of
    row ny-2 that step's accelerate refused).  start: (obstacles, cells0, (density, accel, omega)) of a point that
    PARAM_GRID does not hold (tests/test_stats_param_space.py)."""
    key = (nx, ny, point, kind)
    if key not in _TRAJECTORY or len(_TRAJECTORY[key]) < nsteps:
        if start is None:
            ob, cells = param_state(point, nx, ny, _seed(nx, ny), kind)
            prm = _orc_param(O, point, nx, ny)
            rho0 = float(np.float32(PARAM_GRID[point][0]))
        else:
            ob, cells, triple = start
            prm = O.OrcParam(nx, ny, 100, 10, *(float(np.float32(v)) for v in triple))
            rho0 = float(np.float32(triple[0]))
        a, b, out = cells.copy(), np.empty_like(cells), []
        for _ in range(max(nsteps, 21)):
            ref = refused(prm.density, prm.accel, ob, a)
            oracle.timestep(prm, a, b, ob)
            a, b = b, a
            assert np.all(np.isfinite(a))
            rho = a.astype(np.float64).sum(axis=-1)[ob == 0]
            out.append((float(rho.min()) / rho0, float(np.abs(a).max()) / rho0, ref))
        _TRAJECTORY[key] = out
    return _TRAJECTORY[key][:nsteps]


@pytest.mark.parametrize("path,point", CASES)
def test_case_holds_what_it_claims(O, oracle, path, point):
    """Tame over its run on the float oracle; refusing where it says so -- inside a full pass at a step >= 2, and at a
    probes' sample step a probed fluid cell of row ny-2 refused and another accepted; every body with counted cells in rows
    ny-3 .. ny-1; probes of every kind; periods with every kind of sample step."""
    nx, ny, K, n, (pe, me, se), kind, ob, cells, body, xy = _case(path, point)
    assert (K + 5 if point in REFUSING else 2 * K + 5) <= n <= (16 if point in REFUSING else 3 * K + 5), n
    steps = _trajectory(O, oracle, nx, ny, point, kind, n)
    assert min(s[0] for s in steps) >= 0.25 and max(s[1] for s in steps) <= 1.0, [(round(s[0], 2), round(s[1], 2)) for s in steps]
    probed = np.zeros(nx, bool)
    probed[xy[xy[:, 1] == ny - 2, 0]] = True
    probed &= ob[ny - 2] == 0
    if point in REFUSING:
        full = n // K * K
        assert not steps[0][2].any()                               # from rest: step 1 refuses nothing
        assert any(steps[t - 1][2].any() for t in range(2, full + 1)), "no refusal inside a full pass"
        assert any((steps[t - 1][2] & probed).any() and (~steps[t - 1][2] & probed).any() for t in range(pe, n + 1, pe)), \
            "no probes' sample step with a refused and an accepted probe in row ny-2"
    elif kind == "guard":
        assert steps[0][2].sum() >= 5
    # bodies
    counted = _fluid_source(ob) & (body > 0)
    assert np.all(body[ob == 0] == 0) and set(np.unique(body)) == set(range(NBODIES + 1))
    for jj in (ny - 3, ny - 2, ny - 1):
        for b in range(1, NBODIES + 1):
            assert np.any(counted[jj] & (body[jj] == b)), (jj, b)
    # probes
    assert len(np.unique(xy, axis=0)) == len(xy) and 40 <= len(xy) <= 100, len(xy)
    at = ob[xy[:, 1], xy[:, 0]]
    assert np.any(at != 0) and probed.sum() >= 8
    assert {0, ny - 1} <= set(xy[:, 1].tolist()) and {0, nx - 1} <= set(xy[:, 0].tolist())
    ecols, erows = _edges(path)
    assert set(ecols) <= set(xy[:, 0].tolist()) and set(erows) <= set(xy[:, 1].tolist())
    kindp = PATHS[path][6]
    if kindp == "wave":
        assert len(ecols) >= 2 and (ecols[0] + 1) % (64 - 2 * K) == 0
    if kindp == "tiles":
        assert {63, 64} <= set(ecols) and len(erows) >= 4
    if "nslabs" in PATHS[path][5]:
        assert len(erows) >= 2
    if path == "wave8_cols2_ragged":
        assert {23, 24, 47, 48} <= set(erows)
    if path == "wave6_partial_column":
        assert nx % (64 - 2 * K) not in (0, 64 - 2 * K) and nx % 64
    # periods
    for every in (pe, me, se):
        assert n // every >= 1
        if K > 1:
            assert all(_placement(K, n, every)), (K, n, every)
    m = n // me
    assert m >= 3 and not _power_of_two(m), (n, me)


# ---------------------------------------------------------------------------------------------------------------- GPU
WAVE_KEYS = ("forces_in_wave", "probes_in_wave", "samples_in_wave", "mean_in_wave")
TILE_KEYS = ("forces_in_kernel", "probes_in_kernel", "samples_in_kernel", "mean_in_kernel")
SINGLE = {"forces": 0, "probes": 1, "fields": 2, "mean": 3}          # index into WAVE_KEYS / TILE_KEYS
WORST = {"fields": 0.0, "forces": 0.0, "mean": 0.0}


def _open(L, path, p, ob, cells, body, xy, monkeypatch):
    _, _, _, options, _, kw, _ = PATHS[path]
    if kw.get("rccl"):
        monkeypatch.setenv("LBM_FORCE_EXCHANGE", "1")
        lat_kw = dict(rank=0, nranks=1, device=0, unique_id=L.rccl_unique_id(), exchange=L.EXCHANGE_RCCL)
    elif kw:
        ex = L.EXCHANGE_COPY if kw["exchange"] == "copy" else L.EXCHANGE_P2P
        lat_kw = dict(nslabs=kw["nslabs"], devices=[0] * kw["nslabs"], exchange=ex)
    else:
        lat_kw = {}
    lat = L.Lattice(p, ob, cells, **lat_kw)
    for key, v in options:
        lat.set_option(key, v)
    lat.set_bodies(body, NBODIES)
    lat.set_probes(xy)
    return lat


_REF = {}


def _reference(L, O, path, point):
    """Once per (shape, point, state, maths): S_t, X_t and av_vels of the one-step kernel for the longest run any case
    needs there, X_t held to the double oracle; the float64 forces of S_t with their rounding scale; the forces of
    lbm_run_forces on the one-step path."""
    nx, ny, K, n, _, kind, ob, cells, body, _ = _case(path, point)
    variant = dict(PATHS[path][3]).get("kernel_variant")
    key = (nx, ny, point, kind, variant)
    if key not in _REF:
        nmax = max(_case(q, pt)[3] for q, pt in CASES
                   if pt == point and PATHS[q][:2] == (nx, ny) and dict(PATHS[q][3]).get("kernel_variant") == variant)
        _REF[key] = _reference_run(L, O, key, ob, cells, body, _lparam(L, point, nx, ny), _orc_param(O, point, nx, ny), nmax)
    return _REF[key]


def _reference_run(L, O, key, ob, cells, body, p, prm, nmax):
    """_reference's run: key = (nx, ny, point, state, maths) names it; p and prm the parameters of the library and the oracle
    (tests/test_stats_param_space.py runs it at a point that PARAM_GRID does not hold)."""
    nx, ny, point, kind, variant = key
    o64 = O.Oracle("strict")
    opts = [("engine", 1), ("time_block", 1)] + ([("kernel_variant", variant)] if variant is not None else [])
    S, X, F64, A, av, worst = [], [], [], [], [], 0.0
    with L.Lattice(p, ob, cells) as lat:
        for k, v in opts:
            lat.set_option(k, v)
        for t in range(1, nmax + 1):
            av.append(lat.run(1))
            st, x = lat.read_state(), lat.final_state()
            assert lat.info("engine_last") == 1 and lat.info("time_block_active") == 1
            fo = o64.final_state(prm, st.astype(np.float64), ob).reshape(ny, nx, 4)
            err, bar = np.abs(x - fo), 2e-6 * np.abs(fo) + 8 * U
            worst = max(worst, float(np.max(err / bar)))
            assert np.all(err <= bar), (key, t, float(np.max(err / bar)))
            f, a = forces_from_state(st, ob, body, NBODIES)
            S.append(st), X.append(x), F64.append(f), A.append(a)
    with L.Lattice(p, ob, cells) as lat:
        for k, v in opts:
            lat.set_option(k, v)
        lat.set_bodies(body, NBODIES)
        av1, F1 = lat.run_forces(nmax)
        assert lat.info("engine_last") == 1 and lat.info("forces_in_kernel") == 0 and lat.info("forces_in_wave") == 0
    assert np.array_equal(_bits(av1), _bits(np.concatenate(av)))
    ref = dict(S=np.stack(S), X=np.stack(X), F64=np.array(F64), A=np.array(A), av=np.concatenate(av), F1=F1)
    for a in ref.values():
        a.setflags(write=False)
    WORST["fields"] = max(WORST["fields"], worst)
    print(f"reference {nx}x{ny} {point} {kind}: {nmax} steps, worst |X_t - f64| {worst:.3f} of its bar")
    return ref


def _expected_info(path, call, K, n, pe, me, se):
    """The observer keys after `call`: "forces" / "probes" / "fields" / "mean" (the single calls), "all" (lbm_run_observed
    with the four), "pair" (with forces and probes)."""
    kind = PATHS[path][6]
    want = {}
    if call == "plain":
        return want
    if call in SINGLE:
        i = SINGLE[call]
        want[WAVE_KEYS[i]] = 1 if kind == "wave" else 0
        want[TILE_KEYS[i]] = 1 if kind == "tiles" else 0
    elif call == "pair":
        want["observed_in_wave"] = 3 if kind == "wave" else 0
        want["observed_in_kernel"] = 3 if kind == "tiles" else 0
        if kind != "split":
            want["observed_pieces"] = 1
    else:
        # the pieces end on the sample steps of the means and the snapshots; lbm_wave takes a piece of K steps or more
        # (and of the probes where neither the register tiles nor lbm_wave take them)
        cuts = sorted({n} | set(range(me, n + 1, me)) | set(range(se, n + 1, se)) | (set(range(pe, n + 1, pe)) if kind == "split" else set()))
        pieces = np.diff([0] + cuts)
        want["observed_pieces"] = len(pieces)
        want["observed_in_wave"] = 3 if kind == "wave" and pieces.max() >= K else 0
        want["observed_in_kernel"] = 3 if kind == "tiles" else 0
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("path,point", CASES)
def test_observers_on_the_parameter_grid(gpu, O, monkeypatch, path, point):
    L = gpu
    nx, ny, K, n, (pe, me, se), kind, ob, cells, body, xy = _case(path, point)
    _, _, _, options, info_want, kw, pkind = PATHS[path]
    ref = _reference(L, O, path, point)
    p = _lparam(L, point, nx, ny)
    where = (path, point, n, pe, me, se)

    def call(name, fn):
        with _open(L, path, p, ob, cells, body, xy, monkeypatch) as lat:
            if kw.get("rccl"):
                assert lat.slab_rows(0) == (0, ny)                # every probe lies in the rank's own rows
            out = fn(lat)
            got = {k: int(lat.info(k)) for k in _expected_info(path, name, K, n, pe, me, se)}
            assert got == _expected_info(path, name, K, n, pe, me, se), (where, name, got)
            for key, v in info_want.items():
                if key == "exchange":
                    v = {"rccl": L.EXCHANGE_RCCL}[v]
                assert lat.info(key) == v, (where, name, key, lat.info(key))
            st = lat.read_state()
        if name != "plain":
            assert np.array_equal(_bits(st), _bits(st0)), (where, name, "lattice")
        return out, st

    av0, st0 = call("plain", lambda lat: lat.run(n))
    assert np.array_equal(_bits(st0), _bits(ref["S"][n - 1])), (where, "the lattice of the one-step kernel")

    def check_av(name, av):
        exact = pkind == "tiles" or (pkind == "wave" and name != "all")
        if exact:
            assert np.array_equal(_bits(av), _bits(av0)), (where, name, "av_vels")
        assert np.allclose(av, av0, rtol=2e-6, atol=0), (where, name, "av_vels")

    # 1. snapshots
    (av, fields), _ = call("fields", lambda lat: lat.run_sampled(n, se))
    check_av("fields", av)
    want = ref["X"][se - 1:n:se][:n // se]
    assert fields.shape == want.shape and np.array_equal(_bits(fields), _bits(want)), (where, "snapshots")
    # 2. probes
    (av, probes), _ = call("probes", lambda lat: lat.run_probes(n, pe))
    check_av("probes", av)
    want = ref["X"][pe - 1:n:pe][:n // pe][:, xy[:, 1], xy[:, 0]]
    assert probes.shape == want.shape == (n // pe, len(xy), 4)
    bad = np.argwhere(_bits(probes) != _bits(want))
    assert len(bad) == 0, (where, "probes", len(bad), [(int(j), tuple(xy[i]), int(k)) for j, i, k in bad[:8]])
    blocked = ob[xy[:, 1], xy[:, 0]] != 0
    const = np.array([0.0, 0.0, 0.0, np.float32(p.density) * ONE_THIRD], dtype=np.float32)
    assert blocked.any() and np.all(_bits(probes[:, blocked]) == _bits(const)), (where, "blocked probes")
    # 3. mean
    (av, mean), _ = call("mean", lambda lat: lat.run_mean(n, me))
    check_av("mean", av)
    Xm = ref["X"][me - 1:n:me][:n // me]
    m = len(Xm)
    bad = np.argwhere(_bits(mean) != _bits(mean_of(Xm)))
    assert len(bad) == 0, (where, "mean", len(bad), [tuple(int(v) for v in b) for b in bad[:8]])
    X64 = Xm.astype(np.float64)
    err = np.abs(mean.astype(np.float64) - X64.mean(axis=0))
    lim = (m - 1) * U * np.abs(X64).sum(axis=0) + U * np.abs(mean.astype(np.float64))
    worst_mean = float(np.max(err / np.maximum(lim, 1e-300)))
    assert np.all(err <= lim), (where, "mean against float64", worst_mean)
    # 4. forces
    (av, F), _ = call("forces", lambda lat: lat.run_forces(n))
    check_av("forces", av)
    assert F.shape == (n, NBODIES, 2)
    worst_force = float(np.max(np.abs(F - ref["F64"][:n]) / np.maximum(ref["A"][:n], 1e-30)))
    if path in FORCE_BITS:
        assert np.array_equal(_bits(F), _bits(ref["F1"][:n])), (where, "forces", float(np.abs(F - ref["F1"][:n]).max()))
    assert _close(F, ref["F64"][:n], ref["A"][:n]), (where, "forces against float64", worst_force)
    if point in REFUSING:
        # (step 1 from rest refuses nothing: test_case_holds_what_it_claims)
        f0 = np.abs(F[0]).max(axis=1)
        moved = (np.abs(F[1:] - F[0]).max(axis=2) > 0.1 * f0) & (f0 > 0)
        assert moved.any(), (where, "the forces do not feel the refusals")
    # 5. all four in one run, and forces with probes alone
    res, _ = call("all", lambda lat: lat.run_observed(n, forces=True, probes_every=pe, mean_every=me, fields_every=se))
    check_av("all", res["av_vels"])
    for name, single in (("forces", F), ("probes", probes), ("mean", mean), ("fields", fields)):
        assert res[name].shape == single.shape and np.array_equal(_bits(res[name]), _bits(single)), (where, "observed", name)
    res, _ = call("pair", lambda lat: lat.run_observed(n, forces=True, probes_every=pe))
    check_av("pair", res["av_vels"])
    for name, single in (("forces", F), ("probes", probes)):
        assert res[name].shape == single.shape and np.array_equal(_bits(res[name]), _bits(single)), (where, "forces + probes", name)
    WORST["forces"] = max(WORST["forces"], worst_force / 1e-5)
    WORST["mean"] = max(WORST["mean"], worst_mean)
    print(f"{path} {point}: {n} steps, periods {pe}/{me}/{se}; forces {worst_force / 1e-5:.4f} of the 1e-5 scale bar, mean"
          f" {worst_mean:.3f} of its bound; worst so far: X_t {WORST['fields']:.3f} of its bar, forces {WORST['forces']:.4f},"
          f" mean {WORST['mean']:.3f}")
