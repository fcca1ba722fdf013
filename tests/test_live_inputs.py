"""lbm_set_obstacles and lbm_write_state: the obstacle map and the lattice as live inputs of a context
(Lattice.set_obstacles, Lattice.write_state).

The yardstick is the definition (include/lbm_mi355x.h).  A LIVE context runs n1 steps from (A, S0), then takes
set_obstacles(B, refill) or write_state(W).  A FRESH context is created from (B, S') -- S' made here in numpy from the state
read just before the call -- or from (A, W), under the same options, acceleration and probe set.  Both are issued the same
later calls; every output, the final read_state and the scalar results are compared as bit patterns, and the info keys say
which kernels ran: a silent fallback fails the test.

CASES is the table of (path, input): COVERAGE, checked without a GPU, names what every path must run, so trimming the GPU
cases fails there.  The lbm_wave paths of the table run in tests/test_wave_live_inputs.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, deck_paths
from test_sampled_run import TILINGS

LBM_EINVAL, LBM_ENODEV = 1, 2
KEEP, REST = 0, 1
INPUTS = ("keep", "rest", "write")
W_EQ = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float32)
WAVE_KERNELS = [(4, 1), (6, 1), (8, 1), (8, 2)]                 # KERNELS and SHAPES of tests/test_wave_fields.py
WAVE_SHAPES = [(256, 64, 11), (200, 72, 12)]
WAVE_ROWS = 24                                                  # chunk edges at rows 24 and 48


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------- the table
def _tile_opts(ty, r, asy):
    return (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3))


def _wave_opts(K, cols):
    return (("engine", 1), ("march_kernel", 1), ("time_block", K), ("wave_cols", cols), ("wave_rows", WAVE_ROWS))


FULL = ("run", "probes", "forces", "window", "driven_observed")
BASIC = ("run", "probes")
# path -> (nx, ny, seed, options, Lattice kwargs by name, steps per pass, the later calls, info that must hold after "run")
PATHS = {"tiles_deck_128x128": (128, 128, 31, (), None, 1, FULL, {"engine_last": 3})}
for _ty, _r, _asy, _nx, _ny in TILINGS:
    PATHS["tiles_%dx%d_%d_%d_%d" % (_nx, _ny, _ty, _r, _asy)] = (_nx, _ny, 32, _tile_opts(_ty, _r, _asy), None, 1, FULL, {"engine_last": 3})
for _n, _ex in ((2, "copy"), (4, "copy"), (2, "p2p")):
    PATHS["slabs_%d_%s" % (_n, _ex)] = (256, 256, 33, (), (_n, _ex), 1, BASIC, {"engine_last": 3} if _ex == "p2p" else {})
PATHS["one_step"] = (128, 16, 34, (("engine", 1), ("time_block", 1)), None, 1, BASIC, {"engine_last": 1, "time_block_active": 1})
PATHS["two_step"] = (128, 16, 34, (("engine", 1), ("time_block", 2)), None, 2, BASIC, {"engine_last": 1, "time_block_active": 2})
PATHS["lbm_march"] = (256, 64, 11, (("engine", 1), ("march_kernel", 0), ("time_block", 4), ("wave_cols", 1)), None, 4, BASIC,
                      {"engine_last": 1, "time_block_active": 4, "march_kernel": 0})
for _K, _cols in WAVE_KERNELS:
    for _nx, _ny, _seed in WAVE_SHAPES:
        PATHS["wave%d_cols%d_%dx%d" % (_K, _cols, _nx, _ny)] = (
            _nx, _ny, _seed, _wave_opts(_K, _cols), None, _K, FULL,
            {"engine_last": 1, "time_block_active": _K, "march_kernel": 1, "wave_cols_active": _cols, "wave_rows": WAVE_ROWS})
CASES = [(path, inp) for path in PATHS for inp in INPUTS]
WAVE_CASES = [c for c in CASES if c[0].startswith("wave")]
HERE_CASES = [c for c in CASES if not c[0].startswith("wave")]

# what the issue asks of every family of paths: (prefix of the path's name, how many paths, the later calls)
COVERAGE = (("tiles_deck", 1, FULL), ("tiles_", 1 + len(TILINGS), FULL), ("slabs_", 3, BASIC), ("one_step", 1, BASIC),
            ("two_step", 1, BASIC), ("lbm_march", 1, BASIC), ("wave", len(WAVE_KERNELS) * len(WAVE_SHAPES), FULL))
# the info key that says a later call ran where its path should run it: family -> call -> (key, value)
IN_KERNEL = {
    "tiles": {"probes": ("probes_in_kernel", 1), "forces": ("forces_in_kernel", 1), "window": ("window_in_kernel", 1),
              "driven_observed": ("driven_observed_in_kernel", 3)},
    "wave": {"probes": ("probes_in_wave", 1), "forces": ("forces_in_wave", 1), "window": ("window_in_wave", 1),
             "driven_observed": ("driven_observed_in_wave", 3)},
}


def n1_of(K, inp):
    """Steps before the input: odd under "keep" and "write", at least one full pass of the path's kernel."""
    return {"keep": 2 * K + 1, "rest": K + 2, "write": 2 * K + 3}[inp]


# ---------------------------------------------------------------------------------------------------------------- the inputs
def maps_and_states(nx, ny, seed, borders=()):
    """(A, B, S0, W): two random maps at about 10 % blocked with different fluid counts, B blocking cells of the accelerate
    row and differing from A in rows 0 and ny - 1 and either side of every row in `borders`; two random lattices."""
    rng = np.random.default_rng(seed)
    A = (rng.random((ny, nx)) < 0.10).astype(np.int32)
    B = (rng.random((ny, nx)) < 0.12).astype(np.int32)
    S0 = (0.1 * W_EQ * (1.0 + 0.2 * (rng.random((ny, nx, 9), dtype=np.float32) - 0.5))).astype(np.float32)
    W = (0.1 * W_EQ * (1.0 + 0.2 * (rng.random((ny, nx, 9), dtype=np.float32) - 0.5))).astype(np.float32)
    assert (A == 0).sum() != (B == 0).sum() and B[ny - 2].any()
    for row in (0, ny - 1) + tuple(r for b in borders for r in (b - 1, b)):
        assert (A[row] != B[row]).any() and ((A[row] != 0) & (B[row] == 0)).any(), row
    return A, B, S0, W


def refilled(old, new):
    return (np.asarray(old) != 0) & (np.asarray(new) == 0)


def rest_values(density):
    """The nine rest values in float, by the C expressions: density * 4.f / 9.f, density / 9.f, density / 36.f."""
    d = np.float32(density)
    w0, w1, w2 = d * np.float32(4) / np.float32(9), d / np.float32(9), d / np.float32(36)
    return np.array([w0] + [w1] * 4 + [w2] * 4, dtype=np.float32)


def s_prime(S, old, new, refill, density):
    out = np.array(S, dtype=np.float32, copy=True)
    if refill == REST:
        out[refilled(old, new)] = rest_values(density)
    return out


def probe_set(A, B, seed):
    """Seven cells: one that A leaves fluid and B blocks, one in row 0, one in the accelerate row, four anywhere."""
    ny, nx = A.shape
    rng = np.random.default_rng(seed + 1000)
    ys, xs = np.nonzero(((A == 0) & (B != 0))[1:ny - 2])
    xy = [(int(xs[0]), int(ys[0]) + 1), (3, 0), (nx - 2, ny - 2)]
    while len(xy) < 7:
        q = (int(rng.integers(nx)), int(rng.integers(ny)))
        if q not in xy:
            xy.append(q)
    return np.array(xy, dtype=np.int32)


def labels(ob, nb=3):
    """Labels 1..nb on the blocked cells, by column band; the cells of row 0 are left uncounted (label 0)."""
    ny, nx = ob.shape
    lab = np.where(ob != 0, 1 + (np.arange(nx)[None, :] * nb // nx), 0).astype(np.int32)
    lab[0] = 0
    return lab


def _kwargs(L, kind):
    if kind is None:
        return {}
    n, ex = kind
    return dict(nslabs=n, devices=[0] * n, exchange=L.EXCHANGE_COPY if ex == "copy" else L.EXCHANGE_P2P)


def _borders(ny, kind):
    return () if kind is None else tuple(i * ny // kind[0] for i in range(1, kind[0]))


def _context(L, p, ob, cells, options, xy, accel, **kw):
    lat = L.Lattice(p, ob, cells, **kw)
    for k, v in options:
        lat.set_option(k, v)
    lat.set_accel(accel)
    lat.set_probes(xy)
    return lat


def later_calls(L, lat, path, ob, n2, relabel):
    """The later calls of the path on `lat`, whose map is ob: (outputs by name, info by name).  relabel: lbm_set_bodies on ob
    in front of the forces run (else the labelling the context holds must serve)."""
    nx, ny, _, _, _, K, calls, want = PATHS[path]
    family = "tiles" if path.startswith("tiles") else "wave" if path.startswith("wave") else None
    out, info = {}, {}
    for call in calls:
        launches = lat.info("wave_launches")
        if call == "run":
            out["run.av"] = lat.run(n2)
            info[call] = {k: int(lat.info(k)) for k in ("engine_last", "time_block_active", "march_kernel", "wave_cols_active", "wave_rows")}
            assert {k: info[call][k] for k in want} == want, (path, info[call])
        elif call == "probes":
            out["probes.av"], out["probes"] = lat.run_probes(n2, 3)
        elif call == "forces":
            if relabel:
                lat.set_bodies(labels(ob), 3)
            out["forces.av"], out["forces"] = lat.run_forces(n2)
        elif call == "window":
            out["window.av"], out["window"] = lat.run_window(n2, 3, L.Window(5, 0, nx // 4, ny // 2, 3, 2))
        elif call == "driven_observed":
            t = np.arange(n2)
            sched = (lat.info("accel") * (1 + 0.5 * np.sin(2 * np.pi * t / 7))).astype(np.float32)
            res = lat.run_driven_observed(sched, forces=True, probes_every=2)
            for k, v in res.items():
                out["driven_observed." + k] = v
        if family and call in IN_KERNEL[family]:
            key, value = IN_KERNEL[family][call]
            info[call] = {key: int(lat.info(key)), "engine_last": int(lat.info("engine_last"))}
            assert info[call][key] == value, (path, call, info[call])
        if family == "wave":
            assert lat.info("wave_launches") > launches, (path, call)
        out[call + ".state"] = lat.read_state()
    out["final_state"] = lat.final_state()
    out["av_velocity"] = np.array([lat.av_velocity()], dtype=np.float32)
    out["reynolds"] = np.array([lat.reynolds()], dtype=np.float32)
    out["total_density"] = np.array([lat.total_density()], dtype=np.float64)
    out["fluid_cells"] = np.array([lat.info("fluid_cells")], dtype=np.float64)
    return out, info


def check_case(L, path, inp):
    nx, ny, seed, options, kind, K, calls, _ = PATHS[path]
    kw = _kwargs(L, kind)
    p = L.Param(nx, ny, 100, 10, 0.1, 0.01, 1.85)
    if path == "tiles_deck_128x128":
        p = L.read_params(deck_paths("128x128")[0])
    A, B, S0, W = maps_and_states(nx, ny, seed, _borders(ny, kind))
    xy = probe_set(A, B, seed)
    accel = 0.0137                                       # (lbm_set_accel's value, not lbm_create's: it must survive)
    n1, n2 = n1_of(K, inp), 2 * K + 5
    lib = L.load_library()
    with _context(L, p, A, S0, options, xy, accel, **kw) as live:
        live.set_bodies(labels(A), 3)
        live.run(n1)
        S = live.read_state()
        if inp == "write":
            live.write_state(W)
            assert _same(live.read_state(), W)
            new_map, start = A, W
            assert live.info("obstacle_updates") == 0
        else:
            refill = KEEP if inp == "keep" else REST
            live.set_obstacles(B, refill)
            new_map, start = B, s_prime(S, A, B, refill, p.density)
            assert _same(live.read_state(), start)      # ("keep": S itself, bit for bit)
            assert live.info("obstacle_updates") == 1
            assert live.info("refilled_cells") == (int(refilled(A, B).sum()) if refill == REST else 0)
            assert live.info("fluid_cells") == int((B == 0).sum())
            # the bodies went with the map: a forces run is refused until they are set again
            av = np.empty(2, np.float32)
            f = np.empty((2, 3, 2), np.float32)
            assert lib.lbm_run_forces(live._ctx, 2, av.ctypes.data, f.ctypes.data) == LBM_EINVAL
            assert b"no bodies" in lib.lbm_last_error()
            assert _same(live.read_state(), start)
        assert np.float32(live.info("accel")) == np.float32(accel)
        got, info = later_calls(L, live, path, new_map, n2, inp != "write")
    with _context(L, p, new_map, start, options, xy, accel, **kw) as fresh:
        if inp == "write":
            fresh.set_bodies(labels(A), 3)              # (write_state keeps the bodies)
        want, info_f = later_calls(L, fresh, path, new_map, n2, inp != "write")
    assert info == info_f, (path, inp, info, info_f)
    assert sorted(got) == sorted(want)
    for k in want:
        assert _same(got[k], want[k]), (path, inp, k, info)
    assert np.all(np.isfinite(want[calls[-1] + ".state"]))


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_live_inputs_are_declared_exported_and_bound(L):
    assert "lbm_set_obstacles" in L.ABI_SYMBOLS and "lbm_write_state" in L.ABI_SYMBOLS
    hdr = open(L.HEADER_PATH).read()
    assert "int lbm_set_obstacles(lbm_ctx* ctx, const int* obstacles, int refill);" in hdr
    assert "int lbm_write_state(lbm_ctx* ctx, const float* cells);" in hdr
    assert "#define LBM_REFILL_KEEP 0" in hdr and "#define LBM_REFILL_REST 1" in hdr
    assert (L.REFILL_KEEP, L.REFILL_REST) == (KEEP, REST)
    lib = L.load_library()
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "lbm_set_obstacles") and hasattr(raw, "lbm_write_state")
    assert lib.lbm_set_obstacles.argtypes == [C.c_void_p, C.c_void_p, C.c_int] and lib.lbm_set_obstacles.restype == C.c_int
    assert lib.lbm_write_state.argtypes == [C.c_void_p, C.c_void_p] and lib.lbm_write_state.restype == C.c_int
    built = open(L.LIB_PATH, "rb").read()
    for key in (b"obstacle_updates", b"refilled_cells"):
        assert '"%s"' % key.decode() in hdr, key
        assert key + b"\0" in built, key
    assert "refilled_cells" in L.Lattice.set_obstacles.__doc__ and "read_state" in L.Lattice.write_state.__doc__


def test_null_arguments_are_refused_and_no_device_is_an_error(L):
    lib = L.load_library()
    ob = np.zeros((8, 8), np.int32)
    cells = np.zeros((8, 8, 9), np.float32)
    assert lib.lbm_set_obstacles(None, ob.ctypes.data, KEEP) == LBM_EINVAL and b"ctx" in lib.lbm_last_error()
    assert lib.lbm_set_obstacles(None, None, REST) == LBM_EINVAL
    assert lib.lbm_write_state(None, cells.ctypes.data) == LBM_EINVAL and b"NULL" in lib.lbm_last_error()
    assert lib.lbm_write_state(None, None) == LBM_EINVAL
    if L.device_count() == 0:
        # (as tests/test_abi.py: without a device there is no context to give either call, and creating one says why)
        ctx = C.c_void_p()
        p = L.Param(8, 8, 1, 1, 0.1, 0.005, 1.85)
        assert lib.lbm_create(C.byref(p), ob.ctypes.data, cells.ctypes.data, 1, None, 0, C.byref(ctx)) == LBM_ENODEV
        assert not ctx.value


def test_write_state_refuses_what_is_no_lattice_in_python(L):
    lat = L.Lattice.__new__(L.Lattice)                   # (never created: the size check comes before the library)
    lat.params, lat.rank_mode = L.Param(8, 8, 1, 1, 0.1, 0.005, 1.85), False
    with pytest.raises(L.LbmError, match="expected 576"):
        L.Lattice.write_state(lat, np.zeros((8, 8, 8), np.float32))
    with pytest.raises(L.LbmError, match="64 cells"):
        L.Lattice.set_obstacles(lat, np.zeros((8, 7), np.int32))


def test_the_cases_cover_every_path_input_and_later_call():
    assert len(set(CASES)) == len(CASES) == len(PATHS) * len(INPUTS)
    assert sorted(HERE_CASES + WAVE_CASES) == sorted(CASES)
    for prefix, count, calls in COVERAGE:
        paths = [k for k in PATHS if k.startswith(prefix)]
        assert len(paths) == count, (prefix, paths)
        for k in paths:
            assert set(calls) <= set(PATHS[k][6]), k
            for inp in INPUTS:
                assert (k, inp) in CASES
            assert any(n1_of(PATHS[k][5], inp) % 2 == 1 for inp in INPUTS)
    # every (path, input, later call) of the table is a test case of one of the two files, and the in-kernel keys are named
    import test_wave_live_inputs as TW
    assert TW.CASES == WAVE_CASES
    for fam, prefix in (("tiles", "tiles"), ("wave", "wave")):
        assert set(IN_KERNEL[fam]) == set(FULL) - {"run"}
    tilings = {(PATHS[k][3][0][1], PATHS[k][3][1][1], PATHS[k][0], PATHS[k][1]) for k in PATHS if k.startswith("tiles_") and PATHS[k][3]}
    assert tilings == {(ty * 10 + r, asy, nx, ny) for ty, r, asy, nx, ny in TILINGS}
    waves = {(PATHS[k][5], PATHS[k][3][3][1], PATHS[k][0], PATHS[k][1]) for k in PATHS if k.startswith("wave")}
    assert waves == {(K, c, nx, ny) for K, c in WAVE_KERNELS for nx, ny, _ in WAVE_SHAPES}


def test_the_inputs_are_what_they_say():
    for nx, ny, kind in ((128, 16, None), (256, 256, (4, "copy")), (200, 72, None)):
        A, B, S0, W = maps_and_states(nx, ny, 5, _borders(ny, kind))
        assert 0.07 < A.mean() < 0.13 and 0.09 < B.mean() < 0.15
        xy = probe_set(A, B, 5)
        assert xy.shape == (7, 2) and len({tuple(q) for q in xy}) == 7 and A[xy[0, 1], xy[0, 0]] == 0 and B[xy[0, 1], xy[0, 0]] == 1
        Sp = s_prime(S0, A, B, REST, 0.1)
        m = refilled(A, B)
        assert m.sum() > 0 and np.array_equal(Sp[~m], S0[~m]) and np.all(Sp[m] == rest_values(0.1))
        assert _same(s_prime(S0, A, B, KEEP, 0.1), S0)
        lab = labels(B)
        assert lab.max() == 3 and not lab[0].any() and np.all((lab > 0) <= (B != 0))
    assert _borders(256, (4, "copy")) == (64, 128, 192)
    r = rest_values(0.1)
    assert r.dtype == np.float32 and r[0] == np.float32(0.1) * np.float32(4) / np.float32(9)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("path,inp", HERE_CASES)
def test_a_live_context_is_the_fresh_context(gpu, path, inp):
    check_case(gpu, path, inp)


@pytest.mark.gpu
def test_read_write_read_is_the_identity_on_bit_patterns(gpu):
    L = gpu
    A, B, S0, W = maps_and_states(128, 16, 40)
    p = L.Param(128, 16, 100, 10, 0.1, 0.01, 1.85)
    ys, xs = np.nonzero(A)
    X = W.copy()
    X[3, 5, 2] = np.float32(-0.0)
    X.view(np.uint32)[ys[0], xs[0], 4] = 0x7fc12345           # a NaN with a payload, in a blocked cell
    X.view(np.uint32)[ys[1], xs[1], 0] = 0xffa00001
    for n1 in (0, 3, 4):
        with L.Lattice(p, A, S0) as lat:
            lat.run(n1)
            lat.write_state(X)
            back = lat.read_state()
            assert np.array_equal(back.view(np.uint32), X.view(np.uint32)), n1
            lat.write_state(back)
            assert np.array_equal(lat.read_state().view(np.uint32), X.view(np.uint32)), n1
            assert np.signbit(back[3, 5, 2]) and back[3, 5, 2] == 0


@pytest.mark.gpu
def test_refusals_leave_the_context_alone(gpu):
    """Every LBM_EINVAL leaves read_state and a following run identical to a context that never saw the call."""
    L = gpu
    A, B, S0, W = maps_and_states(128, 16, 41)
    p = L.Param(128, 16, 100, 10, 0.1, 0.01, 1.85)
    lib = L.load_library()
    with L.Lattice(p, A, S0) as twin:
        twin.run(3)
        st0 = twin.read_state()
        av0, st1 = twin.run(5), twin.read_state()
    with L.Lattice(p, A, S0) as lat:
        lat.run(3)
        bad = (lambda: lib.lbm_set_obstacles(lat._ctx, None, KEEP), lambda: lib.lbm_set_obstacles(lat._ctx, B.ctypes.data, 2),
               lambda: lib.lbm_set_obstacles(lat._ctx, B.ctypes.data, -1), lambda: lib.lbm_write_state(lat._ctx, None))
        for i, call in enumerate(bad):
            assert call() == LBM_EINVAL, i
            assert _same(lat.read_state(), st0), i
            assert lat.info("obstacle_updates") == 0 and lat.info("fluid_cells") == int((A == 0).sum()), i
        av, st = lat.run(5), lat.read_state()
    assert _same(av, av0) and _same(st, st1)


_DEVICE_INPUT = r'''
import sys
import numpy as np
import torch
for p in ({root!r}, {tests!r}):
    if p not in sys.path:
        sys.path.insert(0, p)
import advanced_hpc_lbm_amd as L
from test_live_inputs import maps_and_states
A, B, S0, W = maps_and_states(128, 16, 42)
p = L.Param(128, 16, 100, 10, 0.1, 0.01, 1.85)
res = []
for on_device in (False, True):
    with L.Lattice(p, A, S0) as lat:
        lat.run(3)
        if on_device:
            t = torch.from_numpy(W).to("cuda:0")
            lat.write_state(t)
            assert np.array_equal(t.cpu().numpy().view(np.uint32), W.view(np.uint32))
            lat.write_state(int(t.data_ptr()))
        else:
            lat.write_state(W)
        a = lat.read_state()
        assert np.array_equal(a.view(np.uint32), W.view(np.uint32))
        res.append((a, lat.run(5), lat.read_state()))
for x, y in zip(*res):
    assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
print("device input ok")
'''


@pytest.mark.gpu
def test_device_input_is_the_host_input(gpu):
    from test_mean_run import _child
    assert "device input ok" in _child(_DEVICE_INPUT)


@pytest.mark.gpu
def test_a_block_moves_through_one_context(gpu, O, oracle):
    """A 6 x 6 block on the 128x128 deck moves one column east every 7 steps, 8 moves, under LBM_REFILL_REST; after each
    move it is labelled again and lbm_run_forces covers the 7 steps.  A shadow context under engine 1, time_block 1 gets the
    same calls: the lattices match bit for bit after every piece.  The pieces that end within the first 50 steps are held to
    the strict float oracle -- Oracle.run piecewise, the map swapped and the refill applied in numpy between pieces -- with
    the bars of tests/test_gpu_parity.py::test_fifty_steps_against_float_oracle (lattice 5e-5 of the largest population,
    av_vels rtol 1e-4)."""
    L = gpu
    pf, of = deck_paths("128x128")
    p = L.read_params(pf)
    deck = np.ascontiguousarray(L.read_obstacles(of, p), dtype=np.int32).reshape(p.ny, p.nx)
    op = O.read_params(pf)

    def with_block(k):
        ob, lab = deck.copy(), np.zeros_like(deck)
        ob[60:66, 20 + k:26 + k] = 1
        lab[60:66, 20 + k:26 + k] = 1
        return ob, lab

    ob, lab = with_block(0)
    cells = oracle.init_cells(op, np.float32)
    main = L.Lattice(p, ob)
    shadow = L.Lattice(p, ob)
    shadow.set_option("engine", 1)
    shadow.set_option("time_block", 1)
    steps, total_refilled = 0, 0
    with main, shadow:
        for k in range(9):
            if k > 0:
                new, lab = with_block(k)
                m = refilled(ob, new)
                for lat in (main, shadow):
                    lat.set_obstacles(new, REST)
                    assert lat.info("refilled_cells") == int(m.sum()) and lat.info("obstacle_updates") == k
                cells[m] = rest_values(p.density)
                total_refilled += int(m.sum())
                ob = new
            for lat in (main, shadow):
                lat.set_bodies(lab, 1)
            av, F = main.run_forces(7)
            av_s, F_s = shadow.run_forces(7)
            assert main.info("engine_last") == 3 and main.info("forces_in_kernel") == 1 and shadow.info("engine_last") == 1
            st = main.read_state()
            assert _same(st, shadow.read_state()), k
            assert F.shape == F_s.shape == (7, 1, 2) and np.all(np.isfinite(F)) and np.all(np.isfinite(F_s))
            steps += 7
            if steps <= 50:
                av_o = oracle.run(op, cells, ob, 7)
                print("piece %d: lattice %.3g of the largest population, av_vels %.3g relative" %
                      (k, np.abs(st - cells).max() / np.abs(cells).max(), np.max(np.abs(av - av_o) / np.abs(av_o))))
                assert np.abs(st - cells).max() <= 5e-5 * np.abs(cells).max(), k
                assert np.allclose(av, av_o, rtol=1e-4, atol=0), k
                assert np.allclose(av_s, av_o, rtol=1e-4, atol=0), k
    assert total_refilled > 0 and steps == 63


# ---------------------------------------------------------------------------------------------------------------- ranks
def _rank_worker(rank, nranks, shape, steps, conn, outdir):
    for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        if p_ not in sys.path:
            sys.path.insert(0, p_)
    os.environ["LBM_REGTILE_SLABS_NO_AGREEMENT"] = "1"     # (as tests/test_gpu_parity.py: no communicator on one GPU)
    import advanced_hpc_lbm_amd as L
    A, B, S0, W = maps_and_states(shape[0], shape[1], 43, tuple(i * shape[1] // nranks for i in range(1, nranks)))
    p = L.Param(shape[0], shape[1], 100, 10, 0.1, 0.01, 1.85)
    lat = L.Lattice(p, A, S0, rank=rank, nranks=nranks, device=0, unique_id=None, exchange=L.EXCHANGE_P2P)
    conn.send(lat.p2p_handle())
    lat.p2p_connect(conn.recv())
    r0, r1 = lat.slab_rows(0)
    lat.run(steps[0])
    lat.set_obstacles(B, REST)                             # the global map on every rank
    refilled_here = int(lat.info("refilled_cells"))
    conn.send(("updated", refilled_here))
    conn.recv()                                            # the test's barrier: every rank has returned from the call
    lat.run(steps[1])
    np.save(os.path.join(outdir, f"mid_{rank}.npy"), lat.read_state())
    conn.send("ran")
    conn.recv()
    lat.write_state(W[r0:r1])                              # the rank's own rows
    conn.send("written")
    conn.recv()
    lat.run(steps[2])
    np.save(os.path.join(outdir, f"end_{rank}.npy"), lat.read_state())
    conn.send(("done", int(lat.info("fluid_cells"))))
    conn.recv()          # keep the mappings until every rank has finished
    lat.close()


@pytest.mark.gpu
def test_rank_contexts_take_the_global_map_and_their_own_rows(gpu, tmp_path):
    """Two processes on one GPU (started as tests/test_gpu_parity.py::test_register_tiles_between_processes starts its ranks):
    the global B on both, each rank's rows back through write_state, a barrier of the test's own between an update and the
    run behind it; each rank's rows against the undivided lattice."""
    import multiprocessing as mp
    L = gpu
    nranks, shape, steps = 2, (256, 64), (5, 6, 7)
    A, B, S0, W = maps_and_states(shape[0], shape[1], 43, (32,))
    p = L.Param(shape[0], shape[1], 100, 10, 0.1, 0.01, 1.85)
    with L.Lattice(p, A, S0) as lat:
        lat.set_option("time_block", 1)
        lat.run(steps[0])
        lat.set_obstacles(B, REST)
        lat.run(steps[1])
        mid = lat.read_state()
        lat.write_state(W)
        lat.run(steps[2])
        end = lat.read_state()
    ctx = mp.get_context("spawn")
    pipes = [ctx.Pipe() for _ in range(nranks)]
    procs = [ctx.Process(target=_rank_worker, args=(r, nranks, shape, steps, pipes[r][1], str(tmp_path))) for r in range(nranks)]
    for pr in procs:
        pr.start()
    try:
        def gather(what):
            msgs = []
            for r in range(nranks):
                assert pipes[r][0].poll(120), f"rank {r}: no {what}"
                msgs.append(pipes[r][0].recv())
            return msgs

        def release(x):
            for r in range(nranks):
                pipes[r][0].send(x)

        release(gather("handle"))
        upd = gather("update")
        assert all(m[0] == "updated" for m in upd)
        bounds = [(r * shape[1] // nranks, (r + 1) * shape[1] // nranks) for r in range(nranks)]
        assert [m[1] for m in upd] == [int(refilled(A, B)[a:b].sum()) for a, b in bounds]
        release("go")
        assert gather("run") == ["ran"] * nranks
        release("go")
        assert gather("write") == ["written"] * nranks
        release("go")
        done = gather("end")
        assert all(m == ("done", int((B == 0).sum())) for m in done), done
        release("bye")
    finally:
        for pr in procs:
            pr.join(60)
            if pr.is_alive():
                pr.kill()
    assert all(pr.exitcode == 0 for pr in procs)
    for name, whole in (("mid", mid), ("end", end)):
        got = np.concatenate([np.load(tmp_path / f"{name}_{r}.npy") for r in range(nranks)], axis=0)
        assert _same(got, whole), name
