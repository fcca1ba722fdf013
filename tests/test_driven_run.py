"""lbm_set_accel and lbm_run_driven: the acceleration as an input of the run (Lattice.set_accel, Lattice.run_driven).

Contract (include/lbm_mi355x.h): step t of a driven call is the reference's step with params.accel = accel[t], its two
accelerate constants made on the host by lbm_run's expression.  The lattice is bit-identical to
`for a in accel: set_accel(a); run(1)` from the same state on every engine; av_vels are the engine's own per-step sums --
that loop's within float rounding of the per-step sum, and with a constant schedule equal to the context's acceleration
lbm_run's bits wherever the register tiles ran.  The register tiles read the schedule inside their kernel
(driven_in_kernel = 1); a lattice alone under lbm_wave takes it in its launches (driven_in_wave = 1, tests/test_wave_driven.py);
every other engine runs the one-step kernel with each step's own constants.

The reference of every GPU test is loop_reference: set_accel + run(1) on a fresh context under engine 1, time_block 1 -- the
one-step kernel, which tests/test_gpu_parity.py and tests/test_param_space.py pin to the oracle.  A reference runs once per
(case, schedule) over the longest run; a shorter run is compared with the state the loop held after that many steps (the
schedule of a shorter run is the prefix of the longer one's)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, deck_paths, load_kat
from test_sampled_run import TILINGS

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden import PARAM_GRID, param_state, refused  # noqa: E402

LBM_EINVAL = 1
SPLIT = (("engine", 1), ("time_block", 1))
INFO = ("engine_last", "driven_in_kernel", "driven_in_wave", "wave_launches")
AV_RTOL = 2e-6                     # "lbm_run's to rounding": the bar of tests/test_wave_window.py for the split paths


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def schedules(accel, n, seed, spikes=None):
    """The schedules of n steps around `accel`, float32, by name:
      a        constant accel;
      b        n distinct values drawn from [0.5, 1.5] accel: any index slip changes bits;
      c        accel cos(2 pi t / 11): both signs, zeros of slope;
      d<k>     a spike: zero except 4 accel at index k (k in `spikes`; default 0, n // 2, n - 1): an off-by-one reads plainly;
      e        a positive ramp with a ripple: accel (1 + 0.5 t / n) (1 + 0.25 sin(2 pi t / 7))."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    b = accel * (0.5 + rng.permutation(n) / max(n - 1, 1))
    out = {
        "a": np.full(n, accel, dtype=np.float32),
        "b": b.astype(np.float32),
        "c": (accel * np.cos(2 * np.pi * t / 11)).astype(np.float32),
        "e": (accel * (1 + 0.5 * t / n) * (1 + 0.25 * np.sin(2 * np.pi * t / 7))).astype(np.float32),
    }
    assert len(set(out["b"].tolist())) == n
    for k in sorted(set((0, n // 2, n - 1) if spikes is None else spikes)):
        if 0 <= k < n:
            d = np.zeros(n, dtype=np.float32)
            d[k] = 4 * accel
            out["d%d" % k] = d
    return out


def driven_oracle(oracle, prm, cells, ob, accel):
    """The definition on the CPU: Oracle.timestep looped with prm.accel = accel[t]; advances `cells` in place, returns
    av_vels (cells' dtype).  prm is left as it was."""
    keep = prm.accel
    a, b = cells, np.empty_like(cells)
    av = np.empty(len(accel), dtype=cells.dtype)
    try:
        for t, acc in enumerate(accel):
            prm.accel = float(acc)
            av[t] = oracle.timestep(prm, a, b, ob)
            a, b = b, a
    finally:
        prm.accel = keep
    if a is not cells:
        cells[...] = a
    return av


def loop_reference(L, p, ob, cells, accel, marks, options=SPLIT, **kw):
    """set_accel(accel[t]) + run(1) on a fresh context: (av_vels, {n: the lattice after n steps, n in marks})."""
    av, states = [], {}
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        for t, a in enumerate(accel):
            lat.set_accel(float(a))
            av.append(lat.run(1))
            assert lat.info("engine_last") == 1
            if t + 1 in marks:
                states[t + 1] = lat.read_state()
    return np.concatenate(av) if av else np.empty(0, np.float32), states


def driven(L, p, ob, cells, accel, options=(), **kw):
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        av = lat.run_driven(accel)
        info = {k: int(lat.info(k)) for k in INFO}
        assert np.float32(lat.info("accel")) == np.float32(p.accel)
        st = lat.read_state()
    return av, st, info


_REF = {}


def reference(L, key, p, ob, cells, accel, marks, options=SPLIT):
    k = (key, accel.tobytes(), tuple(sorted(marks)), options)
    if k not in _REF:
        av, states = loop_reference(L, p, ob, cells, accel, set(marks), options)
        av.setflags(write=False)
        for s in states.values():
            assert np.all(np.isfinite(s))
            s.setflags(write=False)
        _REF[k] = (av, states)
    return _REF[k]


def _random_case(L, nx, ny, seed, blocked=0.1):
    rng = np.random.default_rng(seed)
    p = L.Param(nx, ny, 100, 10, 0.1, 0.01, 1.85)
    ob = (rng.random((ny, nx)) < blocked).astype(np.int32)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float32)
    cells = (0.1 * w * (1.0 + 0.2 * (rng.random((ny, nx, 9), dtype=np.float32) - 0.5))).astype(np.float32)
    return p, ob, cells


def _deck(L, deck):
    pf, of = deck_paths(deck)
    p = L.read_params(pf)
    return p, np.ascontiguousarray(L.read_obstacles(of, p), dtype=np.int32).reshape(p.ny, p.nx)


def _tile_opts(ty, r, asy, *more):
    return (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3)) + more


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_driven_run_is_declared_and_bound(L):
    assert "lbm_set_accel" in L.ABI_SYMBOLS and "lbm_run_driven" in L.ABI_SYMBOLS
    hdr = open(L.HEADER_PATH).read()
    assert "int lbm_set_accel(lbm_ctx* ctx, float accel);" in hdr
    assert "int lbm_run_driven(lbm_ctx* ctx, int nsteps, float* av_vels, const float* accel);" in hdr
    lib = L.load_library()
    built = open(L.LIB_PATH, "rb").read()
    for key in (b"accel", b"driven_in_kernel", b"driven_in_wave"):
        assert '"%s"' % key.decode() in hdr, key
        assert key + b"\0" in built, key
        v = C.c_double(-1.0)
        assert lib.lbm_get_info(None, key, C.byref(v)) == LBM_EINVAL and v.value == -1.0
    assert lib.lbm_set_accel(None, 0.01) == LBM_EINVAL and b"ctx" in lib.lbm_last_error()
    assert lib.lbm_run_driven(None, 3, None, None) == LBM_EINVAL and b"ctx" in lib.lbm_last_error()
    assert "driven_in_kernel" in L.Lattice.run_driven.__doc__ and "driven_in_wave" in L.Lattice.run_driven.__doc__
    assert "info(\"accel\")" in L.Lattice.set_accel.__doc__


def test_run_driven_refuses_what_is_no_schedule_in_python(L):
    """Before the library is asked (no context needed: the checks come first)."""
    lat = L.Lattice.__new__(L.Lattice)                   # (never created: run_driven must refuse before it touches it)
    for bad in (np.zeros((3, 2), np.float32), np.float32(0.01), np.array([], dtype=object).reshape(0, 1),
                np.array(["0.01", "0.02"]), np.array([None, None], dtype=object), np.array([1 + 2j, 3])):
        with pytest.raises(L.LbmError):
            L.Lattice.run_driven(lat, bad)


def test_schedules_are_what_they_say():
    s = schedules(0.01, 23, 3)
    assert sorted(s) == ["a", "b", "c", "d0", "d11", "d22", "e"]
    assert all(v.dtype == np.float32 and v.shape == (23,) for v in s.values())
    assert np.all(s["a"] == np.float32(0.01))
    assert s["b"].min() >= 0.005 * (1 - 1e-6) and s["b"].max() <= 0.015 * (1 + 1e-6) and len(set(s["b"].tolist())) == 23
    assert (s["c"] > 0).any() and (s["c"] < 0).any()
    assert np.count_nonzero(s["d11"]) == 1 and s["d11"][11] == np.float32(0.04)
    assert s["e"][0] == np.float32(0.01) and np.all(s["e"] > 0)
    assert np.array_equal(schedules(0.01, 23, 3)["b"], s["b"])          # (a seed gives one schedule)
    assert sorted(schedules(0.01, 13, 1, spikes=(0, 3, 4, 5, 8, 12, 99))) == ["a", "b", "c", "d0", "d12", "d3", "d4", "d5", "d8", "e"]


@pytest.mark.parametrize("deck", ["128x128", "256x256"])
def test_driven_oracle_is_the_oracles_run_under_a_constant_schedule(O, oracle, deck):
    """The tests' own reference: driven_oracle under schedule (a) equals Oracle.run bit for bit, lattice and av_vels, in
    float and in double, over 50 steps from rest.
    Also measured here (printed), the deviation the bars of test_fifty_driven_steps_against_the_float_oracle must leave room
    for: max |av_float - av_double| / |av_double| over the 50 steps, under schedule (e) and under (a):
        128x128: (e) 7.1e-05, (a) 6.7e-05;   256x256: (e) 1.14e-04, (a) 1.0e-04
    -- the same order (asserted: (e) within twice (a)), so the bars of test_fifty_steps_against_float_oracle carry over."""
    pf, of = deck_paths(deck)
    op = O.read_params(pf)
    ob = O.read_obstacles(of, op.nx, op.ny)
    n = 50
    s = schedules(float(np.float32(op.accel)), n, 5)
    dev = {}
    for dtype in (np.float32, np.float64):
        ref = oracle.init_cells(op, dtype)
        av_ref = oracle.run(op, ref, ob, n)
        got = oracle.init_cells(op, dtype)
        accel = s["a"] if dtype == np.float32 else np.full(n, op.accel)
        av = driven_oracle(oracle, op, got, ob, accel)
        assert av.tobytes() == av_ref.tobytes() and got.tobytes() == ref.tobytes(), dtype
        for name in ("a", "e"):
            cells = oracle.init_cells(op, dtype)
            dev.setdefault(name, []).append(driven_oracle(oracle, op, cells, ob, s[name].astype(np.float64)).astype(np.float64))
    for name in ("a", "e"):
        f32, f64 = dev[name]
        dev[name] = float(np.max(np.abs(f32 - f64) / np.abs(f64)))
    print("%s: float against double av_vels, schedule (e) %.3g, schedule (a) %.3g" % (deck, dev["e"], dev["a"]))
    assert dev["e"] <= 2 * dev["a"]                      # (else: a milder schedule, not a wider bar)


# ---------------------------------------------------------------------------------------------------------------- GPU
NMAX = 23
NSTEPS = (1, 2, NMAX)


def _check_tiling(L, key, p, ob, cells, opts, names, extra=()):
    s = schedules(p.accel, NMAX, 17)
    for name in names:
        av_l, states = reference(L, key, p, ob, cells, s[name], NSTEPS, SPLIT + extra)
        for n in NSTEPS:
            av, st, info = driven(L, p, ob, cells, s[name][:n], opts + extra)
            where = (key, opts, name, n, info)
            assert info["driven_in_kernel"] == 1 and info["engine_last"] == 3 and info["driven_in_wave"] == 0, where
            assert av.shape == (n,) and np.array_equal(_bits(st), _bits(states[n])), where
            print(where, "av_vels: worst relative difference %.3g" % np.max(np.abs(av - av_l[:n]) / np.abs(av_l[:n])))
            assert np.allclose(av, av_l[:n], rtol=AV_RTOL, atol=0), where


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", TILINGS)
def test_driven_runs_of_every_register_tiling(gpu, ty, r, asy, nx, ny):
    L = gpu
    p, ob, cells = _random_case(L, nx, ny, 7)
    opts = _tile_opts(ty, r, asy)
    _check_tiling(L, (nx, ny, 7), p, ob, cells, opts, ("b", "c", "d0", "d11", "d22"))
    # schedule (a) is lbm_run on the same tiling: av_vels and the lattice, bit for bit
    s = schedules(p.accel, NMAX, 17)
    with L.Lattice(p, ob, cells) as lat:
        for k, v in opts:
            lat.set_option(k, v)
        av0, st0 = lat.run(NMAX), lat.read_state()
        assert lat.info("engine_last") == 3
    av, st, info = driven(L, p, ob, cells, s["a"], opts)
    assert info["driven_in_kernel"] == 1
    assert np.array_equal(_bits(av), _bits(av0)) and np.array_equal(_bits(st), _bits(st0))
    # a call cut in two gives the lattice of the whole
    _, whole, _ = driven(L, p, ob, cells, s["b"], opts)
    with L.Lattice(p, ob, cells) as lat:
        for k, v in opts:
            lat.set_option(k, v)
        lat.run_driven(s["b"][:9])
        lat.run_driven(s["b"][9:])
        assert lat.info("driven_in_kernel") == 1
        assert np.array_equal(_bits(lat.read_state()), _bits(whole))


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", [TILINGS[2], TILINGS[4]])
def test_driven_runs_with_ieee_maths(gpu, ty, r, asy, nx, ny):
    L = gpu
    assert r in (2, 4)
    p, ob, cells = _random_case(L, nx, ny, 8)
    _check_tiling(L, (nx, ny, 8), p, ob, cells, _tile_opts(ty, r, asy), ("b", "d11"), (("kernel_variant", 0),))


@pytest.mark.gpu
@pytest.mark.parametrize("options", [_tile_opts(8, 4, 1), SPLIT], ids=["register_tiles", "one_step_kernel"])
def test_set_accel(gpu, options):
    L = gpu
    p, ob, cells = _random_case(L, 256, 256, 9)
    x, n = 0.0173, 12
    px = L.Param(p.nx, p.ny, p.maxIters, p.reynolds_dim, p.density, x, p.omega)

    def ctx(prm):
        lat = L.Lattice(prm, ob, cells)
        for k, v in options:
            lat.set_option(k, v)
        return lat

    # set_accel(x); run(n) equals a fresh context created with accel = x
    with ctx(px) as fresh:
        av_x, st_x = fresh.run(n), fresh.read_state()
        eng = fresh.info("engine_last")
    with ctx(p) as lat:
        assert np.float32(lat.info("accel")) == np.float32(p.accel)
        lat.set_accel(x)
        assert np.float32(lat.info("accel")) == np.float32(x)
        av, st = lat.run(n), lat.read_state()
        assert lat.info("engine_last") == eng
    assert np.array_equal(_bits(av), _bits(av_x)) and np.array_equal(_bits(st), _bits(st_x))
    # run_driven leaves info("accel") and a following run untouched
    s = schedules(p.accel, n, 4)["b"]
    with ctx(p) as lat:
        lat.run_driven(s)
        assert np.float32(lat.info("accel")) == np.float32(p.accel)
        av2, st2 = lat.run(n), lat.read_state()
    with ctx(p) as twin:
        for a in s:
            twin.set_accel(float(a))
            twin.run(1)
        twin.set_accel(p.accel)
        av2_t, st2_t = twin.run(n), twin.read_state()
    assert np.array_equal(_bits(st2), _bits(st2_t)) and np.array_equal(_bits(av2), _bits(av2_t))
    # a set_accel between two run_forces calls gives the forces of two contexts created with those values
    body = (ob != 0).astype(np.int32)
    with ctx(p) as lat:
        lat.set_bodies(body, 1)
        av_1, f_1 = lat.run_forces(n)
        mid = lat.read_state()
        lat.set_accel(x)
        av_2, f_2 = lat.run_forces(n)
        end = lat.read_state()
    with ctx(p) as one:
        one.set_bodies(body, 1)
        want_av1, want_f1 = one.run_forces(n)
    with L.Lattice(px, ob, mid) as two:
        for k, v in options:
            two.set_option(k, v)
        two.set_bodies(body, 1)
        want_av2, want_f2 = two.run_forces(n)
        want_end = two.read_state()
    assert np.array_equal(_bits(f_1), _bits(want_f1)) and np.array_equal(_bits(av_1), _bits(want_av1))
    assert np.array_equal(_bits(f_2), _bits(want_f2)) and np.array_equal(_bits(av_2), _bits(want_av2))
    assert np.array_equal(_bits(end), _bits(want_end))


@pytest.mark.gpu
@pytest.mark.parametrize("nslabs,exchange", [(2, "copy"), (4, "copy"), (2, "p2p")])
def test_slabs_give_the_loops_lattice(gpu, nslabs, exchange):
    L = gpu
    p, ob = _deck(L, "256x256")
    s = schedules(p.accel, NMAX, 21)
    ex = L.EXCHANGE_COPY if exchange == "copy" else L.EXCHANGE_P2P
    for name in ("b", "d11"):
        av_l, states = reference(L, "256x256", p, ob, None, s[name], (NMAX,))
        av, st, info = driven(L, p, ob, None, s[name], nslabs=nslabs, devices=[0] * nslabs, exchange=ex)
        assert np.array_equal(_bits(st), _bits(states[NMAX])), (name, info)
        assert np.allclose(av, av_l, rtol=AV_RTOL, atol=0), (name, info)
        assert info["driven_in_kernel"] == (1 if info["engine_last"] == 3 else 0) and info["driven_in_wave"] == 0, info
        if exchange == "p2p":                # register tiles across slabs
            assert info["engine_last"] == 3, info


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["rccl", "p2p"])
def test_rank_context_ring_of_one_gives_the_single_slab_run(gpu, exchange):
    L = gpu
    p, ob = _deck(L, "128x256")
    s = schedules(p.accel, 13, 22)["b"]
    av_l, states = reference(L, "128x256", p, ob, None, s, (13,))
    av1, st1, info1 = driven(L, p, ob, None, s)
    assert info1["driven_in_kernel"] == 1 and np.array_equal(_bits(st1), _bits(states[13]))
    os.environ["LBM_FORCE_EXCHANGE"] = "1"
    try:
        ex = L.EXCHANGE_RCCL if exchange == "rccl" else L.EXCHANGE_P2P
        av, st, info = driven(L, p, ob, None, s, rank=0, nranks=1, device=0, unique_id=L.rccl_unique_id(), exchange=ex)
    finally:
        del os.environ["LBM_FORCE_EXCHANGE"]
    assert np.array_equal(_bits(st), _bits(st1)), info
    assert np.allclose(av, av1, rtol=AV_RTOL, atol=0), info
    assert info["driven_in_kernel"] == (1 if info["engine_last"] == 3 else 0) and info["driven_in_wave"] == 0, info


@pytest.mark.gpu
@pytest.mark.parametrize("time_block", [1, 2, 4, 8])
def test_streaming_engines_give_the_register_tiles_lattice(gpu, time_block):
    L = gpu
    p, ob = _deck(L, "256x256")
    s = schedules(p.accel, 21, 23)["b"]
    av_t, st_t, info_t = driven(L, p, ob, None, s)
    assert info_t["driven_in_kernel"] == 1 and info_t["engine_last"] == 3
    # (march_kernel 0 keeps lbm_wave away at time_block 4 and 8 here: its own flavour has its own test file)
    av, st, info = driven(L, p, ob, None, s, (("engine", 1), ("march_kernel", 0), ("time_block", time_block)))
    assert info == dict(engine_last=1, driven_in_kernel=0, driven_in_wave=0, wave_launches=0), info
    assert np.array_equal(_bits(st), _bits(st_t))
    assert np.allclose(av, av_t, rtol=AV_RTOL, atol=0)


@pytest.mark.gpu
def test_a_lattice_that_does_not_tile(gpu):
    L = gpu
    k = load_kat("kat_33x20")
    p = L.Param(int(k["nx"]), int(k["ny"]), 10, int(k["reynolds_dim"]), float(k["density"]), float(k["accel"]), float(k["omega"]))
    ob = np.ascontiguousarray(k["obstacles"], dtype=np.int32)
    cells = np.ascontiguousarray(k["cells0"], dtype=np.float32)
    s = schedules(p.accel, NMAX, 24)
    for name in ("b", "c", "d0", "d22"):
        av_l, states = reference(L, "kat_33x20", p, ob, cells, s[name], (NMAX,))
        av, st, info = driven(L, p, ob, cells, s[name])
        assert info["engine_last"] == 1 and info["driven_in_kernel"] == 0 and info["driven_in_wave"] == 0, info
        assert np.array_equal(_bits(st), _bits(states[NMAX])), name
        assert np.allclose(av, av_l, rtol=AV_RTOL, atol=0), name


# (register tiling 8 x 4 on 256 x 256; lbm_wave<8> with two columns per lane on 256 x 64, as tests/test_param_space.py's engines)
REFUSING = {
    "regtile_8x4": (256, 256, _tile_opts(8, 4, 1), dict(driven_in_kernel=1, driven_in_wave=0, engine_last=3)),
    "wave8_cols2": (256, 64, (("engine", 1), ("march_kernel", 1), ("time_block", 8), ("wave_cols", 2)),
                    dict(driven_in_kernel=0, driven_in_wave=1, engine_last=1)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("engine", sorted(REFUSING))
def test_where_the_accelerate_guard_refuses(gpu, O, oracle, engine):
    """The (density, accel, omega) point of tests/test_param_space.py at which the guard refuses cells of row ny - 2 during
    the run, from rest, with schedule (b) around its acceleration: the refusals happen at write time inside the kernels'
    passes (counted on the float oracle's driven run), and the lattice is the loop's, bit for bit."""
    L = gpu
    nx, ny, opts, want = REFUSING[engine]
    d, a, o = PARAM_GRID["refusal"]
    ob, cells = param_state("refusal", nx, ny, 51, "rest")
    p = L.Param(nx, ny, 100, 10, d, a, o)
    n = 21
    s = schedules(a, n, 25)["b"]
    op = O.OrcParam(nx, ny, 100, 10, float(np.float32(d)), float(np.float32(a)), float(np.float32(o)))
    x, counts = cells.copy(), []
    for t in range(n):
        counts.append(int(refused(op.density, float(s[t]), ob, x).sum()))
        driven_oracle(oracle, op, x, ob, s[t:t + 1])
    assert np.all(np.isfinite(x)) and sum(counts[1:]) > 0, counts
    av_l, states = reference(L, ("refusal", nx, ny), p, ob, cells, s, (n,))
    av, st, info = driven(L, p, ob, cells, s, opts)
    assert {k: info[k] for k in want} == want, info
    assert np.array_equal(_bits(st), _bits(states[n])), engine
    assert np.allclose(av, av_l, rtol=AV_RTOL, atol=0), engine


@pytest.mark.gpu
def test_refusals_leave_the_lattice_alone(gpu):
    L = gpu
    p, ob, cells = _random_case(L, 128, 16, 10)
    lib = L.load_library()
    good = np.full(5, 0.01, dtype=np.float32)
    with L.Lattice(p, ob, cells) as lat:
        lat.run(3)
        st0 = lat.read_state()

        def untouched(what):
            assert np.array_equal(_bits(lat.read_state()), _bits(st0)), what
            assert np.float32(lat.info("accel")) == np.float32(p.accel), what

        assert lib.lbm_run_driven(lat._ctx, 5, None, None) == LBM_EINVAL and b"accel" in lib.lbm_last_error()
        untouched("NULL schedule")
        assert lib.lbm_run_driven(lat._ctx, -1, None, good.ctypes.data) == LBM_EINVAL and b"nsteps" in lib.lbm_last_error()
        untouched("nsteps < 0")
        for bad in (np.nan, np.inf, -np.inf):
            s = good.copy()
            s[3] = bad
            with pytest.raises(L.LbmError, match=r"accel\[3\]"):
                lat.run_driven(s)
            untouched(bad)
            with pytest.raises(L.LbmError, match="finite"):
                lat.set_accel(bad)
            untouched(("set_accel", bad))
        assert lat.run_driven(np.empty(0, np.float32)).shape == (0,)          # nsteps = 0: success, nothing runs
        untouched("nsteps = 0")
        assert lat.run_driven([0.01, 0.02]).shape == (2,)                     # (a list of Python floats is a schedule)


@pytest.mark.gpu
@pytest.mark.parametrize("deck", ["128x128", "256x256"])
def test_fifty_driven_steps_against_the_float_oracle(gpu, O, oracle, deck):
    """50 steps from rest under schedule (e), which starts at the deck's own acceleration, against driven_oracle in float, with
    the bars of test_gpu_parity.test_fifty_steps_against_float_oracle: lattice 5e-5 of the largest population, av_vels
    rtol 1e-4, pressure 1e-5, velocities 2e-4 of the largest speed.  The default engine and, on the 128-wide deck,
    lbm_wave<4> (time_block 4).  The float oracle's own deviation from the double oracle under (e) is of the order of the constant
    schedule (test_driven_oracle_is_the_oracles_run_under_a_constant_schedule: 7.1e-05 against 6.7e-05 on 128x128,
    1.14e-04 against 1.0e-04 on 256x256)."""
    L = gpu
    pf, of = deck_paths(deck)
    p = L.read_params(pf)
    ob = L.read_obstacles(of, p)
    op = O.read_params(pf)
    s = schedules(float(np.float32(p.accel)), 50, 5)["e"]
    cells = oracle.init_cells(op, np.float32)
    av_o = driven_oracle(oracle, op, cells, ob, s)
    fo = oracle.final_state(op, cells, ob)
    combos = [((), dict(engine_last=3, driven_in_kernel=1, driven_in_wave=0))]
    if p.nx == 128:
        combos.append(((("engine", 1), ("time_block", 4)), dict(engine_last=1, driven_in_kernel=0, driven_in_wave=1)))
    for opts, want in combos:
        with L.Lattice(p, ob) as lat:
            for k, v in opts:
                lat.set_option(k, v)
            av = lat.run_driven(s)
            info = {k: int(lat.info(k)) for k in want}
            st = lat.read_state()
            fs = lat.final_state()
        assert info == want, (opts, info)
        print(deck, opts, "lattice %.3g of the largest population, av_vels %.3g relative" %
              (np.abs(st - cells).max() / np.abs(cells).max(), np.max(np.abs(av - av_o) / np.abs(av_o))))
        assert np.abs(st - cells).max() <= 5e-5 * np.abs(cells).max(), opts
        assert np.allclose(av, av_o, rtol=1e-4, atol=0), opts
        assert np.allclose(fs[..., 3], fo[..., 3], rtol=1e-5, atol=0)           # pressure
        assert np.allclose(fs[..., :3], fo[..., :3], rtol=0, atol=2e-4 * np.abs(fo[..., 2]).max())
