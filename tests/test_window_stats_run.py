"""lbm_run_window_stats: the means and second moments of a window's cells (Lattice.run_window_stats).

Contract (include/lbm_mi355x.h): with W_j the samples of lbm_run_window at the same `every` from the same state, a window
cell's eight floats are what lbm_run_stats defines from X_j = W_j[r][c] -- tests/test_stats_run.py's stats_of of
tests/test_window_run.py's cut of the snapshots, bit for bit -- and so lbm_run_stats' output in the window's cells.  The
register tiles take the samples inside their kernels, `window_stats_chunk` sample steps a launch, staged and folded into
the sums by lbm_window_stats_fold (window_stats_in_kernel = 1; av_vels and the lattice are lbm_run's bits wherever the call
is cut); every other engine here runs the steps in pieces of `every` with lbm_window_stats_add behind each (lbm_wave:
tests/test_wave_window_stats.py).  Every comparison is on bit patterns unless it says otherwise.

The expected value is always stats_of(cut(snaps, w), p0), snaps the snapshots of the split path (engine 1, time_block 1,
run_sampled at every = 1) computed once per case and sliced.

Everything here runs at density 0.1, omega 1.85 and the decks' acceleration, and all but test_one_context_through_mixed_calls on
a fresh context per call.  Away from that point -- the other densities, density 0.3 where density * (1.f / 3.f) is not
density / 3.f, the refusing accelerate row, chunk cuts on every path -- tests/test_window_stats_param_space.py (100 GPU cases;
second moments at most 0.053 and variances 0.034 of the double oracle's bounds; nothing found); on one long-lived context --
the window table shared with lbm_run_window, re-tilings, the chunk option, the pieces across TAG_WRAP and SLAB_TAG_MARK, live
maps and written lattices in front -- the window_stats entries of tests/test_observer_sequences.py and
tests/test_live_sequences.py."""
import ctypes as C

import numpy as np
import pytest

from test_sampled_run import TILINGS
from test_mean_run import _deck, _random_case, _kat_case, _plain, _child
from test_probe_run import _bits, _tiling, awkward_set, _pick
from test_stats_run import p0_of, stats_of, _oracle_moment_bound
from test_window_run import cut, awkward_windows, _same, _slab_windows, _refusals, _oracle_window

LBM_EINVAL = 1
SPLIT = (("engine", 1), ("time_block", 1))
INFO = ("engine_last", "window_stats_in_kernel", "window_stats_in_wave", "window_stats_pieces")
DECL = "int lbm_run_window_stats(lbm_ctx* ctx, int nsteps, float* av_vels, int every, const lbm_window* win, float* stats_out);"


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_window_stats_run_is_declared_and_bound(L):
    assert "lbm_run_window_stats" in L.ABI_SYMBOLS
    hdr = open(L.HEADER_PATH).read()
    assert DECL in hdr
    lib = L.load_library()
    assert lib.lbm_run_window_stats is not None
    built = open(L.LIB_PATH, "rb").read()
    for key in (b"window_stats_in_wave", b"window_stats_in_kernel", b"window_stats_pieces", b"window_stats_chunk"):
        assert b'"' + key + b'"' in hdr.encode(), key
        assert key + b"\0" in built, key
        v = C.c_double(-1.0)
        assert lib.lbm_get_info(None, key, C.byref(v)) == LBM_EINVAL and v.value == -1.0
    assert callable(L.Lattice.run_window_stats)
    for key in ("window_stats_in_wave", "window_stats_in_kernel", "window_stats_pieces", "window_stats_chunk"):
        assert key in L.Lattice.run_window_stats.__doc__, key


def test_the_header_states_the_definition_and_what_is_not_offered(L):
    hdr = open(L.HEADER_PATH).read()
    doc = hdr[hdr.index("lbm_run_stats over a window"):hdr.index("int lbm_run_window_stats(")]
    doc = " ".join(doc.replace("\n *", " ").split())
    for phrase in ("Definition, bit for bit", "lbm_run_window(ctx, nsteps, av_vels, every, win, ...)", "S_j = S_(j-1) + X_j",
                   "T_j = T_(j-1) + Q_j", "p0 = density * (1.f / 3.f)", "one rounding per operation", "no fma", "in step order",
                   "(float)m", "stats_out[win->y0 + r win->sy][win->x0 + c win->sx][:]", "32 bytes per window cell",
                   "wherever the call is cut", "Not offered", "lbm_run_observed", "under a schedule", "windows that wrap",
                   "block averaging", "command-line tool"):
        assert phrase in doc, phrase


def test_null_arguments_are_refused(L):
    lib = L.load_library()
    w = L.Window(0, 0, 1, 1)
    out = np.full(8, np.nan, np.float32)
    for args, word in (((None, 10, None, 5, C.byref(w), out.ctypes.data), b"ctx"),
                       ((None, 10, None, 5, None, out.ctypes.data), b"win"),
                       ((None, 10, None, 5, C.byref(w), None), b"stats_out")):
        assert lib.lbm_run_window_stats(*args) == LBM_EINVAL, word
        assert word in lib.lbm_last_error(), (word, lib.lbm_last_error())
    assert np.isnan(out).all()


def test_stats_of_a_cut_on_a_series_worked_out_by_hand(L):
    """density 0.75: p0 = 0.25 exactly (tests/test_stats_run.py works it out).  Two snapshots of a 2 x 3 lattice, the window
    the cells (0, 1) and (2, 1) -- row 1, columns 0 and 2 (sx = 2) -- every value a small dyadic fraction (nothing rounds):
      cell (0, 1)   X_1 = (0.5, -0.25, 0.5, 0.5)    d = 0.25    Q_1 = (0.25,   0.0625, -0.125,   0.0625)
                    X_2 = (0.25, 0.25, 0.25, 0.375) d = 0.125   Q_2 = (0.0625, 0.0625,  0.0625,  0.015625)
                    S_2 = (0.75, 0, 0.75, 0.875)    T_2 = (0.3125, 0.125, -0.0625, 0.078125)
                    out = (0.375, 0, 0.375, 0.4375, 0.15625, 0.0625, -0.03125, 0.0390625)
      cell (2, 1)   blocked: X_1 = X_2 = (0, 0, 0, 0.25), d = 0: out = (0, 0, 0, 0.25, 0, 0, 0, 0)
    Every other cell holds NaN: the cut must not touch it."""
    p0 = p0_of(0.75)
    assert p0 == np.float32(0.25)
    snaps = np.full((2, 2, 3, 4), np.nan, np.float32)
    snaps[0, 1, 0] = (0.5, -0.25, 0.5, 0.5)
    snaps[1, 1, 0] = (0.25, 0.25, 0.25, 0.375)
    snaps[:, 1, 2] = (0, 0, 0, 0.25)
    w = L.Window(0, 1, 2, 1, 2, 1)
    got = stats_of(cut(snaps, w), p0)
    want = np.array([[[0.375, 0, 0.375, 0.4375, 0.15625, 0.0625, -0.03125, 0.0390625], [0, 0, 0, 0.25, 0, 0, 0, 0]]], np.float32)
    assert got.shape == (1, 2, 8) and np.array_equal(_bits(got), _bits(want))


# ---------------------------------------------------------------------------------------------------------------- GPU
_REF = {}


def _snaps(L, key, p, ob, cells, nsteps):
    """Once per case: the snapshots of the split path at every step of nsteps steps, read-only."""
    if key not in _REF:
        with L.Lattice(p, ob, cells) as lat:
            for k, v in SPLIT:
                lat.set_option(k, v)
            _, S1 = lat.run_sampled(nsteps, 1)
            assert lat.info("samples_in_kernel") == 0 and lat.info("samples_in_wave") == 0 and lat.info("engine_last") == 1
        assert S1.shape == (nsteps, p.ny, p.nx, 4) and not np.isnan(S1).any()
        S1.setflags(write=False)
        _REF[key] = S1
    S1 = _REF[key]
    assert len(S1) >= nsteps
    return S1


def _want(S1, w, p0, nsteps, every):
    return stats_of(cut(S1[every - 1:nsteps:every][:nsteps // every], w), p0)


def _wstats(L, p, ob, cells, nsteps, every, windows, options=(), **kw):
    """One fresh context per window, the options, one run_window_stats: [(av_vels, stats, lattice, info)]."""
    res = []
    for w in windows:
        with L.Lattice(p, ob, cells, **kw) as lat:
            for k, v in options:
                lat.set_option(k, v)
            av, out = lat.run_window_stats(nsteps, every, w)
            res.append((av, out, lat.read_state(), {k: int(lat.info(k)) for k in INFO}))
    return res


def _full_stats(L, p, ob, cells, nsteps, every, options=(), **kw):
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        return lat.run_stats(nsteps, every)[1]


def _cut8(stats, w):
    return cut(stats[None], w)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", TILINGS)
def test_window_stats_of_every_register_tiling(gpu, ty, r, asy, nx, ny):
    L = gpu
    p, ob, cells = _random_case(L, nx, ny, 7)
    p0 = p0_of(p.density)
    nsteps = 13
    opts = (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3))
    S1 = _snaps(L, (nx, ny, 7), p, ob, cells, nsteps)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts)
    ws = awkward_windows(L, nx, ny, ty, r)
    for every in (1, 2, 5):
        full = _full_stats(L, p, ob, cells, nsteps, every, opts)
        for w, (av, out, st, info) in zip(ws, _wstats(L, p, ob, cells, nsteps, every, ws, opts)):
            where = (w, every, info)
            assert info["engine_last"] == 3 and info["window_stats_in_kernel"] == 1 and info["window_stats_in_wave"] == 0, where
            _same(out, _want(S1, w, p0, nsteps, every), where)
            _same(out, _cut8(full, w), where)
            assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(av), _bits(av0)), where


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", [TILINGS[5], TILINGS[0]])
def test_chunk_cuts_change_nothing(gpu, ty, r, asy, nx, ny):
    """Eight waves a tile (16 rows, 2 a wave) and one row a wave; 13 steps at every = 2 are six samples and a tail of one
    step: one piece of six samples (automatic), six of one, three of two, one of four and one of two -- and the tail."""
    L = gpu
    assert (ty // r >= 8 and r > 1) or r == 1
    p, ob, cells = _random_case(L, nx, ny, 7)
    p0 = p0_of(p.density)
    nsteps, every = 13, 2
    opts = (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3))
    S1 = _snaps(L, (nx, ny, 7), p, ob, cells, nsteps)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts)
    all_ws = awkward_windows(L, nx, ny, ty, r)
    ws = [all_ws[0], all_ws[4], all_ws[5]]
    for chunk, pieces in ((0, 2), (1, 7), (2, 4), (4, 3)):
        for w, (av, out, st, info) in zip(ws, _wstats(L, p, ob, cells, nsteps, every, ws, opts + (("window_stats_chunk", chunk),))):
            where = (w, chunk, info)
            assert info["engine_last"] == 3 and info["window_stats_in_kernel"] == 1, where
            assert info["window_stats_pieces"] == pieces, where
            _same(out, _want(S1, w, p0, nsteps, every), where)
            assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(av), _bits(av0)), where


@pytest.mark.gpu
@pytest.mark.parametrize("nslabs,exchange", [(2, "copy"), (4, "copy"), (2, "p2p")])
def test_slabs_give_the_single_slab_result(gpu, nslabs, exchange):
    L = gpu
    p, ob = _deck(L, "256x256")
    p0 = p0_of(p.density)
    nsteps, every = 10, 4
    with L.Lattice(p, ob) as lat:
        ty, r = _tiling(lat)
    ws = _slab_windows(L, p, ty, r, nslabs)
    S1 = _snaps(L, "256x256", p, ob, None, 21)
    av1, st1 = _plain(L, p, ob, None, nsteps)
    ones = _wstats(L, p, ob, None, nsteps, every, ws)
    ex = L.EXCHANGE_COPY if exchange == "copy" else L.EXCHANGE_P2P
    many = _wstats(L, p, ob, None, nsteps, every, ws, nslabs=nslabs, devices=[0] * nslabs, exchange=ex)
    for w, (_, want, _, info1), (av, out, st, info) in zip(ws, ones, many):
        assert info1["window_stats_in_kernel"] == 1 and info1["engine_last"] == 3, (w, info1)
        _same(want, _want(S1, w, p0, nsteps, every), (w, info1))
        _same(out, want, (w, info))
        assert np.array_equal(_bits(st), _bits(st1)), w
        assert np.allclose(av, av1, rtol=2e-6, atol=0), w
        assert info["window_stats_in_wave"] == 0, (w, info)
        assert info["window_stats_in_kernel"] == (1 if info["engine_last"] == 3 else 0), (w, info)
        if exchange == "p2p":                # register tiles across slabs
            assert info["engine_last"] == 3 and info["window_stats_in_kernel"] == 1, (w, info)
            assert np.array_equal(_bits(av), _bits(av1)), w


# a rank context as a ring of one, in a child process of its own (the environment variable and the communicator stay there)
_RING_OF_ONE = r"""
import os, sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_window_stats_run import _bits, _deck, _plain, _same, _tiling, _wstats, awkward_windows
p, ob = _deck(L, "128x256")
nsteps, every = 13, 5
with L.Lattice(p, ob) as lat:
    ty, r = _tiling(lat)
ws = awkward_windows(L, p.nx, p.ny, ty, r)
ws = [ws[0], ws[5]]                # the whole lattice; strided (a communicator each, and the first takes seconds)
av1, st1 = _plain(L, p, ob, None, nsteps)
ones = _wstats(L, p, ob, None, nsteps, every, ws)
os.environ["LBM_FORCE_EXCHANGE"] = "1"
name = {name!r}
ex = L.EXCHANGE_RCCL if name == "rccl" else L.EXCHANGE_P2P
for w, (_, want, _, info1) in zip(ws, ones):
    assert info1["window_stats_in_kernel"] == 1, (w, info1)
    (av, out, st, info), = _wstats(L, p, ob, None, nsteps, every, [w], rank=0, nranks=1, device=0,
                                   unique_id=L.rccl_unique_id(), exchange=ex)          # (a fresh id per communicator)
    _same(out, want, (name, w, info))
    assert np.array_equal(_bits(st), _bits(st1)), (name, w)
    assert np.allclose(av, av1, rtol=2e-6, atol=0), (name, w)
print("ring of one ok")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["rccl", "p2p"])
def test_rank_context_ring_of_one_gives_the_single_slab_result(gpu, exchange):
    assert "ring of one ok" in _child(_RING_OF_ONE.replace("{name!r}", repr(exchange)))


@pytest.mark.gpu
@pytest.mark.parametrize("time_block", [1, 2, 4, 8])
def test_streaming_engines_give_the_register_tiles_result(gpu, time_block):
    L = gpu
    p, ob = _deck(L, "256x256")
    p0 = p0_of(p.density)
    nsteps, every = 21, 3
    with L.Lattice(p, ob) as lat:
        ty, r = _tiling(lat)
    ws = awkward_windows(L, p.nx, p.ny, ty, r)
    S1 = _snaps(L, "256x256", p, ob, None, 21)
    tiles = _wstats(L, p, ob, None, nsteps, every, ws)
    # (march_kernel 0 keeps lbm_wave away at time_block 4 and 8 here: its own flavour has its own test file)
    opts = (("engine", 1), ("march_kernel", 0), ("time_block", time_block))
    av0, st0 = _plain(L, p, ob, None, nsteps, opts)
    for w, (_, want, st_t, info_t), (av, out, st, info) in zip(ws, tiles, _wstats(L, p, ob, None, nsteps, every, ws, opts)):
        assert info_t["window_stats_in_kernel"] == 1 and info_t["engine_last"] == 3, (w, info_t)
        assert info == dict(engine_last=1, window_stats_in_kernel=0, window_stats_in_wave=0, window_stats_pieces=nsteps // every), (w, info)
        _same(want, _want(S1, w, p0, nsteps, every), (w, "tiles"))
        _same(out, want, (w, time_block))
        assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(st), _bits(st_t)), w
        assert np.allclose(av, av0, rtol=2e-6, atol=0), w


@pytest.mark.gpu
def test_a_lattice_that_does_not_tile(gpu):
    L = gpu
    nx, ny = 200, 72
    p, ob, cells = _random_case(L, nx, ny, 12)
    p0 = p0_of(p.density)
    nsteps, every = 11, 3
    opts = (("time_block", 1),)
    S1 = _snaps(L, (nx, ny, 12), p, ob, cells, nsteps)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts)
    ws = [L.Window(0, 0, nx, ny), L.Window(199, 71, 1, 1), L.Window(0, ny - 2, nx, 1), L.Window(1, 2, 67, 14, 3, 5),
          L.Window(150, 0, 50, 72)]
    for w, (av, out, st, info) in zip(ws, _wstats(L, p, ob, cells, nsteps, every, ws, opts)):
        assert info == dict(engine_last=1, window_stats_in_kernel=0, window_stats_in_wave=0, window_stats_pieces=4), (w, info)
        _same(out, _want(S1, w, p0, nsteps, every), w)
        assert np.array_equal(_bits(st), _bits(st0)), w
        assert np.allclose(av, av0, rtol=2e-6, atol=0), w


# torch and the library share libamdhip64: torch is imported FIRST, in a child process of its own
_DEVICE_OUTPUT = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_window_stats_run import _bits, _deck
p, ob = _deck(L, "128x256")
nsteps, every = 12, 5
for w in (L.Window(0, 0, p.nx, p.ny), L.Window(61, 15, 7, 5), L.Window(0, 0, 43, 52, 3, 5)):
    for engine, key in ((0, 1), (1, 0)):                # the register tiles; the streaming engines' pieces
        with L.Lattice(p, ob) as lat:
            lat.set_option("engine", engine)
            av_h, want = lat.run_window_stats(nsteps, every, w)
            assert lat.info("window_stats_in_kernel") == key
            st_h = lat.read_state()
        out = torch.full((w.ny, w.nx, 8), float("nan"), dtype=torch.float32, device="cuda:0")
        with L.Lattice(p, ob) as lat:
            lat.set_option("engine", engine)
            av, got = lat.run_window_stats(nsteps, every, w, out=out)
            assert got is out and lat.info("window_stats_in_kernel") == key and lat.info("window_stats_in_wave") == 0
            st = lat.read_state()
        torch.cuda.synchronize()
        assert not np.isnan(want).any()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (w, engine)
        assert np.array_equal(_bits(st), _bits(st_h)) and np.array_equal(_bits(av), _bits(av_h)), (w, engine)
print("device output ok")
"""


@pytest.mark.gpu
def test_device_output_is_the_host_output(gpu):
    assert "device output ok" in _child(_DEVICE_OUTPUT)


@pytest.mark.gpu
def test_the_probe_set_survives_a_window_stats_run(gpu):
    L = gpu
    p, ob = _deck(L, "128x256")
    p0 = p0_of(p.density)
    w = L.Window(0, 0, (p.nx + 2) // 3, (p.ny + 4) // 5, 3, 5)
    with L.Lattice(p, ob) as lat:
        ty, r = _tiling(lat)
        xy = awkward_set(p.nx, p.ny, ob, ty, r)
        lat.set_probes(xy)
        _, pr1 = lat.run_probes(8, 3)
        assert lat.info("probes_in_kernel") == 1
        _, ws = lat.run_window_stats(8, 3, w)
        assert lat.info("window_stats_in_kernel") == 1 and lat.info("engine_last") == 3
        assert lat.info("probes_in_kernel") == 1                   # (the probes' key belongs to the probes' calls)
        _, pr3 = lat.run_probes(8, 3)                              # the set and its table, untouched by the window-stats run
        assert lat.info("probes_in_kernel") == 1 and lat.info("engine_last") == 3
    with L.Lattice(p, ob) as ref:
        f1, f2, f3 = (ref.run_sampled(8, 3)[1] for _ in range(3))
    assert np.array_equal(_bits(pr1), _bits(_pick(f1, xy)))
    _same(ws, stats_of(cut(f2, w), p0), "window stats behind a probe run")
    assert np.array_equal(_bits(pr3), _bits(_pick(f3, xy)))


@pytest.mark.gpu
def test_one_context_through_mixed_calls(gpu):
    """run_window_stats, run, run_stats, run_window and run_window_stats again on one register-tile context: after each call
    the lattice and av_vels are those of a twin that only calls run; the keys are reset by each call."""
    L = gpu
    p, ob = _deck(L, "128x256")
    p0 = p0_of(p.density)
    w = L.Window(61, 15, 20, 9, 3, 2)
    with L.Lattice(p, ob) as lat, L.Lattice(p, ob) as twin, L.Lattice(p, ob) as ref:

        def same(av):
            assert np.array_equal(_bits(av), _bits(twin.run(len(av))))
            assert np.array_equal(_bits(lat.read_state()), _bits(twin.read_state()))

        def keys():
            return tuple(int(lat.info(k)) for k in ("window_stats_in_kernel", "window_stats_in_wave", "window_stats_pieces"))

        lat.set_option("window_stats_chunk", 2)
        av, s1 = lat.run_window_stats(11, 2, w)                    # samples 2, 4 | 6, 8 | 10 | the tail
        assert keys() == (1, 0, 4)
        same(av)
        _same(s1, stats_of(cut(ref.run_sampled(11, 2)[1], w), p0), "first")
        same(lat.run(5))
        ref.run(5)
        av, full = lat.run_stats(6, 3)
        same(av)
        _same(full, stats_of(ref.run_sampled(6, 3)[1], p0), "run_stats")
        assert keys() == (1, 0, 4)                                 # (another call's: not touched)
        av, win = lat.run_window(7, 3, w)
        assert lat.info("window_in_kernel") == 1
        same(av)
        _same(win, cut(ref.run_sampled(7, 3)[1], w), "run_window")
        lat.set_option("engine", 1)
        twin.set_option("engine", 1)
        av, s2 = lat.run_window_stats(9, 4, w)                     # off the tiles: two pieces of four steps and the tail
        assert keys() == (0, 0, 3) and lat.info("engine_last") == 1
        assert np.allclose(av, twin.run(9), rtol=2e-6, atol=0)
        assert np.array_equal(_bits(lat.read_state()), _bits(twin.read_state()))
        _same(s2, stats_of(cut(ref.run_sampled(9, 4)[1], w), p0), "second")
        lat.set_option("engine", 0)
        twin.set_option("engine", 0)
        lat.set_option("window_stats_chunk", 0)
        av, s3 = lat.run_window_stats(8, 4, w)
        assert keys() == (1, 0, 1)
        same(av)
        _same(s3, stats_of(cut(ref.run_sampled(8, 4)[1], w), p0), "third")


@pytest.mark.gpu
def test_refusals_leave_the_lattice_alone(gpu):
    L = gpu
    lib = L.load_library()
    p, ob = _deck(L, "128x128")
    ok = L.Window(3, 5, 20, 10, 2, 3)
    out = np.full((10, 20, 8), np.nan, np.float32)

    def refused(rc, *words):
        assert rc == LBM_EINVAL
        msg = lib.lbm_last_error().decode()
        for wd in words:
            assert wd in msg, (wd, msg)

    with L.Lattice(p, ob) as lat:
        lat.run(3)
        run = lambda *a: lib.lbm_run_window_stats(lat._ctx, *a)
        refused(run(10, None, 1, None, out.ctypes.data), "win")
        refused(run(10, None, 1, C.byref(ok), None), "stats_out")
        for w in _refusals(L, p.nx, p.ny):
            refused(run(10, None, 1, C.byref(w), out.ctypes.data), "window")
        refused(run(-1, None, 1, C.byref(ok), out.ctypes.data), "nsteps")
        refused(run(10, None, 0, C.byref(ok), out.ctypes.data), "every")
        refused(run(10, None, -1, C.byref(ok), out.ctypes.data), "every")
        refused(run(10, None, 11, C.byref(ok), out.ctypes.data), "no sample step")       # m = 0
        refused(run(0, None, 1, C.byref(ok), out.ctypes.data), "no sample step")
        with pytest.raises(L.LbmError):
            lat.run_window_stats(10, 1, L.Window(0, 0, p.nx + 1, 1))
        with pytest.raises(L.LbmError):
            lat.set_option("window_stats_chunk", -1)
        assert lat.info("window_stats_chunk") == 0
        assert np.isnan(out).all()
        assert lat.info("window_stats_in_kernel") == 0 and lat.info("window_stats_pieces") == 0
        av = lat.run(10)
        st1 = lat.read_state()
    with L.Lattice(p, ob) as ref:
        av_ref = ref.run(13)
        assert np.array_equal(_bits(st1), _bits(ref.read_state()))
        assert np.array_equal(_bits(av), _bits(av_ref[3:]))


_OTHER_DEVICE = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import ctypes as C
import numpy as np
import advanced_hpc_lbm_amd as L
from test_window_stats_run import _bits, _deck
p, ob = _deck(L, "128x128")
w = L.Window(3, 5, 20, 10, 2, 3)
out = torch.full((10, 20, 8), float("nan"), dtype=torch.float32, device="cuda:1")
torch.cuda.synchronize(1)
with L.Lattice(p, ob) as lat:
    st = lat.read_state()
    rc = L.load_library().lbm_run_window_stats(lat._ctx, 10, None, 1, C.byref(w), out.data_ptr())
    assert rc == 1 and b"device" in L.load_library().lbm_last_error()
    assert np.array_equal(_bits(lat.read_state()), _bits(st))
assert bool(torch.isnan(out).all())
print("other device ok")
"""


@pytest.mark.gpu
def test_a_device_pointer_on_another_device_is_refused(gpu):
    """As tests/test_driven_observed.py's test of the same name, which needs two devices too."""
    if gpu.device_count() < 2:
        pytest.skip("needs two HIP devices")
    assert "other device ok" in _child(_OTHER_DEVICE)


@pytest.mark.gpu
def test_second_moments_against_the_float_oracle(gpu, O, oracle):
    """64 x 40 known-answer lattice, 10 steps, every step a sample, the window rows 0, 19, 38 x all 64 columns: floats 4..7
    against the float64 fold of the strict float oracle's per-step fields in the window's cells, inside
    tests/test_stats_run.py's _oracle_moment_bound -- its bound, cut to the window; no tolerance of this file's own."""
    L = gpu
    k, p, ob, op = _kat_case(L, O)
    w = _oracle_window(L)
    want, bound, ref = _oracle_moment_bound(k, p, ob, op, oracle)
    assert np.array_equal(ref, k["cells_after_10"])
    (_, stats, st, info), = _wstats(L, p, ob, k["cells0"], 10, 1, [w])
    assert info["window_stats_in_kernel"] == 1 and stats.shape == (3, 64, 8), info
    assert np.all(np.abs(st - ref) <= 2e-5 * np.abs(ref))
    got = stats[..., 4:].astype(np.float64)
    err = np.abs(got - _cut8(want, w))
    lim = _cut8(bound, w) + 2.0 ** -24 * np.abs(got)
    print("second moments in the window against the oracle: max error %.3g, worst error - bound %.3g" % (err.max(), np.max(err - lim)))
    assert np.all(err <= lim), float(np.max(err - lim))
