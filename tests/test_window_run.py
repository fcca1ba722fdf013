"""lbm_run_window: snapshots of a window -- a sub-rectangle of the lattice, optionally strided -- stored from inside the
kernels (Lattice.run_window, window_rows).

Contract (include/lbm_mi355x.h): window_out[j][r][c][:] equals fields_out[j][y0 + r sy][x0 + c sx][:] of lbm_run_sampled at
the same `every` from the same state, bit for bit; a window run leaves av_vels and the lattice as lbm_run_sampled does.  The
register-tile engines take the window inside their kernels, in the probe flavour fed window tables (window_in_kernel = 1,
the probe set untouched); every other engine here runs the steps in pieces with lbm_derive_window behind each (lbm_wave:
tests/test_wave_window.py).  Every comparison is on bit patterns unless it says otherwise."""
import ctypes as C
import os

import numpy as np
import pytest

from test_sampled_run import TILINGS
from test_mean_run import _deck, _random_case, _oracle_fields, _kat_case, _plain, _sampled, _child
from test_probe_run import _bits, _tiling, awkward_set, _pick

LBM_EINVAL, LBM_ENOMEM = 1, 5
INT_MAX = 2 ** 31 - 1
INFO = ("engine_last", "window_in_kernel", "window_in_wave")


def cut(fields, w):
    """The window's cells of run_sampled's fields (m, ny, nx, 4): the definition."""
    return fields[:, w.y0:w.y0 + (w.ny - 1) * w.sy + 1:w.sy, w.x0:w.x0 + (w.nx - 1) * w.sx + 1:w.sx, :]


def awkward_windows(L, nx, ny, ty, r):
    """The windows used throughout, for an nx x ny lattice in 64-column tiles of ty rows, r rows per wave: the whole lattice;
    a single cell; the accelerate row and column 63 (the lanes that carry mail); 7 x 5 cells from (61, ty - 1), across a tile
    border in x and in y where the lattice has room; the whole extent at strides (3, 5), a column pattern that differs from
    tile to tile; strides (64, ty) from (63, ty - 1), only mail lanes in the last rows of tiles; on lattices from 256 x 256
    a 40-column window inside one tile, so that tiles (and waves) without a window cell exist."""
    W = L.Window
    ws = [W(0, 0, nx, ny), W(nx // 2 + 3, ny // 2 + 1, 1, 1), W(0, ny - 2, nx, 1), W(63, 0, 1, ny),
          W(61, ty - 1, min(7, nx - 61), min(5, ny - (ty - 1))),
          W(0, 0, (nx + 2) // 3, (ny + 4) // 5, 3, 5),
          W(63, ty - 1, (nx - 64) // 64 + 1, (ny - ty) // ty + 1, 64, ty)]
    if nx >= 256 and ny >= 256:
        rows = min(40, ty)
        inside = W(64 + 12, 2 * ty, 40, rows)
        assert inside.x0 // 64 == (inside.x0 + 39) // 64 and inside.y0 // ty == (inside.y0 + rows - 1) // ty
        assert (nx // 64) * (ny // ty) > 1                      # tiles without a window cell exist
        if rows > r:
            assert ty // r > (rows + r - 1) // r or (ny // ty) > 1   # ... and waves without one
        ws.append(inside)
    for w in ws:
        assert w.nx >= 1 and w.ny >= 1 and w.x0 + (w.nx - 1) * w.sx < nx and w.y0 + (w.ny - 1) * w.sy < ny, w
    return ws


def _windows(L, p, ob, cells, nsteps, every, windows, options=(), **kw):
    """One fresh context per window, the options, one run_window: [(av_vels, windows, lattice, info)]."""
    res = []
    for w in windows:
        with L.Lattice(p, ob, cells, **kw) as lat:
            for k, v in options:
                lat.set_option(k, v)
            av, out = lat.run_window(nsteps, every, w)
            res.append((av, out, lat.read_state(), {k: int(lat.info(k)) for k in INFO}))
    return res


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_window_run_is_declared_and_bound(L):
    assert "lbm_run_window" in L.ABI_SYMBOLS and "lbm_window_rows" in L.ABI_SYMBOLS
    hdr = open(L.HEADER_PATH).read()
    assert "typedef struct { int x0, y0, nx, ny, sx, sy; } lbm_window;" in hdr
    assert ("int lbm_run_window(lbm_ctx* ctx, int nsteps, float* av_vels, int every, const lbm_window* win, float* window_out);"
            in hdr)
    assert ("int lbm_window_rows(const lbm_window* win, int nx, int ny, int row_begin, int row_end, int* first, int* count);"
            in hdr)
    assert '"window_in_kernel"' in hdr and '"window_in_wave"' in hdr and "Which kernels take the window" in hdr
    lib = L.load_library()
    assert lib.lbm_run_window and lib.lbm_window_rows
    built = open(L.LIB_PATH, "rb").read()
    for key in (b"window_in_kernel", b"window_in_wave"):
        assert key + b"\0" in built, key
        v = C.c_double(-1.0)
        assert lib.lbm_get_info(None, key, C.byref(v)) == LBM_EINVAL and v.value == -1.0
    assert callable(L.Lattice.run_window) and callable(L.window_rows)
    assert "window_in_kernel" in L.Lattice.run_window.__doc__ and "window_in_wave" in L.Lattice.run_window.__doc__
    assert C.sizeof(L.Window) == 24


def test_window_calls_reject_null_arguments(L):
    lib = L.load_library()
    w = L.Window(0, 0, 1, 1)
    assert lib.lbm_run_window(None, 10, None, 5, C.byref(w), None) == LBM_EINVAL
    assert b"ctx" in lib.lbm_last_error()
    f, n = C.c_int(-7), C.c_int(-7)
    assert lib.lbm_window_rows(None, 64, 64, 0, 64, C.byref(f), C.byref(n)) == LBM_EINVAL
    assert b"win" in lib.lbm_last_error() and f.value == -7 and n.value == -7


def _brute(w, row_begin, row_end):
    return [r for r in range(w.ny) if row_begin <= w.y0 + r * w.sy < row_end]


def test_window_rows_against_brute_force(L):
    rng = np.random.default_rng(5)
    nx, ny = 96, 256
    checked = empty = between = 0
    for _ in range(400):
        sy = int(rng.integers(1, 40))
        y0 = int(rng.integers(0, ny))
        wny = int(rng.integers(1, (ny - 1 - y0) // sy + 2))
        w = L.Window(int(rng.integers(0, nx)), y0, 1, wny, int(rng.integers(1, 9)), sy)
        a = int(rng.integers(0, ny + 1))
        b = int(rng.integers(a, ny + 1))
        ranges = [(a, b), (a, a), (0, ny), (0, 0), (ny, ny)]
        if sy > 2 and wny > 1:
            ranges.append((y0 + 1, y0 + sy))                      # between two window rows
        ranges += [(k * ny // n, (k + 1) * ny // n) for n in (2, 3, 4, 8) for k in range(n)]
        for lo, hi in ranges:
            want = _brute(w, lo, hi)
            first, count = L.window_rows(w, nx, ny, lo, hi)
            assert count == len(want), (w, lo, hi, first, count, want)
            if want:
                assert first == want[0] and want == list(range(first, first + count)), (w, lo, hi, first, count)
            else:
                assert 0 <= first <= w.ny
                empty += 1
                between += (lo, hi) == (y0 + 1, y0 + sy)
            checked += 1
        for n in (2, 3, 4, 8):                                   # the slabs' rows partition the window's
            parts = [L.window_rows(w, nx, ny, k * ny // n, (k + 1) * ny // n) for k in range(n)]
            assert sum(c for _, c in parts) == w.ny
    assert checked > 5000 and empty > 500 and between > 50


def _refusals(L, nx, ny):
    W = L.Window
    return [W(0, 0, 0, 1), W(0, 0, 1, 0), W(0, 0, 1, 1, 0, 1), W(0, 0, 1, 1, 1, 0), W(0, 0, -1, 1), W(0, 0, 1, 1, -1, 1),
            W(-1, 0, 1, 1), W(0, -1, 1, 1), W(nx, 0, 1, 1), W(0, ny, 1, 1), W(0, 0, nx + 1, 1), W(0, 0, 1, ny + 1),
            W(1, 0, nx, 1), W(0, 0, nx // 2 + 1, 1, 2, 1), W(0, 1, 1, ny),
            # 32-bit products and sums that wrap to something small
            W(0, 0, 3, 1, INT_MAX, 1), W(0, 0, 1, 3, 1, INT_MAX), W(0, 0, INT_MAX, 1, 2, 1), W(0, 0, 1, INT_MAX, 1, 2),
            W(INT_MAX, 0, 1, 1), W(0, INT_MAX, 1, 1), W(1, 0, 2, 1, INT_MAX, 1), W(0, 1, 1, 2, 1, INT_MAX),
            W(0, 0, 65537, 1, 65536, 1), W(0, 0, 1, 65537, 1, 65536), W(2, 0, INT_MAX, 1, INT_MAX, 1)]


def test_window_rows_refuses_what_is_no_window(L):
    lib = L.load_library()
    nx, ny = 128, 64
    for w in _refusals(L, nx, ny):
        assert lib.lbm_window_rows(C.byref(w), nx, ny, 0, ny, None, None) == LBM_EINVAL, w
        assert lib.lbm_last_error()
    ok = L.Window(0, 0, nx, ny)
    assert lib.lbm_window_rows(C.byref(ok), nx, ny, 0, ny, None, None) == 0
    assert lib.lbm_window_rows(C.byref(ok), nx, ny, 5, 4, None, None) == LBM_EINVAL
    assert L.window_rows(L.Window(nx - 1, ny - 1, 1, 1, INT_MAX, INT_MAX), nx, ny, 0, ny) == (0, 1)   # (one cell: any stride)


def _oracle_window(L):
    return L.Window(0, 0, 64, 3, 1, 19)                           # rows 0, 19, 38 x all 64 columns


def test_the_oracles_own_fields_pass_the_window_bound(L, O, oracle):
    """The bar of test_window_against_the_float_oracle tests the kernel, not the bound: the strict float oracle's own float32
    final_state values in the window's cells sit inside the per-element bound of _oracle_fields at every step."""
    k, p, ob, op = _kat_case(L, O)
    w = _oracle_window(L)
    assert (p.nx, p.ny) == (64, 40)
    ref = k["cells0"].copy()
    worst = 0.0
    for _ in range(10):
        oracle.run(op, ref, ob, 1)
        want, tol = _oracle_fields(ref.reshape(p.ny, p.nx, 9), ob, k["density"])
        own = oracle.final_state(op, ref, ob).reshape(p.ny, p.nx, 4)
        err = np.abs(cut(own[None], w)[0].astype(np.float64) - cut(want[None], w)[0])
        lim = cut(tol[None], w)[0]
        assert err.shape == (3, 64, 4) and np.all(err <= lim), float(np.max(err - lim))
        worst = max(worst, float(np.max(err[lim > 0] / lim[lim > 0])))
    assert np.array_equal(ref, k["cells_after_10"])
    print("oracle's own window: worst error / bound %.3g" % worst)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _same(out, want, where):
    assert out.shape == want.shape, (where, out.shape, want.shape)
    bad = np.argwhere(_bits(out) != _bits(want))
    assert len(bad) == 0, (where, len(bad), [tuple(int(v) for v in b) for b in bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", TILINGS)
def test_windows_of_every_register_tiling(gpu, ty, r, asy, nx, ny):
    L = gpu
    p, ob, cells = _random_case(L, nx, ny, 7)
    nsteps = 11
    opts = (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3))
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts)
    ws = awkward_windows(L, nx, ny, ty, r)
    for every in (1, 4):
        _, fields, _ = _sampled(L, p, ob, cells, nsteps, every, opts)
        for w, (av, out, st, info) in zip(ws, _windows(L, p, ob, cells, nsteps, every, ws, opts)):
            assert info["engine_last"] == 3 and info["window_in_kernel"] == 1 and info["window_in_wave"] == 0, (w, info)
            _same(out, cut(fields, w), (w, every))
            assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(av), _bits(av0)), (w, every)


@pytest.mark.gpu
@pytest.mark.parametrize("deck", ["128x128", "1024x1024"])
def test_windows_on_the_shipped_decks(gpu, deck):
    L = gpu
    p, ob = _deck(L, deck)
    nsteps, every = 9, 4
    with L.Lattice(p, ob) as lat:
        ty, r = _tiling(lat)
    av0, st0 = _plain(L, p, ob, None, nsteps)
    _, fields, _ = _sampled(L, p, ob, None, nsteps, every)
    ws = awkward_windows(L, p.nx, p.ny, ty, r)
    for w, (av, out, st, info) in zip(ws, _windows(L, p, ob, None, nsteps, every, ws)):
        assert info["engine_last"] == 3 and info["window_in_kernel"] == 1, (w, info)
        _same(out, cut(fields, w), w)
        assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(av), _bits(av0)), w


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", [TILINGS[2], TILINGS[4]])
def test_windows_with_ieee_maths(gpu, ty, r, asy, nx, ny):
    L = gpu
    assert r in (2, 4)
    p, ob, cells = _random_case(L, nx, ny, 8)
    nsteps, every = 11, 4
    opts = (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3), ("kernel_variant", 0))
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts)
    _, fields, _ = _sampled(L, p, ob, cells, nsteps, every, opts)
    ws = awkward_windows(L, nx, ny, ty, r)
    for w, (av, out, st, info) in zip(ws, _windows(L, p, ob, cells, nsteps, every, ws, opts)):
        assert info["window_in_kernel"] == 1, (w, info)
        _same(out, cut(fields, w), w)
        assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(av), _bits(av0)), w


@pytest.mark.gpu
def test_the_probe_set_survives_a_window_run(gpu):
    L = gpu
    p, ob = _deck(L, "128x256")
    w = L.Window(0, 0, (p.nx + 2) // 3, (p.ny + 4) // 5, 3, 5)
    with L.Lattice(p, ob) as lat:
        ty, r = _tiling(lat)
        xy = awkward_set(p.nx, p.ny, ob, ty, r)
        lat.set_probes(xy)
        _, pr1 = lat.run_probes(8, 3)
        assert lat.info("probes_in_kernel") == 1
        _, win = lat.run_window(8, 3, w)
        assert lat.info("window_in_kernel") == 1 and lat.info("engine_last") == 3
        _, pr3 = lat.run_probes(8, 3)                              # the set and its tables, untouched by the window run
        assert lat.info("probes_in_kernel") == 1 and lat.info("engine_last") == 3
    with L.Lattice(p, ob) as twin:                                 # the equal state, recreated: no window run before the probes
        twin.run(16)
        twin.set_probes(xy)
        _, pr3_twin = twin.run_probes(8, 3)
    with L.Lattice(p, ob) as ref:
        f1, f2, f3 = (ref.run_sampled(8, 3)[1] for _ in range(3))
    assert np.array_equal(_bits(pr1), _bits(_pick(f1, xy)))
    _same(win, cut(f2, w), "window behind a probe run")
    assert np.array_equal(_bits(pr3), _bits(pr3_twin)) and np.array_equal(_bits(pr3), _bits(_pick(f3, xy)))


def _slab_windows(L, p, ty, r, nslabs):
    nyl = p.ny // nslabs
    ws = awkward_windows(L, p.nx, p.ny, ty, r)
    ws.append(L.Window(3, nyl + 1, 9, 3, 7, 2))                                  # every row in slab 1
    ws.append(L.Window(0, nyl - 1, (p.nx + 6) // 7, (nslabs - 2) * nyl + 2, 7, 1))   # rows on both sides of every border
    return ws


@pytest.mark.gpu
@pytest.mark.parametrize("deck,nslabs,exchange", [("256x256", 2, "copy"), ("256x256", 4, "copy"), ("256x256", 2, "p2p"),
                                                   ("256x256", 4, "p2p"), ("1024x1024", 2, "p2p")])
def test_slabs_give_the_single_slab_windows(gpu, deck, nslabs, exchange):
    L = gpu
    p, ob = _deck(L, deck)
    nsteps, every = 10, 4
    with L.Lattice(p, ob) as lat:
        ty, r = _tiling(lat)
    ws = _slab_windows(L, p, ty, r, nslabs)
    av1, st1 = _plain(L, p, ob, None, nsteps)
    ones = _windows(L, p, ob, None, nsteps, every, ws)
    ex = L.EXCHANGE_COPY if exchange == "copy" else L.EXCHANGE_P2P
    many = _windows(L, p, ob, None, nsteps, every, ws, nslabs=nslabs, devices=[0] * nslabs, exchange=ex)
    for w, (_, want, _, info1), (av, out, st, info) in zip(ws, ones, many):
        assert info1["window_in_kernel"] == 1
        _same(out, want, (w, info))
        assert np.array_equal(_bits(st), _bits(st1)), w
        assert np.allclose(av, av1, rtol=2e-6, atol=0), w
        if info["engine_last"] == 3:
            assert info["window_in_kernel"] == 1
        if exchange == "p2p":                # register tiles across slabs
            assert info["engine_last"] == 3 and info["window_in_kernel"] == 1, (w, info)


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["rccl", "p2p"])
def test_rank_context_ring_of_one_gives_the_single_slab_windows(gpu, exchange):
    L = gpu
    p, ob = _deck(L, "128x256")
    nsteps, every = 13, 5
    with L.Lattice(p, ob) as lat:
        ty, r = _tiling(lat)
    ws = awkward_windows(L, p.nx, p.ny, ty, r)
    av1, st1 = _plain(L, p, ob, None, nsteps)
    ones = _windows(L, p, ob, None, nsteps, every, ws)
    os.environ["LBM_FORCE_EXCHANGE"] = "1"
    try:
        ex = L.EXCHANGE_RCCL if exchange == "rccl" else L.EXCHANGE_P2P
        ring = [_windows(L, p, ob, None, nsteps, every, [w], rank=0, nranks=1, device=0, unique_id=L.rccl_unique_id(),
                         exchange=ex)[0] for w in ws]             # (a fresh id per communicator)
    finally:
        del os.environ["LBM_FORCE_EXCHANGE"]
    for w, (_, want, _, _), (av, out, st, info) in zip(ws, ones, ring):
        _same(out, want, (w, info))
        assert np.array_equal(_bits(st), _bits(st1)), w
        assert np.allclose(av, av1, rtol=2e-6, atol=0), w


@pytest.mark.gpu
@pytest.mark.parametrize("time_block", [1, 2, 4, 8])
def test_streaming_engines_give_the_register_tiles_windows(gpu, time_block):
    L = gpu
    p, ob = _deck(L, "256x256")
    nsteps, every = 21, 3
    with L.Lattice(p, ob) as lat:
        ty, r = _tiling(lat)
    ws = awkward_windows(L, p.nx, p.ny, ty, r)
    tiles = _windows(L, p, ob, None, nsteps, every, ws)
    # (march_kernel 0 keeps lbm_wave away at time_block 4 and 8 here: its own flavour has its own test file)
    opts = (("engine", 1), ("march_kernel", 0), ("time_block", time_block))
    av0, st0 = _plain(L, p, ob, None, nsteps, opts)
    for w, (_, want, st_t, info_t), (av, out, st, info) in zip(ws, tiles, _windows(L, p, ob, None, nsteps, every, ws, opts)):
        assert info_t["window_in_kernel"] == 1
        assert info == dict(engine_last=1, window_in_kernel=0, window_in_wave=0), (w, info)
        _same(out, want, (w, time_block))
        assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(st), _bits(st_t)), w
        assert np.allclose(av, av0, rtol=2e-6, atol=0), w


@pytest.mark.gpu
def test_a_lattice_that_does_not_tile_gives_the_sliced_snapshots(gpu):
    L = gpu
    nx, ny = 200, 72
    p, ob, cells = _random_case(L, nx, ny, 12)
    nsteps, every = 11, 3
    opts = (("time_block", 1),)
    _, fields, st0 = _sampled(L, p, ob, cells, nsteps, every, opts)
    ws = [L.Window(0, 0, nx, ny), L.Window(199, 71, 1, 1), L.Window(0, ny - 2, nx, 1), L.Window(1, 2, 67, 14, 3, 5),
          L.Window(150, 0, 50, 72)]
    for w, (av, out, st, info) in zip(ws, _windows(L, p, ob, cells, nsteps, every, ws, opts)):
        assert info == dict(engine_last=1, window_in_kernel=0, window_in_wave=0), (w, info)
        _same(out, cut(fields, w), w)
        assert np.array_equal(_bits(st), _bits(st0)), w


# torch and the library share libamdhip64: torch is imported FIRST, in a child process of its own
_DEVICE_OUTPUT = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_window_run import _deck, _sampled, _bits, cut
p, ob = _deck(L, "128x256")
nsteps, every = 12, 5
_, fields, st_h = _sampled(L, p, ob, None, nsteps, every)
for w in (L.Window(0, 0, p.nx, p.ny), L.Window(61, 15, 7, 5), L.Window(0, 0, 43, 52, 3, 5)):
    want = cut(fields, w)
    for engine, key in ((0, 1), (1, 0)):                # the register tiles; the streaming engines' pieces
        out = torch.full((nsteps // every, w.ny, w.nx, 4), float("nan"), dtype=torch.float32, device="cuda:0")
        with L.Lattice(p, ob) as lat:
            lat.set_option("engine", engine)
            av, got = lat.run_window(nsteps, every, w, out=out)
            assert got is out and lat.info("window_in_kernel") == key and lat.info("window_in_wave") == 0
            st = lat.read_state()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (w, engine)
        assert np.array_equal(_bits(st), _bits(st_h))
print("device output ok")
"""


@pytest.mark.gpu
def test_device_output_is_the_host_output(gpu):
    assert "device output ok" in _child(_DEVICE_OUTPUT)


@pytest.mark.gpu
def test_refusals_leave_the_lattice_alone(gpu):
    L = gpu
    lib = L.load_library()
    p, ob = _deck(L, "128x128")
    ok = L.Window(3, 5, 20, 10, 2, 3)
    out = np.full((10, 10, 20, 4), np.nan, np.float32)

    def refused(rc, *words):
        assert rc == LBM_EINVAL
        msg = lib.lbm_last_error().decode()
        for wd in words:
            assert wd in msg, (wd, msg)

    with L.Lattice(p, ob) as lat:
        lat.run(3)
        refused(lib.lbm_run_window(lat._ctx, 10, None, 1, None, out.ctypes.data), "win")
        for w in _refusals(L, p.nx, p.ny):
            refused(lib.lbm_run_window(lat._ctx, 10, None, 1, C.byref(w), out.ctypes.data), "window")
        refused(lib.lbm_run_window(lat._ctx, -1, None, 1, C.byref(ok), out.ctypes.data), "nsteps")
        refused(lib.lbm_run_window(lat._ctx, 10, None, -1, C.byref(ok), out.ctypes.data), "every")
        refused(lib.lbm_run_window(lat._ctx, 10, None, 5, C.byref(ok), None), "window_out")
        with pytest.raises(L.LbmError):
            lat.run_window(10, 1, L.Window(0, 0, p.nx + 1, 1))
        assert np.isnan(out).all()
        av = lat.run(10)
        st1 = lat.read_state()
    with L.Lattice(p, ob) as ref:
        av_ref = ref.run(13)
        assert np.array_equal(_bits(st1), _bits(ref.read_state()))
        assert np.array_equal(_bits(av), _bits(av_ref[3:]))


@pytest.mark.gpu
def test_no_samples_is_lbm_run(gpu):
    L = gpu
    lib = L.load_library()
    p, ob = _deck(L, "128x128")
    av0, st0 = _plain(L, p, ob, None, 12)
    w = L.Window(3, 5, 20, 10, 2, 3)
    out = np.full((12, 10, 20, 4), np.nan, np.float32)
    for every in (0, 13):
        with L.Lattice(p, ob) as lat:
            av = np.empty(12, np.float32)
            assert lib.lbm_run_window(lat._ctx, 12, av.ctypes.data, every, C.byref(w), out.ctypes.data) == 0
            assert lat.info("window_in_kernel") == 0 and lat.info("window_in_wave") == 0 and lat.info("engine_last") == 3
            assert np.array_equal(_bits(av), _bits(av0)) and np.array_equal(_bits(lat.read_state()), _bits(st0))
            _, none = lat.run_window(5, every, w)                  # (window_out may be NULL)
            assert none.shape == (0, 10, 20, 4)
    assert np.isnan(out).all()


@pytest.mark.gpu
def test_window_against_the_float_oracle(gpu, O, oracle):
    """64 x 40 known-answer lattice, 10 steps, every step a sample, the window rows 0, 19, 38 x all 64 columns (sy = 19),
    against fields derived from the strict float oracle's lattice at each step: the lattice to 2e-5 relative, as smoke(),
    carried through the derive -- the per-element bound of _oracle_fields, derived, not tuned."""
    L = gpu
    k, p, ob, op = _kat_case(L, O)
    w = _oracle_window(L)
    (_, out, st, info), = _windows(L, p, ob, k["cells0"], 10, 1, [w])
    assert info["window_in_kernel"] == 1 and out.shape == (10, 3, 64, 4)
    ref = k["cells0"].copy()
    for j in range(10):
        oracle.run(op, ref, ob, 1)
        want, tol = _oracle_fields(ref.reshape(p.ny, p.nx, 9), ob, k["density"])
        err = np.abs(out[j].astype(np.float64) - cut(want[None], w)[0])
        lim = cut(tol[None], w)[0]
        print("step %d: max error %.3g, worst error - bound %.3g" % (j + 1, err.max(), np.max(err - lim)))
        assert np.all(err <= lim), (j, float(np.max(err - lim)))
    assert np.array_equal(ref, k["cells_after_10"])
