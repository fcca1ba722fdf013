"""lbm_run_window_stats where lbm_wave runs (a lattice alone, time_block 4 / 6 / 8): the sums ride in lbm_wave's launches.

Contract (include/lbm_mi355x.h): at a sample level of a pass the window-stats flavour of lbm_wave tests the level's row
against the window (wave-uniform), then each of a lane's cells against the window's columns, as the window flavour does,
and adds a window cell's four fields and their products into its record of eight floats, as the stats flavour does, in the
order of the steps.  So the output is tests/test_stats_run.py's stats_of of tests/test_window_run.py's cut of the split
path's snapshots (engine 1, time_block 1, lbm_run_sampled at every = 1, once per case: _reference of
tests/test_wave_fields.py) bit for bit; av_vels and the lattice are lbm_run's bits; info "window_stats_in_wave" reads 1,
"window_stats_in_kernel" 0, and "wave_launches" n // K on a fresh context: one kernel per pass, a pass without a sample step
in the plain kernel.  Runs shorter than K and slabs with neighbours keep the split path: the same bits, the key 0.

Shapes, kernels and windows: those of tests/test_wave_window.py."""
import numpy as np
import pytest

from test_body_forces import _bits, _plain
from test_stats_run import p0_of, stats_of
from test_wave_fields import KERNELS, SHAPES, NMAX, _context, _lbm_run, _reference
from test_wave_probes import _opts
from test_wave_window import wave_windows
from test_window_run import cut, _same

INFO = ("window_stats_in_wave", "window_stats_in_kernel", "window_stats_pieces", "engine_last", "time_block_active", "wave_launches")


def _run(L, p, ob, cells, nsteps, every, w, options=(), **kw):
    with _context(L, p, ob, cells, options, **kw) as lat:
        av, out = lat.run_window_stats(nsteps, every, w)
        info = {k: int(lat.info(k)) for k in INFO}
        st = lat.read_state()
    return av, out, st, info


def _expected(S1, w, p0, nsteps, every):
    return stats_of(cut(S1[every - 1:nsteps:every][:nsteps // every], w), p0)


def _check(L, nx, ny, seed, K, cols, nsteps, every, rows=0, in_wave=1, extra=(), windows=None):
    (p, ob, cells), S1 = _reference(L, nx, ny, seed, extra)
    p0 = p0_of(p.density)
    opts = _opts(K, cols, rows) + extra
    av0, st0 = _lbm_run(L, (nx, ny, seed), p, ob, cells, nsteps, opts)
    for w in (windows or wave_windows(L, nx, ny, K, cols)):
        av, out, st, info = _run(L, p, ob, cells, nsteps, every, w, opts)
        where = (w, nx, ny, K, cols, rows, nsteps, every, info)
        assert info["window_stats_in_wave"] == in_wave and info["window_stats_in_kernel"] == 0 and info["engine_last"] == 1, where
        assert info["time_block_active"] == K, where
        if in_wave:                                       # a fresh context: one lbm_wave kernel per pass, sample step or none
            assert info["wave_launches"] == nsteps // K and info["window_stats_pieces"] == 1, where
        _same(out, _expected(S1, w, p0, nsteps, every), where)
        assert np.array_equal(_bits(st), _bits(st0)), where
        if in_wave:
            assert np.array_equal(_bits(av), _bits(av0)), where
        else:                                             # the split path: lbm_run's to rounding
            assert np.allclose(av, av0, rtol=2e-6, atol=0), where


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_window_stats_are_the_bits_of_the_split_path(gpu, K, cols):
    """2 K + 5 steps: two passes, then two pairs and a single step.  every = 1: every level of every pass and every
    left-over step; 3: divides no K; K; K + 1: the first pass holds no sample and runs the plain kernel."""
    assert 2 * K + 5 <= NMAX
    for nx, ny, seed, rows in SHAPES:
        for every in (1, 3, K, K + 1):
            _check(gpu, nx, ny, seed, K, cols, 2 * K + 5, every, rows=rows)


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_window_stats_at_one_pass_and_below(gpu, K, cols):
    L = gpu
    nx, ny, seed, rows = SHAPES[0]
    ws = wave_windows(L, nx, ny, K, cols)
    few = [ws[0], ws[1], ws[-4]]
    _check(L, nx, ny, seed, K, cols, K, 1, rows=rows, windows=few)                        # one pass, no left-over step
    _check(L, nx, ny, seed, K, cols, K - 1, 1, rows=rows, in_wave=0, windows=few)         # below one pass: the split path


@pytest.mark.gpu
def test_wave_window_stats_with_ieee_maths(gpu):
    """kernel_variant 0 (IEEE division and square root), one kernel per shape, against the split path under the same."""
    ieee = (("kernel_variant", 0),)
    for (nx, ny, seed, rows), (K, cols) in zip(SHAPES, ((8, 2), (6, 1))):
        for every in (1, 3):
            _check(gpu, nx, ny, seed, K, cols, 2 * K + 5, every, rows=rows, extra=ieee)


@pytest.mark.gpu
def test_two_slabs_keep_the_split_path(gpu):
    L = gpu
    nx, ny, seed, _ = SHAPES[0]
    (p, ob, cells), S1 = _reference(L, nx, ny, seed)
    p0 = p0_of(p.density)
    nsteps, every = 13, 3
    opts, kw = (("engine", 1), ("time_block", 8)), dict(nslabs=2, devices=[0, 0], exchange=L.EXCHANGE_COPY)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts, **kw)
    for w in wave_windows(L, nx, ny, 8, 2):
        av, out, st, info = _run(L, p, ob, cells, nsteps, every, w, opts, **kw)
        assert info["window_stats_in_wave"] == 0 and info["window_stats_in_kernel"] == 0, (w, info)
        assert info["engine_last"] == 1 and info["wave_launches"] == 0 and info["window_stats_pieces"] == 5, (w, info)
        _same(out, _expected(S1, w, p0, nsteps, every), w)
        assert np.array_equal(_bits(st), _bits(st0))
        assert np.allclose(av, av0, rtol=2e-6, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", [(6, 1), (8, 2)])
def test_the_whole_lattice_window_is_run_stats(gpu, K, cols):
    """Floats 0..7 of the whole-lattice window equal lbm_run_stats' output under the same options, both in lbm_wave."""
    L = gpu
    nx, ny, seed, rows = SHAPES[0]
    (p, ob, cells), _ = _reference(L, nx, ny, seed)
    opts = _opts(K, cols, rows)
    nsteps = 2 * K + 5
    for every in (1, 3):
        with _context(L, p, ob, cells, opts) as lat:
            av_s, full = lat.run_stats(nsteps, every)
            assert lat.info("stats_in_wave") == 1
        av, out, _, info = _run(L, p, ob, cells, nsteps, every, L.Window(0, 0, nx, ny), opts)
        assert info["window_stats_in_wave"] == 1, info
        _same(out, full, (K, cols, every))
        assert np.array_equal(_bits(av), _bits(av_s))
