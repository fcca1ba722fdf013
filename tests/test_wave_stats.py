"""lbm_run_stats where lbm_wave runs (a lattice alone, time_block 4 / 6 / 8): the eight sums ride in lbm_wave's launches.

Contract (include/lbm_mi355x.h): at a sample level of a pass the stats flavour of lbm_wave takes derive_cell of every
delivered cell, as the field flavour does, and adds the four fields and their products (u_x^2, u_y^2, u_x u_y, (p - p0)^2)
into the cell's record of eight floats, in the order of the steps.  So the output is tests/test_stats_run.py's stats_of of
the split path's snapshots (engine 1, time_block 1, lbm_run_sampled at every = 1, once per case: _reference of
tests/test_wave_fields.py) bit for bit; floats 0..3 are lbm_run_mean's bits under the same options; av_vels and the lattice
are lbm_run's bits; info "stats_in_wave" reads 1, "mean_in_kernel" 0, and "wave_launches" n // K on a fresh context: one
kernel per pass, a pass without a sample step in the plain kernel.  Runs shorter than K and slabs with neighbours keep the
split path: the same bits, the key 0.

Shapes and kernels: those of tests/test_wave_fields.py -- 256 x 64 with wave_rows 24, 200 x 72; (K, columns) = (4, 1), (6, 1),
(8, 1), (8, 2); 2 K + 5 steps; every = 1, 3, K, K + 1."""
import numpy as np
import pytest

from test_body_forces import _bits, _plain
from test_stats_run import p0_of, stats_of
from test_wave_fields import KERNELS, SHAPES, SPLIT, _context, _lbm_run, _reference, _run
from test_wave_probes import _opts

INFO = ("stats_in_wave", "mean_in_wave", "mean_in_kernel", "engine_last", "time_block_active", "wave_launches")


def _stats(L, p, ob, cells, nsteps, every, options=(), **kw):
    with _context(L, p, ob, cells, options, **kw) as lat:
        av, out = lat.run_stats(nsteps, every)
        info = {k: int(lat.info(k)) for k in INFO}
        st = lat.read_state()
    return av, out, st, info


def _expected(S1, p0, nsteps, every):
    return stats_of(S1[every - 1:nsteps:every][:nsteps // every], p0)


def _check(L, nx, ny, seed, K, cols, nsteps, every, rows=0, in_wave=1, extra=()):
    (p, ob, cells), S1 = _reference(L, nx, ny, seed, extra)
    p0 = p0_of(p.density)
    blocked = np.asarray(ob).reshape(ny, nx) != 0
    assert blocked.any() and np.all(_bits(S1[0][blocked][:, 3]) == _bits(p0))        # p0 is a blocked cell's snapshot pressure
    opts = _opts(K, cols, rows) + extra
    av, out, st, info = _stats(L, p, ob, cells, nsteps, every, opts)
    av0, st0 = _lbm_run(L, (nx, ny, seed), p, ob, cells, nsteps, opts)
    where = (nx, ny, K, cols, rows, nsteps, every, info)
    assert info["stats_in_wave"] == in_wave and info["mean_in_kernel"] == 0 and info["mean_in_wave"] == 0, where
    assert info["engine_last"] == 1 and info["time_block_active"] == K, where
    if in_wave:                                       # a fresh context: one lbm_wave kernel per pass, sample step or none
        assert info["wave_launches"] == nsteps // K, where
    want = _expected(S1, p0, nsteps, every)
    assert out.shape == want.shape == (ny, nx, 8), where
    bad = np.argwhere(_bits(out) != _bits(want))
    assert len(bad) == 0, (where, len(bad), [tuple(int(v) for v in b) for b in bad[:8]])
    _, mean, _, minfo = _run(L, "mean", p, ob, cells, nsteps, every, opts)
    assert minfo["mean_in_wave"] == in_wave, (where, minfo)
    assert np.array_equal(_bits(out[..., :4]), _bits(mean)), where
    assert np.all(_bits(out[blocked][:, 4:]) == 0) and np.all(_bits(out[blocked][:, :3]) == 0), where
    assert np.array_equal(_bits(st), _bits(st0)), where
    if in_wave:
        assert np.array_equal(_bits(av), _bits(av0)), where
    else:                                             # the split path: lbm_run's to rounding
        assert np.allclose(av, av0, rtol=2e-6, atol=0), where


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_stats_are_the_bits_of_the_split_path(gpu, K, cols):
    """2 K + 5 steps: two passes, then two pairs and a single step.  every = 1: every level of every pass and every
    left-over step; 3: divides no K; K; K + 1: the first pass holds no sample and runs the plain kernel."""
    for nx, ny, seed, rows in SHAPES:
        for every in (1, 3, K, K + 1):
            _check(gpu, nx, ny, seed, K, cols, 2 * K + 5, every, rows=rows)


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_stats_at_one_pass_and_below(gpu, K, cols):
    nx, ny, seed, rows = SHAPES[0]
    _check(gpu, nx, ny, seed, K, cols, K, 1, rows=rows)                        # one pass, no left-over step
    _check(gpu, nx, ny, seed, K, cols, K - 1, 1, rows=rows, in_wave=0)         # below one pass: the split path


@pytest.mark.gpu
def test_wave_stats_with_ieee_maths(gpu):
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
    nsteps, every = 13, 3
    opts, kw = (("engine", 1), ("time_block", 8)), dict(nslabs=2, devices=[0, 0], exchange=L.EXCHANGE_COPY)
    av, out, st, info = _stats(L, p, ob, cells, nsteps, every, opts, **kw)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts, **kw)
    assert info["stats_in_wave"] == 0 and info["engine_last"] == 1 and info["wave_launches"] == 0, info
    assert np.array_equal(_bits(out), _bits(_expected(S1, p0_of(p.density), nsteps, every)))
    assert np.array_equal(_bits(st), _bits(st0))
    assert np.allclose(av, av0, rtol=2e-6, atol=0)


@pytest.mark.gpu
def test_one_context_through_mixed_calls(gpu):
    """run_stats, run, run_mean and run_stats again on one context where lbm_wave runs: after each call the lattice and
    av_vels are those of a twin that only calls run; the key is reset by each call; the second result is a fresh context's
    and stats_of of the split path's snapshots from the same step."""
    L = gpu
    nx, ny, seed, rows = SHAPES[0]
    (p, ob, cells), S1 = _reference(L, nx, ny, seed)
    p0 = p0_of(p.density)
    opts = _opts(8, 2, rows)
    with _context(L, p, ob, cells, opts) as lat, _context(L, p, ob, cells, opts) as twin:

        def same(av):
            assert np.array_equal(_bits(av), _bits(twin.run(len(av))))
            assert np.array_equal(_bits(lat.read_state()), _bits(twin.read_state()))

        av, s1 = lat.run_stats(19, 2)
        assert lat.info("stats_in_wave") == 1 and lat.info("wave_launches") == 2
        same(av)
        assert np.array_equal(_bits(s1), _bits(stats_of(S1[1:19:2], p0)))
        same(lat.run(9))
        av, _ = lat.run_stats(7, 1)                   # shorter than K: the split path, the key reset
        assert lat.info("stats_in_wave") == 0
        assert np.allclose(av, twin.run(7), rtol=2e-6, atol=0)
        assert np.array_equal(_bits(lat.read_state()), _bits(twin.read_state()))
        av, _ = lat.run_mean(20, 4)
        assert lat.info("mean_in_wave") == 1
        same(av)
        av, s2 = lat.run_stats(21, 4)
        assert lat.info("stats_in_wave") == 1 and lat.info("engine_last") == 1
        same(av)
    with _context(L, p, ob, cells, SPLIT) as fresh:
        fresh.run(55)
        _, fields = fresh.run_sampled(21, 4)
    assert np.array_equal(_bits(s2), _bits(stats_of(fields, p0)))
