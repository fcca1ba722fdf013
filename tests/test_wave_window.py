"""lbm_run_window where lbm_wave runs (a lattice alone, time_block 4 / 6 / 8): the window rides in lbm_wave's launches.

Contract (include/lbm_mi355x.h): at a sample level of a pass the window flavour of lbm_wave tests the level's row against
the window (wave-uniform), then each of a lane's cells against the window's columns, and stores derive_cell of a window
cell's populations -- after collide_cell, before accelerate_cell -- into its place of the sample's window.  So the windows
are the BITS of the split path's snapshots (engine 1, time_block 1: pieces of `every` steps, lbm_derive behind each) in the
window's cells; av_vels and the lattice are the bits of lbm_run under the same options; info "window_in_wave" reads 1
("window_in_kernel" keeps meaning the register tiles: 0 here); "wave_launches" grows by ONE kernel per pass.  Contexts where
lbm_march runs, slabs with neighbours and runs shorter than K keep the split path.

Shapes and kernels are those of tests/test_wave_fields.py: 256 x 64 with wave_rows 24 (chunks of 24, 24 and 16 rows) and
200 x 72; the split path runs once per shape, at every = 1 over the longest run (21 steps), and is sliced."""
import numpy as np
import pytest

from test_body_forces import _bits, _plain
from test_mean_run import _child
from test_wave_probes import _opts
from test_wave_fields import KERNELS, SHAPES, NMAX, _reference, _lbm_run, _context
from test_window_run import cut, _same

MI355X_HBM_BYTES = 288 * 2 ** 30          # the device's memory (8 stacks of 36 GiB)
INFO = ("window_in_wave", "window_in_kernel", "engine_last", "time_block_active", "wave_launches")


def wave_windows(L, nx, ny, K, cols):
    """The whole lattice; rows 22..25 and 46..49 x all columns (chunk edges at 24 and 48); four columns around every strip
    edge (multiples of 64 cols - 2 K: 56, 48, 112, and the last, narrower strip) x all rows; strides (3, 3) from (1, 1) (two
    columns per lane: alternately a lane's first and second cell); strides (2, 1) from x0 = 1 (second cells only); the rows
    ny - 2, ny - 1 and 0; a single cell."""
    W = L.Window
    vw = 64 * cols - 2 * K
    ws = [W(0, 0, nx, ny), W(0, 22, nx, 4), W(0, 46, nx, 4)]
    edges = list(range(vw, nx, vw))
    assert edges and (nx - edges[-1]) <= vw
    for e in edges:
        ws.append(W(e - 2, 0, min(4, nx - (e - 2)), ny))
    ws += [W(1, 1, (nx - 2) // 3 + 1, (ny - 2) // 3 + 1, 3, 3), W(1, 0, (nx - 2) // 2 + 1, ny, 2, 1),
           W(0, ny - 2, nx, 2), W(0, 0, nx, 1), W(nx - 1, ny // 2, 1, 1), W(17, 0, 1, 1, 5, 7)]
    for w in ws:
        assert w.x0 + (w.nx - 1) * w.sx < nx and w.y0 + (w.ny - 1) * w.sy < ny, w
    return ws


def _run(L, p, ob, cells, nsteps, every, w, options=(), **kw):
    with _context(L, p, ob, cells, options, **kw) as lat:
        av, out = lat.run_window(nsteps, every, w)
        info = {k: int(lat.info(k)) for k in INFO}
        st = lat.read_state()
    return av, out, st, info


def _check(L, nx, ny, seed, K, cols, nsteps, every, rows=0, in_wave=1, extra=(), windows=None):
    (p, ob, cells), S1 = _reference(L, nx, ny, seed, extra)
    opts = _opts(K, cols, rows) + extra
    av0, st0 = _lbm_run(L, (nx, ny, seed), p, ob, cells, nsteps, opts)
    snaps = S1[every - 1:nsteps:every][:nsteps // every]
    for w in (windows or wave_windows(L, nx, ny, K, cols)):
        av, out, st, info = _run(L, p, ob, cells, nsteps, every, w, opts)
        where = (w, nx, ny, K, cols, rows, nsteps, every, info)
        assert info["window_in_wave"] == in_wave and info["window_in_kernel"] == 0 and info["engine_last"] == 1, where
        assert info["time_block_active"] == K, where
        if in_wave:                                       # a fresh context: one lbm_wave kernel per pass, sample step or none
            assert info["wave_launches"] == nsteps // K, where
        _same(out, cut(snaps, w), where)
        assert np.array_equal(_bits(st), _bits(st0)), where
        if in_wave:
            assert np.array_equal(_bits(av), _bits(av0)), where
        else:                                             # the split path: lbm_run's to rounding
            assert np.allclose(av, av0, rtol=2e-6, atol=0), where


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_windows_are_the_bits_of_the_split_path(gpu, K, cols):
    """2 K + 5 steps: two passes, then two pairs and a single step.  every = 1: every level of every pass and every left-over
    step; 3: divides no K; K + 1: the first pass holds no sample and runs the plain kernel."""
    assert 2 * K + 5 <= NMAX
    for nx, ny, seed, rows in SHAPES:
        for every in (1, 3, K + 1):
            _check(gpu, nx, ny, seed, K, cols, 2 * K + 5, every, rows=rows)


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_windows_at_one_pass_and_below(gpu, K, cols):
    L = gpu
    nx, ny, seed, rows = SHAPES[0]
    ws = wave_windows(L, nx, ny, K, cols)
    few = [ws[0], ws[1], ws[-4]]
    _check(L, nx, ny, seed, K, cols, K, 1, rows=rows, windows=few)                        # one pass, no left-over step
    _check(L, nx, ny, seed, K, cols, K - 1, 1, rows=rows, in_wave=0, windows=few)         # below one pass: the split path


@pytest.mark.gpu
def test_wave_windows_with_ieee_maths(gpu):
    """kernel_variant 0 (IEEE division and square root), one kernel per shape, against the split path under the same."""
    ieee = (("kernel_variant", 0),)
    for (nx, ny, seed, rows), (K, cols) in zip(SHAPES, ((8, 2), (6, 1))):
        for every in (1, 3):
            _check(gpu, nx, ny, seed, K, cols, 2 * K + 5, every, rows=rows, extra=ieee)


@pytest.mark.gpu
@pytest.mark.parametrize("context", ["lbm_march", "two_slabs"])
def test_contexts_that_keep_the_split_path(gpu, context):
    L = gpu
    nx, ny, seed, _ = SHAPES[0]
    (p, ob, cells), S1 = _reference(L, nx, ny, seed)
    nsteps, every = 13, 3
    if context == "lbm_march":
        opts, kw = _opts(4, kernel=0), {}
    else:
        opts, kw = (("engine", 1), ("time_block", 8)), dict(nslabs=2, devices=[0, 0], exchange=L.EXCHANGE_COPY)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts, **kw)
    snaps = S1[every - 1:nsteps:every][:nsteps // every]
    for w in wave_windows(L, nx, ny, 8, 2):
        av, out, st, info = _run(L, p, ob, cells, nsteps, every, w, opts, **kw)
        assert info["window_in_wave"] == 0 and info["window_in_kernel"] == 0 and info["engine_last"] == 1, (w, info)
        if context == "lbm_march":
            assert info["time_block_active"] == 4
        _same(out, cut(snaps, w), (context, w))
        assert np.array_equal(_bits(st), _bits(st0))
        assert np.allclose(av, av0, rtol=2e-6, atol=0)


# torch and the library share libamdhip64: torch is imported FIRST, in a child process of its own
_DEVICE_OUTPUT = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_wave_window import _bits, _context, _opts, wave_windows
from test_body_forces import _random_case
p, ob, cells, _ = _random_case(L, 256, 64, 11)
nsteps, every = 21, 3
for K, cols in ((6, 1), (8, 2)):
    ws = wave_windows(L, 256, 64, K, cols)
    for w in (ws[0], ws[1], ws[3], ws[-6]):
        with _context(L, p, ob, cells, _opts(K, cols, 24)) as lat:
            av_h, want = lat.run_window(nsteps, every, w)
            assert lat.info("window_in_wave") == 1
            st_h = lat.read_state()
        out = torch.full((nsteps // every, w.ny, w.nx, 4), float("nan"), dtype=torch.float32, device="cuda:0")
        with _context(L, p, ob, cells, _opts(K, cols, 24)) as lat:
            av, got = lat.run_window(nsteps, every, w, out=out)
            assert got is out and lat.info("window_in_wave") == 1
            st = lat.read_state()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (K, cols, w)
        assert np.array_equal(_bits(av), _bits(av_h)) and np.array_equal(_bits(st), _bits(st_h))
print("device output ok")
"""


@pytest.mark.gpu
def test_device_output_is_the_host_output(gpu):
    assert "device output ok" in _child(_DEVICE_OUTPUT)


@pytest.mark.gpu
def test_a_series_the_full_snapshots_could_not_stage(gpu):
    """8192 x 1024, where lbm_wave is the default engine, from the rest equilibrium; every step a sample, and so many steps
    that the snapshots of lbm_run_sampled (128 MiB each) would pass the device's memory: its one staging could not exist.
    The window, 64 x 32 cells at strides (128, 32), stages 32 KiB per sample.  Samples 0, 7, 8 (both sides of a pass border)
    and the last are the window's cells of lbm_final_state of a fresh context run that many steps.  (Info "hbm_bytes" is what
    the CONTEXT holds on the device, 0.6 GB here, which five snapshots pass; the series is sized against the larger figure,
    the 288 GiB of the device itself: 2305 steps.)"""
    L = gpu
    from test_large_observers import PARAMS
    nx, ny = 8192, 1024
    p = L.Param(nx, ny, 10, 10, *PARAMS)
    ob = np.zeros((ny, nx), np.int32)
    w = L.Window(5, 3, 64, 32, 128, 32)
    with L.Lattice(p, ob) as lat:
        hbm = max(lat.info("hbm_bytes"), float(MI355X_HBM_BYTES))
        nsteps = int(hbm // (nx * ny * 16)) + 1
        assert nsteps * nx * ny * 16 > MI355X_HBM_BYTES > lat.info("hbm_bytes") and nsteps == 2305, (hbm, nsteps)
        av, out = lat.run_window(nsteps, 1, w)
        info = {k: int(lat.info(k)) for k in INFO}
    print("hbm_bytes %.0f, %d steps, %.1f MB of windows, %s" % (hbm, nsteps, out.nbytes / 1e6, info))
    assert info["window_in_wave"] == 1 and info["window_in_kernel"] == 0 and info["time_block_active"] == 8, info
    assert info["wave_launches"] == nsteps // 8, info                 # (a split run would launch none)
    assert out.shape == (nsteps, 32, 64, 4) and not np.isnan(out).any()
    with L.Lattice(p, ob) as ref:
        done = 0
        for j in (0, 7, 8):
            ref.run(j + 1 - done)
            done = j + 1
            _same(out[j:j + 1], cut(ref.final_state()[None], w), ("sample", j))
        av_tail = ref.run(nsteps - done)
        _same(out[-1:], cut(ref.final_state()[None], w), "the last sample")
    with L.Lattice(p, ob) as plain:
        av0 = plain.run(nsteps)
    assert np.array_equal(_bits(av), _bits(av0))
