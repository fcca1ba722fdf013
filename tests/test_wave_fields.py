"""lbm_run_sampled and lbm_run_mean where lbm_wave runs (a lattice alone, time_block 4 / 6 / 8): the fields ride in
lbm_wave's launches.

Contract (include/lbm_mi355x.h): at a sample level of a pass the field flavour of lbm_wave evaluates derive_cell on the
populations every delivered cell holds after collide_cell and before accelerate_cell -- the values the stored lattice of
that step would hold at the end of a run -- and stores them into the snapshot (lbm_run_sampled) or adds them into the sums
(lbm_run_mean), in the order of the steps.  So the snapshots are the BITS of the split path (engine 1, time_block 1: pieces
of `every` steps, lbm_derive behind each), the mean is test_mean_run.mean_of of those snapshots bit for bit; av_vels and
the lattice are the bits of lbm_run under the same options; info "samples_in_wave" / "mean_in_wave" reads 1
("samples_in_kernel" / "mean_in_kernel" keep meaning the register tiles: 0 here).  Contexts where lbm_march runs, slabs with
neighbours and runs shorter than K keep the split path.  Info "wave_launches" counts the lbm_wave kernels a context has
launched: a run of n steps in wave launches n // K of them, ONE per pass whether the pass holds a sample step or not -- a
field pass that also ran the plain kernel over the same lattices would leave every bit as it is and show only there.

Shapes (those of tests/test_wave_probes.py): 256 x 64 with wave_rows 24 (several wave columns, two blocks, chunks of 24, 24
and 16 rows) and 200 x 72 (a width that is no multiple of 64 - 2 K, nor of 64).  The fields of step s depend on the lattice
after step s alone, so the split path runs once per case, at every = 1 over the longest run (21 steps), and a run at another
period is compared with its rows every - 1, 2 every - 1, ..."""
import ctypes as C

import numpy as np
import pytest

from test_body_forces import _bits, _plain, _random_case
from test_mean_run import _child, _kat_case, _oracle_mean_bound, _within, mean_of
from test_wave_probes import _opts, probe_set

LBM_EINVAL = 1
NMAX = 21                     # 2 K + 5 at K = 8
SPLIT = (("engine", 1), ("time_block", 1))
KERNELS = [(4, 1), (6, 1), (8, 1), (8, 2)]
SHAPES = [(256, 64, 11, 24), (200, 72, 12, 0)]        # nx, ny, seed, wave_rows
KEYS = {"mean": ("mean_in_wave", "mean_in_kernel"), "sampled": ("samples_in_wave", "samples_in_kernel")}
INFO = ("samples_in_wave", "mean_in_wave", "samples_in_kernel", "mean_in_kernel", "engine_last", "time_block_active",
        "wave_launches")


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_fields_in_wave_are_declared_and_bound(L):
    hdr = open(L.HEADER_PATH).read()
    assert '"samples_in_wave"' in hdr and '"mean_in_wave"' in hdr
    assert '"samples_in_kernel"' in hdr and '"mean_in_kernel"' in hdr
    assert "Which kernels take the snapshots" in hdr and "Which kernels take the sums" in hdr
    lib = L.load_library()
    built = open(L.LIB_PATH, "rb").read()             # (no context without a GPU: the keys' strings in the built library;
    assert '"wave_launches"' in hdr
    for key in (b"samples_in_wave", b"mean_in_wave", b"wave_launches"):   # the GPU tests below read them through lbm_get_info)
        assert key + b"\0" in built, key
        v = C.c_double(-1.0)
        assert lib.lbm_get_info(None, key, C.byref(v)) == LBM_EINVAL
        assert v.value == -1.0
    assert "samples_in_wave" in L.Lattice.run_sampled.__doc__
    assert "mean_in_wave" in L.Lattice.run_mean.__doc__


def test_the_left_over_steps_of_the_cases_hold_a_pair_that_starts_on_a_sample_step():
    """2 K + 5 steps: two passes, then the pairs (2 K + 1, 2 K + 2), (2 K + 3, 2 K + 4) and the single step 2 K + 5.  At
    every = 3 a pair's first step is a sample step at K = 4 (9) and K = 6 (15); at every = 1 at every K; at every = K + 1
    the first pass holds no sample step (it runs the plain kernel), the second holds step K + 1, and step 2 K + 2 is the
    second step of a left-over pair that further steps follow."""
    starts = {K: [s for s in (2 * K + 1, 2 * K + 3) if s % 3 == 0] for K, _ in KERNELS}
    assert starts[4] == [9] and starts[6] == [15] and starts[8] == []
    for K, _ in KERNELS:
        samples = [s for s in range(1, 2 * K + 6) if s % (K + 1) == 0]
        assert samples == [K + 1, 2 * K + 2] and not any(s <= K for s in samples) and K < K + 1 <= 2 * K


# ---------------------------------------------------------------------------------------------------------------- GPU
def _context(L, p, ob, cells, options=(), **kw):
    lat = L.Lattice(p, ob, cells, **kw)
    for k, v in options:
        lat.set_option(k, v)
    return lat


def _run(L, which, p, ob, cells, nsteps, every, options=(), **kw):
    with _context(L, p, ob, cells, options, **kw) as lat:
        av, out = (lat.run_mean if which == "mean" else lat.run_sampled)(nsteps, every)
        info = {k: int(lat.info(k)) for k in INFO}
        st = lat.read_state()
    return av, out, st, info


_REF, _PLAIN = {}, {}


def _reference(L, nx, ny, seed, extra=()):
    """The case and -- once per case -- the snapshots of the unchanged split path at every step of NMAX steps."""
    key = (nx, ny, seed, extra)
    if key not in _REF:
        p, ob, cells, _ = _random_case(L, nx, ny, seed)
        _, S1, _, info = _run(L, "sampled", p, ob, cells, NMAX, 1, SPLIT + extra)
        assert info["samples_in_wave"] == 0 and info["mean_in_wave"] == 0, info
        assert info["samples_in_kernel"] == 0 and info["mean_in_kernel"] == 0 and info["engine_last"] == 1, info
        assert S1.shape == (NMAX, ny, nx, 4) and not np.isnan(S1).any() and np.all(S1[..., 3] > 0)
        S1.setflags(write=False)
        _REF[key] = ((p, ob, cells), S1)
    return _REF[key]


def _lbm_run(L, key, p, ob, cells, nsteps, opts, **kw):
    k = (key, nsteps, opts, tuple(sorted(kw)))
    if k not in _PLAIN:
        _PLAIN[k] = _plain(L, p, ob, cells, nsteps, opts, **kw)
    return _PLAIN[k]


def _expected(which, S1, nsteps, every):
    snaps = S1[every - 1:nsteps:every][:nsteps // every]
    return mean_of(snaps) if which == "mean" else snaps


def _check(L, which, nx, ny, seed, K, cols, nsteps, every, rows=0, in_wave=1, extra=()):
    (p, ob, cells), S1 = _reference(L, nx, ny, seed, extra)
    opts = _opts(K, cols, rows) + extra
    av, out, st, info = _run(L, which, p, ob, cells, nsteps, every, opts)
    av0, st0 = _lbm_run(L, (nx, ny, seed), p, ob, cells, nsteps, opts)
    where = (which, nx, ny, K, cols, rows, nsteps, every, info)
    wave, tiles = KEYS[which]
    assert info[wave] == in_wave and info[tiles] == 0 and info["engine_last"] == 1 and info["time_block_active"] == K, where
    if in_wave:                                       # a fresh context: one lbm_wave kernel per pass, sample step or none
        assert info["wave_launches"] == nsteps // K, where
    want = _expected(which, S1, nsteps, every)
    assert out.shape == want.shape, where
    bad = np.argwhere(_bits(out) != _bits(want))
    assert len(bad) == 0, (where, len(bad), [tuple(int(v) for v in b) for b in bad[:8]])
    assert np.array_equal(_bits(st), _bits(st0)), where
    if in_wave:
        assert np.array_equal(_bits(av), _bits(av0)), where
    else:                                             # the split path, as before: lbm_run's to rounding
        assert np.allclose(av, av0, rtol=2e-6, atol=0), where


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["mean", "sampled"])
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_fields_are_the_bits_of_the_split_path(gpu, K, cols, which):
    """2 K + 5 steps: two passes, then two pairs and a single step.  every = 1: every level of every pass and every
    left-over step; 3: divides no K; K; K + 1: the first pass holds no sample and runs the plain kernel."""
    for nx, ny, seed, rows in SHAPES:
        for every in (1, 3, K, K + 1):
            _check(gpu, which, nx, ny, seed, K, cols, 2 * K + 5, every, rows=rows)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["mean", "sampled"])
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_fields_at_one_pass_and_below(gpu, K, cols, which):
    nx, ny, seed, rows = SHAPES[0]
    _check(gpu, which, nx, ny, seed, K, cols, K, 1, rows=rows)                        # one pass, no left-over step
    _check(gpu, which, nx, ny, seed, K, cols, K - 1, 1, rows=rows, in_wave=0)         # below one pass: the split path


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["mean", "sampled"])
def test_wave_fields_with_ieee_maths(gpu, which):
    """kernel_variant 0 (IEEE division and square root), one kernel per shape, against the split path under the same."""
    ieee = (("kernel_variant", 0),)
    for (nx, ny, seed, rows), (K, cols) in zip(SHAPES, ((8, 2), (6, 1))):
        for every in (1, 3):
            _check(gpu, which, nx, ny, seed, K, cols, 2 * K + 5, every, rows=rows, extra=ieee)


# torch and the library share libamdhip64: torch is imported FIRST, in a child process of its own
_DEVICE_OUTPUT = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_wave_fields import _bits, _context, _opts, _random_case
p, ob, cells, _ = _random_case(L, 256, 64, 11)
nsteps, every = 21, 3
for K, cols in ((6, 1), (8, 2)):
    for name, key, shape in (("run_mean", "mean_in_wave", (64, 256, 4)), ("run_sampled", "samples_in_wave", (7, 64, 256, 4))):
        with _context(L, p, ob, cells, _opts(K, cols, 24)) as lat:
            av_h, want = getattr(lat, name)(nsteps, every)
            assert lat.info(key) == 1
            st_h = lat.read_state()
        out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda:0")
        with _context(L, p, ob, cells, _opts(K, cols, 24)) as lat:
            av, got = getattr(lat, name)(nsteps, every, out=out)
            assert got is out and lat.info(key) == 1
            st = lat.read_state()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (K, cols, name)
        assert np.array_equal(_bits(av), _bits(av_h)) and np.array_equal(_bits(st), _bits(st_h))
print("device output ok")
"""


@pytest.mark.gpu
def test_device_output_is_the_host_output(gpu):
    assert "device output ok" in _child(_DEVICE_OUTPUT)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["mean", "sampled"])
@pytest.mark.parametrize("context", ["lbm_march", "two_slabs"])
def test_contexts_that_keep_the_split_path(gpu, context, which):
    L = gpu
    nx, ny, seed, _ = SHAPES[0]
    (p, ob, cells), S1 = _reference(L, nx, ny, seed)
    nsteps, every = 13, 3
    if context == "lbm_march":
        opts, kw = _opts(4, kernel=0), {}
    else:
        opts, kw = (("engine", 1), ("time_block", 8)), dict(nslabs=2, devices=[0, 0], exchange=L.EXCHANGE_COPY)
    av, out, st, info = _run(L, which, p, ob, cells, nsteps, every, opts, **kw)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts, **kw)
    assert info["samples_in_wave"] == 0 and info["mean_in_wave"] == 0 and info["engine_last"] == 1, info
    assert info["samples_in_kernel"] == 0 and info["mean_in_kernel"] == 0, info
    if context == "lbm_march":
        assert info["time_block_active"] == 4
    assert np.array_equal(_bits(out), _bits(_expected(which, S1, nsteps, every)))
    assert np.array_equal(_bits(st), _bits(st0))
    assert np.allclose(av, av0, rtol=2e-6, atol=0)


@pytest.mark.gpu
def test_one_context_through_mixed_calls(gpu):
    """run_mean, run, run_sampled, run_probes and run_mean again on one context, all where lbm_wave runs: after each call
    the lattice and av_vels are those of a twin that only calls run; the second mean is a fresh context's."""
    L = gpu
    nx, ny, seed, rows = SHAPES[0]
    (p, ob, cells), S1 = _reference(L, nx, ny, seed)
    opts = _opts(8, 2, rows)
    xy = probe_set(nx, ny, ob)
    with _context(L, p, ob, cells, opts) as lat, _context(L, p, ob, cells, opts) as twin:
        lat.set_probes(xy)

        def same(av):
            assert np.array_equal(_bits(av), _bits(twin.run(len(av))))
            assert np.array_equal(_bits(lat.read_state()), _bits(twin.read_state()))

        av, mean1 = lat.run_mean(19, 2)
        assert lat.info("mean_in_wave") == 1 and lat.info("mean_in_kernel") == 0
        same(av)
        assert np.array_equal(_bits(mean1), _bits(mean_of(S1[1:19:2])))
        same(lat.run(9))
        av, _ = lat.run_sampled(17, 5)
        assert lat.info("samples_in_wave") == 1 and lat.info("samples_in_kernel") == 0
        same(av)
        av, _ = lat.run_probes(10, 3)
        assert lat.info("probes_in_wave") == 1
        same(av)
        av, mean2 = lat.run_mean(21, 4)
        assert lat.info("mean_in_wave") == 1 and lat.info("engine_last") == 1
        same(av)
    with _context(L, p, ob, cells, opts) as fresh:
        fresh.run(55)
        _, m2 = fresh.run_mean(21, 4)
        assert fresh.info("mean_in_wave") == 1
    assert np.array_equal(_bits(mean2), _bits(m2))
    with _context(L, p, ob, cells, SPLIT) as fresh:
        fresh.run(55)
        _, fields = fresh.run_sampled(21, 4)
    assert np.array_equal(_bits(mean2), _bits(mean_of(fields)))


@pytest.mark.gpu
def test_every_call_in_wave_launches_one_kernel_per_pass(gpu):
    """One context: lbm_run, a mean at every step, a mean at every tenth, snapshots and probes each add nsteps // K to
    "wave_launches" -- the field, probe and plain flavours alike, one kernel per pass."""
    L = gpu
    nx, ny, seed, rows = SHAPES[0]
    (p, ob, cells), _ = _reference(L, nx, ny, seed)
    for K, cols in KERNELS:
        with _context(L, p, ob, cells, _opts(K, cols, rows)) as lat:
            lat.set_probes(probe_set(nx, ny, ob))
            assert lat.info("wave_launches") == 0
            n, seen = 3 * K + 1, 0
            for call in (lambda: lat.run(n), lambda: lat.run_mean(n, 1), lambda: lat.run_mean(n, 10), lambda: lat.run_sampled(n, 2),
                         lambda: lat.run_sampled(n, n), lambda: lat.run_probes(n, 1)):
                call()
                seen += n // K
                assert lat.info("wave_launches") == seen, (K, cols, seen)
            assert lat.info("mean_in_wave") == 1 and lat.info("samples_in_wave") == 1 and lat.info("probes_in_wave") == 1


@pytest.mark.gpu
def test_a_lone_mean_or_snapshot_series_through_run_observed_rides_in_wave(gpu):
    """lbm_run_observed hands a lone observer to its own call: a lone mean, or a lone snapshot series, on a wave context
    takes the new path there -- one piece, the key of its call 1, nothing taken by the observed flavours, the bits of the
    single call."""
    L = gpu
    nx, ny, seed, rows = SHAPES[0]
    (p, ob, cells), S1 = _reference(L, nx, ny, seed)
    K, nsteps, every = 8, 21, 3
    for which, arg, res, key in (("mean", "mean_every", "mean", "mean_in_wave"), ("sampled", "fields_every", "fields", "samples_in_wave")):
        with _context(L, p, ob, cells, _opts(K, 2, rows)) as lat:
            got = lat.run_observed(nsteps, **{arg: every})
            assert lat.info(key) == 1 and lat.info("observed_pieces") == 1, which
            assert lat.info("observed_in_wave") == 0 and lat.info("observed_in_kernel") == 0, which
            assert lat.info("wave_launches") == nsteps // K, which
            st = lat.read_state()
        av0, st0 = _lbm_run(L, (nx, ny, seed), p, ob, cells, nsteps, _opts(K, 2, rows))
        assert np.array_equal(_bits(got[res]), _bits(_expected(which, S1, nsteps, every))), which
        assert np.array_equal(_bits(got["av_vels"]), _bits(av0)) and np.array_equal(_bits(st), _bits(st0)), which


@pytest.mark.gpu
def test_refusals_leave_the_lattice_alone(gpu):
    L = gpu
    lib = L.load_library()
    nx, ny, seed, rows = SHAPES[0]
    (p, ob, cells), _ = _reference(L, nx, ny, seed)
    opts = _opts(8, 1, rows)
    out = np.zeros((2, ny, nx, 4), np.float32)
    with _context(L, p, ob, cells, opts) as lat, _context(L, p, ob, cells, opts) as twin:
        lat.run(3)
        twin.run(3)
        st = lat.read_state()
        assert lib.lbm_run_mean(lat._ctx, 20, None, 0, out.ctypes.data) == LBM_EINVAL           # every = 0
        assert lib.lbm_run_mean(lat._ctx, 20, None, -1, out.ctypes.data) == LBM_EINVAL          # every < 0
        assert lib.lbm_run_mean(lat._ctx, 20, None, 21, out.ctypes.data) == LBM_EINVAL          # m = 0: nothing to average
        assert lib.lbm_run_mean(lat._ctx, 20, None, 5, None) == LBM_EINVAL                      # no output
        assert lib.lbm_run_sampled(lat._ctx, 20, None, -1, out.ctypes.data) == LBM_EINVAL       # every < 0
        assert lib.lbm_run_sampled(lat._ctx, 20, None, 10, None) == LBM_EINVAL                  # no output, two snapshots due
        assert not out.any()
        assert np.array_equal(_bits(lat.read_state()), _bits(st))
        assert lat.info("mean_in_wave") == 0 and lat.info("samples_in_wave") == 0
        av, _ = lat.run_mean(20, 5)
        assert lat.info("mean_in_wave") == 1
        assert np.array_equal(_bits(av), _bits(twin.run(20)))
        assert np.array_equal(_bits(lat.read_state()), _bits(twin.read_state()))


@pytest.mark.gpu
def test_wave_mean_against_the_float_oracle(gpu, O, oracle):
    """Independent of the split path: the 64 x 40 known-answer lattice, K = 4 in lbm_wave, 10 steps (two passes and a pair),
    every step a sample, inside the bound of tests/test_mean_run.py (_oracle_mean_bound)."""
    L = gpu
    k, p, ob, op = _kat_case(L, O)
    want, bound, _, ref = _oracle_mean_bound(k, p, ob, op, oracle)
    assert np.array_equal(ref, k["cells_after_10"])
    av, mean, st, info = _run(L, "mean", p, ob, k["cells0"], 10, 1, _opts(4))
    assert info["mean_in_wave"] == 1 and info["mean_in_kernel"] == 0 and info["engine_last"] == 1, info
    assert info["time_block_active"] == 4
    assert np.all(np.abs(st - ref) <= 2e-5 * np.abs(ref))
    err, lim = _within(mean, want, bound)
    print("wave mean against the oracle: max error %.3g, worst error - bound %.3g" % (err.max(), np.max(err - lim)))
    assert np.all(err <= lim), float(np.max(err - lim))
