"""lbm_run_forces where lbm_wave runs (a lattice alone, time_block 4 / 6 / 8): the forces ride in lbm_wave's launches.

Contract (include/lbm_mi355x.h): the force flavour of lbm_wave evaluates body_force_cell on the populations a counted cell
holds after collide_cell at every level of a pass -- the values the stored lattice of that step would hold -- and a fold
kernel adds them up in lbm_body_forces's order.  So the forces are the BITS of the one-step path (time_block 1), av_vels and
the lattice are the bits of lbm_run under the same options, and info "forces_in_wave" reads 1 ("forces_in_kernel" keeps
meaning the register tiles: 0 here).  Contexts where lbm_march runs, slabs with neighbours and runs shorter than K keep the
one-step path.

Shapes: 256 x 64 (where tests/test_param_space.py reaches these kernels: several wave columns, two blocks), chunks of 24, 24
and 16 rows, and 200 x 72 (a width that is no multiple of 64: the last wave column delivers 8 of its 48 columns at K = 8).
_random_case puts counted cells on strip edges, chunk edges, rows 0 and ny - 1 and the accelerate row.  The per-step
reference and the one-step forces of a case are computed once for the longest run (21 steps) and sliced: the forces of step
t depend on the lattice after step t alone."""
import ctypes as C

import numpy as np
import pytest

from test_body_forces import _bits, _close, _forces, _per_step, _plain, _random_case

LBM_EINVAL = 1
NMAX = 21                     # 2 K + 5 at K = 8
INFO = ("forces_in_wave", "forces_in_kernel", "engine_last", "time_block_active")


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_forces_in_wave_is_declared_and_bound(L):
    hdr = open(L.HEADER_PATH).read()
    assert '"forces_in_wave"' in hdr and '"forces_in_kernel"' in hdr
    # the rewritten lbm_run_forces comment
    assert "Where lbm_wave runs" in hdr and "the forces ride in its launches" in hdr
    assert "av_vels is lbm_run's, bit for bit" in hdr
    assert "the forces are the bits of the one-step path" in hdr
    lib = L.load_library()
    v = C.c_double(-1.0)
    assert lib.lbm_get_info(None, b"forces_in_wave", C.byref(v)) == LBM_EINVAL
    assert v.value == -1.0
    assert "forces_in_wave" in L.Lattice.run_forces.__doc__


# ---------------------------------------------------------------------------------------------------------------- GPU
def _opts(K, cols=1, rows=0, kernel=1):
    o = [("engine", 1), ("march_kernel", kernel), ("time_block", K), ("wave_cols", cols)]
    if rows:
        o.append(("wave_rows", rows))                 # (after time_block, which forgets the chunk height)
    return tuple(o)


def _run(L, p, ob, cells, body, nb, nsteps, options=(), **kw):
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        lat.set_bodies(body, nb)
        av, F = lat.run_forces(nsteps)
        info = {k: int(lat.info(k)) for k in INFO}
        st = lat.read_state()
    return av, F, st, info


_REF = {}


def _reference(L, nx, ny, seed, labelling="random"):
    """The case, and -- once per case -- its per-step reference in float64 with the rounding scale, and the forces and
    av_vels of the one-step path (engine 1, time_block 1), all for NMAX steps."""
    key = (nx, ny, seed, labelling)
    if key not in _REF:
        p, ob, cells, body = _random_case(L, nx, ny, seed)
        if labelling == "one_chunk":                  # counted cells in rows 26 .. 45 only: the middle chunk of 24-row chunks
            rows = np.arange(ny)[:, None]
            body = np.where((rows >= 26) & (rows < 46), body, 0).astype(np.int32)
        elif labelling == "fluid_only":               # labels on fluid cells only: nothing is counted
            rng = np.random.default_rng(seed + 1)
            body = np.where(ob == 0, rng.integers(1, 5, size=ob.shape), 0).astype(np.int32)
        want, scale, _, _ = _per_step(L, p, ob, cells, body, 4, NMAX)
        av1, F1, _, info = _forces(L, p, ob, cells, body, 4, NMAX, (("engine", 1), ("time_block", 1)))
        assert info["engine_last"] == 1 and info["forces_in_kernel"] == 0
        for a in (want, scale, av1, F1):
            a.setflags(write=False)
        _REF[key] = ((p, ob, cells, body), want, scale, av1, F1)
    return _REF[key]


def _check(L, nx, ny, seed, K, cols, nsteps, rows=0, labelling="random", in_wave=1):
    (p, ob, cells, body), want, scale, av1, F1 = _reference(L, nx, ny, seed, labelling)
    opts = _opts(K, cols, rows)
    av, F, st, info = _run(L, p, ob, cells, body, 4, nsteps, opts)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts)
    where = (nx, ny, K, cols, rows, nsteps, labelling, info)
    assert info == dict(forces_in_wave=in_wave, forces_in_kernel=0, engine_last=1, time_block_active=K), where
    assert F.shape == (nsteps, 4, 2)
    assert np.array_equal(_bits(F), _bits(F1[:nsteps])), (where, np.abs(F - F1[:nsteps]).max())
    assert np.array_equal(_bits(st), _bits(st0)), where
    if in_wave:
        assert np.array_equal(_bits(av), _bits(av0)), where
    else:                                             # the one-step path, as before: its own av_vels, lbm_run's to rounding
        assert np.array_equal(_bits(av), _bits(av1[:nsteps])), where
        assert np.allclose(av, av0, rtol=2e-6, atol=0), where
    assert _close(F, want[:nsteps], scale[:nsteps]), (where, np.abs(F - want[:nsteps]).max())
    return F


KERNELS = [(4, 1), (6, 1), (8, 1), (8, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_forces_are_the_bits_of_the_one_step_path(gpu, K, cols):
    F = _check(gpu, 256, 64, 11, K, cols, 2 * K + 5)
    assert np.all(np.abs(F).max(axis=(0, 2)) > 0)     # every body feels something


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_forces_with_ragged_chunks(gpu, K, cols):
    """256 x 64 in chunks of 24, 24 and 16 rows."""
    _check(gpu, 256, 64, 11, K, cols, 2 * K + 5, rows=24)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [4, 6, 8])
def test_wave_forces_with_a_partial_wave_column(gpu, K):
    """200 x 72, one column per lane: 200 is no multiple of 64 - 2 K, nor of 64."""
    _check(gpu, 200, 72, 12, K, 1, 2 * K + 5)


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", [(4, 1), (8, 2)])
def test_wave_forces_without_leftover_steps_and_below_one_group(gpu, K, cols):
    _check(gpu, 256, 64, 11, K, cols, K)
    _check(gpu, 256, 64, 11, K, cols, 2 * K)
    _check(gpu, 256, 64, 11, K, cols, K - 1, in_wave=0)


@pytest.mark.gpu
def test_wave_forces_with_counted_cells_in_one_chunk_and_with_none(gpu):
    F = _check(gpu, 256, 64, 11, 8, 1, 21, rows=24, labelling="one_chunk")
    assert np.abs(F).max() > 0
    (p, ob, cells, body), _, _, _, _ = _reference(gpu, 256, 64, 11, "fluid_only")
    opts = _opts(6)
    av, F, st, info = _run(gpu, p, ob, cells, body, 4, 17, opts)
    av0, st0 = _plain(gpu, p, ob, cells, 17, opts)
    assert info["forces_in_kernel"] == 0 and info["engine_last"] == 1
    assert np.array_equal(_bits(F), np.zeros(F.shape, np.uint32))
    assert np.array_equal(_bits(av), _bits(av0)) and np.array_equal(_bits(st), _bits(st0))


@pytest.mark.gpu
def test_wave_force_maps_follow_a_new_labelling(gpu):
    L = gpu
    (p, ob, cells, body), _, _, _, _ = _reference(L, 256, 64, 11)
    other = np.where(body != 0, 5 - body, 0).astype(np.int32)
    other[:, :100] = 0                                # fewer counted cells, other labels
    K = 8

    def sequence(options):
        with L.Lattice(p, ob, cells) as lat:
            for k, v in options:
                lat.set_option(k, v)
            lat.set_bodies(body, 4)
            _, Fa = lat.run_forces(2 * K)
            wa = int(lat.info("forces_in_wave"))
            lat.set_bodies(other, 4)
            _, Fb = lat.run_forces(2 * K + 1)
            wb = int(lat.info("forces_in_wave"))
            return Fa, Fb, wa, wb, lat.read_state()

    Fa, Fb, wa, wb, st = sequence(_opts(K))
    Fa1, Fb1, wa1, wb1, st1 = sequence((("engine", 1), ("time_block", 1)))
    assert (wa, wb, wa1, wb1) == (1, 1, 0, 0)
    assert np.array_equal(_bits(Fa), _bits(Fa1)) and np.array_equal(_bits(Fb), _bits(Fb1))
    assert np.all(np.abs(Fb).max(axis=(0, 2)) > 0)    # (the second labelling counts cells of every body)
    assert np.array_equal(_bits(st), _bits(st1))


@pytest.mark.gpu
def test_wave_forces_refuse_a_run_without_bodies(gpu):
    L = gpu
    lib = L.load_library()
    (p, ob, cells, body), _, _, _, _ = _reference(L, 256, 64, 11)
    out = np.zeros((8, 4, 2), dtype=np.float32)
    with L.Lattice(p, ob, cells) as lat:
        for k, v in _opts(8):
            lat.set_option(k, v)
        lat.set_bodies(body, 4)
        lat.run_forces(8)
        assert lat.info("forces_in_wave") == 1
        lat.set_bodies(None, 0)
        st0 = lat.read_state()
        assert lib.lbm_run_forces(lat._ctx, 8, None, out.ctypes.data) == LBM_EINVAL
        assert np.array_equal(_bits(lat.read_state()), _bits(st0))


@pytest.mark.gpu
def test_observed_forces_and_means_agree_with_the_single_calls_on_the_wave_path(gpu):
    """Forces with mean_every = 10 over 25 steps at K = 8: pieces of 10, 10 and 5 steps -- one lbm_wave group and two
    left-over steps each, then a piece below one group -- against lbm_run_forces's three groups and one step."""
    L = gpu
    (p, ob, cells, body), want, scale, _, F1 = _reference(L, 256, 64, 11)
    opts = _opts(8)

    def context():
        lat = L.Lattice(p, ob, cells)
        for k, v in opts:
            lat.set_option(k, v)
        lat.set_bodies(body, 4)
        return lat

    with context() as lat:
        res = lat.run_observed(25, forces=True, mean_every=10)
        st = lat.read_state()
    with context() as lat:
        _, F = lat.run_forces(25)
        assert lat.info("forces_in_wave") == 1
        st_f = lat.read_state()
    with context() as lat:
        _, mean = lat.run_mean(25, 10)
    assert np.array_equal(_bits(res["forces"]), _bits(F))
    assert np.array_equal(_bits(F[:NMAX]), _bits(F1))
    assert np.array_equal(_bits(res["mean"]), _bits(mean))
    assert np.array_equal(_bits(st), _bits(st_f))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lbm_march", "two_slabs"])
def test_contexts_that_keep_the_one_step_path(gpu, which):
    L = gpu
    (p, ob, cells, body), want, scale, _, _ = _reference(L, 256, 64, 11)
    nsteps = 13
    if which == "lbm_march":
        opts, kw = _opts(4, kernel=0), {}
    else:
        opts, kw = (("engine", 1), ("time_block", 8)), dict(nslabs=2, devices=[0, 0], exchange=L.EXCHANGE_COPY)
    av, F, st, info = _run(L, p, ob, cells, body, 4, nsteps, opts, **kw)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts, **kw)
    assert info["forces_in_wave"] == 0 and info["forces_in_kernel"] == 0 and info["engine_last"] == 1, info
    if which == "lbm_march":
        assert info["time_block_active"] == 4
    assert _close(F, want[:nsteps], scale[:nsteps])
    assert np.array_equal(_bits(st), _bits(st0))
    assert np.allclose(av, av0, rtol=2e-6, atol=0)
