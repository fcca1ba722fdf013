"""lbm_run_probes where lbm_wave runs (a lattice alone, time_block 4 / 6 / 8): the probes ride in lbm_wave's launches.

Contract (include/lbm_mi355x.h): at a sample level of a pass the probe flavour of lbm_wave evaluates derive_cell on the
populations a probe's cell holds after collide_cell and before accelerate_cell -- the values the stored lattice of that step
would hold at the end of a run -- and stores them into the probe's place.  So the probes are the BITS of the split path
(engine 1, time_block 1: pieces of `every` steps, lbm_probe_gather behind each), which are lbm_run_sampled's values in those
cells; av_vels and the lattice are the bits of lbm_run under the same options; info "probes_in_wave" reads 1
("probes_in_kernel" keeps meaning the register tiles: 0 here).  lbm_run_observed with forces and probes rides in the
force-and-probe flavour, in one piece.  Contexts where lbm_march runs, slabs with neighbours and runs shorter than K keep
the split path.

Shapes: 256 x 64 (several wave columns, two blocks; with wave_rows 24 chunks of 24, 24 and 16 rows) and 200 x 72 (a width
that is no multiple of 64 - 2 K, nor of 64).  One probe set per shape serves every kernel: it holds the strip edges of all
four.  The probes of step s depend on the lattice after step s alone, so the split path runs once per case, at every = 1
over the longest run (21 steps), and a run at another period is compared with its rows every - 1, 2 every - 1, ..."""
import ctypes as C

import numpy as np
import pytest

from test_body_forces import _bits, _plain, _random_case
from test_mean_run import _child
from test_probe_run import _pick, awkward_set

LBM_EINVAL = 1
NMAX = 21                     # 2 K + 5 at K = 8
INFO = ("probes_in_wave", "probes_in_kernel", "engine_last", "time_block_active")
SPLIT = (("engine", 1), ("time_block", 1))
KERNELS = [(4, 1), (6, 1), (8, 1), (8, 2)]
STRIPS = (56, 52, 48, 112)    # columns a wave delivers: 64 - 2 K at K = 4, 6, 8; 128 - 16 with two columns per lane


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_probes_in_wave_is_declared_and_bound(L):
    hdr = open(L.HEADER_PATH).read()
    assert '"probes_in_wave"' in hdr and '"observed_in_wave"' in hdr and '"probes_in_kernel"' in hdr
    # the rewritten comments of lbm_run_probes and lbm_run_observed
    assert "Which kernels take the probes" in hdr and "the probes ride in its launches" in hdr
    assert "the probes are the bits of the split path" in hdr
    assert "forces and probes ride together in its launches" in hdr
    lib = L.load_library()
    built = open(L.LIB_PATH, "rb").read()             # (no context without a GPU: the keys' strings in the built library;
    for key in (b"probes_in_wave", b"observed_in_wave"):     # the GPU tests below read both through lbm_get_info)
        assert key + b"\0" in built, key
        v = C.c_double(-1.0)
        assert lib.lbm_get_info(None, key, C.byref(v)) == LBM_EINVAL
        assert v.value == -1.0
    assert "probes_in_wave" in L.Lattice.run_probes.__doc__
    assert "observed_in_wave" in L.Lattice.run_observed.__doc__


def probe_set(nx, ny, ob):
    """awkward_set's corners, rows 0 / ny - 2 / ny - 1, blocked-and-fluid pair and several probes per row, with the chunk
    edges of 24-row chunks (rows 23, 24, 47, 48); the strip edges VW - 1, VW of every kernel in a chunk-edge row, the
    accelerate row and an interior row; both cells of a lane's pair at two columns per lane; a second blocked cell with the
    fluid cell beside it; shuffled."""
    ob = np.asarray(ob).reshape(ny, nx)
    cells = {tuple(int(v) for v in q) for q in awkward_set(nx, ny, ob, 0, 1, extra_rows=(23, 24, 47, 48))}
    for vw in STRIPS:
        for ii in (vw - 1, vw):
            for jj in (5, 23, 24, ny - 2):
                cells.add((ii, jj))
    for jj in (30, ny - 2):
        cells |= {(130, jj), (131, jj)}                          # columns 2 i, 2 i + 1: one lane's pair
    pair = np.argwhere((ob[:, :-1] == 0) & (ob[:, 1:] != 0))     # fluid, then blocked
    jj, ii = (int(v) for v in pair[len(pair) // 3])
    cells |= {(ii, jj), (ii + 1, jj)}
    xy = np.array(sorted(cells), dtype=np.int32)
    xy = xy[np.random.default_rng(5).permutation(len(xy))]
    rows = set(xy[:, 1].tolist())
    assert {0, 23, 24, 47, 48, ny - 2, ny - 1} <= rows
    assert np.any((xy[:, 1] == ny - 2) & (ob[xy[:, 1], xy[:, 0]] == 0))            # a fluid probe in the accelerate row
    assert np.any(ob[xy[:, 1], xy[:, 0]] != 0) and max(np.bincount(xy[:, 1])) >= 3
    assert np.any(np.diff(xy[:, 0]) < 0) and np.any(np.diff(xy[:, 1]) < 0)
    return xy


# ---------------------------------------------------------------------------------------------------------------- GPU
def _opts(K, cols=1, rows=0, kernel=1):
    o = [("engine", 1), ("march_kernel", kernel), ("time_block", K), ("wave_cols", cols)]
    if rows:
        o.append(("wave_rows", rows))                 # (after time_block, which forgets the chunk height)
    return tuple(o)


def _context(L, p, ob, cells, options=(), xy=None, body=None, **kw):
    lat = L.Lattice(p, ob, cells, **kw)
    for k, v in options:
        lat.set_option(k, v)
    if xy is not None:
        lat.set_probes(xy)
    if body is not None:
        lat.set_bodies(body, 4)
    return lat


def _run(L, p, ob, cells, xy, nsteps, every, options=(), **kw):
    with _context(L, p, ob, cells, options, xy, **kw) as lat:
        av, pr = lat.run_probes(nsteps, every)
        info = {k: int(lat.info(k)) for k in INFO}
        st = lat.read_state()
    return av, pr, st, info


_REF, _PLAIN = {}, {}


def _reference(L, nx, ny, seed):
    """The case with its probe set and -- once per case -- the probes of the split path at every step of NMAX steps."""
    key = (nx, ny, seed)
    if key not in _REF:
        p, ob, cells, body = _random_case(L, nx, ny, seed)
        xy = probe_set(nx, ny, ob)
        _, P1, _, info = _run(L, p, ob, cells, xy, NMAX, 1, SPLIT)
        assert info["probes_in_wave"] == 0 and info["probes_in_kernel"] == 0 and info["engine_last"] == 1
        assert not np.isnan(P1).any() and np.all(P1[:, :, 3] > 0)
        for a in (xy, P1, body):
            a.setflags(write=False)
        _REF[key] = ((p, ob, cells, body), xy, P1)
    return _REF[key]


def _lbm_run(L, key, p, ob, cells, nsteps, opts, **kw):
    k = (key, nsteps, opts, tuple(sorted(kw)))
    if k not in _PLAIN:
        _PLAIN[k] = _plain(L, p, ob, cells, nsteps, opts, **kw)
    return _PLAIN[k]


def _check(L, nx, ny, seed, K, cols, nsteps, every, rows=0, in_wave=1):
    (p, ob, cells, _), xy, P1 = _reference(L, nx, ny, seed)
    opts = _opts(K, cols, rows)
    av, pr, st, info = _run(L, p, ob, cells, xy, nsteps, every, opts)
    av0, st0 = _lbm_run(L, (nx, ny, seed), p, ob, cells, nsteps, opts)
    where = (nx, ny, K, cols, rows, nsteps, every, info)
    assert info == dict(probes_in_wave=in_wave, probes_in_kernel=0, engine_last=1, time_block_active=K), where
    want = P1[every - 1:nsteps:every][:nsteps // every]
    assert pr.shape == want.shape == (nsteps // every, len(xy), 4), where
    bad = np.argwhere(_bits(pr) != _bits(want))
    assert len(bad) == 0, (where, len(bad), [(int(j), tuple(xy[i]), int(k)) for j, i, k in bad[:8]])
    assert np.array_equal(_bits(st), _bits(st0)), where
    if in_wave:
        assert np.array_equal(_bits(av), _bits(av0)), where
    else:                                             # the split path, as before: lbm_run's to rounding
        assert np.allclose(av, av0, rtol=2e-6, atol=0), where


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_probes_are_the_bits_of_the_split_path(gpu, K, cols):
    """2 K + 5 steps: two passes, then two pairs and a single step.  every = 1: every level samples, every left-over pair
    starts on a sample step; 3 and K; K + 3: the second pass holds no sample."""
    for every in (1, 3, K, K + 3):
        _check(gpu, 256, 64, 11, K, cols, 2 * K + 5, every)


@pytest.mark.gpu
def test_the_split_path_reference_is_run_sampled_in_those_cells(gpu):
    L = gpu
    (p, ob, cells, _), xy, P1 = _reference(L, 256, 64, 11)
    with _context(L, p, ob, cells, SPLIT) as lat:
        _, fields = lat.run_sampled(NMAX, 1)
    assert np.array_equal(_bits(P1), _bits(_pick(fields, xy)))


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_probes_with_ragged_chunks(gpu, K, cols):
    """256 x 64 in chunks of 24, 24 and 16 rows: probes in rows 23, 24, 47, 48."""
    for every in (1, 3, K, K + 3):
        _check(gpu, 256, 64, 11, K, cols, 2 * K + 5, every, rows=24)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [4, 6, 8])
def test_wave_probes_with_a_partial_wave_column(gpu, K):
    """200 x 72, one column per lane: 200 is no multiple of 64 - 2 K, nor of 64."""
    for every in (1, 3, K, K + 3):
        _check(gpu, 200, 72, 12, K, 1, 2 * K + 5, every)


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_wave_probes_at_group_boundaries(gpu, K, cols):
    _check(gpu, 256, 64, 11, K, cols, K, 1)                       # no left-over step
    _check(gpu, 256, 64, 11, K, cols, 2 * K, 3)
    _check(gpu, 256, 64, 11, K, cols, K - 1, 1, in_wave=0)        # below one group: the split path
    _check(gpu, 256, 64, 11, K, cols, 2 * K + 5, 2 * K + 5)       # the only sample is the last left-over step
    # every = 2: the samples of the left-over steps are the SECOND steps of their pairs, the first of which is followed by
    # further steps (the pair is stored without the next accelerate phase, gathered, then accelerated); pairs that START on a
    # sample step: every = 1 and 3 above (steps 2 K + 1, 2 K + 3; 9 at K = 4, 15 at K = 6)
    _check(gpu, 256, 64, 11, K, cols, 2 * K + 5, 2)


# torch and the library share libamdhip64: torch is imported FIRST, in a child process of its own
_DEVICE_OUTPUT = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_wave_probes import _bits, _context, _opts, _random_case, probe_set
p, ob, cells, _ = _random_case(L, 256, 64, 11)
xy = probe_set(256, 64, ob)
nsteps, every = 21, 3
for K, cols in ((6, 1), (8, 2)):
    with _context(L, p, ob, cells, _opts(K, cols), xy) as lat:
        av_h, want = lat.run_probes(nsteps, every)
        assert lat.info("probes_in_wave") == 1
        st_h = lat.read_state()
    out = torch.full((nsteps // every, len(xy), 4), float("nan"), dtype=torch.float32, device="cuda:0")
    with _context(L, p, ob, cells, _opts(K, cols), xy) as lat:
        av, got = lat.run_probes(nsteps, every, out=out)
        assert got is out and lat.info("probes_in_wave") == 1
        st = lat.read_state()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(av), _bits(av_h)) and np.array_equal(_bits(st), _bits(st_h))
print("device output ok")
"""


@pytest.mark.gpu
def test_device_output_is_the_host_output(gpu):
    assert "device output ok" in _child(_DEVICE_OUTPUT)


@pytest.mark.gpu
def test_wave_probe_maps_follow_a_new_set_and_no_set_is_refused(gpu):
    L = gpu
    lib = L.load_library()
    (p, ob, cells, _), xy, _ = _reference(L, 256, 64, 11)
    some = [(int(i), int(j)) for i, j in xy[::3]]    # a third of the set, other cells beside them, another order
    other = np.array(some + [q for q in ((7, 9), (200, 33), (111, 61), (49, 40)) if q not in some], dtype=np.int32)[::-1]
    K = 8

    def sequence(options):
        with _context(L, p, ob, cells, options, xy) as lat:
            _, Pa = lat.run_probes(2 * K, 1)
            wa = int(lat.info("probes_in_wave"))
            lat.set_probes(other)
            _, Pb = lat.run_probes(2 * K + 1, 2)
            wb = int(lat.info("probes_in_wave"))
            st = lat.read_state()
            lat.set_probes(None)
            out = np.zeros((8, len(other), 4), dtype=np.float32)
            assert lib.lbm_run_probes(lat._ctx, 8, None, 1, out.ctypes.data) == LBM_EINVAL
            assert not out.any() and np.array_equal(_bits(lat.read_state()), _bits(st))
            return Pa, Pb, wa, wb, st

    Pa, Pb, wa, wb, st = sequence(_opts(K))
    Pa1, Pb1, wa1, wb1, st1 = sequence(SPLIT)
    assert (wa, wb, wa1, wb1) == (1, 1, 0, 0)
    assert np.array_equal(_bits(Pa), _bits(Pa1)) and np.array_equal(_bits(Pb), _bits(Pb1))
    assert Pb.shape == (K, len(other), 4)
    assert np.array_equal(_bits(st), _bits(st1))


OBS = ("observed_in_wave", "observed_in_kernel", "observed_pieces", "forces_in_wave")


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_observed_forces_and_probes_ride_together(gpu, K, cols):
    L = gpu
    (p, ob, cells, body), xy, P1 = _reference(L, 256, 64, 11)
    opts, nsteps, every = _opts(K, cols), 2 * K + 5, 3
    with _context(L, p, ob, cells, opts, xy, body) as lat:
        res = lat.run_observed(nsteps, forces=True, probes_every=every)
        info = {k: int(lat.info(k)) for k in OBS}
        st = lat.read_state()
    assert info == dict(observed_in_wave=3, observed_in_kernel=0, observed_pieces=1, forces_in_wave=1), (K, cols, info)
    with _context(L, p, ob, cells, opts, xy, body) as lat:
        _, F = lat.run_forces(nsteps)
        assert lat.info("forces_in_wave") == 1
        st_f = lat.read_state()
    with _context(L, p, ob, cells, opts, xy, body) as lat:
        _, P = lat.run_probes(nsteps, every)
        assert lat.info("probes_in_wave") == 1
    av0, st0 = _lbm_run(L, (256, 64, 11), p, ob, cells, nsteps, opts)
    assert np.array_equal(_bits(res["forces"]), _bits(F)) and np.abs(F).max() > 0
    assert np.array_equal(_bits(res["probes"]), _bits(P))
    assert np.array_equal(_bits(P), _bits(P1[every - 1:nsteps:every]))
    assert np.array_equal(_bits(st), _bits(st_f)) and np.array_equal(_bits(st), _bits(st0))
    assert np.array_equal(_bits(res["av_vels"]), _bits(av0))


@pytest.mark.gpu
def test_observed_probes_keep_their_phase_across_the_pieces_means_cut(gpu):
    """Forces, probes every 3 and mean_every = 10 over 25 steps at K = 8: pieces of 10, 10 and 5 steps (one pass and two
    left-over steps, twice; then a piece below one pass); the probes' samples 12 and 21 are the second and the first step
    of a piece."""
    L = gpu
    (p, ob, cells, body), xy, P1 = _reference(L, 256, 64, 11)
    opts = _opts(8)
    with _context(L, p, ob, cells, opts, xy, body) as lat:
        res = lat.run_observed(25, forces=True, probes_every=3, mean_every=10)
        info = {k: int(lat.info(k)) for k in OBS}
        st = lat.read_state()
    assert info == dict(observed_in_wave=3, observed_in_kernel=0, observed_pieces=3, forces_in_wave=1), info
    with _context(L, p, ob, cells, opts, xy, body) as lat:
        _, F = lat.run_forces(25)
        st_f = lat.read_state()
    with _context(L, p, ob, cells, opts, xy, body) as lat:
        _, P = lat.run_probes(25, 3)
        assert lat.info("probes_in_wave") == 1
    with _context(L, p, ob, cells, opts, xy, body) as lat:
        _, mean = lat.run_mean(25, 10)
    assert np.array_equal(_bits(res["forces"]), _bits(F))
    assert np.array_equal(_bits(res["probes"]), _bits(P))
    assert np.array_equal(_bits(P[:NMAX // 3]), _bits(P1[2:NMAX:3]))
    assert np.array_equal(_bits(res["mean"]), _bits(mean))
    assert np.array_equal(_bits(st), _bits(st_f))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lbm_march", "two_slabs"])
def test_contexts_that_keep_the_split_path(gpu, which):
    L = gpu
    (p, ob, cells, _), xy, P1 = _reference(L, 256, 64, 11)
    nsteps, every = 13, 3
    if which == "lbm_march":
        opts, kw = _opts(4, kernel=0), {}
    else:
        opts, kw = (("engine", 1), ("time_block", 8)), dict(nslabs=2, devices=[0, 0], exchange=L.EXCHANGE_COPY)
    av, pr, st, info = _run(L, p, ob, cells, xy, nsteps, every, opts, **kw)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts, **kw)
    assert info["probes_in_wave"] == 0 and info["probes_in_kernel"] == 0 and info["engine_last"] == 1, info
    if which == "lbm_march":
        assert info["time_block_active"] == 4
    assert np.array_equal(_bits(pr), _bits(P1[every - 1:nsteps:every]))
    assert np.array_equal(_bits(st), _bits(st0))
    assert np.allclose(av, av0, rtol=2e-6, atol=0)
