"""lbm_run_driven_observed where lbm_wave runs (a lattice alone, time_block 4 / 6 / 8): forces and probes ride in
lbm_wave's launches beside the K pairs of a pass.

Contract (include/lbm_mi355x.h): one flavour of lbm_wave takes forces, probes and the schedule; an observer that is not
wanted marks nothing in its map.  Forces and probes cut no piece (info "driven_observed_in_wave" = 3,
"driven_observed_pieces" = 1, "wave_launches" grows by one kernel per pass: nsteps // K, which is 2 over 2 K + 5 steps at
K = 6 and 8 and 3 at K = 4); means and snapshots cut pieces at their sample steps and are taken behind them, and a piece
shorter than K goes through the one-step kernel.  Forces are the BITS of `set_accel(accel[t]); run_forces(1)` under engine 1,
time_block 1; probes, snapshots and means the bits of their definitions on that loop's fields; the lattice the loop's.

Shapes, kernels and spikes are those of tests/test_wave_driven.py; the reference is test_driven_observed.observed_loop."""
import numpy as np
import pytest

from test_body_forces import _random_case as _random_case_with_bodies
from test_driven_observed import KEYS, _bits, check, observed, observed_loop, pieces_of, reference
from test_driven_run import schedules
from test_probe_run import awkward_set
from test_wave_driven import KERNELS, SHAPES, _spikes
from test_wave_probes import _opts

NONE = dict(forces=False, probes_every=0, mean_every=0, fields_every=0)
BOTH = dict(NONE, forces=True, probes_every=1)


def _case(L, nx, ny, seed, rows):
    p, ob, cells, body = _random_case_with_bodies(L, nx, ny, seed)
    # probes on the chunk edges too (rows of wave_rows; the accelerate row ny - 2 is in awkward_set's own rows)
    xy = awkward_set(nx, ny, ob, 0, 1, extra_rows=(rows - 1, rows) if rows else ())
    return p, ob, cells, body, xy


def _run(L, case, s, want, opts, **kw):
    p, ob, cells, body, xy = case
    return observed(L, p, ob, cells, s, want, body, 4, xy, opts, **kw)


def _in_wave(res, n, K, bits, pieces, launches, where):
    got = res["info"]
    assert got["engine_last"] == 1 and got["driven_observed_in_kernel"] == 0, where
    assert got["driven_observed_in_wave"] == bits and got["driven_observed_pieces"] == pieces, where
    assert got["wave_launches"] == launches, where


def _passes(n, K, *everys):
    """lbm_wave launches of a call of n steps cut at the multiples of `everys`: the full passes of every piece."""
    cuts = sorted({n} | {m for e in everys if e for m in range(e, n + 1, e)})
    return sum((b - a) // K for a, b in zip([0] + cuts[:-1], cuts))


def test_the_cut_run_holds_a_piece_shorter_than_a_pass():
    for K, _ in KERNELS:
        n = 2 * K + 5
        cuts = sorted({n} | set(range(K + 1, n + 1, K + 1)) | set(range(2 * K, n + 1, 2 * K)))
        lengths = [b - a for a, b in zip([0] + cuts[:-1], cuts)]
        assert pieces_of(n, K + 1, 2 * K) == len(lengths) == 4 and lengths[0] == K + 1 and lengths[1] == K - 1, (K, lengths)
        assert _passes(n, K, K + 1, 2 * K) == 1 and _passes(n, K) == n // K


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,seed,rows", SHAPES)
@pytest.mark.parametrize("K,cols", KERNELS)
def test_forces_and_probes_ride_in_the_driven_wave(gpu, K, cols, nx, ny, seed, rows):
    L = gpu
    case = _case(L, nx, ny, seed, rows)
    p, ob, cells, body, xy = case
    n = 2 * K + 5
    opts = _opts(K, cols, rows)
    s = schedules(p.accel, n, 30 + K, spikes=_spikes(K))
    spikes = ["d%d" % k for k in (K - 1, K, K + 1, 2 * K)]
    for name in ["b"] + spikes:
        ref = reference(L, (nx, ny, seed), p, ob, cells, body, 4, s[name], (n,), numpy_forces=False)
        res = _run(L, case, s[name], BOTH, opts)
        where = (nx, ny, K, cols, name, res["info"])
        _in_wave(res, n, K, 3, 1, n // K, where)
        check(res, ref, n, xy, BOTH, where, tile_forces=False)
    # the same run cut by a mean every K + 1 and a snapshot every 2 K: one piece is shorter than K (the one-step kernel)
    for name in ("b", spikes[2]):
        ref = reference(L, (nx, ny, seed), p, ob, cells, body, 4, s[name], (n,), numpy_forces=False)
        want = dict(BOTH, mean_every=K + 1, fields_every=2 * K)
        res = _run(L, case, s[name], want, opts)
        where = (nx, ny, K, cols, name, "cut", res["info"])
        _in_wave(res, n, K, 3, 4, _passes(n, K, K + 1, 2 * K), where)
        check(res, ref, n, xy, want, where, tile_forces=False)
    # forces alone and probes alone: the empty map of the other
    ref = reference(L, (nx, ny, seed), p, ob, cells, body, 4, s["b"], (n,), numpy_forces=False)
    for want, bits in ((dict(NONE, forces=True), 1), (dict(NONE, probes_every=1), 2), (dict(NONE, probes_every=K), 2)):
        res = _run(L, case, s["b"], want, opts)
        where = (nx, ny, K, cols, want, res["info"])
        _in_wave(res, n, K, bits, 1, n // K, where)
        check(res, ref, n, xy, want, where, tile_forces=False)


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_one_pass_and_a_run_shorter_than_a_pass(gpu, K, cols):
    L = gpu
    nx, ny, seed, rows = SHAPES[0]
    case = _case(L, nx, ny, seed, rows)
    p, ob, cells, body, xy = case
    opts = _opts(K, cols, rows)
    s = schedules(p.accel, K, 40 + K)["b"]
    ref = reference(L, (nx, ny, seed), p, ob, cells, body, 4, s, (K - 1, K), numpy_forces=False)
    res = _run(L, case, s, BOTH, opts)                                   # nsteps = K: one pass, no tail
    _in_wave(res, K, K, 3, 1, 1, res["info"])
    check(res, ref, K, xy, BOTH, (K, cols, res["info"]), tile_forces=False)
    res = _run(L, case, s[:K - 1], BOTH, opts)                           # nsteps = K - 1: the one-step path
    assert [res["info"][k] for k in KEYS] == [0, 0, 0] and res["info"]["wave_launches"] == 0, res["info"]
    check(res, ref, K - 1, xy, BOTH, (K, cols, res["info"]), tile_forces=False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kernel", [(SHAPES[0], KERNELS[3]), (SHAPES[1], KERNELS[1])])
def test_the_driven_observed_wave_with_ieee_maths(gpu, shape, kernel):
    L = gpu
    (nx, ny, seed, rows), (K, cols) = shape, kernel
    case = _case(L, nx, ny, seed, rows)
    p, ob, cells, body, xy = case
    n = 2 * K + 5
    ieee = (("kernel_variant", 0),)
    s = schedules(p.accel, n, 50)
    want = dict(BOTH, mean_every=K + 1)
    for name in ("b", "d%d" % (n // 2)):
        ref = reference(L, (nx, ny, seed), p, ob, cells, body, 4, s[name], (n,), (("engine", 1), ("time_block", 1)) + ieee,
                        numpy_forces=False)
        res = _run(L, case, s[name], want, _opts(K, cols, rows) + ieee)
        assert res["info"]["driven_observed_in_wave"] == 3 and res["info"]["driven_observed_pieces"] == pieces_of(n, K + 1), res["info"]
        check(res, ref, n, xy, want, (nx, ny, K, cols, name, res["info"]), tile_forces=False)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lbm_march", "two_slabs"])
def test_contexts_that_keep_the_one_step_path(gpu, which):
    L = gpu
    nx, ny, seed, rows = SHAPES[0]
    case = _case(L, nx, ny, seed, rows)
    p, ob, cells, body, xy = case
    n = 13
    s = schedules(p.accel, n, 60)["b"]
    ref = reference(L, (nx, ny, seed), p, ob, cells, body, 4, s, (n,), numpy_forces=False)
    want = dict(BOTH, mean_every=5, fields_every=4)
    if which == "lbm_march":
        res = _run(L, case, s, want, _opts(4, 1, 0, kernel=0))
    else:
        # (two slabs add up their own forces: those are the bits of the loop on two slabs; its fields are the lone loop's)
        kw = dict(nslabs=2, devices=[0, 0], exchange=L.EXCHANGE_COPY)
        res = _run(L, case, s, want, _opts(4, 1, 0), **kw)
        slabs = observed_loop(L, p, ob, cells, body, 4, s, {n}, numpy_forces=False, **kw)
        assert np.array_equal(_bits(slabs["fields"]), _bits(ref["fields"]))
        ref = dict(ref, forces=slabs["forces"])
    assert res["info"]["engine_last"] == 1 and res["info"]["wave_launches"] == 0, (which, res["info"])
    assert [res["info"][k] for k in KEYS] == [0, 0, 0], (which, res["info"])
    check(res, ref, n, xy, want, (which, res["info"]), tile_forces=False)
