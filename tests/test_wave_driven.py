"""lbm_run_driven where lbm_wave runs (a lattice alone, time_block 4 / 6 / 8): the schedule rides in lbm_wave's launches.

Contract (include/lbm_mi355x.h): a pass that starts at step tt carries the accelerate constants of steps tt + 1 .. tt + K in
its arguments, one pair per level; the prologue launch takes entry 0 of the call; the steps left over behind the last full
pass go one at a time through the one-step kernel, each with its own constants.  The lattice is the BITS of
`for a in accel: set_accel(a); run(1)` (test_driven_run.loop_reference: engine 1, time_block 1); av_vels are that loop's to
rounding, and under a constant schedule lbm_run's bits for the steps inside full passes; info "driven_in_wave" reads 1,
"driven_in_kernel" 0, and "wave_launches" grows by one kernel per pass (2 K + 5 steps: two passes and a five-step tail at
K = 6 and 8, three passes and one step at K = 4).  Contexts where lbm_march runs, slabs with neighbours
and runs shorter than K keep the one-step path.

Shapes and kernels are those of tests/test_wave_fields.py: 256 x 64 with wave_rows 24 (several wave columns, two blocks,
chunks of 24, 24 and 16 rows: the accelerate row ny - 2 lies in the last chunk and in the fill rows of the first) and
200 x 72 (a width that is no multiple of 64 - 2 K, nor of 64)."""
import numpy as np
import pytest

from test_body_forces import _plain
from test_driven_run import AV_RTOL, _bits, _random_case, driven, reference, schedules
from test_wave_fields import KERNELS, SHAPES
from test_wave_probes import _opts


def _case(L, nx, ny, seed):
    return _random_case(L, nx, ny, seed)


def _spikes(K):
    n = 2 * K + 5
    return (0, K - 1, K, K + 1, 2 * K, n - 1)


def test_the_spikes_sit_on_both_sides_of_a_pass_boundary():
    """2 K + 5 steps: passes over steps 0 .. K - 1 and K .. 2 K - 1 (0-based), then five single steps -- at K = 6 and 8; at
    K = 4 the 13 steps hold a third pass (steps 8 .. 11) and one single step.  Entry K - 1 is what level K - 1 of the first
    pass applies, entry K what its level K applies under accel_out, entry K + 1 level 1 of the second pass; entry 2 K is
    applied by the second pass's level K, entry n - 1 by the last but one single step (K = 4: by the third pass's level K);
    entry 0 by the prologue launch."""
    for K, _ in KERNELS:
        k = _spikes(K)
        assert k[1] // K == 0 and k[2] // K == 1 and k[3] // K == 1 and k[4] == 2 * K and k[5] == 2 * K + 4
        assert len(set(k)) == 6
        assert (2 * K + 5) // K == (3 if K == 4 else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,seed,rows", SHAPES)
@pytest.mark.parametrize("K,cols", KERNELS)
def test_driven_wave_runs_are_the_bits_of_the_loop(gpu, K, cols, nx, ny, seed, rows):
    L = gpu
    p, ob, cells = _case(L, nx, ny, seed)
    n = 2 * K + 5
    opts = _opts(K, cols, rows)
    s = schedules(p.accel, n, 30 + K, spikes=_spikes(K))
    for name in ["b", "c"] + ["d%d" % k for k in _spikes(K)]:
        av_l, states = reference(L, (nx, ny, seed), p, ob, cells, s[name], (n,))
        av, st, info = driven(L, p, ob, cells, s[name], opts)
        where = (nx, ny, K, cols, name, info)
        assert info == dict(engine_last=1, driven_in_kernel=0, driven_in_wave=1, wave_launches=n // K), where
        bad = np.argwhere(_bits(st) != _bits(states[n]))
        assert len(bad) == 0, (where, len(bad), [tuple(int(v) for v in b) for b in bad[:8]])
        print(where, "av_vels: worst relative difference %.3g" % np.max(np.abs(av - av_l) / np.abs(av_l)))
        assert np.allclose(av, av_l, rtol=AV_RTOL, atol=0), where
    # schedule (a): lbm_run under the same options -- the lattice, and av_vels of the steps inside the full passes
    av0, st0 = _plain(L, p, ob, cells, n, opts)
    av, st, info = driven(L, p, ob, cells, s["a"], opts)
    inside = (n // K) * K
    assert info["driven_in_wave"] == 1 and info["wave_launches"] == n // K and inside >= 2 * K
    assert np.array_equal(_bits(st), _bits(st0))
    assert np.array_equal(_bits(av[:inside]), _bits(av0[:inside])) and np.allclose(av, av0, rtol=AV_RTOL, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("K,cols", KERNELS)
def test_one_pass_and_a_run_shorter_than_a_pass(gpu, K, cols):
    L = gpu
    nx, ny, seed, rows = SHAPES[0]
    p, ob, cells = _case(L, nx, ny, seed)
    opts = _opts(K, cols, rows)
    s = schedules(p.accel, K, 40 + K)["b"]
    av_l, states = reference(L, (nx, ny, seed), p, ob, cells, s, (K - 1, K))
    av, st, info = driven(L, p, ob, cells, s, opts)                      # nsteps = K: one pass, no tail
    assert info == dict(engine_last=1, driven_in_kernel=0, driven_in_wave=1, wave_launches=1), info
    assert np.array_equal(_bits(st), _bits(states[K])) and np.allclose(av, av_l, rtol=AV_RTOL, atol=0)
    av, st, info = driven(L, p, ob, cells, s[:K - 1], opts)              # nsteps = K - 1: the one-step path
    assert info == dict(engine_last=1, driven_in_kernel=0, driven_in_wave=0, wave_launches=0), info
    assert np.array_equal(_bits(st), _bits(states[K - 1])) and np.allclose(av, av_l[:K - 1], rtol=AV_RTOL, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kernel", [(SHAPES[0], KERNELS[3]), (SHAPES[1], KERNELS[1])])
def test_driven_wave_runs_with_ieee_maths(gpu, shape, kernel):
    L = gpu
    (nx, ny, seed, rows), (K, cols) = shape, kernel
    p, ob, cells = _case(L, nx, ny, seed)
    n = 2 * K + 5
    ieee = (("kernel_variant", 0),)
    s = schedules(p.accel, n, 50)
    for name in ("b", "d%d" % (n // 2)):
        av_l, states = reference(L, (nx, ny, seed), p, ob, cells, s[name], (n,), (("engine", 1), ("time_block", 1)) + ieee)
        av, st, info = driven(L, p, ob, cells, s[name], _opts(K, cols, rows) + ieee)
        assert info["driven_in_wave"] == 1 and info["wave_launches"] == n // K, info
        assert np.array_equal(_bits(st), _bits(states[n])), (name, info)
        assert np.allclose(av, av_l, rtol=AV_RTOL, atol=0), name


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lbm_march", "two_slabs"])
def test_contexts_that_keep_the_one_step_path(gpu, which):
    L = gpu
    nx, ny, seed, rows = SHAPES[0]
    p, ob, cells = _case(L, nx, ny, seed)
    n = 13
    s = schedules(p.accel, n, 60)["b"]
    av_l, states = reference(L, (nx, ny, seed), p, ob, cells, s, (n,))
    if which == "lbm_march":
        av, st, info = driven(L, p, ob, cells, s, _opts(4, 1, 0, kernel=0))
    else:
        av, st, info = driven(L, p, ob, cells, s, _opts(4, 1, 0), nslabs=2, devices=[0, 0], exchange=L.EXCHANGE_COPY)
    assert info == dict(engine_last=1, driven_in_kernel=0, driven_in_wave=0, wave_launches=0), (which, info)
    assert np.array_equal(_bits(st), _bits(states[n])), which
    assert np.allclose(av, av_l, rtol=AV_RTOL, atol=0), which
