"""lbm_run_stats: the means and the second moments of a run (Lattice.run_stats).

Contract (include/lbm_mi355x.h): with X_j = (u_x, u_y, |u|, p) the snapshots of lbm_run_sampled at the same `every` and
p0 = density * (1.f / 3.f), the float a blocked cell reads as pressure, a cell's eight floats are the float sums
S_j = S_(j-1) + X_j and T_j = T_(j-1) + (X.x X.x, X.y X.y, X.x X.y, (X.w - p0)^2) from +0, in step order, one rounding per
operation, divided by the number of snapshots -- bit for bit, which `stats_of` restates in numpy (float32 arrays: numpy
rounds every product and every sum once and fuses nothing).  Floats 0..3 are lbm_run_mean's.  The sums ride in lbm_wave's
launches where it runs (tests/test_wave_stats.py); every other engine -- here -- runs the steps in pieces with lbm_stats_add
behind each, pieces on a register-tile context on the tiles.

The register tilings: a tiling belongs to a lattice shape, so each tiling of tests/test_mean_run.py (TILINGS) runs on its
own lattice there, and the 64 x 40 known-answer lattice runs on the tiling the default picks for it (engine_last = 3).  On the
tiles the pieces run in the flavour lbm_run_observed's pieces use, so av_vels is lbm_run's bit for bit there (exact_av)."""
import os

import numpy as np
import pytest

from test_mean_run import TILINGS, _bits, _child, _kat_case, _oracle_fields, _plain, _sampled, mean_of
from test_mean_run import _random_case as _random3
from test_wave_probes import _opts

LBM_EINVAL = 1
INFO = ("engine_last", "stats_in_wave", "mean_in_kernel", "wave_launches")


def p0_of(density):
    return np.float32(density) * (np.float32(1) / np.float32(3))


def stats_of(snaps, p0):                # snaps: (m, rows, nx, 4) float32 from run_sampled; float32 throughout
    snaps = np.asarray(snaps)
    assert snaps.dtype == np.float32 and type(p0) is np.float32
    S = np.zeros(snaps.shape[1:], np.float32)
    T = np.zeros(snaps.shape[1:], np.float32)
    for X in snaps:
        d = X[..., 3] - p0
        S = S + X
        T = T + np.stack([X[..., 0] * X[..., 0], X[..., 1] * X[..., 1], X[..., 0] * X[..., 1], d * d], axis=-1)
    out = np.concatenate([S, T], axis=-1) / np.float32(len(snaps))
    assert out.dtype == np.float32
    return out


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_stats_run_is_declared_and_bound(L):
    assert "lbm_run_stats" in L.ABI_SYMBOLS
    hdr = open(L.HEADER_PATH).read()
    assert "int lbm_run_stats(lbm_ctx* ctx, int nsteps, float* av_vels, int every, float* stats_out);" in hdr
    assert '"stats_in_wave"' in hdr
    lib = L.load_library()
    assert lib.lbm_run_stats is not None
    assert b"stats_in_wave\0" in open(L.LIB_PATH, "rb").read()
    assert "stats_in_wave" in L.Lattice.run_stats.__doc__


def test_the_header_says_why_the_pressure_is_shifted_and_what_is_not_offered(L):
    hdr = open(L.HEADER_PATH).read()
    doc = hdr[hdr.index("lbm_run_mean with the second moments"):hdr.index("int lbm_run_stats(")]
    doc = " ".join(doc.replace("\n *", " ").split())
    for phrase in ("Why the pressure is shifted", "E[xy] - E[x] E[y]", "in double", "Not offered", "lbm_run_observed",
                   "under a schedule", "over a window", "higher moments", "command-line tool", "register tiles"):
        assert phrase in doc, phrase


def test_stats_run_rejects_a_null_context(L):
    lib = L.load_library()
    assert lib.lbm_run_stats(None, 10, None, 1, None) == LBM_EINVAL
    assert b"ctx" in lib.lbm_last_error()


def test_stats_of_on_a_series_worked_out_by_hand():
    """density 0.75: p0 = float32(0.75) * float32(1/3) = 0.75 * 11184811 * 2^-25 = 33554433 * 2^-27, which rounds to
    2^25 * 2^-27 = 0.25 exactly.  Two snapshots of a 1 x 2 lattice, every value a small dyadic fraction (nothing rounds):
      cell 0   X_1 = (0.5, -0.0, 0.5, 0.5)       d = 0.25    Q_1 = (0.25,   +0.0, -0.0, 0.0625)
               X_2 = (0.25, -0.0, 0.25, 0.375)   d = 0.125   Q_2 = (0.0625, +0.0, -0.0, 0.015625)
               S_2 = (0.75, +0.0, 0.75, 0.875)   T_2 = (0.3125, +0.0, +0.0, 0.078125)
               out = (0.375, +0.0, 0.375, 0.4375, 0.15625, +0.0, +0.0, 0.0390625)
               (-0.0 * -0.0 = +0.0; 0.5 * -0.0 = -0.0, and +0.0 + -0.0 = +0.0: no negative zero survives the sums)
      cell 1   blocked: X_1 = X_2 = (0, 0, 0, 0.25), d = 0: out = (0, 0, 0, 0.25, 0, 0, 0, 0)"""
    p0 = p0_of(0.75)
    assert type(p0) is np.float32 and p0 == np.float32(0.25)
    snaps = np.array([[[[0.5, -0.0, 0.5, 0.5], [0, 0, 0, 0.25]]], [[[0.25, -0.0, 0.25, 0.375], [0, 0, 0, 0.25]]]], np.float32)
    assert snaps.shape == (2, 1, 2, 4) and np.signbit(snaps[:, 0, 0, 1]).all()
    got = stats_of(snaps, p0)
    want = np.array([[[0.375, 0.0, 0.375, 0.4375, 0.15625, 0.0, 0.0, 0.0390625], [0, 0, 0, 0.25, 0, 0, 0, 0]]], np.float32)
    assert got.shape == (1, 2, 8) and np.array_equal(_bits(got), _bits(want))
    assert not np.signbit(got).any()
    assert np.array_equal(_bits(got[..., :4]), _bits(mean_of(snaps)))


# ---------------------------------------------------------------------------------------------------------------- GPU
def _stats(L, p, ob, cells, nsteps, every, options=(), **kw):
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        av, stats = lat.run_stats(nsteps, every)
        info = {k: int(lat.info(k)) for k in INFO}
        st = lat.read_state()
    return av, stats, st, info


def _check_case(L, p, ob, cells, nsteps, everys, options=(), engine=None, exact_av=False, **kw):
    """Bit-identical to stats_of of the context's own lbm_run_sampled; the lattice lbm_run's; blocked cells (0, 0, 0, p0, 0...)."""
    p0 = p0_of(p.density)
    av0, st0 = _plain(L, p, ob, cells, nsteps, options, **kw)
    for every in everys:
        _, fields, _ = _sampled(L, p, ob, cells, nsteps, every, options, **kw)
        av, stats, st, info = _stats(L, p, ob, cells, nsteps, every, options, **kw)
        where = (p.nx, p.ny, nsteps, every, options, info)
        assert info["stats_in_wave"] == 0 and info["mean_in_kernel"] == 0, where
        if engine is not None:
            assert info["engine_last"] == engine, where
        assert stats.shape == fields.shape[1:3] + (8,), where
        blocked = np.asarray(ob).reshape(p.ny, p.nx) != 0
        if stats.shape[0] == p.ny and blocked.any():
            assert np.all(_bits(fields[0][blocked][:, 3]) == _bits(p0)), where         # p0 is a blocked cell's snapshot pressure
        want = stats_of(fields, p0)
        bad = np.argwhere(_bits(stats) != _bits(want))
        assert len(bad) == 0, (where, len(bad), [tuple(int(v) for v in b) for b in bad[:8]])
        assert np.array_equal(_bits(st), _bits(st0)), where
        if exact_av:
            assert np.array_equal(_bits(av), _bits(av0)), where
        else:
            assert np.allclose(av, av0, rtol=2e-6, atol=0), where


@pytest.mark.gpu
def test_kat_lattice_on_the_register_tiles(gpu, O):
    """The pieces stay on the tiles (engine_last = 3); 10 steps at every = 1 (ten pieces of one step) and 3."""
    L = gpu
    k, p, ob, _ = _kat_case(L, O)
    _check_case(L, p, ob, k["cells0"], 10, (1, 3), engine=3, exact_av=True)


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", TILINGS)
def test_stats_of_every_register_tiling(gpu, ty, r, asy, nx, ny):
    L = gpu
    p, ob, cells = _random3(L, nx, ny, 7)
    opts = (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3))
    _check_case(L, p, ob, cells, 11, (3,), opts, engine=3, exact_av=True)


@pytest.mark.gpu
def test_two_slabs_with_copies(gpu, O):
    L = gpu
    k, p, ob, _ = _kat_case(L, O)
    _check_case(L, p, ob, k["cells0"], 10, (1, 4), nslabs=2, devices=[0, 0], exchange=L.EXCHANGE_COPY)


@pytest.mark.gpu
def test_rank_context_ring_of_one(gpu):
    L = gpu
    from test_mean_run import _deck
    p, ob = _deck(L, "128x256")
    os.environ["LBM_FORCE_EXCHANGE"] = "1"
    nsteps, every = 13, 5
    _, fields, st1 = _sampled(L, p, ob, None, nsteps, every)
    av1, _ = _plain(L, p, ob, None, nsteps)
    try:
        av, stats, st, info = _stats(L, p, ob, None, nsteps, every, rank=0, nranks=1, device=0, unique_id=L.rccl_unique_id(),
                                     exchange=L.EXCHANGE_RCCL)
        assert info["stats_in_wave"] == 0, info
        assert stats.shape == (p.ny, p.nx, 8)       # (rank-local rows: the ring of one holds them all)
        assert np.array_equal(_bits(stats), _bits(stats_of(fields, p0_of(p.density))))
        assert np.array_equal(_bits(st), _bits(st1))
        assert np.allclose(av, av1, rtol=2e-6, atol=0)
    finally:
        del os.environ["LBM_FORCE_EXCHANGE"]


@pytest.mark.gpu
def test_lbm_march_keeps_the_split_path(gpu):
    """256 x 64 at time_block 4 with lbm_march (the smallest marching shape of tests/test_wave_fields.py)."""
    L = gpu
    p, ob, cells = _random3(L, 256, 64, 11)
    _check_case(L, p, ob, cells, 13, (1, 3), _opts(4, kernel=0), engine=1)


# torch and the library share libamdhip64: torch is imported FIRST, in a child process of its own
_DEVICE_OUTPUT = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_stats_run import _bits, _opts, _random3, _stats
p, ob, cells = _random3(L, 256, 64, 11)
nsteps, every = 21, 3
for opts, in_wave in ((_opts(8, 2, 24), 1), (_opts(6, 1, 24), 1), ((("engine", 1), ("time_block", 1)), 0)):
    av_h, want, st_h, info = _stats(L, p, ob, cells, nsteps, every, opts)
    assert info["stats_in_wave"] == in_wave, (opts, info)
    out = torch.full((64, 256, 8), float("nan"), dtype=torch.float32, device="cuda:0")
    with L.Lattice(p, ob, cells) as lat:
        for k, v in opts:
            lat.set_option(k, v)
        av, got = lat.run_stats(nsteps, every, out=out)
        assert got is out and lat.info("stats_in_wave") == in_wave
        st = lat.read_state()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), opts
    assert np.array_equal(_bits(av), _bits(av_h)) and np.array_equal(_bits(st), _bits(st_h)), opts
print("device output ok")
"""


@pytest.mark.gpu
def test_device_output_is_the_host_output(gpu):
    assert "device output ok" in _child(_DEVICE_OUTPUT)


@pytest.mark.gpu
def test_refusals_leave_the_lattice_alone(gpu, O):
    """Every refusal that can be asked for without breaking something: negative nsteps, every <= 0, m = 0, no output -- on a
    register-tile context and on an lbm_wave context.  (No room for the sums and a failed peer-to-peer wait are not provoked.)"""
    L = gpu
    lib = L.load_library()
    k, p, ob, _ = _kat_case(L, O)
    p2, ob2, cells2 = _random3(L, 256, 64, 11)
    for prm, obs, cells, opts in ((p, ob, k["cells0"], ()), (p2, ob2, cells2, _opts(8, 1, 24))):
        out = np.zeros((prm.ny, prm.nx, 8), np.float32)
        with L.Lattice(prm, obs, cells) as lat, L.Lattice(prm, obs, cells) as twin:
            for key, v in opts:
                lat.set_option(key, v)
                twin.set_option(key, v)
            lat.run(3)
            twin.run(3)
            st = lat.read_state()
            with pytest.raises(L.LbmError):
                lat.run_stats(10, 0)
            assert lib.lbm_run_stats(lat._ctx, -1, None, 1, out.ctypes.data) == LBM_EINVAL         # nsteps < 0
            assert lib.lbm_run_stats(lat._ctx, 10, None, 0, out.ctypes.data) == LBM_EINVAL         # every = 0
            assert lib.lbm_run_stats(lat._ctx, 10, None, -1, out.ctypes.data) == LBM_EINVAL        # every < 0
            assert lib.lbm_run_stats(lat._ctx, 10, None, 11, out.ctypes.data) == LBM_EINVAL        # m = 0
            assert lib.lbm_run_stats(lat._ctx, 10, None, 5, None) == LBM_EINVAL                    # no output
            assert not out.any()
            assert np.array_equal(_bits(lat.read_state()), _bits(st))
            assert lat.info("stats_in_wave") == 0
            av, _ = lat.run_stats(10, 5)
            assert np.allclose(av, twin.run(10), rtol=2e-6, atol=0)
            assert np.array_equal(_bits(lat.read_state()), _bits(twin.read_state()))


def _oracle_moment_bound(k, p, ob, op, oracle, nsteps=10):
    """The strict float oracle stepped one step at a time: (the float64 fold of Q_j over its per-step float64 fields, the
    bound on |stats[4..7] - that| per element).  Built as _oracle_mean_bound of tests/test_mean_run.py builds its own: the
    per-element bounds dx of _oracle_fields carried through each product, |x| dy + |y| dx + dx dy, averaged over the steps;
    + nsteps 2^-24 mean|Q_j| (the float sum); the caller adds 2^-24 |result| (the division).  Blocked cells: exactly 0."""
    p0 = float(p0_of(k["density"]))
    ref = k["cells0"].copy()
    Q, tq = [], []
    blocked = ob.reshape(p.ny, p.nx) != 0
    for _ in range(nsteps):
        oracle.run(op, ref, ob, 1)
        w, t = _oracle_fields(ref.reshape(p.ny, p.nx, 9), ob, k["density"])
        x, y, d = w[..., 0], w[..., 1], w[..., 3] - p0
        dx, dy, dd = t[..., 0], t[..., 1], t[..., 3]
        q = np.stack([x * x, y * y, x * y, d * d], axis=-1)
        e = np.stack([2 * np.abs(x) * dx + dx * dx, 2 * np.abs(y) * dy + dy * dy, np.abs(x) * dy + np.abs(y) * dx + dx * dy,
                      2 * np.abs(d) * dd + dd * dd], axis=-1)
        q[blocked] = 0.0
        e[blocked] = 0.0
        Q.append(q)
        tq.append(e)
    want = np.mean(Q, axis=0)
    bound = np.mean(tq, axis=0) + nsteps * 2.0 ** -24 * np.mean(np.abs(Q), axis=0)
    return want, bound, ref


@pytest.mark.gpu
def test_second_moments_against_the_float_oracle(gpu, O, oracle):
    """64 x 40 known-answer lattice, 10 steps, every step a sample: floats 4..7 against the float64 fold of the strict float
    oracle's per-step fields, inside _oracle_moment_bound."""
    L = gpu
    k, p, ob, op = _kat_case(L, O)
    want, bound, ref = _oracle_moment_bound(k, p, ob, op, oracle)
    assert np.array_equal(ref, k["cells_after_10"])
    _, stats, st, info = _stats(L, p, ob, k["cells0"], 10, 1)
    assert np.all(np.abs(st - ref) <= 2e-5 * np.abs(ref))
    got = stats[..., 4:].astype(np.float64)
    err = np.abs(got - want)
    lim = bound + 2.0 ** -24 * np.abs(got)
    print("second moments against the oracle: max error %.3g, worst error - bound %.3g, worst error / bound %.3g"
          % (err.max(), np.max(err - lim), np.max(err / np.where(lim > 0, lim, 1.0))))
    assert np.all(err <= lim), float(np.max(err - lim))
