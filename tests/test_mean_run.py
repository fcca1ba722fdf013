"""lbm_run_mean: time-averaged fields of a run (Lattice.run_mean).

Contract (include/lbm_mi355x.h): with X_j the snapshots of lbm_run_sampled at the same `every`, the mean is the float sum
S_j = S_(j-1) + X_j from S_0 = +0, in step order, divided by the number of snapshots -- bit for bit, which `mean_of` restates
in numpy -- and a mean run leaves av_vels and the lattice bit-identical to lbm_run.  The register-tile engines keep the sums
inside their kernels (mean_in_kernel = 1); every other engine runs the steps in pieces with an add kernel behind each."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, deck_paths, load_kat
from test_sampled_run import DECK_CASES, TILINGS

LBM_EINVAL, LBM_ENOMEM = 1, 5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mean_of(snaps):                     # snaps: (m, rows, nx, 4) float32 from run_sampled / final_state
    s = np.zeros(snaps.shape[1:], np.float32)
    for x in snaps:
        s = s + x                       # float32 adds, step order
    return s / np.float32(len(snaps))


def _oracle_fields(cells, ob, density, rel=2e-5):
    """The fields of write_values() from the oracle's lattice (float64), and the bound on |gpu - oracle| per element that
    follows from every population agreeing to `rel` relative (smoke()'s bar for the lattice): the numerators of u_x, u_y
    carry rel x the sum of their six populations, rho carries rel x rho; plus float32 rounding of the derive itself.
    (The construction of test_sampled_run.py.)"""
    f = cells.astype(np.float64)
    rho = f.sum(axis=2)
    nx_ = f[..., 1] + f[..., 5] + f[..., 8] - (f[..., 3] + f[..., 6] + f[..., 7])
    ny_ = f[..., 2] + f[..., 5] + f[..., 6] - (f[..., 4] + f[..., 7] + f[..., 8])
    ax = f[..., 1] + f[..., 5] + f[..., 8] + f[..., 3] + f[..., 6] + f[..., 7]
    ay = f[..., 2] + f[..., 5] + f[..., 6] + f[..., 4] + f[..., 7] + f[..., 8]
    ux, uy = nx_ / rho, ny_ / rho
    u = np.sqrt(ux * ux + uy * uy)
    want = np.stack([ux, uy, u, rho / 3], axis=-1)
    eps = 1e-6                                   # a few float32 ulps of the derive's own operations
    ex = rel * (ax / rho + np.abs(ux)) + eps * ax / rho
    ey = rel * (ay / rho + np.abs(uy)) + eps * ay / rho
    tol = np.stack([ex, ey, ex + ey, (rel + eps) * rho / 3], axis=-1)
    b = ob.reshape(rho.shape) != 0
    want[b] = (0.0, 0.0, 0.0, np.float32(density) / np.float32(3))
    tol[b] = 0.0
    return want, tol


def _kat_case(L, O):
    k = load_kat("kat_64x40")
    p = L.Param(int(k["nx"]), int(k["ny"]), 10, int(k["reynolds_dim"]), float(k["density"]), float(k["accel"]),
                float(k["omega"]))
    ob = np.ascontiguousarray(k["obstacles"], dtype=np.int32)
    op = O.OrcParam(p.nx, p.ny, 10, p.reynolds_dim, float(k["density"]), float(k["accel"]), float(k["omega"]))
    return k, p, ob, op


def _oracle_mean_bound(k, p, ob, op, oracle, nsteps=10):
    """The strict float oracle stepped one step at a time: (mean of the per-step float64 fields, the bound on
    |mean - that| per element, the oracle's own float32 fields per step, its last lattice).  Bound = mean of the per-step
    bounds of _oracle_fields + (nsteps) 2^-24 mean|want_j| (a float sum of nsteps terms from zero: at most nsteps - 1
    roundings that matter, each within 2^-24 of a partial sum no larger than the sum of |want_j|; the issue's figure, 10,
    is kept for the 10 steps) + 2^-24 |mean| (the division)."""
    ref = k["cells0"].copy()
    wants, tols, own = [], [], []
    for _ in range(nsteps):
        oracle.run(op, ref, ob, 1)
        w, t = _oracle_fields(ref.reshape(p.ny, p.nx, 9), ob, k["density"])
        wants.append(w)
        tols.append(t)
        own.append(oracle.final_state(op, ref, ob).reshape(p.ny, p.nx, 4))
    want = np.mean(wants, axis=0)
    bound = np.mean(tols, axis=0) + nsteps * 2.0 ** -24 * np.mean(np.abs(wants), axis=0)
    return want, bound, np.stack(own), ref


def _within(mean, want, bound):
    err = np.abs(mean.astype(np.float64) - want)
    lim = bound + 2.0 ** -24 * np.abs(mean.astype(np.float64))
    return err, lim


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_mean_run_is_declared_and_bound(L):
    assert "lbm_run_mean" in L.ABI_SYMBOLS
    hdr = open(L.HEADER_PATH).read()
    assert "int lbm_run_mean(lbm_ctx* ctx, int nsteps, float* av_vels, int every, float* mean_out);" in hdr
    assert '"mean_in_kernel"' in hdr


def test_mean_run_rejects_a_null_context(L):
    lib = L.load_library()
    assert lib.lbm_run_mean(None, 10, None, 1, None) == LBM_EINVAL
    assert b"ctx" in lib.lbm_last_error()


def test_isa_audit_covers_the_mean_flavour():
    """tools/audit_regtile_isa.py lists the asynchronous mean-flavour instantiations (mode bit 65536) of lbm_regtile and
    lbm_regtile_slabs for R = 2 and 4, fast and IEEE maths, each with 0 findings, and nothing else has one either."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_regtile_isa.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = {}
    for name, rr, mode, nf in re.findall(r"^(lbm_regtile(?:_slabs)?)<(\d+), (\d+)>: \d+ asm loads audited, (\d+) finding\(s\)",
                                         r.stdout, flags=re.M):
        seen[(name, int(rr), int(mode))] = int(nf)
    for name, slab in (("lbm_regtile", 0), ("lbm_regtile_slabs", 8192)):
        for rr in (2, 4):
            for fast in (0, 1):
                key = (name, rr, 65536 | 4096 | slab | fast)
                assert key in seen, (key, r.stdout)
                assert seen[key] == 0, (key, r.stdout)


def test_the_oracles_own_fields_pass_the_oracle_bound(L, O, oracle):
    """The bar of test_mean_against_the_float_oracle tests the kernel, not the bound: the strict float oracle's own
    per-step float32 fields, averaged with mean_of, sit far inside it (blocked cells included)."""
    k, p, ob, op = _kat_case(L, O)
    want, bound, own, ref = _oracle_mean_bound(k, p, ob, op, oracle)
    assert np.array_equal(ref, k["cells_after_10"])
    err, lim = _within(mean_of(own), want, bound)
    print("oracle's own mean: max error %.3g, worst error / bound %.3g" % (err.max(), np.max(err / np.where(lim > 0, lim, 1.0))))
    assert np.all(err <= lim)
    assert np.all(err[lim > 0] <= 0.05 * lim[lim > 0])      # (1.3 % at worst when this was written)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _deck(L, deck):
    pf, of = deck_paths(deck)
    p = L.read_params(pf)
    return p, L.read_obstacles(of, p)


def _random_case(L, nx, ny, seed, blocked=0.1):
    rng = np.random.default_rng(seed)
    p = L.Param(nx, ny, 100, 10, 0.1, 0.01, 1.85)
    ob = (rng.random((ny, nx)) < blocked).astype(np.int32)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float32)
    cells = (0.1 * w * (1.0 + 0.2 * (rng.random((ny, nx, 9), dtype=np.float32) - 0.5))).astype(np.float32)
    return p, ob, cells


INFO = ("engine_last", "mean_in_kernel")


def _mean(L, p, ob, cells, nsteps, every, options=(), **kw):
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        av, mean = lat.run_mean(nsteps, every)
        info = {k: lat.info(k) for k in INFO}
        st = lat.read_state()
    return av, mean, st, info


def _sampled(L, p, ob, cells, nsteps, every, options=(), **kw):
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        av, fields = lat.run_sampled(nsteps, every)
        st = lat.read_state()
    return av, fields, st


def _plain(L, p, ob, cells, nsteps, options=(), **kw):
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        av = lat.run(nsteps)
        st = lat.read_state()
    return av, st


@pytest.mark.gpu
@pytest.mark.parametrize("deck,nsteps,everys", DECK_CASES)
def test_mean_is_the_float_sum_of_the_snapshots_on_the_shipped_decks(gpu, deck, nsteps, everys):
    L = gpu
    p, ob = _deck(L, deck)
    av0, st0 = _plain(L, p, ob, None, nsteps)
    for every in everys:
        _, fields, _ = _sampled(L, p, ob, None, nsteps, every)
        av, mean, st, info = _mean(L, p, ob, None, nsteps, every)
        assert info["engine_last"] == 3 and info["mean_in_kernel"] == 1, (deck, every, info)
        assert mean.shape == (p.ny, p.nx, 4)
        assert np.array_equal(_bits(mean), _bits(mean_of(fields))), (deck, every)
        assert np.array_equal(_bits(av), _bits(av0)) and np.array_equal(_bits(st), _bits(st0)), (deck, every)


@pytest.mark.gpu
def test_one_long_window(gpu):
    """2000 steps, every step a sample: where a reassociated or fused sum would show."""
    L = gpu
    p, ob = _deck(L, "128x128")
    nsteps, chunk = 2000, 250
    s = np.zeros((p.ny, p.nx, 4), np.float32)
    with L.Lattice(p, ob) as lat:
        for _ in range(nsteps // chunk):
            _, fields = lat.run_sampled(chunk, 1)
            for x in fields:
                s = s + x
        st0 = lat.read_state()
    want = s / np.float32(nsteps)
    av, mean, st, info = _mean(L, p, ob, None, nsteps, 1)
    assert info["engine_last"] == 3 and info["mean_in_kernel"] == 1
    assert np.array_equal(_bits(mean), _bits(want))
    assert np.array_equal(_bits(st), _bits(st0))


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", TILINGS)
def test_mean_of_every_register_tiling(gpu, ty, r, asy, nx, ny):
    L = gpu
    p, ob, cells = _random_case(L, nx, ny, 7)
    nsteps = 11
    opts = (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3))
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts)
    for every in (3, 1):
        _, fields, _ = _sampled(L, p, ob, cells, nsteps, every, opts)
        av, mean, st, info = _mean(L, p, ob, cells, nsteps, every, opts)
        assert info["engine_last"] == 3 and info["mean_in_kernel"] == 1
        assert np.array_equal(_bits(mean), _bits(mean_of(fields))), every
        assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(av), _bits(av0))


@pytest.mark.gpu
@pytest.mark.parametrize("asy", [0, 1])
def test_mean_with_ieee_maths(gpu, asy):
    L = gpu
    p, ob, cells = _random_case(L, 256, 256, 7)
    nsteps = 11
    opts = (("regtile", 84), ("regtile_async", asy), ("engine", 3), ("kernel_variant", 0))
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts)
    for every in (3, 1):
        _, fields, _ = _sampled(L, p, ob, cells, nsteps, every, opts)
        av, mean, st, info = _mean(L, p, ob, cells, nsteps, every, opts)
        assert info["engine_last"] == 3 and info["mean_in_kernel"] == 1
        assert np.array_equal(_bits(mean), _bits(mean_of(fields))), every
        assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(av), _bits(av0))


@pytest.mark.gpu
@pytest.mark.parametrize("time_block", [1, 2, 4, 8])
def test_streaming_engines_give_the_register_tiles_mean(gpu, time_block):
    L = gpu
    p, ob = _deck(L, "256x256")
    nsteps = 21
    for every in (3, 8):                 # 3: not a multiple of any time_block > 1
        av_t, want, st_t, info_t = _mean(L, p, ob, None, nsteps, every)
        assert info_t["mean_in_kernel"] == 1
        av, mean, st, info = _mean(L, p, ob, None, nsteps, every, (("engine", 1), ("time_block", time_block)))
        assert info["engine_last"] == 1 and info["mean_in_kernel"] == 0
        assert np.array_equal(_bits(mean), _bits(want)), (time_block, every)
        assert np.array_equal(_bits(st), _bits(st_t))
        assert np.allclose(av, av_t, rtol=2e-6, atol=0)


@pytest.mark.gpu
def test_a_size_that_does_not_tile(gpu):
    L = gpu
    k = load_kat("kat_33x20")
    p = L.Param(int(k["nx"]), int(k["ny"]), 10, int(k["reynolds_dim"]), float(k["density"]), float(k["accel"]),
                float(k["omega"]))
    ob = np.ascontiguousarray(k["obstacles"], dtype=np.int32)
    nsteps = 10
    av0, st0 = _plain(L, p, ob, k["cells0"], nsteps)
    for every in (1, 3):
        _, fields, _ = _sampled(L, p, ob, k["cells0"], nsteps, every)
        av, mean, st, info = _mean(L, p, ob, k["cells0"], nsteps, every)
        assert info["mean_in_kernel"] == 0 and info["engine_last"] == 1
        assert np.array_equal(_bits(mean), _bits(mean_of(fields))), every
        assert np.array_equal(_bits(st), _bits(st0))
        assert np.allclose(av, av0, rtol=2e-6, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("deck,nslabs,exchange", [("256x256", 2, "copy"), ("256x256", 4, "copy"), ("256x256", 2, "p2p"),
                                                   ("256x256", 4, "p2p"), ("1024x1024", 2, "p2p")])
def test_slabs_give_the_single_slab_mean(gpu, deck, nslabs, exchange):
    L = gpu
    p, ob = _deck(L, deck)
    nsteps, every = 10, 4
    av1, want, st1, _ = _mean(L, p, ob, None, nsteps, every)
    ex = L.EXCHANGE_COPY if exchange == "copy" else L.EXCHANGE_P2P
    av, mean, st, info = _mean(L, p, ob, None, nsteps, every, nslabs=nslabs, devices=[0] * nslabs, exchange=ex)
    assert np.array_equal(_bits(mean), _bits(want))
    assert np.array_equal(_bits(st), _bits(st1))
    assert np.allclose(av, av1, rtol=2e-6, atol=0)
    if info["engine_last"] == 3:
        assert info["mean_in_kernel"] == 1
    if exchange == "p2p":                # register tiles across slabs
        assert info["engine_last"] == 3 and info["mean_in_kernel"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["rccl", "p2p"])
def test_rank_context_ring_of_one_gives_the_single_slab_mean(gpu, exchange):
    L = gpu
    p, ob = _deck(L, "128x256")
    nsteps, every = 13, 5
    av1, want, st1, _ = _mean(L, p, ob, None, nsteps, every)
    os.environ["LBM_FORCE_EXCHANGE"] = "1"
    try:
        ex = L.EXCHANGE_RCCL if exchange == "rccl" else L.EXCHANGE_P2P
        av, mean, st, _ = _mean(L, p, ob, None, nsteps, every, rank=0, nranks=1, device=0,
                                unique_id=L.rccl_unique_id(), exchange=ex)
    finally:
        del os.environ["LBM_FORCE_EXCHANGE"]
    assert mean.shape == want.shape            # (rank-local rows: the ring of one holds them all)
    assert np.array_equal(_bits(mean), _bits(want))
    assert np.array_equal(_bits(st), _bits(st1))
    assert np.allclose(av, av1, rtol=2e-6, atol=0)


@pytest.mark.gpu
def test_mean_against_the_float_oracle(gpu, O, oracle):
    """64 x 40 known-answer lattice, 10 steps, every step a sample, against the mean of fields derived from the strict
    float oracle's lattice at every step: the lattice to 2e-5 relative, as smoke(), carried through the derive, plus the
    derived bounds of a 10-term float sum and of the division (see _oracle_mean_bound)."""
    L = gpu
    k, p, ob, op = _kat_case(L, O)
    want, bound, _, ref = _oracle_mean_bound(k, p, ob, op, oracle)
    assert np.array_equal(ref, k["cells_after_10"])
    _, mean, st, info = _mean(L, p, ob, k["cells0"], 10, 1)
    assert info["mean_in_kernel"] == 1
    assert np.all(np.abs(st - ref) <= 2e-5 * np.abs(ref))
    err, lim = _within(mean, want, bound)
    print("mean against the oracle: max error %.3g, worst error - bound %.3g" % (err.max(), np.max(err - lim)))
    assert np.all(err <= lim), float(np.max(err - lim))


# torch and the library share libamdhip64: torch is imported FIRST, in a child process of its own
_DEVICE_OUTPUT = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_mean_run import _deck, _mean, _bits
p, ob = _deck(L, "128x256")
nsteps, every = 12, 5
av_h, want, st_h, _ = _mean(L, p, ob, None, nsteps, every)
out = torch.full((p.ny, p.nx, 4), float("nan"), dtype=torch.float32, device="cuda:0")
with L.Lattice(p, ob) as lat:
    av, got = lat.run_mean(nsteps, every, out=out)
    assert got is out and lat.info("mean_in_kernel") == 1
    st = lat.read_state()
torch.cuda.synchronize()
assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
assert np.array_equal(_bits(av), _bits(av_h)) and np.array_equal(_bits(st), _bits(st_h))
out.fill_(float("nan"))                   # the streaming engines' pieces, into device memory as well
torch.cuda.synchronize()
with L.Lattice(p, ob) as lat:
    lat.set_option("engine", 1)
    lat.run_mean(nsteps, every, out=out)
    assert lat.info("mean_in_kernel") == 0
torch.cuda.synchronize()
assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
print("device output ok")
"""


def _child(code):
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", code.format(root=os.path.dirname(tests), tests=tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
def test_device_output_is_the_host_output(gpu):
    assert "device output ok" in _child(_DEVICE_OUTPUT)


@pytest.mark.gpu
def test_refusals_leave_the_lattice_alone(gpu):
    L = gpu
    lib = L.load_library()
    p, ob = _deck(L, "128x128")
    out = np.zeros((p.ny, p.nx, 4), np.float32)
    with L.Lattice(p, ob) as lat:
        lat.run(3)
        with pytest.raises(L.LbmError):
            lat.run_mean(10, 0)
        assert lib.lbm_run_mean(lat._ctx, 10, None, 0, out.ctypes.data) == LBM_EINVAL          # every = 0
        assert lib.lbm_run_mean(lat._ctx, 10, None, -1, out.ctypes.data) == LBM_EINVAL         # every < 0
        assert lib.lbm_run_mean(lat._ctx, 10, None, 11, out.ctypes.data) == LBM_EINVAL         # every > nsteps: nothing to average
        assert lib.lbm_run_mean(lat._ctx, 10, None, 5, None) == LBM_EINVAL                     # no output
        assert lib.lbm_run_mean(lat._ctx, -1, None, 1, out.ctypes.data) == LBM_EINVAL
        assert not out.any()
        av = lat.run(10)
        st1 = lat.read_state()
    with L.Lattice(p, ob) as ref:
        av_ref = ref.run(13)
        assert np.array_equal(_bits(st1), _bits(ref.read_state()))
        assert np.array_equal(_bits(av), _bits(av_ref[3:]))


@pytest.mark.gpu
def test_one_context_through_mixed_calls(gpu):
    L = gpu
    p, ob = _deck(L, "128x256")
    body = np.where(L.read_obstacles(deck_paths("128x256")[1], p) != 0, 1, 0).astype(np.int32)
    with L.Lattice(p, ob) as lat:
        lat.set_bodies(body, 1)
        avs = [lat.run(7)]
        a, mean1 = lat.run_mean(9, 2)
        avs.append(a)
        a, _ = lat.run_sampled(8, 3)
        avs.append(a)
        a, _ = lat.run_forces(5)
        avs.append(a)
        a, mean2 = lat.run_mean(11, 4)
        avs.append(a)
        assert lat.info("mean_in_kernel") == 1
        st = lat.read_state()
    with L.Lattice(p, ob) as ref:
        av_ref = ref.run(40)
        assert np.array_equal(_bits(st), _bits(ref.read_state()))
        assert np.array_equal(_bits(np.concatenate(avs)), _bits(av_ref))
    with L.Lattice(p, ob) as fresh:
        fresh.run(7)
        _, m1 = fresh.run_mean(9, 2)
        assert np.array_equal(_bits(mean1), _bits(m1))
    with L.Lattice(p, ob) as fresh:
        fresh.run(29)
        _, fields = fresh.run_sampled(11, 4)
    assert np.array_equal(_bits(mean2), _bits(mean_of(fields)))
    with L.Lattice(p, ob) as fresh:
        fresh.run(29)
        _, m2 = fresh.run_mean(11, 4)
    assert np.array_equal(_bits(mean2), _bits(m2))
