"""lbm_run_sampled: snapshots of the derived fields during a run (Lattice.run_sampled).

Contract: snapshot j is bit-identical to lbm_final_state after (j+1) every steps, and a sampled run leaves av_vels and the
lattice bit-identical to lbm_run.  The register-tile engines write the snapshots from inside their kernels
(samples_in_kernel = 1); every other engine runs the steps in pieces with a derive after each."""
import os

import numpy as np
import pytest

from conftest import deck_paths, load_kat

LBM_EINVAL, LBM_ENOMEM = 1, 5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_sampled_run_is_declared_and_bound(L):
    assert "lbm_run_sampled" in L.ABI_SYMBOLS
    hdr = open(L.HEADER_PATH).read()
    assert "int lbm_run_sampled(lbm_ctx* ctx, int nsteps, float* av_vels, int every, float* fields_out);" in hdr
    assert '"samples_in_kernel"' in hdr


def test_sampled_run_rejects_a_null_context(L):
    lib = L.load_library()
    assert lib.lbm_run_sampled(None, 10, None, 5, None) == LBM_EINVAL
    assert b"ctx" in lib.lbm_last_error()


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


def _chunked(L, p, ob, cells, nsteps, every, **kw):
    """What the snapshots must be: lbm_final_state after every `every` steps of separate runs (each a complete run)."""
    snaps, avs = [], []
    with L.Lattice(p, ob, cells, **kw) as lat:
        done = 0
        while done + every <= nsteps:
            avs.append(lat.run(every))
            snaps.append(lat.final_state())
            done += every
        avs.append(lat.run(nsteps - done))
        st = lat.read_state()
    m = nsteps // every
    shape = (m,) + (snaps[0].shape if snaps else (0, 0, 4))
    return np.concatenate(avs), (np.stack(snaps) if snaps else np.empty(shape, np.float32)), st


def _sampled(L, p, ob, cells, nsteps, every, options=(), **kw):
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        av, fields = lat.run_sampled(nsteps, every)
        info = {k: lat.info(k) for k in ("engine_last", "samples_in_kernel")}
        st = lat.read_state()
    return av, fields, st, info


# (deck, nsteps, every values): every == 1, and values that do not divide nsteps; short runs on 1024^2
DECK_CASES = [("128x128", 23, (1, 5, 7)), ("128x256", 17, (4, 17)), ("256x256", 14, (3, 7)), ("1024x1024", 9, (1, 4))]


@pytest.mark.gpu
@pytest.mark.parametrize("deck,nsteps,everys", DECK_CASES)
def test_snapshots_equal_separate_runs_on_the_shipped_decks(gpu, deck, nsteps, everys):
    L = gpu
    p, ob = _deck(L, deck)
    with L.Lattice(p, ob) as lat:
        av0 = lat.run(nsteps)
        st0 = lat.read_state()
    for every in everys:
        av_c, want, _ = _chunked(L, p, ob, None, nsteps, every)
        av, fields, st, info = _sampled(L, p, ob, None, nsteps, every)
        # the in-kernel path really ran (the default engine on every shipped deck)
        assert info["engine_last"] == 3 and info["samples_in_kernel"] == 1, (deck, every, info)
        assert fields.shape == (nsteps // every, p.ny, p.nx, 4)
        assert np.array_equal(_bits(fields), _bits(want)), (deck, every)
        # sampling does not perturb the run
        assert np.array_equal(_bits(av), _bits(av0)) and np.array_equal(_bits(st), _bits(st0)), (deck, every)
    # snapshot j against a FRESH context after (j+1) every steps (the last one)
    every = everys[-1]
    m = nsteps // every
    with L.Lattice(p, ob) as lat:
        lat.run(m * every)
        last = lat.final_state()
    _, fields, _, _ = _sampled(L, p, ob, None, nsteps, every)
    assert np.array_equal(_bits(fields[m - 1]), _bits(last))


@pytest.mark.gpu
def test_no_samples_is_lbm_run(gpu):
    L = gpu
    p, ob = _deck(L, "128x128")
    with L.Lattice(p, ob) as lat:
        av0 = lat.run(12)
        st0 = lat.read_state()
    for nsteps, every in ((12, 0), (12, 13)):
        av, fields, st, info = _sampled(L, p, ob, None, nsteps, every)
        assert fields.shape[0] == 0 and info["samples_in_kernel"] == 0 and info["engine_last"] == 3
        assert np.array_equal(_bits(av), _bits(av0)) and np.array_equal(_bits(st), _bits(st0))


# (tile rows, rows per wave, regtile_async, nx, ny): R = 1, 2, 4; the compiler-scheduled and the asynchronous loop
TILINGS = [(16, 1, 0, 128, 16), (8, 2, 0, 128, 16), (8, 2, 1, 128, 16), (8, 4, 0, 256, 256), (8, 4, 1, 256, 256),
           (16, 2, 1, 256, 256), (32, 4, 1, 192, 96), (4, 4, 0, 64, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", TILINGS)
def test_snapshots_of_every_register_tiling(gpu, ty, r, asy, nx, ny):
    L = gpu
    p, ob, cells = _random_case(L, nx, ny, 7)
    nsteps, every = 11, 3
    opts = (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3))
    av_c, want, st_c = _chunked(L, p, ob, cells, nsteps, every)
    av, fields, st, info = _sampled(L, p, ob, cells, nsteps, every, opts)
    assert info["engine_last"] == 3 and info["samples_in_kernel"] == 1
    assert np.array_equal(_bits(fields), _bits(want))
    assert np.array_equal(_bits(st), _bits(st_c))
    _, _, st_plain, _ = _sampled(L, p, ob, cells, nsteps, 0, opts)
    assert np.array_equal(_bits(st), _bits(st_plain))


@pytest.mark.gpu
@pytest.mark.parametrize("time_block", [1, 2, 4, 8])
def test_streaming_engines_give_the_register_tiles_snapshots(gpu, time_block):
    L = gpu
    p, ob = _deck(L, "256x256")
    nsteps = 21
    for every in (3, 8):                 # 3: not a multiple of any time_block > 1
        av_t, want, st_t, info_t = _sampled(L, p, ob, None, nsteps, every)
        assert info_t["samples_in_kernel"] == 1
        av, fields, st, info = _sampled(L, p, ob, None, nsteps, every, (("engine", 1), ("time_block", time_block)))
        assert info["engine_last"] == 1 and info["samples_in_kernel"] == 0
        assert np.array_equal(_bits(fields), _bits(want)), (time_block, every)
        assert np.array_equal(_bits(st), _bits(st_t))
        assert np.allclose(av, av_t, rtol=2e-6, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("deck,nslabs,exchange", [("256x256", 2, "copy"), ("256x256", 4, "copy"), ("256x256", 2, "p2p"),
                                                   ("256x256", 4, "p2p"), ("1024x1024", 2, "p2p")])
def test_slabs_give_the_single_slab_snapshots(gpu, deck, nslabs, exchange):
    L = gpu
    p, ob = _deck(L, deck)
    nsteps, every = 10, 4
    av1, want, st1, _ = _sampled(L, p, ob, None, nsteps, every)
    ex = L.EXCHANGE_COPY if exchange == "copy" else L.EXCHANGE_P2P
    av, fields, st, info = _sampled(L, p, ob, None, nsteps, every, nslabs=nslabs, devices=[0] * nslabs, exchange=ex)
    assert np.array_equal(_bits(fields), _bits(want))
    assert np.array_equal(_bits(st), _bits(st1))
    assert np.allclose(av, av1, rtol=2e-6, atol=0)
    if info["engine_last"] == 3:
        assert info["samples_in_kernel"] == 1
    if exchange == "p2p":                # register tiles across slabs
        assert info["engine_last"] == 3 and info["samples_in_kernel"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["rccl", "p2p"])
def test_rank_context_ring_of_one_gives_the_single_slab_snapshots(gpu, exchange):
    L = gpu
    p, ob = _deck(L, "128x256")
    nsteps, every = 13, 5
    av1, want, st1, _ = _sampled(L, p, ob, None, nsteps, every)
    os.environ["LBM_FORCE_EXCHANGE"] = "1"
    try:
        ex = L.EXCHANGE_RCCL if exchange == "rccl" else L.EXCHANGE_P2P
        av, fields, st, _ = _sampled(L, p, ob, None, nsteps, every, rank=0, nranks=1, device=0,
                                     unique_id=L.rccl_unique_id(), exchange=ex)
    finally:
        del os.environ["LBM_FORCE_EXCHANGE"]
    assert fields.shape == want.shape          # (rank-local rows: the ring of one holds them all)
    assert np.array_equal(_bits(fields), _bits(want))
    assert np.array_equal(_bits(st), _bits(st1))
    assert np.allclose(av, av1, rtol=2e-6, atol=0)


def _oracle_fields(cells, ob, density, rel=2e-5):
    """The fields of write_values() from the oracle's lattice (float64), and the bound on |gpu - oracle| per element that
    follows from every population agreeing to `rel` relative (smoke()'s bar for the lattice): the numerators of u_x, u_y
    carry rel x the sum of their six populations, rho carries rel x rho; plus float32 rounding of the derive itself."""
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


@pytest.mark.gpu
def test_snapshots_against_the_float_oracle(gpu, O, oracle):
    """64 x 40 known-answer lattice, every 5 steps over 10, against fields derived from the strict float oracle's lattice at
    those steps: the lattice to 2e-5 relative, as smoke(), carried through the derive (see _oracle_fields)."""
    L = gpu
    k = load_kat("kat_64x40")
    p = L.Param(int(k["nx"]), int(k["ny"]), 10, int(k["reynolds_dim"]), float(k["density"]), float(k["accel"]),
                float(k["omega"]))
    ob = np.ascontiguousarray(k["obstacles"], dtype=np.int32)
    op = O.OrcParam(p.nx, p.ny, 10, p.reynolds_dim, float(k["density"]), float(k["accel"]), float(k["omega"]))
    ref = k["cells0"].copy()
    wants = []
    for _ in range(2):
        oracle.run(op, ref, ob, 5)
        wants.append(_oracle_fields(ref.reshape(p.ny, p.nx, 9), ob, k["density"]))
    assert np.array_equal(ref, k["cells_after_10"])
    _, fields, st, info = _sampled(L, p, ob, k["cells0"], 10, 5)
    assert info["samples_in_kernel"] == 1
    assert np.all(np.abs(st - ref) <= 2e-5 * np.abs(ref))
    for j, (want, tol) in enumerate(wants):
        err = np.abs(fields[j].astype(np.float64) - want)
        assert np.all(err <= tol), (j, float(np.max(err - tol)))


# torch and the library share libamdhip64: torch is imported FIRST, in a child process of its own
_DEVICE_OUTPUT = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_sampled_run import _deck, _sampled, _bits
p, ob = _deck(L, "128x256")
nsteps, every = 12, 5
av_h, want, st_h, _ = _sampled(L, p, ob, None, nsteps, every)
out = torch.full((nsteps // every, p.ny, p.nx, 4), float("nan"), dtype=torch.float32, device="cuda:0")
with L.Lattice(p, ob) as lat:
    av, got = lat.run_sampled(nsteps, every, out=out)
    assert got is out and lat.info("samples_in_kernel") == 1
    st = lat.read_state()
torch.cuda.synchronize()
assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
assert np.array_equal(_bits(av), _bits(av_h)) and np.array_equal(_bits(st), _bits(st_h))
out.fill_(float("nan"))                   # the streaming engines' pieces, into device memory as well
torch.cuda.synchronize()
with L.Lattice(p, ob) as lat:
    lat.set_option("engine", 1)
    lat.run_sampled(nsteps, every, out=out)
    assert lat.info("samples_in_kernel") == 0
torch.cuda.synchronize()
assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
print("device output ok")
"""

_SPAN = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import ctypes as C
import numpy as np
import advanced_hpc_lbm_amd as L
from test_sampled_run import _deck, _bits
p, ob = _deck(L, "256x256")
with L.Lattice(p, ob, nslabs=2, devices=[0, 1], exchange=L.EXCHANGE_COPY) as lat:
    st0 = lat.read_state()
    out = torch.zeros((2, p.ny, p.nx, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert L.load_library().lbm_run_sampled(lat._ctx, 10, None, 5, C.c_void_p(out.data_ptr())) == 1
    assert np.array_equal(_bits(lat.read_state()), _bits(st0))
print("span ok")
"""


def _child(code):
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", code.format(root=os.path.dirname(tests), tests=tests)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
def test_device_output_is_the_host_output(gpu):
    assert "device output ok" in _child(_DEVICE_OUTPUT)


@pytest.mark.gpu
def test_argument_errors_leave_the_lattice_alone(gpu):
    L = gpu
    lib = L.load_library()
    p, ob = _deck(L, "128x128")
    with L.Lattice(p, ob) as lat:
        lat.run(3)
        st0 = lat.read_state()
        with pytest.raises(L.LbmError):
            lat.run_sampled(10, -1)
        assert lib.lbm_run_sampled(lat._ctx, 10, None, -1, None) == LBM_EINVAL
        assert lib.lbm_run_sampled(lat._ctx, 10, None, 5, None) == LBM_EINVAL      # m = 2, no output
        assert lib.lbm_run_sampled(lat._ctx, 10, None, 11, None) == 0               # m = 0: no output needed
        st1 = lat.read_state()
    with L.Lattice(p, ob) as ref:
        ref.run(13)
        assert np.array_equal(_bits(st1), _bits(ref.read_state()))
    with L.Lattice(p, ob) as lat:
        lat.run(3)
        assert np.array_equal(_bits(lat.read_state()), _bits(st0))
    # staging that cannot be allocated: LBM_ENOMEM before anything runs (the host buffer is never touched)
    p, ob = _deck(L, "1024x1024")
    with L.Lattice(p, ob) as lat:
        assert lat.info("engine_next") == 3
        st0 = lat.read_state()
        small = np.zeros(4, dtype=np.float32)
        # 2^20 snapshots of 16 MiB: 16 TiB of staging
        rc = lib.lbm_run_sampled(lat._ctx, 1 << 20, None, 1, small.ctypes.data)
        assert rc in (LBM_ENOMEM, LBM_EINVAL), rc
        assert np.array_equal(_bits(lat.read_state()), _bits(st0))


@pytest.mark.gpu
def test_device_output_needs_every_slab_on_its_device(gpu):
    if gpu.device_count() < 2:
        pytest.skip("needs two HIP devices")
    assert "span ok" in _child(_SPAN)
