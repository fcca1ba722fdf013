"""lbm_set_probes / lbm_run_probes: per-step time series at chosen cells (Lattice.set_probes, Lattice.run_probes).

Contract (include/lbm_mi355x.h): probes_out[j][p][:] equals fields_out[j][jj_p][ii_p][:] of lbm_run_sampled at the same
`every` from the same state, bit for bit, in the order the probes were given; a probe run leaves av_vels and the lattice
bit-identical to lbm_run.  The register-tile engines take the values inside their kernels (probes_in_kernel = 1); every
other engine runs the steps in pieces with a gather kernel behind each.  Every comparison is on bit patterns unless it
says otherwise."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, deck_paths, load_kat
from test_sampled_run import DECK_CASES, TILINGS
from test_mean_run import _deck, _random_case, _oracle_fields, _kat_case, _plain, _sampled, _child

LBM_EINVAL, LBM_ENOMEM = 1, 5
LBM_MAX_PROBES = 4096
INFO = ("engine_last", "probes_in_kernel")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def awkward_set(nx, ny, ob, ty, r, extra_rows=()):
    """The probe set used throughout, for an nx x ny lattice tiled into 64-column tiles of ty rows, r rows per wave (ty = 0:
    no tiling): the four corners; columns 0, 63, 64, nx - 1 (tile edges: the lanes that carry mail) in rows 0, ny - 2 (the
    accelerate row), ny - 1 and one interior row; the first and last row of a wave and of a tile; several probes per row;
    a blocked cell and a fluid cell beside it (where the obstacle map has such a pair); both columns of `extra_rows`;
    shuffled, so that the order is neither row- nor column-sorted."""
    ob = np.asarray(ob).reshape(ny, nx)
    cols = sorted({0, min(63, nx - 1), min(64, nx - 1), nx - 1})
    interior = min(ny // 2 + 1, ny - 1)
    cells = {(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)}
    for jj in (0, max(ny - 2, 0), ny - 1, interior):
        for ii in cols:
            cells.add((ii, jj))
    if ty > 0:
        t0 = ((ny // ty) // 2) * ty                      # a tile in the middle: its first and last row
        w0 = t0 + ((ty // r) // 2) * r                   # a wave in the middle of it: its first and last row
        for jj in (t0, t0 + ty - 1, w0, w0 + r - 1):
            for ii in (5 % nx, 17 % nx, (nx // 2 + 3) % nx):
                cells.add((ii, jj))
    for jj in extra_rows:
        for ii in (1 % nx, nx - 2):
            cells.add((ii, jj % ny))
    pair = np.argwhere((ob[:, :-1] != 0) & (ob[:, 1:] == 0))
    if len(pair):
        jj, ii = (int(v) for v in pair[len(pair) // 2])
        cells.add((ii, jj))
        cells.add((ii + 1, jj))
    xy = np.array(sorted(cells), dtype=np.int32)
    xy = xy[np.random.default_rng(11).permutation(len(xy))]
    assert np.any(np.diff(xy[:, 0]) < 0) and np.any(np.diff(xy[:, 1]) < 0)          # neither column- nor row-sorted
    assert max(np.bincount(xy[:, 1])) >= 3                                            # at least three probes in one row
    if ty > 0 and nx * ny >= 256 * 256:                                               # tiles without any probe exist
        assert len({(ii // 64, jj // ty) for ii, jj in xy}) < (nx // 64) * (ny // ty)
    return xy


def _pick(fields, xy):                  # fields: (m, ny, nx, 4) from run_sampled -> (m, nprobes, 4)
    return fields[:, xy[:, 1], xy[:, 0], :]


def _tiling(lat):
    v = int(lat.info("regtile"))
    return v // 10, v % 10


def _probes(L, p, ob, cells, nsteps, every, xy=None, options=(), **kw):
    """A fresh context, the options, the probe set (xy = None: the awkward set of the tiling the context runs), one
    run_probes: (av_vels, probes, lattice, info, xy)."""
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        if xy is None:
            ty, r = _tiling(lat)
            xy = awkward_set(p.nx, p.ny, ob, ty, r)
        lat.set_probes(xy)
        av, pr = lat.run_probes(nsteps, every)
        info = {k: lat.info(k) for k in INFO}
        st = lat.read_state()
    return av, pr, st, info, xy


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_probe_run_is_declared_and_bound(L):
    assert "lbm_set_probes" in L.ABI_SYMBOLS and "lbm_run_probes" in L.ABI_SYMBOLS
    hdr = open(L.HEADER_PATH).read()
    assert "#define LBM_MAX_PROBES 4096" in hdr
    assert "int lbm_set_probes(lbm_ctx* ctx, const int* xy, int nprobes);" in hdr
    assert "int lbm_run_probes(lbm_ctx* ctx, int nsteps, float* av_vels, int every, float* probes_out);" in hdr
    assert '"probes_in_kernel"' in hdr
    assert callable(L.Lattice.set_probes) and callable(L.Lattice.run_probes)


def test_probe_calls_reject_a_null_context(L):
    lib = L.load_library()
    assert lib.lbm_set_probes(None, None, 0) == LBM_EINVAL
    assert b"ctx" in lib.lbm_last_error()
    assert lib.lbm_run_probes(None, 10, None, 1, None) == LBM_EINVAL
    assert b"ctx" in lib.lbm_last_error()


def test_isa_audit_covers_the_probe_flavour():
    """tools/audit_regtile_isa.py lists the asynchronous probe-flavour instantiations (mode bit 131072) of lbm_regtile and
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
                key = (name, rr, 131072 | 4096 | slab | fast)
                assert key in seen, (key, r.stdout)
                assert seen[key] == 0, (key, r.stdout)
    assert all(nf == 0 for nf in seen.values()), r.stdout


def _three_rows(p):
    rows = (0, p.ny // 2, p.ny - 2)
    return np.array([(ii, jj) for jj in rows for ii in range(p.nx)], dtype=np.int32)


def test_the_oracles_own_fields_pass_the_probe_bound(L, O, oracle):
    """The bar of test_probes_against_the_float_oracle tests the kernel, not the bound: the strict float oracle's own float32
    final_state values in the probed cells sit inside the per-element bound of _oracle_fields at every step."""
    k, p, ob, op = _kat_case(L, O)
    xy = _three_rows(p)
    ref = k["cells0"].copy()
    worst = 0.0
    for _ in range(10):
        oracle.run(op, ref, ob, 1)
        want, tol = _oracle_fields(ref.reshape(p.ny, p.nx, 9), ob, k["density"])
        own = oracle.final_state(op, ref, ob).reshape(p.ny, p.nx, 4)
        err = np.abs(own[xy[:, 1], xy[:, 0]].astype(np.float64) - want[xy[:, 1], xy[:, 0]])
        lim = tol[xy[:, 1], xy[:, 0]]
        assert np.all(err <= lim), float(np.max(err - lim))
        worst = max(worst, float(np.max(err[lim > 0] / lim[lim > 0])))
    assert np.array_equal(ref, k["cells_after_10"])
    print("oracle's own probes: worst error / bound %.3g" % worst)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("deck,nsteps,everys", DECK_CASES)
def test_probes_are_the_snapshots_cells_on_the_shipped_decks(gpu, deck, nsteps, everys):
    L = gpu
    p, ob = _deck(L, deck)
    av0, st0 = _plain(L, p, ob, None, nsteps)
    for every in everys:
        _, fields, _ = _sampled(L, p, ob, None, nsteps, every)
        av, pr, st, info, xy = _probes(L, p, ob, None, nsteps, every)
        assert info["engine_last"] == 3 and info["probes_in_kernel"] == 1, (deck, every, info)
        assert pr.shape == (nsteps // every, len(xy), 4)
        assert np.array_equal(_bits(pr), _bits(_pick(fields, xy))), (deck, every)
        assert np.array_equal(_bits(av), _bits(av0)) and np.array_equal(_bits(st), _bits(st0)), (deck, every)


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", TILINGS)
def test_probes_of_every_register_tiling(gpu, ty, r, asy, nx, ny):
    L = gpu
    p, ob, cells = _random_case(L, nx, ny, 7)
    nsteps = 11
    opts = (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3))
    xy = awkward_set(nx, ny, ob, ty, r)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts)
    for every in (3, 1):
        _, fields, _ = _sampled(L, p, ob, cells, nsteps, every, opts)
        av, pr, st, info, _ = _probes(L, p, ob, cells, nsteps, every, xy, opts)
        assert info["engine_last"] == 3 and info["probes_in_kernel"] == 1
        assert np.array_equal(_bits(pr), _bits(_pick(fields, xy))), every
        assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(av), _bits(av0))


@pytest.mark.gpu
@pytest.mark.parametrize("asy", [0, 1])
def test_probes_with_ieee_maths(gpu, asy):
    L = gpu
    p, ob, cells = _random_case(L, 256, 256, 7)
    nsteps = 11
    opts = (("regtile", 84), ("regtile_async", asy), ("engine", 3), ("kernel_variant", 0))
    xy = awkward_set(256, 256, ob, 8, 4)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts)
    for every in (3, 1):
        _, fields, _ = _sampled(L, p, ob, cells, nsteps, every, opts)
        av, pr, st, info, _ = _probes(L, p, ob, cells, nsteps, every, xy, opts)
        assert info["engine_last"] == 3 and info["probes_in_kernel"] == 1
        assert np.array_equal(_bits(pr), _bits(_pick(fields, xy))), every
        assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(av), _bits(av0))


@pytest.mark.gpu
@pytest.mark.parametrize("line", ["column", "row"])
def test_a_full_column_and_a_full_row(gpu, line):
    L = gpu
    p, ob = _deck(L, "256x256")
    nsteps = 14
    if line == "column":
        xy = np.array([(p.nx // 2, jj) for jj in range(p.ny)], dtype=np.int32)
    else:
        xy = np.array([(ii, p.ny - 2) for ii in range(p.nx)], dtype=np.int32)
    av0, st0 = _plain(L, p, ob, None, nsteps)
    for every in (3, 1):
        _, fields, _ = _sampled(L, p, ob, None, nsteps, every)
        av, pr, st, info, _ = _probes(L, p, ob, None, nsteps, every, xy)
        assert info["engine_last"] == 3 and info["probes_in_kernel"] == 1
        assert np.array_equal(_bits(pr), _bits(_pick(fields, xy))), (line, every)
        assert np.array_equal(_bits(st), _bits(st0)) and np.array_equal(_bits(av), _bits(av0))


@pytest.mark.gpu
def test_a_blocked_probe_reads_the_constant(gpu):
    L = gpu
    p, ob = _deck(L, "128x128")
    jj, ii = (int(v) for v in np.argwhere(np.asarray(ob).reshape(p.ny, p.nx) != 0)[0])
    xy = np.array([(ii, jj)], dtype=np.int32)
    _, pr, _, info, _ = _probes(L, p, ob, None, 23, 1, xy)
    assert info["probes_in_kernel"] == 1 and pr.shape == (23, 1, 4)
    want = np.array([0.0, 0.0, 0.0, np.float32(p.density) / np.float32(3)], dtype=np.float32)
    assert np.array_equal(_bits(pr), _bits(np.broadcast_to(want, pr.shape)))


@pytest.mark.gpu
def test_one_long_window(gpu):
    """2000 steps, every step a sample, 64 probes: where a cursor that drifts or a staging overrun would show."""
    L = gpu
    p, ob = _deck(L, "128x128")
    nsteps, chunk = 2000, 250
    rng = np.random.default_rng(5)
    flat = rng.choice(p.nx * p.ny, size=64, replace=False)
    xy = np.stack([flat % p.nx, flat // p.nx], axis=1).astype(np.int32)
    want = []
    with L.Lattice(p, ob) as lat:
        for _ in range(nsteps // chunk):
            _, fields = lat.run_sampled(chunk, 1)
            want.append(_pick(fields, xy))
        st0 = lat.read_state()
    want = np.concatenate(want)
    av, pr, st, info, _ = _probes(L, p, ob, None, nsteps, 1, xy)
    assert info["engine_last"] == 3 and info["probes_in_kernel"] == 1
    assert pr.shape == (nsteps, 64, 4)
    assert np.array_equal(_bits(pr), _bits(want))
    assert np.array_equal(_bits(st), _bits(st0))


@pytest.mark.gpu
@pytest.mark.parametrize("time_block", [1, 2, 4, 8])
def test_streaming_engines_give_the_register_tiles_probes(gpu, time_block):
    L = gpu
    p, ob = _deck(L, "256x256")
    nsteps = 21
    for every in (3, 8):                 # 3: not a multiple of any time_block > 1
        av_t, want, st_t, info_t, xy = _probes(L, p, ob, None, nsteps, every)
        assert info_t["probes_in_kernel"] == 1
        av, pr, st, info, _ = _probes(L, p, ob, None, nsteps, every, xy, (("engine", 1), ("time_block", time_block)))
        assert info["engine_last"] == 1 and info["probes_in_kernel"] == 0
        assert np.array_equal(_bits(pr), _bits(want)), (time_block, every)
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
    xy = awkward_set(p.nx, p.ny, ob, 0, 0)
    av0, st0 = _plain(L, p, ob, k["cells0"], nsteps)
    for every in (1, 3):
        _, fields, _ = _sampled(L, p, ob, k["cells0"], nsteps, every)
        av, pr, st, info, _ = _probes(L, p, ob, k["cells0"], nsteps, every, xy)
        assert info["probes_in_kernel"] == 0 and info["engine_last"] == 1
        assert np.array_equal(_bits(pr), _bits(_pick(fields, xy))), every
        assert np.array_equal(_bits(st), _bits(st0))
        assert np.allclose(av, av0, rtol=2e-6, atol=0)


def _slab_set(L, p, ob, nslabs):
    """The awkward set of the single-slab tiling, with probes on both sides of every slab border (the wrap included)."""
    with L.Lattice(p, ob) as lat:
        ty, r = _tiling(lat)
    borders = []
    for k in range(nslabs):
        borders += [k * (p.ny // nslabs) - 1, k * (p.ny // nslabs)]
    return awkward_set(p.nx, p.ny, ob, ty, r, extra_rows=borders)


@pytest.mark.gpu
@pytest.mark.parametrize("deck,nslabs,exchange", [("256x256", 2, "copy"), ("256x256", 4, "copy"), ("256x256", 2, "p2p"),
                                                   ("256x256", 4, "p2p"), ("1024x1024", 2, "p2p")])
def test_slabs_give_the_single_slab_probes(gpu, deck, nslabs, exchange):
    L = gpu
    p, ob = _deck(L, deck)
    nsteps, every = 10, 4
    xy = _slab_set(L, p, ob, nslabs)
    av1, want, st1, _, _ = _probes(L, p, ob, None, nsteps, every, xy)
    ex = L.EXCHANGE_COPY if exchange == "copy" else L.EXCHANGE_P2P
    av, pr, st, info, _ = _probes(L, p, ob, None, nsteps, every, xy, nslabs=nslabs, devices=[0] * nslabs, exchange=ex)
    assert np.array_equal(_bits(pr), _bits(want))
    assert np.array_equal(_bits(st), _bits(st1))
    assert np.allclose(av, av1, rtol=2e-6, atol=0)
    if info["engine_last"] == 3:
        assert info["probes_in_kernel"] == 1
    if exchange == "p2p":                # register tiles across slabs
        assert info["engine_last"] == 3 and info["probes_in_kernel"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["rccl", "p2p"])
def test_rank_context_ring_of_one_gives_the_single_slab_probes(gpu, exchange):
    L = gpu
    p, ob = _deck(L, "128x256")
    nsteps, every = 13, 5
    av1, want, st1, _, xy = _probes(L, p, ob, None, nsteps, every)
    os.environ["LBM_FORCE_EXCHANGE"] = "1"
    try:
        ex = L.EXCHANGE_RCCL if exchange == "rccl" else L.EXCHANGE_P2P
        av, pr, st, _, _ = _probes(L, p, ob, None, nsteps, every, xy, rank=0, nranks=1, device=0,
                                   unique_id=L.rccl_unique_id(), exchange=ex)
    finally:
        del os.environ["LBM_FORCE_EXCHANGE"]
    assert np.array_equal(_bits(pr), _bits(want))
    assert np.array_equal(_bits(st), _bits(st1))
    assert np.allclose(av, av1, rtol=2e-6, atol=0)


# torch and the library share libamdhip64: torch is imported FIRST, in a child process of its own
_DEVICE_OUTPUT = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_probe_run import _deck, _probes, _bits
p, ob = _deck(L, "128x256")
nsteps, every = 12, 5
av_h, want, st_h, info_h, xy = _probes(L, p, ob, None, nsteps, every)
assert info_h["probes_in_kernel"] == 1
out = torch.full((nsteps // every, len(xy), 4), float("nan"), dtype=torch.float32, device="cuda:0")
with L.Lattice(p, ob) as lat:
    lat.set_probes(xy)
    av, got = lat.run_probes(nsteps, every, out=out)
    assert got is out and lat.info("probes_in_kernel") == 1
    st = lat.read_state()
torch.cuda.synchronize()
assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
assert np.array_equal(_bits(av), _bits(av_h)) and np.array_equal(_bits(st), _bits(st_h))
out.fill_(float("nan"))                   # the streaming engines' pieces, into device memory as well
torch.cuda.synchronize()
with L.Lattice(p, ob) as lat:
    lat.set_option("engine", 1)
    lat.set_probes(xy)
    _, got = lat.run_probes(nsteps, every, out=out)
    assert got is out and lat.info("probes_in_kernel") == 0
torch.cuda.synchronize()
assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
print("device output ok")
"""


@pytest.mark.gpu
def test_device_output_is_the_host_output(gpu):
    assert "device output ok" in _child(_DEVICE_OUTPUT)


@pytest.mark.gpu
def test_refusals_leave_the_lattice_and_the_set_alone(gpu):
    L = gpu
    lib = L.load_library()
    p, ob = _deck(L, "128x128")
    xy = np.array([(3, 5), (64, 126), (127, 0)], dtype=np.int32)
    out = np.zeros((10, 3, 4), np.float32)

    def refused(rc, *words):
        assert rc == LBM_EINVAL
        msg = lib.lbm_last_error().decode()
        for w in words:
            assert w in msg, (w, msg)

    with L.Lattice(p, ob) as lat:
        lat.run(3)
        refused(lib.lbm_run_probes(lat._ctx, 10, None, 1, out.ctypes.data), "probes")          # no probes set yet
        lat.set_probes(xy)
        big = np.zeros((LBM_MAX_PROBES + 1, 2), np.int32)
        refused(lib.lbm_set_probes(lat._ctx, big.ctypes.data, -1), "nprobes")
        refused(lib.lbm_set_probes(lat._ctx, big.ctypes.data, LBM_MAX_PROBES + 1), "nprobes")
        refused(lib.lbm_set_probes(lat._ctx, None, 2), "xy")
        for bad in ((-1, 0), (p.nx, 0), (0, -1), (0, p.ny)):
            one = np.array([(1, 1), bad], dtype=np.int32)
            refused(lib.lbm_set_probes(lat._ctx, one.ctypes.data, 2), "xy[1]")
        twice = np.array([(7, 9), (1, 1), (8, 9), (7, 9)], dtype=np.int32)
        refused(lib.lbm_set_probes(lat._ctx, twice.ctypes.data, 4), "xy[0]", "xy[3]")
        with pytest.raises(L.LbmError):
            lat.set_probes(twice)
        with pytest.raises(L.LbmError):
            lat.run_probes(10, 0)
        refused(lib.lbm_run_probes(lat._ctx, 10, None, 0, out.ctypes.data), "every")
        refused(lib.lbm_run_probes(lat._ctx, 10, None, -1, out.ctypes.data), "every")
        refused(lib.lbm_run_probes(lat._ctx, 10, None, 11, out.ctypes.data), "every", "nsteps")    # m = 0
        refused(lib.lbm_run_probes(lat._ctx, 10, None, 5, None), "probes_out")
        refused(lib.lbm_run_probes(lat._ctx, -1, None, 1, out.ctypes.data), "nsteps")
        assert not out.any()
        av = lat.run(10)
        st1 = lat.read_state()
        _, pr = lat.run_probes(6, 2)                   # the earlier set is still there
        assert pr.shape == (3, 3, 4)
    with L.Lattice(p, ob) as ref:
        av_ref = ref.run(13)
        assert np.array_equal(_bits(st1), _bits(ref.read_state()))
        assert np.array_equal(_bits(av), _bits(av_ref[3:]))
        _, fields = ref.run_sampled(6, 2)
    assert np.array_equal(_bits(pr), _bits(_pick(fields, xy)))


@pytest.mark.gpu
def test_the_largest_set_is_accepted(gpu):
    L = gpu
    lib = L.load_library()
    p, ob = _deck(L, "128x128")
    flat = np.random.default_rng(3).permutation(p.nx * p.ny)[:LBM_MAX_PROBES + 1]
    xy = np.stack([flat % p.nx, flat // p.nx], axis=1).astype(np.int32)
    with L.Lattice(p, ob) as lat:
        assert lib.lbm_set_probes(lat._ctx, xy.ctypes.data, LBM_MAX_PROBES + 1) == LBM_EINVAL
        lat.set_probes(xy[:LBM_MAX_PROBES])
        _, pr = lat.run_probes(5, 2)
        assert lat.info("probes_in_kernel") == 1
    _, fields, _ = _sampled(L, p, ob, None, 5, 2)
    assert np.array_equal(_bits(pr), _bits(_pick(fields, xy[:LBM_MAX_PROBES])))


@pytest.mark.gpu
def test_one_context_through_mixed_calls(gpu):
    L = gpu
    p, ob = _deck(L, "128x256")
    with L.Lattice(p, ob) as lat:
        ty, r = _tiling(lat)
        other = (8, 2) if (ty, r) != (8, 2) else (16, 4)
        xy_a = awkward_set(p.nx, p.ny, ob, ty, r)
        xy_b = awkward_set(p.nx, p.ny, ob, *other)[::-1][:-3].copy()
        assert not np.array_equal(xy_a, xy_b)
        lat.set_probes(xy_a)
        a, pr1 = lat.run_probes(9, 2)
        avs = [a]
        assert lat.info("probes_in_kernel") == 1
        a, _ = lat.run_mean(8, 3)
        avs.append(a)
        lat.set_probes(xy_b)
        lat.set_option("regtile", other[0] * 10 + other[1])
        a, pr2 = lat.run_probes(11, 4)
        avs.append(a)
        assert lat.info("probes_in_kernel") == 1 and lat.info("engine_last") == 3
        lat.set_probes(None)
        avs.append(lat.run(5))
        with pytest.raises(L.LbmError):
            lat.run_probes(4, 1)
        st = lat.read_state()
    # (a tiling adds its tiles' speed sums in its own order, and a launch folds its last step's sum with another instruction
    # sequence than the steps before it: the reference is plain runs of the same lengths under the same tilings)
    with L.Lattice(p, ob) as ref:
        av_ref = [ref.run(9), ref.run(8)]
        ref.set_option("regtile", other[0] * 10 + other[1])
        av_ref = np.concatenate(av_ref + [ref.run(11), ref.run(5)])
        assert np.array_equal(_bits(st), _bits(ref.read_state()))
        assert np.array_equal(_bits(np.concatenate(avs)), _bits(av_ref))
    with L.Lattice(p, ob) as fresh:
        _, fields = fresh.run_sampled(9, 2)
    assert np.array_equal(_bits(pr1), _bits(_pick(fields, xy_a)))
    with L.Lattice(p, ob) as fresh:
        fresh.run(17)
        _, fields = fresh.run_sampled(11, 4)
    assert np.array_equal(_bits(pr2), _bits(_pick(fields, xy_b)))


@pytest.mark.gpu
def test_probes_against_the_float_oracle(gpu, O, oracle):
    """64 x 40 known-answer lattice, 10 steps, every step a sample, every cell of three rows a probe, against fields derived
    from the strict float oracle's lattice at each step: the lattice to 2e-5 relative, as smoke(), carried through the
    derive -- the per-element bound of _oracle_fields, derived, not tuned."""
    L = gpu
    k, p, ob, op = _kat_case(L, O)
    xy = _three_rows(p)
    _, pr, st, info, _ = _probes(L, p, ob, k["cells0"], 10, 1, xy)
    assert info["probes_in_kernel"] == 1
    ref = k["cells0"].copy()
    for j in range(10):
        oracle.run(op, ref, ob, 1)
        want, tol = _oracle_fields(ref.reshape(p.ny, p.nx, 9), ob, k["density"])
        err = np.abs(pr[j].astype(np.float64) - want[xy[:, 1], xy[:, 0]])
        lim = tol[xy[:, 1], xy[:, 0]]
        print("step %d: max error %.3g, worst error - bound %.3g" % (j + 1, err.max(), np.max(err - lim)))
        assert np.all(err <= lim), (j, float(np.max(err - lim)))
    assert np.array_equal(ref, k["cells_after_10"])
    assert np.all(np.abs(st - ref) <= 2e-5 * np.abs(ref))
