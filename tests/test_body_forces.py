"""lbm_run_forces: drag and lift on labelled bodies, step by step (Lattice.set_bodies / Lattice.run_forces).

Contract (include/lbm_mi355x.h): F_b(t) = 2 sum over the blocked cells B of label b, over the directions i whose source cell
B - c_i is fluid, of c_i f~_i(B, t), where f~_i(B, t) -- the population B pulled along i in step t -- is plane opp(i) of B in
the lattice stored after step t.  So the forces follow from lbm_read_state alone (forces_from_state below), and a forces run
leaves av_vels and the lattice bit-identical to lbm_run.  The register tiles take the sums inside their kernels
(forces_in_kernel = 1); every other engine runs the one-step kernel with a force kernel behind each step, so where lbm_run
would take several steps per launch, av_vels is the one-step kernel's: lbm_run's to float rounding."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, deck_paths

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden import PARAM_GRID, accel_weights, param_state, refused  # noqa: E402

LBM_EINVAL, LBM_ENOMEM = 1, 5
# directions 1..8: E N W S NE NW SW SE (index 0: rest)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])
OPP = np.array([0, 3, 4, 1, 2, 7, 8, 5, 6])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def forces_from_state(lattice, obstacles, body, nbodies):
    """(F[nbodies, 2], A[nbodies, 2]) from a stored lattice (ny, nx, 9): F by the definition, in float64; A = the same sum
    of absolute contributions, the scale of the rounding of any float32 evaluation."""
    lat = np.asarray(lattice, dtype=np.float64).reshape(obstacles.shape + (9,))
    blocked = np.asarray(obstacles) != 0
    F = np.zeros((nbodies, 2))
    A = np.zeros((nbodies, 2))
    for i in range(1, 9):
        fluid_src = np.roll(~blocked, shift=(CY[i], CX[i]), axis=(0, 1))     # [y, x] = fluid at (x - cx, y - cy)
        link = blocked & fluid_src
        v = lat[..., OPP[i]]
        for b in range(nbodies):
            s = v[link & (body == b + 1)].sum()
            a = np.abs(v[link & (body == b + 1)]).sum()
            F[b] += 2.0 * s * np.array([CX[i], CY[i]])
            A[b] += 2.0 * a * np.abs(np.array([CX[i], CY[i]]))
    return F, A


def momentum_fluid(lattice, obstacles):
    lat = np.asarray(lattice, dtype=np.float64).reshape(obstacles.shape + (9,))
    fl = np.asarray(obstacles) == 0
    return np.array([(lat[fl] * CX).sum(), (lat[fl] * CY).sum()])


def momentum_out_of_blocked(lattice, obstacles):
    """E0: sum of c_i f_i(B) over the links from blocked B to fluid B + c_i."""
    lat = np.asarray(lattice, dtype=np.float64).reshape(obstacles.shape + (9,))
    blocked = np.asarray(obstacles) != 0
    e = np.zeros(2)
    for i in range(1, 9):
        dst_fluid = np.roll(~blocked, shift=(-CY[i], -CX[i]), axis=(0, 1))   # [y, x] = fluid at (x + cx, y + cy)
        e += lat[..., i][blocked & dst_fluid].sum() * np.array([CX[i], CY[i]])
    return e


def _balance(F, accel_x, P0, PT, E0):
    """Both sides of  sum F(t) = sum (A(t), 0) - (P(T) - P(0)) + F(T)/2 + E0  (F: [T, 2], accel_x: [T])."""
    lhs = F.sum(axis=0)
    rhs = np.array([accel_x.sum(), 0.0]) - (PT - P0) + F[-1] / 2 + E0
    return lhs, rhs


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_forces_are_declared_and_bound(L):
    hdr = open(L.HEADER_PATH).read()
    for sym, decl in (("lbm_set_bodies", "int lbm_set_bodies(lbm_ctx* ctx, const int* body, int nbodies);"),
                      ("lbm_run_forces", "int lbm_run_forces(lbm_ctx* ctx, int nsteps, float* av_vels, float* forces);")):
        assert sym in L.ABI_SYMBOLS and decl in hdr
        getattr(L.load_library(), sym)
    assert "#define LBM_MAX_BODIES 4" in hdr and '"forces_in_kernel"' in hdr
    assert "F_b(t) = 2 * Σ_{B blocked, label(B) = b}  Σ_{i = 1..8 : cell B - c_i is fluid}  c_i * f~_i(B, t)" in hdr
    assert hasattr(L.Lattice, "set_bodies") and hasattr(L.Lattice, "run_forces")


def test_forces_reject_a_null_context(L):
    lib = L.load_library()
    assert lib.lbm_set_bodies(None, None, 0) == LBM_EINVAL
    assert lib.lbm_run_forces(None, 10, None, None) == LBM_EINVAL
    assert b"ctx" in lib.lbm_last_error()


def test_reference_forces_balance_momentum_on_the_double_oracle(L, O, oracle):
    """200 steps of the 128 x 128 deck in float64, every blocked cell labelled 1: the momentum balance to 1e-10."""
    pf, of = deck_paths("128x128")
    p = L.read_params(pf)
    ob = np.ascontiguousarray(L.read_obstacles(of, p), dtype=np.int32).reshape(p.ny, p.nx)
    prm = O.OrcParam(p.nx, p.ny, 1, p.reynolds_dim, p.density, p.accel, p.omega)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
    cells = np.ascontiguousarray(np.broadcast_to(p.density * w, (p.ny, p.nx, 9)), dtype=np.float64)
    a1, a2 = p.density * p.accel / 9.0, p.density * p.accel / 36.0
    body = (ob != 0).astype(np.int32)
    P0, E0 = momentum_fluid(cells, ob), momentum_out_of_blocked(cells, ob)
    F, acc = [], []
    for _ in range(200):
        row = cells[-2]
        ok = (ob[-2] == 0) & (row[:, 3] - a1 > 0) & (row[:, 6] - a2 > 0) & (row[:, 7] - a2 > 0)
        acc.append(int(ok.sum()) * (2 * a1 + 4 * a2))
        oracle.run(prm, cells, ob, 1)
        F.append(forces_from_state(cells, ob, body, 1)[0][0])
    F = np.array(F)
    assert np.all(np.isfinite(F)) and F[-1, 0] > 0          # drag on the body, along the +x acceleration
    lhs, rhs = _balance(F, np.array(acc), P0, momentum_fluid(cells, ob), E0)
    scale = np.abs(F).sum(axis=0).max()
    assert np.all(np.abs(lhs - rhs) <= 1e-10 * scale), (lhs, rhs)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _deck(L, deck):
    pf, of = deck_paths(deck)
    p = L.read_params(pf)
    return p, np.ascontiguousarray(L.read_obstacles(of, p), dtype=np.int32).reshape(p.ny, p.nx)


def _walls(ob):
    w = np.zeros(ob.shape, dtype=bool)
    w[0] = ob[0] != 0
    w[-1] = ob[-1] != 0
    return w


def _labellings(ob):
    """bodies = the non-wall obstacle cells, the walls, and both (1 and 2)."""
    blocked, walls = ob != 0, _walls(ob)
    obstacle = (blocked & ~walls).astype(np.int32)
    both = np.where(walls, 1, np.where(blocked, 2, 0)).astype(np.int32)
    return [("obstacle", obstacle, 1), ("walls", walls.astype(np.int32), 1), ("both", both, 2)]


def _random_case(L, nx, ny, seed, blocked=0.1):
    rng = np.random.default_rng(seed)
    p = L.Param(nx, ny, 100, 10, 0.1, 0.01, 1.85)
    ob = (rng.random((ny, nx)) < blocked).astype(np.int32)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float32)
    cells = (0.1 * w * (1.0 + 0.2 * (rng.random((ny, nx, 9), dtype=np.float32) - 0.5))).astype(np.float32)
    body = np.where(ob != 0, rng.integers(0, 5, size=ob.shape), 0).astype(np.int32)
    return p, ob, cells, body


def _per_step(L, p, ob, cells, body, nb, nsteps, **kw):
    """n x (run(1) + read_state) and the numpy forces of each state: (F[n, nb, 2], scale[n, nb, 2], av, final state)."""
    F, S, av = [], [], []
    with L.Lattice(p, ob, cells, **kw) as lat:
        for _ in range(nsteps):
            av.append(lat.run(1))
            st = lat.read_state()
            f, a = forces_from_state(st, ob, body, nb)
            F.append(f)
            S.append(a)
    return np.array(F), np.array(S), np.concatenate(av), st


def _forces(L, p, ob, cells, body, nb, nsteps, options=(), **kw):
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        lat.set_bodies(body, nb)
        av, F = lat.run_forces(nsteps)
        info = {k: lat.info(k) for k in ("engine_last", "forces_in_kernel")}
        st = lat.read_state()
    return av, F, st, info


def _plain(L, p, ob, cells, nsteps, options=(), **kw):
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        av = lat.run(nsteps)
        return av, lat.read_state()


def _close(F, want, scale):
    return np.all(np.abs(np.asarray(F, np.float64) - want) <= 1e-5 * scale + 1e-30)


DECK_STEPS = [("128x128", 30), ("128x256", 20), ("256x256", 20), ("1024x1024", 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("deck,nsteps", DECK_STEPS)
def test_forces_against_the_per_step_reference_on_the_shipped_decks(gpu, deck, nsteps):
    L = gpu
    p, ob = _deck(L, deck)
    av0, st0 = _plain(L, p, ob, None, nsteps)
    for name, body, nb in _labellings(ob):
        want, scale, _, _ = _per_step(L, p, ob, None, body, nb, nsteps)
        av, F, st, info = _forces(L, p, ob, None, body, nb, nsteps)
        assert info["engine_last"] == 3 and info["forces_in_kernel"] == 1, (deck, name, info)
        assert F.shape == (nsteps, nb, 2)
        assert _close(F, want, scale), (deck, name, np.abs(F - want).max())
        assert np.array_equal(_bits(av), _bits(av0)) and np.array_equal(_bits(st), _bits(st0)), (deck, name)
    if deck == "128x128":
        assert want[-1, 0, 0] != 0.0


TILINGS = [(16, 1, 0, 128, 16), (8, 2, 0, 128, 16), (8, 2, 1, 128, 16), (8, 4, 0, 256, 256), (8, 4, 1, 256, 256),
           (16, 2, 1, 256, 256), (32, 4, 1, 192, 96), (4, 4, 0, 64, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", TILINGS)
def test_forces_of_every_register_tiling(gpu, ty, r, asy, nx, ny):
    L = gpu
    p, ob, cells, body = _random_case(L, nx, ny, 7)
    nsteps = 11
    opts = (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3))
    want, scale, _, _ = _per_step(L, p, ob, cells, body, 4, nsteps)
    av0, st0 = _plain(L, p, ob, cells, nsteps, opts)
    av, F, st, info = _forces(L, p, ob, cells, body, 4, nsteps, opts)
    assert info["engine_last"] == 3 and info["forces_in_kernel"] == 1
    assert _close(F, want, scale), np.abs(F - want).max()
    assert np.array_equal(_bits(av), _bits(av0)) and np.array_equal(_bits(st), _bits(st0))


@pytest.mark.gpu
@pytest.mark.parametrize("time_block", [1, 2, 4, 6, 8])
def test_streaming_engines_give_the_register_tile_forces(gpu, time_block):
    L = gpu
    p, ob = _deck(L, "256x256")
    body = _labellings(ob)[2][1]
    nsteps = 21
    _, scale, _, _ = _per_step(L, p, ob, None, body, 2, nsteps)
    av_t, F_t, st_t, info_t = _forces(L, p, ob, None, body, 2, nsteps)
    assert info_t["forces_in_kernel"] == 1
    opts = (("engine", 1), ("time_block", time_block))
    av0, st0 = _plain(L, p, ob, None, nsteps, opts)
    av, F, st, info = _forces(L, p, ob, None, body, 2, nsteps, opts)
    assert info["engine_last"] == 1 and info["forces_in_kernel"] == 0
    assert _close(F, F_t, scale)
    assert np.array_equal(_bits(st), _bits(st_t)) and np.array_equal(_bits(st), _bits(st0))
    # av_vels: the one-step kernel's, which sums a step's speeds in the order of its own blocks -- lbm_run's exactly at
    # time_block 1, within rounding of the multi-step kernels' sums otherwise (the lattices are the same bits)
    if time_block == 1:
        assert np.array_equal(_bits(av), _bits(av0))
    assert np.allclose(av, av0, rtol=2e-6, atol=0) and np.allclose(av, av_t, rtol=2e-6, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("nslabs,exchange", [(2, "copy"), (4, "copy"), (2, "p2p"), (4, "p2p")])
def test_slabs_give_the_single_slab_forces(gpu, nslabs, exchange):
    L = gpu
    p, ob = _deck(L, "256x256")
    body = _labellings(ob)[2][1]
    nsteps = 10
    _, scale, _, _ = _per_step(L, p, ob, None, body, 2, nsteps)
    _, F1, st1, _ = _forces(L, p, ob, None, body, 2, nsteps)
    ex = L.EXCHANGE_COPY if exchange == "copy" else L.EXCHANGE_P2P
    kw = dict(nslabs=nslabs, devices=[0] * nslabs, exchange=ex)
    av0, st0 = _plain(L, p, ob, None, nsteps, **kw)
    av, F, st, info = _forces(L, p, ob, None, body, 2, nsteps, **kw)
    assert _close(F, F1, scale)
    assert np.array_equal(_bits(st), _bits(st1)) and np.array_equal(_bits(st), _bits(st0))
    assert np.array_equal(_bits(av), _bits(av0))
    assert info["forces_in_kernel"] == (1 if info["engine_last"] == 3 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["rccl", "p2p"])
def test_rank_context_ring_of_one_gives_the_single_slab_forces(gpu, exchange):
    L = gpu
    p, ob = _deck(L, "128x256")
    body = _labellings(ob)[2][1]
    nsteps = 13
    _, scale, _, _ = _per_step(L, p, ob, None, body, 2, nsteps)
    _, F1, st1, _ = _forces(L, p, ob, None, body, 2, nsteps)
    os.environ["LBM_FORCE_EXCHANGE"] = "1"
    try:
        ex = L.EXCHANGE_RCCL if exchange == "rccl" else L.EXCHANGE_P2P
        kw = dict(rank=0, nranks=1, device=0, exchange=ex)
        av0, st0 = _plain(L, p, ob, None, nsteps, unique_id=L.rccl_unique_id(), **kw)    # (one id per communicator)
        av, F, st, info = _forces(L, p, ob, None, body, 2, nsteps, unique_id=L.rccl_unique_id(), **kw)
    finally:
        del os.environ["LBM_FORCE_EXCHANGE"]
    assert _close(F, F1, scale)
    assert np.array_equal(_bits(st), _bits(st1)) and np.array_equal(_bits(st), _bits(st0))
    # av_vels: lbm_run's bits where the same kernel runs (register tiles across slabs); under RCCL lbm_run takes two steps per
    # launch and the forces run one, whose per-step speed sums agree to rounding (see the streaming-engine test)
    if info["engine_last"] == 3:
        assert info["forces_in_kernel"] == 1 and np.array_equal(_bits(av), _bits(av0))
    assert np.allclose(av, av0, rtol=2e-6, atol=0)


@pytest.mark.gpu
def test_labels_split_permute_and_ignore_fluid(gpu):
    L = gpu
    p, ob = _deck(L, "128x128")
    nsteps = 25
    blocked, walls = ob != 0, _walls(ob)
    _, F_all, _, _ = _forces(L, p, ob, None, blocked.astype(np.int32), 1, nsteps)
    split = np.where(walls, 1, np.where(blocked, 2, 0)).astype(np.int32)
    _, scale, _, _ = _per_step(L, p, ob, None, blocked.astype(np.int32), 1, nsteps)
    _, F_split, _, _ = _forces(L, p, ob, None, split, 2, nsteps)
    assert _close(F_split.sum(axis=1, keepdims=True), F_all, scale)
    # permuting the labels permutes the output
    rng = np.random.default_rng(3)
    lab = np.where(blocked, rng.integers(1, 5, size=ob.shape), 0).astype(np.int32)
    _, F4, _, _ = _forces(L, p, ob, None, lab, 4, nsteps)
    perm = np.array([0, 3, 1, 4, 2])                   # label k -> perm[k]
    _, F4p, _, _ = _forces(L, p, ob, None, perm[lab].astype(np.int32), 4, nsteps)
    for k in range(1, 5):
        assert np.array_equal(_bits(F4p[:, perm[k] - 1]), _bits(F4[:, k - 1]))
    # labels on fluid cells change nothing
    noisy = np.where(blocked, lab, rng.integers(0, 5, size=ob.shape)).astype(np.int32)
    _, F4n, _, _ = _forces(L, p, ob, None, noisy, 4, nsteps)
    assert np.array_equal(_bits(F4n), _bits(F4))


def _gpu_balance(L, O, p, ob, cells0, nsteps, opts=()):
    """The momentum balance of a GPU forces run (every blocked cell labelled 1), A(t) counted on the float oracle."""
    prm = O.OrcParam(p.nx, p.ny, 1, p.reynolds_dim, p.density, p.accel, p.omega)
    a1, a2 = accel_weights(p.density, p.accel)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float32)
    c = (np.ascontiguousarray(cells0, dtype=np.float32).reshape(p.ny, p.nx, 9).copy() if cells0 is not None
         else np.ascontiguousarray(np.broadcast_to(np.float32(p.density) * w, (p.ny, p.nx, 9)), dtype=np.float32))
    start = c.copy()
    acc = []
    orc = O.Oracle("strict")
    for _ in range(nsteps):
        acc.append((int((ob[-2] == 0).sum()) - int(refused(p.density, p.accel, ob, c).sum())) * (2.0 * a1 + 4.0 * a2))
        orc.run(prm, c, ob, 1)
    body = (ob != 0).astype(np.int32)
    _, F, st, info = _forces(L, p, ob, start if cells0 is not None else None, body, 1, nsteps, opts)
    F = F[:, 0].astype(np.float64)
    lhs, rhs = _balance(F, np.array(acc, dtype=np.float64), momentum_fluid(start, ob), momentum_fluid(st, ob),
                        momentum_out_of_blocked(start, ob))
    return lhs, rhs, F, acc


@pytest.mark.gpu
def test_momentum_balance_over_a_long_gpu_run(gpu, O):
    L = gpu
    p, ob = _deck(L, "128x128")
    lhs, rhs, F, _ = _gpu_balance(L, O, p, ob, None, 2000)
    assert F[-1, 0] > 0
    assert np.all(np.abs(lhs - rhs) <= 1e-4 * np.abs(lhs).max()), (lhs, rhs)


@pytest.mark.gpu
def test_momentum_balance_where_the_guard_refuses(gpu, O):
    L = gpu
    nx, ny = 128, 64
    ob, cells = param_state("refusal", nx, ny, 1, "rest")
    ob = np.ascontiguousarray(ob, dtype=np.int32).reshape(ny, nx)
    density, accel, omega = PARAM_GRID["refusal"]
    p = L.Param(nx, ny, 40, 10, density, accel, omega)
    lhs, rhs, F, acc = _gpu_balance(L, O, p, ob, cells, 40)
    a1, a2 = accel_weights(density, accel)
    full = int((ob[-2] == 0).sum()) * (2.0 * a1 + 4.0 * a2)
    assert min(acc) < full                            # the guard did refuse cells
    assert np.all(np.abs(lhs - rhs) <= 1e-4 * np.abs(lhs).max()), (lhs, rhs)


@pytest.mark.gpu
def test_argument_errors_leave_the_lattice_alone(gpu):
    L = gpu
    lib = L.load_library()
    p, ob = _deck(L, "128x128")
    body = (ob != 0).astype(np.int32)
    out = np.zeros((10, 4, 2), dtype=np.float32)
    with L.Lattice(p, ob) as lat:
        lat.run(3)
        st0 = lat.read_state()
        assert lib.lbm_run_forces(lat._ctx, 10, None, out.ctypes.data) == LBM_EINVAL          # no bodies set
        bad = body * 3
        assert lib.lbm_set_bodies(lat._ctx, bad.ctypes.data, 2) == LBM_EINVAL                # label 3 > nbodies
        neg = -body
        assert lib.lbm_set_bodies(lat._ctx, neg.ctypes.data, 1) == LBM_EINVAL
        assert lib.lbm_set_bodies(lat._ctx, body.ctypes.data, 5) == LBM_EINVAL               # > LBM_MAX_BODIES
        assert lib.lbm_run_forces(lat._ctx, 10, None, out.ctypes.data) == LBM_EINVAL          # (still none)
        assert lib.lbm_set_bodies(lat._ctx, body.ctypes.data, 1) == 0
        assert lib.lbm_run_forces(lat._ctx, 10, None, None) == LBM_EINVAL                     # NULL forces
        assert lib.lbm_set_bodies(lat._ctx, None, 0) == 0                                     # cleared
        assert lib.lbm_run_forces(lat._ctx, 10, None, out.ctypes.data) == LBM_EINVAL
        assert np.array_equal(_bits(lat.read_state()), _bits(st0))
        assert lib.lbm_set_bodies(lat._ctx, body.ctypes.data, 1) == 0
        assert lib.lbm_run_forces(lat._ctx, 0, None, None) == 0                               # nothing to write
        assert np.array_equal(_bits(lat.read_state()), _bits(st0))
