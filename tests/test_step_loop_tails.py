"""The step loop's tails under every halo transport, with forces and schedules: groups of K steps, then a pair, then a
single step (K + 3 steps), and two groups with a single step behind them (2 K + 1), through lbm_run, lbm_run_forces and
lbm_run_driven, on a lattice alone, on two slabs with copies and with peer-to-peer halos, and on rank rings of one over RCCL
and peer-to-peer.  256 x 64 is the smallest lattice at which lbm_march runs across two slabs.  The reference of every case
is the same call on the lattice alone at time_block 1, computed once per call and step count."""
import os

import numpy as np
import pytest

from test_body_forces import _close, _per_step
from test_driven_run import AV_RTOL
from test_gpu_parity import _random_case
from test_param_space import ENGINE_AV_RTOL

NX, NY, BORDER = 256, 64, 32            # two slabs: rows 0..31 and 32..63
CONTEXTS = ["alone", "copy2", "p2p2", "rccl_ring", "p2p_ring"]
CALLS = ["run", "run_forces", "run_driven"]
# time_block 4 is run where the context reports it active (never forced), 8 on the lattice alone; where 4 must be active
# for the test to mean anything (the marching kernels across slabs are what it is about) it is asserted
MARCHES_AT_4 = {"alone": True, "copy2": True, "p2p2": True, "p2p_ring": True, "rccl_ring": False}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _case(L):
    p, ob, cells = _random_case(L, NX, NY, 21)
    ob[BORDER - 2:BORDER + 2, 100:104] = 1          # one body of 16 blocked cells, two rows either side of the slab border
    body = np.zeros((NY, NX), np.int32)
    body[BORDER - 2:BORDER + 2, 100:104] = 1
    return p, ob, cells, body


def _schedule(p, n):
    """n accelerations that all differ, around the deck's own."""
    return (np.float32(p.accel) * (1.0 + 0.05 * np.arange(1, n + 1))).astype(np.float32)


def _context(L, kind, p, ob, cells):
    if kind == "alone":
        return L.Lattice(p, ob, cells)
    if kind in ("copy2", "p2p2"):
        return L.Lattice(p, ob, cells, nslabs=2, devices=[0, 0], exchange=L.EXCHANGE_COPY if kind == "copy2" else L.EXCHANGE_P2P)
    ex = L.EXCHANGE_RCCL if kind == "rccl_ring" else L.EXCHANGE_P2P
    os.environ["LBM_FORCE_EXCHANGE"] = "1"          # (read at create: a ring of one trades halos with itself)
    try:
        return L.Lattice(p, ob, cells, rank=0, nranks=1, device=0, unique_id=L.rccl_unique_id(), exchange=ex)
    finally:
        del os.environ["LBM_FORCE_EXCHANGE"]


def _call(lat, call, p, n):
    """(av_vels, forces or None, state) of one call of n steps."""
    F = None
    if call == "run":
        av = lat.run(n)
    elif call == "run_forces":
        av, F = lat.run_forces(n)
    else:
        av = lat.run_driven(_schedule(p, n))
    assert lat.info("engine_last") == 1
    return av, F, lat.read_state()


_REFERENCE = {}


def _reference(L, call, n):
    """The call on the lattice alone at time_block 1, and (forces) the scale of _close: computed once, never changed."""
    if (call, n) not in _REFERENCE:
        p, ob, cells, body = _case(L)
        with L.Lattice(p, ob, cells) as lat:
            lat.set_option("engine", 1)
            lat.set_option("time_block", 1)
            lat.set_bodies(body, 1)
            av, F, st = _call(lat, call, p, n)
        scale = _per_step(L, p, ob, cells, body, 1, n)[1] if call == "run_forces" else None
        for a in (av, F, st, scale):
            if a is not None:
                a.setflags(write=False)
        _REFERENCE[(call, n)] = (av, F, st, scale)
    return _REFERENCE[(call, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("kind", CONTEXTS)
def test_tails_of_the_step_loop_under_every_transport(gpu, kind, call):
    L = gpu
    p, ob, cells, body = _case(L)
    ran = []
    with _context(L, kind, p, ob, cells) as lat:
        lat.set_option("engine", 1)
        lat.set_bodies(body, 1)
        for tb in (1, 2, 4, 8) if kind == "alone" else (1, 2, 4):
            lat.set_option("time_block", tb)
            K = int(lat.info("time_block_active"))
            if tb == 4:
                assert (K == 4) == MARCHES_AT_4[kind], (kind, K)
            if tb >= 4 and K != tb:
                continue                              # (the context would not march at this K: nothing is forced)
            if kind == "alone":
                assert K == tb
            for n in sorted({K + 3, 2 * K + 1}):
                lat.write_state(cells)
                av, F, st = _call(lat, call, p, n)
                av0, F0, st0, scale = _reference(L, call, n)
                where = (kind, call, tb, K, n)
                assert np.array_equal(_bits(st), _bits(st0)), where
                print(where, "av_vels max rel:", float(np.max(np.abs(av - av0) / np.abs(av0))))
                assert np.allclose(av, av0, rtol=AV_RTOL if call == "run_driven" else ENGINE_AV_RTOL, atol=0), where
                if call == "run_forces":
                    assert F.shape == (n, 1, 2) and np.any(F0 != 0.0)
                    print(where, "forces max abs diff:", float(np.abs(F.astype(np.float64) - F0).max()))
                    assert _close(F, F0, scale), where
                ran.append((tb, n))
    assert len(ran) == 3 + 2 * MARCHES_AT_4[kind] + 2 * (kind == "alone"), ran      # (time blocks 1 and 2: 3, 4 and 5 steps)
