"""Pins the float oracle bit for bit to the reference's own timestep_new2: (a) known-answer
vectors (tests/golden/kat_*.npz); (b) the shipped decks and random states
(tests/golden/ref_strict_*.npz).  All were made by tests/golden/make_golden.py from a
strict-IEEE build of the reference's d2q9-bgk.c (oracle/Makefile, oracle/_ref/)."""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, KATS, deck_paths, load_kat

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden import RANDOM_STEPS, REF_STRICT_DECKS, REF_STRICT_RANDOM, random_param  # noqa: E402


def _kat_param(O, k):
    return O.OrcParam(int(k["nx"]), int(k["ny"]), 10, int(k["reynolds_dim"]),
                      float(k["density"]), float(k["accel"]), float(k["omega"]))


@pytest.mark.parametrize("name", KATS)
def test_oracle_matches_reference_known_answers_bitwise(O, oracle, name):
    k = load_kat(name)
    prm = _kat_param(O, k)
    ob = np.ascontiguousarray(k["obstacles"], dtype=np.int32)
    a = k["cells0"].copy()
    b = np.empty_like(a)
    av = []
    for tt in range(1, 11):
        av.append(oracle.timestep(prm, a, b, ob))
        a, b = b, a
        if tt in (1, 2, 10):
            assert np.array_equal(a.view(np.uint32), k[f"cells_after_{tt}"].view(np.uint32)), f"step {tt}"
    assert np.array_equal(np.array(av, np.float32).view(np.uint32), k["av_vels"].view(np.uint32))
    assert np.float32(oracle.reynolds(prm, a, ob)) == k["reynolds_after_10"]


def test_known_answers_exercise_every_branch():
    """The vectors must contain blocked cells, open top/bottom rows (y-wrap live), and
    accelerate-row cells that the guard (f3-w1 > 0 ...) refuses."""
    for name in KATS:
        k = load_kat(name)
        ob, ny = k["obstacles"], int(k["ny"])
        assert ob.sum() > 0 and ob[0].sum() < ob.shape[1] and ob[ny - 1].sum() < ob.shape[1]
        a1 = np.float32(k["density"]) * np.float32(k["accel"]) / np.float32(9)
        row = k["cells0"][ny - 2]
        refused = (~ob[ny - 2].astype(bool)) & (row[:, 3] - a1 <= 0)
        assert refused.any()


def _strict_vectors(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("deck,nsteps", REF_STRICT_DECKS)
def test_oracle_equals_reference_on_shipped_decks_bitwise(O, oracle, deck, nsteps):
    """From rest on the shipped decks: every step's av_vels, the final lattice (sha256 of its bytes), av_velocity and
    the Reynolds number equal what the strict build of the reference computed (tests/golden/ref_strict_decks.npz)."""
    k = _strict_vectors("ref_strict_decks.npz")
    pf, of = deck_paths(deck)
    prm = O.read_params(pf)
    ob = O.read_obstacles(of, prm.nx, prm.ny)
    a = oracle.init_cells(prm, np.float32)
    b = np.empty_like(a)
    av = []
    for _ in range(nsteps):
        av.append(oracle.timestep(prm, a, b, ob))
        a, b = b, a
    assert np.array_equal(np.array(av, np.float32).view(np.uint32), k[f"{deck}.av_vels"].view(np.uint32))
    assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == str(k[f"{deck}.state_sha256"])
    assert np.float32(oracle.av_velocity(prm, a, ob)) == k[f"{deck}.av_velocity"]
    assert np.float32(oracle.reynolds(prm, a, ob)) == k[f"{deck}.reynolds"]


@pytest.mark.parametrize("nx,ny,seed", REF_STRICT_RANDOM)
def test_oracle_equals_reference_on_random_lattices_bitwise(O, oracle, nx, ny, seed):
    """Ragged and minimum sizes (the peeled reference needs nx, ny >= 2), dense random obstacles: every step's
    av_vels and the final lattice equal the strict reference's (tests/golden/ref_strict_random.npz)."""
    k = _strict_vectors("ref_strict_random.npz")
    key = f"{nx}x{ny}_{seed}"
    prm, ob, a = random_param(nx, ny), k[f"{key}.obstacles"], k[f"{key}.cells0"].copy()
    b = np.empty_like(a)
    av = []
    for _ in range(RANDOM_STEPS):
        av.append(oracle.timestep(prm, a, b, ob))
        a, b = b, a
    assert np.array_equal(np.array(av, np.float32).view(np.uint32), k[f"{key}.av_vels"].view(np.uint32))
    assert np.array_equal(a.view(np.uint32), k[f"{key}.cells"].view(np.uint32))
