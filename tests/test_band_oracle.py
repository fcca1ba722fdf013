"""The oracle by row bands and by chunks (oracle/lbm_oracle.py: run_band, step_chunks / step_chunked), which hold lattices
far beyond what the serial oracle can run whole (tests/test_large_lattices.py) to the double oracle.  No GPU.

  * run_band equals Oracle.run of the whole lattice bit for bit, in float and in double, for a band at every start row:
    bands that wrap across row 0 / ny-1, that hold the accelerate row ny-2 or not, and the whole-lattice fall-back;
  * step_chunked equals Oracle.timestep bit for bit, for chunks of one row up to the whole lattice; its speed sum over
    its fluid cells is the double oracle's step average up to the order of the double additions;
  * the light cone: one population changed K rows outside a band changes the band after K steps, one changed K + 1 rows
    outside does not -- so a helper that reads one row too few per side cannot pass;
  * run_band_steps (the band after EVERY step of one band run: tests/test_large_observers.py) equals Oracle.run of the
    whole lattice step by step, and run_band at every K, bit for bit, on the same bands;
  * band_forces (the force definition of include/lbm_mi355x.h on a window of rows, float64) equals the whole-lattice
    evaluation of tests/test_body_forces.py: the window [0, ny), windows that wrap, and the windows of a partition of the
    rows added up; its counts and its smallest link are what a direct loop over the cells finds."""
import numpy as np
import pytest

U = 2.0 ** -24
PARAMS = (0.1, 0.01, 1.85)
STRONG = (0.1, 0.05, 1.7)         # a larger accel: the accelerate row moves populations by 5e-4, far from rounding


def _case(O, nx, ny, seed, params=PARAMS):
    """Equilibrium +-10 % at random with 10 % random obstacles, row ny-2 part blocked; parameters as the float32 the
    reference reads."""
    rng = np.random.default_rng(seed)
    d, a, o = (float(np.float32(v)) for v in params)
    prm = O.OrcParam(nx, ny, 1, 10, d, a, o)
    ob = (rng.random((ny, nx)) < 0.1).astype(np.int32)
    ob[ny - 2, ::5] = 1
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
    cells = (d * w * (1.0 + 0.2 * (rng.random((ny, nx, 9)) - 0.5))).astype(np.float32)
    return prm, ob, cells


def _whole(O, prm, ob, cells, K, dtype):
    a = cells.astype(dtype)
    if K:
        O.Oracle("strict").run(prm, a, ob, K)
    return a


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# (nx, ny, steps K, band heights): K + band + K < ny takes the band path, otherwise the whole-lattice fall-back
BAND_CASES = [(64, 40, 1, (1, 6)), (64, 40, 7, (3,)), (64, 40, 13, (2, 14)), (33, 20, 4, (1, 5)), (33, 20, 9, (3,)),
              (130, 37, 3, (1, 8)), (130, 37, 17, (2,)), (24, 100, 19, (1, 30)), (24, 100, 19, (61, 62))]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nx,ny,K,heights", BAND_CASES)
def test_run_band_equals_whole_oracle_run(O, nx, ny, K, heights, dtype):
    prm, ob, cells = _case(O, nx, ny, nx * ny + K, STRONG if K % 2 else PARAMS)
    want = _whole(O, prm, ob, cells, K, dtype)
    paths = set()
    for h in heights:
        for j0 in range(ny):
            got = O.run_band(prm, cells, ob, j0, j0 + h, K, dtype)
            assert got.dtype == np.dtype(dtype) and got.shape == (h, nx, 9)
            rows = np.arange(j0, j0 + h) % ny
            assert np.array_equal(_bits(got), _bits(want[rows])), (j0, h)
            paths.add(2 * K + h >= ny)
    if max(heights) + 2 * K < ny:
        assert paths == {False}
    if nx * ny == 33 * 20 and K == 9:
        assert paths == {True}


def test_run_band_covers_the_wrap_and_the_accelerate_row(O):
    """The bands above include ones that wrap (j0 + h > ny) and ones that hold row ny-2 or not, on the band path; and
    the accelerate changes the answer (a band stepped without it differs where the cone holds row ny-2)."""
    nx, ny, K, h = 64, 40, 7, 3
    kinds = set()
    for j0 in range(ny):
        rows = O.band_rows(ny, j0, j0 + h, K)
        kinds.add((bool(rows[-1] < rows[0]), bool(np.any(rows == ny - 2))))
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    prm, ob, cells = _case(O, nx, ny, 7, STRONG)
    still = O.OrcParam(nx, ny, 1, 10, prm.density, 0.0, prm.omega)
    j0 = ny - 2 - 3
    assert not np.array_equal(O.run_band(prm, cells, ob, j0, j0 + h, K), O.run_band(still, cells, ob, j0, j0 + h, K))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nx,ny", [(64, 40), (33, 20), (130, 37), (17, 3)])
def test_step_chunked_equals_one_oracle_step(O, nx, ny, dtype):
    prm, ob, cells = _case(O, nx, ny, 100 + nx, STRONG)
    orc = O.Oracle("strict")
    a = cells.astype(dtype)
    b = np.empty_like(a)
    av = orc.timestep(prm, a, b, ob)
    for rows in sorted({1, 2, 5, 7, ny - 1, ny, ny + 3}):
        got, tot, cnt = O.step_chunked(prm, cells, ob, rows, dtype)
        assert np.array_equal(_bits(got), _bits(b)), rows
        assert cnt == int((ob == 0).sum())
        if dtype == np.float64:
            assert abs(tot / cnt - av) <= 1e-13 * av, (rows, tot / cnt, av)
        else:                     # (chunk sums in float, added in double: a serial float sum of cnt terms is off by <= cnt u)
            assert abs(tot / cnt - av) <= cnt * U * av, (rows, tot / cnt, av)
        seen = []
        _, tot2, cnt2 = O.step_chunked(prm, cells, ob, rows, dtype,
                                       visit=lambda r0, r1, new: seen.append((r0, r1, new.copy())))
        assert (tot2, cnt2) == (tot, cnt) and _ is None
        assert [s[:2] for s in seen] == [(r, min(ny, r + rows)) for r in range(0, ny, rows)]
        assert np.array_equal(_bits(np.concatenate([s[2] for s in seen])), _bits(b))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("j0,h,K", [(20, 4, 9), (0, 3, 12), (36, 5, 6), (30, 1, 19)])
def test_run_band_light_cone(O, j0, h, K, dtype):
    """f2 (moving north) changed in a fluid cell K rows below the band, f4 (moving south) K rows above it: the band's
    rows change after K steps, and equal the whole run's from the changed lattice.  The same change one row further
    out leaves them bit for bit as they were."""
    nx, ny = 48, 80
    prm, ob, cells = _case(O, nx, ny, 5, PARAMS)
    base = O.run_band(prm, cells, ob, j0, j0 + h, K, dtype)
    for k, below in ((2, True), (4, False)):
        for extra, inside in ((0, True), (1, False)):
            r = (j0 - K - extra) % ny if below else (j0 + h - 1 + K + extra) % ny
            x = int(np.nonzero(ob[r] == 0)[0][0])
            c2 = cells.copy()
            c2[r, x, k] *= np.float32(1.25)
            got = O.run_band(prm, c2, ob, j0, j0 + h, K, dtype)
            want = _whole(O, prm, ob, c2, K, dtype)[np.arange(j0, j0 + h) % ny]
            assert np.array_equal(_bits(got), _bits(want)), (k, extra)
            assert (not np.array_equal(_bits(got), _bits(base))) == inside, (k, extra, r)


@pytest.mark.parametrize("nx,ny,rows", [(64, 40, 7), (130, 37, 37), (33, 20, 1)])
def test_av_velocity_chunked_equals_double_oracle(O, nx, ny, rows):
    prm, ob, cells = _case(O, nx, ny, 9)
    tot, cnt = O.av_velocity_chunked(prm, cells, ob, rows)
    want = O.Oracle("strict").av_velocity(prm, cells.astype(np.float64), ob)
    assert cnt == int((ob == 0).sum()) and abs(tot / cnt - want) <= 1e-13 * want


# ---------------------------------------------------------------------------------------------------------------- run_band_steps
STEP_CASES = [(64, 40, 7, (3,)), (64, 40, 13, (2, 14)), (33, 20, 4, (1, 5)), (33, 20, 9, (3,)), (130, 37, 3, (8,)),
              (24, 100, 19, (30, 61, 62))]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nx,ny,n,heights", STEP_CASES)
def test_run_band_steps_equals_whole_oracle_run_step_by_step(O, nx, ny, n, heights, dtype):
    """Every start row: bands that wrap, with and without row ny-2, the band path and the whole-lattice fall-back."""
    prm, ob, cells = _case(O, nx, ny, nx * ny + n, STRONG if n % 2 else PARAMS)
    whole = [_whole(O, prm, ob, cells, t, dtype) for t in range(1, n + 1)]
    paths, kinds = set(), set()
    for h in heights:
        for j0 in range(ny):
            rows = np.arange(j0, j0 + h) % ny
            seen = []
            for t, got in O.run_band_steps(prm, cells, ob, j0, j0 + h, n, dtype):
                assert got.dtype == np.dtype(dtype) and got.shape == (h, nx, 9) and got.flags.owndata
                assert np.array_equal(_bits(got), _bits(whole[t - 1][rows])), (j0, h, t)
                seen.append(t)
            assert seen == list(range(1, n + 1))
            paths.add(2 * n + h >= ny)
            if 2 * n + h < ny:
                cone = O.band_rows(ny, j0, j0 + h, n)
                kinds.add((bool(cone[-1] < cone[0]), bool(np.any(cone == ny - 2))))
    if max(heights) + 2 * n < ny:
        assert paths == {False} and kinds == {(False, False), (False, True), (True, False), (True, True)}
    if (nx, ny, n) == (33, 20, 9):
        assert paths == {True}
    if (nx, ny, n) == (24, 100, 19):
        assert paths == {False, True}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_run_band_steps_agrees_with_run_band_at_every_K(O, dtype):
    nx, ny, n, h = 48, 80, 19, 7
    prm, ob, cells = _case(O, nx, ny, 11, STRONG)
    for j0 in (0, 30, ny - 2 - 3, ny - 3, ny - 1):
        steps = dict(O.run_band_steps(prm, cells, ob, j0, j0 + h, n, dtype))
        for K in range(1, n + 1):
            assert np.array_equal(_bits(steps[K]), _bits(O.run_band(prm, cells, ob, j0, j0 + h, K, dtype))), (j0, K)
    assert list(O.run_band_steps(prm, cells, ob, 5, 9, 0, dtype)) == []
    with pytest.raises(ValueError):
        list(O.run_band_steps(prm, cells, ob, ny, ny + 2, 3, dtype))


# ---------------------------------------------------------------------------------------------------------------- band_forces
def _force_case(O, nx, ny, seed):
    prm, ob, cells = _case(O, nx, ny, seed)
    rng = np.random.default_rng(seed + 1)
    body = rng.integers(0, 5, size=ob.shape).astype(np.int32)          # (labels on fluid cells too: ignored)
    state = _whole(O, prm, ob, cells, 3, np.float32)
    return ob, body, state


def _ext(ob, j0, j1):
    return ob[np.arange(j0 - 1, j1 + 1) % ob.shape[0]]


@pytest.mark.parametrize("nx,ny", [(64, 40), (33, 20), (130, 37)])
def test_band_forces_is_the_whole_lattice_evaluation(O, nx, ny):
    from test_body_forces import forces_from_state
    ob, body, state = _force_case(O, nx, ny, nx + ny)
    F, A = forces_from_state(state, ob, body, 4)
    whole = O.band_forces(state, _ext(ob, 0, ny), body, 4)
    assert np.all(np.abs(whole["F"] - F) <= 1e-13 * A) and np.all(np.abs(whole["A"] - A) <= 1e-13 * A)
    assert np.all(A > 0) and np.all(whole["cells"] > 0)
    # a window that wraps holds the same cells; the windows of a partition add up (links, cells, A, F)
    for j0 in (ny - 3, ny - 1, 5):
        rows = np.arange(j0, j0 + ny) % ny
        w = O.band_forces(state[rows], _ext(ob, j0, j0 + ny), body[rows], 4)
        assert np.all(np.abs(w["F"] - F) <= 1e-13 * A) and np.array_equal(w["cells"], whole["cells"])
    for cuts in ([0, 1, 2, ny - 2, ny - 1, ny], [0, 7, ny], [3, 11, ny + 3]):
        parts = [O.band_forces(state[np.arange(a, b) % ny], _ext(ob, a, b), body[np.arange(a, b) % ny], 4)
                 for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.all(np.abs(sum(q["F"] for q in parts) - F) <= 1e-13 * A)
        assert np.all(np.abs(sum(q["A"] for q in parts) - A) <= 1e-13 * A)
        assert np.array_equal(sum(q["cells"] for q in parts), whole["cells"])
        assert np.array_equal(sum(q["links"] for q in parts), whole["links"])
        assert np.array_equal(np.min([q["min_link"] for q in parts], axis=0), whole["min_link"])


def test_band_forces_counts_what_a_loop_over_the_cells_counts(O):
    """Cell by cell in Python on a small window: the force, the links, the counted cells and the smallest link; the
    obstacle rows either side of the window decide (one link fewer where the row below is blocked instead of fluid)."""
    nx, ny = 33, 20
    ob, body, state = _force_case(O, nx, ny, 3)
    j0, j1 = 17, 23                                   # rows 17, 18, 19, 0, 1, 2
    rows = np.arange(j0, j1) % ny
    got = O.band_forces(state[rows], _ext(ob, j0, j1), body[rows], 4)
    F, A, links = np.zeros((4, 2)), np.zeros((4, 2)), np.zeros((4, 2))
    cells, least = np.zeros(4, int), np.full(4, np.inf)
    for y in rows:
        for x in range(nx):
            b = int(body[y, x])
            if not ob[y, x] or b == 0:
                continue
            hit = False
            for i in range(1, 9):
                if ob[(y - O.CY[i]) % ny, (x - O.CX[i]) % nx]:
                    continue
                hit = True
                f = float(state[y, x, O.OPP[i]])
                c = np.array([O.CX[i], O.CY[i]], float)
                F[b - 1] += 2 * f * c
                A[b - 1] += 2 * abs(f) * np.abs(c)
                links[b - 1] += np.abs(c)
                least[b - 1] = min(least[b - 1], 2 * abs(f))
            cells[b - 1] += hit
    assert np.all(np.abs(got["F"] - F) <= 1e-13 * A) and np.all(np.abs(got["A"] - A) <= 1e-13 * A)
    assert np.array_equal(got["links"], links) and np.array_equal(got["cells"], cells) and np.array_equal(got["min_link"], least)
    assert cells.min() >= 1
    ext = _ext(ob, j0, j1).copy()
    x = int(np.nonzero((ob[rows[0]] != 0) & (body[rows[0]] > 0) & (ob[(j0 - 1) % ny] == 0))[0][0])
    ext[0, x] = 1                                     # the source of direction N (2) of that cell, now blocked
    fewer = O.band_forces(state[rows], ext, body[rows], 4)
    assert fewer["links"].sum() < got["links"].sum()
    with pytest.raises(ValueError):
        O.band_forces(state[rows], ob[rows], body[rows], 4)
