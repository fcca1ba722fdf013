"""lbm_set_obstacles and lbm_write_state on slabs of more than 2^20 cells: the second pass of lbm_swap_blocked.

A launch of lbm_swap_blocked has at most kSwapBlocksMax x kBlock = 4096 x 256 = 2^20 threads; a thread walks the slab's cells
with that stride.  No slab of the other live-input tests has more than 256 x 256 cells, so `c += stride`, the long index
arithmetic behind it and the refills counted in a later pass had never run.  Two shapes:

  * 1024 x 1040 alone: 1 064 960 cells, the smallest lattice of this width and a multiple of 16 rows past 2^20;
  * 1024 x 2080 in two copy slabs of 1040 rows, so that the second slab's `obstacles + row0 * nx` meets the stride too.

A, S0: test_large_lattices._case (7 % random obstacles, dashed rows and columns, the equilibrium +-10 %).  B is A with 1 % of
the cells flipped at random and, in every slab, explicit edits (asserted without a GPU): refilled are the cell of index
exactly 2^20 (column 0 of the slab's row 1024), the slab's last cell, a pair c and c + 2^20 -- one thread in two passes --
and cells of rows 1023 and 1024; cells below and above 2^20 turn blocked.

After RUNS[0] steps and set_obstacles(B, LBM_REFILL_REST): refilled_cells is numpy's count (the whole, and the slabs' counts
summed as the call sums them), read_state is S' (test_live_inputs.s_prime) bit for bit, fluid_cells, and total_density
against the double sum of in-order float cell sums (1e-12).  Then sum(RUNS) more steps, two ways: bit for bit against a
FRESH context lbm_create makes from (B, S'), LIVE and FRESH reporting the same engine keys (which engine that is at 1040
rows is not pinned here); and against the band oracle from (B, S') at the bar of tests/test_large_lattices.py,
|gpu - f64| <= 4 |f32 - f64| + 8 u max|f64|, in bands over the slab's rows 1024..1039 (wrapping into row 0), the accelerate
row, the slab seam and the middle of a slab.  Last, write_state(W) and read_state, bit for bit."""
import time

import numpy as np
import pytest

from test_large_lattices import BAND, K, RUNS, Bands, _case, _engine, _orc_param, _probe_chunk_rows
from test_live_inputs import REST, _same, refilled, s_prime

STRIDE = 4096 * 256                 # kSwapBlocksMax * kBlock (lbm_live.hip.h)
NX, SLAB_ROWS = 1024, 1040
SHAPES = {"1024x1040": 1, "1024x2080_two_copy_slabs": 2}
# slab-local (row, column) of the explicit edits
AT_STRIDE = (1024, 0)
LAST = (SLAB_ROWS - 1, NX - 1)
PAIR = ((5, 17), (5 + 1024, 17))
ROWS_EITHER_SIDE = [(r, x) for r in (1023, 1024) for x in range(100, 112, 2)]
TURN_BLOCKED = ((7, 33), (1030, 35))


def _index(rc):
    return rc[0] * NX + rc[1]


_MAPS = {}


def maps(L, nslabs):
    """(p, A, B, S0) of a shape"""
    if nslabs not in _MAPS:
        ny = SLAB_ROWS * nslabs
        p, A, S0 = _case(L, NX, ny, NX * 7 + ny, 0, 64)
        rng = np.random.default_rng(ny)
        flip = rng.random((ny, NX), dtype=np.float32) < 0.01
        B = np.where(flip, 1 - A, A).astype(np.int32)
        for s in range(nslabs):
            r0 = s * SLAB_ROWS
            for r, x in (AT_STRIDE, LAST) + PAIR + tuple(ROWS_EITHER_SIDE):
                A[r0 + r, x], B[r0 + r, x] = 1, 0
            for r, x in TURN_BLOCKED:
                A[r0 + r, x], B[r0 + r, x] = 0, 1
        for a in (A, B, S0):
            a.setflags(write=False)
        _MAPS[nslabs] = (p, A, B, S0)
    return _MAPS[nslabs]


# ---------------------------------------------------------------------------------------------------------------- no GPU
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_maps_refill_where_they_say(L, shape):
    nslabs = SHAPES[shape]
    p, A, B, S0 = maps(L, nslabs)
    ny = SLAB_ROWS * nslabs
    assert (p.nx, p.ny) == (NX, ny) and SLAB_ROWS % 16 == 0 and NX * SLAB_ROWS > STRIDE >= NX * (SLAB_ROWS - 16)
    assert STRIDE == 2 ** 20 and _index(AT_STRIDE) == STRIDE and _index(LAST) == NX * SLAB_ROWS - 1
    assert _index(PAIR[1]) == _index(PAIR[0]) + STRIDE
    assert [L.slab_bounds(ny, nslabs, s) for s in range(nslabs)] == [(s * SLAB_ROWS, (s + 1) * SLAB_ROWS) for s in range(nslabs)]
    m = refilled(A, B)
    for s in range(nslabs):
        ms = m[s * SLAB_ROWS:(s + 1) * SLAB_ROWS].reshape(-1)            # the slab's cells as the kernel indexes them
        for rc in (AT_STRIDE, LAST) + PAIR + tuple(ROWS_EITHER_SIDE):
            assert ms[_index(rc)], (s, rc)
        assert ms[:STRIDE].sum() > 100 and ms[STRIDE:].sum() >= 10, (s, int(ms[STRIDE:].sum()))
        turned = ((A == 0) & (B != 0))[s * SLAB_ROWS:(s + 1) * SLAB_ROWS].reshape(-1)
        assert all(turned[_index(rc)] for rc in TURN_BLOCKED) and turned[:STRIDE].sum() > 100 and turned[STRIDE:].sum() >= 10
    assert (A == 0).sum() != (B == 0).sum()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _density_sum(cells):
    want = 0.0
    for r0 in range(0, cells.shape[0], 128):     # a cell's density in float, f0 .. f8 in order; the cells in double
        c = cells[r0:r0 + 128]
        rho = c[..., 0].copy()
        for k in range(1, 9):
            rho += c[..., k]
        want += float(rho.sum(dtype=np.float64))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_slab_beyond_the_stride_of_the_swap(gpu, O, shape):
    L = gpu
    t0 = time.time()
    nslabs = SHAPES[shape]
    p, A, B, S0 = maps(L, nslabs)
    ny = p.ny
    prm = _orc_param(O, NX, ny)
    kw = dict(nslabs=nslabs, devices=[0] * nslabs, exchange=L.EXCHANGE_COPY) if nslabs > 1 else {}
    m = refilled(A, B)
    per_slab = [int(m[s * SLAB_ROWS:(s + 1) * SLAB_ROWS].sum()) for s in range(nslabs)]
    with L.Lattice(p, A, S0, **kw) as live:
        assert live.num_slabs == nslabs and [live.slab_rows(s) for s in range(nslabs)] == [(s * SLAB_ROWS, (s + 1) * SLAB_ROWS) for s in range(nslabs)]
        live.run(RUNS[0])
        S = live.read_state()
        live.set_obstacles(B, REST)
        Sp = s_prime(S, A, B, REST, p.density)
        del S
        assert live.info("refilled_cells") == int(m.sum()) == sum(per_slab), (live.info("refilled_cells"), per_slab)
        assert live.info("obstacle_updates") == 1 and live.info("fluid_cells") == int((B == 0).sum())
        assert _same(live.read_state(), Sp), shape
        mass, want = live.total_density(), _density_sum(Sp)
        assert abs(mass - want) <= 1e-12 * mass, (mass, want)
        av = np.concatenate([live.run(n) for n in RUNS])
        keys = _engine(live)
        st = live.read_state()
        rng = np.random.default_rng(ny + 1)
        W = (Sp * (np.float32(0.95) + np.float32(0.1) * rng.random(Sp.shape, dtype=np.float32))).astype(np.float32)
        live.write_state(W)
        assert _same(live.read_state(), W), shape
        del W
    with L.Lattice(p, B, Sp, **kw) as fresh:
        av_f = np.concatenate([fresh.run(n) for n in RUNS])
        assert _engine(fresh) == keys, (shape, keys, _engine(fresh))
        assert _same(av, av_f) and _same(st, fresh.read_state()), shape
    H, _ = _probe_chunk_rows(L, NX, ny)
    bands = Bands(O, prm, B, Sp, H)
    for name, j0 in [("slab_middle", SLAB_ROWS // 2 - BAND // 2)] + [("slab_seam", s * SLAB_ROWS - BAND // 2) for s in range(1, nslabs)]:
        rows = np.arange(j0, j0 + BAND) % ny
        if any(int(r[0]) == j0 for _, r, _, _ in bands.items):     # (the middle of the lattice is one of them already)
            continue
        bands.items.append((name, rows, O.run_band(prm, Sp, B, j0, j0 + BAND, K, np.float64), O.run_band(prm, Sp, B, j0, j0 + BAND, K, np.float32)))
    covered = np.unique(np.concatenate([rows for _, rows, _, _ in bands.items]))
    for s in range(nslabs):                      # the slab's rows 1023 .. 1039 and the row behind them, the accelerate row
        assert np.isin((s * SLAB_ROWS + np.arange(1023, SLAB_ROWS + 1)) % ny, covered).all(), s
    assert np.isin([ny - 3, ny - 2, ny - 1, 0], covered).all()
    print(f"\n{shape}: {int(m.sum())} cells refilled ({per_slab} by slab), engine {keys}, bands {[(n, int(r[0])) for n, r, _, _ in bands.items]}")
    g, f = bands.check(st, "behind the refill")
    print(f"  {shape}: total_density rel {abs(mass - want) / mass:.1e}; worst band at {g / (4 * f + 8):.2f} of its bar; {time.time() - t0:.1f} s")
