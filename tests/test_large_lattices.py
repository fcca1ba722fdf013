"""Lattices beyond 1024^2 against the double oracle, in row bands and chunks (oracle/lbm_oracle.py: run_band,
step_chunks, av_velocity_chunked; their CPU tests are tests/test_band_oracle.py).

The serial oracle cannot run these lattices whole, but K steps of rows [j0, j1) depend only on rows [j0 - K, j1 + K), and
one step of a chunk only on the chunk and one row either side.  So every check here is against the oracle, not against
another GPU kernel, and would see a fault that all engines share (upload / download, blocked packing, lbm_derive, the
partial sums behind av_vels, the accelerate row, chunk and strip edges).  Starting lattices: the equilibrium +-10 % at
random (uploaded: never cells = NULL), 7 % random obstacles, and dashed obstacle rows / columns where code changes
behaviour: rows 0, 1, ny-3, ny-2, ny-1, columns 0 and nx-1, the default chunk edges and strip edges (wave_out_cols, else
64 columns), and at 16384^2 the rows where the AoS float index 9 c passes 2^31 and its byte offset 2^32.

u = 2^-24; bars are those of tests/test_param_space.py:
  (a) at t = 0: read_state bit for bit; final_state of blocked cells exactly (0, 0, 0, float32(density) float32(1/3)), of
      fluid cells in the bands within 2e-6 |f64| + 8 u; total_density against the double sum of in-order float cell sums
      (1e-12); av_velocity / reynolds against the chunked double evaluation (1e-5 + 8 u);
  (b) one step of the whole lattice, shadowed chunk by chunk in double and in strict float from the GPU's state: every
      element within 8 u rho of double and the worst within 2 x the float oracle's worst + 1 u rho; the step's average
      within 2 |av32 - av64| + 4 u; at 8192^2 and 16384^2 the first three steps (run(1) + read_state);
  (c) runs [16, 3] of the default (two passes of eight and a remainder), rows checked in bands: |gpu - f64| <= 4 |f32 - f64|
      + 8 u max|f64| in every band; at 4096^2 also every engine forced once, each against the bands.
Every case asserts which engine ran (info keys) and prints its deviations."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ONE_THIRD = np.float32(1.0 / 3.0)
PARAMS = (0.1, 0.01, 1.85)
RUNS = [16, 3]
K = sum(RUNS)
BAND = 96
CHUNK = 128                      # rows per oracle chunk (a float64 chunk of 16384-wide rows: 150 MB)


def _orc_param(O, nx, ny):
    d, a, o = (float(np.float32(v)) for v in PARAMS)
    return O.OrcParam(nx, ny, 100, 10, d, a, o)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _probe_chunk_rows(L, nx, ny):
    """The default chunk height (wave_rows after a run, else march_rows) on this lattice; 0 where no marching kernel runs.
    A lattice at the equilibrium (cells = NULL, obstacles none): the chunking does not depend on either."""
    p = L.Param(nx, ny, 10, 10, *PARAMS)
    with L.Lattice(p, np.zeros((ny, nx), np.int32)) as lat:
        tb = int(lat.info("time_block_active"))
        if tb < 4 or lat.info("engine_next") == 3:
            return 0, 64
        lat.run(tb)
        if lat.info("march_kernel") == 1:
            return int(lat.info("wave_rows")), int(lat.info("wave_out_cols"))
        return int(lat.info("march_rows")), 64


def _special_rows(nx, ny):
    """Rows of the AoS index 9 c passing 2^31 and of its byte offset 36 c passing 2^32, where the lattice has them."""
    rows = {}
    for name, lim, per in (("9c>=2^31", 2 ** 31, 9), ("36c>=2^32", 2 ** 32, 36)):
        r = -(-lim // (per * nx))
        if r < ny:
            rows[name] = r
    return rows


def _case(L, nx, ny, seed, H, W):
    rng = np.random.default_rng(seed)
    ob = (rng.random((ny, nx), dtype=np.float32) < 0.07).astype(np.int32)
    for r in (0, 1, ny - 3, ny - 2, ny - 1):
        ob[r, r % 3::3] = 1
    for c in (0, nx - 1):
        ob[c % 3::3, c] = 1
    if H:
        for m in range(1, -(-ny // H)):
            ob[m * H - 1, 1::4] = 1
            ob[m * H, 2::4] = 1
    for s in range(W, nx, W):
        ob[s % 4::4, s - 1] = 1
        ob[(s + 1) % 4::4, s] = 1
    for r in _special_rows(nx, ny).values():
        ob[r - 1, 0::5] = 1
        ob[r, 3::5] = 1
    w = (np.float32(PARAMS[0]) * np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, np.float32))
    cells = np.empty((ny, nx, 9), np.float32)
    step = max(1, (1 << 24) // nx)
    for r0 in range(0, ny, step):               # (in row blocks: no lattice-sized temporaries)
        x = rng.random((min(ny, r0 + step) - r0, nx, 9), dtype=np.float32)
        x -= np.float32(0.5)
        x *= np.float32(0.2)
        x += np.float32(1.0)
        x *= w
        cells[r0:r0 + step] = x
    return L.Param(nx, ny, 100, 10, *PARAMS), ob, cells


def _bands(nx, ny, H):
    """(name, j0, rows) of the checked bands, BAND rows each: the top (wrapping across ny-1 / 0), the bottom, around ny-2, across
    chunk edges, across the 2^31 / 2^32 rows and the middle."""
    if ny < 4 * BAND:                           # a short lattice: one band round the accelerate row, across ny-1 / 0
        h = min(BAND, ny - 2 * K - 1)
        return [("accel_row_wrap", (ny - 2 - h // 2) % ny, h)]
    b = [("top", ny - BAND // 2), ("bottom", 0), ("accel_row", ny - 2 - BAND // 2), ("middle", ny // 2 - BAND // 2)]
    if H and H < ny:
        m = max(1, (ny // H) // 3)
        b.append(("chunk_edge", m * H - BAND // 2))
        if H < BAND:
            b.append(("chunk_edges", (m + 3) * H - BAND // 2 + H // 2))
    for name, r in _special_rows(nx, ny).items():
        b.append((name, r - BAND // 2))
    return [(n, j0 % ny, BAND) for n, j0 in b]


class Bands:
    """Rows of the checked bands after K steps, by the oracle in double and in strict float, from the input lattice."""

    def __init__(self, O, prm, ob, cells, H):
        self.items = []
        for name, j0, h in _bands(prm.nx, prm.ny, H):
            rows = np.arange(j0, j0 + h) % prm.ny
            self.items.append((name, rows, O.run_band(prm, cells, ob, j0, j0 + h, K, np.float64),
                               O.run_band(prm, cells, ob, j0, j0 + h, K, np.float32)))

    def check(self, st, tag):
        worst = []
        for name, rows, c64, c32 in self.items:
            d32 = float(np.max(np.abs(c32 - c64)))
            dg = float(np.max(np.abs(st[rows] - c64)))
            top = float(np.max(np.abs(c64)))
            worst.append((dg / (U * top), d32 / (U * top)))
            assert dg <= 4 * d32 + 8 * U * top, (tag, name, int(rows[0]), dg, d32)
        g, f = max(w[0] for w in worst), max(w[1] for w in worst)
        print(f"  {tag}: {K} steps in {len(worst)} bands: |gpu - f64| {g:.2f} u max, |f32 - f64| {f:.2f} u max")
        return g, f


def _shadow_step(O, prm, ob, x, st, av, tag):
    """One step from x (the GPU's state before it) chunk by chunk in double and float, against st / av of the GPU."""
    e_g = e_f = 0.0
    t64 = t32 = 0.0
    cnt = 0
    for (r0, r1, n64, s64, c64), (_, _, n32, s32, _) in zip(O.step_chunks(prm, x, ob, CHUNK, np.float64),
                                                         O.step_chunks(prm, x, ob, CHUNK, np.float32)):
        urho = U * n64.sum(axis=-1)
        e32 = float(np.max(np.abs(n32 - n64).max(axis=-1) / urho))
        e = float(np.max(np.abs(st[r0:r1] - n64).max(axis=-1) / urho))
        assert e <= 8.0, (tag, r0, e, e32)
        e_g, e_f = max(e_g, e), max(e_f, e32)
        t64 += s64
        t32 += s32
        cnt += c64
    assert e_g <= 2.0 * e_f + 1.0, (tag, e_g, e_f)
    av64, av32 = t64 / cnt, t32 / cnt
    assert abs(av - av64) <= 2.0 * abs(av32 - av64) + 4 * U, (tag, av, av32, av64)
    print(f"  {tag}: one step |gpu - f64| {e_g:.2f} u rho, float oracle {e_f:.2f} u rho;"
          f" av_vels |gpu - f64| {abs(av - av64) / U:.3f} u, float {abs(av32 - av64) / U:.3f} u")
    return e_g, e_f


def _round_trip(O, L, lat, prm, p, ob, cells, bands):
    """(a): t = 0 read back, derived fields and sums."""
    st = lat.read_state()
    assert np.array_equal(_bits(st), _bits(cells)), "read_state after lbm_create is not the input"
    del st
    fs = lat.final_state()
    blocked = ob.astype(bool)
    assert np.all(fs[blocked][:, :3] == 0) and np.all(fs[blocked][:, 3] == np.float32(p.density) * ONE_THIRD)
    worst = 0.0
    for name, rows, _, _ in bands.items:
        fo = O.Oracle("strict").final_state(O.band_param(prm, len(rows)), np.ascontiguousarray(cells[rows], np.float64),
                                            np.ascontiguousarray(ob[rows]))
        d = np.abs(fs[rows] - fo)
        assert np.all(d <= 2e-6 * np.abs(fo) + 8 * U), (name, float(np.max(d)))
        worst = max(worst, float(np.max(d / (2e-6 * np.abs(fo) + 8 * U))))
    del fs
    mass = lat.total_density()
    want = 0.0
    for r0 in range(0, prm.ny, CHUNK):           # a cell's density in float, f0 .. f8 in order; the cells in double
        c = cells[r0:r0 + CHUNK]
        rho = c[..., 0].copy()
        for k in range(1, 9):
            rho += c[..., k]
        want += float(rho.sum(dtype=np.float64))
    assert abs(mass - want) <= 1e-12 * mass, (mass, want)
    tot, n = O.av_velocity_chunked(prm, cells, ob, CHUNK)
    av_o = tot / n
    re_o = av_o * prm.reynolds_dim / (1.0 / 6.0 * (2.0 / prm.omega - 1.0))
    avv, re = lat.av_velocity(), lat.reynolds()
    assert n == int(lat.info("fluid_cells"))
    assert abs(avv - av_o) <= 1e-5 * av_o + 8 * U, (avv, av_o)
    assert abs(re - re_o) <= (1e-5 + 8 * U / av_o) * re_o, (re, re_o)
    print(f"  t=0: read_state bit-exact; final_state bands at {worst:.2f} of the bar; total_density rel {abs(mass - want) / mass:.1e};"
          f" av_velocity rel {abs(avv - av_o) / av_o:.2e}, reynolds rel {abs(re - re_o) / re_o:.2e}")


def _engine(lat):
    return {k: int(lat.info(k)) for k in ("engine_last", "time_block_active", "march_kernel", "wave_cols_active",
                                          "wave_rows", "march_rows", "kernel_variant", "vector_width", "regtile")}


# lattice -> (info that must hold after the default run of RUNS[0] steps, steps shadowed one by one (b, d))
DEFAULTS = {
    (2048, 2048): ({"engine_last": 1, "time_block_active": 4, "march_kernel": 0}, 1),
    (2050, 2048): ({"engine_last": 1, "time_block_active": 6, "march_kernel": 1}, 1),
    (4096, 4096): ({"engine_last": 1, "time_block_active": 8, "march_kernel": 1, "wave_cols_active": 2}, 1),
    (8192, 8192): ({"engine_last": 1, "time_block_active": 8, "march_kernel": 1, "wave_cols_active": 2}, 3),
    (16384, 16384): ({"engine_last": 1, "time_block_active": 8, "march_kernel": 1, "wave_cols_active": 2}, 3),
    (65536, 128): ({}, 1),
    (128, 65536): ({}, 1),
    ("regtile_limit", 1024): ({"engine_last": 3}, 1),
}
# the chunk heights the 256-CU table of tests/test_gpu_parity.py pins (75 / 304 rows)
CHUNK_ROWS = {(4096, 4096): (75, 76), (8192, 8192): (304, 305, 149)}


def _regtile_limit_rows(L, nx, ncu):
    """The tallest lattice of nx columns that lbm_regtile tiles onto ncu CUs (host rule, lbm_plan_tiles)."""
    for rows in range(64 * ncu // (nx // 64), 0, -1):
        if L.plan_tiles(nx, rows, 1, ncu) is not None:
            return rows
    raise AssertionError("no register tiling at all")


def _forced_engines():
    """(name, options, info after RUNS[0] steps): every streaming engine at 4096^2, each against the bands."""
    return [
        ("sweep2", [("time_block", 2)], {"engine_last": 1, "time_block_active": 2}),
        ("march", [("march_kernel", 0), ("time_block", 4)], {"time_block_active": 4, "march_kernel": 0}),
        ("wave4", [("march_kernel", 1), ("time_block", 4), ("wave_cols", 1)],
         {"time_block_active": 4, "march_kernel": 1, "wave_cols_active": 1}),
        ("wave6", [("march_kernel", 1), ("time_block", 6), ("wave_cols", 1)],
         {"time_block_active": 6, "march_kernel": 1, "wave_cols_active": 1}),
        ("wave8", [("march_kernel", 1), ("time_block", 8), ("wave_cols", 1)],
         {"time_block_active": 8, "march_kernel": 1, "wave_cols_active": 1}),
        ("wave8_cols2", [("march_kernel", 1), ("time_block", 8), ("wave_cols", 2)],
         {"time_block_active": 8, "march_kernel": 1, "wave_cols_active": 2}),
        ("variant0_ieee", [("kernel_variant", 0)],
         {"time_block_active": 8, "march_kernel": 1, "wave_cols_active": 2, "kernel_variant": 0}),
        ("variant7", [("kernel_variant", 7)],
         {"time_block_active": 8, "march_kernel": 1, "wave_cols_active": 2, "kernel_variant": 7}),
    ]


@pytest.mark.parametrize("shape", list(DEFAULTS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_large_lattice_against_double_oracle(gpu, O, shape):
    L = gpu
    t_start = time.time()
    want, nshadow = DEFAULTS[shape]
    nx, ny = shape
    if nx == "regtile_limit":
        with L.Lattice(L.Param(64, 64, 1, 1, *PARAMS), np.zeros((64, 64), np.int32)) as lat:
            ncu = int(lat.info("compute_units"))
        nx, ny = 1024, _regtile_limit_rows(L, 1024, ncu)
        want = dict(want, regtile=(lambda t: t[0] * 10 + t[1])(L.plan_tiles(nx, ny, 1, ncu)))
    H, W = _probe_chunk_rows(L, nx, ny)
    p, ob, cells = _case(L, nx, ny, nx * 7 + ny, H, W)
    prm = _orc_param(O, nx, ny)
    bands = Bands(O, prm, ob, cells, H)
    print(f"\n{nx}x{ny}: chunk rows {H}, strip columns {W}, bands {[(n, int(r[0])) for n, r, _, _ in bands.items]}")
    # (a) + (b) / (d): t = 0, then steps one at a time from the GPU's own state
    with L.Lattice(p, ob, cells) as lat:
        _round_trip(O, L, lat, prm, p, ob, cells, bands)
        x = cells
        for t in range(1, nshadow + 1):
            av = float(lat.run(1)[0])
            st = lat.read_state()
            _shadow_step(O, prm, ob, x, st, av, f"step {t} ({_engine(lat)['time_block_active']}-step default)")
            if x is not cells:
                del x
            x = st
            del st
        del x
    # (c) the default over RUNS, in bands
    with L.Lattice(p, ob, cells) as lat:
        av = lat.run(RUNS[0])
        info = _engine(lat)
        for k, v in want.items():
            assert info[k] == v, (shape, k, info)
        if info["time_block_active"] >= 4 and info["engine_last"] == 1:
            rows = info["wave_rows"] if info["march_kernel"] == 1 else info["march_rows"]
            assert rows == H, (rows, H)
            if (nx, ny) in CHUNK_ROWS and lat.info("compute_units") == 256 and lat.info("wave_capacity") == 2048:
                assert H in CHUNK_ROWS[(nx, ny)], H
        av = np.concatenate([av, lat.run(RUNS[1])])
        st = lat.read_state()
    print(f"  default engine: {info}")
    bands.check(st, "default")
    del st
    if (nx, ny) == (4096, 4096):
        for name, options, must in _forced_engines():
            with L.Lattice(p, ob, cells) as lat:
                for key, v in options:
                    lat.set_option(key, v)
                lat.run(RUNS[0])
                info = _engine(lat)
                for k, v in must.items():
                    assert info[k] == v, (name, k, info)
                lat.run(RUNS[1])
                st = lat.read_state()
            bands.check(st, name)
            del st
        # (b) for vector widths 1, 2, 4 of the one-step kernel
        for V in (1, 2, 4):
            with L.Lattice(p, ob, cells) as lat:
                lat.set_option("time_block", 1)
                lat.set_option("vector_width", V)
                av1 = float(lat.run(1)[0])
                info = _engine(lat)
                assert info["engine_last"] == 1 and info["time_block_active"] == 1 and info["vector_width"] == V, info
                st = lat.read_state()
            _shadow_step(O, prm, ob, cells, st, av1, f"one-step kernel V={V}")
            del st
    print(f"  {nx}x{ny}: {time.time() - t_start:.1f} s")
