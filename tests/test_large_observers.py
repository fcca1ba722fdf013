"""lbm_run_forces, lbm_run_probes, lbm_run_mean, lbm_run_sampled and lbm_run_observed beyond 1024^2, where lbm_wave is the
DEFAULT engine and the observers ride in its launches, against the oracle in light-cone row bands
(oracle/lbm_oracle.py: run_band_steps, band_forces; their CPU tests are tests/test_band_oracle.py).

Every other test of those paths forces lbm_wave by options onto a lattice of at most 256 x 72.  Here the library picks the
engine, the chunk height, the columns per lane and the admission of the observers itself, and a quiet fall-back to the
split path -- which gives the same bits -- shows in the info keys.

Shapes (SHAPES): 8192 x 1024 and 4096 x 4096 (lbm_wave<8>, two columns per lane), 2050 x 2048 (lbm_wave<6>, a ragged last
strip), 128 x 65536 and 65536 x 128 (hundreds of chunks / of wave columns), 2048 x 2048 (lbm_march: the observers on the
split / one-step path, every *_in_wave and *_in_kernel key 0).  Starting lattice and obstacles: _case of
tests/test_large_lattices.py (equilibrium +-10 %, 7 % random obstacles, dashed rows and columns at every edge); the
control point (0.1, 0.01, 1.85).  n = 2 K + 3 steps (two passes, a pair, a single step); the periods of
tests/test_observer_param_space.py (_periods).

Placement (_place, from the chunk height H and the strip width W the default reports): three bands of 32 rows -- across
the wrap (rows ny-16 .. 15), across a chunk edge (where the lattice has none: at ny / 4), in the middle of a chunk.
Bodies 1-3: the blocked cells of a window of one band each (its middle 16 rows), wide enough to span two strip edges (the first two, the
middle two, the last two -- the ragged strip -- in turn; where the lattice has fewer than two strip edges, its whole
width); body 4: every other blocked cell.  Probes: LBM_MAX_PROBES at 8192 x 1024, 256 elsewhere; three quarters inside
the bands (blocked cells, rows 0, 1, ny-3, ny-2, ny-1, columns 0 and nx-1, both sides of every chunk edge inside a band,
both sides of the strip edges -- all of them at 4096 probes, those of the band's body window and the last one at 256 --
filled up at random), one quarter scattered over the lattice, no two alike.

What is asserted (u = 2^-24; `band` = over the cells of one band, per field component):
  path     on the lbm_wave shapes forces_in_wave, probes_in_wave, samples_in_wave, mean_in_wave = 1, observed_in_wave = 3
           for forces + probes, wave_launches = n // K on the fresh context, engine_last = 1, and the chunk height, the
           columns per lane, the strip width and the time block (PLAN_KEYS) those lbm_run reported on that lattice; on
           2048^2 all of the keys 0.  (lbm_run_observed with all four at 8192 x 1024 has periods of 2 < K steps, so it runs
           in pieces of at most 2 steps on the small kernels and reads observed_in_wave = 0: it is held to the same values,
           not to the lbm_wave flavours.)
  bits     snapshots and probes = the split path's (engine 1, time_block 1); mean = mean_of those snapshots; forces = the
           one-step path's; probes = the snapshot's cells where both sampled a step; the lattice after every call =
           lbm_run's; av_vels = lbm_run's bits on lbm_wave, within 2e-6 relative on 2048^2
  oracle   snapshots and in-band probes at step s: |X_gpu - X64| <= 4 max|X32 - X64| + 2e-6 max|X64| + 8 u, X64 / X32 =
           Oracle.final_state of the double / float band state (bar (c) of test_large_lattices.py through its bar (a) of
           the derive); a blocked cell exactly (0, 0, 0, float32(density) float32(1/3));
           means: that bar averaged over the sample steps, plus (m - 1) u sum |X_j| of include/lbm_mi355x.h;
           forces of bodies 1-3 at every step t against band_forces of the double band state:
             2 L_b e_t + (ceil(n_b / 256) + 8) u A_b,  e_t = 4 max|f32 - f64| + 8 u max|f64| over the band (bar (c)),
             L_b = sum |c_ik| over the counted links, n_b the counted cells, A_b twice the absolute contributions
             (a thread of body_forces_block adds ceil(n_b / 256) floats in turn);
           CONDITION (CPU, and again before the GPU runs): that bar is below half the smallest |2 f_opp(i)| of any counted
           link of the body -- one link missed or counted twice fails;
           forces of all four bodies at the last step against band_forces of the final lbm_read_state:
             (ceil(n_b / 256) + 8) u A_b -- the only place the hundreds of thousands of cells of body 4 meet a reference.
Every case prints its engine, its keys and its deviations as fractions of their bars.

Outputs past 2^31 floats and 2^32 bytes (test_snapshot_outputs_past_2_31_floats_and_2_32_bytes, a child process that
imports torch first): 8192 x 1024, lbm_run_sampled(65, every = 1) into a device tensor of 65 x 128 MiB filled with NaN --
snapshot 32 starts at byte 2^32, snapshot 64 at float index 2^31 -- and lbm_run_sampled(33, every = 1) into host memory
(the staging and the copy-out cross 2^32 bytes).  Snapshots 0, 31, 32, 63, 64 (host: 0, 31, 32) are the bits of
lbm_final_state after lbm_run of that many steps on the split path and lie inside the bar above in the bands (a light cone
of 65 rows); every other snapshot holds no NaN and a positive pressure; samples_in_wave = 1."""
import math
import queue
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from contextlib import closing

import numpy as np
import pytest

from test_large_lattices import CHUNK_ROWS, DEFAULTS, ONE_THIRD, PARAMS, U, _bits, _case, _orc_param, _probe_chunk_rows
from test_mean_run import _child, mean_of
from test_observer_param_space import _fluid_source, _periods, _placement, _power_of_two
from test_wave_fields import SPLIT

BAND = 32
NBODIES = 4
MAX_PROBES = 4096                # LBM_MAX_PROBES of include/lbm_mi355x.h
FEW_PROBES = 256
WAVE_KEYS = ("forces_in_wave", "probes_in_wave", "samples_in_wave", "mean_in_wave")
TILE_KEYS = ("forces_in_kernel", "probes_in_kernel", "samples_in_kernel", "mean_in_kernel")
PLAN_KEYS = ("wave_cols_active", "wave_out_cols", "wave_rows", "time_block_active")      # the chunk plan of lbm_wave
ENGINE_KEYS = ("engine_last", "time_block_active", "march_kernel", "wave_cols_active", "wave_rows", "march_rows",
               "wave_out_cols", "wave_launches")

# lattice -> (the default that must hold after a run: tests/test_gpu_parity.py KERNEL_SELECTION and
# tests/test_large_lattices.py DEFAULTS, probes)
SHAPES = {
    (8192, 1024): ({"engine_last": 1, "time_block_active": 8, "march_kernel": 1, "wave_cols_active": 2}, MAX_PROBES),
    (4096, 4096): ({"engine_last": 1, "time_block_active": 8, "march_kernel": 1, "wave_cols_active": 2}, FEW_PROBES),
    (2050, 2048): ({"engine_last": 1, "time_block_active": 6, "march_kernel": 1, "wave_cols_active": 1}, FEW_PROBES),
    (128, 65536): ({"engine_last": 1, "march_kernel": 1}, FEW_PROBES),
    (65536, 128): ({"engine_last": 1, "march_kernel": 1}, FEW_PROBES),
    (2048, 2048): ({"engine_last": 1, "time_block_active": 4, "march_kernel": 0}, FEW_PROBES),
}
CALLS = ("fields", "probes", "mean", "forces", "pair")
CASES = [(s, c) for s in SHAPES for c in CALLS + (("all",) if s == (8192, 1024) else ())]


# ---------------------------------------------------------------------------------------------------------------- placement
def _observer_bands(ny, H):
    """(name, first row, rows) of the three bands: across the wrap, across a chunk edge (at ny / 4 where the lattice has
    no chunk edge), in the middle of a chunk."""
    chunked = 0 < H < ny
    bands = [("wrap", ny - BAND // 2, BAND)]
    if chunked:
        bands.append(("chunk_edge", max(1, (ny // H) // 3) * H - BAND // 2, BAND))
        h = min(BAND, H)
        bands.append(("mid_chunk", ((ny // H) // 2) * H + H // 2 - h // 2, h))
    else:
        bands.append(("quarter", ny // 4 - BAND // 2, BAND))
        bands.append(("mid_chunk", ny // 2 - BAND // 2, BAND))
    return [(name, j0 % ny, h) for name, j0, h in bands]


def _chunk_edges_in(ny, H, j0, h):
    """the rows e = m H of chunk edges with both e - 1 and e among rows j0 .. j0 + h - 1 (taken modulo ny)"""
    if not 0 < H < ny:
        return []
    rows = set((np.arange(j0, j0 + h) % ny).tolist())
    return [e for e in range(H, ny, H) if e in rows and e - 1 in rows]


def _window_rows(rows):
    """the rows of a band's body window: the middle half of the band (the wrap, or the chunk edge, in their middle) --
    half the links of the whole band, which keeps the force bar well below half the smallest link"""
    h = len(rows)
    return rows[h // 4:h - h // 4]


def _place(nx, ny, H, W, ob, nprobes, seed=11):
    """dict(bands, windows [(c0, c1) per band], body int32 (ny, nx), xy int32 (nprobes, 2), in_band bool (nprobes))"""
    ob = np.asarray(ob).reshape(ny, nx)
    bands = _observer_bands(ny, H)
    sedges = list(range(W, nx, W))
    body = np.where(ob != 0, NBODIES, 0).astype(np.int32)
    windows = []
    for k, (name, j0, h) in enumerate(bands):
        rows = np.arange(j0, j0 + h) % ny
        if len(sedges) >= 2:
            i = (0, (len(sedges) - 2) // 2, len(sedges) - 2)[k]
            c0, c1 = max(0, sedges[i] - 8), min(nx, sedges[i + 1] + 8)
        else:
            c0, c1 = 0, nx
        sub = np.ix_(_window_rows(rows), np.arange(c0, c1))
        body[sub] = np.where(ob[sub] != 0, k + 1, 0)
        windows.append((c0, c1))
    rng = np.random.default_rng(seed)
    cells = set()
    for k, (name, j0, h) in enumerate(bands):
        rows = np.arange(j0, j0 + h) % ny
        c0, c1 = windows[k]
        bl = np.argwhere(ob[rows] != 0)
        for r, c in bl[np.linspace(0, len(bl) - 1, 6).astype(int)]:
            cells.add((int(c), int(rows[r])))
        for r in sorted(set(rows.tolist()) & {0, 1, ny - 3, ny - 2, ny - 1}):
            cols = {0, nx - 1, nx // 2, (c0 + c1) // 2}
            cols |= {int(np.flatnonzero(ob[r] == 0)[0]), int(np.flatnonzero(ob[r] != 0)[0])}
            cells |= {(c, r) for c in cols}
        for r in (rows[0], rows[h // 2], rows[-1]):
            cells |= {(0, int(r)), (nx - 1, int(r))}
        erows = []
        for e in _chunk_edges_in(ny, H, j0, h):
            erows += [e - 1, e]
            cells |= {(c, r) for r in (e - 1, e) for c in (0, c0, (c0 + c1) // 2, nx - 1)}
        some = [s for s in sedges if c0 < s < c1] + sedges[-1:]
        for s in (sedges if nprobes >= 1000 else some):
            for r in [int(rows[1]), int(rows[h // 2])] + erows[:2]:
                cells |= {(s - 1, r), (s, r)}
    in_band = 3 * nprobes // 4
    assert len(cells) <= in_band, (len(cells), in_band)
    while len(cells) < in_band:
        name, j0, h = bands[int(rng.integers(len(bands)))]
        cells.add((int(rng.integers(nx)), int((j0 + rng.integers(h)) % ny)))
    inside = len(cells)
    while len(cells) < nprobes:
        cells.add((int(rng.integers(nx)), int(rng.integers(ny))))
    xy = np.array(sorted(cells), dtype=np.int32)
    xy = xy[rng.permutation(len(xy))]
    banded = np.zeros(ny, bool)
    for name, j0, h in bands:
        banded[np.arange(j0, j0 + h) % ny] = True
    return dict(bands=bands, windows=windows, body=body, xy=xy, in_band=banded[xy[:, 1]], placed_in_bands=inside)


def _check_placement(nx, ny, H, W, ob, pl, nprobes):
    """The conditions of the placement, on whatever H and W the default reported."""
    ob = np.asarray(ob).reshape(ny, nx)
    bands, windows, body, xy = pl["bands"], pl["windows"], pl["body"], pl["xy"]
    assert [b[0] for b in bands] in (["wrap", "chunk_edge", "mid_chunk"], ["wrap", "quarter", "mid_chunk"])
    wrap = set((np.arange(bands[0][1], bands[0][1] + bands[0][2]) % ny).tolist())
    assert {ny - 3, ny - 2, ny - 1, 0, 1} <= wrap
    assert all(h + 2 * 19 < ny for _, _, h in bands)
    chunked = 0 < H < ny
    assert (bands[1][0] == "chunk_edge") == chunked
    if chunked:
        assert len(_chunk_edges_in(ny, H, *bands[1][1:])) >= 1
        assert _chunk_edges_in(ny, H, *bands[2][1:]) == [], "the mid-chunk band holds a chunk edge"
    counted = _fluid_source(ob) & (body > 0)
    assert np.all(body[ob == 0] == 0) and set(np.unique(body)) == set(range(NBODIES + 1))
    sedges = list(range(W, nx, W))
    for k, ((name, j0, h), (c0, c1)) in enumerate(zip(bands, windows)):
        rows = np.arange(j0, j0 + h) % ny
        mine = body == k + 1
        inside = np.zeros((ny, nx), bool)
        inside[np.ix_(_window_rows(rows), np.arange(c0, c1))] = True
        assert np.array_equal(mine, inside & (ob != 0)), name          # the blocked cells of the window, no others
        assert sum(c0 < s < c1 for s in sedges) >= min(2, len(sedges)), (name, c0, c1, W)
        assert 48 <= counted[mine].sum(), name
        if name == "chunk_edge":
            e = _chunk_edges_in(ny, H, j0, h)[0]
            assert counted[e - 1, c0:c1].any() and counted[e, c0:c1].any(), "no counted cells on both sides of the edge row"
    n4 = int(counted[body == NBODIES].sum())
    assert n4 >= 100_000 or nx * ny < 4_000_000, n4
    # probes
    assert len(xy) == nprobes and len(np.unique(xy, axis=0)) == nprobes
    assert np.all((xy[:, 0] >= 0) & (xy[:, 0] < nx) & (xy[:, 1] >= 0) & (xy[:, 1] < ny))
    assert pl["in_band"].sum() >= pl["placed_in_bands"] == 3 * nprobes // 4
    assert (~pl["in_band"]).sum() >= nprobes // 8 or ny <= 12 * BAND       # (the scattered quarter; a short lattice is mostly bands)
    at = ob[xy[:, 1], xy[:, 0]]
    got = set(map(tuple, xy.tolist()))
    assert (at != 0).sum() >= 12
    for r in (0, 1, ny - 3, ny - 2, ny - 1):
        here = xy[xy[:, 1] == r]
        assert len(here) >= 4 and np.any(ob[r, here[:, 0]] != 0) and np.any(ob[r, here[:, 0]] == 0), r
    assert {0, nx - 1} <= set(xy[:, 0].tolist())
    for k, (name, j0, h) in enumerate(bands):
        rows = np.arange(j0, j0 + h) % ny
        c0, c1 = windows[k]
        assert (0, int(rows[0])) in got and (nx - 1, int(rows[-1])) in got, name
        for e in _chunk_edges_in(ny, H, j0, h):
            assert {(c0, e - 1), (c0, e), (nx - 1, e - 1), (nx - 1, e)} <= got, (name, e)
        want = sedges if nprobes >= 1000 else [s for s in sedges if c0 < s < c1] + sedges[-1:]
        for s in want:
            assert {(s - 1, int(rows[1])), (s, int(rows[1]))} <= got, (name, s)
    return n4


# ---------------------------------------------------------------------------------------------------------------- the oracle in the bands
def _force_bar(links, cells, A, e):
    """2 L_b e_t + (ceil(n_b / 256) + 8) u A_b, per component"""
    return 2.0 * links * e + (math.ceil(cells / 256) + 8) * U * A


def _ahead(gen):
    """`gen` run in a thread of its own, two items ahead (the oracle steps outside the interpreter lock: the double and the
    float run of a band, and the bands, go side by side)."""
    q = queue.Queue(maxsize=2)
    stop = threading.Event()

    def work():
        try:
            for item in gen:
                if stop.is_set():
                    return
                q.put((item, None))
                if stop.is_set():
                    return
            q.put((None, StopIteration()))
        except BaseException as err:                  # (handed to the consumer)
            q.put((None, err))

    threading.Thread(target=work, daemon=True).start()
    try:
        while True:
            item, err = q.get()
            if isinstance(err, StopIteration):
                return
            if err is not None:
                raise err
            yield item
    finally:                                          # closed early (the consumer raised): let the producer go.  It has at
        stop.set()                                    # most one put pending, which the emptied queue takes; then it sees `stop`
        while True:
            try:
                q.get_nowait()
            except queue.Empty:
                break


class BandRuns:
    """The bands of one case after every step 1 .. n, by the double and the strict float oracle from the input lattice:
    per band and step the bar of the fields (dX = max|X32 - X64|, top = max|X64| per component), e_t, the float64 force of
    the band's body with its bar and its smallest link, X64 in the probed cells; X64 whole at the steps of `keep`."""

    def __init__(self, O, prm, ob, cells, pl, n, keep):
        self.n, self.keep, self.pl = n, set(keep), pl
        nx, ny = prm.nx, prm.ny
        xy = pl["xy"]

        def one(k):
            name, j0, h = pl["bands"][k]
            rows = np.arange(j0, j0 + h) % ny
            c0, c1 = pl["windows"][k]
            cols = np.arange(c0 - 1, c1 + 1) % nx                      # the body's columns and one either side: its sources
            ext = ob[np.arange(j0 - 1, j0 + h + 1) % ny][:, cols]
            lab = np.where(pl["body"][rows][:, cols] == k + 1, 1, 0)
            lab[:, 0] = lab[:, -1] = 0                                  # (band_forces wraps its columns: only into these two)
            ob_rows = np.ascontiguousarray(ob[rows])
            where = {int(r): i for i, r in enumerate(rows)}
            idx = np.array([i for i in range(len(xy)) if int(xy[i, 1]) in where], dtype=int)
            pr = np.array([where[int(xy[i, 1])] for i in idx], dtype=int)
            px = xy[idx, 0]
            o = O.Oracle("strict")
            bp = O.band_param(prm, h)
            res = dict(name=name, rows=rows, probes=idx, dX=[], top=[], e=[], F=[], A=[], bar=[], least=[], P64=[], X64={})
            with closing(_ahead(O.run_band_steps(prm, cells, ob, j0, j0 + h, n, np.float64))) as run64, \
                    closing(_ahead(O.run_band_steps(prm, cells, ob, j0, j0 + h, n, np.float32))) as run32:
                for (t, s64), (_, s32) in zip(run64, run32):
                    x64 = o.final_state(bp, s64, ob_rows)
                    x32 = o.final_state(bp, s32, ob_rows)
                    res["dX"].append(np.abs(x32 - x64).reshape(-1, 4).max(axis=0))
                    res["top"].append(np.abs(x64).reshape(-1, 4).max(axis=0))
                    e = 4.0 * float(np.max(np.abs(s32 - s64))) + 8 * U * float(np.max(np.abs(s64)))
                    f = O.band_forces(s64[:, cols], ext, lab, 1)
                    res["e"].append(e)
                    res["F"].append(f["F"][0])
                    res["A"].append(f["A"][0])
                    res["bar"].append(_force_bar(f["links"][0], int(f["cells"][0]), f["A"][0], e))
                    res["least"].append(float(f["min_link"][0]))
                    res["cells"], res["links"] = int(f["cells"][0]), f["links"][0]
                    res["P64"].append(x64[pr, px])
                    if t in self.keep:
                        res["X64"][t] = x64
            return res

        with ThreadPoolExecutor(max_workers=len(pl["bands"])) as pool:      # (the oracle runs outside the interpreter lock)
            self.items = list(pool.map(one, range(len(pl["bands"]))))

    def field_bar(self, b, t):
        return 4.0 * b["dX"][t - 1] + 2e-6 * b["top"][t - 1] + 8 * U

    def condition(self):
        """worst (force bar) / (half the smallest counted link) over bands, steps and components: must stay below 1"""
        worst = 0.0
        for b in self.items:
            for t in range(self.n):
                worst = max(worst, float(np.max(b["bar"][t]) / (0.5 * b["least"][t])))
        return worst

    def check_fields(self, X, t, tag):
        """a whole snapshot X (ny, nx, 4) of step t"""
        worst = 0.0
        for b in self.items:
            d = np.abs(X[b["rows"]] - b["X64"][t]).reshape(-1, 4).max(axis=0)
            bar = self.field_bar(b, t)
            worst = max(worst, float(np.max(d / bar)))
            assert np.all(d <= bar), (tag, b["name"], t, d, bar)
        return worst

    def check_probes(self, P, t, tag):
        """the probes P (nprobes, 4) of step t, those inside the bands"""
        worst = 0.0
        for b in self.items:
            d = np.abs(P[b["probes"]] - b["P64"][t - 1]).max(axis=0)
            bar = self.field_bar(b, t)
            worst = max(worst, float(np.max(d / bar)))
            assert np.all(d <= bar), (tag, b["name"], t, d, bar)
        return worst

    def check_mean(self, mean, steps, tag):
        m, worst = len(steps), 0.0
        for b in self.items:
            X = np.stack([b["X64"][t] for t in steps])
            bar = sum(self.field_bar(b, t) for t in steps) / m + (m - 1) * U * np.abs(X).sum(axis=0)
            d = np.abs(mean[b["rows"]] - X.mean(axis=0))
            worst = max(worst, float(np.max(d / bar)))
            assert np.all(d <= bar), (tag, b["name"], float(np.max(d / bar)))
        return worst

    def check_forces(self, F, tag):
        """F (n, 4, 2): bodies 1-3 (one per band) at every step"""
        worst = 0.0
        for k, b in enumerate(self.items):
            for t in range(self.n):
                d = np.abs(F[t, k].astype(np.float64) - b["F"][t])
                worst = max(worst, float(np.max(d / b["bar"][t])))
                assert np.all(d <= b["bar"][t]), (tag, b["name"], t + 1, d, b["bar"][t], b["least"][t])
        return worst


# ---------------------------------------------------------------------------------------------------------------- no GPU
# (nx, ny, chunk rows H, strip columns W, steps per pass K): the chunk heights CHUNK_ROWS pins (75 at 4096^2, 304 at
# 8192^2) at a width that keeps the oracle quick, lbm_wave<6>'s 64 rows at a ragged width, a lattice of one chunk
PLACEMENTS = [(1024, 1216, 75, 112, 8), (1024, 1216, 304, 112, 8), (450, 600, 64, 52, 6), (1024, 128, 128, 112, 8),
              (128, 2048, 64, 112, 8)]


def test_the_pinned_chunk_heights_are_the_placed_ones():
    """PLACEMENTS holds the chunk heights tests/test_large_lattices.py pins, and SHAPES asks for nothing its DEFAULTS and
    KERNEL_SELECTION of tests/test_gpu_parity.py do not pin: (engine, time block, lbm_wave, columns per lane)."""
    from test_gpu_parity import KERNEL_SELECTION
    assert {p[2] for p in PLACEMENTS} >= {CHUNK_ROWS[(4096, 4096)][0], CHUNK_ROWS[(8192, 8192)][0]} == {75, 304}
    for shape, (want, _) in SHAPES.items():
        pinned = dict(DEFAULTS.get(shape, ({},))[0])
        if shape + (1, "none") in KERNEL_SELECTION:
            engine, tb, kernel, cols = KERNEL_SELECTION[shape + (1, "none")]
            pinned.update(engine_last=engine, time_block_active=tb, march_kernel=kernel)
            if kernel:
                pinned["wave_cols_active"] = cols
        elif shape in ((128, 65536), (65536, 128)):       # no table pins a time block here: lbm_wave, as the default finds it
            pinned.update(engine_last=1, march_kernel=1)
        assert want == pinned, (shape, want, pinned)


@pytest.mark.parametrize("nx,ny,H,W,K", PLACEMENTS)
def test_placement_and_force_bar_condition_on_the_oracle(L, O, nx, ny, H, W, K):
    """The placement conditions for the pinned chunk heights, the periods, and -- from the oracle alone -- the CONDITION:
    the force bar of bodies 1-3 stays below half their smallest counted link at every step."""
    p, ob, cells = _case(L, nx, ny, nx * 7 + ny, H, W)
    for nprobes in (FEW_PROBES, MAX_PROBES):
        pl = _place(nx, ny, H, W, ob, nprobes)
        _check_placement(nx, ny, H, W, ob, pl, nprobes)
    n = 2 * K + 3
    pe, me, se = _periods(K, n)
    for every in (pe, me, se):
        assert all(_placement(K, n, every)), (K, n, every)
    assert n // me >= 3 and not _power_of_two(n // me)
    pl = _place(nx, ny, H, W, ob, FEW_PROBES)
    bands = BandRuns(O, _orc_param(O, nx, ny), ob, cells, pl, n, ())
    worst = bands.condition()
    print(f"{nx}x{ny} H={H} W={W}: bodies of {[b['cells'] for b in bands.items]} counted cells, force bar at most"
          f" {worst:.3f} of half the smallest link")
    assert worst < 1.0


# ---------------------------------------------------------------------------------------------------------------- GPU
def _default_plan(L, nx, ny):
    """(K, chunk rows H, strip columns W) of the default on this lattice: H and W as _probe_chunk_rows of
    tests/test_large_lattices.py reports them, K the time block of a fresh context (no run: the edges must be known before
    the obstacles are drawn, and neither depends on them)."""
    H, W = _probe_chunk_rows(L, nx, ny)
    p = L.Param(nx, ny, 10, 10, *PARAMS)
    with L.Lattice(p, np.zeros((ny, nx), np.int32)) as lat:
        K = int(lat.info("time_block_active"))
    assert K >= 4 and H > 0, (nx, ny, K, H, W)
    return K, H, W


_SHAPE = {}


def _setup(L, O, shape):
    """Once per shape (one shape cached at a time): the case, its placement, the bands by the oracle, lbm_run under the
    defaults, and the split / one-step references."""
    if shape in _SHAPE:
        return _SHAPE[shape]
    _SHAPE.clear()
    t0 = time.time()
    nx, ny = shape
    want, nprobes = SHAPES[shape]
    K, H, W = _default_plan(L, nx, ny)
    wave = want["march_kernel"] == 1
    n = 2 * K + 3
    pe, me, se = _periods(K, n)
    for every in (pe, me, se):
        assert all(_placement(K, n, every)), (K, n, every)
    m = n // me
    assert m >= 3 and not _power_of_two(m)
    p, ob, cells = _case(L, nx, ny, nx * 7 + ny, H, W)
    pl = _place(nx, ny, H, W, ob, nprobes)
    n4 = _check_placement(nx, ny, H, W, ob, pl, nprobes)
    g = math.gcd(me, se)
    t1 = time.time()
    bands = BandRuns(O, _orc_param(O, nx, ny), ob, cells, pl, n, set(range(me, n + 1, me)) | set(range(se, n + 1, se)))
    cond = bands.condition()
    assert cond < 1.0, (shape, "force bar against half the smallest link", cond)
    t2 = time.time()
    # lbm_run under the defaults
    with L.Lattice(p, ob, cells) as lat:
        av0 = lat.run(n)
        info = {k: int(lat.info(k)) for k in ENGINE_KEYS}
        st0 = lat.read_state()
    for k, v in want.items():
        assert info[k] == v, (shape, k, info)
    assert (info["wave_rows"] if wave else info["march_rows"]) == H and info["time_block_active"] == K, (info, H, K)
    if wave:
        assert info["wave_out_cols"] == W and info["wave_launches"] == n // K, info
    # the split path: snapshots at every common step of the means and the snapshots, probes, forces of the one-step path
    with L.Lattice(p, ob, cells) as lat:
        for k, v in SPLIT:
            lat.set_option(k, v)
        _, S = lat.run_sampled(n, g)
        assert all(lat.info(k) == 0 for k in WAVE_KEYS + TILE_KEYS) and lat.info("time_block_active") == 1
    with L.Lattice(p, ob, cells) as lat:
        for k, v in SPLIT:
            lat.set_option(k, v)
        lat.set_probes(pl["xy"])
        lat.set_bodies(pl["body"], NBODIES)
        _, P1 = lat.run_probes(n, pe)
        assert all(lat.info(k) == 0 for k in WAVE_KEYS + TILE_KEYS)
    with L.Lattice(p, ob, cells) as lat:
        for k, v in SPLIT:
            lat.set_option(k, v)
        lat.set_bodies(pl["body"], NBODIES)
        _, F1 = lat.run_forces(n)
        assert all(lat.info(k) == 0 for k in WAVE_KEYS + TILE_KEYS) and lat.info("engine_last") == 1
        assert np.array_equal(_bits(lat.read_state()), _bits(st0)), (shape, "the lattice of the one-step kernel")
    final = O.band_forces(st0, ob[np.arange(-1, ny + 1) % ny], pl["body"], NBODIES)
    for a in (ob, cells, av0, st0, S, P1, F1, pl["xy"], pl["body"]):
        a.setflags(write=False)
    print(f"\n{nx}x{ny}: default {info}; K = {K}, chunk rows {H}, strip columns {W}; {n} steps, periods {pe}/{me}/{se};"
          f" bands {[(b[0], b[1]) for b in pl['bands']]}; bodies {[b['cells'] for b in bands.items] + [n4]} counted cells, force bar at"
          f" most {cond:.3f} of half the smallest link; set-up {time.time() - t0:.1f} s (oracle {t2 - t1:.1f} s)")
    _SHAPE[shape] = dict(p=p, ob=ob, cells=cells, pl=pl, bands=bands, K=K, H=H, W=W, n=n, periods=(pe, me, se), g=g, wave=wave,
                         want=want, info=info, av0=av0, st0=st0, S=S, P1=P1, F1=F1, final=final, blocked=ob != 0)
    return _SHAPE[shape]


def _expected_keys(call, wave, n, K, pe, me, se):
    want = {}
    if call in CALLS[:4]:
        i = ("forces", "probes", "fields", "mean").index(call)
        want[WAVE_KEYS[i]] = 1 if wave else 0
        want[TILE_KEYS[i]] = 0
    elif call == "pair":
        want.update(observed_in_wave=3 if wave else 0, observed_in_kernel=0)
        if wave:
            want["observed_pieces"] = 1
    else:                                             # the pieces end on the sample steps of the means and the snapshots
        cuts = sorted({n} | set(range(me, n + 1, me)) | set(range(se, n + 1, se)) | (set() if wave else set(range(pe, n + 1, pe))))
        pieces = np.diff([0] + cuts)
        want.update(observed_pieces=len(pieces), observed_in_wave=3 if wave and pieces.max() >= K else 0, observed_in_kernel=0)
    if wave and call != "all":
        want["wave_launches"] = n // K                # a fresh context: one lbm_wave kernel per pass
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("shape,call", CASES, ids=[f"{s[0]}x{s[1]}-{c}" for s, c in CASES])
def test_observers_where_the_default_engine_runs(gpu, O, shape, call):
    L = gpu
    t_start = time.time()
    c = _setup(L, O, shape)
    nx, ny = shape
    p, ob, cells, pl, bands, K, n, wave = c["p"], c["ob"], c["cells"], c["pl"], c["bands"], c["K"], c["n"], c["wave"]
    pe, me, se = c["periods"]
    g, S = c["g"], c["S"]
    xy = pl["xy"]
    where = (shape, call, n, pe, me, se)
    const = np.array([0.0, 0.0, 0.0, np.float32(p.density) * ONE_THIRD], dtype=np.float32)
    path = []

    def run(fn):
        with L.Lattice(p, ob, cells) as lat:
            lat.set_bodies(pl["body"], NBODIES)
            lat.set_probes(xy)
            out = fn(lat)
            want = _expected_keys(call, wave, n, K, pe, me, se)
            keys = {k: int(lat.info(k)) for k in want}
            info = {k: int(lat.info(k)) for k in ENGINE_KEYS}
            print(f"  {nx}x{ny} {call}: {info} {keys}")
            path.append((keys, want, info, lat.info("compute_units") == 256 and lat.info("wave_capacity") == 2048))
            st = lat.read_state()
        assert np.array_equal(_bits(st), _bits(c["st0"])), (where, "lattice")
        return out

    def check_path():
        """Last, behind the values: a quiet fall-back gives the same bits and fails here alone."""
        (keys, want, info, pinned), = path
        assert keys == want, (where, "the path", keys, want)
        for k, v in c["want"].items():
            assert info[k] == v, (where, k, info)
        assert (info["wave_rows"] if wave else info["march_rows"]) == c["H"] and info["time_block_active"] == K, (where, info)
        if wave:                                      # the chunk height, the columns per lane and the strip width of lbm_run
            for k in PLAN_KEYS:
                assert info[k] == c["info"][k], (where, k, info, c["info"])
            assert info["wave_out_cols"] == c["W"], (where, info)
        if (nx, ny) in CHUNK_ROWS and pinned:
            assert c["H"] in CHUNK_ROWS[(nx, ny)], c["H"]

    def check_av(av, exact=True):
        if wave and exact:
            assert np.array_equal(_bits(av), _bits(c["av0"])), (where, "av_vels")
        assert np.allclose(av, c["av0"], rtol=2e-6, atol=0), (where, "av_vels")

    def check_fields(fields):
        want = S[se // g - 1::se // g][:n // se]
        assert fields.shape == want.shape == (n // se, ny, nx, 4)
        worst = 0.0
        for j in range(n // se):
            assert np.array_equal(_bits(fields[j]), _bits(want[j])), (where, "snapshot", j)
            assert np.all(_bits(fields[j][c["blocked"]]) == _bits(const)), (where, "blocked cells of snapshot", j)
            worst = max(worst, bands.check_fields(fields[j], (j + 1) * se, where))
        return worst

    def check_probes(probes):
        assert probes.shape == c["P1"].shape == (n // pe, len(xy), 4)
        bad = np.argwhere(_bits(probes) != _bits(c["P1"]))
        assert len(bad) == 0, (where, "probes", len(bad), [(int(j), tuple(xy[i]), int(k)) for j, i, k in bad[:8]])
        blocked = c["blocked"][xy[:, 1], xy[:, 0]]
        assert blocked.any() and np.all(_bits(probes[:, blocked]) == _bits(const)), (where, "blocked probes")
        worst, shared = 0.0, 0
        for j in range(n // pe):
            t = (j + 1) * pe
            if t % g == 0:                            # a step the split snapshots hold too
                shared += 1
                assert np.array_equal(_bits(probes[j]), _bits(S[t // g - 1][xy[:, 1], xy[:, 0]])), (where, "probes against the snapshot", t)
            worst = max(worst, bands.check_probes(probes[j], t, where))
        assert shared >= 1
        return worst

    def check_mean(mean):
        steps = list(range(me, n + 1, me))
        assert np.array_equal(_bits(mean), _bits(mean_of(S[me // g - 1::me // g][:len(steps)]))), (where, "mean")
        return bands.check_mean(mean, steps, where)

    def check_forces(F):
        assert F.shape == (n, NBODIES, 2)
        assert np.array_equal(_bits(F), _bits(c["F1"])), (where, "forces", float(np.abs(F - c["F1"]).max()))
        worst = bands.check_forces(F, where)
        fin = c["final"]
        last, frac = 0.0, np.zeros(NBODIES)
        for b in range(NBODIES):
            bar = (math.ceil(int(fin["cells"][b]) / 256) + 8) * U * fin["A"][b]
            d = np.abs(F[n - 1, b].astype(np.float64) - fin["F"][b])
            assert np.all(d <= bar), (where, "forces from the final lattice", b + 1, d, bar)
            last = max(last, float(np.max(d / bar)))
            frac[b] = float(np.max(d / fin["A"][b]))
        print(f"  {nx}x{ny} {call}: forces at most {worst:.3f} of the band bar; at the last step {last:.4f} of the bar from the final"
              f" lattice, |F - F64| / A_b = {', '.join(f'{v:.2e}' for v in frac)} for {fin['cells'].tolist()} counted cells")
        return worst

    if call == "fields":
        av, fields = run(lambda lat: lat.run_sampled(n, se))
        check_av(av)
        print(f"  {nx}x{ny} fields: {n // se} snapshots at most {check_fields(fields):.3f} of the bar in the bands")
    elif call == "probes":
        av, probes = run(lambda lat: lat.run_probes(n, pe))
        check_av(av)
        print(f"  {nx}x{ny} probes: {pl['in_band'].sum()} of {len(xy)} probes in the bands at most {check_probes(probes):.3f} of the bar")
    elif call == "mean":
        av, mean = run(lambda lat: lat.run_mean(n, me))
        check_av(av)
        print(f"  {nx}x{ny} mean: m = {n // me}, at most {check_mean(mean):.3f} of the bar in the bands")
    elif call == "forces":
        av, F = run(lambda lat: lat.run_forces(n))
        check_av(av)
        check_forces(F)
    elif call == "pair":
        res = run(lambda lat: lat.run_observed(n, forces=True, probes_every=pe))
        check_av(res["av_vels"])
        check_forces(res["forces"])
        print(f"  {nx}x{ny} pair: probes at most {check_probes(res['probes']):.3f} of the bar")
    else:
        res = run(lambda lat: lat.run_observed(n, forces=True, probes_every=pe, mean_every=me, fields_every=se))
        check_av(res["av_vels"], exact=False)         # (cut into pieces shorter than K: the small kernels' sums)
        check_forces(res["forces"])
        print(f"  {nx}x{ny} all: probes {check_probes(res['probes']):.3f}, mean {check_mean(res['mean']):.3f}, snapshots"
              f" {check_fields(res['fields']):.3f} of their bars")
    check_path()
    print(f"  {nx}x{ny} {call}: {time.time() - t_start:.1f} s")


# ---------------------------------------------------------------------------------------------------------------- 2^31 floats, 2^32 bytes
BIG = (8192, 1024)
BIG_STEPS, BIG_HOST_STEPS = 65, 33
BIG_CHECKED = (0, 31, 32, 63, 64)
NEED_BYTES = 9 * 2 ** 30


def test_the_big_output_crosses_what_it_claims():
    nx, ny = BIG
    slot = ny * nx * 4                                # floats per snapshot
    assert slot * 4 == 128 * 2 ** 20 and 32 * slot * 4 == 2 ** 32 and 64 * slot == 2 ** 31
    assert (BIG_STEPS - 1) * slot >= 2 ** 31 and BIG_HOST_STEPS * slot * 4 > 2 ** 32 >= (BIG_HOST_STEPS - 1) * slot * 4
    assert BIG_STEPS * slot * 4 < NEED_BYTES and set(BIG_CHECKED) >= {31, 32, 63, 64}
    assert 2 * BIG_STEPS + BAND < ny                  # the light cone of 65 rows either side of a band: the band path


def _big_outputs_child():
    """Runs in the child process, torch imported first.  Skips, with the reason, where the device has less than 9 GiB
    free: the output takes 8.125 GiB, the context's two lattices 0.56 GiB, its maps 0.04 GiB."""
    import torch
    import advanced_hpc_lbm_amd as L
    import lbm_oracle as O
    t0 = time.time()
    nx, ny = BIG
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_BYTES:                                 # (the output 8.125 GiB, two lattices 0.56 GiB, the maps 0.04 GiB)
        print(f"SKIP: {free / 2 ** 30:.1f} GiB of device memory free, the output and the lattice need {NEED_BYTES / 2 ** 30:.0f} GiB")
        return
    K, H, W = _default_plan(L, nx, ny)
    with L.Lattice(L.Param(nx, ny, 10, 10, *PARAMS), np.zeros((ny, nx), np.int32)) as lat:      # what a plain lbm_run reports
        lat.run(K)
        plain = {k: int(lat.info(k)) for k in ENGINE_KEYS}
    for k, v in SHAPES[BIG][0].items():
        assert plain[k] == v, (k, plain)
    assert plain["wave_rows"] == H and plain["wave_out_cols"] == W and plain["time_block_active"] == K, (plain, K, H, W)
    keys = ("samples_in_wave", "samples_in_kernel", "wave_launches", "engine_last", "march_kernel") + PLAN_KEYS
    p, ob, cells = _case(L, nx, ny, nx * 7 + ny, H, W)
    pl = _place(nx, ny, H, W, ob, FEW_PROBES)
    steps = [j + 1 for j in BIG_CHECKED]
    bands = BandRuns(O, _orc_param(O, nx, ny), ob, cells, pl, BIG_STEPS, steps)
    t1 = time.time()
    want = {}
    with L.Lattice(p, ob, cells) as lat:                  # lbm_final_state after lbm_run of that many steps, the split path
        for k, v in SPLIT:
            lat.set_option(k, v)
        done = 0
        for t in steps:
            lat.run(t - done)
            done = t
            want[t] = lat.final_state()
        assert lat.info("time_block_active") == 1 and lat.info("engine_last") == 1
    worst = 0.0
    # device output
    out = torch.full((BIG_STEPS, ny, nx, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    assert out.numel() > 2 ** 31 and out.numel() * 4 > 2 ** 33
    with L.Lattice(p, ob, cells) as lat:
        av, got = lat.run_sampled(BIG_STEPS, 1, out=out)
        info = {k: int(lat.info(k)) for k in keys}
        print(f"device output: {info}")
        assert got is out and info["samples_in_wave"] == 1 and info["samples_in_kernel"] == 0 and info["engine_last"] == 1, info
        assert info["wave_launches"] == BIG_STEPS // K and info["march_kernel"] == 1, info
        for k in PLAN_KEYS:
            assert info[k] == plain[k], ("device output", k, info, plain)
    torch.cuda.synchronize()
    for j in range(BIG_STEPS):
        if j in BIG_CHECKED:
            x = out[j].cpu().numpy()
            assert np.array_equal(_bits(x), _bits(want[j + 1])), ("device output", j)
            worst = max(worst, bands.check_fields(x, j + 1, ("device output", j)))
        else:
            assert not bool(torch.isnan(out[j]).any()) and bool((out[j, :, :, 3] > 0).all()), ("device output", j)
    del out, got
    torch.cuda.empty_cache()
    t2 = time.time()
    # host output: the staging and the copy-out cross 2^32 bytes
    with L.Lattice(p, ob, cells) as lat:
        av, fields = lat.run_sampled(BIG_HOST_STEPS, 1)
        info = {k: int(lat.info(k)) for k in keys}
        print(f"host output: {info}")
        assert info["samples_in_wave"] == 1 and info["samples_in_kernel"] == 0 and info["wave_launches"] == BIG_HOST_STEPS // K, info
        assert info["engine_last"] == 1 and info["march_kernel"] == 1, info
        for k in PLAN_KEYS:
            assert info[k] == plain[k], ("host output", k, info, plain)
    assert fields.nbytes > 2 ** 32
    for j in range(BIG_HOST_STEPS):
        if j in BIG_CHECKED:
            assert np.array_equal(_bits(fields[j]), _bits(want[j + 1])), ("host output", j)
            worst = max(worst, bands.check_fields(fields[j], j + 1, ("host output", j)))
        else:
            assert not np.isnan(fields[j]).any() and np.all(fields[j][..., 3] > 0), ("host output", j)
    print(f"big outputs ok: snapshots at most {worst:.3f} of the bar in the bands; oracle {t1 - t0:.1f} s, device {t2 - t1:.1f} s,"
          f" host {time.time() - t2:.1f} s")


_BIG_OUTPUTS = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import conftest
import test_large_observers
test_large_observers._big_outputs_child()
"""


@pytest.mark.gpu
def test_snapshot_outputs_past_2_31_floats_and_2_32_bytes(gpu):
    got = _child(_BIG_OUTPUTS)
    print(got)
    if "SKIP:" in got:
        pytest.skip(got[got.index("SKIP:") + 6:].strip())
    assert "big outputs ok" in got
