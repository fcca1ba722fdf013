"""lbm_run_window_stats away from the shipped decks: the 100 (path, point) cases of tests/test_stats_param_space.py -- the 20
observer paths at their four grid points and at "thirds" = (0.3, 0.01, 1.85) -- on the three windows of
tests/test_window_driven_param_space.py (windows_of: the whole extent at strides (3, 5), the accelerate row ny-2, 7 x 7 cells
across a column edge and a row edge of the path).

What the call's own files cannot see (they run at density 0.1, omega 1.85 and the decks' acceleration).  The density reaches
p0 in three places of its own: the argument of launch_window (the split paths), the argument of
lbm_window_stats_fold (the register tiles) and WaveArgs::density of lbm_wave's WINDOW+STATS flavour.  A site that kept 0.1
passes every test at the control point; one that formed p0 as density / 3.f passes wherever that is the float
density * (1.f / 3.f), which is every density of the grid that a smooth run has.  At "thirds" the two differ by one ulp:
test_thirds_tells_the_two_forms_of_p0_apart_in_every_window shows on the CPU that float 7 then differs in a cell of every window
of every path and is non-zero in its blocked cells, so the GPU test can tell.  And the accelerate row, the light fluid and
omega at the stability edge were never a window's cells.

Everything is test_stats_param_space's: its cases (_case), parameters (_lib_param, _oracle_param), states (thirds_state through
_case), blocked_record, its reference (_reference: the one-step kernel, one step at a time, S_t = read_state, X_t = final_state,
X_t held to the double oracle's final_state of S_t at 2e-6 |fo| + 8 x 2^-24) and its bounds (bounds_from_fields: bQ and the
variance bounds of that file's docstring, here on the window's cells of fo, X and the output; no tolerance of this file's own).

Periods: the case's mean period `me` (m >= 3, no power of two); on the lbm_wave paths every = 1 as well.
Chunk: on the tile paths "window_stats_chunk" is 0, 1 or 2 in turn by case index, so the grid runs the automatic single piece,
a piece per sample, and pieces of two samples with a cut last piece; with the tail piece wherever n is no multiple of every.

Per case and period one lbm_run_stats under the path's options; per window a fresh context under the path's options:

  bits       stats_out = stats_of(cut(X[every - 1:n:every], w), p0), p0 = float32(density) * (float32(1) / float32(3))
  the cut    stats_out = cut of lbm_run_stats' output
  blocked    a blocked window cell reads exactly blocked_record(p0, m)
  lattice    the bits of S_n
  av_vels    lbm_run's bits on the register tiles and on lbm_wave; within ENGINE_AV_RTOL (2e-6) elsewhere
  info       window_stats_in_kernel / window_stats_in_wave = 1/0 on the tiles, 0/1 on lbm_wave, 0/0 on the split paths; the
             path's own keys; window_stats_pieces = test_driven_observed.window_stats_pieces_of(n, every, chunk, kind)
  moments    floats 4..7 and the four variances against the double oracle's fields in the window's cells, inside
             bounds_from_fields' bounds; exactly 0 in blocked cells as that file states

No GPU: every case's windows are legal and together hold blocked and fluid cells; at a refusing point the accelerate-row window
holds, in front of a sample step, a cell the guard refused and one it accepted on the float oracle; the piece count agrees with
the four (chunk, pieces) pairs of tests/test_window_stats_run.py's test_chunk_cuts_change_nothing.

Measured on one MI355X (printed by the tests; DESIGN.md section 4, "Window stats on the grid"): the second moments at most
0.053 of their bound (wave8 at refusal), the variances at most 0.034 of theirs (march at refusal) -- below the whole lattice's
0.058 and 0.036, as a subset's must be; 38.1 s for the 100 cases beside tests/test_stats_param_space.py's 23.4 s in the same
visit (1.6 times: three windows a case, not two in rotation).  All 100 passed on the library as it stood: nothing found."""
import time

import numpy as np
import pytest

import test_observer_param_space as OBS
from test_driven_observed import window_stats_pieces_of
from test_observer_param_space import PATHS, U, _bits
from test_param_space import ENGINE_AV_RTOL, REFUSING
from test_stats_param_space import (CASES, THIRDS, THIRDS_STEPS, _case, _everys, _float_oracle_fields, _lib_param, _oracle_param,
                                    _reference, _steps, _triple, blocked_record, bounds_from_fields, double_oracle_fields, p0_divided)
from test_stats_run import p0_of, stats_of
from test_window_driven_param_space import _blocked_in, windows_of
from test_window_run import cut

WINDOW_NAMES = ("strided", "accelerate row", "7 x 7")


def _chunk(path, point):
    """window_stats_chunk of a case on the tile paths: 0, 1, 2 in turn by case index (None elsewhere: the option is left alone)"""
    return CASES.index((path, point)) % 3 if PATHS[path][6] == "tiles" else None


def _cut8(a, w):
    return cut(a[None], w)[0]


def _most_cells(path, w):
    """the window cells of the slab that holds the most (automatic chunk: the staging bound)"""
    ny = PATHS[path][1]
    ns = PATHS[path][5].get("nslabs", 1)
    rows = [w.y0 + r * w.sy for r in range(w.ny)]
    return w.nx * max(sum(s * ny // ns <= y < (s + 1) * ny // ns for y in rows) for s in range(ns))


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_the_piece_count_is_what_the_chunk_test_asserts():
    """(tests/test_window_stats_run.py, test_chunk_cuts_change_nothing: 13 steps at every = 2)"""
    for chunk, pieces in ((0, 2), (1, 7), (2, 4), (4, 3)):
        assert window_stats_pieces_of(13, 2, chunk, "tiles") == pieces
        assert window_stats_pieces_of(13, 2, chunk, "tiles", cells=128 * 128) == pieces
    assert window_stats_pieces_of(13, 2, 3, "wave") == 1 and window_stats_pieces_of(13, 2, 3, "split") == 7
    assert window_stats_pieces_of(12, 2, 0, "tiles") == 1 and window_stats_pieces_of(12, 2, 4, "split") == 6
    assert window_stats_pieces_of(11, 2, 2, "tiles") == 4          # (test_one_context_through_mixed_calls: 2, 4 | 6, 8 | 10 | tail)
    assert window_stats_pieces_of(9, 1, 0, "tiles", cells=1024 * 1024) == 3      # 16 MiB a sample: four to a piece


def test_the_chunks_meet_every_kind_of_piece():
    """Over the tile cases: every chunk value at every point kind; chunk 2 with a cut last piece (m odd) and chunk 1 or 2 with a
    tail somewhere; every path meets two chunk values at least."""
    tiles = [(path, point) for path, point in CASES if PATHS[path][6] == "tiles"]
    assert len(tiles) == 40
    seen = {}
    for path, point in tiles:
        _, _, _, n, me, *_ = _case(path, point)
        seen.setdefault(_chunk(path, point), []).append((n // me, n % me != 0, point))
    assert set(seen) == {0, 1, 2}
    assert any(m % 2 for m, _, _ in seen[2]) and any(t for _, t, _ in seen[1]) and any(t for _, t, _ in seen[2]) and any(t for _, t, _ in seen[0])
    for c in (0, 1, 2):
        assert {pt for _, _, pt in seen[c]} >= {"thirds", "refusal", "stability_edge", "light_fluid"}, c
    for path in {p for p, _ in tiles}:
        assert len({_chunk(path, pt) for p, pt in tiles if p == path}) >= 2, path


@pytest.mark.parametrize("path,point", CASES)
def test_windows_hold_what_they_claim(L, O, oracle, path, point):
    nx, ny, K, n, me, kind, ob, cells, _, _ = _case(path, point)
    ws = windows_of(L, path, ob)
    assert len(ws) == 3
    held = []
    for w in ws:
        assert w.nx >= 1 and w.ny >= 1 and 0 <= w.x0 and 0 <= w.y0 and w.sx >= 1 and w.sy >= 1
        assert w.x0 + (w.nx - 1) * w.sx < nx and w.y0 + (w.ny - 1) * w.sy < ny, w
        assert L.window_rows(w, nx, ny, 0, ny) == (0, w.ny)
        held.append(_blocked_in(ob, w))
        assert held[-1].shape == (w.ny, w.nx)
    assert any(b.any() for b in held) and any((~b).any() for b in held), (path, point)
    whole, row, rect = ws
    assert (whole.sx, whole.sy) == (3, 5) and (row.x0, row.y0, row.nx, row.ny) == (0, ny - 2, nx, 1) and (rect.nx, rect.ny) == (7, 7)
    if point in REFUSING:
        # step t's accelerate shapes the fields of step t: a sample step t >= 2 (or a step in front of one) at which the guard
        # refused one fluid cell of the row and accepted another
        steps = _steps(O, oracle, path, point, n)
        fluid = ob[ny - 2] == 0
        last = n // me * me
        assert any((steps[t - 1][2] & fluid).any() and (~steps[t - 1][2] & fluid).any() for t in range(2, last + 1)), (path, point)


_THIRDS_X = {}


def _thirds_fields(O, oracle, path):
    """X_t of the strict float oracle at "thirds" over THIRDS_STEPS steps, once per shape (one state per shape there)"""
    nx, ny, _, _, _, _, ob, cells, _, _ = _case(path, "thirds")
    if (nx, ny) not in _THIRDS_X:
        prm = O.OrcParam(nx, ny, 100, 10, *(float(np.float32(v)) for v in THIRDS))
        X = _float_oracle_fields(oracle, prm, ob, cells, THIRDS_STEPS)
        X.setflags(write=False)
        _THIRDS_X[(nx, ny)] = (ob, X)
    held, X = _THIRDS_X[(nx, ny)]
    assert held is ob or np.array_equal(held, ob)
    return X


@pytest.mark.parametrize("path", list(PATHS))
def test_thirds_tells_the_two_forms_of_p0_apart_in_every_window(L, O, oracle, path):
    """On the float oracle's fields of the case at "thirds", at each of its periods and in each of its windows: the expected
    output under p0 = density / 3.f has the same floats 0..6 and another float 7 in at least one cell, and in EVERY blocked
    cell of the window (where the right float 7 is +0 and the wrong one is positive); under density 0.1 likewise."""
    nx, ny, K, n, me, kind, ob, cells, _, _ = _case(path, "thirds")
    X = _thirds_fields(O, oracle, path)
    assert n <= THIRDS_STEPS
    p0 = p0_of(THIRDS[0])
    assert _bits(p0) != _bits(p0_divided(THIRDS[0]))
    for every in _everys(path, "thirds"):
        m = n // every
        for w in windows_of(L, path, ob):
            Xw = cut(X[every - 1:n:every][:m], w)
            want = stats_of(Xw, p0)
            blocked = _blocked_in(ob, w)
            assert np.all(_bits(want[blocked]) == _bits(blocked_record(p0, m)))
            for other in (p0_divided(THIRDS[0]), p0_of(0.1)):
                got = stats_of(Xw, other)
                differ = _bits(got[..., 7]) != _bits(want[..., 7])
                assert np.array_equal(_bits(got[..., :7]), _bits(want[..., :7])) and differ.any(), (path, every, w)
                assert differ[blocked].all() and np.all(got[blocked][:, 7] > 0), (path, every, w)


# ---------------------------------------------------------------------------------------------------------------- GPU
WORST = {"moments": 0.0, "variances": 0.0, "seconds": 0.0}


@pytest.mark.gpu
@pytest.mark.parametrize("path,point", CASES)
def test_window_stats_on_the_parameter_grid(gpu, O, monkeypatch, path, point):
    L = gpu
    t0 = time.perf_counter()
    nx, ny, K, n, me, kind, ob, cells, body, xy = _case(path, point)
    _, _, _, options, info_want, kw, pkind = PATHS[path]
    ref = _reference(L, O, path, point)
    p, prm = _lib_param(L, point, nx, ny), _oracle_param(O, point, nx, ny)
    p0 = p0_of(p.density)
    assert _bits(p0) == _bits(p0_of(_triple(point)[0]))
    chunk = _chunk(path, point)
    ws = windows_of(L, path, ob)

    def call(name, fn, every=0, w=None):
        where = (path, point, n, every, name, w, chunk)
        with OBS._open(L, path, p, ob, cells, body, xy, monkeypatch) as lat:
            if name == "window_stats" and chunk is not None:
                lat.set_option("window_stats_chunk", chunk)
            out = fn(lat)
            if name == "window_stats":
                got = {k: int(lat.info(k)) for k in ("window_stats_in_kernel", "window_stats_in_wave", "window_stats_pieces")}
                want = dict(window_stats_in_kernel=int(pkind == "tiles"), window_stats_in_wave=int(pkind == "wave"),
                            window_stats_pieces=window_stats_pieces_of(n, every, chunk or 0, pkind, _most_cells(path, w)))
                assert got == want, (where, got, want)
            for key, v in info_want.items():
                if key == "exchange":
                    v = {"rccl": L.EXCHANGE_RCCL}[v]
                assert lat.info(key) == v, (where, key, lat.info(key))
            st = lat.read_state()
        return out, st

    av0, st0 = call("plain", lambda lat: lat.run(n))
    assert np.array_equal(_bits(st0), _bits(ref["S"][n - 1])), (path, point, "the lattice of the one-step kernel")
    worst = [0.0, 0.0]
    for every in _everys(path, point):
        m = n // every
        (_, full), _ = call("stats", lambda lat: lat.run_stats(n, every), every)
        Xs, Ss = ref["X"][every - 1:n:every][:m], ref["S"][every - 1:n:every][:m]
        fo = double_oracle_fields(O, prm, ob, Ss)
        const = blocked_record(p0, m)
        for wname, w in zip(WINDOW_NAMES, ws):
            where = (path, point, n, every, wname, chunk)
            (av, out), st = call("window_stats", lambda lat: lat.run_window_stats(n, every, w), every, w)
            want = stats_of(cut(Xs, w), p0)
            assert out.shape == want.shape == (w.ny, w.nx, 8) and out.dtype == np.float32, where
            bad = np.argwhere(_bits(out) != _bits(want))
            assert len(bad) == 0, (where, "stats_of the cut", len(bad), [tuple(int(v) for v in b) for b in bad[:8]])
            assert np.array_equal(_bits(out), _bits(_cut8(full, w))), (where, "the cut of lbm_run_stats")
            blocked = _blocked_in(ob, w)
            assert np.all(_bits(out[blocked]) == _bits(const)), (where, "blocked cells")
            assert np.array_equal(_bits(st), _bits(ref["S"][n - 1])), (where, "lattice")
            if pkind in ("tiles", "wave"):
                assert np.array_equal(_bits(av), _bits(av0)), (where, "av_vels")
            assert av.shape == (n,) and np.allclose(av, av0, rtol=ENGINE_AV_RTOL, atol=0), (where, "av_vels")
            rQ, rV = bounds_from_fields(cut(fo, w), blocked, cut(Xs, w), out, p0)
            worst = [max(worst[0], rQ), max(worst[1], rV)]
    WORST["moments"], WORST["variances"] = max(WORST["moments"], worst[0]), max(WORST["variances"], worst[1])
    WORST["seconds"] += time.perf_counter() - t0
    print(f"{path} {point}: {n} steps, every {_everys(path, point)}, chunk {chunk}; second moments {worst[0]:.3f} of their bound,"
          f" variances {worst[1]:.3f} of theirs; worst so far: {WORST['moments']:.3f}, {WORST['variances']:.3f};"
          f" {WORST['seconds']:.1f} s in this test so far")
