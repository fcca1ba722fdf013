"""One context through live maps, restarts and every observer call: lbm_set_obstacles and lbm_write_state among the running
calls of ONE long-lived context, in the manner of tests/test_observer_sequences.py (a table of programs, a model, a coverage
check without a GPU, one GPU runner).

New table entries: set_map(name, refill), write(name), refused_live(what).  lbm_run_stats is the tenth kind of running call
(TEN): on every path family it is the first call behind a map change under either refill, and behind a write.
lbm_run_window_stats is the eleventh (ELEVEN), in four programs of its own: likewise the first call behind either refill on every
path family and behind a write, and twice over one window either side of a LBM_REFILL_REST that turns cells of the window both
ways -- lbm_window_stats_add and the tiles read the live blocked bytes while the window table's key still hits.

The shadow never takes a live input.  It stays the one-step kernel (engine 1, time_block 1, a lattice alone; a slab context
where slabs add up forces off the tiles, as in the older file), and at every live input it is DESTROYED AND CREATED AGAIN by
lbm_create from (new map, S'): S' made in numpy from the shadow's own read_state by the header's definition
(test_live_inputs.s_prime with rest_values), or the written array; the acceleration, the bodies (behind a write) and the step
count are carried over.  So the live context is held to "the context lbm_create would have made", never to a second call of
lbm_set_obstacles.

After every call, as the older runner: the outputs bit for bit against numpy on the shadow's per-step fields, forces on the
tiles by test_body_forces._close against forces_from_state under the CURRENT map (elsewhere the shadow's run_forces(1) bits),
the lattice bit for bit, av_vels (AV_RTOL; bit for bit on tb1 of a lattice alone), the path and the info keys, regtile_tag
(a live input leaves it), info("accel"); and obstacle_updates, refilled_cells and fluid_cells against numpy.  After every
live input also read_state against S' and test_call_sequences._check_derived (total_density to 1e-12 of the double sum of
in-order float cell sums, av_velocity, reynolds) under the new map.  The shadow is anchored to the strict float oracle over
each program's first <= 50 steps at the bars of the older file (hold_anchor), the oracle run piecewise with the map swapped
and the refill applied in numpy between the pieces; every program has at least two live inputs inside those steps, one of
them a LBM_REFILL_REST that refills cells.

Maps.  Every case has A, B, C and "empty".  A is the builder's map with the stamps below; B and C are A with 2 % of the
cells flipped at random (seeded) and the same stamps: in every special row (0, 1, ny-3, ny-2, ny-1, either side of every
slab seam, of a tile seam of the program's tilings and of a wave_rows chunk edge) and every special column (0, nx-1, 63, 64)
six cells take the six patterns of (A, B, C) that are not constant, so that every ordered pair of the three has cells
changing in both directions in each of those places, and every LBM_REFILL_REST between two of them refills there.  (A call
from "empty" can refill nothing; one to "empty" refills every obstacle.)  C marks its blocked cells 1, 2, -1 and INT_MIN in
turn.  The labelling "U" labels every cell that any map blocks: under each map it holds newly blocked cells and labels on
fluid cells, which the contract ignores.  The probe set "L" and the window "live" hold the stamps of two special rows.

The start.  The decks' builders start from rest, where the step averages are 1e-5 .. 3e-4 and the anchor's rtol 1e-4 on av_vels
is an absolute 1e-9 .. 3e-8: less than the rounding of one cell's speed (2^-24 = 6e-8; tests/test_param_space.py allows a step
average 4 x 2^-24).  Measured on the stamped 128 x 128 deck from rest, the one-step kernel alone, no live input: every step
within 3 u rho of the double oracle from the kernel's own state (the float oracle: 3.9), and the free-running step average
+6.8e-5 from the double oracle's by step 21 (the float oracle's: -1e-5); with B refilled behind step 5 and C behind step 12
+1.7e-4 at steps 14 .. 17, under kernel_variant 0 as well, each single step still within 3.3 u rho.  So three programs that
stay near rest for all their anchored steps ("tiles_128_every_kind_behind_a_map", the 256 x 256 walk and the four slabs)
start from the rest equilibrium +-10 % at random, as the builders of the smaller cases do; "tiles_128_writes_and_pairs" and the
rank rings keep the start from rest.  The bars are the older file's, unchanged."""
import time

import numpy as np
import pytest

from test_body_forces import _close
from test_call_sequences import (ANCHOR_STEPS, TILE_PATHS, _check_derived, _kept, _labels, _open, _p1, _p2, _p3, _p4, _p5, _p6, _p7,
                                 bodies, forces, opt, run, sampled)
from test_driven_observed import mean_from_fields
from test_driven_run import AV_RTOL, driven_oracle
from test_live_inputs import KEEP, LBM_EINVAL, REST, refilled, rest_values, s_prime
from test_observer_sequences import (B3, B5, B9, FP, F, InChunks, M, ObserverModel, P, S, Shadow, _call, _chains, _check_engine,
                                     _is, _probe_sets, _refuse, _same, _schedule, driven, driven_observed, hold_anchor, mean, observed,
                                     probe_set, probes, refused, stats, window, window_stats)
from test_stats_run import p0_of, stats_of
from test_window_run import cut

NINE = ("run", "sampled", "forces", "probes", "mean", "observed", "window", "driven", "driven_observed")
TEN = NINE + ("stats",)
ELEVEN = TEN + ("window_stats",)
INT_MIN = -2 ** 31
PATTERNS = ((0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0))      # (A, B, C) in the six stamped cells
WAVE_ROWS = 24
SCHEDS = (B3, B5, B9)


# ---------------------------------------------------------------------------------------------------------------- table
def set_map(name, refill):
    return ("set_map", name, refill)


def write(name):
    return ("write", name)


def refused_live(what):
    """A live input that must return LBM_EINVAL: "null map", "refill 2", "refill -1", "null cells"."""
    return ("refused_live", what)


def _kind_call(kind, path, K, i):
    """The call of `kind` on a path of K steps per pass: two passes and one step more, sample steps at level K."""
    n, ev = (2 * K + 1, K) if K > 1 else (7, 3)
    return {"run": run(n, path), "sampled": sampled(n, ev, path), "forces": forces(n, path), "probes": probes(n, 2, path),
            "mean": mean(n, ev, path), "observed": observed(n, (F, P, M), 2, ev, 0, path), "window": window(n, ev, "live", path),
            "driven": driven(n, SCHEDS[i % 3], path),
            "driven_observed": driven_observed(n, SCHEDS[(i + 1) % 3], FP, 2, 0, 0, path), "stats": stats(n, ev, path),
            "window_stats": window_stats(n, ev, "live", path)}[kind]


def _relabel():
    return [refused("forces", 3), bodies("U", 3)]


CYCLE = (("B", REST), ("C", KEEP), ("A", REST), ("B", REST), ("C", REST), ("A", KEEP), ("B", REST), ("C", REST), ("A", REST), ("B", REST),
         ("C", KEEP))


def each_kind_behind_a_map(path, K, kinds=TEN):
    """From map A: every kind in turn as the first running call behind a set_map (B, C, A, B, ... : never the map in
    place); a kind that takes forces follows refused("forces") and a relabel; stats, the last of the ten, behind a
    LBM_REFILL_REST and once more behind a LBM_REFILL_KEEP."""
    out = []
    for i, kind in enumerate(kinds):
        out.append(set_map(*CYCLE[i]))
        if kind in ("forces", "observed", "driven_observed"):
            out += _relabel()
        out.append(_kind_call(kind, path, K, i))
    if kinds is TEN:
        out += [set_map(*CYCLE[10]), _kind_call("stats", path, K, 10)]
    return out


def each_kind_behind_a_write(path, K):
    return [c for i, kind in enumerate(TEN) for c in (write("W" if i % 2 == 0 else "V"), _kind_call(kind, path, K, i))]


def same_tables_across_a_map(path, K, first, second):
    """The same window, then the same probe set, on both sides of a set_map with nothing set again between."""
    return [_kind_call("window", path, K, 0), set_map(*first), _kind_call("window", path, K, 1),
            _kind_call("probes", path, K, 0), set_map(*second), _kind_call("probes", path, K, 1)]


# ---------------------------------------------------------------------------------------------------------------- cases
def _spread(allowed, k):
    return [allowed[(j * len(allowed) // 6 + 5 * k) % len(allowed)] for j in range(6)]


def _live_case(L, builder, tiling, rows, live_rows, stirred=False):
    """The builder's case with maps A, B, C, "empty" (module docstring), the labelling "U", the probe set "L", the window
    "live" (the full width of the two rows live_rows) and the written lattices "W" and "V"; stirred: the start is the rest
    equilibrium +-10 % at random instead of the builder's (module docstring, "The start")."""
    p, ob, cells, _ = builder(L)
    nx, ny = p.nx, p.ny
    srows = sorted({0, 1, ny - 3, ny - 2, ny - 1} | set(rows))
    scols = sorted({0, nx - 1, 63, 64})
    rng = np.random.default_rng(nx * 13 + ny)
    A = np.array(ob, dtype=np.int32)
    maps = [A, np.where(rng.random((ny, nx)) < 0.02, 1 - A, A).astype(np.int32), np.where(rng.random((ny, nx)) < 0.02, 1 - A, A).astype(np.int32)]
    free_cols = [x for x in range(nx) if x not in scols]
    free_rows = [y for y in range(ny) if y not in srows]
    stamps = {}
    for k, r in enumerate(srows):
        stamps[("row", r)] = [(r, x) for x in _spread(free_cols, k)]
    for k, c in enumerate(scols):
        stamps[("col", c)] = [(y, c) for y in _spread(free_rows, k)]
    for where in stamps.values():
        assert len(set(where)) == 6
        for (y, x), pat in zip(where, PATTERNS):
            for m, v in zip(maps, pat):
                m[y, x] = v
    C = maps[2]
    blocked = np.flatnonzero(C.reshape(-1))
    C.reshape(-1)[blocked] = np.array([1, 2, -1, INT_MIN], np.int32)[np.arange(len(blocked)) % 4]
    maps = {"A": maps[0], "B": maps[1], "C": C, "empty": np.zeros((ny, nx), np.int32)}
    union = ((maps["A"] != 0) | (maps["B"] != 0) | (maps["C"] != 0)).astype(np.int32)
    w = rest_values(p.density)
    writes = {k: (w * (np.float32(1) + np.float32(0.2) * (np.random.default_rng(s).random((ny, nx, 9), dtype=np.float32) - np.float32(0.5)))).astype(np.float32)
              for k, s in (("W", 3), ("V", 4))}
    if stirred:
        cells = (w * (np.float32(1) + np.float32(0.2) * (np.random.default_rng(5).random((ny, nx, 9), dtype=np.float32) - np.float32(0.5)))).astype(np.float32)
    xy = _probe_sets(p, maps["A"], tiling[0], tiling[1])["A"]
    mine = [(x, y) for r in live_rows for y, x in stamps[("row", r)]]
    have = {tuple(q) for q in xy.tolist()}
    xy = np.concatenate([xy, np.array([q for q in mine if q not in have], dtype=np.int32).reshape(-1, 2)])
    assert live_rows[1] == live_rows[0] + 1 and set(live_rows) <= set(srows)
    for a in list(maps.values()) + list(writes.values()) + [xy]:
        a.setflags(write=False)
    return dict(p=p, ob=maps["A"], cells=cells, labellings={"U": _labels(union, 17, 3)}, psets={"L": xy}, maps=maps, writes=writes,
                windows={"live": L.Window(0, live_rows[0], nx, 2)}, stamps=stamps, srows=srows, scols=scols, live_rows=live_rows)


_CASES = {}


def _cached(key, *args, **kw):
    def f(L):
        if key not in _CASES:
            _CASES[key] = _live_case(L, *args, **kw)
        return _CASES[key]
    return f


_l1 = _cached("128x128", _p1, (2, 1), (63, 64), (63, 64))                              # 128 x 128 deck, tiling 2 x 1
_l1s = _cached("128x128 stirred", _p1, (2, 1), (63, 64), (63, 64), stirred=True)
_l2 = _cached("256x256", _p2, (8, 4), (127, 128, WAVE_ROWS - 1, WAVE_ROWS), (127, 128), stirred=True)    # 256 x 256 deck, tilings 8 x 4 and 16 x 2
_l4 = _cached("130x37", _p7, (0, 1), (WAVE_ROWS - 1, WAVE_ROWS), (WAVE_ROWS - 1, WAVE_ROWS))  # never tiles; lbm_wave<6> in chunks of 24 and 13
_l5 = _cached("128x16", _p3, (2, 1), (7, 8), (7, 8))
_l6 = _cached("256x256 slabs", _p4, (4, 1), (63, 64, 127, 128, 191, 192, 67, 68), (63, 64), stirred=True)   # four slabs of 64 rows, tiling 4 x 1
_l7 = _cached("256x32 slabs", _p5, (2, 1), (15, 16, 7, 8), (15, 16))                   # two slabs of 16 rows
_l8 = _cached("1024x128 rank", _p6, (8, 1), (63, 64), (63, 64))                        # a rank ring of one: tiling 8 x 1

_START = [bodies("U", 3), probe_set("L")]
PROGRAMS = {
    "tiles_128_every_kind_behind_a_map": (_l1s, None, _START + [run(5, "tiles")] + each_kind_behind_a_map("tiles", 3)),
    "tiles_128_writes_and_pairs": (_l1, None, _START + [run(4, "tiles"), set_map("B", REST), bodies("U", 3)] + each_kind_behind_a_write("tiles", 3) + [
        # the pairs with no run between
        set_map("C", KEEP), set_map("A", REST), run(5, "tiles"),
        set_map("B", REST), bodies("U", 3), set_map("B", REST), refused("forces", 3), run(4, "tiles"),
        write("W"), set_map("C", REST), run(5, "tiles"),
        set_map("A", REST), write("V"), run(4, "tiles"),
        set_map("empty", REST), set_map("A", REST), run(5, "tiles"),
        refused_live("null map"), refused_live("refill 2"), refused_live("refill -1"), refused_live("null cells"), run(4, "tiles"),
    ] + same_tables_across_a_map("tiles", 3, ("B", REST), ("C", REST))),
    # the tiling changes mid-program; then the engines in turn, every switch behind a map call, every engine's first call
    # behind the switch under a map it has never run with
    "lone_256_retile_and_engine_walk": (_l2, None, _START + [
        opt("regtile", 84), run(5, "tiles"), set_map("B", REST), probes(7, 2, "tiles"),
        opt("regtile", 162), set_map("A", KEEP), window(7, 3, "live", "tiles"),
        set_map("C", REST), opt("time_block", 8), opt("wave_rows", WAVE_ROWS), mean(17, 8, "wave"),
        set_map("B", REST), opt("time_block", 4), opt("march_kernel", 0), probes(9, 4, "march"),
        set_map("C", REST), opt("engine", 3), bodies("U", 3), observed(7, FP, 2, 0, 0, "tiles"),
        set_map("B", KEEP), opt("time_block", 2), opt("engine", 1), window(5, 2, "live", "tb2"),
        set_map("A", REST), opt("time_block", 8), opt("march_kernel", 1), opt("wave_rows", WAVE_ROWS), driven(17, B3, "wave"),
        set_map("empty", REST), opt("time_block", 4), opt("march_kernel", 0), run(9, "march"),
        set_map("C", REST), opt("engine", 3), sampled(6, 3, "tiles"),
    ]),
    "never_tiles_tb1_tb2": (_l4, None, [opt("time_block", 1)] + _START + [run(5, "tb1")] + each_kind_behind_a_map("tb1", 1) + [
        opt("time_block", 2), run(4, "tb2")] + each_kind_behind_a_map("tb2", 2, ("probes", "forces", "mean", "driven_observed")) + [
        write("W"), window(5, 2, "live", "tb2"), refused_live("refill 2"), run(3, "tb2"), write("V"), stats(5, 2, "tb2")]),
    "wave6_130x37_every_kind_behind_a_map": (_l4, None, [opt("time_block", 6), opt("wave_rows", WAVE_ROWS)] + _START + [run(13, "wave")]
                                             + each_kind_behind_a_map("wave", 6)),
    "wave6_130x37_writes_and_tables": (_l4, None, [opt("time_block", 6), opt("wave_rows", WAVE_ROWS)] + _START + [run(14, "wave"), set_map("B", REST), bodies("U", 3)]
                                       + each_kind_behind_a_write("wave", 6) + same_tables_across_a_map("wave", 6, ("C", REST), ("A", REST)) + [
        refused_live("null map"), refused_live("null cells"), set_map("B", KEEP), set_map("C", REST), run(13, "wave")]),
    "lone_128x16_pairs": (_l5, None, _START + [
        run(3, "tiles"), set_map("B", KEEP), set_map("C", REST), refused("forces", 2), bodies("U", 3), forces(6, "tiles"),
        write("W"), set_map("A", REST), run(4, "tiles"), set_map("B", REST), write("V"), probes(6, 2, "tiles"),
        refused_live("refill -1"), set_map("empty", REST), set_map("B", REST), mean(6, 3, "tiles"),
    ]),
    "slabs_p2p_tiles_every_kind_behind_a_map": (_l6, ("slabs", 4, "p2p"), _START + [run(5, "slab-tiles")] + each_kind_behind_a_map("slab-tiles", 3)
                                                + same_tables_across_a_map("slab-tiles", 3, ("B", REST), ("C", REST)) + [
        bodies("U", 3), write("W"), forces(4, "slab-tiles"), refused_live("refill 2"), set_map("A", KEEP), set_map("B", REST), run(4, "slab-tiles"),
        write("V"), stats(7, 3, "slab-tiles")]),
    "slabs_copy_streaming_walk": (_l7, ("slabs", 2, "copy"), [opt("time_block", 2)] + _START + [
        run(5, "tb2"), set_map("B", REST), mean(5, 2, "tb2"), set_map("C", REST), bodies("U", 3), forces(4, "tb2"),
        set_map("A", REST), opt("time_block", 4), probes(9, 4, "march"), set_map("B", KEEP), sampled(9, 4, "march"),
        write("W"), run(9, "march"), set_map("C", REST), bodies("U", 3), observed(9, (F, P, S), 3, 0, 4, "march"),
        set_map("A", REST), opt("engine", 3), window(6, 3, "live", "slab-tiles"), set_map("B", REST), probes(6, 2, "slab-tiles"),
    ]),
    "rank_ring_of_one_p2p": (_l8, ("rank", "p2p"), _START + [
        run(5, "slab-tiles"), set_map("B", REST), refused("forces", 3), bodies("U", 3), forces(6, "slab-tiles"),
        set_map("C", KEEP), mean(6, 3, "slab-tiles"), window(6, 3, "live", "slab-tiles"),
        write("W"), probes(6, 2, "slab-tiles"), bodies("U", 3), driven_observed(8, B5, FP, 2, 0, 0, "slab-tiles"),
    ]),
    "rank_ring_of_one_rccl": (_l8, ("rank", "rccl"), [opt("time_block", 2)] + _START + [
        run(5, "tb2"), set_map("B", REST), refused("forces", 3), bodies("U", 3), forces(5, "tb2"),
        write("W"), mean(6, 3, "tb2"), set_map("A", KEEP), bodies("U", 3), observed(8, (F, P, M), 2, 4, 0, "tb2"), probes(6, 3, "tb2"),
    ]),
    # lbm_run_window_stats, the eleventh kind (ELEVEN), in programs of its own (the older programs and their indices stay): the
    # first call behind a map change under either refill on every path family, and behind a write off the lone tiles; the second
    # call of each pair runs the SAME window behind a LBM_REFILL_REST that turns cells of it from fluid to blocked and others from
    # blocked to fluid (the stamps), so on the tiles the window table's key hits while the blocked bytes the kernels read changed
    "window_stats_tiles_128_behind_maps": (_l1s, None, _START + [
        run(5, "tiles"), set_map("B", KEEP), window_stats(7, 3, "live", "tiles", 1), set_map("C", REST), window_stats(7, 3, "live", "tiles"),
    ]),
    "window_stats_wave6_130x37_behind_maps": (_l4, None, [opt("time_block", 6), opt("wave_rows", WAVE_ROWS)] + _START + [
        run(13, "wave"), set_map("B", KEEP), _kind_call("window_stats", "wave", 6, 0), set_map("C", REST), _kind_call("window_stats", "wave", 6, 0),
    ]),
    "window_stats_split_130x37_behind_maps_and_a_write": (_l4, None, [opt("time_block", 1)] + _START + [
        run(5, "tb1"), set_map("B", KEEP), _kind_call("window_stats", "tb1", 1, 0), set_map("C", REST), _kind_call("window_stats", "tb1", 1, 0),
        write("W"), window_stats(5, 2, "live", "tb1"), opt("time_block", 2), set_map("A", REST), window_stats(5, 2, "live", "tb2"),
    ]),
    "window_stats_slabs_p2p_behind_maps_and_a_write": (_l6, ("slabs", 4, "p2p"), _START + [
        run(5, "slab-tiles"), set_map("B", KEEP), window_stats(7, 3, "live", "slab-tiles", 2), set_map("C", REST),
        window_stats(7, 3, "live", "slab-tiles"), write("W"), window_stats(6, 2, "live", "slab-tiles", 1),
    ]),
}
LIVE = ("set_map", "write", "refused_live")
FAMILY = {"tiles": "tiles", "slab-tiles": "slab-tiles", "wave": "wave", "tb1": "split", "tb2": "split", "march": "split"}


# ---------------------------------------------------------------------------------------------------------------- model
class LiveModel(ObserverModel):
    """ObserverModel with the live inputs: the map in place (self.ob follows it: the bodies a labelling keeps, the force
    slots), the counters of lbm_get_info, and for the coverage check what lies between two running calls."""

    def __init__(self, L, case, ctx):
        super().__init__(L, case, ctx)
        self.maps, self.map, self.updates, self.count = case["maps"], "A", 0, 0
        self.steps, self.ran, self.behind, self.prev, self.wave_rows = 0, {}, [], None, 0

    def apply(self, call):
        op = call[0]
        if op in LIVE:
            e = dict(i=len(self.trace), op=op, call=call, running=False, ty=self.ty, r=self.r, asy=self.async_, pset=self.pset,
                     label=self.label_name, nb=self.nb, body=self.body, accel=self.accel, tb=self.tb, old=self.map, before=self.prev)
            if op == "set_map":
                self.count = int(refilled(self.maps[self.map], self.maps[call[1]]).sum()) if call[2] == REST else 0
                self.map, self.ob = call[1], self.maps[call[1]]
                self.updates += 1
                self.body, self.nb, self.label_name, self.last_forces = None, 0, None, None
                e.update(new=call[1], refill=call[2], count=self.count)
            e["tag"], e["accel_after"] = self.rtag, self.accel
            self.trace.append(e)
        else:
            if op == "opt" and call[1] == "wave_rows":
                self.wave_rows = call[2]
            if op == "opt" and call[1] == "time_block":
                self.wave_rows = 0                                # (time_block forgets the chunk height)
            e = super().apply(call)
        e.update(map=self.map, updates=self.updates, count_after=self.count, steps0=self.steps, behind=tuple(self.behind))
        if e["running"]:
            ran = self.ran.setdefault(e["path"], set())
            e.update(new_map_for_path=self.map not in ran, prev_path=self.prev["path"] if self.prev else None, wave_rows=self.wave_rows)
            ran.add(self.map)
            self.steps += e["n"]
            self.behind, self.prev = [], e
        elif op in LIVE:
            self.behind.append(e)
        return e


def _walk(L, name, programs=None):
    setup, ctx, calls = (programs or PROGRAMS)[name]
    case = setup(L)
    m = LiveModel(L, case, ctx)
    for c in calls:
        m.apply(c)
    return m, case


# ---------------------------------------------------------------------------------------------------------------- no GPU
def _both_ways(case, old, new, cells):
    """cells (rows, columns): one turns from blocked to fluid and another from fluid to blocked between the two maps"""
    a, b = case["maps"][old][cells] != 0, case["maps"][new][cells] != 0
    return bool((a & ~b).any() and (~a & b).any())


def _window_cells(case, name):
    w = case["windows"][name]
    ys, xs = np.meshgrid(w.y0 + np.arange(w.ny) * w.sy, w.x0 + np.arange(w.nx) * w.sx, indexing="ij")
    return ys.reshape(-1), xs.reshape(-1)


def _not_live_or_set(e):
    return not e["running"] and e["op"] not in ("probe_set", "write", "refused_live")


def found(L, programs):
    """The coverage tokens the table holds."""
    out = set()
    for name, (setup, ctx, calls) in programs.items():
        m, case = _walk(L, name, programs)
        t = m.trace
        context = "lone" if ctx is None else " ".join(str(v) for v in (ctx[0], ctx[-1]))
        out.add("context: " + context)
        xy = case["psets"]["L"]
        for e in t:
            if e["running"] and e["behind"]:
                fam, lives = FAMILY[e["path"]], [b for b in e["behind"] if b["op"] != "refused_live"]
                if lives:
                    out.add(f"{fam}: {e['op']} first behind a {lives[-1]['op']}")
                    if e["op"] in ("stats", "window_stats") and lives[-1]["op"] == "set_map":
                        out.add(f"{fam}: {e['op']} first behind a set_map {'REST' if lives[-1]['refill'] == REST else 'KEEP'}")
                    out.add(f"{fam}: a live input behind an {'odd' if e['steps0'] % 2 else 'even'} step count")
                    before = lives[0]["before"]
                    if before and before["path"] in ("wave", "march") and before["pieces"][-1] % before["tb"]:
                        out.add(f"{before['path']}: a live input behind a remainder shorter than time_block")
                    if e["prev_path"] and e["prev_path"] != e["path"] and e["new_map_for_path"] and any(b["op"] == "set_map" for b in lives):
                        out.add(f"{context}: {e['prev_path']} -> {e['path']} across a map call, onto a map it never ran with")
                    if lives[-1]["op"] == "write" and F in e["kinds"] and not any(x["op"] == "bodies" for x in t[lives[-1]["i"]:e["i"]]):
                        out.add("a forces run behind a write without a relabel")
            if e["op"] == "refused_live" and any(x["running"] for x in t[:e["i"]]) and any(x["running"] for x in t[e["i"]:]):
                out.add("refused: " + e["call"][1])
        for a, s, b in _chains(t, [_is("window"), _is("set_map"), _is("window")], _not_live_or_set):
            if a["wkey"] == b["wkey"] and a["path"] == b["path"] and _both_ways(case, s["old"], s["new"], _window_cells(case, a["win"])):
                out.add(f"{FAMILY[a['path']]}: the same window either side of a set_map, cells turning both ways")
        for a, s, b in _chains(t, [_is("window_stats"), _is("set_map", refill=REST), _is("window_stats")], lambda e: False):
            if a["wkey"] == b["wkey"] and a["path"] == b["path"] and a["ty"] == b["ty"] and _both_ways(case, s["old"], s["new"], _window_cells(case, a["win"])):
                out.add(f"{FAMILY[a['path']]}: window_stats over one window either side of a set_map REST, cells turning both ways")
        for a, s, b in _chains(t, [_is("probes"), _is("set_map"), _is("probes")], _not_live_or_set):
            if a["pset"] == b["pset"] and a["path"] == b["path"] and _both_ways(case, s["old"], s["new"], (xy[:, 1], xy[:, 0])):
                out.add(f"{FAMILY[a['path']]}: the same probe set either side of a set_map, cells turning both ways")
        for s, r, b, f in _chains(t, [_is("set_map"), _is("refused", what="forces"), _is("bodies"), lambda e: e["running"] and F in e["kinds"]],
                                  lambda e: False):
            lab, old, new = case["labellings"][b["call"][1]], case["maps"][s["old"]], case["maps"][s["new"]]
            if ((lab > 0) & (old == 0) & (new != 0)).any() and ((lab > 0) & (new == 0)).any():
                out.add(f"forces refused behind set_map {'REST' if s['refill'] == REST else 'KEEP'}, a relabel, a forces run")
        quiet = [e for e in t]
        for a, b in zip(quiet, quiet[1:]):
            if a["op"] == "set_map" and b["op"] == "set_map" and a["refill"] == KEEP and b["refill"] == REST and a["old"] != b["new"]:
                if b["count"] == int(refilled(case["maps"][a["new"]], case["maps"][b["new"]]).sum()) != int(refilled(case["maps"][a["old"]], case["maps"][b["new"]]).sum()):
                    out.add("pair: set_map KEEP then set_map REST, the refill counted from the map between")
            if a["op"] == "write" and b["op"] == "set_map" and b["refill"] == REST and b["count"] > 0:
                out.add("pair: write then set_map REST")
            if a["op"] == "set_map" and a["refill"] == REST and a["count"] > 0 and b["op"] == "write":
                out.add("pair: set_map REST then write")
            if a["op"] == "set_map" and a["new"] == "empty" and a["refill"] == REST and b["op"] == "set_map" and b["new"] != "empty":
                if a["count"] == int((case["maps"][a["old"]] != 0).sum()) > 0:
                    out.add("pair: every obstacle refilled by the empty map, then a map back")
        for a, lab, b, r in _chains(t, [_is("set_map"), _is("bodies"), _is("set_map"), _is("refused", what="forces")], lambda e: False):
            if a["new"] == b["new"] and b["refill"] == REST and b["count"] == 0 and a["count"] > 0 and lab["nb"] > 0:
                out.add("pair: the same map twice, bodies cleared again")
        tilings = [(e["ty"], e["r"]) for e in t if e["running"] and e["path"] == "tiles" and e["behind"]]
        if len(set(tilings)) > 1:
            out.add("live inputs under two tilings of one context")
    return out


DECLARED = (
    [f"{fam}: {kind} first behind a set_map" for fam in ("tiles", "slab-tiles", "wave", "split") for kind in TEN]
    + [f"{fam}: {kind} first behind a write" for fam in ("tiles", "wave") for kind in TEN]
    + [f"{fam}: stats first behind a set_map {r}" for fam in ("tiles", "slab-tiles", "wave", "split") for r in ("KEEP", "REST")]
    + [f"{fam}: stats first behind a write" for fam in ("slab-tiles", "split")]
    + [f"{fam}: window_stats first behind a set_map" for fam in ("tiles", "slab-tiles", "wave", "split")]
    + [f"{fam}: window_stats first behind a set_map {r}" for fam in ("tiles", "slab-tiles", "wave", "split") for r in ("KEEP", "REST")]
    + [f"{fam}: window_stats first behind a write" for fam in ("slab-tiles", "split")]
    + [f"{fam}: window_stats over one window either side of a set_map REST, cells turning both ways" for fam in ("tiles", "slab-tiles", "wave", "split")]
    + [f"lone: {a} -> {b} across a map call, onto a map it never ran with" for a, b in (("tiles", "wave"), ("wave", "march"), ("march", "tiles"), ("tiles", "tb2"))]
    + [f"slabs copy: {a} -> {b} across a map call, onto a map it never ran with" for a, b in (("tb2", "march"), ("march", "slab-tiles"))]
    + [f"{fam}: the same {what} either side of a set_map, cells turning both ways" for fam in ("tiles", "slab-tiles", "wave") for what in ("window", "probe set")]
    + [f"forces refused behind set_map {r}, a relabel, a forces run" for r in ("KEEP", "REST")]
    + ["a forces run behind a write without a relabel", "pair: set_map KEEP then set_map REST, the refill counted from the map between",
       "pair: the same map twice, bodies cleared again", "pair: write then set_map REST", "pair: set_map REST then write",
       "pair: every obstacle refilled by the empty map, then a map back", "live inputs under two tilings of one context"]
    + [f"{fam}: a live input behind an {par} step count" for fam in ("tiles", "slab-tiles", "wave", "split") for par in ("odd", "even")]
    + [f"{p}: a live input behind a remainder shorter than time_block" for p in ("wave", "march")]
    + ["refused: " + w for w in ("null map", "refill 2", "refill -1", "null cells")]
    + ["context: " + c for c in ("lone", "slabs p2p", "slabs copy", "rank p2p", "rank rccl")]
)


def missing(L, programs):
    have = found(L, programs)
    return [tok for tok in DECLARED if tok not in have]


def test_program_table_covers_the_declared_list(L):
    assert not missing(L, PROGRAMS), missing(L, PROGRAMS)
    for name, (setup, ctx, calls) in PROGRAMS.items():
        m, case = _walk(L, name)
        total = sum(e["n"] for e in m.trace if e["running"])
        anchor = min(ANCHOR_STEPS, total)
        inside = [e for e in m.trace if e["op"] in ("set_map", "write") and e["steps0"] < anchor]
        assert len(inside) >= 2 and any(e["op"] == "set_map" and e["refill"] == REST and e["count"] > 0 for e in inside), name
        for e in m.trace:
            where = (name, e["i"], e["call"])
            if e["op"] == "set_map":
                assert e["old"] != e["new"] or e["count"] == 0, where
            if not e["running"]:
                continue
            assert e["path"] in FAMILY and (e["path"] == "slab-tiles") == (ctx is not None and e["path"] in TILE_PATHS), where
            assert 1 <= e["n"] <= 20, where
            assert e["fam"] != "wave" or (e["n"] >= e["tb"] >= 4 and e["wave_rows"] == WAVE_ROWS), where
            assert (P not in e["kinds"] or e["pset"]) and (F not in e["kinds"] or e["nb"] > 0), where
            for k, ev in ((P, e["pe"]), (M, e["me"]), (S, e["fe"])):
                assert (k in e["kinds"] or (k == S and bool(e["win"]))) == (ev > 0) and ev <= e["n"], where
            if F in e["kinds"]:
                assert _kept(case["maps"][e["map"]], e["body"]).any(), where


def test_the_maps_are_what_they_say(L):
    for name, (setup, ctx, calls) in PROGRAMS.items():
        m, case = _walk(L, name)
        maps, p = case["maps"], case["p"]
        nx, ny = p.nx, p.ny
        nslabs = ctx[1] if ctx and ctx[0] == "slabs" else 1
        rows = {0, 1, ny - 3, ny - 2, ny - 1} | {r for s in range(1, nslabs) for r in (s * ny // nslabs - 1, s * ny // nslabs)}
        for e in m.trace:
            if e["running"] and e["path"] in TILE_PATHS:          # a seam of the tiling in place, rows and columns
                assert any(r % e["ty"] == 0 and r - 1 in case["srows"] for r in case["srows"] if r > 1), (name, e["ty"])
                assert {63, 64} <= set(case["scols"])
            if e["running"] and e["path"] == "wave":
                assert {e["wave_rows"] - 1, e["wave_rows"]} <= set(case["srows"]) and e["wave_rows"] < ny
        assert rows <= set(case["srows"]) and {0, nx - 1} <= set(case["scols"]), name
        assert not maps["empty"].any() and set(np.unique(maps["C"])) == {INT_MIN, -1, 0, 1, 2}
        assert set(np.unique(maps["A"])) == set(np.unique(maps["B"])) == {0, 1}
        places = [(np.full(nx, r), np.arange(nx)) for r in case["srows"]] + [(np.arange(ny), np.full(ny, c)) for c in case["scols"]]
        used = {(e["old"], e["new"]) for e in m.trace if e["op"] == "set_map" and "empty" not in (e["old"], e["new"]) and e["old"] != e["new"]}
        assert used, name
        for old, new in used:
            for cells in places:
                assert _both_ways(case, old, new, cells), (name, old, new, int(cells[0][0]), int(cells[1][0]))
        for e in m.trace:                                         # every REST call (not from the empty map, not onto itself) refills there
            if e["op"] == "set_map" and e["refill"] == REST and e["old"] != "empty" and e["old"] != e["new"]:
                mask = refilled(maps[e["old"]], maps[e["new"]])
                assert all(mask[cells].any() for cells in places), (name, e["call"])
        lab = case["labellings"]["U"]
        assert lab.max() == 3 and all(np.all((mp != 0) <= (lab > 0)) for mp in maps.values())
        xy, (wy, wx) = case["psets"]["L"], _window_cells(case, "live")
        assert len({tuple(q) for q in xy.tolist()}) == len(xy)
        for old, new in used:
            assert _both_ways(case, old, new, (xy[:, 1], xy[:, 0])) and _both_ways(case, old, new, (wy, wx)), (name, old, new)
        for wname, arr in case["writes"].items():
            assert arr.shape == (ny, nx, 9) and arr.dtype == np.float32 and np.all(arr > 0)


@pytest.mark.parametrize("drop", [("tiles_128_every_kind_behind_a_map", 21), ("tiles_128_writes_and_pairs", 9), ("tiles_128_writes_and_pairs", 28),
                                  ("lone_256_retile_and_engine_walk", 9), ("never_tiles_tb1_tb2", 22), ("wave6_130x37_writes_and_tables", 28),
                                  ("slabs_p2p_tiles_every_kind_behind_a_map", 32), ("slabs_copy_streaming_walk", 9), ("rank_ring_of_one_rccl", None),
                                  # stats: the map call in front of it (REST, KEEP), the write in front of it, the call itself
                                  ("tiles_128_every_kind_behind_a_map", 27), ("wave6_130x37_every_kind_behind_a_map", 31),
                                  ("tiles_128_writes_and_pairs", 23), ("slabs_p2p_tiles_every_kind_behind_a_map", 28),
                                  ("never_tiles_tb1_tb2", 30), ("never_tiles_tb1_tb2", -1),
                                  # window_stats: the KEEP and the REST map call in front of it (the REST one lies between two
                                  # calls over one window), the write in front of it, the call itself, a program
                                  ("window_stats_tiles_128_behind_maps", 3), ("window_stats_tiles_128_behind_maps", 5),
                                  ("window_stats_wave6_130x37_behind_maps", 5), ("window_stats_wave6_130x37_behind_maps", 7),
                                  ("window_stats_split_130x37_behind_maps_and_a_write", 4), ("window_stats_split_130x37_behind_maps_and_a_write", 8),
                                  ("window_stats_slabs_p2p_behind_maps_and_a_write", 5), ("window_stats_slabs_p2p_behind_maps_and_a_write", 7),
                                  ("window_stats_slabs_p2p_behind_maps_and_a_write", 6), ("window_stats_slabs_p2p_behind_maps_and_a_write", None)])
def test_a_trimmed_table_fails_the_coverage_check(L, drop):
    """Without one live input (the map call in front of a kind, a write, one of a pair, the map call between two engines or
    between two runs of one window), one stats or window_stats call or one program (a context) the table no longer covers the
    declared list."""
    name, index = drop
    programs = dict(PROGRAMS)
    if index is None:
        del programs[name]
    else:
        setup, ctx, calls = programs[name]
        assert calls[index][0] in LIVE or calls[index][0] in ("stats", "window_stats"), calls[index]
        programs[name] = (setup, ctx, calls[:index] + calls[index + 1:] if index != -1 else calls[:-1])
    assert missing(L, programs)


# ---------------------------------------------------------------------------------------------------------------- GPU
class LiveShadow(Shadow):
    """test_observer_sequences.Shadow, destroyed and created again at every live input (module docstring); keeps the live
    inputs with the step they came behind, for the piecewise oracle."""

    def __init__(self, L, p, ob, cells, anchor, kw):
        super().__init__(L, p, ob, cells, anchor, kw)
        self.L, self.p, self.kw, self.inputs = L, p, kw, []

    def live(self, new_map, refill, written):
        if written is None:
            start = s_prime(self.lat.read_state(), self.ob, new_map, refill, self.p.density)
            self.ob, self.body, self.nb = new_map, None, 0
        else:
            start = written
        self.lat.close()
        self.lat = self.L.Lattice(self.p, self.ob, start, **self.kw)
        self.lat.set_option("time_block", 1)
        if self.nb:
            self.lat.set_bodies(self.body, self.nb)
        self.inputs.append((self.done, new_map, refill, written))
        return start


def _refuse_live(L, lat, what, case):
    lib = L.load_library()
    B = case["maps"]["B"]
    rc = {"null map": lambda: lib.lbm_set_obstacles(lat._ctx, None, KEEP), "refill 2": lambda: lib.lbm_set_obstacles(lat._ctx, B.ctypes.data, 2),
          "refill -1": lambda: lib.lbm_set_obstacles(lat._ctx, B.ctypes.data, -1), "null cells": lambda: lib.lbm_write_state(lat._ctx, None)}[what]()
    assert rc == LBM_EINVAL, what


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_live_sequence(gpu, O, oracle, monkeypatch, name):
    L = gpu
    t0 = time.perf_counter()
    setup, ctx, calls = PROGRAMS[name]
    case = setup(L)
    p, cells0, maps = case["p"], case["cells"], case["maps"]
    model = LiveModel(L, case, ctx)
    op = O.OrcParam(p.nx, p.ny, p.maxIters, p.reynolds_dim, p.density, p.accel, p.omega)
    trace = _walk(L, name)[0].trace
    anchor = min(ANCHOR_STEPS, sum(e["n"] for e in trace if e["running"]))
    split_forces = ctx is not None and ctx[0] == "slabs" and any(e["running"] and F in e["kinds"] and e["fam"] != "tiles" for e in trace)
    kw = dict(nslabs=ctx[1], devices=[0] * ctx[1], exchange=L.EXCHANGE_P2P if ctx[2] == "p2p" else L.EXCHANGE_COPY) if split_forces else {}
    sh = LiveShadow(L, p, maps["A"], cells0, anchor, kw)
    chunks = InChunks(O, oracle)
    try:
        if ctx is not None and ctx[0] == "rank":
            monkeypatch.setenv("LBM_FORCE_EXCHANGE", "1")
        with _open(L, p, maps["A"], cells0, ctx) as lat:
            xy, ob, slow = None, maps["A"], []
            for call in calls:
                t_call = time.perf_counter()
                e = model.apply(call)
                kind = e["op"]
                where = (name, e["i"], call)
                start = None
                if kind == "opt":
                    lat.set_option(call[1], call[2])
                elif kind == "bodies":
                    lat.set_bodies(case["labellings"][call[1]], call[2])
                    sh.set_bodies(case["labellings"][call[1]], call[2])
                elif kind == "probe_set":
                    xy = case["psets"][call[1]]
                    lat.set_probes(xy)
                elif kind == "refused":
                    _refuse(L, lat, e, case)
                elif kind == "refused_live":
                    _refuse_live(L, lat, call[1], case)
                elif kind == "set_map":
                    ob = maps[call[1]]
                    lat.set_obstacles(ob, call[2])
                    start = sh.live(ob, call[2], None)
                elif kind == "write":
                    lat.write_state(case["writes"][call[1]])
                    start = sh.live(None, None, case["writes"][call[1]])
                else:
                    n, kinds, tiles = e["n"], e["kinds"], e["fam"] == "tiles"
                    acc = _schedule(e["sched"], p, e["accel"], n)
                    want_fields = any(k in kinds for k in (P, M, S, "window", "stats", "window_stats"))
                    if kind == "run":
                        av_sh, F_sh, X, numpy_forces = sh.run(n), None, None, None
                    else:
                        av_sh, F_sh, X, numpy_forces = sh.steps(acc, want_fields, tiles and F in kinds)
                    av, out = _call(lat, e, case, acc)
                    exp = {}
                    if P in kinds:
                        exp[P] = X[e["pe"] - 1::e["pe"]][:, xy[:, 1], xy[:, 0], :]
                    if M in kinds:
                        exp[M] = mean_from_fields(X, e["me"])
                    if S in kinds:
                        exp[S] = X[e["fe"] - 1::e["fe"]]
                    if "window" in kinds:
                        exp["window"] = cut(X[e["fe"] - 1::e["fe"]], case["windows"][e["win"]])
                    if "stats" in kinds:
                        exp["stats"] = stats_of(X[e["ste"] - 1::e["ste"]], p0_of(p.density))
                    if "window_stats" in kinds:
                        exp["window_stats"] = stats_of(cut(X[e["fe"] - 1::e["fe"]], case["windows"][e["win"]]), p0_of(p.density))
                    assert sorted(out) == sorted(kinds), (where, sorted(out))
                    for k, v in exp.items():
                        _same(out[k], v, where + (k,))
                    if F in kinds:
                        assert out[F].shape == (n, e["nb"], 2), where
                        if tiles:
                            assert _close(out[F], *numpy_forces), (where, np.abs(out[F] - numpy_forces[0]).max())
                        else:
                            _same(out[F], F_sh, where + (F,))
                    assert av.shape == (n,) and np.allclose(av, av_sh, rtol=AV_RTOL, atol=0), (where, np.max(np.abs(av - av_sh) / np.abs(av_sh)))
                    if ctx is None and e["path"] == "tb1":
                        _same(av, av_sh, where + ("av_vels",))
                    _check_engine(lat, e)
                    if e["path"] == "wave":
                        assert lat.info("wave_rows") == e["wave_rows"], (where, lat.info("wave_rows"))
                # ---- after every call: the tag, the acceleration, the counters, the lattice
                assert lat.info("regtile_tag") == e["tag"], (where, lat.info("regtile_tag"), e["tag"])
                assert np.float32(lat.info("accel")) == model.accel, (where, lat.info("accel"), model.accel)
                got = tuple(int(lat.info(k)) for k in ("obstacle_updates", "refilled_cells", "fluid_cells"))
                assert got == (e["updates"], e["count_after"], int((ob == 0).sum())), (where, got, e["updates"], e["count_after"])
                st = lat.read_state()
                _same(st, sh.lat.read_state(), where + ("lattice",))
                if start is not None:
                    _same(st, start, where + ("S'",))
                    if kind == "set_map" and call[2] == REST:
                        assert np.all(st[refilled(maps[e["old"]], ob)] == rest_values(p.density)), where
                    _check_derived(lat, st, chunks, op, (ob != 0).astype(np.int32))
                slow.append((round(time.perf_counter() - t_call, 2), e["i"], kind))
            t_calls = time.perf_counter() - t0
        t_close = time.perf_counter() - t0 - t_calls
        # ---- the shadow against the strict float oracle over the first steps, piecewise
        ref, cur = cells0.copy(), maps["A"]
        ref64 = ref.astype(np.float64)
        av_o, av_64 = [], []
        for t, a in enumerate(sh.accels[:anchor]):
            for step, new_map, refill, written in sh.inputs:
                if step == t:
                    if written is None:
                        if refill == REST:
                            ref64[refilled(cur, new_map)] = rest_values(p.density).astype(np.float64)
                        ref, cur = s_prime(ref, cur, new_map, refill, p.density), new_map
                    else:
                        ref, ref64 = written.copy(), written.astype(np.float64)
            blocked = (cur != 0).astype(np.int32)
            av_o.append(driven_oracle(oracle, op, ref, blocked, np.array([a], dtype=np.float32))[0])
            av_64.append(driven_oracle(oracle, op, ref64, blocked, np.array([a], dtype=np.float32))[0])
        assert sh.at_anchor is not None and len(av_o) == anchor
        av_s, av_o, av_64 = np.concatenate(sh.av)[:anchor].astype(np.float64), np.array(av_o, np.float64), np.array(av_64, np.float64)
        dev, own = np.abs(av_s - av_o) / np.abs(av_o), np.abs(av_o - av_64) / np.abs(av_64)
        t = int(np.argmax(dev))
        print("%s: av_vels of the shadow against the float oracle at worst %.1e (step %d; the float oracle against the double oracle there %.1e, at worst %.1e);"
              " live inputs behind steps %s" % (name, dev[t], t, own[t], own.max(), [i[0] for i in sh.inputs if i[0] < anchor]))
        worst = hold_anchor(sh.at_anchor, ref, np.concatenate(sh.av)[:anchor], np.array(av_o))
    finally:
        sh.lat.close()
    lives = sum(1 for e in model.trace if e["op"] in ("set_map", "write"))
    print("%s: %d calls, %d live inputs; anchor over %d steps at %.2f (lattice) and %.2f (av_vels) of the bars; %.1f s (setup and calls %.1f s, closing the context %.1f s), the slowest calls %s"
          % (name, len(calls), lives, anchor, worst[0], worst[1], time.perf_counter() - t0, t_calls, t_close, sorted(slow)[-2:]))


# ---------------------------------------------------------------------------------------------------------------- ranks
RANK_SHAPE, RANK_STEPS, RANK_WINDOW = (256, 64), (5, 6, 6, 6), (10, 29, 40, 6)      # the window: rows 29 .. 34, across the border


def _rank_case():
    """(A, B, S0, labelling): test_live_inputs.maps_and_states for two ranks of 32 rows; every blocked cell of B labelled 1..3
    by column band, row 0 included."""
    from test_live_inputs import maps_and_states
    nx, ny = RANK_SHAPE
    A, B, S0, _ = maps_and_states(nx, ny, 43, (ny // 2,))
    lab = np.where(B != 0, 1 + (np.arange(nx)[None, :] * 3 // nx), 0).astype(np.int32)
    return A, B, S0, lab


def test_the_rank_case_changes_the_rows_either_side_of_both_borders():
    A, B, S0, lab = _rank_case()
    ny = RANK_SHAPE[1]
    kept = _kept(B, lab)
    for r in (ny // 2 - 1, ny // 2, ny - 1, 0):
        assert refilled(A, B)[r].any() and ((A[r] == 0) & (B[r] != 0) & kept[r]).any(), r
    assert lab.max() == 3 and (lab[0] > 0).any()
    x0, y0, wx, wy = RANK_WINDOW
    assert y0 < ny // 2 - 1 and y0 + wy > ny // 2 + 1 and (B[y0:y0 + wy, x0:x0 + wx] != 0).any() and refilled(A, B)[y0:y0 + wy, x0:x0 + wx].any()


def _rank_worker(rank, nranks, conn, outdir):
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p_ in (os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle"), here):
        if p_ not in sys.path:
            sys.path.insert(0, p_)
    os.environ["LBM_REGTILE_SLABS_NO_AGREEMENT"] = "1"     # (as tests/test_live_inputs.py: no communicator on one GPU)
    import advanced_hpc_lbm_amd as L
    A, B, S0, lab = _rank_case()
    nx, ny = RANK_SHAPE
    p = L.Param(nx, ny, 100, 10, 0.1, 0.01, 1.85)
    lat = L.Lattice(p, A, S0, rank=rank, nranks=nranks, device=0, unique_id=None, exchange=L.EXCHANGE_P2P)
    conn.send(lat.p2p_handle())
    lat.p2p_connect(conn.recv())
    lat.run(RANK_STEPS[0])
    lat.set_obstacles(B, REST)                             # the global map on every rank
    conn.send(("updated", int(lat.info("refilled_cells"))))
    conn.recv()                                            # the test's barrier: every rank has returned from the call
    lat.set_bodies(lab, 3)
    _, forces_ = lat.run_forces(RANK_STEPS[1])
    info = {k: int(lat.info(k)) for k in ("engine_last", "forces_in_kernel")}
    _, mean_ = lat.run_mean(RANK_STEPS[2], 3)
    _, win = lat.run_window(RANK_STEPS[3], 3, L.Window(*RANK_WINDOW))
    np.savez(os.path.join(outdir, f"rank_{rank}.npz"), forces=forces_, mean=mean_, window=win, state=lat.read_state())
    conn.send(("done", info))
    conn.recv()          # keep the mappings until every rank has finished
    lat.close()


@pytest.mark.gpu
def test_rank_contexts_label_bodies_across_the_border_behind_a_new_map(gpu, tmp_path):
    """Two rank processes on one GPU (the pattern of test_live_inputs.test_rank_contexts_take_the_global_map_and_their_own_rows):
    run, set_obstacles(B, LBM_REFILL_REST) on both, the test's barrier, then lbm_set_bodies -- whose link mask looks one row
    across the rank border, into the rows lbm_set_obstacles rebuilt -- and run_forces, run_mean, run_window across the border.
    Without a communicator a rank returns its own contribution: the SUM of the ranks' forces is held by
    test_body_forces._close to forces_from_state on the per-step states of the undivided lattice (the one-step kernel, a
    lattice alone, created from (B, S')); the ranks' rows of the mean, the window and the lattice are its bits."""
    import multiprocessing as mp
    from test_body_forces import forces_from_state
    L = gpu
    nranks = 2
    A, B, S0, lab = _rank_case()
    nx, ny = RANK_SHAPE
    p = L.Param(nx, ny, 100, 10, 0.1, 0.01, 1.85)
    with L.Lattice(p, A, S0) as lat:
        lat.set_option("time_block", 1)
        lat.run(RANK_STEPS[0])
        Sp = s_prime(lat.read_state(), A, B, REST, p.density)
    want_F, scale = [], []
    with L.Lattice(p, B, Sp) as lat:
        lat.set_option("time_block", 1)
        for _ in range(RANK_STEPS[1]):
            lat.run(1)
            f, a = forces_from_state(lat.read_state(), B, lab, 3)
            want_F.append(f)
            scale.append(a)
        _, mean_w = lat.run_mean(RANK_STEPS[2], 3)
        _, win_w = lat.run_window(RANK_STEPS[3], 3, L.Window(*RANK_WINDOW))
        assert lat.info("engine_last") == 1 and lat.info("time_block_active") == 1
        end = lat.read_state()
    ctx = mp.get_context("spawn")
    pipes = [ctx.Pipe() for _ in range(nranks)]
    procs = [ctx.Process(target=_rank_worker, args=(r, nranks, pipes[r][1], str(tmp_path))) for r in range(nranks)]
    for pr in procs:
        pr.start()
    try:
        def gather(what):
            msgs = []
            for r in range(nranks):
                assert pipes[r][0].poll(120), f"rank {r}: no {what}"
                msgs.append(pipes[r][0].recv())
            return msgs

        def release(x):
            for r in range(nranks):
                pipes[r][0].send(x)

        release(gather("handle"))
        upd = gather("update")
        bounds = [(r * ny // nranks, (r + 1) * ny // nranks) for r in range(nranks)]
        assert upd == [("updated", int(refilled(A, B)[a:b].sum())) for a, b in bounds], upd
        release("go")
        done = gather("end")
        assert all(m[0] == "done" for m in done) and done[0][1] == done[1][1], done
        release("bye")
    finally:
        for pr in procs:
            pr.join(60)
            if pr.is_alive():
                pr.kill()
    assert all(pr.exitcode == 0 for pr in procs)
    got = [np.load(tmp_path / f"rank_{r}.npz") for r in range(nranks)]
    F_sum = got[0]["forces"].astype(np.float64) + got[1]["forces"].astype(np.float64)
    want_F, scale = np.array(want_F), np.array(scale)
    assert F_sum.shape == want_F.shape == (RANK_STEPS[1], 3, 2) and np.all(np.abs(want_F).max(axis=(0, 2)) > 0)
    print("two ranks, %s: the summed forces at %.2g of their bar" % (done[0][1], np.max(np.abs(F_sum - want_F) / (1e-5 * scale + 1e-30))))
    assert _close(F_sum, want_F, scale), np.abs(F_sum - want_F).max()
    _same(np.concatenate([g["mean"] for g in got], axis=0), mean_w, "mean")
    _same(np.concatenate([g["state"] for g in got], axis=0), end, "lattice")
    y0, wy = RANK_WINDOW[1], RANK_WINDOW[3]
    mine = np.array([0 if y < ny // 2 else 1 for y in range(y0, y0 + wy)])
    for r in range(nranks):
        assert np.all(got[r]["window"][:, mine != r] == 0), r
    win = np.where((mine == 0)[None, :, None, None], got[0]["window"], got[1]["window"])
    _same(win, win_w, "window")
