"""One context through windows, schedules and every observer call (lbm_run_probes, lbm_run_mean, lbm_run_observed,
lbm_run_window, lbm_set_accel, lbm_run_driven, lbm_run_driven_observed, lbm_run_stats beside lbm_run, lbm_run_sampled, lbm_run_forces,
lbm_set_bodies, lbm_set_probes and lbm_set_option on ONE long-lived context).

tests/test_call_sequences.py drives a context through plain, sampled and forces runs; this file does the same for the calls
that came after it.  What a context carries from call to call has grown with them: the register tiles' per-tiling tables
(forces, probes, the window table with its key, the table of -1s), lbm_wave's maps, the schedule table that only grows, the
sums of a mean, the probe set, the acceleration.  Each program below is one context and a list of calls, every running call
with the path it must take.

The shadow is ONE long-lived context on the same initial lattice under engine 1, time_block 1 (the one-step kernel that
tests/test_gpu_parity.py and tests/test_param_space.py pin to the oracle), a lattice alone -- or, where the program takes
forces across slabs off the register tiles, the same kind of context, because slabs add up their own forces
(tests/test_driven_observed.py: observed_loop).  It mirrors every call step by step: set_accel(a_t), then run_forces(1), or
run(1) when no bodies are set; final_state after each step whose fields an output needs, read_state where forces are
compared in numpy; behind a driven call it puts the context's own acceleration back.  Everything expected is numpy on those
per-step fields by the header's definitions: snapshots fields[every - 1::every], probes the snapshots at [:, jj, ii, :],
windows the snapshots at [:, y0::sy, x0::sx, :] cut to ny x nx, means test_driven_observed.mean_from_fields, the eight floats
of lbm_run_stats test_stats_run.stats_of of the snapshots with p0 = float32(density) x float32(1/3).

After every call: the outputs (snapshots, probes, windows and means bit for bit on every path; forces on the register tiles
held to the numpy forces of the shadow's lattices by test_body_forces._close, elsewhere the shadow's run_forces(1) bits), the
lattice bit for bit (after configuration calls and refused calls too), av_vels (rtol 2e-6; bit for bit on tb1 of a lattice
alone; a constant schedule equal to the context's acceleration against the same call without the schedule, bit for bit on
the tiles), the path taken and the keys of the call, the mailbox tag, info("accel"), and after a change of call kind the
derived quantities (test_call_sequences._check_derived, handed the float oracle 64 cells at a time: InChunks says why).  The
shadow is anchored to the strict float oracle (test_driven_run.driven_oracle with the program's
per-step accelerations) over each program's first <= 50 steps.

The mailbox tag.  lbm_host_run.inc advances the tag once per register-tile LAUNCH: `c->rtag += nsteps + 1` with nsteps the
steps of that launch.  A call the tiles run in several pieces (lbm_run_observed with two or more observers, every
lbm_run_driven_observed: cut at the sample steps of means and snapshots) therefore advances it by n_i + 1 per piece, and the
wrap (a lattice alone: cleared in front of the piece that would reach TAG_WRAP) and the restart (slabs: behind the piece
that passes SLAB_TAG_MARK) are tested per piece.  lbm_run_stats off lbm_wave is cut at every sample step, on the tiles too:
a launch per piece there.  lbm_run_window_stats (the eighth kind, window_stats(n, every, name, path, chunk)) on the tiles runs
pieces of c every steps, c = min("window_stats_chunk", m) or automatic (the samples 64 MiB of staging hold of the slab with the
most window cells), and one piece more for the steps behind the last sample: a launch and n_i + 1 tags per piece, so a call may
pass a mark between two pieces; ONE run on lbm_wave; elsewhere a piece per sample step.  Its output is
stats_of(cut(fields[every - 1::every], w), p0).  It shares the per-slab window table and its (tiling, window) key with
lbm_run_window, and is fed that table where a probes call is fed the probe set's.  ObserverModel.apply restates exactly that.

The table is checked without a GPU against a declared coverage list (path x kind, contexts, transitions, refused calls), so
that trimming it fails on CPU."""
import re
import time

import numpy as np
import pytest

from test_body_forces import _bits, _close, forces_from_state
from test_call_sequences import (ANCHOR_STEPS, SLAB_TAG_MARK, TAG_WRAP, TILE_PATHS, W_EQ, Model, _check_derived, _grow, _kept, _labels,
                                 _open, _p1, _p2, _p3, _p4, _p5, _p6, _p7, _p8, _p9, bodies, clear, forces, opt, run, sampled)
from test_driven_observed import mean_from_fields, pieces_of, window_stats_pieces_of
from test_driven_run import AV_RTOL, driven_oracle, schedules
from test_probe_run import awkward_set
from test_stats_run import p0_of, stats_of
from test_window_run import cut

from make_golden import PARAM_GRID                      # noqa: E402  (test_call_sequences put tests/golden on the path)
from make_golden import refused as guard_refuses        # noqa: E402

KINDS = ("probes", "mean", "observed", "window", "driven", "driven_observed", "stats", "window_stats")
RUNNING = ("run", "sampled", "forces") + KINDS
PATHS = TILE_PATHS + ("tb1", "tb2", "march", "wave")
X_ACCEL = 0.0123                                         # what set_accel sets in the programs


# ---------------------------------------------------------------------------------------------------------------- table
# run, sampled, forces, bodies, clear and opt are test_call_sequences' own.  kinds: a tuple of "forces", "probes", "mean",
# "fields"; pe, me, fe: the periods of probes, means and snapshots (0 where the observer is not wanted).  schedule: "const"
# (every entry the context's acceleration) or (name, seed) of test_driven_run.schedules around lbm_create's acceleration,
# "d<k>" with its spike at index k.
def probes(n, every, path):
    return ("probes", n, every, path)


def mean(n, every, path):
    return ("mean", n, every, path)


def observed(n, kinds, pe, me, fe, path):
    return ("observed", n, kinds, pe, me, fe, path)


def window(n, every, name, path):
    return ("window", n, every, name, path)


def driven(n, schedule, path):
    return ("driven", n, schedule, path)


def driven_observed(n, schedule, kinds, pe, me, fe, path):
    return ("driven_observed", n, schedule, kinds, pe, me, fe, path)


def stats(n, every, path):
    return ("stats", n, every, path)


def window_stats(n, every, name, path, chunk=None):
    """lbm_run_window_stats over the window `name`; chunk: "window_stats_chunk" is set to it in front of the call (and stays)."""
    return ("window_stats", n, every, name, chunk, path)


def set_accel(x):
    return ("set_accel", x)


def probe_set(name):
    return ("probe_set", name)


def clear_probes():
    return ("probe_set", None)


def refused(what, *args):
    """A call that must return LBM_EINVAL: "window" (n, every, name of a window outside the lattice), "schedule" (n, index
    of the non-finite entry, its value), "probes" (n, every), "forces" (n), "mean" (n, every > n), "observed mean"
    (n, mean_every > n), "stats" (n, every > n), "window_stats window" (n, every, name of a window outside the lattice),
    "window_stats every" (n, every > n, name of a window)."""
    return ("refused", what) + args


F, P, M, S = "forces", "probes", "mean", "fields"


def _probe_sets(p, ob, ty, r, extra_rows=()):
    """A: test_probe_run.awkward_set; B: every other cell of A backwards with a blocked one and nine cells A does not hold."""
    a = awkward_set(p.nx, p.ny, ob, ty, r, extra_rows)
    cells = [tuple(c) for c in a.tolist()]
    blocked = [c for c in cells if ob[c[1], c[0]] != 0]
    assert blocked, "no blocked cell among the probes"
    b = cells[::2][::-1]
    if blocked[0] not in b:
        b.append(blocked[0])
    rng = np.random.default_rng(5)
    while len(b) < len(cells[::2]) + 10:
        c = (int(rng.integers(p.nx)), int(rng.integers(p.ny)))
        if c not in cells and c not in b:
            b.append(c)
    return {"A": a, "B": np.array(b, dtype=np.int32)}


def _case(L, builder, tiling, windows, extra_rows=(), more_labels=None):
    p, ob, cells, labellings = builder(L)
    labellings = dict(labellings)
    if more_labels:
        labellings.update(more_labels(ob))
    return dict(p=p, ob=ob, cells=cells, labellings=labellings, psets=_probe_sets(p, ob, tiling[0], tiling[1], extra_rows),
                windows={k: L.Window(*v) for k, v in windows.items()})


def _c1(L):       # 128 x 128 deck, default tiling 2 x 1
    return _case(L, _p1, (2, 1), {"A": (60, 1, 8, 4), "B": (20, 65, 8, 4), "wake": (3, 2, 40, 30, 3, 4)})


def _c2(L):       # 256 x 256 deck, tilings 8 x 4 and 16 x 2: the window straddles a tile seam of both, in x and in y
    return _case(L, _p2, (8, 4), {"seam": (61, 7, 7, 12)})


def _c3(L):       # 256 x 256 deck, tiling 16 x 2: the whole lattice at stride 1
    return _case(L, _p2, (16, 2), {"all": (0, 0, 256, 256)})


def _c4(L):       # 130 x 37, never tiles: a single row (the accelerate row), a single column
    return _case(L, _p7, (0, 1), {"row": (5, 35, 120, 1), "column": (64, 0, 1, 37), "outside": (100, 30, 40, 5)},
                 more_labels=lambda ob: {"random4b": _labels(ob, 74, 4)})


def _c5(L):       # 128 x 16
    return _case(L, _p3, (2, 1), {})


def _c6(L):       # 256 x 256 deck in four slabs of 64 rows, tiling 4 x 1: windows across a slab seam, in one slab, in all
    return _case(L, _p4, (4, 1), {"A": (60, 62, 8, 5), "B": (120, 126, 8, 5), "top": (10, 200, 30, 6, 2, 3),
                                  "every4th": (0, 0, 64, 64, 4, 4)}, extra_rows=(63, 64, 191, 192))


def _c7(L):       # 256 x 32 in two slabs of 16 rows
    return _case(L, _p5, (2, 1), {"seam": (60, 14, 9, 4)}, extra_rows=(15, 16))


def _c8(L):       # 1024 x 128 cut from the 1024 x 1024 deck, a rank ring of one: tiling 8 x 1
    return _case(L, _p6, (8, 1), {"mail": (63, 7, 15, 15, 64, 8), "row": (0, 126, 1024, 1)})


def _c9(L):       # 128 x 64, tiling 4 x 4
    return _case(L, _p8, (4, 4), {"seam": (62, 3, 4, 2)})


def _c10(L):      # 256 x 64 at the refusal point, from rest: the accelerate row, where the guard refuses
    return _case(L, _p9, (2, 1), {"row": (0, 62, 256, 1)})


THIRDS = (0.3, 0.01, 1.85)                               # tests/test_stats_param_space.py: the density at which the two forms of p0 differ


def _p10(L):      # 256 x 64 at "thirds", every population within +-10 % of the equilibrium at rest
    nx, ny = 256, 64
    rng = np.random.default_rng(101)
    ob = (rng.random((ny, nx)) < 0.1).astype(np.int32)
    cells = (np.float32(THIRDS[0]) * W_EQ * (1.0 + 0.2 * (rng.random((ny, nx, 9)) - 0.5))).astype(np.float32)
    return L.Param(nx, ny, 100, 10, *THIRDS), ob, cells, {"blocked": (ob != 0).astype(np.int32)}


def _c11(L):      # 256 x 64 at the "thirds" point
    return _case(L, _p10, (2, 1), {"row": (0, 62, 256, 1)})


def _c12(L):      # 128 x 128 deck as _c1, with a window that leaves the lattice (the programs of lbm_run_window_stats)
    return _case(L, _p1, (2, 1), {"A": (60, 1, 8, 4), "B": (20, 65, 8, 4), "wake": (3, 2, 40, 30, 3, 4), "outside": (120, 100, 20, 5)})


def _c13(L):      # 256 x 64 at the "thirds" point: the accelerate row and the whole lattice
    return _case(L, _p10, (2, 1), {"row": (0, 62, 256, 1), "all": (0, 0, 256, 64)})


B3, B5, B9 = ("b", 3), ("b", 5), ("b", 9)
FP, FM = (F, P), (F, M)
# ctx as in test_call_sequences: None = a lattice alone; ("slabs", n, exchange); ("rank", exchange) = a rank ring of one
PROGRAMS = {
    # every RegFlavour and the table of -1s on one tiled context; the means' buffer; windows A, B, A
    "lone_128_flavour_walk": (_c1, None, [
        bodies("A", 4), probe_set("A"),
        observed(12, FP, 2, 0, 0, "tiles"), driven_observed(11, B3, (F,), 0, 0, 0, "tiles"), forces(6, "tiles"),
        window(10, 3, "wake", "tiles"), probes(9, 2, "tiles"), driven(8, ("d4", 4), "tiles"), run(5, "tiles"),
        sampled(6, 3, "tiles"), mean(8, 4, "tiles"), mean(9, 3, "tiles"),
        driven_observed(12, ("d4", 7), (M,), 0, 4, 0, "tiles"), mean(6, 2, "tiles"),
        window(6, 2, "A", "tiles"), window(6, 3, "B", "tiles"), window(6, 2, "A", "tiles"),
    ]),
    "lone_256_r4_r2_async1": (_c2, None, [
        bodies("walls+rest", 2), probe_set("A"), opt("regtile", 84),
        probes(8, 2, "tiles"), window(6, 2, "seam", "tiles"), probes(6, 3, "tiles"), mean(9, 3, "tiles"),
        observed(10, (F, P, M, S), 1, 5, 4, "tiles"),
        window(8, 4, "seam", "tiles"), opt("regtile", 162), window(8, 4, "seam", "tiles"),
        observed(10, FM, 0, 5, 0, "tiles"), opt("regtile", 84), observed(10, FM, 0, 5, 0, "tiles"),
        probe_set("B"), observed(8, FP, 2, 0, 0, "tiles"),
        driven(9, B3, "tiles"), driven_observed(12, B5, (P, S), 3, 0, 6, "tiles"),
        set_accel(X_ACCEL), driven(7, ("d3", 6), "tiles"), run(6, "tiles"),
    ]),
    "lone_256_r2_async0_engine_walk": (_c3, None, [
        bodies("walls+rest", 2), probe_set("A"), opt("regtile", 162), opt("regtile_async", 0),
        probes(6, 3, "tiles"), mean(6, 2, "tiles"), window(6, 3, "all", "tiles"), driven(6, B3, "tiles"),
        set_accel(X_ACCEL), observed(8, (P, M), 2, 4, 0, "tiles"), driven_observed(8, B5, FP, 2, 0, 0, "tiles"),
        opt("time_block", 8), window(17, 8, "all", "wave"), driven(17, B9, "wave"), mean(16, 8, "wave"),
        opt("time_block", 4), opt("march_kernel", 0), window(9, 4, "all", "march"), driven(9, B3, "march"),
        opt("engine", 3), window(6, 3, "all", "tiles"), driven(6, B5, "tiles"), mean(6, 3, "tiles"),
    ]),
    "never_tiles_tb1_tb2": (_c4, None, [
        opt("time_block", 1), bodies("random4", 4), probe_set("A"),
        probes(7, 3, "tb1"), window(7, 3, "row", "tb1"), probes(6, 2, "tb1"), mean(6, 2, "tb1"), driven(5, B3, "tb1"),
        observed(9, (F, P, M, S), 2, 3, 4, "tb1"), driven_observed(9, B5, (F, P, M), 1, 4, 0, "tb1"),
        opt("time_block", 2),
        probes(7, 3, "tb2"), refused("window", 6, 2, "outside"), mean(6, 2, "tb2"), refused("schedule", 6, 3, float("nan")),
        window(7, 3, "column", "tb2"), refused("mean", 5, 6), driven(5, B9, "tb2"), refused("observed mean", 5, 6),
        observed(9, (F, P, S), 2, 0, 4, "tb2"), driven_observed(9, B3, (P, M), 2, 3, 0, "tb2"),
    ]),
    # lbm_wave<6>: the force-and-probe map follows both the bodies and the probe set
    "wave6_maps_130x37": (_c4, None, [
        opt("time_block", 6), bodies("random4", 4), probe_set("A"),
        driven_observed(14, B3, FP, 2, 0, 0, "wave"), probe_set("B"), driven_observed(14, B5, FP, 2, 0, 0, "wave"),
        bodies("random4b", 4), driven_observed(14, B9, FP, 2, 0, 0, "wave"),
        bodies("random2", 2), driven_observed(14, B3, FP, 2, 0, 0, "wave"),
        forces(13, "wave"), set_accel(X_ACCEL), forces(13, "wave"),
        probes(13, 3, "wave"), window(13, 4, "column", "wave"), probes(12, 6, "wave"),
        mean(12, 6, "wave"), observed(14, (F, P, M), 2, 7, 0, "wave"),
        clear_probes(), refused("probes", 12, 4), probe_set("A"), probes(12, 4, "wave"),
        clear(), refused("forces", 7), run(7, "wave"),
    ]),
    # the schedule table grows past its first capacity; later pieces read it at an offset
    "schedule_table_128x16": (_c5, None, [
        run(3, "tiles"), bodies("random4", 4), probe_set("A"),
        driven(20, B3, "tiles"), driven(1100, B5, "tiles"),
        driven_observed(48, B9, (F, M, S), 0, 12, 16, "tiles"), probes(4, 2, "tiles"),
    ]),
    "slabs_p2p_tiles_tag_restart": (_c6, ("slabs", 4, "p2p"), [
        bodies("walls+rest", 2), probe_set("A"),
        probes(8, 2, "slab-tiles"), mean(8, 4, "slab-tiles"),
        window(8, 4, "A", "slab-tiles"), window(8, 4, "B", "slab-tiles"), window(8, 4, "A", "slab-tiles"),
        window(6, 3, "top", "slab-tiles"), window(6, 3, "every4th", "slab-tiles"),
        driven(9, B3, "slab-tiles"), driven(8, "const", "slab-tiles"), observed(10, (F, P, M), 2, 5, 0, "slab-tiles"),
        opt("regtile_tag", SLAB_TAG_MARK - 7), driven_observed(12, B5, (F, P, M, S), 1, 4, 6, "slab-tiles"),
        run(5, "slab-tiles"), stats(6, 3, "slab-tiles"),
    ]),
    "slabs_copy_streaming": (_c7, ("slabs", 2, "copy"), [
        opt("time_block", 2), bodies("random3", 3), probe_set("A"),
        probes(7, 3, "tb2"), window(7, 3, "seam", "tb2"), driven(6, B3, "tb2"), driven_observed(8, B5, (F, P, M), 2, 4, 0, "tb2"),
        opt("time_block", 4),
        probes(9, 4, "march"), mean(8, 4, "march"), window(9, 4, "seam", "march"), driven(9, B9, "march"),
        observed(9, (F, P, S), 3, 0, 4, "march"), driven_observed(9, B3, (F, P, M), 3, 4, 0, "march"),
        opt("engine", 3), window(6, 3, "seam", "slab-tiles"), probes(6, 2, "slab-tiles"),
    ]),
    "rank_ring_of_one_p2p": (_c8, ("rank", "p2p"), [
        bodies("walls+rest", 2), probe_set("A"),
        probes(6, 2, "slab-tiles"), window(6, 3, "mail", "slab-tiles"), driven(7, B3, "slab-tiles"),
        observed(8, (F, P, M), 2, 4, 0, "slab-tiles"), driven_observed(8, B5, (P, S), 2, 0, 4, "slab-tiles"),
        mean(6, 3, "slab-tiles"), run(3, "slab-tiles"), stats(6, 2, "slab-tiles"), window_stats(7, 3, "mail", "slab-tiles", 1),
    ]),
    "rank_ring_of_one_rccl": (_c8, ("rank", "rccl"), [
        opt("time_block", 2), bodies("walls+rest", 2), probe_set("A"),
        probes(6, 3, "tb2"), window(6, 3, "row", "tb2"), driven(6, B3, "tb2"), observed(8, (F, P, M), 2, 4, 0, "tb2"),
        driven_observed(8, B5, FP, 2, 0, 0, "tb2"), mean(6, 3, "tb2"), run(3, "tb2"), stats(6, 3, "tb2"), window_stats(7, 3, "row", "tb2"),
    ]),
    "lone_tag_wrap_in_flavours": (_c9, None, [
        opt("regtile", 44), bodies("random4", 4), probe_set("A"), run(5, "tiles"),
        opt("regtile_tag", TAG_WRAP - 10), window(12, 4, "seam", "tiles"),
        opt("regtile_tag", TAG_WRAP - 5), driven(9, B3, "tiles"),
        opt("regtile_tag", TAG_WRAP - 8), observed(12, (F, P, M), 1, 4, 0, "tiles"),
        driven(8, "const", "tiles"), driven_observed(8, "const", FP, 2, 0, 0, "tiles"), probes(6, 2, "tiles"), run(4, "tiles"),
        stats(6, 2, "tiles"),
    ]),
    "refusal_point_mixed": (_c10, None, [
        bodies("blocked", 1), probe_set("A"),
        driven(6, B3, "tiles"), window(6, 2, "row", "tiles"), observed(6, (F, P, M), 1, 3, 0, "tiles"),
        opt("time_block", 4), opt("march_kernel", 0),
        driven(9, B5, "march"), window(9, 4, "row", "march"), observed(8, FP, 2, 0, 0, "march"),
        opt("time_block", 8), opt("march_kernel", 1), opt("wave_cols", 2),
        driven(10, B9, "wave"), window(10, 5, "row", "wave"), observed(16, (F, P, M), 2, 8, 0, "wave"),
        opt("engine", 3), run(4, "tiles"),
    ]),
    # lbm_run_stats beside every other observer call: directly behind and in front of each, on the tiles ...
    "stats_neighbours_on_tiles_128": (_c1, None, [
        bodies("A", 4), probe_set("A"),
        mean(6, 2, "tiles"), stats(7, 3, "tiles"), mean(6, 3, "tiles"),
        observed(8, (F, P, M), 2, 4, 0, "tiles"), stats(6, 2, "tiles"), observed(8, (P, M), 2, 4, 0, "tiles"),
        window(6, 3, "A", "tiles"), stats(8, 3, "tiles"), window(6, 2, "B", "tiles"),
        driven(6, B3, "tiles"), stats(5, 1, "tiles"), driven(6, B5, "tiles"),
        driven_observed(8, B5, (P, M), 2, 4, 0, "tiles"), stats(9, 4, "tiles"), driven_observed(8, B9, FP, 2, 0, 0, "tiles"),
        set_accel(X_ACCEL), stats(6, 2, "tiles"), refused("stats", 5, 6), run(4, "tiles"),
    ]),
    # ... and inside lbm_wave<6> (every stats call one run of a pass or more: the sums ride in the launches)
    "stats_neighbours_on_wave6_130x37": (_c4, None, [
        opt("time_block", 6), bodies("random4", 4), probe_set("A"),
        mean(12, 6, "wave"), stats(13, 3, "wave"), mean(12, 4, "wave"),
        observed(14, (F, P, M), 2, 7, 0, "wave"), stats(12, 1, "wave"), observed(14, (F, P, M), 2, 7, 0, "wave"),
        window(13, 4, "column", "wave"), stats(14, 6, "wave"), window(12, 6, "row", "wave"),
        driven(13, B3, "wave"), stats(13, 5, "wave"), driven(12, B5, "wave"),
        driven_observed(14, B5, FP, 2, 0, 0, "wave"), stats(17, 7, "wave"), driven_observed(14, B9, FP, 2, 0, 0, "wave"),
        set_accel(X_ACCEL), stats(12, 2, "wave"), refused("stats", 5, 6), run(7, "wave"),
    ]),
    # the pieces of a stats call are plain register-tile launches: behind a re-tiling, under both loops, across the tag wrap
    # (three pieces of 4 + 1 from TAG_WRAP - 9: the second would reach the mark, so the wrap falls between two pieces)
    "stats_tilings_and_tag_wrap_128x16": (_c5, None, [
        run(3, "tiles"), bodies("random4", 4), probe_set("A"), stats(5, 2, "tiles"),
        opt("regtile", 82), stats(7, 2, "tiles"), opt("regtile_async", 0), stats(6, 3, "tiles"),
        opt("regtile_tag", TAG_WRAP - 9), stats(12, 4, "tiles"), mean(6, 3, "tiles"), run(4, "tiles"),
    ]),
    # slabs with copies: off the tiles (lbm_stats_add per slab), then on them, the pieces passing the restart mark
    "stats_slabs_copy_256x32": (_c7, ("slabs", 2, "copy"), [
        opt("time_block", 2), bodies("random3", 3), probe_set("A"),
        stats(7, 3, "tb2"), mean(6, 3, "tb2"), opt("time_block", 4), stats(9, 4, "march"),
        opt("engine", 3), stats(6, 2, "slab-tiles"),
        opt("regtile_tag", SLAB_TAG_MARK - 7), stats(12, 4, "slab-tiles"), run(5, "slab-tiles"),
    ]),
    "stats_never_tiles_tb1": (_c4, None, [
        opt("time_block", 1), bodies("random4", 4), probe_set("A"),
        stats(7, 3, "tb1"), mean(6, 2, "tb1"), run(5, "tb1"), opt("time_block", 2), stats(7, 1, "tb2"), run(3, "tb2"),
    ]),
    # density 0.3, where density * (1.f / 3.f) and density / 3.f are different floats: every engine kind of a lattice alone
    "stats_at_thirds_256x64": (_c11, None, [
        bodies("blocked", 1), probe_set("A"),
        stats(7, 3, "tiles"), mean(6, 3, "tiles"), window(6, 2, "row", "tiles"),
        opt("time_block", 8), opt("march_kernel", 1), opt("wave_cols", 2),
        stats(17, 4, "wave"), mean(16, 8, "wave"), stats(16, 1, "wave"),
        opt("time_block", 4), opt("march_kernel", 0), stats(9, 4, "march"),
        opt("engine", 3), stats(6, 2, "tiles"),
    ]),
    # lbm_run_window_stats.  The window table and its key are lbm_run_window's: window(A) then stats over A (a hit), stats over
    # A then over B then window(B) (a miss, then a hit from the other call); the probe table and the table of -1s either side
    # of a call that is fed window tables as probe tables; the chunk option between two calls; a changed acceleration; its
    # whole-lattice cousin on either side; refused between running calls
    "window_stats_walk_on_tiles_128": (_c12, None, [
        bodies("A", 4), probe_set("A"),
        window(6, 2, "A", "tiles"), window_stats(6, 2, "A", "tiles"), window_stats(7, 3, "B", "tiles"), window(6, 3, "B", "tiles"),
        probes(8, 2, "tiles"), window_stats(9, 2, "wake", "tiles", 2), probes(8, 2, "tiles"),
        window_stats(9, 2, "wake", "tiles", 1),
        set_accel(X_ACCEL), window_stats(6, 3, "A", "tiles", 0), run(3, "tiles"),
        stats(6, 2, "tiles"), window_stats(7, 2, "wake", "tiles"), stats(6, 3, "tiles"),
        refused("window_stats window", 6, 2, "outside"), run(4, "tiles"),
    ]),
    # the same window either side of a re-tiling (the key's ty), under both loops, and its pieces across the tag wrap: three
    # pieces of 4 + 1 from TAG_WRAP - 9, the second would reach the mark
    "window_stats_retile_and_tag_wrap_256": (_c2, None, [
        bodies("walls+rest", 2), probe_set("A"), opt("regtile", 84),
        window_stats(8, 4, "seam", "tiles"), opt("regtile", 162), window_stats(8, 4, "seam", "tiles"),
        opt("regtile_async", 0), window_stats(7, 2, "seam", "tiles", 2),
        opt("regtile_tag", TAG_WRAP - 9), window_stats(12, 4, "seam", "tiles", 1), run(4, "tiles"),
    ]),
    "window_stats_on_wave6_130x37": (_c4, None, [
        opt("time_block", 6), bodies("random4", 4), probe_set("A"),
        window(13, 4, "column", "wave"), window_stats(13, 4, "column", "wave"),
        stats(13, 3, "wave"), window_stats(14, 6, "row", "wave"), stats(12, 1, "wave"), run(7, "wave"),
        set_accel(X_ACCEL), window_stats(12, 1, "column", "wave"),
        refused("window_stats every", 5, 6, "row"), window_stats(17, 7, "row", "wave"), run(7, "wave"),
    ]),
    "window_stats_never_tiles_tb1_tb2": (_c4, None, [
        opt("time_block", 1), bodies("random4", 4), probe_set("A"),
        window_stats(7, 3, "row", "tb1"), window(6, 2, "row", "tb1"), run(5, "tb1"),
        opt("time_block", 2), window_stats(7, 1, "column", "tb2"), run(3, "tb2"),
    ]),
    "window_stats_slabs_copy_256x32": (_c7, ("slabs", 2, "copy"), [
        opt("time_block", 2), bodies("random3", 3), probe_set("A"),
        window_stats(7, 3, "seam", "tb2"), window(6, 3, "seam", "tb2"), opt("time_block", 4), window_stats(9, 4, "seam", "march"),
        opt("engine", 3), window_stats(6, 2, "seam", "slab-tiles"), run(5, "slab-tiles"),
    ]),
    # four p2p slabs: the shared table per slab (a window without a row in three of them), a piece per sample past the restart mark
    # (three pieces of 4 + 1 from SLAB_TAG_MARK - 7: cleared behind the second)
    "window_stats_slabs_p2p_tag_restart": (_c6, ("slabs", 4, "p2p"), [
        bodies("walls+rest", 2), probe_set("A"),
        window(8, 4, "A", "slab-tiles"), window_stats(8, 4, "A", "slab-tiles"), window_stats(8, 4, "B", "slab-tiles"), window(8, 4, "B", "slab-tiles"),
        window_stats(6, 3, "top", "slab-tiles"), window_stats(7, 3, "every4th", "slab-tiles", 1),
        opt("regtile_tag", SLAB_TAG_MARK - 7), window_stats(12, 4, "A", "slab-tiles"), run(5, "slab-tiles"),
    ]),
    # density 0.3: the three places of its own where the density reaches p0 (lbm_window_stats_fold, lbm_wave's WINDOW+STATS
    # flavour, lbm_window_stats_add)
    "window_stats_at_thirds_256x64": (_c13, None, [
        bodies("blocked", 1), probe_set("A"),
        window_stats(7, 3, "row", "tiles"), window(6, 2, "row", "tiles"), window_stats(6, 2, "all", "tiles", 2),
        opt("time_block", 8), opt("march_kernel", 1), opt("wave_cols", 2),
        window_stats(17, 4, "row", "wave"), window_stats(16, 1, "all", "wave"),
        opt("time_block", 4), opt("march_kernel", 0), window_stats(9, 4, "row", "march"),
        opt("engine", 3), window_stats(6, 2, "row", "tiles"),
    ]),
}
REFUSING = {"refusal_point_mixed"}
# (as test_call_sequences: float and double part once a refusal flips on rounding; the first two calls, inside which the
# guard already refuses)
ANCHOR_OVERRIDE = {"refusal_point_mixed": 12}
LONG_CALLS = {"schedule_table_128x16"}                   # the one program whose calls may pass 60 steps


# ---------------------------------------------------------------------------------------------------------------- model
def _bounds(n, *everys):
    """The ends of the step-loop pieces of a call of n steps cut at the multiples of `everys` (0: not wanted)."""
    return sorted({n} | {k for e in everys if e for k in range(e, n + 1, e)})


class ObserverModel(Model):
    """test_call_sequences.Model with the newer calls: what the host keeps across them (the probe set, the acceleration,
    the schedule table's capacity, the streaming options), the pieces of a call and the tag they leave, and a trace of
    every call for the coverage check."""

    def __init__(self, L, case, ctx):
        super().__init__(L, case["p"], case["ob"], case["labellings"], ctx)
        self.windows, self.psets = case["windows"], case["psets"]
        self.accel = np.float32(case["p"].accel)
        self.pset, self.tb, self.wave_cols, self.dtab_cap = None, 0, 1, 0
        self.ws_chunk = 0                                        # the option "window_stats_chunk"
        self.context = "lone" if ctx is None else " ".join(str(v) for v in (ctx[0], ctx[-1]))
        self.trace, self.waves = [], set()

    def window_rows(self, w):
        """Per slab: the window rows that lie in its lattice rows."""
        ny = self.p.ny
        rows = [w.y0 + r * w.sy for r in range(w.ny)]
        return [sum(s * ny // self.nslabs <= y < (s + 1) * ny // self.nslabs for y in rows) for s in range(self.nslabs)]

    def _launch(self, n, e, piece):
        """One register-tile launch of n steps: the tag rule of run_regtile."""
        if self.lone and self.rtag + n >= TAG_WRAP:              # cleared in front of the launch
            self.rtag = 1
            e["restarts"].append(piece)
        restart = not self.lone and self.rtag + n >= SLAB_TAG_MARK
        self.rtag += n + 1
        if restart:                                              # cleared behind the launch
            self.rtag = 1
            e["restarts"].append(piece)

    def apply(self, call):
        """Advances the model over `call`; returns its entry of the trace ("tag": the expected mailbox tag after it)."""
        op = call[0]
        e = dict(i=len(self.trace), op=op, call=call, running=op in RUNNING, ty=self.ty, r=self.r, asy=self.async_,
                 pset=self.pset, label=self.label_name, nb=self.nb, body=self.body, accel=self.accel, tb=self.tb, context=self.context)
        if op == "opt":
            e.update(key=call[1], value=call[2])
            if call[1] == "time_block":
                self.tb = call[2]
            elif call[1] == "wave_cols":
                self.wave_cols = call[2]
            elif call[1] == "window_stats_chunk":
                self.ws_chunk = call[2]
            super().apply(call)
        elif op == "bodies":
            super().apply(call)
            e.update(label=self.label_name, nb=self.nb)
        elif op == "probe_set":
            self.pset = e["pset"] = call[1]
        elif op == "set_accel":
            self.accel = np.float32(call[1])
        elif op == "refused":
            e.update(what=call[1], args=call[2:])
        else:
            self._run(call, e)
        e["tag"], e["accel_after"] = self.rtag, self.accel
        self.trace.append(e)
        return e

    def _run(self, call, e):
        op, n, path = call[0], call[1], call[-1]
        fam = "tiles" if path in TILE_PATHS else "wave" if path == "wave" else "split"
        kinds, pe, me, fe, sched, win, ste = (), 0, 0, 0, None, None, 0
        if op == "sampled":
            kinds, fe = (S,), call[2]
        elif op == "forces":
            kinds = (F,)
        elif op == "probes":
            kinds, pe = (P,), call[2]
        elif op == "mean":
            kinds, me = (M,), call[2]
        elif op == "window":
            kinds, fe, win = ("window",), call[2], call[3]
        elif op == "driven":
            sched = call[2]
        elif op == "stats":
            kinds, ste = ("stats",), call[2]
        elif op == "window_stats":
            kinds, fe, win = ("window_stats",), call[2], call[3]
            if call[4] is not None:
                self.ws_chunk = call[4]
        elif op == "observed":
            kinds, pe, me, fe = call[2:6]
        elif op == "driven_observed":
            sched, kinds, pe, me, fe = call[2:7]
        pe, me = (pe if P in kinds else 0), (me if M in kinds else 0)
        fe = fe if S in kinds or win else 0
        multi = op == "driven_observed" or (op == "observed" and len(kinds) >= 2)
        # the pieces: means and snapshots cut them; probes too where neither the register tiles nor lbm_wave take them
        # (lbm_run_stats: ONE run where lbm_wave takes the sums; everywhere else, the register tiles too, a plain run per sample)
        if multi:
            cutters = (me, fe) + ((pe,) if fam == "split" else ())
        elif op == "stats":
            cutters = () if fam == "wave" else (ste,)
        elif fam == "split" and op not in ("run", "forces", "driven"):
            cutters = (pe, me, fe)                               # the split path of the single calls
        else:
            cutters = ()
        ends = _bounds(n, *cutters)
        if op == "window_stats":
            # lbm_host_observe.inc: ONE run where lbm_wave takes the sums; on the tiles a launch per piece of c sample steps --
            # c = min(chunk, m), or automatic: the samples that 64 MiB of staging hold of the slab with the most window cells,
            # at least 1, at most m -- and one more for the steps behind the last sample; elsewhere a piece per sample (cutters)
            w = self.windows[win]
            m, cells = n // fe, w.nx * max(self.window_rows(w))
            if fam == "tiles":
                c = min(self.ws_chunk, m) if self.ws_chunk > 0 else min(m, max(1, (64 << 20) // (16 * cells)))
                ends = sorted({min(k + c, m) * fe for k in range(0, m, c)} | {n})
            e.update(chunk=self.ws_chunk, wcells=cells, m=m)
        e.update(n=n, path=path, fam=fam, kinds=tuple(kinds), pe=pe, me=me, fe=fe, ste=ste, sched=sched, win=win, multi=multi,
                 cutters=cutters, ends=ends, pieces=[b - a for a, b in zip([0] + ends, ends)], restarts=[],
                 sched_name=None if sched is None else sched if sched == "const" else sched[0],
                 labels=self.label(path), lone=self.lone, dtab_grew=False)
        if win:
            w = self.windows[win]
            e.update(wkey=(w.x0, w.y0, w.nx, w.ny, w.sx, w.sy), wslabs=self.window_rows(w))
        if fam == "wave":
            self.waves.add((self.tb, self.wave_cols))
        if op in ("run", "sampled", "forces"):
            super().apply(call)
            return
        for lab in e["labels"]:
            self.pairs.add((lab, op))
        if fam == "tiles":
            if sched is not None and n > self.dtab_cap:          # drive_table_room: Slab::dtab, geometric from 1024 pairs
                e["dtab_grew"] = self.dtab_cap > 0
                self.dtab_cap = _grow(self.dtab_cap, n)
            for j, m in enumerate(e["pieces"]):
                self._launch(m, e, j)
        self.history.append((op, "tiles" if fam == "tiles" else "streaming", self.ty))


def expected_keys(e):
    """The info keys of a running call and what they must read: where the observers were taken, and in how many pieces."""
    op, kinds = e["op"], e["kinds"]
    T, W = e["fam"] == "tiles", e["fam"] == "wave"
    # (inside lbm_wave launches: the pieces that hold a full pass of time_block steps)
    W = W and any(m >= e["tb"] for m in e["pieces"])
    bits = (1 if F in kinds else 0) | (2 if P in kinds else 0)
    single = {"sampled": "samples", "forces": "forces", "probes": "probes", "mean": "mean", "window": "window", "driven": "driven"}
    if op in single:
        return {single[op] + "_in_kernel": int(T), single[op] + "_in_wave": int(W)}
    if op == "stats":                                            # (the ONE piece on lbm_wave: n >= time_block; no *_in_kernel key)
        return {"stats_in_wave": int(W)}
    if op == "window_stats":
        return {"window_stats_in_kernel": int(T), "window_stats_in_wave": int(W), "window_stats_pieces": len(e["pieces"])}
    if op == "observed":
        return {"observed_in_kernel": bits if T else 0, "observed_in_wave": bits if W else 0, "observed_pieces": len(e["pieces"])}
    if op == "driven_observed":
        return {"driven_observed_in_kernel": bits if T else 0, "driven_observed_in_wave": bits if W else 0,
                "driven_observed_pieces": len(e["pieces"]) if T or W else 0}
    return {}


def _walk(L, name):
    setup, ctx, calls = PROGRAMS[name]
    case = setup(L)
    m = ObserverModel(L, case, ctx)
    for c in calls:
        m.apply(c)
    return m, case


# ---------------------------------------------------------------------------------------------------------------- no GPU
def _is(op=None, path=None, fam=None, has=(), **eq):
    def f(e):
        return ((op is None or e["op"] == op) and (path is None or e.get("path") == path) and (fam is None or e.get("fam") == fam)
                and all(k in e.get("kinds", ()) for k in has) and all(e.get(k) == v for k, v in eq.items()))
    return f


def _quiet(e):
    return not e["running"]


def _chains(trace, preds, between=None):
    """Every tuple of entries, in trace order, that satisfy `preds` one each; between: what every entry strictly between
    two of them must satisfy (None: anything)."""
    out = []

    def go(start, got):
        if len(got) == len(preds):
            out.append(tuple(got))
            return
        for j in range(start, len(trace)):
            if preds[len(got)](trace[j]):
                go(j + 1, got + [trace[j]])
            if got and between is not None and not between(trace[j]):
                return
    go(0, [])
    return out


def _abawindows(path):
    def f(t):
        return any(a["wkey"] == c["wkey"] != b["wkey"] and a["wkey"][2:] == b["wkey"][2:]
                   for a, b, c in _chains(t, [_is("window", path)] * 3, _quiet))
    return f


def _relabel(same_nb):
    def f(t):
        return any(a["label"] != b["label"] and (a["nb"] == b["nb"]) == same_nb
                   for a, _, b in _chains(t, [_is("driven_observed", "wave", has=FP), _is("bodies"), _is("driven_observed", "wave", has=FP)], _quiet))
    return f


def _engine_walk(op):
    return lambda t: bool(_chains(t, [_is(op, fam="tiles"), _is(op, "wave"), _is(op, "march"), _is(op, fam="tiles")]))


def _spike_on_a_boundary(t):
    for e in t:
        m = re.fullmatch(r"d(\d+)", e.get("sched_name") or "")
        if e["op"] == "driven_observed" and m and int(m.group(1)) in e["ends"][:-1]:
            return True
    return False


def _restart(op, lone, mid=False):
    return lambda t: any(e["op"] == op and e["fam"] == "tiles" and e["lone"] == lone and any(j >= (1 if mid else 0) for j in e["restarts"])
                         for e in t if e["running"])


# the transitions of the issue: name -> does the trace of ONE program hold it
TRANSITIONS = {
    "windows A, B, A on tiles": _abawindows("tiles"),
    "windows A, B, A on slab-tiles": _abawindows("slab-tiles"),
    "a window, a retile, the same window": lambda t: any(
        a["wkey"] == b["wkey"] and a["ty"] != b["ty"]
        for a, _, b in _chains(t, [_is("window", "tiles"), _is("opt", key="regtile"), _is("window", "tiles")], _quiet)),
    "a window without a cell in some slab, then one with": lambda t: any(
        any(x == 0 and y > 0 for x, y in zip(a["wslabs"], b["wslabs"]))
        for a, b in _chains(t, [_is("window", "slab-tiles")] * 2, _quiet)),
    "probes, window, probes on tiles": lambda t: bool(_chains(t, [_is("probes", "tiles"), _is("window", "tiles"), _is("probes", "tiles")], _quiet)),
    "probes, window, probes on wave": lambda t: bool(_chains(t, [_is("probes", "wave"), _is("window", "wave"), _is("probes", "wave")], _quiet)),
    "probes, window, probes on a split path": lambda t: bool(
        _chains(t, [_is("probes", fam="split"), _is("window", fam="split"), _is("probes", fam="split")], _quiet)),
    "probe set replaced between two observed calls": lambda t: any(
        a["pset"] != b["pset"] for a, _, b in _chains(t, [_is("observed", has=(P,)), _is("probe_set"), _is("observed", has=(P,))])),
    "probe set replaced between two driven_observed calls on wave with forces": lambda t: any(
        a["pset"] != b["pset"]
        for a, _, b in _chains(t, [_is("driven_observed", "wave", has=FP), _is("probe_set"), _is("driven_observed", "wave", has=FP)], _quiet)),
    "relabel, same nb, between two such wave calls": _relabel(True),
    "relabel, different nb, between two such wave calls": _relabel(False),
    "clear_probes, a refused probes call, a new set": lambda t: bool(
        _chains(t, [_is("probe_set", pset=None), _is("refused", what="probes"), lambda e: e["op"] == "probe_set" and e["pset"], _is(has=(P,))], _quiet)),
    "every register-tile flavour on one context": lambda t: any(
        a["kinds"] == FP and b["kinds"] == (F,)
        for a, b, *_ in _chains(t, [_is("observed", "tiles"), _is("driven_observed", "tiles"), _is("forces", "tiles"), _is("window", "tiles"),
                                    _is("probes", "tiles"), _is("driven", "tiles"), _is("run", "tiles")], _quiet)),
    "a retile between two observed calls with forces and means only": lambda t: any(
        a["ty"] != b["ty"] for a, _, b in _chains(t, [_is("observed", "tiles", kinds=FM), _is("opt", key="regtile"), _is("observed", "tiles", kinds=FM)], _quiet)),
    "the schedule table grows, later pieces read it at an offset": lambda t: any(
        not a["dtab_grew"] and b["dtab_grew"] and len(c["pieces"]) > 2
        for a, b, c in _chains(t, [_is("driven", fam="tiles"), _is("driven", fam="tiles"), _is("driven_observed", fam="tiles", has=(M, S))], _quiet)),
    "a driven call cut in two": lambda t: any(a["path"] == b["path"] for a, b in _chains(t, [_is("driven"), _is("driven")], _quiet)),
    "schedule b under observers": lambda t: any(e["op"] == "driven_observed" and e["sched_name"] == "b" for e in t),
    "a spike on a piece boundary": _spike_on_a_boundary,
    "a constant schedule on the tiles": lambda t: (any(e["op"] == "driven" and e["sched"] == "const" and e["fam"] == "tiles" for e in t)),
    "a constant schedule under observers on the tiles": lambda t: any(
        e["op"] == "driven_observed" and e["sched"] == "const" and e["fam"] == "tiles" and e["kinds"] == FP for e in t),
    "set_accel, driven, run": lambda t: any(
        r["accel"] == s["accel_after"] != s["accel"] for s, _, r in _chains(t, [_is("set_accel"), _is("driven"), _is("run")], _quiet)),
    "set_accel, observed, another engine, mean": lambda t: any(
        o["fam"] != m["fam"] and m["accel"] == s["accel_after"] != s["accel"]
        for s, o, _, m in _chains(t, [_is("set_accel"), _is("observed"), lambda e: e["op"] == "opt" and e["key"] in ("engine", "time_block"), _is("mean")],
                                  lambda e: e["op"] != "set_accel")),
    "set_accel between two forces calls on wave": lambda t: bool(_chains(t, [_is("forces", "wave"), _is("set_accel"), _is("forces", "wave")], _quiet)),
    "mean, then a mean with another period": lambda t: any(a["me"] != b["me"] and a["path"] == b["path"] for a, b in _chains(t, [_is("mean")] * 2, _quiet)),
    "a mean on wave, then a mean on tiles": lambda t: bool(_chains(t, [_is("mean", "wave"), _is("mean", fam="tiles")])),
    "driven_observed with a mean, then a plain mean": lambda t: bool(_chains(t, [_is("driven_observed", has=(M,)), _is("mean")], _quiet)),
    "tiles, wave, march, tiles with a window before and after": _engine_walk("window"),
    "tiles, wave, march, tiles with a driven call before and after": _engine_walk("driven"),
    "lone tag restart inside a window call": _restart("window", True),
    "lone tag restart inside a driven call": _restart("driven", True),
    "lone tag restart between two pieces of an observed call": _restart("observed", True, mid=True),
    "slab tag restart inside a driven_observed call": _restart("driven_observed", False),
    "lone tag restart between two pieces of a stats call": _restart("stats", True, mid=True),
    "slab tag restart behind a piece of a stats call": _restart("stats", False),
    "set_accel, stats on tiles": lambda t: any(
        r["accel"] == s["accel_after"] != s["accel"] for s, r in _chains(t, [_is("set_accel"), _is("stats", fam="tiles")], _quiet)),
    "set_accel, stats on wave": lambda t: any(
        r["accel"] == s["accel_after"] != s["accel"] for s, r in _chains(t, [_is("set_accel"), _is("stats", "wave")], _quiet)),
    "a stats call, a retile, a stats call": lambda t: any(
        a["ty"] != b["ty"] for a, _, b in _chains(t, [_is("stats", "tiles"), _is("opt", key="regtile"), _is("stats", "tiles")], _quiet)),
}
# lbm_run_stats directly behind and directly in front of each of these, on the tiles and inside lbm_wave
STATS_NEIGHBOURS = {"mean": {}, "observed": dict(has=(M,)), "window": {}, "driven": {}, "driven_observed": {}}
for _fam in ("tiles", "wave"):
    for _k, _kw in STATS_NEIGHBOURS.items():
        TRANSITIONS[f"{_k}, then stats on {_fam}"] = (
            lambda t, k=_k, kw=_kw, fam=_fam: bool(_chains(t, [_is(k, fam=fam, **kw), _is("stats", fam=fam)], _quiet)))
        TRANSITIONS[f"stats, then {_k} on {_fam}"] = (
            lambda t, k=_k, kw=_kw, fam=_fam: bool(_chains(t, [_is("stats", fam=fam), _is(k, fam=fam, **kw)], _quiet)))
# lbm_run_window_stats: the window table it shares with lbm_run_window, the tables and options around it, its pieces and the tag
def _same_window(first, second, path):
    return lambda t: any(a["wkey"] == b["wkey"] and a["ty"] == b["ty"] for a, b in _chains(t, [_is(first, path), _is(second, path)], _quiet))


def _ws_a_b_then_window_b(path):
    return lambda t: any(a["wkey"] != b["wkey"] == c["wkey"]
                         for a, b, c in _chains(t, [_is("window_stats", path), _is("window_stats", path), _is("window", path)], _quiet))


def _ws_restart(context):
    return lambda t: any(e["op"] == "window_stats" and e["fam"] == "tiles" and e["context"] == context and len(e["pieces"]) >= 3
                         and any(0 < j < len(e["pieces"]) - 1 for j in e["restarts"]) for e in t if e["running"])


TRANSITIONS.update({
    "window(A), then window_stats(A) on tiles": _same_window("window", "window_stats", "tiles"),
    "window(A), then window_stats(A) on slab-tiles": _same_window("window", "window_stats", "slab-tiles"),
    "window(A), then window_stats(A) on wave": _same_window("window", "window_stats", "wave"),
    "window_stats(A), window_stats(B), window(B) on tiles": _ws_a_b_then_window_b("tiles"),
    "window_stats(A), window_stats(B), window(B) on slab-tiles": _ws_a_b_then_window_b("slab-tiles"),
    "a window_stats call, a retile, the same window": lambda t: any(
        a["wkey"] == b["wkey"] and a["ty"] != b["ty"]
        for a, _, b in _chains(t, [_is("window_stats", "tiles"), _is("opt", key="regtile"), _is("window_stats", "tiles")], _quiet)),
    "probes, window_stats, probes with the same set on tiles": lambda t: any(
        a["pset"] == b["pset"] == c["pset"] and a["ty"] == c["ty"]
        for a, b, c in _chains(t, [_is("probes", "tiles"), _is("window_stats", "tiles"), _is("probes", "tiles")], lambda e: False)),
    "set_accel, window_stats on tiles": lambda t: any(
        r["accel"] == s["accel_after"] != s["accel"] for s, r in _chains(t, [_is("set_accel"), _is("window_stats", fam="tiles")], _quiet)),
    "set_accel, window_stats on wave": lambda t: any(
        r["accel"] == s["accel_after"] != s["accel"] for s, r in _chains(t, [_is("set_accel"), _is("window_stats", "wave")], _quiet)),
    "window_stats_chunk changed between two window_stats calls with one window": lambda t: any(
        a["chunk"] != b["chunk"] and a["wkey"] == b["wkey"] and a["n"] == b["n"] and a["pieces"] != b["pieces"]
        for a, b in _chains(t, [_is("window_stats", fam="tiles")] * 2, lambda e: e["op"] != "window_stats")),
    "the pieces of a window_stats call pass TAG_WRAP on a lattice alone": _ws_restart("lone"),
    "the pieces of a window_stats call pass SLAB_TAG_MARK across p2p slabs": _ws_restart("slabs p2p"),
    "a window_stats call on slab-tiles without a window row in some slab": lambda t: any(
        e["op"] == "window_stats" and e["path"] == "slab-tiles" and 0 in e["wslabs"] for e in t if e["running"]),
})
for _fam in ("tiles", "wave"):
    TRANSITIONS[f"stats, then window_stats on {_fam}"] = (
        lambda t, fam=_fam: bool(_chains(t, [_is("stats", fam=fam), _is("window_stats", fam=fam)], _quiet)))
    TRANSITIONS[f"window_stats, then stats on {_fam}"] = (
        lambda t, fam=_fam: bool(_chains(t, [_is("window_stats", fam=fam), _is("stats", fam=fam)], _quiet)))
# (context, path family) in which lbm_run_stats must run; "thirds": a lattice alone at density 0.3
STATS_AT = ([(c, "tiles") for c in ("lone", "slabs p2p", "slabs copy", "rank p2p")] + [("lone", "wave"), ("lone", "split"), ("slabs copy", "split"),
            ("rank rccl", "split"), ("thirds", "tiles"), ("thirds", "wave")])
WINDOW_STATS_AT = list(STATS_AT) + [("thirds", "split")]     # ... and lbm_run_window_stats: the three sites of its own that hand on the density
REFUSALS = ("window", "schedule", "probes", "forces", "mean", "observed mean", "stats", "window_stats window", "window_stats every")
COVERAGE_PATHS = ("tiles R1", "tiles R2", "tiles R4", "tiles async0", "tiles async1", "slab-tiles", "tb1", "tb2", "march", "wave")
COVERAGE_CONTEXTS = ("lone", "slabs p2p", "slabs copy", "rank p2p", "rank rccl")
WINDOW_SHAPES = ("stride > 1", "a single row", "a single column", "across a tile seam", "across a slab seam", "the whole lattice")


def _window_shapes(m, case, op="window"):
    """Which of WINDOW_SHAPES the window runs (op "window_stats": the window-stats runs) of a program hold."""
    out = set()
    for e in m.trace:
        if e["op"] != op:
            continue
        x0, y0, nx, ny, sx, sy = e["wkey"]
        if (sx > 1 and nx > 1) or (sy > 1 and ny > 1):
            out.add("stride > 1")
        if ny == 1 and nx > 1:
            out.add("a single row")
        if nx == 1 and ny > 1:
            out.add("a single column")
        if e["fam"] == "tiles" and sx == 1 and sy == 1 and x0 // 64 != (x0 + nx - 1) // 64 and y0 // e["ty"] != (y0 + ny - 1) // e["ty"]:
            out.add("across a tile seam")
        if m.nslabs > 1 and sy == 1 and sum(1 for c in e["wslabs"] if c > 0) > 1:
            out.add("across a slab seam")
        if (x0, y0, nx, ny, sx, sy) == (0, 0, m.p.nx, m.p.ny, 1, 1):
            out.add("the whole lattice")
    return out


def coverage(L, programs):
    """What a table of programs covers: (pairs, contexts, transitions, refusals, window shapes, waves, mixes at the refusal point,
    (context, path family) of the stats calls and, as "window_stats at" pairs and "window_stats: " shapes, of the window-stats calls)."""
    pairs, contexts, found, refusals, shapes, waves, refusing, stats_at = set(), set(), set(), set(), set(), set(), False, set()
    for name, (setup, ctx, calls) in programs.items():
        case = setup(L)
        m = ObserverModel(L, case, ctx)
        for c in calls:
            m.apply(c)
        assert 5 <= len(calls) <= 25, name
        pairs |= {pk for pk in m.pairs if pk[1] in KINDS}
        context = "lone" if ctx is None else " ".join(str(v) for v in (ctx[0], ctx[-1]))
        contexts.add(context)
        stats_at |= {(context, e["fam"]) for e in m.trace if e["op"] == "stats"}
        if ctx is None and np.float32(m.p.density) == np.float32(THIRDS[0]):
            stats_at |= {("thirds", e["fam"]) for e in m.trace if e["op"] == "stats"}
        # (the window-stats calls in the same two sets, marked: the tuple this function returns keeps its length)
        thirds = ctx is None and np.float32(m.p.density) == np.float32(THIRDS[0])
        stats_at |= {("window_stats", c, e["fam"]) for e in m.trace if e["op"] == "window_stats" for c in ((context, "thirds") if thirds else (context,))}
        found |= {t for t, holds in TRANSITIONS.items() if holds(m.trace)}
        shapes |= _window_shapes(m, case) | {"window_stats: " + s for s in _window_shapes(m, case, "window_stats")}
        waves |= m.waves
        for e in m.trace:
            if e["op"] == "refused":                             # in the middle of a program: a running call before and after
                if any(x["running"] for x in m.trace[:e["i"]]) and any(x["running"] for x in m.trace[e["i"] + 1:]):
                    refusals.add(e["what"])
        point = tuple(np.float32(v) for v in (m.p.density, m.p.accel, m.p.omega))
        if point == tuple(np.float32(v) for v in PARAM_GRID["refusal"]):
            mix = {(e["op"], e["path"]) for e in m.trace if e["running"]}
            refusing = refusing or (all((k, q) in mix for k in ("driven", "window", "observed") for q in ("tiles", "march", "wave"))
                                    and any(e["op"] == "driven" and e["sched_name"] == "b" for e in m.trace))
    return pairs, contexts, found, refusals, shapes, waves, refusing, stats_at


def missing(L, programs):
    pairs, contexts, found, refusals, shapes, waves, refusing, stats_at = coverage(L, programs)
    out = [(lab, k) for lab in COVERAGE_PATHS for k in KINDS if (lab, k) not in pairs]
    out += [c for c in COVERAGE_CONTEXTS if c not in contexts]
    out += [t for t in TRANSITIONS if t not in found]
    out += ["refused: " + r for r in REFUSALS if r not in refusals]
    out += ["window: " + s for s in WINDOW_SHAPES if s not in shapes]
    out += ["stats on %s, %s" % at for at in STATS_AT if at not in stats_at]
    out += ["window: window_stats: " + s for s in WINDOW_SHAPES if "window_stats: " + s not in shapes]
    out += ["window_stats on %s, %s" % at for at in WINDOW_STATS_AT if ("window_stats",) + at not in stats_at]
    if len({k for k, _ in waves if k in (4, 6, 8)}) < 2:
        out.append("lbm_wave at two of K = 4, 6, 8")
    if not any(c == 2 for _, c in waves):
        out.append("wave_cols 2")
    if not refusing:
        out.append("no program mixes driven (b), window and observed over tiles, march and wave where the guard refuses cells")
    return out


def test_program_table_covers_every_path_and_transition(L):
    assert not missing(L, PROGRAMS), missing(L, PROGRAMS)
    for name, (setup, ctx, calls) in PROGRAMS.items():
        m, case = _walk(L, name)
        assert any(case["ob"][jj, ii] != 0 for xy in case["psets"].values() for ii, jj in xy) and len(case["psets"]) == 2, name
        assert not {tuple(c) for c in case["psets"]["B"].tolist()} <= {tuple(c) for c in case["psets"]["A"].tolist()}, name
        for e in m.trace:
            if not e["running"]:
                continue
            where = (name, e["call"])
            assert e["path"] in PATHS and (e["path"] == "slab-tiles") == (ctx is not None and e["path"] in TILE_PATHS), where
            assert 1 <= e["n"] <= 60 or name in LONG_CALLS, where
            assert (e["fam"] != "wave") or e["n"] >= e["tb"] >= 4, where              # lbm_wave runs: a full pass at least
            if e["op"] == "observed":
                assert len(e["kinds"]) >= 2, where                                     # (one observer alone is its own call)
            assert all(k in (F, P, M, S, "window", "stats", "window_stats") for k in e["kinds"]), where
            assert ("stats" in e["kinds"]) == (e["op"] == "stats") == (e["ste"] > 0) and e["ste"] <= e["n"], where
            for k, ev in ((P, e["pe"]), (M, e["me"]), (S, e["fe"])):
                assert (k in e["kinds"] or (k == S and bool(e["win"]))) == (ev > 0) and ev <= e["n"], where
            if e["win"]:
                assert 0 < e["fe"] <= e["n"], where
            assert (P not in e["kinds"] or e["pset"]) and (F not in e["kinds"] or e["nb"] > 0), where
            assert sum(e["pieces"]) == e["n"] and all(k > 0 for k in e["pieces"]), where
            if e["op"] == "window_stats":
                assert ("window_stats" in e["kinds"]) and e["m"] >= 1 and 0 <= e["chunk"] <= 2, where
                assert len(e["pieces"]) == window_stats_pieces_of(e["n"], e["fe"], e["chunk"], e["fam"], e["wcells"]), where
                if e["fam"] == "tiles":                          # every piece but the tail ends on a sample step
                    assert all(b % e["fe"] == 0 for b in e["ends"][:-1]) and e["ends"][-1] == e["n"], where
            else:
                assert len(e["pieces"]) == pieces_of(e["n"], *e["cutters"]), where
        for e in m.trace:                                        # the windows the programs run are windows; the refused one is not
            if e["op"] in ("window", "window_stats"):
                L.window_rows(case["windows"][e["win"]], m.p.nx, m.p.ny, 0, m.p.ny)
            if e["op"] == "refused" and e["what"] in ("window", "window_stats window"):
                with pytest.raises(L.LbmError):
                    L.window_rows(case["windows"][e["args"][2]], m.p.nx, m.p.ny, 0, m.p.ny)
            if e["op"] == "refused" and e["what"] == "window_stats every":
                assert e["args"][1] > e["args"][0] > 0
                L.window_rows(case["windows"][e["args"][2]], m.p.nx, m.p.ny, 0, m.p.ny)


@pytest.mark.parametrize("drop", [("lone_128_flavour_walk", 4), ("wave6_maps_130x37", 6), ("slabs_p2p_tiles_tag_restart", 12),
                                  ("rank_ring_of_one_rccl", None), ("schedule_table_128x16", 4), ("never_tiles_tb1_tb2", 12),
                                  ("stats_neighbours_on_tiles_128", 9), ("stats_neighbours_on_wave6_130x37", 13),
                                  ("stats_tilings_and_tag_wrap_128x16", 9), ("stats_slabs_copy_256x32", 10), ("stats_at_thirds_256x64", None),
                                  ("rank_ring_of_one_p2p", 9), ("stats_never_tiles_tb1", 3),
                                  # lbm_run_window_stats: the window call in front of one over the same window; the second of
                                  # A, B, window(B); the retile between two; the probes behind one; set_accel in front of one;
                                  # the second of two chunks; the tag option in front of the wrap and of the restart; the stats
                                  # call behind and in front of one; the two refused ones; a context, a path, the split path at
                                  # density 0.3; the 0.3 program
                                  ("window_stats_walk_on_tiles_128", 2), ("window_stats_slabs_p2p_tag_restart", 4),
                                  ("window_stats_retile_and_tag_wrap_256", 4), ("window_stats_walk_on_tiles_128", 8),
                                  ("window_stats_on_wave6_130x37", 9), ("window_stats_walk_on_tiles_128", 9),
                                  ("window_stats_retile_and_tag_wrap_256", 8), ("window_stats_slabs_p2p_tag_restart", 8),
                                  ("window_stats_walk_on_tiles_128", 15), ("window_stats_on_wave6_130x37", 5),
                                  ("window_stats_walk_on_tiles_128", 16), ("window_stats_on_wave6_130x37", 11),
                                  ("rank_ring_of_one_rccl", 11), ("rank_ring_of_one_p2p", 10), ("window_stats_never_tiles_tb1_tb2", 3),
                                  ("window_stats_slabs_copy_256x32", 8), ("window_stats_at_thirds_256x64", 12),
                                  ("window_stats_at_thirds_256x64", None)])
def test_a_trimmed_table_fails_the_coverage_check(L, drop):
    """Without one call (a flavour of the walk, a relabel, the tag option, the long driven call, a refused call; a stats call
    between two windows or two driven calls, the tag option in front of one, the one whose pieces pass a mark, the one of a
    context or a path; the calls around a window-stats call listed above) or one program (a context, the density 0.3) the
    table no longer covers the list."""
    name, index = drop
    programs = dict(PROGRAMS)
    if index is None:
        del programs[name]
    else:
        setup, ctx, calls = programs[name]
        programs[name] = (setup, ctx, calls[:index] + calls[index + 1:])
    assert missing(L, programs)


def test_model_restates_the_tag_and_capacity_rules(L):
    """The model's own arithmetic on the programs that cross the marks and grow the schedule table (so a wrong model cannot
    pass the GPU test vacuously)."""
    m, _ = _walk(L, "lone_tag_wrap_in_flavours")
    t = {e["i"]: e for e in m.trace}
    assert t[3]["tag"] == 1 + 6
    assert t[5]["tag"] == 1 + 13 and t[5]["restarts"] == [0]                       # cleared in front of the window run
    assert t[7]["tag"] == 1 + 10 and t[7]["restarts"] == [0]
    assert t[9]["pieces"] == [4, 4, 4] and t[9]["restarts"] == [1]                 # the second piece would reach the mark
    assert t[9]["tag"] == 1 + 5 + 5
    assert t[10]["tag"] == 11 + 9 and t[11]["tag"] == 20 + 9 and t[13]["tag"] == 29 + 7 + 5
    m, _ = _walk(L, "slabs_p2p_tiles_tag_restart")
    e = m.trace[13]
    assert e["op"] == "driven_observed" and e["pieces"] == [4, 2, 2, 4] and e["restarts"] == [1]
    assert e["tag"] == 1 + 3 + 5 and m.trace[14]["tag"] == 9 + 6                   # cleared behind the second piece
    assert m.trace[15]["op"] == "stats" and m.trace[15]["pieces"] == [3, 3] and m.trace[15]["tag"] == 15 + 4 + 4
    assert m.trace[11]["pieces"] == [5, 5] and m.trace[11]["tag"] - m.trace[10]["tag"] == 6 + 6
    m, _ = _walk(L, "schedule_table_128x16")
    first, second, third = m.trace[3], m.trace[4], m.trace[5]
    assert _grow(0, first["n"]) == 1024 < second["n"] and not first["dtab_grew"] and second["dtab_grew"] and m.dtab_cap == 2048
    assert third["pieces"] == [12, 4, 8, 8, 4, 12] and not third["dtab_grew"]      # the pieces start at pairs 12, 16, 24, 32, 36
    assert third["tag"] - second["tag"] == 48 + 6
    assert expected_keys(third) == {"driven_observed_in_kernel": 1, "driven_observed_in_wave": 0, "driven_observed_pieces": 6}
    m, _ = _walk(L, "wave6_maps_130x37")
    e = next(x for x in m.trace if x["op"] == "observed")
    assert e["pieces"] == [7, 7] and expected_keys(e) == {"observed_in_kernel": 0, "observed_in_wave": 3, "observed_pieces": 2}
    m, _ = _walk(L, "never_tiles_tb1_tb2")
    e = next(x for x in m.trace if x["op"] == "driven_observed")
    assert e["pieces"] == [1, 1, 1, 1, 1, 1, 1, 1, 1] and set(expected_keys(e).values()) == {0}
    e = next(x for x in m.trace if x["op"] == "observed")
    assert e["ends"] == [2, 3, 4, 6, 8, 9] and expected_keys(e)["observed_pieces"] == 6
    assert all(x["tag"] == 1 for x in m.trace)
    # lbm_run_stats: a plain launch per sample on the tiles, the marks tested per piece; one run inside lbm_wave
    m, _ = _walk(L, "stats_tilings_and_tag_wrap_128x16")
    e = m.trace[9]
    assert e["call"] == stats(12, 4, "tiles") and e["pieces"] == [4, 4, 4] and e["restarts"] == [1] and e["tag"] == 1 + 5 + 5
    assert m.trace[3]["pieces"] == [2, 2, 1] and m.trace[3]["tag"] == 1 + 4 + 3 + 3 + 2 and expected_keys(e) == {"stats_in_wave": 0}
    m, _ = _walk(L, "stats_slabs_copy_256x32")
    e = m.trace[10]
    assert e["call"] == stats(12, 4, "slab-tiles") and e["pieces"] == [4, 4, 4] and e["restarts"] == [1] and e["tag"] == 1 + 5
    assert m.trace[3]["pieces"] == [3, 3, 1] and m.trace[3]["tag"] == 1 and expected_keys(m.trace[3]) == {"stats_in_wave": 0}
    m, _ = _walk(L, "stats_neighbours_on_wave6_130x37")
    e = m.trace[4]
    assert e["call"] == stats(13, 3, "wave") and e["pieces"] == [13] and expected_keys(e) == {"stats_in_wave": 1} and e["tag"] == 1
    # lbm_run_window_stats: pieces of `chunk` sample steps and the tail on the tiles, n_i + 1 tags a piece, the marks per piece
    m, _ = _walk(L, "window_stats_walk_on_tiles_128")
    t = {e["i"]: e for e in m.trace}
    assert t[2]["tag"] == 1 + 7 and t[3]["pieces"] == [6] and t[3]["tag"] == 8 + 7              # automatic: one piece of three samples
    assert t[4]["pieces"] == [6, 1] and t[4]["tag"] == 15 + 7 + 2                               # ... and the tail
    assert t[7]["call"] == window_stats(9, 2, "wake", "tiles", 2) and t[7]["pieces"] == [4, 4, 1] and t[7]["tag"] - t[6]["tag"] == 5 + 5 + 2
    assert t[9]["pieces"] == [2, 2, 2, 2, 1] and t[9]["tag"] - t[8]["tag"] == 4 * 3 + 2 and t[9]["chunk"] == 1
    assert expected_keys(t[9]) == {"window_stats_in_kernel": 1, "window_stats_in_wave": 0, "window_stats_pieces": 5}
    assert t[11]["chunk"] == 0 and t[11]["pieces"] == [6] and t[14]["chunk"] == 0 and t[14]["pieces"] == [6, 1]
    m, _ = _walk(L, "window_stats_retile_and_tag_wrap_256")
    e = m.trace[9]
    assert e["call"] == window_stats(12, 4, "seam", "tiles", 1) and e["pieces"] == [4, 4, 4] and e["restarts"] == [1] and e["tag"] == 1 + 5 + 5
    assert m.trace[7]["pieces"] == [4, 2, 1] and m.trace[7]["chunk"] == 2                       # three samples in chunks of two: a cut piece
    m, _ = _walk(L, "window_stats_slabs_p2p_tag_restart")
    e = m.trace[9]
    assert e["call"] == window_stats(12, 4, "A", "slab-tiles") and e["chunk"] == 1 and e["pieces"] == [4, 4, 4] and e["restarts"] == [1] and e["tag"] == 1 + 5
    assert m.trace[6]["wslabs"] == [0, 0, 0, 6] and m.trace[3]["wslabs"] == [2, 3, 0, 0]        # in one slab; across the first seam
    m, _ = _walk(L, "window_stats_on_wave6_130x37")
    e = m.trace[4]
    assert e["pieces"] == [13] and e["tag"] == 1 and expected_keys(e) == {"window_stats_in_kernel": 0, "window_stats_in_wave": 1, "window_stats_pieces": 1}
    m, _ = _walk(L, "window_stats_slabs_copy_256x32")
    e = m.trace[3]
    assert e["pieces"] == [3, 3, 1] and e["tag"] == 1 and expected_keys(e) == {"window_stats_in_kernel": 0, "window_stats_in_wave": 0, "window_stats_pieces": 3}
    # the automatic chunk where the bound bites: 16 MiB a sample of a 1024 x 1024 window, four to a piece
    assert window_stats_pieces_of(9, 1, 0, "tiles", cells=1024 * 1024) == 3


# ---------------------------------------------------------------------------------------------------------------- GPU
class InChunks:
    """The float oracle's av_velocity and reynolds of a state with the rows' sums added in double: what
    test_call_sequences._check_derived is handed here.  Its bar (1e-5 per 65536 cells) allows for the order of the
    additions; but the oracle adds all the cells' speeds serially in float, and a few steps from rest, where most speeds
    are tiny, that sum alone is further than the bar from the same float speeds added in double: on 1024 x 128 up to 4.4e-5
    over the first 40 steps (steps 3 to 13 all between 1.1e-5 and 4.4e-5; measured on the CPU, the test below), against
    the 2e-5 the bar leaves that lattice.  The library adds per block in float and the blocks in double.  Here the oracle's
    own function runs on 64 cells at a time (its per-cell float arithmetic, no cell looks at a neighbour; at most 64 serial
    float additions) and the chunks are combined in double, weighted by their fluid cells; the bars stay.  reynolds is
    av_velocity times a constant of the parameters (reynolds_dim over the viscosity): the oracle's own ratio on the state."""
    CHUNK = 64

    def __init__(self, O, oracle):
        self.O, self.oracle = O, oracle

    def av_velocity(self, prm, st, ob):
        st = np.ascontiguousarray(st, dtype=np.float32).reshape(-1, 9)
        ob = np.ascontiguousarray(ob, dtype=np.int32).reshape(-1)
        tot, cnt = 0.0, 0
        for c0 in range(0, len(ob), self.CHUNK):
            cells, blocked = st[c0:c0 + self.CHUNK], ob[c0:c0 + self.CHUNK]
            n = int((blocked == 0).sum())
            if n:
                row = self.O.OrcParam(len(blocked), 1, prm.maxIters, prm.reynolds_dim, prm.density, prm.accel, prm.omega)
                tot += float(self.oracle.av_velocity(row, cells, blocked)) * n
                cnt += n
        return tot / cnt

    def reynolds(self, prm, st, ob):
        whole = float(self.oracle.av_velocity(prm, st, ob))
        return self.av_velocity(prm, st, ob) * float(self.oracle.reynolds(prm, st, ob)) / whole


def test_the_derived_reference_is_the_float_oracles_without_its_long_sum(L, O, oracle):
    """InChunks on the 1024 x 128 case over the first 13 steps from rest: within 2e-6 (_check_derived's own bar for it) of the
    same per-cell float speeds summed in double, reynolds in the oracle's own ratio -- while the oracle's sum over the whole
    lattice passes the 2e-5 that _check_derived leaves this lattice."""
    case = _c8(L)
    p, ob = case["p"], case["ob"]
    op = O.OrcParam(p.nx, p.ny, p.maxIters, p.reynolds_dim, p.density, p.accel, p.omega)
    chunks, f, worst = InChunks(O, oracle), case["cells"].copy(), 0.0
    for _ in range(13):
        oracle.run(op, f, ob, 1)
        rho = f[..., 0].copy()
        for k in range(1, 9):
            rho = rho + f[..., k]
        ux = (f[..., 1] + f[..., 5] + f[..., 8] - (f[..., 3] + f[..., 6] + f[..., 7])) / rho
        uy = (f[..., 2] + f[..., 5] + f[..., 6] - (f[..., 4] + f[..., 7] + f[..., 8])) / rho
        want = float(np.sqrt(ux * ux + uy * uy, dtype=np.float32)[ob == 0].astype(np.float64).sum() / (ob == 0).sum())
        got, whole = chunks.av_velocity(op, f, ob), float(oracle.av_velocity(op, f, ob))
        assert abs(got - want) <= 2e-6 * want, (got, want)
        ratio = float(oracle.reynolds(op, f, ob)) / whole
        assert abs(chunks.reynolds(op, f, ob) / got - ratio) <= 1e-6 * ratio
        worst = max(worst, abs(whole - want) / want)
    assert worst > 2e-5, worst


class Shadow:
    """The one-step kernel on its own long-lived context, one step per call wherever anything is wanted of a step; keeps
    its av_vels, the acceleration of every step and its state at the anchor step."""

    def __init__(self, L, p, ob, cells, anchor, kw):
        self.lat = L.Lattice(p, ob, cells, **kw)
        self.lat.set_option("time_block", 1)
        assert self.lat.info("engine") == 1 and (kw or self.lat.info("time_block_active") == 1)
        self.ob, self.anchor, self.done, self.av, self.accels, self.at_anchor = ob, anchor, 0, [], [], None
        self.accel, self.body, self.nb = np.float32(p.accel), None, 0

    def set_bodies(self, body, nb):
        self.lat.set_bodies(body, nb)
        self.body, self.nb = body, nb

    def _stepped(self, av, accels):
        self.done += len(av)
        self.av.append(av)
        self.accels.extend(float(a) for a in accels)
        if self.done == self.anchor and self.at_anchor is None:
            self.at_anchor = self.lat.read_state()
        assert self.lat.info("engine_last") == 1

    def run(self, n):
        """n steps under the context's acceleration (splitting a one-step run changes no bit)."""
        self.lat.set_accel(float(self.accel))
        out = []
        k = self.anchor - self.done
        for m in ((k, n - k) if 0 < k < n else (n,)):
            out.append(self.lat.run(m))
            self._stepped(out[-1], [self.accel] * m)
        return np.concatenate(out)

    def steps(self, accels, fields, states):
        """One step per entry of accels: (av_vels, forces or None, fields after every step or None, numpy forces and their
        scale or None)."""
        av, Fs, X, W, A = [], [], [], [], []
        for a in accels:
            self.lat.set_accel(float(a))
            if self.nb:
                a1, f1 = self.lat.run_forces(1)
                Fs.append(f1[0])
            else:
                a1 = self.lat.run(1)
            self._stepped(a1, [a])
            av.append(a1)
            if fields:
                X.append(self.lat.final_state())
            if states:
                w, s = forces_from_state(self.lat.read_state(), self.ob, self.body, self.nb)
                W.append(w)
                A.append(s)
        self.lat.set_accel(float(self.accel))                    # (a driven call leaves the context's own acceleration)
        return (np.concatenate(av), np.array(Fs) if self.nb else None, np.array(X) if fields else None,
                (np.array(W), np.array(A)) if states else None)


def hold_anchor(st_a, ref, av, av_o):
    """The anchor's bars: the shadow's lattice st_a and av_vels against the strict float oracle's ref and av_o.  Returns the
    worst deviations as fractions of the bars."""
    ref = ref.reshape(st_a.shape)
    bar = 2e-5 * np.abs(ref) + 2e-6 * np.abs(ref).max()
    assert np.all(np.abs(st_a - ref) <= bar)
    assert np.allclose(av, av_o, rtol=1e-4, atol=0)
    return float(np.max(np.abs(st_a - ref) / bar)), float(np.max(np.abs(av - av_o) / (1e-4 * np.abs(av_o))))


def _schedule(sched, p, accel, n):
    if sched is None or sched == "const":
        return np.full(n, accel, dtype=np.float32)
    name, seed = sched
    spikes = (int(name[1:]),) if name[0] == "d" else None
    return schedules(float(np.float32(p.accel)), n, seed, spikes)[name]


def _check_engine(lat, e):
    path = e["path"]
    info = {k: lat.info(k) for k in ("engine_last", "time_block_active", "march_kernel", "regtile", "regtile_async", "time_block", "wave_cols_active")}
    where = (e["call"], info)
    if path in TILE_PATHS:
        assert info["engine_last"] == 3, where
        assert info["regtile"] == e["ty"] * 10 + e["r"], where
        if path == "tiles":
            assert info["regtile_async"] == e["asy"], where
    else:
        assert info["engine_last"] == 1, where
        assert info["time_block_active"] == {"tb1": 1, "tb2": 2, "march": 4}.get(path, e["tb"]), where
        if path in ("march", "wave") or e["lone"]:       # (slabs report the kernel their K would march with, marching or not)
            assert info["march_kernel"] == (1 if path == "wave" else 0), where
    for key, v in expected_keys(e).items():
        assert lat.info(key) == v, (e["call"], key, lat.info(key), v)


def _same(got, want, where):
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (where, len(bad), [tuple(int(v) for v in b) for b in bad[:6]])


def _want(e):
    return dict(forces=F in e["kinds"], probes_every=e["pe"], mean_every=e["me"], fields_every=e["fe"])


def _call(lat, e, case, acc):
    """The call on a context: (av_vels, {"forces", "probes", "mean", "fields", "window": what it returned})."""
    op, n = e["op"], e["n"]
    if op == "run":
        return lat.run(n), {}
    if op == "sampled":
        av, out = lat.run_sampled(n, e["fe"])
        return av, {S: out}
    if op == "forces":
        av, out = lat.run_forces(n)
        return av, {F: out}
    if op == "probes":
        av, out = lat.run_probes(n, e["pe"])
        return av, {P: out}
    if op == "mean":
        av, out = lat.run_mean(n, e["me"])
        return av, {M: out}
    if op == "window":
        av, out = lat.run_window(n, e["fe"], case["windows"][e["win"]])
        return av, {"window": out}
    if op == "driven":
        return lat.run_driven(acc), {}
    if op == "stats":
        av, out = lat.run_stats(n, e["ste"])
        return av, {"stats": out}
    if op == "window_stats":
        if e["call"][4] is not None:
            lat.set_option("window_stats_chunk", e["call"][4])
        assert lat.info("window_stats_chunk") == e["chunk"]
        av, out = lat.run_window_stats(n, e["fe"], case["windows"][e["win"]])
        return av, {"window_stats": out}
    res = lat.run_observed(n, **_want(e)) if op == "observed" else lat.run_driven_observed(acc, **_want(e))
    return res.pop("av_vels"), res


def _unscheduled(L, case, ctx, e, st0, xy):
    """The same call without its schedule on a fresh context of the same kind, tiling, state, acceleration, bodies and
    probes: (av_vels, outputs)."""
    p = case["p"]
    px = L.Param(p.nx, p.ny, p.maxIters, p.reynolds_dim, p.density, float(e["accel"]), p.omega)
    with _open(L, px, case["ob"], st0, ctx) as twin:
        if ctx is None:
            twin.set_option("regtile", e["ty"] * 10 + e["r"])
        twin.set_option("regtile_async", e["asy"])
        if e["nb"]:
            twin.set_bodies(e["body"], e["nb"])
        if xy is not None:
            twin.set_probes(xy)
        plain = dict(e, op="run" if e["op"] == "driven" else "observed")
        out = _call(twin, plain, case, None)
        assert twin.info("engine_last") == 3
    return out


def _refuse(L, lat, e, case):
    what, a = e["what"], e["args"]
    with pytest.raises(L.LbmError, match=r"\[lbm error 1\]"):
        if what == "window":
            lat.run_window(a[0], a[1], case["windows"][a[2]])
        elif what == "schedule":
            s = schedules(float(np.float32(case["p"].accel)), a[0], 3)["b"].copy()
            s[a[1]] = a[2]
            lat.run_driven(s)
        elif what == "probes":
            lat.run_probes(a[0], a[1])
        elif what == "forces":
            lat.run_forces(a[0])
        elif what == "mean":
            lat.run_mean(a[0], a[1])
        elif what == "stats":
            lat.run_stats(a[0], a[1])
        elif what in ("window_stats window", "window_stats every"):
            lat.run_window_stats(a[0], a[1], case["windows"][a[2]])
        else:
            assert what == "observed mean"
            lat.run_observed(a[0], forces=e["nb"] > 0, mean_every=a[1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_observer_sequence(gpu, O, oracle, monkeypatch, name):
    L = gpu
    t0 = time.perf_counter()
    setup, ctx, calls = PROGRAMS[name]
    case = setup(L)
    p, ob, cells0 = case["p"], case["ob"], case["cells"]
    model = ObserverModel(L, case, ctx)
    op = O.OrcParam(p.nx, p.ny, p.maxIters, p.reynolds_dim, p.density, p.accel, p.omega)
    total = sum(c[1] for c in calls if c[0] in RUNNING)
    anchor = min(ANCHOR_OVERRIDE.get(name, ANCHOR_STEPS), total)
    # forces across slabs off the register tiles are the bits of the loop on such a context: the shadow is one
    split_forces = ctx is not None and ctx[0] == "slabs" and any(e["running"] and F in e["kinds"] and e["fam"] != "tiles"
                                                                  for e in _walk(L, name)[0].trace)
    kw = {}
    if split_forces:
        kw = dict(nslabs=ctx[1], devices=[0] * ctx[1], exchange=L.EXCHANGE_P2P if ctx[2] == "p2p" else L.EXCHANGE_COPY)
    sh = Shadow(L, p, ob, cells0, anchor, kw)
    try:
        if ctx is not None and ctx[0] == "rank":
            monkeypatch.setenv("LBM_FORCE_EXCHANGE", "1")
        with _open(L, p, ob, cells0, ctx) as lat:
            prev_kind, derived_checks, xy = None, 0, None
            for call in calls:
                e = model.apply(call)
                kind = e["op"]
                where = (name, e["i"], call)
                if kind == "opt":
                    lat.set_option(call[1], call[2])
                elif kind == "bodies":
                    lat.set_bodies(case["labellings"][call[1]] if call[1] else None, call[2])
                    sh.set_bodies(case["labellings"][call[1]] if call[1] else None, call[2])
                elif kind == "probe_set":
                    xy = case["psets"][call[1]] if call[1] else None
                    lat.set_probes(xy)
                elif kind == "set_accel":
                    lat.set_accel(call[1])
                    sh.accel = np.float32(call[1])
                elif kind == "refused":
                    _refuse(L, lat, e, case)
                else:
                    n, kinds, tiles = e["n"], e["kinds"], e["fam"] == "tiles"
                    acc = _schedule(e["sched"], p, e["accel"], n)
                    want_fields = any(k in kinds for k in (P, M, S, "window", "stats", "window_stats"))
                    st0 = lat.read_state() if e["sched"] == "const" else None
                    if kind == "run":
                        av_sh, F_sh, X, numpy_forces = sh.run(n), None, None, None
                    else:
                        av_sh, F_sh, X, numpy_forces = sh.steps(acc, want_fields, tiles and F in kinds)
                    av, out = _call(lat, e, case, acc)
                    # ---- the outputs
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
                        if not _kept(ob, e["body"]).any():
                            assert np.all(out[F] == 0), where
                    # ---- av_vels
                    assert av.shape == (n,) and np.allclose(av, av_sh, rtol=AV_RTOL, atol=0), (where, np.max(np.abs(av - av_sh) / np.abs(av_sh)))
                    if ctx is None and e["path"] == "tb1":
                        _same(av, av_sh, where + ("av_vels",))                         # the same one-step kernel ran
                    if e["sched"] == "const":
                        assert tiles, where
                        av_p, out_p = _unscheduled(L, case, ctx, e, st0, xy)
                        _same(av, av_p, where + ("av_vels without the schedule",))
                        for k in out_p:
                            _same(out[k], out_p[k], where + (k, "without the schedule"))
                    _check_engine(lat, e)
                # ---- after every call: the tag, the acceleration, the lattice
                assert lat.info("regtile_tag") == e["tag"], (where, lat.info("regtile_tag"), e["tag"])
                assert np.float32(lat.info("accel")) == model.accel, (where, lat.info("accel"), model.accel)
                st = lat.read_state()
                _same(st, sh.lat.read_state(), where + ("lattice",))
                if not e["running"]:
                    continue
                if prev_kind is not None and kind != prev_kind:
                    _check_derived(lat, st, InChunks(O, oracle), op, ob)
                    derived_checks += 1
                prev_kind = kind
            assert derived_checks >= 1
        # the shadow against the strict float oracle over the first steps, with the accelerations it was given
        ref = cells0.copy()
        av_o, refusals = [], 0
        for a in sh.accels[:anchor]:
            refusals += int(guard_refuses(p.density, a, ob, ref).sum())
            av_o.append(driven_oracle(oracle, op, ref, ob, np.array([a], dtype=np.float32))[0])
        st_a = sh.at_anchor
        assert st_a is not None and len(av_o) == anchor
        hold_anchor(st_a, ref, np.concatenate(sh.av)[:anchor], np.array(av_o))
        if name in REFUSING:
            assert refusals > 0                   # the guard refused cells inside the sequence
    finally:
        sh.lat.close()
    print("%s: %.1f s" % (name, time.perf_counter() - t0))
