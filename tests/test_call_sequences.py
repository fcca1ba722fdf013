"""One context through mixed runs, relabels and option changes (lbm_run, lbm_run_sampled, lbm_run_forces, lbm_set_bodies,
lbm_set_option on ONE long-lived context).

Every other GPU test opens a fresh context and drives it through one kind of call.  A context carries state from call to
call -- the lattice parity, the mailbox tags of the register tiles, their force tables (keyed on the tile height), buffers
that only grow, the bodies, the engine options -- and a mistake there shows up only on the second or third call.  Each
program below is one context and a short list of calls, with the path each call must take.  A shadow context on the same
initial lattice (engine 1, time_block 1: lbm_sweep alone, the kernel pinned to the reference's known answers) mirrors every
call: plain runs as plain runs, forces runs as one step + lbm_read_state at a time with the forces evaluated in float64 from
each state (tests/test_body_forces.py: forces_from_state), sampled runs in pieces with lbm_final_state at the sample steps.
After every call: the lattice bit for bit, av_vels, forces, snapshots, the path taken (no silent fall-back), the mailbox tag
the context reports, and, after a change of run kind, the derived quantities from the state.  The shadow itself is anchored
to the strict float oracle over each program's first <= 50 steps.

The table is checked without a GPU against a declared coverage list (engine path x run kind, and the state transitions),
so that trimming it fails on CPU."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, deck_paths
from test_body_forces import CX, CY, LBM_EINVAL, _bits, _close, forces_from_state

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden import PARAM_GRID, param_state, refused  # noqa: E402

MAX_BODIES = 4
TAG_WRAP = 0x7fffff00            # a lattice alone clears its mailboxes in front of the run that would reach this tag
SLAB_TAG_MARK = 0x60000000       # slabs clear theirs behind the run that passes this one
ANCHOR_STEPS = 50
W_EQ = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)


# ---------------------------------------------------------------------------------------------------------------- table
# Calls.  path: "tiles" (lbm_regtile, a lattice alone), "slab-tiles" (lbm_regtile_slabs), "tb1" (lbm_sweep), "tb2" (lbm_sweep2,
# where the lattice takes it), "march" (lbm_march), "wave" (lbm_wave<time_block>).  For the streaming engines the path is the
# kernel the context's options select; a forces run there always steps with the one-step kernel and a force kernel behind it.
def run(n, path):
    return ("run", n, path)


def sampled(n, every, path):
    return ("sampled", n, every, path)


def forces(n, path):
    return ("forces", n, path)


def forces_refused(n):
    return ("forces_refused", n)


def bodies(name, nb):
    return ("bodies", name, nb)


def clear():
    return ("bodies", None, 0)


def opt(key, value):
    return ("opt", key, value)


def _deck(L, deck):
    pf, of = deck_paths(deck)
    p = L.read_params(pf)
    ob = np.ascontiguousarray(L.read_obstacles(of, p), dtype=np.int32).reshape(p.ny, p.nx)
    cells = np.ascontiguousarray(np.broadcast_to((np.float32(p.density) * W_EQ).astype(np.float32), (p.ny, p.nx, 9)))
    return p, ob, cells


def _random(L, nx, ny, seed, max_iters=100, blocked=0.1):
    rng = np.random.default_rng(seed)
    p = L.Param(nx, ny, max_iters, 10, 0.1, 0.01, 1.85)
    ob = (rng.random((ny, nx)) < blocked).astype(np.int32)
    cells = (0.1 * W_EQ * (1.0 + 0.2 * (rng.random((ny, nx, 9)) - 0.5))).astype(np.float32)
    return p, ob, cells


def _labels(ob, seed, nb, zero=False):
    """Labels 1..nb (and 0, not counted, if zero) at random on the blocked cells."""
    rng = np.random.default_rng(seed)
    return np.where(ob != 0, rng.integers(0 if zero else 1, nb + 1, size=ob.shape), 0).astype(np.int32)


def _walls_and_rest(ob):
    walls = np.zeros(ob.shape, dtype=bool)
    walls[0], walls[-1] = ob[0] != 0, ob[-1] != 0
    return np.where(walls, 1, np.where(ob != 0, 2, 0)).astype(np.int32)


def _p1(L):
    p, ob, cells = _deck(L, "128x128")
    a = _labels(ob, 31, 4)
    perm = np.array([0, 3, 1, 4, 2])                  # B: the same cells, the same nb, the labels permuted
    return p, ob, cells, {"A": a, "B": perm[a].astype(np.int32)}


def _p2(L):
    p, ob, cells = _deck(L, "256x256")
    return p, ob, cells, {"walls+rest": _walls_and_rest(ob)}


def _p3(L):
    p, ob, cells = _random(L, 128, 16, 41, max_iters=8)
    return p, ob, cells, {"random4": _labels(ob, 42, 4, zero=True)}


def _p4(L):
    p, ob, cells = _deck(L, "256x256")
    return p, ob, cells, {"walls+rest": _walls_and_rest(ob)}


def _p5(L):
    p, ob, cells = _random(L, 256, 32, 51)
    return p, ob, cells, {"random3": _labels(ob, 52, 3)}


def _p6(L):
    pf, of = deck_paths("1024x1024")
    p0 = L.read_params(pf)
    p = L.Param(1024, 128, p0.maxIters, p0.reynolds_dim, p0.density, p0.accel, p0.omega)
    ob = np.ascontiguousarray(L.read_obstacles(of, p0)[:128], dtype=np.int32)
    cells = np.ascontiguousarray(np.broadcast_to((np.float32(p.density) * W_EQ).astype(np.float32), (p.ny, p.nx, 9)))
    return p, ob, cells, {"walls+rest": _walls_and_rest(ob)}


def _p7(L):
    p, ob, cells = _random(L, 130, 37, 71, blocked=0.12)
    ob[15:20, 60:65] = 1                              # a solid 5 x 5 block: its 3 x 3 core has no fluid neighbour
    core = np.zeros(ob.shape, dtype=np.int32)
    core[16:19, 61:64] = 1
    return p, ob, cells, {"random4": _labels(ob, 72, 4, zero=True), "random2": _labels(ob, 73, 2), "core": core}


def _p8(L):
    p, ob, cells = _random(L, 128, 64, 81)
    return p, ob, cells, {"random4": _labels(ob, 82, 4)}


def _p9(L):
    nx, ny = 256, 64
    ob, cells = param_state("refusal", nx, ny, 91, "rest")
    density, accel, omega = PARAM_GRID["refusal"]
    p = L.Param(nx, ny, 100, 10, density, accel, omega)
    ob = np.ascontiguousarray(ob, dtype=np.int32).reshape(ny, nx)
    return p, ob, np.ascontiguousarray(cells, dtype=np.float32), {"blocked": (ob != 0).astype(np.int32)}


# ctx: None = a lattice alone; ("slabs", n, exchange) = n slabs of one process on device 0; ("rank", exchange) = a rank
# context that is a ring of one (LBM_FORCE_EXCHANGE=1, as the ring-of-one tests)
PROGRAMS = {
    "lone_128_default_tiles": (_p1, None, [
        run(7, "tiles"), bodies("A", 4), forces(9, "tiles"), sampled(10, 3, "tiles"), bodies("B", 4), forces(6, "tiles"),
        clear(), forces_refused(3), run(5, "tiles"),
    ]),
    "lone_256_tilings_and_engines": (_p2, None, [
        bodies("walls+rest", 2), opt("regtile", 84), forces(5, "tiles"), opt("regtile", 162), forces(5, "tiles"),
        opt("regtile_async", 0), sampled(8, 8, "tiles"), opt("time_block", 8), run(17, "wave"), forces(4, "wave"),
        opt("time_block", 4), opt("march_kernel", 0), sampled(9, 4, "march"), opt("engine", 3), run(9, "tiles"),
        opt("regtile", 84), forces(3, "tiles"),
    ]),
    "capacities_128x16": (_p3, None, [
        run(3, "tiles"), bodies("random4", 4), forces(20, "tiles"), run(1100, "tiles"), forces(300, "tiles"),
        sampled(40, 1, "tiles"), run(2, "tiles"),
    ]),
    "slabs_p2p_tiles_tag_restart": (_p4, ("slabs", 4, "p2p"), [
        bodies("walls+rest", 2), run(5, "slab-tiles"), forces(12, "slab-tiles"), sampled(9, 4, "slab-tiles"),
        opt("regtile_tag", SLAB_TAG_MARK - 10), forces(20, "slab-tiles"), run(7, "slab-tiles"), sampled(5, 5, "slab-tiles"),
    ]),
    "slabs_copy_streaming": (_p5, ("slabs", 2, "copy"), [
        opt("time_block", 2), bodies("random3", 3), run(6, "tb2"), sampled(7, 3, "tb2"), forces(5, "tb2"),
        opt("time_block", 4), run(9, "march"), sampled(8, 4, "march"), forces(3, "march"),
        opt("time_block", 8), run(9, "tb2"),           # slabs of 16 rows are too short for eight steps per pass
        opt("engine", 3), run(5, "slab-tiles"),
    ]),
    "rank_ring_of_one_p2p": (_p6, ("rank", "p2p"), [
        bodies("walls+rest", 2), run(9, "slab-tiles"), forces(6, "slab-tiles"), sampled(8, 4, "slab-tiles"),
        run(3, "slab-tiles"),
    ]),
    "rank_ring_of_one_rccl": (_p6, ("rank", "rccl"), [
        opt("time_block", 2), bodies("walls+rest", 2), run(9, "tb2"), forces(6, "tb2"), sampled(8, 4, "tb2"), run(3, "tb2"),
    ]),
    "never_tiles_130x37": (_p7, None, [
        opt("time_block", 1), bodies("random4", 4), run(5, "tb1"), forces(4, "tb1"), sampled(7, 3, "tb1"),
        opt("time_block", 2), bodies("random2", 2), forces(5, "tb2"), run(7, "tb2"), sampled(6, 4, "tb2"),
        opt("time_block", 6), bodies("core", 1), forces(4, "wave"), run(13, "wave"), sampled(12, 6, "wave"),
        clear(), forces_refused(2), run(2, "wave"),
    ]),
    "lone_tag_wrap_flavoured": (_p8, None, [
        opt("regtile", 44), run(5, "tiles"), bodies("random4", 4), forces(6, "tiles"),
        opt("regtile_tag", TAG_WRAP - 30), sampled(12, 4, "tiles"), forces(20, "tiles"),
        opt("regtile_tag", TAG_WRAP - 5), sampled(9, 3, "tiles"), run(4, "tiles"),
    ]),
    "refusal_point_mixed": (_p9, None, [
        bodies("blocked", 1), run(6, "tiles"), sampled(6, 2, "tiles"), forces(5, "tiles"),
        opt("time_block", 4), opt("march_kernel", 0), run(9, "march"), forces(4, "march"),
        opt("time_block", 8), opt("march_kernel", 1), sampled(10, 5, "wave"), opt("engine", 3), run(4, "tiles"),
    ]),
}
REFUSING = {"refusal_point_mixed"}
# where the guard refuses cells, float and double runs part once a refusal flips on rounding (after ~20 steps here): the
# oracle anchor there covers the first two calls, inside which the guard already refuses
ANCHOR_OVERRIDE = {"refusal_point_mixed": 12}
TILE_PATHS = ("tiles", "slab-tiles")
KIND_OF = {"run": "plain", "sampled": "sampled", "forces": "forces"}


# ---------------------------------------------------------------------------------------------------------------- model
def _kept(ob, body):
    """Blocked labelled cells with a fluid source: the cells lbm_set_bodies keeps."""
    blocked = ob != 0
    src = np.zeros(ob.shape, dtype=bool)
    for i in range(1, 9):
        src |= np.roll(~blocked, shift=(CY[i], CX[i]), axis=(0, 1))
    return blocked & (body > 0) & src


def _force_slots(ob, body, ty, nslabs):
    """Per slab: tiles (64 columns x ty rows) that hold a kept cell -- the register tiles' force slots."""
    ny = ob.shape[0]
    k = _kept(ob, body)
    out = []
    for s in range(nslabs):
        ks = k[s * ny // nslabs:(s + 1) * ny // nslabs]
        ys, xs = np.nonzero(ks)
        out.append(len(set(zip((ys // ty).tolist(), (xs // 64).tolist()))))
    return out


def _grow(cap, need):
    cap = max(1024, cap)
    while cap < need:
        cap *= 2
    return cap


class Model:
    """What the host keeps across calls, restated: tiling, mailbox tag, capacities, bodies; and what the calls crossed."""

    def __init__(self, L, p, ob, labellings, ctx):
        self.p, self.ob, self.labellings = p, ob, labellings
        self.lone = ctx is None
        self.nslabs = ctx[1] if ctx is not None and ctx[0] == "slabs" else 1
        if self.lone:
            t = L.plan_tiles(p.nx, p.ny)
        else:
            t = L.plan_tiles(p.nx, p.ny // self.nslabs, slabs_per_device=self.nslabs)
        self.ty, self.r = t if t is not None else (0, 0)
        self.async_ = 1
        self.rtag = 1
        self.sums_cap = _grow(0, max(p.maxIters, 1))
        self.rpart_cap = 0
        self.fpart_cap = [0] * self.nslabs
        self.body, self.nb, self.label_name = None, 0, None
        self.events = set()
        self.pairs = set()
        self.history = []            # (kind, family, ty) of every call that ran
        self.last_forces = None      # (label name, nb, family, ty)

    def _need_sums(self, need):
        if need > self.sums_cap:
            self.events.add("capacity: step sums")
            self.sums_cap = _grow(self.sums_cap, need)

    def label(self, path):
        """Coverage labels of a call on `path` in the current state."""
        if path == "tiles":
            out = [f"tiles R{self.r}"]
            if self.r > 1:
                out.append(f"tiles async{self.async_}")
            return out
        return [path]

    def apply(self, call):
        """Advances the model over `call`; returns the expected mailbox tag after it."""
        op = call[0]
        if op == "opt":
            _, key, v = call
            if key == "regtile":
                self.ty, self.r, self.rpart_cap = v // 10, v % 10, 0
            elif key == "regtile_async":
                self.async_ = v
            elif key == "regtile_tag":
                self.rtag = v
            return self.rtag
        if op == "bodies":
            _, name, nb = call
            if nb == 0:
                self.events.add("clear")
                self.body, self.nb, self.label_name = None, 0, None
            else:
                self.body, self.nb, self.label_name = self.labellings[name], nb, name
                if not _kept(self.ob, self.body).any():
                    self.events.add("labelling without a fluid source")
            return self.rtag
        if op == "forces_refused":
            if self.nb == 0 and "clear" in self.events:
                self.events.add("forces refused after a clear")
            return self.rtag
        kind = KIND_OF[op]
        n, path = call[1], call[-1]
        tiles = path in TILE_PATHS
        for lab in self.label(path):
            self.pairs.add((lab, kind))
        if kind == "forces":
            self._need_sums(n + 1 + 2 * self.nb * n)
            fam = "tiles" if tiles else "streaming"
            if self.last_forces is not None:
                name0, nb0, fam0, ty0 = self.last_forces
                if name0 != self.label_name:
                    self.events.add("relabel, same nb" if nb0 == self.nb else "relabel, different nb")
                if fam0 != fam:
                    self.events.add("forces on one engine, then another")
                if tiles and fam0 == "tiles" and ty0 != self.ty:
                    self.events.add("tiling change between force runs")
            self.last_forces = (self.label_name, self.nb, fam, self.ty)
            if tiles:
                for s, slots in enumerate(_force_slots(self.ob, self.body, self.ty, self.nslabs)):
                    need = n * slots * 8
                    if need > self.fpart_cap[s]:
                        if self.fpart_cap[s] > 0:
                            self.events.add("capacity: force partials")
                        self.fpart_cap[s] = need
        if tiles:
            if n > self.rpart_cap:
                if self.rpart_cap > 0:
                    self.events.add("capacity: per-step tile sums")
                self.rpart_cap = _grow(self.rpart_cap, n)
            self._need_sums(n + 1)
            if self.lone and self.rtag + n >= TAG_WRAP:      # cleared in front of the run
                self.rtag = 1
                if kind != "plain":
                    self.events.add("lone tag restart in a flavoured run")
            restart = not self.lone and self.rtag + n >= SLAB_TAG_MARK
            self.rtag += n + 1
            if restart:                                      # cleared behind the run
                self.rtag = 1
                if kind != "plain":
                    self.events.add("slab tag restart in a flavoured run")
            fams = [h[1] for h in self.history]
            if "streaming" in fams and "tiles" in fams[:fams.index("streaming")]:
                self.events.add("tiles, streaming, tiles")
        elif kind == "sampled":
            self._need_sums(call[2])
        elif kind == "plain":
            self._need_sums(n)
        self.history.append((kind, "tiles" if tiles else "streaming", self.ty))
        return self.rtag


def _walk(L, name):
    setup, ctx, calls = PROGRAMS[name]
    p, ob, cells, labellings = setup(L)
    m = Model(L, p, ob, labellings, ctx)
    tags = [m.apply(c) for c in calls]
    return m, tags


# ---------------------------------------------------------------------------------------------------------------- no GPU
COVERAGE_PATHS = ("tiles R1", "tiles R2", "tiles R4", "tiles async0", "tiles async1", "slab-tiles", "tb1", "tb2", "march",
                  "wave")
COVERAGE_TRANSITIONS = (
    "relabel, same nb", "relabel, different nb", "clear", "forces refused after a clear", "labelling without a fluid source",
    "tiling change between force runs", "forces on one engine, then another", "tiles, streaming, tiles",
    "capacity: per-step tile sums", "capacity: step sums", "capacity: force partials",
    "lone tag restart in a flavoured run", "slab tag restart in a flavoured run",
)


COVERAGE_CONTEXTS = ("lone", "slabs p2p", "slabs copy", "rank p2p", "rank rccl")


def test_program_table_covers_every_path_and_transition(L):
    pairs, events, contexts, refusing = set(), set(), set(), False
    for name, (_, ctx, calls) in PROGRAMS.items():
        assert 5 <= len(calls) <= 20, name
        m, _ = _walk(L, name)
        pairs |= m.pairs
        events |= m.events
        contexts.add("lone" if ctx is None else " ".join(str(v) for v in (ctx[0], ctx[-1])))
        point = tuple(np.float32(v) for v in (m.p.density, m.p.accel, m.p.omega))
        if point == tuple(np.float32(v) for v in PARAM_GRID["refusal"]):
            refusing = refusing or {k for _, k in m.pairs} == {"plain", "sampled", "forces"}
        for c in calls:                                      # every running call declares a path the runner knows
            if c[0] in KIND_OF:
                assert c[-1] in TILE_PATHS + ("tb1", "tb2", "march", "wave"), (name, c)
                assert (c[-1] == "slab-tiles") == (ctx is not None and c[-1] in TILE_PATHS), (name, c)
    missing = [(lab, kind) for lab in COVERAGE_PATHS for kind in ("plain", "sampled", "forces") if (lab, kind) not in pairs]
    assert not missing, missing
    assert not [t for t in COVERAGE_TRANSITIONS if t not in events], [t for t in COVERAGE_TRANSITIONS if t not in events]
    assert set(COVERAGE_CONTEXTS) <= contexts, contexts
    assert refusing, "no program mixes the three run kinds where the accelerate guard refuses cells"


def test_model_restates_the_tag_and_capacity_rules(L):
    """The model's own arithmetic on the programs that cross the marks (so a wrong model cannot pass the GPU test vacuously)."""
    m, tags = _walk(L, "lone_tag_wrap_flavoured")
    assert tags[6] == 1 + 21 and tags[-1] == 1 + 10 + 5          # both flavoured runs that reach the mark start over
    assert "lone tag restart in a flavoured run" in m.events
    m, tags = _walk(L, "slabs_p2p_tiles_tag_restart")
    assert tags[5] == 1 and tags[-1] == 1 + 8 + 6
    m, _ = _walk(L, "capacities_128x16")
    assert m.rpart_cap == 2048 and m.sums_cap == 4096
    assert {"capacity: per-step tile sums", "capacity: step sums", "capacity: force partials"} <= m.events


# ---------------------------------------------------------------------------------------------------------------- GPU
class Shadow:
    """The one-step kernel on its own context; keeps its av_vels and its state at the anchor step."""

    def __init__(self, L, p, ob, cells, anchor):
        self.lat = L.Lattice(p, ob, cells)
        self.lat.set_option("time_block", 1)
        assert self.lat.info("engine") == 1 and self.lat.info("time_block_active") == 1
        self.ob, self.anchor, self.done, self.av, self.at_anchor = ob, anchor, 0, [], None

    def run(self, n):
        out = []
        if self.done < self.anchor < self.done + n:           # (splitting a one-step run changes no bit)
            k = self.anchor - self.done
            out.append(self.lat.run(k))
            self.done += k
            n -= k
            self.at_anchor = self.lat.read_state()
        out.append(self.lat.run(n))
        self.done += n
        if self.done == self.anchor and self.at_anchor is None:
            self.at_anchor = self.lat.read_state()
        assert self.lat.info("engine_last") == 1
        av = np.concatenate(out)
        self.av.append(av)
        return av

    def forces(self, n, body, nb):
        av, F, S = [], [], []
        for _ in range(n):
            av.append(self.run(1))
            f, a = forces_from_state(self.lat.read_state(), self.ob, body, nb)
            F.append(f)
            S.append(a)
        return np.concatenate(av), np.array(F).reshape(n, nb, 2), np.array(S).reshape(n, nb, 2)

    def sampled(self, n, every):
        av, snaps, done = [], [], 0
        while done + every <= n:
            av.append(self.run(every))
            snaps.append(self.lat.final_state())
            done += every
        if done < n:
            av.append(self.run(n - done))
        return np.concatenate(av), np.stack(snaps)


def _check_path(lat, call, model):
    kind, path = KIND_OF[call[0]], call[-1]
    info = {k: lat.info(k) for k in ("engine_last", "samples_in_kernel", "forces_in_kernel", "time_block_active", "march_kernel",
                                     "regtile", "regtile_async", "regtile_tag")}
    where = (call, info)
    if path in TILE_PATHS:
        assert info["engine_last"] == 3, where
        assert info["regtile"] == model.ty * 10 + model.r, where
        if path == "tiles":
            assert info["regtile_async"] == model.async_, where
    else:
        assert info["engine_last"] == 1, where
        k = {"tb1": 1, "tb2": 2, "march": 4}.get(path, lat.info("time_block"))
        assert info["time_block_active"] == k, where
        if path in ("march", "wave") or model.lone:     # (slabs report the kernel their K would march with, marching or not)
            assert info["march_kernel"] == (1 if path == "wave" else 0), where
    if kind == "sampled":
        assert info["samples_in_kernel"] == (1 if path in TILE_PATHS else 0), where
    if kind == "forces":
        assert info["forces_in_kernel"] == (1 if path in TILE_PATHS else 0), where


def _check_derived(lat, st, oracle, op, ob):
    """total_density: the library sums each cell's nine populations in float (in order, as lbm_final_state's pressure) and
    the cells in double -- restated here to 1e-12; against the float64 sum of the populations the per-cell float rounding
    allows 8 x 2^-24 relative.  av_velocity / reynolds: the oracle's on the same state, as on a resident state elsewhere."""
    mass = lat.total_density()
    f = st.astype(np.float32)
    rho = f[..., 0].copy()
    for k in range(1, 9):
        rho = rho + f[..., k]
    want32, want64 = float(rho.astype(np.float64).sum()), float(st.astype(np.float64).sum())
    assert abs(mass - want32) <= 1e-12 * abs(want32), (mass, want32)
    assert abs(mass - want64) <= 8 * 2.0 ** -24 * abs(want64), (mass, want64)
    # the oracle adds the cells' speeds serially in float, the library per block in float and the blocks in double: 1e-5
    # covers the order difference on 65536 cells (the resident-state test), in proportion beyond; the same per-cell float
    # operations summed in double (restated here) hold to 2e-6
    avv, re = lat.av_velocity(), lat.reynolds()
    bar = 1e-5 * max(1.0, st.shape[0] * st.shape[1] / 65536)
    assert abs(avv - oracle.av_velocity(op, st, ob)) <= bar * avv
    assert abs(re - oracle.reynolds(op, st, ob)) <= bar * re
    ux = (f[..., 1] + f[..., 5] + f[..., 8] - (f[..., 3] + f[..., 6] + f[..., 7])) / rho
    uy = (f[..., 2] + f[..., 5] + f[..., 6] - (f[..., 4] + f[..., 7] + f[..., 8])) / rho
    fluid = ob.reshape(rho.shape) == 0
    sp = np.sqrt(ux * ux + uy * uy, dtype=np.float32)[fluid]
    assert abs(avv - float(sp.astype(np.float64).sum() / fluid.sum())) <= 2e-6 * avv


def _open(L, p, ob, cells, ctx):
    if ctx is None:
        return L.Lattice(p, ob, cells)
    if ctx[0] == "slabs":
        ex = L.EXCHANGE_P2P if ctx[2] == "p2p" else L.EXCHANGE_COPY
        return L.Lattice(p, ob, cells, nslabs=ctx[1], devices=[0] * ctx[1], exchange=ex)
    ex = L.EXCHANGE_P2P if ctx[1] == "p2p" else L.EXCHANGE_RCCL
    return L.Lattice(p, ob, cells, rank=0, nranks=1, device=0, unique_id=L.rccl_unique_id(), exchange=ex)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_call_sequence(gpu, O, oracle, monkeypatch, name):
    L = gpu
    lib = L.load_library()
    setup, ctx, calls = PROGRAMS[name]
    p, ob, cells0, labellings = setup(L)
    model = Model(L, p, ob, labellings, ctx)
    op = O.OrcParam(p.nx, p.ny, p.maxIters, p.reynolds_dim, p.density, p.accel, p.omega)
    total = sum(c[1] for c in calls if c[0] in KIND_OF)
    anchor = min(ANCHOR_OVERRIDE.get(name, ANCHOR_STEPS), total)
    sh = Shadow(L, p, ob, cells0, anchor)
    try:
        if ctx is not None and ctx[0] == "rank":
            monkeypatch.setenv("LBM_FORCE_EXCHANGE", "1")
        with _open(L, p, ob, cells0, ctx) as lat:
            prev_kind, derived_checks = None, 0
            for call in calls:
                op_ = call[0]
                st0 = lat.read_state() if op_ == "forces_refused" else None
                if op_ == "opt":
                    lat.set_option(call[1], call[2])
                elif op_ == "bodies":
                    lat.set_bodies(labellings[call[1]] if call[1] else None, call[2])
                elif op_ == "forces_refused":
                    n = call[1]
                    buf = np.full((n, MAX_BODIES, 2), np.nan, dtype=np.float32)     # room for any nb
                    assert lib.lbm_run_forces(lat._ctx, n, None, buf.ctypes.data) == LBM_EINVAL, call
                    assert np.array_equal(_bits(lat.read_state()), _bits(st0)), call
                elif op_ == "run":
                    av = lat.run(call[1])
                    av_sh = sh.run(call[1])
                elif op_ == "sampled":
                    av, fields = lat.run_sampled(call[1], call[2])
                    av_sh, want = sh.sampled(call[1], call[2])
                    assert np.array_equal(_bits(fields), _bits(want)), call
                elif op_ == "forces":
                    av, F = lat.run_forces(call[1])
                    av_sh, want, scale = sh.forces(call[1], model.body, model.nb)
                    assert F.shape == want.shape and _close(F, want, scale), (call, np.abs(F - want).max())
                    if not _kept(ob, model.body).any():
                        assert np.all(F == 0) and np.all(want == 0), call
                tag = model.apply(call)
                assert lat.info("regtile_tag") == tag, (call, lat.info("regtile_tag"), tag)
                st = lat.read_state()
                assert np.array_equal(_bits(st), _bits(sh.lat.read_state())), call
                if op_ not in KIND_OF:
                    continue
                _check_path(lat, call, model)
                assert np.allclose(av, av_sh, rtol=2e-6, atol=0), call
                if ctx is None and (call[-1] == "tb1" or (op_ == "forces" and call[-1] not in TILE_PATHS)):
                    assert np.array_equal(_bits(av), _bits(av_sh)), call       # the same one-step kernel ran
                if prev_kind is not None and op_ != prev_kind:
                    _check_derived(lat, st, oracle, op, ob)
                    derived_checks += 1
                prev_kind = op_
            assert derived_checks >= 1
        # the shadow against the strict float oracle over the first steps
        ref = cells0.copy()
        av_o, refusals = [], 0
        for _ in range(anchor):
            refusals += int(refused(p.density, p.accel, ob, ref).sum())
            av_o.append(oracle.run(op, ref, ob, 1)[0])
        st_a = sh.at_anchor
        assert st_a is not None
        assert np.all(np.abs(st_a - ref) <= 2e-5 * np.abs(ref) + 2e-6 * np.abs(ref).max())
        assert np.allclose(np.concatenate(sh.av)[:anchor], np.array(av_o), rtol=1e-4, atol=0)
        if name in REFUSING:
            assert refusals > 0                   # the guard refused cells inside the sequence
    finally:
        sh.lat.close()
