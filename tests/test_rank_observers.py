"""The observer calls on rank contexts of SEVERAL ranks: every lbm_run_* call held to its rank-local convention
(include/lbm_mi355x.h) on ranks whose first row is not row 0.

  probes, windows      the coordinates are global on every rank; a rank fills what lies in its own lattice rows and writes
                       +0.0f to the rest
  means, stats,        the rows of lbm_final_state: the rank's own
  snapshots
  forces               without a communicator, the rank's own contribution; the caller adds them
  driven runs          every rank passes the same schedule

The ranks are processes sharing one GPU, started as tests/test_live_inputs.py::_rank_worker and
tests/test_gpu_parity.py::_regtile_rank_worker start theirs: peer-to-peer halos, the handles through the parent's pipes, no
communicator.  One spawn per case: a worker runs the case's LIST of calls on one context, each from a fresh write_state of
the initial cells, between two barriers of the parent's (every rank's run has returned before any rank writes; every rank
has written before any rank runs), and saves every output.  Every output array is the worker's, filled with the bit pattern
SENTINEL before the call -- host arrays through Lattice._output, device tensors through the wrapper's out= -- so a +0.0f
in a row the rank does not own is something the library wrote.

Every case is held to two references:
  1. the strict float oracle on the CPU, stepped from the same cells: the fields of _oracle_fields with its derived bound
     (tests/test_mean_run.py), means and stats through mean_of / stats_of on those fields in float32 with the bar
     _oracle_mean_bound states for a float sum of m terms, forces through forces_from_state in float64 with _close of
     tests/test_body_forces.py -- per rank against the blocked cells of the rank's rows, and summed against the whole;
  2. the undivided context (one process, one slab, time_block 1) given the same calls: every field output, assembled from
     the ranks, and the lattice are its BITS; av_vels, summed over the ranks in double, to rtol 2e-6.

Cases: A the 33 x 20 known-answer lattice on 3 ranks (rows 6, 7, 7; the streaming one-step kernel), B the 16 x 12 one on 2
ranks with every probe in rank 0 and a window wholly in rank 1, C the two shapes of
test_register_tiles_between_processes on the register tiles (kernels of different processes are not promised to run at
once on one GPU: a piece that gives up falls back, which is reported, not asserted), R the refusals.

NOT covered here: ranks_agree's all-reduce between several ranks.  Two processes on one GPU cannot form a RCCL communicator
(LBM_REGTILE_SLABS_NO_AGREEMENT stands in for it), so agreeing on a path and failing together across ranks needs one GPU
per rank and stays untested."""
import functools
import os
import sys
import types
import warnings

import numpy as np
import pytest

from conftest import ROOT, load_kat
from test_body_forces import _close, forces_from_state
from test_gpu_parity import _random_case
from test_mean_run import _oracle_fields, mean_of
from test_stats_run import p0_of, stats_of

NSTEPS = 12
NBODIES = 4
SENTINEL = 0x7fc0dead                   # a quiet NaN with a payload: neither +0.0f nor anything a kernel computes
STREAMING = (("engine", 1), ("time_block", 1))      # every rank on the one-step kernel by construction
# name -> (the lattice: a known-answer file or the shape of _random_case(.., 13); ranks; options of every rank)
CASES = {"A": ("kat_33x20", 3, STREAMING), "B": ("kat_16x12", 2, STREAMING), "R": ("kat_16x12", 2, STREAMING),
         "C2": ((256, 64), 2, ()), "C3": ((128, 96), 3, ())}
# blocked cells (x, y) added to the test's own copy of a known-answer map, for the bodies below
EXTRA = {"kat_33x20": ((10, 0),), "kat_16x12": ((7, 11), (4, 5), (10, 6))}
WINDOWS = ("whole", "straddle", "skip", "strided", "one", "in_last")
# the info key that says a call of case C ran inside the register tiles
IN_KERNEL = {"forces": "forces_in_kernel", "probes": "probes_in_kernel", "sampled": "samples_in_kernel", "mean": "mean_in_kernel",
             "wstats": "window_stats_in_kernel", "driven_observed": "driven_observed_in_kernel"}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the cases
def rank_bounds(ny, nranks):
    return [r * ny // nranks for r in range(nranks + 1)]


def make_bodies(ob, bounds):
    """Labels 1..4: 1 the blocked cells of the two rows either side of every rank boundary, 2 those of rows 0 and ny - 1 (the
    periodic closure between the last rank and rank 0), 3 those strictly inside the middle rank, 4 on fluid cells alone."""
    ny, nx = ob.shape
    body = np.zeros((ny, nx), np.int32)
    mid = (len(bounds) - 1) // 2
    body[bounds[mid] + 1:bounds[mid + 1] - 1] = 3
    for b in bounds[1:-1]:
        body[b - 1:b + 1] = 1
    body[0] = body[ny - 1] = 2
    body[ob == 0] = 0
    ys, xs = np.nonzero(ob[1:ny - 1] == 0)
    body[ys[::7] + 1, xs[::7]] = 4      # (labels on fluid cells are ignored)
    return body


def links_across(ob, body, label, row, to):
    """(straight, diagonal): has a blocked cell of `label` on lattice row `row` a fluid neighbour on row `to`, straight
    above or below it / diagonally (columns wrap)."""
    ny, nx = ob.shape
    xs = np.nonzero((ob[row % ny] != 0) & (body[row % ny] == label))[0]
    fluid = ob[to % ny] == 0
    return bool(fluid[xs].any()), bool((fluid[(xs - 1) % nx] | fluid[(xs + 1) % nx]).any())


def probe_set(ob, bounds, ranks):
    """Six probes in the rows of each rank of `ranks` -- column 0 of its first row, column nx - 1 of its last, one more on
    either row, two blocked cells -- in an order that is not the rows'."""
    ny, nx = ob.shape
    per = []
    for r in ranks:
        r0, r1 = bounds[r], bounds[r + 1]
        cells = [(0, r0), (nx - 1, r1 - 1), (nx // 2, r0), (1, r1 - 1)]
        ys, xs = np.nonzero(ob[r0:r1])
        blocked = [(int(x), int(y) + r0) for x, y in zip(xs, ys) if (int(x), int(y) + r0) not in cells]
        per.append(cells + [blocked[0], blocked[-1]])
    return np.array([per[i][j] for j in range(6) for i in reversed(range(len(per)))], dtype=np.int32)


def window_set(nx, ny, bounds):
    """name -> (x0, y0, nx, ny, sx, sy): the whole lattice; rows that straddle every rank boundary; rows of which one rank
    holds none (sy steps over it); sx = 3 from x0 = 1; one cell on the last rank's first row; a window wholly inside the last
    rank."""
    lo, hi = bounds[1], bounds[-2]
    skip = (0, lo - 1, nx, 2, 1, bounds[2] - lo + 1) if len(bounds) > 3 else (0, 1, nx, lo // 2, 1, 2)
    return {"whole": (0, 0, nx, ny, 1, 1), "straddle": (2, lo - 2, min(10, nx - 2), hi - lo + 4, 1, 1), "skip": skip,
            "strided": (1, 0, (nx - 2) // 3 + 1, (ny + 1) // 2, 3, 2), "one": (7, hi, 1, 1, 1, 1),
            "in_last": (1, hi + 1, 5, bounds[-1] - hi - 2, 3, 1)}


def window_cells(w):
    x0, y0, wnx, wny, sx, sy = w
    return y0 + sy * np.arange(wny), x0 + sx * np.arange(wnx)


def _with_device_variants(calls, which):
    return [c + (False,) for c in calls] + [c + (True,) for c in calls if c[0] in which or c[:2] in which]


def call_list(name):
    """(kind, argument, output in device memory) of every call of a case, in order."""
    if name == "R":
        return [("refuse_bodies", None, False), ("refuse_probe", None, False), ("probes", 1, False), ("forces", None, False)]
    if name in ("A", "B"):
        calls = [("forces", None), ("probes", 1), ("probes", 5), ("sampled", 4), ("mean", 3), ("stats", 3)]
        calls += [("window", (4, w)) for w in WINDOWS] + [("wstats", (3, w, 0)) for w in WINDOWS]
        calls += [("observed", (True, 2, 3, 4)), ("driven", None), ("driven_observed", (True, 2, 3, 0))]
        dev = {("probes", 5), "sampled", "mean", "stats", ("window", (4, "straddle")), ("window", (4, "skip")),
               ("wstats", (3, "straddle", 0)), ("wstats", (3, "skip", 0)), "observed", "driven_observed"}
        return _with_device_variants(calls, dev)
    calls = [("forces", None), ("probes", 3), ("mean", 6), ("sampled", 6), ("wstats", (4, "straddle", 2)), ("wstats", (4, "skip", 2)),
             ("driven_observed", (True, 6, 6, 0))]
    return _with_device_variants(calls, {"probes", "mean", "sampled"})


def periods(call):
    """output name -> its sample period, of the field outputs of a call"""
    kind, arg = call[:2]
    if kind in ("observed", "driven_observed"):
        return {k: e for k, e in zip(("probes", "mean", "fields"), arg[1:]) if e}
    one = {"probes": "probes", "sampled": "fields", "mean": "mean", "stats": "stats", "window": "window", "wstats": "wstats"}
    return {one[kind]: arg if isinstance(arg, int) else arg[0]} if kind in one else {}


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything a rank, the undivided context and the oracle need of a case, made the same way in every process."""
    import advanced_hpc_lbm_amd as L
    src, nranks, options = CASES[name]
    if isinstance(src, str):
        k = load_kat(src)
        nx, ny = int(k["nx"]), int(k["ny"])
        prm = (nx, ny, NSTEPS, int(k["reynolds_dim"]), float(k["density"]), float(k["accel"]), float(k["omega"]))
        ob = np.array(k["obstacles"], dtype=np.int32).reshape(ny, nx)
        for x, y in EXTRA[src]:
            assert ob[y, x] == 0
            ob[y, x] = 1
        cells0 = np.ascontiguousarray(k["cells0"], dtype=np.float32).reshape(ny, nx, 9)
    else:
        p, ob, cells0 = _random_case(L, src[0], src[1], 13)
        nx, ny = src
        prm = (nx, ny, NSTEPS, p.reynolds_dim, p.density, p.accel, p.omega)
    bounds = rank_bounds(ny, nranks)
    c = types.SimpleNamespace(name=name, nranks=nranks, options=options, prm=prm, nx=nx, ny=ny, ob=np.ascontiguousarray(ob),
                              cells0=cells0, bounds=bounds, body=make_bodies(ob, bounds), windows=window_set(nx, ny, bounds),
                              calls=call_list(name))
    c.xy = probe_set(ob, bounds, range(nranks) if name in ("A", "C2", "C3") else [0])
    c.sched = (np.float32(prm[5]) * np.linspace(1.5, -1.0, NSTEPS)).astype(np.float32)      # a ramp that changes sign
    ys, xs = np.nonzero(ob[bounds[1] + 1:bounds[2]])
    c.bad_cell = (int(xs[0]), int(ys[0]) + bounds[1] + 1)                                   # a blocked cell of rank 1's rows
    return c


# ---------------------------------------------------------------------------------------------------------------- assembly
def owner_of_rows(rows, bounds):
    """the rank that owns each lattice row of `rows`"""
    return np.searchsorted(np.asarray(bounds), np.asarray(rows), side="right") - 1


def window_row_owner(L, w, nx, ny, bounds):
    """the rank that owns each window row, from lbm_window_rows (first, count) per rank"""
    owner = np.full(w[3], -1)
    for r in range(len(bounds) - 1):
        first, count = L.window_rows(L.Window(*w), nx, ny, bounds[r], bounds[r + 1])
        assert np.all(owner[first:first + count] == -1)
        owner[first:first + count] = r
    assert np.all(owner >= 0)
    return owner


def assemble(parts, owner, axis):
    """Entry i along `axis` from parts[owner[i]] (probes, windows): selected, not added -- a sum would turn -0.0f into +0.0f."""
    out = np.empty_like(parts[0])
    assert all(p.shape == out.shape for p in parts) and out.shape[axis] == len(owner)
    idx = [slice(None)] * out.ndim
    for i, r in enumerate(owner):
        idx[axis] = i
        out[tuple(idx)] = parts[r][tuple(idx)]
    return out


def foreign_is_plus_zero(parts, owner, axis):
    """Every entry along `axis` that rank r does not own has the bits 0x00000000 in parts[r] (not -0.0f, not the sentinel)."""
    for r, p in enumerate(parts):
        foreign = np.take(_bits(p), np.nonzero(np.asarray(owner) != r)[0], axis=axis)
        if foreign.any():
            return False
    return True


def sentinel_survives(a):
    return bool((_bits(a) == SENTINEL).any())


# ---------------------------------------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def oracle_steps(name, driven):
    """The strict float oracle's lattice after each of the NSTEPS steps from the case's cells (driven: under its schedule)."""
    import lbm_oracle as O
    c = case(name)
    orc = O.Oracle("strict")
    ref, out = c.cells0.copy(), []
    for t in range(NSTEPS):
        accel = float(c.sched[t]) if driven else c.prm[5]
        orc.run(O.OrcParam(c.nx, c.ny, 1, c.prm[3], c.prm[4], accel, c.prm[6]), ref, c.ob, 1)
        out.append(ref.copy())
    return out


@functools.lru_cache(maxsize=None)
def oracle_fields(name, driven):
    c = case(name)
    return [_oracle_fields(s, c.ob, c.prm[4]) for s in oracle_steps(name, driven)]


def sample_steps(every):
    return [j * every - 1 for j in range(1, NSTEPS // every + 1)]


def fields_bound(name, driven, every, rows=None, cols=None):
    """(want, tol)[m, rows, cols, 4] of _oracle_fields at the sample steps, of the whole lattice or of the cells rows x cols"""
    F = oracle_fields(name, driven)
    sel = (slice(None), slice(None)) if rows is None else np.ix_(rows, cols)
    return np.stack([F[t][0][sel] for t in sample_steps(every)]), np.stack([F[t][1][sel] for t in sample_steps(every)])


def mean_bound(want, tol):
    """(reference, bound) of a mean over the samples want[m, ...]: mean_of on the oracle's fields in float32, and the bar of
    tests/test_mean_run.py::_oracle_mean_bound -- the mean of the per-step bounds + m 2^-24 mean|want_j| (a float sum of m
    terms) + 2^-24 |mean| (the division)."""
    m = len(want)
    ref = mean_of(want.astype(np.float32)).astype(np.float64)
    return ref, tol.mean(axis=0) + m * 2.0 ** -24 * np.abs(want).mean(axis=0) + 2.0 ** -24 * np.abs(ref)


def moment_bound(want, tol, density):
    """(reference, bound) of floats 4..7 of the stats: stats_of on the oracle's fields in float32, and the bound of
    tests/test_stats_run.py::_oracle_moment_bound -- the per-element bounds dx of _oracle_fields carried through each
    product, |x| dy + |y| dx + dx dy, averaged over the samples, + m 2^-24 mean|Q_j| + 2^-24 |result|.  A blocked cell's
    fields are constants: the same float operations on either side."""
    m = len(want)
    p0 = p0_of(density)
    ref = stats_of(want.astype(np.float32), p0)[..., 4:].astype(np.float64)
    x, y, d = want[..., 0], want[..., 1], want[..., 3] - float(p0)
    dx, dy, dd = tol[..., 0], tol[..., 1], tol[..., 3]
    q = np.stack([x * x, y * y, x * y, d * d], axis=-1)
    e = np.stack([2 * np.abs(x) * dx + dx * dx, 2 * np.abs(y) * dy + dy * dy, np.abs(x) * dy + np.abs(y) * dx + dx * dy,
                  2 * np.abs(d) * dd + dd * dd], axis=-1)
    return ref, e.mean(axis=0) + m * 2.0 ** -24 * np.abs(q).mean(axis=0) + 2.0 ** -24 * np.abs(ref)


def _inside(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    lim = bound + 2.0 ** -24 * np.abs(got.astype(np.float64))
    print("%s: max error %.3g, worst error / bound %.3g" % (what, err.max(), np.max(err / np.where(lim > 0, lim, 1.0), initial=0.0)))
    assert np.all(err <= lim), (what, float(np.max(err - lim)))


# ---------------------------------------------------------------------------------------------------------------- the calls
def run_call(L, lat, c, call, out_for=None):
    """One call of a case on `lat`, NSTEPS steps: its outputs by name, as numpy arrays.  out_for(shape): the device tensor an
    output goes to (None: host arrays of the wrapper's making)."""
    kind, arg = call[:2]
    n, rows, nx, npb = NSTEPS, lat._local_rows(), c.nx, len(c.xy)

    def dev(shape):
        return out_for(shape) if out_for else None

    def host(a):
        return a if isinstance(a, np.ndarray) else a.cpu().numpy()

    if kind == "forces":
        av, f = lat.run_forces(n)
        return {"av": av, "forces": f}
    if kind == "probes":
        av, o = lat.run_probes(n, arg, out=dev((n // arg, npb, 4)))
        return {"av": av, "probes": host(o)}
    if kind == "sampled":
        av, o = lat.run_sampled(n, arg, out=dev((n // arg, rows, nx, 4)))
        return {"av": av, "fields": host(o)}
    if kind == "mean":
        av, o = lat.run_mean(n, arg, out=dev((rows, nx, 4)))
        return {"av": av, "mean": host(o)}
    if kind == "stats":
        av, o = lat.run_stats(n, arg, out=dev((rows, nx, 8)))
        return {"av": av, "stats": host(o)}
    if kind == "window":
        w = c.windows[arg[1]]
        av, o = lat.run_window(n, arg[0], L.Window(*w), out=dev((n // arg[0], w[3], w[2], 4)))
        return {"av": av, "window": host(o)}
    if kind == "wstats":
        w = c.windows[arg[1]]
        lat.set_option("window_stats_chunk", arg[2])
        av, o = lat.run_window_stats(n, arg[0], L.Window(*w), out=dev((w[3], w[2], 8)))
        return {"av": av, "wstats": host(o)}
    if kind == "driven":
        return {"av": lat.run_driven(c.sched)}
    assert kind in ("observed", "driven_observed"), kind
    f, pe, me, fe = arg
    kw = dict(forces=f, probes_every=pe, mean_every=me, fields_every=fe, probes_out=dev((n // pe, npb, 4)) if pe else None,
              mean_out=dev((rows, nx, 4)) if me else None, fields_out=dev((n // fe, rows, nx, 4)) if fe else None)
    res = lat.run_observed(n, **kw) if kind == "observed" else lat.run_driven_observed(c.sched, **kw)
    out = {k: host(v) for k, v in res.items()}
    out["av"] = out.pop("av_vels")
    return out


def _refusal(L, lat, c, kind):
    """"accepted", or the library's words for refusing: a label outside [0, NBODIES] on a blocked cell of rank 1's rows; a
    probe outside the lattice behind three legal ones."""
    try:
        if kind == "refuse_bodies":
            bad = c.body.copy()
            bad[c.bad_cell[1], c.bad_cell[0]] = NBODIES + 5
            lat.set_bodies(bad, NBODIES)
        else:
            lat.set_probes(np.concatenate([c.xy[:3], [[c.nx, 0]]]))
    except L.LbmError as e:
        return str(e)
    return "accepted"


def _rank_worker(rank, nranks, name, conn, outdir):
    import traceback
    try:
        for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
            if p_ not in sys.path:
                sys.path.insert(0, p_)
        os.environ["LBM_REGTILE_SLABS_NO_AGREEMENT"] = "1"     # (as tests/test_gpu_parity.py: no communicator on one GPU)
        import torch                                           # (before the library: see load_library)
        import advanced_hpc_lbm_amd as L
        c = case(name)

        def filled(shape):
            a = np.empty(shape, dtype=np.float32)
            a.view(np.uint32)[...] = SENTINEL
            return a

        def out_for(shape):
            return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda:0").view(torch.float32)

        class Lattice(L.Lattice):                              # host outputs that hold the sentinel before the call
            def _output(self, out, shape, what):
                if out is not None:
                    return super()._output(out, shape, what)
                arr = filled(shape)
                return arr, (arr.ctypes.data if arr.size else None)

            def run_forces(self, nsteps):
                av, f = np.empty(nsteps, dtype=np.float32), filled((nsteps, self._nbodies, 2))
                L._check(self._lib.lbm_run_forces(self._ctx, nsteps, av.ctypes.data, f.ctypes.data))
                return av, f

        lat = Lattice(L.Param(*c.prm), c.ob, c.cells0, rank=rank, nranks=nranks, device=0, unique_id=None, exchange=L.EXCHANGE_P2P)
        for k, v in c.options:
            lat.set_option(k, v)
        conn.send(lat.p2p_handle())
        lat.p2p_connect(conn.recv())
        r0, r1 = lat.slab_rows(0)
        lat.set_probes(c.xy)
        lat.set_bodies(c.body, NBODIES)
        out_for((1,)).cpu()                                    # (torch's own start-up, in front of the first barrier)
        notes = {"rows": (r0, r1), "engine_next": int(lat.info("engine_next"))}
        for i, call in enumerate(c.calls):
            conn.send(("idle", i))                             # every rank's last run has returned ...
            conn.recv()
            lat.write_state(c.cells0[r0:r1])
            conn.send(("written", i))                          # ... and every rank has written before any rank runs
            conn.recv()
            if call[0].startswith("refuse"):
                notes[i] = _refusal(L, lat, c, call[0])
                continue
            outs = run_call(L, lat, c, call, out_for if call[2] else None)
            outs["state"] = lat.read_state()
            np.savez(os.path.join(outdir, "%s_%d_%d.npz" % (name, rank, i)), **outs)
            notes[i] = (int(lat.info("engine_last")), int(lat.info(IN_KERNEL[call[0]])) if call[0] in IN_KERNEL else None)
        conn.send(("done", notes))
        conn.recv()          # keep the mappings until every rank has finished
        lat.close()
    except BaseException:
        try:
            conn.send(("error", traceback.format_exc()))
        except Exception:
            pass
        raise


def _spawn(name, outdir):
    """The ranks of a case, one process each; returns their notes."""
    import multiprocessing as mp
    c = case(name)
    n = c.nranks
    ctx = mp.get_context("spawn")
    pipes = [ctx.Pipe() for _ in range(n)]
    procs = [ctx.Process(target=_rank_worker, args=(r, n, name, pipes[r][1], str(outdir))) for r in range(n)]
    for pr in procs:
        pr.start()
    for r in range(n):
        pipes[r][1].close()          # (the rank holds its end: a rank that dies reads as the end of its pipe here)
    try:
        def gather(what):
            msgs = []
            for r in range(n):
                assert pipes[r][0].poll(120), "rank %d: no %s" % (r, what)
                msgs.append(pipes[r][0].recv())
                assert not (isinstance(msgs[-1], tuple) and msgs[-1][0] == "error"), "rank %d at %s:\n%s" % (r, what, msgs[-1][1])
            return msgs

        def release(x):
            for r in range(n):
                pipes[r][0].send(x)

        release(gather("handle"))
        for i, call in enumerate(c.calls):
            assert gather("end of the run before call %d %r" % (i, call)) == [("idle", i)] * n
            release("go")
            assert gather("write_state before call %d %r" % (i, call)) == [("written", i)] * n
            release("go")
        done = gather("end")
        assert all(m[0] == "done" for m in done)
        release("bye")
    finally:
        for r in range(n):
            pipes[r][0].close()      # (a rank still waiting for the parent ends on this, not on the kill below)
        for pr in procs:
            pr.join(60)
            if pr.is_alive():
                pr.kill()
    assert all(pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
    return [m[1] for m in done]


def _undivided(L, c):
    """(kind, argument) -> the outputs of the same calls on one undivided context, time_block 1, host output"""
    out = {}
    with L.Lattice(L.Param(*c.prm), c.ob, c.cells0) as lat:
        lat.set_option("time_block", 1)
        lat.set_probes(c.xy)
        lat.set_bodies(c.body, NBODIES)
        for call in c.calls:
            if call[:2] in out or call[0].startswith("refuse"):
                continue
            lat.write_state(c.cells0)
            o = run_call(L, lat, c, call)
            o["state"] = lat.read_state()
            out[call[:2]] = o
    return out


_RUNS = {}


@pytest.fixture
def ran(gpu, tmp_path_factory):
    """ran(name): the case run once -- one spawn -- and kept for every test of the file; a run that failed fails them all."""
    def get(name):
        if name not in _RUNS:
            c = case(name)
            try:
                d = tmp_path_factory.mktemp("ranks_" + name)
                U = _undivided(gpu, c)
                notes = _spawn(name, d)
                R = [{i: dict(np.load(d / ("%s_%d_%d.npz" % (name, r, i)))) for i, call in enumerate(c.calls) if not call[0].startswith("refuse")}
                     for r in range(c.nranks)]
                _RUNS[name] = types.SimpleNamespace(c=c, U=U, R=R, notes=notes, L=gpu)
            except BaseException as e:
                _RUNS[name] = e
                raise
        if isinstance(_RUNS[name], BaseException):
            pytest.fail("the ranks of case %s did not run: %r" % (name, _RUNS[name]))
        return _RUNS[name]
    return get


# ---------------------------------------------------------------------------------------------------------------- the checks
def check_lattice(run, i):
    """The lattice and av_vels behind call i: the undivided context's bits; the oracle's lattice to smoke()'s bar."""
    c = run.c
    call = c.calls[i]
    parts, U = [run.R[r][i] for r in range(c.nranks)], run.U[call[:2]]
    st = np.concatenate([p["state"] for p in parts], axis=0)
    assert np.array_equal(_bits(st), _bits(U["state"])), (c.name, call)
    ref = oracle_steps(c.name, call[0].startswith("driven"))[-1]
    print("%s %r: lattice within %.3g relative of the oracle's" % (c.name, call, np.max(np.abs(st - ref) / np.abs(ref))))
    assert np.all(np.abs(st - ref) <= 2e-5 * np.abs(ref)), (c.name, call)
    av = sum(p["av"].astype(np.float64) for p in parts)
    assert np.allclose(U["av"], av, rtol=2e-6, atol=0), (c.name, call)


def check_fields(run, i):
    """The field outputs of call i: no sentinel left, +0.0f in what a rank does not own, the undivided context's bits once
    assembled, the oracle's fields inside their bounds."""
    c, L = run.c, run.L
    call = c.calls[i]
    parts, U = [run.R[r][i] for r in range(c.nranks)], run.U[call[:2]]
    driven = call[0].startswith("driven")
    density = c.prm[4]
    for key, every in periods(call).items():
        what = "%s %r %s" % (c.name, call, key)
        ps = [p[key] for p in parts]
        assert not any(sentinel_survives(p) for p in ps), what
        if key == "probes":
            owner = owner_of_rows(c.xy[:, 1], c.bounds)
            assert foreign_is_plus_zero(ps, owner, 1), what
            got = assemble(ps, owner, 1)
            want, tol = fields_bound(c.name, driven, every)
            want, tol = want[:, c.xy[:, 1], c.xy[:, 0]], tol[:, c.xy[:, 1], c.xy[:, 0]]
        elif key in ("window", "wstats"):
            w = c.windows[call[1][1]]
            owner = window_row_owner(L, w, c.nx, c.ny, c.bounds)
            axis = 1 if key == "window" else 0
            assert foreign_is_plus_zero(ps, owner, axis), what
            got = assemble(ps, owner, axis)
            want, tol = fields_bound(c.name, driven, every, *window_cells(w))
        else:
            got = np.concatenate(ps, axis=1 if key == "fields" else 0)
            want, tol = fields_bound(c.name, driven, every)
        assert got.shape == U[key].shape and np.array_equal(_bits(got), _bits(U[key])), what
        if key in ("probes", "fields", "window"):
            err = np.abs(got.astype(np.float64) - want)
            print("%s: max error %.3g, worst error / bound %.3g" % (what, err.max(), np.max(err / np.where(tol > 0, tol, 1.0))))
            assert np.all(err <= tol), what
        else:
            _inside(got[..., :4], *mean_bound(want, tol), what)
            if key in ("stats", "wstats"):
                _inside(got[..., 4:], *moment_bound(want, tol, density), what + " (moments)")


def check_forces(run, i):
    """The forces of call i: each rank's contribution against the blocked cells of its own rows, exactly 0.0 for a body of
    which it holds no cell, the float64 sum over the ranks against the whole and against the undivided context."""
    c = run.c
    call = c.calls[i]
    parts, U = [run.R[r][i]["forces"] for r in range(c.nranks)], run.U[call[:2]]["forces"]
    steps = oracle_steps(c.name, call[0].startswith("driven"))
    blocked = c.ob != 0
    worst = 0.0
    for r, F in enumerate(parts):
        assert F.shape == (NSTEPS, NBODIES, 2) and not sentinel_survives(F), (c.name, call, r)
        mine = np.zeros(c.ny, bool)
        mine[c.bounds[r]:c.bounds[r + 1]] = True
        body_r = np.where(mine[:, None], c.body, 0)
        for b in range(NBODIES):
            if not ((body_r == b + 1) & blocked).any():
                assert np.all(F[:, b] == 0.0), (c.name, call, r, b)
        for t in range(NSTEPS):
            want, scale = forces_from_state(steps[t], c.ob, body_r, NBODIES)
            worst = max(worst, float(np.max(np.abs(F[t] - want) / np.where(scale > 0, scale, 1.0))))
            assert _close(F[t], want, scale), (c.name, call, r, t)
    total = sum(F.astype(np.float64) for F in parts)
    for t in range(NSTEPS):
        want, scale = forces_from_state(steps[t], c.ob, c.body, NBODIES)
        assert _close(total[t], want, scale), (c.name, call, t)
        assert _close(total[t], U[t].astype(np.float64), scale), (c.name, call, t)
    print("%s %r: a rank's forces within %.3g of the sum of the magnitudes" % (c.name, call, worst))


def runs_of(c):
    return [i for i, call in enumerate(c.calls) if not call[0].startswith("refuse")]


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_assembly_on_hand_made_arrays():
    z, s = np.float32(0.0), np.array([SENTINEL], np.uint32).view(np.float32)[0]
    a = np.array([[1, z, 3, z], [5, z, 7, z]], np.float32)          # rank 0 owns entries 0 and 2
    b = np.array([[z, -z, z, 4], [z, 6, z, 8]], np.float32)         # rank 1 owns 1 and 3, and computed a -0.0f
    owner = [0, 1, 0, 1]
    got = assemble([a, b], owner, 1)
    assert np.array_equal(_bits(got), _bits(np.array([[1, -z, 3, 4], [5, 6, 7, 8]], np.float32)))
    assert np.signbit(got[0, 1]) and not np.signbit((a + b)[0, 1])  # (what a sum would have lost)
    assert foreign_is_plus_zero([a, b], owner, 1)
    for bad in (-z, s, np.float32(1e-45)):
        a2 = a.copy()
        a2[1, 3] = bad
        assert not foreign_is_plus_zero([a2, b], owner, 1)
        assert foreign_is_plus_zero([a2, b * np.float32([1, 1, 1, 0])], [0, 1, 0, 0], 1)       # (the entry is rank 0's own there)
    with_s = a.copy()
    with_s[0, 1] = s
    assert sentinel_survives(with_s) and not sentinel_survives(a) and np.isnan(s)
    rows = [np.arange(8, dtype=np.float32).reshape(2, 2, 2), np.arange(8, 20, dtype=np.float32).reshape(3, 2, 2)]
    assert np.array_equal(np.concatenate(rows, axis=0), np.arange(20, dtype=np.float32).reshape(5, 2, 2))
    assert np.array_equal(assemble([np.zeros((3, 2)), np.ones((3, 2))], [1, 0, 1], 0), [[1, 1], [0, 0], [1, 1]])
    assert list(owner_of_rows([0, 5, 6, 12, 13, 19], [0, 6, 13, 20])) == [0, 0, 1, 1, 2, 2]


def test_window_rows_against_brute_force(L):
    """lbm_window_rows, called through the ABI, against the definition for every window and rank of every case; one window of
    every case leaves a rank without a row, and one lies wholly in the last rank."""
    for name in CASES:
        c = case(name)
        for wname, w in c.windows.items():
            x0, y0, wnx, wny, sx, sy = w
            assert x0 + (wnx - 1) * sx < c.nx and y0 + (wny - 1) * sy < c.ny and min(w[2:]) >= 1, (name, wname)
            counts = []
            for r in range(c.nranks):
                r0, r1 = c.bounds[r], c.bounds[r + 1]
                brute = [k for k in range(wny) if r0 <= y0 + k * sy < r1]
                first, count = L.window_rows(L.Window(*w), c.nx, c.ny, r0, r1)
                assert count == len(brute) and (count == 0 or first == brute[0]), (name, wname, r)
                counts.append(count)
            owner = window_row_owner(L, w, c.nx, c.ny, c.bounds)
            assert np.array_equal(owner, owner_of_rows(window_cells(w)[0], c.bounds)), (name, wname)
            if wname == "whole":
                assert counts == list(np.diff(c.bounds))
            if wname == "straddle":
                assert all(n >= 2 for n in counts) and all(b - 1 in window_cells(w)[0] and b in window_cells(w)[0] for b in c.bounds[1:-1])
            if wname == "skip":
                assert counts[1] == 0 and sum(counts) == wny and (c.nranks == 2 or min(counts[0], counts[2]) > 0)
            if wname == "strided":
                assert (x0, sx) == (1, 3)
            if wname == "one":
                assert counts == [0] * (c.nranks - 1) + [1] and y0 == c.bounds[-2]
            if wname == "in_last":
                assert counts == [0] * (c.nranks - 1) + [wny] and wny >= 2


def test_case_geometry():
    """The cases have the edges they are there for."""
    assert case("A").bounds == [0, 6, 13, 20] and case("A").nx == 33 and case("B").bounds == [0, 6, 12]
    for name in CASES:
        c = case(name)
        ob, body, nr = c.ob, c.body, c.nranks
        blocked = ob != 0
        assert body.max() == NBODIES and np.all(body[~blocked] % NBODIES == 0)
        # body 1 on either side of every boundary, with fluid across it both ways, straight and diagonal
        for b in c.bounds[1:-1]:
            assert links_across(ob, body, 1, b - 1, b) == (True, True), (name, b)
            assert links_across(ob, body, 1, b, b - 1) == (True, True), (name, b)
        # body 2 on rows 0 and ny - 1, the periodic closure, likewise
        assert links_across(ob, body, 2, c.ny - 1, 0) == (True, True) and links_across(ob, body, 2, 0, c.ny - 1) == (True, True), name
        # body 3 in one rank alone; body 4 on no blocked cell; so some rank holds no cell of bodies 2, 3 and 4
        rows3 = np.unique(np.nonzero(blocked & (body == 3))[0])
        assert len(rows3) and len(set(owner_of_rows(rows3, c.bounds))) == 1
        assert (body == 4).any() and not (blocked & (body == 4)).any()
        if nr == 3:
            assert not (blocked & (body == 2))[c.bounds[1]:c.bounds[2]].any()
        # the probes
        xy = c.xy
        assert len({tuple(q) for q in xy}) == len(xy) and np.any(np.diff(xy[:, 1]) < 0) and np.any(np.diff(xy[:, 1]) > 0)
        owner = owner_of_rows(xy[:, 1], c.bounds)
        for r in (range(nr) if name in ("A", "C2", "C3") else [0]):
            mine = xy[owner == r]
            r0, r1 = c.bounds[r], c.bounds[r + 1]
            assert (mine[:, 1] == r0).any() and (mine[:, 1] == r1 - 1).any() and (mine[:, 0] == 0).any() and (mine[:, 0] == c.nx - 1).any()
            assert blocked[mine[:, 1], mine[:, 0]].sum() >= 2, (name, r)
        if name in ("B", "R"):
            assert np.all(owner == 0)
        assert blocked[c.bad_cell[1], c.bad_cell[0]] and owner_of_rows([c.bad_cell[1]], c.bounds)[0] == 1
        # the calls: every kind the case is there for, the schedule changes sign
        kinds = {call[0] for call in c.calls}
        if name in ("A", "B"):
            assert kinds == {"forces", "probes", "sampled", "mean", "stats", "window", "wstats", "observed", "driven", "driven_observed"}
            assert {call[1][1] for call in c.calls if call[0] in ("window", "wstats")} == set(WINDOWS)
            assert ("observed", (True, 2, 3, 4), False) in c.calls and ("probes", 1, False) in c.calls and ("probes", 5, False) in c.calls
        if name in ("C2", "C3"):
            assert {"forces", "probes", "mean", "wstats", "driven_observed"} <= kinds and c.options == ()
        assert any(call[2] for call in c.calls) or name == "R"
        assert c.sched[0] > 0 > c.sched[-1] and c.sched.dtype == np.float32 and len(c.sched) == NSTEPS
    assert len([n for n in CASES]) <= 6          # (one spawn each)


def test_the_oracles_own_outputs_pass_their_bounds():
    """The bounds test the kernels, not themselves: the oracle's own float32 fields, through mean_of and stats_of, sit
    inside mean_bound and moment_bound with room to spare."""
    import lbm_oracle as O
    c = case("A")
    orc = O.Oracle("strict")
    op = O.OrcParam(c.nx, c.ny, 1, c.prm[3], c.prm[4], c.prm[5], c.prm[6])
    for every in (3, 6):
        own = np.stack([orc.final_state(op, oracle_steps("A", False)[t], c.ob).reshape(c.ny, c.nx, 4) for t in sample_steps(every)])
        want, tol = fields_bound("A", False, every)
        st = stats_of(own.astype(np.float32), p0_of(c.prm[4]))
        _inside(st[..., :4], *mean_bound(want, tol), "the oracle's own means")
        _inside(st[..., 4:], *moment_bound(want, tol, c.prm[4]), "the oracle's own moments")


# ---------------------------------------------------------------------------------------------------------------- GPU
RUN_CASES = ("A", "B", "C2", "C3")


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUN_CASES)
def test_ranks_leave_the_undivided_lattice_and_av_vels(ran, name):
    run = ran(name)
    c = run.c
    assert [tuple(n["rows"]) for n in run.notes] == [(c.bounds[r], c.bounds[r + 1]) for r in range(c.nranks)]
    for i in runs_of(c):
        check_lattice(run, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUN_CASES)
def test_rank_fields_assemble_to_the_undivided_bits_inside_the_oracle_bounds(ran, name):
    run = ran(name)
    for i in runs_of(run.c):
        check_fields(run, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUN_CASES)
def test_rank_forces_are_contributions_of_the_ranks_own_rows(ran, name):
    run = ran(name)
    n = 0
    for i in runs_of(run.c):
        if "forces" in run.R[0][i]:
            check_forces(run, i)
            n += 1
    assert n >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("C2", "C3"))
def test_register_tile_ranks_say_where_their_calls_ran(ran, name):
    """Every rank had a register tiling.  Which calls then ran inside the tiles is reported, not asserted: kernels of
    different processes are not promised to run at once on one GPU, and a piece that gives up falls back to the same bits."""
    run = ran(name)
    c = run.c
    assert all(n["engine_next"] == 3 for n in run.notes), [n["engine_next"] for n in run.notes]
    fell = [(r, c.calls[i]) for r in range(c.nranks) for i in runs_of(c) if run.notes[r][i][0] != 3 or run.notes[r][i][1] == 0]
    total = c.nranks * len(runs_of(c))
    print("case %s: %d of %d (rank, call) pairs fell back from the register tiles" % (name, len(fell), total))
    if fell:
        warnings.warn("case %s: %d of %d (rank, call) pairs fell back from the register tiles on this machine: %r"
                      % (name, len(fell), total, fell))


@pytest.mark.gpu
def test_refusals_on_ranks(ran):
    """A label outside [0, nbodies] on a blocked cell of rank 1's rows is refused there and accepted on rank 0, whose rows it
    is not in; a probe outside the lattice is refused on every rank; the probes and bodies set before serve the runs behind
    the refusals -- rank 1, which owns no probe, included."""
    run = ran("R")
    c = run.c
    kinds = [call[0] for call in c.calls]
    ib, ip = kinds.index("refuse_bodies"), kinds.index("refuse_probe")
    assert run.notes[0][ib] == "accepted", run.notes[0][ib]
    assert "label %d of blocked cell (%d, %d) is outside [0, %d]" % ((NBODIES + 5,) + c.bad_cell + (NBODIES,)) in run.notes[1][ib]
    for r in range(c.nranks):
        assert "(%d, 0) is outside the %d x %d lattice" % (c.nx, c.nx, c.ny) in run.notes[r][ip], run.notes[r][ip]
    for i in runs_of(c):
        check_lattice(run, i)
        check_fields(run, i)
        if "forces" in run.R[0][i]:
            check_forces(run, i)
    probes = [run.R[r][kinds.index("probes")]["probes"] for r in range(c.nranks)]
    assert not _bits(probes[1]).any() and _bits(probes[0]).any() and probes[1].shape == (NSTEPS, len(c.xy), 4)
