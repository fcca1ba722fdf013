"""lbm_run_driven_observed: observers under an acceleration schedule (Lattice.run_driven_observed).

Contract (include/lbm_mi355x.h): lbm_run_driven that also fills the outputs of an lbm_observe.  With X_t the fields
lbm_final_state returns after step t of the loop `set_accel(accel[t]); run(1)`: probes, snapshots and means are defined from
X_t as their single calls define them from lbm_run_sampled's snapshots, and are that bit for bit on every engine; forces[t] is
F_b on the lattice stored after step t -- the bits of `set_accel(accel[t]); run_forces(1)` under engine 1, time_block 1 where
lbm_wave or the one-step kernel took them, the register tiles' own fixed-order sums (held to the numpy forces of the loop's
lattices by test_body_forces._close) where those ran.  The lattice is lbm_run_driven's; av_vels are the loop's to rounding.

The reference of every GPU test is observed_loop: a fresh context under engine 1, time_block 1 -- the one-step kernel, which
tests/test_gpu_parity.py and tests/test_param_space.py pin to the oracle -- stepped by set_accel + run_forces(1), final_state
after every step, read_state at the marked steps; probes, snapshots and means are built from those fields in numpy.  It runs
once per (case, schedule) over the longest run; a shorter run is compared with the prefix."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, deck_paths, load_kat
from test_body_forces import _close, forces_from_state
from test_body_forces import _random_case as _random_case_with_bodies
from test_driven_run import AV_RTOL, REFUSING, SPLIT, _tile_opts, driven_oracle, schedules
from test_mean_run import _child, _kat_case, _oracle_fields, _oracle_mean_bound, _within, mean_of
from test_observed_run import _open
from test_probe_run import awkward_set
from test_sampled_run import TILINGS

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
from make_golden import PARAM_GRID, param_state  # noqa: E402

LBM_EINVAL = 1
KEYS = ("driven_observed_in_kernel", "driven_observed_in_wave", "driven_observed_pieces")
INFO = ("engine_last", "wave_launches") + KEYS
PE, ME, FE = 1, 3, 5               # the periods of the issue: the pieces cut at steps 3, 5, 6, 9, 10, 12, ...
NMAX = 23
NSTEPS = (1, 2, NMAX)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mean_from_fields(fields, every):
    """The mean of the samples after steps every, 2 every, ... of fields[t] = the fields after step t + 1: float32 adds
    in step order from +0, one float32 division."""
    picked = fields[every - 1::every]
    acc = np.zeros(fields.shape[1:], dtype=np.float32)
    for f in picked:
        acc = np.add(acc, f, dtype=np.float32)
    return np.divide(acc, np.float32(len(picked)), dtype=np.float32)


def expected(ref, n, xy, pe=0, me=0, fe=0):
    """The outputs of a call of n steps from the loop's per-step fields."""
    f = ref["fields"][:n]
    out = {}
    if pe:
        out["probes"] = f[pe - 1::pe][:, xy[:, 1], xy[:, 0], :]
    if me:
        out["mean"] = mean_from_fields(f, me)
    if fe:
        out["fields"] = f[fe - 1::fe]
    return out


def pieces_of(n, *everys):
    """The step-loop pieces of a call of n steps cut at the multiples of `everys` (0: not wanted)."""
    cuts = {n}
    for e in everys:
        if e:
            cuts |= set(range(e, n + 1, e))
    return len(cuts)


def window_stats_pieces_of(n, every, chunk, kind, cells=0):
    """The step-loop pieces of lbm_run_window_stats over n steps, restated from lbm_host_observe.inc.  kind "tiles": pieces of
    c sample steps, c = min(chunk, m) or, at chunk 0, as many samples as 64 MiB of staging hold of the `cells` window cells
    of the slab with the most (16 bytes a cell and sample; at least 1, at most m), and one piece more for the steps behind
    the last sample step; "wave": the one run; "split": a piece per sample step, and the tail."""
    m = n // every
    assert m >= 1 and chunk >= 0
    tail = 1 if n > m * every else 0
    if kind == "wave":
        return 1
    if kind == "split":
        return m + tail
    assert kind == "tiles"
    c = min(chunk, m) if chunk > 0 else min(m, max(1, (64 << 20) // (16 * cells))) if cells else m
    return -(-m // c) + tail


def want_for(n, forces=True, pe=PE, me=ME, fe=FE):
    """run_driven_observed's keyword arguments for a run of n steps: a mean whose first sample step lies beyond n is a
    refusal, so a run that short asks for none (snapshots beyond n are legal and write nothing)."""
    return dict(forces=forces, probes_every=pe, mean_every=me if me and n >= me else 0, fields_every=fe)


def observed_loop(L, p, ob, cells, body, nb, accel, marks, options=SPLIT, numpy_forces=True, **kw):
    """The reference: set_accel(accel[t]) + run_forces(1) on a fresh context; final_state after every step.
    kw: the context's kind (default: a lattice alone) -- slabs add up their own forces, so the forces of a context of slabs
    off the register tiles are the bits of the loop on such a context."""
    ob2 = np.asarray(ob).reshape(p.ny, p.nx)
    av, F, Fw, scale, fields, states = [], [], [], [], [], {}
    with L.Lattice(p, ob, cells, **kw) as lat:
        for k, v in options:
            lat.set_option(k, v)
        lat.set_bodies(body, nb)
        for t, a in enumerate(accel):
            lat.set_accel(float(a))
            a1, f1 = lat.run_forces(1)
            assert lat.info("engine_last") == 1
            av.append(a1)
            F.append(f1[0])
            fields.append(lat.final_state())
            if numpy_forces or t + 1 in marks:
                st = lat.read_state()
            if numpy_forces:
                w, s = forces_from_state(st, ob2, body, nb)
                Fw.append(w)
                scale.append(s)
            if t + 1 in marks:
                states[t + 1] = st
    ref = dict(av_vels=np.concatenate(av), forces=np.array(F), fields=np.array(fields), states=states)
    if numpy_forces:
        ref["numpy_forces"], ref["scale"] = np.array(Fw), np.array(scale)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            assert np.all(np.isfinite(v))
            v.setflags(write=False)
    return ref


_REF = {}


def reference(L, key, p, ob, cells, body, nb, accel, marks, options=SPLIT, numpy_forces=True):
    k = (key, accel.tobytes(), tuple(sorted(marks)), options, numpy_forces)
    if k not in _REF:
        _REF[k] = observed_loop(L, p, ob, cells, body, nb, accel, set(marks), options, numpy_forces)
    return _REF[k]


def observed(L, p, ob, cells, accel, want, body, nb, xy, options=(), **kw):
    """A fresh context, one run_driven_observed: its dict, with "state" and "info" added."""
    with _open(L, p, ob, cells, body, nb, xy, options, kw) as lat:
        res = lat.run_driven_observed(accel, **want)
        res["info"] = {k: int(lat.info(k)) for k in INFO}
        assert np.float32(lat.info("accel")) == np.float32(p.accel)          # the context's own acceleration is untouched
        res["state"] = lat.read_state()
    return res


def check(res, ref, n, xy, want, where, tile_forces):
    """Every wanted output against the reference's prefix of n steps; the lattice; av_vels to rounding."""
    exp = expected(ref, n, xy, want["probes_every"], want["mean_every"], want["fields_every"])
    for name in ("probes", "mean", "fields"):
        assert (name in res) == (name in exp), (where, name)
        if name in exp:
            assert res[name].shape == exp[name].shape, (where, name, res[name].shape, exp[name].shape)
            bad = np.argwhere(_bits(res[name]) != _bits(exp[name]))
            assert len(bad) == 0, (where, name, len(bad), [tuple(int(v) for v in b) for b in bad[:6]])
    if want["forces"]:
        assert res["forces"].shape == ref["forces"][:n].shape, where
        if tile_forces:
            print(where, "forces: worst error / scale %.3g" %
                  float(np.max(np.abs(res["forces"] - ref["numpy_forces"][:n]) / np.maximum(ref["scale"][:n], 1e-30))))
            assert _close(res["forces"], ref["numpy_forces"][:n], ref["scale"][:n]), where
        else:
            assert np.array_equal(_bits(res["forces"]), _bits(ref["forces"][:n])), where
    if n in ref["states"]:
        assert np.array_equal(_bits(res["state"]), _bits(ref["states"][n])), (where, "lattice")
    av, av_l = res["av_vels"], ref["av_vels"][:n]
    assert av.shape == (n,), where
    print(where, "av_vels: worst relative difference %.3g" % (np.max(np.abs(av - av_l) / np.maximum(np.abs(av_l), 1e-30)) if n else 0.0))
    assert np.allclose(av, av_l, rtol=AV_RTOL, atol=0), where


def _deck(L, deck):
    pf, of = deck_paths(deck)
    p = L.read_params(pf)
    ob = np.ascontiguousarray(L.read_obstacles(of, p), dtype=np.int32).reshape(p.ny, p.nx)
    body = np.where(ob != 0, 1 + (np.arange(p.nx)[None, :] >= p.nx // 2), 0).astype(np.int32)       # two bodies: west, east
    return p, ob, body


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_driven_observed_run_is_declared_and_bound(L):
    assert "lbm_run_driven_observed" in L.ABI_SYMBOLS
    hdr = open(L.HEADER_PATH).read()
    assert ("int lbm_run_driven_observed(lbm_ctx* ctx, int nsteps, float* av_vels, const float* accel, "
            "const lbm_observe* what);") in hdr
    lib = L.load_library()
    assert lib.lbm_run_driven_observed.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(L.Observe)]
    built = open(L.LIB_PATH, "rb").read()
    for key in KEYS:
        assert '"%s"' % key in hdr, key
        assert key.encode() + b"\0" in built, key
        v = C.c_double(-1.0)
        assert lib.lbm_get_info(None, key.encode(), C.byref(v)) == LBM_EINVAL and v.value == -1.0
    assert lib.lbm_run_driven_observed(None, 3, None, None, None) == LBM_EINVAL and b"ctx" in lib.lbm_last_error()
    doc = L.Lattice.run_driven_observed.__doc__
    assert all(key in doc for key in KEYS)


def test_run_driven_observed_refuses_what_is_no_schedule_in_python(L):
    """Before the library is asked (no context needed: the checks come first)."""
    lat = L.Lattice.__new__(L.Lattice)                   # (never created: the call must refuse before it touches it)
    for bad in (np.zeros((3, 2), np.float32), np.float32(0.01), np.array(["0.01", "0.02"]),
                np.array([None, None], dtype=object), np.array([1 + 2j, 3])):
        with pytest.raises(L.LbmError):
            L.Lattice.run_driven_observed(lat, bad, forces=True)


def test_the_numpy_mean_is_test_mean_runs_definition(L, O, oracle):
    """mean_from_fields on the strict float oracle's own per-step fields of the 64 x 40 known-answer case: the bits of
    test_mean_run.mean_of on the same samples, and within the oracle bound of tests/test_mean_run.py."""
    k, p, ob, op = _kat_case(L, O)
    want, bound, own, _ = _oracle_mean_bound(k, p, ob, op, oracle)
    for every in (1, 3, 5):
        got = mean_from_fields(own, every)
        assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(mean_of(own[every - 1::every])))
    err, lim = _within(mean_from_fields(own, 1), want, bound)
    assert np.all(err <= lim)
    assert pieces_of(23, ME, FE) == 11 and pieces_of(23, 0, 0) == 1 and pieces_of(2, ME, FE) == 1 and pieces_of(15, ME, FE) == 7


# ---------------------------------------------------------------------------------------------------------------- GPU
def _tiling_case(L, ty, r, nx, ny, seed):
    p, ob, cells, body = _random_case_with_bodies(L, nx, ny, seed)
    return p, ob, cells, body, awkward_set(nx, ny, ob, ty, r)


def _check_tiling(L, key, case, opts, names, extra=()):
    p, ob, cells, body, xy = case
    s = schedules(p.accel, NMAX, 17)
    for name in names:
        ref = reference(L, key, p, ob, cells, body, 4, s[name], NSTEPS, SPLIT + extra)
        for n in NSTEPS:
            want = want_for(n)
            res = observed(L, p, ob, cells, s[name][:n], want, body, 4, xy, opts + extra)
            where = (key, opts, name, n, res["info"])
            assert res["info"]["engine_last"] == 3 and res["info"]["driven_observed_in_kernel"] == 3, where
            assert res["info"]["driven_observed_in_wave"] == 0, where
            assert res["info"]["driven_observed_pieces"] == pieces_of(n, want["mean_every"], want["fields_every"]), where
            check(res, ref, n, xy, want, where, tile_forces=True)


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", TILINGS)
def test_observers_under_a_schedule_on_every_register_tiling(gpu, ty, r, asy, nx, ny):
    L = gpu
    case = _tiling_case(L, ty, r, nx, ny, 7)
    p, ob, cells, body, xy = case
    opts = _tile_opts(ty, r, asy)
    _check_tiling(L, (nx, ny, 7), case, opts, ("b", "d0", "d11", "d22"))
    # schedule (a) is lbm_run_observed with the same `what` on the same tiling: every output, forces and av_vels, bit for bit
    s = schedules(p.accel, NMAX, 17)
    want = want_for(NMAX)
    with _open(L, p, ob, cells, body, 4, xy, opts, {}) as lat:
        plain = lat.run_observed(NMAX, **want)
        assert lat.info("engine_last") == 3 and lat.info("observed_in_kernel") == 3
        st0 = lat.read_state()
    res = observed(L, p, ob, cells, s["a"], want, body, 4, xy, opts)
    assert res["info"]["driven_observed_in_kernel"] == 3
    for name in ("av_vels", "forces", "probes", "mean", "fields"):
        assert np.array_equal(_bits(res[name]), _bits(plain[name])), name
    assert np.array_equal(_bits(res["state"]), _bits(st0))
    # a call cut in two at a common multiple of the periods, 15 + 8 steps, against the one call
    whole = observed(L, p, ob, cells, s["b"], want, body, 4, xy, opts)
    with _open(L, p, ob, cells, body, 4, xy, opts, {}) as lat:
        one = lat.run_driven_observed(s["b"][:15], **want_for(15))
        assert lat.info("driven_observed_pieces") == pieces_of(15, ME, FE)
        two = lat.run_driven_observed(s["b"][15:], **want_for(8))
        assert lat.info("driven_observed_in_kernel") == 3 and lat.info("driven_observed_pieces") == pieces_of(8, ME, FE)
        assert np.array_equal(_bits(lat.read_state()), _bits(whole["state"]))
    for name in ("probes", "fields"):
        assert np.array_equal(_bits(np.concatenate([one[name], two[name]])), _bits(whole[name])), name
    ref = reference(L, (nx, ny, 7), p, ob, cells, body, 4, s["b"], NSTEPS)
    both = np.concatenate([one["forces"], two["forces"]])
    assert _close(both, ref["numpy_forces"], ref["scale"])
    assert np.allclose(np.concatenate([one["av_vels"], two["av_vels"]]), whole["av_vels"], rtol=AV_RTOL, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", [TILINGS[2], TILINGS[4]])
def test_observers_under_a_schedule_with_ieee_maths(gpu, ty, r, asy, nx, ny):
    L = gpu
    assert r in (2, 4) and asy == 1
    _check_tiling(L, (nx, ny, 8), _tiling_case(L, ty, r, nx, ny, 8), _tile_opts(ty, r, asy), ("b", "d11"), (("kernel_variant", 0),))


@pytest.mark.gpu
def test_each_observer_alone_and_none(gpu):
    """Tiling (8, 4, 1) at 256 x 256.  Forces alone, probes alone and the pair run as ONE piece, and av_vels are then
    lbm_run_driven's bits; a mean or a snapshot series alone cuts its pieces; no observer is lbm_run_driven itself."""
    L = gpu
    ty, r, asy, nx, ny = 8, 4, 1, 256, 256
    assert (ty, r, asy, nx, ny) in TILINGS
    case = _tiling_case(L, ty, r, nx, ny, 9)
    p, ob, cells, body, xy = case
    opts = _tile_opts(ty, r, asy)
    s = schedules(p.accel, NMAX, 18)["b"]
    ref = reference(L, (nx, ny, 9), p, ob, cells, body, 4, s, (NMAX,))
    with _open(L, p, ob, cells, None, 0, None, opts, {}) as lat:
        av_d = lat.run_driven(s)
        assert lat.info("driven_in_kernel") == 1
        st_d = lat.read_state()
    assert np.array_equal(_bits(st_d), _bits(ref["states"][NMAX]))
    wants = {"forces": (dict(forces=True), 1, 1), "probes": (dict(probes_every=PE), 2, 1),
             "forces+probes": (dict(forces=True, probes_every=PE), 3, 1),
             "mean": (dict(mean_every=ME), 0, pieces_of(NMAX, ME)), "fields": (dict(fields_every=FE), 0, pieces_of(NMAX, FE))}
    for name, (kw, bits, pieces) in wants.items():
        want = dict(dict(forces=False, probes_every=0, mean_every=0, fields_every=0), **kw)
        res = observed(L, p, ob, cells, s, want, body, 4, xy, opts)
        where = (name, res["info"])
        assert res["info"]["engine_last"] == 3 and res["info"]["driven_observed_in_kernel"] == bits, where
        assert res["info"]["driven_observed_pieces"] == pieces and res["info"]["driven_observed_in_wave"] == 0, where
        check(res, ref, NMAX, xy, want, where, tile_forces=True)
        if pieces == 1:
            assert np.array_equal(_bits(res["av_vels"]), _bits(av_d)), where
    # what = NULL, and all four pointers NULL: lbm_run_driven, lattice and av_vels bit for bit
    lib = L.load_library()
    for what in (None, L.Observe()):
        with _open(L, p, ob, cells, body, 4, xy, opts, {}) as lat:
            av = np.zeros(NMAX, np.float32)
            assert lib.lbm_run_driven_observed(lat._ctx, NMAX, av.ctypes.data, s.ctypes.data,
                                               C.byref(what) if what is not None else None) == 0
            assert lat.info("engine_last") == 3 and lat.info("driven_observed_in_kernel") == 0
            assert np.array_equal(_bits(lat.read_state()), _bits(st_d)) and np.array_equal(_bits(av), _bits(av_d))
    with _open(L, p, ob, cells, body, 4, xy, opts, {}) as lat:
        res = lat.run_driven_observed(s)
        assert sorted(res) == ["av_vels"] and np.array_equal(_bits(res["av_vels"]), _bits(av_d))


def _off_the_tiles(L, key, p, ob, cells, body, nb, xy, s, n, options=(), numpy_ref=False, **kw):
    """One call with all four observers on a context of another kind against the lone loop: same bits everywhere; the
    three keys read 0 off the tiles, and what the register tiles across slabs took is held as on a lattice alone."""
    ref = reference(L, key, p, ob, cells, body, nb, s, (n,), numpy_forces=numpy_ref)
    want = want_for(n)
    res = observed(L, p, ob, cells, s, want, body, nb, xy, options, **kw)
    where = (key, options, sorted(kw), res["info"])
    tiles = res["info"]["engine_last"] == 3
    assert not tiles or numpy_ref, where
    if tiles:
        assert res["info"]["driven_observed_in_kernel"] == 3, where
        assert res["info"]["driven_observed_pieces"] == pieces_of(n, want["mean_every"], want["fields_every"]), where
    else:
        assert [res["info"][k] for k in KEYS] == [0, 0, 0], where
    check(res, ref, n, xy, want, where, tile_forces=tiles)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("nslabs,exchange", [(2, "copy"), (4, "copy"), (2, "p2p")])
def test_slabs_give_the_loops_outputs(gpu, nslabs, exchange):
    L = gpu
    p, ob, body = _deck(L, "256x256")
    rows = p.ny // nslabs
    xy = awkward_set(p.nx, p.ny, ob, 0, 1, extra_rows=(rows - 1, rows, p.ny - rows))
    s = schedules(p.accel, NMAX, 21)
    ex = L.EXCHANGE_COPY if exchange == "copy" else L.EXCHANGE_P2P
    for name in ("b", "d11"):
        res = _off_the_tiles(L, "256x256", p, ob, None, body, 2, xy, s[name], NMAX, numpy_ref=True,
                             nslabs=nslabs, devices=[0] * nslabs, exchange=ex)
        if exchange == "p2p":                # register tiles across slabs
            assert res["info"]["engine_last"] == 3, res["info"]


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["rccl", "p2p"])
def test_rank_context_ring_of_one_gives_the_loops_outputs(gpu, exchange):
    L = gpu
    p, ob, body = _deck(L, "128x256")
    xy = awkward_set(p.nx, p.ny, ob, 0, 1)
    s = schedules(p.accel, 13, 22)["b"]
    os.environ["LBM_FORCE_EXCHANGE"] = "1"
    try:
        ex = L.EXCHANGE_RCCL if exchange == "rccl" else L.EXCHANGE_P2P
        _off_the_tiles(L, "128x256", p, ob, None, body, 2, xy, s, 13, numpy_ref=True,
                       rank=0, nranks=1, device=0, unique_id=L.rccl_unique_id(), exchange=ex)
    finally:
        del os.environ["LBM_FORCE_EXCHANGE"]


@pytest.mark.gpu
@pytest.mark.parametrize("time_block", [1, 2, 4, 8])
def test_streaming_engines_give_the_loops_outputs(gpu, time_block):
    L = gpu
    p, ob, body = _deck(L, "256x256")
    xy = awkward_set(p.nx, p.ny, ob, 0, 1)
    s = schedules(p.accel, 21, 23)["b"]
    # (march_kernel 0 keeps lbm_wave away at time_block 4 and 8 here: its own flavour has its own test file)
    res = _off_the_tiles(L, "256x256", p, ob, None, body, 2, xy, s, 21, (("engine", 1), ("march_kernel", 0), ("time_block", time_block)))
    assert res["info"]["engine_last"] == 1 and res["info"]["wave_launches"] == 0


@pytest.mark.gpu
def test_a_lattice_that_does_not_tile(gpu):
    L = gpu
    k = load_kat("kat_33x20")
    p = L.Param(int(k["nx"]), int(k["ny"]), 10, int(k["reynolds_dim"]), float(k["density"]), float(k["accel"]), float(k["omega"]))
    ob = np.ascontiguousarray(k["obstacles"], dtype=np.int32).reshape(p.ny, p.nx)
    cells = np.ascontiguousarray(k["cells0"], dtype=np.float32)
    body = (ob != 0).astype(np.int32)
    xy = awkward_set(p.nx, p.ny, ob, 0, 1)
    s = schedules(p.accel, NMAX, 24)
    for name in ("b", "d0", "d22"):
        res = _off_the_tiles(L, "kat_33x20", p, ob, cells, body, 1, xy, s[name], NMAX)
        assert res["info"]["engine_last"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("engine", sorted(REFUSING))
def test_where_the_accelerate_guard_refuses(gpu, engine):
    """The (density, accel, omega) point of tests/test_param_space.py at which the guard refuses cells of row ny - 2 during
    the run, from rest, with schedule (b) around its acceleration (tests/test_driven_run.py counts the refusals on the
    oracle): the outputs are the loop's.  Under lbm_wave<8> the mean and the snapshots come every 16 and every 8 steps, so
    that the pieces (8, 8 and 5 steps) hold full passes."""
    L = gpu
    nx, ny, opts, want_info = REFUSING[engine]
    d, a, o = PARAM_GRID["refusal"]
    ob, cells = param_state("refusal", nx, ny, 51, "rest")
    ob = np.ascontiguousarray(ob, dtype=np.int32).reshape(ny, nx)
    p = L.Param(nx, ny, 100, 10, d, a, o)
    body = (ob != 0).astype(np.int32)
    n = 21
    s = schedules(a, n, 25)["b"]
    tiles = want_info["engine_last"] == 3
    xy = awkward_set(nx, ny, ob, 8 if tiles else 0, 4 if tiles else 1)
    ref = reference(L, ("refusal", nx, ny), p, ob, cells, body, 1, s, (n,))
    want = want_for(n) if tiles else want_for(n, me=16, fe=8)
    res = observed(L, p, ob, cells, s, want, body, 1, xy, opts)
    assert res["info"]["engine_last"] == want_info["engine_last"], res["info"]
    assert res["info"]["driven_observed_pieces"] == pieces_of(n, want["mean_every"], want["fields_every"]), res["info"]
    assert res["info"]["driven_observed_in_kernel"] == (3 if tiles else 0) and res["info"]["driven_observed_in_wave"] == (0 if tiles else 3)
    check(res, ref, n, xy, want, (engine, res["info"]), tile_forces=tiles)


# torch and the library share libamdhip64: torch is imported FIRST, in a child process of its own
_DEVICE_OUTPUT = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_driven_observed import _bits, _deck, observed, want_for
from test_driven_run import schedules
from test_observed_run import _open
from test_probe_run import awkward_set
p, ob, body = _deck(L, "128x256")
xy = awkward_set(p.nx, p.ny, ob, 0, 1)
n = 12
s = schedules(p.accel, n, 26)["b"]
want = want_for(n, pe=2, me=5, fe=4)
nan = float("nan")
for engine in (0, 1):
    opts = (("engine", engine),)
    host = observed(L, p, ob, None, s, want, body, 2, xy, opts)
    outs = dict(probes_out=torch.full((n // 2, len(xy), 4), nan, dtype=torch.float32, device="cuda:0"),
                mean_out=torch.full((p.ny, p.nx, 4), nan, dtype=torch.float32, device="cuda:0"),
                fields_out=torch.full((n // 4, p.ny, p.nx, 4), nan, dtype=torch.float32, device="cuda:0"))
    with _open(L, p, ob, None, body, 2, xy, opts, {{}}) as lat:
        res = lat.run_driven_observed(s, **want, **outs)
        assert (lat.info("driven_observed_in_kernel") == 3) == (engine == 0)
        assert np.array_equal(_bits(lat.read_state()), _bits(host["state"]))
    torch.cuda.synchronize()
    for name, key in (("probes", "probes_out"), ("mean", "mean_out"), ("fields", "fields_out")):
        assert res[name] is outs[key], name
        assert np.array_equal(_bits(res[name].cpu().numpy()), _bits(host[name])), (engine, name)
    assert np.array_equal(_bits(res["forces"]), _bits(host["forces"])) and np.array_equal(_bits(res["av_vels"]), _bits(host["av_vels"]))
print("device output ok")
"""


@pytest.mark.gpu
def test_device_output_is_the_host_output(gpu):
    assert "device output ok" in _child(_DEVICE_OUTPUT)


@pytest.mark.gpu
def test_refusals_leave_the_lattice_alone(gpu):
    """Every refusal returns its code with a message, and a following run(5) gives the bits of a fresh context's run(5)."""
    L = gpu
    lib = L.load_library()
    p, ob, body = _deck(L, "128x128")
    xy = awkward_set(p.nx, p.ny, ob, 0, 1)
    n = 10
    good = schedules(p.accel, n, 27)["b"]
    F = np.zeros((n, 2, 2), np.float32)
    P = np.zeros((n, len(xy), 4), np.float32)
    M = np.zeros((p.ny, p.nx, 4), np.float32)
    S = np.zeros((n, p.ny, p.nx, 4), np.float32)
    with L.Lattice(p, ob) as fresh:
        av5, st5 = fresh.run(5), fresh.read_state()

    def obs(forces=None, probes=None, mean=None, fields=None, pe=1, me=1, fe=1):
        w = L.Observe()
        w.forces = forces.ctypes.data if forces is not None else None
        w.probes_out = probes.ctypes.data if probes is not None else None
        w.mean_out = mean.ctypes.data if mean is not None else None
        w.fields_out = fields.ctypes.data if fields is not None else None
        w.probes_every, w.mean_every, w.fields_every = pe, me, fe
        return w

    def refused(setup, nsteps, accel, w, *words):
        with L.Lattice(p, ob) as lat:
            if setup:
                lat.set_bodies(body, 2)
                lat.set_probes(xy)
            tag = lat.info("regtile_tag")
            rc = lib.lbm_run_driven_observed(lat._ctx, nsteps, None, accel.ctypes.data if accel is not None else None,
                                             C.byref(w) if w is not None else None)
            msg = lib.lbm_last_error().decode()
            assert rc == LBM_EINVAL and msg, (rc, msg, words)
            for word in words:
                assert word in msg, (word, msg)
            assert lat.info("regtile_tag") == tag                      # nothing was queued
            assert np.float32(lat.info("accel")) == np.float32(p.accel)
            av = lat.run(5)
            assert np.array_equal(_bits(av), _bits(av5)) and np.array_equal(_bits(lat.read_state()), _bits(st5)), words

    assert lib.lbm_run_driven_observed(None, n, None, good.ctypes.data, None) == LBM_EINVAL and lib.lbm_last_error()
    refused(True, -1, good, obs(forces=F, probes=P), "nsteps")
    refused(True, n, None, obs(forces=F, probes=P), "accel")
    refused(True, n, None, None, "accel")
    for bad in (np.nan, np.inf, -np.inf):
        s = good.copy()
        s[3] = bad
        refused(True, n, s, obs(forces=F, probes=P), "accel[3]")
        refused(True, n, s, None, "accel[3]")
    refused(False, n, good, obs(forces=F, mean=M), "bodies")
    refused(False, n, good, obs(probes=P, mean=M), "probes")
    refused(False, n, good, obs(forces=F), "bodies")
    for bad in (0, -1):
        refused(True, n, good, obs(forces=F, probes=P, pe=bad), "probes_every")
        refused(True, n, good, obs(probes=P, pe=bad), "probes_every")
        refused(True, n, good, obs(forces=F, mean=M, me=bad), "mean_every")
        refused(True, n, good, obs(mean=M, me=bad), "mean_every")
    refused(True, n, good, obs(forces=F, probes=P, pe=n + 1), "probes_every", "nsteps")
    refused(True, n, good, obs(mean=M, me=n + 1), "mean_every")
    refused(True, n, good, obs(forces=F, fields=S, fe=-1), "fields_every")
    refused(True, n, good, obs(fields=S, fe=-1), "fields_every")
    assert not F.any() and not P.any() and not M.any() and not S.any()
    with L.Lattice(p, ob) as lat:
        lat.set_bodies(body, 2)
        lat.set_probes(xy)
        # nsteps = 0: success, nothing runs
        assert lib.lbm_run_driven_observed(lat._ctx, 0, None, None, C.byref(obs(forces=F))) == 0
        assert lib.lbm_run_driven_observed(lat._ctx, 0, None, None, None) == 0
        assert sorted(lat.run_driven_observed(np.empty(0, np.float32), forces=True)) == ["av_vels", "forces"]
        # fields_every = 0, or no sample step: legal, nothing written
        for fe in (0, n + 1):
            S[:] = 7.0
            assert lib.lbm_run_driven_observed(lat._ctx, 0, None, None, C.byref(obs(forces=F, fields=S, fe=fe))) == 0
            assert np.all(S == 7.0)
        av = lat.run(5)
        assert np.array_equal(_bits(av), _bits(av5)) and np.array_equal(_bits(lat.read_state()), _bits(st5))


@pytest.mark.gpu
def test_a_device_pointer_on_another_device_is_refused(gpu):
    """A probe output in the memory of a device that holds no slab: LBM_EINVAL, nothing queued (as
    tests/test_sampled_run.py::test_device_output_needs_every_slab_on_its_device, which needs two devices too)."""
    if gpu.device_count() < 2:
        pytest.skip("needs two HIP devices")
    assert "other device ok" in _child(_OTHER_DEVICE)


_OTHER_DEVICE = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_driven_observed import _bits, _deck
from test_probe_run import awkward_set
p, ob, body = _deck(L, "128x128")
xy = awkward_set(p.nx, p.ny, ob, 0, 1)
s = np.full(10, p.accel, dtype=np.float32)
with L.Lattice(p, ob) as fresh:
    av5, st5 = fresh.run(5), fresh.read_state()
out = torch.zeros((10, len(xy), 4), dtype=torch.float32, device="cuda:1")
with L.Lattice(p, ob) as lat:
    lat.set_probes(xy)
    try:
        lat.run_driven_observed(s, probes_every=1, probes_out=out)
    except L.LbmError as e:
        assert "device" in str(e)
    else:
        raise AssertionError("not refused")
    av = lat.run(5)
    assert np.array_equal(_bits(av), _bits(av5)) and np.array_equal(_bits(lat.read_state()), _bits(st5))
print("other device ok")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("deck", ["128x128", "256x256"])
def test_fifty_driven_observed_steps_against_the_float_oracle(gpu, O, oracle, deck):
    """50 steps from rest under schedule (e) with probes every step, a snapshot after step 50 and forces, on the default
    engine.  The lattice against driven_oracle in float with the bars of
    test_driven_run.test_fifty_driven_steps_against_the_float_oracle (5e-5 of the largest population, av_vels rtol 1e-4);
    the snapshot and the probes against the fields derived from the oracle's lattice within the per-element bound of
    _oracle_fields as tests/test_sampled_run.py and tests/test_mean_run.py call it (the lattice to 2e-5 relative, carried
    through the derive)."""
    L = gpu
    pf, of = deck_paths(deck)
    p = L.read_params(pf)
    ob = np.ascontiguousarray(L.read_obstacles(of, p), dtype=np.int32).reshape(p.ny, p.nx)
    op = O.read_params(pf)
    n = 50
    s = schedules(float(np.float32(p.accel)), n, 5)["e"]
    body = (ob != 0).astype(np.int32)
    xy = awkward_set(p.nx, p.ny, ob, 0, 1)
    res = observed(L, p, ob, None, s, dict(forces=True, probes_every=1, mean_every=0, fields_every=n), body, 1, xy)
    assert res["info"]["engine_last"] == 3 and res["info"]["driven_observed_in_kernel"] == 3, res["info"]
    cells = oracle.init_cells(op, np.float32)
    for t in range(n):
        driven_oracle(oracle, op, cells, ob, s[t:t + 1])
        if t + 1 in (1, 10, 25, n):
            w, tol = _oracle_fields(cells.reshape(p.ny, p.nx, 9), ob, p.density)
            err = np.abs(res["probes"][t].astype(np.float64) - w[xy[:, 1], xy[:, 0]])
            lim = tol[xy[:, 1], xy[:, 0]]
            print(deck, "step %d: max probe error %.3g, worst error - bound %.3g" % (t + 1, err.max(), np.max(err - lim)))
            assert np.all(err <= lim), (t, float(np.max(err - lim)))
    st = res["state"].reshape(cells.shape)
    print(deck, "lattice %.3g of the largest population" % (np.abs(st - cells).max() / np.abs(cells).max()))
    assert np.abs(st - cells).max() <= 5e-5 * np.abs(cells).max()
    av_o = driven_oracle(oracle, op, oracle.init_cells(op, np.float32), ob, s)
    assert np.allclose(res["av_vels"], av_o, rtol=1e-4, atol=0)
    err = np.abs(res["fields"][0].astype(np.float64) - w)
    print(deck, "snapshot after step 50: max error %.3g, worst error - bound %.3g" % (err.max(), np.max(err - tol)))
    assert np.all(err <= tol), float(np.max(err - tol))
