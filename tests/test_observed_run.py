"""lbm_run_observed: forces, probes, means and snapshots of ONE run (Lattice.run_observed).

Contract (include/lbm_mi355x.h): every wanted output is, bit for bit, what its own call (lbm_run_forces, lbm_run_probes,
lbm_run_mean, lbm_run_sampled) writes from the same state with the same options, bodies, probes and period; the lattice is
lbm_run's, and so is av_vels wherever the register tiles ran the call.  The reference of every test below is therefore the
single calls, each on a fresh context from the same start.  Forces with probes ride in one register-tile launch (flavour
kRegForce | kRegProbe, info "observed_in_kernel" = 3, "observed_pieces" = 1); means and snapshots cut the step loop into
pieces."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_body_forces import DECK_STEPS, _close, _labellings, _per_step, forces_from_state
from test_body_forces import _random_case as _random_case_with_bodies
from test_mean_run import _child, _kat_case, _oracle_fields
from test_probe_run import _bits, _deck, _slab_set, _three_rows, _tiling, awkward_set
from test_sampled_run import TILINGS

LBM_EINVAL = 1
KINDS = ("forces", "probes", "mean", "fields")
INFO = ("engine_last", "observed_in_kernel", "observed_pieces")


def _want(kinds, probes_every=1, mean_every=7, fields_every=5):
    """keyword arguments of Lattice.run_observed for a subset of KINDS"""
    return dict(forces="forces" in kinds, probes_every=probes_every if "probes" in kinds else 0,
                mean_every=mean_every if "mean" in kinds else 0, fields_every=fields_every if "fields" in kinds else 0)


def _open(L, p, ob, cells, body, nb, xy, options, kw):
    lat = L.Lattice(p, ob, cells, **kw)
    for k, v in options:
        lat.set_option(k, v)
    if body is not None:
        lat.set_bodies(body, nb)
    if xy is not None:
        lat.set_probes(xy)
    return lat


def _observed(L, p, ob, cells, nsteps, want, body=None, nb=0, xy=None, options=(), **kw):
    """A fresh context, one run_observed: its dict, with "state" and "info" added."""
    with _open(L, p, ob, cells, body, nb, xy, options, kw) as lat:
        res = lat.run_observed(nsteps, **want)
        res["info"] = {k: lat.info(k) for k in INFO}
        res["state"] = lat.read_state()
    return res


def _singles(L, p, ob, cells, nsteps, want, body=None, nb=0, xy=None, options=(), skip=0, **kw):
    """The reference: lbm_run and each wanted single call, each on a fresh context from the same start (after `skip` plain
    steps) with the same options, bodies and probes."""
    ref = {}
    with _open(L, p, ob, cells, body, nb, xy, options, kw) as lat:
        lat.run(skip)
        ref["av_vels"] = lat.run(nsteps)
        ref["state"] = lat.read_state()
    calls = []
    if want["forces"]:
        calls.append(("forces", lambda lat: lat.run_forces(nsteps)))
    if want["probes_every"]:
        calls.append(("probes", lambda lat: lat.run_probes(nsteps, want["probes_every"])))
    if want["mean_every"]:
        calls.append(("mean", lambda lat: lat.run_mean(nsteps, want["mean_every"])))
    if want["fields_every"]:
        calls.append(("fields", lambda lat: lat.run_sampled(nsteps, want["fields_every"])))
    for name, call in calls:
        with _open(L, p, ob, cells, body, nb, xy, options, kw) as lat:
            lat.run(skip)
            _, ref[name] = call(lat)
    return ref


def _same(res, ref, what=""):
    """every output of the reference is there, bit for bit; the lattice too"""
    for name in KINDS:
        assert (name in res) == (name in ref), (what, name)
        if name in ref:
            assert res[name].shape == ref[name].shape, (what, name, res[name].shape, ref[name].shape)
            assert np.array_equal(_bits(res[name]), _bits(ref[name])), (what, name)
    assert np.array_equal(_bits(res["state"]), _bits(ref["state"])), (what, "lattice")


def _same_av(res, ref, what=""):
    assert np.array_equal(_bits(res["av_vels"]), _bits(ref["av_vels"])), (what, "av_vels")


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_observed_run_is_declared_and_bound(L):
    assert "lbm_run_observed" in L.ABI_SYMBOLS
    hdr = open(L.HEADER_PATH).read()
    assert "int lbm_run_observed(lbm_ctx* ctx, int nsteps, float* av_vels, const lbm_observe* what);" in hdr
    assert '"observed_in_kernel"' in hdr and '"observed_pieces"' in hdr
    assert callable(L.Lattice.run_observed)
    lib = L.load_library()
    assert lib.lbm_run_observed.argtypes[3] == C.POINTER(L.Observe)


def test_the_ctypes_structure_has_the_layout_the_header_states(L):
    hdr = open(L.HEADER_PATH).read()
    m = re.search(r"sizeof\(lbm_observe\) = (\d+); offsets ([^(]*)\(", hdr)
    assert m, "the header states the layout of lbm_observe"
    assert C.sizeof(L.Observe) == int(m.group(1)) == 48
    stated = {name: int(off) for name, off in re.findall(r"(\w+) (\d+)", m.group(2))}
    fields = [f[0] for f in L.Observe._fields_]
    assert fields == ["forces", "probes_out", "mean_out", "fields_out", "probes_every", "mean_every", "fields_every"]
    assert stated == {name: getattr(L.Observe, name).offset for name in fields}
    # the members as the header declares them, in this order
    body = re.search(r"typedef struct \{([^{}]*)\} lbm_observe;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)\s*[;,]", body) == fields


def test_observed_run_rejects_a_null_context(L):
    lib = L.load_library()
    assert lib.lbm_run_observed(None, 10, None, None) == LBM_EINVAL
    assert b"ctx" in lib.lbm_last_error()
    what = L.Observe()
    assert lib.lbm_run_observed(None, 10, None, C.byref(what)) == LBM_EINVAL
    assert b"ctx" in lib.lbm_last_error()


def test_isa_audit_covers_the_force_and_probe_flavour():
    """tools/audit_regtile_isa.py lists the asynchronous force + probe instantiations (mode bits 32768 | 131072) of
    lbm_regtile and lbm_regtile_slabs for R = 2 and 4, fast and IEEE maths, each with 0 findings, and nothing else has one
    either."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_regtile_isa.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = {}
    for name, rr, mode, nf in re.findall(r"^(lbm_regtile(?:_slabs)?)<(\d+), (\d+)>: \d+ asm loads audited, (\d+) finding\(s\)",
                                         r.stdout, flags=re.M):
        seen[(name, int(rr), int(mode))] = int(nf)
    for name, slab in (("lbm_regtile", 0), ("lbm_regtile_slabs", 8192)):
        for rr in (2, 4):
            for fast in (0, 1):
                key = (name, rr, 32768 | 131072 | 4096 | slab | fast)
                assert key in seen, (key, r.stdout)
                assert seen[key] == 0, (key, r.stdout)
    assert len(seen) >= 48 and all(nf == 0 for nf in seen.values()), r.stdout


def _tile_categories(nx, ny, ty, body_counted, xy):
    """per tile of 64 columns x ty rows: (holds a counted labelled cell, holds a probe)"""
    ntx, nty = nx // 64, ny // ty
    has_f = body_counted.reshape(nty, ty, ntx, 64).any(axis=(1, 3))
    has_p = np.zeros((nty, ntx), bool)
    for ii, jj in xy:
        has_p[jj // ty, ii // 64] = True
    return {(bool(has_f[j, i]), bool(has_p[j, i])) for j in range(nty) for i in range(ntx)}


def _counted(ob, body):
    """blocked labelled cells with a fluid cell among their eight neighbours (the lattice wraps): what the force tables hold"""
    fluid = ob == 0
    near = np.zeros(ob.shape, bool)
    for dy, dx in itertools.product((-1, 0, 1), repeat=2):
        if dy or dx:
            near |= np.roll(np.roll(fluid, dy, axis=0), dx, axis=1)
    return (ob != 0) & (body > 0) & near


ORDER = ((True, True), (False, True), (True, False), (False, False))     # tile t takes ORDER[t % 4]


def _tiling_case(L, ty, r, nx, ny):
    """Random lattice, four labels, and bodies / probes arranged tile by tile: tile t (row-major) holds labelled cells and
    probes as ORDER[t % 4] says; a tile with both has one probe ON a counted cell, so that one wave row holds both."""
    p, ob, cells, body = _random_case_with_bodies(L, nx, ny, 7)
    ntx, nty = nx // 64, ny // ty
    rng = np.random.default_rng(5)
    xy = []
    for t in range(ntx * nty):
        f, pr = ORDER[t % 4]
        j0, i0 = (t // ntx) * ty, (t % ntx) * 64
        if not f:
            body[j0:j0 + ty, i0:i0 + 64] = 0
        if pr:
            picks = {(i0 + int(rng.integers(64)), j0 + int(rng.integers(ty))) for _ in range(3)} | {(i0, j0), (i0 + 63, j0 + ty - 1)}
            if f:
                c = np.argwhere(_counted(ob, body)[j0:j0 + ty, i0:i0 + 64])
                assert len(c)
                picks.add((i0 + int(c[len(c) // 2][1]), j0 + int(c[len(c) // 2][0])))
            xy += sorted(picks)
    xy = np.array(xy, dtype=np.int32)
    xy = xy[rng.permutation(len(xy))]
    return p, ob, cells, body, xy


@pytest.mark.parametrize("ty,r,asy,nx,ny", TILINGS)
def test_the_tiling_cases_hold_every_kind_of_tile(L, ty, r, asy, nx, ny):
    """The inputs of test_forces_and_probes_of_every_register_tiling cannot silently degenerate: a tile with a counted cell
    and a probe, one with probes only, one with counted cells only, one with neither -- as many of these, in this order, as
    the tiling has tiles (two of the TILINGS have only two)."""
    p, ob, cells, body, xy = _tiling_case(L, ty, r, nx, ny)
    ntiles = (nx // 64) * (ny // ty)
    cats = _tile_categories(nx, ny, ty, _counted(ob, body), xy)
    assert cats == set(ORDER[:min(4, ntiles)]), (cats, ntiles)
    assert len(np.unique(xy, axis=0)) == len(xy)
    assert {int(v) for v in np.unique(body)} == {0, 1, 2, 3, 4}


# ---------------------------------------------------------------------------------------------------------------- GPU
_CACHE = {}


def _deck_case(L, deck):
    """deck, the walls-and-obstacle labelling (two bodies), the awkward probe set of its default tiling"""
    if deck not in _CACHE:
        p, ob = _deck(L, deck)
        ob = np.ascontiguousarray(ob, dtype=np.int32).reshape(p.ny, p.nx)
        ty, r = L.plan_tiles(p.nx, p.ny)
        _CACHE[deck] = (p, ob, _labellings(ob)[2][1], awkward_set(p.nx, p.ny, ob, ty, r))
    return _CACHE[deck]


def _cached_singles(L, key, *args, **kw):
    if key not in _CACHE:
        _CACHE[key] = _singles(L, *args, **kw)
    return _CACHE[key]


SUBSETS = [c for n in range(1, 5) for c in itertools.combinations(KINDS, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", SUBSETS, ids=["+".join(c) for c in SUBSETS])
def test_every_subset_gives_its_single_calls_outputs(gpu, kinds):
    """256 x 256 deck, register tiles, 23 steps, probes every step, means every 7, snapshots every 5."""
    L = gpu
    assert len(SUBSETS) == 15
    p, ob, body, xy = _deck_case(L, "256x256")
    nsteps = 23
    full = _cached_singles(L, "subsets", p, ob, None, nsteps, _want(KINDS), body, 2, xy)
    want = _want(kinds)
    res = _observed(L, p, ob, None, nsteps, want, body, 2, xy)
    ref = {k: v for k, v in full.items() if k in kinds or k in ("av_vels", "state")}
    _same(res, ref, kinds)
    _same_av(res, ref, kinds)
    assert res["info"]["engine_last"] == 3, res["info"]
    if len(kinds) > 1 and "probes" in kinds:
        assert int(res["info"]["observed_in_kernel"]) & 2
    if len(kinds) > 1 and "forces" in kinds:
        assert int(res["info"]["observed_in_kernel"]) & 1


@pytest.mark.gpu
@pytest.mark.parametrize("deck,nsteps", DECK_STEPS)
def test_forces_with_probes_ride_in_one_launch_on_the_shipped_decks(gpu, deck, nsteps):
    L = gpu
    p, ob, body, xy = _deck_case(L, deck)
    for every in (1, 3):
        want = _want(("forces", "probes"), probes_every=every)
        ref = _singles(L, p, ob, None, nsteps, want, body, 2, xy)
        res = _observed(L, p, ob, None, nsteps, want, body, 2, xy)
        assert res["info"] == {"engine_last": 3, "observed_in_kernel": 3, "observed_pieces": 1}, (deck, every, res["info"])
        _same(res, ref, (deck, every))
        _same_av(res, ref, (deck, every))


@pytest.mark.gpu
@pytest.mark.parametrize("ty,r,asy,nx,ny", TILINGS)
def test_forces_and_probes_of_every_register_tiling(gpu, ty, r, asy, nx, ny):
    L = gpu
    p, ob, cells, body, xy = _tiling_case(L, ty, r, nx, ny)
    nsteps = 11
    opts = (("regtile", ty * 10 + r), ("regtile_async", asy), ("engine", 3))
    for every in (1, 4):
        want = _want(("forces", "probes"), probes_every=every)
        ref = _singles(L, p, ob, cells, nsteps, want, body, 4, xy, opts)
        res = _observed(L, p, ob, cells, nsteps, want, body, 4, xy, opts)
        assert res["info"] == {"engine_last": 3, "observed_in_kernel": 3, "observed_pieces": 1}, res["info"]
        _same(res, ref, every)
        _same_av(res, ref, every)


@pytest.mark.gpu
def test_pieces_keep_the_probes_phase(gpu):
    """1024 x 1024, 13 steps, forces + probes every 4 + means every 6: pieces of 6, 6 and 1 steps, whose probe samples (after
    steps 4, 8, 12) fall 4, 2 and -- in the last piece -- no steps into them."""
    L = gpu
    p, ob, body, xy = _deck_case(L, "1024x1024")
    want = _want(("forces", "probes", "mean"), probes_every=4, mean_every=6)
    ref = _singles(L, p, ob, None, 13, want, body, 2, xy)
    res = _observed(L, p, ob, None, 13, want, body, 2, xy)
    info = res["info"]
    assert info["observed_pieces"] > 1 and int(info["observed_in_kernel"]) & 3 == 3 and info["engine_last"] == 3, info
    _same(res, ref)
    _same_av(res, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("time_block", [1, 2, 4, 6, 8])
def test_streaming_engines_give_the_single_calls_outputs(gpu, time_block):
    L = gpu
    p, ob, body, xy = _deck_case(L, "256x256")
    nsteps = 21
    opts = (("engine", 1), ("time_block", time_block))
    want = _want(KINDS)
    ref = _singles(L, p, ob, None, nsteps, want, body, 2, xy, opts)
    res = _observed(L, p, ob, None, nsteps, want, body, 2, xy, opts)
    assert res["info"]["observed_in_kernel"] == 0 and res["info"]["engine_last"] == 1, res["info"]
    _same(res, ref, time_block)
    # av_vels: the one-step kernel's where forces are wanted (tests/test_body_forces.py, the streaming-engine test)
    if time_block == 1:
        _same_av(res, ref)
    assert np.allclose(res["av_vels"], ref["av_vels"], rtol=2e-6, atol=0)


def _slab_check(L, res, ref_same, ref_one, scale):
    """ref_same: the single calls on the same kind of context; ref_one: on a lattice alone"""
    _same(res, ref_same)
    for name in ("probes", "mean", "fields"):
        assert np.array_equal(_bits(res[name]), _bits(ref_one[name])), name
    assert _close(res["forces"], ref_one["forces"], scale)
    assert np.array_equal(_bits(res["state"]), _bits(ref_one["state"]))
    assert np.allclose(res["av_vels"], ref_one["av_vels"], rtol=2e-6, atol=0)
    assert np.allclose(res["av_vels"], ref_same["av_vels"], rtol=2e-6, atol=0)
    if res["info"]["engine_last"] == 3:
        _same_av(res, ref_same)


@pytest.mark.gpu
@pytest.mark.parametrize("nslabs,exchange", [(2, "copy"), (4, "copy"), (2, "p2p"), (4, "p2p")])
def test_slabs_give_the_single_slab_outputs(gpu, nslabs, exchange):
    L = gpu
    p, ob, body, _ = _deck_case(L, "256x256")
    nsteps = 10
    xy = _slab_set(L, p, ob, nslabs)
    want = _want(KINDS, probes_every=3, mean_every=4, fields_every=5)
    _, scale, _, _ = _per_step(L, p, ob, None, body, 2, nsteps)
    ref_one = _singles(L, p, ob, None, nsteps, want, body, 2, xy)
    ex = L.EXCHANGE_COPY if exchange == "copy" else L.EXCHANGE_P2P
    kw = dict(nslabs=nslabs, devices=[0] * nslabs, exchange=ex)
    ref_same = _singles(L, p, ob, None, nsteps, want, body, 2, xy, **kw)
    res = _observed(L, p, ob, None, nsteps, want, body, 2, xy, **kw)
    _slab_check(L, res, ref_same, ref_one, scale)
    if exchange == "p2p":                # register tiles across slabs
        assert res["info"]["engine_last"] == 3 and int(res["info"]["observed_in_kernel"]) & 3 == 3, res["info"]


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["rccl", "p2p"])
def test_rank_context_ring_of_one_gives_the_single_slab_outputs(gpu, exchange):
    L = gpu
    p, ob, body, xy = _deck_case(L, "128x256")
    nsteps = 13
    want = _want(KINDS, probes_every=3, mean_every=4, fields_every=5)
    _, scale, _, _ = _per_step(L, p, ob, None, body, 2, nsteps)
    ref_one = _singles(L, p, ob, None, nsteps, want, body, 2, xy)
    os.environ["LBM_FORCE_EXCHANGE"] = "1"
    try:
        ex = L.EXCHANGE_RCCL if exchange == "rccl" else L.EXCHANGE_P2P

        def kw():                        # (one id per communicator)
            return dict(rank=0, nranks=1, device=0, exchange=ex, unique_id=L.rccl_unique_id())
        ref_same = _ring_singles(L, p, ob, nsteps, want, body, xy, kw)
        res = _observed(L, p, ob, None, nsteps, want, body, 2, xy, **kw())
    finally:
        del os.environ["LBM_FORCE_EXCHANGE"]
    _slab_check(L, res, ref_same, ref_one, scale)


def _ring_singles(L, p, ob, nsteps, want, body, xy, kw):
    """_singles for rank contexts: every context gets a communicator id of its own"""
    ref = {}
    with _open(L, p, ob, None, body, 2, xy, (), kw()) as lat:
        ref["av_vels"] = lat.run(nsteps)
        ref["state"] = lat.read_state()
    with _open(L, p, ob, None, body, 2, xy, (), kw()) as lat:
        _, ref["forces"] = lat.run_forces(nsteps)
    with _open(L, p, ob, None, body, 2, xy, (), kw()) as lat:
        _, ref["probes"] = lat.run_probes(nsteps, want["probes_every"])
    with _open(L, p, ob, None, body, 2, xy, (), kw()) as lat:
        _, ref["mean"] = lat.run_mean(nsteps, want["mean_every"])
    with _open(L, p, ob, None, body, 2, xy, (), kw()) as lat:
        _, ref["fields"] = lat.run_sampled(nsteps, want["fields_every"])
    return ref


# torch and the library share libamdhip64: torch is imported FIRST, in a child process of its own
_DEVICE_OUTPUT = r"""
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import advanced_hpc_lbm_amd as L
from test_observed_run import KINDS, _bits, _deck_case, _open, _singles, _want
p, ob, body, xy = _deck_case(L, "128x256")
nsteps = 12
want = _want(KINDS, probes_every=2, mean_every=5, fields_every=4)
refs = {{e: _singles(L, p, ob, None, nsteps, want, body, 2, xy, (("engine", e),)) for e in (0, 1)}}   # (the same options)
nan = float("nan")
def tensors():
    return dict(probes_out=torch.full((nsteps // 2, len(xy), 4), nan, dtype=torch.float32, device="cuda:0"),
                mean_out=torch.full((p.ny, p.nx, 4), nan, dtype=torch.float32, device="cuda:0"),
                fields_out=torch.full((nsteps // 4, p.ny, p.nx, 4), nan, dtype=torch.float32, device="cuda:0"))
def check(res, outs):
    torch.cuda.synchronize()
    for name, key in (("probes", "probes_out"), ("mean", "mean_out"), ("fields", "fields_out")):
        got = res[name]
        if key in outs:
            assert got is outs[key], name
            got = got.cpu().numpy()
        else:
            assert isinstance(got, np.ndarray), name
        assert np.array_equal(_bits(got), _bits(ref[name])), name
    assert isinstance(res["forces"], np.ndarray) and np.array_equal(_bits(res["forces"]), _bits(ref["forces"]))
    assert np.array_equal(_bits(res["av_vels"]), _bits(ref["av_vels"]))
for engine in (0, 1):
    ref = refs[engine]
    for keys in (("probes_out", "mean_out", "fields_out"), ("mean_out",), ("probes_out",), ("fields_out",)):
        outs = {{k: v for k, v in tensors().items() if k in keys}}
        with _open(L, p, ob, None, body, 2, xy, (("engine", engine),), {{}}) as lat:
            res = lat.run_observed(nsteps, **want, **outs)
            assert np.array_equal(_bits(lat.read_state()), _bits(ref["state"]))
            assert (lat.info("observed_in_kernel") == 3) == (engine == 0)
        if engine == 0:
            check(res, outs)
        else:                                            # (the streaming engines' av_vels: within rounding, see the engine test)
            ref_av, ref["av_vels"] = ref["av_vels"], res["av_vels"]
            check(res, outs)
            ref["av_vels"] = ref_av
            assert np.allclose(res["av_vels"], ref_av, rtol=2e-6, atol=0)
print("device output ok")
"""


@pytest.mark.gpu
def test_device_output_is_the_host_output(gpu):
    assert "device output ok" in _child(_DEVICE_OUTPUT)


@pytest.mark.gpu
def test_refusals_leave_the_lattice_alone(gpu):
    L = gpu
    lib = L.load_library()
    p, ob, body, xy = _deck_case(L, "128x128")
    n = 10
    F = np.zeros((n, 2, 2), np.float32)
    P = np.zeros((n, len(xy), 4), np.float32)
    M = np.zeros((p.ny, p.nx, 4), np.float32)
    S = np.zeros((n, p.ny, p.nx, 4), np.float32)

    def obs(forces=None, probes=None, mean=None, fields=None, pe=1, me=1, fe=1):
        w = L.Observe()
        w.forces = forces.ctypes.data if forces is not None else None
        w.probes_out = probes.ctypes.data if probes is not None else None
        w.mean_out = mean.ctypes.data if mean is not None else None
        w.fields_out = fields.ctypes.data if fields is not None else None
        w.probes_every, w.mean_every, w.fields_every = pe, me, fe
        return w

    def refused(lat, nsteps, w, *words):
        before = lat.read_state()
        tag = lat.info("regtile_tag")
        assert lib.lbm_run_observed(lat._ctx, nsteps, None, C.byref(w)) == LBM_EINVAL
        msg = lib.lbm_last_error().decode()
        for word in words:
            assert word in msg, (word, msg)
        assert lat.info("regtile_tag") == tag                      # nothing was queued
        assert np.array_equal(_bits(lat.read_state()), _bits(before))

    with L.Lattice(p, ob) as lat:
        lat.run(3)
        refused(lat, n, obs(forces=F, mean=M), "bodies")
        refused(lat, n, obs(probes=P, mean=M), "probes")
        lat.set_bodies(body, 2)
        lat.set_probes(xy)
        refused(lat, -1, obs(forces=F, probes=P), "nsteps")
        refused(lat, -1, obs(), "nsteps")
        for bad in (0, -1):
            refused(lat, n, obs(forces=F, probes=P, pe=bad), "probes_every")
            refused(lat, n, obs(forces=F, mean=M, me=bad), "mean_every")
        refused(lat, n, obs(forces=F, probes=P, pe=n + 1), "probes_every", "nsteps")
        refused(lat, n, obs(forces=F, mean=M, me=n + 1), "mean_every")
        refused(lat, n, obs(forces=F, fields=S, fe=-1), "fields_every")
        assert not F.any() and not P.any() and not M.any() and not S.any()
        # fields_every = 0, or no sample step: legal, nothing written
        for fe in (0, n + 1):
            S[:] = 7.0
            av = np.zeros(n, np.float32)
            assert lib.lbm_run_observed(lat._ctx, n, av.ctypes.data, C.byref(obs(forces=F, fields=S, fe=fe))) == 0
            assert np.all(S == 7.0)
        st = lat.read_state()
    with L.Lattice(p, ob) as ref:
        ref.set_bodies(body, 2)
        ref.run(3 + n)
        av_ref, F_ref = ref.run_forces(n)
        assert np.array_equal(_bits(st), _bits(ref.read_state()))
        assert np.array_equal(_bits(av), _bits(av_ref)) and np.array_equal(_bits(F), _bits(F_ref))
    # what = NULL and all four NULL: exactly lbm_run
    av0 = None
    for w in (None, obs()):
        with L.Lattice(p, ob) as lat:
            av = np.zeros(n, np.float32)
            assert lib.lbm_run_observed(lat._ctx, n, av.ctypes.data, C.byref(w) if w is not None else None) == 0
            assert lat.info("observed_pieces") == 1 and lat.info("observed_in_kernel") == 0
            st = lat.read_state()
        if av0 is None:
            with L.Lattice(p, ob) as ref:
                av0, st0 = ref.run(n), ref.read_state()
        assert np.array_equal(_bits(av), _bits(av0)) and np.array_equal(_bits(st), _bits(st0))


# One context, many calls.  Each entry: (call, arguments); "observed": (nsteps, kinds, probes_every, mean_every, fields_every).
def _program(lone):
    return [("run", 7),
            ("observed", 12, ("forces", "probes"), 2, 0, 0),
            ("bodies", 1),                                           # relabel: the obstacle alone, one body
            ("option", ("regtile", 82) if lone else ("regtile_async", 0)),
            ("observed", 11, KINDS, 3, 4, 5),
            ("probes", 9, 2),
            ("observed", 10, ("probes", "mean"), 1, 3, 0),
            ("observed", 6, ("forces", "fields"), 0, 0, 2)]


def test_the_programs_cover_what_they_claim():
    for lone in (True, False):
        prog = _program(lone)
        names = [c[0] for c in prog]
        assert names[:2] == ["run", "observed"] and names.count("observed") >= 3
        assert names.index("bodies") < names.index("option") < len(names) - 1 - names[::-1].index("observed")
        i = names.index("probes")
        assert "observed" in names[:i] and "observed" in names[i + 1:]
        kinds = {c[2] for c in prog if c[0] == "observed"}
        assert ("forces", "probes") in kinds and KINDS in kinds      # one launch; every observer in pieces


@pytest.mark.gpu
@pytest.mark.parametrize("lone", [True, False], ids=["lone", "p2p-slabs"])
def test_one_context_through_many_calls(gpu, lone):
    """The context under test runs the program; a twin runs lbm_run of the same lengths under the same options (lattice and
    av_vels after every call); the outputs of every run_observed come from the single calls on fresh contexts brought to the
    same step with the same options, bodies and probes."""
    L = gpu
    p, ob, both, xy = _deck_case(L, "128x256")
    kw = {} if lone else dict(nslabs=2, devices=[0, 0], exchange=L.EXCHANGE_P2P)
    labellings = {2: both, 1: _labellings(ob)[0][1]}
    body, nb, options, t = both, 2, [], 0
    twin_results = []
    with L.Lattice(p, ob, **kw) as twin:                 # (one context at a time: the twin first, alone)
        for call in _program(lone):
            if call[0] == "option":
                twin.set_option(*call[1])
            elif call[0] != "bodies":
                twin_results.append((twin.run(call[1]), twin.read_state(), twin.info("regtile_tag")))
    twin_results.reverse()
    with _open(L, p, ob, None, body, nb, xy, (), kw) as lat:
        for step, call in enumerate(_program(lone)):
            if call[0] == "bodies":
                nb = call[1]
                body = labellings[nb]
                lat.set_bodies(body, nb)
                continue
            if call[0] == "option":
                options.append(call[1])
                lat.set_option(*call[1])
                continue
            n = call[1]
            if call[0] == "run":
                av = lat.run(n)
            elif call[0] == "probes":
                av, pr = lat.run_probes(n, call[2])
                ref = _singles(L, p, ob, None, n, _want(("probes",), call[2]), body, nb, xy, options, skip=t, **kw)
                assert np.array_equal(_bits(pr), _bits(ref["probes"])), step
            else:
                want = _want(call[2], *call[3:])
                res = lat.run_observed(n, **want)
                av = res["av_vels"]
                res["state"] = lat.read_state()
                assert lat.info("engine_last") == 3, step
                ref = _singles(L, p, ob, None, n, want, body, nb, xy, options, skip=t, **kw)
                _same(res, ref, step)
                if len(call[2]) > 1:
                    bits = (1 if "forces" in call[2] else 0) | (2 if "probes" in call[2] else 0)
                    assert int(lat.info("observed_in_kernel")) & 3 == bits, step
            av_t, st_t, tag_t = twin_results.pop()
            t += n
            assert np.array_equal(_bits(av), _bits(av_t)), step
            assert np.array_equal(_bits(lat.read_state()), _bits(st_t)), step
            assert lat.info("regtile_tag") >= tag_t > 1, step


@pytest.mark.gpu
def test_observed_run_against_the_float_oracle(gpu, O, oracle):
    """64 x 40 known-answer lattice, 50 steps, forces + probes every step + means every 5 in one call (pieces of 5 steps):
    the probes within the per-element bound of _oracle_fields of the strict float oracle's lattice at each step (the bar of
    tests/test_probe_run.py), the forces within _close of the numpy restatement on the per-step states (the bar of
    tests/test_body_forces.py)."""
    L = gpu
    k, p, ob, op = _kat_case(L, O)
    nsteps = 50
    ob2 = ob.reshape(p.ny, p.nx)
    body = (ob2 != 0).astype(np.int32)
    xy = _three_rows(p)
    want = _want(("forces", "probes", "mean"), probes_every=1, mean_every=5)
    res = _observed(L, p, ob, k["cells0"], nsteps, want, body, 1, xy)
    assert res["info"]["engine_last"] == 3 and int(res["info"]["observed_in_kernel"]) & 3 == 3, res["info"]
    assert res["info"]["observed_pieces"] == 10
    ref = k["cells0"].copy()
    for j in range(nsteps):
        oracle.run(op, ref, ob, 1)
        w, tol = _oracle_fields(ref.reshape(p.ny, p.nx, 9), ob, k["density"])
        err = np.abs(res["probes"][j].astype(np.float64) - w[xy[:, 1], xy[:, 0]])
        lim = tol[xy[:, 1], xy[:, 0]]
        if j % 10 == 9:
            print("step %d: max probe error %.3g, worst error - bound %.3g" % (j + 1, err.max(), np.max(err - lim)))
        assert np.all(err <= lim), (j, float(np.max(err - lim)))
        if j == 9:
            assert np.array_equal(ref, k["cells_after_10"])
    Fw, scale, _, st = _per_step(L, p, ob2, k["cells0"], body, 1, nsteps)
    print("max force error / scale %.3g" % float(np.max(np.abs(res["forces"] - Fw) / np.maximum(scale, 1e-30))))
    assert _close(res["forces"], Fw, scale)
    assert np.array_equal(_bits(res["state"]), _bits(st))
    with _open(L, p, ob, k["cells0"], None, 0, None, (), {}) as lat:
        _, mean = lat.run_mean(nsteps, 5)
    assert np.array_equal(_bits(res["mean"]), _bits(mean))
