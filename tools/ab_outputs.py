#!/usr/bin/env python3
"""A/B of two builds of the library by their OUTPUTS: the same cases in one process per build (LBM_MI355X_LIB picks it),
every output hashed, every entry compared.  For refactors of the host code that must leave every bit where it was.

    python tools/ab_outputs.py parent/liblbm_mi355x.so advanced-hpc-lbm_amd/liblbm_mi355x.so [--json out.json]

An entry is one call on one context: sha256 over av_vels, read_state, the forces, the text of a failure (code and
lbm_last_error) and the info keys engine_last, time_block_active, march_kernel, exchange.  Cases: streaming engine on
  * 256 x 64, random obstacles and state: alone, 2 slabs with copies and peer-to-peer, rank rings of one (RCCL, peer-to-peer);
  * the 1024x1024 deck on 4 and 8 slabs and the 128x256 deck on 2, copies and peer-to-peer;
  * thin slabs, 64 wide: (ny, nslabs) = (8, 8), (9, 4), (6, 2);
  * time_block 1, 2, 4, 8 (a refusal is an entry too), step counts 1, 2, 3, K, K + 1, 2 K + 3 (K: the active time block);
  * run, run_forces (one body across the first slab border) and run_driven (a schedule of entries that all differ);
  * what lbm_create and lbm_create_rank_ex refuse.
Exit status 0: every entry equal."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO = ("engine_last", "time_block_active", "march_kernel", "exchange")


def _random_case(L, nx, ny, seed):
    rng = np.random.default_rng(seed)
    p = L.Param(nx, ny, 100, 10, 0.1, 0.01, 1.85)
    ob = (rng.random((ny, nx)) < 0.1).astype(np.int32)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float32)
    cells = (0.1 * w * (1.0 + 0.2 * (rng.random((ny, nx, 9), dtype=np.float32) - 0.5))).astype(np.float32)
    return p, ob, cells


def _contexts(L):
    """(name, params, obstacles, cells or None, Lattice keywords, force LBM_FORCE_EXCHANGE)"""
    out = []
    p, ob, cells = _random_case(L, 256, 64, 21)
    out.append(("256x64 alone", p, ob, cells, {}, False))
    for name, ex in (("copy", L.EXCHANGE_COPY), ("p2p", L.EXCHANGE_P2P)):
        out.append((f"256x64 2 slabs {name}", p, ob, cells, dict(nslabs=2, devices=[0, 0], exchange=ex), False))
    for name, ex in (("rccl", L.EXCHANGE_RCCL), ("p2p", L.EXCHANGE_P2P)):
        out.append((f"256x64 ring of one {name}", p, ob, cells, dict(rank=0, nranks=1, device=0, unique_id=True, exchange=ex), True))
    for deck, slabs in (("1024x1024", (4, 8)), ("128x256", (2,))):
        dp = L.read_params(os.path.join(ROOT, f"input_{deck}.params"))
        dob = L.read_obstacles(os.path.join(ROOT, f"obstacles_{deck}.dat"), dp)
        for n in slabs:
            for name, ex in (("copy", L.EXCHANGE_COPY), ("p2p", L.EXCHANGE_P2P)):
                out.append((f"{deck} {n} slabs {name}", dp, dob, None, dict(nslabs=n, devices=[0] * n, exchange=ex), False))
    for ny, n in ((8, 8), (9, 4), (6, 2)):
        p, ob, cells = _random_case(L, 64, ny, 100 + ny)
        for name, ex in (("copy", L.EXCHANGE_COPY), ("p2p", L.EXCHANGE_P2P)):
            out.append((f"64x{ny} {n} slabs {name}", p, ob, cells, dict(nslabs=n, devices=[0] * n, exchange=ex), False))
    return out


def _digest(*parts):
    h = hashlib.sha256()
    for x in parts:
        h.update(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else repr(x).encode())
        h.update(b"|")
    return h.hexdigest()


def _refusals(L, entries):
    lib = L.load_library()
    p, ob, cells = _random_case(L, 64, 8, 5)
    obp, ctx = ob.ctypes.data, C.c_void_p()
    uid = L.rccl_unique_id()
    ndev = L.device_count()
    pp = C.byref(p)
    bad = L.Param(0, 8, 100, 10, 0.1, 0.01, 1.85)
    two = (C.c_int * 2)(0, ndev + 3)
    calls = {
        "create: out NULL": lambda: lib.lbm_create(pp, obp, None, 1, None, 0, None),
        "create: params NULL": lambda: lib.lbm_create(None, obp, None, 1, None, 0, C.byref(ctx)),
        "create: bad lattice": lambda: lib.lbm_create(C.byref(bad), obp, None, 1, None, 0, C.byref(ctx)),
        "create: obstacles NULL": lambda: lib.lbm_create(pp, None, None, 1, None, 0, C.byref(ctx)),
        "create: nslabs 0": lambda: lib.lbm_create(pp, obp, None, 0, None, 0, C.byref(ctx)),
        "create: nslabs > ny": lambda: lib.lbm_create(pp, obp, None, 9, None, 0, C.byref(ctx)),
        "create: exchange 7": lambda: lib.lbm_create(pp, obp, None, 1, None, 7, C.byref(ctx)),
        "create: exchange -1": lambda: lib.lbm_create(pp, obp, None, 1, None, -1, C.byref(ctx)),
        "create: device out of range": lambda: lib.lbm_create(pp, obp, None, 2, two, L.EXCHANGE_COPY, C.byref(ctx)),
        "create: p2p, one row per slab": lambda: lib.lbm_create(pp, obp, None, 8, None, L.EXCHANGE_P2P, C.byref(ctx)),
        "create: p2p, one row per slab, bad device": lambda: lib.lbm_create(pp, obp, None, 8, (C.c_int * 8)(*([ndev] * 8)), L.EXCHANGE_P2P, C.byref(ctx)),
        "rank: out NULL": lambda: lib.lbm_create_rank_ex(pp, obp, None, 0, 1, 0, uid, L.EXCHANGE_RCCL, None),
        "rank: params NULL": lambda: lib.lbm_create_rank_ex(None, obp, None, 0, 1, 0, uid, L.EXCHANGE_RCCL, C.byref(ctx)),
        "rank: obstacles NULL": lambda: lib.lbm_create_rank_ex(pp, None, None, 0, 1, 0, uid, L.EXCHANGE_RCCL, C.byref(ctx)),
        "rank: rank 2 of 2": lambda: lib.lbm_create_rank_ex(pp, obp, None, 2, 2, 0, uid, L.EXCHANGE_RCCL, C.byref(ctx)),
        "rank: nranks > ny": lambda: lib.lbm_create_rank_ex(pp, obp, None, 0, 9, 0, uid, L.EXCHANGE_RCCL, C.byref(ctx)),
        "rank: exchange copy": lambda: lib.lbm_create_rank_ex(pp, obp, None, 0, 1, 0, uid, L.EXCHANGE_COPY, C.byref(ctx)),
        "rank: device out of range": lambda: lib.lbm_create_rank_ex(pp, obp, None, 0, 1, ndev + 3, uid, L.EXCHANGE_RCCL, C.byref(ctx)),
        "rank: device -1": lambda: lib.lbm_create_rank_ex(pp, obp, None, 0, 1, -1, uid, L.EXCHANGE_RCCL, C.byref(ctx)),
        "rank: unique_id NULL of 2": lambda: lib.lbm_create_rank_ex(pp, obp, None, 0, 2, 0, None, L.EXCHANGE_RCCL, C.byref(ctx)),
        "rank: p2p, one row per slab": lambda: lib.lbm_create_rank_ex(pp, obp, None, 0, 8, 0, None, L.EXCHANGE_P2P, C.byref(ctx)),
    }
    for name, call in calls.items():
        ctx.value = 12345                              # (a refusal that reaches `out` clears it)
        rc = call()
        entries["refusal / " + name] = _digest(rc, lib.lbm_last_error().decode(), ctx.value)
        if rc == 0:
            lib.lbm_destroy(ctx)


def child(out_path):
    sys.path.insert(0, ROOT)
    import advanced_hpc_lbm_amd as L
    entries = {}
    _refusals(L, entries)
    for name, p, ob, cells, kw, forced in _contexts(L):
        kw = dict(kw)
        if kw.get("unique_id"):
            kw["unique_id"] = L.rccl_unique_id()
        if forced:
            os.environ["LBM_FORCE_EXCHANGE"] = "1"
        try:
            lat = L.Lattice(p, ob, cells, **kw)
        except L.LbmError as e:
            entries[name + " / create"] = _digest(str(e))
            continue
        finally:
            os.environ.pop("LBM_FORCE_EXCHANGE", None)
        with lat:
            lat.set_option("engine", 1)
            start = lat.read_state()
            border = p.ny // kw.get("nslabs", 2)                       # the first slab border (two slabs where there is one)
            body = np.zeros((p.ny, p.nx), np.int32)
            body[[(border - 1) % p.ny, border % p.ny], :] = 1          # (labels count on blocked cells only)
            lat.set_bodies(body, 1)
            for tb in (1, 2, 4, 8):
                try:
                    lat.set_option("time_block", tb)
                except L.LbmError as e:
                    entries[f"{name} / time_block {tb}"] = _digest(str(e))
                    continue
                K = int(lat.info("time_block_active"))
                for n in sorted({1, 2, 3, K, K + 1, 2 * K + 3}):
                    sched = (np.float32(p.accel) * (1.0 + 0.05 * np.arange(1, n + 1))).astype(np.float32)
                    for call in ("run", "run_forces", "run_driven"):
                        lat.write_state(start)
                        out = []
                        try:
                            if call == "run":
                                out = [lat.run(n)]
                            elif call == "run_forces":
                                out = list(lat.run_forces(n))
                            else:
                                out = [lat.run_driven(sched)]
                            out.append(lat.read_state())
                        except L.LbmError as e:
                            out.append(str(e))
                        info = [(k, lat.info(k)) for k in INFO]
                        entries[f"{name} / time_block {tb} / {n} steps / {call}"] = _digest(*out, info)
    with open(out_path, "w") as f:                     # (not stdout: the libraries underneath may write there)
        json.dump(entries, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("libs", nargs="*", help="the builds to compare (two or more)")
    ap.add_argument("--json", help="write every build's entries here")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=420, help="seconds one build's process may take")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if len(a.libs) < 2:
        ap.error("give at least two builds")
    results = []
    for lib in a.libs:
        env = dict(os.environ, LBM_MI355X_LIB=os.path.abspath(lib))
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "entries.json")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, timeout=a.timeout)
            if r.returncode != 0:
                print(f"{lib}: the process ended with status {r.returncode}; nothing more is started", flush=True)
                return 2
            with open(out) as f:
                results.append(json.load(f))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(zip(a.libs, results)), f, indent=1)
    first, bad = results[0], 0
    for lib, other in zip(a.libs[1:], results[1:]):
        for key in sorted(set(first) | set(other)):
            if first.get(key) != other.get(key):
                bad += 1
                print(f"DIFFERS  {key}  ({a.libs[0]} against {lib})")
    print(f"{len(first)} entries per build, {len(a.libs)} builds: {'all equal' if not bad else str(bad) + ' differ'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
