"""ctypes front-end of the CPU oracle -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import
this module.  The product (advanced-hpc-lbm_amd/) never does.

It wraps
  * oracle/liblbm_oracle.so       -- our strict-IEEE restatement (float + double),
  * oracle/liblbm_oracle_fast.so  -- same source, reference Makefile flags (timing),
  * oracle/_ref/libd2q9_ref_strict.so -- the reference's own d2q9-bgk.c compiled
    with strict flags (only where oracle/Makefile could build it / it was shipped
    prebuilt); used to pin the restatement bit for bit,
and holds small numpy helpers for the reference's text formats
(/root/reference/d2q9-bgk.c:2736-2762 params, 2844-2857 obstacles,
2978/2993 output lines).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class OrcParam(C.Structure):
    """Mirror of orc_param in lbm_oracle.c (doubles: cast per flavour in C)."""
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("maxIters", C.c_int),
                ("reynolds_dim", C.c_int), ("density", C.c_double),
                ("accel", C.c_double), ("omega", C.c_double)]


class RefParam(C.Structure):
    """Mirror of the reference's t_param (d2q9-bgk.c:64-73)."""
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("maxIters", C.c_int),
                ("reynolds_dim", C.c_int), ("density", C.c_float),
                ("accel", C.c_float), ("omega", C.c_float)]


def build(quiet: bool = True) -> None:
    """(Re)build the oracle libraries and, where /root/reference exists, oracle/_ref."""
    subprocess.run(["make", "-C", HERE, "all"], check=True,
                   stdout=subprocess.DEVNULL if quiet else None)


_libs: dict = {}


def _load(name: str):
    if name in _libs:
        return _libs[name]
    path = os.path.join(HERE, name)
    if not os.path.exists(path) and not name.startswith("_ref"):
        build()
    if not os.path.exists(path):
        return None
    lib = C.CDLL(path)
    _libs[name] = lib
    return lib


_F = {np.float32: ("f32", C.c_float), np.float64: ("f64", C.c_double)}


class Oracle:
    """dtype-generic handle on liblbm_oracle{,_fast}.so."""

    def __init__(self, flavour: str = "strict"):
        name = "liblbm_oracle.so" if flavour == "strict" else "liblbm_oracle_fast.so"
        self.lib = _load(name)
        if self.lib is None:
            raise RuntimeError(f"oracle library {name} could not be built")
        self.lib.orc_build_flavour.restype = C.c_char_p
        assert self.lib.orc_build_flavour().decode() == flavour
        for suf, ct in (("f32", C.c_float), ("f64", C.c_double)):
            for fn in ("orc_sweep_", "orc_timestep_", "orc_av_velocity_", "orc_reynolds_",
                       "orc_total_density_"):
                getattr(self.lib, fn + suf).restype = ct
            for fn in ("orc_init_cells_", "orc_accelerate_", "orc_run_", "orc_final_state_",
                       "orc_sweep_rows_", "orc_accelerate_row_"):
                getattr(self.lib, fn + suf).restype = None

    @staticmethod
    def _suf(dtype):
        return _F[np.dtype(dtype).type][0]

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(C.c_void_p)

    def init_cells(self, prm: OrcParam, dtype=np.float32) -> np.ndarray:
        cells = np.empty((prm.ny, prm.nx, 9), dtype=dtype)
        getattr(self.lib, "orc_init_cells_" + self._suf(dtype))(C.byref(prm), self._p(cells))
        return cells

    def accelerate(self, prm, cells, obstacles):
        getattr(self.lib, "orc_accelerate_" + self._suf(cells.dtype))(
            C.byref(prm), self._p(cells), self._p(obstacles))

    def sweep(self, prm, cells, tmp, obstacles) -> float:
        return getattr(self.lib, "orc_sweep_" + self._suf(cells.dtype))(
            C.byref(prm), self._p(cells), self._p(tmp), self._p(obstacles))

    def sweep_rows(self, prm, cells, tmp, obstacles, row_begin: int, row_end: int):
        """Sweep rows [row_begin, row_end) only -> (speed_sum, fluid_cells)."""
        ct = _F[np.dtype(cells.dtype).type][1]
        tot, cnt = ct(0), C.c_int(0)
        getattr(self.lib, "orc_sweep_rows_" + self._suf(cells.dtype))(
            C.byref(prm), self._p(cells), self._p(tmp), self._p(obstacles),
            C.c_int(row_begin), C.c_int(row_end), C.byref(tot), C.byref(cnt))
        return tot.value, cnt.value

    def accelerate_row(self, prm, cells, obstacles, row: int):
        getattr(self.lib, "orc_accelerate_row_" + self._suf(cells.dtype))(
            C.byref(prm), self._p(cells), self._p(obstacles), C.c_int(row))

    def timestep(self, prm, cells, tmp, obstacles) -> float:
        return getattr(self.lib, "orc_timestep_" + self._suf(cells.dtype))(
            C.byref(prm), self._p(cells), self._p(tmp), self._p(obstacles))

    def run(self, prm, cells, obstacles, nsteps: int) -> np.ndarray:
        """Advance `cells` in place by nsteps; returns av_vels[nsteps]."""
        assert cells.flags.c_contiguous and obstacles.dtype == np.int32
        tmp = np.empty_like(cells)
        av = np.empty(nsteps, dtype=cells.dtype)
        getattr(self.lib, "orc_run_" + self._suf(cells.dtype))(
            C.byref(prm), self._p(cells), self._p(tmp), self._p(obstacles),
            C.c_int(nsteps), self._p(av))
        return av

    def av_velocity(self, prm, cells, obstacles) -> float:
        return getattr(self.lib, "orc_av_velocity_" + self._suf(cells.dtype))(
            C.byref(prm), self._p(cells), self._p(obstacles))

    def reynolds(self, prm, cells, obstacles) -> float:
        return getattr(self.lib, "orc_reynolds_" + self._suf(cells.dtype))(
            C.byref(prm), self._p(cells), self._p(obstacles))

    def total_density(self, prm, cells) -> float:
        return getattr(self.lib, "orc_total_density_" + self._suf(cells.dtype))(
            C.byref(prm), self._p(cells))

    def final_state(self, prm, cells, obstacles) -> np.ndarray:
        """(ny, nx, 4) = u_x, u_y, |u|, pressure."""
        out = np.empty((prm.ny, prm.nx, 4), dtype=cells.dtype)
        getattr(self.lib, "orc_final_state_" + self._suf(cells.dtype))(
            C.byref(prm), self._p(cells), self._p(obstacles), self._p(out))
        return out


class ReferenceStrict:
    """The reference's own timestep_new2 / av_velocity (strict-flag build), if present."""

    def __init__(self):
        self.lib = _load(os.path.join("_ref", "libd2q9_ref_strict.so"))
        if self.lib is None:
            raise FileNotFoundError("oracle/_ref/libd2q9_ref_strict.so not built")
        vp = C.c_void_p
        self.lib.timestep_new2.restype = C.c_float
        self.lib.timestep_new2.argtypes = [RefParam, vp, vp, vp]
        self.lib.av_velocity.restype = C.c_float
        self.lib.av_velocity.argtypes = [RefParam, vp, vp]
        self.lib.calc_reynolds.restype = C.c_float
        self.lib.calc_reynolds.argtypes = [RefParam, vp, vp]

    @staticmethod
    def available() -> bool:
        return os.path.exists(os.path.join(HERE, "_ref", "libd2q9_ref_strict.so"))

    def timestep_new2(self, rp: RefParam, cells, tmp, obstacles) -> float:
        assert cells.dtype == np.float32 and obstacles.dtype == np.int32
        return self.lib.timestep_new2(rp, cells.ctypes.data, tmp.ctypes.data, obstacles.ctypes.data)

    def av_velocity(self, rp, cells, obstacles) -> float:
        return self.lib.av_velocity(rp, cells.ctypes.data, obstacles.ctypes.data)

    def calc_reynolds(self, rp, cells, obstacles) -> float:
        return self.lib.calc_reynolds(rp, cells.ctypes.data, obstacles.ctypes.data)



# ---------------------------------------------------------------- row bands and chunks
# One D2Q9 step of a row reads only the rows either side of it, so K steps of rows [j0, j1) depend on rows
# [j0 - K, j1 + K) alone.  Those rows, treated as a periodic lattice of their own, advance rows [j0, j1) exactly as the
# whole lattice would: the wrong values the band's own wrap brings in move one row per step and reach row j0 - K + K =
# j0 only after K steps.  The cell arithmetic is the oracle's (orc_sweep_rows_ / orc_accelerate_row_), so a band equals
# Oracle.run of the whole lattice bit for bit, in either flavour, for a cost that does not grow with ny.

def band_rows(ny: int, j0: int, j1: int, K: int) -> np.ndarray:
    """Global rows j0 - K .. j1 + K - 1, wrapped into [0, ny)."""
    return np.arange(j0 - K, j1 + K) % ny


def band_param(prm: OrcParam, rows: int) -> OrcParam:
    return OrcParam(prm.nx, rows, prm.maxIters, prm.reynolds_dim, prm.density, prm.accel, prm.omega)


def _oracle_for(dtype):
    if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("dtype must be float32 (the strict float oracle) or float64")
    return Oracle("strict")


def run_band(prm: OrcParam, cells: np.ndarray, obstacles: np.ndarray, j0: int, j1: int, K: int,
             dtype=np.float64) -> np.ndarray:
    """Rows [j0, j1) (taken modulo ny; 0 <= j0 < ny, j0 < j1 <= j0 + ny) of the lattice `cells` (ny, nx, 9) after K
    steps of the strict oracle in `dtype` (float32: the reference's float arithmetic; float64: the double oracle from
    the same float input).  Only rows j0 - K .. j1 + K - 1 are read and stepped; where those would cover the lattice
    the whole lattice is run instead.  Returns (j1 - j0, nx, 9) in `dtype`."""
    ny, nx = prm.ny, prm.nx
    if not (0 <= j0 < ny and j0 < j1 <= j0 + ny and K >= 0):
        raise ValueError(f"band [{j0}, {j1}) of {K} steps on {ny} rows")
    orc = _oracle_for(dtype)
    out_rows = np.arange(j0, j1) % ny
    if 2 * K + (j1 - j0) >= ny:
        a = np.ascontiguousarray(cells, dtype=dtype).copy()
        if K:
            orc.run(prm, a, np.ascontiguousarray(obstacles, dtype=np.int32), K)
        return a[out_rows]
    rows = band_rows(ny, j0, j1, K)
    a = np.ascontiguousarray(cells[rows], dtype=dtype)
    b = np.empty_like(a)
    ob = np.ascontiguousarray(obstacles[rows], dtype=np.int32)
    bp = band_param(prm, len(rows))
    acc = np.nonzero(rows == ny - 2)[0]          # the accelerate row, where the band holds it (at most once here)
    for _ in range(K):
        for r in acc:
            orc.accelerate_row(bp, a, ob, int(r))
        orc.sweep_rows(bp, a, b, ob, 0, len(rows))
        a, b = b, a
    return a[K:K + (j1 - j0)].copy()


def run_band_steps(prm: OrcParam, cells: np.ndarray, obstacles: np.ndarray, j0: int, j1: int, nsteps: int,
                   dtype=np.float64):
    """run_band after EVERY step: yields (t, rows [j0, j1) after step t) for t = 1 .. nsteps, each (j1 - j0, nx, 9) in
    `dtype` and the caller's own (a copy), each what run_band(..., K = t, ...) returns, from ONE run of rows
    j0 - nsteps .. j1 + nsteps - 1 (the same wrap, accelerate row and whole-lattice fall-back as run_band): after step t
    the band's own wrap has spoilt t rows at either end, never rows [j0, j1).  So a series over the steps -- forces,
    probes -- costs one band run, not nsteps of them."""
    ny = prm.ny
    if not (0 <= j0 < ny and j0 < j1 <= j0 + ny and nsteps >= 0):
        raise ValueError(f"band [{j0}, {j1}) of {nsteps} steps on {ny} rows")
    orc = _oracle_for(dtype)
    if 2 * nsteps + (j1 - j0) >= ny:
        out_rows = np.arange(j0, j1) % ny
        a = np.ascontiguousarray(cells, dtype=dtype).copy()
        ob = np.ascontiguousarray(obstacles, dtype=np.int32)
        for t in range(1, nsteps + 1):
            orc.run(prm, a, ob, 1)
            yield t, a[out_rows]
        return
    rows = band_rows(ny, j0, j1, nsteps)
    a = np.ascontiguousarray(cells[rows], dtype=dtype)
    b = np.empty_like(a)
    ob = np.ascontiguousarray(obstacles[rows], dtype=np.int32)
    bp = band_param(prm, len(rows))
    acc = np.nonzero(rows == ny - 2)[0]
    for t in range(1, nsteps + 1):
        for r in acc:
            orc.accelerate_row(bp, a, ob, int(r))
        orc.sweep_rows(bp, a, b, ob, 0, len(rows))
        a, b = b, a
        yield t, a[nsteps:nsteps + (j1 - j0)].copy()


# directions 1..8: E N W S NE NW SW SE (index 0: rest), and the direction opposite to each
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])
OPP = np.array([0, 3, 4, 1, 2, 7, 8, 5, 6])


def band_forces(rows: np.ndarray, obstacles_ext: np.ndarray, body: np.ndarray, nbodies: int) -> dict:
    """The force definition of include/lbm_mi355x.h on a window of rows, in plain numpy float64:
        F_b = 2 sum over the blocked cells B of label b, over the directions i whose source cell B - c_i is fluid, of
              c_i f_opp(i)(B)
    rows: the stored lattice in the window (h, nx, 9), any float type; obstacles_ext: the obstacle rows of the window
    AND one row either side (h + 2, nx) -- whether B - c_i is fluid is asked of the row below and the row above;
    body: the labels in the window (h, nx), 0 = not counted (labels on fluid cells are ignored).  Columns wrap.  The
    whole lattice is the window [0, ny) with obstacles_ext = obstacles[arange(-1, ny + 1) % ny].  Returns, per body b
    (index b - 1) and where it applies per component k (x, y):
      F[nb, 2]        the force;
      A[nb, 2]        2 sum |c_ik| |f_opp(i)(B)| over the counted links: the scale of any float32 evaluation's rounding;
      links[nb, 2]    sum |c_ik| over the counted links (how far an error of every population can move F / 2);
      cells[nb]       the counted cells: labelled b, blocked, with at least one fluid source;
      min_link[nb]    the smallest |2 f_opp(i)(B)| of any counted link (inf where there is none)."""
    lat = np.asarray(rows)
    h, nx = lat.shape[:2]
    blocked = np.asarray(obstacles_ext) != 0
    if blocked.shape != (h + 2, nx) or np.shape(body) != (h, nx):
        raise ValueError("obstacles_ext must hold the window's rows and one row either side; body the window's rows")
    label = np.where(blocked[1:-1], np.asarray(body), 0).astype(np.int64)
    if label.min(initial=0) < 0 or label.max(initial=0) > nbodies:
        raise ValueError("labels must lie in [0, nbodies]")
    F, A, links = (np.zeros((nbodies, 2)) for _ in range(3))
    min_link = np.full(nbodies, np.inf)
    counted = np.zeros((h, nx), bool)
    for i in range(1, 9):
        src_fluid = np.roll(~blocked[1 - CY[i]:1 - CY[i] + h], CX[i], axis=1)      # [y, x] = fluid at (x - cx, y - cy)
        lab = np.where(src_fluid, label, 0).ravel()
        counted |= (lab > 0).reshape(h, nx)
        v = lat[..., OPP[i]].astype(np.float64).ravel()
        c = np.array([CX[i], CY[i]], dtype=np.float64)
        s = np.bincount(lab, weights=v, minlength=nbodies + 1)[1:nbodies + 1]
        a = np.bincount(lab, weights=np.abs(v), minlength=nbodies + 1)[1:nbodies + 1]
        n = np.bincount(lab, minlength=nbodies + 1)[1:nbodies + 1]
        F += 2.0 * s[:, None] * c
        A += 2.0 * a[:, None] * np.abs(c)
        links += n[:, None] * np.abs(c)
        on = lab > 0
        if on.any():
            m = np.full(nbodies + 1, np.inf)
            np.minimum.at(m, lab[on], 2.0 * np.abs(v[on]))
            min_link = np.minimum(min_link, m[1:])
    cells = np.bincount(label[counted], minlength=nbodies + 1)[1:nbodies + 1]
    return dict(F=F, A=A, links=links, cells=cells, min_link=min_link)


def step_chunks(prm: OrcParam, cells: np.ndarray, obstacles: np.ndarray, rows_per_chunk: int, dtype=np.float64):
    """One whole-lattice step (accelerate + sweep) of the strict oracle in `dtype`, chunk by chunk: yields
    (r0, r1, new rows [r0, r1) as (r1 - r0, nx, 9) in dtype, speed sum of the chunk, fluid cells of the chunk).  Each
    chunk reads its rows and one row either side; nothing lattice-sized is allocated.  The speed sum adds up the rows' sums
    (each in dtype, over nx cells) in double, so that in float it carries the rounding of one row's sum, not of a lattice's."""
    ny = prm.ny
    if rows_per_chunk < 1:
        raise ValueError("rows_per_chunk must be >= 1")
    orc = _oracle_for(dtype)
    for r0 in range(0, ny, rows_per_chunk):
        r1 = min(ny, r0 + rows_per_chunk)
        rows = band_rows(ny, r0, r1, 1)
        a = np.ascontiguousarray(cells[rows], dtype=dtype)
        b = np.empty_like(a)
        ob = np.ascontiguousarray(obstacles[rows], dtype=np.int32)
        bp = band_param(prm, len(rows))
        for r in np.nonzero(rows == ny - 2)[0]:   # in a halo row, or the chunk's own (or both, on a lattice of few rows)
            orc.accelerate_row(bp, a, ob, int(r))
        tot, cnt = 0.0, 0
        for r in range(1, len(rows) - 1):         # (a row's speeds summed in dtype, the rows in double)
            t, n = orc.sweep_rows(bp, a, b, ob, r, r + 1)
            tot += float(t)
            cnt += n
        yield r0, r1, b[1:len(rows) - 1], tot, cnt


def step_chunked(prm: OrcParam, cells: np.ndarray, obstacles: np.ndarray, rows_per_chunk: int, dtype=np.float64,
                 visit=None):
    """step_chunks gathered: (new lattice in dtype -- or None where `visit(r0, r1, rows)` takes each chunk instead --,
    speed sum over all fluid cells added up in double, fluid cells).  speed sum / fluid cells is the step's av_vels
    entry; in float64 it is the double oracle's up to the order of the double additions."""
    out = None if visit is not None else np.empty(cells.shape, dtype=dtype)
    tot, cnt = 0.0, 0
    for r0, r1, new, t, n in step_chunks(prm, cells, obstacles, rows_per_chunk, dtype):
        if visit is None:
            out[r0:r1] = new
        else:
            visit(r0, r1, new)
        tot += t
        cnt += n
    return out, tot, cnt


def av_velocity_chunked(prm: OrcParam, cells: np.ndarray, obstacles: np.ndarray, rows_per_chunk: int):
    """(speed sum, fluid cells) of the lattice `cells` as the double oracle's av_velocity sees it, chunk by chunk:
    sum / cells is its av_velocity up to the order of the double additions."""
    orc = Oracle("strict")
    tot, cnt = 0.0, 0
    for r0 in range(0, prm.ny, rows_per_chunk):
        r1 = min(prm.ny, r0 + rows_per_chunk)
        ob = np.ascontiguousarray(obstacles[r0:r1], dtype=np.int32)
        n = int((ob == 0).sum())
        if n:
            tot += orc.av_velocity(band_param(prm, r1 - r0), np.ascontiguousarray(cells[r0:r1], dtype=np.float64), ob) * n
            cnt += n
    return tot, cnt


# ---------------------------------------------------------------- text formats

def read_params(path: str) -> OrcParam:
    """7 whitespace-separated tokens: nx ny maxIters reynolds_dim density accel omega."""
    tok = open(path).read().split()
    if len(tok) < 7:
        raise ValueError(f"could not read param file: {path}")
    return OrcParam(int(tok[0]), int(tok[1]), int(tok[2]), int(tok[3]),
                    float(tok[4]), float(tok[5]), float(tok[6]))


def to_ref_param(prm: OrcParam) -> RefParam:
    return RefParam(prm.nx, prm.ny, prm.maxIters, prm.reynolds_dim,
                    prm.density, prm.accel, prm.omega)


def read_obstacles(path: str, nx: int, ny: int) -> np.ndarray:
    """Lines 'x y 1' -> int32 (ny, nx) 0/1 map, with the reference's range checks."""
    obst = np.zeros((ny, nx), dtype=np.int32)
    data = np.loadtxt(path, dtype=np.int64, ndmin=2)
    if data.size:
        if data.shape[1] != 3:
            raise ValueError("expected 3 values per line in obstacle file")
        x, y, b = data[:, 0], data[:, 1], data[:, 2]
        if (x < 0).any() or (x > nx - 1).any():
            raise ValueError("obstacle x-coord out of range")
        if (y < 0).any() or (y > ny - 1).any():
            raise ValueError("obstacle y-coord out of range")
        if (b != 1).any():
            raise ValueError("obstacle blocked value should be 1")
        obst[y, x] = 1
    return obst


def read_av_vels(path: str) -> np.ndarray:
    return np.loadtxt(path, usecols=[1])


def read_final_state(path: str) -> np.ndarray:
    """Columns x y u_x u_y u pressure flag -> float64 (n, 7)."""
    return np.loadtxt(path)


def format_av_vels(av) -> str:
    """'%d:\\t%.12E\\n' per step (d2q9-bgk.c:2993)."""
    return "".join("%d:\t%.12E\n" % (i, float(v)) for i, v in enumerate(av))


def format_final_state(fs: np.ndarray, obstacles: np.ndarray) -> str:
    """'%d %d %.12E %.12E %.12E %.12E %d\\n' per cell, jj outer / ii inner (d2q9-bgk.c:2978);
    flag column = obstacles[jj, ii] as in the shipped goldens."""
    ny, nx = obstacles.shape
    lines = []
    for jj in range(ny):
        row = fs[jj]
        ob = obstacles[jj]
        for ii in range(nx):
            lines.append("%d %d %.12E %.12E %.12E %.12E %d\n" % (
                ii, jj, row[ii, 0], row[ii, 1], row[ii, 2], row[ii, 3], ob[ii]))
    return "".join(lines)
