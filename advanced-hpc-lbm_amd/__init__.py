"""advanced-hpc-lbm on MI355X: Python face of the C ABI (include/lbm_mi355x.h).

This package is plumbing for tests and bench.py: it binds
`liblbm_mi355x.so` (hand-written HIP kernels for gfx950 + the C ABI) with
ctypes and mirrors the names of the reference's own interface for the
time-step path (/root/reference/d2q9-bgk.c):

    t_param                      -> Param            (d2q9-bgk.c:64-73)
    initialise(param, obst)      -> initialise()     (d2q9-bgk.c:2716-2869)
    timestep_new2(...) + swap    -> timestep_new2()  (d2q9-bgk.c:98,182,190,228)
    main's step loop             -> Lattice.run()    (d2q9-bgk.c:180-201)
    av_velocity / calc_reynolds  -> Lattice.av_velocity() / .reynolds()
    write_values                 -> write_values()   (d2q9-bgk.c:2918-2999)

There is NO CPU fallback here: if the shared library is missing or no HIP
device is visible, loading / creating a lattice raises LbmError.  The CPU
oracle lives under oracle/ and is imported by tests only.

The directory name carries a hyphen, so `import advanced_hpc_lbm_amd` (the
one-file shim at the repo root) is the import path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LBM_MI355X_LIB") or os.path.join(_HERE, "liblbm_mi355x.so")   # (the override is for A/B timing of two builds)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lbm_mi355x.h")

NSPEEDS = 9
EXCHANGE_AUTO, EXCHANGE_COPY, EXCHANGE_RCCL, EXCHANGE_P2P = 0, 1, 2, 3
REFILL_KEEP, REFILL_REST = 0, 1      # lbm_set_obstacles

# every symbol include/lbm_mi355x.h declares
ABI_SYMBOLS = (
    "lbm_last_error", "lbm_device_count", "lbm_create", "lbm_rccl_unique_id", "lbm_create_rank",
    "lbm_create_rank_ex", "lbm_p2p_handle", "lbm_p2p_connect",
    "lbm_slab_rows", "lbm_num_slabs", "lbm_run", "lbm_run_sampled", "lbm_run_mean", "lbm_run_stats", "lbm_set_bodies", "lbm_run_forces",
    "lbm_set_probes", "lbm_run_probes", "lbm_run_observed", "lbm_run_window", "lbm_window_rows", "lbm_run_window_stats",
    "lbm_set_accel", "lbm_run_driven", "lbm_run_driven_observed",
    "lbm_last_run_ms", "lbm_read_state", "lbm_set_obstacles", "lbm_write_state",
    "lbm_av_velocity", "lbm_reynolds", "lbm_total_density", "lbm_final_state", "lbm_destroy",
    "lbm_timestep", "lbm_set_option", "lbm_get_info", "lbm_plan_tiles",
)


class LbmError(RuntimeError):
    pass


class Param(C.Structure):
    """Field-for-field the reference's t_param (d2q9-bgk.c:64-73) = lbm_param."""
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("maxIters", C.c_int),
                ("reynolds_dim", C.c_int), ("density", C.c_float),
                ("accel", C.c_float), ("omega", C.c_float)]

    def __repr__(self):
        return ("Param(nx=%d, ny=%d, maxIters=%d, reynolds_dim=%d, density=%g, accel=%g, omega=%g)"
                % (self.nx, self.ny, self.maxIters, self.reynolds_dim, self.density, self.accel, self.omega))


class Observe(C.Structure):
    """Field-for-field lbm_observe (include/lbm_mi355x.h): a NULL pointer = that observer is not wanted."""
    _fields_ = [("forces", C.c_void_p), ("probes_out", C.c_void_p), ("mean_out", C.c_void_p), ("fields_out", C.c_void_p),
                ("probes_every", C.c_int), ("mean_every", C.c_int), ("fields_every", C.c_int)]


class Window(C.Structure):
    """Field-for-field lbm_window (include/lbm_mi355x.h): the cells (x0 + c sx, y0 + r sy), c < nx, r < ny, of the global
    lattice.  Window(x0, y0, nx, ny) is a plain sub-rectangle (strides 1)."""
    _fields_ = [("x0", C.c_int), ("y0", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("sx", C.c_int), ("sy", C.c_int)]

    def __init__(self, x0=0, y0=0, nx=1, ny=1, sx=1, sy=1):
        super().__init__(x0, y0, nx, ny, sx, sy)

    def __repr__(self):
        return "Window(x0=%d, y0=%d, nx=%d, ny=%d, sx=%d, sy=%d)" % (self.x0, self.y0, self.nx, self.ny, self.sx, self.sy)


_lib = None


def load_library():
    """Loads liblbm_mi355x.so; raises LbmError if it has not been built.

    Import torch BEFORE calling this in a process that also uses torch: both
    link libamdhip64.so.7, and the first one loaded is the one shared.
    """
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LbmError(f"{LIB_PATH} is missing: run `make lib` (or __graft_entry__.build()); "
                       "there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    vp, ip, fp, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double)
    lib.lbm_last_error.restype = C.c_char_p
    lib.lbm_last_error.argtypes = []
    lib.lbm_device_count.argtypes = [ip]
    lib.lbm_create.argtypes = [C.POINTER(Param), vp, vp, C.c_int, vp, C.c_int, C.POINTER(vp)]
    lib.lbm_rccl_unique_id.argtypes = [vp]
    lib.lbm_create_rank.argtypes = [C.POINTER(Param), vp, vp, C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]
    lib.lbm_create_rank_ex.argtypes = [C.POINTER(Param), vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(vp)]
    lib.lbm_p2p_handle.argtypes = [vp, vp]
    lib.lbm_p2p_connect.argtypes = [vp, vp, C.c_int]
    lib.lbm_slab_rows.argtypes = [vp, C.c_int, ip, ip]
    lib.lbm_num_slabs.argtypes = [vp]
    lib.lbm_run.argtypes = [vp, C.c_int, vp]
    lib.lbm_run_sampled.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    lib.lbm_run_mean.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    lib.lbm_run_stats.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    lib.lbm_set_bodies.argtypes = [vp, vp, C.c_int]
    lib.lbm_set_probes.argtypes = [vp, vp, C.c_int]
    lib.lbm_run_probes.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    lib.lbm_run_forces.argtypes = [vp, C.c_int, vp, vp]
    lib.lbm_run_observed.argtypes = [vp, C.c_int, vp, C.POINTER(Observe)]
    lib.lbm_run_window.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(Window), vp]
    lib.lbm_run_window_stats.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(Window), vp]
    lib.lbm_window_rows.argtypes = [C.POINTER(Window), C.c_int, C.c_int, C.c_int, C.c_int, ip, ip]
    lib.lbm_set_accel.argtypes = [vp, C.c_float]
    lib.lbm_run_driven.argtypes = [vp, C.c_int, vp, vp]
    lib.lbm_run_driven_observed.argtypes = [vp, C.c_int, vp, vp, C.POINTER(Observe)]
    lib.lbm_last_run_ms.argtypes = [vp, dp, dp]
    lib.lbm_read_state.argtypes = [vp, vp]
    lib.lbm_set_obstacles.argtypes = [vp, vp, C.c_int]
    lib.lbm_write_state.argtypes = [vp, vp]
    lib.lbm_av_velocity.argtypes = [vp, fp]
    lib.lbm_reynolds.argtypes = [vp, fp]
    lib.lbm_total_density.argtypes = [vp, dp]
    lib.lbm_final_state.argtypes = [vp, vp]
    lib.lbm_destroy.argtypes = [vp]
    lib.lbm_timestep.argtypes = [C.POINTER(Param), vp, vp, vp, fp]
    lib.lbm_set_option.argtypes = [vp, C.c_char_p, C.c_long]
    lib.lbm_get_info.argtypes = [vp, C.c_char_p, dp]
    for name in ABI_SYMBOLS:
        if name != "lbm_last_error":
            getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


def _check(rc: int):
    if rc != 0:
        raise LbmError(f"[lbm error {rc}] {load_library().lbm_last_error().decode()}")


def plan_tiles(nx: int, rows: int, slabs_per_device: int = 1, compute_units: int = 256):
    """(rows per tile, rows per wavefront) of lbm_regtile's default tiling, or None where the lattice does not tile."""
    ty, r = C.c_int(0), C.c_int(0)
    rc = load_library().lbm_plan_tiles(nx, rows, slabs_per_device, compute_units, C.byref(ty), C.byref(r))
    return (ty.value, r.value) if rc == 0 else None


def window_rows(window: Window, nx: int, ny: int, row_begin: int, row_end: int):
    """(first, count): the rows first .. first + count - 1 of `window` lie in rows [row_begin, row_end) of an nx x ny
    lattice (lbm_window_rows: host arithmetic, no device).  Raises LbmError where the window is not legal there."""
    first, count = C.c_int(0), C.c_int(0)
    _check(load_library().lbm_window_rows(C.byref(window), nx, ny, row_begin, row_end, C.byref(first), C.byref(count)))
    return first.value, count.value


def device_count() -> int:
    n = C.c_int(0)
    _check(load_library().lbm_device_count(C.byref(n)))
    return n.value


def rccl_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _check(load_library().lbm_rccl_unique_id(buf))
    return buf.raw


def _as_obstacles(obstacles, p: Param) -> np.ndarray:
    ob = np.ascontiguousarray(obstacles, dtype=np.int32)
    if ob.size != p.nx * p.ny:
        raise LbmError(f"obstacles has {ob.size} entries, lattice has {p.nx * p.ny} cells")
    return ob


def _as_cells(cells, p: Param):
    if cells is None:
        return None
    a = np.ascontiguousarray(cells, dtype=np.float32)
    if a.size != p.nx * p.ny * NSPEEDS:
        raise LbmError(f"cells has {a.size} floats, expected {p.nx * p.ny * NSPEEDS}")
    return a


class Lattice:
    """A lattice resident on the GPU(s): handle on an lbm_ctx."""

    def __init__(self, params: Param, obstacles, cells=None, nslabs: int = 1, devices=None,
                 exchange: int = EXCHANGE_AUTO, *, rank=None, nranks=None, device=0, unique_id=None):
        self._lib = load_library()
        self.params = params
        self._ctx = C.c_void_p()
        ob = _as_obstacles(obstacles, params)
        ce = _as_cells(cells, params)
        cp = ce.ctypes.data if ce is not None else None
        if rank is None:
            dv = None
            if devices is not None:
                dv = np.ascontiguousarray(devices, dtype=np.int32)
                if dv.size != nslabs:
                    raise LbmError("devices must list one HIP device per slab")
            _check(self._lib.lbm_create(C.byref(params), ob.ctypes.data, cp, nslabs,
                                        dv.ctypes.data if dv is not None else None, exchange,
                                        C.byref(self._ctx)))
        else:
            idbuf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
            if exchange == EXCHANGE_AUTO:
                _check(self._lib.lbm_create_rank(C.byref(params), ob.ctypes.data, cp, rank, nranks, device,
                                                 idbuf, C.byref(self._ctx)))
            else:
                _check(self._lib.lbm_create_rank_ex(C.byref(params), ob.ctypes.data, cp, rank, nranks, device,
                                                    idbuf, exchange, C.byref(self._ctx)))
        self.rank_mode = rank is not None

    # -- peer-to-peer halos without RCCL: the caller trades the handles ------------
    def p2p_handle(self) -> bytes:
        buf = C.create_string_buffer(64)
        _check(self._lib.lbm_p2p_handle(self._ctx, buf))
        return buf.raw

    def p2p_connect(self, handles):
        """handles: the 64-byte handles of all ranks, in rank order."""
        blob = b"".join(handles)
        buf = C.create_string_buffer(blob, len(blob))
        _check(self._lib.lbm_p2p_connect(self._ctx, buf, len(handles)))

    # -- the step loop -----------------------------------------------------
    def run(self, nsteps: int) -> np.ndarray:
        """nsteps x (timestep_new2 + swap); returns av_vels[nsteps] (float32)."""
        av = np.empty(max(nsteps, 0), dtype=np.float32)
        _check(self._lib.lbm_run(self._ctx, nsteps, av.ctypes.data))
        return av

    def set_accel(self, accel: float):
        """Replaces the context's acceleration for every later run (lbm_set_accel): only the value is stored, nothing is
        queued; info("accel") reads it.  A non-finite value is refused and the old one kept.  `params` is the caller's and
        is not touched."""
        _check(self._lib.lbm_set_accel(self._ctx, float(accel)))

    def run_driven(self, accel) -> np.ndarray:
        """lbm_run with a per-step acceleration: step t of the call is driven by accel[t] instead of the context's value
        (a ramp, a pulsatile or oscillatory forcing, a controller's output); nsteps = len(accel); returns av_vels[nsteps].
        accel is anything np.asarray turns into a one-dimensional array of real numbers (converted to contiguous float32);
        every entry must be finite.  The lattice is bit-identical to `for a in accel: set_accel(a); run(1)`; the context's
        own acceleration is untouched.  The register tiles read the schedule inside their kernel
        (info("driven_in_kernel") == 1), a lattice alone under lbm_wave takes it in its launches
        (info("driven_in_wave") == 1); elsewhere the one-step kernel runs each step with its own constants."""
        arr = np.asarray(accel)
        if arr.ndim != 1:
            raise LbmError(f"accel must be one-dimensional (one value per step), got shape {arr.shape}")
        if arr.dtype.kind not in "fiu":
            raise LbmError(f"accel must hold real numbers, got dtype {arr.dtype}")
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        av = np.empty(arr.size, dtype=np.float32)
        _check(self._lib.lbm_run_driven(self._ctx, arr.size, av.ctypes.data, arr.ctypes.data if arr.size else None))
        return av

    def run_sampled(self, nsteps: int, every: int, out=None):
        """lbm_run with snapshots after steps every, 2 every, ...: returns (av_vels[nsteps], fields) where fields is
        (m, rows, nx, 4) float32 (u_x, u_y, |u|, pressure; m = nsteps // every; as final_state), a numpy array -- or
        `out`, a contiguous float32 torch tensor of that shape on the context's GPU, filled there.  The register tiles
        write the snapshots inside their kernels (info("samples_in_kernel") == 1); where lbm_wave runs they ride in its
        launches (info("samples_in_wave") == 1: av_vels is run()'s bits, the fields are the split path's bits); elsewhere
        the steps run in pieces of `every` with a derive kernel behind each."""
        m = nsteps // every if every > 0 else 0
        shape = (m, self._local_rows(), self.params.nx, 4)
        av = np.empty(max(nsteps, 0), dtype=np.float32)
        fields, ptr = self._output(out, shape, "out")
        _check(self._lib.lbm_run_sampled(self._ctx, nsteps, av.ctypes.data, every, ptr))
        return av, fields

    def run_mean(self, nsteps: int, every: int = 1, out=None):
        """lbm_run with the time-averaged fields over the sample steps every, 2 every, ...: returns (av_vels[nsteps], mean)
        where mean is (rows, nx, 4) float32 (u_x, u_y, |u|, pressure; the float sum of run_sampled's snapshots in step
        order, divided by their number), a numpy array -- or `out`, a contiguous float32 torch tensor of that shape on
        the context's GPU, filled there.  The register tiles keep the sums inside their kernels
        (info("mean_in_kernel") == 1); where lbm_wave runs they ride in its launches (info("mean_in_wave") == 1: av_vels is
        run()'s bits, the mean is the split path's bits); elsewhere the steps run in pieces of `every` with an add kernel
        behind each."""
        shape = (self._local_rows(), self.params.nx, 4)
        av = np.empty(max(nsteps, 0), dtype=np.float32)
        mean, ptr = self._output(out, shape, "out")
        _check(self._lib.lbm_run_mean(self._ctx, nsteps, av.ctypes.data, every, ptr))
        return av, mean

    def run_stats(self, nsteps: int, every: int = 1, out=None):
        """lbm_run with the means and second moments over the sample steps every, 2 every, ...: returns (av_vels[nsteps],
        stats) where stats is (rows, nx, 8) float32 -- floats 0..3 run_mean's output, bit for bit (the means of u_x, u_y,
        |u|, pressure), floats 4..7 the means of u_x^2, u_y^2, u_x u_y and (p - p0)^2 with p0 = float32(density) * float32(1/3) as a
        blocked cell reads it -- a numpy array, or `out`, a contiguous float32 torch tensor of that shape on the context's
        GPU, filled there.  Variances and covariances are the caller's to form, in double, as E[xy] - E[x] E[y].  Where
        lbm_wave runs the sums ride in its launches (info("stats_in_wave") == 1: av_vels is run()'s bits); elsewhere the
        steps run in pieces of `every` (on the register tiles where they run) with an add kernel behind each."""
        shape = (self._local_rows(), self.params.nx, 8)
        av = np.empty(max(nsteps, 0), dtype=np.float32)
        stats, ptr = self._output(out, shape, "out")
        _check(self._lib.lbm_run_stats(self._ctx, nsteps, av.ctypes.data, every, ptr))
        return av, stats

    def set_probes(self, xy):
        """The cells run_probes records: xy is anything np.asarray turns into int32[n, 2] of (column, row) in the global
        lattice, in the order the series are wanted; None or an empty set clears it."""
        if xy is None or np.size(xy) == 0:
            _check(self._lib.lbm_set_probes(self._ctx, None, 0))
            self._nprobes = 0
            return
        arr = np.ascontiguousarray(np.asarray(xy), dtype=np.int32)
        if arr.ndim != 2 or arr.shape[1] != 2:
            raise LbmError(f"xy must have shape (n, 2), got {arr.shape}")
        _check(self._lib.lbm_set_probes(self._ctx, arr.ctypes.data, arr.shape[0]))
        self._nprobes = arr.shape[0]

    def run_probes(self, nsteps: int, every: int = 1, out=None):
        """lbm_run with the time series of the probes (set_probes): returns (av_vels[nsteps], probes) where probes is
        (nsteps // every, nprobes, 4) float32 -- u_x, u_y, |u|, pressure of each probe after steps every, 2 every, ...,
        the bits run_sampled has in those cells -- a numpy array, or `out`, a contiguous float32 torch tensor of that
        shape on the context's GPU, filled there.  The register tiles take the values inside their kernels
        (info("probes_in_kernel") == 1); where lbm_wave runs they ride in its launches (info("probes_in_wave") == 1:
        av_vels is run()'s bits, the probes are the split path's bits); elsewhere the steps run in pieces of `every`
        with a gather kernel behind each."""
        n = getattr(self, "_nprobes", 0)
        shape = (max(nsteps, 0) // every if every > 0 else 0, n, 4)
        av = np.empty(max(nsteps, 0), dtype=np.float32)
        probes, ptr = self._output(out, shape, "out")
        _check(self._lib.lbm_run_probes(self._ctx, nsteps, av.ctypes.data, every, ptr))
        return av, probes

    def run_window(self, nsteps: int, every: int, window: Window, out=None):
        """lbm_run with snapshots of a window after steps every, 2 every, ...: returns (av_vels[nsteps], windows) where
        windows is (m, window.ny, window.nx, 4) float32 (m = nsteps // every) -- the bits run_sampled has in the cells
        (window.x0 + c window.sx, window.y0 + r window.sy) of the global lattice -- a numpy array, or `out`, a contiguous
        float32 torch tensor of that shape on the context's GPU, filled there.  A rank context fills the window rows that
        lie in its own lattice rows (window_rows with slab_rows) and zeroes the others.  The register tiles take the
        window inside their kernels (info("window_in_kernel") == 1); where lbm_wave runs it rides in its launches
        (info("window_in_wave") == 1); elsewhere the steps run in pieces of `every` with a windowed derive kernel behind
        each.  Traffic, staging and host copy scale with the window, not with the lattice."""
        m = max(nsteps, 0) // every if every > 0 else 0
        shape = (m, window.ny, window.nx, 4)
        av = np.empty(max(nsteps, 0), dtype=np.float32)
        windows, ptr = self._output(out, shape, "out")
        _check(self._lib.lbm_run_window(self._ctx, nsteps, av.ctypes.data, every, C.byref(window), ptr))
        return av, windows

    def run_window_stats(self, nsteps: int, every: int, window: Window, out=None):
        """run_stats over a window: returns (av_vels[nsteps], stats) where stats is (window.ny, window.nx, 8) float32 -- the
        eight floats run_stats has in the cells (window.x0 + c window.sx, window.y0 + r window.sy) of the global lattice, bit
        for bit: the means of u_x, u_y, |u|, pressure and of u_x^2, u_y^2, u_x u_y, (p - p0)^2 over the sample steps every,
        2 every, ... -- a numpy array, or `out`, a contiguous float32 torch tensor of that shape on the context's GPU, filled
        there.  A rank context fills the window rows that lie in its own lattice rows and zeroes the others.  Device memory
        for the sums is 32 bytes per window cell.  Where lbm_wave runs the sums ride in its launches
        (info("window_stats_in_wave") == 1); the register tiles take the samples inside their kernels, set_option(
        "window_stats_chunk") sample steps a launch, and a fold kernel adds them up (info("window_stats_in_kernel") == 1;
        info("window_stats_pieces"): the launches); either way av_vels is run()'s bits.  Elsewhere the steps run in pieces
        of `every` with a windowed add kernel behind each."""
        shape = (window.ny, window.nx, 8)
        av = np.empty(max(nsteps, 0), dtype=np.float32)
        stats, ptr = self._output(out, shape, "out")
        _check(self._lib.lbm_run_window_stats(self._ctx, nsteps, av.ctypes.data, every, C.byref(window), ptr))
        return av, stats

    def set_bodies(self, body, nbodies: int):
        """Labels blocked cells 1..nbodies (0: not counted) for run_forces: body is int[ny, nx] over the global lattice
        (labels on fluid cells are ignored); nbodies = 0 clears the labelling."""
        if nbodies == 0 and body is None:
            _check(self._lib.lbm_set_bodies(self._ctx, None, 0))
            self._nbodies = 0
            return
        b = np.ascontiguousarray(body, dtype=np.int32)
        if b.size != self.params.nx * self.params.ny:
            raise LbmError(f"body must hold {self.params.ny} x {self.params.nx} labels")
        _check(self._lib.lbm_set_bodies(self._ctx, b.ctypes.data, nbodies))
        self._nbodies = nbodies

    def run_forces(self, nsteps: int):
        """lbm_run that also returns the force of the fluid on every body at every step: (av_vels[nsteps],
        forces[nsteps, nbodies, 2]) with (F_x, F_y) per body (definition: include/lbm_mi355x.h).  The register tiles sum
        them inside their kernels (info("forces_in_kernel") == 1); where lbm_wave runs they ride in its launches
        (info("forces_in_wave") == 1: av_vels is run()'s bits, the forces are the one-step path's bits); elsewhere the
        one-step kernel runs with a force kernel behind each step."""
        nb = getattr(self, "_nbodies", 0)
        av = np.empty(max(nsteps, 0), dtype=np.float32)
        forces = np.empty((max(nsteps, 0), nb, 2), dtype=np.float32)
        _check(self._lib.lbm_run_forces(self._ctx, nsteps, av.ctypes.data, forces.ctypes.data if forces.size else None))
        return av, forces

    def _output(self, out, shape, name):
        """(array or tensor, pointer) of one output of a run_* call: a fresh numpy array, or `out`, a contiguous float32
        CUDA tensor of that shape, waited for.  The pointer is None where there is nothing to write."""
        if out is None:
            arr = np.empty(shape, dtype=np.float32)
            return arr, (arr.ctypes.data if arr.size else None)
        import torch
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or not out.is_cuda
                or not out.is_contiguous() or tuple(out.shape) != shape):
            raise LbmError(f"{name} must be a contiguous float32 CUDA tensor of shape {shape}")
        torch.cuda.synchronize(out.device)      # (the library's streams do not follow torch's)
        return out, (out.data_ptr() if out.numel() else None)

    def run_observed(self, nsteps: int, forces: bool = False, probes_every: int = 0, mean_every: int = 0,
                     fields_every: int = 0, probes_out=None, mean_out=None, fields_out=None):
        """lbm_run with any subset of the observers in ONE run: forces=True (run_forces), probes_every > 0 (run_probes),
        mean_every > 0 (run_mean), fields_every > 0 (run_sampled).  Returns a dict with "av_vels" and one entry per wanted
        observer -- "forces", "probes", "mean", "fields" -- each the bits its own call returns: numpy arrays, or the
        contiguous float32 CUDA tensors given as probes_out / mean_out / fields_out, filled on the GPU.  Where lbm_wave
        runs, forces and probes ride together in its launches and cut no piece (info("observed_in_wave"): bits 1 forces,
        2 probes; info("observed_in_kernel") means the register tiles and reads 0 there)."""
        av, res, what = self._observe(max(nsteps, 0), forces, probes_every, mean_every, fields_every, probes_out, mean_out, fields_out)
        _check(self._lib.lbm_run_observed(self._ctx, nsteps, av.ctypes.data if av.size else None, C.byref(what)))
        return res

    def run_driven_observed(self, accel, forces: bool = False, probes_every: int = 0, mean_every: int = 0,
                            fields_every: int = 0, probes_out=None, mean_out=None, fields_out=None):
        """run_driven that also observes (lbm_run_driven_observed): step t is driven by accel[t], nsteps = len(accel), and
        the keyword arguments and the returned dict are run_observed's.  No observer wanted: exactly run_driven.  One
        observer alone is legal.  Probes, means and snapshots are bit for bit what their definitions give from the lattices
        of `for a in accel: set_accel(a); run(1)`; the context's own acceleration is untouched.  The register tiles run
        every piece in one flavour that reads the schedule from a device table (info("driven_observed_in_kernel"): bits
        1 forces, 2 probes); where lbm_wave runs, forces and probes ride in its launches with the K pairs of a pass
        (info("driven_observed_in_wave")); info("driven_observed_pieces") counts the step-loop pieces."""
        arr = np.asarray(accel)
        if arr.ndim != 1:
            raise LbmError(f"accel must be one-dimensional (one value per step), got shape {arr.shape}")
        if arr.dtype.kind not in "fiu":
            raise LbmError(f"accel must hold real numbers, got dtype {arr.dtype}")
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        av, res, what = self._observe(arr.size, forces, probes_every, mean_every, fields_every, probes_out, mean_out, fields_out)
        _check(self._lib.lbm_run_driven_observed(self._ctx, arr.size, av.ctypes.data if av.size else None,
                                                 arr.ctypes.data if arr.size else None, C.byref(what)))
        return res

    def _observe(self, n, forces, probes_every, mean_every, fields_every, probes_out, mean_out, fields_out):
        """The outputs of one run_observed / run_driven_observed call of n steps: (av_vels, the dict to return, the
        lbm_observe that names them)."""
        av = np.empty(n, dtype=np.float32)
        res = {"av_vels": av}
        what = Observe()
        if forces:
            f = np.empty((n, getattr(self, "_nbodies", 0), 2), dtype=np.float32)
            res["forces"] = f
            what.forces = f.ctypes.data if f.size else av.ctypes.data    # (wanted, but nothing to write: any non-NULL pointer)
        rows, nx = self._local_rows(), self.params.nx
        if probes_every != 0 or probes_out is not None:
            shape = (n // probes_every if probes_every > 0 else 0, getattr(self, "_nprobes", 0), 4)
            res["probes"], ptr = self._output(probes_out, shape, "probes_out")
            what.probes_out = ptr if ptr is not None else av.ctypes.data
            what.probes_every = probes_every
        if mean_every != 0 or mean_out is not None:
            res["mean"], ptr = self._output(mean_out, (rows, nx, 4), "mean_out")
            what.mean_out = ptr
            what.mean_every = mean_every
        if fields_every != 0 or fields_out is not None:
            shape = (n // fields_every if fields_every > 0 else 0, rows, nx, 4)
            res["fields"], ptr = self._output(fields_out, shape, "fields_out")
            what.fields_out = ptr if ptr is not None else av.ctypes.data
            what.fields_every = fields_every
        return av, res, what

    def last_run_ms(self):
        g, w = C.c_double(0), C.c_double(0)
        _check(self._lib.lbm_last_run_ms(self._ctx, C.byref(g), C.byref(w)))
        return g.value, w.value

    # -- state --------------------------------------------------------------
    def slab_rows(self, slab: int = 0):
        a, b = C.c_int(0), C.c_int(0)
        _check(self._lib.lbm_slab_rows(self._ctx, slab, C.byref(a), C.byref(b)))
        return a.value, b.value

    @property
    def num_slabs(self) -> int:
        return self._lib.lbm_num_slabs(self._ctx)

    def _local_rows(self) -> int:
        if self.rank_mode:
            a, b = self.slab_rows(0)
            return b - a
        return self.params.ny

    def read_state(self) -> np.ndarray:
        """Current lattice, reference AoS layout: (rows, nx, 9) float32."""
        out = np.empty((self._local_rows(), self.params.nx, NSPEEDS), dtype=np.float32)
        _check(self._lib.lbm_read_state(self._ctx, out.ctypes.data))
        return out

    def set_obstacles(self, obstacles, refill: int = REFILL_KEEP):
        """Replaces the obstacle map for every later call (lbm_set_obstacles): obstacles is int[ny, nx] over the global
        lattice (in rank mode the global array on every rank).  Afterwards the context is, bit for bit, a fresh one made
        from (obstacles, the lattice as it stands) with the same options, acceleration and probe set; refill =
        REFILL_REST puts the rest equilibrium into the cells that turn from blocked to fluid (the total density changes),
        REFILL_KEEP leaves what bounce-back left there.  The body labelling is cleared: set_bodies again before
        run_forces.  info("refilled_cells") / info("obstacle_updates") count.  Rank contexts: every rank returns from this
        call before any rank runs."""
        ob = _as_obstacles(obstacles, self.params)
        _check(self._lib.lbm_set_obstacles(self._ctx, ob.ctypes.data, int(refill)))
        self._nbodies = 0

    def write_state(self, cells):
        """Replaces the lattice (lbm_write_state), the inverse of read_state: cells is (rows, nx, 9) float32 -- a numpy
        array (or anything np.ascontiguousarray takes), or a contiguous float32 CUDA torch tensor of that size on the
        context's GPU, or an int device pointer to such memory -- rows = the whole lattice, in rank mode this rank's own.
        Values are not inspected.  Options, acceleration, probes and bodies are kept."""
        n = self._local_rows() * self.params.nx * NSPEEDS
        if isinstance(cells, int):
            ptr = cells
        elif type(cells).__module__.split(".")[0] == "torch":
            import torch
            if (cells.dtype != torch.float32 or not cells.is_cuda or not cells.is_contiguous() or cells.numel() != n):
                raise LbmError(f"cells must be a contiguous float32 CUDA tensor of {n} floats")
            torch.cuda.synchronize(cells.device)      # (the library's streams do not follow torch's)
            ptr = cells.data_ptr()
        else:
            a = np.ascontiguousarray(cells, dtype=np.float32)
            if a.size != n:
                raise LbmError(f"cells has {a.size} floats, expected {n}")
            ptr = a.ctypes.data
        _check(self._lib.lbm_write_state(self._ctx, ptr))

    def final_state(self) -> np.ndarray:
        """(rows, nx, 4) = u_x, u_y, |u|, pressure, computed on the GPU."""
        out = np.empty((self._local_rows(), self.params.nx, 4), dtype=np.float32)
        _check(self._lib.lbm_final_state(self._ctx, out.ctypes.data))
        return out

    def av_velocity(self) -> float:
        v = C.c_float(0)
        _check(self._lib.lbm_av_velocity(self._ctx, C.byref(v)))
        return v.value

    def reynolds(self) -> float:
        v = C.c_float(0)
        _check(self._lib.lbm_reynolds(self._ctx, C.byref(v)))
        return v.value

    def total_density(self) -> float:
        v = C.c_double(0)
        _check(self._lib.lbm_total_density(self._ctx, C.byref(v)))
        return v.value

    def set_option(self, key: str, value: int):
        _check(self._lib.lbm_set_option(self._ctx, key.encode(), value))

    def info(self, key: str) -> float:
        v = C.c_double(0)
        _check(self._lib.lbm_get_info(self._ctx, key.encode(), C.byref(v)))
        return v.value

    def close(self):
        if self._ctx:
            self._lib.lbm_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def timestep_new2(params: Param, cells: np.ndarray, tmp_cells: np.ndarray, obstacles) -> float:
    """The reference's call shape (d2q9-bgk.c:98): one step on host arrays.

    Mutates `cells` (accelerate phase, row ny-2) and overwrites `tmp_cells`,
    exactly like the reference; the caller swaps.  Returns the average speed.
    """
    lib = load_library()
    if cells.dtype != np.float32 or tmp_cells.dtype != np.float32 or not cells.flags.c_contiguous \
            or not tmp_cells.flags.c_contiguous:
        raise LbmError("cells/tmp_cells must be C-contiguous float32 arrays")
    ob = _as_obstacles(obstacles, params)
    av = C.c_float(0)
    _check(lib.lbm_timestep(C.byref(params), cells.ctypes.data, tmp_cells.ctypes.data, ob.ctypes.data, C.byref(av)))
    return av.value


# ------------------------------------------------------------------ host I/O
def _die(message: str):
    raise LbmError(message)


def read_params(paramfile: str) -> Param:
    """Seven values `nx ny maxIters reynolds_dim density accel omega` (d2q9-bgk.c:2736-2762)."""
    try:
        tokens = open(paramfile).read().split()
    except OSError:
        _die(f"could not open input parameter file: {paramfile}")
    names = ("nx", "ny", "maxIters", "reynolds_dim", "density", "accel", "omega")
    vals = []
    for i, name in enumerate(names):
        try:
            vals.append(int(tokens[i]) if i < 4 else float(tokens[i]))
        except (IndexError, ValueError):
            _die(f"could not read param file: {name}")
    return Param(*vals)


def read_obstacles(obstaclefile: str, params: Param) -> np.ndarray:
    """Lines `x y 1` -> int32 (ny, nx) map, the reference's checks and messages (d2q9-bgk.c:2844-2857)."""
    try:
        text = open(obstaclefile).read()
    except OSError:
        _die(f"could not open input obstacles file: {obstaclefile}")
    ob = np.zeros((params.ny, params.nx), dtype=np.int32)
    tok = text.split()
    if len(tok) % 3:
        _die("expected 3 values per line in obstacle file")
    try:
        arr = np.array(tok, dtype=np.int64).reshape(-1, 3)
    except ValueError:
        _die("expected 3 values per line in obstacle file")
    if arr.size:
        if (arr[:, 0] < 0).any() or (arr[:, 0] > params.nx - 1).any():
            _die("obstacle x-coord out of range")
        if (arr[:, 1] < 0).any() or (arr[:, 1] > params.ny - 1).any():
            _die("obstacle y-coord out of range")
        if (arr[:, 2] != 1).any():
            _die("obstacle blocked value should be 1")
        ob[arr[:, 1], arr[:, 0]] = 1
    return ob


def initialise(paramfile: str, obstaclefile: str):
    """(params, cells, obstacles): parse both inputs, rest-equilibrium lattice (d2q9-bgk.c:2716-2869)."""
    p = read_params(paramfile)
    ob = read_obstacles(obstaclefile, p)
    d = np.float32(p.density)
    w = np.array([d * np.float32(4) / np.float32(9)] + [d / np.float32(9)] * 4 + [d / np.float32(36)] * 4,
                 dtype=np.float32)
    cells = np.broadcast_to(w, (p.ny, p.nx, NSPEEDS)).copy()
    return p, cells, ob


def write_values(params: Param, state4: np.ndarray, obstacles: np.ndarray, av_vels,
                 final_state_file="final_state.dat", av_vels_file="av_vels.dat"):
    """Both output files in the reference's line formats (d2q9-bgk.c:2978, 2993)."""
    ob = np.asarray(obstacles).reshape(params.ny, params.nx)
    s4 = np.asarray(state4, dtype=np.float32).reshape(params.ny, params.nx, 4)
    with open(final_state_file, "w") as fp:
        for jj in range(params.ny):
            fp.write("".join("%d %d %.12E %.12E %.12E %.12E %d\n" % (
                ii, jj, s4[jj, ii, 0], s4[jj, ii, 1], s4[jj, ii, 2], s4[jj, ii, 3], ob[jj, ii])
                for ii in range(params.nx)))
    with open(av_vels_file, "w") as fp:
        fp.write("".join("%d:\t%.12E\n" % (i, float(v)) for i, v in enumerate(av_vels)))


# ------------------------------------------------------------------ row slabs
# What crosses a slab boundary each step (the pull stencil, d2q9-bgk.c:971-998): a slab's
# bottom row is pulled into by the slab to the south through directions 4,7,8, its top row by
# the slab to the north through 2,5,6 -- three planes of one row per direction, 3*nx floats.
HALO_PLANES_TO_SOUTH = (4, 7, 8)   # of the sender's row 0
HALO_PLANES_TO_NORTH = (2, 5, 6)   # of the sender's last row
# Two steps per pass (lbm_sweep2) trade halos once per PAIR of steps: the adjacent row's cells are
# recomputed as the tile ring, which takes its centre planes 0,1,3, the three planes that stream
# across the boundary, and those three planes of the row behind it -- nine rows of nx floats
# (lbm_kernels.hip.h, kHaloSlots): (row offset from the sender's edge row, plane) per slot.
HALO9_TO_SOUTH = ((0, 0), (0, 1), (0, 3), (0, 4), (0, 7), (0, 8), (1, 4), (1, 7), (1, 8))
HALO9_TO_NORTH = ((0, 0), (0, 1), (0, 3), (0, 2), (0, 5), (0, 6), (1, 2), (1, 5), (1, 6))
TWO_STEP_TILE = (64, 16)           # lattice must tile: nx % 64 == 0, rows per slab % 16 == 0


def slab_bounds(ny: int, nslabs: int, slab: int):
    """Rows [begin, end) of slab `slab`: the library's own partition rule."""
    return slab * ny // nslabs, (slab + 1) * ny // nslabs


def ring_neighbours(rank: int, nranks: int):
    """(south, north) ranks of the periodic ring (the lattice wraps in y, d2q9-bgk.c:2132,2134)."""
    return (rank - 1) % nranks, (rank + 1) % nranks
