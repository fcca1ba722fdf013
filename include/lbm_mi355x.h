/*
 * lbm_mi355x.h -- C ABI of the MI355X-native D2Q9-BGK time-step path.
 *
 * This is the drop-in boundary for the hot path of ChuyueL/advanced-hpc-lbm:
 * the per-time-step sweep `timestep_new2` and the loop that drives it
 * (reference d2q9-bgk.c:180-201, 228-1813).  The reference has no FFI of its
 * own; its boundary is one in-process call site (d2q9-bgk.c:182,190)
 *
 *     av_vels[tt] = timestep_new2(params, cells, tmp_cells, obstacles);
 *     swap(&cells, &tmp_cells);
 *
 * plus the functions main calls once around it.  A per-step host-returning
 * call would force a device sync every step, so the unit here is "run N
 * steps": the library keeps both lattices resident in HBM (SoA planes), and
 * the host hands over / takes back the reference's own host layouts
 * (t_speed AoS cells, int obstacles, t_param).
 *
 * Conventions
 *   - Plain C types only.  Every function returns 0 on success and a non-zero
 *     LBM_E* code on failure; lbm_last_error() returns the message for the
 *     calling thread (the CLI host prints it through the reference's die()
 *     convention, d2q9-bgk.c:3001-3007).
 *   - Host arrays use the reference's layouts exactly:
 *       cells      float[ny*nx*9]  = t_speed[ny*nx]   (d2q9-bgk.c:76-79), index ii + jj*nx
 *       obstacles  int[ny*nx], 0 = fluid, non-zero = blocked (d2q9-bgk.c:2797,2856)
 *   - There is no CPU fallback: without a usable HIP device every compute
 *     entry point fails with LBM_ENODEV.
 */
#ifndef LBM_MI355X_H
#define LBM_MI355X_H

#ifdef __cplusplus
extern "C" {
#endif

#define LBM_NSPEEDS 9

/* error codes */
#define LBM_OK        0
#define LBM_EINVAL    1  /* bad argument / unsupported size */
#define LBM_ENODEV    2  /* no HIP device, or fewer than requested */
#define LBM_EHIP      3  /* a HIP runtime call failed */
#define LBM_ERCCL     4  /* RCCL missing or a RCCL call failed */
#define LBM_ENOMEM    5

/* Same fields, order and types as the reference's t_param (d2q9-bgk.c:64-73). */
typedef struct {
  int   nx;            /* no. of cells in x-direction */
  int   ny;            /* no. of cells in y-direction */
  int   maxIters;      /* no. of iterations */
  int   reynolds_dim;  /* dimension for Reynolds number */
  float density;       /* density per link */
  float accel;         /* density redistribution */
  float omega;         /* relaxation parameter */
} lbm_param;

typedef struct lbm_ctx lbm_ctx;

/* How neighbouring row slabs trade their one-row halos each step. */
#define LBM_EXCHANGE_AUTO   0  /* 1 slab: none (periodic self-wrap); >1 slabs: RCCL, or peer
                                  copies when the device list repeats a device (RCCL wants
                                  one rank per GPU) */
#define LBM_EXCHANGE_COPY   1  /* hipMemcpyAsync between slabs of ONE process (peer copies) */
#define LBM_EXCHANGE_RCCL   2  /* ncclSend/ncclRecv pairs over xGMI, own stream, overlapped */
#define LBM_EXCHANGE_P2P    3  /* kernels store their halo rows straight into the neighbour's
                                  buffers over xGMI and hand off through flags (no host, no
                                  collective call in the step loop); needs peer access (one
                                  process) or hipIpc (one process per GPU) and uncached device
                                  memory.  A halo wait gives up after 4 s: ranks must enter
                                  lbm_run within 4 s of each other, and when a neighbour stops,
                                  lbm_run returns LBM_EHIP within seconds (every queued launch
                                  sees the sticky error word and drains); the lattice is then
                                  undefined and later lbm_run calls on the context fail */

/* Message of the last failure on this thread ("" if none). */
const char* lbm_last_error(void);

/* Number of visible HIP devices (0 is a valid answer). */
int lbm_device_count(int* count);

/*
 * Replaces: initialise()'s allocation + the first-touch of cells/tmp_cells/
 * obstacles (d2q9-bgk.c:2787-2857), for a whole lattice owned by ONE process.
 *   params     global lattice parameters
 *   obstacles  int[ny*nx] blocked map (copied; caller keeps ownership)
 *   cells      float[ny*nx*9] initial lattice, or NULL for the reference's
 *              rest-equilibrium start (d2q9-bgk.c:2802-2823)
 *   nslabs     number of row slabs (>=1): slab r owns rows [r*ny/nslabs, (r+1)*ny/nslabs)
 *   devices    int[nslabs] HIP device per slab, or NULL for 0..nslabs-1
 *              (repeating a device is allowed: several slabs on one GPU)
 *   exchange   LBM_EXCHANGE_*
 */
int lbm_create(const lbm_param* params, const int* obstacles, const float* cells,
               int nslabs, const int* devices, int exchange, lbm_ctx** out);

/*
 * One-process-per-GPU form (bench.py under torch.distributed.run): this
 * process owns slab `rank` of `nranks` on HIP device `device`; halos travel
 * by RCCL.  `unique_id` is the 128-byte ncclUniqueId made by
 * lbm_rccl_unique_id() on rank 0 and broadcast by the caller.
 * `obstacles`/`cells` are the GLOBAL arrays (each rank keeps its rows only);
 * cells may be NULL as above.
 */
int lbm_rccl_unique_id(void* id128);
int lbm_create_rank(const lbm_param* params, const int* obstacles, const float* cells,
                    int rank, int nranks, int device, const void* unique_id, lbm_ctx** out);

/*
 * Same, with the halo transport chosen by the caller (LBM_EXCHANGE_RCCL or LBM_EXCHANGE_P2P;
 * lbm_create_rank = RCCL unless the environment says LBM_RANK_EXCHANGE=p2p).
 *   unique_id != NULL: the library forms a RCCL communicator (used for the end-of-run
 *     reductions, for RCCL halos, and to trade the hipIpc handles of peer-to-peer halos);
 *     if peer-to-peer set-up fails on ANY rank, all ranks fall back to RCCL halos together.
 *   unique_id == NULL (peer-to-peer only): no RCCL at all.  The caller trades the 64-byte
 *     handles itself -- lbm_p2p_handle() on every rank, all-gather by any means,
 *     lbm_p2p_connect() with all nranks handles in rank order -- before the first lbm_run;
 *     lbm_run / lbm_av_velocity / lbm_total_density then return this rank's CONTRIBUTION
 *     (slab sum over the global fluid-cell count), to be added across ranks by the caller.
 */
int lbm_create_rank_ex(const lbm_param* params, const int* obstacles, const float* cells,
                       int rank, int nranks, int device, const void* unique_id, int exchange,
                       lbm_ctx** out);
#define LBM_P2P_HANDLE_BYTES 64
int lbm_p2p_handle(lbm_ctx* ctx, void* handle64);
int lbm_p2p_connect(lbm_ctx* ctx, const void* handles, int nranks);

/* Rows [row_begin, row_end) of the global lattice held by slab `slab` of this context. */
int lbm_slab_rows(const lbm_ctx* ctx, int slab, int* row_begin, int* row_end);
int lbm_num_slabs(const lbm_ctx* ctx);

/*
 * Replaces: the time-step loop, d2q9-bgk.c:180-201 --
 *     for (tt...) { av_vels[tt] = timestep_new2(params, cells, tmp_cells, obstacles); swap(); }
 * Advances the resident lattice by `nsteps` steps and writes the per-step
 * average fluid speed (timestep_new2's return value, d2q9-bgk.c:1811) to
 * av_vels[0..nsteps) (may be NULL).  Synchronous: returns when the GPU work
 * is complete.  In rank mode every rank receives the global av_vels.
 */
int lbm_run(lbm_ctx* ctx, int nsteps, float* av_vels);

/*
 * lbm_run with snapshots of the derived fields taken during the run, after steps every, 2 every, ..., m every
 * (m = nsteps / every; every = 0: none, exactly lbm_run; every < 0: LBM_EINVAL).  fields_out: float[m][rows][nx][4],
 * snapshot j = what lbm_final_state would return after (j+1) every steps (same rows and rank-local convention), bit for
 * bit (a blocked cell: 0, 0, 0, density * (1.f / 3.f), in float); NULL only when m = 0.  av_vels, the lattice and
 * everything after are bit-identical to lbm_run(ctx, nsteps, av_vels).
 * fields_out may be host memory, or device memory of the device that holds every slab of the context (then nothing is
 * copied to the host).  The register-tile engines write the snapshots from inside their kernels (info
 * "samples_in_kernel" = 1); the other engines run the steps in pieces with a derive after each.  LBM_ENOMEM /
 * LBM_EINVAL before anything runs when the device staging or the snapshots do not fit: the lattice is untouched.
 * Which kernels take the snapshots:
 * - The register-tile engines write them from inside their kernels ("samples_in_kernel" = 1); av_vels is lbm_run's, bit
 *   for bit.
 * - Where lbm_wave runs (a lattice alone on its GPU with time_block 4, 6 or 8 and the wave kernel, nsteps >= time_block),
 *   the snapshots ride in its launches (info "samples_in_wave" = 1, "samples_in_kernel" = 0): a field flavour of lbm_wave
 *   stores every cell's four floats at every sample step of a pass, read between the collision and the next step's
 *   accelerate phase -- the values the stored lattice of that step would hold; passes without a sample step run the plain
 *   kernel, and the steps left over behind the last full pass go as lbm_run's do, with the derive kernel behind those that
 *   are sample steps.  In lbm_wave, av_vels is lbm_run's, bit for bit; the fields are the bits of the split path (below).
 *   Device output is written in place; host output goes through one device staging of the m snapshots, and if that
 *   staging has no room the run falls back to the split path: the same fields, no error.
 * - The remaining engines are unchanged: contexts where lbm_march runs, slabs with neighbours, rank contexts and runs
 *   shorter than time_block run the steps in pieces of `every` with a derive after each (the split path; correct, not
 *   fast; both keys read 0).
 * With forces, probes or means in one run: lbm_run_observed.
 */
int lbm_run_sampled(lbm_ctx* ctx, int nsteps, float* av_vels, int every, float* fields_out);

/*
 * lbm_run with the time-averaged fields of the run: the mean of u_x, u_y, |u| and pressure per cell over the sample steps
 * of lbm_run_sampled (after steps every, 2 every, ..., m every; m = nsteps / every).  With X_j = snapshot j of
 * lbm_run_sampled(ctx, nsteps, av_vels, every, ...), the definition is, per cell and field, bit for bit:
 *     S_0 = +0.0f;  S_j = S_(j-1) + X_j  in float, in step order (one rounding per add, no fma, no reassociation);
 *     mean_out = S_m / (float)m  (a correctly rounded float division).
 * Blocked cells take part like any other (their X_j is the constant 0, 0, 0, density * (1.f / 3.f), in float).
 * mean_out: float[rows][nx][4]
 * with the rows and the rank-local convention of lbm_final_state; host memory, or device memory of the device that holds
 * every slab of the context (then nothing is copied to the host).  av_vels, the lattice and everything after are
 * bit-identical to lbm_run(ctx, nsteps, av_vels).  The register-tile engines keep the sums inside their kernels (info
 * "mean_in_kernel" = 1: no memory traffic for them until the run ends, then one 16-byte store per cell); the other engines
 * run the steps in pieces of `every` with a small kernel behind each that adds into a per-slab buffer on the device
 * (correct, not fast; same adds in the same order, the same bits).
 * LBM_EINVAL when every <= 0, m = 0 (nothing to average), mean_out is NULL or nsteps < 0; LBM_ENOMEM when the per-slab
 * buffer (16 bytes per cell) does not fit; in both cases before anything runs: the lattice is untouched.
 * A window that starts late is lbm_run(ctx, skip, ...) followed by lbm_run_mean; the means of consecutive calls can be
 * combined by the caller in double (weights m).  Accuracy: a plain float sum of m terms carries at most (m - 1) 2^-24
 * relative to the sum of |X_j| per cell.
 * Which kernels take the sums:
 * - The register-tile engines keep them inside their kernels ("mean_in_kernel" = 1); av_vels is lbm_run's, bit for bit.
 * - Where lbm_wave runs (a lattice alone on its GPU with time_block 4, 6 or 8 and the wave kernel, nsteps >= time_block),
 *   the sums ride in its launches (info "mean_in_wave" = 1, "mean_in_kernel" = 0): at every sample step of a pass the
 *   field flavour of lbm_wave adds every cell's four floats into the per-slab buffer (one lane owns a cell through all
 *   steps of a pass and passes follow each other on one stream: the adds keep the order of the steps); the steps left
 *   over behind the last full pass go as lbm_run's do, with the add kernel behind those that are sample steps.  In
 *   lbm_wave, av_vels is lbm_run's, bit for bit; the fields are the bits of the split path (below).  The buffer is the one
 *   every path allocates: where it has no room the call fails as before, and a context that cannot run lbm_wave falls
 *   back to the split path.
 * - The remaining engines are unchanged: contexts where lbm_march runs, slabs with neighbours, rank contexts and runs
 *   shorter than time_block keep the split path (pieces of `every` steps, the add kernel behind each; both keys read 0).
 * With snapshots, forces or probes in one run: lbm_run_observed.
 */
int lbm_run_mean(lbm_ctx* ctx, int nsteps, float* av_vels, int every, float* mean_out);

/*
 * lbm_run_mean with the second moments beside the means: what Reynolds stresses, r.m.s. velocity and r.m.s. pressure are
 * formed from.  stats_out: float[rows][nx][8], rows, rank-local convention and memory (host, or the device that holds every
 * slab) as lbm_run_mean's.  With X_j = (u_x, u_y, |u|, p) = snapshot j of lbm_run_sampled(ctx, nsteps, av_vels, every, ...)
 * from the same state (sample steps every, 2 every, ..., m every; m = nsteps / every) and p0 = density * (1.f / 3.f), the
 * float a blocked cell reads as pressure, the definition is, per cell, bit for bit, in float with one rounding per
 * operation, no fma and no reassociation:
 *     d   = X_j.w - p0
 *     Q_j = ( X_j.x * X_j.x,  X_j.y * X_j.y,  X_j.x * X_j.y,  d * d )
 *     S_0 = T_0 = +0.0f;   S_j = S_(j-1) + X_j;   T_j = T_(j-1) + Q_j      (step order)
 *     stats_out[cell][0..3] = S_m / (float)m;   stats_out[cell][4..7] = T_m / (float)m
 * So floats 0..3 of every cell are lbm_run_mean's output with the same arguments, bit for bit, and a blocked cell reads
 * (0, 0, 0, p0', 0, 0, 0, 0) with p0' = (p0 + p0 + ... + p0) / (float)m by the sums above: p0 itself where that float sum
 * does not round (m = 1, 2, 4 always), else within an ulp or two of it.
 * Why the pressure is shifted: p sits at about p0 with fluctuations orders of magnitude smaller; a float sum of
 * p^2 loses them in its rounding, a sum of (p - p0)^2 does not.  Variances and covariances are the caller's to form, in
 * double, as E[xy] - E[x] E[y]: var(u_x) = [4] - [0]^2, var(u_y) = [5] - [1]^2, cov(u_x, u_y) = [6] - [0] [1],
 * var(p) = [7] - ([3] - p0)^2.
 * av_vels, the lattice and everything after the call are bit-identical to lbm_run(ctx, nsteps, av_vels) wherever the
 * register tiles or lbm_wave ran the steps; on the split path av_vels is equal to rounding of the per-step sum, as for
 * lbm_run_mean.
 * LBM_EINVAL when ctx is NULL, nsteps < 0, every <= 0, m = 0, stats_out is NULL or device memory of another device than the
 * slabs'; LBM_ENOMEM when the sums (32 bytes per cell) do not fit -- the ranks of a rank context agree on that first;
 * LBM_EHIP after a failed peer-to-peer wait; each with nothing queued and the lattice untouched.
 * Which kernels take the sums:
 * - Where lbm_wave runs (admission as lbm_run_mean's: a lattice alone with time_block 4, 6 or 8 and the wave kernel, nsteps
 *   >= time_block), the sums ride in its launches (info "stats_in_wave" = 1, reset at the start of each call): a stats
 *   flavour of lbm_wave adds every cell's eight terms into its 32-byte record at the sample levels of a pass, one kernel
 *   per pass of K steps; a pass without a sample step runs the plain kernel; the steps left over behind the last full pass
 *   go as lbm_run's do, with the add kernel behind those that are sample steps.
 * - Everywhere else -- the register tiles, lbm_march, slabs with neighbours, rank contexts, runs shorter than time_block --
 *   the steps run in pieces of `every` with the add kernel behind each ("stats_in_wave" = 0); pieces on a register-tile
 *   context stay on the tiles, in the flavour lbm_run_observed's pieces run in, which folds a piece's last step sum as a
 *   whole run folds it there: av_vels does not depend on where the call is cut.  The same adds in the same order, the same
 *   bits.
 * Not offered: sums inside the register tiles (their mean flavour keeps three sums per cell in LDS; seven would want about
 * 112 KB of a CU's 160 KB at 4096 cells per tile, beside the mailboxes: unverified); stats inside lbm_run_observed, whose
 * struct is frozen; stats under a schedule; higher moments; the command-line tool.  (Stats over a window are a call of
 * their own: lbm_run_window_stats.)
 */
int lbm_run_stats(lbm_ctx* ctx, int nsteps, float* av_vels, int every, float* stats_out);

/*
 * Drag and lift on labelled bodies, step by step.
 *
 * Directions are the reference's: 1 E, 2 N, 3 W, 4 S, 5 NE, 6 NW, 7 SW, 8 SE. c_i is the lattice vector and opp(i)
 * is the reverse direction. The lattice wraps in x and y. For body b and step t (t = 1..nsteps of the call):
 *
 *     F_b(t) = 2 * Σ_{B blocked, label(B) = b}  Σ_{i = 1..8 : cell B - c_i is fluid}  c_i * f~_i(B, t)
 *
 * f~_i(B, t) is the population that B pulled along direction i in step t, after that step's accelerate. It is also the
 * value in plane opp(i) of B in the lattice stored after step t, so F can be computed from `lbm_read_state` alone.
 * This is the force *on* the body: with the shipped decks' +x acceleration, the steady drag is positive.
 */
#define LBM_MAX_BODIES 4
/* body: int[ny*nx] over the GLOBAL lattice (in both modes); 0 = not counted, 1..nbodies = the body a blocked cell
   belongs to; labels on fluid cells are ignored.  Replaces any earlier labelling; nbodies = 0 clears it.
   LBM_EINVAL (the earlier labelling kept) when nbodies is outside [0, LBM_MAX_BODIES], body is NULL with nbodies > 0, or
   a blocked cell of this context's rows carries a label outside [0, nbodies]. */
int lbm_set_bodies(lbm_ctx* ctx, const int* body, int nbodies);
/* lbm_run that also writes forces[nsteps][nbodies][2] = (F_x, F_y) of each body at each step (definition above).
   The lattice and everything after the call are bit-identical to lbm_run(ctx, nsteps, av_vels).
   Which kernels take the forces:
   - The register tiles take the sums inside their kernels (info "forces_in_kernel" = 1); av_vels is lbm_run's, bit for bit.
   - Where lbm_wave runs (a lattice alone on its GPU with time_block 4, 6 or 8 and the wave kernel, nsteps >= time_block),
     the forces ride in its launches (info "forces_in_wave" = 1, "forces_in_kernel" = 0): a force flavour of lbm_wave
     stores every counted cell's contribution at every step of a pass and a small kernel behind each launch adds them up;
     the steps left over behind the last full pass go as lbm_run's do, with a force kernel behind each.  There
     av_vels is lbm_run's, bit for bit, and the forces are the bits of the one-step path (below), whichever steps fell
     inside an lbm_wave launch.  If the force maps (5 bytes per cell) do not fit on the device, the run takes the one-step
     path: the same forces, no error.
   - The remaining engines are unchanged: contexts where lbm_march runs, slabs with neighbours, rank contexts and runs
     shorter than time_block run the one-step kernel with a small force kernel behind each step (correct, not fast; both
     keys read 0).  Where lbm_run would take several steps per launch there, av_vels is the one-step kernel's: equal to
     lbm_run's within float rounding of the per-step sum.
   Rank contexts: every rank gets the global forces (without RCCL: its own contribution), as with av_vels.
   LBM_EINVAL with nothing queued and the lattice untouched when no bodies are set or forces is NULL with nsteps > 0;
   LBM_ENOMEM likewise when the register tiles' partials do not fit.
   With snapshots, probes or means in one run: lbm_run_observed. */
int lbm_run_forces(lbm_ctx* ctx, int nsteps, float* av_vels, float* forces);

/*
 * Time series at chosen cells: u_x, u_y, |u| and pressure of a set of probes after every sample step of a run (pressure
 * taps on a body, a velocity probe in a wake, a monitor point, a line of cells across the channel).
 */
#define LBM_MAX_PROBES 4096
/* xy: int[nprobes][2] = (ii, jj), column and row in the GLOBAL lattice (in both modes).  Replaces any earlier set;
   nprobes = 0 clears it (xy may then be NULL).  Blocked cells are legal probes.  The set survives runs of every kind,
   lbm_set_bodies and option changes (a new "regtile" tiling rebuilds the register tiles' per-tile tables at the next
   lbm_run_probes).  LBM_EINVAL (the earlier set kept) when nprobes is outside [0, LBM_MAX_PROBES], xy is NULL with
   nprobes > 0, a coordinate is outside the lattice, or two entries name the same cell (the message says which two);
   LBM_ENOMEM (the earlier set kept) when the per-slab lists do not fit on the device. */
int lbm_set_probes(lbm_ctx* ctx, const int* xy, int nprobes);
/* lbm_run that also writes probes_out[m][nprobes][4] = u_x, u_y, |u|, pressure of every probe after steps
   every, 2 every, ..., m every (m = nsteps / every).
   Definition, bit for bit: probes_out[j][p][:] equals fields_out[j][jj_p][ii_p][:] of
   lbm_run_sampled(ctx, nsteps, av_vels, every, fields_out) from the same state; a blocked cell reads the constant
   0, 0, 0, density * (1.f / 3.f) (in float).  Probes keep the order in which they were given.  The lattice and
   everything after the call are bit-identical to lbm_run(ctx, nsteps, av_vels).  probes_out: host memory, or device memory of the device that holds
   every slab of the context (then nothing is copied to the host).
   Rank contexts: xy is global on every rank; each rank fills the entries of the probes that lie in its own rows
   (lbm_slab_rows) and writes +0.0f to the others; no communication is added.  Combining the ranks' arrays is the caller's
   business: a float sum turns a probe's -0.0f into +0.0f, so selecting each entry from the rank that owns its row is the
   bit-exact way.
   Which kernels take the probes:
   - The register-tile engines take the values inside their kernels (info "probes_in_kernel" = 1): a sample step moves 16
     bytes per probe and nothing else; av_vels is lbm_run's, bit for bit.
   - Where lbm_wave runs (a lattice alone on its GPU with time_block 4, 6 or 8 and the wave kernel, nsteps >= time_block),
     the probes ride in its launches (info "probes_in_wave" = 1, "probes_in_kernel" = 0): a probe flavour of lbm_wave
     stores a probe's four floats at every sample step of a pass, read between the collision and the next step's
     accelerate phase -- the values the stored lattice of that step would hold; the steps left over behind the last full
     pass go as lbm_run's do, with the gather kernel behind those that are sample steps.  There av_vels is lbm_run's, bit
     for bit, and the probes are the bits of the split path (below), whichever steps fell inside an lbm_wave launch.  If
     the probe maps (5 bytes per cell) do not fit on the device, the run takes the split path: the same probes, no error.
   - The remaining engines are unchanged: contexts where lbm_march runs, slabs with neighbours, rank contexts and runs
     shorter than time_block run the steps in pieces of `every` with a small gather kernel behind each (correct, not fast;
     the same bits; both keys read 0).  There av_vels is as for lbm_run_sampled / lbm_run_mean on those engines: equal
     to lbm_run's within float rounding of the per-step sum.
   LBM_EINVAL with nothing queued and the lattice untouched when no probes are set, every <= 0, nsteps < 0, m = 0 or
   probes_out is NULL; LBM_ENOMEM likewise when the device staging of host output (16 m nprobes bytes per slab that holds
   a probe) or the register tiles' tables do not fit.  Rank contexts agree on both before anything is queued.
   With snapshots, forces or means in one run: lbm_run_observed. */
int lbm_run_probes(lbm_ctx* ctx, int nsteps, float* av_vels, int every, float* probes_out);

/*
 * One run, any subset of the four observers: drag and lift per step (lbm_run_forces), time series at the probes
 * (lbm_run_probes), time-averaged fields (lbm_run_mean) and snapshots (lbm_run_sampled) of the SAME steps.
 * Layout (plain C, LP64): sizeof(lbm_observe) = 48; offsets forces 0, probes_out 8, mean_out 16, fields_out 24,
 * probes_every 32, mean_every 36, fields_every 40 (4 bytes of padding at the end).
 */
typedef struct {
  float* forces;       /* [nsteps][nbodies][2] as lbm_run_forces, or NULL: not wanted                       */
  float* probes_out;   /* [nsteps / probes_every][nprobes][4] as lbm_run_probes, or NULL                     */
  float* mean_out;     /* [rows][nx][4] as lbm_run_mean, or NULL                                             */
  float* fields_out;   /* [nsteps / fields_every][rows][nx][4] as lbm_run_sampled, or NULL                   */
  int probes_every, mean_every, fields_every;   /* read only where the pointer beside it is not NULL         */
} lbm_observe;
/* An observer is wanted exactly when its pointer is not NULL; what == NULL, or all four NULL: exactly lbm_run.
   The three periods are independent (probes every step, means every 10, a snapshot every 500); sample steps count from
   the start of the call, as in the single calls.
   Each output is, bit for bit, what its own call (lbm_run_forces, lbm_run_probes, lbm_run_mean, lbm_run_sampled) writes
   from the same state with the same options, bodies, probes and period: the rank-local conventions (rows of
   lbm_final_state; probes of other ranks' rows read +0.0f; forces global through the run's all-reduce, or the rank's
   contribution without RCCL), host or device memory per pointer, independently (forces: host memory), and the -0
   handling of the mean included.
   The lattice and everything after the call are bit-identical to lbm_run(ctx, nsteps, av_vels).  av_vels is bit-identical
   to lbm_run's wherever the register tiles ran the call (info "engine_last" = 3), in one launch or in pieces; on the
   streaming engines it is equal to lbm_run's within float rounding of the per-step sum, as for lbm_run_forces there.
   How: forces with probes ride inside one register-tile launch (a kernel flavour of its own); where lbm_wave runs (a
   lattice alone, as for lbm_run_probes) forces and probes ride together in its launches, in a force-and-probe flavour,
   and cut no piece: with those two alone the call is one piece and av_vels is lbm_run's, bit for bit; inside the pieces
   that means and snapshots cut, the probes' sample steps keep counting from the start of the call.  Means and snapshots
   -- and probes where neither the register tiles nor lbm_wave run -- are taken behind pieces of the step loop that end on their sample steps
   (each piece a launch of that flavour), by the small kernels the single calls fall back to (a 1024 x 1024 run with forces and mean_every = 100 stays on the
   register tiles and pays their per-run fixed cost once per 100 steps).  One observer alone simply runs its own call.
   Info "observed_in_kernel": bits 1 forces, 2 probes, 4 means, 8 snapshots -- what the last lbm_run_observed took inside
   register-tile launches; "observed_in_wave": bits 1 forces, 2 probes -- what it took inside lbm_wave launches (then
   "observed_in_kernel" reads 0); "observed_pieces": the step-loop pieces it ran (1 = the whole call in one).  What the four
   single calls' "*_in_kernel" keys read after lbm_run_observed is unspecified.  lbm_last_run_ms: the sums over the pieces.
   LBM_EINVAL with nothing queued and the lattice untouched: nsteps < 0; forces wanted without bodies; probes wanted
   without a probe set; probes or means wanted with every <= 0 or no sample step in nsteps; fields_every < 0 (0, or no
   sample step: legal, nothing written); a device pointer on another device than the slabs'.  LBM_ENOMEM likewise when a
   staging, table or partial buffer does not fit.  Rank contexts agree on room and on the path before anything is queued.
   Overlapping observers of one kind with different periods: not offered. */
int lbm_run_observed(lbm_ctx* ctx, int nsteps, float* av_vels, const lbm_observe* what);

/*
 * Snapshots of a window: a sub-rectangle of the lattice, optionally every sx-th column and sy-th row of it, stored from
 * inside the kernels (a movie of the wake behind a body, a quarter-resolution view of the whole channel).  Traffic,
 * staging and host copy scale with the window, not with the lattice.
 * Layout (plain C): sizeof(lbm_window) = 24, six ints, no padding.
 */
typedef struct { int x0, y0, nx, ny, sx, sy; } lbm_window;
/* The window holds the cells (x0 + c sx, y0 + r sy), c in [0, nx), r in [0, ny), of the GLOBAL lattice (in every mode).
   Points are sampled, not averaged.  It does not wrap: nx, ny, sx, sy >= 1; x0, y0 >= 0; x0 + (nx - 1) sx < lattice nx,
   y0 + (ny - 1) sy < lattice ny (checked in 64-bit arithmetic).  The whole lattice at stride 1 is a legal window.

   lbm_run that also writes window_out[m][win->ny][win->nx][4] = u_x, u_y, |u|, pressure of the window's cells after steps
   every, 2 every, ..., m every (m = nsteps / every; every = 0, or no sample step in nsteps: none, exactly lbm_run, nothing
   written, window_out may be NULL).
   Definition, bit for bit: window_out[j][r][c][:] equals fields_out[j][win->y0 + r win->sy][win->x0 + c win->sx][:] of
   lbm_run_sampled(ctx, nsteps, av_vels, every, fields_out) from the same state with the same options; a blocked cell
   reads 0, 0, 0, density * (1.f / 3.f) (in float).  av_vels, the lattice and everything after the call are what they are
   for lbm_run_sampled on the same context: lbm_run's bits wherever the register tiles or lbm_wave took the window, within
   float rounding of the per-step sum on the split path.  window_out: host memory, or device memory of the device that holds every slab of
   the context (then nothing is copied to the host).  Single-process contexts with several slabs write the whole window.
   Rank contexts: the window is global on every rank and every rank's array has the full window shape; a rank fills the
   window rows that lie in its own lattice rows (lbm_window_rows with lbm_slab_rows tells which) and writes +0.0f to the
   others; no communication is added.
   Which kernels take the window:
   - The register-tile engines take it inside their kernels (info "window_in_kernel" = 1), in the probe flavour fed per-slab
     window tables (one word per cell of a tile that holds a window cell: its place in the window + 1): on a sample step
     one 16-byte store per window cell, a row without one costs a scalar branch, a tile without one nothing.  The probe
     set of lbm_set_probes and its tables are untouched.  Host output: each slab stages its own window rows only
     (16 m win->nx rows bytes), copied out after the run.  av_vels is lbm_run's, bit for bit.
   - Where lbm_wave runs (a lattice alone on its GPU with time_block 4, 6 or 8 and the wave kernel, nsteps >= time_block;
     the register tiles refuse first), the window rides in its launches (info "window_in_wave" = 1, "window_in_kernel" =
     0): a window flavour of lbm_wave tests the row of a sample level against the window (wave-uniform), then each of a
     lane's cells against its columns (arithmetic on the six ints, no map, no division), and stores a window cell's four
     floats in one 16-byte store; passes without a sample step run the plain kernel, one kernel per pass; the steps left
     over behind the last full pass go as lbm_run's do, with lbm_derive_window behind those that are sample steps.
     av_vels is lbm_run's, bit for bit.  Host output goes through ONE device staging of m windows; if that does not fit
     (or a window's extent times its stride passes 2^32) the run takes the split path: the same bits, no error.
   - Every other engine -- contexts where lbm_march runs, slabs with neighbours under copy / RCCL / streaming peer-to-peer,
     rank contexts, runs shorter than time_block, a register-tile run that gave up -- runs the steps in pieces of `every`
     with lbm_derive_window behind each piece on every local slab: one thread per window cell of the slab (correct, not
     fast; the same bits; both keys read 0).
   LBM_EINVAL with nothing queued and the lattice untouched: NULL ctx or win; a window outside the rules above; nsteps < 0;
   every < 0; window_out NULL with m > 0; a device pointer on another device than the slabs'; m x window floats past the
   address space.  LBM_ENOMEM likewise when a staging or table does not fit and no path with the same bits is left.
   Rank contexts agree on room and on the path before anything is queued.
   Not offered: windows inside lbm_run_observed (its struct layout is frozen), block-averaged downsampling, windows that
   wrap, windows from the command-line tool.  (Means and second moments over a window: lbm_run_window_stats.) */
int lbm_run_window(lbm_ctx* ctx, int nsteps, float* av_vels, int every, const lbm_window* win, float* window_out);
/* Host arithmetic only (no device needed, as lbm_plan_tiles): validates win against an nx x ny lattice (LBM_EINVAL: not a
   legal window, or row_begin > row_end) and returns which window rows lie in lattice rows [row_begin, row_end): rows
   *first .. *first + *count - 1 of the window (*count may be 0; first and count may be NULL). */
int lbm_window_rows(const lbm_window* win, int nx, int ny, int row_begin, int row_end, int* first, int* count);

/*
 * lbm_run_stats over a window: the means and second moments of the window's cells, with device memory, traffic and host
 * copy that scale with the window, not with the lattice (Reynolds stresses in the wake behind a body without paying for
 * the whole channel).  stats_out: float[win->ny][win->nx][8], host memory, or device memory of the device that holds every
 * slab; the rules are those of lbm_run_window (the window, global in every mode; rank contexts) and of lbm_run_stats.
 * Definition, bit for bit: let W_j[r][c] be sample j of lbm_run_window(ctx, nsteps, av_vels, every, win, ...) from the same
 * state with the same options, m = nsteps / every, and p0 = density * (1.f / 3.f).  Then stats_out[r][c][0..7] is what
 * lbm_run_stats defines from X_j = W_j[r][c]: S_j = S_(j-1) + X_j and T_j = T_(j-1) + Q_j with
 * Q_j = (x * x, y * y, x * y, (w - p0) * (w - p0)), float arithmetic with one rounding per operation, no fma, in step order,
 * starting from +0.0f; each sum divided by (float)m, correctly rounded.  So stats_out[r][c][:] equals lbm_run_stats'
 * stats_out[win->y0 + r win->sy][win->x0 + c win->sx][:], and a blocked cell reads as it does there.
 * av_vels, the lattice and everything after the call are bit-identical to lbm_run(ctx, nsteps, av_vels) wherever the
 * register tiles or lbm_wave ran the steps; on the split path they are equal within rounding of the per-step sum.
 * Rank contexts: as lbm_run_window -- every rank's array has the full window shape, a rank fills the window rows that lie
 * in its own lattice rows and writes +0.0f to the others; no communication is added.
 * Device memory for the sums: 32 bytes per window cell of a slab, never per lattice cell.
 * LBM_EINVAL with nothing queued and the lattice untouched: NULL ctx, win or stats_out; a window outside lbm_window's
 * rules; nsteps < 0; every <= 0; m = 0; a device pointer on another device than the slabs'.  LBM_ENOMEM likewise when the
 * sums do not fit -- the ranks of a rank context agree on that first; LBM_EHIP after a failed peer-to-peer wait.
 * Which kernels take the sums (info keys reset at the start of each call):
 * - Where lbm_wave runs (a lattice alone with time_block 4, 6 or 8 and the wave kernel, nsteps >= time_block), the sums
 *   ride in its launches ("window_stats_in_wave" = 1): a window-stats flavour of lbm_wave tests a sample level's row and
 *   then each of a lane's cells against the window as the window flavour does (no map, no division) and adds a window
 *   cell's eight terms into its 32-byte record as the stats flavour does, the record index 64-bit; one kernel per pass of K
 *   steps, a pass without a sample step runs the plain kernel; the steps left over behind the last full pass go as
 *   lbm_run's do, with the add kernel behind those that are sample steps.  A window whose extent times its stride passes
 *   2^32 takes the split path: the same bits, no error.
 * - On the register tiles, alone and across slabs ("window_stats_in_kernel" = 1), the call runs in pieces of c every steps:
 *   each piece is one launch of the flavour lbm_run_observed's pieces run in, fed the window's tables as its probe tables
 *   (the probe set of lbm_set_probes and its table stay untouched); it stores its c samples of the slab's window rows
 *   into a device staging, and a fold kernel behind it adds them, in step order, into the sums.  That flavour folds a cut
 *   piece's last step sum as a whole run folds it, so av_vels is lbm_run's bits wherever the call is cut.  c is the option
 *   "window_stats_chunk", or automatic (0): as many samples as 64 MiB of staging per slab hold, at least 1, at most m.
 *   The steps past m every run as one more piece without samples.  A piece that gives up has stepped nothing; the call
 *   continues from the same step on the split path.
 * - Everywhere else -- lbm_march, slabs or ranks off the tiles, runs shorter than time_block, a lattice that does not tile
 *   -- the steps run in pieces of `every` with an add kernel behind each on every slab that holds a window row: one thread
 *   per window cell of the slab.  The same adds in the same order, the same bits; both keys read 0.
 * "window_stats_pieces": the step-loop pieces of the last call (1 where lbm_wave took it).
 * Not offered: window stats inside lbm_run_observed (its struct layout is frozen); window stats under a schedule; windows
 * that wrap; block averaging (points are sampled); the command-line tool.
 */
int lbm_run_window_stats(lbm_ctx* ctx, int nsteps, float* av_vels, int every, const lbm_window* win, float* stats_out);

/*
 * The acceleration as an input of the run (a ramp over the first thousand steps instead of an impulsive start, a pulsatile
 * or oscillatory channel, a loop closed on av_vels) -- the one PARAMETER of a context that is not frozen at lbm_create (the
 * obstacle map and the lattice are inputs too: lbm_set_obstacles, lbm_write_state, below).
 */
/* Replaces the context's acceleration for every later run (lbm_run and all lbm_run_* calls).  Only stores the value: queues
   nothing, rebuilds no table, changes no engine choice (every run makes its accelerate constants from the context's
   parameters when it starts).  Info "accel" reads it.  Rank contexts: the caller sets the same value on every rank.
   LBM_EINVAL: NULL ctx, or a non-finite value (the old value is kept). */
int lbm_set_accel(lbm_ctx* ctx, float accel);
/* lbm_run with step t (0-based within the call) driven by accel[t] instead of the context's value.
   Definition: step t of the call is the reference's step (accelerate, stream, bounce-back, collide; d2q9-bgk.c:228-1813)
   with params.accel = accel[t].  The two accelerate constants of a step are made on the host, in float, by the expression
   every run uses: density * accel[t] / 9.f and density * accel[t] / 36.f -- a schedule whose every entry equals the
   context's acceleration is therefore lbm_run, constant for constant.  Any finite value is legal, of either sign, and zero:
   what the accelerate guard (d2q9-bgk.c:238-241) does with it is what the reference's statements do with that value;
   nothing is special-cased.  accel: host memory, float[nsteps].
   The lattice and everything after the call are bit-identical to
       for (t = 0; t < nsteps; ++t) { lbm_set_accel(ctx, accel[t]); lbm_run(ctx, 1, ...); }
   from the same state with the same options, on every engine -- except that the context's own acceleration is untouched
   by lbm_run_driven.  av_vels: the engine's own per-step sums; equal to that loop's within float rounding of the per-step
   sum; with a constant schedule equal to the context's acceleration bit-identical to lbm_run's wherever the register tiles
   ran, and in lbm_wave for the steps inside full passes.
   Which kernels take the schedule:
   - The register-tile engines, alone and across slabs, run a flavour of their own (info "driven_in_kernel" = 1): the
     (a1, a2) pairs go to the device before the launch (8 bytes per step), and the waves that hold the accelerate row read a
     step's pair with one scalar load.  If the flavour cannot be resident, the table has no room or the run gives up (lattice
     untouched), the one-step path below runs the same schedule.
   - Where lbm_wave runs (a lattice alone on its GPU with time_block 4, 6 or 8 and the wave kernel, nsteps >= time_block),
     a driven flavour of lbm_wave takes the K pairs of a pass in its arguments (info "driven_in_wave" = 1,
     "driven_in_kernel" = 0; "wave_launches" grows by one per pass); the steps left over behind the last full pass go one
     at a time through the one-step kernel, each with its own constants.
   - Every other engine -- contexts where lbm_march or lbm_sweep2 would run, slabs with neighbours under copy / RCCL /
     streaming peer-to-peer, rank contexts off the register tiles, runs shorter than time_block, a register-tile run that
     gave up -- runs the one-step kernel, each step with its own constants (correct, not fast; the same lattice bits; both
     keys read 0).
   Rank contexts: every rank passes the same schedule and gets the global av_vels, as with lbm_run; the ranks agree on the
   path before anything is queued.
   LBM_EINVAL with nothing queued and the lattice untouched: NULL ctx; nsteps < 0; accel NULL with nsteps > 0; a non-finite
   entry (the message names its index).  LBM_ENOMEM likewise when the device table does not fit and no path with the same
   bits is left (the one-step path needs no table).  nsteps = 0: success, nothing runs.
   Observers under a schedule: lbm_run_driven_observed, below.
   Not offered: a schedule inside the single observer calls or lbm_run_window (lbm_run_driven_observed with one observer
   serves the former); schedules for omega or density; a schedule from the command-line tool; device-memory schedules. */
int lbm_run_driven(lbm_ctx* ctx, int nsteps, float* av_vels, const float* accel);
/* lbm_run_driven(ctx, nsteps, av_vels, accel) that also fills the outputs named in `what` (lbm_observe, as lbm_run_observed
   takes it: layout, periods, rank conventions, host or device memory per pointer, forces in host memory).  what NULL, or
   all four pointers NULL: exactly lbm_run_driven, av_vels bits included.  One observer alone is legal (there are no driven
   single calls: this call serves them).  Sample steps count from the start of the call, the three periods are independent.
   The context's own acceleration is untouched.
   Definition: let X_t be what lbm_final_state returns after step t of the loop
       lbm_set_accel(ctx, accel[t]); lbm_run(ctx, 1, ...);
   from the same state with the same options.  Probes, snapshots and means are defined from X_t exactly as lbm_run_probes,
   lbm_run_sampled and lbm_run_mean define theirs from lbm_run_sampled's snapshots (the float sum in step order, the
   correctly rounded division, the blocked cells' constants, the -0 handling), and are bit for bit that on every engine.
   forces[t] is F_b (lbm_run_forces) on the lattice stored after step t of that loop.
   Bit for bit, and to rounding:
   - the lattice and everything after the call: lbm_run_driven's, hence the loop's, on every engine;
   - forces where lbm_wave or the one-step kernel took them: the bits of lbm_set_accel(accel[t]); lbm_run_forces(ctx, 1, ...)
     per step under engine 1, time_block 1 ("the bits of the one-step path"); where the register tiles took them: their own
     fixed-order sums, as for lbm_run_forces there;
   - with a constant schedule equal to the context's acceleration, forces and av_vels are bit-identical to
     lbm_run_observed's with the same `what` on the same context and options, wherever the register tiles ran, and in
     lbm_wave for the steps inside full passes;
   - av_vels otherwise: lbm_run_driven's contract (the loop's within float rounding of the per-step sum).
   Which kernels run:
   - The register-tile engines, alone and across slabs: EVERY piece of the call runs one flavour, forces and probes under
     a schedule, whichever observers are wanted (one that is not gets a table of -1s).  The whole call's (a1, a2) pairs go
     to the device once; a piece that starts `done` steps into the call reads from pair `done` on, by scalar loads.  Forces
     and probes cut no piece; means and snapshots are taken behind pieces that end on their sample steps.
   - Where lbm_wave runs (lbm_run_driven's terms, and lbm_run_forces' / lbm_run_probes' for their maps): one flavour of
     lbm_wave with forces, probes and the K pairs of a pass (an observer that is not wanted marks nothing in its map);
     forces and probes cut no piece; means and snapshots cut pieces at their sample steps and are taken behind them; the
     steps left over behind the last full pass of a piece go through the one-step kernel, each with its own pair, forces and
     probes taken behind them.  Maps that do not fit: the one-step path, no error.
   - Every other engine, pieces shorter than time_block, a register-tile piece that gave up or whose flavour is not
     resident (it has stepped nothing: that piece again from the same step, off the tiles for the rest of the call): the
     one-step kernel with each step's own constants, and behind a step the small kernels it calls for.  Correct, not fast,
     the same bits; the three keys below read 0.
   Info "driven_observed_in_kernel" (bits 1 forces, 2 probes, 4 means, 8 snapshots: what the last call took inside
   register-tile launches), "driven_observed_in_wave" (bits 1 forces, 2 probes), "driven_observed_pieces" (the step-loop
   pieces of the last call; 0 where the whole call took the one-step path).  What "observed_*", "driven_in_*" and the single calls' "*_in_kernel" / "*_in_wave" keys read
   after this call is unspecified.
   Refusals, all with nothing queued and the lattice untouched -- LBM_EINVAL: NULL ctx; nsteps < 0; accel NULL with
   nsteps > 0; a non-finite entry (the message names its index); forces wanted without bodies; probes wanted without a
   probe set; probes or means wanted with every <= 0 or no sample step in nsteps (nsteps = 0 included); fields_every < 0;
   a device pointer on another device than the slabs'.  LBM_ENOMEM when a staging, table or partial buffer does not fit and
   no path with the same bits is left (a schedule table that does not fit: the call keeps off the register tiles and does
   not fail).  nsteps = 0 otherwise: success, nothing runs.  Rank contexts agree on room and on the path before anything is
   queued.
   Not offered: windows under a schedule; schedules for omega or density; device-memory schedules; the command-line tool. */
int lbm_run_driven_observed(lbm_ctx* ctx, int nsteps, float* av_vels, const float* accel, const lbm_observe* what);

/* GPU time of the step loop of the last lbm_run, from HIP events on the
 * compute stream of slab 0 (ms), and host wall time of the same region. */
int lbm_last_run_ms(const lbm_ctx* ctx, double* gpu_ms, double* wall_ms);

/* Copies the current lattice back in the reference's AoS layout
 * (what `cells` holds after the swap at d2q9-bgk.c:190).
 * Single-process contexts: the whole lattice, float[ny*nx*9].
 * Rank contexts: this rank's rows only, float[(row_end-row_begin)*nx*9]. */
int lbm_read_state(lbm_ctx* ctx, float* cells_out);

/*
 * Live inputs: the obstacle map and the lattice of a context replaced in place (shape iteration, a valve, a moving body,
 * a restart from a saved state, a perturbed spun-up flow) without destroying and creating it again.  Code objects,
 * buffers, tiling, mailboxes, peer handles, options, acceleration and the probe set all stay.  Neither call communicates.
 */
#define LBM_REFILL_KEEP 0
#define LBM_REFILL_REST 1
/* Replaces the obstacle map for every later call.  obstacles: int[ny*nx] over the GLOBAL lattice, host memory, nonzero =
   blocked -- whatever lbm_create accepts as a map; in rank mode the global array on every rank (as lbm_create_rank and
   lbm_set_bodies take theirs).
   Definition: let S be what lbm_read_state would return just before the call.  Afterwards the context behaves, bit for bit
   and for every later call (lbm_run, every lbm_run_*, lbm_read_state, lbm_final_state, lbm_av_velocity, lbm_reynolds,
   lbm_total_density, info "fluid_cells"), like a fresh context created with lbm_create*(params, obstacles, S', ...) on the
   same slabs, devices and exchange, given the same options, the same acceleration (lbm_set_accel's value) and the same
   probe set.
   - LBM_REFILL_KEEP: S' = S.  A cell that turns from blocked to fluid keeps the populations bounce-back left in it.
   - LBM_REFILL_REST: S' = S, except that every cell blocked under the old map and fluid under the new one holds the rest
     equilibrium of lbm_create's NULL-cells start: density * 4.f / 9.f, density / 9.f (x 4), density / 36.f (x 4), in float.
     The total density therefore CHANGES with such a call (by the refilled cells' rest mass less what they held).
   A cell that turns from fluid to blocked keeps its populations under either mode.
   What survives: the probe set, the options, the acceleration, the engine choice, the tiling, the mailbox tag sequence of
   the register tiles.  What does not: the body labelling is cleared, as by lbm_set_bodies(ctx, NULL, 0) -- the library
   keeps no label array, and labels are validated against the map; label the new map again before lbm_run_forces.
   One kernel per slab on its compute stream reads the old bytes and the new map, writes the new bytes, refills and counts;
   the call returns when it is complete.
   ORDERING: nothing is communicated.  In rank contexts, and wherever peer-to-peer neighbours read each other's obstacle
   bytes in place, EVERY rank must have returned from this call before ANY rank starts a run (a barrier of the caller's
   choice, as for lbm_destroy); every rank passes the same map.
   Info "obstacle_updates": the successful calls on this context.  "refilled_cells": the cells the last call refilled in
   this process's rows (0 under LBM_REFILL_KEEP).
   Refusals, with the map unchanged, the lattice untouched and nothing queued -- LBM_EINVAL: NULL ctx or map, a refill value
   other than the two; LBM_EHIP: a context whose peer-to-peer halo wait failed earlier; LBM_ENOMEM: a staging buffer that
   does not fit.
   Not offered: a per-step geometry schedule inside the kernels; maps in device memory; the command-line tool. */
int lbm_set_obstacles(lbm_ctx* ctx, const int* obstacles, int refill);
/* The inverse of lbm_read_state, same layout and conventions: single-process contexts take the whole lattice,
   float[ny*nx*9]; rank contexts take this rank's rows, float[(row_end-row_begin)*nx*9] -- lbm_read_state's buffer goes
   straight back in.  cells: host memory, or device memory of the device that holds every slab of the context (as the
   outputs of the lbm_run_* calls); device memory is converted straight from the caller's pointer, nothing is staged through
   the host (work queued on the caller's own streams that writes `cells` must be complete).
   Definition: afterwards the context is, bit for bit and for every later call, a fresh context created with the same map
   and `cells`, given the same options, acceleration, probe set and bodies -- all kept.  Values are not inspected (NaNs,
   negative zeros and the contents of blocked cells go in as they are, as in lbm_create).  Holds after any number of steps.
   ORDERING, as for lbm_set_obstacles: nothing is communicated; where neighbouring ranks read each other's rows in place,
   every rank's last run has returned before any rank writes, and every rank has returned from this call before any runs.
   Refusals, all with the lattice untouched -- LBM_EINVAL: NULL arguments, a device pointer on another device than the
   slabs'; LBM_EHIP: a context whose peer-to-peer halo wait failed earlier; LBM_ENOMEM: a staging buffer that does not fit.
   Not offered: the command-line tool. */
int lbm_write_state(lbm_ctx* ctx, const float* cells);

/* Replaces: av_velocity() and calc_reynolds(), d2q9-bgk.c:2665-2714, 2893-2898,
 * evaluated on the resident lattice (global value in every mode). */
int lbm_av_velocity(lbm_ctx* ctx, float* out);
int lbm_reynolds(lbm_ctx* ctx, float* out);

/* Sum of all 9*nx*ny distribution values (total_density(), d2q9-bgk.c:2900-2916);
 * constant from step to step.  Accumulated in double. */
int lbm_total_density(lbm_ctx* ctx, double* out);

/* Replaces: the per-cell arithmetic of write_values(), d2q9-bgk.c:2935-2976.
 * out[4*(ii + jj*nx) + {0,1,2,3}] = u_x, u_y, |u|, pressure, computed on the GPU
 * (blocked cells: 0, 0, 0, density * (1.f / 3.f), the product in float, as the reference's c_sq = 1.f / 3.f gives
 * it; at some densities, 0.3 and 0.02 among them, that is one ulp from density / 3.f).  Same slab-local convention as
 * lbm_read_state in rank mode. */
int lbm_final_state(lbm_ctx* ctx, float* out);

/* Replaces: finalise(), d2q9-bgk.c:2871-2890.
 * Rank contexts with peer-to-peer halos: the neighbours' last launches still store into this
 * context's halo block, so destroy it only after EVERY rank's last lbm_run has returned
 * (a barrier of the caller's choice); the RCCL and single-process forms need no such care. */
int lbm_destroy(lbm_ctx* ctx);

/*
 * Parity shim with the reference's own call shape (d2q9-bgk.c:98,228):
 * one step on host arrays.  Like the reference it applies the accelerate
 * phase to `cells` IN PLACE (row ny-2), fully overwrites `tmp_cells`, reads
 * `obstacles`, and returns the average speed through *av_vel.  Uploads and
 * downloads every call: for tests, not for speed.
 */
int lbm_timestep(const lbm_param* params, float* cells, float* tmp_cells,
                 const int* obstacles, float* av_vel);

/*
 * The tiling the register-resident engine (lbm_regtile: the whole lbm_run in one launch, replacing the loop of
 * d2q9-bgk.c:180-201) would give a lattice -- or each of several equal slabs -- of nx columns x rows rows on a device
 * with `compute_units` CUs that holds `slabs_per_device` such slabs: 64-column tiles of *tile_rows rows, one per CU,
 * *rows_per_wave rows per wavefront.  Host arithmetic only (no device needed).  LBM_EINVAL: it does not tile.
 */
int lbm_plan_tiles(int nx, int rows, int slabs_per_device, int compute_units, int* tile_rows, int* rows_per_wave);

/* Tuning / introspection (never needed for correctness; the table of keys is INTEGRATION.md section 3).
 * Options: "engine" (0 auto, 1 streaming kernels, 3 register tiles -- alone or across slabs -- or fail), "time_block"
 * (1, 2, 4, 6, 8 steps per pass), "march_kernel", "march_rows", "wave_rows", "wave_cols" (1, 2), "regtile" (tiling),
 * "regtile_async" (0, 1), "regtile_tag" (test hook: the next mailbox tag), "window_stats_chunk" (the most sample steps one
 * register-tile piece of lbm_run_window_stats holds; 0 automatic; below 0: LBM_EINVAL), "kernel_variant" (bits: 1 fast rcp / sqrt, 2 / 4 nontemporal stores / loads, 8 the reference's
 * form of the speed sum, d2q9-bgk.c:1783-1811, 256 one-step kernel only), "vector_width", "t2_threads".
 * Info: "engine_last", "engine_next", "samples_in_kernel" (1: the last lbm_run_sampled's snapshots came from the register
 * tiles), "forces_in_kernel" (1: the last lbm_run_forces took its sums inside the register tiles),
 * "forces_in_wave" (1: the last lbm_run_forces took its per-cell contributions inside lbm_wave launches),
 * "mean_in_kernel" (1: the last lbm_run_mean took its sums inside the register tiles),
 * "samples_in_wave" (1: the last lbm_run_sampled took its snapshots inside lbm_wave launches),
 * "mean_in_wave" (1: the last lbm_run_mean took its sums inside lbm_wave launches),
 * "stats_in_wave" (1: the last lbm_run_stats took its sums inside lbm_wave launches),
 * "wave_launches" (the lbm_wave kernels this context has launched on a lattice alone, every flavour: one per pass of K steps),
 * "probes_in_kernel" (1: the last lbm_run_probes took its values inside the register tiles),
 * "probes_in_wave" (1: the last lbm_run_probes took its values inside lbm_wave launches),
 * "window_in_kernel" (1: the last lbm_run_window took its window inside the register tiles),
 * "window_in_wave" (1: the last lbm_run_window took its window inside lbm_wave launches),
 * "window_stats_in_wave" (1: the last lbm_run_window_stats took its sums inside lbm_wave launches),
 * "window_stats_in_kernel" (1: ... its samples inside the register tiles), "window_stats_pieces" (... the step-loop
 * pieces it ran), "window_stats_chunk" (the option's value), "observed_in_kernel",
 * "observed_in_wave", "observed_pieces" (lbm_run_observed), "accel" (the context's acceleration: lbm_create's, or the last lbm_set_accel's),
 * "driven_in_kernel" (1: the last lbm_run_driven ran inside the register tiles), "driven_in_wave" (1: the last lbm_run_driven
 * ran its groups of K steps inside lbm_wave launches), "driven_observed_in_kernel", "driven_observed_in_wave",
 * "driven_observed_pieces" (lbm_run_driven_observed), "resident_fallback", "time_block_active", "march_kernel", "wave_rows",
 * "wave_cols_active", "wave_out_cols", "regtile", "regtile_blocks_per_cu", "exchange", "compute_units", "fluid_cells",
 * "obstacle_updates", "refilled_cells" (lbm_set_obstacles), "pitch", "hbm_bytes". */
int lbm_set_option(lbm_ctx* ctx, const char* key, long value);  /* e.g. "kernel_variant" */
int lbm_get_info(const lbm_ctx* ctx, const char* key, double* value);

#ifdef __cplusplus
}
#endif
#endif /* LBM_MI355X_H */
