/* mw_quench.h -- C ABI of libmw_quench.so: inherent structures.  Every one of many periodic boxes is moved downhill on the
 * full-box mW energy at fixed cell, from the given positions to the local minimum below them (or for max_iter steps), on a
 * gfx950 device.  Every box follows its own trajectory; no host decision enters it.
 *
 * A library of its own beside libmw_hip.so (include/mw_energy.h) and the analysis libraries (include/mw_tet.h and its
 * siblings): it needs cells and positions only, so it takes plain arrays and works on any configuration, with or without
 * mw_init in the same process.  It has its own stream, scratch memory and event timers.  Its results are plain positions
 * again: they go straight into the other libraries' entries.
 *
 * Inputs.  `cells` holds 9 doubles per box in the layout of mw_set_cell (cells[9 b + 3 k + a] = component a of h_(k+1)),
 * `pos` holds nwater positions in bohr as [box][nwater][3], wrapped or not.  Energies are in Hartree, forces in Hartree / bohr,
 * times in atomic units with unit mass.
 *
 * Energy.  The one mw_model_energy evaluates: with the entries of molecule i all pairs (j, n), n an integer lattice
 * translation, (j, n) != (i, 0), d = r_j + H n - r_i and |d|^2 < (a sigma)^2,
 *   E = sum_i [ 1/2 sum_k phi(r_k) + lambda eps 1/2 sum_{k != l} g_k g_l (u_k . u_l - cos0)^2 ],
 * phi and g from pair_terms of mw_common.hip.h.  An image of i itself is an entry of i: it is part of the energy and of i's
 * moments and exerts no force (its d is constant).  F = -dE/dr from the moment formulation: the force on
 * a molecule is one lane's sum over its own moments and its neighbours' moments; there are no floating-point atomics.
 *
 * Supported range.  w_k = volume / |h_l x h_m| are the perpendicular widths of the cell.  Supported:
 * a sigma (1 + 1e-9) <= min_k w_k for every box of the call (a sigma = 8.13808... bohr; the cells are sorted at every
 * iteration, so this is the radius that must fit and no wider one); 1 <= nwater <= 2^22; 1 <= nboxes <= 2^24;
 * 0 <= max_iter <= 10^6; ftol > 0 and finite; every fire parameter as below.  Anything else (NaN or inf included) is
 * rejected with a message that names the entry, the argument and the first offending box, and nothing is launched or written.
 *
 * Minimiser: FIRE, per box, unit mass.  fire[8] = (dt0, dtmax, maxstep, alpha0, f_alpha, f_inc, f_dec, n_min); NULL means
 * MW_QUENCH_FIRE_DEFAULTS = (20, 200, 0.2 bohr, 0.1, 0.99, 1.1, 0.5, 5).  Each must be positive and finite, with
 * f_dec < 1 < f_inc, alpha0 <= 1 and f_alpha < 1.  State: x = pos, v = 0, dt = dt0, alpha = alpha0, npos = 0.  At iteration
 * t = 0, 1, ...:
 *   1. E and F at x; fmax = the largest |F| over molecules and components.
 *   2. fmax <= ftol: the box is converged with iterations = t and stops.
 *   3. t = max_iter: it stops unconverged.
 *   4. P = sum F.v.
 *   5. P > 0: npos += 1; v = (1 - alpha) v + alpha F sqrt(sum v^2 / sum F^2); then if npos > n_min:
 *      dt = min(dt f_inc, dtmax), alpha *= f_alpha.
 *   6. else: npos = 0, v = 0, dt *= f_dec, alpha = alpha0.
 *   7. v += dt F, dx = dt v.
 *   8. if the largest |dx_i| (Euclidean, per molecule) exceeds maxstep, all of dx is scaled by maxstep over it.
 *   9. x += dx.
 * max_iter = 0 is a single-point evaluation of E and F.  FIRE is not monotone: some steps raise E.  Positions are never
 * wrapped: pos_out is the input plus the accumulated steps, so pos_out - pos is the displacement, and as the forces add up
 * to zero the centre of mass stays where it was.
 *
 * Outputs (any may be NULL):
 *   pos_out[nboxes][nwater][3] doubles: the final positions.
 *   forces[nboxes][nwater][3] doubles: the forces at the final positions.
 *   stats[nboxes][6] doubles: E at the start, E at the end, fmax at the start, fmax at the end, the largest and the rms
 *     displacement |pos_out_i - pos_i| over the molecules.
 *   iters[nboxes][2] ints: iterations, converged 0/1.
 *
 * Arithmetic (part of the contract).  H^-1 is formed once per box on the host; at every evaluation s = H^-1 x is reduced to
 * [0, 1) once per molecule and d = H (ds + n) from the difference of fractional coordinates plus the integer image shift;
 * everything is spelled out in fma / mul / add with contraction off.  A molecule's moments, energy and force are one
 * lane's sums in the order of the walk of its geometry (below).  The box sums (E, P, sum v^2, sum F^2 and the maxima) run
 * in a fixed order: the lanes of a wavefront through one DPP tree, the wavefronts of a workgroup in order, the workgroups
 * of a box in order.  A box that has stopped is frozen on the device at that iteration, whatever the others do.
 * Hence the bytes of a box's results depend on its cell, its positions, ftol, max_iter and fire alone: not on the other boxes
 * of the call, on batch versus single calls, on host versus device pointers, on chunking, on how often the host looks at the
 * stop flags or on how many iterations one launch carries.
 *
 * Geometry.  Which of two geometries a box takes depends on nwater alone.
 *   general (nwater > 64): per iteration the counting sort into the fractional cell grid of a sigma (the grid rules of
 *     include/mw_tet.h), a moment pass (one lane per molecule in sorted order over the 27 cells: the ten moments and the
 *     molecule's energy), a force pass (a second walk over the molecule's own moments and those of every entry; the
 *     workgroup's partial sums) and the step (the box decision by one workgroup per box, the velocity mix, the move).  The
 *     host enqueues a block of iterations, reads the stop flags once per block and ends the chunk when all have stopped.
 *   small (nwater <= 64): one wavefront per box, four boxes per workgroup, lane = molecule, fractional positions and
 *     moments in LDS, every reduction through DPP; many iterations run inside one launch with no traffic to memory between
 *     them, at most a fixed number per launch, the state carried in scratch from launch to launch.
 * Diagnostic switches read by mw_quench_init (they must not and do not change a byte of any result): MW_QUENCH_LOOK, the
 * iterations between two looks of the host at the stop flags (1..4096, default 32), and MW_QUENCH_SLICE, the iterations one
 * launch of the small geometry carries (1..256, default 64).
 *
 * Scratch.  Positions, velocities, forces, moments, the cell tables and the FIRE scalars of every box live in scratch
 * memory; a call is processed in chunks of as many boxes as fit the budget: 256 MiB, or MW_QUENCH_SCRATCH_MB (MiB, read
 * by mw_quench_init), and each chunk is quenched to its end.  A box that does not fit alone is an error.
 *
 * Out of scope: relaxation of the cell, the virial, a Fortran binding, and any change to libmw_hip.so.
 *
 * Every function returns 0, or nonzero with the reason in mw_quench_last_error().  A rejected call launches nothing and
 * writes nothing; its message names the entry and the argument, and box indices in messages count from 0.  Arguments are
 * checked before the library's state, so a call with bad arguments says so with or without a device.  The library lives on
 * the device given to mw_quench_init: every function that touches it makes that device current for the call and puts the
 * caller's current device back before it returns.
 */
#ifndef MW_QUENCH_H
#define MW_QUENCH_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_QUENCH_PLAN_FIELDS 9
#define MW_QUENCH_MAX_ITER 1000000
#define MW_QUENCH_FIRE_DEFAULTS {20.0, 200.0, 0.2, 0.1, 0.99, 1.1, 0.5, 5.0}

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0.  A failed init
 * gives back the stream and events it made and leaves the library not initialised. */
int mw_quench_init(int device);
int mw_quench_finalize(void);
int mw_quench_is_initialised(void);
const char *mw_quench_last_error(void);

/* Host pointers. */
int mw_quench_compute(int nboxes, int nwater, const double *cells, const double *pos, double ftol, int max_iter,
                      const double *fire, double *pos_out, double *forces, double *stats, int *iters);
/* Device pointers on the library's device for every array but `fire`, which is always 8 doubles on the host or NULL.  Work
 * queued on the device before the call is waited for, and the results are complete on return. */
int mw_quench_compute_device(int nboxes, int nwater, const double *cells, const double *pos, double ftol, int max_iter,
                             const double *fire, double *pos_out, double *forces, double *stats, int *iters);

/* The launch rules for nboxes boxes of nwater molecules with the cell `cell` (9 doubles, host) -- host arithmetic only,
 * no device and no mw_quench_init needed (the scratch budget is then the default one).  Writes
 * min(nout, MW_QUENCH_PLAN_FIELDS) ints:
 *   [0] boxes per chunk   [1] chunks = ceil(nboxes / [0])   [2] 1: small geometry, 0: general
 *   [3] [4] [5] the cell grid g_1, g_2, g_3 of a sigma (the small geometry reports it and does not use it)
 *   [6] LDS of a workgroup, bytes (the largest of the kernels)   [7] scratch per box, bytes
 *   [8] boxes per workgroup (small) or 0 */
int mw_quench_plan(int nwater, const double *cell, int nboxes, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box. */
int mw_quench_last(int *out, int nout);
/* Event timers of the last call, summed over its iterations and chunks: the sort, the moment pass, the force pass and the
 * step (decision, velocity mix and move).  The small geometry is one kernel: its time is reported as the force pass and the
 * others are 0. */
int mw_quench_elapsed_ms(float *sort, float *moments, float *forces, float *step);

#ifdef __cplusplus
}
#endif
#endif
