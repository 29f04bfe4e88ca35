/* mw_npt.h -- C ABI of libmw_npt.so: molecular dynamics at constant pressure.  Every one of many periodic boxes is moved in
 * time on the full-box mW energy by the BAOAB step of include/mw_md.h, and its cell is part of its state: an isotropic
 * stochastic-cell-rescaling barostat in eps = ln V scales cell, positions and velocities every baro_every steps, on a gfx950
 * device.  Every box follows its own trajectory and its own cell; no host decision enters either, and the host reads nothing
 * back while a call runs.
 *
 * A library of its own beside libmw_md.so (whose exported names, dependencies and bytes it leaves alone): it sits over the same
 * host, cell and force layers, takes plain arrays, has its own stream, scratch memory and event timers, and works with or
 * without mw_init or mw_md_init in the same process.  There is no CPU path.
 *
 * Units, input layout, supported range and error contract are those of include/mw_md.h: bohr, Hartree, atomic time units,
 * electron masses; `cells` 9 doubles per box in the layout of mw_set_cell, `pos`, `vel` (NULL: zero), `pos_ref` (NULL: `pos`)
 * [box][nwater][3], `streams` [box] (NULL: the box's index in the call), `seed`, `step0`; the cell rule a sigma (1 + 1e-9) <=
 * the smallest perpendicular width of every input cell; 1 <= nwater <= 2^22, 1 <= nboxes <= 2^24, 0 <= nsteps <= 10^8
 * (MW_NPT_MAX_STEPS), dt > 0, mass > 0, kT >= 0, gamma >= 0, sample_every >= 1, every position and velocity finite.  In
 * addition: `pressure` in Hartree / bohr^3, any finite value; `tau_p` > 0, the barostat's time constant in atomic time units;
 * `beta_T` > 0, the isothermal compressibility it assumes, in bohr^3 / Hartree; `baro_every` >= 0, the steps between two
 * applications, 0: no barostat.  Anything else (NaN or inf included) is rejected with a message that names the entry, the
 * argument and the first offending box, and nothing is launched or written.  (The device-pointer entry looks at its positions
 * and velocities with one kernel before the run and reads its verdict; that kernel writes nothing but the verdict.)
 *
 * State and step.  The state of a box is its cell h, x (never wrapped), v, the origin pos_ref of its displacements, and E, F and
 * the scalar virial W at x.  Stages 1 - 6 of a step are those of include/mw_md.h, unchanged and part of this contract: the same
 * constants hk, hd, c1, c2, hm, lim2 formed on the host in the same way, the same BAOAB order, the same Philox4x32-10 counter
 * (step index low, high, molecule, 0) and key (stream identity XOR seed) and Box-Muller rule, the same guard before each half
 * drift.  With baro_every = 0, pos_out, vel_out, forces, fields 0 - 3 of the trace and the status are byte for byte those of
 * mw_md_run on the same inputs, and cells_out is cells.
 *
 * The virial.  W = tr of the virial of include/mw_energy.h = -3 V dE/dV under isotropic scaling; the pressure is
 * P = (2 K + W) / (3 V), which is (N kT + W / 3) / V at equipartition.  It is formed from the entries the force walk visits: the
 * force e the entry at d puts on the centre molecule is added to the lane's sum dw as dw = dw + fma(d_x, e_x, fma(d_y, e_y,
 * d_z e_z)) in the order of the walk, the lane's share is -0.5 dw, and the shares are added like the energies.
 *
 * Barostat stage.  It follows stage 6 of the step with index t = step0 + s when baro_every > 0 and (t + 1) % baro_every == 0, so
 * chained calls apply it at the same steps.  There x, v, E, F and W belong to the same state.  Formed once on the host in
 * double: dtb = (double)baro_every * dt, cb = beta_T * dtb / tau_p, cn = sqrt(2.0 * kT * cb).  Per box, one lane:
 *   V   = the |det h| of the cell routine (below); K = hm * sum v.v, W: the box sums of the row of this step
 *   P   = (2.0 * K + W) / (3.0 * V)
 *   de  = -(cb * (pressure - P));  if kT > 0: de = fma(cn, xi / sqrt(V), de)
 *         xi = sqrt(-2 ln u_0) cos(2 pi u_1), u_k = (w_k + 0.5) 2^-32 from the Philox words of the counter (low word of t, high
 *         word of t, 0xFFFFFFFF, 1) under the box's key: one normal per box and application, from a counter no molecule has
 *         (molecule indices end below 2^22 and their fourth word is 0).  With kT = 0 no random number is drawn.
 *   mu  = exp(de / 3.0)
 *   h  <- mu * h (nine multiplications);  then for every molecule x <- mu * x, pos_ref <- mu * pos_ref, v <- v / mu
 *   E, F and W again at the scaled state, from a fresh sort into the grid of the scaled cell.  No stage 6 follows this
 *   evaluation; stage 1 of the next step, with its guard, does.  K of the row is hm * sum v.v of the scaled velocities, and the
 *   trace row of the step is this one.
 * In the eps form there is no further kT / V drift term: for particles without forces the stationary law is
 * p(V) ~ V^N exp(-pressure V / kT).
 *
 * Barostat guard.  The application is refused when de is not finite, when |de| > MW_NPT_MAX_DLNV, or when the scaled cell
 * breaks the cell rule (a sigma (1 + 1e-9) <= its smallest perpendicular width; a determinant that is zero or not finite
 * breaks it too).  The box is then frozen at the state before the application for the rest of the call: h, x, v, pos_ref, E, F
 * and the trace row those after stage 6 of that step, which counts as completed; its status is (steps completed, 2).  Status 1
 * remains the drift guard of include/mw_md.h.  Rows after a freeze repeat the last one.  No cell index or address is ever
 * formed from a cell that failed this test: par and grid of a box are replaced only by a cell that passed.  A run that
 * collapses or explodes is a result, not a fault.
 *
 * Cell on the device.  par (h and h^-1) and the grid of a box are computed on the device from the box's nine cell doubles by one
 * routine, at the start of a call and after every application: the cofactors fma(a, b, -(c d)), det = fma(, fma(, )), h^-1 =
 * cofactor / det and the widths |det| / sqrt(x x + y y + z z) of the cross products as the host layer forms them,
 * g_k = floor(w_k / (a sigma (1 + 1e-9))) capped at 1024 and lowered, largest first, to the 2 nwater (at least 64) cells the
 * scratch is sized for.  The host validates the input cells by the same rule before anything is launched and supplies neither
 * par nor grid, so a cell that came out of cells_out gives the par and grid bits of the run that produced it.
 *
 * Outputs (any may be NULL):
 *   pos_out, vel_out, forces [nboxes][nwater][3]: x, v and F (at pos_out) after the last step.
 *   cells_out [nboxes][9]: the cell after the last step.   ref_out [nboxes][nwater][3]: pos_ref as the library scaled it.
 *   trace[nboxes][nsteps / sample_every + 1][6] (MW_NPT_TRACE_FIELDS): E, K, the mean squared displacement from the scaled
 *     pos_ref, the largest |F| component, V and P, at step 0 and after every sample_every-th step.
 *   status[nboxes][2] ints: steps completed; 0, 1 (drift guard) or 2 (barostat guard).
 * A run of 2 K steps is byte for byte two runs of K steps chained through pos_out -> pos, vel_out -> vel, cells_out -> cells,
 * ref_out -> pos_ref (without a barostat application in the first run that is the first run's pos_ref) and step0 += K.
 *
 * Arithmetic (part of the contract).  As in include/mw_md.h: fma / mul / add spelled out with contraction off, a molecule's
 * sums in the order of the walk of its geometry, the box sums (E, sum v.v, sum |x - pos_ref|^2, W, the largest |F|) in a fixed
 * order, no floating-point atomics.  The bytes of a box's results depend on its cell, positions, velocities, pos_ref, stream
 * identity, seed, step0 and the call's scalars alone: not on the other boxes, on batching, on host versus device pointers, on
 * chunking or on how many steps one launch carries.
 *
 * Geometry, by nwater alone as in include/mw_md.h.  General (nwater > 64): the kernel sequence of libmw_md.so with W as a fifth
 * partial sum; at a barostat step one lane per box decides de and writes mu, the cell, par, the grid and the flags, one lane per
 * molecule scales x, v and pos_ref, and sort, moments, forces and row run again.  Small (nwater <= 64): one wavefront per box
 * over up to MW_NPT_SLICE steps per launch; a launch ends at a barostat step, the same two barostat kernels run, and the next
 * launch begins with the second evaluation (with the stage inside it the step kernel needs more than the 256 vector registers
 * that let two wavefronts share a SIMD; the bytes of the results do not depend on where the stage runs).  The host only enqueues: whether a step has a barostat stage depends on t alone.
 * Diagnostic switches read by mw_npt_init (they change no byte of any result): MW_NPT_SLICE (1..256, default 64) and
 * MW_NPT_SCRATCH_MB (default 256); a call is processed in chunks of as many boxes as fit the budget, and a box that does not
 * fit alone is an error.
 *
 * Out of scope: anisotropic or fully flexible cells, Nose-Hoover or MTK chains, variable-cell quenches, a Fortran binding, any
 * change to libmw_hip.so, to libmw_md.so and to bench.py.
 *
 * Every function returns 0, or nonzero with the reason in mw_npt_last_error().  A rejected call launches nothing and writes
 * nothing; box indices in messages count from 0.  Arguments are checked before the library's state, so a call with bad
 * arguments says so with or without a device.  The library lives on the device given to mw_npt_init: every function that
 * touches it makes that device current for the call and puts the caller's current device back before it returns.
 */
#ifndef MW_NPT_H
#define MW_NPT_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_NPT_PLAN_FIELDS 10
#define MW_NPT_TRACE_FIELDS 6
#define MW_NPT_MAX_STEPS 100000000
/* the largest |change of ln V| one application may make */
#define MW_NPT_MAX_DLNV 0.3

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0. */
int mw_npt_init(int device);
int mw_npt_finalize(void);
int mw_npt_is_initialised(void);
const char *mw_npt_last_error(void);

/* Host pointers. */
int mw_npt_run(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *pos_ref,
               const unsigned long long *streams, unsigned long long seed, unsigned long long step0, int nsteps, int sample_every,
               double dt, double mass, double kT, double gamma, double pressure, double tau_p, double beta_T, int baro_every,
               double *pos_out, double *vel_out, double *forces, double *cells_out, double *ref_out, double *trace, int *status);
/* Device pointers on the library's device for every array, the scalars by value.  Work queued on the device before the
 * call is waited for, and the results are complete on return. */
int mw_npt_run_device(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *pos_ref,
                      const unsigned long long *streams, unsigned long long seed, unsigned long long step0, int nsteps,
                      int sample_every, double dt, double mass, double kT, double gamma, double pressure, double tau_p,
                      double beta_T, int baro_every, double *pos_out, double *vel_out, double *forces, double *cells_out,
                      double *ref_out, double *trace, int *status);

/* The launch rules for nboxes boxes of nwater molecules with the cell `cell` (9 doubles, host) -- host arithmetic only, no
 * device and no mw_npt_init needed.  Writes min(nout, MW_NPT_PLAN_FIELDS) ints, the fields of mw_md_plan:
 *   [0] boxes per chunk   [1] chunks   [2] 1: small geometry, 0: general   [3] [4] [5] the cell grid of `cell`
 *   [6] LDS of a workgroup, bytes   [7] scratch per box, bytes   [8] boxes per workgroup (small) or 0
 *   [9] steps per launch: MW_NPT_SLICE (small) or 1 */
int mw_npt_plan(int nwater, const double *cell, int nboxes, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box's input cell. */
int mw_npt_last(int *out, int nout);
/* Event timers of the last call, summed over its steps and chunks: the sort, the moment pass, the force pass (with the trace
 * row), the drift and the barostat (decision and scaling; the evaluation after it counts as sort, moments and forces).  The
 * small geometry's step kernel is reported as the force pass. */
int mw_npt_elapsed_ms(float *sort, float *moments, float *forces, float *drift, float *barostat);

#ifdef __cplusplus
}
#endif
#endif
