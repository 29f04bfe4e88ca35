/* mw_ti.h -- C ABI of libmw_ti.so: Einstein-crystal thermodynamic integration (Frenkel-Ladd).  Every one of many periodic
 * boxes is moved in time on the mixed energy
 *
 *     U_lambda(x) = (1 - lambda) E_mW(x) + lambda 1/2 k sum_i |x_i - s_i|^2
 *
 * with a lambda, a spring constant k and Einstein sites s of its own, by the BAOAB step of include/mw_md.h (NVE or
 * Langevin), on a gfx950 device, and the block averages of the integrand's ingredients are taken on the device at every step.
 * A lambda-integration is 10 - 20 independent boxes per lattice and walker: one call integrates a whole farm.
 *
 * A library of its own beside libmw_md.so (whose step it restates) over the same host, cell and force layers: it takes plain
 * arrays and works with or without mw_init / mw_md_init in the same process.  It has its own stream, scratch memory and event
 * timers.  There is no CPU path.
 *
 * Units: those of include/mw_md.h; the springs are in Hartree / bohr^2.
 *
 * Inputs.  All of mw_md_run's, with `sites` in the place of pos_ref, and:
 *   sites   [box][nwater][3]  the Einstein sites: required, finite, never wrapped; the origin of the displacements
 *                             u_i = x_i - s_i.
 *   lambdas [box]             each in [0, 1].
 *   springs [box]             each > 0 and finite.
 *   equil_steps >= 0, block_steps >= 0 (0: no blocks).
 *   pos may be NULL: the boxes start on their sites.
 * Anything else (NaN included) is rejected with a message that names the entry, the argument and the first offending box, and
 * nothing is launched or written.  The device-pointer entry reads lambdas and springs back (8 bytes per box each) and looks at
 * pos, vel and sites with one kernel that writes nothing but its verdict.
 *
 * Step.  Stages 1 - 6, the constants, the Philox counter and key, the Box-Muller rule and the drift guard are those of
 * include/mw_md.h, unchanged.  Only the force that enters stages 1 and 6 differs.  Per box the host forms oml = 1.0 - lambda
 * and nlk = -(lambda * k) once; per component
 *     F_tot = fma(nlk, u, oml * F_mW).
 * For a box with lambda = 0 the spring term is skipped (F_tot = F_mW: the bits of libmw_md.so); for a box with lambda = 1 the
 * mW term is skipped (F_tot = nlk * u: a non-finite F_mW of two coinciding molecules that no longer interact stays out of the
 * state).  Both are wavefront-uniform branches per box.  E_mW and F_mW are evaluated in every case.  A state that goes
 * non-finite fails the drift guard as in libmw_md.so: a result, not a fault.
 *
 * Outputs (any may be NULL):
 *   pos_out, vel_out, forces [nboxes][nwater][3]: x, v and F_tot (at pos_out) after the last step.
 *   trace[nboxes][nsteps / sample_every + 1][5] (MW_TI_TRACE_FIELDS):
 *     0  E_mW (unscaled)              1  K = hm sum v.v             2  sum |u|^2 / nwater
 *     3  the largest |F_tot| component                              4  |sum u / nwater|^2
 *     Fields 0 - 3 are formed exactly as mw_md's fields 0 - 3 with pos_ref = sites.  Field 4: the three box sums of u_x, u_y,
 *     u_z in the same fixed order (DPP tree, wavefronts in order, workgroups in order), c_a = sum_a / (double)nwater,
 *     fma(c_x, c_x, fma(c_y, c_y, c_z c_z)).  The host derives U_E = 1/2 k N f2 and, free of the centre of mass,
 *     U_E' = 1/2 k N (f2 - f4): U_mW is translation invariant and the springs are equal, so the centre of mass factorises
 *     exactly and is the same for two lattices of equal N; no constraint enters the dynamics.
 *   blocks[nboxes][nblocks][5], nblocks = (nsteps - equil_steps) / block_steps (integer division; 0 if block_steps = 0 or
 *     nsteps < equil_steps): entry j is the sum of the five fields after each of the steps equil_steps + j block_steps ...
 *     + block_steps - 1 of the call (steps count from 0), added one after the other in step order from 0.0 and then divided by
 *     (double)block_steps.  The accumulation happens on the device at every step, independent of sample_every, of the steps
 *     per launch and of chunking; the accumulator is carried in memory between launches.  A frozen box contributes its last
 *     row, as the trace does.
 *   status[nboxes][2]: steps completed, frozen 0 / 1.
 *
 * Contract.  A run of 2 K steps is byte for byte two chained runs of K in state and trace (blocks belong to a call).  With
 * every lambda = 0, pos_out, vel_out, forces, trace fields 0 - 3 and status are byte for byte mw_md_run's with pos_ref = sites.
 * The bytes of a box's results depend on that box's arrays, lambda, k, stream identity, seed, step0 and the call's scalars
 * alone: not on the other boxes, batch versus single calls, host versus device pointers, chunking or steps per launch.  The
 * arithmetic is spelled out in fma / mul / add with contraction off; there are no floating-point atomics.
 *
 * Geometry, by nwater alone as in include/mw_md.h:
 *   general (nwater > 64): mw_md's kernel sequence; the force pass also gathers the site of its molecule and forms F_tot
 *     before stages 6 and 1; the row kernel adds the block accumulators.
 *   small (nwater <= 64): one wavefront per box, four boxes per workgroup, up to MW_TI_SLICE steps per launch (1..256,
 *     default 64), lambda and k per wavefront; lane 0 writes the accumulators.
 * MW_TI_SCRATCH_MB: the scratch budget in MiB (default 256), as MW_MD_SCRATCH_MB.  Neither switch changes a byte of a result.
 *
 * Out of scope: fixed-centre-of-mass constraints, non-linear lambda paths, nonequilibrium switching, NPT, a Fortran binding.
 *
 * Every function returns 0, or nonzero with the reason in mw_ti_last_error().  Arguments are checked before the library's
 * state, so a call with bad arguments says so with or without a device.
 */
#ifndef MW_TI_H
#define MW_TI_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_TI_PLAN_FIELDS 10
#define MW_TI_TRACE_FIELDS 5
#define MW_TI_MAX_STEPS 100000000

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0. */
int mw_ti_init(int device);
int mw_ti_finalize(void);
int mw_ti_is_initialised(void);
const char *mw_ti_last_error(void);

/* Host pointers. */
int mw_ti_run(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *sites,
              const double *lambdas, const double *springs, const unsigned long long *streams, unsigned long long seed,
              unsigned long long step0, int nsteps, int sample_every, int equil_steps, int block_steps, double dt, double mass,
              double kT, double gamma, double *pos_out, double *vel_out, double *forces, double *trace, double *blocks,
              int *status);
/* Device pointers on the library's device for every array, the scalars by value.  Work queued on the device before the
 * call is waited for, and the results are complete on return. */
int mw_ti_run_device(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *sites,
                     const double *lambdas, const double *springs, const unsigned long long *streams, unsigned long long seed,
                     unsigned long long step0, int nsteps, int sample_every, int equil_steps, int block_steps, double dt,
                     double mass, double kT, double gamma, double *pos_out, double *vel_out, double *forces, double *trace,
                     double *blocks, int *status);

/* The fields of mw_md_plan (include/mw_md.h) for this library: host arithmetic only, no device and no mw_ti_init needed. */
int mw_ti_plan(int nwater, const double *cell, int nboxes, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box. */
int mw_ti_last(int *out, int nout);
/* Event timers of the last call as in mw_md_elapsed_ms: sort, moment pass, force pass (with the row), drift. */
int mw_ti_elapsed_ms(float *sort, float *moments, float *forces, float *drift);

#ifdef __cplusplus
}
#endif
#endif
