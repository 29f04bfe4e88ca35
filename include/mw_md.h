/* mw_md.h -- C ABI of libmw_md.so: molecular dynamics.  Every one of many periodic boxes is moved in time on the full-box mW
 * energy at fixed cell, at constant energy (NVE) or in contact with a Langevin thermostat, on a gfx950 device.  Every box
 * follows its own trajectory; no host decision enters it, and the host reads nothing back while it runs.
 *
 * A library of its own beside libmw_hip.so (include/mw_energy.h), the analysis libraries and the quenches
 * (include/mw_quench.h, whose force pass it shares): it needs cells and positions only, so it takes plain arrays and works on
 * any configuration, with or without mw_init in the same process.  It has its own stream, scratch memory and event timers.
 * Its results are plain positions and velocities again: they go straight into the other libraries' entries and back into
 * this one.  There is no CPU path.
 *
 * Units.  Positions in bohr, energies in Hartree, forces in Hartree / bohr, times in atomic units (hbar / Hartree), masses
 * in electron masses, velocities in bohr per atomic time unit, kT in Hartree, gamma in inverse atomic time units.
 * MW_MD_MASS_WATER is the mass of a water molecule, 18.01528 amu x 1822.888486209 electron masses per amu.
 *
 * Inputs.  `cells` holds 9 doubles per box in the layout of mw_set_cell (cells[9 b + 3 k + a] = component a of h_(k+1)),
 * `pos` holds nwater positions as [box][nwater][3], wrapped or not.  `vel` [box][nwater][3] are the velocities (NULL: zero),
 * `pos_ref` [box][nwater][3] the origin of the mean squared displacement (NULL: `pos`), `streams` [box] the 64-bit stream
 * identities of the boxes' noise (NULL: the box's index in the call), `seed` the 64-bit seed and `step0` the index of the
 * call's first step.  The energy and the forces are those of include/mw_quench.h, from the same device routines.
 *
 * Supported range.  The cell rule of include/mw_quench.h: a sigma (1 + 1e-9) <= the smallest perpendicular width of every
 * box.  1 <= nwater <= 2^22; 1 <= nboxes <= 2^24; 0 <= nsteps <= 10^8 (MW_MD_MAX_STEPS); dt > 0, mass > 0, kT >= 0,
 * gamma >= 0, all finite; sample_every >= 1; every position and velocity finite.  Anything else (NaN or inf included) is
 * rejected with a message that names the entry, the argument and the first offending box, and nothing is launched or
 * written.  (The device-pointer entry looks at its positions and velocities with one kernel before the run and reads its
 * verdict; that kernel writes nothing but the verdict.)
 *
 * State and step.  The state of a box is x (never wrapped: pos_out is the input plus the accumulated drifts), v, and F at x.
 * The constants of a call are formed once on the host in double: hk = dt / (2 mass) (as dt / (2.0 * mass)), hd = dt / 2,
 * c1 = exp(-gamma dt), c2 = sqrt((kT / mass) (1 - c1 c1)), hm = mass / 2, lim2 = (a sigma / 4)^2.  One step is BAOAB:
 *   1. v = fma(hk, F, v)
 *   2. the guard (below) on v, then x = x + hd v.
 *   3. if gamma > 0: v = fma(c1, v, c2 xi).  With gamma = 0 this stage is skipped entirely and no random number is drawn:
 *      the run is NVE and time-reversible.
 *   4. the guard on v, then x = x + hd v.
 *   5. E and F at x.
 *   6. v = fma(hk, F, v)
 * A call evaluates E and F at its first positions before the first step (nsteps = 0 is a single-point evaluation), so a
 * run of 2 K steps is byte for byte two runs of K steps chained through pos_out -> pos, vel_out -> vel, pos_ref = the first
 * pos and step0 += K.
 *
 * Noise.  Philox4x32-10 (the generator of the engine's Monte Carlo moves).  Counter = (low word of the step index, high
 * word of the step index, molecule index, 0); key = (low, high) words of the box's stream identity XOR those of the seed;
 * the step index of the s-th step of a call (s = 0, 1, ...) is step0 + s.  The four output words w0..w3 become
 * u_k = (w_k + 0.5) 2^-32 in (0, 1) and two Box-Muller pairs: r = sqrt(-2 ln u_0), t = 2 pi u_1 (the double nearest 2 pi
 * times u_1): xi_x = r cos t, xi_y = r sin t; r' = sqrt(-2 ln u_2), t' = 2 pi u_3: xi_z = r' cos t' (the fourth normal is
 * not used).  A box's noise is a function of (seed, its stream identity, step index, molecule) and of nothing else.
 *
 * Guard.  Before each half drift every molecule's d2 = |hd v_i|^2 (fma(dx, dx, fma(dy, dy, dz dz)), dx = hd v_x ...) is
 * held against lim2: the guard passes if d2 <= lim2 for every molecule of the box, which is the same as the box's largest
 * hd |v_i| being at most a sigma / 4, written so that a NaN fails.  a sigma / 4 because the cell grid's cells are at
 * least a sigma wide: the two half drifts of a step together cannot carry a molecule further than half a cell, so no
 * molecule crosses a whole grid cell between two sorts, and a coordinate that passed is finite.  When the guard fails the
 * box is frozen at the state before that drift for the rest of the call: x and v as they are there (v includes the half
 * kick of stage 1 and, at the second guard, the thermostat), E, F and the trace row those of the last completed step.
 * Its status is (steps completed, 1).  No kernel forms a cell index or an address from a coordinate that failed this test,
 * and the cell of a coordinate is clamped into the table whatever its value: a run that blows up is a result, not a fault.
 *
 * Outputs (any may be NULL):
 *   pos_out, vel_out, forces [nboxes][nwater][3] doubles: x, v and F (at pos_out) after the last step.
 *   trace[nboxes][nsteps / sample_every + 1][4] doubles (MW_MD_TRACE_FIELDS): the potential energy E, the kinetic energy
 *     hm sum v.v, the mean squared displacement sum |x - pos_ref|^2 / nwater and the largest |F| component, at step 0
 *     (before the first step) and after every sample_every-th step of the call.  Rows after a freeze repeat the row of the
 *     last completed step.
 *   status[nboxes][2] ints: steps completed, frozen 0 / 1.
 *
 * Arithmetic (part of the contract).  As in include/mw_quench.h: H^-1 is formed once per box on the host, everything is
 * spelled out in fma / mul / add with contraction off, a molecule's moments, energy and force are one lane's sums in the
 * order of the walk of its geometry, and the box sums (E, sum v.v, sum |x - pos_ref|^2, the largest |F|) run in a fixed
 * order: the lanes of a wavefront through one DPP tree, the wavefronts of a workgroup in order, the workgroups of a box in
 * order.  There are no floating-point atomics.  Hence the bytes of a box's results depend on its cell, positions,
 * velocities, pos_ref, stream identity, seed, step0, nsteps, sample_every, dt, mass, kT and gamma alone: not on the other
 * boxes of the call, on batch versus single calls, on host versus device pointers, on chunking or on how many steps one
 * launch carries.
 *
 * Geometry.  Which of two geometries a box takes depends on nwater alone.
 *   general (nwater > 64): per step the drift kernels (stages 2 - 4), the counting sort into the cell grid of a sigma, the
 *     moment pass, the force pass (which also applies stage 6 and stage 1 of the next step and tests the first guard, so
 *     the velocities are passed over once) and one workgroup per box that adds the partial sums in order and writes the
 *     trace row.  The host only enqueues.
 *   small (nwater <= 64): one wavefront per box, four boxes per workgroup, lane = molecule, fractional positions and moments
 *     in LDS, x, v and F in registers over up to MW_MD_SLICE steps per launch, the trace rows written from lane 0.
 * Diagnostic switches read by mw_md_init (they must not and do not change a byte of any result): MW_MD_SLICE, the steps one
 * launch of the small geometry carries (1..256, default 64), and MW_MD_SCRATCH_MB, the scratch budget in MiB (default 256).
 * A call is processed in chunks of as many boxes as fit the budget, each chunk run to its end; a box that does not fit alone
 * is an error.
 *
 * Out of scope: dynamics of the cell and barostats, constraint or rigid-body integrators, a Fortran binding, any change to
 * libmw_hip.so and any change to bench.py.
 *
 * Every function returns 0, or nonzero with the reason in mw_md_last_error().  A rejected call launches nothing and writes
 * nothing; its message names the entry and the argument, and box indices in messages count from 0.  Arguments are checked
 * before the library's state, so a call with bad arguments says so with or without a device.  The library lives on the
 * device given to mw_md_init: every function that touches it makes that device current for the call and puts the caller's
 * current device back before it returns.
 */
#ifndef MW_MD_H
#define MW_MD_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_MD_PLAN_FIELDS 10
#define MW_MD_TRACE_FIELDS 4
#define MW_MD_MAX_STEPS 100000000
/* 18.01528 amu x 1822.888486209 electron masses per amu */
#define MW_MD_MASS_WATER (18.01528 * 1822.888486209)

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0. */
int mw_md_init(int device);
int mw_md_finalize(void);
int mw_md_is_initialised(void);
const char *mw_md_last_error(void);

/* Host pointers. */
int mw_md_run(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *pos_ref,
              const unsigned long long *streams, unsigned long long seed, unsigned long long step0, int nsteps, int sample_every,
              double dt, double mass, double kT, double gamma, double *pos_out, double *vel_out, double *forces, double *trace,
              int *status);
/* Device pointers on the library's device for every array, the scalars by value.  Work queued on the device before the
 * call is waited for, and the results are complete on return. */
int mw_md_run_device(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *pos_ref,
                     const unsigned long long *streams, unsigned long long seed, unsigned long long step0, int nsteps,
                     int sample_every, double dt, double mass, double kT, double gamma, double *pos_out, double *vel_out,
                     double *forces, double *trace, int *status);

/* The launch rules for nboxes boxes of nwater molecules with the cell `cell` (9 doubles, host) -- host arithmetic only, no
 * device and no mw_md_init needed (the scratch budget and the slice are then the default ones).  Writes
 * min(nout, MW_MD_PLAN_FIELDS) ints:
 *   [0] boxes per chunk   [1] chunks = ceil(nboxes / [0])   [2] 1: small geometry, 0: general
 *   [3] [4] [5] the cell grid g_1, g_2, g_3 of a sigma (the small geometry reports it and does not use it)
 *   [6] LDS of a workgroup, bytes (the largest of the kernels)   [7] scratch per box, bytes
 *   [8] boxes per workgroup (small) or 0   [9] steps per launch: MW_MD_SLICE (small) or 1 */
int mw_md_plan(int nwater, const double *cell, int nboxes, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box. */
int mw_md_last(int *out, int nout);
/* Event timers of the last call, summed over its steps and chunks: the sort, the moment pass, the force pass (with the
 * trace row) and the drift (stages 2 - 4).  The small geometry is one kernel: its time is reported as the force pass and the
 * others are 0. */
int mw_md_elapsed_ms(float *sort, float *moments, float *forces, float *drift);

#ifdef __cplusplus
}
#endif
#endif
