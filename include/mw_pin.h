/* mw_pin.h -- C ABI of libmw_pin.so: interface pinning (Pedersen, Hummel, Kresse, Kahl, Dellago, Phys. Rev. B 88, 094101 (2013);
 * Pedersen, J. Chem. Phys. 139, 104102 (2013)).  Every one of many periodic boxes is moved in time by the step of
 * include/mw_flex.h -- BAOAB on the full-box mW energy, NVE or Langevin, with the per-axis stochastic-cell-rescaling barostat in
 * all four couplings -- on the energy E_mW + U_b, where U_b is a harmonic bias on the modulus of one collective density mode of
 * the box.  A two-phase box held at a chosen amount of crystal by such a bias reports, as the mean force the bias exerts, the
 * difference of the chemical potentials of solid and liquid at that temperature and pressure; T_m(p) follows from a few runs.
 * The force of the bias depends on a sum over the whole box; it enters every step on the device, with no host decision.
 *
 * A library of its own beside libmw_flex.so (whose exported names, dependencies and bytes it leaves alone) over the same host,
 * cell and force layers: plain arrays, its own stream, scratch memory and event timers.  There is no CPU path.
 *
 * Units, input layout, supported range and error contract are those of include/mw_flex.h for every argument the two share:
 * `cells`, `pos`, `vel`, `pos_ref`, `streams`, `seed`, `step0`, nsteps, sample_every, dt, mass, kT, gamma, pressure, tau_p,
 * beta_T, baro_every (0: fixed cell), coupling 0..3 and axis 0..2.  In addition:
 *   nvec    [box][3] int     the integer triple n of the box's mode: |n_a| <= 255 (MW_PIN_MAX_N), n != (0, 0, 0).
 *   kappas  [box]            the stiffness kappa, Hartree: >= 0 and finite.  kappa = 0: no bias (below).
 *   anchors [box]            the anchor a of Q (a pure number): >= 0 and finite.
 *   equil_steps >= 0, block_steps >= 0 (0: no blocks), exactly as in include/mw_ti.h.
 * Anything else (NaN included) is rejected with a message that names the entry, the argument and the first offending box, and
 * nothing is launched or written.  The host-pointer entry checks everything before the library's state, without a device; the
 * device-pointer entry reads nvec, kappas and anchors back (28 bytes per box) before anything is launched.
 *
 * The bias.  H is the cell (columns: the cell vectors), s_j = H^-1 r_j reduced to [0, 1) as the cell sort reduces it, and
 * theta_j = 2 pi n.s_j.  n is an integer triple, so the reduction changes nothing of exp(i theta_j).
 *     C = sum_j cos theta_j,  S = sum_j sin theta_j,  R = sqrt(C^2 + S^2),  Q = R / sqrt(N)
 *     U_b = 1/2 kappa (Q - a)^2
 *     F_b,j = g (S cos theta_j - C sin theta_j) k,   g = -kappa (Q - a) / (R sqrt(N)),   k = 2 pi H^-T n
 * Q is sqrt(S(k)) of include/mw_sk.h: about 1 for a liquid, of the order sqrt(N) for a crystal at one of its Bragg vectors.
 * dQ/dr_j = (C dC/dr_j + S dS/dr_j) / (R sqrt(N)) with dC/dr_j = -sin theta_j k and dS/dr_j = cos theta_j k gives F_b,j =
 * -kappa (Q - a) dQ/dr_j.  The sum of F_b over the molecules is g (S C - C S) k = 0.  With R = 0 the force of the bias is zero.
 *
 * Arithmetic of the bias (part of the contract; contraction off; I = H^-1 row-major, the last nine doubles of the box's par):
 *     ph = fma(n_1, s_1, fma(n_2, s_2, n_3 * s_3));  sincospi(2.0 * ph, &sin_j, &cos_j)     one per molecule and evaluation
 *     R = sqrt(fma(C, C, S * S));  rn = sqrt((double)N);  Q = R / rn;  d = Q - a;  U_b = (0.5 * kappa) * (d * d)
 *     g = R > 0 ? -(kappa * d) / (R * rn) : 0;   gk_a = g * (2 pi * fma(n_1, I[a], fma(n_2, I[3 + a], n_3 * I[6 + a])))
 *     w_j = fma(S, cos_j, -(C * sin_j));   F_tot,a = fma(w_j, gk_a, F_mW,a)                 one fma per component
 * No recurrence forms a phase from another.  k is formed from the box's par on the device at every evaluation, so it follows the
 * cell after every barostat application.  C and S are box sums in a fixed order: small geometry, lane i = molecule i, the DPP
 * tree of the wavefront; general geometry, the molecules in the order of the cell sort, the lanes of a wavefront by the DPP
 * tree, the wavefronts of a workgroup in order, the workgroups in order.  There are no floating-point atomics.
 *
 * The step.  State and stages are those of include/mw_flex.h, restated; the force that enters stages 1 and 6, that `forces`
 * returns and whose largest component is column 3 of the trace is F_tot = F_mW + F_b.  A box with kappa = 0 takes none of the
 * bias's branches, all uniform over a wavefront: its pos_out, vel_out, forces, cells_out, ref_out, trace columns 0 - 14 and
 * status are byte for byte those of mw_flex_run on the same inputs, and its columns 15 and 16 and the first two entries of its
 * blocks are 0.
 *
 * The virial.  U_b depends on the positions through the fractional coordinates s_j alone.  The barostat's scaling -- and any
 * affine change of the cell H -> A H with r_j -> A r_j -- leaves every s_j = H^-1 r_j unchanged, so dU_b/d eps = 0 for every
 * strain eps at fixed s: the bias adds nothing to W, to W_ab or to any pressure, and the barostat stage is that of
 * include/mw_flex.h, word for word.  (In Cartesian terms: sum_j r_j,a F_b,j,b is cancelled exactly by the change of k with the
 * cell.)  A bias on a wavevector k fixed in space would have a virial of its own unless k lay in the plane the barostat does not
 * move, which is Pedersen's restriction; with k = 2 pi H^-T n following the cell it is not needed, for any n and any coupling.
 * P and P_ab in the trace remain the mW pressure and pressure tensor; E (column 0) remains E_mW.
 *
 * Outputs (any may be NULL): pos_out, vel_out, forces, cells_out, ref_out, status as in include/mw_flex.h (status 1: frozen by the
 * drift guard, as a huge kappa may cause; 2: by the barostat guard; results, not errors), and
 *   trace[nboxes][nsteps / sample_every + 1][17] (MW_PIN_TRACE_FIELDS): the fifteen columns of include/mw_flex.h (0 E_mW,
 *     3 the largest |F_tot| component), then 15 Q and 16 U_b.
 *   blocks[nboxes][nblocks][4] (MW_PIN_BLOCK_FIELDS), nblocks = (nsteps - equil_steps) / block_steps (integer division; 0 if
 *     block_steps = 0 or nsteps < equil_steps): entry j holds the sums of Q, Q * Q, V and E_mW of the rows after each of the
 *     steps equil_steps + j block_steps ... + block_steps - 1 of the call (steps count from 0; the row of a step with a barostat
 *     application is the one after it), added one after the other in step order from 0.0 and then divided by
 *     (double)block_steps.  The accumulation happens on the device at every step, independent of sample_every, of the steps per
 *     launch and of chunking; the accumulator is carried in memory between launches.  A frozen box contributes its last row, as
 *     the trace does.
 *
 * Contract.  A run of 2 K steps is byte for byte two chained runs of K in state and trace (pos_out -> pos, vel_out -> vel,
 * cells_out -> cells, ref_out -> pos_ref, step0 += K; blocks belong to a call).  The bytes of a box's results depend on its own
 * arrays, triple, kappa, a, stream identity, seed, step0 and the call's scalars alone: not on the other boxes, on batching, on
 * host versus device pointers, on chunking or on how many steps a launch carries.
 *
 * Geometry, by nwater alone.  Small (nwater <= 64): one wavefront per box as in include/mw_flex.h; C and S are the DPP tree over
 * the lanes, formed before the two walks of an evaluation; w_j and g k wait in LDS and enter after the force walk, before the
 * kick.  General: each lane of the moment pass forms (cos theta, sin theta) from the sorted s it already holds, stores the pair in sorted order (16 bytes per molecule, global memory: the pair is read by
 * another kernel) and contributes to two partial sums per workgroup; a kernel of one wavefront per box adds the partials in
 * workgroup order and writes C, S, g k, Q and U_b; the force kernel reads its molecule's pair and five doubles of its box.
 * Diagnostic switches read by mw_pin_init (they change no byte of any result): MW_PIN_SLICE (1..256, default 64) and
 * MW_PIN_SCRATCH_MB (default 256).
 *
 * Out of scope: a two-phase box builder (a crystal started with the anchor at half its own Q melts half of itself under the
 * bias, which is how such a box is usually made), biases on other collective variables, several modes per box, the root search
 * for T_m, a Fortran binding.
 *
 * Every function returns 0, or nonzero with the reason in mw_pin_last_error().  A rejected call launches nothing and writes
 * nothing; box indices in messages count from 0.  The library lives on the device given to mw_pin_init: every function that
 * touches it makes that device current for the call and puts the caller's current device back before it returns.
 */
#ifndef MW_PIN_H
#define MW_PIN_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_PIN_PLAN_FIELDS 10
#define MW_PIN_TRACE_FIELDS 17
#define MW_PIN_BLOCK_FIELDS 4
#define MW_PIN_MAX_STEPS 100000000
#define MW_PIN_MAX_N 255
/* the barostat's guards, those of include/mw_flex.h */
#define MW_PIN_MAX_DLNV 0.3
#define MW_PIN_MAX_DLNL 0.1

#define MW_PIN_ISO 0
#define MW_PIN_ANISO 1
#define MW_PIN_SEMI 2
#define MW_PIN_UNIAXIAL 3

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0. */
int mw_pin_init(int device);
int mw_pin_finalize(void);
int mw_pin_is_initialised(void);
const char *mw_pin_last_error(void);

/* Host pointers. */
int mw_pin_run(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *pos_ref,
               const int *nvec, const double *kappas, const double *anchors, const unsigned long long *streams,
               unsigned long long seed, unsigned long long step0, int nsteps, int sample_every, int equil_steps, int block_steps,
               double dt, double mass, double kT, double gamma, double pressure, double tau_p, double beta_T, int baro_every,
               int coupling, int axis, double *pos_out, double *vel_out, double *forces, double *cells_out, double *ref_out,
               double *trace, double *blocks, int *status);
/* Device pointers on the library's device for every array, the scalars by value.  Work queued on the device before the
 * call is waited for, and the results are complete on return. */
int mw_pin_run_device(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *pos_ref,
                      const int *nvec, const double *kappas, const double *anchors, const unsigned long long *streams,
                      unsigned long long seed, unsigned long long step0, int nsteps, int sample_every, int equil_steps,
                      int block_steps, double dt, double mass, double kT, double gamma, double pressure, double tau_p,
                      double beta_T, int baro_every, int coupling, int axis, double *pos_out, double *vel_out, double *forces,
                      double *cells_out, double *ref_out, double *trace, double *blocks, int *status);

/* The fields of mw_flex_plan (include/mw_flex.h) for this library: host arithmetic only, no device and no mw_pin_init needed. */
int mw_pin_plan(int nwater, const double *cell, int nboxes, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box's input cell. */
int mw_pin_last(int *out, int nout);
/* Event timers of the last call, summed over its steps and chunks: the five of mw_flex_elapsed_ms, and `rho`, the kernel that adds
 * the partial sums of the mode and forms C, S, g k, Q and U_b of every box (general geometry; the phasors themselves are formed
 * inside the moment pass and count there).  The small geometry's step kernel is reported as the force pass. */
int mw_pin_elapsed_ms(float *sort, float *moments, float *forces, float *drift, float *barostat, float *rho);

#ifdef __cplusplus
}
#endif
#endif
