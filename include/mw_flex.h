/* mw_flex.h -- C ABI of libmw_flex.so: molecular dynamics at constant pressure with a cell whose Cartesian axes move on their
 * own.  Every one of many periodic boxes is moved in time on the full-box mW energy by the BAOAB step of include/mw_md.h; its
 * cell is part of its state, and a per-axis stochastic-cell-rescaling barostat scales the Cartesian components of cell,
 * positions and velocities every baro_every steps, on a gfx950 device.  The force pass forms the full virial tensor and the
 * kinetic tensor, and every trace row carries the pressure tensor.  Every box follows its own trajectory and its own cell; no
 * host decision enters either, and the host reads nothing back while a call runs.
 *
 * A library of its own beside libmw_md.so and libmw_npt.so (whose exported names, dependencies and bytes it leaves alone): it
 * sits over the same host, cell and force layers, takes plain arrays, has its own stream, scratch memory and event timers, and
 * works with or without the other libraries in the same process.  There is no CPU path.
 *
 * Units, input layout, supported range and error contract are those of include/mw_npt.h: bohr, Hartree, atomic time units,
 * electron masses; `cells` 9 doubles per box in the layout of mw_set_cell (cells[3 k + a] is the Cartesian component a of
 * the cell vector k), `pos`, `vel` (NULL: zero), `pos_ref` (NULL: `pos`) [box][nwater][3], `streams` [box] (NULL: the box's
 * index in the call), `seed`, `step0`; the cell rule a sigma (1 + 1e-9) <= the smallest perpendicular width of every input
 * cell; 1 <= nwater <= 2^22, 1 <= nboxes <= 2^24, 0 <= nsteps <= 10^8 (MW_FLEX_MAX_STEPS), dt > 0, mass > 0, kT >= 0,
 * gamma >= 0, sample_every >= 1, `pressure` finite, `tau_p` > 0, `beta_T` > 0, `baro_every` >= 0 (0: no barostat), every
 * position and velocity finite.  In addition `coupling` is one of 0..3 (below) and `axis` one of 0..2 (x, y, z; it is checked
 * in every coupling and used by MW_FLEX_SEMI and MW_FLEX_UNIAXIAL).  Anything else is rejected with a message that names the
 * entry, the argument and the first offending box, and nothing is launched or written; coupling and axis are checked before
 * the library's state, without a device.
 *
 * State and step.  The state of a box is its cell h, x (never wrapped), v, the origin pos_ref of its displacements, and E, F,
 * the scalar virial W and the virial tensor W_ab at x.  Stages 1 - 6 of a step are those of include/mw_md.h, unchanged: the
 * same constants hk, hd, c1, c2, hm, lim2 formed on the host in the same way, the same BAOAB order, the same Philox4x32-10
 * counter (step index low, high, molecule, 0) and key (stream identity XOR seed) and Box-Muller rule, the same guard before
 * each half drift.  With baro_every = 0, pos_out, vel_out, forces, fields 0 - 3 of the trace and the status are byte for byte
 * those of mw_md_run on the same inputs, and cells_out is cells.
 *
 * The tensors.  The scalar virial W and the scalar pressure P = (2 K + W) / (3 V) are those of include/mw_npt.h, formed from
 * the same sums in the same order (dw = dw + fma(d_x, e_x, fma(d_y, e_y, d_z e_z)) per entry, the lane's share -0.5 dw).
 * Beside them the force walk keeps six sums per lane, in the order xx, yy, zz, xy, xz, yz: with e the force the entry at d
 * puts on the centre molecule, s_aa = fma(d_a, e_a, s_aa) and s_ab = s_ab + fma(d_a, e_b, d_b * e_a).  Every pair is visited
 * from both ends, so the lane's share of the virial tensor is -0.5 s_aa and -0.25 s_ab: W_aa = -dE/d eps_a for a stretch of
 * the Cartesian axis a, W_ab = -dE/d gamma_ab for the symmetric shear, and W_xx + W_yy + W_zz = W up to rounding.  The
 * kinetic tensor is K_ab = sum over the molecules of hm * (v_a * v_b), and P_ab = (2.0 * K_ab + W_ab) / V.  The scalar P is
 * formed from the scalar sums, not from the trace of P_ab.
 *
 * Barostat stage.  It follows stage 6 of the step with index t = step0 + s when baro_every > 0 and (t + 1) % baro_every == 0,
 * as in include/mw_npt.h, from the row of that step.  Formed once on the host in double: dtb = (double)baro_every * dt,
 * cb = beta_T * dtb / tau_p, cn = sqrt(2.0 * kT * cb), cb3 = cb / 3.0, cn_m = sqrt(2.0 * kT * cb3 / m) for m = 1, 2.  The
 * Cartesian axes are split into groups (c = `axis`; a, b the other two axes):
 *   0 MW_FLEX_ISO       {x, y, z}        the stage of include/mw_npt.h, word for word
 *   1 MW_FLEX_ANISO     {x}, {y}, {z}    the shape of a crystal, c/a
 *   2 MW_FLEX_SEMI      {a, b}, {c}      slabs, interfaces with a tension
 *   3 MW_FLEX_UNIAXIAL  {c}              NP_zT, direct coexistence; a and b are not touched
 * Coupling 0: P = (2.0 * K + W) / (3.0 * V), de = -(cb * (pressure - P)); if kT > 0: de = fma(cn, xi / sqrt(V), de) with the
 * normal of the counter (t low, t high, 0xFFFFFFFF, 1); refused when |de| > MW_FLEX_MAX_DLNV; mu = exp(de / 3.0) for all three
 * axes.  pos_out, vel_out, forces, cells_out, ref_out, fields 0 - 5 of the trace and the status are byte for byte those of
 * mw_npt_run.  Couplings 1 - 3, per group G of m axes, one lane per box:
 *   P_G  = P_aa (m = 1) or 0.5 * (P_aa + P_bb) with a < b (m = 2), from the row of this step
 *   de_G = -(cb3 * (pressure - P_G));  if kT > 0: de_G = fma(cn_m, xi_G / sqrt(V), de_G)
 *          xi_G = the first Box-Muller normal of the Philox counter (t low, t high, 0xFFFFFFFF, 2 + the lowest axis index of
 *          G) under the box's key.  The fourth word 1 remains the isotropic normal; no molecule has these counters.
 *   mu_G = exp(de_G)
 * Every axis a of G is then scaled by mu_G, one multiplication each and no other arithmetic: cells[3 k + a] for k = 0, 1, 2,
 * x_a and pos_ref_a of every molecule, and v_a <- v_a / mu_G.  An axis outside every group is not touched: its cell components,
 * coordinates and velocities keep their bits.  Then E, F, W and the tensors again at the scaled state, from a fresh sort into
 * the grid of the scaled cell; no stage 6 follows this evaluation, stage 1 of the next step does, and the trace row of the step
 * is this one.
 *
 * Why this form.  Let eps_G be the logarithm of the scale factor of group G, so that V ~ exp(sum_G m_G eps_G).  The stage is
 * one Euler step of the overdamped Langevin equation in the eps_G with the diffusion constant D_G = kT beta_T / (3 m_G tau_p V),
 * for which dD_G/d eps_G = -m_G D_G.  The target density in the eps is pi ~ V^(N + 1) exp(-(U + pressure V) / kT): V^N from the
 * scaled coordinates and one more V from the Jacobian of the eps.  Then d ln pi / d eps_G = m_G (N + 1) + (sum_{a in G} W_aa -
 * m_G pressure V) / kT, and with 2 K_aa = N kT the drift D_G d ln pi / d eps_G + dD_G / d eps_G equals
 * (beta_T / (3 tau_p)) (P_G - pressure): the -m_G D_G of the second term takes the 1 of N + 1 away, and no further kT / V term
 * is left.  The noise of one application has the variance 2 D_G dtb = cn_m^2 / V.  For particles without forces the volume
 * therefore follows p(V) ~ V^N exp(-pressure V / kT) with respect to dV in every coupling: <V> = (N + 1) kT / pressure and
 * var V = (N + 1) (kT / pressure)^2.  In coupling 3 the two fixed lengths are constants and the law of V is the same.  With one
 * group of three axes the sum of the three eps steps is the stage of include/mw_npt.h.  The shape modes of an ideal gas have no
 * restoring force and diffuse freely; that is the correct behaviour, not a defect.
 *
 * Barostat guard.  In couplings 1 - 3 the application is refused when any de_G is not finite, when any |de_G| >
 * MW_FLEX_MAX_DLNL, or when the scaled cell breaks the cell rule (a determinant that is zero or not finite breaks it too); in
 * coupling 0 by the rule of include/mw_npt.h.  The box is then frozen at the state before the application for the rest of
 * the call, with the status (steps completed, 2), exactly as include/mw_npt.h describes; status 1 remains the drift guard.
 * par and grid of a box are replaced only by a cell that passed.
 *
 * Cell on the device.  As in include/mw_npt.h: par (h and h^-1), the grid and V = |det h| of a box come from its nine cell
 * doubles by one device routine, at the start of a call and after every application.
 *
 * Outputs (any may be NULL):
 *   pos_out, vel_out, forces, ref_out [nboxes][nwater][3], cells_out [nboxes][9], status [nboxes][2]: as in include/mw_npt.h.
 *   trace[nboxes][nsteps / sample_every + 1][15] (MW_FLEX_TRACE_FIELDS): the six columns of include/mw_npt.h (E, K, the mean
 *     squared displacement, the largest |F| component, V, P), then P_xx, P_yy, P_zz, P_xy, P_xz, P_yz, then the lengths of the
 *     three cell vectors, sqrt(fma(h_x, h_x, fma(h_y, h_y, h_z h_z))) each.
 * A run of 2 K steps is byte for byte two runs of K steps chained through pos_out -> pos, vel_out -> vel, cells_out -> cells,
 * ref_out -> pos_ref and step0 += K.
 *
 * Arithmetic (part of the contract).  fma / mul / add spelled out with contraction off, a molecule's sums in the order of the
 * walk of its geometry, the sixteen box sums (E, sum v.v, sum |x - pos_ref|^2, W, six hm v_a v_b, six shares of the stress) and
 * the largest |F| component in a fixed order, no floating-point atomics.  The bytes of a box's results depend on its cell,
 * positions, velocities, pos_ref, stream identity, seed, step0 and the call's scalars alone: not on the other boxes, on
 * batching, on host versus device pointers, on chunking or on how many steps one launch carries.
 *
 * Geometry, by nwater alone.  General (nwater > 64): the kernel sequence of libmw_npt.so with seventeen partial values per
 * workgroup; at a barostat step one lane per box decides the three mu and writes the cell, par, the grid and the flags, one
 * lane per molecule scales x, v and pos_ref by axis, and sort, moments, forces and row run again.  Small (nwater <= 64): one
 * wavefront per box over up to MW_FLEX_SLICE steps per launch; a launch ends at a barostat step.  Diagnostic switches read by
 * mw_flex_init (they change no byte of any result): MW_FLEX_SLICE (1..256, default 64) and MW_FLEX_SCRATCH_MB (default 256).
 *
 * Out of scope: shear degrees of freedom of the cell (the shears of P are reported, not acted on), Nose-Hoover or MTK chains,
 * variable-cell quenches, a two-phase box builder, a Fortran binding.
 *
 * Every function returns 0, or nonzero with the reason in mw_flex_last_error().  A rejected call launches nothing and writes
 * nothing; box indices in messages count from 0.  Arguments are checked before the library's state.  The library lives on the
 * device given to mw_flex_init: every function that touches it makes that device current for the call and puts the caller's
 * current device back before it returns.
 */
#ifndef MW_FLEX_H
#define MW_FLEX_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_FLEX_PLAN_FIELDS 10
#define MW_FLEX_TRACE_FIELDS 15
#define MW_FLEX_MAX_STEPS 100000000
/* coupling 0: the largest |change of ln V| one application may make */
#define MW_FLEX_MAX_DLNV 0.3
/* couplings 1 - 3: the largest |change of the logarithm of a length| one application may make */
#define MW_FLEX_MAX_DLNL 0.1

#define MW_FLEX_ISO 0
#define MW_FLEX_ANISO 1
#define MW_FLEX_SEMI 2
#define MW_FLEX_UNIAXIAL 3

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0. */
int mw_flex_init(int device);
int mw_flex_finalize(void);
int mw_flex_is_initialised(void);
const char *mw_flex_last_error(void);

/* Host pointers. */
int mw_flex_run(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *pos_ref,
                const unsigned long long *streams, unsigned long long seed, unsigned long long step0, int nsteps, int sample_every,
                double dt, double mass, double kT, double gamma, double pressure, double tau_p, double beta_T, int baro_every,
                int coupling, int axis, double *pos_out, double *vel_out, double *forces, double *cells_out, double *ref_out,
                double *trace, int *status);
/* Device pointers on the library's device for every array, the scalars by value.  Work queued on the device before the
 * call is waited for, and the results are complete on return. */
int mw_flex_run_device(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *pos_ref,
                       const unsigned long long *streams, unsigned long long seed, unsigned long long step0, int nsteps,
                       int sample_every, double dt, double mass, double kT, double gamma, double pressure, double tau_p,
                       double beta_T, int baro_every, int coupling, int axis, double *pos_out, double *vel_out, double *forces,
                       double *cells_out, double *ref_out, double *trace, int *status);

/* The launch rules for nboxes boxes of nwater molecules with the cell `cell` (9 doubles, host) -- host arithmetic only, no
 * device and no mw_flex_init needed.  Writes min(nout, MW_FLEX_PLAN_FIELDS) ints, the fields of mw_md_plan:
 *   [0] boxes per chunk   [1] chunks   [2] 1: small geometry, 0: general   [3] [4] [5] the cell grid of `cell`
 *   [6] LDS of a workgroup, bytes   [7] scratch per box, bytes   [8] boxes per workgroup (small) or 0
 *   [9] steps per launch: MW_FLEX_SLICE (small) or 1 */
int mw_flex_plan(int nwater, const double *cell, int nboxes, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box's input cell. */
int mw_flex_last(int *out, int nout);
/* Event timers of the last call, summed over its steps and chunks: the sort, the moment pass, the force pass (with the trace
 * row), the drift and the barostat (decision and scaling; the evaluation after it counts as sort, moments and forces).  The
 * small geometry's step kernel is reported as the force pass. */
int mw_flex_elapsed_ms(float *sort, float *moments, float *forces, float *drift, float *barostat);

#ifdef __cplusplus
}
#endif
#endif
