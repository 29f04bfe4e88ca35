/* mw_nuc.h -- C ABI of libmw_nuc.so: molecular dynamics that watches the size of the largest solid-like cluster of every box and
 * ends a box's trajectory, on the device, when that size reaches a bound.  It is the primitive of seeding, committor runs and
 * forward-flux sampling: every one of many periodic boxes is moved in time by the step of include/mw_flex.h, untouched; every
 * check_every steps the size lambda of its largest cluster of solid-like molecules is evaluated on the device; one lane per box
 * then decides whether the box goes on.  No host decision enters the rule, and the host reads nothing back while a call runs.
 *
 * A library of its own beside libmw_flex.so and libmw_boo.so (whose exported names, dependencies and bytes it leaves alone): it
 * sits over the same host, cell and force layers, shares the l = 6 harmonics with libmw_boo.so through one header, takes plain
 * arrays, has its own stream, scratch memory and event timers, and works with or without the other libraries in the same
 * process.  There is no CPU path.
 *
 * Arguments.  Every argument that mw_flex_run has keeps its meaning, its range, its checks and its messages (units, layouts,
 * the cell rule, the stream identities, seed and step0: include/mw_flex.h).  In addition:
 *   rc           the bond cutoff in bohr: 0 < rc, finite, and rc (1 + 1e-9) <= a sigma, the mW cutoff.  With that rule every
 *                entry within rc lies in the 27 cells the force evaluation walks: its cell grid and its sort serve the order
 *                parameter, and no second sort is made.
 *   threshold    finite, in [-1, 1].
 *   min_conn     1 <= min_conn <= 64 (MW_NUC_MAX_CONN).
 *   check_every  >= 1, and nsteps % check_every == 0 (nsteps = 0 is a single point).
 *   lam_lo, lam_hi  [box] ints with -1 <= lam_lo[b] < lam_hi[b].  lam_lo = -1 disables the lower test (no size is <= -1),
 *                lam_hi > nwater the upper one (no size is >= it).
 * nwater must be at least MW_NUC_MIN_WATER = 65: a nucleus in 64 molecules is not a use case, and the one-wavefront-per-box
 * geometry of the other libraries is out of scope here; the call is rejected with a message that says so.  Everything is checked
 * before the library's state, without a device (the device-pointer entry reads lam_lo and lam_hi back first, and its cells,
 * positions and velocities as mw_flex_run_device does).  A rejected call launches nothing and writes nothing; a message names the
 * entry, the argument and the first offending box.
 *
 * Order parameter.  The definitions are those of include/mw_boo.h restricted to l = 6.  The entries of molecule i are the
 * (j, image) with 0 < |d| < rc; n_i is their number.  q_6m(i) = (1 / n_i) sum over the entries of Y_6m(d / |d|) (0 when n_i = 0),
 * |q_6(i)| its norm.  Per entry s_ij = q_6(i) . q_6(j) / (|q_6(i)| |q_6(j)|); conn_i = #{entries: s_ij > threshold}, and an entry
 * with |q_6(i)| |q_6(j)| = 0 makes no connection.  Molecule i is SOLID-LIKE iff conn_i >= min_conn.  Solid-like i and j are
 * BONDED iff j is an entry of i or i is an entry of j; an image of i itself is no bond, several images of one j are one bond.
 * Clusters are the connected components through the periodic boundary, and lambda is the size of the largest one (0 when no
 * molecule is solid-like).
 *
 * Arithmetic of the order parameter (part of the contract).  A molecule's thirteen sums are added in the order of the walk of
 * mw_lib_cells.h on the grid of the force evaluation of that state (the grid of a sigma, not of rc), from Y formed by the shared
 * routine of mw_lib_harmonics.h; the division by n_i, the norm (fma in component order), the dot product (fma in component
 * order), den = |q_6(i)| * |q_6(j)|, and the test den > 0 && dot / den > threshold are formed exactly as k_boo_pass2 of
 * libmw_boo.so forms them.  Contraction is off.  Everything downstream of q_6m is an integer.  Cluster labels are canonical: 0
 * for a molecule that is not solid-like, otherwise the 1-based index of the smallest molecule of its cluster; a tie for the
 * largest cluster goes to the smallest label.
 *
 * When the evaluation runs.  At entry, on the input state, and after every step e of the call (e = 0 .. nsteps - 1) with
 * (e + 1) % check_every == 0, on the final state of that step: after the barostat application if there is one, from the fresh
 * sort of that state's force evaluation.  The phase is that of the call, not of step0.  A box frozen by a guard is not evaluated
 * again; for such a box nn, label and op (below) are evaluated once more on its final state at the end of the call, and its trace
 * columns keep the latest evaluation it had while it ran.
 *
 * Stopping rule.  One lane per box, after each evaluation of a box that is not frozen:
 *   lambda >= lam_hi            the box is frozen with the status (steps completed, 3);
 *   otherwise lambda <= lam_lo  the box is frozen with the status (steps completed, 4).
 * A frozen box keeps its state for the rest of the call, exactly as the guards freeze a box; statuses 1 and 2 remain the guards
 * of include/mw_flex.h.  The state of a stopped box is the state at the end of that step: stage 1 of the next step is applied
 * only after the rule has let the box go on, by a kernel of its own, with the same arithmetic and the same guard.
 *
 * Outputs (any may be NULL).  pos_out, vel_out, forces, cells_out, ref_out, status: as in include/mw_flex.h (status codes 0 - 4).
 *   trace[nboxes][nsteps / sample_every + 1][18] (MW_NUC_TRACE_FIELDS): the fifteen columns of include/mw_flex.h, then
 *     15 lambda, 16 the number of solid-like molecules, 17 the number of clusters, as doubles: the latest evaluation at or before
 *     the row.  Row 0 holds the entry evaluation.  The rows after a freeze repeat the box's last row.
 *   nn[nboxes][nwater][2] = (n_i, conn_i), int, of the box's final state.
 *   label[nboxes][nwater], int, of the box's final state.
 *   op[nboxes][4] = (solid-like molecules, clusters, lambda, the label of the largest cluster), int, of the box's final state.
 * Because nsteps is a multiple of check_every, the final state of every box that no guard froze has been evaluated.
 *
 * Contracts.
 *   Bounds disabled equals flex: with both tests disabled in a box, pos_out, vel_out, forces, cells_out, ref_out, trace columns
 *     0 - 14 and status are byte for byte those of mw_flex_run on the same inputs.
 *   A stopped box equals flex of that length: a box stopped with the status (h, 3 or 4) has pos_out, vel_out, forces, cells_out
 *     and ref_out byte for byte from mw_flex_run with nsteps = h.
 *   Chaining: a run of 2 K steps (K a multiple of check_every) is byte for byte two chained runs of K (pos_out -> pos, vel_out ->
 *     vel, cells_out -> cells, ref_out -> pos_ref, step0 += K), for boxes whose first run ends with the status (K, 0).
 *   Independence: the bytes of a box's results depend on its own arrays, bounds, stream identity, seed, step0 and the call's
 *     scalars alone: not on the other boxes, on batching, on host versus device pointers, on chunking or on where the cluster
 *     labels live.  There are no floating-point atomics; the cluster pass uses integer atomics whose result does not depend on
 *     the order they land in (the argument of the engine's mw_ice_clusters.hip.h).
 *
 * Kernels.  The sequence of libmw_flex.so's general geometry, and at an evaluation k_nuc_q6 (one lane per molecule in sorted
 * order: n_i, the 14-double record q_6m, |q_6|, and the first MW_NUC_LIST entries as a list), k_nuc_conn (the same walk over the
 * neighbours' records: conn_i and the solid-like flag) and k_nuc_clusters (one workgroup per box, hook / compress rounds until
 * one passes without a change; a molecule with more than MW_NUC_LIST entries walks its cells instead of its list; labels and
 * sizes in LDS, 8 bytes per molecule, where that fits 160 KiB less the static arrays, in global memory through device-scope
 * relaxed atomics otherwise; its tail writes op, the three trace columns and applies the stopping rule).  Diagnostic switches read
 * by mw_nuc_init (they change no byte of any result): MW_NUC_SCRATCH_MB (default 256) and MW_NUC_LABELS_LDS (0: the labels live
 * in global memory at any size; default 1).
 *
 * Out of scope: nwater <= 64, CHILL+-based or averaged-q6 order parameters, a bias on lambda, storing crossing configurations on
 * the device, a Fortran binding.  One workgroup per box is slow for a single box of 10^5 molecules or more; it is correct there.
 *
 * Every function returns 0, or nonzero with the reason in mw_nuc_last_error().  Box indices in messages count from 0.  The
 * library lives on the device given to mw_nuc_init: every function that touches it makes that device current for the call and
 * puts the caller's current device back before it returns.
 */
#ifndef MW_NUC_H
#define MW_NUC_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_NUC_PLAN_FIELDS 12
#define MW_NUC_TRACE_FIELDS 18
#define MW_NUC_MAX_STEPS 100000000
#define MW_NUC_MIN_WATER 65
#define MW_NUC_MAX_CONN 64
/* entries of a molecule kept as a list between the rounds of the cluster pass */
#define MW_NUC_LIST 12
/* status codes beside 0 (ran), 1 (drift guard) and 2 (barostat guard) */
#define MW_NUC_REACHED_HI 3
#define MW_NUC_REACHED_LO 4

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0. */
int mw_nuc_init(int device);
int mw_nuc_finalize(void);
int mw_nuc_is_initialised(void);
const char *mw_nuc_last_error(void);

/* Host pointers. */
int mw_nuc_run(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *pos_ref,
               const unsigned long long *streams, unsigned long long seed, unsigned long long step0, int nsteps, int sample_every,
               double dt, double mass, double kT, double gamma, double pressure, double tau_p, double beta_T, int baro_every,
               int coupling, int axis, double rc, double threshold, int min_conn, int check_every, const int *lam_lo,
               const int *lam_hi, double *pos_out, double *vel_out, double *forces, double *cells_out, double *ref_out,
               double *trace, int *status, int *nn, int *label, int *op);
/* Device pointers on the library's device for every array, the scalars by value.  Work queued on the device before the
 * call is waited for, and the results are complete on return. */
int mw_nuc_run_device(int nboxes, int nwater, const double *cells, const double *pos, const double *vel, const double *pos_ref,
                      const unsigned long long *streams, unsigned long long seed, unsigned long long step0, int nsteps,
                      int sample_every, double dt, double mass, double kT, double gamma, double pressure, double tau_p,
                      double beta_T, int baro_every, int coupling, int axis, double rc, double threshold, int min_conn,
                      int check_every, const int *lam_lo, const int *lam_hi, double *pos_out, double *vel_out, double *forces,
                      double *cells_out, double *ref_out, double *trace, int *status, int *nn, int *label, int *op);

/* The launch rules for nboxes boxes of nwater molecules with the cell `cell` (9 doubles, host) -- host arithmetic only, no
 * device and no mw_nuc_init needed.  Writes min(nout, MW_NUC_PLAN_FIELDS) ints, the fields of mw_flex_plan and two more:
 *   [0] boxes per chunk   [1] chunks   [2] 0: the general geometry   [3] [4] [5] the cell grid of `cell` (that of a sigma)
 *   [6] LDS of a workgroup of the cluster pass, bytes   [7] scratch per box, bytes   [8] 0   [9] steps per launch: 1
 *   [10] 1: the cluster labels live in LDS, 0: in global memory
 *   [11] mw_nuc_plan: 0.  mw_nuc_last: the hook / compress rounds of the last call, summed over the evaluations of its first box. */
int mw_nuc_plan(int nwater, const double *cell, int nboxes, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box's input cell. */
int mw_nuc_last(int *out, int nout);
/* Event timers of the last call, summed over its steps and chunks: the five of mw_flex_elapsed_ms, then `order` (k_nuc_q6 and
 * k_nuc_conn) and `clusters` (k_nuc_clusters).  The stage 1 a check step defers counts as drift. */
int mw_nuc_elapsed_ms(float *sort, float *moments, float *forces, float *drift, float *barostat, float *order, float *clusters);

#ifdef __cplusplus
}
#endif
#endif
