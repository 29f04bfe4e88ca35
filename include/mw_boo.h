/* mw_boo.h -- C ABI of libmw_boo.so: the Steinhardt bond-order parameters q4, q6, their neighbour averages and the
 * solid-like connection count of every molecule of many periodic boxes on a gfx950 device.
 *
 * A library of its own beside libmw_hip.so (include/mw_energy.h) and libmw_sk.so (include/mw_sk.h): bond order needs
 * positions, cells and a cutoff only, so it takes plain arrays and works on any configuration, with or without mw_init in
 * the same process.  It has its own stream, scratch memory and event timers.
 *
 * Inputs.  `cells` holds 9 doubles per box in the layout of mw_set_cell (cells[9 b + 3 k + a] = component a of h_(k+1)),
 * `pos` holds nwater positions in bohr as [box][nwater][3], wrapped or not.  `rc` (bohr) is the bond cutoff, `threshold`
 * the connection threshold, finite and in [-1, 1].
 *
 * Cell widths and cutoff range.  w_k = volume / |h_l x h_m| are the perpendicular widths of the cell.  Supported:
 * 0 < rc and rc (1 + 1e-9) <= min_k w_k for every box of the call.  Anything else (NaN included) is rejected with a message
 * that names rc and the first offending box, and nothing is launched.
 *
 * Neighbour entries of molecule i: all pairs (j, n), n an integer lattice translation, (j, n) != (i, 0), with
 * d = r_j + H n - r_i and 0 < |d| < rc.  Within the supported range i never neighbours its own image; one j may appear
 * with several images in a narrow cell, and each entry counts.  n_i is the number of entries.
 *
 * Per molecule, with u = d / |d| and Y_lm a real orthonormal basis of the harmonics of degree l (9 components for l = 4,
 * 13 for l = 6):
 *     q_lm(i)    = (1 / n_i) sum_entries Y_lm(u)                 (0 where n_i = 0)
 *     q_l(i)     = sqrt(4 pi / (2 l + 1) sum_m q_lm(i)^2)
 *     qbar_lm(i) = (q_lm(i) + sum_entries q_lm(j)) / (n_i + 1),   qbar_l(i) from qbar_lm as q_l from q_lm
 *     s_ij       = sum_m q_6m(i) q_6m(j) / (|q_6(i)| |q_6(j)|)    for every entry;  conn_i = #{entries: s_ij > threshold};
 *                  |q_6| = 0 on either side makes no connection.
 * Per box:  Q_l from Q_lm = sum_i n_i q_lm(i) / sum_i n_i (0 when the box has no bonds), and the plain means over the
 * molecules of qbar_4 and qbar_6.
 *
 * Outputs (any may be NULL):  q[nboxes][nwater][4] = (q4, q6, qbar4, qbar6) doubles;  nn[nboxes][nwater][2] = (n_i, conn_i)
 * ints;  summary[nboxes][4] = (Q4, Q6, <qbar4>, <qbar6>) doubles.
 *
 * Arithmetic (part of the contract).  The basis is held scaled by sqrt(4 pi / (2 l + 1)), so that sum_m Y_lm(u) Y_lm(v) =
 * P_l(u . v) and q_l^2 is the plain sum of squares: component (m, cos) = c_lm P_l^(m)(u_z) Re (u_x + i u_y)^m and (m, sin)
 * the same with Im, c_lm^2 = (2 - delta_m0) (l - m)! / (l + m)!, P_l^(m) the m-th derivative of the Legendre polynomial.
 * H^-1 is formed once per box on the host; s = H^-1 r is reduced to [0, 1) once per molecule; d = H ds from the
 * difference ds of fractional coordinates plus the integer image shift; 1 / |d| by an IEEE square root and division.
 * Everything is spelled out in fma / mul / add with contraction off.
 *
 * Geometry.  Which of two geometries a box takes depends on nwater alone; its cell grid on the box and rc alone.
 *   general (nwater > 64): a fractional cell grid of g_k = max(1, floor(w_k / (rc (1 + 1e-9)))) cells per axis (each at most
 *     1024, then the largest lowered until g_1 g_2 g_3 <= max(64, 2 nwater)).  A counting sort puts the molecules in cell
 *     order, inside a cell by index.  A molecule's entries are added in the order of the 27 cell offsets (z slowest, x
 *     fastest, each -1, 0, +1, every offset with its own explicit image shift -- no minimum-image rounding: with g_k = 1
 *     or 2 the three offsets are the three images) and inside a cell in index order.
 *   small (nwater <= 64): one wavefront per box, four boxes per workgroup, the box in LDS; the entries of i run over j in
 *     index order and for each j over the eight combinations of the two images per axis that can come within rc.
 * Box sums are added in a fixed order with no floating-point atomics.  Hence the bytes of a box's results depend on its
 * cell, its positions, rc and threshold alone: not on the other boxes of the call, on batch versus single calls, on host
 * versus device pointers, on chunking or on the run.
 *
 * Scratch.  The general geometry keeps the sorted fractional positions, the cell tables and 24 doubles per molecule in
 * scratch memory; a call is processed in chunks of as many boxes as fit the budget: 256 MiB, or MW_BOO_SCRATCH_MB (MiB,
 * read by mw_boo_init).  A box that does not fit alone is an error.  The small geometry needs no scratch and takes up to
 * 2^20 boxes per chunk.
 *
 * Every function returns 0, or nonzero with the reason in mw_boo_last_error().  A rejected call launches nothing and writes
 * nothing; its message names the argument, and box indices in messages count from 0.  Arguments are checked before the
 * library's state, so a call with bad arguments says so with or without a device.  The library lives on the device given to
 * mw_boo_init: every function that touches it makes that device current for the call and puts the caller's current device
 * back before it returns.
 */
#ifndef MW_BOO_H
#define MW_BOO_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_BOO_PLAN_FIELDS 9

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0.  A failed init
 * gives back the stream and events it made and leaves the library not initialised. */
int mw_boo_init(int device);
int mw_boo_finalize(void);
int mw_boo_is_initialised(void);
const char *mw_boo_last_error(void);

/* Host pointers. */
int mw_boo_compute(int nboxes, int nwater, const double *cells, const double *pos, double rc, double threshold,
                   double *q, int *nn, double *summary);
/* Device pointers on the library's device for every array.  Work queued on the device before the call is waited for,
 * and the results are complete on return. */
int mw_boo_compute_device(int nboxes, int nwater, const double *cells, const double *pos, double rc, double threshold,
                          double *q, int *nn, double *summary);

/* The launch rules for nboxes boxes of nwater molecules with the cell `cell` (9 doubles, host) and the cutoff rc -- host
 * arithmetic only, no device and no mw_boo_init needed (the scratch budget is then the default one).  Writes
 * min(nout, MW_BOO_PLAN_FIELDS) ints:
 *   [0] boxes per chunk   [1] chunks = ceil(nboxes / [0])   [2] 1: small geometry, 0: general
 *   [3] [4] [5] the cell grid g_1, g_2, g_3 (the small geometry reports it and does not use it)
 *   [6] LDS of a workgroup, bytes   [7] scratch per box, bytes   [8] boxes per workgroup (small) or 0 */
int mw_boo_plan(int nwater, const double *cell, double rc, int nboxes, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box. */
int mw_boo_last(int *out, int nout);
/* Event timers of the last call, summed over its chunks: the binning pass, pass 1, pass 2 and the summary pass.  The small
 * geometry is one kernel: its time is reported as pass 1 and the others are 0. */
int mw_boo_elapsed_ms(float *binning, float *pass1, float *pass2, float *summary);

#ifdef __cplusplus
}
#endif
#endif
