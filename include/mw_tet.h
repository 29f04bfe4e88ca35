/* mw_tet.h -- C ABI of libmw_tet.so: the order parameters of the water literature that come from a molecule's nearest
 * neighbours sorted by distance -- the Errington-Debenedetti tetrahedral order q, its translational companion S_k
 * (Chau-Hardwick), the fifth-neighbour distance d5 and the local structure index (LSI) -- and the four-nearest-neighbour
 * network, for every molecule of many periodic boxes on a gfx950 device.
 *
 * A library of its own beside libmw_hip.so (include/mw_energy.h), libmw_sk.so (include/mw_sk.h) and libmw_boo.so
 * (include/mw_boo.h): it needs positions, cells and two radii only, so it takes plain arrays and works on any
 * configuration, with or without mw_init in the same process.  It has its own stream, scratch memory and event timers.
 *
 * Inputs.  `cells` holds 9 doubles per box in the layout of mw_set_cell (cells[9 b + 3 k + a] = component a of h_(k+1)),
 * `pos` holds nwater positions in bohr as [box][nwater][3], wrapped or not.  `r_search` (bohr) bounds the neighbour search,
 * `r_lsi` (bohr) is the radius of the local structure index.
 *
 * Supported range.  w_k = volume / |h_l x h_m| are the perpendicular widths of the cell.  Supported: 0 < r_lsi <= r_search
 * and r_search (1 + 1e-9) <= min_k w_k for every box of the call; 1 <= nwater <= 2^22; 1 <= nboxes <= 2^24.  Anything else
 * (NaN or inf included) is rejected with a message that names the argument and the first offending box, and nothing is
 * launched.
 *
 * Entries of molecule i: all pairs (j, n), n an integer lattice translation, (j, n) != (i, 0), with d = r_j + H n - r_i and
 * 0 < |d| < r_search.  Within the supported range i never meets its own image; one j may appear with several images in a
 * narrow cell, and each entry counts.
 *
 * Rank.  The entries of i are ranked ascending by r^2 = |d|^2; entries of equal r^2 are ranked in the order in which the
 * walk of the geometry (below) enumerates them.  Only the MW_TET_KEEP = 16 nearest are kept.  r_a and u_a = d_a / r_a are
 * the distance and the unit vector of rank a = 1, 2, ...
 *
 * Outputs (any may be NULL):
 *   counts[nboxes][nwater][2] ints: (n_search, n_lsi), the numbers of entries with |d| < r_search and with |d| < r_lsi,
 *     not capped at 16.
 *   near[nboxes][nwater][4] ints: the molecule index j (from 0) of ranks 1..4; -1 where n_search is smaller.
 *   order[nboxes][nwater][4] doubles: (q, s_k, d5, lsi),
 *     q   = 1 - 3/8 sum_{a<b<=4} (u_a . u_b + 1/3)^2, the pairs in the order (1,2) (1,3) (1,4) (2,3) (2,4) (3,4);
 *     s_k = 1 - 1/3 sum_{a<=4} (r_a - rbar)^2 / (4 rbar^2), rbar the mean of the four;
 *           q and s_k are defined when n_search >= 4;
 *     d5  = r_5 (bohr), defined when n_search >= 5;
 *     lsi = 1/n sum_{a<=n} (D_a - Dbar)^2 (bohr^2) with n = n_lsi, D_a = r_(a+1) - r_a and Dbar their mean; defined when
 *           1 <= n and n + 1 <= min(n_search, 16).
 *     A value that is not defined is the quiet NaN with the bits 0x7ff8000000000000.
 *   summary[nboxes][8] doubles: the means of q, s_k, d5, lsi over the molecules where each is defined (that NaN where none
 *     is), then the four numbers of molecules where each is defined.
 *
 * Arithmetic (part of the contract).  H^-1 is formed once per box on the host; s = H^-1 r is reduced to [0, 1) once per
 * molecule; d = H (ds + n) from the difference ds of fractional coordinates plus the integer image shift; r_a by an IEEE
 * square root of r^2, u_a = d_a (1 / r_a) with an IEEE division; the sums above run in the order written, (r_1 + r_2) +
 * r_3 ... from the left.  Everything is spelled out in fma / mul / add with contraction off.  An entry counts towards
 * n_search when r^2 < r_search^2 and towards n_lsi when r^2 < r_lsi^2, the squares rounded once.
 *
 * Geometry.  Which of two geometries a box takes depends on nwater alone; its cell grid on the box and r_search alone.
 *   general (nwater > 64): a fractional cell grid of g_k = max(1, floor(w_k / (r_search (1 + 1e-9)))) cells per axis (each
 *     at most 1024, then the largest lowered until g_1 g_2 g_3 <= max(64, 2 nwater)).  A counting sort puts the molecules
 *     in cell order, inside a cell by index.  One lane per molecule enumerates its entries in the order of the 27 cell
 *     offsets (z slowest, x fastest, each -1, 0, +1, every offset with its own explicit image shift -- no minimum-image
 *     rounding: with g_k = 1 or 2 the three offsets are the three images) and inside a cell in index order.
 *   small (nwater <= 64): one wavefront per box, four boxes per workgroup, the box in LDS; the entries of i are enumerated
 *     over j in index order and for each j over the eight combinations of the two images per axis that can come within
 *     r_search (combination bit k choosing the second image along axis k).
 * The box sums of the summary are added in a fixed order with no floating-point atomics.  Hence the bytes of a box's
 * results depend on its cell, its positions and the two radii alone: not on the other boxes of the call, on batch versus
 * single calls, on host versus device pointers, on chunking or on the run.
 *
 * Scratch.  The general geometry keeps the sorted fractional positions, the cell tables and the four values of every
 * molecule in scratch memory; a call is processed in chunks of as many boxes as fit the budget: 256 MiB, or
 * MW_TET_SCRATCH_MB (MiB, read by mw_tet_init).  A box that does not fit alone is an error.  The small geometry needs no
 * scratch and takes up to 2^20 boxes per chunk.
 *
 * Every function returns 0, or nonzero with the reason in mw_tet_last_error().  A rejected call launches nothing and writes
 * nothing; its message names the entry and the argument, and box indices in messages count from 0.  Arguments are checked
 * before the library's state, so a call with bad arguments says so with or without a device.  The library lives on the
 * device given to mw_tet_init: every function that touches it makes that device current for the call and puts the caller's
 * current device back before it returns.
 */
#ifndef MW_TET_H
#define MW_TET_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_TET_PLAN_FIELDS 9
#define MW_TET_KEEP 16

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0.  A failed init
 * gives back the stream and events it made and leaves the library not initialised. */
int mw_tet_init(int device);
int mw_tet_finalize(void);
int mw_tet_is_initialised(void);
const char *mw_tet_last_error(void);

/* Host pointers. */
int mw_tet_compute(int nboxes, int nwater, const double *cells, const double *pos, double r_search, double r_lsi,
                   double *order, int *near, int *counts, double *summary);
/* Device pointers on the library's device for every array.  Work queued on the device before the call is waited for,
 * and the results are complete on return. */
int mw_tet_compute_device(int nboxes, int nwater, const double *cells, const double *pos, double r_search, double r_lsi,
                          double *order, int *near, int *counts, double *summary);

/* The launch rules for nboxes boxes of nwater molecules with the cell `cell` (9 doubles, host) and the search radius --
 * host arithmetic only, no device and no mw_tet_init needed (the scratch budget is then the default one).  Writes
 * min(nout, MW_TET_PLAN_FIELDS) ints:
 *   [0] boxes per chunk   [1] chunks = ceil(nboxes / [0])   [2] 1: small geometry, 0: general
 *   [3] [4] [5] the cell grid g_1, g_2, g_3 (the small geometry reports it and does not use it)
 *   [6] LDS of a workgroup, bytes   [7] scratch per box, bytes   [8] boxes per workgroup (small) or 0 */
int mw_tet_plan(int nwater, const double *cell, double r_search, int nboxes, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box. */
int mw_tet_last(int *out, int nout);
/* Event timers of the last call, summed over its chunks: the binning pass, the selection pass and the summary pass.  The
 * small geometry is one kernel: its time is reported as the selection pass and the others are 0. */
int mw_tet_elapsed_ms(float *binning, float *select, float *summary);

#ifdef __cplusplus
}
#endif
#endif
