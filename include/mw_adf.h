/* mw_adf.h -- C ABI of libmw_adf.so: the distribution of the O-O-O angle between the first-shell neighbours of a molecule,
 * P(theta), the second structural figure of the mW literature beside g(r) -- as integer histograms of cos(theta) over
 * caller-supplied bin edges, for every box of many periodic boxes on a gfx950 device, optionally one histogram per group
 * of centre molecules (ice-like and liquid-like centres apart, say).
 *
 * A library of its own beside libmw_hip.so (include/mw_energy.h), libmw_sk.so (include/mw_sk.h), libmw_boo.so
 * (include/mw_boo.h) and libmw_tet.so (include/mw_tet.h): it needs positions, cells, one radius and the bin edges only, so
 * it takes plain arrays and works on any configuration, with or without mw_init in the same process.  It has its own stream,
 * scratch memory and event timers.
 *
 * Inputs.  `cells` holds 9 doubles per box in the layout of mw_set_cell (cells[9 b + 3 k + a] = component a of h_(k+1)),
 * `pos` holds nwater positions in bohr as [box][nwater][3], wrapped or not.  `r_cut` (bohr) bounds the neighbours.
 *
 * Supported range.  w_k = volume / |h_l x h_m| are the perpendicular widths of the cell.  Supported: 0 < r_cut and
 * r_cut (1 + 1e-9) <= min_k w_k for every box of the call; 1 <= nwater <= 2^22; 1 <= nboxes <= 2^24; 1 <= nbins <= 1024;
 * 1 <= ngroups <= 8.  Anything else (NaN or inf included) is rejected with a message that names the argument and the first
 * offending box, and nothing is launched.
 *
 * Entries of molecule i: all pairs (j, n), n an integer lattice translation, (j, n) != (i, 0), with d = r_j + H n - r_i and
 * 0 < r^2 = |d|^2 < r_cut^2, the squares rounded once.  Within the supported range i never meets its own image; one j may
 * appear with several images in a narrow cell, and each entry counts.  n_i is the number of entries of i.  The first
 * MW_ADF_KEEP = 32 entries of i in the order in which the walk of the geometry (below) enumerates them are KEPT; the others
 * are counted in n_i and take no part in the angles.
 *
 * Angles.  For every centre i (see Groups) and every unordered pair a < b of its kept entries: u_a = d_a (1 / r_a) with an
 * IEEE square root r_a of r_a^2 and an IEEE division, c = fma(u_ax, u_bx, fma(u_ay, u_by, u_az u_bz)), clamped to [-1, 1].
 * A centre with k = min(n_i, 32) kept entries enumerates k (k - 1) / 2 pairs.
 *
 * Bins.  `edges` holds nbins + 1 HOST doubles (in both compute entries), shared by all boxes of the call: finite, strictly
 * ascending, -1 <= edges[0] and edges[nbins] <= 1.  They are edges in cos(theta), so the caller chooses between a histogram
 * uniform in cos(theta) and one uniform in theta (edges cos(theta_m), ascending) and the device needs no acos.  A pair falls
 * in bin m when edges[m] <= c < edges[m + 1]; c == edges[nbins] falls in the last bin; c outside [edges[0], edges[nbins]] is
 * enumerated but not binned.  The comparisons are exact comparisons of doubles.
 *
 * Groups.  `group` is NULL or holds nwater ints per box as [box][nwater].  group[b][i] = g in [0, ngroups): i is a centre
 * and its pairs go to histogram g of box b.  -1: i is no centre -- it is still everybody's neighbour and still has its
 * count.  Any other value is an error whose message names the box and the molecule.  group == NULL: every molecule is a
 * centre of group 0, and ngroups must be 1.
 *
 * Outputs (any may be NULL):
 *   hist[nboxes][ngroups][nbins] long long: the number of pairs per bin.
 *   counts[nboxes][nwater] ints: n_i, not capped at 32, of every molecule, centre or not.
 *   summary[nboxes][ngroups][4] long long: the centres of the group; the pairs they enumerated, sum of k (k - 1) / 2; the
 *     pairs binned (= the sum of hist over the bins); the centres with n_i > 32, whose pairs are therefore incomplete.
 *
 * Arithmetic (part of the contract, that of mw_tet.h).  H^-1 is formed once per box on the host; s = H^-1 r is reduced to
 * [0, 1) once per molecule; d = H (ds + n) from the difference ds of fractional coordinates plus the integer image shift.
 * Everything is spelled out in fma / mul / add with contraction off.  No floating-point number leaves the device and there
 * is no floating-point atomic: the results are integers, added up with integer atomics, whose order does not matter.
 *
 * Geometry.  Which of two geometries a box takes depends on nwater alone; its cell grid on the box and r_cut alone.
 *   general (nwater > 64): a fractional cell grid of g_k = max(1, floor(w_k / (r_cut (1 + 1e-9)))) cells per axis (each at
 *     most 1024, then the largest lowered until g_1 g_2 g_3 <= max(64, 2 nwater)).  A counting sort puts the molecules in
 *     cell order, inside a cell by index.  One lane per molecule enumerates its entries in the order of the 27 cell offsets
 *     (z slowest, x fastest, each -1, 0, +1, every offset with its own explicit image shift -- no minimum-image rounding:
 *     with g_k = 1 or 2 the three offsets are the three images) and inside a cell in index order.
 *   small (nwater <= 64): one wavefront per box, one box per workgroup, the box in LDS; the entries of i are enumerated over
 *     j in index order and for each j over the eight combinations of the two images per axis that can come within r_cut
 *     (ds_k itself and ds_k - 1 if ds_k > 0, else ds_k + 1; combination bit k choosing the second image along axis k,
 *     combinations 0..7 in order).
 * That order decides which 32 entries are kept where n_i > 32, and nothing else.  Hence the bytes of a box's results depend
 * on its cell, its positions, its groups, r_cut and the edges alone: not on the other boxes of the call, on batch versus
 * single calls, on host versus device pointers, on chunking or on the run.
 *
 * Scratch.  The general geometry keeps the sorted fractional positions and the cell tables in scratch memory; a call is
 * processed in chunks of as many boxes as fit the budget: 256 MiB, or MW_ADF_SCRATCH_MB (MiB, read by mw_adf_init).  The
 * histogram and the summary of a box (8 ngroups nbins + 32 ngroups bytes) count towards its scratch in both geometries.  A
 * box that does not fit alone is an error.  The small geometry takes up to 2^20 boxes per chunk.
 *
 * Every function returns 0, or nonzero with the reason in mw_adf_last_error().  A rejected call launches nothing and writes
 * nothing; its message names the entry and the argument, and box and molecule indices in messages count from 0.  Arguments
 * are checked before the library's state, so a call with bad arguments says so with or without a device (the device-pointer
 * entry can read its cells and groups only once the library is live, and checks them then, before it launches).  The library
 * lives on the device given to mw_adf_init: every function that touches it makes that device current for the call and puts
 * the caller's current device back before it returns.
 */
#ifndef MW_ADF_H
#define MW_ADF_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_ADF_PLAN_FIELDS 9
#define MW_ADF_KEEP 32
#define MW_ADF_MAX_BINS 1024
#define MW_ADF_MAX_GROUPS 8

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0.  A failed init
 * gives back the stream and events it made and leaves the library not initialised. */
int mw_adf_init(int device);
int mw_adf_finalize(void);
int mw_adf_is_initialised(void);
const char *mw_adf_last_error(void);

/* Host pointers. */
int mw_adf_compute(int nboxes, int nwater, const double *cells, const double *pos, double r_cut, int nbins, const double *edges,
                   int ngroups, const int *group, long long *hist, int *counts, long long *summary);
/* Device pointers on the library's device for every array but `edges`, which stays a host pointer.  Work queued on the
 * device before the call is waited for, and the results are complete on return. */
int mw_adf_compute_device(int nboxes, int nwater, const double *cells, const double *pos, double r_cut, int nbins, const double *edges,
                          int ngroups, const int *group, long long *hist, int *counts, long long *summary);

/* The launch rules for nboxes boxes of nwater molecules with the cell `cell` (9 doubles, host), the radius and the sizes of
 * the histograms -- host arithmetic only, no device and no mw_adf_init needed (the scratch budget is then the default one).
 * Writes min(nout, MW_ADF_PLAN_FIELDS) ints, the fields of mw_tet_plan:
 *   [0] boxes per chunk   [1] chunks = ceil(nboxes / [0])   [2] 1: small geometry, 0: general
 *   [3] [4] [5] the cell grid g_1, g_2, g_3 (the small geometry reports it and does not use it)
 *   [6] LDS of a workgroup, bytes   [7] scratch per box, bytes   [8] boxes per workgroup (small) or 0 */
int mw_adf_plan(int nwater, const double *cell, double r_cut, int nbins, int ngroups, int nboxes, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box. */
int mw_adf_last(int *out, int nout);
/* Event timers of the last call, summed over its chunks: the binning pass (the counting sort; 0 in the small geometry), the
 * angle pass (the walk, the pairs, the histograms in LDS and their flush) and the reduce pass (the zeroing of the hist and
 * summary that the flush adds into). */
int mw_adf_elapsed_ms(float *binning, float *angles, float *reduce);

#ifdef __cplusplus
}
#endif
#endif
