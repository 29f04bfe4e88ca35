/* mw_rings.h -- C ABI of libmw_rings.so: the primitive (shortest-path) rings of 3 to 7 members of the bond network of every
 * box of many periodic boxes on a gfx950 device -- the ring-size histogram, the rings every molecule sits in and, on request,
 * the list of the rings themselves, from which chair/boat rings and cages are host arithmetic.  Ice is the network in which
 * every molecule sits in twelve 6-rings; supercooled mW is described by its 5-, 6- and 7-rings.
 *
 * A library of its own beside libmw_hip.so (include/mw_energy.h), libmw_sk.so (include/mw_sk.h), libmw_boo.so
 * (include/mw_boo.h), libmw_tet.so (include/mw_tet.h) and libmw_adf.so (include/mw_adf.h): it needs positions, cells and one
 * radius only, so it takes plain arrays and works on any configuration, with or without mw_init in the same process.  It has
 * its own stream, scratch memory and event timers.
 *
 * Inputs.  `cells` holds 9 doubles per box in the layout of mw_set_cell (cells[9 b + 3 k + a] = component a of h_(k+1): column
 * k of the 3 x 3 matrix H is h_k), `pos` holds nwater positions in bohr as [box][nwater][3], wrapped or not.  `r_cut` (bohr)
 * bounds a bond.
 *
 * Supported range.  w_k = volume / |h_l x h_m| are the perpendicular widths of the cell.  Supported: 0 < r_cut and
 * r_cut (1 + 1e-9) <= min_k w_k for every box of the call; 1 <= nwater <= 2^22; 1 <= nboxes <= 2^24; list_cap >= 0.  Anything
 * else (NaN or inf included) is rejected with a message that names the entry, the argument and the first offending box, and
 * nothing is launched.
 *
 * Entries of molecule i (those of mw_adf.h): all pairs (j, n), n an integer lattice translation, (j, n) != (i, 0), with
 * d = H (s_j - s_i + n) and 0 < r^2 = |d|^2 < r_cut^2, the squares rounded once; s = H^-1 r reduced to [0, 1) once per molecule,
 * H^-1 formed once per box on the host, everything spelled out in fma / mul / add with contraction off.  Within the supported
 * range every n_k is -1, 0 or 1 and i never meets its own image; one j may appear with several images in a narrow cell, and
 * each is an entry.  n_i is the number of entries of i.  (j, n) is an entry of i exactly when (i, -n) is one of j: the
 * arithmetic of one is the negation of the other's.
 *
 * Graph.  A node is (molecule, lattice translation m).  (i, m) and (j, m + n) are joined when (j, n) is an entry of i and
 * n_i <= MW_RINGS_DEG = 8 and n_j <= 8.  A molecule with more than 8 entries has no edges at all: it is counted
 * (summary[0]), and nothing depends on the order in which a walk met its entries.
 *
 * Closed paths.  A closed path of length L, 3 <= L <= 7, is L distinct nodes v_0 ... v_(L-1), consecutive ones joined and
 * v_(L-1) joined to v_0 itself: the image shifts round the path sum to zero, and a path that comes back to another image of
 * its first molecule is not closed.  Rings are counted once per unit cell.  Each of the 2 L rooted, directed readings of a
 * ring is the sequence of tuples (molecule, n_1, n_2, n_3) of its nodes with the root's translation taken off; the ring is
 * counted at the lexicographically smallest reading (no two readings of a finite ring are equal).  In the common case -- the
 * root's index is below every other member's and mol(v_1) != mol(v_(L-1)) -- that is "the root has the smallest index and
 * mol(v_1) < mol(v_(L-1))"; a ring that holds its smallest molecule at two images, or the same molecule on both sides of
 * the root, takes the comparison of all readings.
 *
 * Primitive rings.  A closed path is a primitive ring if no two of its nodes are closer in the graph than round the ring:
 * no two nodes that are not neighbours in the ring are joined, and no two nodes three apart round the ring (L = 6, 7) have a
 * common neighbour, images included.
 *
 * Outputs (any may be NULL; indices count from 0; size index t stands for L = t + 3):
 *   hist[nboxes][5] long long: the primitive rings of 3 ... 7 members.
 *   closed[nboxes][5] long long: the closed paths, before the shortest-path test.
 *   member[nboxes][nwater][5] ints: how many nodes of primitive rings of each size are images of the molecule; summed over
 *     a box this is L hist[L].
 *   counts[nboxes][nwater] ints: n_i, not capped.
 *   summary[nboxes][4] long long: the molecules with n_i > 8; the undirected edges per cell; the primitive rings outside the common
 *     case above (the ones that took the comparison of all readings); the primitive rings of all sizes.
 *   list[nboxes][list_cap][8] ints: one row (L, m_0 ... m_6) per primitive ring, the molecules of its smallest reading, -1
 *     beyond L.  Rows by ascending root; the rings of one root in the order a depth-first walk from it meets them that tries
 *     the entries of every node in ascending (j, n_1, n_2, n_3).  Rings beyond list_cap are not written -- summary[.][3] is
 *     what the caller needed --, rows not used are filled with -1, and list_cap = 0 writes nothing.
 * The bytes of a box's results depend on its cell, its positions and r_cut alone: not on the other boxes of the call, on
 * batch versus single calls, on host versus device pointers, on chunking, on which outputs were asked for or on the run.  No
 * floating-point number leaves the device and there is no floating-point atomic.
 *
 * Geometry.  The entries are found in one of two geometries, chosen by nwater alone (those of mw_adf.h):
 *   general (nwater > 64): a fractional cell grid of g_k = max(1, floor(w_k / (r_cut (1 + 1e-9)))) cells per axis (each at
 *     most 1024, then the largest lowered until g_1 g_2 g_3 <= max(64, 2 nwater)), a counting sort, one lane per molecule
 *     over the 27 neighbouring cells, every offset with its own explicit image shift.
 *   small (nwater <= 64): one wavefront per box, the box in LDS, per j the eight combinations of the two images per axis
 *     that can come within r_cut.
 * Either writes n_i and the first 8 entries of every molecule to scratch; a second pass sorts every row by (j, n) and drops
 * the entries of and to molecules over the cap.  The walk then takes one lane per (root, first edge).
 *
 * Scratch.  The rows, the per-lane ring counts of the list and (general geometry) the sorted fractional positions and cell
 * tables live in scratch memory; a call is processed in chunks of as many boxes as fit the budget: 256 MiB, or
 * MW_RINGS_SCRATCH_MB (MiB, read by mw_rings_init), at most 65535 boxes.  A box that does not fit alone is an error.
 *
 * Every function returns 0, or nonzero with the reason in mw_rings_last_error().  A rejected call launches nothing and
 * writes nothing; box indices in messages count from 0.  Arguments are checked before the library's state, so a call with bad
 * arguments says so with or without a device (the device-pointer entry can read its cells only once the library is live, and
 * checks them then, before it launches).  The library lives on the device given to mw_rings_init: every function that
 * touches it makes that device current for the call and puts the caller's current device back before it returns.
 */
#ifndef MW_RINGS_H
#define MW_RINGS_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_RINGS_PLAN_FIELDS 9
#define MW_RINGS_DEG 8
#define MW_RINGS_SIZES 5
#define MW_RINGS_MAX 7

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0.  A failed init
 * gives back the stream and events it made and leaves the library not initialised. */
int mw_rings_init(int device);
int mw_rings_finalize(void);
int mw_rings_is_initialised(void);
const char *mw_rings_last_error(void);

/* Host pointers. */
int mw_rings_compute(int nboxes, int nwater, const double *cells, const double *pos, double r_cut, int list_cap, long long *hist,
                     long long *closed, int *member, int *counts, long long *summary, int *list);
/* Device pointers on the library's device for every array.  Work queued on the device before the call is waited for, and
 * the results are complete on return. */
int mw_rings_compute_device(int nboxes, int nwater, const double *cells, const double *pos, double r_cut, int list_cap, long long *hist,
                            long long *closed, int *member, int *counts, long long *summary, int *list);

/* The launch rules for nboxes boxes of nwater molecules with the cell `cell` (9 doubles, host) and the radius -- host
 * arithmetic only, no device and no mw_rings_init needed (the scratch budget is then the default one).  Writes
 * min(nout, MW_RINGS_PLAN_FIELDS) ints, the fields of mw_tet_plan:
 *   [0] boxes per chunk   [1] chunks = ceil(nboxes / [0])   [2] 1: small geometry, 0: general
 *   [3] [4] [5] the cell grid g_1, g_2, g_3 (the small geometry reports it and does not use it)
 *   [6] LDS of a workgroup of the walk, bytes   [7] scratch per box, bytes   [8] boxes per workgroup (small) or 0 */
int mw_rings_plan(int nwater, const double *cell, double r_cut, int nboxes, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box. */
int mw_rings_last(int *out, int nout);
/* Event timers of the last call, summed over its chunks: the binning pass (the counting sort; 0 in the small geometry), the
 * adjacency pass (the entries and the sorted rows) and the walk pass (the zeroing of the results, the walk and, where a
 * list was asked for, the scan and the second walk). */
int mw_rings_elapsed_ms(float *binning, float *adjacency, float *walk);

#ifdef __cplusplus
}
#endif
#endif
