/* mw_coll.h -- C ABI of libmw_coll.so: collective time correlations of trajectories.  For every one of many periodic boxes,
 * from frames equally spaced in time: the density modes rho(n, t) of every frame, the coherent intermediate scattering
 * function F(n, t), integer histograms of the distinct van Hove function G_d(r, t) and the sums of the overlap Q(t0, t) and of
 * its square (for the four-point susceptibility chi_4(t)), each over every time origin, on a gfx950 device.
 *
 * A library of its own beside libmw_hip.so (include/mw_energy.h) and the other device libraries: it takes plain arrays of
 * unwrapped positions and the boxes' cells, needs no neighbour list, and has its own stream, scratch memory and event timers.
 * It is the collective half of what the single-particle time correlation library leaves out.  There is no CPU path.
 *
 * Inputs.  `cells` [nboxes][9] doubles in mw_sk.h's layout (cells[9 b + 3 k + a] = component a of cell vector h_(k+1)); a box's
 * cell is fixed over the trajectory.  `pos` [nframes][nboxes][nwater][3] doubles, unwrapped, frame-major.  Lags
 * l = 0 .. nlags - 1 (in frames), 1 <= nlags <= nframes.  origin_every = s >= 1: the origins are t0 = 0, s, 2 s, ... with
 * t0 + l <= nframes - 1, so lag l has o_l = (nframes - 1 - l) / s + 1 origins (integer division), ascending.  `nvec` [M][3]
 * integer triples, 0 <= M <= MW_COLL_MAX_VECTORS, |n_a| <= MW_COLL_MAX_COMPONENT.  `r_max` (bohr), `nbins`
 * (0, or 1 .. MW_COLL_MAX_BINS) and `hist_lags` [nh] (0 <= nh <= MW_COLL_MAX_HIST_LAGS, each in [0, nlags)) select the
 * distinct van Hove work.  `overlap_a` (bohr): 0 is off, otherwise finite and > 0.  cells, nvec and hist_lags are host arrays
 * in both compute entries.
 *
 * Supported range.  1 <= nframes <= MW_COLL_MAX_FRAMES; 1 <= nwater <= 2^22; 1 <= nboxes <= 2^24; every position finite; every
 * cell with a determinant that is finite and not 0; ceil(nwater / 64) x o_0 < 2^31 when the overlap is asked for.  A call
 * whose counts could pass 2^62 is rejected: o_0 x nwater^2 x images for `gd` (images = the translations of the box's image
 * rule below, 1 to 27), o_0 x nwater^2 for `q2sum`.  `rho` or `fkt` with M = 0, `gd` with nbins = 0 or nh = 0 or an r_max that
 * is not finite and > 0, `qsum` or `q2sum` with overlap_a = 0: all rejected.  A rejected call launches nothing and writes
 * nothing, and its message names the entry, the argument and the first offending frame, box or index.  (The device-pointer
 * entry looks at its positions with one kernel before the run and reads its verdict; that kernel writes nothing but the
 * verdict.)  Any output may be NULL, and the work for a NULL output is not done.
 *
 * Outputs and their arithmetic (part of the contract).  Contraction is off; everything is spelled out in fma / mul / add /
 * sqrt / div.  No floating-point atomics anywhere.
 *
 * 1. rho [nframes][nboxes][M][2] (re, im): the density modes rho(n) = sum_j exp(-2 pi i n . s_j), s_j = H^-1 r_j, of every
 *    frame.  The arithmetic is mw_sk.h's, restated: H^-1 once per box on the host (cofactors and determinant by fma chains, one
 *    division per element); s_j once per molecule by the fma chain fma(I_a0, x, fma(I_a1, y, I_a2 z)), reduced by s - rint(s);
 *    the per-axis phasors E_a(m) = exp(2 pi i m s_a), m = 0 .. max |n_a|, each by one sincospi((2 m) s_a); a negative component
 *    takes the conjugate of the same entry; with P = E_1 E_2 as (fma(e0.x, e1.x, -(y0 y1)), fma(e0.x, y1, y0 e1.x)) and
 *    R = P E_3 likewise, molecule j adds (R.re, -R.im).  The molecules are summed in segments of 1024 x ceil(nwater / 8192)
 *    consecutive molecules, each sequentially from 0, and the segments' sums are added in segment order onto the first.  Hence
 *    rho of a frame is byte for byte what mw_sk_compute returns for that frame's positions and the box's cell, and rho(-n) is
 *    bit for bit the conjugate of rho(n).
 *
 * 2. fkt [nboxes][nlags][M][2]: F_b(n, l) = sum_t0 rho(n, t0 + l) conj rho(n, t0) / (o_l nwater).  With A = rho(n, t0 + l),
 *    B = rho(n, t0), (re, im) = (0, 0) and the origins ascending from 0:
 *        re = fma(A_re, B_re, fma(A_im, B_im, re))
 *        im = fma(A_im, B_re, fma(-A_re, B_im, im))
 *    then one division of each by the double (double)o_l * (double)nwater.  rho(-n) is bitwise conj rho(n) and every rounding
 *    is odd, so fkt(-n) is bitwise conj fkt(n).  The bytes depend on the box's frames, its cell, n and the call's scalars alone.
 *
 * 3. gd [nboxes][nh][nbins], 64-bit counts: for lag l = hist_lags[h] the number of ordered (i, j, lattice translation n) with
 *    (j, n) != (i, 0), over all origins of l, with d = |r_j(t0 + l) + n . h - r_i(t0)|, 0 <= d < r_max, in bin
 *    floor(d nbins / r_max).  The arithmetic is mw_rdf's: with c0 = h2 x h3, c1 = h3 x h1, c2 = h1 x h2 (each component
 *    a b - c d, two products and a difference), det = h1 . c0 (three products added left to right), inv = 1 / det, the rows
 *    of the inverse are g_k = c_k inv, and the perpendicular widths w_k = |det| / |c_k| (|c_k| = sqrt of three squares added
 *    left to right).  s = (fma(g_k0, x, fma(g_k1, y, g_k2 z)))_k of a molecule, once; ds = s_j - s_i, ds -= rint(ds);
 *    d0 = (fma(h1_a, ds_1, fma(h2_a, ds_2, h3_a ds_3)))_a; per axis k the images n_k = 0 alone where
 *    r_max (1 + 1e-9) <= w_k / 2, else n_k in {-1, 0, 1}; t1 = fma(n_1, h1, d0), t2 = fma(n_2, h2, t1), d = fma(n_3, h3, t2)
 *    per component; r2 = fma(dx, dx, fma(dy, dy, dz dz)); counted where r2 < r_max r_max, in bin
 *    min((int)(sqrt(r2) * ((double)nbins / r_max)), nbins - 1).  Admission: r_max (1 + 1e-9) <= 1.5 x the smallest w_k of
 *    every box, or the call is rejected and names the first box that fails.  The excluded term is (j = i, n = 0), by index, not
 *    by d > 0: at l > 0 a pair j != i may sit at d = 0, and it counts.  At l = 0 a row is o_0 pair histograms of single
 *    frames, added.  Counters: 32-bit in LDS, flushed to the 64-bit result with integer atomics.  In the tile geometry a
 *    workgroup adds at most 256 x 256 x 27 = 1 769 472 per tile of j and flushes every MW_COLL_FLUSH_TILES = 2048 of them:
 *    3.62e9 < 2^32.  In the one-wavefront geometry (nwater <= 64) a wavefront adds at most 64 x 64 x 27 = 110 592 per origin and
 *    takes at most ceil(65536 / MW_COLL_SLABS) = 2048 origins: 2.3e8 < 2^32.
 *
 * 4. qsum, q2sum [nboxes][nlags], 64-bit: Q(t0, l) = #{j : d2_j < a a}, a = overlap_a, with D = x_j(t0 + l) - x_j(t0) per
 *    component on the unwrapped positions as they are (no centre is removed) and d2 = fma(Dx, Dx, fma(Dy, Dy, Dz Dz));
 *    qsum = sum_t0 Q, q2sum = sum_t0 Q Q.  Q of an (origin, lag) is complete for the whole box, in an integer scratch, before
 *    a second pass squares it.
 *
 * Integers do not depend on any order.  Hence the bytes of a box's results depend on that box's frames, its cell and the
 * call's scalars and lists alone: not on the other boxes of the call, on batch versus single calls, on host versus device
 * pointers, on chunking or on the scratch budget.
 *
 * Mechanism.  The mode pass runs the structure-factor kernels on (frames x boxes) "boxes", a launch of as many as the scratch
 * holds, and also keeps rho transposed in scratch, [box][vector][re | im][frame], so that the correlation pass -- one lane per
 * (box, vector, lag), origins sequential -- reads consecutive doubles in lanes at consecutive lags.  The pair pass: a workgroup
 * of 256 lanes takes (box, selected lag, slab of origins, tile of 256 molecules i), keeps s_i(t0) in registers and streams the
 * tiles of s_j(t0 + l) through LDS; every j is met, there is no i <-> j halving across two frames.  The origins of a lag are
 * cut into at most MW_COLL_SLABS slabs.  Boxes of at most 64 molecules: one wavefront per (box, selected lag, slab), four to a
 * workgroup, each with its own LDS.  The overlap: a wavefront per (box, origin, tile of 64 molecules) counts every lag into an
 * integer scratch [box][lag][origin] (32-bit integer atomics), and one lane per (box, lag) adds Q and Q Q.  A call is
 * processed in chunks of as many boxes as fit the scratch budget (MW_COLL_SCRATCH_MB, MiB, read by mw_coll_init, default 256:
 * the transposed modes, kept only when fkt is asked for, and the overlap counts of every box of the chunk; the mode pass keeps a quarter of the budget for its
 * tables and partial sums -- at least those of one frame of one box, at most those of 65535 -- and takes what the chunk's
 * boxes leave); a box that does not fit alone is an error.  The host-pointer entry stages the whole trajectory on the device, outside that budget.
 *
 * Out of scope: cells that move during the trajectory, removal of the centre of mass, the distinct part of the overlap,
 * multiple-tau schemes, stress correlations, a Fortran binding.
 *
 * Every function returns 0, or nonzero with the reason in mw_coll_last_error().  Arguments are checked before the library's
 * state, so a call with bad arguments says so with or without a device; frame, box and list indices in messages count from 0.
 * The library lives on the device given to mw_coll_init: every function that touches it makes that device current for the
 * call and puts the caller's current device back before it returns.
 */
#ifndef MW_COLL_H
#define MW_COLL_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_COLL_PLAN_FIELDS 14
#define MW_COLL_MAX_VECTORS 4096
#define MW_COLL_MAX_COMPONENT 255
#define MW_COLL_MAX_BINS 4096
#define MW_COLL_MAX_HIST_LAGS 64
#define MW_COLL_MAX_FRAMES 65536
#define MW_COLL_PAIR_TILE 256
#define MW_COLL_FLUSH_TILES 2048
#define MW_COLL_SLABS 32
#define MW_COLL_LAG_BLOCK 64

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0. */
int mw_coll_init(int device);
int mw_coll_finalize(void);
int mw_coll_is_initialised(void);
const char *mw_coll_last_error(void);

/* Host pointers.  rho [nframes][nboxes][M][2]; fkt [nboxes][nlags][M][2]; gd [nboxes][nh][nbins]; qsum, q2sum [nboxes][nlags]. */
int mw_coll_compute(int nframes, int nboxes, int nwater, const double *cells, const double *pos, int nlags, int origin_every, int M,
                    const int *nvec, double r_max, int nbins, int nh, const int *hist_lags, double overlap_a, double *rho, double *fkt,
                    long long *gd, long long *qsum, long long *q2sum);
/* Device pointers on the library's device for pos and the five outputs; cells, nvec and hist_lags stay host arrays.  Work
 * queued on the device before the call is waited for, and the results are complete on return. */
int mw_coll_compute_device(int nframes, int nboxes, int nwater, const double *cells, const double *pos, int nlags, int origin_every,
                           int M, const int *nvec, double r_max, int nbins, int nh, const int *hist_lags, double overlap_a, double *rho,
                           double *fkt, long long *gd, long long *qsum, long long *q2sum);

/* The launch rules of such a call with every output asked for (overlap: nonzero if the overlap is) -- host arithmetic only, no
 * device and no mw_coll_init needed (the scratch budget is then the default one).  nmax[3]: the largest |n_a| per axis (NULL
 * with M = 0).  Writes min(nout, MW_COLL_PLAN_FIELDS) ints:
 *   [0] boxes per chunk   [1] chunks = ceil(nboxes / [0])   [2] (frame, box) units per launch of the mode pass
 *   [3] molecule segments of the mode sums   [4] molecules per segment   [5] 1: small-box geometry of the mode pass
 *   [6] the lag block of the correlation pass, MW_COLL_LAG_BLOCK   [7] the pair tile, MW_COLL_PAIR_TILE
 *   [8] tiles of a box in the pair pass = ceil(nwater / [7]), 1 in the one-wavefront geometry
 *   [9] 1: one-wavefront geometry of the pair pass (nwater <= 64)   [10] slabs of origins = min(o_0, MW_COLL_SLABS)
 *   [11] origins per slab = ceil(o_0 / [10])   [12] LDS of a workgroup, bytes (the largest of the kernels)
 *   [13] scratch per box, bytes (the shared tables of the mode pass not counted) */
int mw_coll_plan(int nframes, int nwater, int nlags, int origin_every, int M, const int nmax[3], int nbins, int nh, int overlap,
                 int nboxes, int *out, int nout);
/* The same fields for the last call that launched. */
int mw_coll_last(int *out, int nout);
/* Event timers of the last call, summed over its chunks: the mode pass, the correlation pass, the pair pass (the distinct
 * van Hove histograms) and the overlap passes. */
int mw_coll_elapsed_ms(float *modes, float *correlate, float *pairs, float *overlap);

#ifdef __cplusplus
}
#endif
#endif
