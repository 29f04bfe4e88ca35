/* mw_sk.h -- C ABI of libmw_sk.so: the static structure factor S(k) of many periodic boxes on a gfx950 device.
 *
 * A library of its own beside libmw_hip.so (include/mw_energy.h): S(k) needs positions and cells only -- no neighbour
 * list, no image vectors, no engine state -- so it takes plain arrays and works on any configuration, with or without
 * mw_init in the same process.  It has its own stream, scratch memory and event timers.
 *
 * Definition.  Box b has the cell H with columns h1, h2, h3: `cells` holds 9 doubles per box in the layout of mw_set_cell
 * (cells[9 b + 3 k + a] = component a of h_(k+1)), and `pos` holds nwater positions r_j in bohr as [box][nwater][3], as
 * mw_download_positions_range writes them; wrapped or not makes no difference.  For an integer triple n = (n1, n2, n3)
 *
 *     k_n = 2 pi H^-T n,   s_j = H^-1 r_j,   rho_b(n) = sum_j exp(-2 pi i n . s_j),   S_b(n) = |rho_b(n)|^2 / nwater.
 *
 * One call takes M triples nvec[M][3], shared by all boxes of the call: 1 <= M <= 2^20, |n_a| <= 255.  n = 0 is allowed
 * (rho = nwater exactly); duplicates and both signs are the caller's business; there is no binning by |k| on the device.
 * Outputs: rho[nboxes][M][2] (re, im) and S[nboxes][M], doubles; either may be NULL.
 *
 * Arithmetic (part of the contract).  H^-1 is formed once per box (cofactors and determinant by fma chains, one division
 * per element); s_j once per molecule by an fma chain, reduced by s - rint(s); the per-axis phasors
 * E_a(m) = exp(2 pi i m s_a), m = 0 .. max |n_a|, each by one sincospi(2 m s_a), never by a recurrence; a negative
 * component takes the conjugate of the same entry; molecule j contributes conj((E_1 E_2) E_3).  The molecules are summed
 * in segments of 1024 * ceil(nwater / 8192) consecutive molecules, each sequentially, and the segments' sums are added in
 * segment order: no floating-point atomics.  Hence rho(-n) is bit for bit the conjugate of rho(n), S(-n) == S(n), and the bits of
 * rho_b(n) depend on the box's cell, its positions and n alone -- not on M, on the place of n in the list, on the other
 * boxes of the call, or on how the call is cut into chunks.
 *
 * Scratch.  The phasor tables (nwater * sum_a (nmax_a + 1) * 16 bytes per box) and the segments' partial sums
 * (segments * M * 16 bytes per box) live in scratch memory; a call is processed in chunks of as many boxes as fit the
 * budget: 256 MiB, or MW_SK_SCRATCH_MB (MiB, read by mw_sk_init).  A box that does not fit alone is an error.  Boxes of at
 * most 64 molecules whose tables fit one workgroup's LDS make their tables inside the sum kernel (no table scratch).
 *
 * Every function returns 0, or nonzero with the reason in mw_sk_last_error().  A rejected call launches nothing and
 * writes nothing; its message names the argument, and box / vector indices in messages count from 0.  Arguments are
 * checked before the library's state, so a call with bad arguments says so with or without a device.  The library lives on
 * the device given to mw_sk_init: every function that touches it makes that device current for the call and puts the
 * caller's current device back before it returns.
 */
#ifndef MW_SK_H
#define MW_SK_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_SK_MAX_VECTORS   (1 << 20)
#define MW_SK_MAX_COMPONENT 255
#define MW_SK_PLAN_FIELDS   9

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0.  A failed init
 * gives back the stream and events it made and leaves the library not initialised. */
int mw_sk_init(int device);
int mw_sk_finalize(void);
int mw_sk_is_initialised(void);
const char *mw_sk_last_error(void);

/* Host pointers. */
int mw_sk_compute(int nboxes, int nwater, const double *cells, const double *pos, int M, const int *nvec,
                  double *rho, double *S);
/* Device pointers on the library's device for every array.  Work queued on the device before the call is waited for,
 * and the results are complete on return. */
int mw_sk_compute_device(int nboxes, int nwater, const double *cells, const double *pos, int M, const int *nvec,
                         double *rho, double *S);
/* Host pointers.  Box w * ngroups + g is walker w's box of group g (nboxes % ngroups == 0, W = nboxes / ngroups):
 * S_mean[g][m] = (S[0 * ngroups + g][m] + S[1 * ngroups + g][m] + ...) / W, added in walker order starting from 0.0,
 * one division at the end.  The per-box results stay on the device. */
int mw_sk_mean(int nboxes, int nwater, const double *cells, const double *pos, int M, const int *nvec, int ngroups,
               double *S_mean);

/* The launch rules for boxes of nwater molecules, largest components nmax[3], M vectors and nboxes boxes -- host
 * arithmetic only, no device and no mw_sk_init needed (the scratch budget is then the default one).  Writes
 * min(nout, MW_SK_PLAN_FIELDS) ints:
 *   [0] boxes per chunk   [1] chunks = ceil(nboxes / [0])   [2] k-vectors per lane   [3] molecule segments
 *   [4] dynamic LDS of the sum kernel, bytes   [5] 1: small-box geometry (tables made in the sum kernel)
 *   [6] molecules per LDS tile   [7] molecules per segment   [8] k-vectors per workgroup */
int mw_sk_plan(int nwater, const int nmax[3], int M, int nboxes, int *out, int nout);
/* The same fields for the last call that launched. */
int mw_sk_last(int *out, int nout);
/* Event timers of the last call, summed over its chunks: the table pass (0 with the small-box geometry) and the sums. */
int mw_sk_elapsed_ms(float *phasors, float *sums);

#ifdef __cplusplus
}
#endif
#endif
