/* mw_tcf.h -- C ABI of libmw_tcf.so: time correlation functions of trajectories.  For every one of many boxes, from frames
 * equally spaced in time: the mean squared displacement, the mean quartic displacement (for the non-Gaussian parameter),
 * the velocity autocorrelation function, the self-intermediate scattering function F_s(q, t) and integer histograms of the
 * squared displacement (the self part of the van Hove function), each averaged over every time origin and every molecule,
 * on a gfx950 device.
 *
 * A library of its own beside libmw_hip.so (include/mw_energy.h) and the other device libraries: it takes plain arrays of
 * unwrapped positions (and velocities), needs no cell and no neighbour, and has its own stream, scratch memory and event
 * timers.  Frames of any origin are accepted as they are: chained molecular-dynamics calls at fixed or at moving cell
 * produce them.  There is no CPU path.
 *
 * Inputs.  `pos` [nframes][nboxes][nwater][3] doubles, unwrapped, frame-major; `vel` of the same shape or NULL (then `vacf`
 * must be NULL).  Lags l = 0 .. nlags - 1 (in frames), 1 <= nlags <= nframes.  origin_every = s >= 1: the origins are
 * t0 = 0, s, 2 s, ... with t0 + l <= nframes - 1, so lag l has o_l = (nframes - 1 - l) / s + 1 origins (integer division).
 * `q` [nq] wave numbers (inverse bohr), each > 0 and finite, 0 <= nq <= MW_TCF_MAX_Q.  `edges2` [nedges] ascending edges in
 * bohr^2 (squared distances), nedges = 0 or 2 <= nedges <= MW_TCF_MAX_EDGES; `hist_lags` [nh] lags in [0, nlags),
 * 0 <= nh <= MW_TCF_MAX_HIST_LAGS.  q, edges2 and hist_lags are host arrays in both compute entries.  `flags`: bit 0 is
 * MW_TCF_REMOVE_COM; any other bit is rejected.
 *
 * Supported range.  1 <= nframes <= 2^20; 1 <= nwater <= 2^22; 1 <= nboxes <= 2^24; ceil(nwater / MW_TCF_TILE) x
 * ceil(nlags / MW_TCF_LAG_BLOCK) < 2^31; every position and velocity finite.  `fs` without q (nq = 0), `hist` without edges or
 * without hist_lags, `vacf` without `vel`, edges that are not finite or not strictly ascending, a q that is not finite or not
 * > 0, a hist_lag outside [0, nlags): all rejected, with a message that names the entry, the argument and the first
 * offending frame and box (or index), and nothing is launched or written.  (The device-pointer entry looks at its positions
 * and velocities with one kernel before the run and reads its verdict; that kernel writes nothing but the verdict.)
 *
 * Definitions, for box b and lag l, with n_l = o_l x nwater terms:
 *   y_j(t) = x_j(t), or x_j(t) - c(t) under MW_TCF_REMOVE_COM, c(t) = (sum_j x_j(t)) / nwater per component (one rounding
 *     for the difference).  Velocities likewise, with the box's mean velocity removed.
 *   D = y_j(t0 + l) - y_j(t0) per component;  d2 = fma(Dx, Dx, fma(Dy, Dy, Dz Dz)).
 *   msd[b][l]   = (sum d2) / n_l
 *   mqd[b][l]   = (sum d2^2) / n_l, accumulated as acc = fma(d2, d2, acc)
 *   vacf[b][l]  = (sum fma(vx, vx', fma(vy, vy', vz vz'))) / n_l with v = v_j(t0), v' = v_j(t0 + l)
 *   fs[b][l][a] = (sum sinc(q_a sqrt(d2))) / n_l, sinc(0) = 1, otherwise sin(x) / x with the device library's double sin:
 *     the exact isotropic average of exp(i q . D), so no list of wave vectors is needed
 *   hist[b][h][nedges + 1] 64-bit counts of d2 at lag hist_lags[h]: [0] d2 < edges2[0]; [1 + k] edges2[k] <= d2 <
 *     edges2[k + 1]; [nedges] d2 >= edges2[nedges - 1].  A row adds up to n_l exactly.
 * Any output may be NULL, and the work for a NULL output is not done.
 *
 * Arithmetic (part of the contract).  Contraction is off; everything is spelled out in fma / mul / add / sqrt / div.
 *   Centre: one wavefront per (frame, box); lane L adds the molecules L, L + 64, ... ascending onto 0, then the lanes are
 *     combined by s = s + s(lane xor m) for m = 32, 16, 8, 4, 2, 1, and the sum is divided by nwater once.
 *   Sums: molecules are cut into tiles of MW_TCF_TILE consecutive ones.  The partial sum of (tile, lag) starts at 0 and takes
 *     its terms origins ascending, molecules ascending within an origin.  A second kernel adds the tiles' partial sums
 *     onto 0 in tile order and divides by n_l (as a double) once.  No floating-point atomics anywhere.
 *   Histograms: 32-bit counters in LDS, flushed with 64-bit integer atomics; integers do not depend on the order.
 * Hence the bytes of a box's results depend on that box's frames and the call's scalars and lists alone: not on the other
 * boxes of the call, on batch versus single calls, on host versus device pointers, on chunking or on the scratch budget.
 * In particular msd[b][0] = 0 and fs[b][0][a] = 1 exactly.
 *
 * Mechanism.  The correlation kernel: a workgroup of MW_TCF_LAG_BLOCK lanes takes (box, tile, block of MW_TCF_LAG_BLOCK
 * lags), lane = lag.  Per chunk of MW_TCF_ORIGIN_CHUNK consecutive frames that holds an origin it stages the chunk's frames
 * and the window of MW_TCF_LAG_BLOCK + MW_TCF_ORIGIN_CHUNK - 1 target frames of its tile in LDS as [molecule][component]
 * [frame] -- lanes at consecutive lags read consecutive doubles, the origin's coordinate is a broadcast --, centred while
 * they are loaded; the sums live in registers.  Positions and velocities take turns in the same LDS.  The histograms are a
 * kernel of their own, one workgroup per (box, selected lag, slab of terms), straight from memory.  A call is processed in
 * chunks of as many boxes as fit the scratch budget (MW_TCF_SCRATCH_MB, MiB, read by mw_tcf_init, default 256: the tiles'
 * partial sums and the centres); a box that does not fit alone is an error.  The host-pointer entry stages the whole
 * trajectory on the device, outside that budget.
 *
 * Out of scope: collective F(k, t) and the distinct van Hove function (libmw_coll.so has them: include/mw_coll.h),
 * per-molecule mobilities, multiple-tau schemes, stress correlations, a Fortran binding.
 *
 * Every function returns 0, or nonzero with the reason in mw_tcf_last_error().  Arguments are checked before the library's
 * state, so a call with bad arguments says so with or without a device; frame, box and list indices in messages count from 0.
 * The library lives on the device given to mw_tcf_init: every function that touches it makes that device current for the
 * call and puts the caller's current device back before it returns.
 */
#ifndef MW_TCF_H
#define MW_TCF_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_TCF_PLAN_FIELDS 10
#define MW_TCF_TILE 8
#define MW_TCF_LAG_BLOCK 128
#define MW_TCF_ORIGIN_CHUNK 32
#define MW_TCF_MAX_Q 16
#define MW_TCF_MAX_EDGES 1025
#define MW_TCF_MAX_HIST_LAGS 64
#define MW_TCF_MAX_FRAMES 1048576
#define MW_TCF_REMOVE_COM 1u

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0. */
int mw_tcf_init(int device);
int mw_tcf_finalize(void);
int mw_tcf_is_initialised(void);
const char *mw_tcf_last_error(void);

/* Host pointers.  msd, mqd, vacf [nboxes][nlags]; fs [nboxes][nlags][nq]; hist [nboxes][nh][nedges + 1]. */
int mw_tcf_compute(int nframes, int nboxes, int nwater, const double *pos, const double *vel, int nlags, int origin_every, int nq,
                   const double *q, int nedges, const double *edges2, int nh, const int *hist_lags, unsigned flags, double *msd,
                   double *mqd, double *vacf, double *fs, long long *hist);
/* Device pointers on the library's device for pos, vel and the five outputs; q, edges2 and hist_lags stay host arrays.  Work
 * queued on the device before the call is waited for, and the results are complete on return. */
int mw_tcf_compute_device(int nframes, int nboxes, int nwater, const double *pos, const double *vel, int nlags, int origin_every,
                          int nq, const double *q, int nedges, const double *edges2, int nh, const int *hist_lags, unsigned flags,
                          double *msd, double *mqd, double *vacf, double *fs, long long *hist);

/* The launch rules of such a call -- host arithmetic only, no device and no mw_tcf_init needed (the scratch budget is then
 * the default one).  Writes min(nout, MW_TCF_PLAN_FIELDS) ints:
 *   [0] boxes per chunk   [1] chunks = ceil(nboxes / [0])   [2] the tile, MW_TCF_TILE   [3] the lag block, MW_TCF_LAG_BLOCK
 *   [4] the origin chunk, MW_TCF_ORIGIN_CHUNK   [5] the frame window = [3] + [4] - 1 target frames staged at a time
 *   [6] LDS of a workgroup, bytes (the largest of the kernels)   [7] scratch per box, bytes
 *   [8] tiles per box = ceil(nwater / [2])   [9] lag blocks = ceil(nlags / [3]) */
int mw_tcf_plan(int nframes, int nwater, int nlags, int nq, int nedges, unsigned flags, int nboxes, int *out, int nout);
/* The same fields for the last call that launched. */
int mw_tcf_last(int *out, int nout);
/* Event timers of the last call, summed over its chunks: the centring pass (0 without MW_TCF_REMOVE_COM), the correlation
 * pass (with the histograms) and the reduction of the tiles' partial sums. */
int mw_tcf_elapsed_ms(float *centre, float *correlate, float *reduce);

#ifdef __cplusplus
}
#endif
#endif
