/* mw_hess.h -- C ABI of libmw_hess.so: the second derivatives of the full-box mW energy.  For every one of many periodic
 * boxes, on a gfx950 device: products of the Hessian H = d2E / dr dr with given vectors (mw_hess_matvec) and the dense
 * Gamma-point Hessian (mw_hess_dense), each with the energy and the largest force component of the box beside it, from
 * which a caller reads whether the box is at a minimum.
 *
 * A library of its own beside libmw_hip.so (include/mw_energy.h) and the other device libraries: it needs cells and positions
 * only, so it takes plain arrays and works on any configuration, with or without mw_init in the same process.  It has its
 * own stream, scratch memory and event timers.  The positions of include/mw_quench.h's minima go straight into it.
 *
 * Inputs.  `cells` holds 9 doubles per box in the layout of mw_set_cell (cells[9 b + 3 k + a] = component a of h_(k+1)),
 * `pos` holds nwater positions in bohr as [box][nwater][3], wrapped or not.  Energies are in Hartree, forces in Hartree / bohr,
 * the Hessian in Hartree / bohr^2.
 *
 * Energy.  The one of include/mw_quench.h: with the entries of molecule i all pairs (j, n), n an integer lattice
 * translation, d = r_j + H n - r_i and |d|^2 < (a sigma)^2,
 *   E = sum_i [ 1/2 sum_k phi(r_k) + lambda eps T_i ],   T_i = 1/2 sum_{k != l} g_k g_l (u_k . u_l - cos0)^2.
 * Two images of the same j can both be entries of i.
 *
 * Second derivatives through the moments.  With f(d) = g(r) (1, u, u (x) u), the moments of a centre are
 * M = sum_k f(d_k) and T = 1/2 M^T W M - 1/2 (1 - cos0)^2 sum_k g_k^2 with the constant diagonal W = (cos0^2, -2 cos0, 1), so
 * for two entries k != l of a centre d2E_i / dd_k dd_l = lambda eps J_k^T W J_l, J = df / dd, and
 *   d2E_i / dd_k dd_k = lambda eps J_k^T W J_k + K_k,   K_k = dd [ 1/2 phi - 1/2 lambda eps (1 - cos0)^2 g^2 + lambda eps (W M) . f ] / dd dd.
 * A product H v is a perturbed moment pass, dM_i = sum_k J_k (v_jk - v_i), and one force-like pass over the moments and the
 * perturbed moments of a molecule and of its entries; (H v)_i is one lane's sum in the order of its walk.
 *
 * Supported range.  w_k = volume / |h_l x h_m| are the perpendicular widths of the cell.  Supported:
 * a sigma (1 + 1e-9) <= min_k w_k for every box of the call (so a molecule's own image is never an entry);
 * 1 <= nwater <= 2^22 (mw_hess_dense: <= MW_HESS_MAX_DENSE_WATER); 1 <= nboxes <= 2^24; 1 <= nvec <= MW_HESS_MAX_VEC.  Anything
 * else (a NaN or inf in the cells, and through host pointers in pos or vecs, included) is rejected with a message that names
 * the entry, the argument and the first offending box, and nothing is launched or written.  Positions and vectors behind
 * device pointers are not looked at: a molecule whose position is not finite there has no entries and is nobody's entry, and a
 * vector element that is not finite comes out as NaN in the products of its own box and vector alone.
 *
 * Arithmetic (part of the contract).  H^-1 is formed once per box on the host; s = H^-1 x is reduced to [0, 1) once per
 * molecule and d = H (ds + n) from the difference of fractional coordinates plus the integer image shift; everything is
 * spelled out in fma / mul / add with contraction off.  One geometry serves every nwater: the counting sort into the
 * fractional cell grid of a sigma (the grid rules of include/mw_tet.h) and a walk over the 27 cells around a molecule's own,
 * z outermost, the members of a cell in index order.  Every sum of a molecule runs in the order of that walk; E and the
 * largest |F| run over the lanes of a wavefront through one DPP tree, the wavefronts of a workgroup in order, the
 * workgroups of a box in order.  There is no floating-point atomic.  Hence the bytes of out[b][v] depend on the cell and the
 * positions of box b and on that vector alone, and the bytes of hess[b] and ef[b] on the cell and the positions alone: not on
 * the other boxes or vectors of the call, on batch versus single calls, on host versus device pointers, on chunking or on
 * how the vectors are grouped.
 *
 * Dense matrix.  hess[b] is [3 nwater][3 nwater], row 3 i + a, column 3 j + b, every element written (zeros included), the
 * blocks of all images of j summed into column j.  A centre c with entries k, l and the block B_kl = d2E_c / dd_k dd_l adds
 * +B_kl to (j_k, j_l), -B_kl to (j_k, c) and (c, j_l) and +B_kl to (c, c).  The matrices are cleared; then a wavefront owns
 * the 3 x 3 nwater strip of a row molecule: its first lane walks the centres that touch the molecule (itself, then every
 * entry, and for each of those its entries) in the order of the walk and adds with plain loads and stores -- the first 64
 * distinct columns in a table in LDS, which the wavefront then writes out, any further column in the strip itself.
 *
 * Scratch.  The cell tables, moments, perturbed moments and sorted vectors live in scratch memory; a call is processed in
 * chunks of as many boxes as fit the budget, and the vectors of mw_hess_matvec in groups of at most MW_HESS_VEC_GROUP: 256 MiB,
 * or MW_HESS_SCRATCH_MB (MiB, read by mw_hess_init).  A box that does not fit alone is an error.  mw_hess_dense (host
 * pointers) stages the matrices of a chunk in that budget too; mw_hess_dense_device writes into the caller's array.
 *
 * Out of scope: iterative eigensolvers on the products, dispersion away from Gamma, cell and strain derivatives, a Fortran
 * binding, and any change to libmw_hip.so.
 *
 * Every function returns 0, or nonzero with the reason in mw_hess_last_error().  Arguments are checked before the library's
 * state, so a call with bad arguments says so with or without a device; box indices in messages count from 0.  The library
 * lives on the device given to mw_hess_init: every function that touches it makes that device current for the call and puts
 * the caller's current device back before it returns.
 */
#ifndef MW_HESS_H
#define MW_HESS_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_HESS_PLAN_FIELDS 8
#define MW_HESS_MAX_VEC 1024
#define MW_HESS_VEC_GROUP 32
#define MW_HESS_MAX_DENSE_WATER 8192

/* Without a HIP device: fails with "no HIP device" (there is no CPU fallback).  device < 0: device 0. */
int mw_hess_init(int device);
int mw_hess_finalize(void);
int mw_hess_is_initialised(void);
const char *mw_hess_last_error(void);

/* out[b][v] = H_b vecs[b][v]; vecs and out are [nboxes][nvec][nwater][3] doubles.  ef[nboxes][2] (may be NULL): E and the
 * largest |F| component of every box.  Host pointers. */
int mw_hess_matvec(int nboxes, int nwater, const double *cells, const double *pos, int nvec, const double *vecs, double *out,
                   double *ef);
/* Device pointers on the library's device for every array.  Work queued on the device before the call is waited for, and the
 * results are complete on return. */
int mw_hess_matvec_device(int nboxes, int nwater, const double *cells, const double *pos, int nvec, const double *vecs,
                          double *out, double *ef);

/* hess[nboxes][3 nwater][3 nwater] doubles; ef as above.  Host pointers: a box's matrix must fit the scratch budget. */
int mw_hess_dense(int nboxes, int nwater, const double *cells, const double *pos, double *hess, double *ef);
int mw_hess_dense_device(int nboxes, int nwater, const double *cells, const double *pos, double *hess, double *ef);

/* The launch rules for nboxes boxes of nwater molecules with the cell `cell` (9 doubles, host) -- host arithmetic only, no
 * device and no mw_hess_init needed (the scratch budget is then the default one).  dense = 0: mw_hess_matvec with nvec vectors;
 * dense != 0: mw_hess_dense through host pointers (nvec is not looked at).  Writes min(nout, MW_HESS_PLAN_FIELDS) ints:
 *   [0] boxes per chunk   [1] chunks = ceil(nboxes / [0])   [2] [3] [4] the cell grid g_1, g_2, g_3 of a sigma
 *   [5] LDS of a workgroup, bytes (the largest of the kernels)
 *   [6] scratch per box, bytes (with the vectors of a group, or with the staged matrix; 2^31 - 1 where it is beyond that)
 *   [7] vectors per group (0 for dense) */
int mw_hess_plan(int nwater, const double *cell, int nboxes, int nvec, int dense, int *out, int nout);
/* The same fields for the last call that launched; the grid is that of its first box. */
int mw_hess_last(int *out, int nout);
/* Event timers of the last call, summed over its chunks and groups: the sort; the moment pass with the forces behind ef;
 * the products (the vectors into sorted order, the perturbed moments, the apply pass); the dense assembly (the summed
 * Jacobians and the rows).  What a call did not run is 0. */
int mw_hess_elapsed_ms(float *sort, float *moments, float *apply, float *assemble);

#ifdef __cplusplus
}
#endif
#endif
