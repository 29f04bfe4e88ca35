// libmw_coll.so -- the collective time correlations of include/mw_coll.h: the density modes rho(n, t) of every frame of a
// frame-major trajectory, the coherent intermediate scattering function F(n, t), the histograms of the distinct van Hove
// function G_d(r, t) and the sums of the overlap Q and of Q^2 over the time origins.  k_coll_check is the verdict-only look at
// device arrays; k_coll_phasors, k_coll_sum and k_coll_finish are the mode pass (mw_sk.h's arithmetic restated, run on
// (frame, box) units, with rho also kept transposed in scratch); k_coll_corr -- one lane per (box, vector, lag), origins
// sequential -- forms F; k_coll_pairs (a workgroup per box, selected lag, slab of origins and tile of i) and k_coll_pairs_small
// (a wavefront per box, selected lag and slab; boxes of at most 64 molecules) count the pair distances across two frames in
// 32-bit LDS counters flushed with 64-bit integer atomics; k_coll_overlap counts Q of every (origin, lag) into an integer
// scratch and k_coll_overlap_sum adds Q and Q^2.  No floating-point atomic anywhere: every sum has the order the header states.
#include "../../include/mw_coll.h"

#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too

namespace mwcoll {

constexpr int kThreads = 256;
constexpr int kVecPerLane = 2;
constexpr int kVecPerWg = kThreads * kVecPerLane;
constexpr int kSegment = 1024;                 // molecules per partial sum of a mode, times ceil(N / 8192) (mw_sk.h's rule)
constexpr int kSmallN = 64;
constexpr int kLdsCap = 64 * 1024;             // dynamic LDS a workgroup may ask for
constexpr int kMaxTile = 32;
constexpr int kMaxWater = 1 << 22;
constexpr int kMaxBoxes = 1 << 24;
constexpr int kMaxFrames = MW_COLL_MAX_FRAMES;
constexpr int kMaxChunkBoxes = 65535;          // a chunk's boxes are a grid dimension
constexpr int kMaxUnits = 65535;               // and so are the (frame, box) units of a launch of the mode pass
constexpr int kLagBlock = MW_COLL_LAG_BLOCK;   // = the threads of k_coll_corr
constexpr int kPairTile = MW_COLL_PAIR_TILE;   // = the threads of k_coll_pairs
constexpr int kFlushTiles = MW_COLL_FLUSH_TILES;
static_assert((unsigned long long)kFlushTiles * kPairTile * kPairTile * 27 < (1ULL << 32), "the 32-bit counters of k_coll_pairs");
constexpr int kSlabs = MW_COLL_SLABS;
static_assert((unsigned long long)((kMaxFrames + kSlabs - 1) / kSlabs) * 64 * 64 * 27 < (1ULL << 32), "the 32-bit counters of k_coll_pairs_small");
constexpr int kSmallWaves = 4;                 // wavefronts of a workgroup of k_coll_pairs_small, while their LDS fits kLdsCap
constexpr int kOverlapTile = 64;               // = the threads of k_coll_overlap
constexpr unsigned long long kNoVerdict = ~0ULL;

__host__ __device__ constexpr size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// What the pair pass knows of a box: the cell, the rows of its inverse and the image range per axis (the header's arithmetic).
struct PairCell {
    double h[9];                               // h[3 k + a]: component a of cell vector k
    double g[9];                               // g[3 k + a]: component a of row k of the inverse, s_k = g_k . r
    int m[3];                                  // n_k in -m[k] .. m[k]
    int images;
};

// ---- the verdict-only check of device arrays: the smallest index of an element that is not finite -------------------------
__global__ __launch_bounds__(256) void k_coll_check(size_t count, const double* __restrict__ a, unsigned long long* __restrict__ verdict)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const double v = a[i];
        if (!(v - v == 0.0)) atomicMin(verdict, (unsigned long long)i);
    }
}

// ---- the mode pass ------------------------------------------------------------------------------------------------------------
// A unit is one (frame, box of the chunk): unit u0 + u of the chunk is frame (u0 + u) / nb, box (u0 + u) % nb.  `pos` is the
// trajectory from the chunk's first box on, [frame][nbs boxes][n][3]; `inv` the chunk's inverse cells.  A chunk has up to
// 65535 x 65536 units, so u0 is 64 bits wide.
__device__ __forceinline__ const double* unit_positions(const double* __restrict__ pos, long long gu, int nb, int nbs, int n, int& bl)
{
    const int f = (int)(gu / nb);
    bl = (int)(gu - (long long)f * nb);
    return pos + ((size_t)f * nbs + bl) * n * 3;
}

// s_a = (H^-1 r)_a reduced to [-1/2, 1/2]; I = H^-1, row-major
__device__ __forceinline__ double frac_coord(const double* __restrict__ I, int a, double x, double y, double z)
{
    const double s = __builtin_fma(I[3 * a], x, __builtin_fma(I[3 * a + 1], y, I[3 * a + 2] * z));
    return s - __builtin_rint(s);
}

// E(m) = exp(2 pi i m s) as (cos, sin)
__device__ __forceinline__ double2 phasor(double s, int m)
{
    double sn, cs;
    sincospi((2.0 * (double)m) * s, &sn, &cs);
    return make_double2(cs, sn);
}

__device__ __forceinline__ double flip(double v, int signbit) { return __hiloint2double(__double2hiint(v) ^ signbit, __double2loint(v)); }

// One lane per (unit, molecule): s_j and the three tables, T[unit][row][j] with row = (axis, m), j fastest.
__global__ __launch_bounds__(kThreads) void k_coll_phasors(int nu, long long u0, int nb, int nbs, int n, int nmax0, int nmax1, int nmax2,
                                                           const double* __restrict__ inv, const double* __restrict__ pos, double2* __restrict__ T)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)nu * n) return;
    const int u = (int)(t / n), j = (int)(t - (long long)u * n);
    int bl;
    const double* r = unit_positions(pos, u0 + u, nb, nbs, n, bl) + 3 * (size_t)j;
    const double* I = inv + 9 * (size_t)bl;
    const double x = r[0], y = r[1], z = r[2];
    const int rows = nmax0 + nmax1 + nmax2 + 3;
    double2* out = T + (size_t)u * rows * n + j;
    const int nmax[3] = {nmax0, nmax1, nmax2};
    int row = 0;
    for (int a = 0; a < 3; ++a) {
        const double s = frac_coord(I, a, x, y, z);
        for (int m = 0; m <= nmax[a]; ++m, ++row) out[(size_t)row * n] = phasor(s, m);
    }
}

// Workgroup (k-tile, segment, unit): lane l owns vectors tile * kVecPerWg + l + q * kThreads, q < kVecPerLane, and adds the
// molecules of its segment one after the other.  LDS tile[row][jj], row stride `stride` 16-byte slots (odd).  FUSED: the box
// has <= 64 molecules and the tile, the whole box, is computed here instead of copied from T.
template <bool FUSED>
__global__ __launch_bounds__(kThreads) void k_coll_sum(long long u0, int nb, int nbs, int n, int M, int nmax0, int nmax1, int nmax2, int jtlog, int stride,
                                                       int seglen, const int* __restrict__ nvec, const double2* __restrict__ T,
                                                       const double* __restrict__ inv, const double* __restrict__ pos, double2* __restrict__ part)
{
    extern __shared__ double2 tile[];
    const int tid = threadIdx.x, seg = blockIdx.y, u = blockIdx.z, nseg = gridDim.y;
    const int off1 = nmax0 + 1, off2 = off1 + nmax1 + 1, rows = off2 + nmax2 + 1;
    int a0[kVecPerLane], a1[kVecPerLane], a2[kVecPerLane], f0[kVecPerLane], f1[kVecPerLane], f2[kVecPerLane];
    double re[kVecPerLane], im[kVecPerLane];
#pragma unroll
    for (int q = 0; q < kVecPerLane; ++q) {
        const int v = blockIdx.x * kVecPerWg + q * kThreads + tid;
        int c0 = 0, c1 = 0, c2 = 0;
        if (v < M) { c0 = nvec[3 * (size_t)v]; c1 = nvec[3 * (size_t)v + 1]; c2 = nvec[3 * (size_t)v + 2]; }
        a0[q] = abs(c0) * stride;           f0[q] = c0 < 0 ? (int)0x80000000 : 0;
        a1[q] = (off1 + abs(c1)) * stride;  f1[q] = c1 < 0 ? (int)0x80000000 : 0;
        a2[q] = (off2 + abs(c2)) * stride;  f2[q] = c2 < 0 ? (int)0x80000000 : 0;
        re[q] = 0.0; im[q] = 0.0;
    }
    const int jbeg = seg * seglen, jend = min(n, jbeg + seglen);
    const int jt = FUSED ? n : (1 << jtlog);
    const double2* Tu = FUSED ? nullptr : T + (size_t)u * rows * n;
    for (int j0 = jbeg; j0 < jend; j0 += jt) {
        const int cnt = min(jt, jend - j0);
        if constexpr (FUSED) {
            int bl;
            const double* r = unit_positions(pos, u0 + u, nb, nbs, n, bl);
            const double* I = inv + 9 * (size_t)bl;
            for (int idx = tid; idx < rows * n; idx += kThreads) {
                const int row = idx / n, jj = idx - row * n;
                const int a = (row >= off1) + (row >= off2);
                const int m = row - (a == 0 ? 0 : a == 1 ? off1 : off2);
                const double s = frac_coord(I, a, r[3 * jj], r[3 * jj + 1], r[3 * jj + 2]);
                tile[row * stride + jj] = phasor(s, m);
            }
        } else {
            for (int idx = tid; idx < (rows << jtlog); idx += kThreads) {
                const int row = idx >> jtlog, jj = idx & (jt - 1);
                if (jj < cnt) tile[row * stride + jj] = Tu[(size_t)row * n + j0 + jj];
            }
        }
        __syncthreads();
        for (int jj = 0; jj < cnt; ++jj) {
#pragma unroll
            for (int q = 0; q < kVecPerLane; ++q) {
                const double2 e0 = tile[a0[q] + jj], e1 = tile[a1[q] + jj], e2 = tile[a2[q] + jj];
                const double y0 = flip(e0.y, f0[q]), y1 = flip(e1.y, f1[q]), y2 = flip(e2.y, f2[q]);
                const double pr = __builtin_fma(e0.x, e1.x, -(y0 * y1));
                const double pi = __builtin_fma(e0.x, y1, y0 * e1.x);
                const double qr = __builtin_fma(pr, e2.x, -(pi * y2));
                const double qi = __builtin_fma(pr, y2, pi * e2.x);
                re[q] = re[q] + qr;
                im[q] = im[q] - qi;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < kVecPerLane; ++q) {
        const int v = blockIdx.x * kVecPerWg + q * kThreads + tid;
        if (v < M) part[((size_t)u * nseg + seg) * M + v] = make_double2(re[q], im[q]);
    }
}

// One lane per (unit, vector): the segments' sums in segment order; rho in the caller's layout [frame][nbs boxes][M][2] (from
// the chunk's first box on) and transposed, rhoT[box of the chunk][M][re | im][frame].
__global__ __launch_bounds__(kThreads) void k_coll_finish(int nu, long long u0, int nb, int nbs, int M, int nseg, int nframes,
                                                          const double2* __restrict__ part, double* __restrict__ rho, double* __restrict__ rhoT)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)nu * M) return;
    const int u = (int)(t / M), v = (int)(t - (long long)u * M);
    const long long gu = u0 + u;
    const int f = (int)(gu / nb), bl = (int)(gu - (long long)f * nb);
    const double2* p = part + (size_t)u * nseg * M + v;
    double re = p[0].x, im = p[0].y;
    for (int s = 1; s < nseg; ++s) { const double2 w = p[(size_t)s * M]; re = re + w.x; im = im + w.y; }
    if (rho) {
        double* o = rho + (((size_t)f * nbs + bl) * M + v) * 2;
        o[0] = re; o[1] = im;
    }
    if (rhoT) {
        double* o = rhoT + (((size_t)bl * M + v) * 2) * nframes + f;
        o[0] = re; o[(size_t)nframes] = im;
    }
}

// ---- the correlation pass: workgroup (lag block, vector; box of the chunk), lane = lag, origins ascending ----------------------
__global__ __launch_bounds__(kLagBlock) void k_coll_corr(int n, int M, int nframes, int nlags, int every, const double* __restrict__ rhoT,
                                                         double* __restrict__ fkt)
{
    const int v = blockIdx.x % M, lb = blockIdx.x / M, b = blockIdx.y;
    const int L0 = lb * kLagBlock, lag = L0 + threadIdx.x, last = nframes - 1;
    const double* R = rhoT + (((size_t)b * M + v) * 2) * nframes;
    const double* Q = R + nframes;
    double re = 0.0, im = 0.0;
    for (int t0 = 0; t0 + L0 <= last; t0 += every) {
        if (lag < nlags && t0 + lag <= last) {
            const double Are = R[t0 + lag], Aim = Q[t0 + lag], Bre = R[t0], Bim = Q[t0];
            re = __builtin_fma(Are, Bre, __builtin_fma(Aim, Bim, re));
            im = __builtin_fma(Aim, Bre, __builtin_fma(-Are, Bim, im));
        }
    }
    if (lag < nlags) {
        const double nl = (double)((last - lag) / every + 1) * (double)n;
        double* o = fkt + (((size_t)b * nlags + lag) * M + v) * 2;
        o[0] = re / nl; o[1] = im / nl;
    }
}

// ---- the pair pass ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pair_frac(const PairCell& c, const double* __restrict__ p, double& sx, double& sy, double& sz)
{
    const double x = p[0], y = p[1], z = p[2];
    sx = __builtin_fma(c.g[0], x, __builtin_fma(c.g[1], y, c.g[2] * z));
    sy = __builtin_fma(c.g[3], x, __builtin_fma(c.g[4], y, c.g[5] * z));
    sz = __builtin_fma(c.g[6], x, __builtin_fma(c.g[7], y, c.g[8] * z));
}

// One pair: every image of j (at t0 + l) around i (at t0); `self`: j = i, whose n = 0 term is no pair.
__device__ __forceinline__ void pair_images(const PairCell& c, double six, double siy, double siz, double sjx, double sjy, double sjz, bool self,
                                            double rmax2, double scale, int nbins, unsigned* hist)
{
    double ax = sjx - six, ay = sjy - siy, az = sjz - siz;
    ax -= __builtin_rint(ax); ay -= __builtin_rint(ay); az -= __builtin_rint(az);
    const double d0x = __builtin_fma(c.h[0], ax, __builtin_fma(c.h[3], ay, c.h[6] * az));
    const double d0y = __builtin_fma(c.h[1], ax, __builtin_fma(c.h[4], ay, c.h[7] * az));
    const double d0z = __builtin_fma(c.h[2], ax, __builtin_fma(c.h[5], ay, c.h[8] * az));
    for (int n1 = -c.m[0]; n1 <= c.m[0]; ++n1) {
        const double f1 = (double)n1;
        const double t1x = __builtin_fma(f1, c.h[0], d0x), t1y = __builtin_fma(f1, c.h[1], d0y), t1z = __builtin_fma(f1, c.h[2], d0z);
        for (int n2 = -c.m[1]; n2 <= c.m[1]; ++n2) {
            const double f2 = (double)n2;
            const double t2x = __builtin_fma(f2, c.h[3], t1x), t2y = __builtin_fma(f2, c.h[4], t1y), t2z = __builtin_fma(f2, c.h[5], t1z);
            for (int n3 = -c.m[2]; n3 <= c.m[2]; ++n3) {
                const double f3 = (double)n3;
                const double dx = __builtin_fma(f3, c.h[6], t2x), dy = __builtin_fma(f3, c.h[7], t2y), dz = __builtin_fma(f3, c.h[8], t2z);
                const double r2 = __builtin_fma(dx, dx, __builtin_fma(dy, dy, dz * dz));
                const bool none = self && (n1 | n2 | n3) == 0;
                if (r2 < rmax2 && !none) {
                    const double d = __builtin_sqrt(r2);
                    int b = (int)(d * scale);                              // floor: d * scale >= 0
                    b = b < nbins ? b : nbins - 1;                        // (d within an ulp of r_max)
                    atomicAdd(&hist[b], 1u);
                }
            }
        }
    }
}

// the origins of a lag that are not beyond the trajectory (the host has rejected lags outside [0, nlags))
__device__ __forceinline__ int origins_of(int nframes, int lag, int every) { return lag >= 0 && lag < nframes ? (nframes - 1 - lag) / every + 1 : 0; }

// Boxes of more than 64 molecules.  Workgroup (slab of origins x tile I of i; selected lag; box of the chunk): s_i(t0) in
// registers, one molecule per lane, every tile of s_j(t0 + l) through LDS.  `pos` and `out` start at the chunk's first box.
__global__ __launch_bounds__(kPairTile) void k_coll_pairs(int nframes, int nbs, int n, int every, int nbins, double r_max, int nh, int T, int ops,
                                                          const PairCell* __restrict__ cells, const int* __restrict__ hist_lags,
                                                          const double* __restrict__ pos, unsigned long long* __restrict__ out)
{
    extern __shared__ unsigned pair_hist[];                // [nbins]
    __shared__ double tsx[kPairTile], tsy[kPairTile], tsz[kPairTile];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int slab = (int)(blockIdx.x / (unsigned)T), I = (int)(blockIdx.x - (unsigned)slab * (unsigned)T);
    const int lag = hist_lags[h], ol = origins_of(nframes, lag, every);
    const PairCell c = cells[b];
    const double rmax2 = r_max * r_max, scale = (double)nbins / r_max;
    unsigned long long* H = out + ((size_t)b * nh + h) * nbins;
    for (int k = tid; k < nbins; k += kPairTile) pair_hist[k] = 0u;
    const int i = I * kPairTile + tid;
    const int oend = min(ol, (slab + 1) * ops);
    int steps = 0;
    for (int oi = slab * ops; oi < oend; ++oi) {
        const size_t t0 = (size_t)oi * every;
        const double* Pi = pos + ((t0 * nbs + b) * n) * 3;
        const double* Pj = pos + (((t0 + lag) * nbs + b) * n) * 3;
        double six = 0.0, siy = 0.0, siz = 0.0;
        if (i < n) pair_frac(c, Pi + 3 * (size_t)i, six, siy, siz);
        for (int J = 0; J < T; ++J, ++steps) {
            const int j0 = J * kPairTile, nj = min(kPairTile, n - j0);
            __syncthreads();                               // the tile before this one has been read (and the zeroing is done)
            if (steps > 0 && (steps % kFlushTiles) == 0) { // uniform: keep the 32-bit counters from overflowing
                for (int k = tid; k < nbins; k += kPairTile) {
                    const unsigned v = pair_hist[k];
                    if (v) { atomicAdd(&H[k], (unsigned long long)v); pair_hist[k] = 0u; }
                }
                __syncthreads();
            }
            if (tid < nj) {
                double x, y, z;
                pair_frac(c, Pj + 3 * (size_t)(j0 + tid), x, y, z);
                tsx[tid] = x; tsy[tid] = y; tsz[tid] = z;
            }
            __syncthreads();
            if (i < n) {
#pragma unroll 2
                for (int j = 0; j < nj; ++j) pair_images(c, six, siy, siz, tsx[j], tsy[j], tsz[j], j0 + j == i, rmax2, scale, nbins, pair_hist);
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < nbins; k += kPairTile) {
        const unsigned v = pair_hist[k];
        if (v) atomicAdd(&H[k], (unsigned long long)v);
    }
}

// Boxes of at most 64 molecules: wavefront w of workgroup x takes slab x * waves + w of (selected lag, box), with its own
// positions and histogram in LDS; every wavefront makes `ops` trips so that the barriers are met by all.
__global__ __launch_bounds__(64 * kSmallWaves) void k_coll_pairs_small(int nframes, int nbs, int n, int every, int nbins, double r_max, int nh, int nslabs,
                                                                        int ops, const PairCell* __restrict__ cells, const int* __restrict__ hist_lags,
                                                                        const double* __restrict__ pos, unsigned long long* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pair_smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, waves = blockDim.x >> 6;
    const int h = blockIdx.y, b = blockIdx.z, slab = (int)blockIdx.x * waves + wave;
    double* sx = reinterpret_cast<double*>(pair_smem) + (size_t)wave * 3 * kSmallN;
    double* sy = sx + kSmallN;
    double* sz = sy + kSmallN;
    unsigned* hist = reinterpret_cast<unsigned*>(pair_smem + (size_t)waves * 3 * kSmallN * sizeof(double)) + (size_t)wave * nbins;
    const int lag = hist_lags[h], ol = origins_of(nframes, lag, every);
    const PairCell c = cells[b];
    const double rmax2 = r_max * r_max, scale = (double)nbins / r_max;
    for (int k = lane; k < nbins; k += 64) hist[k] = 0u;
    for (int k = 0; k < ops; ++k) {
        const int oi = slab * ops + k;
        const bool mine = slab < nslabs && oi < ol && lane < n;
        double six = 0.0, siy = 0.0, siz = 0.0;
        __syncthreads();                                   // the trip before this one has read its positions
        if (mine) {
            const size_t t0 = (size_t)oi * every;
            pair_frac(c, pos + ((t0 * nbs + b) * n + lane) * 3, six, siy, siz);
            double x, y, z;
            pair_frac(c, pos + (((t0 + lag) * nbs + b) * n + lane) * 3, x, y, z);
            sx[lane] = x; sy[lane] = y; sz[lane] = z;
        }
        __syncthreads();
        if (mine)
            for (int j = 0; j < n; ++j) pair_images(c, six, siy, siz, sx[j], sy[j], sz[j], j == lane, rmax2, scale, nbins, hist);
    }
    __syncthreads();
    if (slab < nslabs) {
        unsigned long long* H = out + ((size_t)b * nh + h) * nbins;
        for (int k = lane; k < nbins; k += 64) {
            const unsigned v = hist[k];
            if (v) atomicAdd(&H[k], (unsigned long long)v);
        }
    }
}

// ---- the overlap ----------------------------------------------------------------------------------------------------------------
// Wavefront (origin x tile of 64 molecules; box of the chunk): Q of every lag the origin has, into qs[box][lag][origin index]
// (zeroed before the launch), one 32-bit integer atomic per (tile, lag) that counted any.
__global__ __launch_bounds__(kOverlapTile) void k_coll_overlap(int nframes, int nbs, int n, int nlags, int every, int o0, int tiles, double a2,
                                                               const double* __restrict__ pos, unsigned* __restrict__ qs)
{
    const int lane = threadIdx.x, b = blockIdx.y;
    const int oi = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)oi * (unsigned)tiles);
    const int j = tile * kOverlapTile + lane, last = nframes - 1;
    const size_t t0 = (size_t)oi * every;
    const bool mine = j < n;
    double x0 = 0.0, y0 = 0.0, z0 = 0.0;
    if (mine) {
        const double* p = pos + ((t0 * nbs + b) * n + j) * 3;
        x0 = p[0]; y0 = p[1]; z0 = p[2];
    }
    for (int l = 0; l < nlags && (int)t0 + l <= last; ++l) {
        bool in = false;
        if (mine) {
            const double* p = pos + (((t0 + l) * nbs + b) * n + j) * 3;
            const double dx = p[0] - x0, dy = p[1] - y0, dz = p[2] - z0;
            const double d2 = __builtin_fma(dx, dx, __builtin_fma(dy, dy, dz * dz));
            in = d2 < a2;
        }
        const unsigned cnt = (unsigned)__popcll(__ballot(in));
        if (lane == 0 && cnt) atomicAdd(qs + ((size_t)b * nlags + l) * o0 + oi, cnt);
    }
}

// One lane per (box of the chunk, lag): Q and Q^2 over the lag's origins.
__global__ __launch_bounds__(kThreads) void k_coll_overlap_sum(int nb, int nframes, int nlags, int every, int o0, const unsigned* __restrict__ qs,
                                                               long long* __restrict__ qsum, long long* __restrict__ q2sum)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)nb * nlags) return;
    const int l = (int)(t % nlags);
    const int ol = (nframes - 1 - l) / every + 1;
    const unsigned* q = qs + (size_t)t * o0;
    unsigned long long s = 0, s2 = 0;
    for (int oi = 0; oi < ol; ++oi) {
        const unsigned long long v = q[oi];
        s += v;
        s2 += v * v;
    }
    if (qsum) qsum[t] = (long long)s;
    if (q2sum) q2sum[t] = (long long)s2;
}

}  // namespace mwcoll

namespace {

using namespace mwcoll;

struct State : Runtime<5> {
    Buf scratch, verdict, inv, cells, nvec, lags, pos, rho, fkt, gd, qsum, q2sum;
    int last[MW_COLL_PLAN_FIELDS] = {0};
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
} g;

struct Plan {
    int bpc, chunks, upl;
    int small, rows, tile, jtlog, stride, nseg, seglen;     // the mode pass (mw_sk.h's launch rules)
    int ptiles, psmall, pwaves, slabs, ops, o0, otiles;
    size_t mode_lds, pair_lds, lds, unit, rhot_bytes, qs_bytes, per_box;
};

void plan_fields(const Plan& p, int* f)
{
    f[0] = p.bpc; f[1] = p.chunks; f[2] = p.upl; f[3] = p.nseg; f[4] = p.seglen; f[5] = p.small; f[6] = kLagBlock; f[7] = kPairTile;
    f[8] = p.ptiles; f[9] = p.psmall; f[10] = p.slabs; f[11] = p.ops; f[12] = (int)p.lds;
    f[13] = (int)(p.per_box > 0x7fffffffu ? 0x7fffffffu : p.per_box);
}

// The launch rules.  Scratch: per box the transposed modes [M][2][nframes] doubles and the overlap counts [nlags][o_0] 32-bit
// integers; shared by the boxes of a chunk, the mode pass's tables and partial sums of `upl` (frame, box) units at a time.
int make_plan(const char* who, int nframes, int n, int nlags, int every, int M, const int nmax[3], bool correlate, int nbins, int overlap, int nboxes,
              size_t budget, Plan& p)
{
    if (every > nframes) every = nframes;
    p.o0 = (nframes - 1) / every + 1;
    p.seglen = kSegment * ((n + 8 * kSegment - 1) / (8 * kSegment));
    if (M > 0) {
        p.rows = nmax[0] + nmax[1] + nmax[2] + 3;
        const int small_stride = n | 1;
        p.small = n <= kSmallN && (size_t)p.rows * small_stride * 16 <= (size_t)kLdsCap;
        if (p.small) {
            p.tile = n; p.jtlog = 0; p.stride = small_stride; p.nseg = 1;
        } else {
            p.tile = kMaxTile; p.jtlog = 5;
            while ((size_t)p.rows * (p.tile + 1) * 16 > (size_t)kLdsCap) { p.tile >>= 1; --p.jtlog; }
            p.stride = p.tile + 1;
            p.nseg = (n + p.seglen - 1) / p.seglen;
        }
        p.mode_lds = (size_t)p.rows * p.stride * 16;
        p.unit = (p.small ? 0 : (size_t)n * p.rows * 16) + (size_t)p.nseg * M * 16;
        p.rhot_bytes = correlate ? up16(16 * (size_t)M * nframes) : 0;          // rho alone keeps no transposed copy
    } else {
        p.rows = 0; p.small = n <= kSmallN; p.tile = 0; p.jtlog = 0; p.stride = 1; p.nseg = p.small ? 1 : (n + p.seglen - 1) / p.seglen;
        p.mode_lds = 0; p.unit = 0; p.rhot_bytes = 0;
    }
    p.psmall = n <= kSmallN;
    p.ptiles = p.psmall ? 1 : (n + kPairTile - 1) / kPairTile;
    p.slabs = p.o0 < kSlabs ? p.o0 : kSlabs;
    p.ops = (p.o0 + p.slabs - 1) / p.slabs;
    p.pwaves = kSmallWaves;
    if (nbins > 0) {
        if (p.psmall) {
            if ((size_t)kSmallWaves * (3 * kSmallN * 8 + 4 * (size_t)nbins) > (size_t)kLdsCap) p.pwaves = 1;
            p.pair_lds = (size_t)p.pwaves * (3 * kSmallN * 8 + 4 * (size_t)nbins);
        } else {
            p.pair_lds = 4 * (size_t)nbins + 3 * kPairTile * 8;
        }
    } else {
        p.pair_lds = 0;
    }
    p.lds = p.mode_lds > p.pair_lds ? p.mode_lds : p.pair_lds;
    p.otiles = (n + kOverlapTile - 1) / kOverlapTile;
    if (overlap && (long long)p.otiles * p.o0 > 0x7fffffffLL)
        return fail("%s: nwater = %d and %d origins make %d tiles x %d origins, beyond 2^31 - 1 workgroups of a box", who, n, p.o0, p.otiles, p.o0);
    p.qs_bytes = overlap ? up16(4 * (size_t)nlags * p.o0) : 0;
    p.per_box = p.rhot_bytes + p.qs_bytes;
    if (p.unit + p.per_box > budget)
        return fail("%s: one box needs %zu bytes of scratch (nframes = %d, nwater = %d, nlags = %d, M = %d) and does not fit the budget of %zu "
                    "bytes (MW_COLL_SCRATCH_MB)", who, p.unit + p.per_box, nframes, n, nlags, M, budget);
    // The mode pass keeps a quarter of the budget (at least one unit, at most what kMaxUnits units need) before the boxes
    // are counted, and then takes whatever the chunk's boxes leave: a launch of a few units would leave the device idle.
    size_t keep = 0;
    if (p.unit) {
        keep = budget / 4 > p.unit ? budget / 4 : p.unit;
        if (keep > p.unit * (size_t)kMaxUnits) keep = p.unit * (size_t)kMaxUnits;
        if (keep + p.per_box > budget) keep = p.unit;
    }
    size_t fit = p.per_box ? (budget - keep) / p.per_box : (size_t)kMaxChunkBoxes;
    if (fit > (size_t)kMaxChunkBoxes) fit = kMaxChunkBoxes;
    p.bpc = (int)fit;
    if (p.bpc > nboxes) p.bpc = nboxes;
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    size_t units = (size_t)p.bpc * nframes;
    if (units > (size_t)kMaxUnits) units = kMaxUnits;
    if (p.unit) {
        const size_t room = (budget - p.per_box * (size_t)p.bpc) / p.unit;
        if (units > room) units = room;
    }
    p.upl = (int)units;
    return 0;
}

int check_counts(const char* who, int nframes, int nboxes, int n, int nlags, int every, int M, int nbins, int nh)
{
    if (nframes < 1 || nframes > kMaxFrames) return fail("%s: nframes = %d outside 1..%d", who, nframes, kMaxFrames);
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    if (nlags < 1 || nlags > nframes) return fail("%s: nlags = %d outside 1..nframes = %d", who, nlags, nframes);
    if (every < 1) return fail("%s: origin_every = %d is not >= 1", who, every);
    if (M < 0 || M > MW_COLL_MAX_VECTORS) return fail("%s: M = %d outside 0..%d", who, M, MW_COLL_MAX_VECTORS);
    if (nbins < 0 || nbins > MW_COLL_MAX_BINS) return fail("%s: nbins = %d outside 0..%d", who, nbins, MW_COLL_MAX_BINS);
    if (nh < 0 || nh > MW_COLL_MAX_HIST_LAGS) return fail("%s: nh = %d outside 0..%d", who, nh, MW_COLL_MAX_HIST_LAGS);
    return 0;
}

int check_nvec(const char* who, int M, const int* nvec, int nmax[3])
{
    nmax[0] = nmax[1] = nmax[2] = 0;
    for (int v = 0; v < M; ++v)
        for (int a = 0; a < 3; ++a) {
            const int c = nvec[3 * (size_t)v + a];
            if (c > MW_COLL_MAX_COMPONENT || c < -MW_COLL_MAX_COMPONENT)
                return fail("%s: nvec: component %d of vector %d is %d, beyond %d", who, a, v, c, MW_COLL_MAX_COMPONENT);
            const int m = c < 0 ? -c : c;
            if (m > nmax[a]) nmax[a] = m;
        }
    return 0;
}

// The cell of the pair pass by the header's arithmetic: cofactor rows times 1 / det, the widths, the image range.
// False where r_max is beyond what three images per axis cover.
bool pair_cell(const double* h, double r_max, PairCell& c, double w[3])
{
    const double c0[3] = {h[4] * h[8] - h[5] * h[7], h[5] * h[6] - h[3] * h[8], h[3] * h[7] - h[4] * h[6]};   // h2 x h3
    const double c1[3] = {h[7] * h[2] - h[8] * h[1], h[8] * h[0] - h[6] * h[2], h[6] * h[1] - h[7] * h[0]};   // h3 x h1
    const double c2[3] = {h[1] * h[5] - h[2] * h[4], h[2] * h[3] - h[0] * h[5], h[0] * h[4] - h[1] * h[3]};   // h1 x h2
    const double det = h[0] * c0[0] + h[1] * c0[1] + h[2] * c0[2];
    const double vol = det < 0.0 ? -det : det;
    w[0] = vol / std::sqrt(c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2]);
    w[1] = vol / std::sqrt(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
    w[2] = vol / std::sqrt(c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2]);
    const double inv = 1.0 / det;
    for (int a = 0; a < 3; ++a) { c.g[a] = c0[a] * inv; c.g[3 + a] = c1[a] * inv; c.g[6 + a] = c2[a] * inv; }
    for (int k = 0; k < 9; ++k) c.h[k] = h[k];
    const double r = r_max * (1.0 + 1e-9);
    c.images = 1;
    for (int k = 0; k < 3; ++k) {
        if (r <= 0.5 * w[k]) c.m[k] = 0;
        else if (r <= 1.5 * w[k]) c.m[k] = 1;
        else return false;
        c.images *= 2 * c.m[k] + 1;
    }
    return true;
}

struct HostCells {
    std::vector<double> inv;                   // [nboxes][9], H^-1 row-major (the mode pass)
    std::vector<PairCell> pair;                // [nboxes] (the pair pass)
};

constexpr long double kCountCap = 4611686018427387904.0L;   // 2^62

// what both compute entries can check on the host before they look at the library's state
int check_host_side(const char* who, int nframes, int nboxes, int n, const double* cells, const double* pos, int nlags, int every, int M,
                    const int* nvec, double r_max, int nbins, int nh, const int* hist_lags, double a, const double* rho, const double* fkt,
                    const long long* gd, const long long* qsum, const long long* q2sum, int nmax[3], HostCells& hc)
{
    if (check_counts(who, nframes, nboxes, n, nlags, every, M, nbins, nh)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (M > 0 && !nvec) return fail("%s: nvec is NULL and M = %d", who, M);
    if (check_nvec(who, M, nvec, nmax)) return 1;
    if (rho && M == 0) return fail("%s: rho is asked for and M = 0", who);
    if (fkt && M == 0) return fail("%s: fkt is asked for and M = 0", who);
    if (nh > 0 && !hist_lags) return fail("%s: hist_lags is NULL and nh = %d", who, nh);
    for (int h = 0; h < nh; ++h)
        if (hist_lags[h] < 0 || hist_lags[h] >= nlags) return fail("%s: hist_lags[%d] = %d outside 0..nlags - 1 = %d", who, h, hist_lags[h], nlags - 1);
    if (gd && nbins == 0) return fail("%s: gd is asked for and nbins = 0", who);
    if (gd && nh == 0) return fail("%s: gd is asked for and nh = 0 (hist_lags selects its lags)", who);
    if (gd && (!(r_max > 0.0) || !std::isfinite(r_max))) return fail("%s: r_max = %g is not a finite range > 0", who, r_max);
    if (!std::isfinite(a) || a < 0.0) return fail("%s: overlap_a = %g is neither 0 nor a finite length > 0", who, a);
    if ((qsum || q2sum) && a == 0.0) return fail("%s: %s is asked for and overlap_a = 0", who, qsum ? "qsum" : "q2sum");
    const int e = every > nframes ? nframes : every;
    const long double o0 = (long double)((nframes - 1) / e + 1), n2 = (long double)n * (long double)n;
    hc.inv.resize(9 * (size_t)nboxes);
    if (gd) hc.pair.resize((size_t)nboxes);
    for (int b = 0; b < nboxes; ++b) {
        double det;
        if (!invert_cell(cells + 9 * (size_t)b, hc.inv.data() + 9 * (size_t)b, &det))
            return fail("%s: cells: the determinant of box %d is %g (zero or not finite)", who, b, det);
        if (gd) {
            double w[3];
            if (!pair_cell(cells + 9 * (size_t)b, r_max, hc.pair[b], w))
                return fail("%s: r_max = %.17g is beyond 1.5 x the smallest perpendicular width of box %d (%.17g, %.17g, %.17g): three images per "
                            "axis do not cover it", who, r_max, b, w[0], w[1], w[2]);
            if (o0 * n2 * (long double)hc.pair[b].images > kCountCap)
                return fail("%s: gd: %d origins x nwater^2 = %d^2 x %d images of box %d could pass 2^62 counts", who, (int)o0, n, hc.pair[b].images, b);
        }
    }
    if (q2sum && o0 * n2 > kCountCap) return fail("%s: q2sum: %d origins x nwater^2 = %d^2 could pass 2^62", who, (int)o0, n);
    Plan p;
    return make_plan(who, nframes, n, nlags, every, (rho || fkt) ? M : 0, nmax, fkt != nullptr, gd ? nbins : 0, qsum || q2sum, nboxes, g.live ? g.budget : kDefaultBudget, p);
}

int check_finite(const char* who, const char* name, int nframes, int nboxes, int n, const double* a)
{
    const size_t per_box = 3 * (size_t)n, count = (size_t)nframes * nboxes * per_box;
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(a[i]))
            return fail("%s: %s of molecule %zu of frame %zu of box %zu is not finite", who, name, i % per_box / 3, i / per_box / nboxes, i / per_box % nboxes);
    return 0;
}

int check_live(const char* who) { return check_live(who, "mw_coll_init", g); }

// The work of both entries, arguments already checked; pos and the outputs are device pointers, the lists host arrays.
int run(const char* who, int nframes, int nboxes, int n, const HostCells& hc, const double* pos, int nlags, int every, int M, const int* nvec,
        const int nmax[3], double r_max, int nbins, int nh, const int* hist_lags, double a, double* rho, double* fkt, long long* gd, long long* qsum,
        long long* q2sum)
{
    const bool want_overlap = qsum || q2sum, want_modes = rho || fkt;
    if (!gd) { nbins = 0; nh = 0; }
    if (!want_modes) M = 0;
    Plan p;
    if (make_plan(who, nframes, n, nlags, every, M, nmax, fkt != nullptr, nbins, want_overlap, nboxes, g.budget, p)) return 1;
    if (every > nframes) every = nframes;                                 // the same single origin, and no overflow in the kernels' arithmetic
    if (reserve(g.scratch, p.per_box * (size_t)p.bpc + p.unit * (size_t)p.upl + 16)) return 1;
    if (want_modes) {
        if (reserve(g.inv, hc.inv.size() * sizeof(double)) || reserve(g.nvec, 12 * (size_t)M)) return 1;
        HIPOK(hipMemcpyAsync(g.inv.p, hc.inv.data(), hc.inv.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
        HIPOK(hipMemcpyAsync(g.nvec.p, nvec, 12 * (size_t)M, hipMemcpyHostToDevice, g.stream));
    }
    if (gd) {
        if (reserve(g.cells, hc.pair.size() * sizeof(PairCell)) || reserve(g.lags, 4 * (size_t)nh)) return 1;
        HIPOK(hipMemcpyAsync(g.cells.p, hc.pair.data(), hc.pair.size() * sizeof(PairCell), hipMemcpyHostToDevice, g.stream));
        HIPOK(hipMemcpyAsync(g.lags.p, hist_lags, 4 * (size_t)nh, hipMemcpyHostToDevice, g.stream));
    }
    char* base = (char*)g.scratch.p;
    double* rhoT = fkt ? (double*)base : nullptr;
    unsigned* qs = (unsigned*)(base + p.rhot_bytes * (size_t)p.bpc);
    double2* T = (double2*)(base + p.per_box * (size_t)p.bpc);
    double2* part = T + (p.small ? 0 : (size_t)n * p.rows * p.upl);
    const size_t box_doubles = 3 * (size_t)n, gd_box = (size_t)nh * nbins;
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const double* d_pos = pos + box_doubles * b0;
        HIPOK(hipEventRecord(g.ev[0], g.stream));
        if (want_modes) {
            const double* d_inv = (const double*)g.inv.p + 9 * (size_t)b0;
            double* d_rho = rho ? rho + 2 * (size_t)M * b0 : nullptr;
            const long long total = (long long)nb * nframes;
            for (long long u0 = 0; u0 < total; u0 += p.upl) {
                const int nu = (int)(total - u0 < p.upl ? total - u0 : p.upl);
                if (!p.small) {
                    const long long lanes = (long long)nu * n;
                    hipLaunchKernelGGL(k_coll_phasors, dim3((unsigned)((lanes + kThreads - 1) / kThreads)), dim3(kThreads), 0, g.stream, nu, u0, nb,
                                       nboxes, n, nmax[0], nmax[1], nmax[2], d_inv, d_pos, T);
                    HIPOK(hipGetLastError());
                }
                const dim3 grid((unsigned)((M + kVecPerWg - 1) / kVecPerWg), (unsigned)p.nseg, (unsigned)nu);
                if (p.small)
                    hipLaunchKernelGGL(k_coll_sum<true>, grid, dim3(kThreads), p.mode_lds, g.stream, u0, nb, nboxes, n, M, nmax[0], nmax[1], nmax[2],
                                       p.jtlog, p.stride, p.seglen, (const int*)g.nvec.p, (const double2*)nullptr, d_inv, d_pos, part);
                else
                    hipLaunchKernelGGL(k_coll_sum<false>, grid, dim3(kThreads), p.mode_lds, g.stream, u0, nb, nboxes, n, M, nmax[0], nmax[1], nmax[2],
                                       p.jtlog, p.stride, p.seglen, (const int*)g.nvec.p, (const double2*)T, d_inv, d_pos, part);
                HIPOK(hipGetLastError());
                const long long outs = (long long)nu * M;
                hipLaunchKernelGGL(k_coll_finish, dim3((unsigned)((outs + kThreads - 1) / kThreads)), dim3(kThreads), 0, g.stream, nu, u0, nb, nboxes,
                                   M, p.nseg, nframes, (const double2*)part, d_rho, rhoT);
                HIPOK(hipGetLastError());
            }
        }
        HIPOK(hipEventRecord(g.ev[1], g.stream));
        if (fkt) {
            const int nlb = (nlags + kLagBlock - 1) / kLagBlock;
            hipLaunchKernelGGL(k_coll_corr, dim3((unsigned)(nlb * M), (unsigned)nb), dim3(kLagBlock), 0, g.stream, n, M, nframes, nlags, every,
                               (const double*)rhoT, fkt + 2 * (size_t)nlags * M * b0);
            HIPOK(hipGetLastError());
        }
        HIPOK(hipEventRecord(g.ev[2], g.stream));
        if (gd) {
            long long* d_gd = gd + gd_box * b0;
            HIPOK(hipMemsetAsync(d_gd, 0, 8 * gd_box * nb, g.stream));
            const PairCell* d_cells = (const PairCell*)g.cells.p + b0;
            if (p.psmall)
                hipLaunchKernelGGL(k_coll_pairs_small, dim3((unsigned)((p.slabs + p.pwaves - 1) / p.pwaves), (unsigned)nh, (unsigned)nb), dim3(64 * p.pwaves),
                                   p.pair_lds, g.stream, nframes, nboxes, n, every, nbins, r_max, nh, p.slabs, p.ops, d_cells, (const int*)g.lags.p, d_pos,
                                   (unsigned long long*)d_gd);
            else
                hipLaunchKernelGGL(k_coll_pairs, dim3((unsigned)(p.slabs * p.ptiles), (unsigned)nh, (unsigned)nb), dim3(kPairTile), 4 * (size_t)nbins,
                                   g.stream, nframes, nboxes, n, every, nbins, r_max, nh, p.ptiles, p.ops, d_cells, (const int*)g.lags.p, d_pos,
                                   (unsigned long long*)d_gd);
            HIPOK(hipGetLastError());
        }
        HIPOK(hipEventRecord(g.ev[3], g.stream));
        if (want_overlap) {
            HIPOK(hipMemsetAsync(qs, 0, p.qs_bytes * (size_t)nb, g.stream));
            unsigned* q0 = qs;                                             // [nb][nlags][o0], packed: the kernels index it so
            hipLaunchKernelGGL(k_coll_overlap, dim3((unsigned)(p.o0 * p.otiles), (unsigned)nb), dim3(kOverlapTile), 0, g.stream, nframes, nboxes, n, nlags,
                               every, p.o0, p.otiles, a * a, d_pos, q0);
            HIPOK(hipGetLastError());
            const long long outs = (long long)nb * nlags;
            hipLaunchKernelGGL(k_coll_overlap_sum, dim3((unsigned)((outs + kThreads - 1) / kThreads)), dim3(kThreads), 0, g.stream, nb, nframes, nlags,
                               every, p.o0, (const unsigned*)q0, qsum ? qsum + (size_t)nlags * b0 : nullptr, q2sum ? q2sum + (size_t)nlags * b0 : nullptr);
            HIPOK(hipGetLastError());
        }
        HIPOK(hipEventRecord(g.ev[4], g.stream));
        HIPOK(hipStreamSynchronize(g.stream));                              // the next chunk reuses the scratch
        for (int k = 0; k < 4; ++k) {
            float t = 0.0f;
            HIPOK(hipEventElapsedTime(&t, g.ev[k], g.ev[k + 1]));
            ms[k] += t;
        }
    }
    plan_fields(p, g.last);
    g.have_last = true;
    for (int k = 0; k < 4; ++k) g.ms[k] = ms[k];
    return 0;
}

// The first element of a device array that is not finite, by one kernel that writes nothing but its verdict.
int check_device_array(const char* who, const char* name, int nframes, int nboxes, int n, const double* a)
{
    const size_t per_box = 3 * (size_t)n, count = (size_t)nframes * nboxes * per_box;
    if (reserve(g.verdict, sizeof(unsigned long long))) return 1;
    unsigned long long v = kNoVerdict;
    HIPOK(hipMemcpyAsync(g.verdict.p, &v, sizeof v, hipMemcpyHostToDevice, g.stream));
    size_t blocks = (count + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_coll_check, dim3((unsigned)blocks), dim3(256), 0, g.stream, count, a, (unsigned long long*)g.verdict.p);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(&v, g.verdict.p, sizeof v, hipMemcpyDeviceToHost, g.stream));
    HIPOK(hipStreamSynchronize(g.stream));
    if (v != kNoVerdict)
        return fail("%s: %s of molecule %zu of frame %zu of box %zu is not finite", who, name, (size_t)(v % per_box / 3), (size_t)(v / per_box / nboxes),
                    (size_t)(v / per_box % nboxes));
    return 0;
}

}  // namespace

extern "C" {

const char* mw_coll_last_error(void) { return g_err; }
int mw_coll_is_initialised(void) { return g.live ? 1 : 0; }

int mw_coll_init(int device) { return runtime_init("mw_coll_init", "MW_COLL_SCRATCH_MB", device, g); }

int mw_coll_finalize(void)
{
    if (runtime_finalize(g, {&g.scratch, &g.verdict, &g.inv, &g.cells, &g.nvec, &g.lags, &g.pos, &g.rho, &g.fkt, &g.gd, &g.qsum, &g.q2sum})) return 1;
    g = State{};
    return 0;
}

int mw_coll_compute(int nframes, int nboxes, int nwater, const double* cells, const double* pos, int nlags, int origin_every, int M, const int* nvec,
                    double r_max, int nbins, int nh, const int* hist_lags, double overlap_a, double* rho, double* fkt, long long* gd, long long* qsum,
                    long long* q2sum)
{
    const char* who = "mw_coll_compute";
    int nmax[3];
    HostCells hc;
    if (check_host_side(who, nframes, nboxes, nwater, cells, pos, nlags, origin_every, M, nvec, r_max, nbins, nh, hist_lags, overlap_a, rho, fkt, gd, qsum,
                        q2sum, nmax, hc))
        return 1;
    if (check_finite(who, "pos", nframes, nboxes, nwater, pos)) return 1;
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    const size_t traj = 24 * (size_t)nframes * nboxes * nwater, rho_bytes = 16 * (size_t)nframes * nboxes * M, fkt_bytes = 16 * (size_t)nboxes * nlags * M;
    const size_t gd_bytes = 8 * (size_t)nboxes * nh * nbins, q_bytes = 8 * (size_t)nboxes * nlags;
    if (reserve(g.pos, traj)) return 1;
    if (rho && reserve(g.rho, rho_bytes)) return 1;
    if (fkt && reserve(g.fkt, fkt_bytes)) return 1;
    if (gd && reserve(g.gd, gd_bytes)) return 1;
    if (qsum && reserve(g.qsum, q_bytes)) return 1;
    if (q2sum && reserve(g.q2sum, q_bytes)) return 1;
    HIPOK(hipMemcpyAsync(g.pos.p, pos, traj, hipMemcpyHostToDevice, g.stream));
    if (run(who, nframes, nboxes, nwater, hc, (const double*)g.pos.p, nlags, origin_every, M, nvec, nmax, r_max, nbins, nh, hist_lags, overlap_a,
            rho ? (double*)g.rho.p : nullptr, fkt ? (double*)g.fkt.p : nullptr, gd ? (long long*)g.gd.p : nullptr, qsum ? (long long*)g.qsum.p : nullptr,
            q2sum ? (long long*)g.q2sum.p : nullptr))
        return 1;
    if (rho) HIPOK(hipMemcpyAsync(rho, g.rho.p, rho_bytes, hipMemcpyDeviceToHost, g.stream));
    if (fkt) HIPOK(hipMemcpyAsync(fkt, g.fkt.p, fkt_bytes, hipMemcpyDeviceToHost, g.stream));
    if (gd) HIPOK(hipMemcpyAsync(gd, g.gd.p, gd_bytes, hipMemcpyDeviceToHost, g.stream));
    if (qsum) HIPOK(hipMemcpyAsync(qsum, g.qsum.p, q_bytes, hipMemcpyDeviceToHost, g.stream));
    if (q2sum) HIPOK(hipMemcpyAsync(q2sum, g.q2sum.p, q_bytes, hipMemcpyDeviceToHost, g.stream));
    HIPOK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_coll_compute_device(int nframes, int nboxes, int nwater, const double* cells, const double* pos, int nlags, int origin_every, int M,
                           const int* nvec, double r_max, int nbins, int nh, const int* hist_lags, double overlap_a, double* rho, double* fkt, long long* gd,
                           long long* qsum, long long* q2sum)
{
    const char* who = "mw_coll_compute_device";
    int nmax[3];
    HostCells hc;
    if (check_host_side(who, nframes, nboxes, nwater, cells, pos, nlags, origin_every, M, nvec, r_max, nbins, nh, hist_lags, overlap_a, rho, fkt, gd, qsum,
                        q2sum, nmax, hc))
        return 1;
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    HIPOK(hipDeviceSynchronize());                                          // work queued before the call is waited for
    if (check_device_array(who, "pos", nframes, nboxes, nwater, pos)) return 1;
    return run(who, nframes, nboxes, nwater, hc, pos, nlags, origin_every, M, nvec, nmax, r_max, nbins, nh, hist_lags, overlap_a, rho, fkt, gd, qsum, q2sum);
}

int mw_coll_plan(int nframes, int nwater, int nlags, int origin_every, int M, const int nmax[3], int nbins, int nh, int overlap, int nboxes, int* out,
                 int nout)
{
    const char* who = "mw_coll_plan";
    if (check_counts(who, nframes, nboxes, nwater, nlags, origin_every, M, nbins, nh)) return 1;
    if (M > 0 && !nmax) return fail("%s: nmax is NULL and M = %d", who, M);
    for (int a = 0; a < 3 && M > 0; ++a)
        if (nmax[a] < 0 || nmax[a] > MW_COLL_MAX_COMPONENT) return fail("%s: nmax[%d] = %d outside 0..%d", who, a, nmax[a], MW_COLL_MAX_COMPONENT);
    if (!out || nout < 1) return fail("%s: out is NULL or nout < 1", who);
    Plan p;
    if (make_plan(who, nframes, nwater, nlags, origin_every, M, nmax, true, nbins, overlap, nboxes, g.live ? g.budget : kDefaultBudget, p)) return 1;
    int f[MW_COLL_PLAN_FIELDS];
    plan_fields(p, f);
    copy_fields(f, MW_COLL_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_coll_last(int* out, int nout)
{
    if (check_live("mw_coll_last")) return 1;
    if (!g.have_last) return fail("mw_coll_last: no call has launched yet");
    copy_fields(g.last, MW_COLL_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_coll_elapsed_ms(float* modes, float* correlate, float* pairs, float* overlap)
{
    if (check_live("mw_coll_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_coll_elapsed_ms: no call has launched yet");
    if (modes) *modes = g.ms[0];
    if (correlate) *correlate = g.ms[1];
    if (pairs) *pairs = g.ms[2];
    if (overlap) *overlap = g.ms[3];
    return 0;
}

}  // extern "C"
