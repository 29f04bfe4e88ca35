// mw_rdf.hip.h -- gfx950 (MI355X, CDNA4) device code of the mW energy engine: the pair-distance histogram of every box, from
// which the host forms the radial distribution function g(r) and the running coordination number n(r).  k_rdf_tiles (boxes of
// more than kRdfSmallMax molecules), k_rdf_small (one wavefront per box).  The reference has no counterpart.
#pragma once

#include "mw_common.hip.h"

namespace mw {

// =====================================================================================
// hist[b] = the number of ordered triples (i, j, n), n an integer lattice translation, (j, n) != (i, 0), with
// d = |r_j + n1 h1 + n2 h2 + n3 h3 - r_i|, 0 < d < r_max and b = floor(d nbins / r_max): the pair-distance histogram of the
// periodic system, not a minimum-image approximation.  The Verlet list reaches a sigma only, so this is all pairs.
//
// Every molecule is taken to fractional coordinates s = H^-1 r once (when it is staged); a pair is then ds = s_j - s_i,
// ds -= rint(ds) (every component in [-1/2, 1/2]), d0 = H ds, and d = d0 + (n1 h1 + n2 h2 + n3 h3) for every translation
// of the box's image set.  With w_k the perpendicular width of the cell along k, a translation n_k != 0 can only reach inside
// r_max if |n_k| < r_max / w_k + 1/2 (|ds_k + n_k| w_k <= |d|), so along k: n_k = 0 alone where r_max (1 + 1e-9) <= w_k / 2,
// else n_k in {-1, 0, 1}, which is complete up to r_max (1 + 1e-9) <= 1.5 w_k (the host refuses anything larger).  The set
// is symmetric under n -> -n and rint is odd, so (i, j, n) and (j, i, -n) have bitwise the same d: an unordered pair is
// evaluated once and counted twice.
//
// All arithmetic on positions is explicit fma chains: the s of a molecule is the same bits wherever it is formed, so that
// j = i gives ds = 0 exactly (its n = 0 term has d = 0 and is not counted; its images are).
// Counts are integers from the first LDS atomic to the int64 result: exact in any order.
// =====================================================================================
constexpr int kRdfSmallMax = 64;          // boxes up to here: one wavefront per box (k_rdf_small)
constexpr int kRdfSmallWaves = 4;         // ... and this many boxes per workgroup
constexpr int kRdfTile = 256;             // molecules per tile of k_rdf_tiles = its workgroup size
constexpr int kRdfMaxBins = 4096;
// 32-bit LDS counters of k_rdf_tiles: a tile pair adds at most kRdfTile^2 pairs x 27 images x 2 = 3 538 944 to a workgroup's
// histogram, so it is flushed every kRdfFlushTiles tile pairs: 1024 x 3 538 944 = 3.62e9 < 2^32.  (k_rdf_small: at most
// 64 x 33 x 27 x 2 per box.)
constexpr int kRdfFlushTiles = 1024;

struct RdfCell {
    double h[9];                           // h[3 k + a]: component a of cell vector k (d_hmat's layout)
    double g[9];                           // g[3 k + a]: component a of row k of the inverse, s_k = g_k . r
    int m[3];                              // image range along k: n_k in -m[k] .. m[k]
};

// Perpendicular widths of the cell and (optionally) its inverse; the image rule of the host and of the kernels.
__host__ __device__ inline void rdf_cell_widths(const double* h, double* g, double w[3])
{
    const double c0[3] = {h[4] * h[8] - h[5] * h[7], h[5] * h[6] - h[3] * h[8], h[3] * h[7] - h[4] * h[6]};   // h2 x h3
    const double c1[3] = {h[7] * h[2] - h[8] * h[1], h[8] * h[0] - h[6] * h[2], h[6] * h[1] - h[7] * h[0]};   // h3 x h1
    const double c2[3] = {h[1] * h[5] - h[2] * h[4], h[2] * h[3] - h[0] * h[5], h[0] * h[4] - h[1] * h[3]};   // h1 x h2
    const double det = h[0] * c0[0] + h[1] * c0[1] + h[2] * c0[2];
    const double vol = det < 0.0 ? -det : det;
    w[0] = vol / sqrt(c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2]);
    w[1] = vol / sqrt(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
    w[2] = vol / sqrt(c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2]);
    if (g) {
        const double inv = 1.0 / det;
        for (int a = 0; a < 3; ++a) { g[a] = c0[a] * inv; g[3 + a] = c1[a] * inv; g[6 + a] = c2[a] * inv; }
    }
}
// images along an axis of width w: 0 (n_k = 0 alone) or 1 (n_k = -1, 0, 1); -1: r_max is beyond what three images cover
__host__ __device__ inline int rdf_axis_images(double r_max, double w)
{
    const double r = r_max * (1.0 + 1e-9);
    if (r <= 0.5 * w) return 0;
    if (r <= 1.5 * w) return 1;
    return -1;
}

__device__ __forceinline__ void rdf_load_cell(const double* __restrict__ hmat, int b, double r_max, RdfCell& c)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) c.h[k] = hmat[(size_t)b * 9 + k];
    double w[3];
    rdf_cell_widths(c.h, c.g, w);
#pragma unroll
    for (int k = 0; k < 3; ++k) c.m[k] = rdf_axis_images(r_max, w[k]) != 0 ? 1 : 0;   // (the host has refused -1)
}

__device__ __forceinline__ void rdf_frac(const RdfCell& c, const double* __restrict__ p, double& sx, double& sy, double& sz)
{
    const double x = p[0], y = p[1], z = p[2];
    sx = __builtin_fma(c.g[0], x, __builtin_fma(c.g[1], y, c.g[2] * z));
    sy = __builtin_fma(c.g[3], x, __builtin_fma(c.g[4], y, c.g[5] * z));
    sz = __builtin_fma(c.g[6], x, __builtin_fma(c.g[7], y, c.g[8] * z));
}

// One pair: every image of j around i, `weight` counts each.  hist: this wavefront's / workgroup's LDS histogram.
__device__ __forceinline__ void rdf_pair(const RdfCell& c, double six, double siy, double siz, double sjx, double sjy, double sjz,
                                         double rmax2, double scale, int nbins, unsigned weight, unsigned* hist)
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
                if (r2 < rmax2 && r2 > 0.0) {
                    const double d = __builtin_sqrt(r2);
                    int b = (int)(d * scale);                              // floor: d * scale >= 0
                    b = b < nbins ? b : nbins - 1;                        // (d within an ulp of r_max)
                    atomicAdd(&hist[b], weight);
                }
            }
        }
    }
}

// Boxes of more than kRdfSmallMax molecules.  T = ceil(N / kRdfTile) tiles; workgroup (box, I) keeps tile I in registers (one
// molecule per lane) and streams tiles J = I, I + 1, ... I + T / 2 (mod T) through LDS -- every unordered tile pair once: for
// even T the offset T / 2 is taken by I < T / 2 only.  J != I: every pair counts twice.  J = I: all ordered pairs of the tile,
// counted once (j = i contributes its images).
__global__ __launch_bounds__(kRdfTile)
void k_rdf_tiles(const double* __restrict__ pos, const double* __restrict__ hmat, double r_max, int nbins,
                 unsigned long long* __restrict__ out,     // [box - box0][nbins], zeroed before the launch
                 int N, int T, int box0)
{
    extern __shared__ unsigned rdf_hist[];                 // [nbins]
    __shared__ double tsx[kRdfTile], tsy[kRdfTile], tsz[kRdfTile];
    const int tid = threadIdx.x;
    const int lb = (int)(blockIdx.x / (unsigned)T), I = (int)(blockIdx.x - (unsigned)lb * (unsigned)T);
    const int b = box0 + lb;
    const double* P = pos + (size_t)b * N * 3;
    unsigned long long* H = out + (size_t)lb * nbins;

    RdfCell c;
    rdf_load_cell(hmat, b, r_max, c);
    const double rmax2 = r_max * r_max;
    const double scale = (double)nbins / r_max;
    for (int k = tid; k < nbins; k += kRdfTile) rdf_hist[k] = 0u;

    const int i = I * kRdfTile + tid;
    double six = 0.0, siy = 0.0, siz = 0.0;
    if (i < N) rdf_frac(c, P + 3 * (size_t)i, six, siy, siz);

    const int noff = (T & 1) ? (T - 1) / 2 : (I < T / 2 ? T / 2 : T / 2 - 1);     // offsets 0 .. noff
    for (int o = 0; o <= noff; ++o) {
        int J = I + o;
        if (J >= T) J -= T;
        const int j0 = J * kRdfTile;
        const int nj = min(kRdfTile, N - j0);
        __syncthreads();                                   // the tile before this one has been read (and the zeroing is done)
        if (o > 0 && (o % kRdfFlushTiles) == 0) {          // uniform: keep the 32-bit counters from overflowing
            for (int k = tid; k < nbins; k += kRdfTile) {
                const unsigned v = rdf_hist[k];
                if (v) { atomicAdd(&H[k], (unsigned long long)v); rdf_hist[k] = 0u; }
            }
            __syncthreads();
        }
        if (tid < nj) {
            double x, y, z;
            rdf_frac(c, P + 3 * (size_t)(j0 + tid), x, y, z);
            tsx[tid] = x; tsy[tid] = y; tsz[tid] = z;
        }
        __syncthreads();
        if (i < N) {
            const unsigned weight = o == 0 ? 1u : 2u;
#pragma unroll 2
            for (int j = 0; j < nj; ++j)
                rdf_pair(c, six, siy, siz, tsx[j], tsy[j], tsz[j], rmax2, scale, nbins, weight, rdf_hist);
        }
    }
    __syncthreads();
    for (int k = tid; k < nbins; k += kRdfTile) {
        const unsigned v = rdf_hist[k];
        if (v) atomicAdd(&H[k], (unsigned long long)v);
    }
}

// Boxes of at most kRdfSmallMax molecules: one wavefront per box, kRdfSmallWaves boxes per workgroup, each wavefront with its
// own positions and histogram in LDS.  Lane i meets j = i + o (mod N) for o = 0 .. N / 2: o = 0 is i itself (its images),
// counted once; 0 < o < N / 2 reaches every unordered pair once, counted twice; o = N / 2 (even N) is reached from both ends,
// counted once each.  The wavefront is its box's only writer: plain stores of all nbins counts, no zeroing needed.
__global__ __launch_bounds__(64 * kRdfSmallWaves)
void k_rdf_small(const double* __restrict__ pos, const double* __restrict__ hmat, double r_max, int nbins,
                 unsigned long long* __restrict__ out,     // [box - box0][nbins]
                 int N, int count, int box0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rdf_smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lb = (int)blockIdx.x * kRdfSmallWaves + wave;
    const bool live = lb < count;
    const int b = box0 + (live ? lb : 0);
    double* sx = reinterpret_cast<double*>(rdf_smem) + (size_t)wave * 3 * kRdfSmallMax;
    double* sy = sx + kRdfSmallMax;
    double* sz = sy + kRdfSmallMax;
    unsigned* hist = reinterpret_cast<unsigned*>(rdf_smem + (size_t)kRdfSmallWaves * 3 * kRdfSmallMax * sizeof(double)) + (size_t)wave * nbins;

    RdfCell c;
    rdf_load_cell(hmat, b, r_max, c);
    const double rmax2 = r_max * r_max;
    const double scale = (double)nbins / r_max;
    for (int k = lane; k < nbins; k += 64) hist[k] = 0u;
    const bool mine = live && lane < N;
    double six = 0.0, siy = 0.0, siz = 0.0;
    if (mine) {
        rdf_frac(c, pos + ((size_t)b * N + lane) * 3, six, siy, siz);
        sx[lane] = six; sy[lane] = siy; sz[lane] = siz;
    }
    __syncthreads();
    if (mine) {
        const int half = N / 2;
        for (int o = 0; o <= half; ++o) {
            int j = lane + o;
            if (j >= N) j -= N;
            const unsigned weight = (o == 0 || 2 * o == N) ? 1u : 2u;
            rdf_pair(c, six, siy, siz, sx[j], sy[j], sz[j], rmax2, scale, nbins, weight, hist);
        }
    }
    __syncthreads();
    if (live) {
        unsigned long long* H = out + (size_t)lb * nbins;
        for (int k = lane; k < nbins; k += 64) H[k] = (unsigned long long)hist[k];
    }
}

}  // namespace mw
