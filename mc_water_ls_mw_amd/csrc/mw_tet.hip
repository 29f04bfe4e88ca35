// libmw_tet.so -- the nearest-neighbour order parameters of include/mw_tet.h: the tetrahedral order q, its translational
// companion s_k, the fifth-neighbour distance d5 and the local structure index of every molecule, the four nearest
// neighbours and the box means, for many boxes.  General geometry (nwater > 64): a counting sort into a fractional cell grid
// (k_tet_bin, k_tet_scan, k_tet_place, k_tet_rank), then k_tet_select, one lane per molecule in sorted order, walks the 27
// neighbouring cells and keeps the 16 nearest entries sorted in registers, and k_tet_summary adds the box up.  Small geometry
// (nwater <= 64): k_tet_small, one wavefront per box with the box in LDS.  Every bit of a box's results depends on the box and
// the two radii alone (mw_tet.h): the arithmetic below is spelled out in fma / mul / add with contraction off, and the order
// of every sum and of every ranking is fixed.  (The binning kernels and the grid rules are those of mw_boo.hip, written out
// again here: the two libraries share host code only.)
#include "../../include/mw_tet.h"

#include "mw_common.hip.h"

#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too

namespace mwtet {

constexpr int kThreads = 256;
constexpr int kSmallN = 64;
constexpr int kSmallBoxesPerWg = kThreads / 64;   // one wavefront per box
constexpr int kKeep = MW_TET_KEEP;
constexpr int kOrd = 4;                           // doubles per molecule in scratch: q, s_k, d5, lsi
constexpr int kSums = 8;                          // box sums: the four values over the molecules where defined, and how many
constexpr int kMaxGrid = 1024;
constexpr int kMaxWater = 1 << 22;
constexpr int kMaxBoxes = 1 << 24;
constexpr int kMaxChunkBoxes = 65535;             // grid y
constexpr int kSmallChunkBoxes = 1 << 20;
constexpr double kGuard = 1.0 + 1e-9;
constexpr int kSmallLds = kSmallBoxesPerWg * 3 * 64 * 8;
constexpr int kPlaceBits = 22;                    // an entry: the place (or index) of j in the low bits, its image above
constexpr int kPlaceMask = (1 << kPlaceBits) - 1;
static_assert(kMaxWater <= (1 << kPlaceBits), "an entry holds a molecule in kPlaceBits bits");

__device__ __forceinline__ double undefined() { return __longlong_as_double(0x7ff8000000000000LL); }

// s_a = (H^-1 r)_a reduced to [0, 1); I = H^-1, row-major
__device__ __forceinline__ double frac_coord(const double* __restrict__ I, int a, double x, double y, double z)
{
    double s = __builtin_fma(I[3 * a], x, __builtin_fma(I[3 * a + 1], y, I[3 * a + 2] * z));
    s = s - __builtin_floor(s);
    return s >= 1.0 ? 0.0 : s;                 // (-1e-17 - floor = 1.0 after rounding)
}

// the cell of s along an axis of g cells, inside the table whatever s is
__device__ __forceinline__ int cell_of(double s, int g)
{
    const int c = (int)(s * (double)g);
    return c < 0 ? 0 : c >= g ? g - 1 : c;
}

// d = H ds (c = the cell's 9 doubles: c[3 k + a] = component a of h_(k+1)); returns |d|^2
__device__ __forceinline__ double bond_vector(const double* __restrict__ c, double a0, double a1, double a2, double& dx, double& dy, double& dz)
{
    dx = __builtin_fma(c[0], a0, __builtin_fma(c[3], a1, c[6] * a2));
    dy = __builtin_fma(c[1], a0, __builtin_fma(c[4], a1, c[7] * a2));
    dz = __builtin_fma(c[2], a0, __builtin_fma(c[5], a1, c[8] * a2));
    return __builtin_fma(dx, dx, __builtin_fma(dy, dy, dz * dz));
}

// Offset o in {-1, 0, 1} from cell c of g: the cell it lands in and the image shift that goes with it.
__device__ __forceinline__ void wrap_cell(int c, int o, int g, int& cw, int& shift)
{
    cw = c + o; shift = 0;
    if (cw < 0) { cw += g; shift = -1; }
    if (cw >= g) { cw -= g; shift = 1; }
}

// ---- the 16 nearest, sorted in registers ---------------------------------------------------------------------------------
// k[a] / e[a]: r^2 and the entry of rank a + 1, +inf / -1 where there is none yet.  Every index below is a compile-time
// constant after unrolling, so both arrays live in registers.
struct Nearest {
    double k[kKeep];
    int e[kKeep];
    int n_search = 0, n_lsi = 0;
    __device__ __forceinline__ Nearest()
    {
#pragma unroll
        for (int a = 0; a < kKeep; ++a) { k[a] = __builtin_inf(); e[a] = -1; }
    }
    // An entry within r_search.  It goes in front of the first kept one with a larger r^2 -- behind its equals, which came
    // earlier in the walk -- and the chain is entered only when it beats the current 16th.
    __device__ __forceinline__ void add(double r2, double rl2, int entry)
    {
        ++n_search;
        if (r2 < rl2) ++n_lsi;
        if (!(r2 < k[kKeep - 1])) return;
#pragma unroll
        for (int a = kKeep - 1; a >= 1; --a) {
            const bool above = r2 < k[a - 1], here = r2 < k[a];
            k[a] = above ? k[a - 1] : here ? r2 : k[a];
            e[a] = above ? e[a - 1] : here ? entry : e[a];
        }
        const bool first = r2 < k[0];
        k[0] = first ? r2 : k[0];
        e[0] = first ? entry : e[0];
    }
};

// (q, s_k, d5, lsi) from the ranked r^2 and the vectors d[a] of ranks 1..4 (read only where the rank exists)
__device__ __forceinline__ void order_values(const Nearest& t, const double (&d)[4][3], double (&o)[kOrd])
{
    double r[kKeep];
#pragma unroll
    for (int a = 0; a < kKeep; ++a) r[a] = __builtin_sqrt(t.k[a]);
    o[0] = o[1] = o[2] = o[3] = undefined();
    if (t.n_search >= 4) {
        double u[4][3];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double rinv = 1.0 / r[a];
            u[a][0] = d[a][0] * rinv; u[a][1] = d[a][1] * rinv; u[a][2] = d[a][2] * rinv;
        }
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a + 1; b < 4; ++b) {
                const double c = __builtin_fma(u[a][0], u[b][0], __builtin_fma(u[a][1], u[b][1], u[a][2] * u[b][2]));
                const double v = c + 1.0 / 3.0;
                acc = __builtin_fma(v, v, acc);
            }
        o[0] = __builtin_fma(-0.375, acc, 1.0);
        const double rbar = 0.25 * (((r[0] + r[1]) + r[2]) + r[3]);
        double dev = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double v = r[a] - rbar;
            dev = __builtin_fma(v, v, dev);
        }
        o[1] = 1.0 - dev / (12.0 * (rbar * rbar));
    }
    if (t.n_search >= 5) o[2] = r[4];
    const int kept = t.n_search < kKeep ? t.n_search : kKeep, n = t.n_lsi;
    if (n >= 1 && n + 1 <= kept) {
        const double m = (double)n;
        double sum = 0.0;
#pragma unroll
        for (int a = 0; a + 1 < kKeep; ++a)
            if (a < n) sum = sum + (r[a + 1] - r[a]);
        const double mean = sum / m;
        double var = 0.0;
#pragma unroll
        for (int a = 0; a + 1 < kKeep; ++a)
            if (a < n) {
                const double v = (r[a + 1] - r[a]) - mean;
                var = __builtin_fma(v, v, var);
            }
        o[3] = var / m;
    }
}

// the means over the molecules where each value is defined, and their numbers, from the box sums t[kSums]
__device__ __forceinline__ void write_summary(const double* t, double* out)
{
    for (int k = 0; k < 4; ++k) {
        out[k] = t[4 + k] > 0.0 ? t[k] / t[4 + k] : undefined();
        out[4 + k] = t[4 + k];
    }
}

// ---- general geometry ----------------------------------------------------------------------------------------------------
// par[box][18]: the cell (9) and its inverse (9).  grid[box][4]: g_1, g_2, g_3, cells.  Per box in scratch: su [n][3] fractional
// positions by index, cid [n], tmp [n] (members of the cells in arrival order), cnt / start [cap + 1]; then in cell order:
// idx [n] the molecule, ss [n][3], ord [n][kOrd].

// One lane per molecule: s, its cell, the cell's count.
__global__ __launch_bounds__(kThreads) void k_tet_bin(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                      const double* __restrict__ pos, double* __restrict__ su, int* __restrict__ cid,
                                                      int* __restrict__ cnt)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const double* I = par + 18 * (size_t)b + 9;
    const int* g = grid + 4 * (size_t)b;
    const size_t m = (size_t)b * n + i;
    const double x = pos[3 * m], y = pos[3 * m + 1], z = pos[3 * m + 2];
    const double s0 = frac_coord(I, 0, x, y, z), s1 = frac_coord(I, 1, x, y, z), s2 = frac_coord(I, 2, x, y, z);
    su[3 * m] = s0; su[3 * m + 1] = s1; su[3 * m + 2] = s2;
    const int c = (cell_of(s2, g[2]) * g[1] + cell_of(s1, g[1])) * g[0] + cell_of(s0, g[0]);
    cid[m] = c;
    atomicAdd(cnt + (size_t)b * (cap + 1) + c, 1);
}

// One workgroup per box: start[c] = the members of the cells before c, start[cells] = n.
__global__ __launch_bounds__(kThreads) void k_tet_scan(int cap, const int* __restrict__ grid, const int* __restrict__ cnt, int* __restrict__ start)
{
    __shared__ int part[kThreads];
    const int b = blockIdx.x, tid = threadIdx.x, cells = grid[4 * (size_t)b + 3];
    const int* cn = cnt + (size_t)b * (cap + 1);
    int* st = start + (size_t)b * (cap + 1);
    const int per = (cells + kThreads - 1) / kThreads, c0 = min(tid * per, cells), c1 = min(c0 + per, cells);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += cn[c];
    part[tid] = sum;
    __syncthreads();
    int before = 0;
    for (int t = 0; t < tid; ++t) before += part[t];
    for (int c = c0; c < c1; ++c) { st[c] = before; before += cn[c]; }
    if (tid == kThreads - 1) st[cells] = before;
}

// One lane per molecule: a place among its cell's members, in arrival order (k_tet_rank puts them in index order).
__global__ __launch_bounds__(kThreads) void k_tet_place(int n, int cap, const int* __restrict__ cid, const int* __restrict__ start,
                                                        int* __restrict__ cnt, int* __restrict__ tmp)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t m = (size_t)b * n + i, t = (size_t)b * (cap + 1);
    const int c = cid[m];
    const int slot = start[t + c] + atomicSub(cnt + t + c, 1) - 1;
    tmp[(size_t)b * n + slot] = i;
}

// One lane per member: its rank by molecule index among the members of its cell is its place in the sorted order.
__global__ __launch_bounds__(kThreads) void k_tet_rank(int n, int cap, const int* __restrict__ cid, const int* __restrict__ start,
                                                       const int* __restrict__ tmp, const double* __restrict__ su, int* __restrict__ idx,
                                                       double* __restrict__ ss)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const size_t o = (size_t)b * n, t = (size_t)b * (cap + 1);
    const int i = tmp[o + p], c = cid[o + i];
    const int q0 = start[t + c], q1 = start[t + c + 1];
    int rank = 0;
    for (int q = q0; q < q1; ++q) rank += tmp[o + q] < i ? 1 : 0;
    const size_t d = o + q0 + rank;
    idx[d] = i;
    ss[3 * d] = su[3 * (o + i)]; ss[3 * d + 1] = su[3 * (o + i) + 1]; ss[3 * d + 2] = su[3 * (o + i) + 2];
}

// The selection pass, one lane per molecule in sorted order: the walk of the 27 cells in the contract's order, every entry
// within r_search offered to the lane's Nearest; then the values of the molecule.  An entry is the sorted place of j with the
// image shift (-1, 0, 1 per axis, base 3) above it, enough to form d again for the four that end up nearest.
__global__ __launch_bounds__(kThreads) void k_tet_select(int n, int cap, double rs2, double rl2, const double* __restrict__ par,
                                                         const int* __restrict__ grid, const int* __restrict__ start, const double* __restrict__ ss,
                                                         const int* __restrict__ idx, double* __restrict__ ord, double* __restrict__ order,
                                                         int* __restrict__ near_, int* __restrict__ counts)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const double* H = par + 18 * (size_t)b;
    const int* g = grid + 4 * (size_t)b;
    const int* st = start + (size_t)b * (cap + 1);
    const size_t o = (size_t)b * n;
    const double* S = ss + 3 * o;
    const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
    const int g0 = g[0], g1 = g[1], g2 = g[2];
    const int c0 = cell_of(s0, g0), c1 = cell_of(s1, g1), c2 = cell_of(s2, g2);
    Nearest t;
    for (int oz = -1; oz <= 1; ++oz) {
        int wz, hz;
        wrap_cell(c2, oz, g2, wz, hz);
        for (int oy = -1; oy <= 1; ++oy) {
            int wy, hy;
            wrap_cell(c1, oy, g1, wy, hy);
            for (int ox = -1; ox <= 1; ++ox) {
                int wx, hx;
                wrap_cell(c0, ox, g0, wx, hx);
                const int c = (wz * g1 + wy) * g0 + wx;
                const int image = (((hz + 1) * 3 + (hy + 1)) * 3 + (hx + 1)) << kPlaceBits;
                const double fx = (double)hx, fy = (double)hy, fz = (double)hz;
                const int q1 = st[c + 1];
                for (int q = st[c]; q < q1; ++q) {
                    const double a0 = (S[3 * (size_t)q] - s0) + fx, a1 = (S[3 * (size_t)q + 1] - s1) + fy, a2 = (S[3 * (size_t)q + 2] - s2) + fz;
                    double dx, dy, dz;
                    const double r2 = bond_vector(H, a0, a1, a2, dx, dy, dz);
                    if (r2 < rs2 && r2 > 0.0) t.add(r2, rl2, image | q);
                }
            }
        }
    }
    double d[4][3];
    int who[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        d[a][0] = d[a][1] = d[a][2] = 0.0;
        who[a] = -1;
        if (a < t.n_search) {                                  // (an entry is a place only where the rank exists)
            const int q = t.e[a] & kPlaceMask, image = t.e[a] >> kPlaceBits;
            const double fx = (double)(image % 3 - 1), fy = (double)(image / 3 % 3 - 1), fz = (double)(image / 9 - 1);
            (void)bond_vector(H, (S[3 * (size_t)q] - s0) + fx, (S[3 * (size_t)q + 1] - s1) + fy, (S[3 * (size_t)q + 2] - s2) + fz,
                              d[a][0], d[a][1], d[a][2]);
            who[a] = idx[o + q];
        }
    }
    double v[kOrd];
    order_values(t, d, v);
    double* w = ord + kOrd * (o + p);
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
    const size_t i = o + idx[o + p];
    if (order) { order[4 * i] = v[0]; order[4 * i + 1] = v[1]; order[4 * i + 2] = v[2]; order[4 * i + 3] = v[3]; }
    if (near_) { near_[4 * i] = who[0]; near_[4 * i + 1] = who[1]; near_[4 * i + 2] = who[2]; near_[4 * i + 3] = who[3]; }
    if (counts) { counts[2 * i] = t.n_search; counts[2 * i + 1] = t.n_lsi; }
}

// One workgroup per box: lane t adds the sorted places t, t + 256, ... in that order, a fixed tree adds the lanes of a
// wavefront and thread 0 the four wavefronts in order.
__global__ __launch_bounds__(kThreads) void k_tet_summary(int n, const double* __restrict__ ord, double* __restrict__ summary)
{
    __shared__ double part[kThreads / 64][kSums];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* O = ord + kOrd * (size_t)b * n;
    double t[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) t[k] = 0.0;
    for (int p = tid; p < n; p += kThreads) {
#pragma unroll
        for (int k = 0; k < kOrd; ++k) {
            const double v = O[kOrd * (size_t)p + k];
            const bool defined = v == v;
            t[k] = t[k] + (defined ? v : 0.0);
            t[4 + k] = t[4 + k] + (defined ? 1.0 : 0.0);
        }
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
        const double w = mw::wave_sum(t[k]);
        if ((tid & 63) == 0) part[tid >> 6][k] = w;
    }
    __syncthreads();
    if (tid == 0) {
        double tot[kSums];
        for (int k = 0; k < kSums; ++k) {
            double a = part[0][k];
            for (int w = 1; w < kThreads / 64; ++w) a = a + part[w][k];
            tot[k] = a;
        }
        write_summary(tot, summary + kSums * (size_t)b);
    }
}

// ---- small geometry: one wavefront per box, lane i = molecule i, the box's fractional positions in LDS ----------------------
// The entries of i: j in index order, and for each j the eight combinations of ds_k and ds_k -/+ 1 (the only two images per
// axis that can come within r_search <= w_k), combination bit k choosing the second along axis k.  An entry is j with the
// combination above it.
__global__ __launch_bounds__(kThreads) void k_tet_small(int nb, int n, double rs2, double rl2, const double* __restrict__ par,
                                                        const double* __restrict__ pos, double* __restrict__ order, int* __restrict__ near_,
                                                        int* __restrict__ counts, double* __restrict__ summary)
{
    __shared__ double lds[kSmallBoxesPerWg][3 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * kSmallBoxesPerWg + wave;
    if (b >= nb) return;                                   // the whole wavefront; no workgroup barrier below
    double* S = lds[wave];
    const double* H = par + 18 * (size_t)b;
    const bool active = lane < n;
    const size_t m = (size_t)b * n + (active ? lane : 0);
    const double s0 = frac_coord(H + 9, 0, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s1 = frac_coord(H + 9, 1, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s2 = frac_coord(H + 9, 2, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    S[lane] = s0; S[64 + lane] = s1; S[128 + lane] = s2;
    mw::wave_fence();

    Nearest t;
    for (int j = 0; j < n; ++j) {
        const double e0 = S[j] - s0, e1 = S[64 + j] - s1, e2 = S[128 + j] - s2;
        const double f0 = e0 > 0.0 ? e0 - 1.0 : e0 + 1.0, f1 = e1 > 0.0 ? e1 - 1.0 : e1 + 1.0, f2 = e2 > 0.0 ? e2 - 1.0 : e2 + 1.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            double dx, dy, dz;
            const double r2 = bond_vector(H, (c & 1) ? f0 : e0, (c & 2) ? f1 : e1, (c & 4) ? f2 : e2, dx, dy, dz);
            if (active && r2 < rs2 && r2 > 0.0) t.add(r2, rl2, (c << kPlaceBits) | j);
        }
    }
    double d[4][3];
    int who[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        d[a][0] = d[a][1] = d[a][2] = 0.0;
        who[a] = -1;
        if (a < t.n_search) {
            const int j = t.e[a] & kPlaceMask, c = t.e[a] >> kPlaceBits;
            const double e0 = S[j] - s0, e1 = S[64 + j] - s1, e2 = S[128 + j] - s2;
            const double f0 = e0 > 0.0 ? e0 - 1.0 : e0 + 1.0, f1 = e1 > 0.0 ? e1 - 1.0 : e1 + 1.0, f2 = e2 > 0.0 ? e2 - 1.0 : e2 + 1.0;
            (void)bond_vector(H, (c & 1) ? f0 : e0, (c & 2) ? f1 : e1, (c & 4) ? f2 : e2, d[a][0], d[a][1], d[a][2]);
            who[a] = j;
        }
    }
    double v[kOrd];
    order_values(t, d, v);
    if (active) {
        if (order) { order[4 * m] = v[0]; order[4 * m + 1] = v[1]; order[4 * m + 2] = v[2]; order[4 * m + 3] = v[3]; }
        if (near_) { near_[4 * m] = who[0]; near_[4 * m + 1] = who[1]; near_[4 * m + 2] = who[2]; near_[4 * m + 3] = who[3]; }
        if (counts) { counts[2 * m] = t.n_search; counts[2 * m + 1] = t.n_lsi; }
    }
    if (summary) {                                         // wave-uniform: lanes beyond n and undefined values add +0.0
        double tot[kSums];
#pragma unroll
        for (int k = 0; k < kOrd; ++k) {
            const bool defined = active && v[k] == v[k];
            tot[k] = mw::wave_sum(defined ? v[k] : 0.0);
            tot[4 + k] = mw::wave_sum(defined ? 1.0 : 0.0);
        }
        if (lane == 0) write_summary(tot, summary + kSums * (size_t)b);
    }
}

}  // namespace mwtet

namespace {

using namespace mwtet;

struct State : Runtime<4> {
    Buf scratch, par, grid, pos, order, near_, counts, summary;
    int last[MW_TET_PLAN_FIELDS] = {0};
    float ms[3] = {0.0f, 0.0f, 0.0f};
} g;

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// The scratch of one box of the general geometry, piece by piece (byte offsets inside a chunk are these times boxes per chunk).
struct Layout {
    int cap;                                                // cells a box may have
    size_t su, cid, tmp, cnt, start, idx, ss, ord, per_box;
};

Layout make_layout(int n)
{
    Layout l;
    l.cap = 2 * n > 64 ? 2 * n : 64;
    const size_t tab = align16(4 * ((size_t)l.cap + 1));
    size_t o = 0;
    l.su = o;    o += align16(24 * (size_t)n);
    l.cid = o;   o += align16(4 * (size_t)n);
    l.tmp = o;   o += align16(4 * (size_t)n);
    l.cnt = o;   o += tab;
    l.start = o; o += tab;
    l.idx = o;   o += align16(4 * (size_t)n);
    l.ss = o;    o += align16(24 * (size_t)n);
    l.ord = o;   o += align16(8 * (size_t)kOrd * n);
    l.per_box = o;
    return l;
}

struct Plan {
    int small, bpc, chunks, lds, boxes_per_wg;
    Layout lay;
    size_t per_box;
};

int make_plan(const char* who, int n, int nboxes, size_t budget, Plan& p)
{
    p.small = n <= kSmallN;
    p.lay = make_layout(n);
    if (p.small) {
        p.per_box = 0; p.lds = kSmallLds; p.boxes_per_wg = kSmallBoxesPerWg;
        p.bpc = nboxes < kSmallChunkBoxes ? nboxes : kSmallChunkBoxes;
    } else {
        p.per_box = p.lay.per_box; p.lds = (int)sizeof(double) * (kThreads / 64) * kSums; p.boxes_per_wg = 0;
        const size_t fit = budget / p.per_box;
        if (fit < 1)
            return fail("%s: one box needs %zu bytes of scratch (nwater = %d) and does not fit the budget of %zu bytes (MW_TET_SCRATCH_MB)",
                        who, p.per_box, n, budget);
        p.bpc = (int)(fit < (size_t)kMaxChunkBoxes ? fit : (size_t)kMaxChunkBoxes);
        if (p.bpc > nboxes) p.bpc = nboxes;
    }
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

void plan_fields(const Plan& p, const int grid[3], int* f)
{
    f[0] = p.bpc; f[1] = p.chunks; f[2] = p.small; f[3] = grid[0]; f[4] = grid[1]; f[5] = grid[2];
    f[6] = p.lds; f[7] = (int)p.per_box; f[8] = p.boxes_per_wg;
}

// w_k = |det| / |h_l x h_m|
void cell_widths(const double* c, double det, double w[3])
{
    for (int k = 0; k < 3; ++k) {
        const double* a = c + 3 * ((k + 1) % 3);
        const double* b = c + 3 * ((k + 2) % 3);
        const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
        w[k] = std::fabs(det) / std::sqrt(x * x + y * y + z * z);
    }
}

// g_k = max(1, floor(w_k / (r_search (1 + 1e-9)))), each at most kMaxGrid, the largest lowered until the product fits `cap` cells
void cell_grid(const double w[3], double rs, int cap, int g[3])
{
    for (int k = 0; k < 3; ++k) {
        const double f = std::floor(w[k] / (rs * kGuard));
        g[k] = f >= (double)kMaxGrid ? kMaxGrid : f >= 1.0 ? (int)f : 1;
    }
    while ((long long)g[0] * g[1] * g[2] > cap) {
        int k = 0;
        if (g[1] > g[k]) k = 1;
        if (g[2] > g[k]) k = 2;
        --g[k];
    }
}

int check_scalars(const char* who, int nboxes, int n, double rs, double rl)
{
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    if (!(rs > 0.0) || !std::isfinite(rs)) return fail("%s: r_search = %g bohr is not a finite radius > 0", who, rs);
    if (!(rl > 0.0) || !std::isfinite(rl)) return fail("%s: r_lsi = %g bohr is not a finite radius > 0", who, rl);
    if (!(rl <= rs)) return fail("%s: r_lsi = %.17g bohr is beyond r_search = %.17g bohr (0 < r_lsi <= r_search is required)", who, rl, rs);
    return 0;
}

// Every box's cell: invertible, and no narrower than r_search (1 + 1e-9).  Fills par [nboxes][18] and grid [nboxes][4].
int check_cells(const char* who, int nboxes, int n, const double* cells, double rs, std::vector<double>& par, std::vector<int>& grid)
{
    par.resize(18 * (size_t)nboxes);
    grid.resize(4 * (size_t)nboxes);
    const int cap = make_layout(n).cap;
    for (int b = 0; b < nboxes; ++b) {
        const double* c = cells + 9 * (size_t)b;
        double* P = par.data() + 18 * (size_t)b;
        double det, w[3];
        if (!invert_cell(c, P + 9, &det))
            return fail("%s: cells: the determinant of box %d is %g (zero or not finite)", who, b, det);
        memcpy(P, c, 9 * sizeof(double));
        cell_widths(c, det, w);
        const double wmin = std::fmin(w[0], std::fmin(w[1], w[2]));
        if (!(rs * kGuard <= wmin))
            return fail("%s: r_search = %.17g bohr is beyond the narrowest width %.17g bohr of box %d (r_search (1 + 1e-9) <= every cell "
                        "width is required)", who, rs, wmin, b);
        int* G = grid.data() + 4 * (size_t)b;
        cell_grid(w, rs, cap, G);
        G[3] = G[0] * G[1] * G[2];
    }
    return 0;
}

int check_live(const char* who) { return check_live(who, "mw_tet_init", g); }

dim3 per_molecule(int n, int nb) { return dim3((unsigned)((n + kThreads - 1) / kThreads), (unsigned)nb); }

// The work of both entries, arguments already checked.  par and grid are on the host; pos and the outputs are device pointers
// when `dev`, host pointers otherwise.
int run(const char* who, int nboxes, int n, const std::vector<double>& par, const std::vector<int>& grid, const double* pos, double rs,
        double rl, bool dev, double* order, int* near_, int* counts, double* summary)
{
    Plan p;
    if (make_plan(who, n, nboxes, g.budget, p)) return 1;
    const Layout& l = p.lay;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (!p.small && reserve(g.scratch, p.per_box * (size_t)p.bpc)) return 1;
    if (reserve(g.par, par.size() * sizeof(double))) return 1;
    if (reserve(g.grid, grid.size() * sizeof(int))) return 1;
    HIPOK(hipMemcpyAsync(g.par.p, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPOK(hipMemcpyAsync(g.grid.p, grid.data(), grid.size() * sizeof(int), hipMemcpyHostToDevice, g.stream));
    if (!dev) {
        if (reserve(g.pos, 24 * (size_t)n * p.bpc)) return 1;
        if (order && reserve(g.order, 32 * (size_t)n * p.bpc)) return 1;
        if (near_ && reserve(g.near_, 16 * (size_t)n * p.bpc)) return 1;
        if (counts && reserve(g.counts, 8 * (size_t)n * p.bpc)) return 1;
        if (summary && reserve(g.summary, 8 * (size_t)kSums * p.bpc)) return 1;
    }
    if (!p.small && !summary && reserve(g.summary, 8 * (size_t)kSums * p.bpc)) return 1;     // the summary pass always runs
    const double rs2 = rs * rs, rl2 = rl * rl;
    float ms[3] = {0.0f, 0.0f, 0.0f};
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const double* d_pos = pos + 3 * (size_t)n * b0;
        if (!dev) {
            HIPOK(hipMemcpyAsync(g.pos.p, d_pos, 24 * (size_t)n * nb, hipMemcpyHostToDevice, g.stream));
            d_pos = (const double*)g.pos.p;
        }
        const double* d_par = (const double*)g.par.p + 18 * (size_t)b0;
        const int* d_grid = (const int*)g.grid.p + 4 * (size_t)b0;
        double* d_order = !order ? nullptr : dev ? order + 4 * (size_t)n * b0 : (double*)g.order.p;
        int* d_near = !near_ ? nullptr : dev ? near_ + 4 * (size_t)n * b0 : (int*)g.near_.p;
        int* d_counts = !counts ? nullptr : dev ? counts + 2 * (size_t)n * b0 : (int*)g.counts.p;
        double* d_sum = !summary ? nullptr : dev ? summary + kSums * (size_t)b0 : (double*)g.summary.p;
        if (p.small) {
            HIPOK(hipEventRecord(g.ev[0], g.stream));
            hipLaunchKernelGGL(k_tet_small, dim3((unsigned)((nb + kSmallBoxesPerWg - 1) / kSmallBoxesPerWg)), dim3(kThreads), 0, g.stream,
                               nb, n, rs2, rl2, d_par, d_pos, d_order, d_near, d_counts, d_sum);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[1], g.stream));
        } else {
            if (!d_sum) d_sum = (double*)g.summary.p;
            char* base = (char*)g.scratch.p;
            const size_t B = (size_t)p.bpc;
            double* su = (double*)(base + l.su * B);
            int* cid = (int*)(base + l.cid * B);
            int* tmp = (int*)(base + l.tmp * B);
            int* cnt = (int*)(base + l.cnt * B);
            int* start = (int*)(base + l.start * B);
            int* idx = (int*)(base + l.idx * B);
            double* ss = (double*)(base + l.ss * B);
            double* ord = (double*)(base + l.ord * B);
            const dim3 grid_m = per_molecule(n, nb);
            HIPOK(hipEventRecord(g.ev[0], g.stream));
            HIPOK(hipMemsetAsync(cnt, 0, 4 * ((size_t)l.cap + 1) * nb, g.stream));
            hipLaunchKernelGGL(k_tet_bin, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, d_par, d_grid, d_pos, su, cid, cnt);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_tet_scan, dim3((unsigned)nb), dim3(kThreads), 0, g.stream, l.cap, d_grid, (const int*)cnt, start);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_tet_place, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, (const int*)cid, (const int*)start, cnt, tmp);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_tet_rank, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, (const int*)cid, (const int*)start, (const int*)tmp,
                               (const double*)su, idx, ss);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[1], g.stream));
            hipLaunchKernelGGL(k_tet_select, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, rs2, rl2, d_par, d_grid, (const int*)start,
                               (const double*)ss, (const int*)idx, ord, d_order, d_near, d_counts);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[2], g.stream));
            hipLaunchKernelGGL(k_tet_summary, dim3((unsigned)nb), dim3(kThreads), 0, g.stream, n, (const double*)ord, d_sum);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[3], g.stream));
        }
        if (!dev) {
            if (order) HIPOK(hipMemcpyAsync(order + 4 * (size_t)n * b0, g.order.p, 32 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (near_) HIPOK(hipMemcpyAsync(near_ + 4 * (size_t)n * b0, g.near_.p, 16 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (counts) HIPOK(hipMemcpyAsync(counts + 2 * (size_t)n * b0, g.counts.p, 8 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (summary) HIPOK(hipMemcpyAsync(summary + kSums * (size_t)b0, g.summary.p, 8 * (size_t)kSums * nb, hipMemcpyDeviceToHost, g.stream));
        }
        HIPOK(hipStreamSynchronize(g.stream));               // the next chunk reuses the scratch and the staging buffers
        if (p.small) {
            float t = 0.0f;
            HIPOK(hipEventElapsedTime(&t, g.ev[0], g.ev[1]));
            ms[1] += t;
        } else {
            for (int k = 0; k < 3; ++k) {
                float t = 0.0f;
                HIPOK(hipEventElapsedTime(&t, g.ev[k], g.ev[k + 1]));
                ms[k] += t;
            }
        }
    }
    plan_fields(p, grid.data(), g.last);
    g.have_last = true;
    for (int k = 0; k < 3; ++k) g.ms[k] = ms[k];
    return 0;
}

}  // namespace

extern "C" {

const char* mw_tet_last_error(void) { return g_err; }
int mw_tet_is_initialised(void) { return g.live ? 1 : 0; }

int mw_tet_init(int device) { return runtime_init("mw_tet_init", "MW_TET_SCRATCH_MB", device, g); }

int mw_tet_finalize(void)
{
    if (runtime_finalize(g, {&g.scratch, &g.par, &g.grid, &g.pos, &g.order, &g.near_, &g.counts, &g.summary})) return 1;
    g = State{};
    return 0;
}

int mw_tet_compute(int nboxes, int nwater, const double* cells, const double* pos, double r_search, double r_lsi, double* order, int* near_,
                   int* counts, double* summary)
{
    const char* who = "mw_tet_compute";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, r_search, r_lsi)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (check_cells(who, nboxes, nwater, cells, r_search, par, grid)) return 1;
    if (check_live(who)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, r_search, r_lsi, false, order, near_, counts, summary);
}

int mw_tet_compute_device(int nboxes, int nwater, const double* cells, const double* pos, double r_search, double r_lsi, double* order,
                          int* near_, int* counts, double* summary)
{
    const char* who = "mw_tet_compute_device";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, r_search, r_lsi)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    HIPOK(hipDeviceSynchronize());                            // whoever made the inputs (another stream, PyTorch's) is done
    std::vector<double> h_cells(9 * (size_t)nboxes);
    HIPOK(hipMemcpy(h_cells.data(), cells, h_cells.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (check_cells(who, nboxes, nwater, h_cells.data(), r_search, par, grid)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, r_search, r_lsi, true, order, near_, counts, summary);
}

int mw_tet_plan(int nwater, const double* cell, double r_search, int nboxes, int* out, int nout)
{
    const char* who = "mw_tet_plan";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, r_search, r_search)) return 1;
    if (!cell) return fail("%s: cell is NULL", who);
    if (!out || nout < 1) return fail("%s: out is NULL or nout < 1", who);
    if (check_cells(who, 1, nwater, cell, r_search, par, grid)) return 1;
    Plan p;
    if (make_plan(who, nwater, nboxes, g.live ? g.budget : kDefaultBudget, p)) return 1;
    int f[MW_TET_PLAN_FIELDS];
    plan_fields(p, grid.data(), f);
    copy_fields(f, MW_TET_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_tet_last(int* out, int nout)
{
    if (check_live("mw_tet_last")) return 1;
    if (!out || nout < 1) return fail("mw_tet_last: out is NULL or nout < 1");
    if (!g.have_last) return fail("mw_tet_last: no call has launched yet");
    copy_fields(g.last, MW_TET_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_tet_elapsed_ms(float* binning, float* select, float* summary)
{
    if (check_live("mw_tet_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_tet_elapsed_ms: no call has launched yet");
    if (binning) *binning = g.ms[0];
    if (select) *select = g.ms[1];
    if (summary) *summary = g.ms[2];
    return 0;
}

}  // extern "C"
