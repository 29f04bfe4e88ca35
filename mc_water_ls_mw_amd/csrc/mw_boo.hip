// libmw_boo.so -- the Steinhardt bond-order parameters of include/mw_boo.h: q4, q6, their neighbour averages, the solid-like
// connection count of every molecule and the box summary (Q4, Q6, <qbar4>, <qbar6>), for many boxes.  General geometry
// (nwater > 64): a counting sort into a fractional cell grid (k_boo_bin, k_boo_scan, k_boo_place, k_boo_rank), then one
// lane per molecule in sorted order walks the 27 neighbouring cells twice -- k_boo_pass1 for n_i and the 22 harmonic sums,
// k_boo_pass2 for the neighbours' vectors -- and k_boo_summary adds the box up.  Small geometry (nwater <= 64): k_boo_small,
// one wavefront per box with the box in LDS.  Every bit of a box's results depends on the box, rc and the threshold alone
// (mw_boo.h): the arithmetic below is spelled out in fma / mul / add with contraction off, and the order of every sum is fixed.
#include "../../include/mw_boo.h"

#include "mw_common.hip.h"

#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too

namespace mwboo {

constexpr int kThreads = 256;
constexpr int kSmallN = 64;
constexpr int kSmallBoxesPerWg = kThreads / 64;   // one wavefront per box
constexpr int kNY = 22;                           // 9 components of l = 4, then 13 of l = 6
constexpr int kRec = 24;                          // doubles per molecule in scratch: q_lm, |q_6|, n_i
constexpr int kSums = 25;                         // box sums: 22 of n_i q_lm, sum n_i, sum qbar4, sum qbar6
constexpr int kMaxGrid = 1024;
constexpr int kMaxWater = 1 << 22;
constexpr int kMaxBoxes = 1 << 24;
constexpr int kMaxChunkBoxes = 65535;             // grid y
constexpr int kSmallChunkBoxes = 1 << 20;
constexpr double kGuard = 1.0 + 1e-9;
constexpr int kSmallLds = kSmallBoxesPerWg * (3 + kRec) * 64 * 8;

// c_lm = sqrt((2 - delta_m0) (l - m)! / (l + m)!)
constexpr double k41 = 0.31622776601683794, k42 = 0.07453559924999299, k43 = 0.019920476822239894, k44 = 0.0070429521227376385;
constexpr double k61 = 0.21821789023599236, k62 = 0.03450327796711771, k63 = 0.005750546327852952, k64 = 0.00104990131391452,
                 k65 = 0.00022383971222927231, k66 = 6.461695905544936e-05;

// The 22 components of the unit vector (x, y, z): c_lm P_l^(m)(z) Re / Im (x + i y)^m, order (l = 4: m = 0, 1c, 1s, ... 4c, 4s; l = 6
// likewise).  sum_m Y_lm(u) Y_lm(v) = P_l(u . v).
__device__ __forceinline__ void harmonics(double x, double y, double z, double (&Y)[kNY])
{
    const double z2 = z * z;
    const double c2 = __builtin_fma(x, x, -(y * y)), s2 = 2.0 * (x * y);
    const double c3 = __builtin_fma(c2, x, -(s2 * y)), s3 = __builtin_fma(c2, y, s2 * x);
    const double c4 = __builtin_fma(c3, x, -(s3 * y)), s4 = __builtin_fma(c3, y, s3 * x);
    const double c5 = __builtin_fma(c4, x, -(s4 * y)), s5 = __builtin_fma(c4, y, s4 * x);
    const double c6 = __builtin_fma(c5, x, -(s5 * y)), s6 = __builtin_fma(c5, y, s5 * x);
    const double p41 = z * __builtin_fma(17.5 * k41, z2, -7.5 * k41);
    const double p42 = __builtin_fma(52.5 * k42, z2, -7.5 * k42);
    const double p43 = (105.0 * k43) * z;
    Y[0] = __builtin_fma(__builtin_fma(4.375, z2, -3.75), z2, 0.375);
    Y[1] = p41 * x;  Y[2] = p41 * y;
    Y[3] = p42 * c2; Y[4] = p42 * s2;
    Y[5] = p43 * c3; Y[6] = p43 * s3;
    Y[7] = (105.0 * k44) * c4; Y[8] = (105.0 * k44) * s4;
    const double p61 = z * __builtin_fma(__builtin_fma(86.625 * k61, z2, -78.75 * k61), z2, 13.125 * k61);
    const double p62 = __builtin_fma(__builtin_fma(433.125 * k62, z2, -236.25 * k62), z2, 13.125 * k62);
    const double p63 = z * __builtin_fma(1732.5 * k63, z2, -472.5 * k63);
    const double p64 = __builtin_fma(5197.5 * k64, z2, -472.5 * k64);
    const double p65 = (10395.0 * k65) * z;
    Y[9] = __builtin_fma(__builtin_fma(__builtin_fma(14.4375, z2, -19.6875), z2, 6.5625), z2, -0.3125);
    Y[10] = p61 * x;  Y[11] = p61 * y;
    Y[12] = p62 * c2; Y[13] = p62 * s2;
    Y[14] = p63 * c3; Y[15] = p63 * s3;
    Y[16] = p64 * c4; Y[17] = p64 * s4;
    Y[18] = p65 * c5; Y[19] = p65 * s5;
    Y[20] = (10395.0 * k66) * c6; Y[21] = (10395.0 * k66) * s6;
}

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

__device__ __forceinline__ void unit_harmonics(double r2, double dx, double dy, double dz, double (&Y)[kNY])
{
    const double rinv = 1.0 / __builtin_sqrt(r2);
    harmonics(dx * rinv, dy * rinv, dz * rinv, Y);
}

__device__ __forceinline__ double norm_of(const double* v, int first, int count)
{
    double s = 0.0;
    for (int k = first; k < first + count; ++k) s = __builtin_fma(v[k], v[k], s);
    return __builtin_sqrt(s);
}

// Offset o in {-1, 0, 1} from cell c of g: the cell it lands in and the image shift that goes with it.
__device__ __forceinline__ void wrap_cell(int c, int o, int g, int& cw, double& shift)
{
    cw = c + o; shift = 0.0;
    if (cw < 0) { cw += g; shift = -1.0; }
    if (cw >= g) { cw -= g; shift = 1.0; }
}

// ---- general geometry ----------------------------------------------------------------------------------------------------
// par[box][18]: the cell (9) and its inverse (9).  grid[box][4]: g_1, g_2, g_3, cells.  Per box in scratch: su [n][3] fractional
// positions by index, cid [n], tmp [n] (members of the cells in arrival order), cnt / start [cap + 1]; then in cell order:
// idx [n] the molecule, ss [n][3], rec [n][kRec], qbar [n][2].

// One lane per molecule: s, its cell, the cell's count.
__global__ __launch_bounds__(kThreads) void k_boo_bin(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
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
__global__ __launch_bounds__(kThreads) void k_boo_scan(int cap, const int* __restrict__ grid, const int* __restrict__ cnt, int* __restrict__ start)
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

// One lane per molecule: a place among its cell's members, in arrival order (k_boo_rank puts them in index order).
__global__ __launch_bounds__(kThreads) void k_boo_place(int n, int cap, const int* __restrict__ cid, const int* __restrict__ start,
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
__global__ __launch_bounds__(kThreads) void k_boo_rank(int n, int cap, const int* __restrict__ cid, const int* __restrict__ start,
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

// The walk both passes share: calls hit(q, r2, dx, dy, dz) for every entry of the molecule at sorted place p, in the
// contract's order.
template <typename Hit>
__device__ __forceinline__ void walk_cells(int p, double rc2, const double* __restrict__ H, const int* __restrict__ g, const int* __restrict__ st,
                                           const double* __restrict__ S, Hit hit)
{
    const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
    const int g0 = g[0], g1 = g[1], g2 = g[2];
    const int c0 = cell_of(s0, g0), c1 = cell_of(s1, g1), c2 = cell_of(s2, g2);
    for (int oz = -1; oz <= 1; ++oz) {
        int wz; double hz;
        wrap_cell(c2, oz, g2, wz, hz);
        for (int oy = -1; oy <= 1; ++oy) {
            int wy; double hy;
            wrap_cell(c1, oy, g1, wy, hy);
            for (int ox = -1; ox <= 1; ++ox) {
                int wx; double hx;
                wrap_cell(c0, ox, g0, wx, hx);
                const int c = (wz * g1 + wy) * g0 + wx;
                const int q1 = st[c + 1];
                for (int q = st[c]; q < q1; ++q) {
                    const double a0 = (S[3 * (size_t)q] - s0) + hx, a1 = (S[3 * (size_t)q + 1] - s1) + hy, a2 = (S[3 * (size_t)q + 2] - s2) + hz;
                    double dx, dy, dz;
                    const double r2 = bond_vector(H, a0, a1, a2, dx, dy, dz);
                    if (r2 < rc2 && r2 > 0.0) hit(q, r2, dx, dy, dz);
                }
            }
        }
    }
}

// Pass 1, one lane per molecule in sorted order: n_i and q_lm(i) into rec.
__global__ __launch_bounds__(kThreads) void k_boo_pass1(int n, int cap, double rc2, const double* __restrict__ par, const int* __restrict__ grid,
                                                        const int* __restrict__ start, const double* __restrict__ ss, double* __restrict__ rec)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    double acc[kNY];
#pragma unroll
    for (int k = 0; k < kNY; ++k) acc[k] = 0.0;
    int cnt = 0;
    walk_cells(p, rc2, par + 18 * (size_t)b, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), ss + 3 * (size_t)b * n,
               [&](int, double r2, double dx, double dy, double dz) {
                   double Y[kNY];
                   unit_harmonics(r2, dx, dy, dz, Y);
#pragma unroll
                   for (int k = 0; k < kNY; ++k) acc[k] = acc[k] + Y[k];
                   ++cnt;
               });
    double* r = rec + kRec * ((size_t)b * n + p);
    const double m = (double)cnt;
#pragma unroll
    for (int k = 0; k < kNY; ++k) acc[k] = cnt ? acc[k] / m : 0.0;
    const double n6 = norm_of(acc, 9, 13);
#pragma unroll
    for (int k = 0; k < kNY; ++k) r[k] = acc[k];
    r[22] = n6;
    r[23] = m;
}

// Pass 2, the same walk: the neighbours' vectors for qbar and the connections; the outputs by molecule index.
__global__ __launch_bounds__(kThreads) void k_boo_pass2(int n, int cap, double rc2, double thr, const double* __restrict__ par,
                                                        const int* __restrict__ grid, const int* __restrict__ start, const double* __restrict__ ss,
                                                        const int* __restrict__ idx, const double* __restrict__ rec, double* __restrict__ qbar,
                                                        double* __restrict__ q, int* __restrict__ nn)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const double* R = rec + kRec * (size_t)b * n;
    double own[kRec], bar[kNY];
#pragma unroll
    for (int k = 0; k < kRec; ++k) own[k] = R[kRec * (size_t)p + k];
#pragma unroll
    for (int k = 0; k < kNY; ++k) bar[k] = own[k];
    int conn = 0;
    walk_cells(p, rc2, par + 18 * (size_t)b, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), ss + 3 * (size_t)b * n,
               [&](int j, double, double, double, double) {
                   const double* rj = R + kRec * (size_t)j;
                   double dot = 0.0;
#pragma unroll
                   for (int k = 0; k < kNY; ++k) {
                       const double v = rj[k];
                       bar[k] = bar[k] + v;
                       if (k >= 9) dot = __builtin_fma(own[k], v, dot);
                   }
                   const double den = own[22] * rj[22];
                   if (den > 0.0 && dot / den > thr) ++conn;
               });
    const double m = own[23] + 1.0;
#pragma unroll
    for (int k = 0; k < kNY; ++k) bar[k] = bar[k] / m;
    const double b4 = norm_of(bar, 0, 9), b6 = norm_of(bar, 9, 13);
    const size_t o = (size_t)b * n;
    qbar[2 * (o + p)] = b4; qbar[2 * (o + p) + 1] = b6;
    const size_t i = o + idx[o + p];
    if (q) { q[4 * i] = norm_of(own, 0, 9); q[4 * i + 1] = own[22]; q[4 * i + 2] = b4; q[4 * i + 3] = b6; }
    if (nn) { nn[2 * i] = (int)own[23]; nn[2 * i + 1] = conn; }
}

// (Q4, Q6, <qbar4>, <qbar6>) from the box sums t[kSums]
__device__ __forceinline__ void write_summary(const double* t, int n, double* out)
{
    double Q[kNY];
    for (int k = 0; k < kNY; ++k) Q[k] = t[22] > 0.0 ? t[k] / t[22] : 0.0;
    out[0] = norm_of(Q, 0, 9); out[1] = norm_of(Q, 9, 13);
    out[2] = t[23] / (double)n; out[3] = t[24] / (double)n;
}

// One workgroup per box: lane t adds the sorted places t, t + 256, ... in that order, a fixed tree adds the lanes of a
// wavefront and thread 0 the four wavefronts in order.
__global__ __launch_bounds__(kThreads) void k_boo_summary(int n, const double* __restrict__ rec, const double* __restrict__ qbar, double* __restrict__ summary)
{
    __shared__ double part[kThreads / 64][kSums];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* R = rec + kRec * (size_t)b * n;
    const double* B = qbar + 2 * (size_t)b * n;
    double t[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) t[k] = 0.0;
    for (int p = tid; p < n; p += kThreads) {
        const double* r = R + kRec * (size_t)p;
        const double m = r[23];
#pragma unroll
        for (int k = 0; k < kNY; ++k) t[k] = t[k] + m * r[k];
        t[22] = t[22] + m;
        t[23] = t[23] + B[2 * (size_t)p];
        t[24] = t[24] + B[2 * (size_t)p + 1];
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
        write_summary(tot, n, summary + 4 * (size_t)b);
    }
}

// ---- small geometry: one wavefront per box, lane i = molecule i, the box's fractional positions and records in LDS ---------
// The entries of i: j in index order, and for each j the eight combinations of ds_k and ds_k -/+ 1 (the only two images per
// axis that can come within rc <= w_k), combination bit k choosing the second along axis k.
template <typename Hit>
__device__ __forceinline__ void walk_small(int n, bool active, double rc2, const double* __restrict__ H, const double* S, double s0, double s1,
                                           double s2, Hit hit)
{
    for (int j = 0; j < n; ++j) {
        const double e0 = S[j] - s0, e1 = S[64 + j] - s1, e2 = S[128 + j] - s2;
        const double f0 = e0 > 0.0 ? e0 - 1.0 : e0 + 1.0, f1 = e1 > 0.0 ? e1 - 1.0 : e1 + 1.0, f2 = e2 > 0.0 ? e2 - 1.0 : e2 + 1.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            double dx, dy, dz;
            const double r2 = bond_vector(H, (c & 1) ? f0 : e0, (c & 2) ? f1 : e1, (c & 4) ? f2 : e2, dx, dy, dz);
            if (active && r2 < rc2 && r2 > 0.0) hit(j, r2, dx, dy, dz);
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_boo_small(int nb, int n, double rc2, double thr, const double* __restrict__ par,
                                                        const double* __restrict__ pos, double* __restrict__ q, int* __restrict__ nn,
                                                        double* __restrict__ summary)
{
    __shared__ double lds[kSmallBoxesPerWg][(3 + kRec) * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * kSmallBoxesPerWg + wave;
    if (b >= nb) return;                                   // the whole wavefront; no workgroup barrier below
    double* S = lds[wave];
    double* R = S + 3 * 64;                                // R[k * 64 + j]
    const double* H = par + 18 * (size_t)b;
    const bool active = lane < n;
    const size_t m = (size_t)b * n + (active ? lane : 0);
    const double s0 = frac_coord(H + 9, 0, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s1 = frac_coord(H + 9, 1, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s2 = frac_coord(H + 9, 2, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    S[lane] = s0; S[64 + lane] = s1; S[128 + lane] = s2;
    mw::wave_fence();

    double own[kRec];
#pragma unroll
    for (int k = 0; k < kNY; ++k) own[k] = 0.0;
    int cnt = 0;
    walk_small(n, active, rc2, H, S, s0, s1, s2, [&](int, double r2, double dx, double dy, double dz) {
        double Y[kNY];
        unit_harmonics(r2, dx, dy, dz, Y);
#pragma unroll
        for (int k = 0; k < kNY; ++k) own[k] = own[k] + Y[k];
        ++cnt;
    });
    const double mi = (double)cnt;
#pragma unroll
    for (int k = 0; k < kNY; ++k) own[k] = cnt ? own[k] / mi : 0.0;
    own[22] = norm_of(own, 9, 13);
    own[23] = mi;
#pragma unroll
    for (int k = 0; k < kRec; ++k) R[k * 64 + lane] = own[k];
    mw::wave_fence();

    double bar[kNY];
#pragma unroll
    for (int k = 0; k < kNY; ++k) bar[k] = own[k];
    int conn = 0;
    walk_small(n, active, rc2, H, S, s0, s1, s2, [&](int j, double, double, double, double) {
        double dot = 0.0;
#pragma unroll
        for (int k = 0; k < kNY; ++k) {
            const double v = R[k * 64 + j];
            bar[k] = bar[k] + v;
            if (k >= 9) dot = __builtin_fma(own[k], v, dot);
        }
        const double den = own[22] * R[22 * 64 + j];
        if (den > 0.0 && dot / den > thr) ++conn;
    });
    const double m1 = mi + 1.0;
#pragma unroll
    for (int k = 0; k < kNY; ++k) bar[k] = bar[k] / m1;
    const double b4 = norm_of(bar, 0, 9), b6 = norm_of(bar, 9, 13);
    if (active) {
        if (q) { q[4 * m] = norm_of(own, 0, 9); q[4 * m + 1] = own[22]; q[4 * m + 2] = b4; q[4 * m + 3] = b6; }
        if (nn) { nn[2 * m] = cnt; nn[2 * m + 1] = conn; }
    }
    if (summary) {                                         // wave-uniform: lanes beyond n add +0.0
        double t[kSums];
#pragma unroll
        for (int k = 0; k < kNY; ++k) t[k] = mw::wave_sum(active ? mi * own[k] : 0.0);
        t[22] = mw::wave_sum(active ? mi : 0.0);
        t[23] = mw::wave_sum(active ? b4 : 0.0);
        t[24] = mw::wave_sum(active ? b6 : 0.0);
        if (lane == 0) write_summary(t, n, summary + 4 * (size_t)b);
    }
}

}  // namespace mwboo

namespace {

using namespace mwboo;

struct State : Runtime<5> {
    Buf scratch, par, grid, pos, q, nn, summary;
    int last[MW_BOO_PLAN_FIELDS] = {0};
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
} g;

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// The scratch of one box of the general geometry, piece by piece (byte offsets inside a chunk are these times boxes per chunk).
struct Layout {
    int cap;                                                // cells a box may have
    size_t su, cid, tmp, cnt, start, idx, ss, rec, qbar, per_box;
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
    l.rec = o;   o += align16(8 * (size_t)kRec * n);
    l.qbar = o;  o += align16(16 * (size_t)n);
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
            return fail("%s: one box needs %zu bytes of scratch (nwater = %d) and does not fit the budget of %zu bytes (MW_BOO_SCRATCH_MB)",
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

// g_k = max(1, floor(w_k / (rc (1 + 1e-9)))), each at most kMaxGrid, the largest lowered until the product fits `cap` cells
void cell_grid(const double w[3], double rc, int cap, int g[3])
{
    for (int k = 0; k < 3; ++k) {
        const double f = std::floor(w[k] / (rc * kGuard));
        g[k] = f >= (double)kMaxGrid ? kMaxGrid : f >= 1.0 ? (int)f : 1;
    }
    while ((long long)g[0] * g[1] * g[2] > cap) {
        int k = 0;
        if (g[1] > g[k]) k = 1;
        if (g[2] > g[k]) k = 2;
        --g[k];
    }
}

int check_scalars(const char* who, int nboxes, int n, double rc, double threshold)
{
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    if (!(rc > 0.0) || !std::isfinite(rc)) return fail("%s: rc = %g bohr is not a finite cutoff > 0 (box 0)", who, rc);
    if (!(threshold >= -1.0 && threshold <= 1.0)) return fail("%s: threshold = %g outside [-1, 1]", who, threshold);
    return 0;
}

// Every box's cell: invertible, and no narrower than rc (1 + 1e-9).  Fills par [nboxes][18] and grid [nboxes][4].
int check_cells(const char* who, int nboxes, int n, const double* cells, double rc, std::vector<double>& par, std::vector<int>& grid)
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
        if (!(rc * kGuard <= wmin))
            return fail("%s: rc = %.17g bohr is beyond the narrowest width %.17g bohr of box %d (rc (1 + 1e-9) <= every cell width is required)",
                        who, rc, wmin, b);
        int* G = grid.data() + 4 * (size_t)b;
        cell_grid(w, rc, cap, G);
        G[3] = G[0] * G[1] * G[2];
    }
    return 0;
}

int check_live(const char* who) { return check_live(who, "mw_boo_init", g); }

dim3 per_molecule(int n, int nb) { return dim3((unsigned)((n + kThreads - 1) / kThreads), (unsigned)nb); }

// The work of both entries, arguments already checked.  par and grid are on the host; pos and the outputs are device pointers
// when `dev`, host pointers otherwise.
int run(const char* who, int nboxes, int n, const std::vector<double>& par, const std::vector<int>& grid, const double* pos, double rc,
        double thr, bool dev, double* q, int* nn, double* summary)
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
        if (q && reserve(g.q, 32 * (size_t)n * p.bpc)) return 1;
        if (nn && reserve(g.nn, 8 * (size_t)n * p.bpc)) return 1;
        if (summary && reserve(g.summary, 32 * (size_t)p.bpc)) return 1;
    }
    if (!p.small && !summary && reserve(g.summary, 32 * (size_t)p.bpc)) return 1;          // the summary pass always runs
    const double rc2 = rc * rc;
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const double* d_pos = pos + 3 * (size_t)n * b0;
        if (!dev) {
            HIPOK(hipMemcpyAsync(g.pos.p, d_pos, 24 * (size_t)n * nb, hipMemcpyHostToDevice, g.stream));
            d_pos = (const double*)g.pos.p;
        }
        const double* d_par = (const double*)g.par.p + 18 * (size_t)b0;
        const int* d_grid = (const int*)g.grid.p + 4 * (size_t)b0;
        double* d_q = !q ? nullptr : dev ? q + 4 * (size_t)n * b0 : (double*)g.q.p;
        int* d_nn = !nn ? nullptr : dev ? nn + 2 * (size_t)n * b0 : (int*)g.nn.p;
        double* d_sum = !summary ? nullptr : dev ? summary + 4 * (size_t)b0 : (double*)g.summary.p;
        if (p.small) {
            HIPOK(hipEventRecord(g.ev[0], g.stream));
            hipLaunchKernelGGL(k_boo_small, dim3((unsigned)((nb + kSmallBoxesPerWg - 1) / kSmallBoxesPerWg)), dim3(kThreads), 0, g.stream,
                               nb, n, rc2, thr, d_par, d_pos, d_q, d_nn, d_sum);
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
            double* rec = (double*)(base + l.rec * B);
            double* qbar = (double*)(base + l.qbar * B);
            const dim3 grid_m = per_molecule(n, nb);
            HIPOK(hipEventRecord(g.ev[0], g.stream));
            HIPOK(hipMemsetAsync(cnt, 0, 4 * ((size_t)l.cap + 1) * nb, g.stream));
            hipLaunchKernelGGL(k_boo_bin, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, d_par, d_grid, d_pos, su, cid, cnt);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_boo_scan, dim3((unsigned)nb), dim3(kThreads), 0, g.stream, l.cap, d_grid, (const int*)cnt, start);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_boo_place, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, (const int*)cid, (const int*)start, cnt, tmp);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_boo_rank, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, (const int*)cid, (const int*)start, (const int*)tmp,
                               (const double*)su, idx, ss);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[1], g.stream));
            hipLaunchKernelGGL(k_boo_pass1, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, rc2, d_par, d_grid, (const int*)start, (const double*)ss, rec);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[2], g.stream));
            hipLaunchKernelGGL(k_boo_pass2, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, rc2, thr, d_par, d_grid, (const int*)start, (const double*)ss,
                               (const int*)idx, (const double*)rec, qbar, d_q, d_nn);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[3], g.stream));
            hipLaunchKernelGGL(k_boo_summary, dim3((unsigned)nb), dim3(kThreads), 0, g.stream, n, (const double*)rec, (const double*)qbar, d_sum);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[4], g.stream));
        }
        if (!dev) {
            if (q) HIPOK(hipMemcpyAsync(q + 4 * (size_t)n * b0, g.q.p, 32 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (nn) HIPOK(hipMemcpyAsync(nn + 2 * (size_t)n * b0, g.nn.p, 8 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (summary) HIPOK(hipMemcpyAsync(summary + 4 * (size_t)b0, g.summary.p, 32 * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
        }
        HIPOK(hipStreamSynchronize(g.stream));               // the next chunk reuses the scratch and the staging buffers
        if (p.small) {
            float t = 0.0f;
            HIPOK(hipEventElapsedTime(&t, g.ev[0], g.ev[1]));
            ms[1] += t;
        } else {
            for (int k = 0; k < 4; ++k) {
                float t = 0.0f;
                HIPOK(hipEventElapsedTime(&t, g.ev[k], g.ev[k + 1]));
                ms[k] += t;
            }
        }
    }
    plan_fields(p, grid.data(), g.last);
    g.have_last = true;
    for (int k = 0; k < 4; ++k) g.ms[k] = ms[k];
    return 0;
}

}  // namespace

extern "C" {

const char* mw_boo_last_error(void) { return g_err; }
int mw_boo_is_initialised(void) { return g.live ? 1 : 0; }

int mw_boo_init(int device) { return runtime_init("mw_boo_init", "MW_BOO_SCRATCH_MB", device, g); }

int mw_boo_finalize(void)
{
    if (runtime_finalize(g, {&g.scratch, &g.par, &g.grid, &g.pos, &g.q, &g.nn, &g.summary})) return 1;
    g = State{};
    return 0;
}

int mw_boo_compute(int nboxes, int nwater, const double* cells, const double* pos, double rc, double threshold, double* q, int* nn,
                   double* summary)
{
    const char* who = "mw_boo_compute";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, rc, threshold)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (check_cells(who, nboxes, nwater, cells, rc, par, grid)) return 1;
    if (check_live(who)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, rc, threshold, false, q, nn, summary);
}

int mw_boo_compute_device(int nboxes, int nwater, const double* cells, const double* pos, double rc, double threshold, double* q, int* nn,
                          double* summary)
{
    const char* who = "mw_boo_compute_device";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, rc, threshold)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    HIPOK(hipDeviceSynchronize());                            // whoever made the inputs (another stream, PyTorch's) is done
    std::vector<double> h_cells(9 * (size_t)nboxes);
    HIPOK(hipMemcpy(h_cells.data(), cells, h_cells.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (check_cells(who, nboxes, nwater, h_cells.data(), rc, par, grid)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, rc, threshold, true, q, nn, summary);
}

int mw_boo_plan(int nwater, const double* cell, double rc, int nboxes, int* out, int nout)
{
    const char* who = "mw_boo_plan";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, rc, 0.0)) return 1;
    if (!cell) return fail("%s: cell is NULL", who);
    if (!out || nout < 1) return fail("%s: out is NULL or nout < 1", who);
    if (check_cells(who, 1, nwater, cell, rc, par, grid)) return 1;
    Plan p;
    if (make_plan(who, nwater, nboxes, g.live ? g.budget : kDefaultBudget, p)) return 1;
    int f[MW_BOO_PLAN_FIELDS];
    plan_fields(p, grid.data(), f);
    copy_fields(f, MW_BOO_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_boo_last(int* out, int nout)
{
    if (check_live("mw_boo_last")) return 1;
    if (!out || nout < 1) return fail("mw_boo_last: out is NULL or nout < 1");
    if (!g.have_last) return fail("mw_boo_last: no call has launched yet");
    copy_fields(g.last, MW_BOO_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_boo_elapsed_ms(float* binning, float* pass1, float* pass2, float* summary)
{
    if (check_live("mw_boo_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_boo_elapsed_ms: no call has launched yet");
    if (binning) *binning = g.ms[0];
    if (pass1) *pass1 = g.ms[1];
    if (pass2) *pass2 = g.ms[2];
    if (summary) *summary = g.ms[3];
    return 0;
}

}  // extern "C"
