// libmw_pin.so -- the interface-pinning molecular dynamics of include/mw_pin.h: the step of libmw_flex.so (BAOAB on the full-box mW
// energy, a per-axis stochastic-cell-rescaling barostat, the pressure tensor in every row) restated, with the force of a harmonic
// bias on one collective density mode rho(n) = sum_j exp(2 pi i n.s_j) added to the force that enters stages 1 and 6, and block
// averages of Q, Q^2, V and E taken on the device.  General geometry (nwater > 64), per evaluation: the counting sort of
// mw_lib_cells.h, k_pin_moments (the moments, and for a biased box the phasor (cos, sin) of every molecule, stored in sorted order,
// with the workgroup's two partial sums), k_pin_rho (one wavefront per box: the partials added in workgroup order, then C, S, Q, U_b
// and g k of the box), k_pin_forces (the two walks of mw_lib_forces.h, then one fma per component from the molecule's pair and the
// box's five doubles) and k_pin_row (the row, the trace and the block accumulators).  Small geometry (nwater <= 64): k_pin_small, one
// wavefront per box, C and S by the DPP tree before the kick.  k_pin_baro, k_pin_scale, k_pin_begin and k_pin_finish are those of
// mw_flex.hip.  A box with kappa = 0 takes none of the bias's branches (all uniform over its workgroups) and gets the bits of
// libmw_flex.so.  Freeze flags of a box as in mw_flex.hip.
//
// The short pieces of the step, the cell routine and the barostat are restated from mw_flex.hip as that file restates the MD and NPT
// libraries': a header for them would become a dependency of libraries whose lists of dependencies are part of their contracts.
#include "../../include/mw_pin.h"

#include "mw_common.hip.h"

#include <cstdint>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too
#include "mw_lib_cells.h"
#include "mw_lib_forces.h"

namespace mwpin {

using namespace mwcells;
using namespace mwforces;

constexpr int kSmallBoxesPerWg = kThreads / 64;   // one wavefront per box
constexpr int kSmallLdsPerBox = ((3 + kMom) * 64 + MW_PIN_BLOCK_FIELDS + 64 + 4) * 8;   // s, the moments, the accumulators, w and g k
constexpr int kSmallLds = kSmallBoxesPerWg * kSmallLdsPerBox;
constexpr int kSums = 16;                         // a workgroup's partial sums: E, v.v, |x - ref|^2, W, six hm v_a v_b, six shares of the stress
constexpr int kPart = kSums + 1;                  // those and the largest |F| component
constexpr int kOut = MW_PIN_TRACE_FIELDS;         // doubles of a trace row: E, K, msd, fmax, V, P, six P_ab, three lengths, Q, U_b
constexpr int kRow = kOut + 1;                    // a box's current row: those and W
constexpr int kSI = 8;                            // ints: frozen, first guard, second guard, steps completed, barostat guard (3 spare)
constexpr int kCV = 8;                            // doubles: V, the last three mu, the lengths of the three cell vectors (1 spare)
constexpr int kGeneralLds = (kThreads / 64) * kPart * 8;
constexpr int kPin = 5;                           // doubles of a box's bias, from the host: n_1, n_2, n_3, kappa, the anchor
constexpr int kBias = 8;                          // doubles of a box's mode, from k_pin_rho: C, S, g k (3), Q, U_b, 1.0 (all 0.0 without a bias)
constexpr int kAcc = MW_PIN_BLOCK_FIELDS;         // a box's block accumulators: Q, Q Q, V, E
constexpr double kTwoPi = 6.283185307179586476925286766559;

// The constants of a call, formed on the host (mw_pin.h), and what names its noise.
struct Consts {
    double hk, hd, c1, c2, lim2, hm;
    double cb, cn, pressure;
    double cb3, cn1, cn2;
    uint32_t seed_lo, seed_hi;
    int thermostat, nsteps, sample_every, nrows, baro_noise;
    int coupling, axis;
    int equil, block_steps, nblocks;
};

// ---- the noise (the MD library's, restated) ---------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ double unit_open(uint32_t w) { return ((double)w + 0.5) * 0x1p-32; }      // exact

// xi_x, xi_y, xi_z of molecule `mol` of the box with stream identity `id` at step index `step`
__device__ __forceinline__ void normals(const Consts& C, unsigned long long id, unsigned long long step, uint32_t mol, double& a, double& b, double& c)
{
    uint32_t w[4] = {(uint32_t)step, (uint32_t)(step >> 32), mol, 0u};
    philox4x32_10(w, (uint32_t)id ^ C.seed_lo, (uint32_t)(id >> 32) ^ C.seed_hi);
    const double r0 = __builtin_sqrt(-2.0 * log(unit_open(w[0]))), t0 = kTwoPi * unit_open(w[1]);
    const double r1 = __builtin_sqrt(-2.0 * log(unit_open(w[2]))), t1 = kTwoPi * unit_open(w[3]);
    a = r0 * cos(t0);
    b = r0 * sin(t0);
    c = r1 * cos(t1);
}

// a barostat's normal of the box at step index `step`: the counter (step low, step high, 0xFFFFFFFF, word) is no molecule's;
// word 1 is the isotropic normal (the NPT library's), word 2 + a that of the group whose lowest axis is a
__device__ __forceinline__ double box_normal(const Consts& C, unsigned long long id, unsigned long long step, uint32_t word)
{
    uint32_t w[4] = {(uint32_t)step, (uint32_t)(step >> 32), 0xFFFFFFFFu, word};
    philox4x32_10(w, (uint32_t)id ^ C.seed_lo, (uint32_t)(id >> 32) ^ C.seed_hi);
    return __builtin_sqrt(-2.0 * log(unit_open(w[0]))) * cos(kTwoPi * unit_open(w[1]));
}

// ---- the pieces of a step, one molecule (the MD library's, restated) -----------------------------------------------------------
__device__ __forceinline__ void kick(double hk, double fx, double fy, double fz, double& vx, double& vy, double& vz)
{
    vx = __builtin_fma(hk, fx, vx); vy = __builtin_fma(hk, fy, vy); vz = __builtin_fma(hk, fz, vz);
}
// true when the half drift hd v is beyond a sigma / 4 or not a number
__device__ __forceinline__ bool guard_fails(double hd, double lim2, double vx, double vy, double vz)
{
    const double dx = hd * vx, dy = hd * vy, dz = hd * vz;
    const double d2 = __builtin_fma(dx, dx, __builtin_fma(dy, dy, dz * dz));
    return !(d2 <= lim2);
}
__device__ __forceinline__ void drift(double hd, double vx, double vy, double vz, double& x, double& y, double& z)
{
    const double dx = hd * vx, dy = hd * vy, dz = hd * vz;
    x = x + dx; y = y + dy; z = z + dz;
}
__device__ __forceinline__ void thermostat(const Consts& C, unsigned long long id, unsigned long long step, uint32_t mol, double& vx, double& vy,
                                           double& vz)
{
    double a, b, c;
    normals(C, id, step, mol, a, b, c);
    vx = __builtin_fma(C.c1, vx, C.c2 * a); vy = __builtin_fma(C.c1, vy, C.c2 * b); vz = __builtin_fma(C.c1, vz, C.c2 * c);
}
__device__ __forceinline__ double largest_abs(double fx, double fy, double fz)
{
    const double ax = __builtin_fabs(fx), ay = __builtin_fabs(fy), az = __builtin_fabs(fz);
    return ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az);
}
__device__ __forceinline__ double pressure_of(double K, double W, double V) { return (2.0 * K + W) / (3.0 * V); }
__device__ __forceinline__ double pressure_ab(double K, double W, double V) { return (2.0 * K + W) / V; }
__device__ __forceinline__ double length_of(double x, double y, double z) { return __builtin_sqrt(__builtin_fma(x, x, __builtin_fma(y, y, z * z))); }
// whether the barostat moves the Cartesian axis j
__device__ __forceinline__ bool axis_moves(const Consts& C, int j) { return C.coupling != MW_PIN_UNIAXIAL || j == C.axis; }

// ---- the bias (mw_pin.h) --------------------------------------------------------------------------------------------------------
// (cos, sin) of theta = 2 pi n.s of the molecule at the wrapped fractional s: one sincospi, whose argument reduction is exact
__device__ __forceinline__ void phasor(const double* __restrict__ P, double s0, double s1, double s2, double& cs, double& sn)
{
    const double ph = __builtin_fma(P[0], s0, __builtin_fma(P[1], s1, P[2] * s2));
    sincospi(2.0 * ph, &sn, &cs);
}
// Q, U_b and g k of a box from its sums C and S, its bias P [kPin] and the inverse I of its cell (row-major): k_a = 2 pi (n_1 I[a] +
// n_2 I[3 + a] + n_3 I[6 + a]); with R = 0 the force is zero
__device__ __forceinline__ void mode_of(const double* __restrict__ P, const double* __restrict__ I, int n, double C, double S, double& Q, double& U,
                                        double (&gk)[3])
{
    const double R = __builtin_sqrt(__builtin_fma(C, C, S * S)), rn = __builtin_sqrt((double)n);
    Q = R / rn;
    const double d = Q - P[4];
    U = (0.5 * P[3]) * (d * d);
    const double g = R > 0.0 ? -(P[3] * d) / (R * rn) : 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) gk[a] = g * (kTwoPi * __builtin_fma(P[0], I[a], __builtin_fma(P[1], I[3 + a], P[2] * I[6 + a])));
}
// the molecule's share: F_a <- fma(w, g k_a, F_a) with w = S cos theta - C sin theta
__device__ __forceinline__ void bias_force(double C, double S, double cs, double sn, double gk0, double gk1, double gk2, double& fx, double& fy, double& fz)
{
    const double w = __builtin_fma(S, cs, -(C * sn));
    fx = __builtin_fma(w, gk0, fx); fy = __builtin_fma(w, gk1, fy); fz = __builtin_fma(w, gk2, fz);
}
// Which block the row after evaluation e (= after step e - 1 of the call) belongs to, or -1; `last`: it closes the block.
__device__ __forceinline__ int block_of(const Consts& C, int e, bool& last)
{
    last = false;
    if (C.nblocks == 0 || e < 1) return -1;
    const int t = e - 1 - C.equil;
    if (t < 0) return -1;
    const int j = t / C.block_steps;
    if (j >= C.nblocks) return -1;
    last = t - j * C.block_steps == C.block_steps - 1;
    return j;
}

// ---- the cell of a box, on the device (the NPT library's, restated) --------------------------------------------------------------
// par [18] (the cell and its inverse), grid [4] and the volume of the cell c [9] by the arithmetic of invert_cell, cell_widths and
// cell_grid (mw_lib_host.h, mw_lib_cells.h).  False, and nothing written, when the determinant is zero or not finite, an element of
// the inverse is not finite or the cell rule a sigma (1 + 1e-9) <= the smallest width fails; g_1 g_2 g_3 <= cap otherwise.
__device__ __forceinline__ bool cell_setup(const double (&c)[9], int cap, double* __restrict__ par, int* __restrict__ grid, double* __restrict__ vol)
{
    double C[9];                                                        // C[3 i + j], H[a][k] = c[3 k + a]
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            C[3 * i + j] = __builtin_fma(c[3 * j1 + i1], c[3 * j2 + i2], -(c[3 * j2 + i1] * c[3 * j1 + i2]));
        }
    }
    const double det = __builtin_fma(c[0], C[0], __builtin_fma(c[3], C[1], c[6] * C[2]));
    if (!(det != 0.0) || !(det - det == 0.0)) return false;
    double I[9];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            I[3 * a + k] = C[3 * k + a] / det;
            finite = finite && (I[3 * a + k] - I[3 * a + k] == 0.0);
        }
    }
    if (!finite) return false;
    double w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ka = 3 * ((k + 1) % 3), kb = 3 * ((k + 2) % 3);
        const double x = c[ka + 1] * c[kb + 2] - c[ka + 2] * c[kb + 1], y = c[ka + 2] * c[kb] - c[ka] * c[kb + 2], z = c[ka] * c[kb + 1] - c[ka + 1] * c[kb];
        w[k] = __builtin_fabs(det) / __builtin_sqrt(x * x + y * y + z * z);
    }
    const double wmin = __builtin_fmin(w[0], __builtin_fmin(w[1], w[2]));
    if (!(mw::kSigA * kGuard <= wmin)) return false;
    int g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double f = __builtin_floor(w[k] / (mw::kSigA * kGuard));
        g[k] = f >= (double)kMaxGrid ? kMaxGrid : f >= 1.0 ? (int)f : 1;
    }
    int g0 = g[0], g1 = g[1], g2 = g[2];
    while ((long long)g0 * g1 * g2 > cap) {                              // the largest, the first of equals, one down
        if (g2 > g0 && g2 > g1) --g2;
        else if (g1 > g0) --g1;
        else --g0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) { par[k] = c[k]; par[9 + k] = I[k]; }
    grid[0] = g0; grid[1] = g1; grid[2] = g2; grid[3] = g0 * g1 * g2;
    *vol = __builtin_fabs(det);
    return true;
}

// the lengths of the three vectors of the cell c to a box's cv [4 .. 6]
__device__ __forceinline__ void cell_lengths(const double (&c)[9], double* __restrict__ cv)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) cv[4 + k] = length_of(c[3 * k], c[3 * k + 1], c[3 * k + 2]);
}

// ---- both geometries: the verdict on device arrays, the state of a chunk at its start, the results at its end -------------------
// bad[k] = the first box whose array k (pos, vel, pos_ref) holds a value that is not finite; arrays may be NULL.
__global__ __launch_bounds__(kThreads) void k_pin_check(size_t total, int n, const double* __restrict__ pos, const double* __restrict__ vel,
                                                         const double* __restrict__ ref, int* __restrict__ bad)
{
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const int b = (int)(i / (size_t)n);
        const double* arr[3] = {pos, vel, ref};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!arr[k]) continue;
            const double s = arr[k][3 * i] - arr[k][3 * i], t = arr[k][3 * i + 1] - arr[k][3 * i + 1], u = arr[k][3 * i + 2] - arr[k][3 * i + 2];
            if (!(s == 0.0 && t == 0.0 && u == 0.0)) atomicMin(bad + k, b);       // x - x is 0 for a finite x alone
        }
    }
}

// One lane per molecule: x = pos, v = vel or 0, F = 0, the origin = pos_ref or pos; the first lane of a box sets its row, its flags
// and its cell.  A cell the host passed and the device does not (no such cell is known) freezes the box with the barostat's code
// before its first evaluation, over a unit cell of one grid cell: the sort's addresses stay inside its tables.
__global__ __launch_bounds__(kThreads) void k_pin_begin(int n, int cap, const double* __restrict__ cells, const double* __restrict__ pos,
                                                         const double* __restrict__ vel, const double* __restrict__ pos_ref, double* __restrict__ x,
                                                         double* __restrict__ v, double* __restrict__ F, double* __restrict__ ref,
                                                         double* __restrict__ row, int* __restrict__ si, double* __restrict__ cell,
                                                         double* __restrict__ par, int* __restrict__ grid, double* __restrict__ cv,
                                                         double* __restrict__ acc)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    x[m] = pos[m]; x[m + 1] = pos[m + 1]; x[m + 2] = pos[m + 2];
    v[m] = vel ? vel[m] : 0.0; v[m + 1] = vel ? vel[m + 1] : 0.0; v[m + 2] = vel ? vel[m + 2] : 0.0;
    F[m] = F[m + 1] = F[m + 2] = 0.0;
    const double* q = pos_ref ? pos_ref : pos;
    ref[m] = q[m]; ref[m + 1] = q[m + 1]; ref[m + 2] = q[m + 2];
    if (i == 0) {
        for (int k = 0; k < kRow; ++k) row[kRow * (size_t)b + k] = 0.0;
        for (int k = 0; k < kSI; ++k) si[kSI * (size_t)b + k] = 0;
        for (int k = 0; k < kAcc; ++k) acc[kAcc * (size_t)b + k] = 0.0;
        double c[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) { c[k] = cells[9 * (size_t)b + k]; cell[9 * (size_t)b + k] = c[k]; }
        double* V = cv + kCV * (size_t)b;
        V[1] = V[2] = V[3] = 1.0;
        V[7] = 0.0;
        cell_lengths(c, V);
        if (!cell_setup(c, cap, par + 18 * (size_t)b, grid + 4 * (size_t)b, V)) {
            for (int k = 0; k < 18; ++k) par[18 * (size_t)b + k] = (k % 9) % 4 == 0 ? 1.0 : 0.0;
            for (int k = 0; k < 4; ++k) grid[4 * (size_t)b + k] = 1;
            V[0] = 1.0;
            si[kSI * (size_t)b] = 1;
            si[kSI * (size_t)b + 4] = 1;
        }
    }
}

// One lane per molecule: the state out; the first lane of a box writes its status and its cell.
__global__ __launch_bounds__(kThreads) void k_pin_finish(int n, const double* __restrict__ x, const double* __restrict__ v, const double* __restrict__ F,
                                                          const double* __restrict__ ref, const int* __restrict__ si, const double* __restrict__ cell,
                                                          double* __restrict__ pos_out, double* __restrict__ vel_out, double* __restrict__ forces,
                                                          double* __restrict__ ref_out, double* __restrict__ cells_out, int* __restrict__ status)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    if (pos_out) { pos_out[m] = x[m]; pos_out[m + 1] = x[m + 1]; pos_out[m + 2] = x[m + 2]; }
    if (vel_out) { vel_out[m] = v[m]; vel_out[m + 1] = v[m + 1]; vel_out[m + 2] = v[m + 2]; }
    if (forces) { forces[m] = F[m]; forces[m + 1] = F[m + 1]; forces[m + 2] = F[m + 2]; }
    if (ref_out) { ref_out[m] = ref[m]; ref_out[m + 1] = ref[m + 1]; ref_out[m + 2] = ref[m + 2]; }
    if (i == 0) {
        const int* I = si + kSI * (size_t)b;
        if (status) {
            status[2 * (size_t)b] = I[3];
            status[2 * (size_t)b + 1] = I[4] ? 2 : (I[0] | I[1] | I[2]) ? 1 : 0;
        }
        if (cells_out)
            for (int k = 0; k < 9; ++k) cells_out[9 * (size_t)b + k] = cell[9 * (size_t)b + k];
    }
}

// ---- the barostat, both geometries -------------------------------------------------------------------------------------------
// One lane per box after stage 6 of the step with index `step`: the decision of mw_pin.h from the box's row (K, W, P_aa) and
// volume.  Accepted: the three mu, the volume and the lengths to cv, the scaled cell and its par and grid in place.  Refused: the
// box is frozen with the barostat's code and nothing of its cell is touched; `fill` (the small geometry, whose step kernel does not
// visit a frozen box again): the trace rows after this step repeat its row.
__global__ __launch_bounds__(64) void k_pin_baro(int nb, int cap, Consts C, const unsigned long long* __restrict__ streams, int b0,
                                                  unsigned long long step, int fill, const double* __restrict__ row, int* __restrict__ si,
                                                  double* __restrict__ cell, double* __restrict__ par, int* __restrict__ grid, double* __restrict__ cv,
                                                  double* __restrict__ trace)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;
    int* I = si + kSI * (size_t)b;
    if (I[0]) return;
    const double* R = row + kRow * (size_t)b;
    double* CV = cv + kCV * (size_t)b;
    const double V = CV[0];
    const unsigned long long id = streams ? streams[b] : (unsigned long long)(b0 + b);
    bool ok = true;
    double mu0 = 1.0, mu1 = 1.0, mu2 = 1.0;
    if (C.coupling == MW_PIN_ISO) {                                     // the stage of the NPT library
        const double P = pressure_of(R[1], R[kOut], V);
        double de = -(C.cb * (C.pressure - P));
        if (C.baro_noise) {
            const double xi = box_normal(C, id, step, 1u);
            de = __builtin_fma(C.cn, xi / __builtin_sqrt(V), de);
        }
        ok = __builtin_fabs(de) <= MW_PIN_MAX_DLNV;                     // (a NaN fails)
        if (ok) mu0 = mu1 = mu2 = exp(de / 3.0);
    } else {
        double mu[3] = {1.0, 1.0, 1.0};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (!axis_moves(C, j)) continue;
            // the group of axis j: itself, or with MW_PIN_SEMI and j != axis the pair of j and the third axis p
            const bool pair = C.coupling == MW_PIN_SEMI && j != C.axis;
            const int p = pair ? 3 - C.axis - j : j;
            const int lo = p < j ? p : j, hi = p < j ? j : p;
            const double PG = pair ? 0.5 * (R[6 + lo] + R[6 + hi]) : R[6 + j];
            double de = -(C.cb3 * (C.pressure - PG));
            if (C.baro_noise) {
                const double xi = box_normal(C, id, step, 2u + (uint32_t)lo);
                de = __builtin_fma(pair ? C.cn2 : C.cn1, xi / __builtin_sqrt(V), de);
            }
            ok = ok && __builtin_fabs(de) <= MW_PIN_MAX_DLNL;           // (a NaN fails)
            mu[j] = exp(de);
        }
        mu0 = mu[0]; mu1 = mu[1]; mu2 = mu[2];
    }
    if (ok) {
        double c[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double h0 = cell[9 * (size_t)b + 3 * k], h1 = cell[9 * (size_t)b + 3 * k + 1], h2 = cell[9 * (size_t)b + 3 * k + 2];
            c[3 * k] = axis_moves(C, 0) ? mu0 * h0 : h0;
            c[3 * k + 1] = axis_moves(C, 1) ? mu1 * h1 : h1;
            c[3 * k + 2] = axis_moves(C, 2) ? mu2 * h2 : h2;
        }
        ok = cell_setup(c, cap, par + 18 * (size_t)b, grid + 4 * (size_t)b, CV);
        if (ok) {
#pragma unroll
            for (int k = 0; k < 9; ++k) cell[9 * (size_t)b + k] = c[k];
            CV[1] = mu0; CV[2] = mu1; CV[3] = mu2;
            cell_lengths(c, CV);
        }
    }
    if (!ok) {
        I[0] = 1;
        I[4] = 1;
        if (fill && trace)
            for (int t = I[3] / C.sample_every + 1; t < C.nrows; ++t)
                for (int k = 0; k < kOut; ++k) trace[((size_t)b * C.nrows + t) * kOut + k] = R[k];
    }
}

// One lane per molecule of a box whose application was accepted, every axis a that moves: x_a <- mu_a x_a, pos_ref_a <- mu_a
// pos_ref_a, v_a <- v_a / mu_a.
__global__ __launch_bounds__(kThreads) void k_pin_scale(int n, Consts C, const int* __restrict__ si, const double* __restrict__ cv, double* __restrict__ x,
                                                         double* __restrict__ v, double* __restrict__ ref)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (si[kSI * (size_t)b] || i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (!axis_moves(C, j)) continue;
        const double mu = cv[kCV * (size_t)b + 1 + j];
        x[m + j] = mu * x[m + j];
        ref[m + j] = mu * ref[m + j];
        v[m + j] = v[m + j] / mu;
    }
}

// ---- general geometry ----------------------------------------------------------------------------------------------------
// Per box in scratch after the sort's pieces (mw_lib_cells.h): mom [n][kMom] and en [n] in cell order; part [workgroups][kPart];
// then what both geometries carry: x, v, F, ref [n][3] by index; the row [kRow], the ints [kSI], the cell [9], par [18], grid [4]
// and cv [kCV].

// Stages 2 and 3 and the test of stage 4, one lane per molecule.
__global__ __launch_bounds__(kThreads) void k_pin_drift1(int n, Consts C, const unsigned long long* __restrict__ streams, int b0,
                                                          unsigned long long step, double* __restrict__ x, double* __restrict__ v, int* si)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    int* I = si + kSI * (size_t)b;
    if (I[0] || i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    double vx = v[m], vy = v[m + 1], vz = v[m + 2];
    drift(C.hd, vx, vy, vz, x[m], x[m + 1], x[m + 2]);
    if (C.thermostat) {
        thermostat(C, streams ? streams[b] : (unsigned long long)(b0 + b), step, (uint32_t)i, vx, vy, vz);
        v[m] = vx; v[m + 1] = vy; v[m + 2] = vz;
    }
    if (guard_fails(C.hd, C.lim2, vx, vy, vz)) atomicOr(I + 2, 1);
}

// The drift of stage 4, one lane per molecule.
__global__ __launch_bounds__(kThreads) void k_pin_drift2(int n, double hd, double* __restrict__ x, const double* __restrict__ v,
                                                          const int* __restrict__ si)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    const int* I = si + kSI * (size_t)b;
    if (I[0] || I[2] || i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    drift(hd, v[m], v[m + 1], v[m + 2], x[m], x[m + 1], x[m + 2]);
}

// The moment pass, one lane per molecule in sorted order.  In a biased box the lane then forms the phasor of its molecule from the
// sorted s it holds, stores the pair in sorted order and contributes to the workgroup's two partial sums (lanes by the DPP tree,
// wavefronts in order); the branch is uniform over the workgroup.
__global__ __launch_bounds__(kThreads) void k_pin_moments(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                          const int* __restrict__ start, const double* __restrict__ ss, const int* __restrict__ si,
                                                          const double* __restrict__ pin, double* __restrict__ mom, double* __restrict__ en,
                                                          double2* __restrict__ pair, double* __restrict__ rpart)
{
    __shared__ double red[kThreads / 64][2];
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (si[kSI * (size_t)b] || si[kSI * (size_t)b + 2]) return;        // the whole workgroup
    const double* H = par + 18 * (size_t)b;
    const size_t o = (size_t)b * n;
    const double* S = ss + 3 * o;
    const bool live = p < n;
    const size_t at = live ? (size_t)p : 0;
    const double s0 = S[3 * at], s1 = S[3 * at + 1], s2 = S[3 * at + 2];
    if (live) {
        Sums a;
        const CellRegs hc(H);
        walk_cells(s0, s1, s2, mw::kRcSq, hc.c, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), S,
                   [&](int, int, int, int, double r2, double dx, double dy, double dz) { a.add(r2, dx, dy, dz); });
        double M[kMom];
        a.record(M);
        double2* w = reinterpret_cast<double2*>(mom + kMom * (o + p));
#pragma unroll
        for (int c = 0; c < kMom / 2; ++c) w[c] = make_double2(M[2 * c], M[2 * c + 1]);
        en[o + p] = a.energy();
    }
    const double* P = pin + kPin * (size_t)b;
    if (P[3] != 0.0) {
        double val[2] = {0.0, 0.0};
        if (live) {
            phasor(P, s0, s1, s2, val[0], val[1]);
            pair[o + p] = make_double2(val[0], val[1]);
        }
        const double r = block_reduce<2, 0>(val, red);
        if (threadIdx.x < 2) rpart[((size_t)b * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = r;
    }
}

// One wavefront per box that is not frozen, between the moment pass and the force pass: lanes 0 and 1 add the columns C and S
// of the box's partials in workgroup order; lane 0 makes the box's mode of them and of its par: C, S, g k, Q and U_b.
__global__ __launch_bounds__(64) void k_pin_rho(int nwg, int n, const double* __restrict__ par, const int* __restrict__ si, const double* __restrict__ pin,
                                                const double* __restrict__ rpart, double* __restrict__ bias)
{
    __shared__ double sum[2];
    const int b = blockIdx.x, k = threadIdx.x;
    const double* P = pin + kPin * (size_t)b;
    if (si[kSI * (size_t)b] || si[kSI * (size_t)b + 2]) return;
    if (!(P[3] != 0.0)) {                                              // no bias: the flag the force pass reads, and zeros for the row
        if (k < kBias) bias[kBias * (size_t)b + k] = 0.0;
        return;
    }
    if (k < 2) {
        const double* T = rpart + (size_t)b * nwg * 2;
        double a = T[k];
        for (int w = 1; w < nwg; ++w) a = a + T[2 * (size_t)w + k];
        sum[k] = a;
    }
    __syncthreads();
    if (k == 0) {
        double Q, U, gk[3];
        mode_of(P, par + 18 * (size_t)b + 9, n, sum[0], sum[1], Q, U, gk);
        double* B = bias + kBias * (size_t)b;
        B[0] = sum[0]; B[1] = sum[1]; B[2] = gk[0]; B[3] = gk[1]; B[4] = gk[2]; B[5] = Q; B[6] = U; B[7] = 1.0;
    }
}

// The force pass, one lane per molecule in sorted order: the force of the molecule, written by index, its share of the scalar virial
// and of the stress; stage 6 of this step (`do6`: not at the evaluation before the first step and not at the one after a barostat
// application) and stage 1 of the next with its guard (`do1`: not after the last step and not before a barostat application); the
// partial values of the workgroup from the velocities between the two.
__global__ __launch_bounds__(kThreads) void k_pin_forces(int n, int cap, Consts C, int do6, int do1, const double* __restrict__ par,
                                                          const int* __restrict__ grid, const int* __restrict__ start, const double* __restrict__ ss,
                                                          const int* __restrict__ idx, int* si, const double* __restrict__ mom,
                                                          const double* __restrict__ en, const double* __restrict__ ref, const double* __restrict__ x,
                                                          const double2* __restrict__ pair, const double* __restrict__ bias,
                                                          double* __restrict__ v, double* __restrict__ F,
                                                          double* __restrict__ part)
{
    __shared__ double red[kThreads / 64][kPart];
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    int* I = si + kSI * (size_t)b;
    if (I[0] || I[2]) return;                                          // the whole workgroup
    const size_t o = (size_t)b * n;
    double val[kPart];
#pragma unroll
    for (int k = 0; k < kPart; ++k) val[k] = 0.0;
    if (p < n) {
        const double* H = par + 18 * (size_t)b;
        const double* S = ss + 3 * o;
        const double* Mb = mom + kMom * o;
        const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
        double Mi[kMom];
        mw::load_moments(Mb + kMom * (size_t)p, Mi);
        double fx = 0.0, fy = 0.0, fz = 0.0, dw = 0.0;
        double st[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        // (the two addresses of the bias, and three more that are not used before the walk ends, wait in vector registers: the walk
        // has no scalar register to spare, and a spilled one would give the kernel a private segment)
        const double* B = bias + kBias * (size_t)b;
        const double2* E = pair + (o + p);
        asm("" : "+v"(B), "+v"(E), "+v"(ref), "+v"(x), "+v"(en));
        const CellRegs hc(H);
        walk_cells(s0, s1, s2, mw::kRcSq, hc.c, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), S,
                   [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
                       if (q == p) return;                             // an image of the molecule itself: d is constant
                       double Mj[kMom];
                       mw::load_moments(Mb + kMom * (size_t)q, Mj);
                       entry_stress(Mi, Mj, r2, dx, dy, dz, fx, fy, fz, dw, st);
                   });
        if (B[7] != 0.0) {                                             // a biased box, the whole workgroup: F_mW + F_b from here on
            const double2 e = *E;
            bias_force(B[0], B[1], e.x, e.y, B[2], B[3], B[4], fx, fy, fz);
        }
        const size_t m = 3 * (o + idx[o + p]);
        F[m] = fx; F[m + 1] = fy; F[m + 2] = fz;
        double vx = v[m], vy = v[m + 1], vz = v[m + 2];
        if (do6) kick(C.hk, fx, fy, fz, vx, vy, vz);
        const double d0 = x[m] - ref[m], d1 = x[m + 1] - ref[m + 1], d2 = x[m + 2] - ref[m + 2];
        val[0] = en[o + p];
        val[1] = __builtin_fma(vx, vx, __builtin_fma(vy, vy, vz * vz));
        val[2] = __builtin_fma(d0, d0, __builtin_fma(d1, d1, d2 * d2));
        val[3] = lane_virial(dw);
        val[4] = C.hm * (vx * vx); val[5] = C.hm * (vy * vy); val[6] = C.hm * (vz * vz);
        val[7] = C.hm * (vx * vy); val[8] = C.hm * (vx * vz); val[9] = C.hm * (vy * vz);
#pragma unroll
        for (int k = 0; k < 6; ++k) val[10 + k] = lane_stress(st[k], k);
        val[kSums] = largest_abs(fx, fy, fz);
        if (do1) {
            kick(C.hk, fx, fy, fz, vx, vy, vz);
            if (guard_fails(C.hd, C.lim2, vx, vy, vz)) atomicOr(I + 1, 1);
        }
        if (do6 || do1) { v[m] = vx; v[m + 1] = vy; v[m + 2] = vz; }
    }
    const double r = block_reduce<kSums, 1>(val, red);
    if (threadIdx.x < kPart) part[((size_t)b * gridDim.x + blockIdx.x) * kPart + threadIdx.x] = r;
}

// One workgroup of 64 per box after the evaluation that ends step e: lane k < kPart adds column k of the box's partials in
// workgroup order; lane 0 makes the row of them, of the box's volume and of the lengths of its cell; a frozen box keeps its row.
// The row goes to the trace when e is a multiple of sample_every.  Lane 0 counts the step and takes the guards' flags over.
__global__ __launch_bounds__(64) void k_pin_row(int nwg, int n, int e, int tally, Consts C, const double* __restrict__ part, const double* __restrict__ cv,
                                                const double* __restrict__ pin, const double* __restrict__ bias, double* __restrict__ row,
                                                double* __restrict__ acc, int* __restrict__ si, double* __restrict__ trace, double* __restrict__ blocks)
{
    __shared__ double sum[kPart], cur[kRow];
    const int b = blockIdx.x, k = threadIdx.x;
    int* I = si + kSI * (size_t)b;
    const bool frozen = I[0] || I[2];
    const int tripped = I[1];
    if (k < kRow) cur[k] = row[kRow * (size_t)b + k];
    if (k < kPart && !frozen) {
        const double* P = part + (size_t)b * nwg * kPart;
        double a = P[k];
        for (int w = 1; w < nwg; ++w) {
            const double t = P[(size_t)w * kPart + k];
            a = k < kSums ? a + t : (t > a ? t : a);
        }
        sum[k] = a;
    }
    __syncthreads();
    if (k == 0 && !frozen) {
        const double* CV = cv + kCV * (size_t)b;
        const double V = CV[0], K = C.hm * sum[1];
        cur[0] = sum[0]; cur[1] = K; cur[2] = sum[2] / (double)n; cur[3] = sum[kSums]; cur[4] = V; cur[5] = pressure_of(K, sum[3], V);
        for (int f = 0; f < 6; ++f) cur[6 + f] = pressure_ab(sum[4 + f], sum[10 + f], V);
        cur[12] = CV[4]; cur[13] = CV[5]; cur[14] = CV[6];
        const bool biased = pin[kPin * (size_t)b + 3] != 0.0;
        cur[15] = biased ? bias[kBias * (size_t)b + 5] : 0.0;
        cur[16] = biased ? bias[kBias * (size_t)b + 6] : 0.0;
        cur[kOut] = sum[3];
        for (int f = 0; f < kRow; ++f) row[kRow * (size_t)b + f] = cur[f];
    }
    __syncthreads();
    if (k < kOut && trace && e % C.sample_every == 0) trace[((size_t)b * C.nrows + e / C.sample_every) * kOut + k] = cur[k];
    bool last;
    const int j = tally ? block_of(C, e, last) : -1;
    if (k < kAcc && j >= 0) {                                          // lane k: Q, Q Q, V, E
        const double a = k == 0 ? cur[15] : k == 1 ? cur[15] * cur[15] : k == 2 ? cur[4] : cur[0];
        double s = acc[kAcc * (size_t)b + k] + a;
        if (last) {
            if (blocks) blocks[((size_t)b * C.nblocks + j) * kAcc + k] = s / (double)C.block_steps;
            s = 0.0;
        }
        acc[kAcc * (size_t)b + k] = s;
    }
    if (k == 0) {
        if (!frozen) I[3] = e;
        if (frozen || tripped) I[0] = 1;
    }
}

// ---- small geometry: one wavefront per box, lane i = molecule i ----------------------------------------------------------------
// The evaluations e0 .. e0 + ne - 1 of one box (evaluation e ends step e; evaluation 0 is the one before the first step); x, v, F,
// the row and the ints are read from scratch at the start and written back at the end, so that the next launch goes on where
// this one ended.  `again`: evaluation e0 is the one after a barostat application (no drift and no stage 6 before it);
// `hold`: a barostat application follows evaluation e0 + ne - 1 (no stage 1 after it).  The cell does not change inside a launch.
// LDS of a box: s [3][64], then the moments [kMom][64], the block accumulators [kAcc], and w [64] and g k [3] of the bias.  The row lives in scratch: lane 0 writes it after every evaluation, the
// wavefront keeps E, K, the msd, fmax, P and W of the last one.  A box that freezes writes its remaining trace rows at once, lane
// k the column k it has just written or still holds; the launches after add its last row to the block accumulators and do nothing
// else.  The accumulators are uniform over the wavefront; lane 0 writes them.  The row of a step that a barostat application follows
// (`hold`, the last evaluation) is not added here: the launch that begins with the evaluation after the application adds that step's
// row, which is the frozen one if the application was refused.  A biased box forms its phasors before the walks: C and S by the DPP
// tree over the lanes, the mode in every lane alike; one fma per component after the force walk and before the kick.
template <bool THERMOSTAT>
__global__ __launch_bounds__(kThreads) void k_pin_small(int nb, int n, int e0, int ne, int again, int hold, Consts Cs,
                                                         const unsigned long long* __restrict__ streams, int b0, unsigned long long step0,
                                                         const double* __restrict__ par, const double* __restrict__ cv, const double* __restrict__ ref,
                                                         const double* __restrict__ pin, double* __restrict__ x, double* __restrict__ v,
                                                         double* __restrict__ F, double* __restrict__ row, double* __restrict__ acc,
                                                         int* __restrict__ si, double* __restrict__ trace, double* __restrict__ blocks)
{
    __shared__ double lds[kSmallBoxesPerWg][kSmallLdsPerBox / 8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * kSmallBoxesPerWg + wave;
    if (b >= nb) return;                                   // the whole wavefront; no workgroup barrier below
    int* I = si + kSI * (size_t)b;
    double* R = row + kRow * (size_t)b;
    double* A = acc + kAcc * (size_t)b;
    double* S = lds[wave];
    double* AL = S + (3 + kMom) * 64;                      // the box's accumulators while the launch runs, lane k < kAcc its own
    double* WL = AL + kAcc;                                // [64] w of every lane, then g k [3]
    // lane k < kRow holds entry k of the box's row: what the trace rows after a freeze repeat
    double mine = in_vgpr(lane < kRow ? R[lane] : 0.0);
    if (lane < kAcc) AL[lane] = A[lane];
    // the row after evaluation e into the accumulators: Q, Q Q, V, E from the lanes 15, 4 and 0 of the row
    auto tally = [&](int e) {
        bool last;
        const int j = block_of(Cs, e, last);
        if (j < 0) return;
        const double q = mw::readlane_f64(mine, 15), vv = mw::readlane_f64(mine, 4), ee = mw::readlane_f64(mine, 0);
        if (lane < kAcc) {
            double sum = AL[lane] + (lane == 0 ? q : lane == 1 ? q * q : lane == 2 ? vv : ee);
            if (last) {
                if (blocks) blocks[((size_t)b * Cs.nblocks + j) * kAcc + lane] = sum / (double)Cs.block_steps;
                sum = 0.0;
            }
            AL[lane] = sum;
        }
    };
    const int tend = e0 + ne - (hold ? 1 : 0);             // the evaluations from here on are tallied by a later launch
    if (I[0]) {                                            // frozen in an earlier launch: the blocks alone
        for (int e = e0; e < tend; ++e) tally(e);
        if (lane < kAcc) A[lane] = AL[lane];
        return;
    }
    double* ML = S + 3 * 64;
    const double* H = par + 18 * (size_t)b;
    const double* CV = cv + kCV * (size_t)b;
    const CellRegs hc(H), hi(H + 9);
    const bool active = lane < n;
    const size_t m = 3 * ((size_t)b * n + (active ? lane : 0));
    double x0 = active ? x[m] : 0.0, x1 = active ? x[m + 1] : 0.0, x2 = active ? x[m + 2] : 0.0;
    double vx = active ? v[m] : 0.0, vy = active ? v[m + 1] : 0.0, vz = active ? v[m + 2] : 0.0;
    double fx = active ? F[m] : 0.0, fy = active ? F[m + 1] : 0.0, fz = active ? F[m + 2] : 0.0;
    // (the call's constants are kept out of the scalar registers, for the same reason as the cell)
    Consts C = Cs;
    C.hk = in_vgpr(Cs.hk); C.hd = in_vgpr(Cs.hd); C.c1 = in_vgpr(Cs.c1); C.c2 = in_vgpr(Cs.c2); C.lim2 = in_vgpr(Cs.lim2); C.hm = in_vgpr(Cs.hm);
    const double vol = in_vgpr(CV[0]);
    const double* P = pin + kPin * (size_t)b;
    const bool biased = P[3] != 0.0;                       // the whole wavefront
    const unsigned long long id = streams ? streams[b] : (unsigned long long)(b0 + b);
    int steps = I[3];
    bool frozen = false;
    for (int e = e0; e < e0 + ne; ++e) {
        const bool step = e > 0 && !(again && e == e0);
        if (step) {
            drift(C.hd, vx, vy, vz, x0, x1, x2);
            if constexpr (THERMOSTAT) {
                thermostat(C, id, step0 + (unsigned long long)(e - 1), (uint32_t)lane, vx, vy, vz);
                if (!active) vx = vy = vz = 0.0;                       // a lane without a molecule stays out of the box sums
            }
            if (__ballot(active && guard_fails(C.hd, C.lim2, vx, vy, vz))) { frozen = true; break; }
            drift(C.hd, vx, vy, vz, x0, x1, x2);
        }
        const double s0 = frac_coord(hi.c, 0, x0, x1, x2), s1 = frac_coord(hi.c, 1, x0, x1, x2), s2 = frac_coord(hi.c, 2, x0, x1, x2);
        mw::wave_fence();
        S[lane] = s0; S[64 + lane] = s1; S[128 + lane] = s2;
        // entry k of the row goes to lane k as it is made: every total is the same in all lanes
        auto put = [&](int k, double t) { mine = lane == k ? t : mine; };
        if (biased) {
            // the mode before the walks, where registers are to spare; what the force needs after them waits in LDS: w of the lane
            // and g k of the box
            double cs, sn, qm, ub, gk[3];
            phasor(P, s0, s1, s2, cs, sn);
            const double Cm = wave_total(active ? cs : 0.0), Sm = wave_total(active ? sn : 0.0);
            mode_of(P, hi.c, n, Cm, Sm, qm, ub, gk);
            WL[lane] = __builtin_fma(Sm, cs, -(Cm * sn));
            if (lane < 3) WL[64 + lane] = lane == 0 ? gk[0] : lane == 1 ? gk[1] : gk[2];
            put(15, qm); put(16, ub);
        }
        mw::wave_fence();
        Sums a;
        walk_small(n, active, mw::kRcSq, hc.c, S, s0, s1, s2, [&](int, int, double d2, double dx, double dy, double dz) { a.add(d2, dx, dy, dz); });
        double Mi[kMom];
        a.record(Mi);
#pragma unroll
        for (int k = 0; k < kMom; ++k) ML[64 * k + lane] = Mi[k];
        mw::wave_fence();
        fx = fy = fz = 0.0;
        double dw = 0.0;
        double st[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        walk_small(n, active, mw::kRcSq, hc.c, S, s0, s1, s2, [&](int j, int, double d2, double dx, double dy, double dz) {
            if (j == lane) return;                                     // an image of the molecule itself: d is constant
            double Mj[kMom];
#pragma unroll
            for (int k = 0; k < kMom; ++k) Mj[k] = ML[64 * k + j];
            entry_stress(Mi, Mj, d2, dx, dy, dz, fx, fy, fz, dw, st);
        });
        if (biased && active) {                                        // F_mW + F_b from here on
            const double w = WL[lane];
            fx = __builtin_fma(w, WL[64], fx); fy = __builtin_fma(w, WL[65], fy); fz = __builtin_fma(w, WL[66], fz);
        }
        if (step) kick(C.hk, fx, fy, fz, vx, vy, vz);
        // (the origin is read again at every evaluation: three values less to hold across the walks)
        const double* rp = ref + m;
        asm volatile("" : "+v"(rp));
        const double q0 = active ? rp[0] : 0.0, q1 = active ? rp[1] : 0.0, q2 = active ? rp[2] : 0.0;
        const double d0 = x0 - q0, d1 = x1 - q1, d2 = x2 - q2;
        const double K = C.hm * wave_total(__builtin_fma(vx, vx, __builtin_fma(vy, vy, vz * vz)));
        const double W = wave_total(lane_virial(dw));
        put(0, wave_total(active ? a.energy() : 0.0));
        put(1, K);
        put(2, wave_total(__builtin_fma(d0, d0, __builtin_fma(d1, d1, d2 * d2))) / (double)n);
        put(3, wave_largest(largest_abs(fx, fy, fz)));
        put(4, vol);
        put(5, pressure_of(K, W, vol));
        put(6, pressure_ab(wave_total(C.hm * (vx * vx)), wave_total(lane_stress(st[0], 0)), vol));
        put(7, pressure_ab(wave_total(C.hm * (vy * vy)), wave_total(lane_stress(st[1], 1)), vol));
        put(8, pressure_ab(wave_total(C.hm * (vz * vz)), wave_total(lane_stress(st[2], 2)), vol));
        put(9, pressure_ab(wave_total(C.hm * (vx * vy)), wave_total(lane_stress(st[3], 3)), vol));
        put(10, pressure_ab(wave_total(C.hm * (vx * vz)), wave_total(lane_stress(st[4], 4)), vol));
        put(11, pressure_ab(wave_total(C.hm * (vy * vz)), wave_total(lane_stress(st[5], 5)), vol));
        put(12, CV[4]); put(13, CV[5]); put(14, CV[6]);
        put(kOut, W);
        steps = e;
        if (trace && lane < kOut && e % C.sample_every == 0) trace[((size_t)b * C.nrows + e / C.sample_every) * kOut + lane] = mine;
        if (e < tend) tally(e);
        if (e < C.nsteps && !(hold && e == e0 + ne - 1)) {
            kick(C.hk, fx, fy, fz, vx, vy, vz);
            if (__ballot(active && guard_fails(C.hd, C.lim2, vx, vy, vz))) { frozen = true; break; }
        }
    }
    if (active) {
        x[m] = x0; x[m + 1] = x1; x[m + 2] = x2;
        v[m] = vx; v[m + 1] = vy; v[m + 2] = vz;
        F[m] = fx; F[m + 1] = fy; F[m + 2] = fz;
    }
    if (frozen && trace && lane < kOut)
        for (int t = steps / C.sample_every + 1; t < C.nrows; ++t) trace[((size_t)b * C.nrows + t) * kOut + lane] = mine;
    if (frozen)
        for (int e = steps + 1; e < tend; ++e) tally(e);
    if (lane < kRow) R[lane] = mine;
    if (lane < kAcc) A[lane] = AL[lane];
    if (lane == 0) {
        I[3] = steps;
        if (frozen) I[0] = 1;
    }
}

}  // namespace mwpin

namespace {

using namespace mwpin;

constexpr int kPool = 512;                         // event timers between two harvests
constexpr int kPoolSlack = 32;
constexpr int kDefaultSlice = 64, kMaxSlice = 256;
enum { kSort = 0, kMoments = 1, kForces = 2, kDrift = 3, kBaro = 4, kRho = 5, kTimers = 6 };

struct State : Runtime<1> {
    Buf scratch, cells, pos, vel, ref, streams, pin, pos_out, vel_out, forces, cells_out, ref_out, trace, blocks, status, bad;
    std::vector<hipEvent_t> pool;
    std::vector<int> bucket;                       // what the interval that begins at event k is, or -1
    int used = 0;
    int slice = kDefaultSlice;
    int last[MW_PIN_PLAN_FIELDS] = {0};
    float ms[kTimers] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
} g;

// The scratch of one box: the sort's pieces and what the passes keep (general), then what both geometries carry.
struct Layout : SortLayout {
    int nwg = 0;
    size_t mom = 0, en = 0, part = 0, pair = 0, rpart = 0, bias = 0, x = 0, v = 0, F = 0, ref = 0, row = 0, acc = 0, si = 0, cell = 0, par = 0, grid = 0, cv = 0,
           per_box = 0;
};

Layout make_layout(int n, bool small)
{
    Layout l;
    size_t o = 0;
    if (!small) {
        lay_sort(l, n, o);
        l.nwg = (n + kThreads - 1) / kThreads;
        l.mom = o;  o += align16(8 * (size_t)kMom * n);
        l.en = o;   o += align16(8 * (size_t)n);
        l.part = o; o += align16(8 * (size_t)kPart * l.nwg);
        l.pair = o; o += align16(16 * (size_t)n);
        l.rpart = o; o += align16(16 * (size_t)l.nwg);
        l.bias = o; o += align16(8 * (size_t)kBias);
    } else {
        l.cap = cell_cap(n);
    }
    l.x = o;    o += align16(24 * (size_t)n);
    l.v = o;    o += align16(24 * (size_t)n);
    l.F = o;    o += align16(24 * (size_t)n);
    l.ref = o;  o += align16(24 * (size_t)n);
    l.row = o;  o += align16(8 * (size_t)kRow);
    l.acc = o;  o += align16(8 * (size_t)kAcc);
    l.si = o;   o += align16(4 * (size_t)kSI);
    l.cell = o; o += align16(8 * 9);
    l.par = o;  o += align16(8 * 18);
    l.grid = o; o += align16(4 * 4);
    l.cv = o;   o += align16(8 * (size_t)kCV);
    l.per_box = o;
    return l;
}

struct Plan : PlanBase {
    Layout lay;
    int steps_per_launch;
};

int make_plan(const char* who, int n, int nboxes, size_t budget, int slice, Plan& p)
{
    p.small = n <= kSmallN;
    p.lay = make_layout(n, p.small);
    p.per_box = p.lay.per_box;
    p.lds = p.small ? kSmallLds : kGeneralLds;
    p.boxes_per_wg = p.small ? kSmallBoxesPerWg : 0;
    p.steps_per_launch = p.small ? slice : 1;
    const size_t fit = budget / p.per_box;
    if (fit < 1)
        return fail("%s: one box needs %zu bytes of scratch (nwater = %d) and does not fit the budget of %zu bytes (MW_PIN_SCRATCH_MB)",
                    who, p.per_box, n, budget);
    const size_t most = p.small ? (size_t)kSmallChunkBoxes : (size_t)kMaxChunkBoxes;
    p.bpc = (int)(fit < most ? fit : most);
    if (p.bpc > nboxes) p.bpc = nboxes;
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

void pin_fields(const Plan& p, const int* grid, int* f)
{
    plan_fields(p, grid, f);
    f[9] = p.steps_per_launch;
}

int check_counts(const char* who, int nboxes, int n)
{
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    return 0;
}

struct Scalars {
    unsigned long long seed;
    int nsteps, sample_every, equil_steps, block_steps;
    double dt, mass, kT, gamma, pressure, tau_p, beta_T;
    int baro_every, coupling, axis;
};

int check_scalars(const char* who, int nboxes, int n, const Scalars& s, Consts& C)
{
    if (check_counts(who, nboxes, n)) return 1;
    if (s.nsteps < 0 || s.nsteps > MW_PIN_MAX_STEPS) return fail("%s: nsteps = %d outside 0..%d", who, s.nsteps, MW_PIN_MAX_STEPS);
    if (s.sample_every < 1) return fail("%s: sample_every = %d is not at least 1", who, s.sample_every);
    if (s.equil_steps < 0) return fail("%s: equil_steps = %d is negative", who, s.equil_steps);
    if (s.block_steps < 0) return fail("%s: block_steps = %d is negative", who, s.block_steps);
    if (!(s.dt > 0.0) || !std::isfinite(s.dt)) return fail("%s: dt = %g atomic time units is not a finite number > 0", who, s.dt);
    if (!(s.mass > 0.0) || !std::isfinite(s.mass)) return fail("%s: mass = %g electron masses is not a finite number > 0", who, s.mass);
    if (!(s.kT >= 0.0) || !std::isfinite(s.kT)) return fail("%s: kT = %g Hartree is not a finite number >= 0", who, s.kT);
    if (!(s.gamma >= 0.0) || !std::isfinite(s.gamma)) return fail("%s: gamma = %g per atomic time unit is not a finite number >= 0", who, s.gamma);
    if (!std::isfinite(s.pressure)) return fail("%s: pressure = %g Hartree / bohr^3 is not a finite number", who, s.pressure);
    if (!(s.tau_p > 0.0) || !std::isfinite(s.tau_p)) return fail("%s: tau_p = %g atomic time units is not a finite number > 0", who, s.tau_p);
    if (!(s.beta_T > 0.0) || !std::isfinite(s.beta_T)) return fail("%s: beta_T = %g bohr^3 / Hartree is not a finite number > 0", who, s.beta_T);
    if (s.baro_every < 0) return fail("%s: baro_every = %d is negative", who, s.baro_every);
    if (s.coupling < MW_PIN_ISO || s.coupling > MW_PIN_UNIAXIAL) return fail("%s: coupling = %d outside 0..3", who, s.coupling);
    if (s.axis < 0 || s.axis > 2) return fail("%s: axis = %d outside 0..2", who, s.axis);
    C.hk = s.dt / (2.0 * s.mass);
    C.hd = s.dt / 2.0;
    C.c1 = std::exp(-s.gamma * s.dt);
    C.c2 = std::sqrt((s.kT / s.mass) * (1.0 - C.c1 * C.c1));
    C.lim2 = (mw::kSigA / 4.0) * (mw::kSigA / 4.0);
    C.hm = s.mass / 2.0;
    const double dtb = (double)s.baro_every * s.dt;
    C.cb = s.beta_T * dtb / s.tau_p;
    C.cn = std::sqrt(2.0 * s.kT * C.cb);
    C.cb3 = C.cb / 3.0;
    C.cn1 = std::sqrt(2.0 * s.kT * C.cb3 / 1.0);
    C.cn2 = std::sqrt(2.0 * s.kT * C.cb3 / 2.0);
    C.pressure = s.pressure;
    C.seed_lo = (uint32_t)s.seed;
    C.seed_hi = (uint32_t)(s.seed >> 32);
    C.thermostat = s.gamma > 0.0 ? 1 : 0;
    C.nsteps = s.nsteps;
    C.sample_every = s.sample_every;
    C.nrows = s.nsteps / s.sample_every + 1;
    C.baro_noise = s.kT > 0.0 ? 1 : 0;
    C.coupling = s.coupling;
    C.axis = s.axis;
    C.equil = s.equil_steps;
    C.block_steps = s.block_steps;
    C.nblocks = (s.block_steps > 0 && s.nsteps >= s.equil_steps) ? (s.nsteps - s.equil_steps) / s.block_steps : 0;
    if (!std::isfinite(C.hk) || !(C.hk > 0.0)) return fail("%s: dt / (2 mass) = %g with dt = %g and mass = %g is not a finite number > 0", who, C.hk, s.dt, s.mass);
    if (!std::isfinite(C.c2)) return fail("%s: kT = %g over mass = %g is not finite", who, s.kT, s.mass);
    if (!std::isfinite(C.cb) || !std::isfinite(C.cn))
        return fail("%s: beta_T = %g times baro_every dt = %g over tau_p = %g is not finite", who, s.beta_T, dtb, s.tau_p);
    return 0;
}

// the first box of a host array [nboxes][n][3] that holds a value that is not finite, or -1
int first_bad_box(const double* a, int nboxes, int n)
{
    if (!a) return -1;
    const size_t per = 3 * (size_t)n;
    for (int b = 0; b < nboxes; ++b)
        for (size_t k = 0; k < per; ++k)
            if (!std::isfinite(a[per * b + k])) return b;
    return -1;
}

int report_bad(const char* who, int bpos, int bvel, int bref)
{
    if (bpos >= 0) return fail("%s: pos: box %d holds a position that is not finite", who, bpos);
    if (bvel >= 0) return fail("%s: vel: box %d holds a velocity that is not finite", who, bvel);
    if (bref >= 0) return fail("%s: pos_ref: box %d holds a position that is not finite", who, bref);
    return 0;
}

// nvec, kappas and anchors (host) checked, and what the kernels read made of them: pin [box][kPin] = (n_1, n_2, n_3, kappa, a)
int check_bias(const char* who, int nboxes, const int* nvec, const double* kappas, const double* anchors, std::vector<double>& pin)
{
    pin.resize((size_t)kPin * nboxes);
    for (int b = 0; b < nboxes; ++b) {
        const int* v = nvec + 3 * (size_t)b;
        for (int a = 0; a < 3; ++a)
            if (v[a] < -MW_PIN_MAX_N || v[a] > MW_PIN_MAX_N)
                return fail("%s: nvec: box %d holds n = (%d, %d, %d), a component outside -%d..%d", who, b, v[0], v[1], v[2], MW_PIN_MAX_N, MW_PIN_MAX_N);
        if (v[0] == 0 && v[1] == 0 && v[2] == 0) return fail("%s: nvec: box %d holds n = (0, 0, 0)", who, b);
        if (!(kappas[b] >= 0.0) || !std::isfinite(kappas[b]))
            return fail("%s: kappas: box %d holds kappa = %g Hartree, not a finite number >= 0", who, b, kappas[b]);
        if (!(anchors[b] >= 0.0) || !std::isfinite(anchors[b])) return fail("%s: anchors: box %d holds a = %g, not a finite number >= 0", who, b, anchors[b]);
        double* P = pin.data() + (size_t)kPin * b;
        P[0] = (double)v[0]; P[1] = (double)v[1]; P[2] = (double)v[2]; P[3] = kappas[b]; P[4] = anchors[b];
    }
    return 0;
}

const char kRadius[] = "a_sigma";             // the radius the cells are checked against, in the messages

int check_live(const char* who) { return check_live(who, "mw_pin_init", g); }

int env_int(const char* who, const char* name, int lo, int hi, int& value)
{
    const char* s = getenv(name);
    if (!s || !*s) return 0;
    char* end = nullptr;
    const long v = strtol(s, &end, 10);
    if (end == s || *end || v < lo || v > hi) return fail("%s: %s = '%s' is not a number in %d..%d", who, name, s, lo, hi);
    value = (int)v;
    return 0;
}

// An event on the stream; the time from it to the next one belongs to `bucket` (-1: to nothing).
int mark(int bucket)
{
    HIPOK(hipEventRecord(g.pool[g.used], g.stream));
    g.bucket[g.used++] = bucket;
    return 0;
}

// waits for what has been enqueued and adds the marked intervals to ms
int harvest(float* ms)
{
    HIPOK(hipStreamSynchronize(g.stream));
    for (int k = 0; k + 1 < g.used; ++k) {
        if (g.bucket[k] < 0) continue;
        float t = 0.0f;
        HIPOK(hipEventElapsedTime(&t, g.pool[k], g.pool[k + 1]));
        ms[g.bucket[k]] += t;
    }
    g.used = 0;
    return 0;
}

int harvest_if_full(float* ms) { return g.used + kPoolSlack > kPool ? harvest(ms) : 0; }

struct Arrays {
    const double *cells, *pos, *vel, *ref;
    const double* pin;                             // host, [nboxes][kPin], whatever the other arrays are
    const unsigned long long* streams;
    double *pos_out, *vel_out, *forces, *cells_out, *ref_out, *trace, *blocks;
    int* status;
};

// the pointers of a chunk's scratch
struct Chunk {
    int n, nb, b0;
    dim3 grid_m;
    const Layout* l;
    char* base;
    size_t B;
    double *x, *v, *F, *ref, *row, *acc, *cell, *par, *cv, *mom, *en, *part, *rpart, *bias, *trace, *blocks;
    const double* pin;
    double2* pair;
    int *si, *grid;
    const unsigned long long* streams;
};

// sort, moments, forces and row of the general geometry for the evaluation that ends step e
int evaluate_general(const Chunk& k, const Consts& C, int e, int do6, int do1, int tally)
{
    Sorted s;
    if (mark(kSort)) return 1;
    if (sort_into_cells(g.stream, k.n, k.nb, *k.l, k.base, k.B, k.par, k.grid, (const double*)k.x, s)) return 1;
    if (mark(kMoments)) return 1;
    hipLaunchKernelGGL(k_pin_moments, k.grid_m, dim3(kThreads), 0, g.stream, k.n, k.l->cap, (const double*)k.par, (const int*)k.grid, s.start, s.ss,
                       (const int*)k.si, k.pin, k.mom, k.en, k.pair, k.rpart);
    HIPOK(hipGetLastError());
    if (mark(kRho)) return 1;
    hipLaunchKernelGGL(k_pin_rho, dim3((unsigned)k.nb), dim3(64), 0, g.stream, k.l->nwg, k.n, (const double*)k.par, (const int*)k.si, k.pin,
                       (const double*)k.rpart, k.bias);
    HIPOK(hipGetLastError());
    if (mark(kForces)) return 1;
    hipLaunchKernelGGL(k_pin_forces, k.grid_m, dim3(kThreads), 0, g.stream, k.n, k.l->cap, C, do6, do1, (const double*)k.par, (const int*)k.grid, s.start,
                       s.ss, s.idx, k.si, (const double*)k.mom, (const double*)k.en, (const double*)k.ref, (const double*)k.x, (const double2*)k.pair,
                       (const double*)k.bias, k.v, k.F, k.part);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_pin_row, dim3((unsigned)k.nb), dim3(64), 0, g.stream, k.l->nwg, k.n, e, tally, C, (const double*)k.part, (const double*)k.cv, k.pin,
                       (const double*)k.bias, k.row, k.acc, k.si, k.trace, k.blocks);
    HIPOK(hipGetLastError());
    return mark(-1);
}

// the barostat stage after stage 6 of the step with index `step`
int barostat(const Chunk& k, const Consts& C, unsigned long long step, int fill)
{
    if (mark(kBaro)) return 1;
    hipLaunchKernelGGL(k_pin_baro, dim3((unsigned)((k.nb + 63) / 64)), dim3(64), 0, g.stream, k.nb, k.l->cap, C, k.streams, k.b0, step, fill,
                       (const double*)k.row, k.si, k.cell, k.par, k.grid, k.cv, k.trace);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_pin_scale, k.grid_m, dim3(kThreads), 0, g.stream, k.n, C, (const int*)k.si, (const double*)k.cv, k.x, k.v, k.ref);
    HIPOK(hipGetLastError());
    return mark(-1);
}

// The work of both entries, arguments already checked.  `grid0` is the grid of the first box's input cell (the plan fields); the
// arrays of `a` are device pointers when `dev`, host pointers otherwise.
int run(const char* who, int nboxes, int n, const int* grid0, const Consts& C, unsigned long long step0, int baro_every, bool dev, const Arrays& a)
{
    Plan p;
    if (make_plan(who, n, nboxes, g.budget, g.slice, p)) return 1;
    const Layout& l = p.lay;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (reserve(g.scratch, p.per_box * (size_t)p.bpc)) return 1;
    const size_t vec = 24 * (size_t)n, rowbytes = 8 * (size_t)kOut * C.nrows, blockbytes = 8 * (size_t)kAcc * C.nblocks;
    const bool want_blocks = a.blocks && C.nblocks > 0;
    if (reserve(g.pin, 8 * (size_t)kPin * p.bpc)) return 1;
    if (!dev) {
        if (reserve(g.cells, 72 * (size_t)p.bpc)) return 1;
        if (reserve(g.pos, vec * p.bpc)) return 1;
        if (a.vel && reserve(g.vel, vec * p.bpc)) return 1;
        if (a.ref && reserve(g.ref, vec * p.bpc)) return 1;
        if (a.streams && reserve(g.streams, 8 * (size_t)p.bpc)) return 1;
        if (a.pos_out && reserve(g.pos_out, vec * p.bpc)) return 1;
        if (a.vel_out && reserve(g.vel_out, vec * p.bpc)) return 1;
        if (a.forces && reserve(g.forces, vec * p.bpc)) return 1;
        if (a.cells_out && reserve(g.cells_out, 72 * (size_t)p.bpc)) return 1;
        if (a.ref_out && reserve(g.ref_out, vec * p.bpc)) return 1;
        if (a.trace && reserve(g.trace, rowbytes * p.bpc)) return 1;
        if (want_blocks && reserve(g.blocks, blockbytes * p.bpc)) return 1;
        if (a.status && reserve(g.status, 8 * (size_t)p.bpc)) return 1;
    }
    float ms[kTimers] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const int evals = C.nsteps + 1;
    const unsigned long long be = (unsigned long long)baro_every;
    // evaluation e >= 1 ends the step with index t = step0 + e - 1; the barostat follows it when (t + 1) % baro_every == 0
    auto baro_at = [&](int e) { return be > 0 && e > 0 && (step0 + (unsigned long long)e) % be == 0; };
    g.used = 0;
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const size_t first = 3 * (size_t)n * b0;
        const double* d_cells = a.cells + 9 * (size_t)b0;
        const double* d_pos = a.pos + first;
        const double* d_vel = a.vel ? a.vel + first : nullptr;
        const double* d_ref = a.ref ? a.ref + first : nullptr;
        const unsigned long long* d_streams = a.streams ? a.streams + b0 : nullptr;
        HIPOK(hipMemcpyAsync(g.pin.p, a.pin + (size_t)kPin * b0, 8 * (size_t)kPin * nb, hipMemcpyHostToDevice, g.stream));
        if (!dev) {
            HIPOK(hipMemcpyAsync(g.cells.p, d_cells, 72 * (size_t)nb, hipMemcpyHostToDevice, g.stream));
            d_cells = (const double*)g.cells.p;
            HIPOK(hipMemcpyAsync(g.pos.p, d_pos, vec * nb, hipMemcpyHostToDevice, g.stream));
            d_pos = (const double*)g.pos.p;
            if (d_vel) { HIPOK(hipMemcpyAsync(g.vel.p, d_vel, vec * nb, hipMemcpyHostToDevice, g.stream)); d_vel = (const double*)g.vel.p; }
            if (d_ref) { HIPOK(hipMemcpyAsync(g.ref.p, d_ref, vec * nb, hipMemcpyHostToDevice, g.stream)); d_ref = (const double*)g.ref.p; }
            if (d_streams) {
                HIPOK(hipMemcpyAsync(g.streams.p, d_streams, 8 * (size_t)nb, hipMemcpyHostToDevice, g.stream));
                d_streams = (const unsigned long long*)g.streams.p;
            }
        }
        double* d_out = !a.pos_out ? nullptr : dev ? a.pos_out + first : (double*)g.pos_out.p;
        double* d_vout = !a.vel_out ? nullptr : dev ? a.vel_out + first : (double*)g.vel_out.p;
        double* d_forces = !a.forces ? nullptr : dev ? a.forces + first : (double*)g.forces.p;
        double* d_cout = !a.cells_out ? nullptr : dev ? a.cells_out + 9 * (size_t)b0 : (double*)g.cells_out.p;
        double* d_rout = !a.ref_out ? nullptr : dev ? a.ref_out + first : (double*)g.ref_out.p;
        double* d_trace = !a.trace ? nullptr : dev ? a.trace + (size_t)kOut * C.nrows * b0 : (double*)g.trace.p;
        double* d_blocks = !want_blocks ? nullptr : dev ? a.blocks + (size_t)kAcc * C.nblocks * b0 : (double*)g.blocks.p;
        int* d_status = !a.status ? nullptr : dev ? a.status + 2 * (size_t)b0 : (int*)g.status.p;
        Chunk k;
        k.n = n; k.nb = nb; k.b0 = b0; k.l = &l;
        k.grid_m = per_molecule(n, nb);
        k.base = (char*)g.scratch.p;
        k.B = (size_t)p.bpc;
        k.x = (double*)(k.base + l.x * k.B);
        k.v = (double*)(k.base + l.v * k.B);
        k.F = (double*)(k.base + l.F * k.B);
        k.ref = (double*)(k.base + l.ref * k.B);
        k.row = (double*)(k.base + l.row * k.B);
        k.si = (int*)(k.base + l.si * k.B);
        k.cell = (double*)(k.base + l.cell * k.B);
        k.par = (double*)(k.base + l.par * k.B);
        k.grid = (int*)(k.base + l.grid * k.B);
        k.cv = (double*)(k.base + l.cv * k.B);
        k.mom = (double*)(k.base + l.mom * k.B);
        k.en = (double*)(k.base + l.en * k.B);
        k.part = (double*)(k.base + l.part * k.B);
        k.pair = (double2*)(k.base + l.pair * k.B);
        k.rpart = (double*)(k.base + l.rpart * k.B);
        k.bias = (double*)(k.base + l.bias * k.B);
        k.acc = (double*)(k.base + l.acc * k.B);
        k.pin = (const double*)g.pin.p;
        k.trace = d_trace;
        k.blocks = d_blocks;
        k.streams = d_streams;
        hipLaunchKernelGGL(k_pin_begin, k.grid_m, dim3(kThreads), 0, g.stream, n, l.cap, d_cells, d_pos, d_vel, d_ref, k.x, k.v, k.F, k.ref, k.row, k.si,
                           k.cell, k.par, k.grid, k.cv, k.acc);
        HIPOK(hipGetLastError());
        if (p.small) {
            const dim3 grid_s((unsigned)((nb + kSmallBoxesPerWg - 1) / kSmallBoxesPerWg));
            int e0 = 0;
            bool again = false;
            while (e0 < evals) {
                int last = evals - e0 < g.slice ? evals - 1 : e0 + g.slice - 1;
                bool hold = false;
                if (be > 0) {                                                   // the first barostat evaluation from `from` on
                    const int from = again ? e0 + 1 : (e0 > 1 ? e0 : 1);
                    const unsigned long long r = (step0 + (unsigned long long)from) % be;
                    const unsigned long long eb = (unsigned long long)from + (r ? be - r : 0);
                    if (eb <= (unsigned long long)last) { last = (int)eb; hold = true; }
                }
                if (mark(kForces)) return 1;
                hipLaunchKernelGGL(C.thermostat ? k_pin_small<true> : k_pin_small<false>, grid_s, dim3(kThreads), 0, g.stream, nb, n, e0, last - e0 + 1,
                                   again ? 1 : 0, hold ? 1 : 0, C, d_streams, b0, step0, (const double*)k.par, (const double*)k.cv, (const double*)k.ref, k.pin,
                                   k.x, k.v, k.F, k.row, k.acc, k.si, d_trace, d_blocks);
                HIPOK(hipGetLastError());
                if (mark(-1)) return 1;
                if (hold) {
                    if (barostat(k, C, step0 + (unsigned long long)(last - 1), 1)) return 1;
                    e0 = last;
                    again = true;
                } else {
                    e0 = last + 1;
                    again = false;
                }
                if (harvest_if_full(ms)) return 1;
            }
        } else {
            for (int e = 0; e < evals; ++e) {
                const bool baro = baro_at(e);
                if (e > 0) {
                    if (mark(kDrift)) return 1;
                    hipLaunchKernelGGL(k_pin_drift1, k.grid_m, dim3(kThreads), 0, g.stream, n, C, d_streams, b0, step0 + (unsigned long long)(e - 1), k.x, k.v,
                                       k.si);
                    HIPOK(hipGetLastError());
                    hipLaunchKernelGGL(k_pin_drift2, k.grid_m, dim3(kThreads), 0, g.stream, n, C.hd, k.x, (const double*)k.v, (const int*)k.si);
                    HIPOK(hipGetLastError());
                }
                if (evaluate_general(k, C, e, e > 0 ? 1 : 0, e < C.nsteps && !baro ? 1 : 0, baro ? 0 : 1)) return 1;
                if (baro) {
                    if (barostat(k, C, step0 + (unsigned long long)(e - 1), 0)) return 1;
                    if (evaluate_general(k, C, e, 0, e < C.nsteps ? 1 : 0, 1)) return 1;
                }
                if (harvest_if_full(ms)) return 1;
            }
        }
        if (harvest(ms)) return 1;
        hipLaunchKernelGGL(k_pin_finish, k.grid_m, dim3(kThreads), 0, g.stream, n, (const double*)k.x, (const double*)k.v, (const double*)k.F,
                           (const double*)k.ref, (const int*)k.si, (const double*)k.cell, d_out, d_vout, d_forces, d_rout, d_cout, d_status);
        HIPOK(hipGetLastError());
        if (!dev) {
            if (a.pos_out) HIPOK(hipMemcpyAsync(a.pos_out + first, g.pos_out.p, vec * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.vel_out) HIPOK(hipMemcpyAsync(a.vel_out + first, g.vel_out.p, vec * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.forces) HIPOK(hipMemcpyAsync(a.forces + first, g.forces.p, vec * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.cells_out) HIPOK(hipMemcpyAsync(a.cells_out + 9 * (size_t)b0, g.cells_out.p, 72 * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
            if (a.ref_out) HIPOK(hipMemcpyAsync(a.ref_out + first, g.ref_out.p, vec * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.trace) HIPOK(hipMemcpyAsync(a.trace + (size_t)kOut * C.nrows * b0, g.trace.p, rowbytes * nb, hipMemcpyDeviceToHost, g.stream));
            if (want_blocks) HIPOK(hipMemcpyAsync(a.blocks + (size_t)kAcc * C.nblocks * b0, g.blocks.p, blockbytes * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.status) HIPOK(hipMemcpyAsync(a.status + 2 * (size_t)b0, g.status.p, 8 * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
        }
        HIPOK(hipStreamSynchronize(g.stream));               // the next chunk reuses the scratch and the staging buffers
    }
    pin_fields(p, grid0, g.last);
    g.have_last = true;
    for (int t = 0; t < kTimers; ++t) g.ms[t] = ms[t];
    return 0;
}

}  // namespace

extern "C" {

const char* mw_pin_last_error(void) { return g_err; }
int mw_pin_is_initialised(void) { return g.live ? 1 : 0; }

int mw_pin_init(int device)
{
    const char* who = "mw_pin_init";
    if (g.live) return fail("%s: already initialised", who);
    int slice = kDefaultSlice;
    if (env_int(who, "MW_PIN_SLICE", 1, kMaxSlice, slice)) return 1;
    if (runtime_init(who, "MW_PIN_SCRATCH_MB", device, g)) return 1;
    g.slice = slice;
    DeviceScope scope;
    hipError_t e = scope.enter(g.device);
    g.pool.assign((size_t)kPool, nullptr);
    g.bucket.assign((size_t)kPool, -1);
    for (auto& ev : g.pool) {
        if (e != hipSuccess) break;
        e = hipEventCreate(&ev);
    }
    if (e != hipSuccess) {                                     // give back what was made before failing
        for (auto& ev : g.pool) if (ev) (void)hipEventDestroy(ev);
        g.pool.clear();
        (void)runtime_finalize(g, {});
        g = State{};
        return fail("%s: hipEventCreate: %s", who, hipGetErrorString(e));
    }
    return 0;
}

int mw_pin_finalize(void)
{
    if (g.live) {
        DeviceScope scope;
        HIPOK(scope.enter(g.device));
        HIPOK(hipStreamSynchronize(g.stream));
        for (auto& ev : g.pool) HIPOK(hipEventDestroy(ev));
        g.pool.clear();
    }
    if (runtime_finalize(g, {&g.scratch, &g.cells, &g.pos, &g.vel, &g.ref, &g.streams, &g.pin, &g.pos_out, &g.vel_out, &g.forces, &g.cells_out,
                             &g.ref_out, &g.trace, &g.blocks, &g.status, &g.bad}))
        return 1;
    g = State{};
    return 0;
}

int mw_pin_run(int nboxes, int nwater, const double* cells, const double* pos, const double* vel, const double* pos_ref, const int* nvec,
               const double* kappas, const double* anchors, const unsigned long long* streams, unsigned long long seed, unsigned long long step0,
               int nsteps, int sample_every, int equil_steps, int block_steps, double dt, double mass, double kT, double gamma, double pressure,
               double tau_p, double beta_T, int baro_every, int coupling, int axis, double* pos_out, double* vel_out, double* forces,
               double* cells_out, double* ref_out, double* trace, double* blocks, int* status)
{
    const char* who = "mw_pin_run";
    std::vector<double> par, pin;
    std::vector<int> grid;
    Consts C;
    if (check_scalars(who, nboxes, nwater,
                      Scalars{seed, nsteps, sample_every, equil_steps, block_steps, dt, mass, kT, gamma, pressure, tau_p, beta_T, baro_every, coupling, axis}, C))
        return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (!nvec) return fail("%s: nvec is NULL", who);
    if (!kappas) return fail("%s: kappas is NULL", who);
    if (!anchors) return fail("%s: anchors is NULL", who);
    if (check_bias(who, nboxes, nvec, kappas, anchors, pin)) return 1;
    if (check_cells(who, kRadius, nboxes, nwater, cells, mw::kSigA, par, grid)) return 1;
    if (report_bad(who, first_bad_box(pos, nboxes, nwater), first_bad_box(vel, nboxes, nwater), first_bad_box(pos_ref, nboxes, nwater))) return 1;
    if (check_live(who)) return 1;
    return run(who, nboxes, nwater, grid.data(), C, step0, baro_every, false,
               Arrays{cells, pos, vel, pos_ref, pin.data(), streams, pos_out, vel_out, forces, cells_out, ref_out, trace, blocks, status});
}

int mw_pin_run_device(int nboxes, int nwater, const double* cells, const double* pos, const double* vel, const double* pos_ref, const int* nvec,
                      const double* kappas, const double* anchors, const unsigned long long* streams, unsigned long long seed,
                      unsigned long long step0, int nsteps, int sample_every, int equil_steps, int block_steps, double dt, double mass, double kT,
                      double gamma, double pressure, double tau_p, double beta_T, int baro_every, int coupling, int axis, double* pos_out,
                      double* vel_out, double* forces, double* cells_out, double* ref_out, double* trace, double* blocks, int* status)
{
    const char* who = "mw_pin_run_device";
    std::vector<double> par, pin;
    std::vector<int> grid;
    Consts C;
    if (check_scalars(who, nboxes, nwater,
                      Scalars{seed, nsteps, sample_every, equil_steps, block_steps, dt, mass, kT, gamma, pressure, tau_p, beta_T, baro_every, coupling, axis}, C))
        return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (!nvec) return fail("%s: nvec is NULL", who);
    if (!kappas) return fail("%s: kappas is NULL", who);
    if (!anchors) return fail("%s: anchors is NULL", who);
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (fetch_cells(who, kRadius, nboxes, nwater, cells, mw::kSigA, par, grid)) return 1;
    // the bias of every box, read back (20 bytes per box) and checked on the host (fetch_cells has waited for whoever made the inputs)
    std::vector<int> h_nvec(3 * (size_t)nboxes);
    std::vector<double> h_kappas((size_t)nboxes), h_anchors((size_t)nboxes);
    HIPOK(hipMemcpy(h_nvec.data(), nvec, 12 * (size_t)nboxes, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(h_kappas.data(), kappas, 8 * (size_t)nboxes, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(h_anchors.data(), anchors, 8 * (size_t)nboxes, hipMemcpyDeviceToHost));
    if (check_bias(who, nboxes, h_nvec.data(), h_kappas.data(), h_anchors.data(), pin)) return 1;
    // the verdict on the positions and velocities: one kernel that writes three ints, read before anything else is launched
    if (reserve(g.bad, 3 * sizeof(int))) return 1;
    int bad[3] = {nboxes, nboxes, nboxes};
    HIPOK(hipMemcpyAsync(g.bad.p, bad, sizeof bad, hipMemcpyHostToDevice, g.stream));
    const size_t total = (size_t)nboxes * nwater, blocks_ = (total + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_pin_check, dim3((unsigned)(blocks_ < 65536 ? blocks_ : 65536)), dim3(kThreads), 0, g.stream, total, nwater, pos, vel, pos_ref,
                       (int*)g.bad.p);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(bad, g.bad.p, sizeof bad, hipMemcpyDeviceToHost, g.stream));
    HIPOK(hipStreamSynchronize(g.stream));
    if (report_bad(who, bad[0] < nboxes ? bad[0] : -1, bad[1] < nboxes ? bad[1] : -1, bad[2] < nboxes ? bad[2] : -1)) return 1;
    return run(who, nboxes, nwater, grid.data(), C, step0, baro_every, true,
               Arrays{cells, pos, vel, pos_ref, pin.data(), streams, pos_out, vel_out, forces, cells_out, ref_out, trace, blocks, status});
}

int mw_pin_plan(int nwater, const double* cell, int nboxes, int* out, int nout)
{
    const char* who = "mw_pin_plan";
    std::vector<int> grid;
    if (check_counts(who, nboxes, nwater)) return 1;
    if (plan_grid(who, kRadius, nwater, cell, mw::kSigA, out, nout, grid)) return 1;
    Plan p;
    if (make_plan(who, nwater, nboxes, g.live ? g.budget : kDefaultBudget, g.live ? g.slice : kDefaultSlice, p)) return 1;
    int f[MW_PIN_PLAN_FIELDS];
    pin_fields(p, grid.data(), f);
    copy_fields(f, MW_PIN_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_pin_last(int* out, int nout) { return last_fields("mw_pin_last", "mw_pin_init", g, g.last, MW_PIN_PLAN_FIELDS, out, nout); }

int mw_pin_elapsed_ms(float* sort, float* moments, float* forces, float* drift, float* barostat, float* rho)
{
    if (check_live("mw_pin_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_pin_elapsed_ms: no call has launched yet");
    if (sort) *sort = g.ms[kSort];
    if (moments) *moments = g.ms[kMoments];
    if (forces) *forces = g.ms[kForces];
    if (drift) *drift = g.ms[kDrift];
    if (barostat) *barostat = g.ms[kBaro];
    if (rho) *rho = g.ms[kRho];
    return 0;
}

}  // extern "C"
