// libmw_nuc.so -- the nucleus-size molecular dynamics of include/mw_nuc.h: the step of libmw_flex.so's general geometry, restated
// (k_nuc_drift1 / k_nuc_drift2, the counting sort of mw_lib_cells.h, k_nuc_moments, k_nuc_forces, k_nuc_row, and at a barostat step
// k_nuc_baro and k_nuc_scale and the evaluation again), and every check_every steps the size of the largest cluster of solid-like
// molecules of every box: k_nuc_q6 and k_nuc_conn (the two walks of libmw_boo.so's general geometry restricted to l = 6, on the
// grid and the sort of the force evaluation that has just run) and k_nuc_clusters (one workgroup per box, the hook / compress
// scheme of the engine's mw_ice_clusters.hip.h), whose tail applies the stopping rule to the box's flags.  At such a step the
// force pass leaves stage 1 of the next step out and k_nuc_kick1 / k_nuc_latch apply it to the boxes that go on, so that a
// stopped box holds the state mw_flex_run leaves after that many steps.  k_nuc_begin copies the state in and sets every box's
// par and grid up on the device, k_nuc_finish writes the results.  Flags of a box (its ints): [0] frozen, read by every kernel
// and written by k_nuc_row, k_nuc_baro, k_nuc_latch and the tail of k_nuc_clusters (one writer per box and launch); [1] the first
// guard failed (k_nuc_forces, k_nuc_kick1), [2] the second (k_nuc_drift1); [3] steps completed; [4] the barostat guard refused;
// [5] the stopping rule's code (3, 4 or 0); [6] hook rounds, summed over the box's evaluations; [7] spare -- no kernel reads a
// flag that the same launch may write, but k_nuc_clusters its own box's [0], before a barrier that its one writer passes after.
//
// The short pieces of the step (Philox, the normals, kick, drift, guard), the cell routine and the kernels of the step are those
// of libmw_flex.so, restated as that library restates the MD and NPT libraries': a header for them would become a dependency
// of libraries whose lists of dependencies are part of their contracts.  The force pass, the virial and the stress come from
// mw_lib_forces.h alone, the harmonics from mw_lib_harmonics.h, shared with libmw_boo.so.
#include "../../include/mw_nuc.h"
#include "../../include/mw_flex.h"             // the couplings and the barostat's limits (constants only)

#include "mw_common.hip.h"

#include <cstdint>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too
#include "mw_lib_cells.h"
#include "mw_lib_forces.h"
#include "mw_lib_harmonics.h"

namespace mwnuc {

using namespace mwcells;
using namespace mwforces;
using namespace mwharm;

constexpr int kSums = 16;                         // a workgroup's partial sums: E, v.v, |x - ref|^2, W, six hm v_a v_b, six shares of the stress
constexpr int kPart = kSums + 1;                  // those and the largest |F| component
constexpr int kOut = MW_NUC_TRACE_FIELDS;         // doubles of a trace row: E, K, msd, fmax, V, P, six P_ab, three lengths; lambda, solid-like, clusters
constexpr int kOp = 15;                           // the first of the three columns the cluster pass writes; k_nuc_row carries them along
constexpr int kRow = kOut + 1;                    // a box's current row: those and W
constexpr int kSI = 8;                            // ints: frozen, first guard, second guard, steps completed, barostat guard, stop code, hook rounds (1 spare)
constexpr int kRec = 14;                          // doubles per molecule in scratch, sorted order: q_6m, |q_6|
constexpr int kList = MW_NUC_LIST;                // entries of a molecule kept as a list (sorted places) for the cluster rounds
constexpr int kClusterBlock = 1024;
constexpr int kClusterNone = 0x7fffffff;
constexpr int kClusterStaticLds = 512;            // the static __shared__ arrays of k_nuc_clusters fit in this (static_assert there)
constexpr int kLdsBytes = 160 * 1024;
constexpr int kCV = 8;                            // doubles: V, the last three mu, the lengths of the three cell vectors (1 spare)
constexpr double kTwoPi = 6.283185307179586476925286766559;

// The constants of a call, formed on the host (mw_flex.h), and what names its noise.
struct Consts {
    double hk, hd, c1, c2, lim2, hm;
    double cb, cn, pressure;
    double cb3, cn1, cn2;
    uint32_t seed_lo, seed_hi;
    int thermostat, nsteps, sample_every, nrows, baro_noise;
    int coupling, axis;
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
__device__ __forceinline__ bool axis_moves(const Consts& C, int j) { return C.coupling != MW_FLEX_UNIAXIAL || j == C.axis; }

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

// ---- the verdict on device arrays, the state of a chunk at its start, the results at its end -------------------
// bad[k] = the first box whose array k (pos, vel, pos_ref) holds a value that is not finite; arrays may be NULL.
__global__ __launch_bounds__(kThreads) void k_nuc_check(size_t total, int n, const double* __restrict__ pos, const double* __restrict__ vel,
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
__global__ __launch_bounds__(kThreads) void k_nuc_begin(int n, int cap, const double* __restrict__ cells, const double* __restrict__ pos,
                                                         const double* __restrict__ vel, const double* __restrict__ pos_ref, double* __restrict__ x,
                                                         double* __restrict__ v, double* __restrict__ F, double* __restrict__ ref,
                                                         double* __restrict__ row, int* __restrict__ si, double* __restrict__ cell,
                                                         double* __restrict__ par, int* __restrict__ grid, double* __restrict__ cv)
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

// One lane per molecule: the state, (n_i, conn_i) and the label out; the first lane of a box writes its status, its cell and op.
__global__ __launch_bounds__(kThreads) void k_nuc_finish(int n, const double* __restrict__ x, const double* __restrict__ v, const double* __restrict__ F,
                                                          const double* __restrict__ ref, const int* __restrict__ si, const double* __restrict__ cell,
                                                          double* __restrict__ pos_out, double* __restrict__ vel_out, double* __restrict__ forces,
                                                          double* __restrict__ ref_out, double* __restrict__ cells_out, int* __restrict__ status,
                                                          const int* __restrict__ nn, const int* __restrict__ label, const int* __restrict__ op,
                                                          int* __restrict__ nn_out, int* __restrict__ label_out, int* __restrict__ op_out)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    if (pos_out) { pos_out[m] = x[m]; pos_out[m + 1] = x[m + 1]; pos_out[m + 2] = x[m + 2]; }
    if (vel_out) { vel_out[m] = v[m]; vel_out[m + 1] = v[m + 1]; vel_out[m + 2] = v[m + 2]; }
    if (forces) { forces[m] = F[m]; forces[m + 1] = F[m + 1]; forces[m + 2] = F[m + 2]; }
    if (ref_out) { ref_out[m] = ref[m]; ref_out[m + 1] = ref[m + 1]; ref_out[m + 2] = ref[m + 2]; }
    if (nn_out) { nn_out[2 * (m / 3)] = nn[2 * (m / 3)]; nn_out[2 * (m / 3) + 1] = nn[2 * (m / 3) + 1]; }
    if (label_out) label_out[m / 3] = label[m / 3];
    if (i == 0) {
        const int* I = si + kSI * (size_t)b;
        if (status) {
            status[2 * (size_t)b] = I[3];
            status[2 * (size_t)b + 1] = I[5] ? I[5] : I[4] ? 2 : (I[0] | I[1] | I[2]) ? 1 : 0;
        }
        if (op_out)
            for (int k = 0; k < 4; ++k) op_out[4 * (size_t)b + k] = op[4 * (size_t)b + k];
        if (cells_out)
            for (int k = 0; k < 9; ++k) cells_out[9 * (size_t)b + k] = cell[9 * (size_t)b + k];
    }
}

// ---- the barostat ---------------------------------------------------------------------------------------------------------------
// One lane per box after stage 6 of the step with index `step`: the decision of mw_flex.h from the box's row (K, W, P_aa) and
// volume.  Accepted: the three mu, the volume and the lengths to cv, the scaled cell and its par and grid in place.  Refused: the
// box is frozen with the barostat's code and nothing of its cell is touched.
__global__ __launch_bounds__(64) void k_nuc_baro(int nb, int cap, Consts C, const unsigned long long* __restrict__ streams, int b0,
                                                  unsigned long long step, const double* __restrict__ row, int* __restrict__ si,
                                                  double* __restrict__ cell, double* __restrict__ par, int* __restrict__ grid, double* __restrict__ cv)
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
    if (C.coupling == MW_FLEX_ISO) {                                     // the stage of the NPT library
        const double P = pressure_of(R[1], R[kOut], V);
        double de = -(C.cb * (C.pressure - P));
        if (C.baro_noise) {
            const double xi = box_normal(C, id, step, 1u);
            de = __builtin_fma(C.cn, xi / __builtin_sqrt(V), de);
        }
        ok = __builtin_fabs(de) <= MW_FLEX_MAX_DLNV;                     // (a NaN fails)
        if (ok) mu0 = mu1 = mu2 = exp(de / 3.0);
    } else {
        double mu[3] = {1.0, 1.0, 1.0};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (!axis_moves(C, j)) continue;
            // the group of axis j: itself, or with MW_FLEX_SEMI and j != axis the pair of j and the third axis p
            const bool pair = C.coupling == MW_FLEX_SEMI && j != C.axis;
            const int p = pair ? 3 - C.axis - j : j;
            const int lo = p < j ? p : j, hi = p < j ? j : p;
            const double PG = pair ? 0.5 * (R[6 + lo] + R[6 + hi]) : R[6 + j];
            double de = -(C.cb3 * (C.pressure - PG));
            if (C.baro_noise) {
                const double xi = box_normal(C, id, step, 2u + (uint32_t)lo);
                de = __builtin_fma(pair ? C.cn2 : C.cn1, xi / __builtin_sqrt(V), de);
            }
            ok = ok && __builtin_fabs(de) <= MW_FLEX_MAX_DLNL;           // (a NaN fails)
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
    }
}

// One lane per molecule of a box whose application was accepted, every axis a that moves: x_a <- mu_a x_a, pos_ref_a <- mu_a
// pos_ref_a, v_a <- v_a / mu_a.
__global__ __launch_bounds__(kThreads) void k_nuc_scale(int n, Consts C, const int* __restrict__ si, const double* __restrict__ cv, double* __restrict__ x,
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
__global__ __launch_bounds__(kThreads) void k_nuc_drift1(int n, Consts C, const unsigned long long* __restrict__ streams, int b0,
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
__global__ __launch_bounds__(kThreads) void k_nuc_drift2(int n, double hd, double* __restrict__ x, const double* __restrict__ v,
                                                          const int* __restrict__ si)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    const int* I = si + kSI * (size_t)b;
    if (I[0] || I[2] || i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    drift(hd, v[m], v[m + 1], v[m + 2], x[m], x[m + 1], x[m + 2]);
}

// The moment pass, one lane per molecule in sorted order.
__global__ __launch_bounds__(kThreads) void k_nuc_moments(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                           const int* __restrict__ start, const double* __restrict__ ss, const int* __restrict__ si,
                                                           double* __restrict__ mom, double* __restrict__ en)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (si[kSI * (size_t)b] || si[kSI * (size_t)b + 2] || p >= n) return;
    const double* H = par + 18 * (size_t)b;
    const size_t o = (size_t)b * n;
    const double* S = ss + 3 * o;
    const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
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

// The force pass, one lane per molecule in sorted order: the force of the molecule, written by index, its share of the scalar virial
// and of the stress; stage 6 of this step (`do6`: not at the evaluation before the first step and not at the one after a barostat
// application) and stage 1 of the next with its guard (`do1`: not after the last step and not before a barostat application); the
// partial values of the workgroup from the velocities between the two.
__global__ __launch_bounds__(kThreads) void k_nuc_forces(int n, int cap, Consts C, int do6, int do1, const double* __restrict__ par,
                                                          const int* __restrict__ grid, const int* __restrict__ start, const double* __restrict__ ss,
                                                          const int* __restrict__ idx, int* si, const double* __restrict__ mom,
                                                          const double* __restrict__ en, const double* __restrict__ ref, const double* __restrict__ x,
                                                          double* __restrict__ v, double* __restrict__ F, double* __restrict__ part)
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
        const CellRegs hc(H);
        walk_cells(s0, s1, s2, mw::kRcSq, hc.c, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), S,
                   [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
                       if (q == p) return;                             // an image of the molecule itself: d is constant
                       double Mj[kMom];
                       mw::load_moments(Mb + kMom * (size_t)q, Mj);
                       entry_stress(Mi, Mj, r2, dx, dy, dz, fx, fy, fz, dw, st);
                   });
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
__global__ __launch_bounds__(64) void k_nuc_row(int nwg, int n, int e, Consts C, const double* __restrict__ part, const double* __restrict__ cv,
                                                 double* __restrict__ row, int* __restrict__ si, double* __restrict__ trace)
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
        cur[kOut] = sum[3];
        for (int f = 0; f < kRow; ++f) row[kRow * (size_t)b + f] = cur[f];
    }
    __syncthreads();
    if (k < kOut && trace && e % C.sample_every == 0) trace[((size_t)b * C.nrows + e / C.sample_every) * kOut + k] = cur[k];
    if (k == 0) {
        if (!frozen) I[3] = e;
        if (frozen || tripped) I[0] = 1;
    }
}

// ---- the order parameter (include/mw_nuc.h) ---------------------------------------------------------------------------------------
// Per box in scratch, in cell order: rec [n][kRec], cnt [n] (n_i), sol [n] (1: solid-like), list [n][kList] (the sorted places of the
// first kList entries); by molecule index: nn [n][2], label [n], and the working labels and sizes of the cluster pass where they do
// not live in LDS; op [4].  `mode` 0: the boxes that are not frozen (an evaluation of the call); 1: the boxes a guard froze (their
// final state, at the end of the call).
__device__ __forceinline__ bool box_skipped(const int* I, int mode) { return mode ? !(I[0] && !I[5]) : I[0] != 0; }

// One lane per molecule in sorted order, one walk on the force evaluation's grid: n_i, q_6m(i) and |q_6(i)|, the entry list.
__global__ __launch_bounds__(kThreads) void k_nuc_q6(int n, int cap, double rc2, int mode, const double* __restrict__ par, const int* __restrict__ grid,
                                                     const int* __restrict__ start, const double* __restrict__ ss, const int* __restrict__ si,
                                                     double* __restrict__ rec, int* __restrict__ cnt, int* __restrict__ list)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (box_skipped(si + kSI * (size_t)b, mode) || p >= n) return;
    const size_t o = (size_t)b * n;
    const double* S = ss + 3 * o;
    double acc[kN6];
#pragma unroll
    for (int k = 0; k < kN6; ++k) acc[k] = 0.0;
    int c = 0;
    int* L = list + kList * (o + p);
    walk_cells(S[3 * (size_t)p], S[3 * (size_t)p + 1], S[3 * (size_t)p + 2], rc2, par + 18 * (size_t)b, grid + 4 * (size_t)b,
               start + (size_t)b * (cap + 1), S,
               [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
                   double Y[kNY];
                   unit_harmonics(r2, dx, dy, dz, Y);
#pragma unroll
                   for (int k = 0; k < kN6; ++k) acc[k] = acc[k] + Y[kY6 + k];
                   if (c < kList) L[c] = q;
                   ++c;
               });
    const double m = (double)c;
#pragma unroll
    for (int k = 0; k < kN6; ++k) acc[k] = c ? acc[k] / m : 0.0;
    const double n6 = norm_of(acc, 0, kN6);
    double* r = rec + kRec * (o + p);
#pragma unroll
    for (int k = 0; k < kN6; ++k) r[k] = acc[k];
    r[kN6] = n6;
    cnt[o + p] = c;
}

// The same walk over the neighbours' records: conn_i as k_boo_pass2 of libmw_boo.so forms it, and the solid-like flag.
__global__ __launch_bounds__(kThreads) void k_nuc_conn(int n, int cap, double rc2, double thr, int min_conn, int mode, const double* __restrict__ par,
                                                       const int* __restrict__ grid, const int* __restrict__ start, const double* __restrict__ ss,
                                                       const int* __restrict__ idx, const int* __restrict__ si, const double* __restrict__ rec,
                                                       const int* __restrict__ cnt, int* __restrict__ sol, int* __restrict__ nn)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (box_skipped(si + kSI * (size_t)b, mode) || p >= n) return;
    const size_t o = (size_t)b * n;
    const double* S = ss + 3 * o;
    const double* R = rec + kRec * o;
    double own[kRec];
#pragma unroll
    for (int k = 0; k < kRec; ++k) own[k] = R[kRec * (size_t)p + k];
    int conn = 0;
    walk_cells(S[3 * (size_t)p], S[3 * (size_t)p + 1], S[3 * (size_t)p + 2], rc2, par + 18 * (size_t)b, grid + 4 * (size_t)b,
               start + (size_t)b * (cap + 1), S,
               [&](int j, int, int, int, double, double, double, double) {
                   const double* rj = R + kRec * (size_t)j;
                   double dot = 0.0;
#pragma unroll
                   for (int k = 0; k < kN6; ++k) dot = __builtin_fma(own[k], rj[k], dot);
                   const double den = own[kN6] * rj[kN6];
                   if (den > 0.0 && dot / den > thr) ++conn;
               });
    sol[o + p] = conn >= min_conn ? 1 : 0;
    const size_t i = o + idx[o + p];
    nn[2 * i] = cnt[o + p];
    nn[2 * i + 1] = conn;
}

// Relaxed accesses to the label / size words that other lanes change while this one reads: workgroup scope in LDS, device
// scope in global memory (served by L2), as in the engine's mw_ice_clusters.hip.h.
template <bool LDS>
__device__ __forceinline__ int cl_load(const int* p)
{
    if constexpr (LDS) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void cl_store(int* p, int v)
{
    if constexpr (LDS) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void cl_min(int* p, int v)
{
    if constexpr (LDS) (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void cl_inc(int* p)
{
    if constexpr (LDS) (void)__hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else (void)__hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the root of solid-like x: lab[.] <= . and strictly decreasing along the walk, so it ends
template <bool LDS>
__device__ __forceinline__ int cl_root(const int* lab, int x)
{
    for (;;) {
        const int p = cl_load<LDS>(&lab[x]);
        if (p == x) return x;
        x = p;
    }
}

// One workgroup per box: the clusters of its solid-like molecules by the hook / compress rounds of mw_ice_clusters.hip.h, over
// molecule indices (lab[i] = i for solid-like i, kClusterNone otherwise; lab[x] <= x and only ever decreases).  A round hooks, for
// every solid-like i and every entry j of i that is solid-like and is not i, the larger of the two roots under the smaller by an
// integer atomic minimum, then compresses; rounds repeat until one passes without a hook.  Then every bond joins two molecules of
// one tree and a tree's root is its smallest molecule, whatever order the atomics landed in.  Entries come from the molecule's
// list, or from the walk when it has more than kList of them.  Hooking from i's entries and from j's covers "j is an entry of i
// or i is an entry of j".  Sizes by integer atomics on the roots; the largest size and, among equals, the smallest root by one
// 64-bit integer maximum.  The tail (thread 0) writes op, the three trace columns and the box's row, and applies the stopping rule
// (mode 0) to the box's flags.
template <bool LDS>
__global__ __launch_bounds__(kClusterBlock) void k_nuc_clusters(int n, int cap, double rc2, int mode, int e, int sample_every, int nrows,
                                                                const double* __restrict__ par, const int* __restrict__ grid,
                                                                const int* __restrict__ start, const double* __restrict__ ss,
                                                                const int* __restrict__ idx, int* si, const int* __restrict__ cnt,
                                                                const int* __restrict__ sol, const int* __restrict__ list,
                                                                const int* __restrict__ lam_lo, const int* __restrict__ lam_hi, int* glab, int* gsiz,
                                                                int* __restrict__ label, int* __restrict__ op, double* __restrict__ row,
                                                                double* __restrict__ trace)
{
    extern __shared__ __attribute__((aligned(16))) int clds[];
    __shared__ int s_changed, s_count[2];
    __shared__ unsigned long long s_best;
    static_assert(sizeof(int) * 3 + sizeof(unsigned long long) + 16 <= kClusterStaticLds, "static LDS of k_nuc_clusters");
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    int* I = si + kSI * (size_t)b;
    if (box_skipped(I, mode)) return;                                  // the whole workgroup
    const size_t o = (size_t)b * n;
    const int* IDX = idx + o;
    const int* SOL = sol + o;
    const int* CNT = cnt + o;
    const double* S = ss + 3 * o;
    int* lab;
    int* siz;
    if constexpr (LDS) { lab = clds; siz = clds + n; }
    else { lab = glab + o; siz = gsiz + o; }

    for (int p = tid; p < n; p += nthr) {
        const int i = IDX[p];
        cl_store<LDS>(&lab[i], SOL[p] ? i : kClusterNone);
        cl_store<LDS>(&siz[i], 0);
    }
    if (tid == 0) { s_count[0] = 0; s_count[1] = 0; s_best = 0ull; }
    __syncthreads();

    int nrounds = 0;
    for (;;) {
        if (tid == 0) s_changed = 0;
        __syncthreads();
        bool changed = false;
        for (int p = tid; p < n; p += nthr) {
            if (!SOL[p]) continue;
            const int i = IDX[p];
            auto hook = [&](int q) {
                if (!SOL[q]) return;
                const int j = IDX[q];
                if (j == i) return;                                    // (an image of i itself is no bond)
                const int ri = cl_root<LDS>(lab, i), rj = cl_root<LDS>(lab, j);
                if (ri != rj) { cl_min<LDS>(&lab[max(ri, rj)], min(ri, rj)); changed = true; }
            };
            const int c = CNT[p];
            if (c <= kList) {
                const int* L = list + kList * (o + p);
                for (int u = 0; u < c; ++u) hook(L[u]);
            } else {
                walk_cells(S[3 * (size_t)p], S[3 * (size_t)p + 1], S[3 * (size_t)p + 2], rc2, par + 18 * (size_t)b, grid + 4 * (size_t)b,
                           start + (size_t)b * (cap + 1), S, [&](int q, int, int, int, double, double, double, double) { hook(q); });
            }
        }
        if (changed) __hip_atomic_store(&s_changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        const int any = __hip_atomic_load(&s_changed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // the same word for every lane
        for (int p = tid; p < n; p += nthr)
            if (SOL[p]) { const int i = IDX[p]; cl_store<LDS>(&lab[i], cl_root<LDS>(lab, i)); }
        ++nrounds;
        __syncthreads();
        if (!any) break;
    }

    for (int p = tid; p < n; p += nthr)
        if (SOL[p]) cl_inc<LDS>(&siz[cl_load<LDS>(&lab[IDX[p]])]);
    __syncthreads();
    int nsel = 0, nclu = 0;
    unsigned long long best = 0ull;                                    // (size, kClusterNone - root): the largest size, then the smallest root
    for (int p = tid; p < n; p += nthr) {
        const int i = IDX[p];
        const int r = SOL[p] ? cl_load<LDS>(&lab[i]) : kClusterNone;
        label[o + i] = r == kClusterNone ? 0 : r + 1;
        if (r == kClusterNone) continue;
        ++nsel;
        if (r != i) continue;
        ++nclu;
        const unsigned long long key = ((unsigned long long)(unsigned)cl_load<LDS>(&siz[i]) << 32) | (unsigned)(kClusterNone - i);
        best = key > best ? key : best;
    }
    if (nsel) (void)__hip_atomic_fetch_add(&s_count[0], nsel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (nclu) (void)__hip_atomic_fetch_add(&s_count[1], nclu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (best) (void)__hip_atomic_fetch_max(&s_best, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (tid == 0) {
        const unsigned long long top = s_best;
        const int lam = (int)(top >> 32), lab1 = lam > 0 ? kClusterNone - (int)(unsigned)(top & 0xffffffffull) + 1 : 0;
        int* O = op + 4 * (size_t)b;
        O[0] = s_count[0]; O[1] = s_count[1]; O[2] = lam; O[3] = lab1;
        I[6] += nrounds;
        if (mode == 0) {
            double* R = row + kRow * (size_t)b;
            R[kOp] = (double)lam; R[kOp + 1] = (double)s_count[0]; R[kOp + 2] = (double)s_count[1];
            if (trace && e % sample_every == 0) {
                double* T = trace + ((size_t)b * nrows + e / sample_every) * kOut;
                T[kOp] = R[kOp]; T[kOp + 1] = R[kOp + 1]; T[kOp + 2] = R[kOp + 2];
            }
            if (lam >= lam_hi[b]) { I[0] = 1; I[5] = MW_NUC_REACHED_HI; }
            else if (lam <= lam_lo[b]) { I[0] = 1; I[5] = MW_NUC_REACHED_LO; }
        }
    }
}

// Stage 1 of the next step and its guard, one lane per molecule of a box that goes on after a check: what k_nuc_forces does with
// `do1`, from the stored v and F (the same doubles).
__global__ __launch_bounds__(kThreads) void k_nuc_kick1(int n, Consts C, const double* __restrict__ F, double* __restrict__ v, int* si)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    int* I = si + kSI * (size_t)b;
    if (I[0] || i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    double vx = v[m], vy = v[m + 1], vz = v[m + 2];
    kick(C.hk, F[m], F[m + 1], F[m + 2], vx, vy, vz);
    if (guard_fails(C.hd, C.lim2, vx, vy, vz)) atomicOr(I + 1, 1);
    v[m] = vx; v[m + 1] = vy; v[m + 2] = vz;
}

// One lane per box after k_nuc_kick1: a tripped first guard freezes the box, as k_nuc_row does after k_nuc_forces.
__global__ __launch_bounds__(64) void k_nuc_latch(int nb, int* __restrict__ si)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;
    int* I = si + kSI * (size_t)b;
    if (I[1]) I[0] = 1;
}

}  // namespace mwnuc

namespace {

using namespace mwnuc;

constexpr int kPool = 512;                         // event timers between two harvests
constexpr int kPoolSlack = 32;
enum { kSort = 0, kMoments = 1, kForces = 2, kDrift = 3, kBaro = 4, kOrder = 5, kClusters = 6, kTimers = 7 };
constexpr int kClusterLdsBudget = kLdsBytes - kClusterStaticLds;

struct State : Runtime<1> {
    Buf scratch, cells, pos, vel, ref, streams, lo, hi, pos_out, vel_out, forces, cells_out, ref_out, trace, status, nn, label, op, bad;
    std::vector<hipEvent_t> pool;
    std::vector<int> bucket;                       // what the interval that begins at event k is, or -1
    int used = 0;
    int labels_lds = 1;                            // MW_NUC_LABELS_LDS
    bool lds_raised = false;
    int last[MW_NUC_PLAN_FIELDS] = {0};
    float ms[kTimers] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
} g;

// The scratch of one box: the sort's pieces, what the force passes keep, what the order parameter keeps, then the state.
struct Layout : SortLayout {
    int nwg = 0;
    size_t mom = 0, en = 0, part = 0, rec = 0, cnt = 0, sol = 0, list = 0, nn = 0, label = 0, glab = 0, gsiz = 0, op = 0;
    size_t x = 0, v = 0, F = 0, ref = 0, row = 0, si = 0, cell = 0, par = 0, grid = 0, cv = 0, per_box = 0;
};

Layout make_layout(int n)
{
    Layout l;
    size_t o = 0;
    lay_sort(l, n, o);
    l.nwg = (n + kThreads - 1) / kThreads;
    l.mom = o;   o += align16(8 * (size_t)kMom * n);
    l.en = o;    o += align16(8 * (size_t)n);
    l.part = o;  o += align16(8 * (size_t)kPart * l.nwg);
    l.rec = o;   o += align16(8 * (size_t)kRec * n);
    l.cnt = o;   o += align16(4 * (size_t)n);
    l.sol = o;   o += align16(4 * (size_t)n);
    l.list = o;  o += align16(4 * (size_t)kList * n);
    l.nn = o;    o += align16(8 * (size_t)n);
    l.label = o; o += align16(4 * (size_t)n);
    l.glab = o;  o += align16(4 * (size_t)n);
    l.gsiz = o;  o += align16(4 * (size_t)n);
    l.op = o;    o += align16(4 * 4);
    l.x = o;     o += align16(24 * (size_t)n);
    l.v = o;     o += align16(24 * (size_t)n);
    l.F = o;     o += align16(24 * (size_t)n);
    l.ref = o;   o += align16(24 * (size_t)n);
    l.row = o;   o += align16(8 * (size_t)kRow);
    l.si = o;    o += align16(4 * (size_t)kSI);
    l.cell = o;  o += align16(8 * 9);
    l.par = o;   o += align16(8 * 18);
    l.grid = o;  o += align16(4 * 4);
    l.cv = o;    o += align16(8 * (size_t)kCV);
    l.per_box = o;
    return l;
}

size_t cluster_lds_bytes(int n) { return ((size_t)n * 2 * sizeof(int) + 15) & ~(size_t)15; }
bool cluster_lds_fits(int n) { return cluster_lds_bytes(n) <= (size_t)kClusterLdsBudget; }
int cluster_threads(int n) { return n >= kClusterBlock ? kClusterBlock : (n + 63) & ~63; }

struct Plan : PlanBase {
    Layout lay;
    int labels_lds;
};

int make_plan(const char* who, int n, int nboxes, size_t budget, int labels_lds, Plan& p)
{
    p.small = 0;
    p.lay = make_layout(n);
    p.per_box = p.lay.per_box;
    p.labels_lds = labels_lds && cluster_lds_fits(n) ? 1 : 0;
    p.lds = (p.labels_lds ? (int)cluster_lds_bytes(n) : 0) + kClusterStaticLds;
    p.boxes_per_wg = 0;
    const size_t fit = budget / p.per_box;
    if (fit < 1)
        return fail("%s: one box needs %zu bytes of scratch (nwater = %d) and does not fit the budget of %zu bytes (MW_NUC_SCRATCH_MB)",
                    who, p.per_box, n, budget);
    p.bpc = (int)(fit < (size_t)kMaxChunkBoxes ? fit : (size_t)kMaxChunkBoxes);
    if (p.bpc > nboxes) p.bpc = nboxes;
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

void nuc_fields(const Plan& p, const int* grid, int rounds, int* f)
{
    plan_fields(p, grid, f);
    f[9] = 1;
    f[10] = p.labels_lds;
    f[11] = rounds;
}

int check_counts(const char* who, int nboxes, int n)
{
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    if (n < MW_NUC_MIN_WATER)
        return fail("%s: nwater = %d is below %d: the one-wavefront-per-box geometry (nwater <= 64) is out of scope of this library (box 0)", who, n,
                    MW_NUC_MIN_WATER);
    return 0;
}

struct Scalars {
    unsigned long long seed;
    int nsteps, sample_every;
    double dt, mass, kT, gamma, pressure, tau_p, beta_T;
    int baro_every, coupling, axis;
};

// what the order parameter adds to a call
struct Order {
    double rc, threshold;
    int min_conn, check_every;
};

int check_scalars(const char* who, int nboxes, int n, const Scalars& s, Consts& C)
{
    if (check_counts(who, nboxes, n)) return 1;
    if (s.nsteps < 0 || s.nsteps > MW_NUC_MAX_STEPS) return fail("%s: nsteps = %d outside 0..%d", who, s.nsteps, MW_NUC_MAX_STEPS);
    if (s.sample_every < 1) return fail("%s: sample_every = %d is not at least 1", who, s.sample_every);
    if (!(s.dt > 0.0) || !std::isfinite(s.dt)) return fail("%s: dt = %g atomic time units is not a finite number > 0", who, s.dt);
    if (!(s.mass > 0.0) || !std::isfinite(s.mass)) return fail("%s: mass = %g electron masses is not a finite number > 0", who, s.mass);
    if (!(s.kT >= 0.0) || !std::isfinite(s.kT)) return fail("%s: kT = %g Hartree is not a finite number >= 0", who, s.kT);
    if (!(s.gamma >= 0.0) || !std::isfinite(s.gamma)) return fail("%s: gamma = %g per atomic time unit is not a finite number >= 0", who, s.gamma);
    if (!std::isfinite(s.pressure)) return fail("%s: pressure = %g Hartree / bohr^3 is not a finite number", who, s.pressure);
    if (!(s.tau_p > 0.0) || !std::isfinite(s.tau_p)) return fail("%s: tau_p = %g atomic time units is not a finite number > 0", who, s.tau_p);
    if (!(s.beta_T > 0.0) || !std::isfinite(s.beta_T)) return fail("%s: beta_T = %g bohr^3 / Hartree is not a finite number > 0", who, s.beta_T);
    if (s.baro_every < 0) return fail("%s: baro_every = %d is negative", who, s.baro_every);
    if (s.coupling < MW_FLEX_ISO || s.coupling > MW_FLEX_UNIAXIAL) return fail("%s: coupling = %d outside 0..3", who, s.coupling);
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
    if (!std::isfinite(C.hk) || !(C.hk > 0.0)) return fail("%s: dt / (2 mass) = %g with dt = %g and mass = %g is not a finite number > 0", who, C.hk, s.dt, s.mass);
    if (!std::isfinite(C.c2)) return fail("%s: kT = %g over mass = %g is not finite", who, s.kT, s.mass);
    if (!std::isfinite(C.cb) || !std::isfinite(C.cn))
        return fail("%s: beta_T = %g times baro_every dt = %g over tau_p = %g is not finite", who, s.beta_T, dtb, s.tau_p);
    return 0;
}

int check_order(const char* who, int nsteps, const Order& q)
{
    if (!(q.rc > 0.0) || !std::isfinite(q.rc)) return fail("%s: rc = %g bohr is not a finite cutoff > 0 (box 0)", who, q.rc);
    if (!(q.rc * kGuard <= mw::kSigA))
        return fail("%s: rc = %.17g bohr is beyond a sigma = %.17g bohr, the mW cutoff (rc (1 + 1e-9) <= a sigma is required: the cell grid of the "
                    "force evaluation serves the order parameter) (box 0)", who, q.rc, mw::kSigA);
    if (!(q.threshold >= -1.0 && q.threshold <= 1.0)) return fail("%s: threshold = %g outside [-1, 1] (box 0)", who, q.threshold);
    if (q.min_conn < 1 || q.min_conn > MW_NUC_MAX_CONN) return fail("%s: min_conn = %d outside 1..%d (box 0)", who, q.min_conn, MW_NUC_MAX_CONN);
    if (q.check_every < 1) return fail("%s: check_every = %d is not at least 1 (box 0)", who, q.check_every);
    if (nsteps % q.check_every != 0)
        return fail("%s: check_every = %d does not divide nsteps = %d (box 0)", who, q.check_every, nsteps);
    return 0;
}

// -1 <= lam_lo[b] < lam_hi[b] for every box (host arrays)
int check_bounds(const char* who, int nboxes, const int* lo, const int* hi)
{
    for (int b = 0; b < nboxes; ++b) {
        if (lo[b] < -1) return fail("%s: lam_lo = %d of box %d is below -1", who, lo[b], b);
        if (!(lo[b] < hi[b])) return fail("%s: lam_lo = %d is not below lam_hi = %d in box %d", who, lo[b], hi[b], b);
    }
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

const char kRadius[] = "a_sigma";             // the radius the cells are checked against, in the messages

int check_live(const char* who) { return check_live(who, "mw_nuc_init", g); }

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
    const unsigned long long* streams;
    const int *lo, *hi;
    double *pos_out, *vel_out, *forces, *cells_out, *ref_out, *trace;
    int *status, *nn, *label, *op;
};

// the pointers of a chunk's scratch
struct Chunk {
    int n, nb, b0;
    dim3 grid_m;
    const Layout* l;
    char* base;
    size_t B;
    double *x, *v, *F, *ref, *row, *cell, *par, *cv, *mom, *en, *part, *trace, *rec;
    int *si, *grid, *cnt, *sol, *list, *nn, *label, *glab, *gsiz, *op;
    const unsigned long long* streams;
    const int *lo, *hi;
    Sorted sorted;                                 // of the last evaluation
};

// sort, moments, forces and row for the evaluation that ends step e
int evaluate_general(Chunk& k, const Consts& C, int e, int do6, int do1)
{
    Sorted& s = k.sorted;
    if (mark(kSort)) return 1;
    if (sort_into_cells(g.stream, k.n, k.nb, *k.l, k.base, k.B, k.par, k.grid, (const double*)k.x, s)) return 1;
    if (mark(kMoments)) return 1;
    hipLaunchKernelGGL(k_nuc_moments, k.grid_m, dim3(kThreads), 0, g.stream, k.n, k.l->cap, (const double*)k.par, (const int*)k.grid, s.start, s.ss,
                       (const int*)k.si, k.mom, k.en);
    HIPOK(hipGetLastError());
    if (mark(kForces)) return 1;
    hipLaunchKernelGGL(k_nuc_forces, k.grid_m, dim3(kThreads), 0, g.stream, k.n, k.l->cap, C, do6, do1, (const double*)k.par, (const int*)k.grid, s.start,
                       s.ss, s.idx, k.si, (const double*)k.mom, (const double*)k.en, (const double*)k.ref, (const double*)k.x, k.v, k.F, k.part);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_nuc_row, dim3((unsigned)k.nb), dim3(64), 0, g.stream, k.l->nwg, k.n, e, C, (const double*)k.part, (const double*)k.cv, k.row, k.si,
                       k.trace);
    HIPOK(hipGetLastError());
    return mark(-1);
}

// the barostat stage after stage 6 of the step with index `step`
int barostat(const Chunk& k, const Consts& C, unsigned long long step)
{
    if (mark(kBaro)) return 1;
    hipLaunchKernelGGL(k_nuc_baro, dim3((unsigned)((k.nb + 63) / 64)), dim3(64), 0, g.stream, k.nb, k.l->cap, C, k.streams, k.b0, step,
                       (const double*)k.row, k.si, k.cell, k.par, k.grid, k.cv);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_nuc_scale, k.grid_m, dim3(kThreads), 0, g.stream, k.n, C, (const int*)k.si, (const double*)k.cv, k.x, k.v, k.ref);
    HIPOK(hipGetLastError());
    return mark(-1);
}

// The order parameter and the clusters of the state whose force evaluation has just run (its sort is k.sorted), after step e.
// mode 0: the boxes that run, with the stopping rule; mode 1: the boxes a guard froze, their outputs alone.
int order_parameter(const Chunk& k, const Consts& C, const Order& q, bool lds, int mode, int e)
{
    const Sorted& s = k.sorted;
    const double rc2 = q.rc * q.rc;
    if (mark(mode ? -1 : kOrder)) return 1;                            // (the pass over the boxes a guard froze is not timed)
    hipLaunchKernelGGL(k_nuc_q6, k.grid_m, dim3(kThreads), 0, g.stream, k.n, k.l->cap, rc2, mode, (const double*)k.par, (const int*)k.grid, s.start, s.ss,
                       (const int*)k.si, k.rec, k.cnt, k.list);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_nuc_conn, k.grid_m, dim3(kThreads), 0, g.stream, k.n, k.l->cap, rc2, q.threshold, q.min_conn, mode, (const double*)k.par,
                       (const int*)k.grid, s.start, s.ss, s.idx, (const int*)k.si, (const double*)k.rec, (const int*)k.cnt, k.sol, k.nn);
    HIPOK(hipGetLastError());
    if (mark(mode ? -1 : kClusters)) return 1;
    const dim3 blocks((unsigned)k.nb), threads((unsigned)cluster_threads(k.n));
    if (lds)
        hipLaunchKernelGGL(k_nuc_clusters<true>, blocks, threads, cluster_lds_bytes(k.n), g.stream, k.n, k.l->cap, rc2, mode, e, C.sample_every, C.nrows,
                           (const double*)k.par, (const int*)k.grid, s.start, s.ss, s.idx, k.si, (const int*)k.cnt, (const int*)k.sol, (const int*)k.list,
                           k.lo, k.hi, k.glab, k.gsiz, k.label, k.op, k.row, k.trace);
    else
        hipLaunchKernelGGL(k_nuc_clusters<false>, blocks, threads, 0, g.stream, k.n, k.l->cap, rc2, mode, e, C.sample_every, C.nrows,
                           (const double*)k.par, (const int*)k.grid, s.start, s.ss, s.idx, k.si, (const int*)k.cnt, (const int*)k.sol, (const int*)k.list,
                           k.lo, k.hi, k.glab, k.gsiz, k.label, k.op, k.row, k.trace);
    HIPOK(hipGetLastError());
    return mark(-1);
}

// stage 1 of the step after a check, for the boxes that go on
int deferred_kick(const Chunk& k, const Consts& C)
{
    if (mark(kDrift)) return 1;
    hipLaunchKernelGGL(k_nuc_kick1, k.grid_m, dim3(kThreads), 0, g.stream, k.n, C, (const double*)k.F, k.v, k.si);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_nuc_latch, dim3((unsigned)((k.nb + 63) / 64)), dim3(64), 0, g.stream, k.nb, k.si);
    HIPOK(hipGetLastError());
    return mark(-1);
}

// The work of both entries, arguments already checked.  `grid0` is the grid of the first box's input cell (the plan fields); the
// arrays of `a` are device pointers when `dev`, host pointers otherwise.
int run(const char* who, int nboxes, int n, const int* grid0, const Consts& C, const Order& q, unsigned long long step0, int baro_every, bool dev,
        const Arrays& a)
{
    Plan p;
    if (make_plan(who, n, nboxes, g.budget, g.labels_lds, p)) return 1;
    const Layout& l = p.lay;
    const bool lds = p.labels_lds != 0;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (lds && !g.lds_raised) {
        HIPOK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nuc_clusters<true>), hipFuncAttributeMaxDynamicSharedMemorySize, kClusterLdsBudget));
        g.lds_raised = true;
    }
    if (reserve(g.scratch, p.per_box * (size_t)p.bpc)) return 1;
    const size_t vec = 24 * (size_t)n, rowbytes = 8 * (size_t)kOut * C.nrows;
    if (!dev) {
        if (reserve(g.cells, 72 * (size_t)p.bpc)) return 1;
        if (reserve(g.pos, vec * p.bpc)) return 1;
        if (a.vel && reserve(g.vel, vec * p.bpc)) return 1;
        if (a.ref && reserve(g.ref, vec * p.bpc)) return 1;
        if (a.streams && reserve(g.streams, 8 * (size_t)p.bpc)) return 1;
        if (reserve(g.lo, 4 * (size_t)p.bpc)) return 1;
        if (reserve(g.hi, 4 * (size_t)p.bpc)) return 1;
        if (a.pos_out && reserve(g.pos_out, vec * p.bpc)) return 1;
        if (a.vel_out && reserve(g.vel_out, vec * p.bpc)) return 1;
        if (a.forces && reserve(g.forces, vec * p.bpc)) return 1;
        if (a.cells_out && reserve(g.cells_out, 72 * (size_t)p.bpc)) return 1;
        if (a.ref_out && reserve(g.ref_out, vec * p.bpc)) return 1;
        if (a.trace && reserve(g.trace, rowbytes * p.bpc)) return 1;
        if (a.status && reserve(g.status, 8 * (size_t)p.bpc)) return 1;
        if (a.nn && reserve(g.nn, 8 * (size_t)n * p.bpc)) return 1;
        if (a.label && reserve(g.label, 4 * (size_t)n * p.bpc)) return 1;
        if (a.op && reserve(g.op, 16 * (size_t)p.bpc)) return 1;
    }
    float ms[kTimers] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const int evals = C.nsteps + 1;
    const unsigned long long be = (unsigned long long)baro_every;
    // evaluation e >= 1 ends the step with index t = step0 + e - 1; the barostat follows it when (t + 1) % baro_every == 0
    auto baro_at = [&](int e) { return be > 0 && e > 0 && (step0 + (unsigned long long)e) % be == 0; };
    int rounds = 0;
    g.used = 0;
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const size_t first = 3 * (size_t)n * b0;
        const double* d_cells = a.cells + 9 * (size_t)b0;
        const double* d_pos = a.pos + first;
        const double* d_vel = a.vel ? a.vel + first : nullptr;
        const double* d_ref = a.ref ? a.ref + first : nullptr;
        const unsigned long long* d_streams = a.streams ? a.streams + b0 : nullptr;
        const int* d_lo = a.lo + b0;
        const int* d_hi = a.hi + b0;
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
            HIPOK(hipMemcpyAsync(g.lo.p, d_lo, 4 * (size_t)nb, hipMemcpyHostToDevice, g.stream));
            d_lo = (const int*)g.lo.p;
            HIPOK(hipMemcpyAsync(g.hi.p, d_hi, 4 * (size_t)nb, hipMemcpyHostToDevice, g.stream));
            d_hi = (const int*)g.hi.p;
        }
        double* d_out = !a.pos_out ? nullptr : dev ? a.pos_out + first : (double*)g.pos_out.p;
        double* d_vout = !a.vel_out ? nullptr : dev ? a.vel_out + first : (double*)g.vel_out.p;
        double* d_forces = !a.forces ? nullptr : dev ? a.forces + first : (double*)g.forces.p;
        double* d_cout = !a.cells_out ? nullptr : dev ? a.cells_out + 9 * (size_t)b0 : (double*)g.cells_out.p;
        double* d_rout = !a.ref_out ? nullptr : dev ? a.ref_out + first : (double*)g.ref_out.p;
        double* d_trace = !a.trace ? nullptr : dev ? a.trace + (size_t)kOut * C.nrows * b0 : (double*)g.trace.p;
        int* d_status = !a.status ? nullptr : dev ? a.status + 2 * (size_t)b0 : (int*)g.status.p;
        int* d_nn = !a.nn ? nullptr : dev ? a.nn + 2 * (size_t)n * b0 : (int*)g.nn.p;
        int* d_label = !a.label ? nullptr : dev ? a.label + (size_t)n * b0 : (int*)g.label.p;
        int* d_op = !a.op ? nullptr : dev ? a.op + 4 * (size_t)b0 : (int*)g.op.p;
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
        k.rec = (double*)(k.base + l.rec * k.B);
        k.cnt = (int*)(k.base + l.cnt * k.B);
        k.sol = (int*)(k.base + l.sol * k.B);
        k.list = (int*)(k.base + l.list * k.B);
        k.nn = (int*)(k.base + l.nn * k.B);
        k.label = (int*)(k.base + l.label * k.B);
        k.glab = (int*)(k.base + l.glab * k.B);
        k.gsiz = (int*)(k.base + l.gsiz * k.B);
        k.op = (int*)(k.base + l.op * k.B);
        k.trace = d_trace;
        k.streams = d_streams;
        k.lo = d_lo; k.hi = d_hi;
        // (a box whose cell the device refuses is never evaluated by mode 0; its nn, label and op come from mode 1)
        hipLaunchKernelGGL(k_nuc_begin, k.grid_m, dim3(kThreads), 0, g.stream, n, l.cap, d_cells, d_pos, d_vel, d_ref, k.x, k.v, k.F, k.ref, k.row, k.si,
                           k.cell, k.par, k.grid, k.cv);
        HIPOK(hipGetLastError());
        for (int e = 0; e < evals; ++e) {
            const bool baro = baro_at(e), check = e % q.check_every == 0;
            const int next = e < C.nsteps ? 1 : 0;               // a step follows: its stage 1 belongs to this evaluation, or to the check
            if (e > 0) {
                if (mark(kDrift)) return 1;
                hipLaunchKernelGGL(k_nuc_drift1, k.grid_m, dim3(kThreads), 0, g.stream, n, C, d_streams, b0, step0 + (unsigned long long)(e - 1), k.x, k.v,
                                   k.si);
                HIPOK(hipGetLastError());
                hipLaunchKernelGGL(k_nuc_drift2, k.grid_m, dim3(kThreads), 0, g.stream, n, C.hd, k.x, (const double*)k.v, (const int*)k.si);
                HIPOK(hipGetLastError());
            }
            if (evaluate_general(k, C, e, e > 0 ? 1 : 0, next && !baro && !check ? 1 : 0)) return 1;
            if (baro) {
                if (barostat(k, C, step0 + (unsigned long long)(e - 1))) return 1;
                if (evaluate_general(k, C, e, 0, next && !check ? 1 : 0)) return 1;
            }
            if (check) {
                if (order_parameter(k, C, q, lds, 0, e)) return 1;
                if (next && deferred_kick(k, C)) return 1;
            }
            if (harvest_if_full(ms)) return 1;
        }
        if (order_parameter(k, C, q, lds, 1, C.nsteps)) return 1;
        if (harvest(ms)) return 1;
        hipLaunchKernelGGL(k_nuc_finish, k.grid_m, dim3(kThreads), 0, g.stream, n, (const double*)k.x, (const double*)k.v, (const double*)k.F,
                           (const double*)k.ref, (const int*)k.si, (const double*)k.cell, d_out, d_vout, d_forces, d_rout, d_cout, d_status,
                           (const int*)k.nn, (const int*)k.label, (const int*)k.op, d_nn, d_label, d_op);
        HIPOK(hipGetLastError());
        if (!dev) {
            if (a.pos_out) HIPOK(hipMemcpyAsync(a.pos_out + first, g.pos_out.p, vec * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.vel_out) HIPOK(hipMemcpyAsync(a.vel_out + first, g.vel_out.p, vec * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.forces) HIPOK(hipMemcpyAsync(a.forces + first, g.forces.p, vec * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.cells_out) HIPOK(hipMemcpyAsync(a.cells_out + 9 * (size_t)b0, g.cells_out.p, 72 * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
            if (a.ref_out) HIPOK(hipMemcpyAsync(a.ref_out + first, g.ref_out.p, vec * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.trace) HIPOK(hipMemcpyAsync(a.trace + (size_t)kOut * C.nrows * b0, g.trace.p, rowbytes * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.status) HIPOK(hipMemcpyAsync(a.status + 2 * (size_t)b0, g.status.p, 8 * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
            if (a.nn) HIPOK(hipMemcpyAsync(a.nn + 2 * (size_t)n * b0, g.nn.p, 8 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.label) HIPOK(hipMemcpyAsync(a.label + (size_t)n * b0, g.label.p, 4 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.op) HIPOK(hipMemcpyAsync(a.op + 4 * (size_t)b0, g.op.p, 16 * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
        }
        if (c == 0) HIPOK(hipMemcpyAsync(&rounds, k.si + 6, sizeof(int), hipMemcpyDeviceToHost, g.stream));   // the call's first box (a diagnostic)
        HIPOK(hipStreamSynchronize(g.stream));               // the next chunk reuses the scratch and the staging buffers
    }
    nuc_fields(p, grid0, rounds, g.last);
    g.have_last = true;
    for (int t = 0; t < kTimers; ++t) g.ms[t] = ms[t];
    return 0;
}

}  // namespace

extern "C" {

const char* mw_nuc_last_error(void) { return g_err; }
int mw_nuc_is_initialised(void) { return g.live ? 1 : 0; }

int mw_nuc_init(int device)
{
    const char* who = "mw_nuc_init";
    if (g.live) return fail("%s: already initialised", who);
    int labels_lds = 1;
    if (env_int(who, "MW_NUC_LABELS_LDS", 0, 1, labels_lds)) return 1;
    if (runtime_init(who, "MW_NUC_SCRATCH_MB", device, g)) return 1;
    g.labels_lds = labels_lds;
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

int mw_nuc_finalize(void)
{
    if (g.live) {
        DeviceScope scope;
        HIPOK(scope.enter(g.device));
        HIPOK(hipStreamSynchronize(g.stream));
        for (auto& ev : g.pool) HIPOK(hipEventDestroy(ev));
        g.pool.clear();
    }
    if (runtime_finalize(g, {&g.scratch, &g.cells, &g.pos, &g.vel, &g.ref, &g.streams, &g.lo, &g.hi, &g.pos_out, &g.vel_out, &g.forces, &g.cells_out,
                             &g.ref_out, &g.trace, &g.status, &g.nn, &g.label, &g.op, &g.bad}))
        return 1;
    g = State{};
    return 0;
}

int mw_nuc_run(int nboxes, int nwater, const double* cells, const double* pos, const double* vel, const double* pos_ref,
               const unsigned long long* streams, unsigned long long seed, unsigned long long step0, int nsteps, int sample_every, double dt,
               double mass, double kT, double gamma, double pressure, double tau_p, double beta_T, int baro_every, int coupling, int axis, double rc,
               double threshold, int min_conn, int check_every, const int* lam_lo, const int* lam_hi, double* pos_out, double* vel_out, double* forces,
               double* cells_out, double* ref_out, double* trace, int* status, int* nn, int* label, int* op)
{
    const char* who = "mw_nuc_run";
    std::vector<double> par;
    std::vector<int> grid;
    Consts C;
    const Order q{rc, threshold, min_conn, check_every};
    if (check_scalars(who, nboxes, nwater, Scalars{seed, nsteps, sample_every, dt, mass, kT, gamma, pressure, tau_p, beta_T, baro_every, coupling, axis}, C))
        return 1;
    if (check_order(who, nsteps, q)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (!lam_lo) return fail("%s: lam_lo is NULL", who);
    if (!lam_hi) return fail("%s: lam_hi is NULL", who);
    if (check_bounds(who, nboxes, lam_lo, lam_hi)) return 1;
    if (check_cells(who, kRadius, nboxes, nwater, cells, mw::kSigA, par, grid)) return 1;
    if (report_bad(who, first_bad_box(pos, nboxes, nwater), first_bad_box(vel, nboxes, nwater), first_bad_box(pos_ref, nboxes, nwater))) return 1;
    if (check_live(who)) return 1;
    return run(who, nboxes, nwater, grid.data(), C, q, step0, baro_every, false,
               Arrays{cells, pos, vel, pos_ref, streams, lam_lo, lam_hi, pos_out, vel_out, forces, cells_out, ref_out, trace, status, nn, label, op});
}

int mw_nuc_run_device(int nboxes, int nwater, const double* cells, const double* pos, const double* vel, const double* pos_ref,
                      const unsigned long long* streams, unsigned long long seed, unsigned long long step0, int nsteps, int sample_every, double dt,
                      double mass, double kT, double gamma, double pressure, double tau_p, double beta_T, int baro_every, int coupling, int axis,
                      double rc, double threshold, int min_conn, int check_every, const int* lam_lo, const int* lam_hi, double* pos_out,
                      double* vel_out, double* forces, double* cells_out, double* ref_out, double* trace, int* status, int* nn, int* label, int* op)
{
    const char* who = "mw_nuc_run_device";
    std::vector<double> par;
    std::vector<int> grid;
    Consts C;
    const Order q{rc, threshold, min_conn, check_every};
    if (check_scalars(who, nboxes, nwater, Scalars{seed, nsteps, sample_every, dt, mass, kT, gamma, pressure, tau_p, beta_T, baro_every, coupling, axis}, C))
        return 1;
    if (check_order(who, nsteps, q)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (!lam_lo) return fail("%s: lam_lo is NULL", who);
    if (!lam_hi) return fail("%s: lam_hi is NULL", who);
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (fetch_cells(who, kRadius, nboxes, nwater, cells, mw::kSigA, par, grid)) return 1;
    {
        std::vector<int> lo((size_t)nboxes), hi((size_t)nboxes);       // (fetch_cells has waited for whoever made the inputs)
        HIPOK(hipMemcpy(lo.data(), lam_lo, 4 * (size_t)nboxes, hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(hi.data(), lam_hi, 4 * (size_t)nboxes, hipMemcpyDeviceToHost));
        if (check_bounds(who, nboxes, lo.data(), hi.data())) return 1;
    }
    // the verdict on the positions and velocities: one kernel that writes three ints, read before anything else is launched
    if (reserve(g.bad, 3 * sizeof(int))) return 1;
    int bad[3] = {nboxes, nboxes, nboxes};
    HIPOK(hipMemcpyAsync(g.bad.p, bad, sizeof bad, hipMemcpyHostToDevice, g.stream));
    const size_t total = (size_t)nboxes * nwater, blocks = (total + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_nuc_check, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kThreads), 0, g.stream, total, nwater, pos, vel, pos_ref,
                       (int*)g.bad.p);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(bad, g.bad.p, sizeof bad, hipMemcpyDeviceToHost, g.stream));
    HIPOK(hipStreamSynchronize(g.stream));
    if (report_bad(who, bad[0] < nboxes ? bad[0] : -1, bad[1] < nboxes ? bad[1] : -1, bad[2] < nboxes ? bad[2] : -1)) return 1;
    return run(who, nboxes, nwater, grid.data(), C, q, step0, baro_every, true,
               Arrays{cells, pos, vel, pos_ref, streams, lam_lo, lam_hi, pos_out, vel_out, forces, cells_out, ref_out, trace, status, nn, label, op});
}

int mw_nuc_plan(int nwater, const double* cell, int nboxes, int* out, int nout)
{
    const char* who = "mw_nuc_plan";
    std::vector<int> grid;
    if (check_counts(who, nboxes, nwater)) return 1;
    if (plan_grid(who, kRadius, nwater, cell, mw::kSigA, out, nout, grid)) return 1;
    Plan p;
    if (make_plan(who, nwater, nboxes, g.live ? g.budget : kDefaultBudget, g.live ? g.labels_lds : 1, p)) return 1;
    int f[MW_NUC_PLAN_FIELDS];
    nuc_fields(p, grid.data(), 0, f);
    copy_fields(f, MW_NUC_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_nuc_last(int* out, int nout) { return last_fields("mw_nuc_last", "mw_nuc_init", g, g.last, MW_NUC_PLAN_FIELDS, out, nout); }

int mw_nuc_elapsed_ms(float* sort, float* moments, float* forces, float* drift, float* barostat, float* order, float* clusters)
{
    if (check_live("mw_nuc_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_nuc_elapsed_ms: no call has launched yet");
    if (sort) *sort = g.ms[kSort];
    if (moments) *moments = g.ms[kMoments];
    if (forces) *forces = g.ms[kForces];
    if (drift) *drift = g.ms[kDrift];
    if (barostat) *barostat = g.ms[kBaro];
    if (order) *order = g.ms[kOrder];
    if (clusters) *clusters = g.ms[kClusters];
    return 0;
}

}  // extern "C"
