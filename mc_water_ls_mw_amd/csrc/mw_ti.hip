// libmw_ti.so -- the Einstein-crystal thermodynamic integration of include/mw_ti.h: the BAOAB step of include/mw_md.h on the
// mixed energy (1 - lambda) E_mW + lambda 1/2 k sum |x - s|^2, a lambda, a spring and sites per box, and the block averages of
// the five trace fields taken on the device at every step.  The step, the noise and the guard are restated from mw_md.hip (that
// file belongs to libmw_md.so's code object and keeps its bytes); what is new here is the mixing of the force (mix_force), the
// three sums of the displacements (field 4) and the block accumulators (block_of, and the additions of k_ti_row and k_ti_small).  General geometry (nwater > 64), per step:
// k_ti_drift1, k_ti_drift2, the counting sort of mw_lib_cells.h, k_ti_moments, k_ti_forces (the two walks of mw_lib_forces.h; the
// force pass gathers the site of its molecule, forms F_tot, kicks the velocities at the end of this step and at the start of the
// next and tests the first guard) and k_ti_row (one workgroup per box adds the partial sums in order, counts the step, takes the
// freeze flags over, writes the trace row and adds the row to the block accumulators).  Small geometry (nwater <= 64):
// k_ti_small, one wavefront per box, many steps per launch.  k_ti_begin copies the state in, k_ti_finish writes the results.
// Every sum has a fixed order, there is no floating-point atomic and the host only enqueues.  Freeze flags of a box as in
// mw_md.hip: [0] frozen, written by k_ti_row alone; [1] the first guard failed (k_ti_forces), [2] the second (k_ti_drift1).
#include "../../include/mw_ti.h"

#include "mw_common.hip.h"

#include <cstdint>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too
#include "mw_lib_cells.h"
#include "mw_lib_forces.h"

namespace mwti {

using namespace mwcells;
using namespace mwforces;

constexpr int kSmallBoxesPerWg = kThreads / 64;   // one wavefront per box
constexpr int kSmallLdsPerBox = (3 + kMom) * 64 * 8;
constexpr int kSmallLds = kSmallBoxesPerWg * kSmallLdsPerBox;
constexpr int kPart = 7;                          // a workgroup's partial sums: E, v.v, |u|^2, u_x, u_y, u_z and the largest |F_tot| component
constexpr int kRow = MW_TI_TRACE_FIELDS;          // doubles of a box's current trace row, and of its block accumulators
constexpr int kSI = 4;                            // ints: frozen, first guard failed, second guard failed, steps completed
constexpr int kGeneralLds = (kThreads / 64) * kPart * 8;
constexpr double kTwoPi = 6.283185307179586476925286766559;

// The constants of a call, formed on the host (mw_md.h, mw_ti.h), and what names its noise.
struct Consts {
    double hk, hd, c1, c2, lim2, hm;
    uint32_t seed_lo, seed_hi;
    int thermostat, nsteps, sample_every, nrows, equil, block_steps, nblocks;
};

// How a box mixes its force, decided once on the host: kMd (lambda = 0), kMixed, kEinstein (lambda = 1).
enum : int { kMd = 0, kMixed = 1, kEinstein = 2 };
constexpr int kMix = 3;                           // doubles of a box's mixing: oml, nlk and the mode (0.0, 1.0 or 2.0)

// ---- the noise (restated from mw_md.hip) ---------------------------------------------------------------------------------------
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

// ---- the pieces of a step, one molecule (restated from mw_md.hip) ---------------------------------------------------------------
__device__ __forceinline__ void kick(double hk, double fx, double fy, double fz, double& vx, double& vy, double& vz)
{
    vx = __builtin_fma(hk, fx, vx); vy = __builtin_fma(hk, fy, vy); vz = __builtin_fma(hk, fz, vz);
}
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

// ---- what is this library's own ---------------------------------------------------------------------------------------------------
// F_mW -> F_tot of one molecule with the displacement u; `mode` is uniform over the box.
__device__ __forceinline__ void mix_force(int mode, double oml, double nlk, double u0, double u1, double u2, double& fx, double& fy, double& fz)
{
    if (mode == kMd) return;
    if (mode == kEinstein) {
        fx = nlk * u0; fy = nlk * u1; fz = nlk * u2;
    } else {
        fx = __builtin_fma(nlk, u0, oml * fx); fy = __builtin_fma(nlk, u1, oml * fy); fz = __builtin_fma(nlk, u2, oml * fz);
    }
}
// field 4 of a row from the three sums of the displacements
__device__ __forceinline__ double com_square(double sx, double sy, double sz, int n)
{
    const double cx = sx / (double)n, cy = sy / (double)n, cz = sz / (double)n;
    return __builtin_fma(cx, cx, __builtin_fma(cy, cy, cz * cz));
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

// ---- both geometries: the verdict on device arrays, the state of a chunk at its start, the results at its end -------------------
// bad[k] = the first box whose array k (pos, vel, sites) holds a value that is not finite; arrays may be NULL.
__global__ __launch_bounds__(kThreads) void k_ti_check(size_t total, int n, const double* __restrict__ pos, const double* __restrict__ vel,
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

// One lane per molecule: x = pos, v = vel or 0, F = 0; the first lane of a box sets its row, its accumulators and its flags.
__global__ __launch_bounds__(kThreads) void k_ti_begin(int n, const double* __restrict__ pos, const double* __restrict__ vel, double* __restrict__ x,
                                                       double* __restrict__ v, double* __restrict__ F, double* __restrict__ row,
                                                       double* __restrict__ acc, int* __restrict__ si)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    x[m] = pos[m]; x[m + 1] = pos[m + 1]; x[m + 2] = pos[m + 2];
    v[m] = vel ? vel[m] : 0.0; v[m + 1] = vel ? vel[m + 1] : 0.0; v[m + 2] = vel ? vel[m + 2] : 0.0;
    F[m] = F[m + 1] = F[m + 2] = 0.0;
    if (i == 0) {
        for (int k = 0; k < kRow; ++k) row[kRow * (size_t)b + k] = acc[kRow * (size_t)b + k] = 0.0;
        for (int k = 0; k < kSI; ++k) si[kSI * (size_t)b + k] = 0;
    }
}

// One lane per molecule: the state out; the first lane of a box writes its status.
__global__ __launch_bounds__(kThreads) void k_ti_finish(int n, const double* __restrict__ x, const double* __restrict__ v, const double* __restrict__ F,
                                                        const int* __restrict__ si, double* __restrict__ pos_out, double* __restrict__ vel_out,
                                                        double* __restrict__ forces, int* __restrict__ status)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    if (pos_out) { pos_out[m] = x[m]; pos_out[m + 1] = x[m + 1]; pos_out[m + 2] = x[m + 2]; }
    if (vel_out) { vel_out[m] = v[m]; vel_out[m + 1] = v[m + 1]; vel_out[m + 2] = v[m + 2]; }
    if (forces) { forces[m] = F[m]; forces[m + 1] = F[m + 1]; forces[m + 2] = F[m + 2]; }
    if (i == 0 && status) {
        const int* I = si + kSI * (size_t)b;
        status[2 * (size_t)b] = I[3];
        status[2 * (size_t)b + 1] = (I[0] | I[1] | I[2]) ? 1 : 0;
    }
}

// ---- general geometry ----------------------------------------------------------------------------------------------------
// Per box in scratch after the sort's pieces (mw_lib_cells.h): mom [n][kMom] and en [n] in cell order; part [workgroups][kPart];
// x, v, F [n][3] by index; the row [kRow], the accumulators [kRow] and the ints [kSI].

// Stages 2 and 3 and the test of stage 4, one lane per molecule.
__global__ __launch_bounds__(kThreads) void k_ti_drift1(int n, Consts C, const unsigned long long* __restrict__ streams, int b0,
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
__global__ __launch_bounds__(kThreads) void k_ti_drift2(int n, double hd, double* __restrict__ x, const double* __restrict__ v,
                                                        const int* __restrict__ si)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    const int* I = si + kSI * (size_t)b;
    if (I[0] || I[2] || i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    drift(hd, v[m], v[m + 1], v[m + 2], x[m], x[m + 1], x[m + 2]);
}

// The moment pass, one lane per molecule in sorted order.
__global__ __launch_bounds__(kThreads) void k_ti_moments(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
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

// The force pass, one lane per molecule in sorted order: F_mW of the molecule, mixed with the spring of its site into F_tot and
// written by index; stage 6 of this step (`do6`) and stage 1 of the next with its guard (`do1`); the partial sums of the
// workgroup from the velocities between the two.  mix [box][kMix] = (oml, nlk, the mode).
__global__ __launch_bounds__(kThreads) void k_ti_forces(int n, int cap, Consts C, int do6, int do1, const double* __restrict__ par,
                                                        const int* __restrict__ grid, const int* __restrict__ start, const double* __restrict__ ss,
                                                        const int* __restrict__ idx, int* si, const double* __restrict__ mom,
                                                        const double* __restrict__ en, const double* __restrict__ ref, const double* __restrict__ mix,
                                                        const double* __restrict__ x, double* __restrict__ v, double* __restrict__ F,
                                                        double* __restrict__ part)
{
    __shared__ double red[kThreads / 64][kPart];
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    int* I = si + kSI * (size_t)b;
    if (I[0] || I[2]) return;                                          // the whole workgroup
    const size_t o = (size_t)b * n;
    double val[kPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < n) {
        const double* H = par + 18 * (size_t)b;
        const double* S = ss + 3 * o;
        const double* Mb = mom + kMom * o;
        const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
        double Mi[kMom];
        mw::load_moments(Mb + kMom * (size_t)p, Mi);
        double fx = 0.0, fy = 0.0, fz = 0.0;
        const double* mixb = mix + kMix * (size_t)b;
        asm("" : "+v"(mixb));                                          // (the address waits in a vector register while the walk needs the scalar ones)
        const CellRegs hc(H);
        walk_cells(s0, s1, s2, mw::kRcSq, hc.c, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), S,
                   [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
                       if (q == p) return;                             // an image of the molecule itself: d is constant
                       double Mj[kMom];
                       mw::load_moments(Mb + kMom * (size_t)q, Mj);
                       entry_force(Mi, Mj, r2, dx, dy, dz, fx, fy, fz);
                   });
        const size_t m = 3 * (o + idx[o + p]);
        const double d0 = x[m] - ref[m], d1 = x[m + 1] - ref[m + 1], d2 = x[m + 2] - ref[m + 2];
        mix_force((int)mixb[2], in_vgpr(mixb[0]), in_vgpr(mixb[1]), d0, d1, d2, fx, fy, fz);
        F[m] = fx; F[m + 1] = fy; F[m + 2] = fz;
        double vx = v[m], vy = v[m + 1], vz = v[m + 2];
        if (do6) kick(C.hk, fx, fy, fz, vx, vy, vz);
        val[0] = en[o + p];
        val[1] = __builtin_fma(vx, vx, __builtin_fma(vy, vy, vz * vz));
        val[2] = __builtin_fma(d0, d0, __builtin_fma(d1, d1, d2 * d2));
        val[3] = d0; val[4] = d1; val[5] = d2;
        val[6] = largest_abs(fx, fy, fz);
        if (do1) {
            kick(C.hk, fx, fy, fz, vx, vy, vz);
            if (guard_fails(C.hd, C.lim2, vx, vy, vz)) atomicOr(I + 1, 1);
        }
        if (do6 || do1) { v[m] = vx; v[m + 1] = vy; v[m + 2] = vz; }
    }
    const double r = block_reduce<6, 1>(val, red);
    if (threadIdx.x < kPart) part[((size_t)b * gridDim.x + blockIdx.x) * kPart + threadIdx.x] = r;
}

// One workgroup of 64 per box after the evaluation number e (= the steps completed with it): lane k < kRow makes the row's field k
// from the box's partials added in workgroup order (field 3 from column 6, field 4 from columns 3 - 5); a frozen box keeps its
// row.  The row goes to the trace when e is a multiple of sample_every, and lane k adds field k to the box's block accumulator.
// Lane 0 counts the step and takes the guards' flags over.
__global__ __launch_bounds__(64) void k_ti_row(int nwg, int n, int e, Consts C, const double* __restrict__ part, double* __restrict__ row,
                                               double* __restrict__ acc, int* __restrict__ si, double* __restrict__ trace, double* __restrict__ blocks)
{
    const int b = blockIdx.x, k = threadIdx.x;
    int* I = si + kSI * (size_t)b;
    const bool frozen = I[0] || I[2];
    const int tripped = I[1];
    if (k < kRow) {
        double a = row[kRow * (size_t)b + k];
        if (!frozen) {
            const double* P = part + (size_t)b * nwg * kPart;
            if (k < 4) {
                const int col = k < 3 ? k : 6;
                a = P[col];
                for (int w = 1; w < nwg; ++w) {
                    const double t = P[(size_t)w * kPart + col];
                    a = k < 3 ? a + t : (t > a ? t : a);
                }
                if (k == 1) a = C.hm * a;
                if (k == 2) a = a / (double)n;
            } else {
                double sx = P[3], sy = P[4], sz = P[5];
                for (int w = 1; w < nwg; ++w) {
                    sx = sx + P[(size_t)w * kPart + 3]; sy = sy + P[(size_t)w * kPart + 4]; sz = sz + P[(size_t)w * kPart + 5];
                }
                a = com_square(sx, sy, sz, n);
            }
            row[kRow * (size_t)b + k] = a;
        }
        if (trace && e % C.sample_every == 0) trace[((size_t)b * C.nrows + e / C.sample_every) * kRow + k] = a;
        bool last;
        const int j = block_of(C, e, last);
        if (j >= 0) {
            double s = acc[kRow * (size_t)b + k] + a;
            if (last) {
                if (blocks) blocks[((size_t)b * C.nblocks + j) * kRow + k] = s / (double)C.block_steps;
                s = 0.0;
            }
            acc[kRow * (size_t)b + k] = s;
        }
    }
    if (k == 0) {
        if (!frozen) I[3] = e;
        if (frozen || tripped) I[0] = 1;
    }
}

// ---- small geometry: one wavefront per box, lane i = molecule i ----------------------------------------------------------------
// The evaluations e0 .. e0 + ne - 1 of one box as in mw_md.hip's k_md_small; x, v, F, the row, the accumulators and the ints are
// read from scratch at the start and written back at the end.  The row and the accumulators are uniform over the wavefront; lane 0
// writes them.  A box that freezes writes its remaining trace rows at once; its last row still goes into the blocks step by step,
// for the rest of this launch and in every launch after.
template <bool THERMOSTAT>
__global__ __launch_bounds__(kThreads) void k_ti_small(int nb, int n, int e0, int ne, Consts Cs, const unsigned long long* __restrict__ streams, int b0,
                                                       unsigned long long step0, const double* __restrict__ par, const double* __restrict__ ref,
                                                       const double* __restrict__ mix, double* __restrict__ x, double* __restrict__ v,
                                                       double* __restrict__ F, double* __restrict__ row,
                                                       double* __restrict__ acc, int* __restrict__ si, double* __restrict__ trace,
                                                       double* __restrict__ blocks)
{
    __shared__ double lds[kSmallBoxesPerWg][(3 + kMom) * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * kSmallBoxesPerWg + wave;
    if (b >= nb) return;                                   // the whole wavefront; no workgroup barrier below
    int* I = si + kSI * (size_t)b;
    double* R = row + kRow * (size_t)b;
    double* A = acc + kRow * (size_t)b;
    double r0 = in_vgpr(R[0]), r1 = in_vgpr(R[1]), r2 = in_vgpr(R[2]), r3 = in_vgpr(R[3]), r4 = in_vgpr(R[4]);
    double a0 = in_vgpr(A[0]), a1 = in_vgpr(A[1]), a2 = in_vgpr(A[2]), a3 = in_vgpr(A[3]), a4 = in_vgpr(A[4]);
    double* B = blocks ? blocks + (size_t)b * Cs.nblocks * kRow : nullptr;
    const double per = (double)Cs.block_steps;
    // the row after evaluation e into the accumulators
    auto tally = [&](int e) {
        bool last;
        const int j = block_of(Cs, e, last);
        if (j < 0) return;
        a0 = a0 + r0; a1 = a1 + r1; a2 = a2 + r2; a3 = a3 + r3; a4 = a4 + r4;
        if (last) {
            if (B && lane == 0) {
                double* T = B + (size_t)j * kRow;
                T[0] = a0 / per; T[1] = a1 / per; T[2] = a2 / per; T[3] = a3 / per; T[4] = a4 / per;
            }
            a0 = a1 = a2 = a3 = a4 = 0.0;
        }
    };
    if (I[0]) {                                            // frozen in an earlier launch: the blocks alone
        for (int e = e0; e < e0 + ne; ++e) tally(e);
        if (lane == 0) { A[0] = a0; A[1] = a1; A[2] = a2; A[3] = a3; A[4] = a4; }
        return;
    }
    double* S = lds[wave];
    double* ML = S + 3 * 64;
    const double* H = par + 18 * (size_t)b;
    const CellRegs hc(H), hi(H + 9);
    const bool active = lane < n;
    const size_t m = 3 * ((size_t)b * n + (active ? lane : 0));
    double x0 = active ? x[m] : 0.0, x1 = active ? x[m + 1] : 0.0, x2 = active ? x[m + 2] : 0.0;
    double vx = active ? v[m] : 0.0, vy = active ? v[m + 1] : 0.0, vz = active ? v[m + 2] : 0.0;
    double fx = active ? F[m] : 0.0, fy = active ? F[m + 1] : 0.0, fz = active ? F[m + 2] : 0.0;
    const double q0 = active ? ref[m] : 0.0, q1 = active ? ref[m + 1] : 0.0, q2 = active ? ref[m + 2] : 0.0;
    // (the call's constants and the box's row are kept out of the scalar registers, for the same reason as the cell)
    Consts C = Cs;
    C.hk = in_vgpr(Cs.hk); C.hd = in_vgpr(Cs.hd); C.c1 = in_vgpr(Cs.c1); C.c2 = in_vgpr(Cs.c2); C.lim2 = in_vgpr(Cs.lim2); C.hm = in_vgpr(Cs.hm);
    const double oml = in_vgpr(mix[kMix * (size_t)b]), nlk = in_vgpr(mix[kMix * (size_t)b + 1]);
    const int md = (int)mix[kMix * (size_t)b + 2];
    const unsigned long long id = streams ? streams[b] : (unsigned long long)(b0 + b);
    int steps = I[3];
    bool frozen = false;
    for (int e = e0; e < e0 + ne; ++e) {
        if (e > 0) {
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
        mw::wave_fence();
        Sums a;
        walk_small(n, active, mw::kRcSq, hc.c, S, s0, s1, s2, [&](int, int, double d2, double dx, double dy, double dz) { a.add(d2, dx, dy, dz); });
        double Mi[kMom];
        a.record(Mi);
#pragma unroll
        for (int k = 0; k < kMom; ++k) ML[64 * k + lane] = Mi[k];
        mw::wave_fence();
        fx = fy = fz = 0.0;
        walk_small(n, active, mw::kRcSq, hc.c, S, s0, s1, s2, [&](int j, int, double d2, double dx, double dy, double dz) {
            if (j == lane) return;                                     // an image of the molecule itself: d is constant
            double Mj[kMom];
#pragma unroll
            for (int k = 0; k < kMom; ++k) Mj[k] = ML[64 * k + j];
            entry_force(Mi, Mj, d2, dx, dy, dz, fx, fy, fz);
        });
        const double d0 = x0 - q0, d1 = x1 - q1, d2 = x2 - q2;
        mix_force(md, oml, nlk, d0, d1, d2, fx, fy, fz);
        if (e > 0) kick(C.hk, fx, fy, fz, vx, vy, vz);
        r0 = in_vgpr(wave_total(active ? a.energy() : 0.0));
        r1 = in_vgpr(C.hm * wave_total(__builtin_fma(vx, vx, __builtin_fma(vy, vy, vz * vz))));
        r2 = in_vgpr(wave_total(__builtin_fma(d0, d0, __builtin_fma(d1, d1, d2 * d2))) / (double)n);
        r3 = in_vgpr(wave_largest(largest_abs(fx, fy, fz)));
        r4 = in_vgpr(com_square(wave_total(d0), wave_total(d1), wave_total(d2), n));
        steps = e;
        if (trace && lane == 0 && e % C.sample_every == 0) {
            double* T = trace + ((size_t)b * C.nrows + e / C.sample_every) * kRow;
            T[0] = r0; T[1] = r1; T[2] = r2; T[3] = r3; T[4] = r4;
        }
        tally(e);
        if (e < C.nsteps) {
            kick(C.hk, fx, fy, fz, vx, vy, vz);
            if (__ballot(active && guard_fails(C.hd, C.lim2, vx, vy, vz))) { frozen = true; break; }
        }
    }
    if (active) {
        x[m] = x0; x[m + 1] = x1; x[m + 2] = x2;
        v[m] = vx; v[m + 1] = vy; v[m + 2] = vz;
        F[m] = fx; F[m + 1] = fy; F[m + 2] = fz;
    }
    if (frozen) {
        if (trace) {
            for (int t = steps / C.sample_every + 1 + lane; t < C.nrows; t += 64) {
                double* T = trace + ((size_t)b * C.nrows + t) * kRow;
                T[0] = r0; T[1] = r1; T[2] = r2; T[3] = r3; T[4] = r4;
            }
        }
        for (int e = steps + 1; e < e0 + ne; ++e) tally(e);
    }
    if (lane == 0) {
        R[0] = r0; R[1] = r1; R[2] = r2; R[3] = r3; R[4] = r4;
        A[0] = a0; A[1] = a1; A[2] = a2; A[3] = a3; A[4] = a4;
        I[3] = steps;
        if (frozen) I[0] = 1;
    }
}

}  // namespace mwti

namespace {

using namespace mwti;

constexpr int kEvPerStep = 5;
constexpr int kBlock = 32;                         // evaluations (general) or launches (small) between two harvests of the timers
constexpr int kDefaultSlice = 64, kMaxSlice = 256;

struct State : Runtime<1> {
    Buf scratch, par, grid, mix, pos, vel, ref, streams, pos_out, vel_out, forces, trace, blocks, status, bad;
    std::vector<hipEvent_t> pool;                  // kEvPerStep per evaluation of a block
    int slice = kDefaultSlice;
    int last[MW_TI_PLAN_FIELDS] = {0};
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
} g;

// The scratch of one box: the sort's pieces and what the passes keep (general), then what both geometries carry.
struct Layout : SortLayout {
    int nwg = 0;
    size_t mom = 0, en = 0, part = 0, x = 0, v = 0, F = 0, row = 0, acc = 0, si = 0, per_box = 0;
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
    }
    l.x = o;   o += align16(24 * (size_t)n);
    l.v = o;   o += align16(24 * (size_t)n);
    l.F = o;   o += align16(24 * (size_t)n);
    l.row = o; o += align16(8 * (size_t)kRow);
    l.acc = o; o += align16(8 * (size_t)kRow);
    l.si = o;  o += align16(4 * (size_t)kSI);
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
        return fail("%s: one box needs %zu bytes of scratch (nwater = %d) and does not fit the budget of %zu bytes (MW_TI_SCRATCH_MB)",
                    who, p.per_box, n, budget);
    const size_t most = p.small ? (size_t)kSmallChunkBoxes : (size_t)kMaxChunkBoxes;
    p.bpc = (int)(fit < most ? fit : most);
    if (p.bpc > nboxes) p.bpc = nboxes;
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

void ti_fields(const Plan& p, const int* grid, int* f)
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

int check_scalars(const char* who, int nboxes, int n, unsigned long long seed, int nsteps, int sample_every, int equil_steps, int block_steps, double dt,
                  double mass, double kT, double gamma, Consts& C)
{
    if (check_counts(who, nboxes, n)) return 1;
    if (nsteps < 0 || nsteps > MW_TI_MAX_STEPS) return fail("%s: nsteps = %d outside 0..%d", who, nsteps, MW_TI_MAX_STEPS);
    if (sample_every < 1) return fail("%s: sample_every = %d is not at least 1", who, sample_every);
    if (equil_steps < 0) return fail("%s: equil_steps = %d is negative", who, equil_steps);
    if (block_steps < 0) return fail("%s: block_steps = %d is negative", who, block_steps);
    if (!(dt > 0.0) || !std::isfinite(dt)) return fail("%s: dt = %g atomic time units is not a finite number > 0", who, dt);
    if (!(mass > 0.0) || !std::isfinite(mass)) return fail("%s: mass = %g electron masses is not a finite number > 0", who, mass);
    if (!(kT >= 0.0) || !std::isfinite(kT)) return fail("%s: kT = %g Hartree is not a finite number >= 0", who, kT);
    if (!(gamma >= 0.0) || !std::isfinite(gamma)) return fail("%s: gamma = %g per atomic time unit is not a finite number >= 0", who, gamma);
    C.hk = dt / (2.0 * mass);
    C.hd = dt / 2.0;
    C.c1 = std::exp(-gamma * dt);
    C.c2 = std::sqrt((kT / mass) * (1.0 - C.c1 * C.c1));
    C.lim2 = (mw::kSigA / 4.0) * (mw::kSigA / 4.0);
    C.hm = mass / 2.0;
    C.seed_lo = (uint32_t)seed;
    C.seed_hi = (uint32_t)(seed >> 32);
    C.thermostat = gamma > 0.0 ? 1 : 0;
    C.nsteps = nsteps;
    C.sample_every = sample_every;
    C.nrows = nsteps / sample_every + 1;
    C.equil = equil_steps;
    C.block_steps = block_steps;
    C.nblocks = (block_steps > 0 && nsteps >= equil_steps) ? (nsteps - equil_steps) / block_steps : 0;
    if (!std::isfinite(C.hk) || !(C.hk > 0.0)) return fail("%s: dt / (2 mass) = %g with dt = %g and mass = %g is not a finite number > 0", who, C.hk, dt, mass);
    if (!std::isfinite(C.c2)) return fail("%s: kT = %g over mass = %g is not finite", who, kT, mass);
    return 0;
}

// lambdas and springs (host) checked, and what the kernels read made of them: mix [box][kMix] = (oml, nlk, the mode)
int check_mixing(const char* who, int nboxes, const double* lambdas, const double* springs, std::vector<double>& mix)
{
    mix.resize(kMix * (size_t)nboxes);
    for (int b = 0; b < nboxes; ++b)
        if (!(lambdas[b] >= 0.0 && lambdas[b] <= 1.0)) return fail("%s: lambdas: box %d holds lambda = %g outside 0..1", who, b, lambdas[b]);
    for (int b = 0; b < nboxes; ++b)
        if (!(springs[b] > 0.0) || !std::isfinite(springs[b]))
            return fail("%s: springs: box %d holds k = %g Hartree / bohr^2, not a finite number > 0", who, b, springs[b]);
    for (int b = 0; b < nboxes; ++b) {
        mix[kMix * (size_t)b] = 1.0 - lambdas[b];
        mix[kMix * (size_t)b + 1] = -(lambdas[b] * springs[b]);
        mix[kMix * (size_t)b + 2] = (double)(lambdas[b] == 0.0 ? kMd : lambdas[b] == 1.0 ? kEinstein : kMixed);
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
    if (bref >= 0) return fail("%s: sites: box %d holds a position that is not finite", who, bref);
    return 0;
}

const char kRadius[] = "a_sigma";             // the radius the cells are checked against, in the messages

int check_live(const char* who) { return check_live(who, "mw_ti_init", g); }

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

// waits for what has been enqueued and adds the time between the events e + from and e + from + 1 of every group to ms[to]
int harvest(int used, int per, const int (*map)[2], int nmap, float* ms)
{
    HIPOK(hipStreamSynchronize(g.stream));
    for (int e = 0; e < used; e += per)
        for (int k = 0; k < nmap; ++k) {
            float t = 0.0f;
            HIPOK(hipEventElapsedTime(&t, g.pool[e + map[k][0]], g.pool[e + map[k][0] + 1]));
            ms[map[k][1]] += t;
        }
    return 0;
}

struct Arrays {
    const double *pos, *vel, *ref;
    const unsigned long long* streams;
    double *pos_out, *vel_out, *forces, *trace, *blocks;
    int* status;
};

// The work of both entries, arguments already checked.  par, grid and mix are on the host; the arrays of `a` are device
// pointers when `dev`, host pointers otherwise.
int run(const char* who, int nboxes, int n, const std::vector<double>& par, const std::vector<int>& grid, const std::vector<double>& mix,
        const Consts& C, unsigned long long step0, bool dev, const Arrays& a)
{
    Plan p;
    if (make_plan(who, n, nboxes, g.budget, g.slice, p)) return 1;
    const Layout& l = p.lay;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (reserve(g.scratch, p.per_box * (size_t)p.bpc)) return 1;
    if (reserve(g.par, par.size() * sizeof(double))) return 1;
    if (reserve(g.grid, grid.size() * sizeof(int))) return 1;
    if (reserve(g.mix, mix.size() * sizeof(double))) return 1;
    HIPOK(hipMemcpyAsync(g.par.p, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPOK(hipMemcpyAsync(g.grid.p, grid.data(), grid.size() * sizeof(int), hipMemcpyHostToDevice, g.stream));
    HIPOK(hipMemcpyAsync(g.mix.p, mix.data(), mix.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
    const size_t vec = 24 * (size_t)n, rowbytes = 8 * (size_t)kRow * C.nrows, blockbytes = 8 * (size_t)kRow * C.nblocks;
    const bool want_blocks = a.blocks && C.nblocks > 0;
    if (!dev) {
        if (reserve(g.pos, vec * p.bpc)) return 1;
        if (a.vel && reserve(g.vel, vec * p.bpc)) return 1;
        if (a.ref != a.pos && reserve(g.ref, vec * p.bpc)) return 1;
        if (a.streams && reserve(g.streams, 8 * (size_t)p.bpc)) return 1;
        if (a.pos_out && reserve(g.pos_out, vec * p.bpc)) return 1;
        if (a.vel_out && reserve(g.vel_out, vec * p.bpc)) return 1;
        if (a.forces && reserve(g.forces, vec * p.bpc)) return 1;
        if (a.trace && reserve(g.trace, rowbytes * p.bpc)) return 1;
        if (want_blocks && reserve(g.blocks, blockbytes * p.bpc)) return 1;
        if (a.status && reserve(g.status, 8 * (size_t)p.bpc)) return 1;
    }
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int evals = C.nsteps + 1;
    static const int kGeneralMap[4][2] = {{0, 3}, {1, 0}, {2, 1}, {3, 2}};     // drift, sort, moments, forces
    static const int kSmallMap[1][2] = {{0, 2}};
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const size_t first = 3 * (size_t)n * b0;
        const double* d_pos = a.pos + first;
        const double* d_vel = a.vel ? a.vel + first : nullptr;
        const double* d_ref = a.ref + first;
        const unsigned long long* d_streams = a.streams ? a.streams + b0 : nullptr;
        if (!dev) {
            HIPOK(hipMemcpyAsync(g.pos.p, d_pos, vec * nb, hipMemcpyHostToDevice, g.stream));
            if (a.ref == a.pos) d_ref = (const double*)g.pos.p;
            else { HIPOK(hipMemcpyAsync(g.ref.p, d_ref, vec * nb, hipMemcpyHostToDevice, g.stream)); d_ref = (const double*)g.ref.p; }
            d_pos = (const double*)g.pos.p;
            if (d_vel) { HIPOK(hipMemcpyAsync(g.vel.p, d_vel, vec * nb, hipMemcpyHostToDevice, g.stream)); d_vel = (const double*)g.vel.p; }
            if (d_streams) {
                HIPOK(hipMemcpyAsync(g.streams.p, d_streams, 8 * (size_t)nb, hipMemcpyHostToDevice, g.stream));
                d_streams = (const unsigned long long*)g.streams.p;
            }
        }
        const double* d_par = (const double*)g.par.p + 18 * (size_t)b0;
        const int* d_grid = (const int*)g.grid.p + 4 * (size_t)b0;
        const double* d_mix = (const double*)g.mix.p + kMix * (size_t)b0;
        double* d_out = !a.pos_out ? nullptr : dev ? a.pos_out + first : (double*)g.pos_out.p;
        double* d_vout = !a.vel_out ? nullptr : dev ? a.vel_out + first : (double*)g.vel_out.p;
        double* d_forces = !a.forces ? nullptr : dev ? a.forces + first : (double*)g.forces.p;
        double* d_trace = !a.trace ? nullptr : dev ? a.trace + (size_t)kRow * C.nrows * b0 : (double*)g.trace.p;
        double* d_blocks = !want_blocks ? nullptr : dev ? a.blocks + (size_t)kRow * C.nblocks * b0 : (double*)g.blocks.p;
        int* d_status = !a.status ? nullptr : dev ? a.status + 2 * (size_t)b0 : (int*)g.status.p;
        char* base = (char*)g.scratch.p;
        const size_t B = (size_t)p.bpc;
        double* x = (double*)(base + l.x * B);
        double* v = (double*)(base + l.v * B);
        double* F = (double*)(base + l.F * B);
        double* row = (double*)(base + l.row * B);
        double* acc = (double*)(base + l.acc * B);
        int* si = (int*)(base + l.si * B);
        const dim3 grid_m = per_molecule(n, nb);
        hipLaunchKernelGGL(k_ti_begin, grid_m, dim3(kThreads), 0, g.stream, n, d_pos, d_vel, x, v, F, row, acc, si);
        HIPOK(hipGetLastError());
        int used = 0;                                                          // events recorded since the last harvest
        if (p.small) {
            for (int e0 = 0; e0 < evals; e0 += g.slice) {
                const int ne = evals - e0 < g.slice ? evals - e0 : g.slice;
                HIPOK(hipEventRecord(g.pool[used], g.stream));
                hipLaunchKernelGGL(C.thermostat ? k_ti_small<true> : k_ti_small<false>, dim3((unsigned)((nb + kSmallBoxesPerWg - 1) / kSmallBoxesPerWg)), dim3(kThreads), 0, g.stream, nb, n, e0,
                                   ne, C, d_streams, b0, step0, d_par, d_ref, d_mix, x, v, F, row, acc, si, d_trace, d_blocks);
                HIPOK(hipGetLastError());
                HIPOK(hipEventRecord(g.pool[used + 1], g.stream));
                used += 2;
                if (used + 2 > 2 * kBlock) {
                    if (harvest(used, 2, kSmallMap, 1, ms)) return 1;
                    used = 0;
                }
            }
            if (harvest(used, 2, kSmallMap, 1, ms)) return 1;
        } else {
            double* mom = (double*)(base + l.mom * B);
            double* en = (double*)(base + l.en * B);
            double* part = (double*)(base + l.part * B);
            for (int e = 0; e < evals; ++e) {
                Sorted s;
                HIPOK(hipEventRecord(g.pool[used], g.stream));
                if (e > 0) {
                    hipLaunchKernelGGL(k_ti_drift1, grid_m, dim3(kThreads), 0, g.stream, n, C, d_streams, b0, step0 + (unsigned long long)(e - 1), x, v,
                                       si);
                    HIPOK(hipGetLastError());
                    hipLaunchKernelGGL(k_ti_drift2, grid_m, dim3(kThreads), 0, g.stream, n, C.hd, x, (const double*)v, (const int*)si);
                    HIPOK(hipGetLastError());
                }
                HIPOK(hipEventRecord(g.pool[used + 1], g.stream));
                if (sort_into_cells(g.stream, n, nb, l, base, B, d_par, d_grid, (const double*)x, s)) return 1;
                HIPOK(hipEventRecord(g.pool[used + 2], g.stream));
                hipLaunchKernelGGL(k_ti_moments, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, d_par, d_grid, s.start, s.ss, (const int*)si, mom, en);
                HIPOK(hipGetLastError());
                HIPOK(hipEventRecord(g.pool[used + 3], g.stream));
                hipLaunchKernelGGL(k_ti_forces, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, C, e > 0 ? 1 : 0, e < C.nsteps ? 1 : 0, d_par, d_grid,
                                   s.start, s.ss, s.idx, si, (const double*)mom, (const double*)en, d_ref, d_mix, (const double*)x, v, F, part);
                HIPOK(hipGetLastError());
                hipLaunchKernelGGL(k_ti_row, dim3((unsigned)nb), dim3(64), 0, g.stream, l.nwg, n, e, C, (const double*)part, row, acc, si, d_trace,
                                   d_blocks);
                HIPOK(hipGetLastError());
                HIPOK(hipEventRecord(g.pool[used + 4], g.stream));
                used += kEvPerStep;
                if (used + kEvPerStep > kEvPerStep * kBlock) {
                    if (harvest(used, kEvPerStep, kGeneralMap, 4, ms)) return 1;
                    used = 0;
                }
            }
            if (harvest(used, kEvPerStep, kGeneralMap, 4, ms)) return 1;
        }
        hipLaunchKernelGGL(k_ti_finish, grid_m, dim3(kThreads), 0, g.stream, n, (const double*)x, (const double*)v, (const double*)F, (const int*)si,
                           d_out, d_vout, d_forces, d_status);
        HIPOK(hipGetLastError());
        if (!dev) {
            if (a.pos_out) HIPOK(hipMemcpyAsync(a.pos_out + first, g.pos_out.p, vec * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.vel_out) HIPOK(hipMemcpyAsync(a.vel_out + first, g.vel_out.p, vec * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.forces) HIPOK(hipMemcpyAsync(a.forces + first, g.forces.p, vec * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.trace) HIPOK(hipMemcpyAsync(a.trace + (size_t)kRow * C.nrows * b0, g.trace.p, rowbytes * nb, hipMemcpyDeviceToHost, g.stream));
            if (want_blocks) HIPOK(hipMemcpyAsync(a.blocks + (size_t)kRow * C.nblocks * b0, g.blocks.p, blockbytes * nb, hipMemcpyDeviceToHost, g.stream));
            if (a.status) HIPOK(hipMemcpyAsync(a.status + 2 * (size_t)b0, g.status.p, 8 * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
        }
        HIPOK(hipStreamSynchronize(g.stream));               // the next chunk reuses the scratch and the staging buffers
    }
    ti_fields(p, grid.data(), g.last);
    g.have_last = true;
    for (int k = 0; k < 4; ++k) g.ms[k] = ms[k];
    return 0;
}

// what both entries check before they look at an array: the scalars and the pointers that must be there
int check_call(const char* who, int nboxes, int nwater, const double* cells, const double* sites, const double* lambdas, const double* springs,
               unsigned long long seed, int nsteps, int sample_every, int equil_steps, int block_steps, double dt, double mass, double kT, double gamma,
               Consts& C)
{
    if (check_scalars(who, nboxes, nwater, seed, nsteps, sample_every, equil_steps, block_steps, dt, mass, kT, gamma, C)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!sites) return fail("%s: sites is NULL", who);
    if (!lambdas) return fail("%s: lambdas is NULL", who);
    if (!springs) return fail("%s: springs is NULL", who);
    return 0;
}

}  // namespace

extern "C" {

const char* mw_ti_last_error(void) { return g_err; }
int mw_ti_is_initialised(void) { return g.live ? 1 : 0; }

int mw_ti_init(int device)
{
    const char* who = "mw_ti_init";
    if (g.live) return fail("%s: already initialised", who);
    int slice = kDefaultSlice;
    if (env_int(who, "MW_TI_SLICE", 1, kMaxSlice, slice)) return 1;
    if (runtime_init(who, "MW_TI_SCRATCH_MB", device, g)) return 1;
    g.slice = slice;
    DeviceScope scope;
    hipError_t e = scope.enter(g.device);
    g.pool.assign((size_t)kEvPerStep * kBlock, nullptr);
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

int mw_ti_finalize(void)
{
    if (g.live) {
        DeviceScope scope;
        HIPOK(scope.enter(g.device));
        HIPOK(hipStreamSynchronize(g.stream));
        for (auto& ev : g.pool) HIPOK(hipEventDestroy(ev));
        g.pool.clear();
    }
    if (runtime_finalize(g, {&g.scratch, &g.par, &g.grid, &g.mix, &g.pos, &g.vel, &g.ref, &g.streams, &g.pos_out, &g.vel_out, &g.forces,
                             &g.trace, &g.blocks, &g.status, &g.bad}))
        return 1;
    g = State{};
    return 0;
}

int mw_ti_run(int nboxes, int nwater, const double* cells, const double* pos, const double* vel, const double* sites, const double* lambdas,
              const double* springs, const unsigned long long* streams, unsigned long long seed, unsigned long long step0, int nsteps, int sample_every,
              int equil_steps, int block_steps, double dt, double mass, double kT, double gamma, double* pos_out, double* vel_out, double* forces,
              double* trace, double* blocks, int* status)
{
    const char* who = "mw_ti_run";
    std::vector<double> par, mix;
    std::vector<int> grid;
    Consts C;
    if (check_call(who, nboxes, nwater, cells, sites, lambdas, springs, seed, nsteps, sample_every, equil_steps, block_steps, dt, mass, kT, gamma, C)) return 1;
    if (check_cells(who, kRadius, nboxes, nwater, cells, mw::kSigA, par, grid)) return 1;
    if (check_mixing(who, nboxes, lambdas, springs, mix)) return 1;
    if (report_bad(who, first_bad_box(pos, nboxes, nwater), first_bad_box(vel, nboxes, nwater), first_bad_box(sites, nboxes, nwater))) return 1;
    if (check_live(who)) return 1;
    return run(who, nboxes, nwater, par, grid, mix, C, step0, false,
               Arrays{pos ? pos : sites, vel, sites, streams, pos_out, vel_out, forces, trace, blocks, status});
}

int mw_ti_run_device(int nboxes, int nwater, const double* cells, const double* pos, const double* vel, const double* sites, const double* lambdas,
                     const double* springs, const unsigned long long* streams, unsigned long long seed, unsigned long long step0, int nsteps,
                     int sample_every, int equil_steps, int block_steps, double dt, double mass, double kT, double gamma, double* pos_out,
                     double* vel_out, double* forces, double* trace, double* blocks, int* status)
{
    const char* who = "mw_ti_run_device";
    std::vector<double> par, mix;
    std::vector<int> grid;
    Consts C;
    if (check_call(who, nboxes, nwater, cells, sites, lambdas, springs, seed, nsteps, sample_every, equil_steps, block_steps, dt, mass, kT, gamma, C)) return 1;
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (fetch_cells(who, kRadius, nboxes, nwater, cells, mw::kSigA, par, grid)) return 1;
    std::vector<double> h_lambdas((size_t)nboxes), h_springs((size_t)nboxes);
    HIPOK(hipMemcpy(h_lambdas.data(), lambdas, 8 * (size_t)nboxes, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(h_springs.data(), springs, 8 * (size_t)nboxes, hipMemcpyDeviceToHost));
    if (check_mixing(who, nboxes, h_lambdas.data(), h_springs.data(), mix)) return 1;
    // the verdict on the positions, velocities and sites: one kernel that writes three ints, read before anything else is launched
    if (reserve(g.bad, 3 * sizeof(int))) return 1;
    int bad[3] = {nboxes, nboxes, nboxes};
    HIPOK(hipMemcpyAsync(g.bad.p, bad, sizeof bad, hipMemcpyHostToDevice, g.stream));
    const size_t total = (size_t)nboxes * nwater, nblk = (total + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_ti_check, dim3((unsigned)(nblk < 65536 ? nblk : 65536)), dim3(kThreads), 0, g.stream, total, nwater, pos, vel, sites,
                       (int*)g.bad.p);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(bad, g.bad.p, sizeof bad, hipMemcpyDeviceToHost, g.stream));
    HIPOK(hipStreamSynchronize(g.stream));
    if (report_bad(who, bad[0] < nboxes ? bad[0] : -1, bad[1] < nboxes ? bad[1] : -1, bad[2] < nboxes ? bad[2] : -1)) return 1;
    return run(who, nboxes, nwater, par, grid, mix, C, step0, true,
               Arrays{pos ? pos : sites, vel, sites, streams, pos_out, vel_out, forces, trace, blocks, status});
}

int mw_ti_plan(int nwater, const double* cell, int nboxes, int* out, int nout)
{
    const char* who = "mw_ti_plan";
    std::vector<int> grid;
    if (check_counts(who, nboxes, nwater)) return 1;
    if (plan_grid(who, kRadius, nwater, cell, mw::kSigA, out, nout, grid)) return 1;
    Plan p;
    if (make_plan(who, nwater, nboxes, g.live ? g.budget : kDefaultBudget, g.live ? g.slice : kDefaultSlice, p)) return 1;
    int f[MW_TI_PLAN_FIELDS];
    ti_fields(p, grid.data(), f);
    copy_fields(f, MW_TI_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_ti_last(int* out, int nout) { return last_fields("mw_ti_last", "mw_ti_init", g, g.last, MW_TI_PLAN_FIELDS, out, nout); }

int mw_ti_elapsed_ms(float* sort, float* moments, float* forces, float* drift)
{
    if (check_live("mw_ti_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_ti_elapsed_ms: no call has launched yet");
    if (sort) *sort = g.ms[0];
    if (moments) *moments = g.ms[1];
    if (forces) *forces = g.ms[2];
    if (drift) *drift = g.ms[3];
    return 0;
}

}  // extern "C"
