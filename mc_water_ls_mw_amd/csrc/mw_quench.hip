// libmw_quench.so -- the inherent-structure quenches of include/mw_quench.h: FIRE on the full-box mW energy at fixed cell, every
// box of a call on its own trajectory.  General geometry (nwater > 64), per iteration: the counting sort of mw_lib_cells.h,
// k_quench_moments (one lane per molecule in sorted order walks the 27 cells: the ten moments and the molecule's energy),
// k_quench_forces (a second walk over the molecule's own moments and those of every entry; the workgroup's partial sums),
// k_quench_decide (one workgroup per box adds the partials in order and takes FIRE's decision), k_quench_step (the velocity mix,
// the largest |dx|) and k_quench_move.  Small geometry (nwater <= 64): k_quench_small, one wavefront per box with fractional
// positions and moments in LDS, many iterations per launch.  k_quench_begin copies the positions in, k_quench_finish writes the
// results.  Every bit of a box's results depends on the box, ftol, max_iter and fire alone (mw_quench.h): the arithmetic is
// spelled out in fma / mul / add with contraction off, every sum has a fixed order, there is no floating-point atomic, and a
// box that has stopped is skipped by every kernel.  The moments, the derivatives and the reductions are those of
// mw_lib_forces.h, shared with libmw_md.so; this library shares mw_common.hip.h with the engine and nothing else.
#include "../../include/mw_quench.h"

#include "mw_common.hip.h"

#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too
#include "mw_lib_cells.h"
#include "mw_lib_forces.h"                     // Sums, entry_force, CellRegs and the reductions: shared with libmw_md.so

namespace mwquench {

using namespace mwcells;
using namespace mwforces;

constexpr int kSmallBoxesPerWg = kThreads / 64;   // one wavefront per box
constexpr int kSmallLdsPerBox = (3 + kMom) * 64 * 8;
constexpr int kSmallLds = kSmallBoxesPerWg * kSmallLdsPerBox;
constexpr int kPart = 5;                          // a workgroup's partial sums: E, F.v, v.v, F.F and the largest |F| component
constexpr int kSD = 8;                            // doubles of a box's state: dt, alpha, E, fmax, E at the start, fmax at the start, ca, cb
constexpr int kSI = 8;                            // ints: evaluations done, npos, stopped, converged, mix
constexpr int kGeneralLds = (kThreads / 64) * kPart * 8;

struct Fire {
    double dt0, dtmax, maxstep, alpha0, f_alpha, f_inc, f_dec, n_min, ftol;
    int max_iter;
};

// ---- FIRE -------------------------------------------------------------------------------------------------------------------
// Steps 2 - 6 of the contract for one box, after the evaluation number t.  Returns true when the box stops (conv: converged);
// otherwise dt, alpha and npos are updated and the velocity mix is v = mix ? ca v + cb F : 0.
__device__ __forceinline__ bool fire_decide(const Fire& f, int t, double fmax, double P, double vv, double FF, double& dt, double& alpha,
                                            int& npos, int& conv, int& mix, double& ca, double& cb)
{
    conv = 0; mix = 0; ca = 0.0; cb = 0.0;
    if (fmax <= f.ftol) { conv = 1; return true; }
    if (t >= f.max_iter) return true;
    if (P > 0.0) {
        npos += 1;
        mix = 1;
        ca = 1.0 - alpha;
        cb = alpha * __builtin_sqrt(vv / FF);
        if ((double)npos > f.n_min) {
            const double grown = dt * f.f_inc;
            dt = grown < f.dtmax ? grown : f.dtmax;
            alpha = alpha * f.f_alpha;
        }
    } else {
        npos = 0;
        dt = dt * f.f_dec;
        alpha = f.alpha0;
    }
    return false;
}

// Step 7 for one molecule: the mixed velocity plus dt F; returns |dx|^2 of dx = dt v.
__device__ __forceinline__ double fire_velocity(int mix, double ca, double cb, double dt, double fx, double fy, double fz, double& vx, double& vy,
                                                double& vz)
{
    const double mx = mix ? ca * vx + cb * fx : 0.0, my = mix ? ca * vy + cb * fy : 0.0, mz = mix ? ca * vz + cb * fz : 0.0;
    vx = __builtin_fma(dt, fx, mx); vy = __builtin_fma(dt, fy, my); vz = __builtin_fma(dt, fz, mz);
    const double dx = dt * vx, dy = dt * vy, dz = dt * vz;
    return __builtin_fma(dx, dx, __builtin_fma(dy, dy, dz * dz));
}

// Steps 8 and 9: d2max is the largest |dx|^2 of the box.
__device__ __forceinline__ void fire_move(double maxstep, double d2max, double dt, double vx, double vy, double vz, double& x, double& y, double& z)
{
    const double dmax = __builtin_sqrt(d2max);
    double dx = dt * vx, dy = dt * vy, dz = dt * vz;
    if (dmax > maxstep) {
        const double s = maxstep / dmax;
        dx = dx * s; dy = dy * s; dz = dz * s;
    }
    x = x + dx; y = y + dy; z = z + dz;
}

// ---- both geometries: the state of a chunk at its start, the results at its end ---------------------------------------------------
// One lane per molecule: x = pos, v = F = 0; the first lane of a box sets its scalars.
__global__ __launch_bounds__(kThreads) void k_quench_begin(int n, Fire f, const double* __restrict__ pos, double* __restrict__ x,
                                                           double* __restrict__ v, double* __restrict__ F, double* __restrict__ sd,
                                                           int* __restrict__ si)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    x[m] = pos[m]; x[m + 1] = pos[m + 1]; x[m + 2] = pos[m + 2];
    v[m] = v[m + 1] = v[m + 2] = 0.0;
    F[m] = F[m + 1] = F[m + 2] = 0.0;
    if (i == 0) {
        double* D = sd + kSD * (size_t)b;
        int* I = si + kSI * (size_t)b;
        D[0] = f.dt0; D[1] = f.alpha0;
        for (int k = 2; k < kSD; ++k) D[k] = 0.0;
        for (int k = 0; k < kSI; ++k) I[k] = 0;
    }
}

// One workgroup per box: the positions and forces out, the displacements added up in index order (lane t takes t, t + 256, ...).
__global__ __launch_bounds__(kThreads) void k_quench_finish(int n, const double* __restrict__ pos, const double* __restrict__ x,
                                                            const double* __restrict__ F, const double* __restrict__ sd, const int* __restrict__ si,
                                                            double* __restrict__ pos_out, double* __restrict__ forces, double* __restrict__ stats,
                                                            int* __restrict__ iters)
{
    __shared__ double red[kThreads / 64][2];
    const int b = blockIdx.x, tid = threadIdx.x;
    double val[2] = {0.0, 0.0};
    for (int i = tid; i < n; i += kThreads) {
        const size_t m = 3 * ((size_t)b * n + i);
        const double x0 = x[m], x1 = x[m + 1], x2 = x[m + 2];
        const double d0 = x0 - pos[m], d1 = x1 - pos[m + 1], d2 = x2 - pos[m + 2];
        const double r2 = __builtin_fma(d0, d0, __builtin_fma(d1, d1, d2 * d2));
        val[0] = val[0] + r2;
        val[1] = r2 > val[1] ? r2 : val[1];
        if (pos_out) { pos_out[m] = x0; pos_out[m + 1] = x1; pos_out[m + 2] = x2; }
        if (forces) { forces[m] = F[m]; forces[m + 1] = F[m + 1]; forces[m + 2] = F[m + 2]; }
    }
    const double r = block_reduce<1, 1>(val, red);
    if (tid < 2) red[0][tid] = r;
    __syncthreads();
    if (tid == 0) {
        const double* D = sd + kSD * (size_t)b;
        const int* I = si + kSI * (size_t)b;
        if (stats) {
            double* s = stats + 6 * (size_t)b;
            s[0] = D[4]; s[1] = D[2]; s[2] = D[5]; s[3] = D[3];
            s[4] = __builtin_sqrt(red[0][1]);
            s[5] = __builtin_sqrt(red[0][0] / (double)n);
        }
        if (iters) { iters[2 * (size_t)b] = I[0]; iters[2 * (size_t)b + 1] = I[3]; }
    }
}

// ---- general geometry ----------------------------------------------------------------------------------------------------
// Per box in scratch after the sort's pieces (mw_lib_cells.h): x, v, F [n][3] by index; mom [n][kMom] and en [n] in cell order;
// part [workgroups][kPart]; the scalars sd [kSD], si [kSI] and dmax (the bits of the largest |dx|^2).

// The moment pass, one lane per molecule in sorted order.
__global__ __launch_bounds__(kThreads) void k_quench_moments(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                             const int* __restrict__ start, const double* __restrict__ ss, const int* __restrict__ si,
                                                             double* __restrict__ mom, double* __restrict__ en)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (si[kSI * (size_t)b + 2] || p >= n) return;
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

// The force pass, one lane per molecule in sorted order: the force of the molecule, written by index, and the partial sums
// of its workgroup.
__global__ __launch_bounds__(kThreads) void k_quench_forces(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                            const int* __restrict__ start, const double* __restrict__ ss, const int* __restrict__ idx,
                                                            const int* __restrict__ si, const double* __restrict__ mom, const double* __restrict__ en,
                                                            const double* __restrict__ v, double* __restrict__ F, double* __restrict__ part)
{
    __shared__ double red[kThreads / 64][kPart];
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (si[kSI * (size_t)b + 2]) return;                               // the whole workgroup
    const size_t o = (size_t)b * n;
    double val[kPart] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < n) {
        const double* H = par + 18 * (size_t)b;
        const double* S = ss + 3 * o;
        const double* Mb = mom + kMom * o;
        const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
        double Mi[kMom];
        mw::load_moments(Mb + kMom * (size_t)p, Mi);
        double fx = 0.0, fy = 0.0, fz = 0.0;
        const CellRegs hc(H);
        walk_cells(s0, s1, s2, mw::kRcSq, hc.c, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), S,
                   [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
                       if (q == p) return;                             // an image of the molecule itself: d is constant
                       double Mj[kMom];
                       mw::load_moments(Mb + kMom * (size_t)q, Mj);
                       entry_force(Mi, Mj, r2, dx, dy, dz, fx, fy, fz);
                   });
        const size_t m = 3 * (o + idx[o + p]);
        F[m] = fx; F[m + 1] = fy; F[m + 2] = fz;
        const double vx = v[m], vy = v[m + 1], vz = v[m + 2];
        val[0] = en[o + p];
        val[1] = __builtin_fma(fx, vx, __builtin_fma(fy, vy, fz * vz));
        val[2] = __builtin_fma(vx, vx, __builtin_fma(vy, vy, vz * vz));
        val[3] = __builtin_fma(fx, fx, __builtin_fma(fy, fy, fz * fz));
        const double ax = __builtin_fabs(fx), ay = __builtin_fabs(fy), az = __builtin_fabs(fz);
        val[4] = ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az);
    }
    const double r = block_reduce<4, 1>(val, red);
    if (threadIdx.x < kPart) part[((size_t)b * gridDim.x + blockIdx.x) * kPart + threadIdx.x] = r;
}

// One workgroup of 64 per box: lane k < kPart adds column k of the box's partials in workgroup order; lane 0 decides.
__global__ __launch_bounds__(64) void k_quench_decide(int nwg, Fire f, const double* __restrict__ part, double* __restrict__ sd, int* __restrict__ si,
                                                      unsigned long long* __restrict__ dmax, int* __restrict__ nstopped)
{
    __shared__ double tot[kPart];
    const int b = blockIdx.x, k = threadIdx.x;
    int* I = si + kSI * (size_t)b;
    if (I[2]) return;
    if (k < kPart) {
        const double* P = part + (size_t)b * nwg * kPart;
        double a = P[k];
        for (int w = 1; w < nwg; ++w) {
            const double t = P[(size_t)w * kPart + k];
            a = k < 4 ? a + t : (t > a ? t : a);
        }
        tot[k] = a;
    }
    __syncthreads();
    if (k != 0) return;
    double* D = sd + kSD * (size_t)b;
    const int t = I[0];
    double dt = D[0], alpha = D[1], ca, cb;
    int npos = I[1], conv, mix;
    D[2] = tot[0]; D[3] = tot[4];
    if (t == 0) { D[4] = tot[0]; D[5] = tot[4]; }
    if (fire_decide(f, t, tot[4], tot[1], tot[2], tot[3], dt, alpha, npos, conv, mix, ca, cb)) {
        I[2] = 1; I[3] = conv;
        atomicAdd(nstopped, 1);
        return;
    }
    D[0] = dt; D[1] = alpha; D[6] = ca; D[7] = cb;
    I[0] = t + 1; I[1] = npos; I[4] = mix;
    dmax[b] = 0ull;
}

// One lane per molecule: the new velocity; the largest |dx|^2 of the box as the larger bit pattern (an integer maximum: the
// squares are not negative, so their order is that of their bits).
__global__ __launch_bounds__(kThreads) void k_quench_step(int n, const double* __restrict__ F, double* __restrict__ v, const double* __restrict__ sd,
                                                          const int* __restrict__ si, unsigned long long* __restrict__ dmax)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    const int* I = si + kSI * (size_t)b;
    if (I[2]) return;                                                  // the whole workgroup
    const double* D = sd + kSD * (size_t)b;
    double d2 = 0.0;
    if (i < n) {
        const size_t m = 3 * ((size_t)b * n + i);
        double vx = v[m], vy = v[m + 1], vz = v[m + 2];
        d2 = fire_velocity(I[4], D[6], D[7], D[0], F[m], F[m + 1], F[m + 2], vx, vy, vz);
        v[m] = vx; v[m + 1] = vy; v[m + 2] = vz;
    }
    const double w = dpp_wave_max(d2);
    if ((threadIdx.x & 63) == 63) atomicMax(dmax + b, (unsigned long long)__double_as_longlong(w));
}

// One lane per molecule: x += dx, scaled where the largest |dx| is beyond maxstep.
__global__ __launch_bounds__(kThreads) void k_quench_move(int n, double maxstep, const double* __restrict__ v, double* __restrict__ x,
                                                          const double* __restrict__ sd, const int* __restrict__ si,
                                                          const unsigned long long* __restrict__ dmax)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (si[kSI * (size_t)b + 2] || i >= n) return;
    const size_t m = 3 * ((size_t)b * n + i);
    fire_move(maxstep, __longlong_as_double((long long)dmax[b]), sd[kSD * (size_t)b], v[m], v[m + 1], v[m + 2], x[m], x[m + 1], x[m + 2]);
}

// ---- small geometry: one wavefront per box, lane i = molecule i ----------------------------------------------------------------
// Up to `nslice` iterations of one box per launch; x, v, F and the scalars are read from scratch at the start and written back
// at the end, so that the next launch goes on where this one ended.  LDS of a box: s [3][64], then the moments [kMom][64].
__global__ __launch_bounds__(kThreads) void k_quench_small(int nb, int n, int nslice, Fire fs, const double* __restrict__ par, double* __restrict__ x,
                                                           double* __restrict__ v, double* __restrict__ F, double* __restrict__ sd, int* __restrict__ si,
                                                           int* __restrict__ nstopped)
{
    __shared__ double lds[kSmallBoxesPerWg][(3 + kMom) * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * kSmallBoxesPerWg + wave;
    if (b >= nb) return;                                   // the whole wavefront; no workgroup barrier below
    int* I = si + kSI * (size_t)b;
    if (I[2]) return;
    double* D = sd + kSD * (size_t)b;
    double* S = lds[wave];
    double* ML = S + 3 * 64;
    const double* H = par + 18 * (size_t)b;
    const CellRegs hc(H), hi(H + 9);
    const bool active = lane < n;
    const size_t m = 3 * ((size_t)b * n + (active ? lane : 0));
    double x0 = active ? x[m] : 0.0, x1 = active ? x[m + 1] : 0.0, x2 = active ? x[m + 2] : 0.0;
    double vx = active ? v[m] : 0.0, vy = active ? v[m + 1] : 0.0, vz = active ? v[m + 2] : 0.0;
    double fx = 0.0, fy = 0.0, fz = 0.0;
    // (the box's scalars and FIRE's parameters too are kept out of the scalar registers, for the same reason as the cell)
    const Fire f = {in_vgpr(fs.dt0), in_vgpr(fs.dtmax), in_vgpr(fs.maxstep), in_vgpr(fs.alpha0), in_vgpr(fs.f_alpha), in_vgpr(fs.f_inc),
                    in_vgpr(fs.f_dec), in_vgpr(fs.n_min), in_vgpr(fs.ftol), fs.max_iter};
    double dt = in_vgpr(D[0]), alpha = in_vgpr(D[1]), E = in_vgpr(D[2]), fmax = in_vgpr(D[3]), E0 = in_vgpr(D[4]), f0 = in_vgpr(D[5]);
    int t = I[0], npos = I[1], conv = 0;
    bool stopped = false;
    for (int it = 0; it < nslice; ++it) {
        const double s0 = frac_coord(hi.c, 0, x0, x1, x2), s1 = frac_coord(hi.c, 1, x0, x1, x2), s2 = frac_coord(hi.c, 2, x0, x1, x2);
        mw::wave_fence();
        S[lane] = s0; S[64 + lane] = s1; S[128 + lane] = s2;
        mw::wave_fence();
        Sums a;
        walk_small(n, active, mw::kRcSq, hc.c, S, s0, s1, s2, [&](int, int, double r2, double dx, double dy, double dz) { a.add(r2, dx, dy, dz); });
        double Mi[kMom];
        a.record(Mi);
#pragma unroll
        for (int k = 0; k < kMom; ++k) ML[64 * k + lane] = Mi[k];
        mw::wave_fence();
        fx = fy = fz = 0.0;
        walk_small(n, active, mw::kRcSq, hc.c, S, s0, s1, s2, [&](int j, int, double r2, double dx, double dy, double dz) {
            if (j == lane) return;                                     // an image of the molecule itself: d is constant
            double Mj[kMom];
#pragma unroll
            for (int k = 0; k < kMom; ++k) Mj[k] = ML[64 * k + j];
            entry_force(Mi, Mj, r2, dx, dy, dz, fx, fy, fz);
        });
        E = in_vgpr(wave_total(active ? a.energy() : 0.0));
        const double P = wave_total(__builtin_fma(fx, vx, __builtin_fma(fy, vy, fz * vz)));
        const double vv = wave_total(__builtin_fma(vx, vx, __builtin_fma(vy, vy, vz * vz)));
        const double FF = wave_total(__builtin_fma(fx, fx, __builtin_fma(fy, fy, fz * fz)));
        const double ax = __builtin_fabs(fx), ay = __builtin_fabs(fy), az = __builtin_fabs(fz);
        fmax = in_vgpr(wave_largest(ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az)));
        if (t == 0) { E0 = E; f0 = fmax; }
        int mix;
        double ca, cb;
        if (fire_decide(f, t, fmax, P, vv, FF, dt, alpha, npos, conv, mix, ca, cb)) { stopped = true; break; }
        const double d2 = fire_velocity(mix, ca, cb, dt, fx, fy, fz, vx, vy, vz);
        fire_move(f.maxstep, wave_largest(d2), dt, vx, vy, vz, x0, x1, x2);
        ++t;
    }
    if (active) {
        x[m] = x0; x[m + 1] = x1; x[m + 2] = x2;
        v[m] = vx; v[m + 1] = vy; v[m + 2] = vz;
        F[m] = fx; F[m + 1] = fy; F[m + 2] = fz;
    }
    if (lane == 0) {
        D[0] = dt; D[1] = alpha; D[2] = E; D[3] = fmax; D[4] = E0; D[5] = f0;
        I[0] = t; I[1] = npos;
        if (stopped) { I[2] = 1; I[3] = conv; atomicAdd(nstopped, 1); }
    }
}

}  // namespace mwquench

namespace {

using namespace mwquench;

constexpr int kEvPerIter = 5;
constexpr int kDefaultLook = 32, kMaxLook = 4096, kDefaultSlice = 64, kMaxSlice = 256;
const double kFireDefaults[8] = MW_QUENCH_FIRE_DEFAULTS;
const char* const kFireNames[8] = {"dt0", "dtmax", "maxstep", "alpha0", "f_alpha", "f_inc", "f_dec", "n_min"};

struct State : Runtime<1> {
    Buf scratch, par, grid, pos, pos_out, forces, stats, iters;
    std::vector<hipEvent_t> pool;                  // kEvPerIter per iteration of a block
    int look = kDefaultLook, slice = kDefaultSlice;
    int last[MW_QUENCH_PLAN_FIELDS] = {0};
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
} g;

// The scratch of one box: the sort's pieces and what the passes keep (general), then what both geometries carry.
struct Layout : SortLayout {
    int nwg = 0;
    size_t mom = 0, en = 0, part = 0, x = 0, v = 0, F = 0, sd = 0, si = 0, dmax = 0, per_box = 0;
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
    l.x = o;    o += align16(24 * (size_t)n);
    l.v = o;    o += align16(24 * (size_t)n);
    l.F = o;    o += align16(24 * (size_t)n);
    l.sd = o;   o += align16(8 * (size_t)kSD);
    l.si = o;   o += align16(4 * (size_t)kSI);
    l.dmax = o; o += 16;
    l.per_box = o;
    return l;
}

struct Plan : PlanBase {
    Layout lay;
};

int make_plan(const char* who, int n, int nboxes, size_t budget, Plan& p)
{
    p.small = n <= kSmallN;
    p.lay = make_layout(n, p.small);
    p.per_box = p.lay.per_box;
    p.lds = p.small ? kSmallLds : kGeneralLds;
    p.boxes_per_wg = p.small ? kSmallBoxesPerWg : 0;
    const size_t fit = budget / p.per_box;
    if (fit < 1)
        return fail("%s: one box needs %zu bytes of scratch (nwater = %d) and does not fit the budget of %zu bytes (MW_QUENCH_SCRATCH_MB)",
                    who, p.per_box, n, budget);
    const size_t most = p.small ? (size_t)kSmallChunkBoxes : (size_t)kMaxChunkBoxes;
    p.bpc = (int)(fit < most ? fit : most);
    if (p.bpc > nboxes) p.bpc = nboxes;
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

int check_counts(const char* who, int nboxes, int n)
{
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    return 0;
}

int check_scalars(const char* who, int nboxes, int n, double ftol, int max_iter, const double* fire, Fire& f)
{
    if (check_counts(who, nboxes, n)) return 1;
    if (!(ftol > 0.0) || !std::isfinite(ftol)) return fail("%s: ftol = %g Hartree / bohr is not a finite number > 0", who, ftol);
    if (max_iter < 0 || max_iter > MW_QUENCH_MAX_ITER) return fail("%s: max_iter = %d outside 0..%d", who, max_iter, MW_QUENCH_MAX_ITER);
    const double* p = fire ? fire : kFireDefaults;
    for (int k = 0; k < 8; ++k)
        if (!(p[k] > 0.0) || !std::isfinite(p[k])) return fail("%s: fire[%d] (%s) = %g is not a finite number > 0", who, k, kFireNames[k], p[k]);
    if (!(p[3] <= 1.0)) return fail("%s: fire[3] (alpha0) = %.17g is beyond 1 (0 < alpha0 <= 1 is required)", who, p[3]);
    if (!(p[4] < 1.0)) return fail("%s: fire[4] (f_alpha) = %.17g is not below 1", who, p[4]);
    if (!(p[5] > 1.0)) return fail("%s: fire[5] (f_inc) = %.17g is not above 1", who, p[5]);
    if (!(p[6] < 1.0)) return fail("%s: fire[6] (f_dec) = %.17g is not below 1", who, p[6]);
    f = Fire{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], ftol, max_iter};
    return 0;
}

const char kRadius[] = "a_sigma";             // the radius the cells are checked against, in the messages

int check_live(const char* who) { return check_live(who, "mw_quench_init", g); }

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

// adds the time between events a and b of the pool to ms[k]
int add_elapsed(int a, int b, float& ms)
{
    float t = 0.0f;
    HIPOK(hipEventElapsedTime(&t, g.pool[a], g.pool[b]));
    ms += t;
    return 0;
}

// The work of both entries, arguments already checked.  par and grid are on the host; pos and the outputs are device pointers
// when `dev`, host pointers otherwise.
int run(const char* who, int nboxes, int n, const std::vector<double>& par, const std::vector<int>& grid, const double* pos, const Fire& f,
        bool dev, double* pos_out, double* forces, double* stats, int* iters)
{
    Plan p;
    if (make_plan(who, n, nboxes, g.budget, p)) return 1;
    const Layout& l = p.lay;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (reserve(g.scratch, p.per_box * (size_t)p.bpc + 16)) return 1;         // (+ the chunk's counter of stopped boxes)
    if (reserve(g.par, par.size() * sizeof(double))) return 1;
    if (reserve(g.grid, grid.size() * sizeof(int))) return 1;
    HIPOK(hipMemcpyAsync(g.par.p, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPOK(hipMemcpyAsync(g.grid.p, grid.data(), grid.size() * sizeof(int), hipMemcpyHostToDevice, g.stream));
    if (!dev) {
        if (reserve(g.pos, 24 * (size_t)n * p.bpc)) return 1;
        if (pos_out && reserve(g.pos_out, 24 * (size_t)n * p.bpc)) return 1;
        if (forces && reserve(g.forces, 24 * (size_t)n * p.bpc)) return 1;
        if (stats && reserve(g.stats, 48 * (size_t)p.bpc)) return 1;
        if (iters && reserve(g.iters, 8 * (size_t)p.bpc)) return 1;
    }
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int evals = f.max_iter + 1;                                      // evaluations after which every box has stopped
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const double* d_pos = pos + 3 * (size_t)n * b0;
        if (!dev) {
            HIPOK(hipMemcpyAsync(g.pos.p, d_pos, 24 * (size_t)n * nb, hipMemcpyHostToDevice, g.stream));
            d_pos = (const double*)g.pos.p;
        }
        const double* d_par = (const double*)g.par.p + 18 * (size_t)b0;
        const int* d_grid = (const int*)g.grid.p + 4 * (size_t)b0;
        double* d_out = !pos_out ? nullptr : dev ? pos_out + 3 * (size_t)n * b0 : (double*)g.pos_out.p;
        double* d_forces = !forces ? nullptr : dev ? forces + 3 * (size_t)n * b0 : (double*)g.forces.p;
        double* d_stats = !stats ? nullptr : dev ? stats + 6 * (size_t)b0 : (double*)g.stats.p;
        int* d_iters = !iters ? nullptr : dev ? iters + 2 * (size_t)b0 : (int*)g.iters.p;
        char* base = (char*)g.scratch.p;
        const size_t B = (size_t)p.bpc;
        double* x = (double*)(base + l.x * B);
        double* v = (double*)(base + l.v * B);
        double* F = (double*)(base + l.F * B);
        double* sd = (double*)(base + l.sd * B);
        int* si = (int*)(base + l.si * B);
        unsigned long long* dmax = (unsigned long long*)(base + l.dmax * B);
        int* nstopped = (int*)(base + p.per_box * B);
        const dim3 grid_m = per_molecule(n, nb);
        HIPOK(hipMemsetAsync(nstopped, 0, sizeof(int), g.stream));
        hipLaunchKernelGGL(k_quench_begin, grid_m, dim3(kThreads), 0, g.stream, n, f, d_pos, x, v, F, sd, si);
        HIPOK(hipGetLastError());
        int done = 0;                                                      // evaluations enqueued so far
        while (done < evals) {
            int used = 0;                                                  // events of this block
            if (p.small) {
                const int launches = g.look / g.slice > 1 ? g.look / g.slice : 1;
                for (int k = 0; k < launches && done < evals; ++k) {
                    const int ns = evals - done < g.slice ? evals - done : g.slice;
                    HIPOK(hipEventRecord(g.pool[used], g.stream));
                    hipLaunchKernelGGL(k_quench_small, dim3((unsigned)((nb + kSmallBoxesPerWg - 1) / kSmallBoxesPerWg)), dim3(kThreads), 0, g.stream,
                                       nb, n, ns, f, d_par, x, v, F, sd, si, nstopped);
                    HIPOK(hipGetLastError());
                    HIPOK(hipEventRecord(g.pool[used + 1], g.stream));
                    used += 2;
                    done += ns;
                }
            } else {
                double* mom = (double*)(base + l.mom * B);
                double* en = (double*)(base + l.en * B);
                double* part = (double*)(base + l.part * B);
                const int blk = evals - done < g.look ? evals - done : g.look;
                for (int k = 0; k < blk; ++k) {
                    Sorted s;
                    HIPOK(hipEventRecord(g.pool[used], g.stream));
                    if (sort_into_cells(g.stream, n, nb, l, base, B, d_par, d_grid, (const double*)x, s)) return 1;
                    HIPOK(hipEventRecord(g.pool[used + 1], g.stream));
                    hipLaunchKernelGGL(k_quench_moments, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, d_par, d_grid, s.start, s.ss, (const int*)si,
                                       mom, en);
                    HIPOK(hipGetLastError());
                    HIPOK(hipEventRecord(g.pool[used + 2], g.stream));
                    hipLaunchKernelGGL(k_quench_forces, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, d_par, d_grid, s.start, s.ss, s.idx,
                                       (const int*)si, (const double*)mom, (const double*)en, (const double*)v, F, part);
                    HIPOK(hipGetLastError());
                    HIPOK(hipEventRecord(g.pool[used + 3], g.stream));
                    hipLaunchKernelGGL(k_quench_decide, dim3((unsigned)nb), dim3(64), 0, g.stream, l.nwg, f, (const double*)part, sd, si, dmax, nstopped);
                    HIPOK(hipGetLastError());
                    hipLaunchKernelGGL(k_quench_step, grid_m, dim3(kThreads), 0, g.stream, n, (const double*)F, v, (const double*)sd, (const int*)si, dmax);
                    HIPOK(hipGetLastError());
                    hipLaunchKernelGGL(k_quench_move, grid_m, dim3(kThreads), 0, g.stream, n, f.maxstep, (const double*)v, x, (const double*)sd,
                                       (const int*)si, (const unsigned long long*)dmax);
                    HIPOK(hipGetLastError());
                    HIPOK(hipEventRecord(g.pool[used + 4], g.stream));
                    used += kEvPerIter;
                }
                done += blk;
            }
            int stopped = 0;                                               // the host's look at the chunk
            HIPOK(hipMemcpyAsync(&stopped, nstopped, sizeof(int), hipMemcpyDeviceToHost, g.stream));
            HIPOK(hipStreamSynchronize(g.stream));
            if (p.small) {
                for (int e = 0; e < used; e += 2)
                    if (add_elapsed(e, e + 1, ms[2])) return 1;
            } else {
                for (int e = 0; e < used; e += kEvPerIter)
                    for (int k = 0; k < 4; ++k)
                        if (add_elapsed(e + k, e + k + 1, ms[k])) return 1;
            }
            if (stopped >= nb) break;
        }
        hipLaunchKernelGGL(k_quench_finish, dim3((unsigned)nb), dim3(kThreads), 0, g.stream, n, d_pos, (const double*)x, (const double*)F,
                           (const double*)sd, (const int*)si, d_out, d_forces, d_stats, d_iters);
        HIPOK(hipGetLastError());
        if (!dev) {
            if (pos_out) HIPOK(hipMemcpyAsync(pos_out + 3 * (size_t)n * b0, g.pos_out.p, 24 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (forces) HIPOK(hipMemcpyAsync(forces + 3 * (size_t)n * b0, g.forces.p, 24 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (stats) HIPOK(hipMemcpyAsync(stats + 6 * (size_t)b0, g.stats.p, 48 * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
            if (iters) HIPOK(hipMemcpyAsync(iters + 2 * (size_t)b0, g.iters.p, 8 * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
        }
        HIPOK(hipStreamSynchronize(g.stream));               // the next chunk reuses the scratch and the staging buffers
    }
    plan_fields(p, grid.data(), g.last);
    g.have_last = true;
    for (int k = 0; k < 4; ++k) g.ms[k] = ms[k];
    return 0;
}

}  // namespace

extern "C" {

const char* mw_quench_last_error(void) { return g_err; }
int mw_quench_is_initialised(void) { return g.live ? 1 : 0; }

int mw_quench_init(int device)
{
    const char* who = "mw_quench_init";
    if (g.live) return fail("%s: already initialised", who);
    int look = kDefaultLook, slice = kDefaultSlice;
    if (env_int(who, "MW_QUENCH_LOOK", 1, kMaxLook, look) || env_int(who, "MW_QUENCH_SLICE", 1, kMaxSlice, slice)) return 1;
    if (runtime_init(who, "MW_QUENCH_SCRATCH_MB", device, g)) return 1;
    g.look = look;
    g.slice = slice;
    DeviceScope scope;
    hipError_t e = scope.enter(g.device);
    g.pool.assign((size_t)kEvPerIter * look, nullptr);
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

int mw_quench_finalize(void)
{
    if (g.live) {
        DeviceScope scope;
        HIPOK(scope.enter(g.device));
        HIPOK(hipStreamSynchronize(g.stream));
        for (auto& ev : g.pool) HIPOK(hipEventDestroy(ev));
        g.pool.clear();
    }
    if (runtime_finalize(g, {&g.scratch, &g.par, &g.grid, &g.pos, &g.pos_out, &g.forces, &g.stats, &g.iters})) return 1;
    g = State{};
    return 0;
}

int mw_quench_compute(int nboxes, int nwater, const double* cells, const double* pos, double ftol, int max_iter, const double* fire,
                      double* pos_out, double* forces, double* stats, int* iters)
{
    const char* who = "mw_quench_compute";
    std::vector<double> par;
    std::vector<int> grid;
    Fire f;
    if (check_scalars(who, nboxes, nwater, ftol, max_iter, fire, f)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (check_cells(who, kRadius, nboxes, nwater, cells, mw::kSigA, par, grid)) return 1;
    if (check_live(who)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, f, false, pos_out, forces, stats, iters);
}

int mw_quench_compute_device(int nboxes, int nwater, const double* cells, const double* pos, double ftol, int max_iter, const double* fire,
                             double* pos_out, double* forces, double* stats, int* iters)
{
    const char* who = "mw_quench_compute_device";
    std::vector<double> par;
    std::vector<int> grid;
    Fire f;
    if (check_scalars(who, nboxes, nwater, ftol, max_iter, fire, f)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (fetch_cells(who, kRadius, nboxes, nwater, cells, mw::kSigA, par, grid)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, f, true, pos_out, forces, stats, iters);
}

int mw_quench_plan(int nwater, const double* cell, int nboxes, int* out, int nout)
{
    const char* who = "mw_quench_plan";
    std::vector<int> grid;
    if (check_counts(who, nboxes, nwater)) return 1;
    if (plan_grid(who, kRadius, nwater, cell, mw::kSigA, out, nout, grid)) return 1;
    Plan p;
    if (make_plan(who, nwater, nboxes, g.live ? g.budget : kDefaultBudget, p)) return 1;
    int f[MW_QUENCH_PLAN_FIELDS];
    plan_fields(p, grid.data(), f);
    copy_fields(f, MW_QUENCH_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_quench_last(int* out, int nout) { return last_fields("mw_quench_last", "mw_quench_init", g, g.last, MW_QUENCH_PLAN_FIELDS, out, nout); }

int mw_quench_elapsed_ms(float* sort, float* moments, float* forces, float* step)
{
    if (check_live("mw_quench_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_quench_elapsed_ms: no call has launched yet");
    if (sort) *sort = g.ms[0];
    if (moments) *moments = g.ms[1];
    if (forces) *forces = g.ms[2];
    if (step) *step = g.ms[3];
    return 0;
}

}  // extern "C"
