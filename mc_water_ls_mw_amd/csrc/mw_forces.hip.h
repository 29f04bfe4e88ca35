// mw_forces.hip.h -- gfx950 (MI355X, CDNA4) device code of the mW energy engine: the gradient of the full-box energy.
// k_model_forces (per-molecule forces and per-workgroup virial partials), k_sum_virial.  The reference has no forces;
// this is the derivative of what k_model_energy evaluates (DESIGN.md "Forces and virial").
#pragma once

#include "mw_common.hip.h"
#include "mw_full_energy.hip.h"

namespace mw {

// =====================================================================================
// Forces and virial from the moments.
//
// For molecule i and each in-range entry k of its list (d_k = r_j + ivect_k - r_i, r_k = |d_k|, u_k = d_k / r_k,
// D_k = r_k - a sigma, g_k = exp(gamma sigma / D_k), g'_k = -gamma sigma g_k / D_k^2) and i's moments S0, S1, S2 (d_mom,
// written by k_model_energy from the same positions in the same call):
//   P_k = u_k^T S2 u_k - 2 c0 u_k.S1 + c0^2 S0 - g_k (1 - c0)^2                          dT_i / dg_k
//   t_k = P_k g'_k u_k + (I - u_k u_k^T) 2 g_k (S2 u_k - c0 S1) / r_k                     dT_i / dd_k
// and F_i = sum_k phi'(r_k) u_k + lambda eps sum_k t_k - lambda eps sum_k t'_k, where t'_k is t_k evaluated with the moments
// of j_k and d' = -d_k (i as an arm of the triplets centred on j_k).  An entry with j_k = i (an image of i itself) has a
// constant d_k: no force, but it enters i's moments and the virial
//   W = -1/2 sum_i sum_k phi'(r_k) u_k (x) d_k - lambda eps sum_i sum_k t_k (x) d_k.
//
// One molecule per lane over the slot-major list (column t belongs to molecule order[t], as in k_model_energy); no atomics:
// every force is one lane's sum in list order, the virial one fixed DPP tree per wavefront, the wavefronts of a workgroup in
// order, the workgroups of a box in order (k_sum_virial).  The launch geometry of a box depends on N only, so the results
// are the same bits whatever else shares the launch.
//
// LDSPOS = true : one workgroup per box stages the box's positions in LDS (N*24 B) and walks all its columns.
// LDSPOS = false: positions gathered from global memory (L2-resident), one column per thread, ceil(N / BLOCK) workgroups.
// grid = (nsplit, boxes in the launch); the image vectors are staged in LDS either way.
// =====================================================================================
constexpr int kVirialStride = 9;   // doubles per workgroup partial and per box: W column-major (W_ab at [a + 3 b])

// phi'(r) and g'(r) of an in-range pair next to pair_terms' e1 and g.  Past the kDenClamp clamp e1 = g = 0 and 1/D stays finite
// (|1/D| <= 1/1.2e-3), so both derivatives come out as exactly 0.
__device__ __forceinline__ void pair_derivs(double r2, double rinv, double e1, double g, double& dphi, double& dg)
{
    const double w = fast_rcp(__builtin_fmin(fma_sc(r2, rinv, -kSigA), kDenClamp));   // 1 / (r - a sigma), clamped as in pair_terms
    const double w2 = w * w;
    const double ri2 = rinv * rinv, ri4 = ri2 * ri2;
    // phi = A eps (B sigma^4 r^-4 - 1) e1,  e1 = exp(sigma / D):  phi' = -e1 [4 A eps B sigma^4 r^-5 + A eps (B sigma^4 r^-4 - 1) sigma / D^2]
    dphi = -e1 * __builtin_fma(4.0 * kAepsBSig4 * ri4, rinv, fma_sc(ri4, kAepsBSig4, -kAeps) * (kSigma * w2));
    dg = -kGamSig * g * w2;
}

// t = P g' u + 2 g (v - (u.v) u) / r with v = S2 u + s c0 S1 and P = u^T S2 u + 2 s c0 u.S1 + c0^2 S0 - g (1 - c0)^2: s = -1 is
// dT / dd of the molecule's own triplets (the centre), s = +1 with the sign of the result flipped is a neighbour's, seen from the
// arm (d' = -d, u' = -u).
struct Moments {
    double S0, S1x, S1y, S1z, Sxx, Syy, Sxy, Sxz, Syz, Szz;
    __device__ __forceinline__ void load(const double* __restrict__ m)
    {
        double M[10];
        load_moments(m, M);
        S0 = M[0]; S1x = M[1]; S1y = M[2]; S1z = M[3]; Sxx = M[4]; Syy = M[5]; Sxy = M[6]; Sxz = M[7]; Syz = M[8];
        Szz = S0 - Sxx - Syy;                        // the u_k are unit vectors (mw_common.hip.h, kMomStride)
    }
    template <int SIGN>
    __device__ __forceinline__ void grad(double ux, double uy, double uz, double rinv, double g, double dg,
                                         double& tx, double& ty, double& tz) const
    {
        constexpr double sc = SIGN * kCos0;
        const double ax = Sxx * ux + Sxy * uy + Sxz * uz;
        const double ay = Sxy * ux + Syy * uy + Syz * uz;
        const double az = Sxz * ux + Syz * uy + Szz * uz;
        const double uS1 = S1x * ux + S1y * uy + S1z * uz;
        const double P = (ux * ax + uy * ay + uz * az) + 2.0 * sc * uS1 + kCos0 * kCos0 * S0 - g * ((1.0 - kCos0) * (1.0 - kCos0));
        const double vx = ax + sc * S1x, vy = ay + sc * S1y, vz = az + sc * S1z;
        const double uv = ux * vx + uy * vy + uz * vz;
        const double c = 2.0 * g * rinv, p = P * dg;
        tx = p * ux + c * (vx - uv * ux);
        ty = p * uy + c * (vy - uv * uy);
        tz = p * uz + c * (vz - uv * uz);
    }
};

template <bool LDSPOS, int BLOCK, int LAYOUT>
__global__ __launch_bounds__(BLOCK)
void k_model_forces(const double* __restrict__ pos, const double* __restrict__ ivect, const int* __restrict__ nivect,
                    const uint32_t* __restrict__ list, const int* __restrict__ order, const int* __restrict__ nns,
                    const double* __restrict__ mom,   // [box][N][kMomStride], this call's moments
                    double* __restrict__ force,       // [box][N][3], molecule order
                    double* __restrict__ wpart,       // [box][nsplit][kVirialStride]
                    int N, int S, int ivcap, int box0)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double wred[BLOCK / 64][kVirialStride];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int split = blockIdx.x, nsplit = gridDim.x;
    const int b = box0 + (int)blockIdx.y;
    const double* P = pos + (size_t)b * N * 3;
    const double* IV = ivect + (size_t)b * ivcap * 3;
    const int niv = nivect[b];

    double* spos = smem;
    double* siv = smem + (LDSPOS ? lds_vec_bytes((size_t)N) / 8 : 0);
    const double iv_first = stage_iv_begin<BLOCK>(IV, niv, tid);
    if constexpr (LDSPOS) stage_vecs<LAYOUT, BLOCK>(spos, P, N, N, tid);
    stage_iv_end<LAYOUT, BLOCK>(siv, IV, niv, ivcap, tid, iv_first);
    __syncthreads();

    const LdsVecs<LAYOUT> vpos{spos, N}, viv{siv, ivcap};
    auto getpos = [&](int j, double& x, double& y, double& z) {
        if constexpr (LDSPOS) vpos.get(j, x, y, z);
        else { const double* p = P + 3 * (size_t)j; x = p[0]; y = p[1]; z = p[2]; }
    };
    const uint32_t* L = list + (size_t)b * S * N;
    const double* M = mom + (size_t)b * N * kMomStride;

    double W[kVirialStride];
#pragma unroll
    for (int c = 0; c < kVirialStride; ++c) W[c] = 0.0;

    for (int t = split * BLOCK + tid; t < N; t += nsplit * BLOCK) {
        const int mol = order[(size_t)b * N + t];
        const int n = nns[(size_t)b * N + t] & 0xff;
        double xi, yi, zi;
        getpos(mol, xi, yi, zi);
        Moments mi;
        mi.load(M + (size_t)mol * kMomStride);
        double fx = 0.0, fy = 0.0, fz = 0.0;
        for (int s = 0; s < n; ++s) {
            const uint32_t e = L[(size_t)s * N + t];
            const int j = (int)(e & kJMask);
            double xj, yj, zj, ix, iy, iz;
            getpos(j, xj, yj, zj);
            viv.get((int)(e >> kJBits), ix, iy, iz);
            const double dx = (xj + ix) - xi, dy = (yj + iy) - yi, dz = (zj + iz) - zi;   // molint.F90:447,450
            const double r2 = dist2(dx, dy, dz);
            if (!(r2 < kRcSq)) continue;                                                 // :454
            double rinv, e1, g, dphi, dg;
            pair_terms(r2, rinv, e1, g);
            pair_derivs(r2, rinv, e1, g, dphi, dg);
            const double ux = dx * rinv, uy = dy * rinv, uz = dz * rinv;
            double tx, ty, tz;
            mi.grad<-1>(ux, uy, uz, rinv, g, dg, tx, ty, tz);
            // virial: -1/2 phi' u (x) d - lambda eps t (x) d   (self-image entries included)
            const double ax = -0.5 * dphi * ux - kLamEps * tx;
            const double ay = -0.5 * dphi * uy - kLamEps * ty;
            const double az = -0.5 * dphi * uz - kLamEps * tz;
            W[0] += ax * dx; W[1] += ay * dx; W[2] += az * dx;
            W[3] += ax * dy; W[4] += ay * dy; W[5] += az * dy;
            W[6] += ax * dz; W[7] += ay * dz; W[8] += az * dz;
            if (j == mol) continue;                                                      // an image of i itself: d is constant
            Moments mj;
            mj.load(M + (size_t)j * kMomStride);
            double sx, sy, sz;
            mj.grad<1>(ux, uy, uz, rinv, g, dg, sx, sy, sz);                             // -t'_k
            fx += dphi * ux + kLamEps * (tx + sx);
            fy += dphi * uy + kLamEps * (ty + sy);
            fz += dphi * uz + kLamEps * (tz + sz);
        }
        double* fo = force + ((size_t)b * N + mol) * 3;
        fo[0] = fx; fo[1] = fy; fo[2] = fz;
    }

#pragma unroll
    for (int c = 0; c < kVirialStride; ++c) {
        const double v = dpp_wave_sum(W[c]);            // fixed tree; total in lane 63
        if (lane == 63) wred[wid][c] = v;
    }
    __syncthreads();
    if (tid < kVirialStride) {
        double v = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) v += wred[w][tid];
        wpart[((size_t)b * nsplit + split) * kVirialStride + tid] = v;
    }
}

// The virial of each box: its workgroups' partials added in split order (one thread per component).
__global__ __launch_bounds__(64)
void k_sum_virial(const double* __restrict__ wpart, double* __restrict__ virial, int box0, int count, int nsplit)
{
    const int b = box0 + (int)blockIdx.x, c = threadIdx.x;
    if ((int)blockIdx.x >= count || c >= kVirialStride) return;
    double v = 0.0;
    for (int s = 0; s < nsplit; ++s) v += wpart[((size_t)b * nsplit + s) * kVirialStride + c];
    virial[(size_t)b * kVirialStride + c] = v;
}

}  // namespace mw
