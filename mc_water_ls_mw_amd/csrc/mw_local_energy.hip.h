// mw_local_energy.hip.h -- gfx950 (MI355X, CDNA4) device code of the mW energy engine:
// compute_local_real_energy (molint.F90:220-404), one evaluation at a time: local_energy_wave and its latency-ordered twin
// local_energy_wave_batched.
#pragma once

#include "mw_common.hip.h"

namespace mw {

// =====================================================================================
// Local energy of one molecule = every pair and every triplet it takes part in
// (as centre or as end), the building block of a single-move Delta E.
// One 64-wide wavefront per request; lane l owns slot l of a neighbour list
// (maxneigh <= 64).  Pass 0: the lanes hold imol's own list and evaluate the pair
// term and g for the in-range lanes.  Then for every in-range j (a wave-uniform
// loop over the ballot mask):
//   * j--i--k triplets: lanes above j that are in range combine with j's
//     broadcast vector (molint.F90:302-318: the remaining entries of imol's list);
//   * i--j--k triplets: the lanes re-load jmol's list, shifted by j's image
//     (molint.F90:324-343), and each evaluates its k.
// A slot whose cos(theta) >= 0.99 contributes 0 (molint.F90:367-371; this is how
// the k == i self term drops out) and so does an out-of-range slot (G2).
//
// A request may carry up to two position overrides {index, xyz}: the molecule
// itself at a trial position, and (single-call drop-in path) the previously
// queried molecule whose host copy may have been reverted.  Overrides are used
// from registers wherever that index is gathered; with `commit` they are also
// written to the mirrored positions for later launches.
// =====================================================================================
struct Override { int idx; double x, y, z; };   // idx < 0: none (0-based molecule index)

// COHERENT = true (the resident server below): positions are read past the CU's vector L1 (agent scope, served by
// L2), because the server itself rewrites single positions between requests while its wavefront lives on.
template <bool COHERENT = false>
__device__ __forceinline__ void load_pos(const double* __restrict__ P, int j, const Override& o1, const Override& o2,
                                         double& x, double& y, double& z)
{
    const double* p = P + 3 * (size_t)j;
    if constexpr (COHERENT) {
        x = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        y = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        z = __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        x = p[0]; y = p[1]; z = p[2];
    }
    if (j == o1.idx) { x = o1.x; y = o1.y; z = o1.z; }
    if (j == o2.idx) { x = o2.x; y = o2.y; z = o2.z; }
}

// Returns the local energy in every lane.  `ninter` / `nslots` (wave-uniform) receive the number
// of in-range interactions as the reference enumerates them (pairs + triplet slots with
// cos(theta) < 0.99) and the number of list slots visited (n_i + sum of n_j over in-range j),
// which prices the call's algorithmic bytes.
template <bool COHERENT = false>
__device__ __forceinline__ double local_energy_wave(const double* __restrict__ P, const double* __restrict__ IV,
                                                    const uint32_t* __restrict__ LM, const int* __restrict__ NN,
                                                    int i, const Override& o1, const Override& o2, int lane,
                                                    unsigned int& ninter, unsigned int& nslots)
{
    double xi, yi, zi;
    load_pos<COHERENT>(P, i, o1, o2, xi, yi, zi);                         // molint.F90:258
    const int n_i = NN[i];

    // pass 0: imol's own list, one slot per lane
    const bool has = lane < n_i;
    const uint32_t e = has ? LM[(size_t)i * kRow + lane] : 0u;
    const int j = (int)(e & kJMask), kimg = (int)(e >> kJBits);
    double xj, yj, zj;
    load_pos<COHERENT>(P, j, o1, o2, xj, yj, zj);
    const double jvx = IV[3 * kimg], jvy = IV[3 * kimg + 1], jvz = IV[3 * kimg + 2];
    const double qx = xj + jvx, qy = yj + jvy, qz = zj + jvz;             // :269 position of j's image
    const double dx = qx - xi, dy = qy - yi, dz = qz - zi;                // :272
    const double r2 = dx * dx + dy * dy + dz * dz;                        // :273
    const bool inr = has && (r2 < kRcSq);                                 // :276
    double rinv = 0.0, e1 = 0.0, g = 0.0;
    if (inr) pair_terms(r2, rinv, e1, g);
    const double q = kSigSq * rinv * rinv;
    double acc2 = inr ? (kAeps * (kBigB * (q * q) - 1.0)) * e1 : 0.0;     // :294-297
    double acc3 = 0.0;
    unsigned int ntl = 0;            // per-lane count of triplet slots that contribute

    unsigned long long mask = __ballot(inr);
    ninter = (unsigned int)__popcll(mask);
    nslots = (unsigned int)n_i;
    while (mask) {                                                        // wave-uniform loop over in-range j
        const int jl = __ffsll((long long)mask) - 1;
        mask &= mask - 1ull;
        const double ajx = readlane_f64(dx, jl), ajy = readlane_f64(dy, jl), ajz = readlane_f64(dz, jl);   // jl is wave-uniform
        const double rinv_j = readlane_f64(rinv, jl), g_j = readlane_f64(g, jl);

        // j--i--k: later in-range slots of imol's own list                 :302-318
        if (inr && lane > jl) {
            const double ct = ((ajx * dx + ajy * dy + ajz * dz) * rinv_j) * rinv;     // :316,365
            if (ct < 0.99) { const double d = ct - kCos0; acc3 += g_j * (g * (d * d)); ++ntl; }   // :367-368,385-387
        }

        // i--j--k: jmol's list, translated by j's image                    :324-343
        const int jj = __builtin_amdgcn_readlane(j, jl);
        const double sjx = readlane_f64(jvx, jl), sjy = readlane_f64(jvy, jl), sjz = readlane_f64(jvz, jl);
        const double pjx = readlane_f64(qx, jl), pjy = readlane_f64(qy, jl), pjz = readlane_f64(qz, jl);
        const int n_j = NN[jj];
        nslots += (unsigned int)n_j;
        if (lane < n_j) {
            const uint32_t e2 = LM[(size_t)jj * kRow + lane];
            const int kk = (int)(e2 & kJMask), k2 = (int)(e2 >> kJBits);
            double xk, yk, zk;
            load_pos<COHERENT>(P, kk, o1, o2, xk, yk, zk);
            const double bx = ((xk + IV[3 * k2]) + sjx) - pjx;            // :332,334
            const double by = ((yk + IV[3 * k2 + 1]) + sjy) - pjy;
            const double bz = ((zk + IV[3 * k2 + 2]) + sjz) - pjz;
            const double s2 = bx * bx + by * by + bz * bz;                // :335
            if (s2 < kRcSq) {                                             // :361
                double rinv_k, e1_k, g_k;
                pair_terms(s2, rinv_k, e1_k, g_k);
                const double ct = (-(ajx * bx + ajy * by + ajz * bz) * rinv_j) * rinv_k;   // :320,341,365
                if (ct < 0.99) { const double d = ct - kCos0; acc3 += g_j * (g_k * (d * d)); ++ntl; }
            }
        }
    }
    const double tot = readlane_f64(dpp_wave_sum(acc2 + kLamEps * acc3), 63);                       // :397
    ninter += (unsigned int)__builtin_amdgcn_readlane(dpp_wave_sum_i32((int)ntl), 63);
    return tot;
}

// The same evaluation laid out for LATENCY (the resident server of the drop-in single call): the rows and third-body
// positions of up to eight in-range neighbours are requested together, so the whole call is four dependent memory
// round trips (row of imol -> positions of its entries -> rows of the in-range j -> positions of their entries)
// instead of three per in-range neighbour.  Same terms, same per-term arithmetic as local_energy_wave.
template <bool COHERENT>
__device__ __forceinline__ double local_energy_wave_batched(const double* __restrict__ P, const double* __restrict__ IV,
                                                            const uint32_t* __restrict__ LM, const int* __restrict__ NN,
                                                            int i, const Override& o1, const Override& o2, int lane,
                                                            unsigned int& ninter, unsigned int& nslots)
{
    constexpr int B = 8;
    double xi, yi, zi;
    load_pos<COHERENT>(P, i, o1, o2, xi, yi, zi);                         // molint.F90:258
    const int n_i = NN[i];
    const uint32_t e = LM[(size_t)i * kRow + lane];                       // rows are 64 entries long in memory: no need to wait for n_i
    const bool has = lane < n_i;
    const int j = has ? (int)(e & kJMask) : 0, kimg = has ? (int)(e >> kJBits) : 0;
    double xj, yj, zj;
    load_pos<COHERENT>(P, j, o1, o2, xj, yj, zj);
    const double jvx = IV[3 * kimg], jvy = IV[3 * kimg + 1], jvz = IV[3 * kimg + 2];
    const double qx = xj + jvx, qy = yj + jvy, qz = zj + jvz;             // :269
    const double dx = qx - xi, dy = qy - yi, dz = qz - zi;                // :272
    const double r2 = dx * dx + dy * dy + dz * dz;                        // :273
    const bool inr = has && (r2 < kRcSq);                                 // :276
    double rinv = 0.0, e1 = 0.0, g = 0.0;
    if (inr) pair_terms(r2, rinv, e1, g);
    const double q = kSigSq * rinv * rinv;
    double acc2 = inr ? (kAeps * (kBigB * (q * q) - 1.0)) * e1 : 0.0;     // :294-297
    double acc3 = 0.0;
    unsigned int ntl = 0;

    unsigned long long mask = __ballot(inr);
    ninter = (unsigned int)__popcll(mask);
    nslots = (unsigned int)n_i;
    while (mask) {                                                        // wave-uniform: batches of B in-range j
        // straight-line code, no branches between the loads: a batch shorter than B repeats its last neighbour
        // (harmless duplicate loads) so that every load of a stage is in flight before the first one is waited for
        int jls[B], jjs[B], njs[B];
        uint32_t e2s[B];
        const int left = __popcll(mask);
        const int cb = left < B ? left : B;
        int jlast = 0;
#pragma unroll
        for (int r = 0; r < B; ++r) {
            const int jl = mask ? __ffsll((long long)mask) - 1 : jlast;
            mask = mask ? (mask & (mask - 1ull)) : 0ull;
            jls[r] = jl; jlast = jl;
            jjs[r] = __builtin_amdgcn_readlane(j, jl);
        }
#pragma unroll
        for (int r = 0; r < B; ++r) { njs[r] = NN[jjs[r]]; e2s[r] = LM[(size_t)jjs[r] * kRow + lane]; }
        double xk[B], yk[B], zk[B], kx[B], ky[B], kz[B];
#pragma unroll
        for (int r = 0; r < B; ++r) {                                     // (stale slots past a row's end hold valid old entries)
            const int kk = (int)(e2s[r] & kJMask), k2 = (int)(e2s[r] >> kJBits);
            load_pos<COHERENT>(P, kk, o1, o2, xk[r], yk[r], zk[r]);
            kx[r] = IV[3 * k2]; ky[r] = IV[3 * k2 + 1]; kz[r] = IV[3 * k2 + 2];
        }
#pragma unroll
        for (int r = 0; r < B; ++r) {
            if (r < cb) {
                const int jl = jls[r];
                const double ajx = readlane_f64(dx, jl), ajy = readlane_f64(dy, jl), ajz = readlane_f64(dz, jl);
                const double rinv_j = readlane_f64(rinv, jl), g_j = readlane_f64(g, jl);
                if (inr && lane > jl) {                                               // j--i--k  :302-318
                    const double ct = ((ajx * dx + ajy * dy + ajz * dz) * rinv_j) * rinv;
                    if (ct < 0.99) { const double d = ct - kCos0; acc3 += g_j * (g * (d * d)); ++ntl; }
                }
                const double sjx = readlane_f64(jvx, jl), sjy = readlane_f64(jvy, jl), sjz = readlane_f64(jvz, jl);
                const double pjx = readlane_f64(qx, jl), pjy = readlane_f64(qy, jl), pjz = readlane_f64(qz, jl);
                nslots += (unsigned int)njs[r];
                if (lane < njs[r]) {                                                  // i--j--k  :324-343
                    const double bx = ((xk[r] + kx[r]) + sjx) - pjx;
                    const double by = ((yk[r] + ky[r]) + sjy) - pjy;
                    const double bz = ((zk[r] + kz[r]) + sjz) - pjz;
                    const double s2 = bx * bx + by * by + bz * bz;
                    if (s2 < kRcSq) {
                        double rinv_k, e1_k, g_k;
                        pair_terms(s2, rinv_k, e1_k, g_k);
                        const double ct = (-(ajx * bx + ajy * by + ajz * bz) * rinv_j) * rinv_k;
                        if (ct < 0.99) { const double d = ct - kCos0; acc3 += g_j * (g_k * (d * d)); ++ntl; }
                    }
                }
            }
        }
    }
    const double tot = readlane_f64(dpp_wave_sum(acc2 + kLamEps * acc3), 63);                       // :397
    ninter += (unsigned int)__builtin_amdgcn_readlane(dpp_wave_sum_i32((int)ntl), 63);
    return tot;
}

}  // namespace mw
