// mw_ice.hip.h -- gfx950 (MI355X, CDNA4) device code of the mW energy engine: per-molecule ice structure classes (CHILL+,
// Nguyen & Molinero, J. Phys. Chem. B 119, 9369 (2015)).  k_ice_q (bond-order vectors), k_ice_class (classes and per-box
// counts), k_ice_bonds (every list entry's bond value, the arithmetic check).  The reference has no counterpart: it can only
// write DCD frames for offline analysis (DESIGN.md "Ice structure classes").
#pragma once

#include "mw_common.hip.h"
#include "mw_full_energy.hip.h"

namespace mw {

// =====================================================================================
// CHILL+ from the Verlet list.
//
// Neighbours of i: every list entry k (j_k, image_k) with 0 < |d_k| < r_c, d_k = r_j + ivect_k - r_i (images of i itself and
// several images of one j count separately); n_i of them.  q_i = sum_k Y3(u_k), u_k = d_k / |d_k|, with the seven real l = 3
// spherical harmonics (Y3(a).Y3(b) = 7 / (4 pi) P3(a.b)).  A bond's value is c_ik = q_i.q_j / (|q_i| |q_j|): NaN where
// |q|^2 <= 1e-24 n^2 for i or j (degenerate, e.g. two antipodal neighbours), exactly 1 for an image of i itself.
// Staggered: c <= -0.8, eclipsed: -0.35 <= c <= 0.25.  Class (uint8), tested in this order: n_i != 4 -> 0 (other); 4 staggered
// -> 1 (cubic ice); 3 staggered + 1 eclipsed -> 2 (hexagonal ice); 4 eclipsed -> 4 (clathrate); 3 eclipsed -> 5 (interfacial
// clathrate); >= 2 staggered -> 3 (interfacial ice); else 0.
//
// k_ice_q (pass 1): one molecule per lane over the slot-major list (column t belongs to molecule order[t], as in
// k_model_energy) writes q^_i (kIceQStride doubles: the normalised q_i, then 1 where it is valid and 0 where degenerate, all
// zero then), n_i and the j of i's first four neighbour entries -- a molecule with n_i != 4 is class 0 whatever its bonds are.
// LDSPOS = true : one workgroup per box stages the box's positions in LDS (N*24 B) and walks all its columns.
// LDSPOS = false: positions gathered from global memory (L2-resident), one column per thread, ceil(N / BLOCK) workgroups.
// The image vectors are staged in LDS either way.
// k_ice_class (pass 2): one molecule per lane in molecule order gathers the q^ of its four neighbours and writes its class;
// each wavefront counts its classes by ballot, the workgroup adds them in LDS and then to the box's six counts (integer
// atomics: exact in any order).
// Nothing else is written: not the moments, not the positions, the lists or the energies.
// =====================================================================================
constexpr int kIceQStride = 8;            // doubles per molecule of q^: 7 components + the validity flag (64 B, 4 x b128)
constexpr int kIceClasses = 6;
constexpr int kIceBatch = 8;              // list entries a lane of k_ice_q loads before it uses the first
constexpr double kIceStaggered = -0.8, kIceEclLo = -0.35, kIceEclHi = 0.25;

// Y3(u) for a unit vector, the common factor 1 / (4 sqrt(pi)) included (the orthonormal real harmonics)
__device__ __forceinline__ void ice_y3_add(double x, double y, double z, double* q)
{
    constexpr double kF = 0.14104739588693907;                    // 1 / (4 sqrt(pi))
    constexpr double c0 = 4.183300132670378 * kF;                  // sqrt(35/2)
    constexpr double c1 = 20.493901531919196 * kF;                 // 2 sqrt(105)
    constexpr double c2 = 3.24037034920393 * kF;                   // sqrt(21/2)
    constexpr double c3 = 2.6457513110645907 * kF;                 // sqrt(7)
    constexpr double c5 = 10.246950765959598 * kF;                 // sqrt(105)
    const double x2 = x * x, y2 = y * y, z2 = z * z;
    const double f = 5.0 * z2 - 1.0;
    q[0] += c0 * y * (3.0 * x2 - y2);
    q[1] += c1 * x * y * z;
    q[2] += c2 * y * f;
    q[3] += c3 * z * (5.0 * z2 - 3.0);
    q[4] += c2 * x * f;
    q[5] += c5 * z * (x2 - y2);
    q[6] += c0 * x * (x2 - 3.0 * y2);
}

struct IceQ {
    double v[kIceQStride];
    __device__ __forceinline__ void load(const double* __restrict__ p)
    {
        const double2* p2 = reinterpret_cast<const double2*>(p);
#pragma unroll
        for (int c = 0; c < kIceQStride / 2; ++c) { const double2 a = p2[c]; v[2 * c] = a.x; v[2 * c + 1] = a.y; }
    }
};

// c of a bond between i and j (self: j is an image of i)
__device__ __forceinline__ double ice_bond_value(const IceQ& qi, const IceQ& qj, bool self)
{
    if (qi.v[7] == 0.0 || qj.v[7] == 0.0) return __builtin_nan("");
    if (self) return 1.0;
    double c = 0.0;
#pragma unroll
    for (int m = 0; m < 7; ++m) c = __builtin_fma(qi.v[m], qj.v[m], c);
    return c;
}

__device__ __forceinline__ int ice_class_of(int nst, int necl)
{
    if (nst == 4) return 1;
    if (nst == 3 && necl == 1) return 2;
    if (necl == 4) return 4;
    if (necl == 3) return 5;
    if (nst >= 2) return 3;
    return 0;
}

template <bool LDSPOS, int BLOCK, int LAYOUT>
__global__ __launch_bounds__(BLOCK)
void k_ice_q(const double* __restrict__ pos, const double* __restrict__ ivect, const int* __restrict__ nivect,
             const uint32_t* __restrict__ list, const int* __restrict__ order, const int* __restrict__ nns,
             double rc2,
             double* __restrict__ qhat,        // [box][N][kIceQStride], molecule order
             int4* __restrict__ nbr,           // [box][N]: j (0-based) of the first four neighbour entries, -1 past n_i
             int* __restrict__ nin,            // [box][N]: n_i
             int* __restrict__ counts,         // [box][kIceClasses]: zeroed here for k_ice_class
             int N, int S, int ivcap, int box0)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x;
    const int split = blockIdx.x, nsplit = gridDim.x;
    const int b = box0 + (int)blockIdx.y;
    const double* P = pos + (size_t)b * N * 3;
    const double* IV = ivect + (size_t)b * ivcap * 3;
    const int niv = nivect[b];
    if (split == 0 && tid < kIceClasses) counts[(size_t)b * kIceClasses + tid] = 0;

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

    for (int t = split * BLOCK + tid; t < N; t += nsplit * BLOCK) {
        const int mol = order[(size_t)b * N + t];
        const int n = nns[(size_t)b * N + t] & 0xff;
        double xi, yi, zi;
        getpos(mol, xi, yi, zi);
        double q[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int cnt = 0;
        int nb[4] = {-1, -1, -1, -1};
        for (int s0 = 0; s0 < n; s0 += kIceBatch) {
            uint32_t ev[kIceBatch];                                    // a batch of entries in flight at once, not one
                                                                       // list round trip per entry
#pragma unroll
            for (int u = 0; u < kIceBatch; ++u) ev[u] = s0 + u < n ? L[(size_t)(s0 + u) * N + t] : 0u;
#pragma unroll
            for (int u = 0; u < kIceBatch; ++u) {
                if (s0 + u >= n) break;
                const int j = (int)(ev[u] & kJMask);
                double xj, yj, zj, ix, iy, iz;
                getpos(j, xj, yj, zj);
                viv.get((int)(ev[u] >> kJBits), ix, iy, iz);
                const double dx = (xj + ix) - xi, dy = (yj + iy) - yi, dz = (zj + iz) - zi;   // as the energy kernels form d
                const double r2 = dist2(dx, dy, dz);
                if (!(r2 < rc2 && r2 > 0.0)) continue;
                const double rinv = fast_rsqrt(r2);
                ice_y3_add(dx * rinv, dy * rinv, dz * rinv, q);
                if (cnt < 4) nb[cnt] = j;
                ++cnt;
            }
        }
        double q2 = 0.0;
#pragma unroll
        for (int m = 0; m < 7; ++m) q2 = __builtin_fma(q[m], q[m], q2);
        const bool valid = q2 > 1e-24 * (double)cnt * (double)cnt;
        const double sc = valid ? fast_rsqrt(q2) : 0.0;
        double2* qo = reinterpret_cast<double2*>(qhat + ((size_t)b * N + mol) * kIceQStride);
        qo[0] = make_double2(q[0] * sc, q[1] * sc);
        qo[1] = make_double2(q[2] * sc, q[3] * sc);
        qo[2] = make_double2(q[4] * sc, q[5] * sc);
        qo[3] = make_double2(q[6] * sc, valid ? 1.0 : 0.0);
        nbr[(size_t)b * N + mol] = make_int4(nb[0], nb[1], nb[2], nb[3]);
        nin[(size_t)b * N + mol] = cnt;
    }
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK)
void k_ice_class(const double* __restrict__ qhat, const int4* __restrict__ nbr, const int* __restrict__ nin,
                 uint8_t* __restrict__ cls,        // [box][N], molecule order
                 int* __restrict__ counts,         // [box][kIceClasses], zeroed by k_ice_q
                 int N, int box0)
{
    __shared__ int wcount[kIceClasses];
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = box0 + (int)blockIdx.y;
    const int mol = (int)blockIdx.x * BLOCK + tid;
    if (tid < kIceClasses) wcount[tid] = 0;
    __syncthreads();
    int k = -1;                                            // class; -1: no molecule on this lane
    if (mol < N) {
        const size_t im = (size_t)b * N + mol;
        const int n = nin[im];
        const int4 nb = nbr[im];                           // loaded with n, not after it
        k = 0;
        if (n == 4) {
            IceQ qi;
            qi.load(qhat + im * kIceQStride);
            const int js[4] = {nb.x, nb.y, nb.z, nb.w};
            int nst = 0, necl = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                IceQ qj;
                qj.load(qhat + ((size_t)b * N + js[u]) * kIceQStride);
                const double c = ice_bond_value(qi, qj, js[u] == mol);
                nst += c <= kIceStaggered;
                necl += (c >= kIceEclLo) & (c <= kIceEclHi);
            }
            k = ice_class_of(nst, necl);
        }
        cls[im] = (uint8_t)k;
    }
#pragma unroll
    for (int c = 0; c < kIceClasses; ++c) {
        const int m = __popcll(__ballot(k == c));
        if (lane == 0 && m) atomicAdd(&wcount[c], m);
    }
    __syncthreads();
    if (tid < kIceClasses && wcount[tid]) atomicAdd(&counts[(size_t)b * kIceClasses + tid], wcount[tid]);
}

// Every list entry's bond value in the reference layout (molecule-major, slot fastest: bond[mol][s], s < S) from the
// molecule-major list and k_ice_q's q^ of the same call: c for a neighbour entry, NaN for a degenerate one, exactly 2 for an
// entry that is not a bond (s >= nn, |d| >= r_c or d = 0).  One box, one entry per thread.
__global__ __launch_bounds__(256)
void k_ice_bonds(const double* __restrict__ pos, const double* __restrict__ ivect, const uint32_t* __restrict__ listm,
                 const int* __restrict__ nn, const double* __restrict__ qhat, double rc2,
                 double* __restrict__ bond, int N, int S, int ivcap, int b)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)N * S) return;
    const int mol = (int)(idx / S), s = (int)(idx - (size_t)mol * S);
    const int n = min(nn[(size_t)b * N + mol], S);
    double c = 2.0;
    if (s < n) {
        const uint32_t e = listm[((size_t)b * N + mol) * kRow + s];
        const int j = (int)(e & kJMask);
        const double* P = pos + (size_t)b * N * 3;
        const double* iv = ivect + ((size_t)b * ivcap + (e >> kJBits)) * 3;
        const double dx = (P[3 * (size_t)j] + iv[0]) - P[3 * (size_t)mol];
        const double dy = (P[3 * (size_t)j + 1] + iv[1]) - P[3 * (size_t)mol + 1];
        const double dz = (P[3 * (size_t)j + 2] + iv[2]) - P[3 * (size_t)mol + 2];
        const double r2 = dist2(dx, dy, dz);
        if (r2 < rc2 && r2 > 0.0) {
            IceQ qi, qj;
            qi.load(qhat + ((size_t)b * N + mol) * kIceQStride);
            qj.load(qhat + ((size_t)b * N + j) * kIceQStride);
            c = ice_bond_value(qi, qj, j == mol);
        }
    }
    bond[idx] = c;
}

}  // namespace mw
