// mw_ice_clusters.hip.h -- gfx950 (MI355X, CDNA4) device code of the mW energy engine: connected clusters of molecules of
// selected CHILL+ classes (k_ice_clusters), the largest-cluster observable of ice nucleation, melting and stacking-disorder
// studies.  The reference has no counterpart (DESIGN.md "Ice clusters").
#pragma once

#include "mw_common.hip.h"
#include "mw_ice.hip.h"

namespace mw {

// =====================================================================================
// Clusters of ice-like molecules from the four CHILL+ neighbours k_ice_q leaves behind.
//
// Inputs: the classes cls[i] and the neighbour entries nbr[i] of ONE classification (same call, same r_c), and a class mask:
// bit k selects class k, 1 <= k <= 5 (bit 0, "other", is refused by the host: such molecules need not have four neighbours, so
// nbr does not hold their bonds).  Molecule i is SELECTED iff bit cls[i] of the mask is set; it then has exactly four entries.
// Selected i and selected j are BONDED iff j is one of i's four entries or i is one of j's: undirected by construction (a
// last-ulp disagreement of the two directions at r_c cannot make the result depend on the traversal).  An entry that is an
// image of i itself is no bond, several images of one j are one bond.  Clusters are the connected components, through the
// periodic boundary (the entries are periodic neighbours already).
//
// Outputs per box: label[i] (int32, molecule order) = 0 for a molecule that is not selected, else the 1-based index of the
// smallest molecule of its cluster -- a canonical form, comparable with ==; summary[4] = {selected molecules, clusters, size
// of the largest cluster, its label}, a tie going to the smallest label, all 0 when nothing is selected; rounds = the
// hook / compress rounds the box took (a diagnostic).
//
// One workgroup per box, blockIdx.y = box.  lab[i] = i for selected i, kClusterNone otherwise; lab[x] <= x always and only
// ever decreases, so a walk x -> lab[x] ends at a root (lab[r] == r).  A round:
//   hook     : every selected i, for each entry j: ri = root(i), rj = root(j); where they differ, atomicMin(lab[max], min)
//              and the workgroup's "changed" word is set.  A hook that lands on a node another lane has just hooked elsewhere
//              may REPLACE that link; the bond that made it still joins two roots then and hooks again next round.
//   compress : lab[i] = root(i) (pointer jumping to the end).
// Rounds repeat, uncapped, until one passes with "changed" clear: every bond then joins two molecules of one tree, every
// link joins two molecules of one component, and a tree's root is its smallest molecule -- whatever order the atomics
// landed in.  Every lane reads "changed" after a barrier, so the loop's control flow is uniform.  Then sizes by integer
// atomicAdd on the roots, and cluster count, largest size and its smallest label by a DPP reduction per wavefront and a
// reduction over the wavefronts in LDS: integers, exact in any order.
//
// LDS = true : labels and sizes in LDS (8 B per molecule).
// LDS = false: labels in the output array itself, sizes in global scratch, both through L2 (device-scope relaxed atomics: no
//              stale line of the CU's L1 is ever read, and hooks are L2 atomics anyway).
// Nothing else is written.
// =====================================================================================
constexpr int kClusterNone = 0x7fffffff;
constexpr int kClusterMaxBlock = 1024;
constexpr int kClusterMaskAll = 0x3e;             // classes 1..5
constexpr int kClusterStaticLds = 512;            // the kernel's static __shared__ arrays fit in this (static_assert below)

template <int CTRL, int ROWMASK>
__device__ __forceinline__ int dpp_keep_i32(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, ROWMASK, 0xf, false); }
// Maximum / minimum over the 64 lanes through the DPP network (as dpp_wave_min); lane 63 ends up with it.
__device__ __forceinline__ int dpp_wave_max_i32(int v)
{
    v = max(v, dpp_keep_i32<0x111, 0xf>(v));
    v = max(v, dpp_keep_i32<0x112, 0xf>(v));
    v = max(v, dpp_keep_i32<0x114, 0xf>(v));
    v = max(v, dpp_keep_i32<0x118, 0xf>(v));
    v = max(v, dpp_keep_i32<0x142, 0xa>(v));
    v = max(v, dpp_keep_i32<0x143, 0xc>(v));
    return v;
}
__device__ __forceinline__ int dpp_wave_min_i32(int v)
{
    v = min(v, dpp_keep_i32<0x111, 0xf>(v));
    v = min(v, dpp_keep_i32<0x112, 0xf>(v));
    v = min(v, dpp_keep_i32<0x114, 0xf>(v));
    v = min(v, dpp_keep_i32<0x118, 0xf>(v));
    v = min(v, dpp_keep_i32<0x142, 0xa>(v));
    v = min(v, dpp_keep_i32<0x143, 0xc>(v));
    return v;
}

// Relaxed accesses to the label / size words that other lanes change while this one reads: workgroup scope in LDS, device
// scope in global memory (served by L2).
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
// the root of selected x: lab[.] <= . and strictly decreasing along the walk, so it ends
template <bool LDS>
__device__ __forceinline__ int cl_root(const int* lab, int x)
{
    for (;;) {
        const int p = cl_load<LDS>(&lab[x]);
        if (p == x) return x;
        x = p;
    }
}

template <bool LDS>
__global__ __launch_bounds__(kClusterMaxBlock)
void k_ice_clusters(const uint8_t* __restrict__ cls,     // [box][N]: classes of k_ice_class
                    const int4* __restrict__ nbr,         // [box][N]: the four neighbour entries of k_ice_q
                    int mask,
                    int* __restrict__ label,              // [box][N] out (the working labels too where !LDS)
                    int* __restrict__ gsize,              // [box][N] scratch where !LDS (unused otherwise)
                    int* __restrict__ summary,            // [box][4] out
                    int* __restrict__ rounds,             // [box] out
                    int N, int box0)
{
    extern __shared__ __attribute__((aligned(16))) int clds[];
    __shared__ int s_changed;
    __shared__ int s_red[4][kClusterMaxBlock / 64];
    static_assert(sizeof(int) * (1 + 4 * kClusterMaxBlock / 64) <= kClusterStaticLds, "static LDS of k_ice_clusters");
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
    const int b = box0 + (int)blockIdx.y;
    const uint8_t* C = cls + (size_t)b * N;
    const int4* NB = nbr + (size_t)b * N;
    int* out = label + (size_t)b * N;
    int* lab;
    int* siz;
    if constexpr (LDS) { lab = clds; siz = clds + N; }
    else { lab = out; siz = gsize + (size_t)b * N; }

    for (int i = tid; i < N; i += nthr) {
        cl_store<LDS>(&lab[i], ((mask >> C[i]) & 1) ? i : kClusterNone);
        cl_store<LDS>(&siz[i], 0);
    }
    __syncthreads();

    int nrounds = 0;
    for (;;) {
        if (tid == 0) s_changed = 0;
        __syncthreads();
        bool changed = false;
        for (int i = tid; i < N; i += nthr) {
            if (cl_load<LDS>(&lab[i]) == kClusterNone) continue;
            const int4 nb = NB[i];
            const int js[4] = {nb.x, nb.y, nb.z, nb.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = js[u];
                if ((unsigned)j >= (unsigned)N || j == i) continue;           // (an image of i itself is no bond)
                if (cl_load<LDS>(&lab[j]) == kClusterNone) continue;
                const int ri = cl_root<LDS>(lab, i), rj = cl_root<LDS>(lab, j);
                if (ri != rj) { cl_min<LDS>(&lab[max(ri, rj)], min(ri, rj)); changed = true; }
            }
        }
        if (changed) __hip_atomic_store(&s_changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        const int any = __hip_atomic_load(&s_changed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // the same word for every lane
        for (int i = tid; i < N; i += nthr)
            if (cl_load<LDS>(&lab[i]) != kClusterNone) cl_store<LDS>(&lab[i], cl_root<LDS>(lab, i));
        ++nrounds;
        __syncthreads();
        if (!any) break;
    }

    for (int i = tid; i < N; i += nthr) {
        const int r = cl_load<LDS>(&lab[i]);
        if (r != kClusterNone) cl_inc<LDS>(&siz[r]);
    }
    __syncthreads();
    int nsel = 0, nclu = 0, best = 0, bestlab = kClusterNone;
    for (int i = tid; i < N; i += nthr) {                                      // (i ascending: a tie keeps the smaller root)
        const int r = cl_load<LDS>(&lab[i]);
        if (r == kClusterNone) continue;
        ++nsel;
        if (r != i) continue;
        ++nclu;
        const int s = cl_load<LDS>(&siz[i]);
        if (s > best) { best = s; bestlab = i; }
    }
    nsel = dpp_wave_sum_i32(nsel);
    nclu = dpp_wave_sum_i32(nclu);
    const int wbest = __builtin_amdgcn_readlane(dpp_wave_max_i32(best), 63);
    const int wlab = dpp_wave_min_i32(best == wbest ? bestlab : kClusterNone);
    if (lane == 63) { s_red[0][wave] = nsel; s_red[1][wave] = nclu; s_red[2][wave] = wbest; s_red[3][wave] = wlab; }
    __syncthreads();
    if (tid == 0) {
        int ts = 0, tc = 0, tb = 0, tl = kClusterNone;
        for (int w = 0; w < nwave; ++w) {
            ts += s_red[0][w];
            tc += s_red[1][w];
            const int wb = s_red[2][w], wl = s_red[3][w];
            if (wb > tb || (wb == tb && wl < tl)) { tb = wb; tl = wl; }
        }
        int* sum = summary + 4 * (size_t)b;
        sum[0] = ts; sum[1] = tc; sum[2] = tb; sum[3] = tb > 0 ? tl + 1 : 0;
        rounds[b] = nrounds;
    }
    for (int i = tid; i < N; i += nthr) {
        const int r = cl_load<LDS>(&lab[i]);
        out[i] = r == kClusterNone ? 0 : r + 1;
    }
}

}  // namespace mw
