// mw_move_scan.hip.h -- gfx950 (MI355X, CDNA4) device code of the mW energy engine:
// the fused old/new evaluation of a trial move that scans the rows of the in-range neighbours (move_energy_wave), its
// per-wavefront LDS scratch and the diagnostic stamp arrays.
#pragma once

#include "mw_common.hip.h"

namespace mw {

// -------------------------------------------------------------------------------------
// Batched single-move path: old AND new local energy of a trial move in one pass.
//
// What the two evaluations share is most of the work: the same list rows, the same
// gathered positions and -- for the i--j--k triplets -- the same r_jk, g_jk (only the
// molecule itself sits somewhere else), so each exp(.) of a third body is evaluated
// once and used for both.  Lanes are packed across ALL in-range neighbours j at once:
// the rows of the in-range j's are laid end to end (sum of nn(j) ~ 150 slots) and dealt
// to the 64 lanes, so a pass is ~80 % full instead of one partly filled pass per j.
// Each lane finds the j that owns its slot from the (wave-uniform) prefix sums and
// pulls that j's vector/weights from the owning lane with cross-lane reads.
//
// Cases where a periodic image of the molecule itself takes part: as third body
// (k == i through a non-identical image) both geometries are evaluated in line; a
// molecule that neighbours its own image (cells narrower than the list radius) takes
// the plain one-evaluation-at-a-time routine above.  The k == i self term is skipped
// explicitly (the reference drops it through its cos(theta) >= 0.99 rule).
// -------------------------------------------------------------------------------------
struct MoveRes { double eo, en; unsigned int io, so, in_, sn; };

// Per-wavefront LDS scratch: the in-range neighbours of the molecule, compacted by rank, so
// that any lane can pull neighbour `r`'s record with plain LDS reads (a broadcast when lanes
// of one group read the same record).
constexpr int kCap = 24;                       // more in-range neighbours than this: plain routine
struct WaveScratch {
    double q[3][kCap];                         // position of j's image            (molint.F90:269)
    double c[3][kCap];                         // j's image vector minus that position: takes r_k + ivect(k) into j's frame in ONE add
    double rinvo[kCap], rinvn[kCap];           // 1/r_ij at the old / trial position
    double go[kCap], gn[kCap];                 // exp(gamma sigma/(r_ij - a sigma)) old / trial
    int flag[kCap];                            // bit0 = in range of the old position, bit1 = of the trial position
    unsigned long long cm[kCap];               // bit p of the end-to-end slot numbering set: a row ends at slot p
    uint32_t qe[64];                           // queue of in-range third bodies: packed list entry ...
    int qown[64];                              // ... and rank | (image, inverse image, flags of that rank) << 5 of the j whose row it came from
};
static_assert(sizeof(WaveScratch) % 16 == 0, "scratch records must keep 16-byte alignment");

// Returns false (nothing written) when the request needs the plain routine.
// `row(j, s)` returns list entry s of molecule j and `nnof(j)` its row length: global memory (molecule-major
// list) or, for small systems in the sweep driver, LDS copies.
// SELFIMG = false: the caller guarantees that no periodic image of a molecule can be a third body of its own neighbours
// (cells at least three list radii wide along every cell vector -- every box that goes through the cell-grid builder):
// a row entry with k == i is then the molecule itself, and the both-geometries branch and the inverse-image bookkeeping
// behind it fall away (25 vector instructions per move).
#if defined(MW_SWEEP_STAMPS)   // a diagnostic build of the library only (tools/sweep_stamps.py): shader-clock cycles per stage of walker 0's
                              // first wavefront, summed over the launch -- g_sweep_stamps[16 + k] = cycles between stamp k - 1 and stamp k
__device__ unsigned long long g_sweep_stamps[48];
#define MW_STAMP(k) do { if (blockIdx.x == 0 && threadIdx.x < 64) { const unsigned long long mw_t = clock64(); \
                         if (lane == 0 && (k) > 0) g_sweep_stamps[16 + (k)] += mw_t - mw_tprev; mw_tprev = mw_t; } } while (0)
#elif defined(MW_LAT_STAMPS)      // tools/kbench built with -DMW_LAT_STAMPS only: where one wavefront's time goes (100 MHz ticks)
__device__ unsigned long long g_lat_stamps[16];
#define MW_STAMP(k) do { if (lane == 0) g_lat_stamps[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define MW_STAMP(k) do { } while (0)
#endif

// NOTH > 0 (the Monte Carlo driver's look-ahead, mw_sweep.hip.h): `oth` holds the molecules that moves EARLIER in the chain
// are trying to move at the same time (-1: none); bit o of `cmask` comes back set when this evaluation read the position of
// oth[o] -- it is then only valid if that earlier move is rejected.  (The molecule's own index is the caller's to compare.)
// COUNTS = false (the Monte Carlo driver, which has no use for them): the interaction and slot counts of `res` are left unset and
// their bookkeeping -- a counter per item, a prefix sum's upper half, a wave-wide integer sum -- falls away.
template <bool SELFIMG = true, int NOTH = 0, bool COUNTS = true, typename PosFn, typename IvFn, typename RowFn, typename NnFn>
__device__ __forceinline__ bool move_energy_wave(PosFn getpos, IvFn getiv, RowFn row, NnFn nnof,
                                                 WaveScratch* __restrict__ ws, int niv,
                                                 int i, int n_i, uint32_t e,
                                                 double xo, double yo, double zo,
                                                 double xn, double yn, double zn, int lane, MoveRes& res,
                                                 const int* oth = nullptr, unsigned* cmask = nullptr)
{
    unsigned cm = 0u;                  // (per lane until the end: one wave-wide OR per evaluation, not a ballot per gather step and slot)
#ifdef MW_SWEEP_STAMPS
    unsigned long long mw_tprev = 0ull;
#endif
    // ---- pass 0: imol's own row; lanes 0..31 take slot l against the OLD position, lanes 32..63 the same
    // slot against the TRIAL position, so that one rsqrt/reciprocal/exp sequence serves both evaluations.
    // `e` arrives as entry (lane & 31) of imol's row, fetched by the caller ahead of time (whatever the row
    // length: rows are padded).  Rows longer than 32 entries take the plain routine, and so does a molecule
    // that neighbours one of its own periodic images.
    MW_STAMP(0);
    if (n_i > 32) return false;
    const int half = lane >> 5, sl = lane & 31;
    const bool has = sl < n_i;
    const int j = has ? (int)(e & kJMask) : 0, kimg = has ? (int)(e >> kJBits) : 0;
    if (SELFIMG && __ballot(has && j == i) != 0ull) return false;
    if constexpr (NOTH > 0) {
#pragma unroll
        for (int o = 0; o < NOTH; ++o) cm |= (has && j == oth[o]) ? 1u << o : 0u;
    }
    double xj, yj, zj, jvx, jvy, jvz;
    getpos(j, xj, yj, zj);
    getiv(kimg, jvx, jvy, jvz);
    const int nnj = has ? nnof(j) : 0;
    const double qx = xj + jvx, qy = yj + jvy, qz = zj + jvz;                 // molint.F90:269
    const double rix = half ? xn : xo, riy = half ? yn : yo, riz = half ? zn : zo;
    const double ax = qx - rix, ay = qy - riy, az = qz - riz;                 // :272
    const double r2 = ax * ax + ay * ay + az * az;
    const bool in = has && (r2 < kRcSq);                                      // :276
    const unsigned long long B = __ballot(in);
    const unsigned int mo_ = (unsigned int)B, mn_ = (unsigned int)(B >> 32);  // in range of the old / trial position, by slot
    const unsigned int U = mo_ | mn_;
    const int cntU = __popc(U);
    if (cntU > kCap) return false;
    MW_STAMP(1);

    double t3o = 0.0, t3n = 0.0;
    unsigned int nto = 0, ntn = 0;

    // ---- compact the in-range neighbours (of either position) into the wave's scratch ------------
    const bool inu = (U >> sl) & 1u;
    // (the in-range slots below this lane's: v_mbcnt counts them without a per-lane mask held in a register from move to move)
    const int rank = half ? (int)__builtin_amdgcn_mbcnt_hi(U, 0u) : (int)__builtin_amdgcn_mbcnt_lo(U, 0u);
    // The rows of the in-range j are laid end to end (slots 0..T-1).  An inclusive prefix sum over the 32
    // slot lanes of each half gives every j its first slot, and in its upper 16 bits the list slots each
    // evaluation visits (half 0: old position, half 1: trial position).
    const int mine = (inu ? nnj : 0) | (COUNTS ? ((in ? nnj : 0) << 16) : 0);
    int inc = mine;
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xf, 0xf, true);        // row_shr:1
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xf, 0xf, true);        // row_shr:2
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xf, 0xf, true);        // row_shr:4
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xf, 0xf, true);        // row_shr:8
    const int r15 = __builtin_amdgcn_readlane(inc, 15), r47 = __builtin_amdgcn_readlane(inc, 47);
    inc += (lane & 16) ? (half ? r47 : r15) : 0;
    const int tot0 = __builtin_amdgcn_readlane(inc, 31), tot1 = __builtin_amdgcn_readlane(inc, 63);
    const int T = tot0 & 0xffff;
    const unsigned int so = (unsigned int)n_i + (unsigned int)(tot0 >> 16), sn = (unsigned int)n_i + (unsigned int)(tot1 >> 16);
    const int start = (inc & 0xffff) - (inu ? nnj : 0);
    // lane r of these two holds, for the in-range neighbour of rank r, its molecule and the first slot of
    // its row: the scan below locates a slot's owner from registers alone (no LDS round trips in front of
    // the row fetch).  Lanes that own no record aim at lane 63, which no rank reaches (cntU <= kCap).
    const int dstl = (inu && half == 0) ? rank : 63;
    const int jv  = __builtin_amdgcn_ds_permute(dstl << 2, j);
    const int stv = __builtin_amdgcn_ds_permute(dstl << 2, start);
    // the image that undoes `kimg`: cells are numbered centre first, then lexicographically without the
    // centre (compute_ivects, molint.F90:174-217), so the opposite cell is the mirror position
    const int cc = (niv - 1) >> 1;
    int kinv = 0;
    if constexpr (SELFIMG) {
        const int lin = kimg <= cc ? kimg - 1 : kimg, linv = niv - 1 - lin;
        kinv = kimg == 0 ? 0 : (linv < cc ? linv + 1 : linv);
    }
    // image (10 bits) | inverse image (10 bits) | in range of old, trial position (2 bits), by rank like jv
    const int flg = (int)((mo_ >> sl) & 1u) | (int)(((mn_ >> sl) & 1u) << 1);
    const int wv = __builtin_amdgcn_ds_permute(dstl << 2, kimg | (kinv << 10) | (flg << 20));
    // row-end marks: chunk c of the scan reads mask cm[c]; a slot's owner is the number of marks before it
    {   // (the address is worked out here, from a lane number the compiler cannot hoist: as a loop invariant of the callers'
        //  move loops it was one more register held from move to move -- the one that tipped a build of the driver into a spill)
        int lz = lane;
        asm volatile("" : "+v"(lz));
        if (lz < kCap) ws->cm[lz] = 0ull;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (inu && half == 0 && rank > 0 && start > 0)      // (rows are never empty: j lists i back)
        __hip_atomic_fetch_or(&ws->cm[(start - 1) >> 6], 1ull << ((start - 1) & 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    wave_fence();

    // ---- rows of the in-range j: fetched ahead ----------------------------------------------------
    // The i--j--k stage below walks the rows of all in-range j laid end to end, 64 slots per chunk.  A
    // chunk's slot -> (owner rank, owner's packed word, row entry) fetch is issued TWO CHUNKS AHEAD of its
    // evaluation -- the first two right here, BEFORE the pair terms of pass 0 (a rsqrt, a reciprocal and an exp per
    // lane: the arithmetic the row fetch from global memory hides behind) -- so the scan never waits for a row.
    MW_STAMP(2);
    int nbefore = 0;                                         // row ends in the chunks already fetched (wave-uniform)
    auto fetch = [&](int t, int& own, int& wj, uint32_t& ent) {
        const unsigned long long M = ws->cm[t >> 6];         // one address for the whole wave
        const unsigned int mlo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)M);
        const unsigned int mhi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(M >> 32));
        own = nbefore + (int)__builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
        nbefore += __popc(mlo) + __popc(mhi);
        const int jj = __builtin_amdgcn_ds_bpermute(own << 2, jv);
        const int st = __builtin_amdgcn_ds_bpermute(own << 2, stv);
        wj = __builtin_amdgcn_ds_bpermute(own << 2, wv);
        ent = t < T ? row(jj, t - st) : 0u;
    };
    int own_a = 0, own_b = 0, w_a = 0, w_b = 0; uint32_t ent_a = 0u, ent_b = 0u;
    if (T > 0) fetch(lane, own_a, w_a, ent_a);
    if (T > 64) fetch(64 + lane, own_b, w_b, ent_b);

    // ---- pass 0's pair terms; the in-range neighbours' records into the scratch --------------------
    double rinv = 0.0, e1 = 0.0, g = 0.0;
    if (in) pair_terms(r2, rinv, e1, g);
    const double qq = kSigSq * rinv * rinv;
    const double accp = in ? (kAeps * (kBigB * (qq * qq) - 1.0)) * e1 : 0.0;  // :294-297 (old in lanes 0..31, trial in 32..63)
    if (inu) {
        if (half == 0) {
            ws->q[0][rank] = qx; ws->q[1][rank] = qy; ws->q[2][rank] = qz;
            ws->c[0][rank] = jvx - qx; ws->c[1][rank] = jvy - qy; ws->c[2][rank] = jvz - qz;
            ws->rinvo[rank] = rinv; ws->go[rank] = g;
            ws->flag[rank] = flg;
        } else {
            ws->rinvn[rank] = rinv; ws->gn[rank] = g;
        }
    }
    wave_fence();

    // ---- the triplets, one ITEM per lane ------------------------------------------------------------
    // Two kinds of item share one instruction stream (what differs sits in two short sections that a pass without
    // such items skips):
    //  F  an in-range third body k of an in-range neighbour j, queued by the scan below: the i--j--k triplet
    //     (molint.F90:324-343) -- gather k, rsqrt / reciprocal / exp of r_jk, then cos(theta) at j in both geometries;
    //  P  a pair (a < b) of in-range neighbours: the j--i--k triplet (:302-318; a is the earlier list slot, so cos is
    //     formed in the reference's order) -- everything it needs is in the scratch already.
    // In both, cos = (A . B) r_A r_B with A = r_i - q_A from the molecule to neighbour A's image (A = j for F, a for P),
    // and the term is g_A g_B (cos - cos0)^2.
    MW_STAMP(3);
    const int npairs = cntU * (cntU - 1) / 2;
    int nq = 0;                                              // queued F items (wave-uniform)
    auto items = [&](int nP) {
        wave_fence();
        const int total = nq + nP;
        for (int base = 0; base < total; base += 64) {
            const int idx = base + lane;
            const bool isF = idx < nq, isP = !isF && idx < total;
            int ia = 0, fl = 0;
            double box_ = 0.0, boy_ = 0.0, boz_ = 0.0, bnx = 0.0, bny = 0.0, bnz = 0.0;
            double rbo = 0.0, rbn = 0.0, gbo = 0.0, gbn = 0.0;
            if (isF) {
                const uint32_t e2 = ws->qe[idx];
                const int qw = ws->qown[idx];
                ia = qw & 31; fl = qw >> 25;
                const int kk = (int)(e2 & kJMask), k2 = (int)(e2 >> kJBits);
                // r_jk = (r_k + ivect(k)) + (ivect(j) - q_j)   (:332,334, the last two terms taken together in pass 0: the very
                // expression the scan used for the in-range decision)
                double xk, yk, zk, kvx, kvy, kvz;
                getpos(kk, xk, yk, zk);
                getiv(k2, kvx, kvy, kvz);
                box_ = (xk + kvx) + ws->c[0][ia];
                boy_ = (yk + kvy) + ws->c[1][ia];
                boz_ = (zk + kvz) + ws->c[2][ia];
                const double s2 = box_ * box_ + boy_ * boy_ + boz_ * boz_;       // :335 (in range: tested at scan)
                double rk, gk, e1k;
                pair_terms(s2, rk, e1k, gk);
                bnx = box_; bny = boy_; bnz = boz_;
                rbo = rk; rbn = rk; gbo = gk; gbn = gk;
            } else if (isP) {
                const int p = idx - nq;
                int b;
                tri_pair(p, ia, b, [](float x) { return __builtin_amdgcn_sqrtf(x); });       // (v_sqrt_f32, not the IEEE expansion)
                fl = ws->flag[ia] & ws->flag[b];
                const double qbx = ws->q[0][b], qby = ws->q[1][b], qbz = ws->q[2][b];
                box_ = xo - qbx; boy_ = yo - qby; boz_ = zo - qbz;
                bnx = xn - qbx; bny = yn - qby; bnz = zn - qbz;
                rbo = ws->rinvo[b]; rbn = ws->rinvn[b]; gbo = ws->go[b]; gbn = ws->gn[b];
            }
            if (isF || isP) {
                const double pax = ws->q[0][ia], pay = ws->q[1][ia], paz = ws->q[2][ia];
                const double rao = ws->rinvo[ia], ran = ws->rinvn[ia], gao = ws->go[ia], gan = ws->gn[ia];
                if (fl & 1) {
                    const double ct = (((xo - pax) * box_ + (yo - pay) * boy_ + (zo - paz) * boz_) * rao) * rbo;   // :316,320,341,365
                    if (ct < 0.99) { const double d = ct - kCos0; t3o += gao * (gbo * (d * d)); if constexpr (COUNTS) ++nto; }   // :367-368,385-387
                }
                if (fl & 2) {
                    const double ct = (((xn - pax) * bnx + (yn - pay) * bny + (zn - paz) * bnz) * ran) * rbn;
                    if (ct < 0.99) { const double d = ct - kCos0; t3n += gan * (gbn * (d * d)); if constexpr (COUNTS) ++ntn; }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        nq = 0;
    };

    // The P items run HERE, between the row fetch and the first use of what it brings: without them the scan's first
    // chunk waits for global memory (measured: one merged pass of F and P items at the end saves ~60 instructions per
    // move and LOSES 5 % -- the fetch latency it exposes costs more than the instructions it saves).
    if (npairs > 0) items(npairs);

    // ---- i--j--k triplets (molint.F90:324-343): the rows of all in-range j, end to end --------
    // SCAN: every slot gets the cheap part (gather, distance test); the ~1/3 that are in range are queued (entry + owner
    // rank, 8 bytes) in the wave's scratch as F items; whenever 64 are queued a pass of F items runs with every lane busy.
    MW_STAMP(4);
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool valid = t < T;
        const int own = own_a, wj = w_a;
        const uint32_t e2 = ent_a;
        own_a = own_b; w_a = w_b; ent_a = ent_b;
        if (t0 + 128 < T) fetch(t + 128, own_b, w_b, ent_b);
        const int kk = (int)(e2 & kJMask), k2 = (int)(e2 >> kJBits);
        if constexpr (NOTH > 0) {
#pragma unroll
            for (int o = 0; o < NOTH; ++o) cm |= (valid && kk == oth[o]) ? 1u << o : 0u;
        }
        double xk, yk, zk, kvx, kvy, kvz;
        getpos(kk, xk, yk, zk);
        getiv(k2, kvx, kvy, kvz);
        const double cjx = ws->c[0][own], cjy = ws->c[1][own], cjz = ws->c[2][own];
        const bool self = valid && (kk == i);
        bool selfmove = false;
        if constexpr (SELFIMG) {
            const bool selfimg = self && (k2 == ((wj >> 10) & 1023));   // the molecule itself, not an image: k's shift undoes j's
            selfmove = self && !selfimg;
        }
        const double box_ = (xk + kvx) + cjx;                                    // :332,334 (see the F items)
        const double boy_ = (yk + kvy) + cjy;
        const double boz_ = (zk + kvz) + cjz;
        const double s2o = box_ * box_ + boy_ * boy_ + boz_ * boz_;              // :335
        if (SELFIMG && __ballot(selfmove) != 0ull) {
            // an image of the molecule itself as third body moves with it: both geometries, in line (rare)
            if (selfmove) {
                const int fl = wj >> 20;
                const double pjx = ws->q[0][own], pjy = ws->q[1][own], pjz = ws->q[2][own];
                const double bnx = (xn + kvx) + cjx, bny = (yn + kvy) + cjy, bnz = (zn + kvz) + cjz;
                const double s2n = bnx * bnx + bny * bny + bnz * bnz;
                double rk, gk, e1k;
                if ((s2o < kRcSq) && (fl & 1)) {
                    pair_terms(s2o, rk, e1k, gk);
                    const double ct = (-((pjx - xo) * box_ + (pjy - yo) * boy_ + (pjz - zo) * boz_) * ws->rinvo[own]) * rk;
                    if (ct < 0.99) { const double d = ct - kCos0; t3o += ws->go[own] * (gk * (d * d)); ++nto; }
                }
                if ((s2n < kRcSq) && (fl & 2)) {
                    pair_terms(s2n, rk, e1k, gk);
                    const double ct = (-((pjx - xn) * bnx + (pjy - yn) * bny + (pjz - zn) * bnz) * ws->rinvn[own]) * rk;
                    if (ct < 0.99) { const double d = ct - kCos0; t3n += ws->gn[own] * (gk * (d * d)); ++ntn; }
                }
            }
        }
        const bool inq = valid && !self && (s2o < kRcSq);                        // :361; the k == i self term is dropped
        const unsigned long long mq = __ballot(inq);
        const int c = __popcll(mq);
        if (nq + c > 64) items(0);
        if (inq) {
            const int slot = nq + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(mq >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mq, 0u));
            ws->qe[slot] = e2; ws->qown[slot] = own | (wj << 5);
        }
        nq += c;
    }
    MW_STAMP(5);
    if (nq > 0) items(0);                                    // what the scan left in the queue
    __builtin_amdgcn_wave_barrier();                          // scratch is reused by the wave's next request
    MW_STAMP(6);

    // Wave sums on the DPP network (no LDS round trips): afterwards lane 63 holds the totals.
    double eo, en;                                                                                 // :397
    dpp_wave_sum2(kLamEps * t3o + (half == 0 ? accp : 0.0), kLamEps * t3n + (half == 1 ? accp : 0.0), eo, en);
    res.eo = eo; res.en = en;
    if constexpr (COUNTS) {
        const unsigned int cs = (unsigned int)__builtin_amdgcn_readlane(dpp_wave_sum_i32((int)(nto | (ntn << 16))), 63);
        nto = cs & 0xffffu; ntn = cs >> 16;
        res.io = (unsigned int)__popc(mo_) + nto; res.in_ = (unsigned int)__popc(mn_) + ntn;
        res.so = so; res.sn = sn;
    }
    if constexpr (NOTH > 0) {          // OR over the lanes, on the DPP network
        *cmask = (unsigned)__builtin_amdgcn_readlane((int)dpp_wave_or(cm), 63);
    }
    MW_STAMP(7);
    return true;
}

}  // namespace mw
