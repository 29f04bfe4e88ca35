// mw_move_lanes.hip.h -- gfx950 (MI355X, CDNA4) device code of the mW energy engine:
// the moment path of the batched single-move kernel with a LANE PAIR per trial move (move_energy_mom_lanes).
#pragma once

#include "mw_common.hip.h"
#include "mw_full_energy.hip.h"
#include "mw_move_scan.hip.h"

namespace mw {

// -------------------------------------------------------------------------------------
// move_energy_mom_wave (mw_move_moments.hip.h) gives a request a whole wavefront, and a wave64 instruction costs the same with ten
// live lanes as with 64: on thermal ice its expensive section runs with 15 of 64 lanes live.  Here a wavefront serves a GROUP of 32
// requests: lanes 2r and 2r + 1 serve request r of the group at the old and at the trial position, in lockstep over the same entries,
// the way the full-box kernel serves a molecule per lane (mw_full_energy.hip.h: atom_energy).
//   phase 1  both lanes walk the n_i slots of i's row (up to kRow: no 32-slot limit), each against its own position, and park the
//            entries in range of EITHER position, in row order, in the request's queue in LDS (or rebuild that queue from the mask
//            an earlier scan of the same row left: THE MASK WALK below);
//   phase 2  over the queue: the pair term and i's arm into the lane's own running sums (MomentSums: the j--i--k sum is
//            1/2 [(|S2|^2 - Q) - 2 c0 (|S1|^2 - Q) + c0^2 (S0^2 - Q)] of them, no pair loop), and the i--j--k sum from j's moments less
//            i's OLD arm, as in move_energy_mom_wave.
// A lane's energy is the sum of its own terms in queue order: no cross-lane sum, so a request's bits depend on the request alone --
// not on its group, its lane, its companions or whether counts are on.
//
// THE 0.99 RULE.  Neither sum can drop a term the reference drops (molint.F90:367-371), so a request that owns such a term is
// DECLINED to k_move_fallback.  For a pair (a < b) of entries in range of one position P these are: b within the cutoff of a and
// cos(theta_Pab) or cos(theta_Pba) >= 0.99 - 1e-9 (a third body in j's moments; the test of move_energy_mom_wave), and
// cos(theta_aPb) >= 0.99 - 1e-9 (the j--i--k term the wave routine dropped itself).  All three imply |ab| < cutoff -- an angle
// below 8.2 degrees between two arms shorter than the cutoff -- and |ab| does not depend on P: the two lanes of a pair SHARE the
// pairs of the queue between them (lane `side` takes b = a + 1 + side, a + 3 + side, ...).  |ab| < cutoff alone is no rare event:
// a first-shell neighbour is bonded to the second-shell neighbours beside it in the queue (23 % of a queue's pairs on thermal ice),
// and among a wavefront's 64 pairs one is below the cutoff on 98 % of the trips.  What is rare is THE GATE (mode bit 7 of
// k_move_energy; MW_MOVE_GATE=0 keeps |ab| < cutoff alone): a lane tests its OWN pair against its own position P and its
// partner's P' (taken once per group on the DPP network; nothing is exchanged on a trip).  With Q = |Pa|^2, R = |Pb|^2, S = |ab|^2
// and t = Q + R - S = 2 (a - P).(b - P), the triangle P a b has 4 Area^2 = QR - (t/2)^2, the same number from every vertex, and
// sin^2 of the angle at a vertex is 4 Area^2 over the product of the two squared sides that meet there.  So
//      cos^2 >= kappa^2 at SOME vertex   =>   QR - (t/2)^2 <= (1 - kappa^2) max(QR, QS, RS)                    "thin(Q, R, S)"
// and the gate tests that with kappa = 0.98: the right side is 0.0396 max(..) where a triplet the rule drops has at most 0.0199
// max(..) on the left -- a factor of two, against a rounding error of a few units in 1e-16 QR.  The sign of the cosine and the
// in-range conditions are left out, so the pairs the gate passes are a SUPERSET of the pairs the rule drops at either position
// (tests/test_move_gate_ref.py: no miss among 4e5 constructed triangles), and on thermal ice it passes ~10 pairs per 2048
// requests.  When some lane's gate fires, every lane takes its partner's b as well (DPP) and tests the angles of its own pair and
// of its partner's at its OWN position, on squares (no square root): that block, and so `hard`, is what it was without the gate.
// Also declined: more than kLaneQueue entries in range of either position, and a molecule that lists itself.
// -------------------------------------------------------------------------------------
constexpr int kLaneQueue = 16;                                   // queue entries per request (thermal ice: 9.2 on average, never above 16)
constexpr int kLaneQueueWords = 32 * kLaneQueue;                 // per wavefront: entry c of request r at word c * 32 + r (a trip reads 32 consecutive words)
static_assert(kLaneQueueWords * sizeof(uint32_t) <= sizeof(WaveScratch), "the queues of a wavefront's 32 requests are overlaid on its WaveScratch");

// the partner lane's value (lanes 2r <-> 2r + 1) and the even lane's value in both lanes, on the DPP network (every lane active)
__device__ __forceinline__ int pair_swap_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xb1, 0xf, 0xf, true); }   // quad_perm:[1,0,3,2]
__device__ __forceinline__ int pair_even_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xa0, 0xf, 0xf, true); }   // quad_perm:[0,0,2,2]
__device__ __forceinline__ double pair_even_f64(double v) { return dpp_mov_f64<0xa0, 0xf>(v); }
__device__ __forceinline__ double pair_swap_f64(double v) { return dpp_mov_f64<0xb1, 0xf>(v); }
__device__ __forceinline__ double pair_odd_f64(double v) { return dpp_mov_f64<0xf5, 0xf>(v); }                            // quad_perm:[1,1,3,3]

// r_j + ivect (molint.F90:269) of a row entry: ONE spelling for every in-range decision of the lane-pair routines
template <typename PosFn, typename IvFn>
__device__ __forceinline__ void lanes_image(PosFn getpos, IvFn getiv, uint32_t e, double& qx, double& qy, double& qz)
{
    double xj, yj, zj, vx, vy, vz;
    getpos((int)(e & kJMask), xj, yj, zj);
    getiv((int)(e >> kJBits), vx, vy, vz);
    qx = xj + vx; qy = yj + vy; qz = zj + vz;
}

// THE SCAN of a lane pair (lanes 2r and 2r + 1, `side` = 0 and 1) over the n_i slots of molecule i's row `rowp` (its first four
// entries already in `first`), each lane with its own position (px, py, pz): four slots per load, one load ahead (the last one
// wraps to the row's start: never used).  `cnt` = the entries in range of EITHER position, `self` = the row names i itself.  The
// loop is wave-uniform.
//   STORE   phase 1 of move_energy_mom_lanes: both lanes gather all four slots, each tests them against its own position, and the
//           first kLaneQueue entries in range of either are parked in the request's queue, in row order.
//   else    the count pass of k_move_energy, which sorts an item's requests by `cnt` before any of them is evaluated: nothing is
//           written, and `msk` gets bit s set for every counted slot s < 32 -- the request's ROW-SLOT MASK, which lanes_entries
//           below turns back into the queue.  Here the pair SPLITS A LOAD'S FOUR SLOTS BY PARITY: lane `side` gathers slots side
//           and 2 + side only, tests each against its own position and its partner's (the subtraction and the squares its partner
//           would make, on the same values: the same bits), and the two lanes swap their two "in range of either" bits and the
//           self bit in ONE exchange per load.  Both assemble the nibble of `msk`, the `cnt` and the `self` that four gathers per
//           lane and an exchange per slot gave: half the gathers for the same squared distances.
template <bool STORE, typename ImageFn>
__device__ __forceinline__ void lanes_scan(ImageFn image, const uint32_t* __restrict__ rowp, uint32_t* __restrict__ wq, int r, int side,
                                           int i, int n_i, uint4 first, double px, double py, double pz, int& cnt, bool& self,
                                           uint32_t& msk)
{
    uint4 c4 = first;
    if constexpr (!STORE) {
        const double tx = pair_swap_f64(px), ty = pair_swap_f64(py), tz = pair_swap_f64(pz);       // the partner's position
        for (int s0 = 0; __ballot(s0 < n_i) != 0ull; s0 += 4) {
            const uint4 nx = *reinterpret_cast<const uint4*>(rowp + ((s0 + 4) & (kRow - 1)));
            const uint32_t e0 = side ? c4.y : c4.x, e1 = side ? c4.w : c4.z;
            double q0x, q0y, q0z, q1x, q1y, q1z;
            image(e0, q0x, q0y, q0z);                            // (two slots' gathers in flight together)
            image(e1, q1x, q1y, q1z);
            const bool has0 = s0 + side < n_i, has1 = s0 + 2 + side < n_i;
            const bool in0 = has0 && (dist2(q0x - px, q0y - py, q0z - pz) < kRcSq || dist2(q0x - tx, q0y - ty, q0z - tz) < kRcSq);   // :272,276
            const bool in1 = has1 && (dist2(q1x - px, q1y - py, q1z - pz) < kRcSq || dist2(q1x - tx, q1y - ty, q1z - tz) < kRcSq);
            const bool sf = (has0 && (int)(e0 & kJMask) == i) || (has1 && (int)(e1 & kJMask) == i);
            const int mine = ((in0 ? 1 : 0) | (in1 ? 4 : 0)) << side | (sf ? 16 : 0);   // bits side and 2 + side: this lane's slots
            const int both = mine | pair_swap_i32(mine);         // (unconditionally: every lane takes part in the exchange)
            self = self || (both & 16) != 0;
            msk |= (uint32_t)(both & 15) << (s0 & 31);           // (a row longer than 32 slots: its mask is not used)
            cnt += __popc((unsigned)(both & 15));
            c4 = nx;
        }
    } else {
        for (int s0 = 0; __ballot(s0 < n_i) != 0ull; s0 += 4) {
            const uint4 nx = *reinterpret_cast<const uint4*>(rowp + ((s0 + 4) & (kRow - 1)));
            const uint32_t ent[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
            for (int h = 0; h < 4; h += 2) {                     // two slots' gathers in flight together
                double q[2][3];
#pragma unroll
                for (int u = 0; u < 2; ++u) image(ent[h + u], q[u][0], q[u][1], q[u][2]);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const bool has = s0 + h + u < n_i;
                    const bool mine = has && dist2(q[u][0] - px, q[u][1] - py, q[u][2] - pz) < kRcSq;   // :272,276
                    const int other = pair_swap_i32(mine ? 1 : 0);   // (unconditionally: every lane takes part in the exchange)
                    const bool inu = mine || other != 0;
                    self = self || (has && (int)(ent[h + u] & kJMask) == i);
                    if (inu) {                                   // (both lanes of the pair write the same word)
                        if (cnt < kLaneQueue) wq[cnt * 32 + r] = ent[h + u];
                        ++cnt;                                   // past the cap: counted, never stored
                    }
                }
            }
            c4 = nx;
        }
    }
}

// THE MASK WALK.  The count pass has scanned a sorted item's rows once and kept, per request, the mask lanes_scan<false> makes; a
// request whose row has more than 32 slots keeps kMaskScan, "scan me" (no served request's mask: that has at most kLaneQueue bits).
// The main pass rebuilds a queue from its mask instead of scanning again: the set bits in ascending order are the in-range slots in
// row order, so entry c of the queue is the row's entry at the c-th set bit -- word for word what lanes_scan<true> parks.  The two
// lanes of a pair share the work: lane `side` LOADS the entries of rank side, side + 2, ... (lanes_entries: kLaneWalk loads at most,
// the trips wave-uniform) and later PARKS them (lanes_park), so that the loads can be in flight one group ahead.
constexpr int kLaneWalk = kLaneQueue / 2;
constexpr uint32_t kMaskScan = 0xffffffffu;
static_assert(kLaneQueue < 32, "a served request's mask is never kMaskScan");

// `row` = the list of the box, `at` = the first word of this lane's row in it (32 bits: the loads take a scalar base)
__device__ __forceinline__ void lanes_entries(const uint32_t* __restrict__ row, unsigned at, uint32_t msk, int side, uint32_t (&ent)[kLaneWalk])
{
    uint32_t m = side ? msk & (msk - 1u) : msk;                  // (the odd lane starts at the second set bit)
    bool more = true;                                            // (wave-uniform; no `break`: the loop unrolls, and `ent` stays in registers)
#pragma unroll
    for (int c = 0; c < kLaneWalk; ++c) {
        ent[c] = 0u;
        more = more && __ballot(m != 0u) != 0ull;
        if (more) {
            if (m != 0u) ent[c] = row[at + (unsigned)__builtin_ctz(m)];
            m &= m - 1u; m &= m - 1u;                            // the lowest two set bits: this lane's and its partner's
        }
    }
}

// entry c of lane `side` is entry 2c + side of the queue of request r; nq = the queue's length (0: no request in this lane)
__device__ __forceinline__ void lanes_park(uint32_t* __restrict__ wq, int r, int side, int nq, const uint32_t (&ent)[kLaneWalk])
{
    uint32_t* __restrict__ mine = wq + side * 32 + r;            // (one address: the eight stores differ by constant offsets)
    const int left = nq - side;
    bool more = true;
#pragma unroll
    for (int c = 0; c < kLaneWalk; ++c) {
        more = more && __ballot(2 * c < left) != 0ull;
        if (more && 2 * c < left) mine[c * 64] = ent[c];
    }
}

// THE F32 PAIR GATE (mode bit 8 of k_move_energy; MW_MOVE_PAIRS32=0 clears it).  The pair loop of move_energy_mom_lanes gathers
// every entry of a queue from LDS once per pair it belongs to, in FP64, to decide a factor-two superset test.  A group that WALKS
// THE MASKS has its entries in registers already -- lane `side` holds entries side, side + 2, ... of its request in `ent` -- so it
// first runs the gate from registers, in f32, and the FP64 loop afterwards serves only the queue rows `a` for which some lane's
// f32 gate fired (on thermal ice ~10 pairs per 2048 requests): that loop, its gate and its angle block are unchanged, so `hard`
// is what it was as long as the f32 gate passes every pair the rule drops.
//   set-up  a lane gathers the image of each of its entries once (lanes_image, FP64), forms a - P and a - P' in FP64 (P the OLD
//           position in both lanes, P' the trial one) and keeps five f32 words: v = fl(a - P), Qo = fl(|a - P|^2), Qn = fl(|a - P'|^2).
//           An entry past the queue's end gets v.x = NaN: no pair with it is `near`.
//   pairs   entry a's five words come from their owner to both lanes of the pair on the DPP network (quad_perm [0,0,2,2] for an even
//           a, [1,1,3,3] for an odd one), a lane's b are its OWN entries c with 2c + side > a: the pairs of a queue are split by b's
//           parity, every pair is met once.  A lane index cannot index registers, so the (a, c) triangle is unrolled, with
//           wave-uniform exits at the group's longest queue (groups are sorted by nq: the exits are tight).
//   test    S = |v_b - v_a|^2 < rc^2 (1 + 1e-5) and thin(Qo_a, Qo_b, S) or thin(Qn_a, Qn_b, S) -- the two as one packed evaluation.
// THE BOUND.  A group holding a request moved by more than 16 bohr, or an entry nearer than 0.03 rc to either position, leaves all
// its rows to the FP64 loop (`wide`).  Otherwise every component of v is below 32 bohr, so a component of v_b - v_a is off by at
// most d = 2.4e-6 bohr (two roundings at ulp(32)/2, one of the difference), S by 2 sqrt(3) |ab| d + 3 roundings < 8e-5 bohr^2 = 1.2e-6
// rc^2 where |ab| <= rc -- inside the 1e-5 of `near` -- and t/2 = (Q + R - S)/2 by e <= sqrt(3) (sqrt(Q) + sqrt(R)) d + 2e-7 max(Q, R, S).
// The left side QR - (t/2)^2 moves by 2 sqrt(QR) e + 2e-7 QR: for a dropped triplet (both arms between 0.03 rc and rc, S <= 4 R) below
// 1e-4 QR, where the gate keeps 0.0197 max(QR, QS, RS) over the rule -- the same factor of two, to 0.5 % (tests/test_move_pairs32_ref.py
// holds left <= 0.52 right for dropped triangles in either order of evaluation, fused or not).
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr double kPairsWide2 = 256.0;                            // bohr^2
constexpr float kPairsTiny = (float)(0.03 * 0.03 * kRcSq);
constexpr unsigned long long kEvenLanes = 0x5555555555555555ull;

__device__ __forceinline__ int pair_odd_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xf5, 0xf, 0xf, true); }    // quad_perm:[1,1,3,3]
__device__ __forceinline__ float pair_even_f32(float v) { return __int_as_float(pair_even_i32(__float_as_int(v))); }
__device__ __forceinline__ float pair_odd_f32(float v) { return __int_as_float(pair_odd_i32(__float_as_int(v))); }

// Returns the rows a (bit a) of the group's queues that the FP64 pair loop has to serve: wave-uniform.  (px, py, pz) = this lane's
// position (the old one in the even lane, the trial one in the odd lane); every lane of the wavefront is active.
template <typename ImageFn>
__device__ __forceinline__ uint32_t lanes_pairs32(ImageFn image, const uint32_t (&ent)[kLaneWalk], int side, int nq,
                                                  double px, double py, double pz)
{
    const int left = nq - side;                                  // (entry c of this lane is live when 2c < left, as in lanes_park)
    int nqmax = 0;                                               // the group's longest queue (scalar)
#pragma unroll
    for (int c = 0; c < kLaneWalk; ++c) {
        const unsigned long long m = __ballot(2 * c < left);
        if (m & kEvenLanes) nqmax = 2 * c + 1;
        if (m & ~kEvenLanes) nqmax = 2 * c + 2;
    }
    if (nqmax < 2) return 0u;
    const int cmax = (nqmax + 1) >> 1;                           // registers in use
    const double ox = pair_even_f64(px), oy = pair_even_f64(py), oz = pair_even_f64(pz);          // P
    const double nx = pair_odd_f64(px), ny = pair_odd_f64(py), nz = pair_odd_f64(pz);             // P'
    bool wide = dist2(nx - ox, ny - oy, nz - oz) > kPairsWide2;
    float vx[kLaneWalk], vy[kLaneWalk], vz[kLaneWalk];
    f32x2 qq[kLaneWalk];                                         // (Qo, Qn)
#pragma unroll
    for (int c = 0; c < kLaneWalk; ++c) {
        if (c >= cmax) continue;                                 // (wave-uniform; no `break`: the loop unrolls)
        const bool live = 2 * c < left;
        double qx, qy, qz;
        image(live ? ent[c] : 0u, qx, qy, qz);
        const double dx = qx - ox, dy = qy - oy, dz = qz - oz;
        const double Qo = dist2(dx, dy, dz), Qn = dist2(qx - nx, qy - ny, qz - nz);
        vx[c] = live ? (float)dx : __builtin_nanf("");
        vy[c] = (float)dy; vz[c] = (float)dz;
        qq[c] = f32x2{(float)Qo, (float)Qn};
        wide = wide || (live && fminf(qq[c].x, qq[c].y) < kPairsTiny);
    }
    if (__ballot(wide) != 0ull) return ~0u;

    constexpr float kThin32 = (float)(1.0 - 0.98 * 0.98), kNear32 = (float)(kRcSq * (1.0 + 1e-5));
    uint32_t rows = 0u;
#pragma unroll
    for (int a = 0; a + 1 < kLaneQueue; ++a) {                   // (unrolled: a, and with it the owner's lane and register, are constants)
        if (a + 1 >= nqmax) continue;
        const int k = a >> 1;
        const bool odd = (a & 1) != 0;
        auto from = [&](float v) { return odd ? pair_odd_f32(v) : pair_even_f32(v); };
        const float ax = from(vx[k]), ay = from(vy[k]), az = from(vz[k]);
        const f32x2 Q = {from(qq[k].x), from(qq[k].y)};
        const f32x2 hQ = 0.5f * Q;
        bool fire = false;
#pragma unroll
        for (int c = (a + 1) >> 1; c < kLaneWalk; ++c) {         // (c = k of an even a: the odd lane's pair (a, a + 1) alone)
            if (c >= cmax) continue;
            const float dx = vx[c] - ax, dy = vy[c] - ay, dz = vz[c] - az;
            const float S = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            const f32x2 R = qq[c], S2 = {S, S};
            const f32x2 th = 0.5f * (R - S2) + hQ, QR = Q * R, QS = Q * S2, RS = R * S2;
            const f32x2 left = QR - th * th;
            const bool thin = left.x <= kThin32 * fmaxf(fmaxf(QR.x, QS.x), RS.x) || left.y <= kThin32 * fmaxf(fmaxf(QR.y, QS.y), RS.y);
            const bool mine = 2 * c > a || side != 0;            // 2c + side > a
            fire = fire || (mine && S < kNear32 && thin);
        }
        if (__ballot(fire) != 0ull) rows |= 1u << a;
    }
    return rows;
}

// One group: this lane's request is molecule `i` (row length n_i; 0 = no request in this lane), its row `rowp` = LM + i * kRow, and
// (px, py, pz) the position this lane evaluates: the old one in the even lane, the trial one in the odd lane.  `wq` = the
// wavefront's queue words, `qn` = its 32 queue lengths (bytes).  `walk` (wave-uniform): every request of the group comes with the
// length of its queue, `nq_key` -- at most kLaneQueue, and no molecule lists itself: the count pass has taken those requests out --
// and `ent` = what lanes_entries loaded for this lane; else `ent[0..3]` = the first four entries of the row, and phase 1 scans it.
// Returns false when the request is declined (the same answer in both lanes of a pair); else `E` = the local energy at this lane's
// position and, when `count` (wave-uniform), `ci` / `cs` = its interactions and list slots.  `gate` (wave-uniform): THE GATE above;
// `pairs32` (wave-uniform): a walking group runs THE F32 PAIR GATE in front of it.
template <typename PosFn, typename IvFn, typename NnFn>
__device__ __forceinline__ bool move_energy_mom_lanes(PosFn getpos, IvFn getiv, NnFn nnof, const uint32_t* __restrict__ rowp,
                                                      const double* __restrict__ MOM, uint32_t* __restrict__ wq, unsigned char* __restrict__ qn,
                                                      int i, int n_i, bool walk, int nq_key, const uint32_t (&ent)[kLaneWalk],
                                                      double px, double py, double pz,
                                                      int lane, bool count, bool gate, bool pairs32, double& E, unsigned int& ci, unsigned int& cs)
{
    const int r = lane >> 1, side = lane & 1;
    auto image = [&](uint32_t e, double& qx, double& qy, double& qz) { lanes_image(getpos, getiv, e, qx, qy, qz); };

    // ---- phase 1: the entries in range of either position into the queue, from the mask's loads or by the scan --------------------
    int nq;
    bool decl = false;
    if (walk) {
        lanes_park(wq, r, side, nq_key, ent);
        wave_fence();
        nq = nq_key;
    } else {
        int cnt = 0;
        bool self = false;
        uint32_t none = 0u;
        lanes_scan<true>(image, rowp, wq, r, side, i, n_i, make_uint4(ent[0], ent[1], ent[2], ent[3]), px, py, pz, cnt, self, none);
        decl = self || cnt > kLaneQueue;
        if (side == 0) qn[r] = (unsigned char)(cnt < kLaneQueue ? cnt : kLaneQueue);
        wave_fence();
        nq = (int)qn[r];
    }

    // ---- the 0.99 rule: the queue's pairs, shared between the two lanes --------------------------------------------------------
    bool hard = false;
    constexpr double kThin = 1.0 - 0.98 * 0.98;
    auto thin = [&](double Q, double R, double S) {              // (the header: QR - (t/2)^2 <= kThin max(QR, QS, RS))
        const double th = __builtin_fma(0.5, R - S, 0.5 * Q), QR = Q * R;
        return __builtin_fma(-th, th, QR) <= kThin * fmax(fmax(QR, Q * S), R * S);
    };
    // (a walking group behind THE F32 PAIR GATE: only the rows that gate names)
    const uint32_t rows = walk && gate && pairs32 ? lanes_pairs32(image, ent, side, nq, px, py, pz) : ~0u;
    const double tx = pair_swap_f64(px), ty = pair_swap_f64(py), tz = pair_swap_f64(pz);           // P': the partner's position
    for (int a = 0; (rows >> a) != 0u && __ballot(a + 1 < nq) != 0ull; ++a) {
        if (!(rows >> a & 1u)) continue;
        double ax, ay, az;
        image(a + 1 < nq ? wq[a * 32 + r] : 0u, ax, ay, az);
        double Q = 0.0, Qt = 0.0;
        if (gate) { Q = dist2(ax - px, ay - py, az - pz); Qt = dist2(ax - tx, ay - ty, az - tz); }
        for (int b0 = a + 1; __ballot(b0 < nq) != 0ull; b0 += 2) {
            const int b = b0 + side;
            const bool live = b < nq;
            double bx, by, bz;
            image(live ? wq[b * 32 + r] : 0u, bx, by, bz);
            const double dx = bx - ax, dy = by - ay, dz = bz - az;                                 // a -> b
            const double r2ab = dist2(dx, dy, dz);
            const bool near = live && r2ab < kRcSq;
            bool fire = near;
            if (gate) fire = near && (thin(Q, dist2(bx - px, by - py, bz - pz), r2ab) || thin(Qt, dist2(bx - tx, by - ty, bz - tz), r2ab));
            if (__ballot(fire) != 0ull) {                        // wave-uniform: every lane is in here, and the exchange below is sound
                const int fire_o = pair_swap_i32(fire ? 1 : 0);
                const double ox = pair_swap_f64(bx), oy = pair_swap_f64(by), oz = pair_swap_f64(bz);   // the partner's b
                constexpr double kC2 = (0.99 - 1e-9) * (0.99 - 1e-9);
                auto angles = [&](bool on, double cx, double cy, double cz) {
                    const double ex = cx - ax, ey = cy - ay, ez = cz - az;                             // a -> b
                    const double r2e = dist2(ex, ey, ez);
                    const double Ax = ax - px, Ay = ay - py, Az = az - pz, Bx = cx - px, By = cy - py, Bz = cz - pz;
                    const double r2a = dist2(Ax, Ay, Az), r2b = dist2(Bx, By, Bz);
                    if (on && r2a < kRcSq && r2b < kRcSq) {
                        const double da = -(Ax * ex + Ay * ey + Az * ez), db = Bx * ex + By * ey + Bz * ez;   // (a->P).(a->b), (b->P).(b->a)
                        const double dc = Ax * Bx + Ay * By + Az * Bz;                                    // (P->a).(P->b)
                        hard = hard || (da > 0.0 && da * da >= kC2 * (r2a * r2e)) || (db > 0.0 && db * db >= kC2 * (r2b * r2e)) ||
                               (dc > 0.0 && dc * dc >= kC2 * (r2a * r2b));
                    }
                };
                angles(fire, bx, by, bz);
                angles(fire_o != 0, ox, oy, oz);
            }
        }
    }

    // ---- phase 2: over the queue ------------------------------------------------------------------------------------------------
    MomentSums ms;
    double t3 = 0.0;
    unsigned int packed = (unsigned int)n_i;
    for (int k = 0; __ballot(k < nq) != 0ull; ++k) {
        const bool live = k < nq;
        const uint32_t e = live ? wq[k * 32 + r] : 0u;
        const int j = (int)(e & kJMask);
        double qx, qy, qz;
        image(e, qx, qy, qz);
        const double ax = qx - px, ay = qy - py, az = qz - pz;                                     // :272
        const double r2 = dist2(ax, ay, az);
        const bool in = live && r2 < kRcSq;                                                        // :276
        // From here on NOTHING is conditional: an entry out of this lane's range goes through the same arithmetic with g = e1 = 0, which
        // adds exact zeros to every sum (the lane's bits do not change), and the compiler has no branch to turn into selects that
        // keep two copies of twenty running sums alive.  (Such a lane reads the moments of a molecule it has no use for: harmless.)
        double M[10];
        load_moments(MOM + (size_t)j * kMomStride, M);
                                 // (used after the pair terms)
        double rinv, e1, g;
        pair_terms(in ? r2 : kRcSq, rinv, e1, g);                                                  // (out of range: finite values of no use)
        e1 = in ? e1 : 0.0; g = in ? g : 0.0;
        const double vx = -ax * rinv, vy = -ay * rinv, vz = -az * rinv;                            // unit vector j -> i, this position
        // i's own term inside j's moments belongs to the OLD position (the one the full-box pass saw): the even lane's g (0 when j was
        // out of range there) and unit vector
        const double g_old = pair_even_f64(g), ux = pair_even_f64(vx), uy = pair_even_f64(vy), uz = pair_even_f64(vz);
        ms.add(ax, ay, az, rinv, e1, g);                                                          // :294-297, and i's arm for the j--i--k sum
        double S0 = M[0], S1x = M[1], S1y = M[2], S1z = M[3];
        double Sxx = M[4], Syy = M[5], Sxy = M[6], Sxz = M[7], Syz = M[8];
        double Szz = (S0 - Sxx) - Syy;                           // (trace of sum g u u^T = sum g)
        {                            // one `m -= h * u` expression per component, as moments_arm<-1>
            const double hx = g_old * ux, hy = g_old * uy, hz = g_old * uz;
            S0 -= g_old; S1x -= hx; S1y -= hy; S1z -= hz;
            Sxx -= hx * ux; Syy -= hy * uy; Szz -= hz * uz; Sxy -= hx * uy; Sxz -= hx * uz; Syz -= hy * uz;
        }
        const double wx = Sxx * vx + Sxy * vy + Sxz * vz, wy = Sxy * vx + Syy * vy + Syz * vz, wz = Sxz * vx + Syz * vy + Szz * vz;
        const double quad = vx * wx + vy * wy + vz * wz, lin = vx * S1x + vy * S1y + vz * S1z;
        t3 += g * ((quad - 2.0 * kCos0 * lin) + kCos0 * kCos0 * S0);                                   // :324-343,385-387 summed over k
        if (count) {                 // one word: in-range neighbours << 27 | their other neighbours << 14 | their rows' slots (<= 16, 16 x 64, 17 x 64)
            const bool in_old = pair_even_i32(in ? 1 : 0) != 0;
            packed += in ? (1u << 27) + (((unsigned int)(M[9] + 0.5) - (in_old ? 1u : 0u)) << 14) + (unsigned int)nnof(j) : 0u;
        }
    }
    {   // the j--i--k sum (:302-318) from the lane's own sums, as MomentSums::finish
#pragma clang fp contract(off)
        const double D2 = dist2(ms.Sxx, ms.Syy, ms.Szz), O2 = dist2(ms.Sxy, ms.Sxz, ms.Syz);
        const double F2 = __builtin_fma(2.0, O2, D2);
        const double F1 = dist2(ms.S1x, ms.S1y, ms.S1z);
        const double A = F2 - ms.Q, B = F1 - ms.Q, C = __builtin_fma(ms.S0, ms.S0, -ms.Q);
        const double T = 0.5 * __builtin_fma(kCos0 * kCos0, C, __builtin_fma(-2.0 * kCos0, B, A));
        E = __builtin_fma(kLamEps, t3 + T, ms.e2);                                                 // :397
    }
    // (every pair of the lane's in-range neighbours contributes a j--i--k triplet: anything else was declined)
    const unsigned int nin = packed >> 27;
    ci = nin + nin * (nin - 1u) / 2u + ((packed >> 14) & 0x1fffu);
    cs = packed & 0x3fffu;
    decl = decl || hard;
    const int decl_other = pair_swap_i32(decl ? 1 : 0);
    return !(decl || decl_other != 0);
}

}  // namespace mw
