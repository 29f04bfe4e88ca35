// mw_move_energy.hip.h -- gfx950 (MI355X, CDNA4) device code of the mW energy engine:
// compute_local_real_energy (molint.F90:220-404) and the fused old/new evaluation of a trial move.  The routines live in
//   mw_local_energy.hip.h   local_energy_wave, local_energy_wave_batched
//   mw_move_scan.hip.h      move_energy_wave (WaveScratch, the stamp arrays)
//   mw_move_moments.hip.h   move_energy_mom_wave, moments_commit
//   mw_move_lanes.hip.h     move_energy_mom_lanes
//   mw_local_server.hip.h   k_local_server
// and the kernels k_move_energy, k_move_fallback and k_local_energy_single here (non-template kernels enter the code object in
// the order of their definitions, which this file keeps).
#pragma once
#include <type_traits>

#include "mw_common.hip.h"
#include "mw_local_energy.hip.h"
#include "mw_move_scan.hip.h"
#include "mw_move_moments.hip.h"
#include "mw_move_lanes.hip.h"

namespace mw {

// One workgroup per work item {box, first request, last request+1}: the requests are
// sorted by box on upload, so the workgroup stages that box's positions in LDS once
// (LDSPOS) and its 16 wavefronts then serve the item's requests from LDS gathers.
//   mode bit 0: write e_old (mirrored positions), bit 1: write e_new (trial position), bit 2: the declined list's count word
//   MOMPATH only -- bit 3: count (the interactions and slots of the served requests, summed per item into `mtot`, and the zero words
//   of `counts`: without it the launch computes and writes nothing of them), bit 4: no energy output (nothing written to e_old or
//   e_new, nothing appended to `declined`: the pass that counts on demand, mw_moves_counts), bit 5: sort the item's requests by
//   their number of in-range neighbours before evaluating them (below; MW_MOVE_SORT=0 clears it), bit 6: the pass that counts for
//   the sort keeps every request's row-slot mask, and a group rebuilds its queues from the masks instead of scanning the rows again
//   (THE MASK WALK, mw_move_lanes.hip.h; only where bit 5 sorts; MW_MOVE_MASKS=0 clears it), bit 7: the 0.99 rule's pair pass enters
//   its angle block only for pairs that pass THE GATE (mw_move_lanes.hip.h; MW_MOVE_GATE=0 clears it: every pair with |ab| < cutoff),
//   bit 8: a group that walks the masks runs THE F32 PAIR GATE from its registers first, and the pair pass serves only the queue rows
//   that names (mw_move_lanes.hip.h; only with bit 7; MW_MOVE_PAIRS32=0 clears it)
constexpr int kMoveChunk = 2048;   // requests per work item when the box is staged in LDS

// MOMPATH keeps an item's requests in LDS as 32-bit KEYS: molecule | request index in the item << 13 | nq << 24, nq = the entries
// of the molecule's row in range of the old or the trial position -- what phase 1 of move_energy_mom_lanes queues -- or kKeyNqOver
// for a request that routine declines at once (more than kLaneQueue of them, or a molecule that lists itself).
constexpr int kKeyMolBits = 13, kKeyReqBits = 11, kKeyNqBits = 5;          // (molecules: N <= 4372 where the box is staged, mw_host_ctx.hip.h)
constexpr int kKeyReqShift = kKeyMolBits, kKeyNqShift = kKeyMolBits + kKeyReqBits;
constexpr uint32_t kKeyMolMask = (1u << kKeyMolBits) - 1u, kKeyReqMask = (1u << kKeyReqBits) - 1u;
constexpr int kKeyNqOver = kLaneQueue + 1;
constexpr int kSortBins = kKeyNqOver + 1;                                  // nq = 0 .. kLaneQueue, and kKeyNqOver
constexpr int kSortChunks = kMoveChunk / 64;                               // a wavefront ranks 64 keys at a time
static_assert(kMoveChunk <= (1 << kKeyReqBits) && kKeyNqOver < (1 << kKeyNqBits) && kKeyNqShift + kKeyNqBits <= 32, "the key's fields");
static_assert(kSortChunks == 2 * 16, "two rounds of the sixteen wavefronts rank an item's keys: chunks v and v + 16 in wavefront v");
static_assert((kSortChunks + 1) * kSortBins * sizeof(uint32_t) <= 16 * sizeof(WaveScratch), "the sort's tables are overlaid on the idle queues");
// MOMPATH's use of the sixteen WaveScratch blocks: the queues of wavefront v at byte v * kQueueBytes, and behind the sixteen queues
// the item's row-slot masks (mode bit 6), one word per request, indexed by the request's index in the item as uploaded.
constexpr size_t kQueueBytes = kLaneQueueWords * sizeof(uint32_t);
constexpr size_t kMaskTableAt = 16 * kQueueBytes;
static_assert(kMaskTableAt + kMoveChunk * sizeof(uint32_t) <= 16 * sizeof(WaveScratch), "the queues and the mask table fit the scratch blocks: no new LDS");
static_assert((kSortChunks + 1) * kSortBins * sizeof(uint32_t) <= kMaskTableAt, "the sort's tables lie on the queues and end before the masks");
static_assert(kMaskTableAt % 16 == 0 && kQueueBytes % 16 == 0, "alignment of the queues and of the mask table");

// (LAYOUT: SoA measures 1.4 % faster than the paired layout here -- 1288 vs 1306 us, tools/kbench -- now that the scan
// reads one vector less per slot; the full-box kernel keeps the paired layout, where it is the faster one)
// MOMPATH = true (with LDSPOS, SELFIMG = false): the moment path above, a lane pair per request (move_energy_mom_lanes); `mom` = the box
// moments [box][N][kMomStride] of the launch's boxes.
template <bool LDSPOS, int LAYOUT = kLayoutSoA, bool SELFIMG = true, bool MOMPATH = false>
__global__ __launch_bounds__(1024)
void k_move_energy(const double* __restrict__ pos, const double* __restrict__ ivect,
                   const int* __restrict__ nivect, const uint32_t* __restrict__ listm,
                   const int* __restrict__ nn, const int4* __restrict__ work,
                   const int* __restrict__ req_imol, const double* __restrict__ req_trial,
                   const int* __restrict__ perm,
                   double* __restrict__ e_old, double* __restrict__ e_new,
                   unsigned int* __restrict__ counts,   // [nreq][4]: inter_old, slots_old, inter_new, slots_new
                   int* __restrict__ declined,          // [0], [1] = number of requests left to k_move_fallback (the word of this launch's parity,
                                                        // mode bit 2), then {request, box} pairs
                   int N, int ivcap, int mode, const double* __restrict__ mom = nullptr,
                   unsigned int* __restrict__ mtot = nullptr)   // MOMPATH: [work item][4] = {interactions old, slots old, interactions new, slots new} of the item's served requests
{
    static_assert(!MOMPATH || (LDSPOS && !SELFIMG), "the moment path serves boxes staged in LDS whose cells hold no self-images");
    // (the moment build's static LDS is what it was when a 552-byte pair table stood here: 512 of the bytes are the queue lengths of
    //  the sixteen wavefronts' 32 requests)
    __shared__ unsigned char s_qn[MOMPATH ? kCap * (kCap - 1) : 2];
    unsigned int acc[4] = {0u, 0u, 0u, 0u};
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int4 w = work[blockIdx.x];
    const int b = w.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool count = !MOMPATH || (mode & 8) != 0, quiet = MOMPATH && (mode & 16) != 0;
    const double* P  = pos + (size_t)b * N * 3;
    const double* IV = ivect + (size_t)b * ivcap * 3;
    const uint32_t* LM = listm + (size_t)b * N * kRow;
    const int* NN = nn + (size_t)b * N;
    const int niv = nivect[b];

    // dynamic LDS: [positions when LDSPOS][image vectors][16 wave scratches] and, when LDSPOS, [row lengths, one
    // byte per molecule][the molecules of the item's requests]; positions and image vectors in the layout LAYOUT
    // (LdsVecs, mw_common.hip.h: the paired layout gathers a vector in 6 LDS cycles instead of 10)
    double* spos = smem;
    double* siv = smem + (LDSPOS ? lds_vec_bytes((size_t)N) / 8 : 0);
    WaveScratch* ws = reinterpret_cast<WaveScratch*>(siv + lds_vec_bytes((size_t)ivcap) / 8) + wave;
    unsigned char* snn = reinterpret_cast<unsigned char*>(reinterpret_cast<WaveScratch*>(siv + lds_vec_bytes((size_t)ivcap) / 8) + 16);
    int* simol = reinterpret_cast<int*>(snn + (((size_t)N + 7) & ~(size_t)7));
    __shared__ int s_next;                                                   // next request nobody has taken yet
    const int nreq = w.z - w.y;                                              // <= kMoveChunk when LDSPOS
    const double iv_first = stage_iv_begin<1024>(IV, niv, tid);
    if (LDSPOS) {
        // every staging load of the item in flight before the first wait (a loop of load / wait / store per element costs a
        // dozen HBM round trips in a row): row lengths and request molecules first, into registers, then the box
        constexpr int kB = 4;
        for (int base = 0; base < N; base += kB * 1024) {
            int v[kB];
#pragma unroll
            for (int k = 0; k < kB; ++k) { const int t = base + tid + k * 1024; v[k] = NN[t < N ? t : N - 1]; }
#pragma unroll
            for (int k = 0; k < kB; ++k) { const int t = base + tid + k * 1024; if (t < N) snn[t] = (unsigned char)v[k]; }   // maxneigh <= 64
        }
        for (int base = 0; base < nreq; base += kB * 1024) {
            int v[kB];
#pragma unroll
            for (int k = 0; k < kB; ++k) { const int t = base + tid + k * 1024; v[k] = req_imol[w.y + (t < nreq ? t : nreq - 1)]; }
#pragma unroll
            for (int k = 0; k < kB; ++k) {                       // (MOMPATH: as keys, nq = 0)
                const int t = base + tid + k * 1024;
                if (t < nreq) simol[t] = MOMPATH ? (int)((uint32_t)v[k] | (uint32_t)t << kKeyReqShift) : v[k];
            }
        }
        stage_vecs<LAYOUT, 1024>(spos, P, N, N, tid);
        if (tid == 0) s_next = 16;
    }
    stage_iv_end<LAYOUT, 1024>(siv, IV, niv, ivcap, tid, iv_first);
    __syncthreads();

    const LdsVecs<LAYOUT> vpos{spos, N}, viv{siv, ivcap};
    auto getiv = [&](int k, double& x, double& y, double& z) { viv.get(k, x, y, z); };
    auto getpos = [&](int jx, double& x, double& y, double& z) {
        if constexpr (LDSPOS) vpos.get(jx, x, y, z);
        else { const double* p = P + 3 * (size_t)jx; x = p[0]; y = p[1]; z = p[2]; }
    };
    auto row = [&](int jx, int sl) { return LM[(size_t)jx * kRow + sl]; };
    auto nnof = [&](int jx) { return LDSPOS ? (int)snn[jx] : NN[jx]; };
    auto imol_of = [&](int q) { return LDSPOS ? simol[q] : req_imol[w.y + q]; };

    // Requests are handed out dynamically: the first sixteen go to the sixteen wavefronts, after that a wavefront
    // takes the next untaken one (an LDS counter) when it STARTS a request, and fetches entry (lane & 31) of that
    // molecule's own row right away -- a request never begins by waiting on memory, and a wavefront that drew
    // cheap requests simply serves more of them (static dealing left ~8 % of the wave-time idle at the item's end).
    // (Without LDS staging an item holds at most 16 requests: one per wavefront.)
    // What a request brings with it from global memory -- entry (lane & 31) of its molecule's row, its trial position (lane c < 3
    // holds component c) and its slot in the caller's order, perm[] -- is asked for ONE REQUEST AHEAD with vector loads: the
    // addresses of the last two are the same in every lane, and as scalar loads they would share their counter with the LDS reads,
    // which return in another order -- the next LDS read would wait for them, at the start of the evaluation they were meant to
    // hide behind (in_lanes() keeps the compiler from seeing that).  They are first used after the evaluation.  (On the moment path
    // the evaluation's own wait for the moments, ~130 instructions on, takes them in: the vector-memory counter counts in order and
    // they were issued first.  What is gained there is that nothing waits for them at the request's START.)
    // (Offsets in 32 bits, so that the loads take a scalar base: mw_moves_upload's request count is an int, and 3 x it as unsigned
    // holds up to 1.4e9 requests -- 34 GB of trial positions.)
    auto in_lanes = [](int v) { asm volatile("" : "+v"(v)); return v; };
    auto fetch = [&](int q, int& i_, uint32_t& e_, double& t_, int& o_) {
        i_ = 0; e_ = 0u; t_ = 0.0; o_ = 0;
        if (q < nreq) {
            const int m_ = in_lanes(w.y + q);
            i_ = imol_of(q); e_ = row(i_, lane & 31);
            if (mode & 2) t_ = req_trial[3u * (unsigned)m_ + (lane < 3 ? (unsigned)lane : 0u)];
            o_ = perm[(unsigned)m_];
        }
    };
    if constexpr (MOMPATH) {
        // THE MOMENT PATH (mw_move_lanes.hip.h): a wavefront serves GROUPS of 32 requests of the item, lanes 2r and 2r + 1 request r of
        // the group at the old and at the trial position; the ticket hands out groups, the first sixteen to the sixteen wavefronts.
        //
        // WHICH 32.  The loops of the 0.99 rule and of phase 2 run for the longest queue among a group's requests, and on thermal ice a
        // request queues 4 to 15 entries (9.2 on average): 32 consecutive requests hold a 13 or 14 nearly every time.  So an item of
        // more than one group (mode bit 5) first COUNTS -- every wavefront runs phase 1's scan over its share of the groups, storing
        // nothing, and writes each request's nq into its key -- then SORTS its keys by nq, longest first, stable in the request index
        // (a counting sort over kSortBins bins; its tables lie on the queues, idle until then; four workgroup barriers per item, none
        // in the loop below), and a lane takes its request from the sorted table: the ticket hands out the longest groups first, so the
        // item ends on its cheapest.  Requests of nq = kKeyNqOver sort behind all others, are appended to the declined list here and are
        // left out of the groups.  A request's bits are its own (mw_move_lanes.hip.h), so none of this changes a result.
        // (Cheaper keys do not separate the requests -- bench walkers 0-2, phase-2 / pair-pass trips per item of 2048: 812 / 2577 as
        //  uploaded, 594 / 1424 by nq; 782 / 2400 by the old position's in-range count, 809 / 2558 by row length, 751 / 2248 by a
        //  bound from the displacement.)
        //
        // What a request brings from global memory -- its slot in the caller's order, its trial position, and of its molecule's row the
        // entries its mask names (a group that walks the masks, below) or the first four (a group that scans) -- each lane asks for
        // itself with vector loads, for the NEXT group, before the current group's result stores: the stores wait for nothing, and the
        // loads are in flight across them and the ticket.  The count pass asks one group ahead too.
        uint32_t* wq = reinterpret_cast<uint32_t*>(ws - wave) + wave * kLaneQueueWords;
        uint32_t* smask = reinterpret_cast<uint32_t*>(ws - wave) + kMaskTableAt / sizeof(uint32_t);
        unsigned char* qn = s_qn + wave * 32;
        const double* MOM = mom + (size_t)b * N * kMomStride;
        const int rq = lane >> 1, side = lane & 1;
        uint32_t* skey = reinterpret_cast<uint32_t*>(simol);
        int nserve = nreq;                                        // the requests the groups hold: the first `nserve` keys
        if ((mode & 32) && nreq > 32) {
            // ---- count: wavefront v takes groups v, v + 16, ... of the item as uploaded; only it reads or writes their keys ----
            const int ngrp_up = (nreq + 31) >> 5;
            auto image = [&](uint32_t e, double& qx, double& qy, double& qz) { lanes_image(getpos, getiv, e, qx, qy, qz); };
            auto cfetch = [&](int grp, uint32_t& k_, double (&t_)[3], uint4& c_) {
                k_ = 0u; t_[0] = t_[1] = t_[2] = 0.0; c_ = make_uint4(0u, 0u, 0u, 0u);
                const int q = grp * 32 + rq;
                if (q < nreq) {                                   // (a lane past the item's end: molecule 0, no slots)
                    const unsigned m_ = (unsigned)(w.y + q);
                    k_ = skey[q];
                    c_ = *reinterpret_cast<const uint4*>(LM + (size_t)(k_ & kKeyMolMask) * kRow);
                    if (mode & 2) { t_[0] = req_trial[3u * m_]; t_[1] = req_trial[3u * m_ + 1u]; t_[2] = req_trial[3u * m_ + 2u]; }
                }
            };
            uint32_t k; double t[3]; uint4 c4;
            cfetch(wave, k, t, c4);
            for (int grp = wave; grp < ngrp_up; grp += 16) {
                uint32_t k_nx; double t_nx[3]; uint4 c_nx;
                cfetch(grp + 16, k_nx, t_nx, c_nx);
                const int q = grp * 32 + rq;
                const int i = (int)(k & kKeyMolMask);
                double px, py, pz;
                getpos(i, px, py, pz);
                if ((mode & 2) && side) { px = t[0]; py = t[1]; pz = t[2]; }
                const int n_i = q < nreq ? min(nnof(i), kRow) : 0;
                int cnt = 0;
                bool self = false;
                uint32_t msk = 0u;
                lanes_scan<false>(image, LM + (size_t)i * kRow, wq, rq, side, i, n_i, c4, px, py, pz, cnt, self, msk);
                if (q < nreq && side == 0) {
                    skey[q] = k | (uint32_t)(self || cnt > kLaneQueue ? kKeyNqOver : cnt) << kKeyNqShift;
                    if (mode & 64) smask[q] = n_i > 32 ? kMaskScan : msk;   // (q = the request's index in the item as uploaded)
                }
                k = k_nx; t[0] = t_nx[0]; t[1] = t_nx[1]; t[2] = t_nx[2]; c4 = c_nx;
            }
            __syncthreads();
            // ---- sort: chunk ch = 64 consecutive keys, wavefront v ranks chunks v and v + 16 (only the item's `nch`: an item of up
            //      to 1024 requests has one round, and nothing is done for chunks it does not have); tab[ch][bin] = the chunk's keys of that bin, then the
            //      number of such keys in earlier chunks; tab[kSortChunks][bin] = where the bin starts in the sorted table ----
            uint32_t* tab = reinterpret_cast<uint32_t*>(ws - wave);
            const int nch = (nreq + 63) >> 6;
            uint32_t key[2] = {0u, 0u};
            int rank[2] = {0, 0};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int ch = wave + 16 * h, q = ch * 64 + lane;
                if (ch >= nch) continue;                          // (wave-uniform)
                key[h] = q < nreq ? skey[q] : 0u;
                const int bin = q < nreq ? (int)(key[h] >> kKeyNqShift) : -1;
                unsigned int mine = 0u;
#pragma nounroll
                for (int bn = 0; bn < kSortBins; ++bn) {          // (rolled: unrolled, the masks of all bins are held at once, in registers the main loop then lacks)
                    const unsigned long long m = __ballot(bin == bn);
                    if (bin == bn) rank[h] = __popcll(m & ((1ull << lane) - 1ull));   // the same bin in lower lanes: earlier requests
                    if (lane == bn) mine = (unsigned int)__popcll(m);
                }
                if (lane < kSortBins) tab[ch * kSortBins + lane] = mine;
            }
            __syncthreads();
            if (wave == 0) {                                      // lane l < kSortBins: the bin at place l of the order kLaneQueue .. 0, kKeyNqOver
                const int bin = lane <= kLaneQueue ? kLaneQueue - lane : kKeyNqOver;
                unsigned int run = 0u;
                if (lane < kSortBins) {
#pragma unroll
                    for (int ch = 0; ch < kSortChunks; ++ch)
                        if (ch < nch) { const unsigned int c = tab[ch * kSortBins + bin]; tab[ch * kSortBins + bin] = run; run += c; }
                }
                unsigned int at = 0u;
#pragma nounroll
                for (int l = 0; l + 1 < kSortBins; ++l) { const unsigned int tl = (unsigned int)__builtin_amdgcn_readlane((int)run, l); if (lane > l) at += tl; }
                if (lane < kSortBins) tab[kSortChunks * kSortBins + bin] = at;
            }
            __syncthreads();
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int ch = wave + 16 * h;
                if (ch * 64 + lane < nreq) {
                    const int bin = (int)(key[h] >> kKeyNqShift);
                    skey[tab[kSortChunks * kSortBins + bin] + tab[ch * kSortBins + bin] + (unsigned int)rank[h]] = key[h];
                }
            }
            nserve = __builtin_amdgcn_readfirstlane((int)tab[kSortChunks * kSortBins + kKeyNqOver]);
            __syncthreads();                                      // (the sorted keys stand, and the tables are queues again)
            if (!quiet)
                for (int p = nserve + tid; p < nreq; p += 1024) {
                    const int k2 = atomicAdd(&declined[(mode >> 2) & 1], 1);
                    declined[2 + 2 * k2] = w.y + (int)((skey[p] >> kKeyReqShift) & kKeyReqMask); declined[3 + 2 * k2] = b;
                }
        }
        const int ngrp = (nserve + 31) >> 5;
        // A group WALKS THE MASKS (mw_move_lanes.hip.h) when the item was counted and sorted above with mode bit 6 and none of its
        // requests holds kMaskScan; else it scans its rows as the count pass did.  The decision is the wavefront's, made where the
        // group is fetched: a walking group's lanes bring the row entries at their set bits, up to kLaneWalk each, a scanning group's
        // the first four entries of their rows -- in the same registers.  (A lane past the end has an empty mask and loads nothing.)
        const bool masks = (mode & 64) && (mode & 32) && nreq > 32;
        auto fetch = [&](int grp, uint32_t& k_, int& o_, double (&t_)[3], uint32_t (&e_)[kLaneWalk], bool& walk_) {
            k_ = 0u; o_ = 0; t_[0] = t_[1] = t_[2] = 0.0; walk_ = false;
#pragma unroll
            for (int c = 0; c < kLaneWalk; ++c) e_[c] = 0u;
            if (grp < ngrp) {
                k_ = skey[min(grp * 32 + rq, nserve - 1)];        // (a lane past the end repeats the last request and serves nothing)
                const unsigned m_ = (unsigned)w.y + ((k_ >> kKeyReqShift) & kKeyReqMask);
                const unsigned at = (k_ & kKeyMolMask) * (unsigned)kRow;
                if (masks) {
                    const uint32_t msk = grp * 32 + rq < nserve ? smask[(k_ >> kKeyReqShift) & kKeyReqMask] : 0u;
                    walk_ = __ballot(msk == kMaskScan) == 0ull;
                    if (walk_) lanes_entries(LM, at, msk, side, e_);
                }
                if (!walk_) {
                    const uint4 c_ = *reinterpret_cast<const uint4*>(LM + at);
                    e_[0] = c_.x; e_[1] = c_.y; e_[2] = c_.z; e_[3] = c_.w;
                }
                if (mode & 2) { t_[0] = req_trial[3u * m_]; t_[1] = req_trial[3u * m_ + 1u]; t_[2] = req_trial[3u * m_ + 2u]; }
                o_ = perm[m_];
            }
        };
        int cur = wave;
        uint32_t k; int o; double t[3]; uint32_t e8[kLaneWalk]; bool walk;
        fetch(cur, k, o, t, e8, walk);
        while (cur < ngrp) {
            int nxt = 0;
            if (lane == 0) nxt = __hip_atomic_fetch_add(&s_next, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            nxt = __builtin_amdgcn_readfirstlane(nxt);
            uint32_t k_nx; int o_nx; double t_nx[3]; uint32_t e_nx[kLaneWalk]; bool walk_nx;
            const bool valid = cur * 32 + rq < nserve;
            const int i = (int)(k & kKeyMolMask);
            double px, py, pz;                                    // this lane's position: the old one, in the odd lane the trial one
            getpos(i, px, py, pz);
            if ((mode & 2) && side) { px = t[0]; py = t[1]; pz = t[2]; }
            const int n_i = valid ? min(nnof(i), kRow) : 0;
            double en = 0.0;
            unsigned int ci = 0u, cs = 0u;
            const bool served = move_energy_mom_lanes(getpos, getiv, nnof, LM + (size_t)i * kRow, MOM, wq, qn, i, n_i,
                                                      walk, valid ? (int)(k >> kKeyNqShift) : 0, e8,
                                                      px, py, pz, lane, count, (mode & 128) != 0, (mode & 256) != 0, en, ci, cs);
            // (the next group's loads leave HERE, behind the evaluation and ahead of the result stores: issued at the loop's top they
            //  are up to seventeen registers held across the evaluation, which has none to spare -- and a group starts on memory once
            //  per 32 requests, with three other wavefronts of the SIMD to fill the wait)
            fetch(nxt, k_nx, o_nx, t_nx, e_nx, walk_nx);
            if (valid && !served) {
                // (declined: more than kLaneQueue in-range neighbours, a triplet the 0.99 rule drops, a molecule that lists itself --
                //  left to k_move_fallback like the requests the scan builds decline)
                if (side == 0 && !quiet) {                        // (its index in the item: from its key again, no register across the evaluation)
                    const int k = atomicAdd(&declined[(mode >> 2) & 1], 1);
                    declined[2 + 2 * k] = w.y + (int)((skey[cur * 32 + rq] >> kKeyReqShift) & kKeyReqMask); declined[3 + 2 * k] = b;
                }
            } else if (valid) {
                const size_t so = (size_t)o;
                // (the counts of served requests go to `mtot`, summed per work item; scalar bases: a per-lane choice of pointer is two
                //  more registers held from group to group)
                if (side == 0 && (mode & 1)) { if (!quiet) e_old[so] = en; if (count) { counts[4 * so] = 0u; counts[4 * so + 1] = 0u; } }
                if (side == 1 && (mode & 2)) { if (!quiet) e_new[so] = en; if (count) { counts[4 * so + 2] = 0u; counts[4 * so + 3] = 0u; } }
                if (count) { acc[0] += ci; acc[1] += cs; }        // (this lane's side: sorted out below)
            }
            wave_fence();                                         // (the queues are the next group's)
            cur = nxt; k = k_nx; o = o_nx; t[0] = t_nx[0]; t[1] = t_nx[1]; t[2] = t_nx[2]; walk = walk_nx;
#pragma unroll
            for (int c = 0; c < kLaneWalk; ++c) e8[c] = e_nx[c];
        }
    } else {
        int cur = wave;
        int i, o; uint32_t e; double t;
        fetch(cur, i, e, t, o);
        while (cur < nreq) {
            int nxt = 0;
            if (lane == 0) nxt = __hip_atomic_fetch_add(&s_next, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            nxt = LDSPOS ? __builtin_amdgcn_readfirstlane(nxt) : nreq;
            int i_nx, o_nx; uint32_t e_nx; double t_nx;
            fetch(nxt, i_nx, e_nx, t_nx, o_nx);

            const int m = w.y + cur;
            double xo, yo, zo;
            getpos(i, xo, yo, zo);
            double xn = xo, yn = yo, zn = zo;
            if (mode & 2) { xn = readlane_f64(t, 0); yn = readlane_f64(t, 1); zn = readlane_f64(t, 2); }

            MoveRes r;
            const bool fast = move_energy_wave<SELFIMG>(getpos, getiv, row, nnof, ws, niv, i, nnof(i), e, xo, yo, zo, xn, yn, zn, lane, r);
            // (the next request's three values are taken HERE, ahead of the result stores: taken at the loop's end, the wait for them would
            //  also wait for those stores to be acknowledged, once per request)
            asm volatile("" : "+v"(e_nx), "+v"(t_nx), "+v"(o_nx));
            if (!fast) {
                // a request the fused routine declines (a row longer than 32 entries, more than kCap in-range neighbours, a
                // molecule that neighbours its own image -- never on ice) is left to k_move_fallback: with the plain routine
                // inlined here its registers counted against this loop (37 scalar registers spilled to vector lanes, ~30
                // vector instructions per request on moving them), and calling it out of line costs scratch (+8 % time)
                if (lane == 0 && !quiet) {
                    const int k = atomicAdd(&declined[(mode >> 2) & 1], 1);
                    declined[2 + 2 * k] = m; declined[3 + 2 * k] = b;
                }
            } else if (lane == 0) {
                const size_t so = (size_t)o;
                if (mode & 1) { if (!quiet) e_old[so] = r.eo; if (count) { counts[4 * so] = r.io; counts[4 * so + 1] = r.so; } }
                if (mode & 2) { if (!quiet) e_new[so] = r.en; if (count) { counts[4 * so + 2] = r.in_; counts[4 * so + 3] = r.sn; } }
            }
            cur = nxt; i = i_nx; e = e_nx; t = t_nx; o = o_nx;
        }
    }
    if constexpr (MOMPATH) if (count) {   // (the lane pairs kept their own side's two sums in acc[0], acc[1])
        if (lane & 1) { acc[2] = acc[0]; acc[3] = acc[1]; acc[0] = acc[1] = 0u; }
    }
    if constexpr (MOMPATH) if (count) {   // the item's counts: lanes -> wavefront -> workgroup, ONE plain store per item (thousands of wavefronts adding to
        __shared__ unsigned int s_tot[16][4];                              // four global words serialise: +0.3 ms on a 0.9 ms launch)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int tot = dpp_wave_sum_i32((int)acc[c]);
            if (lane == 63) s_tot[wave][c] = (unsigned int)tot;
        }
        __syncthreads();
        if (tid < 4) {
            unsigned int t = 0u;
            for (int wv = 0; wv < 16; ++wv) t += s_tot[wv][tid];
            mtot[4 * (size_t)blockIdx.x + tid] = t;
        }
    }
}

// The requests k_move_energy declined: TWO wavefronts each, one for the mirrored (old) and one for the trial position, and only the
// sides `mode` asks for.  Each evaluates with local_energy_wave_batched -- the rows and third-body positions of up to eight in-range
// neighbours in flight together: four dependent round trips to global memory where the neighbour-by-neighbour routine makes three
// per in-range neighbour, same terms in the same per-lane order -- and writes its own energy and its own two count words.
//   grid = any, block = 256; exits at once when nothing was declined
// (The batched routine reads all 64 slots of a row whatever its length, and the positions and image vectors the slots past the end
// name: the list is allocated zeroed and only ever holds valid entries, mw_host_init.hip.h -- this kernel depends on that as the
// resident server does.)
// The list has two count words used by alternate launches (mode bit 2): this kernel zeroes the OTHER one, which the next
// launch's k_move_energy will count in -- a memset per launch (a fill kernel and its dispatch gap, ~10 us) is saved.
__global__ __launch_bounds__(256)
void k_move_fallback(const double* __restrict__ pos, const double* __restrict__ ivect,
                     const uint32_t* __restrict__ listm, const int* __restrict__ nn,
                     const int* __restrict__ req_imol, const double* __restrict__ req_trial, const int* __restrict__ perm,
                     double* __restrict__ e_old, double* __restrict__ e_new, unsigned int* __restrict__ counts,
                     int* __restrict__ declined, int N, int ivcap, int mode)
{
    const int par = (mode >> 2) & 1;
    const int n = declined[par];
    if (blockIdx.x == 0 && threadIdx.x == 0) declined[par ^ 1] = 0;
    const int lane = threadIdx.x & 63;
    const int wave = (int)(blockIdx.x * (blockDim.x >> 6)) + (int)(threadIdx.x >> 6), nwaves = (int)(gridDim.x * (blockDim.x >> 6));
    for (int k = wave; k < 2 * n; k += nwaves) {
        const int side = k & 1;                               // 0: the mirrored position, 1: the trial position
        if (!((mode >> side) & 1)) continue;
        const int m = declined[2 + 2 * (k >> 1)], b = declined[3 + 2 * (k >> 1)];
        const double* P  = pos + (size_t)b * N * 3;
        const double* IV = ivect + (size_t)b * ivcap * 3;
        const uint32_t* LM = listm + (size_t)b * N * kRow;
        const int* NN = nn + (size_t)b * N;
        const int i = req_imol[m];
        const size_t o = (size_t)perm[m];
        Override none; none.idx = -1; none.x = none.y = none.z = 0.0;
        Override tr; tr.idx = -1; tr.x = tr.y = tr.z = 0.0;
        if (side) { tr.idx = i; tr.x = req_trial[3 * (size_t)m]; tr.y = req_trial[3 * (size_t)m + 1]; tr.z = req_trial[3 * (size_t)m + 2]; }
        unsigned int ni, ns;
        const double en = local_energy_wave_batched<false>(P, IV, LM, NN, i, tr, none, lane, ni, ns);
        if (lane == 0) {
            (side ? e_new : e_old)[o] = en;
            counts[4 * o + 2 * side] = ni; counts[4 * o + 2 * side + 1] = ns;
        }
    }
}

// Single request with by-value overrides (the drop-in compute_local_real_energy call):
// one wave, result written straight to host-visible memory.
__global__ __launch_bounds__(64)
void k_local_energy_single(double* __restrict__ pos, const double* __restrict__ ivect,
                           const uint32_t* __restrict__ listm, const int* __restrict__ nn,
                           int b, int i, Override o1, Override o2, int commit,
                           double* __restrict__ e_out, int N, int ivcap,
                           unsigned long long* __restrict__ done, unsigned long long seq)
{
    const int lane = threadIdx.x;
    double* P = pos + (size_t)b * N * 3;
    unsigned int ni, ns;
    const double e = local_energy_wave(P, ivect + (size_t)b * ivcap * 3, listm + (size_t)b * N * kRow,
                                       nn + (size_t)b * N, i, o1, o2, lane, ni, ns);
    if (lane == 0) {
        *e_out = e;
        if (commit) {   // these two indices are never read from memory in this launch (overrides win)
            if (o1.idx >= 0) { P[3 * o1.idx] = o1.x; P[3 * o1.idx + 1] = o1.y; P[3 * o1.idx + 2] = o1.z; }
            if (o2.idx >= 0 && o2.idx != o1.idx) { P[3 * o2.idx] = o2.x; P[3 * o2.idx + 1] = o2.y; P[3 * o2.idx + 2] = o2.z; }
        }
        // the host spins on `done` (host-visible memory) instead of going through a stream synchronisation
        __threadfence_system();
        __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace mw

#include "mw_local_server.hip.h"
