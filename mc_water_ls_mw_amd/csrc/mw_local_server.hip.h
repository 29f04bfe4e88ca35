// mw_local_server.hip.h -- gfx950 (MI355X, CDNA4) device code of the mW energy engine:
// the resident mailbox server of the drop-in single call (k_local_server).  Included at the end of mw_move_energy.hip.h.
#pragma once

#include "mw_common.hip.h"
#include "mw_local_energy.hip.h"
#include "mw_move_scan.hip.h"
#include "mw_move_moments.hip.h"

namespace mw {

// =====================================================================================
// Resident server for the drop-in single call (compute_local_real_energy behind the unchanged Fortran call
// sites, mc_moves.F90:1010,1083): a kernel launch plus its completion cost ~30 us, fifteen times what the
// reference spends on the whole evaluation, so the engine keeps ONE small kernel resident instead -- started by
// the first single call, stopped by any entry point that changes device state behind its back (uploads, list
// builds, the batch kernels) and by mw_finalize, and by itself after `idle_limit` empty polls.  Workgroup w (one
// wavefront) serves mail slot w (lattice ils goes to slot (ils - 1) % nslots, so the two lattices of a move can
// be evaluated concurrently from two host threads): it polls the slot's request lines (device memory the host
// writes through the BAR, or host-mapped memory), evaluates the request with move_energy_wave (positions read
// past the L1: this kernel itself commits the two overridden positions between requests), and writes energy +
// sequence word to the reply line in host memory.  The cost of a call is a posted PCIe write each way, a poll
// and the evaluation, not a launch.
// One workgroup per slot, not one wavefront of a shared workgroup: a compute unit's vector memory pipeline returns
// data in order, and with eight wavefronts polling across PCIe (1.3 us a read) every gather of the one that is
// working queued behind their polls -- 8.9 us an evaluation against 3.6 us on a compute unit of its own.
// =====================================================================================
struct MailSlot {                       // 64-byte aligned; one per served slot (request lines and reply line may live in different copies)
    // request, line A (the host writes the fields of both lines, then seq_a, then seq_b, a store fence between them:
    // a line that shows the new sequence word shows its new fields, and seq_b == seq_a says both lines are in)
    unsigned long long seq_a;
    int box, imol;                      // 0-based
    double x1, y1, z1;                  // position of imol, if flags & 2
    int flags, prev;                    // bit 0: commit the positions, bit 1: x1.. present, bit 2: x2.. present; prev 0-based
    unsigned long long pad_a[2];
    // request, line B
    double x2, y2, z2;                  // position of the previously queried molecule, if flags & 4
    unsigned long long pad_b[4];
    unsigned long long seq_b;
    // reply line (device -> host)
    unsigned long long rep_seq;         // the request this reply belongs to (written last)
    double energy;
    unsigned int ninter, nslots;
    unsigned long long pad_c[5];
};
static_assert(sizeof(MailSlot) == 192, "two request lines and one reply line");
struct MailHead { int quit; int exited; int pad[14]; };

template <bool COHERENT>
__global__ __launch_bounds__(64)
void k_local_server(MailHead* __restrict__ head, MailSlot* __restrict__ slots, const MailSlot* __restrict__ reqs,
                    double* __restrict__ pos, const double* __restrict__ ivect, const int* __restrict__ nivect,
                    const uint32_t* __restrict__ listm, const int* __restrict__ nn,
                    int N, int ivcap, long long idle_limit, int stamps,
                    double* mom, double* pm, int* momok,   // the moment path (below), or nullptr
                    int* unc,                               // per box: the molecule whose committed position pm does not hold yet, or -1
                    unsigned long long* __restrict__ counts)   // per box: requests served by the moment path / the scanning routine /
                                                               // the plain routine, moment updates (mw_server_counts)
{
    __shared__ WaveScratch ws;
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x;
    MailSlot* m = slots + w;
    const unsigned long long* words = reinterpret_cast<const unsigned long long*>(reqs + w);    // request lines
    unsigned long long last = __hip_atomic_load(&m->rep_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    long long idle = 0;
    auto word = [&](unsigned long long v, int l) {
        const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, l);
        const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), l);
        return ((unsigned long long)hi << 32) | lo;
    };
    for (;;) {                                                        // every exit condition is reached by every wavefront
        // one load instruction fetches both request lines (lane l reads word l & 15): two PCIe reads in flight together
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        const unsigned long long v = __hip_atomic_load(words + (lane & 15), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const unsigned long long seq = word(v, 0);
        if (seq != last && word(v, 15) == seq) {
            const unsigned long long w1 = word(v, 1), w5 = word(v, 5);
            const int b = (int)(unsigned int)w1, i = (int)(unsigned int)(w1 >> 32);
            const int flags = (int)(unsigned int)w5, prev = (int)(unsigned int)(w5 >> 32);
            Override o1, o2;
            o1.idx = (flags & 2) ? i : -1;
            o1.x = __longlong_as_double((long long)word(v, 2)); o1.y = __longlong_as_double((long long)word(v, 3)); o1.z = __longlong_as_double((long long)word(v, 4));
            o2.idx = (flags & 4) ? prev : -1;
            o2.x = __longlong_as_double((long long)word(v, 8)); o2.y = __longlong_as_double((long long)word(v, 9)); o2.z = __longlong_as_double((long long)word(v, 10));
            double* P = pos + (size_t)b * N * 3;
            const double* IVb = ivect + (size_t)b * ivcap * 3;
            const uint32_t* LMb = listm + (size_t)b * N * kRow;
            const int* NNb = nn + (size_t)b * N;
            const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
            // The lane-packed evaluation of the batched kernel (old and trial position both = the molecule's position): a
            // third of the instructions of the plain routine, which matters for ONE wavefront on its own; the plain
            // routine, with its loads batched, takes the cases that one declines.
            double xi, yi, zi;
            load_pos<COHERENT>(P, i, o1, o2, xi, yi, zi);
            auto getpos = [&](int jx, double& x, double& y, double& z) { load_pos<COHERENT>(P, jx, o1, o2, x, y, z); };
            auto getiv = [&](int k, double& x, double& y, double& z) { x = IVb[3 * k]; y = IVb[3 * k + 1]; z = IVb[3 * k + 2]; };
            auto row = [&](int jx, int sl) { return LMb[(size_t)jx * kRow + sl]; };
            auto nnof = [&](int jx) { return NNb[jx]; };
            MoveRes res;
            double e;
            // THE MOMENT PATH (round 4; move_energy_mom_wave<SWEEP>, as in the Monte Carlo driver): `mom` = every molecule's moments of
            // the served boxes, made by the full-box kernel when the server starts, and `pm` = the positions they were made FROM.  The
            // host changes positions only through the requests' own overrides -- the queried molecule and the one queried before it
            // (anything else is an exclusive entry point, which stops the server) -- so for the drop-in's caller at most `prev` can have moved since: if its
            // committed position is no longer the one in `pm`, its neighbours' moments and its own are brought up to date first
            // (moments_commit: an accepted move of the host's chain, one request in four at most), then the queried molecule is
            // evaluated with pm[i] as the "old" position -- the arm the moments hold -- and the request's as the trial one.
            // Every neighbour is read from `pm`.  A request this does not cover (an uncommitted override of prev, a decline) takes the
            // routines below; one that leaves the moments behind (a declined update) switches the path off for the box.
            // A caller need not name `prev` (mw_local_energy has none), or may name another molecule than the one it asked about last:
            // that molecule's override was committed to `pos` after its reply, and `pm` never heard of it.  unc[b] names it -- the one
            // molecule of the box whose committed position may differ from pm -- and a request whose i and prev do not cover it brings
            // it up to date first, from `pos`, the same way as prev.
            bool served = false;
            int path = 2, nupd = 0;                                     // (for the counters: 0 moment path, 1 scanning routine, 2 plain routine)
            int un = -1;
            if (mom != nullptr) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // (this wavefront's own earlier writes to mom / pm: past the L1)
                double* MOMb = mom + (size_t)b * N * kMomStride;
                double* PMb = pm + (size_t)b * N * 3;
                auto getpm = [&](int jx, double& x, double& y, double& z) { const double* q = PMb + 3 * (size_t)jx; x = q[0]; y = q[1]; z = q[2]; };
                // ONE round trip for everything the path needs to get going (a lone wavefront pays ~0.5 us per dependent load level)
                const int pv = o2.idx >= 0 ? prev : i;
                const int mk = momok[b];
                un = __hip_atomic_load(unc + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (written after the previous reply: past the L1)
                double px, py, pz, qx, qy, qz;
                getpm(pv, px, py, pz);
                getpm(i, qx, qy, qz);
                const uint32_t erow = row(i, lane & 31);
                const int ni = nnof(i);
                unsigned int nocounts[4];
                int cnt = 0;
                bool ok = true;
                const bool late = un >= 0 && un != i && un != o2.idx && mk != 0;    // (the protocol's own caller never is: one more load level)
                // prev has moved since its moments were made (not: a silent revert, nothing to follow) -- decided HERE, on the loads of the
                // round trip above: left to the loop below, the compiler sinks pm[prev]'s load into it, a load level of its own
                const bool moved = (o2.idx >= 0) & (o2.idx != i) & ((px != o2.x) | (py != o2.y) | (pz != o2.z));
#pragma unroll 1
                for (int pass = late ? 0 : 1; pass < (moved ? 2 : 1) && ok; ++pass) {   // the molecules whose moments are behind: unc[b], then prev
                    const int u = pass == 0 ? un : prev;
                    double ox = px, oy = py, oz = pz, nx = o2.x, ny = o2.y, nz = o2.z;
                    if (pass == 0) {
                        const Override none = {-1, 0.0, 0.0, 0.0};
                        getpm(u, ox, oy, oz);
                        load_pos<COHERENT>(P, u, none, none, nx, ny, nz);
                        if (ox == nx && oy == ny && oz == nz) continue;             // (it was asked about where it already was)
                    } else if (!(flags & 1) || mk == 0) { ok = false; break; }      // (prev's override is not committed: the moments must not
                                                                                    //  follow it; the uncovered molecule's position already is)
                    MoveRes r2;
                    if (move_energy_mom_wave<true, 0, 2>(getpm, getiv, nnof, MOMb, &ws, nullptr, u, nnof(u), row(u, lane & 31),
                                                             ox, oy, oz, nx, ny, nz, lane, r2, nocounts, &cnt)) {
                        moments_commit(MOMb, &ws, u, cnt, ox, oy, oz, nx, ny, nz, lane);
                        if (lane == 0) { PMb[3 * u] = nx; PMb[3 * u + 1] = ny; PMb[3 * u + 2] = nz; }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        ++nupd;
                    } else {
                        ok = false;
                        if (lane == 0) momok[b] = 0;               // (the moments no longer follow the positions: off for this box until the server restarts)
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    }
                }
                if (ok && move_energy_mom_wave<true, 0, 2>(getpm, getiv, nnof, MOMb, &ws, nullptr, i, ni, erow,
                                                               qx, qy, qz, xi, yi, zi, lane, res, nocounts, &cnt) && mk != 0) { e = res.en; served = true; path = 0; }
            }
            if (served) {
            } else if (move_energy_wave(getpos, getiv, row, nnof, &ws, nivect[b], i, nnof(i), row(i, lane & 31), xi, yi, zi, xi, yi, zi, lane, res)) {
                e = res.eo;
                path = 1;
            } else {
                unsigned int ni, ns;
                e = local_energy_wave_batched<COHERENT>(P, IVb, LMb, NNb, i, o1, o2, lane, ni, ns);
            }
            const unsigned long long t2 = __builtin_amdgcn_s_memrealtime();
            if (lane == 0) {
                // the reply: energy and sequence word in ONE 16-byte store (one PCIe write: the host reads the word, then the energy)
                typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                const unsigned long long eb = (unsigned long long)__double_as_longlong(e);
                const u32x4 rep = {(unsigned int)seq, (unsigned int)(seq >> 32), (unsigned int)eb, (unsigned int)(eb >> 32)};
                asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" :: "v"(&m->rep_seq), "v"(rep) : "memory");
                if (stamps) {     // 100 MHz stamps for tools/kbench (poll issued -> request decoded -> evaluated): diagnostics only
                    __hip_atomic_store(&m->pad_c[0], t1 - t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(&m->pad_c[1], t2 - t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                if (flags & 1) {  // after the reply is on its way: written through to L2 (agent scope); the kernel's end makes
                                  // them visible to every later launch
                    if (o1.idx >= 0) {
                        __hip_atomic_store(P + 3 * o1.idx, o1.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(P + 3 * o1.idx + 1, o1.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(P + 3 * o1.idx + 2, o1.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    if (o2.idx >= 0 && o2.idx != o1.idx) {
                        __hip_atomic_store(P + 3 * o2.idx, o2.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(P + 3 * o2.idx + 1, o2.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(P + 3 * o2.idx + 2, o2.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                // still after the reply, off the caller's chain: who is uncovered now, and the box's counters (fire-and-forget adds: this
                // wavefront is the only writer of its boxes' counters, the add is atomic only to spare the wait a load would take)
                if (mom != nullptr) {
                    const int now = ((flags & 1) && o1.idx >= 0) ? i : (un == i ? i : -1);
                    if (now != un) __hip_atomic_store(unc + b, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                (void)__hip_atomic_fetch_add(counts + 4 * (size_t)b + path, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (nupd) (void)__hip_atomic_fetch_add(counts + 4 * (size_t)b + 3, (unsigned long long)nupd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            last = seq;
            idle = 0;
        } else {
            const int q = __hip_atomic_load(&head->quit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (q != 0 || ++idle > idle_limit) break;
        }
    }
    if (lane == 0) __hip_atomic_fetch_add(&head->exited, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace mw
