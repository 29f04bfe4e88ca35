// mw_sweep_volume.hip.h -- the Monte Carlo driver's volume move (mc_volume) of one walker by its workgroup.
#pragma once

#include "mw_sweep_common.hip.h"

namespace mw {

// -------------------------------------------------------------------------------------
// Volume move of one walker by its wavefront: mc_volume (mc_moves.F90:1216-1534; ref_ljr,
// which only chain synchronisation reads, is not carried).  Rare (probability ~1/N per move), so it is an
// out-of-line function: one symmetric hmatrix element of both lattices changes, every position is rescaled
// through fractional coordinates (lanes over molecules), image vectors are rebuilt on the device in the
// reference's order and arithmetic, and the full-box energies are recomputed by the wavefront WITH THE
// EXISTING LISTS (atom_energy over the slot-major list); on rejection everything is put back the way the
// reference does it (positions mapped back through the NEW reciprocal matrix, :1413-1506).
// -------------------------------------------------------------------------------------
struct VolCtx {
    double* pos_g;            // global positions of the walker's first box
    double* spos;             // LDS positions [L][N][3] or nullptr
    double* shmat;            // LDS hmatrix   [2][9]
    double* srecip;           // LDS recip     [2][9]
    double* svol;             // LDS volume    [2]
    double* sbk;              // LDS backup of a volume move's old cells [2][27]
    double* siv;              // LDS image vectors [L][ivcap][3]
    int* sniv;                // LDS nivect    [2]
    double* hmat_g;           // global mirrors of the above, walker's first box
    double* vol_g;
    double* ivect_g;
    int* nivect_g;
    const uint32_t* list_g;   // slot-major list (columns in k_list_order's order), walker's first box
    const int* order_g;       // molecule of each column
    const int* nns_g;         // row length of each column
    const int* cmax_g;        // longest row per group of 64 columns
    uint32_t* queue;          // this lane's column of an LDS queue [kSweepQCap + 1][64]
    const unsigned short* srow;   // LDS list rows [L][N][rstride] (16-bit entries) and row lengths [L][N] of walkers entirely in LDS, else nullptr
    const unsigned char* snn;
    int rstride;
    double* mom_trial;        // where a volume move leaves the moments of the trial cell, [L][N][kMomStride], or nullptr
    unsigned* inmask;         // SPLIT builds (volume_move_wg): per molecule the row slots in range, [L][N]
    double* rec;              // ... and the in-range neighbours' {dx, dy, dz, 1/r, e1, g}, [L][N][kSplitQ][6]
    int N, S, ivcap, L;
};
constexpr int kSplitQ = 12;   // in-range neighbours per molecule the split evaluation has room for (more: the one-wavefront routine)

// compute_ivects (molint.F90:174-217) for one lattice, lanes over vectors; returns nivect or -1
__device__ __forceinline__ int dev_compute_ivects(const double* __restrict__ h, double* __restrict__ siv_l,
                                                  double* __restrict__ iv_g, int ivcap, int lane)
{
#pragma clang fp contract(off)
    const double rc = kSmallA * kSigma;
    const int im = (int)floor(rc / sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2])) + 1;       // :189-191
    const int jm = (int)floor(rc / sqrt(h[3] * h[3] + h[4] * h[4] + h[5] * h[5])) + 1;
    const int km = (int)floor(rc / sqrt(h[6] * h[6] + h[7] * h[7] + h[8] * h[8])) + 1;
    const int w1 = 2 * jm + 1, w2 = 2 * km + 1;
    const int n = (2 * im + 1) * w1 * w2;                                                    // :193
    if (n > ivcap) return -1;
    const int central = (im * w1 + jm) * w2 + km;
    for (int k = lane; k < n; k += 64) {
        double vx = 0.0, vy = 0.0, vz = 0.0;                                                 // :197 central cell first
        if (k > 0) {
            const int lin = (k - 1 < central) ? k - 1 : k;                                   // loop order of :200-213
            const int kc = lin % w2 - km, jc = (lin / w2) % w1 - jm, ic = lin / (w2 * w1) - im;
            const double sx0 = (double)ic * h[0], sx1 = (double)ic * h[1], sx2 = (double)ic * h[2];
            const double sy0 = (double)jc * h[3], sy1 = (double)jc * h[4], sy2 = (double)jc * h[5];
            const double sz0 = (double)kc * h[6], sz1 = (double)kc * h[7], sz2 = (double)kc * h[8];
            vx = (sx0 + sy0) + sz0; vy = (sx1 + sy1) + sz1; vz = (sx2 + sy2) + sz2;          // :208
        }
        siv_l[3 * k] = vx; siv_l[3 * k + 1] = vy; siv_l[3 * k + 2] = vz;
        iv_g[3 * k] = vx; iv_g[3 * k + 1] = vy; iv_g[3 * k + 2] = vz;
    }
    return n;
}

// ljr += (H_new * (recip . ljr / 2 pi) - ljr), lanes over molecules (mc_moves.F90:1288-1316)
// (LDSPOS at compile time: a pointer chosen at run time between LDS and global memory makes every access through it a FLAT one --
//  the full-box energy's position gathers, hundreds per volume move, among them)
template <bool LDSPOS>
__device__ __forceinline__ void dev_rescale(const VolCtx& c, int l, const double* recip, const double* hnew, int lane)
{
    const double invPi = 1.0 / 3.141592653589793238462643383279502884197;
    double* Pg = c.pos_g + (size_t)l * c.N * 3;
    double* Ps = c.spos + (size_t)l * c.N * 3;
    for (int i = lane; i < c.N; i += 64) {
        const double* p = LDSPOS ? Ps + 3 * i : Pg + 3 * i;
        const double o0 = p[0], o1 = p[1], o2 = p[2];
        double s0 = MW_HM(recip,1,1) * o0 + MW_HM(recip,2,1) * o1 + MW_HM(recip,3,1) * o2;
        double s1 = MW_HM(recip,1,2) * o0 + MW_HM(recip,2,2) * o1 + MW_HM(recip,3,2) * o2;
        double s2 = MW_HM(recip,1,3) * o0 + MW_HM(recip,2,3) * o1 + MW_HM(recip,3,3) * o2;
        s0 = s0 * 0.5 * invPi; s1 = s1 * 0.5 * invPi; s2 = s2 * 0.5 * invPi;
        double t0 = MW_HM(hnew,1,1) * s0 + MW_HM(hnew,1,2) * s1 + MW_HM(hnew,1,3) * s2;
        double t1 = MW_HM(hnew,2,1) * s0 + MW_HM(hnew,2,2) * s1 + MW_HM(hnew,2,3) * s2;
        double t2 = MW_HM(hnew,3,1) * s0 + MW_HM(hnew,3,2) * s1 + MW_HM(hnew,3,3) * s2;
        t0 = t0 - o0; t1 = t1 - o1; t2 = t2 - o2;
        const double n0 = o0 + t0, n1 = o1 + t1, n2 = o2 + t2;
        Pg[3 * i] = n0; Pg[3 * i + 1] = n1; Pg[3 * i + 2] = n2;
        if constexpr (LDSPOS) { Ps[3 * i] = n0; Ps[3 * i + 1] = n1; Ps[3 * i + 2] = n2; }
    }
}

// compute_model_energy of lattice l by one wavefront (value in every lane).  `mom_l` (walkers entirely in LDS only): every
// molecule's moments too, [N][kMomStride] -- what the translations' moment path reads (move_energy_mom_wave)
// (BATCH4: the distance tests' gathers four at a time -- for the look-ahead builds, which have the registers)
template <bool LDSPOS, bool BATCH4 = false>
__device__ __forceinline__ double dev_wave_model_energy(const VolCtx& c, int l, int lane, double* __restrict__ mom_l = nullptr)
{
    const double* Pg = c.pos_g + (size_t)l * c.N * 3;
    const double* Ps = c.spos + (size_t)l * c.N * 3;
    const double* IVl = c.siv + (size_t)l * c.ivcap * 3;
    const uint32_t* Lg = c.list_g + (size_t)l * c.S * c.N;
    const int* ORD = c.order_g + (size_t)l * c.N;
    const int* NNS = c.nns_g + (size_t)l * c.N;
    const int* CM = c.cmax_g + (size_t)l * ((c.N + 63) >> 6);
    auto getiv = [&](int k, double& x, double& y, double& z) { x = IVl[3 * k]; y = IVl[3 * k + 1]; z = IVl[3 * k + 2]; };
    auto getpos = [&](int j, double& x, double& y, double& z) {
        const double* p = LDSPOS ? Ps + 3 * (size_t)j : Pg + 3 * (size_t)j;
        x = p[0]; y = p[1]; z = p[2];
    };
    double esum = 0.0;
    if (c.srow) {
        // a walker entirely in LDS: its rows are there too (molecule-major, 16-bit entries) -- one lane per molecule, no list read
        // from global memory (the slot-major list cost three dependent global round trips of ~1.5 us each: 9 of a volume move's 19 us)
        uint32_t cur[8];
        for (int base = 0; base < c.N; base += 64) {
            const int mol = base + lane;
            const bool act = mol < c.N;
            const int n = act ? (int)c.snn[l * c.N + mol] : 0;
            const int nmax = __builtin_amdgcn_readfirstlane(wave_max_i(n));
            const unsigned short* row = c.srow + ((size_t)l * c.N + (act ? mol : 0)) * c.rstride;
            auto ent = [&](int s) -> uint32_t { const uint32_t e = s < n ? (uint32_t)row[s] : 0u; return (e & 63u) | ((e >> 6) << kJBits); };
            AtomSum a = atom_energy<64, BATCH4, true, kSweepQCap>(ListRsrc(), kNoColumn, kNoColumn, act ? mol : 0, n, nmax, 0, c.N, c.S, c.queue, getpos, getiv, cur,
                                                                 (mom_l && act) ? mom_l + (size_t)mol * kMomStride : nullptr, ent);
            if (act) esum += a.e;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) esum += __shfl_xor(esum, off, 64);
        return esum;
    }
    const ListRsrc rs = list_rsrc(Lg, c.N, c.S);
    uint32_t cur[8];
    int n_cur = 0, mol = 0;
    uint32_t col = kNoColumn;
    if (lane < c.N) { col = (uint32_t)lane * 4u; n_cur = NNS[lane]; mol = ORD[lane]; }
    for (int base = 0; base < c.N; base += 64) {                 // wave-uniform: one group of 64 list columns per pass
        const bool act = col != kNoColumn;
        const int tn = base + 64 + lane;
        uint32_t col_next = kNoColumn;
        int n_next = 0, mol_next = 0;
        if (tn < c.N) { col_next = (uint32_t)tn * 4u; n_next = NNS[tn]; mol_next = ORD[tn]; }
        const int cm = __builtin_amdgcn_readfirstlane(CM[base >> 6]);
        AtomSum a = atom_energy<64, false, true, kSweepQCap>(rs, col, col_next, mol, act ? (n_cur & 0xff) : 0, cm & 0xff, cm >> 8, c.N, c.S, c.queue, getpos, getiv, cur,
                                                             (mom_l && act) ? mom_l + (size_t)mol * kMomStride : nullptr);
        if (act) esum += a.e;
        n_cur = n_next; mol = mol_next; col = col_next;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) esum += __shfl_xor(esum, off, 64);
    return esum;
}

// SPLIT: a volume move's full-box energy (compute_model_energy, molint.F90:407-499) spread over ALL wavefronts of a look-ahead
// workgroup -- the builds of a handful of walkers, whose wavefronts beyond one per lattice have nothing else to do during a volume
// move, and whose speed is one chain's: the one-wavefront routine above walks a molecule's row and its ~8 in-range neighbours' pair
// terms (rsqrt, reciprocal, exp) one after the other, 7 of a volume move's 16 us.  Walkers entirely in LDS, lane = molecule,
// wavefront `part` of `nparts` of the lattice:
//   A  distance tests of row slots part, part + nparts, ...: the in-range slots are OR-ed into inmask[molecule];
//   B  in-range neighbour q (in list order) of every molecule by wavefront q mod nparts: {d, 1/r, e1, g} into rec[molecule][q];
//   C  the lattice's first wavefront adds the records up in list order with atom_energy's own arithmetic (MomentSums): the energy
//      and the moments are atom_energy's bit for bit, so the chain does not depend on the look-ahead of the build that runs it.
// Between the phases: the caller's workgroup barriers.  B reports a molecule with more than kSplitQ in-range neighbours (`overflow`):
// the caller then takes the one-wavefront routine.
__device__ __forceinline__ void dev_split_tests(const VolCtx& c, int l, int part, int nparts, int lane)
{
    const int mol = lane < c.N ? lane : 0;
    const bool act = lane < c.N;
    const double* Ps = c.spos + (size_t)l * c.N * 3;
    const double* IVl = c.siv + (size_t)l * c.ivcap * 3;
    const int n = act ? (int)c.snn[l * c.N + mol] : 0;
    const int nmax = __builtin_amdgcn_readfirstlane(wave_max_i(n));
    const unsigned short* row = c.srow + ((size_t)l * c.N + mol) * c.rstride;
    const double xi = Ps[3 * mol], yi = Ps[3 * mol + 1], zi = Ps[3 * mol + 2];
    unsigned m = 0u;
    for (int s = part; s < nmax; s += nparts) {
        const uint32_t e = s < n ? (uint32_t)row[s] : 0u;
        const double* pj = Ps + 3 * (size_t)(e & 63u);
        const double* iv = IVl + 3 * (size_t)(e >> 6);
        const double dx = (pj[0] + iv[0]) - xi, dy = (pj[1] + iv[1]) - yi, dz = (pj[2] + iv[2]) - zi;     // molint.F90:447,450
        const double r2 = dist2(dx, dy, dz);
        if (s < n && r2 < kRcSq) m |= 1u << s;                                                          // :454
    }
    if (m != 0u) atomicOr(&c.inmask[l * c.N + mol], m);
}

__device__ __forceinline__ bool dev_split_records(const VolCtx& c, int l, int part, int nparts, int lane)
{
    const int mol = lane < c.N ? lane : 0;
    const bool act = lane < c.N;
    const double* Ps = c.spos + (size_t)l * c.N * 3;
    const double* IVl = c.siv + (size_t)l * c.ivcap * 3;
    const unsigned short* row = c.srow + ((size_t)l * c.N + mol) * c.rstride;
    const double xi = Ps[3 * mol], yi = Ps[3 * mol + 1], zi = Ps[3 * mol + 2];
    const unsigned mask = act ? c.inmask[l * c.N + mol] : 0u;
    const int cnt = __popc(mask);
    double* R = c.rec + ((size_t)l * c.N + mol) * kSplitQ * 6;
    for (int q = part; q < kSplitQ; q += nparts) {            // (uniform bounds; a lane with fewer in-range neighbours sits the step out)
        if (q < cnt) {
            unsigned mm = mask;
            for (int t = 0; t < q; ++t) mm &= mm - 1u;        // the q-th in-range slot
            const int s = __ffs((int)mm) - 1;
            const uint32_t e = (uint32_t)row[s];
            const double* pj = Ps + 3 * (size_t)(e & 63u);
            const double* iv = IVl + 3 * (size_t)(e >> 6);
            const double dx = (pj[0] + iv[0]) - xi, dy = (pj[1] + iv[1]) - yi, dz = (pj[2] + iv[2]) - zi;
            const double r2 = dist2(dx, dy, dz);
            double rinv, e1, g;
            pair_terms(r2, rinv, e1, g);                                                  // :456-462
            double2* r2p = reinterpret_cast<double2*>(R + 6 * q);
            r2p[0] = make_double2(dx, dy); r2p[1] = make_double2(dz, rinv); r2p[2] = make_double2(e1, g);
        }
    }
    return __ballot(cnt > kSplitQ) != 0ull;
}

// (value in every lane, like dev_wave_model_energy)
__device__ __forceinline__ double dev_split_sum(const VolCtx& c, int l, int lane, double* __restrict__ mom_l, double* lane_e = nullptr)
{
    const int mol = lane < c.N ? lane : 0;
    const bool act = lane < c.N;
    const int cnt = act ? __popc(c.inmask[l * c.N + mol]) : 0;
    const double* R = c.rec + ((size_t)l * c.N + mol) * kSplitQ * 6;
    MomentSums ms;
    for (int q = 0; q < cnt; ++q) {
        const double2* r2p = reinterpret_cast<const double2*>(R + 6 * q);
        const double2 a = r2p[0], b = r2p[1], d = r2p[2];
        ms.add(a.x, a.y, b.x, b.y, d.x, d.y);
    }
    double esum = 0.0;
    const double e = ms.finish(cnt, (mom_l && act) ? mom_l + (size_t)mol * kMomStride : nullptr);
    if (lane_e) *lane_e = e;
    if (act) esum += e;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) esum += __shfl_xor(esum, off, 64);
    return esum;
}

// Volume move of one walker (mc_volume, mc_moves.F90:1216-1534; ref_ljr, which only chain synchronisation reads, is not
// carried).  Rare (probability ~1/N per move).  One symmetric hmatrix element of both lattices changes; every wavefront
// rescales ITS lattice through fractional coordinates (lanes over molecules), rebuilds its image vectors in the
// reference's order and arithmetic and recomputes its full-box energy WITH THE EXISTING LISTS (atom_energy over the
// slot-major list); wavefront 0 decides; on rejection every wavefront puts its lattice back the way the reference does
// (positions mapped back through the NEW reciprocal matrix, :1413-1506).
// Returns (every wavefront): 1 accepted, 0 rejected, -1 rejected because a cell needed more image vectors than ivcap.
// With look-ahead (NW > NLAT wavefronts) the wavefronts beyond the first NLAT have no lattice of their own here: they keep
// the workgroup's barriers company.
template <int NLAT, int NW, bool LDSPOS, bool SPLIT, typename DecideFn>
__device__ __forceinline__
int volume_move_wg(const VolCtx& c, const double* __restrict__ U, double dv_max, int wv, int lane,
                   double* __restrict__ sx, int* __restrict__ sdec, DecideFn decide)
{
    constexpr int L = NLAT;
    const bool active = wv < NLAT;
    const int l = active ? wv : 0;                                                 // this wavefront's lattice
    [[maybe_unused]] const unsigned long long tv0 = MW_SW_NOW();
    // the old cell of this lattice, kept in LDS (c.sbk: [lattice][hmatrix 9 | recip 9 | new recip 9]): eighteen wave-uniform
    // doubles are thirty-six vector registers, held across the full-box energy evaluation
    double* bk_h = c.sbk + 27 * l;
    double* bk_r = bk_h + 9;
    double* bk_n = bk_h + 18;
    if (active && lane < 9) { bk_h[lane] = c.shmat[l * 9 + lane]; bk_r[lane] = c.srecip[l * 9 + lane]; }
    const double old_vol_l = c.svol[l];
    const int idim = (int)(U[0] * 3.0) + 1, jdim = (int)(U[1] * 3.0) + 1;                       // :1269-1272
    const double dh = (2.0 * U[2] - 1.0) * dv_max;                                              // :1276
    wg_sync<NW>();                                     // (everybody has read the old cells)
    if (active && lane == 0) {                                                                  // :1281-1282
        MW_HM(c.shmat + 9 * l, idim, jdim) = MW_HM(c.shmat + 9 * l, idim, jdim) + dh;
        if (idim != jdim) MW_HM(c.shmat + 9 * l, jdim, idim) = MW_HM(c.shmat + 9 * l, jdim, idim) + dh;
    }
    wg_sync<NW>();
    // The reference takes the lattices in turn and stops at the first whose new cell needs more image vectors than there
    // is room for (:1285-1358; here: the move counts as rejected and is flagged): lattice 2 is then never touched.
    bool bad0 = false;
    if (L == 2 && l == 1) {
        const double* h = c.shmat;
        const double rc = kSmallA * kSigma;
        const int im = (int)floor(rc / sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2])) + 1;
        const int jm = (int)floor(rc / sqrt(h[3] * h[3] + h[4] * h[4] + h[5] * h[5])) + 1;
        const int km = (int)floor(rc / sqrt(h[6] * h[6] + h[7] * h[7] + h[8] * h[8])) + 1;
        bad0 = (2 * im + 1) * (2 * jm + 1) * (2 * km + 1) > c.ivcap;
    }
    double new_e = 0.0;
    int bad = 0;
    bool rescaled = false;
    [[maybe_unused]] const unsigned long long tv1 = MW_SW_NOW();
    MW_SW_ACC(34, tv1 - tv0);
    if (active && !bad0) {
        dev_rescale<LDSPOS>(c, l, bk_r, c.shmat + 9 * l, lane);
        rescaled = true;
        wave_sync();
        MW_SW_ACC(35, MW_SW_NOW() - tv1);
        const int niv = dev_compute_ivects(c.shmat + 9 * l, c.siv + (size_t)l * c.ivcap * 3,
                                           c.ivect_g + (size_t)l * c.ivcap * 3, c.ivcap, lane);
        if (lane == 0) {
            c.svol[l] = fabs(dev_det3(c.shmat + 9 * l));
            double rcp[9];
            dev_recipmatrix(c.shmat + 9 * l, rcp);
#pragma unroll
            for (int t = 0; t < 9; ++t) c.srecip[l * 9 + t] = rcp[t];
            if (niv >= 0) { c.sniv[l] = niv; c.nivect_g[l] = niv; }
        }
        wave_sync();
        [[maybe_unused]] const unsigned long long tv2 = MW_SW_NOW();
        if (niv < 0) bad = 1;
        else if constexpr (!SPLIT) new_e = dev_wave_model_energy<LDSPOS, (NW > NLAT)>(c, l, lane, c.mom_trial ? c.mom_trial + (size_t)l * c.N * kMomStride : nullptr);
        MW_SW_ACC(36, MW_SW_NOW() - tv2); MW_SW_ACC(37, tv2 - tv1);
    }
    if constexpr (SPLIT) {
        // the full-box energy by every wavefront of the workgroup (see dev_split_tests): sdec[2 + lattice] != 0 -- a cell that is
        // not to be evaluated (bad, or lattice 2 after a bad lattice 1); sdec[0] -- a molecule with more in-range neighbours than
        // the records hold
        [[maybe_unused]] const unsigned long long tv2 = MW_SW_NOW();
        constexpr int P = NW / NLAT;
        const int lw = wv % NLAT, part = wv / NLAT;
        if (active && lane == 0) sdec[2 + l] = bad | (bad0 ? 2 : 0);
        if (part == 1 && lane < c.N) c.inmask[lw * c.N + lane] = 0u;                 // (a wavefront that is idle until here)
        if (wv == NLAT && lane == 0) sdec[0] = 0;
        wg_sync<NW>();                                  // the trial cell -- positions, image vectors -- is there for everybody
        const bool run = sdec[2 + lw] == 0;
        if (run) dev_split_tests(c, lw, part, P, lane);
        wg_sync<NW>();
        if (run && dev_split_records(c, lw, part, P, lane) && lane == 0) sdec[0] = 1;
        wg_sync<NW>();
        if (active && !bad0 && !bad) {
            double* mom_l = c.mom_trial ? c.mom_trial + (size_t)l * c.N * kMomStride : nullptr;
            new_e = sdec[0] != 0 ? dev_wave_model_energy<LDSPOS, true>(c, l, lane, mom_l) : dev_split_sum(c, l, lane, mom_l);
#ifdef MW_SPLIT_CHECK     // diagnostic build (tools/variants.py splitcheck): the split sum against the one-wavefront routine, molecule by molecule
                          // -- g_sweep_stamps[44] lattice energies checked, [45] of them with a molecule that differs, [43], [46], [47] the last such
            if (sdec[0] == 0) {
                double es = 0.0;
                (void)dev_split_sum(c, l, lane, nullptr, &es);
                const int mol = lane < c.N ? lane : 0;
                const int n = lane < c.N ? (int)c.snn[l * c.N + mol] : 0;
                const int nmax = __builtin_amdgcn_readfirstlane(wave_max_i(n));
                const unsigned short* row = c.srow + ((size_t)l * c.N + mol) * c.rstride;
                const double* Ps = c.spos + (size_t)l * c.N * 3;
                const double* IVl = c.siv + (size_t)l * c.ivcap * 3;
                auto getiv = [&](int k, double& x, double& y, double& z) { x = IVl[3 * k]; y = IVl[3 * k + 1]; z = IVl[3 * k + 2]; };
                auto getpos = [&](int j, double& x, double& y, double& z) { const double* p = Ps + 3 * (size_t)j; x = p[0]; y = p[1]; z = p[2]; };
                auto ent = [&](int s) -> uint32_t { const uint32_t e = s < n ? (uint32_t)row[s] : 0u; return (e & 63u) | ((e >> 6) << kJBits); };
                uint32_t cur[8];
                AtomSum a = atom_energy<64, true, true, kSweepQCap>(ListRsrc(), kNoColumn, kNoColumn, mol, n, nmax, 0, c.N, c.S, c.queue, getpos, getiv, cur, nullptr, ent);
                const bool bad_l = lane < c.N && a.e != es;
                const unsigned long long bm = __ballot(bad_l);
                if (blockIdx.x == 0 && lane == 0) atomicAdd(&g_sweep_stamps[44], 1ull);
                if (bm != 0ull && blockIdx.x == 0 && lane == __ffsll((long long)bm) - 1) {
                    atomicAdd(&g_sweep_stamps[45], 1ull);
                    g_sweep_stamps[43] = (unsigned long long)(a.cnt | (__popc(c.inmask[l * c.N + mol]) << 8) | (lane << 16) | (n << 24));
                    g_sweep_stamps[46] = (unsigned long long)__double_as_longlong(a.e); g_sweep_stamps[47] = (unsigned long long)__double_as_longlong(es);
                }
            }
#endif
        }
        MW_SW_ACC(36, MW_SW_NOW() - tv2);
    }
    [[maybe_unused]] const unsigned long long tv3 = MW_SW_NOW();
    if (active && lane == 0) { sx[l] = new_e; sdec[2 + l] = bad; }
    wg_sync<NW>();
    int ok = 0, anybad = 0;
    if (wv == 0) {
        anybad = sdec[2] | (L == 2 ? sdec[3] : 0);
        ok = decide(sx[0], L == 2 ? sx[1] : 0.0, anybad);          // (updates the walker's state; energies in every lane)
        if (lane == 0) { sdec[0] = ok; sdec[1] = anybad; }
    }
    wg_sync<NW>();
    [[maybe_unused]] const unsigned long long tv4 = MW_SW_NOW();
    MW_SW_ACC(38, tv4 - tv3);
    ok = sdec[0]; anybad = sdec[1];
    if (active && !ok) {                                                                         // :1426-1530
        if (lane < 9) bk_n[lane] = c.srecip[l * 9 + lane];
        wave_sync();
        if (lane < 9) { c.shmat[l * 9 + lane] = bk_h[lane]; c.srecip[l * 9 + lane] = bk_r[lane]; }
        if (lane == 0) c.svol[l] = old_vol_l;
        wave_sync();
        if (rescaled) {
            dev_rescale<LDSPOS>(c, l, bk_n, c.shmat + 9 * l, lane);                                      // back through the NEW recip
            const int niv = dev_compute_ivects(c.shmat + 9 * l, c.siv + (size_t)l * c.ivcap * 3,
                                               c.ivect_g + (size_t)l * c.ivcap * 3, c.ivcap, lane);   // :1510-1512
            if (lane == 0 && niv > 0) { c.sniv[l] = niv; c.nivect_g[l] = niv; }
        }
    }
    if (active && lane == 0) {                         // global mirrors of the cell
#pragma unroll
        for (int t = 0; t < 9; ++t) c.hmat_g[l * 9 + t] = c.shmat[l * 9 + t];
        c.vol_g[l] = c.svol[l];
    }
    wg_sync<NW>();
    MW_SW_ACC(39, MW_SW_NOW() - tv4); MW_SW_ACC(40, 1ull); MW_SW_ACC(41, MW_SW_NOW() - tv0);
    return anybad ? -1 : ok;
}

}  // namespace mw
