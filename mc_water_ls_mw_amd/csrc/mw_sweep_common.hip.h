// mw_sweep_common.hip.h -- the Monte Carlo driver's shared device pieces: parameters, random numbers, the order-parameter
// grid, cell algebra, workgroup synchronisation and the LDS layout of a walker's workgroup.
#pragma once

#include "mw_common.hip.h"
#include "mw_full_energy.hip.h"
#include "mw_move_energy.hip.h"

namespace mw {

// =====================================================================================
// Device-resident translation-move driver: mc_water_translation
// (mc_moves.F90:966-1213) with eta_weight (:893-964) and mu_to_bin (:2187-2215), for many
// independent walkers at once.  One workgroup per walker -- one wavefront per lattice -- runs its
// Markov chain move after move: pick a molecule, draw the displacement in the active lattice, map
// it through fractional coordinates into the partner lattice (:1042-1066), fused old/new local
// energy in each lattice (move_energy_wave, the lattices side by side), update the order parameter
// mu and the multicanonical weights' contribution, accept or revert (:1145-1209).  The caller-side
// bookkeeping of model_energy (:1013-1016,1087,1190) is done here on the per-box energies.
// Random numbers: Philox4x32-10, counter (move lo, move hi, walker, call), key = seed -- the same
// stream as the oracle's mwo_move_uniforms.
//   grid = walkers in the launch, block = 64 x lattices
// =====================================================================================
struct SweepParams {
    double beta, max_trans;
    double r_pos, a_pos, r_neg, a_neg, mu_lo, mu_hi;
    int nlat, nbins, eta_interp, start_bin, end_bin, pad;
    // the rest of a translation-only mc_cycle (all off by default)
    int record, samplerun, always_switch, npt;      // mc_update_wl_bins active / fixed weights / switch after every move / ensemble
    double av_binwidth, wl_factor, log_unbiased_norm, pressure;
    double transP, dv_max;                          // move-type threshold (mc_moves.F90:157-166), max cell-element change
    // leshift (userparams.f90:41): ref_enthalpy(1) - ref_enthalpy(2), 0 when off (main.f90:146-150,173; mc_moves.F90:1371,1567-1584)
    double dref;
    // wl_swetnam (mc_moves.F90:1636-1653): the increment follows the histogram's r.m.s. deviation from flat, move by move
    int swetnam, dd;                                // dd: parallel_strategy = 'dd' (window per walker, mc_moves.F90:181-210,659-709)
    double wl_alpha, orig_wl_factor, mu_min, mu_max;
    int eq_cycles, in_window;                       // dd: equilibration length (cycles); in_window: this walker's flag (filled per walker)
    // the reference's -DMINU build (mc_moves.F90:1119-1140,1168-1170,1385-1401,1426-1429): an accepted move also takes the
    // walker to the lattice of lower enthalpy; ref1/ref2 = ref_enthalpy(1:2) under leshift, 0 otherwise
    int minu, pad_minu;
    double ref1, ref2;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ double u53(uint32_t a, uint32_t b)
{
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// -------------------------------------------------------------------------------------
// Order parameter -> bin -> weight, LANE-PARALLEL.  These are scalar computations of the host program (a log, three
// divisions, an exp per call) and a wavefront has no scalar double-precision unit: evaluated one after the other by all
// 64 lanes they cost more vector instructions per move than one lattice's whole energy evaluation (profiles/r03a: 2200
// VALU instructions per two-lattice move with the Wang-Landau update and a switch attempt, 1170 of them energy).  Here
// every value of mu a move needs -- the trial value, the value a rejection restores, the current one -- sits in its own
// lane and ONE instruction stream serves them all; likewise the move's exponentials.
// -------------------------------------------------------------------------------------
struct MuGridDev {                       // per walker, wave-uniform
    double c_pos, c_neg, ilr_pos, ilr_neg, mu_lo, mu_hi;       // c = (1 - r) / a, ilr = 1 / log(r) of the two geometric bin progressions
    int nbins, start_bin, end_bin, eta_interp, in_window;
};

// mc_moves.F90:2187-2215, one mu per lane: bin = nbins/2 + 2 + int(log(1 - (mu - 0.5)(1 - r)/a) / log r) on the positive side.  The
// two divisions are multiplications by per-walker constants and the logarithm is the engine's own (mw_common.hip.h) -- 45 vector
// instructions where the expression as written costs 220; the bin differs from the reference's only for a mu within ~1e-15
// (relative) of a bin boundary, where two libm implementations differ as well.
__device__ __forceinline__ int lane_mu_to_bin(const MuGridDev& g, double mu)
{
    const double a = fabs(mu);
    const bool pos = mu > 0.0;
    const double c = pos ? g.c_pos : g.c_neg, ilr = pos ? g.ilr_pos : g.ilr_neg;
    const double arg = __builtin_fma(-(a - 0.5), c, 1.0);
    const int q = (int)(fast_log_pos(arg) * ilr);
    return a <= 0.5 ? g.nbins / 2 + 1 : (pos ? g.nbins / 2 + 2 + q : g.nbins / 2 - q);
}

// eta_weight (mc_moves.F90:893-964) for one mu per lane, bin k already known; w / mb / bw: 0-based tables in LDS.
// The four interpolation branches of the reference are one expression with selected indices:
//   eta = w(base) + (mu - mu_bin(base)) * 2 (w(hi) - w(lo)) / (binwidth(hi) + binwidth(lo)),   hi = lo + 1
__device__ __forceinline__ double lane_eta(const MuGridDev& g, const double* w, const double* __restrict__ mb,
                                           const double* __restrict__ bw, double mu, int k)
{
    const int nb = g.nbins;
    const int kc = k < 1 ? 1 : (k > nb ? nb : k);               // (a bin outside the table only with mu outside the range: not used then)
    const bool up = (kc == g.start_bin) || (kc != g.end_bin && mu > mb[kc - 1]);
    int hi = up ? kc + 1 : kc;
    hi = hi > nb ? nb : (hi < 2 ? 2 : hi);
    const int lo = hi - 1;
    const int base = (up || kc == g.end_bin) ? kc : (kc > 1 ? kc - 1 : 1);
    double val = w[kc - 1];
    if (g.eta_interp) val = w[base - 1] + (mu - mb[base - 1]) * (2.0 * (w[hi - 1] - w[lo - 1]) / (bw[hi - 1] + bw[lo - 1]));
    // 'dd' walkers that have not reached their window yet carry no weight: the reference returns there without
    // assigning the function result (:913); 0 is what its comment asks for ("don't want to penalise walkers")
    val = (mu < g.mu_lo || mu > g.mu_hi) ? 1.7976931348623157e308 : val;      // huge(1.0_dp)
    return g.in_window ? val : 0.0;
}

#define MW_HM(m, r, c) ((m)[((c) - 1) * 3 + ((r) - 1)])     // Fortran (r,c) of a column-major 3x3
__device__ __forceinline__ void dev_recipmatrix(const double* __restrict__ h, double rc[9])   // util.f90:43-77
{
    MW_HM(rc,1,1) = MW_HM(h,2,2)*MW_HM(h,3,3) - MW_HM(h,2,3)*MW_HM(h,3,2);
    MW_HM(rc,1,2) = MW_HM(h,2,3)*MW_HM(h,3,1) - MW_HM(h,2,1)*MW_HM(h,3,3);
    MW_HM(rc,1,3) = MW_HM(h,2,1)*MW_HM(h,3,2) - MW_HM(h,2,2)*MW_HM(h,3,1);
    MW_HM(rc,2,1) = MW_HM(h,1,3)*MW_HM(h,3,2) - MW_HM(h,1,2)*MW_HM(h,3,3);
    MW_HM(rc,2,2) = MW_HM(h,1,1)*MW_HM(h,3,3) - MW_HM(h,1,3)*MW_HM(h,3,1);
    MW_HM(rc,2,3) = MW_HM(h,1,2)*MW_HM(h,3,1) - MW_HM(h,1,1)*MW_HM(h,3,2);
    MW_HM(rc,3,1) = MW_HM(h,1,2)*MW_HM(h,2,3) - MW_HM(h,1,3)*MW_HM(h,2,2);
    MW_HM(rc,3,2) = MW_HM(h,1,3)*MW_HM(h,2,1) - MW_HM(h,1,1)*MW_HM(h,2,3);
    MW_HM(rc,3,3) = MW_HM(h,1,1)*MW_HM(h,2,2) - MW_HM(h,1,2)*MW_HM(h,2,1);
    const double vol = MW_HM(h,1,1)*MW_HM(rc,1,1) + MW_HM(h,1,2)*MW_HM(rc,1,2) + MW_HM(h,1,3)*MW_HM(rc,1,3);
    const double f = 2.0 * 3.141592653589793238462643383279502884197 / vol;
#pragma unroll
    for (int i = 0; i < 9; ++i) rc[i] *= f;
}

// Diagnostic build only (-DMW_SWEEP_STAMPS, tools/sweep_stamps.py): cycles of walker 0's first wavefront per phase of a round,
// summed over the launch into g_sweep_stamps[0..15] (mw_move_scan.hip.h holds the array and the stages of one evaluation).
#ifdef MW_SWEEP_STAMPS
#define MW_SW_NOW() ((blockIdx.x == 0 && wv == 0) ? (unsigned long long)clock64() : 0ull)
#define MW_SW_ACC(k, d) do { if (blockIdx.x == 0 && wv == 0 && lane == 0) g_sweep_stamps[k] += (d); } while (0)
#else
#define MW_SW_NOW() 0ull
#define MW_SW_ACC(k, d) do { } while (0)
#endif

#ifndef MW_BIG_WHEN
#define MW_BIG_WHEN ((SPEC > 1) ? 1 : 0)      // when the moments of walkers in global memory are asked for (move_energy_mom_wave: WHEN)
#endif

__device__ __forceinline__ double dev_det3(const double* m)                                   // util.f90:16-41
{
    double det = MW_HM(m,1,1) * (MW_HM(m,2,2) * MW_HM(m,3,3) - MW_HM(m,2,3) * MW_HM(m,3,2));
    det = det - MW_HM(m,1,2) * (MW_HM(m,2,1) * MW_HM(m,3,3) - MW_HM(m,2,3) * MW_HM(m,3,1));
    det = det + MW_HM(m,1,3) * (MW_HM(m,2,1) * MW_HM(m,3,2) - MW_HM(m,2,2) * MW_HM(m,3,1));
    return det;
}

// -------------------------------------------------------------------------------------
// The workgroup of a walker: one wavefront per lattice.  Each wavefront evaluates ITS lattice (the fused old/new local
// energy of a translation, the rescaled box of a volume move); wavefront 0 then takes the move's decision -- order
// parameter, weights, Metropolis test, Wang-Landau update, lattice switch -- and hands {accepted, active lattice} back.
// Two workgroup barriers per move for two lattices, none for one.
// -------------------------------------------------------------------------------------
template <int NW>                                           // NW = wavefronts in the workgroup
__device__ __forceinline__ void wg_sync()
{
    if constexpr (NW == 1) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
}
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

constexpr int kSweepQCap = 9;                             // in-range queue of a volume move's full-box energy: sized to fit the scratch record
// moves per batch of uniforms (Philox calls are lanes of one pass): 16, or 8 for the builds with volume moves -- 512 B of LDS that an
// NPT walker of the reference's examples does not have (sweep_lds); the smaller batch costs the translation-only build ~2 %
__host__ __device__ constexpr int sweep_batch(bool withvol, int spec = 1) { return spec > (withvol ? 8 : 16) ? spec : (withvol ? 8 : 16); }
constexpr unsigned kSweepScratch = (unsigned)((sizeof(WaveScratch) + 15) & ~(size_t)15);
constexpr unsigned kSweepScratchVol = (unsigned)(((kSweepQCap + 1) * 64 * sizeof(uint32_t)) > kSweepScratch ? ((kSweepQCap + 1) * 64 * sizeof(uint32_t)) : kSweepScratch);
static_assert(kSweepScratchVol == kSweepScratch, "the builds with volume moves take no more LDS per wavefront than the others");

// Dynamic LDS of a walker's workgroup (byte offsets), the same arithmetic on the host (launch size) and on the device.
// Every byte counts for the reference's own 48-molecule cells: eight walkers share a CU when a workgroup's static + dynamic
// LDS stays within 160 KiB / 8 = 20480 B (mw_sweep_translation_launch).
constexpr int MVS = 8;                                // doubles between two moves' {x, y, z, imol} (sweep_lds: mv)
struct SweepLds { unsigned iv, pos, tab, uni, mv, scr, row, nn, mom, lmask, inmask, rec, total, scr_bytes; };
// (a volume move's full-box energy by all wavefronts of the workgroup: two lattices entirely in LDS, four or more moves in flight)
__host__ __device__ constexpr bool sweep_split(int L, bool ldslist, bool withvol, int spec) { return ldslist && withvol && L == 2 && spec >= 4; }
__host__ __device__ inline SweepLds sweep_lds(int L, int nw, int ivcap, int N, int nbins, bool ldspos, bool ldslist, int rstride, bool withvol,
                                              bool samplerun, int spec = 1)
{
    SweepLds o;
    unsigned p = 0;
    o.iv = p;  p += (unsigned)L * ivcap * 24u;                         // image vectors [L][ivcap][3]
    o.pos = p; p += ldspos ? (unsigned)L * N * 24u : 0u;               // positions     [L][N][3]     (small systems)
    o.tab = p; p += L == 2 ? (samplerun ? 5u : 4u) * nbins * 8u : 0u;  // weight, mu_bin, binwidth, histogram; unbiased_hist in a sample run only
    o.uni = p; p += (unsigned)sweep_batch(withvol, spec) * 8u * 8u;    // uniforms of a batch of moves [kUB][8]
    o.mv = o.uni;                                                      // a translation's molecule + displacement {x, y, z, imol}: written over its
                                                                       // spent uniforms u0..u3 (a volume move keeps its own: it reads them again)
    p = (p + 15u) & ~15u;
    o.scr_bytes = withvol ? kSweepScratchVol : kSweepScratch;          // per wavefront: WaveScratch / the full-box energy's queue
    o.scr = p; p += (unsigned)nw * o.scr_bytes;
    o.row = p; p += ldslist ? (unsigned)L * N * rstride * 2u : 0u;     // list rows, 16-bit entries (j | image << 6; N <= 64)
    o.nn = p;  p += ldslist ? (unsigned)L * N : 0u;                    // row lengths, one byte each
    p = (p + 15u) & ~15u;
    // look-ahead builds (a handful of walkers: LDS to spare) keep the moment path's data here: every molecule's moments, current and
    // a volume move's trial set [2][L][N][kMomStride], and every row's molecules as a bit mask [L][N]
    const bool momlds = ldslist && spec > 1;
    o.mom = p;   p += momlds ? 2u * L * N * (unsigned)kMomStride * 8u : 0u;
    o.lmask = p; p += momlds ? (unsigned)L * N * 8u : 0u;
    const bool split = sweep_split(L, ldslist, withvol, spec);
    o.inmask = p; p += split ? (unsigned)L * N * 4u : 0u;
    p = (p + 15u) & ~15u;
    o.rec = p;    p += split ? (unsigned)L * N * 12u * 48u : 0u;              // [L][N][kSplitQ][6] doubles
    o.total = (p + 15u) & ~15u;
    return o;
}

}  // namespace mw
