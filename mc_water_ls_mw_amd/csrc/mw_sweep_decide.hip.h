// mw_sweep_decide.hip.h -- the Monte Carlo driver's decisions (wavefront 0 of a walker's workgroup): the walker's state between
// moves, the view of the kernel's LDS the decisions work on, and what accepts or rejects a translation or a volume move.
#pragma once

#include "mw_sweep_volume.hip.h"

namespace mw {

struct WalkerCtl {
    // the launch's parameters as this walker sees them (its own window, step sizes, increment)
    double beta, pressure, dref, av_binwidth, log_unbiased_norm, transP, ref1, ref2, wl_alpha, orig_wl_factor, mu_min, mu_max;
    double max_trans, dv_max;
    MuGridDev mg;                            // (mg.in_window changes at the top of a 'dd' cycle)
    int record, samplerun, always_switch, npt, swetnam, dd, minu, eq_cycles, nbins;
    int tab_small;                           // every |weight| < 2^20 (the lattice switch's shortcut; kept up with every update)
    // the walker's state between moves
    double men0, men1, ls_mu, gauge, wlf, sumh, cur_min, lgv12, lgv21;
    unsigned long long acc, nsw, nvol_try, nvol_acc;
    int ls, k_cur, k_valid, flag, cyc, within;
};

// What the decision routines below see of k_sweep's LDS: the walker's state, its cells' volumes and its tables, and the launch's sizes.
// Filled once in the kernel, after its __shared__ declarations.  (It holds what the lifted routines read; decide_round and post_move
// are still lambdas of the kernel and capture the rest.)
struct SweepView {
    WalkerCtl* ctl;
    double* svol;                             // the two cells' volumes
    double *sweight, *smub, *sbw;             // the walker's weight table and bin grid [nbins]
    int N, lane;
};

// The MINU branch of both move types: the lattice the move would end in; diffkT rewritten with the switch's terms if it differs.
// E = trial energies, V = trial volumes, Eb / Vb = energy and volume of the CURRENT lattice before the move.
__device__ __forceinline__ int dev_minu_branch(const WalkerCtl& sp, int ls, double E1, double E2, double V1, double V2,
                                               double Eb, double Vb, bool vol_terms, int N, double new_eta, double old_eta,
                                               double& diffkT)
{
    const double h1 = E1 + sp.pressure * V1 - sp.ref1, h2 = E2 + sp.pressure * V2 - sp.ref2;   // minloc, :1122-1126
    const int lsn = h2 < h1 ? 2 : 1;
    if (lsn != ls) {
        const double En = lsn == 1 ? E1 : E2, Vn = lsn == 1 ? V1 : V2;
        double d;
        if (vol_terms) d = sp.beta * En - sp.beta * Eb + sp.beta * sp.pressure * (Vn - Vb) - (double)N * fast_log_pos(Vn / Vb) + new_eta - old_eta;   // :1131-1133,1396-1397
        else           d = sp.beta * En - sp.beta * Eb + new_eta - old_eta;                                                                  // :1135
        if (sp.ref1 != 0.0 || sp.ref2 != 0.0)                                                                                               // leshift, :1134,1136,1398
            d = d - sp.beta * (lsn == 1 ? sp.ref1 : sp.ref2) + sp.beta * (ls == 1 ? sp.ref1 : sp.ref2);
        diffkT = d;
    }
    return lsn;
}

// mc_lattice_switch's exponent for a walker in lattice lsx with energies E0, E1 (:1557-1572) in two parts: the energy /
// volume terms that stand BEFORE "+ new_eta - old_eta" in the reference's expression, and the leshift terms added after it
__device__ __forceinline__ double switch_dk_terms(const SweepView& v, double E0, double E1, int lsx, double& lesh)
{
    WalkerCtl& C = *v.ctl; const int N = v.N; double* const svol = v.svol;
    const double Els = lsx == 1 ? E0 : E1, Elsn = lsx == 1 ? E1 : E0;
    const double V1 = svol[0], V2 = svol[1];
    const double Vls = lsx == 1 ? V1 : V2, Vlsn = lsx == 1 ? V2 : V1;
    double dk;
    if (C.npt) dk = C.beta * Elsn - C.beta * Els + C.beta * C.pressure * (Vlsn - Vls) - (double)N * (lsx == 1 ? C.lgv21 : C.lgv12);
    else       dk = C.beta * Elsn - C.beta * Els;
    lesh = lsx == 1 ? C.beta * C.dref : -(C.beta * C.dref);               // leshift: - beta ref(lsn) + beta ref(ls), :1567,1572
    return dk;
}
// ... and the whole of it less new_eta - old_eta (= eta_weight(ls_mu) - eta_weight(ls_mu): see post_move in k_sweep)
__device__ __forceinline__ double switch_dk(const SweepView& v, double E0, double E1, int lsx)
{
    double lesh;
    const double dk = switch_dk_terms(v, E0, E1, lsx, lesh);
    return dk + lesh;
}

// mc_volume's decision (wavefront 0; volume_move_wg calls it with the trial cells' full-box energies in every lane): svold = the old
// volumes, U = the move's uniforms; leaves diffkT for the move log and the walker's new state in *v.ctl.  Returns 1 if accepted.
template <int NLAT>
__device__ __forceinline__ int decide_volume(const SweepView& v, const double* svold, const double* U, double& diffkT, double e0n, double e1n, int anybad)
{
    WalkerCtl& C = *v.ctl; const int lane = v.lane; const int N = v.N; double* const svol = v.svol; double* const sweight = v.sweight;
    double* const smub = v.smub; double* const sbw = v.sbw;
    const double Vo0 = svold[0], Vo1 = NLAT == 2 ? svold[1] : 0.0;
    // wavefront 0: mc_volume's acceptance (:1361-1410) and, on rejection, the restored order parameter (:1514-1530)
    const double bk0 = C.men0, bk1 = C.men1;
    const int ls0 = C.ls;
    double ls_mu = C.ls_mu;
    int okv = 0, lsn = ls0;
    if (!anybad) {
        const double Vn0 = svol[0], Vn1 = NLAT == 2 ? svol[1] : 0.0;
        const double dE = (ls0 == 1 ? e0n - bk0 : e1n - bk1);                                // :1361
        const double Vls = ls0 == 1 ? Vn0 : Vn1, Vold = ls0 == 1 ? Vo0 : Vo1;
        double old_eta = 0.0, new_eta = 0.0;
        if (NLAT == 2) {                                                                        // :1363-1371
            double mu = (e0n + C.pressure * Vn0) - (e1n + C.pressure * Vn1);
            mu = mu - C.dref;                                                                // :1371 (leshift)
            mu = mu * C.beta - (double)N * fast_log_pos(Vn0 / Vn1);
            const double mul = lane == 0 ? ls_mu : mu;
            const double el = lane_eta(C.mg, sweight, smub, sbw, mul, lane_mu_to_bin(C.mg, mul));
            old_eta = readlane_f64(el, 0); new_eta = readlane_f64(el, 1);
            ls_mu = mu;
        }
        diffkT = C.beta * dE + new_eta - old_eta + C.beta * C.pressure * (Vls - Vold)
                 - (double)N * fast_log_pos(Vls / Vold);                                     // :1381-1382
        int minu_ls = ls0;
        if (C.minu && NLAT == 2)                                                                // :1385-1401
            minu_ls = dev_minu_branch(C, ls0, e0n, e1n, Vn0, Vn1, ls0 == 1 ? bk0 : bk1, Vold, true, N,
                                      new_eta, old_eta, diffkT);
        double cmp = exp_any(-diffkT);
        cmp = cmp > 1.0 ? 1.0 : cmp;
        okv = U[3] < cmp ? 1 : 0;                                                            // :1410
        if (okv) lsn = minu_ls;                                                              // :1426-1429
    }
    double m0 = e0n, m1 = e1n;
    if (!okv) {
        m0 = bk0; m1 = bk1;                                                                  // :1514
        if (NLAT == 2) {                                                                        // :1516-1520 (the OLD cells)
            double mu = (m0 + C.pressure * Vo0) - (m1 + C.pressure * Vo1);
            mu = mu - C.dref;                                                                // :1526 (leshift)
            mu = mu * C.beta - (double)N * fast_log_pos(Vo0 / Vo1);
            ls_mu = mu;
        }
    }
    if (lane == 0) { C.men0 = m0; C.men1 = m1; C.ls_mu = ls_mu; C.ls = lsn; }
    wave_sync();
    return okv;
}

}  // namespace mw
