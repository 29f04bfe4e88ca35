// mw_host_sweep.hip.h -- the device-resident Monte Carlo driver: its instantiations and every mw_sweep_* entry point.
#pragma once

extern "C" {

// The instantiations of the Monte Carlo driver: lattices per walker x residency (0: positions and rows from global memory /
// L2, 1: positions in LDS, 2: positions and list rows in LDS) x with / without volume moves; and look-ahead over 2 or 4 moves
// (wavefronts per workgroup = lattices x look-ahead) for every residency, 8 and 6 for one kind of walker each.
// X(lattices, look-ahead, positions in LDS, rows in LDS): each is built without and with volume moves.  (The order of this list is
// the order of the kernels in the code object.)
#define MW_SWEEP_BUILDS(X) \
    X(1, 1, false, false) X(1, 1, true, false) X(1, 1, true, true) \
    X(2, 1, false, false) X(2, 1, true, false) X(2, 1, true, true) \
    /* look-ahead 2 / 4, residency 0 */ \
    X(1, 2, false, false) X(1, 4, false, false) X(2, 2, false, false) X(2, 4, false, false) \
    /* the same for walkers entirely in LDS (residency 2): the reference's own handful of 48-molecule walkers is a handful of */ \
    /* chains, and their speed is the chain's */ \
    X(1, 2, true, true) X(1, 4, true, true) X(2, 2, true, true) X(2, 4, true, true) \
    /* ... and for the sizes in between (positions in LDS, rows in global memory) */ \
    X(1, 2, true, false) X(1, 4, true, false) X(2, 2, true, false) X(2, 4, true, false) \
    /* eight moves in flight: ONE lattice, walkers in global memory (a 4096-molecule box or a few of them) */ \
    X(1, 8, false, false) \
    /* six moves in flight: TWO lattices entirely in LDS (twelve wavefronts of the 168-register builds fill a CU: one walker per */ \
    /* CU -- the reference's handful of 48-molecule walkers) */ \
    X(2, 6, true, true)

static const void* sweep_kernel(int nlat, int residency, bool withvol, int spec)
{
    struct Build { int nlat, spec; bool ldspos, ldslist, withvol; const void* kern; };
#define MW_SWEEP_K(L, SP, P, R) {L, SP, P, R, false, reinterpret_cast<const void*>(&mw::k_sweep<L, SP, P, R, false>)}, \
                                {L, SP, P, R, true, reinterpret_cast<const void*>(&mw::k_sweep<L, SP, P, R, true>)},
    static const Build builds[] = {MW_SWEEP_BUILDS(MW_SWEEP_K)};
#undef MW_SWEEP_K
    // 8 and 6 only where they are built; any other look-ahead is 4 or 2
    const int ahead = (spec == 8 || spec == 6) ? spec : (spec > 1 ? (spec == 4 ? 4 : 2) : 1);
    for (const Build& b : builds)
        if (b.nlat == nlat && b.spec == ahead && b.ldspos == (residency >= 1) && b.ldslist == (residency == 2) && b.withvol == withvol) return b.kern;
    return nullptr;
}

int mw_sweep_configure(int nlat, double beta, double max_trans, int nbins, int eta_interp, int start_bin, int end_bin,
                       double r_pos, double a_pos, double r_neg, double a_neg, double mu_lo, double mu_hi,
                       const double* weight, const double* mu_bin, const double* binwidth)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (nlat != 1 && nlat != 2) return fail("mw_sweep_configure: num_lattices = %d (1 or 2)", nlat);
    if (g.nbox % nlat) return fail("mw_sweep_configure: %d boxes do not split into walkers of %d lattices", g.nbox, nlat);
    if (nlat == 2) {
        if (nbins < 3 || !weight || !mu_bin || !binwidth) return fail("mw_sweep_configure: two lattices need the weight tables");
        if (start_bin < 1 || end_bin > nbins || start_bin >= end_bin) return fail("mw_sweep_configure: bins %d..%d outside 1..%d", start_bin, end_bin, nbins);
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    g.sp.beta = beta; g.sp.max_trans = max_trans;
    g.sp.r_pos = r_pos; g.sp.a_pos = a_pos; g.sp.r_neg = r_neg; g.sp.a_neg = a_neg; g.sp.mu_lo = mu_lo; g.sp.mu_hi = mu_hi;
    g.sp.nlat = nlat; g.sp.nbins = nbins; g.sp.eta_interp = eta_interp; g.sp.start_bin = start_bin; g.sp.end_bin = end_bin; g.sp.pad = 0;
    g.sp.record = 0; g.sp.samplerun = 1; g.sp.always_switch = 0; g.sp.npt = 0;
    g.sp.av_binwidth = 1.0; g.sp.wl_factor = 0.0; g.sp.log_unbiased_norm = 0.0; g.sp.pressure = 0.0;
    g.sp.transP = 2.0; g.sp.dv_max = 0.0;       // translations only until mw_sweep_moves says otherwise
    const size_t nb = (size_t)(nbins > 0 ? nbins : 1);
    const size_t nw = (size_t)(g.nbox / nlat);
    if (dev_alloc(g.d_sw_mubin, nb) || dev_alloc(g.d_sw_binwidth, nb) || dev_alloc_zeroed(g.d_wweight, nw * nb) ||
        dev_alloc_zeroed(g.d_whist, nw * nb) || dev_alloc_zeroed(g.d_wuhist, nw * nb)) return 1;
    if (nlat == 2) {
        HIPCHK(hipMemcpy(g.d_sw_mubin, mu_bin, nb * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(g.d_sw_binwidth, binwidth, nb * sizeof(double), hipMemcpyHostToDevice));
        std::vector<double> all(nw * nb);
        for (size_t w = 0; w < nw; ++w) std::memcpy(&all[w * nb], weight, nb * sizeof(double));
        HIPCHK(hipMemcpy(g.d_wweight, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    g.nwalkers = g.nbox / nlat;
    const size_t nx = (size_t)g.nbox;
    if (!g.d_wls && (dev_alloc(g.d_wls, nx) || dev_alloc(g.d_wmu, nx) || dev_alloc(g.d_wacc, nx) || dev_alloc(g.d_wswitch, nx) ||
                     dev_alloc(g.d_wshift, nx) || dev_alloc(g.d_wvol, 2 * nx) || dev_alloc(g.d_wflag, nx) || dev_alloc(g.d_wwin, 4 * nx) ||
                     dev_alloc(g.d_wfac, nx) || dev_alloc(g.d_wsum, nx) || dev_alloc(g.d_winflag, nx) || dev_alloc(g.d_wstep, 2 * nx))) return 1;
    HIPCHK(hipMemset(g.d_wwin, 0, sizeof(double) * 4 * g.nbox));
    HIPCHK(hipMemset(g.d_wfac, 0, sizeof(double) * g.nbox));
    HIPCHK(hipMemset(g.d_wsum, 0, sizeof(double) * g.nbox));
    HIPCHK(hipMemset(g.d_winflag, 0, sizeof(int) * g.nbox));
    g.has_windows = false; g.has_steps = false;
    g.sp.dref = 0.0; g.sp.ref1 = g.sp.ref2 = 0.0; g.sp.minu = 0; g.sp.pad_minu = 0; g.sp.swetnam = 0; g.sp.dd = 0; g.sp.wl_alpha = 1.0; g.sp.orig_wl_factor = 0.0;
    g.sp.mu_min = mu_lo; g.sp.mu_max = mu_hi; g.sp.eq_cycles = 0; g.sp.in_window = 1;
    HIPCHK(hipMemset(g.d_wvol, 0, sizeof(unsigned long long) * 2 * g.nbox));
    HIPCHK(hipMemset(g.d_wflag, 0, sizeof(int) * g.nbox));
    HIPCHK(hipMemset(g.d_wswitch, 0, sizeof(unsigned long long) * g.nbox));
    HIPCHK(hipMemset(g.d_wshift, 0, sizeof(double) * g.nbox));
    std::vector<int> one((size_t)g.nbox, 1);
    HIPCHK(hipMemcpy(g.d_wls, one.data(), sizeof(int) * g.nbox, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(g.d_wmu, 0, sizeof(double) * g.nbox));
    HIPCHK(hipMemset(g.d_wacc, 0, sizeof(unsigned long long) * g.nbox));
    g.sweep_ready = true;
    return 0;
}

static int check_walker(int first, int count)
{
    if (!g.sweep_ready) return fail("mw_sweep: call mw_sweep_configure first");
    if (first < 1 || count < 1 || first + count - 1 > g.nwalkers)
        return fail("mw_sweep: walker range %d..%d outside 1..%d", first, first + count - 1, g.nwalkers);
    return 0;
}

int mw_sweep_set_state(int walker, int ls, double ls_mu)
{
    MW_LOCK;
    if (check_live() || check_walker(walker, 1)) return 1;
    if (ls < 1 || ls > g.sp.nlat) return fail("mw_sweep_set_state: active lattice %d outside 1..%d", ls, g.sp.nlat);
    HIPCHK(hipMemcpyAsync(g.d_wls + (walker - 1), &ls, sizeof(int), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(g.d_wmu + (walker - 1), &ls_mu, sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_sweep_set_states_range(int first_walker, int count, const int* ls, const double* ls_mu)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    if (!ls || !ls_mu) return fail("mw_sweep_set_states_range: null pointer");
    for (int k = 0; k < count; ++k)
        if (ls[k] < 1 || ls[k] > g.sp.nlat) return fail("mw_sweep_set_states_range: active lattice %d of walker %d outside 1..%d", ls[k], first_walker + k, g.sp.nlat);
    HIPCHK(hipMemcpyAsync(g.d_wls + (first_walker - 1), ls, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(g.d_wmu + (first_walker - 1), ls_mu, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_sweep_get_state(int walker, int* ls, double* ls_mu, double* model_energy, long long* accepted)
{
    MW_LOCK;
    if (check_live() || check_walker(walker, 1)) return 1;
    int l = 0; double mu = 0.0; unsigned long long a = 0; double e[2] = {0.0, 0.0};
    HIPCHK(hipMemcpyAsync(&l, g.d_wls + (walker - 1), sizeof(int), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(&mu, g.d_wmu + (walker - 1), sizeof(double), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(&a, g.d_wacc + (walker - 1), sizeof a, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(e, g.d_energy + (size_t)(walker - 1) * g.sp.nlat, sizeof(double) * g.sp.nlat, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    if (ls) *ls = l;
    if (ls_mu) *ls_mu = mu;
    if (accepted) *accepted = (long long)a;
    if (model_energy) { model_energy[0] = e[0]; if (g.sp.nlat == 2) model_energy[1] = e[1]; }
    return 0;
}

int mw_sweep_options(int record, int samplerun, int always_switch, int npt,
                     double av_binwidth, double wl_factor, double log_unbiased_norm, double pressure)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (!g.sweep_ready) return fail("mw_sweep_options: call mw_sweep_configure first");
    if ((record || always_switch) && g.sp.nlat != 2) return fail("mw_sweep_options: histograms and lattice switches need two lattices");
    g.sp.record = record ? 1 : 0; g.sp.samplerun = samplerun ? 1 : 0; g.sp.always_switch = always_switch ? 1 : 0; g.sp.npt = npt ? 1 : 0;
    g.sp.av_binwidth = av_binwidth; g.sp.wl_factor = wl_factor; g.sp.log_unbiased_norm = log_unbiased_norm; g.sp.pressure = pressure;
    if (g.sp.nlat == 2 && !g.sp.swetnam && !g.sp.dd) {           // one increment for every walker ('mw'); per-walker values: mw_sweep_set_factors
        std::vector<double> f((size_t)g.nwalkers, wl_factor);
        HIPCHK(hipMemcpyAsync(g.d_wfac, f.data(), sizeof(double) * g.nwalkers, hipMemcpyHostToDevice, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
    }
    return 0;
}

int mw_sweep_leshift(double ref_enthalpy_1, double ref_enthalpy_2)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (!g.sweep_ready) return fail("mw_sweep_leshift: call mw_sweep_configure first");
    g.sp.dref = ref_enthalpy_1 - ref_enthalpy_2;
    g.sp.ref1 = ref_enthalpy_1; g.sp.ref2 = ref_enthalpy_2;
    return 0;
}

int mw_sweep_minu(int on)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (!g.sweep_ready) return fail("mw_sweep_minu: call mw_sweep_configure first");
    if (on && g.sp.nlat != 2) return fail("mw_sweep_minu: needs two lattices per walker");
    g.sp.minu = on ? 1 : 0;
    return 0;
}

int mw_sweep_swetnam(int on, double wl_alpha, double orig_wl_factor, double mu_min, double mu_max)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (!g.sweep_ready) return fail("mw_sweep_swetnam: call mw_sweep_configure first");
    g.sp.swetnam = on ? 1 : 0; g.sp.wl_alpha = wl_alpha; g.sp.orig_wl_factor = orig_wl_factor;
    g.sp.mu_min = mu_min; g.sp.mu_max = mu_max;
    return 0;
}

int mw_sweep_dd(int on, int eq_mc_cycles)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (!g.sweep_ready) return fail("mw_sweep_dd: call mw_sweep_configure first");
    g.sp.dd = on ? 1 : 0; g.sp.eq_cycles = eq_mc_cycles;
    return 0;
}

int mw_sweep_windows(int first_walker, int count, const int* start_bin, const int* end_bin, const double* mu_lo, const double* mu_hi)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    if (!start_bin || !end_bin || !mu_lo || !mu_hi) { g.has_windows = false; return 0; }
    std::vector<double> w((size_t)count * 4);
    for (int k = 0; k < count; ++k) {
        if (start_bin[k] < 1 || end_bin[k] > g.sp.nbins || start_bin[k] >= end_bin[k])
            return fail("mw_sweep_windows: walker %d has bins %d..%d outside 1..%d", first_walker + k, start_bin[k], end_bin[k], g.sp.nbins);
        w[4 * (size_t)k] = start_bin[k]; w[4 * (size_t)k + 1] = end_bin[k]; w[4 * (size_t)k + 2] = mu_lo[k]; w[4 * (size_t)k + 3] = mu_hi[k];
    }
    if (!g.has_windows) {        // walkers outside the range given keep the window of mw_sweep_configure
        std::vector<double> all((size_t)g.nwalkers * 4);
        for (int k = 0; k < g.nwalkers; ++k) { all[4 * (size_t)k] = g.sp.start_bin; all[4 * (size_t)k + 1] = g.sp.end_bin; all[4 * (size_t)k + 2] = g.sp.mu_lo; all[4 * (size_t)k + 3] = g.sp.mu_hi; }
        HIPCHK(hipMemcpyAsync(g.d_wwin, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
    }
    HIPCHK(hipMemcpyAsync(g.d_wwin + 4 * (size_t)(first_walker - 1), w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    g.has_windows = true;
    return 0;
}

int mw_sweep_set_factors(int first_walker, int count, const double* wl_factor, const double* sumhist)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    if (wl_factor) HIPCHK(hipMemcpyAsync(g.d_wfac + (first_walker - 1), wl_factor, sizeof(double) * count, hipMemcpyHostToDevice, g.stream));
    if (sumhist) HIPCHK(hipMemcpyAsync(g.d_wsum + (first_walker - 1), sumhist, sizeof(double) * count, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_sweep_get_factors(int first_walker, int count, double* wl_factor, double* sumhist, int* in_window)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    if (wl_factor) HIPCHK(hipMemcpyAsync(wl_factor, g.d_wfac + (first_walker - 1), sizeof(double) * count, hipMemcpyDeviceToHost, g.stream));
    if (sumhist) HIPCHK(hipMemcpyAsync(sumhist, g.d_wsum + (first_walker - 1), sizeof(double) * count, hipMemcpyDeviceToHost, g.stream));
    if (in_window) HIPCHK(hipMemcpyAsync(in_window, g.d_winflag + (first_walker - 1), sizeof(int) * count, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_sweep_steps(int first_walker, int count, const double* max_trans_bohr, const double* dv_max_bohr)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    if (!max_trans_bohr || !dv_max_bohr) { g.has_steps = false; return 0; }
    if (!g.has_steps) {          // walkers outside the range given keep the common values
        std::vector<double> all((size_t)g.nwalkers * 2);
        for (int k = 0; k < g.nwalkers; ++k) { all[2 * (size_t)k] = g.sp.max_trans; all[2 * (size_t)k + 1] = g.sp.dv_max; }
        HIPCHK(hipMemcpyAsync(g.d_wstep, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
    }
    std::vector<double> w((size_t)count * 2);
    for (int k = 0; k < count; ++k) {
        if (!(max_trans_bohr[k] > 0.0) || !(dv_max_bohr[k] >= 0.0)) return fail("mw_sweep_steps: walker %d has step sizes %g, %g", first_walker + k, max_trans_bohr[k], dv_max_bohr[k]);
        w[2 * (size_t)k] = max_trans_bohr[k]; w[2 * (size_t)k + 1] = dv_max_bohr[k];
    }
    HIPCHK(hipMemcpyAsync(g.d_wstep + 2 * (size_t)(first_walker - 1), w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    g.has_steps = true;
    return 0;
}

int mw_sweep_get_counters(int first_walker, int count, long long* accepted, long long* vol_attempted, long long* vol_accepted)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    std::vector<unsigned long long> a((size_t)count), v((size_t)count * 2);
    HIPCHK(hipMemcpyAsync(a.data(), g.d_wacc + (first_walker - 1), sizeof(unsigned long long) * count, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(v.data(), g.d_wvol + 2 * (size_t)(first_walker - 1), sizeof(unsigned long long) * 2 * count, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    for (int k = 0; k < count; ++k) {
        if (accepted) accepted[k] = (long long)a[(size_t)k];
        if (vol_attempted) vol_attempted[k] = (long long)v[2 * (size_t)k];
        if (vol_accepted) vol_accepted[k] = (long long)v[2 * (size_t)k + 1];
    }
    return 0;
}

int mw_sweep_moves(double transP, double dv_max_bohr)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (!g.sweep_ready) return fail("mw_sweep_moves: call mw_sweep_configure first");
    if (!(transP > 0.0)) return fail("mw_sweep_moves: transP = %g must be positive", transP);
    g.sp.transP = transP; g.sp.dv_max = dv_max_bohr;
    if (transP < 1.0) {
        // volume moves shrink cells on the device: keep room for one more shell of images along any one axis
        // (a move that still outgrows the table is rejected and flagged, mw_sweep_check_flags)
        int need = g.ivcap;
        for (int b = 0; b < g.nbox; ++b) {
            const int* im = g.h_grid[(size_t)b].im;
            if (g.h_nivect[(size_t)b] < 1) continue;
            const int w0 = 2 * im[0] + 1, w1 = 2 * im[1] + 1, w2 = 2 * im[2] + 1;
            need = std::max(need, std::max((w0 + 2) * w1 * w2, std::max(w0 * (w1 + 2) * w2, w0 * w1 * (w2 + 2))));
        }
        if (need > MW_MAX_IVECT) need = MW_MAX_IVECT;
        if (need > g.ivcap && grow_ivcap(need)) return 1;
    }
    return 0;
}

int mw_sweep_check_flags(int first_walker, int count)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    std::vector<int> flags((size_t)count, 0);
    HIPCHK(hipMemcpyAsync(flags.data(), g.d_wflag + (first_walker - 1), sizeof(int) * count, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    for (int w = 0; w < count; ++w) {
        if (flags[(size_t)w] & 1)
            return fail("mw_sweep: a volume move of walker %d shrank a cell below what %d image vectors cover (the move was rejected)",
                        first_walker + w, g.ivcap);
        if (flags[(size_t)w] & 2)
            return fail("Error : Not all walkers have reached their designated window after %d MC cycles (walker %d)",
                        g.sp.eq_cycles, first_walker + w);
    }
    return 0;
}

int mw_sweep_get_volume_moves(int walker, long long* attempted, long long* accepted)
{
    MW_LOCK;
    if (check_live() || check_walker(walker, 1)) return 1;
    unsigned long long v[2];
    int flag = 0;
    HIPCHK(hipMemcpyAsync(v, g.d_wvol + 2 * (size_t)(walker - 1), sizeof v, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(&flag, g.d_wflag + (walker - 1), sizeof(int), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    if (attempted) *attempted = (long long)v[0];
    if (accepted) *accepted = (long long)v[1];
    if (flag & 1) return fail("mw_sweep: a volume move of walker %d shrank a cell below what %d image vectors cover", walker, g.ivcap);
    return 0;
}

// After volume moves on the device the host mirrors of the cells (image vectors, neighbour-grid descriptors)
// are stale: read the cells back and rebuild them exactly as mw_set_cell does.  Call before rebuilding lists.
int mw_sweep_sync_cells(int first_ils, int count, double* h_out)
{
    MW_LOCK;
    if (check_live() || check_range(first_ils, count)) return 1;
    std::vector<double> h((size_t)count * 9);
    std::vector<int> flags((size_t)g.nbox, 0);
    HIPCHK(hipMemcpyAsync(h.data(), g.d_hmat + 9 * (size_t)(first_ils - 1), h.size() * sizeof(double), hipMemcpyDeviceToHost, g.stream));
    if (g.d_wflag) HIPCHK(hipMemcpyAsync(flags.data(), g.d_wflag, sizeof(int) * g.nbox, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    for (int w = 0; w < g.nbox; ++w)
        if (flags[(size_t)w] & 1) return fail("mw_sweep: a volume move of walker %d shrank a cell below what %d image vectors cover", w + 1, g.ivcap);
    // host mirrors for every box, then four bulk uploads (the device already holds these image vectors: same arithmetic).
    // A farm calls this before every list rebuild for thousands of boxes: the boxes are shared out among the host's cores
    // (one thread did 16 384 boxes in 3.5 ms, ten times per hundred cycles -- an eighth of an NPT farm's wall time).
    std::atomic<int> bad_box{-1}, bad_n{0};
    auto mirror = [&](int lo, int hi) {
        std::vector<double> iv;
        for (int b = lo; b < hi; ++b) {
            const int box = first_ils - 1 + b;
            int imv[3] = {1, 1, 1};
            const int n = host_ivects(&h[(size_t)b * 9], iv, imv);
            if (n < 0 || n > g.ivcap) { int none = -1; if (bad_box.compare_exchange_strong(none, box)) bad_n = n; return; }
            std::memcpy(&g.h_ivect[(size_t)box * g.ivcap * 3], iv.data(), iv.size() * sizeof(double));
            g.h_nivect[box] = n;
            g.h_grid[box] = make_grid(&h[(size_t)b * 9], imv, g.cstride);
            g.h_usegrid[box] = (!g.force_brute && g.h_grid[box].nc[0] > 0) ? 1 : 0;
            if (!g.h_usegrid[box]) g.h_grid[box].nc[0] = 0;
            if (h_out) std::memcpy(h_out + (size_t)b * 9, &h[(size_t)b * 9], 9 * sizeof(double));
        }
    };
    const int nthr = std::max(1, std::min({(int)std::thread::hardware_concurrency(), 16, count / 512}));
    if (nthr == 1) mirror(0, count);
    else {
        std::vector<std::thread> pool;
        for (int t = 0; t < nthr; ++t)
            pool.emplace_back(mirror, (int)((long long)count * t / nthr), (int)((long long)count * (t + 1) / nthr));
        for (auto& th : pool) th.join();
    }
    if (bad_box.load() >= 0)
        return fail("mw_sweep_sync_cells: box %d needs %d image vectors (capacity %d)", bad_box.load() + 1, bad_n.load(), g.ivcap);
    // What goes back to the device is what only the host works out: which boxes take the cell-grid list builder, and their
    // grid descriptors.  The image vectors do NOT: the volume moves rebuilt them on the device in the reference's order and
    // arithmetic (dev_compute_ivects), so the device's tables already equal the mirrors just computed -- 19 MB per call for
    // 16 384 boxes that used to be uploaded regardless, 3 ms of an idle GPU before every list rebuild of an NPT farm.
    // MW_SYNC_CELLS_VERIFY=1 reads the device's tables back instead and compares them bit for bit (tests).
    const size_t b0 = (size_t)(first_ils - 1);
    bool any_grid = g.grid_on_device;
    for (int b = 0; b < count; ++b) any_grid = any_grid || g.h_usegrid[b0 + b] != 0;
    if (any_grid) {
        HIPCHK(hipMemcpyAsync(g.d_grid + b0, &g.h_grid[b0], sizeof(mw::GridDesc) * count, hipMemcpyHostToDevice, g.stream));
        g.grid_on_device = true;
    }
    HIPCHK(hipMemcpyAsync(g.d_usegrid + b0, &g.h_usegrid[b0], sizeof(int) * count, hipMemcpyHostToDevice, g.stream));
    static const bool verify = [] { const char* e = std::getenv("MW_SYNC_CELLS_VERIFY"); return e && std::atoi(e) != 0; }();
    if (verify) {
        std::vector<double> div((size_t)count * g.ivcap * 3);
        std::vector<int> dn((size_t)count);
        HIPCHK(hipMemcpyAsync(div.data(), g.d_ivect + b0 * g.ivcap * 3, div.size() * sizeof(double), hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipMemcpyAsync(dn.data(), g.d_nivect + b0, dn.size() * sizeof(int), hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
        for (int b = 0; b < count; ++b) {
            const int n = g.h_nivect[b0 + b];
            if (dn[(size_t)b] != n)
                return fail("mw_sweep_sync_cells: box %d has %d image vectors on the device, %d by the host's arithmetic", (int)b0 + b + 1, dn[(size_t)b], n);
            if (std::memcmp(&div[(size_t)b * g.ivcap * 3], &g.h_ivect[(b0 + b) * g.ivcap * 3], sizeof(double) * 3 * n) != 0)
                return fail("mw_sweep_sync_cells: the device's image vectors of box %d differ from the host's", (int)b0 + b + 1);
        }
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

static int tables_io(int walker, double* weight, double* hist, double* uhist, bool put)
{
    if (check_live() || check_walker(walker, 1)) return 1;
    const size_t nb = (size_t)g.sp.nbins, off = (size_t)(walker - 1) * nb;
    double* dev[3] = {g.d_wweight + off, g.d_whist + off, g.d_wuhist + off};
    double* host[3] = {weight, hist, uhist};
    for (int t = 0; t < 3; ++t) {
        if (!host[t]) continue;
        if (put) HIPCHK(hipMemcpyAsync(dev[t], host[t], nb * sizeof(double), hipMemcpyHostToDevice, g.stream));
        else     HIPCHK(hipMemcpyAsync(host[t], dev[t], nb * sizeof(double), hipMemcpyDeviceToHost, g.stream));
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_sweep_get_tables(int walker, double* weight, double* histogram, double* unbiased_hist)
{
    MW_LOCK;
    return tables_io(walker, weight, histogram, unbiased_hist, false);
}

int mw_sweep_set_tables(int walker, const double* weight, const double* histogram, const double* unbiased_hist)
{
    MW_LOCK;
    return tables_io(walker, const_cast<double*>(weight), const_cast<double*>(histogram), const_cast<double*>(unbiased_hist), true);
}

int mw_sweep_get_tables_range(int first_walker, int count, double* weight, double* histogram, double* unbiased_hist)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    const size_t nb = (size_t)g.sp.nbins, off = (size_t)(first_walker - 1) * nb, bytes = (size_t)count * nb * sizeof(double);
    if (weight) HIPCHK(hipMemcpyAsync(weight, g.d_wweight + off, bytes, hipMemcpyDeviceToHost, g.stream));
    if (histogram) HIPCHK(hipMemcpyAsync(histogram, g.d_whist + off, bytes, hipMemcpyDeviceToHost, g.stream));
    if (unbiased_hist) HIPCHK(hipMemcpyAsync(unbiased_hist, g.d_wuhist + off, bytes, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_sweep_set_tables_range(int first_walker, int count, const double* weight, const double* histogram, const double* unbiased_hist)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    const size_t nb = (size_t)g.sp.nbins, off = (size_t)(first_walker - 1) * nb, bytes = (size_t)count * nb * sizeof(double);
    if (weight) HIPCHK(hipMemcpyAsync(g.d_wweight + off, weight, bytes, hipMemcpyHostToDevice, g.stream));
    if (histogram) HIPCHK(hipMemcpyAsync(g.d_whist + off, histogram, bytes, hipMemcpyHostToDevice, g.stream));
    if (unbiased_hist) HIPCHK(hipMemcpyAsync(g.d_wuhist + off, unbiased_hist, bytes, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_sweep_get_shifts_range(int first_walker, int count, double* shifts, int reset)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    if (shifts) HIPCHK(hipMemcpyAsync(shifts, g.d_wshift + (first_walker - 1), sizeof(double) * count, hipMemcpyDeviceToHost, g.stream));
    if (reset) HIPCHK(hipMemsetAsync(g.d_wshift + (first_walker - 1), 0, sizeof(double) * count, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

// sum over the walkers of (table + shift - last), per table and bin; NULL last_* / sum_* skips a table
int mw_sweep_reduce_tables(int first_walker, int count, const double* last_w, const double* last_h, const double* last_u,
                           double* sum_w, double* sum_h, double* sum_u, int use_shifts, int reset_shifts)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    const int nb = g.sp.nbins, nchunks = (count + mw::kTableChunk - 1) / mw::kTableChunk;
    const size_t need = (size_t)nb * (6 + (size_t)nchunks);
    if (dev_grow(g.d_tabscratch, g.tabscratch_n, need, need)) return 1;
    const double* last[3] = {last_w, last_h, last_u};
    double* out[3] = {sum_w, sum_h, sum_u};
    const double* tabs[3] = {g.d_wweight, g.d_whist, g.d_wuhist};
    double* d_last = g.d_tabscratch, *d_out = g.d_tabscratch + 3 * (size_t)nb, *d_part = g.d_tabscratch + 6 * (size_t)nb;
    for (int t = 0; t < 3; ++t) {
        if (!last[t] || !out[t]) continue;
        HIPCHK(hipMemcpyAsync(d_last + (size_t)t * nb, last[t], sizeof(double) * nb, hipMemcpyHostToDevice, g.stream));
        hipLaunchKernelGGL(mw::k_tables_partial, dim3(nchunks), dim3(128), 0, g.stream, tabs[t],
                           (t == 0 && use_shifts) ? (const double*)g.d_wshift : (const double*)nullptr,
                           d_last + (size_t)t * nb, d_part, nb, first_walker - 1, count);
        hipLaunchKernelGGL(mw::k_tables_final, dim3(1), dim3(128), 0, g.stream, d_part, d_out + (size_t)t * nb, nb, nchunks);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out[t], d_out + (size_t)t * nb, sizeof(double) * nb, hipMemcpyDeviceToHost, g.stream));
    }
    if (reset_shifts) HIPCHK(hipMemsetAsync(g.d_wshift + (first_walker - 1), 0, sizeof(double) * count, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

// the same row for every walker of the range; NULL skips a table
int mw_sweep_broadcast_tables(int first_walker, int count, const double* weight, const double* histogram, const double* unbiased_hist)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    const int nb = g.sp.nbins;
    if (dev_grow(g.d_tabscratch, g.tabscratch_n, (size_t)nb * 6, (size_t)nb * 8)) return 1;
    const double* rows[3] = {weight, histogram, unbiased_hist};
    double* tabs[3] = {g.d_wweight, g.d_whist, g.d_wuhist};
    for (int t = 0; t < 3; ++t) {
        if (!rows[t]) continue;
        double* d_row = g.d_tabscratch + (size_t)t * nb;
        HIPCHK(hipMemcpyAsync(d_row, rows[t], sizeof(double) * nb, hipMemcpyHostToDevice, g.stream));
        hipLaunchKernelGGL(mw::k_tables_broadcast, dim3(count), dim3(128), 0, g.stream, tabs[t], (const double*)d_row, nb, first_walker - 1);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_sweep_get_switches(int walker, long long* switches)
{
    MW_LOCK;
    if (check_live() || check_walker(walker, 1)) return 1;
    unsigned long long v = 0;
    HIPCHK(hipMemcpyAsync(&v, g.d_wswitch + (walker - 1), sizeof v, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    *switches = (long long)v;
    return 0;
}

int mw_sweep_lds_bytes(int nlat, int nwater, int nbins, int row_stride, int volume_moves, int samplerun, int image_capacity)
{
    if (nlat < 1 || nlat > 2 || nwater < 1 || nwater > 64 || nbins < 0 || row_stride < 2 || row_stride > 32 ||
        image_capacity < 0 || image_capacity > MW_MAX_IVECT) return -1;
    // image vectors per box: what the engine starts with (mw_init); with volume moves, room for one more shell of images
    // along one axis (mw_sweep_moves) -- 45 -> 48 for the 27-image cells of the reference's examples
    const int ivcap = image_capacity > 0 ? image_capacity : (volume_moves ? 48 : 32);
    return (int)mw::sweep_lds(nlat, nlat, ivcap, nwater, nbins, true, true, row_stride, volume_moves != 0, samplerun != 0).total;
}

int mw_sweep_translation_launch(int first_walker, int count, int nmoves, unsigned long long seed, unsigned long long move0, int want_log)
{
    MW_LOCK;
    if (check_live() || check_walker(first_walker, count)) return 1;
    if (nmoves < 0) return fail("mw_sweep_translation: nmoves = %d", nmoves);
    if (nmoves == 0) return 0;
    double* dlog = nullptr;
    if (want_log) {
        const size_t need = (size_t)count * nmoves * 8;
        if (dev_grow(g.d_swlog, g.swlog_cap, need, need)) return 1;
        dlog = g.d_swlog;
    }
    const int L = g.sp.nlat;
    const bool withvol = g.sp.transP < 1.0;          // volume moves: the build that carries mc_volume
    // Residency of a walker's data in LDS.  Small systems (the reference's own 48-molecule cells): positions, and -- when an
    // entry (j, image) fits 16 bits (N <= 64) and no row is longer than 32 -- list rows and row lengths too, so that nothing
    // in the move loop waits on global memory.  Eight walkers per CU (16 wavefronts of <= 128 VGPRs) want <= 20 KiB each.
    const size_t pos_bytes = (size_t)L * g.N * 3 * sizeof(double);
    const bool ldspos = pos_bytes <= 16 * 1024;
    bool ldslist = false;
    int rstride = 32;
    if (ldspos && g.N <= 64) {
        if (g.nnmax_version != g.list_version) {     // once per list rebuild: the longest row of ANY box
            std::vector<int> st((size_t)g.nbox * 2);
            HIPCHK(hipMemcpyAsync(st.data(), g.d_stats, st.size() * sizeof(int), hipMemcpyDeviceToHost, g.stream));
            HIPCHK(hipStreamSynchronize(g.stream));
            int mx = 0;
            for (size_t b = 0; b < st.size() / 2; ++b) mx = std::max(mx, st[2 * b + 1]);
            g.nnmax_cached = mx;                     // stats = {min nn, max nn} of the last list build of each box
            g.nnmax_version = g.list_version;
        }
        if (g.nnmax_cached <= 32) {                  // rows as short as the lists allow (entries are read one at a time: any even
            rstride = std::max(4, (g.nnmax_cached + 1) & ~1);      // stride will do): LDS per walker sets the occupancy -- a replica farm's
            ldslist = mw::sweep_lds(L, L, g.ivcap, g.N, g.sp.nbins, true, true, rstride, withvol, g.sp.samplerun != 0).total <= 24 * 1024;
        }                                            // longest row of 16 384 boxes grows from 22 to 26 entries as the walkers spread out
                                                     // (at a stride of 28 a walker went over 20 KiB: seven per CU instead of eight, -12 %)
    }
    // Look-ahead: as many moves at once as it takes to put ~4 wavefronts on every SIMD, at most 4; MW_SWEEP_AHEAD=1|2|4 overrides.
    // For walkers in global memory, and for walkers entirely in LDS (the reference's 48-molecule cells: a move reads most of such
    // a box, so any ACCEPTED move ends the round -- but nine moves in ten are rejected, and a handful of walkers, which is how the
    // reference itself runs, leaves the chip to their chains), and for the sizes in between.
    int spec = 1;
    {
        // ... as long as every walker of the launch still has a place on the chip: a compute unit holds 16 wavefronts of <= 128
        // VGPRs (12 of the one build that needs more), i.e. 16 / (lattices x look-ahead) workgroups.  Measured on 48-molecule pairs
        // (tools/sweep_measurements.py n48wl_<walkers> / n48npt_<walkers>): 4 ahead wins up to 512 walkers (256 with volume moves),
        // 2 ahead up to 1024 (768), and past that look-ahead only takes places away from other walkers.
        auto all_resident = [&](int ahead) {
            const int per_cu = ((L == 2 && ahead > 1) ? 12 : 16) / (L * ahead);   // (two lattices with look-ahead: the builds of <= 168 VGPRs)
            return (long long)count <= (long long)g.cu * per_cu;
        };
        spec = all_resident(4) ? 4 : (all_resident(2) ? 2 : 1);
        // eight in flight for one-lattice walkers in global memory (large boxes: consecutive moves seldom touch the same molecules)
        const bool has8 = L == 1 && !ldspos;
        if (has8 && all_resident(8)) spec = 8;
        // six for two-lattice walkers entirely in LDS, while there is a CU for each (a round ends with its first accepted move: 3.1 moves
        // per round of four at 16 % acceptance, 4.0 per round of six)
        const bool has6 = L == 2 && ldslist;
        if (has6 && all_resident(6)) spec = 6;
        if (const char* e = getenv("MW_SWEEP_AHEAD")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4 || (v == 8 && has8) || (v == 6 && has6)) spec = v; }
        if (want_log) spec = std::min(spec, g.sweep_log_ahead);
    }
    const mw::SweepLds lay = mw::sweep_lds(L, L * spec, g.ivcap, g.N, g.sp.nbins, ldspos, ldslist, rstride, withvol, g.sp.samplerun != 0, spec);
    const size_t static_lds = 1536;                  // cells and their backups, hand-over words, the walker's control block (generous bound)
    if (lay.total + static_lds > (size_t)160 * 1024 - 8 * 1024)
        return fail("mw_sweep: %u bytes of LDS per walker (image vectors %u, positions %u, list rows %u) exceed what a workgroup may have",
                    lay.total, lay.pos - lay.iv, lay.tab - lay.pos, lay.nn - lay.row);
    const void* kern = sweep_kernel(L, ldslist ? 2 : (ldspos ? 1 : 0), withvol, spec);
    const double* wwin = g.has_windows ? (const double*)g.d_wwin : (const double*)nullptr;
    const double* wstep = g.has_steps ? (const double*)g.d_wstep : (const double*)nullptr;
    int w0 = first_walker - 1;
    // the moment path of walkers entirely in LDS (mw_sweep.hip.h): 2 x L x N x kMomStride doubles of scratch per walker of the launch
    // (MW_SWEEP_MOMENTS=0: the row-scanning evaluation instead)
    double* wmom = nullptr;
    drop_move_counts();                              // (the driver moves molecules)
    {
        const char* e = getenv("MW_SWEEP_MOMENTS");
        const int box_first = (first_walker - 1) * L + 1, nboxes = count * L;          // 1-based
        // (for launches that fill the chip -- four lattices per compute unit and up: 4096-molecule boxes x 512 / 1024 / 2048 walkers
        //  -12 / +4 / +25 %, 2048 x 1536 pairs +22 %; fewer walkers run their chains with look-ahead, where every moment is a global
        //  round trip on a chain's critical path.
        //  By the NUMBER of walkers, not by the look-ahead chosen for them: a launch's chain must not depend on its look-ahead.
        //  MW_SWEEP_MOMENTS=2 forces the path -- the tests', to hold it to the oracle and to itself across look-aheads on a few walkers)
        if (!ldslist && !withvol && !(e && e[0] == '0') && model_geo(nboxes).lds && g.N >= 128 && (nboxes >= 4 * g.cu || (e && e[0] == '2'))) {
            // walkers in global memory, translations only: the engine's own moments, made by the full-box kernel where the driver's
            // earlier launches have not kept them (its `MOMOUT` build: boxes that fit LDS), current afterwards for as long as nothing
            // else writes positions or cells (swm_first / swm_count)
            const bool current = g.d_mom && g.swm_count > 0 && g.swm_first <= box_first && box_first + nboxes <= g.swm_first + g.swm_count;
            if (!current) {
                if (launch_model_energy(box_first, nboxes, true, false)) return 1;
                g.mom_count = 0;                                   // (about to change under the batch kernels' feet)
            }
            g.swm_first = current ? g.swm_first : box_first; g.swm_count = current ? g.swm_count : nboxes;
            wmom = g.d_mom + (size_t)(box_first - 1) * g.N * mw::kMomStride;
        } else {
            drop_driver_moments();                                 // (this launch moves molecules without keeping d_mom)
        }
        if (ldslist && !(e && e[0] == '0')) {
            const size_t need = (size_t)count * 2 * L * g.N * mw::kMomStride;
            if (dev_grow(g.d_wmom, g.wmom_cap, need, need)) return 1;
            wmom = g.d_wmom;
        }
    }
    void* args[] = {&g.d_pos, &g.d_hmat, &g.d_ivect, &g.d_nivect, &g.d_listm, &g.d_list, &g.d_nn, &g.d_order, &g.d_nns, &g.d_cmax,
                    &g.d_energy, &g.d_wls, &g.d_wmu, &g.d_wacc, &g.d_wswitch, &g.d_wshift, &g.sp, &g.d_wweight, &g.d_whist, &g.d_wuhist,
                    &g.d_sw_mubin, &g.d_sw_binwidth, &g.d_volume, &g.d_wvol, &g.d_wflag, &g.N, &g.S, &g.ivcap, &nmoves, &seed, &move0,
                    &w0, &dlog, &rstride, &wwin, &g.d_wfac, &g.d_wsum, &g.d_winflag, &wstep, &wmom};
    HIPCHK(hipLaunchKernel(kern, dim3(count), dim3(64 * L * spec), args, lay.total, g.stream));
    HIPCHK(hipGetLastError());
    g.last_sweep[0] = L; g.last_sweep[1] = spec; g.last_sweep[2] = ldslist ? 2 : (ldspos ? 1 : 0); g.last_sweep[3] = withvol ? 1 : 0;
    g.last_sweep[4] = (int)lay.total; g.last_sweep[5] = ldslist ? rstride : 0;
    return 0;
}

int mw_sweep_last_launch(int* nlat, int* ahead, int* residency, int* volume_moves, int* lds_bytes, int* row_stride)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (g.last_sweep[0] == 0) return fail("mw_sweep_last_launch: no launch of the driver yet");
    int* out[6] = {nlat, ahead, residency, volume_moves, lds_bytes, row_stride};
    for (int k = 0; k < 6; ++k) if (out[k]) *out[k] = g.last_sweep[k];
    return 0;
}

int mw_sweep_translation(int first_walker, int count, int nmoves, unsigned long long seed, unsigned long long move0, double* log)
{
    MW_LOCK;
    if (mw_sweep_translation_launch(first_walker, count, nmoves, seed, move0, log != nullptr)) return 1;
    if (log && nmoves > 0)
        HIPCHK(hipMemcpyAsync(log, g.d_swlog, sizeof(double) * (size_t)count * nmoves * 8, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

#ifdef MW_SWEEP_STAMPS
// Diagnostic build only (tools/sweep_stamps.py): the cycle sums of walker 0's first wavefront; reset != 0 zeroes them afterwards.
int mw_debug_sweep_stamps(unsigned long long* out, int n, int reset)
{
    MW_LOCK;
    if (check_live()) return 1;
    unsigned long long st[48];
    HIPCHK(hipStreamSynchronize(g.stream));
    HIPCHK(hipMemcpyFromSymbol(st, HIP_SYMBOL(mw::g_sweep_stamps), sizeof st));
    for (int k = 0; k < n && k < 48; ++k) out[k] = st[k];
    if (reset) { memset(st, 0, sizeof st); HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(mw::g_sweep_stamps), st, sizeof st)); }
    return 0;
}
#endif

}  // extern "C"
