// mw_host_analysis.hip.h -- what is computed from a configuration besides its energy: forces and virials, CHILL+ ice
// classes and bonds, ice clusters, pair-distance histograms.
#pragma once

namespace {

// Forces and virials of boxes first .. first+count-1 (mw_forces.hip.h): the moments and energies of the current positions,
// then the force pass over the same positions and lists, then the fixed-order virial sums.  The force pass's geometry depends
// on N only: one workgroup of 1024 per box with the box staged in LDS where it fits, else ceil(N / 256) workgroups of 256.
// timer_slot >= 0: event timers timer_slot (moment pass) and timer_slot + 1 (force pass).
constexpr int kForceBlockLds = 1024, kForceBlockGlobal = 256;
int launch_model_forces(const char* who, int first, int count, int timer_slot)
{
    Timers t;
    if (t.open(who, timer_slot, 2)) return 1;
    const bool lds = lds_fits(g.N, g.ivcap);
    const int nsplit = lds ? 1 : (g.N + kForceBlockGlobal - 1) / kForceBlockGlobal;
    if (!g.d_force && (dev_alloc(g.d_force, (size_t)g.nbox * g.N * 3) || dev_alloc(g.d_virial, (size_t)g.nbox * mw::kVirialStride) ||
                       dev_alloc(g.d_wpart, (size_t)g.nbox * ((g.N + kForceBlockGlobal - 1) / kForceBlockGlobal) * mw::kVirialStride))) return 1;
    if (raise_lds_limit(&mw::k_model_forces<true, kForceBlockLds, kFullLayout>, kLdsBudget, kLazyForces)) return 1;
    if (t.start(0) || launch_model_energy(first, count, true, true, true)) return 1;
    if (!g.d_mom) return fail("mw_model_forces: no moment buffer");
    if (t.stop(0) || t.start(1)) return 1;
    const int box0 = first - 1;
    const size_t shmem = lds ? pos_lds_bytes(g.N, g.ivcap) : mw::lds_vec_bytes((size_t)g.ivcap);
    auto launch = [&](auto kernel, int block) {
        hipLaunchKernelGGL(kernel, dim3(nsplit, count), dim3(block), shmem, g.stream, g.d_pos, g.d_ivect, g.d_nivect,
                           g.d_list, g.d_order, g.d_nns, g.d_mom, g.d_force, g.d_wpart, g.N, g.S, g.ivcap, box0);
    };
    if (lds) launch(mw::k_model_forces<true, kForceBlockLds, kFullLayout>, kForceBlockLds);
    else     launch(mw::k_model_forces<false, kForceBlockGlobal, kFullLayout>, kForceBlockGlobal);
    HIPCHK(hipGetLastError());
    { int* d = g.disp[MW_DISPATCH_FORCES]; d[0] = g.ivcap; d[1] = count; d[2] = lds; d[3] = nsplit; d[4] = (int)shmem; }
    hipLaunchKernelGGL(mw::k_sum_virial, dim3(count), dim3(64), 0, g.stream, g.d_wpart, g.d_virial, box0, count, nsplit);
    HIPCHK(hipGetLastError());
    return t.stop(1);
}

int fetch_model_forces(int first, int count, double* e, double* f, double* w)
{
    const size_t b0 = (size_t)(first - 1);
    if (e) HIPCHK(hipMemcpyAsync(e, g.d_energy + b0, sizeof(double) * count, hipMemcpyDeviceToHost, g.stream));
    if (f) HIPCHK(hipMemcpyAsync(f, g.d_force + b0 * g.N * 3, sizeof(double) * 3 * g.N * count, hipMemcpyDeviceToHost, g.stream));
    if (w) HIPCHK(hipMemcpyAsync(w, g.d_virial + b0 * mw::kVirialStride, sizeof(double) * mw::kVirialStride * count, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

// The entry points of a family -- _launch, _batch and the one-box form -- are one function: `who` names the entry point in its
// messages, `form` says which of the three it is (kLaunch leaves the results on the device, the others fetch them).
int model_forces(const char* who, int first, int count, Form form, int timer_slot, double* e, double* f, double* w)
{
    MW_LOCK;
    if (check_live() || check_boxes(first, count, form)) return 1;
    if (form != kLaunch && (!e || !f || !w)) return fail("%s: null pointer", who);
    if (launch_model_forces(who, first, count, timer_slot)) return 1;
    return form != kLaunch ? fetch_model_forces(first, count, e, f, w) : 0;
}

// Ice structure classes of boxes first .. first+count-1 (mw_ice.hip.h) from the mirrored positions and the current lists:
// pass 1 (k_ice_q) with the geometry of the force pass -- one workgroup of 1024 per box with the box staged in LDS where it
// fits, else ceil(N / 256) workgroups of 256 -- then pass 2 (k_ice_class), ceil(N / 256) workgroups of 256 per box.
// timer_slot >= 0: event timers timer_slot (pass 1) and timer_slot + 1 (pass 2).
constexpr int kIceBlockLds = 1024, kIceBlockGlobal = 256, kIceBlockClass = 256;
int check_ice_rc(const char* who, double rc)
{
    return (rc > 0.0 && rc <= mw::kSigA) ? 0 : fail("%s: r_c = %g bohr outside (0, a sigma = %.6f]", who, rc, mw::kSigA);
}

int launch_ice_classes(const char* who, int first, int count, double rc, int timer_slot)
{
    Timers t;
    if (t.open(who, timer_slot, 2)) return 1;
    const bool lds = lds_fits(g.N, g.ivcap);
    const int nsplit = lds ? 1 : (g.N + kIceBlockGlobal - 1) / kIceBlockGlobal;
    const size_t nm = (size_t)g.nbox * g.N;
    if (!g.d_iceq && (dev_alloc(g.d_iceq, nm * mw::kIceQStride) || dev_alloc(g.d_icenb, nm) || dev_alloc(g.d_icen, nm) ||
                      dev_alloc(g.d_icecls, nm) || dev_alloc(g.d_icecnt, (size_t)g.nbox * mw::kIceClasses))) return 1;
    if (raise_lds_limit(&mw::k_ice_q<true, kIceBlockLds, kFullLayout>, kLdsBudget, kLazyIceQ)) return 1;
    if (t.start(0)) return 1;
    const int box0 = first - 1;
    const double rc2 = rc * rc;
    const size_t shmem = lds ? pos_lds_bytes(g.N, g.ivcap) : mw::lds_vec_bytes((size_t)g.ivcap);
    auto launch = [&](auto kernel, int block) {
        hipLaunchKernelGGL(kernel, dim3(nsplit, count), dim3(block), shmem, g.stream, g.d_pos, g.d_ivect, g.d_nivect,
                           g.d_list, g.d_order, g.d_nns, rc2, g.d_iceq, g.d_icenb, g.d_icen, g.d_icecnt, g.N, g.S, g.ivcap, box0);
    };
    if (lds) launch(mw::k_ice_q<true, kIceBlockLds, kFullLayout>, kIceBlockLds);
    else     launch(mw::k_ice_q<false, kIceBlockGlobal, kFullLayout>, kIceBlockGlobal);
    HIPCHK(hipGetLastError());
    { int* d = g.disp[MW_DISPATCH_ICE]; d[0] = g.ivcap; d[1] = count; d[2] = lds; d[3] = nsplit; d[4] = (int)shmem; }
    if (t.stop(0) || t.start(1)) return 1;
    hipLaunchKernelGGL((mw::k_ice_class<kIceBlockClass>), dim3((g.N + kIceBlockClass - 1) / kIceBlockClass, count), dim3(kIceBlockClass), 0,
                       g.stream, g.d_iceq, g.d_icenb, g.d_icen, g.d_icecls, g.d_icecnt, g.N, box0);
    HIPCHK(hipGetLastError());
    return t.stop(1);
}

int fetch_ice_classes(int first, int count, uint8_t* cls, int* counts)
{
    const size_t b0 = (size_t)(first - 1);
    if (cls) HIPCHK(hipMemcpyAsync(cls, g.d_icecls + b0 * g.N, (size_t)g.N * count, hipMemcpyDeviceToHost, g.stream));
    if (counts) HIPCHK(hipMemcpyAsync(counts, g.d_icecnt + b0 * mw::kIceClasses, sizeof(int) * mw::kIceClasses * count,
                                      hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int ice_classes(const char* who, int first, int count, Form form, double rc, int timer_slot, uint8_t* cls, int* counts)
{
    MW_LOCK;
    if (check_live() || check_boxes(first, count, form) || check_ice_rc(who, rc)) return 1;
    if (launch_ice_classes(who, first, count, rc, timer_slot)) return 1;
    return form != kLaunch ? fetch_ice_classes(first, count, cls, counts) : 0;
}

// Clusters of the molecules of the classes in `mask` (mw_ice_clusters.hip.h): the two classification passes above, then
// k_ice_clusters over their classes and neighbour entries, one workgroup per box.  Labels and sizes in LDS (8 B per molecule)
// where that fits 160 KiB less the kernel's static LDS, else in global memory; MW_ICE_CLUSTERS_LDS=0 forces the latter.
// timer_slot >= 0: event timers timer_slot and timer_slot + 1 (the classification passes) and timer_slot + 2 (the cluster pass).
constexpr int kClusterLdsBudget = 160 * 1024 - mw::kClusterStaticLds;
size_t cluster_lds_bytes(int N) { return ((size_t)N * 2 * sizeof(int) + 15) & ~(size_t)15; }
bool cluster_lds_fits(int N) { return cluster_lds_bytes(N) <= (size_t)kClusterLdsBudget; }
int cluster_threads(int N) { return std::min(mw::kClusterMaxBlock, std::max(64, (N + 63) & ~63)); }
int check_cluster_mask(const char* who, int mask)
{
    if (mask & 1) return fail("%s: mask %d selects class 0 (other): such molecules need not have four neighbours, their bonds are not kept", who, mask);
    if (mask <= 0 || (mask & ~mw::kClusterMaskAll)) return fail("%s: mask %d is not a non-empty subset of classes 1..5 (0x%x)", who, mask, mw::kClusterMaskAll);
    return 0;
}

int launch_ice_clusters(const char* who, int first, int count, double rc, int mask, int timer_slot)
{
    Timers t;
    if (t.open(who, timer_slot, 3)) return 1;
    const bool lds = g.clusters_lds && cluster_lds_fits(g.N);
    const size_t nm = (size_t)g.nbox * g.N;
    if (!g.d_icelabel && (dev_alloc(g.d_icelabel, nm) || dev_alloc(g.d_icesum, (size_t)g.nbox * 5))) return 1;
    if (!lds && !g.d_icesize && dev_alloc(g.d_icesize, nm)) return 1;
    if (lds && raise_lds_limit(&mw::k_ice_clusters<true>, kClusterLdsBudget, kLazyClusters)) return 1;
    if (launch_ice_classes(who, first, count, rc, timer_slot)) return 1;
    if (t.start(2)) return 1;
    const int threads = cluster_threads(g.N);
    int* rounds = g.d_icesum + 4 * (size_t)g.nbox;
    auto launch = [&](auto kernel, size_t shmem) {
        hipLaunchKernelGGL(kernel, dim3(1, count), dim3(threads), shmem, g.stream,
                           g.d_icecls, g.d_icenb, mask, g.d_icelabel, g.d_icesize, g.d_icesum, rounds, g.N, first - 1);
    };
    if (lds) launch(mw::k_ice_clusters<true>, cluster_lds_bytes(g.N));
    else     launch(mw::k_ice_clusters<false>, 0);
    HIPCHK(hipGetLastError());
    g.clast[0] = first; g.clast[1] = count; g.clast[2] = lds; g.clast[3] = threads;
    return t.stop(2);
}

int fetch_ice_clusters(int first, int count, int* label, int* summary)
{
    const size_t b0 = (size_t)(first - 1);
    if (label) HIPCHK(hipMemcpyAsync(label, g.d_icelabel + b0 * g.N, sizeof(int) * g.N * count, hipMemcpyDeviceToHost, g.stream));
    if (summary) HIPCHK(hipMemcpyAsync(summary, g.d_icesum + b0 * 4, sizeof(int) * 4 * count, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int ice_clusters(const char* who, int first, int count, Form form, double rc, int mask, int timer_slot, int* label, int* summary)
{
    MW_LOCK;
    if (check_live() || check_boxes(first, count, form) || check_ice_rc(who, rc) || check_cluster_mask(who, mask)) return 1;
    if (launch_ice_clusters(who, first, count, rc, mask, timer_slot)) return 1;
    return form != kLaunch ? fetch_ice_clusters(first, count, label, summary) : 0;
}

// Pair-distance histograms (mw_rdf.hip.h).  The cells are the DEVICE's (d_hmat: authoritative after volume moves), read back
// here for the one check that needs them: r_max (1 + 1e-9) <= 1.5 x the smallest perpendicular width of every box of the call,
// beyond which three images per axis no longer cover r_max.  Nothing is launched or written unless every box passes.
// Boxes of N <= kRdfSmallMax: one wavefront per box (k_rdf_small); larger: ceil(N / kRdfTile) workgroups per box (k_rdf_tiles).
int check_rdf_args(const char* who, double r_max, int nbins)
{
    if (!(r_max > 0.0) || !(r_max < 1e300)) return fail("%s: r_max = %g bohr outside (0, 1.5 x the smallest cell width]", who, r_max);
    if (nbins < 1 || nbins > mw::kRdfMaxBins) return fail("%s: nbins = %d outside 1..%d", who, nbins, mw::kRdfMaxBins);
    return 0;
}

int launch_rdf(const char* who, int first, int count, double r_max, int nbins, int timer_slot)
{
    Timers t;
    if (t.open(who, timer_slot, 1)) return 1;
    const int box0 = first - 1;
    std::vector<double> h((size_t)count * 9);
    HIPCHK(hipMemcpyAsync(h.data(), g.d_hmat + 9 * (size_t)box0, h.size() * sizeof(double), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    int images = 1;
    for (int b = 0; b < count; ++b) {
        double w[3];
        mw::rdf_cell_widths(&h[(size_t)b * 9], nullptr, w);
        int n = 1;
        for (int k = 0; k < 3; ++k) {
            const int m = mw::rdf_axis_images(r_max, w[k]);
            if (m < 0)
                return fail("%s: r_max = %.17g bohr outside (0, %.17g] = 1.5 x the smallest cell width of box %d (widths %g %g %g bohr)",
                            who, r_max, 1.5 * std::min(w[0], std::min(w[1], w[2])) / (1.0 + 1e-9), first + b, w[0], w[1], w[2]);
            n *= 2 * m + 1;
        }
        images = std::max(images, n);
    }
    if (dev_grow(g.d_rdf, g.rdf_bins, (size_t)nbins, (size_t)nbins, (size_t)g.nbox) || t.start()) return 1;
    unsigned long long* out = g.d_rdf + (size_t)box0 * nbins;
    const bool small = g.N <= mw::kRdfSmallMax;
    int per_box = 1;
    size_t lds = 0;
    if (small) {
        lds = (size_t)mw::kRdfSmallWaves * (3 * mw::kRdfSmallMax * sizeof(double) + (size_t)nbins * sizeof(unsigned));
        if (raise_lds_limit(&mw::k_rdf_small, mw::kRdfSmallWaves * (3 * mw::kRdfSmallMax * sizeof(double) + mw::kRdfMaxBins * sizeof(unsigned)),
                            kLazyRdfSmall)) return 1;
        hipLaunchKernelGGL(mw::k_rdf_small, dim3((count + mw::kRdfSmallWaves - 1) / mw::kRdfSmallWaves), dim3(64 * mw::kRdfSmallWaves),
                           lds, g.stream, g.d_pos, g.d_hmat, r_max, nbins, out, g.N, count, box0);
    } else {
        per_box = (g.N + mw::kRdfTile - 1) / mw::kRdfTile;
        if ((unsigned long long)per_box * (unsigned long long)count > 0x7fffffffull)
            return fail("%s: %d boxes x %d workgroups exceed one launch", who, count, per_box);
        HIPCHK(hipMemsetAsync(out, 0, (size_t)count * nbins * sizeof(unsigned long long), g.stream));
        const size_t dyn = (size_t)nbins * sizeof(unsigned);
        lds = dyn + 3 * mw::kRdfTile * sizeof(double);
        hipLaunchKernelGGL(mw::k_rdf_tiles, dim3((unsigned)per_box * (unsigned)count), dim3(mw::kRdfTile), dyn, g.stream,
                           g.d_pos, g.d_hmat, r_max, nbins, out, g.N, per_box, box0);
    }
    HIPCHK(hipGetLastError());
    { int* d = g.disp[MW_DISPATCH_RDF]; d[0] = g.ivcap; d[1] = count; d[2] = small; d[3] = per_box; d[4] = (int)lds; d[5] = images; }
    return t.stop();
}

int fetch_rdf(int first, int count, int nbins, long long* hist)
{
    HIPCHK(hipMemcpyAsync(hist, g.d_rdf + (size_t)(first - 1) * nbins, (size_t)count * nbins * sizeof(long long),
                          hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int rdf(const char* who, int first, int count, Form form, double r_max, int nbins, int timer_slot, long long* hist)
{
    MW_LOCK;
    if (check_live() || check_boxes(first, count, form) || check_rdf_args(who, r_max, nbins)) return 1;
    if (form != kLaunch && !hist) return fail("%s: null pointer", who);
    if (launch_rdf(who, first, count, r_max, nbins, timer_slot)) return 1;
    return form != kLaunch ? fetch_rdf(first, count, nbins, hist) : 0;
}

}  // namespace

extern "C" {

int mw_model_forces_launch(int first_ils, int count, int timer_slot)
{
    return model_forces("mw_model_forces_launch", first_ils, count, kLaunch, timer_slot, nullptr, nullptr, nullptr);
}

int mw_model_forces_batch(int first_ils, int count, double* e, double* f, double* w)
{
    return model_forces("mw_model_forces_batch", first_ils, count, kBatch, -1, e, f, w);
}

int mw_model_forces(int ils, double* e, double* f, double* w) { return model_forces("mw_model_forces", ils, 1, kSingle, -1, e, f, w); }

int mw_ice_classes_launch(int first_ils, int count, double rc, int timer_slot)
{
    return ice_classes("mw_ice_classes_launch", first_ils, count, kLaunch, rc, timer_slot, nullptr, nullptr);
}

int mw_ice_classes_batch(int first_ils, int count, double rc, uint8_t* cls, int* counts)
{
    return ice_classes("mw_ice_classes_batch", first_ils, count, kBatch, rc, -1, cls, counts);
}

int mw_ice_classes(int ils, double rc, uint8_t* cls, int counts[6]) { return ice_classes("mw_ice_classes", ils, 1, kSingle, rc, -1, cls, counts); }

int mw_ice_bonds(int ils, double rc, double* c)
{
    MW_LOCK;
    if (check_live() || check_box(ils) || check_ice_rc("mw_ice_bonds", rc)) return 1;
    if (!c) return fail("mw_ice_bonds: null pointer");
    if (launch_ice_classes("mw_ice_bonds", ils, 1, rc, -1)) return 1;
    const size_t n = (size_t)g.N * g.S;
    if (!g.d_icebond && dev_alloc(g.d_icebond, n)) return 1;
    hipLaunchKernelGGL(mw::k_ice_bonds, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g.stream, g.d_pos, g.d_ivect, g.d_listm,
                       g.d_nn, g.d_iceq, rc * rc, g.d_icebond, g.N, g.S, g.ivcap, ils - 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c, g.d_icebond, n * sizeof(double), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_ice_clusters_launch(int first_ils, int count, double rc, int mask, int timer_slot)
{
    return ice_clusters("mw_ice_clusters_launch", first_ils, count, kLaunch, rc, mask, timer_slot, nullptr, nullptr);
}

int mw_ice_clusters_batch(int first_ils, int count, double rc, int mask, int* label, int* summary)
{
    return ice_clusters("mw_ice_clusters_batch", first_ils, count, kBatch, rc, mask, -1, label, summary);
}

int mw_ice_clusters(int ils, double rc, int mask, int* label, int summary[4])
{
    return ice_clusters("mw_ice_clusters", ils, 1, kSingle, rc, mask, -1, label, summary);
}

int mw_ice_clusters_plan(int nwater, int out[4])
{
    if (nwater < 1 || nwater > (1 << mw::kJBits)) return fail("mw_ice_clusters_plan: nwater = %d outside 1..%d", nwater, 1 << mw::kJBits);
    if (!out) return fail("mw_ice_clusters_plan: null pointer");
    const bool lds = cluster_lds_fits(nwater);
    out[0] = lds;
    out[1] = cluster_threads(nwater);
    out[2] = lds ? (int)cluster_lds_bytes(nwater) : 0;
    out[3] = kClusterLdsBudget / (int)(2 * sizeof(int));
    return 0;
}

int mw_ice_clusters_last(int out[4])
{
    MW_LOCK;
    if (check_live()) return 1;
    if (!out) return fail("mw_ice_clusters_last: null pointer");
    out[0] = g.clast[1]; out[1] = g.clast[2]; out[2] = g.clast[3]; out[3] = 0;
    if (g.clast[1] == 0) return 0;
    std::vector<int> r((size_t)g.clast[1]);
    HIPCHK(hipMemcpyAsync(r.data(), g.d_icesum + 4 * (size_t)g.nbox + (g.clast[0] - 1), sizeof(int) * r.size(), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    for (int v : r) out[3] = std::max(out[3], v);
    return 0;
}

int mw_rdf_launch(int first_ils, int count, double r_max, int nbins, int timer_slot)
{
    return rdf("mw_rdf_launch", first_ils, count, kLaunch, r_max, nbins, timer_slot, nullptr);
}

int mw_rdf_batch(int first_ils, int count, double r_max, int nbins, long long* hist)
{
    return rdf("mw_rdf_batch", first_ils, count, kBatch, r_max, nbins, -1, hist);
}

int mw_rdf(int ils, double r_max, int nbins, long long* hist) { return rdf("mw_rdf", ils, 1, kSingle, r_max, nbins, -1, hist); }

}  // extern "C"
