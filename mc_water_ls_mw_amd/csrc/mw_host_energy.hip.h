// mw_host_energy.hip.h -- the full-box energy: launch geometry, the launch, the mw_model_energy* entry points.
#pragma once

namespace {

// Launch geometry of the full-box kernel for `count` boxes.
struct Geo { bool lds; int block, nsplit, chunk; size_t shmem; };
Geo model_geo(int count)
{
    Geo ge;
    ge.lds = lds_fits(g.N, g.ivcap);
    if (ge.lds) {
        // one workgroup stages the whole box; split a box over several workgroups only
        // when there are too few boxes to occupy the 256 CUs
        ge.block = 1024;
        int want = (2 * g.cu + count - 1) / count;
        int maxsplit = (g.N + ge.block - 1) / ge.block;
        ge.nsplit = want < 1 ? 1 : (want > maxsplit ? maxsplit : want);
        ge.shmem = model_lds_bytes(g.N, g.ivcap);
    } else {
        ge.block = 256;
        ge.nsplit = (g.N + ge.block - 1) / ge.block;
        ge.shmem = kQueue256 + mw::lds_vec_bytes((size_t)g.ivcap);
    }
    if (ge.nsplit > g.nsplit_max) ge.nsplit = g.nsplit_max;
    ge.chunk = (((g.N + ge.nsplit - 1) / ge.nsplit) + 63) & ~63;   // whole groups of 64 list columns (cmax is per group)
    return ge;
}

// mom_global: boxes too large for LDS write their moments too (a build of the global-memory kernel of its own, for the force pass;
// every other caller takes the moment path only where boxes are staged in LDS)
int launch_model_energy(int first, int count, bool with_mom = false, bool write_energy = true, bool mom_global = false)
{
    const Geo ge = model_geo(count);
    double* mom = nullptr;
    if (with_mom && (ge.lds || mom_global)) {
        if (!g.d_mom && dev_alloc(g.d_mom, (size_t)g.nbox * g.N * mw::kMomStride)) return 1;
        mom = g.d_mom;
    }
    const int wen = write_energy ? 1 : 0;
    // whole boxes staged in LDS, one workgroup per box: the workgroups are persistent, one per compute unit (its LDS holds
    // one), each taking every g.cu-th box and reading its next box while the current one's tail drains.  The boxes go out in a fixed
    // ASCENDING order (workgroup y: boxes y, y + g.cu, ...), and mw_moves_upload serves the step's trial moves in DESCENDING box
    // order: the two are meant to be opposite, so that each launch starts on what the one before it touched last.
    dim3 grid(ge.nsplit, g.model_persist && ge.lds && ge.nsplit == 1 ? std::min(count, g.cu) : count);
    const int box0 = first - 1;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(ge.block), ge.shmem, g.stream, g.d_pos, g.d_ivect, g.d_nivect, g.d_list, g.d_order, g.d_nns,
                           g.d_cmax, g.d_partial, g.d_cpartial, g.d_energy, g.d_counts, g.N, g.S, g.ivcap, box0, ge.nsplit, ge.chunk, count, mom, wen);
    };
    if (ge.lds && mom) launch(mw::k_model_energy<true, 1024, kFullLayout, false, true>);
    else if (ge.lds)   launch(mw::k_model_energy<true, 1024, kFullLayout>);
    else if (mom)      launch(mw::k_model_energy<false, 256, kFullLayout, true, true>);
    else               launch(mw::k_model_energy<false, 256, kFullLayout, true>);
    HIPCHK(hipGetLastError());
    {
        int* d = g.disp[MW_DISPATCH_ENERGY];
        d[0] = g.ivcap; d[1] = count; d[2] = ge.lds; d[3] = ge.nsplit; d[4] = ge.chunk; d[5] = (int)grid.y; d[6] = mom != nullptr;
        d[7] = (int)ge.shmem; d[8] = ge.block;
    }
    if (mom) { g.mom_first = first; g.mom_count = count; drop_driver_moments(false); }   // (d_mom rewritten for these boxes: the driver's claim on it ends -- its launch renews it)
    if (ge.nsplit > 1 && write_energy) {           // split boxes: the partials of box b live at [b*nsplit .. b*nsplit+nsplit); unsplit boxes wrote their energy themselves
        hipLaunchKernelGGL(mw::k_sum_partials, dim3(count), dim3(64), 0, g.stream, g.d_partial, g.d_cpartial,
                           g.d_energy, g.d_counts, box0, count, ge.nsplit);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

int mw_model_energy_counts_total(int first_ils, int count, long long* npairs, long long* ntriplets)
{
    MW_LOCK;
    if (check_live() || check_range(first_ils, count)) return 1;
    std::vector<unsigned long long> c((size_t)count * 2);
    HIPCHK(hipMemcpyAsync(c.data(), g.d_counts + 2 * (size_t)(first_ils - 1), c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    long long p = 0, t = 0;
    for (int b = 0; b < count; ++b) { p += (long long)c[2 * (size_t)b]; t += (long long)c[2 * (size_t)b + 1]; }
    if (npairs) *npairs = p;
    if (ntriplets) *ntriplets = t;
    return 0;
}

int mw_model_energy_launch(int first_ils, int count)
{
    MW_LOCK;
    if (check_live() || check_range(first_ils, count)) return 1;
    return launch_model_energy(first_ils, count);
}

int mw_model_energy_fetch(int first_ils, int count, double* e_out)
{
    MW_LOCK;
    if (check_live() || check_range(first_ils, count)) return 1;
    HIPCHK(hipMemcpyAsync(e_out, g.d_energy + (first_ils - 1), sizeof(double) * count, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_model_energy_batch(int first_ils, int count, double* e_out)
{
    MW_LOCK;
    if (mw_model_energy_launch(first_ils, count)) return 1;
    return mw_model_energy_fetch(first_ils, count, e_out);
}

int mw_model_energy(int ils, double* e) { return mw_model_energy_batch(ils, 1, e); }

// compute_model_energy(ils) as the host calls it (molint.F90:407-499; after every volume move, mc_moves.F90:1340): mirror the
// lattice's positions and evaluate, ONE call -- the positions travel through pinned memory, the energy comes back into pinned
// memory, one synchronisation at the end.
int mw_model_energy_of(int ils, const double* xyz, double* e)
{
    MW_LOCK;
    if (check_live() || check_box(ils)) return 1;
    if (!xyz || !e) return fail("mw_model_energy_of: null pointer");
    drop_driver_moments();
    const size_t bytes = (size_t)g.N * 3 * sizeof(double);
    std::memcpy(g.h_stage, xyz, bytes);
    HIPCHK(hipMemcpyAsync(g.d_pos + (size_t)(ils - 1) * g.N * 3, g.h_stage, bytes, hipMemcpyHostToDevice, g.stream));
    if (launch_model_energy(ils, 1)) return 1;
    HIPCHK(hipMemcpyAsync(g.h_pin + 16, g.d_energy + (ils - 1), sizeof(double), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    *e = g.h_pin[16];
    return 0;
}

int mw_model_energy_counts(int ils, long long* npairs, long long* ntriplets)
{
    MW_LOCK;
    if (check_live() || check_box(ils)) return 1;
    unsigned long long c[2];
    HIPCHK(hipMemcpyAsync(c, g.d_counts + 2 * (size_t)(ils - 1), sizeof c, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    if (npairs) *npairs = (long long)c[0];
    if (ntriplets) *ntriplets = (long long)c[1];
    return 0;
}

int mw_set_model_energy(int ils, double e)
{
    MW_LOCK;
    if (check_live() || check_box(ils)) return 1;
    HIPCHK(hipMemcpyAsync(g.d_energy + (ils - 1), &e, sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

}  // extern "C"
