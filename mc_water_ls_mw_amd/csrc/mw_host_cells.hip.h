// mw_host_cells.hip.h -- cells, positions and image vectors: the host mirrors of the reference's hmatrix / ljr / ivect and
// the entry points that set, upload and read them.
#pragma once

namespace {

// Image vectors exactly as compute_ivects builds them (molint.F90:174-217):
// central cell first, then icell, jcell, kcell loops (kcell fastest), (sx+sy)+sz.
int host_ivects(const double h[9], std::vector<double>& out, int imv[3])
{
    const double* h1 = h; const double* h2 = h + 3; const double* h3 = h + 6;
    const double rc = mw::kSmallA * mw::kSigma;
    const int im = (int)std::floor(rc / std::sqrt(h1[0] * h1[0] + h1[1] * h1[1] + h1[2] * h1[2])) + 1;   // :189
    const int jm = (int)std::floor(rc / std::sqrt(h2[0] * h2[0] + h2[1] * h2[1] + h2[2] * h2[2])) + 1;
    const int km = (int)std::floor(rc / std::sqrt(h3[0] * h3[0] + h3[1] * h3[1] + h3[2] * h3[2])) + 1;
    const long long n = (long long)(2 * im + 1) * (2 * jm + 1) * (2 * km + 1);                            // :193
    imv[0] = im; imv[1] = jm; imv[2] = km;
    if (n > MW_MAX_IVECT) return -1;
    out.assign((size_t)n * 3, 0.0);                                                                       // :197
    size_t k = 1;
    for (int ic = -im; ic <= im; ++ic) {
        const double sx[3] = {(double)ic * h1[0], (double)ic * h1[1], (double)ic * h1[2]};               // :201
        for (int jc = -jm; jc <= jm; ++jc) {
            const double sy[3] = {(double)jc * h2[0], (double)jc * h2[1], (double)jc * h2[2]};           // :203
            for (int kc = -km; kc <= km; ++kc) {
                if (ic == 0 && jc == 0 && kc == 0) continue;                                             // :207
                const double sz[3] = {(double)kc * h3[0], (double)kc * h3[1], (double)kc * h3[2]};       // :205
                for (int d = 0; d < 3; ++d) {
                    volatile double s = sx[d] + sy[d];   // keep (sx+sy)+sz unfused and in this order     :208
                    out[3 * k + d] = s + sz[d];
                }
                ++k;
            }
        }
    }
    return (int)n;
}

// Grid for the cell-list neighbour builder: spacing >= list radius along every cell vector.
// nc = 0 means "fewer than 3 cells somewhere": that box keeps the brute-force kernel.
mw::GridDesc make_grid(const double h[9], const int imv[3], int max_cells)
{
    mw::GridDesc G;
    std::memset(&G, 0, sizeof G);
    const double* a = h; const double* b = h + 3; const double* c = h + 6;     // cell vectors
    const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
    const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
    const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double det = a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2];
    G.im[0] = imv[0]; G.im[1] = imv[1]; G.im[2] = imv[2];
    if (!(std::fabs(det) > 0.0)) return G;
    // r = s1 a + s2 b + s3 c  =>  s1 = (b x c).r / det, ...
    for (int d = 0; d < 3; ++d) { G.hinv[d] = bc[d] / det; G.hinv[3 + d] = ca[d] / det; G.hinv[6 + d] = ab[d] / det; }
    const double rn = mw::kRn * (1.0 + 1.0e-9);
    const double* cr[3] = {bc, ca, ab};
    int nc[3];
    for (int d = 0; d < 3; ++d) {
        const double width = std::fabs(det) / std::sqrt(cr[d][0] * cr[d][0] + cr[d][1] * cr[d][1] + cr[d][2] * cr[d][2]);
        const double q = std::floor(width / rn);
        nc[d] = q > 1024.0 ? 1024 : (int)q;
        if (nc[d] < 3) return G;                          // nc stays 0: brute force for this box
        if (imv[d] > 500) return G;
    }
    while ((long long)nc[0] * nc[1] * nc[2] > max_cells) {   // coarser cells are still valid cells
        int big = 0;
        if (nc[1] > nc[big]) big = 1;
        if (nc[2] > nc[big]) big = 2;
        if (nc[big] <= 3) return G;
        --nc[big];
    }
    G.nc[0] = nc[0]; G.nc[1] = nc[1]; G.nc[2] = nc[2];
    G.ncell = nc[0] * nc[1] * nc[2];
    for (int d = 0; d < 9; ++d) G.h[d] = h[d];
    // Error bound of k_cell_pairs' single-precision squared distance.  Coordinates there are relative to a grid
    // cell's origin: |.| <= 2 D for a candidate, D for the molecule itself, D = the grid cell's longest diagonal.
    // Each coordinate difference carries at most 8 ulp(D) of rounding (conversions, the piece offset, the
    // subtraction), the squared sum 2 sqrt(3) r delta + 4 ulp(r^2) at r ~ rn.  Doubled for safety; a pair whose
    // single-precision r^2 lies within eps of rn^2 is re-decided in double precision by the reference's expression.
    double D = 0.0;
    for (int sg = 0; sg < 4; ++sg) {
        const double s1 = (sg & 1) ? -1.0 : 1.0, s2 = (sg & 2) ? -1.0 : 1.0;
        double v[3];
        for (int d = 0; d < 3; ++d) v[d] = a[d] / nc[0] + s1 * b[d] / nc[1] + s2 * c[d] / nc[2];
        D = std::max(D, std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
    }
    const double ulp = 5.9604644775390625e-08, r = mw::kRn + 1.0;      // 2^-24
    G.eps = (float)(2.0 * (2.0 * std::sqrt(3.0) * r * 8.0 * ulp * D + 4.0 * ulp * r * r));
    return G;
}

int grow_ivcap(int need)
{
    int cap = std::max(g.ivcap, (need + 3) & ~3);       // (as much as asked for: the Monte Carlo driver keeps every box's table in LDS,
    if (cap > MW_MAX_IVECT) cap = MW_MAX_IVECT;         //  where a doubled capacity cost the 48-molecule walkers their eighth place per CU)
    std::vector<double> nh((size_t)g.nbox * cap * 3, 0.0);
    for (int b = 0; b < g.nbox; ++b)
        std::memcpy(&nh[(size_t)b * cap * 3], &g.h_ivect[(size_t)b * g.ivcap * 3], sizeof(double) * 3 * g.ivcap);
    if (dev_alloc(g.d_ivect, nh.size())) return 1;      // (waits for the stream before the old table goes)
    HIPCHK(hipMemcpy(g.d_ivect, nh.data(), nh.size() * sizeof(double), hipMemcpyHostToDevice));
    g.h_ivect.swap(nh);
    g.ivcap = cap;
    return 0;
}

// Cells of `count` consecutive boxes in one go: image vectors (compute_ivects, molint.F90:174-217), volume, grid
// descriptors on the host, then ONE copy per device array for the whole range (a farm of thousands of walkers sets up
// in a handful of transfers instead of seven per box).
int set_cells_impl(int first_ils, int count, const double* h, int* nivect_out)
{
    std::vector<std::vector<double>> ivs((size_t)count);
    std::vector<int> ns((size_t)count), imvs((size_t)count * 3);
    int need = 0;
    for (int k = 0; k < count; ++k) {
        int imv[3] = {1, 1, 1};
        const int n = host_ivects(h + 9 * (size_t)k, ivs[k], imv);
        if (n < 0) return fail("mw_set_cell: cell of box %d is so small that it needs more than %d image vectors", first_ils + k, MW_MAX_IVECT);
        ns[k] = n; imvs[3 * k] = imv[0]; imvs[3 * k + 1] = imv[1]; imvs[3 * k + 2] = imv[2];
        need = std::max(need, n);
    }
    if (need > g.ivcap && grow_ivcap(need)) return 1;
    std::vector<double> vol((size_t)count);
    const size_t b0 = (size_t)(first_ils - 1);
    for (int k = 0; k < count; ++k) {
        const size_t off = (b0 + k) * g.ivcap * 3;
        std::memcpy(&g.h_ivect[off], ivs[k].data(), ivs[k].size() * sizeof(double));
        g.h_nivect[b0 + k] = ns[k];
        // volume(ils) = |det hmatrix(:,:,ils)| as util_determinant expands it (util.f90:16-41; molint.F90:125)
        const double* m = h + 9 * (size_t)k;   // m[(c-1)*3 + (r-1)] = hmatrix(r,c)
        double det = m[0] * (m[4] * m[8] - m[7] * m[5]);
        det = det - m[3] * (m[1] * m[8] - m[7] * m[2]);
        det = det + m[6] * (m[1] * m[5] - m[4] * m[2]);
        vol[k] = std::fabs(det);
        g.h_grid[b0 + k] = make_grid(m, &imvs[3 * k], g.cstride);
        g.h_usegrid[b0 + k] = (!g.force_brute && g.h_grid[b0 + k].nc[0] > 0) ? 1 : 0;
        if (!g.h_usegrid[b0 + k]) g.h_grid[b0 + k].nc[0] = 0;
        else g.grid_on_device = true;
        if (nivect_out) nivect_out[k] = ns[k];
    }
    if (count == 1) {
        // One box (the host's volume move calls compute_ivects four times per attempt, mc_moves.F90:1285-1358,1510-1512): the
        // record goes into pinned memory the device reads in place, and one small kernel files it -- a launch and a
        // synchronisation instead of six transfers.
        mw::CellRecord* rec = reinterpret_cast<mw::CellRecord*>(g.h_stage);
        rec->niv = ns[0]; rec->usegrid = g.h_usegrid[b0]; rec->vol = vol[0];
        std::memcpy(rec->h, h, 9 * sizeof(double));
        rec->grid = g.h_grid[b0];
        std::memcpy(g.h_stage + sizeof(mw::CellRecord), ivs[0].data(), ivs[0].size() * sizeof(double));
        hipLaunchKernelGGL(mw::k_set_cell, dim3(1), dim3(256), 0, g.stream, reinterpret_cast<const mw::CellRecord*>(g.d_stage),
                           reinterpret_cast<const double*>(g.d_stage + sizeof(mw::CellRecord)), g.d_ivect + b0 * g.ivcap * 3, g.d_nivect + b0,
                           g.d_hmat + 9 * b0, g.d_volume + b0, g.d_grid + b0, g.d_usegrid + b0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(g.stream));
        return 0;
    }
    HIPCHK(hipMemcpyAsync(g.d_ivect + b0 * g.ivcap * 3, &g.h_ivect[b0 * g.ivcap * 3], (size_t)count * g.ivcap * 3 * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(g.d_nivect + b0, &g.h_nivect[b0], (size_t)count * sizeof(int), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(g.d_hmat + 9 * b0, h, (size_t)count * 9 * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(g.d_volume + b0, vol.data(), (size_t)count * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(g.d_grid + b0, &g.h_grid[b0], (size_t)count * sizeof(mw::GridDesc), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(g.d_usegrid + b0, &g.h_usegrid[b0], (size_t)count * sizeof(int), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));      // `h` and `vol` are the caller's / this frame's
    return 0;
}

// mw_set_cell and mw_set_cells_range
int set_cells(const char* who, int first, int count, Form form, const double* h, int* nivect_out)
{
    MW_LOCK;
    if (check_live() || check_boxes(first, count, form)) return 1;
    if (!h) return fail("%s: null pointer", who);
    drop_driver_moments();
    return set_cells_impl(first, count, h, nivect_out);
}

// mw_upload_positions, mw_download_positions and their range forms: `xyz` to the mirror, or the mirror to `xyz`
enum Copy { kUpload, kDownload };
int copy_positions(const char* who, int first, int count, Form form, Copy dir, double* xyz)
{
    MW_LOCK;
    if (check_live() || check_boxes(first, count, form)) return 1;
    if (!xyz) return fail("%s: null pointer", who);
    double* mirror = g.d_pos + (size_t)(first - 1) * g.N * 3;
    const size_t bytes = (size_t)g.N * 3 * count * sizeof(double);
    if (dir == kUpload) {
        drop_driver_moments();
        HIPCHK(hipMemcpyAsync(mirror, xyz, bytes, hipMemcpyHostToDevice, g.stream));
    } else {
        HIPCHK(hipMemcpyAsync(xyz, mirror, bytes, hipMemcpyDeviceToHost, g.stream));
    }
    HIPCHK(hipStreamSynchronize(g.stream));   // the caller may overwrite its positions right after we return
    return 0;
}

}  // namespace

extern "C" {

int mw_set_cell(int ils, const double h[9], int* nivect_out) { return set_cells("mw_set_cell", ils, 1, kSingle, h, nivect_out); }

int mw_set_cells_range(int first_ils, int count, const double* h, int* nivect_out)
{
    return set_cells("mw_set_cells_range", first_ils, count, kBatch, h, nivect_out);
}

int mw_get_ivects(int ils, double* out, int max_vectors, int* nivect_out)
{
    MW_LOCK;
    if (check_live() || check_box(ils)) return 1;
    const int n = g.h_nivect[ils - 1];
    if (nivect_out) *nivect_out = n;
    if (out) {
        if (max_vectors < n) return fail("mw_get_ivects: buffer holds %d vectors, box %d has %d", max_vectors, ils, n);
        std::memcpy(out, &g.h_ivect[(size_t)(ils - 1) * g.ivcap * 3], sizeof(double) * 3 * n);
    }
    return 0;
}

int mw_upload_positions(int ils, const double* xyz) { return copy_positions("mw_upload_positions", ils, 1, kSingle, kUpload, const_cast<double*>(xyz)); }

int mw_download_positions(int ils, double* xyz) { return copy_positions("mw_download_positions", ils, 1, kSingle, kDownload, xyz); }

int mw_upload_positions_range(int first_ils, int count, const double* xyz)
{
    return copy_positions("mw_upload_positions_range", first_ils, count, kBatch, kUpload, const_cast<double*>(xyz));
}

int mw_download_positions_range(int first_ils, int count, double* xyz)
{
    return copy_positions("mw_download_positions_range", first_ils, count, kBatch, kDownload, xyz);
}

int mw_patch_position(int ils, int imol, const double r[3])
{
    MW_LOCK;
    if (check_live() || check_box(ils) || check_mol(imol)) return 1;
    drop_driver_moments();
    HIPCHK(hipMemcpyAsync(g.d_pos + ((size_t)(ils - 1) * g.N + (imol - 1)) * 3, r, 3 * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

}  // extern "C"
