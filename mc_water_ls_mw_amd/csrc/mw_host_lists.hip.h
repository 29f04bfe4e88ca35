// mw_host_lists.hip.h -- neighbour lists: the launches of the builders and the entry points that build and read lists.
#pragma once

namespace {

int launch_build(int first, int count)
{
    const int box0 = first - 1;
    ++g.list_version;
    for (int b = box0; b < box0 + count; ++b) g.h_listbuilt[(size_t)b] = 1;
    drop_driver_moments();               // (the driver's moments of walkers in global memory are made afresh after every list build: what
                                         //  the accepted moves' updates add in rounding stays bounded by a list interval, as the walkers in LDS
                                         //  have it per launch)
    int ngrid = 0;
    for (int b = box0; b < box0 + count; ++b) ngrid += g.h_usegrid[b] ? 1 : 0;
    const bool fused_sort = ngrid > 0 && g.sort_in_lds && !g.legacy_search;       // k_cell_sort_box resets the statistics itself
    if (!fused_sort) {
        hipLaunchKernelGGL(mw::k_init_stats, dim3((count + 255) / 256), dim3(256), 0, g.stream, g.d_stats, box0, count);   // {min, max} per box
        HIPCHK(hipGetLastError());
    }
    dim3 grid((g.N + 255) / 256, count);
    if (ngrid > 0) {
        if (fused_sort) {
            // boxes whose cell-ordered records fit LDS: bin + scan + scatter in one workgroup per box
            hipLaunchKernelGGL(mw::k_cell_sort_box, dim3(count), dim3(1024), sort_lds_bytes(g.N), g.stream, g.d_pos, g.d_grid,
                               g.d_cstart, g.d_wpos, g.d_wsh, g.d_stats, g.N, g.cstride, box0);
            HIPCHK(hipGetLastError());
        } else {
        HIPCHK(hipMemsetAsync(g.d_ccount + (size_t)box0 * g.cstride, 0, sizeof(int) * (size_t)count * g.cstride, g.stream));
        hipLaunchKernelGGL(mw::k_cell_bin, grid, dim3(256), 0, g.stream, g.d_pos, g.d_grid, g.d_cellid, g.d_shift, g.d_wrel, g.d_ccount,
                           g.N, g.cstride, box0);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(mw::k_cell_scan, dim3(count), dim3(1024), 0, g.stream, g.d_grid, g.d_ccount, g.d_cstart, g.d_ccursor,
                           g.cstride, box0);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(mw::k_cell_scatter, grid, dim3(256), 0, g.stream, g.d_grid, g.d_cellid, g.d_shift, g.d_wrel, g.d_ccursor,
                           g.d_sorted, g.d_wpos, g.d_wsh, g.N, g.cstride, box0);
        HIPCHK(hipGetLastError());
        }
        if (g.legacy_search) {
            hipLaunchKernelGGL(mw::k_cell_search, grid, dim3(256), (size_t)g.S * 256 * sizeof(uint32_t), g.stream, g.d_pos, g.d_ivect,
                               g.d_grid, g.d_cellid, g.d_shift, g.d_cstart, g.d_sorted, g.d_listm, g.d_nn, g.d_cin, g.d_stats,
                               g.N, g.S, g.ivcap, g.cstride, box0);
        } else {
            // one wavefront per block of grid cells along the third axis, four per workgroup; cells per block: enough
            // for ~17 molecules per wavefront -- one block of kPairIB rows, and the block's candidates still fit one
            // register batch (measured on 512 x 4096 ice: 3 cells 1.35 ms, 4 cells 1.18 ms, 5 cells 1.19 ms;
            // MW_PAIR_BCELLS overrides)
            int bcells = 1, maxblocks = 0;
            for (int b = box0; b < box0 + count; ++b)
                if (g.h_usegrid[b]) { bcells = std::max(bcells, (int)(17.5 * g.h_grid[(size_t)b].ncell / g.N + 0.5)); }
            if (const char* ev = std::getenv("MW_PAIR_BCELLS")) bcells = std::atoi(ev);
            bcells = std::max(1, std::min(bcells, mw::kPairMaxB));
            for (int b = box0; b < box0 + count; ++b) {
                if (!g.h_usegrid[b]) continue;
                const mw::GridDesc& G = g.h_grid[(size_t)b];
                const int B = std::min(bcells, G.nc[2]);
                maxblocks = std::max(maxblocks, G.nc[0] * G.nc[1] * ((G.nc[2] + B - 1) / B));
            }
            const int nwg = (maxblocks + 3) / 4, count8 = (count + 7) & ~7;       // a 1-D grid: the kernel maps workgroup -> (box, cell blocks) by XCD
            hipLaunchKernelGGL(mw::k_cell_pairs, dim3((unsigned)nwg * (unsigned)count8), dim3(256), 0, g.stream, g.d_pos, g.d_ivect, g.d_grid,
                               g.d_cstart, g.d_wpos, g.d_wsh, g.d_listm, g.d_nn, g.d_cin, g.d_stats, g.N, g.S, g.ivcap, g.cstride, box0, bcells,
                               nwg, count);
        }
        HIPCHK(hipGetLastError());
    }
    if (ngrid < count) {
        const int bt = std::min(256, (g.N + 63) & ~63);                           // a block no larger than the box needs
        hipLaunchKernelGGL(mw::k_build_neighbours, dim3((g.N + bt - 1) / bt, count), dim3(bt), 0, g.stream, g.d_pos, g.d_ivect, g.d_nivect,
                           g.d_listm, g.d_nn, g.d_cin, g.d_stats, g.d_usegrid, g.N, g.S, g.ivcap, box0);
        HIPCHK(hipGetLastError());
    }
    // the slot-major layout of the full-box kernel, columns sorted by work (mw_neighbours.hip.h, k_list_order)
    {
        const int nseg = (g.N + g.order_seg - 1) / g.order_seg;
        const size_t shmem = order_lds_bytes(g.N, g.order_seg, g.order_kbits);
        const int nthreads = std::min(1024, std::max(64, (std::min(g.N, g.order_seg) + 63) & ~63));
        hipLaunchKernelGGL(mw::k_list_order, dim3(nseg, count), dim3(nthreads), shmem, g.stream, g.d_listm, g.d_nn, g.d_cin, g.d_stats,
                           g.d_list, g.d_order, g.d_nns, g.d_cmax, g.N, g.S, box0, g.order_kbits, g.order_seg);
        HIPCHK(hipGetLastError());
        int* d = g.disp[MW_DISPATCH_BUILD];
        d[0] = g.ivcap; d[1] = count; d[2] = ngrid; d[3] = count - ngrid; d[4] = fused_sort; d[5] = ngrid > 0 && g.legacy_search;
        d[6] = g.order_seg; d[7] = nseg; d[8] = (int)shmem;
    }
    return 0;
}

int finish_build(int first, int count, int* min_nn, int* max_nn)
{
    std::vector<int> st((size_t)count * 2);
    HIPCHK(hipMemcpyAsync(st.data(), g.d_stats + 2 * (first - 1), sizeof(int) * 2 * count, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    int mn = 0x7fffffff, mx = 0, worst = -1;
    for (int b = 0; b < count; ++b) {
        if (st[2 * b] < mn) mn = st[2 * b];
        if (st[2 * b + 1] > mx) { mx = st[2 * b + 1]; worst = first + b; }
    }
    if (min_nn) *min_nn = mn;
    if (max_nn) *max_nn = mx;
    if (first == 1 && count == g.nbox) { g.nnmax_cached = mx; g.nnmax_version = g.list_version; }   // (the driver's launch asks for the longest row
                                                                                                   //  of any box: no second read-back of the same words)
    if (mx > g.S)
        return fail("mw: neighbour list overflow in box %d: a molecule has %d entries, maxneigh = %d", worst, mx, g.S);
    return 0;
}

}  // namespace

extern "C" {

int mw_build_neighbours_launch(int first_ils, int count)
{
    MW_LOCK;
    if (check_live() || check_range(first_ils, count)) return 1;
    for (int b = first_ils; b < first_ils + count; ++b)
        if (g.h_nivect[b - 1] < 1) return fail("mw_build_neighbours: box %d has no cell yet (call mw_set_cell / compute_ivects)", b);
    return launch_build(first_ils, count);
}

int mw_build_neighbours_batch(int first_ils, int count, int* min_nn, int* max_nn)
{
    MW_LOCK;
    if (mw_build_neighbours_launch(first_ils, count)) return 1;
    return finish_build(first_ils, count, min_nn, max_nn);
}

int mw_build_neighbours(int ils, int* min_nn, int* max_nn) { return mw_build_neighbours_batch(ils, 1, min_nn, max_nn); }

int mw_get_neighbours(int ils, int* nn, int* jn, int* vn)
{
    MW_LOCK;
    if (check_live() || check_box(ils)) return 1;
    const size_t N = (size_t)g.N, S = (size_t)g.S, R = (size_t)mw::kRow;
    std::vector<int> hnn(N);
    std::vector<uint32_t> hl(N * R);
    HIPCHK(hipMemcpyAsync(hnn.data(), g.d_nn + (size_t)(ils - 1) * N, N * sizeof(int), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(hl.data(), g.d_listm + (size_t)(ils - 1) * N * R, N * R * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    for (size_t i = 0; i < N; ++i) {
        if (nn) nn[i] = hnn[i];
        for (size_t s = 0; s < S; ++s) {
            const bool used = (int)s < hnn[i];
            const uint32_t e = used ? hl[i * R + s] : 0u;           // molecule-major rows
            if (jn) jn[i * S + s] = used ? (int)(e & mw::kJMask) + 1 : 0;   // reference layout jn(slot, imol)
            if (vn) vn[i * S + s] = used ? (int)(e >> mw::kJBits) + 1 : 0;
        }
    }
    return 0;
}

int mw_neighbour_total(int first_ils, int count, long long* total_entries)
{
    MW_LOCK;
    if (check_live() || check_range(first_ils, count)) return 1;
    std::vector<int> hnn((size_t)count * g.N);
    HIPCHK(hipMemcpyAsync(hnn.data(), g.d_nn + (size_t)(first_ils - 1) * g.N, hnn.size() * sizeof(int), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    long long t = 0;
    for (int v : hnn) t += v;
    *total_entries = t;
    return 0;
}

}  // extern "C"
