// mw_host_moves.hip.h -- staged trial moves: upload, the launch of the move kernels, a Monte Carlo step, the batch wrappers.
#pragma once

namespace {

int ensure_moves(int n)
{
    if (n <= g.mcap) return 0;
    size_t cap = 1024;
    while (cap < (size_t)n) cap *= 2;
    g.mcap = 0;                          // (the arrays are replaced together: no capacity until all of them stand)
    if (dev_alloc(g.d_mimol, cap) || dev_alloc(g.d_mtrial, 3 * cap) || dev_alloc(g.d_meold, cap) || dev_alloc(g.d_menew, cap) ||
        dev_alloc(g.d_mcnt, 4 * cap) || dev_alloc(g.d_mperm, cap) || dev_alloc(g.d_mdecl, 2 * cap + 2)) return 1;
    HIPCHK(hipMemset(g.d_mdecl, 0, 2 * sizeof(int)));
    g.mdecl_par = 0;
    g.mcap = (int)cap;
    return 0;
}

// One launch of a build of k_move_energy over the uploaded work items (the step's launch and the pass that counts on demand).
template <typename Kernel>
void launch_move_kernel(Kernel kernel, size_t shmem, int kmode, const double* mom, unsigned int* tot)
{
    hipLaunchKernelGGL(kernel, dim3(g.mwork_n), dim3(1024), shmem, g.stream,
                       g.d_pos, g.d_ivect, g.d_nivect, g.d_listm, g.d_nn, g.d_mwork, g.d_mimol, g.d_mtrial, g.d_mperm,
                       g.d_meold, g.d_menew, g.d_mcnt, g.d_mdecl, g.N, g.ivcap, kmode, mom, tot);
}

}  // namespace

extern "C" {

int mw_moves_upload(int n, const int* ils, const int* imol, const double* trial_xyz)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (n < 0) return fail("mw_moves_upload: n = %d", n);
    drop_move_counts();                  // (the requests a pending count pass would read are replaced)
    g.mn = 0;
    if (n == 0) return 0;
    if (!ils || !imol) return fail("mw_moves_upload: null request arrays");
    // Bucket the requests by box (stable counting sort): a workgroup then serves requests of ONE
    // box and can stage that box's positions in LDS.  perm maps sorted slot -> caller's index.
    std::vector<int> cnt((size_t)g.nbox + 1, 0);
    for (int m = 0; m < n; ++m) {
        if (ils[m] < 1 || ils[m] > g.nbox) return fail("mw_moves_upload: request %d has box %d outside 1..%d", m, ils[m], g.nbox);
        if (imol[m] < 1 || imol[m] > g.N) return fail("mw_moves_upload: request %d has molecule %d outside 1..%d", m, imol[m], g.N);
        ++cnt[(size_t)ils[m]];
    }
    std::vector<int> start((size_t)g.nbox + 1, 0);
    int used_boxes = 0;
    g.m_noself = true;
    g.m_boxlo = g.nbox; g.m_boxhi = -1; g.m_minreq = n;
    for (int b = 0; b < g.nbox; ++b) {
        start[(size_t)b + 1] = start[b] + cnt[(size_t)b + 1];
        if (cnt[(size_t)b + 1]) {
            ++used_boxes; if (!g.h_usegrid[(size_t)b]) g.m_noself = false;
            g.m_boxlo = std::min(g.m_boxlo, b); g.m_boxhi = std::max(g.m_boxhi, b); g.m_minreq = std::min(g.m_minreq, cnt[(size_t)b + 1]);
        }
    }
    std::vector<int> perm((size_t)n), i0((size_t)n), fill(start.begin(), start.end() - 1);
    std::vector<double> tr(trial_xyz ? (size_t)3 * n : 0);
    for (int m = 0; m < n; ++m) {
        const int s = fill[(size_t)ils[m] - 1]++;
        perm[s] = m; i0[s] = imol[m] - 1;
        if (trial_xyz) { tr[3 * (size_t)s] = trial_xyz[3 * (size_t)m]; tr[3 * (size_t)s + 1] = trial_xyz[3 * (size_t)m + 1]; tr[3 * (size_t)s + 2] = trial_xyz[3 * (size_t)m + 2]; }
    }
    // LDS staging pays when a box's 24N bytes are shared by enough requests
    g.mlds = lds_fits_move(g.N, g.ivcap) && ((long long)n * 2048 >= (long long)used_boxes * 24 * g.N);
    // Requests per work item.  Inside an item the wavefronts draw requests dynamically, so large items waste little
    // at their end and stage the box once for more work; but there must be enough items to fill the chip:
    // aim at >= 2 items per CU, between 256 and the LDS capacity kMoveChunk (measured on 512 x 2048 requests with the sorted,
    // XCD-ordered moment path, profiles/r12_summary.md: items of 512 / 1024 / 2048 requests give a step of 0.504 / 0.492 / 0.488 ms,
    // medians of five alternating runs -- a smaller item sorts into shorter groups and ends on a shorter tail, and still loses to
    // staging the box once more; MW_MOVE_CHUNK overrides).
    int chunk = 16;
    if (g.mlds) {
        const long long want = (long long)n / (2LL * std::max(1, g.cu));
        chunk = 256;
        while (chunk < mw::kMoveChunk && chunk < want) chunk *= 2;
        if (const char* ev = std::getenv("MW_MOVE_CHUNK")) { const int v = std::atoi(ev); if (v >= 64 && v <= mw::kMoveChunk) chunk = v; }
    }
    g.mchunk = chunk;
    { const char* ms = std::getenv("MW_MOVE_SORT"); g.move_sort = !(ms && ms[0] == '0'); }   // (the moment path: mode bit 5 of k_move_energy)
    { const char* mk = std::getenv("MW_MOVE_MASKS"); g.move_masks = !(mk && mk[0] == '0'); }   // (and its bit 6)
    { const char* mg = std::getenv("MW_MOVE_GATE"); g.move_gate = !(mg && mg[0] == '0'); }     // (and its bit 7)
    { const char* mp = std::getenv("MW_MOVE_PAIRS32"); g.move_pairs32 = !(mp && mp[0] == '0'); }   // (and its bit 8)
    // NEWEST BOXES FIRST: the work list holds the boxes in DESCENDING order.  The step's full-box pass, persistent, hands its boxes
    // out in ascending order (launch_model_energy), so what it touched last -- the highest boxes' positions and the moment records it
    // wrote for them -- is what the memory-side cache still holds when the move kernel starts: served first, those first-touch reads
    // are hits where the ascending order found box 0 evicted by the ~0.5 GB of traffic since.  The next step's full-box pass in turn
    // starts on the low boxes the move kernel served last.  No result depends on the order (a request's bits are its own).
    // MW_MOVE_BOX_ORDER=asc restores the ascending order for A/B runs.
    bool desc = true;
    if (const char* bo = std::getenv("MW_MOVE_BOX_ORDER")) desc = !(bo[0] == 'a' || bo[0] == 'A');
    std::vector<int4> work;
    std::vector<int> rank_of((size_t)g.nbox, 0);                 // rank among the boxes that have requests, counted from box 0 in EITHER order
    { int r = 0; for (int b = 0; b < g.nbox; ++b) if (start[(size_t)b + 1] > start[b]) rank_of[(size_t)b] = r++; }
    for (int bb = 0; bb < g.nbox; ++bb) {
        const int b = desc ? g.nbox - 1 - bb : bb;
        const int s0 = start[b], cntb = start[(size_t)b + 1] - s0;
        if (cntb == 0) continue;
        const int nitems = (cntb + chunk - 1) / chunk;           // equal shares: no short item at the end of a box
        for (int k = 0; k < nitems; ++k) {
            int4 w; w.x = b; w.y = s0 + (int)((long long)cntb * k / nitems); w.z = s0 + (int)((long long)cntb * (k + 1) / nitems); w.w = 0;
            work.push_back(w);
        }
    }
    const int first_box = work.empty() ? -1 : work[0].x;         // (before the XCD dealing, which starts every XCD's sequence at once)
    // XCD-aware order.  Workgroups are dealt to the 8 XCDs round-robin (workgroup w runs on XCD w % 8) and every XCD
    // has its own L2, so the work items of one box -- which all stage the same positions and walk the same list
    // rows -- are placed on ONE XCD, one after the other: slot k*8 + x holds the k-th item of the boxes with
    // (box index) % 8 == x.  (When the eight sequences differ in length the tail is dealt out as it comes.)  A box's XCD is its
    // ascending rank % 8 whichever way the list runs -- the XCD whose persistent full-box workgroup wrote its moments when all
    // boxes have requests -- and each XCD's sequence follows the list's order: descending by default.
    if (getenv("MW_NO_XCD_ORDER") == nullptr && work.size() >= 16) {
        constexpr int kXcd = 8;
        std::vector<std::vector<int4>> seq(kXcd);
        for (const int4& w : work) seq[(size_t)(rank_of[(size_t)w.x] % kXcd)].push_back(w);
        std::vector<int4> ordered;
        ordered.reserve(work.size());
        std::vector<size_t> at(kXcd, 0);
        while (ordered.size() < work.size())
            for (int x = 0; x < kXcd; ++x)
                if (at[x] < seq[x].size()) ordered.push_back(seq[x][at[x]++]);
        work.swap(ordered);
    }
    if (ensure_moves(n)) return 1;
    if (dev_grow(g.d_mwork, g.mwork_cap, work.size(), 2 * work.size())) return 1;
    HIPCHK(hipMemcpyAsync(g.d_mwork, work.data(), sizeof(int4) * work.size(), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(g.d_mperm, perm.data(), sizeof(int) * n, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(g.d_mimol, i0.data(), sizeof(int) * n, hipMemcpyHostToDevice, g.stream));
    if (trial_xyz) HIPCHK(hipMemcpyAsync(g.d_mtrial, tr.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    g.mwork_n = (int)work.size();
    g.mwork_first = first_box;
    g.mn = n;
    return 0;
}

static int launch_moves(int mode)
{
    if (g.mn == 0) return 0;
    g.mcnt_state = Ctx::kCountsDropped;          // (until the kernels are issued: a launch that fails on the way leaves no counts to ask for)
    if (dev_grow(g.d_mtot, g.mtot_cap, (size_t)g.mwork_n, 2 * (size_t)g.mwork_n, 4)) return 1;
    g.mtot_n = 0;
    const size_t iv_bytes = kMoveScratch + mw::lds_vec_bytes((size_t)g.ivcap);
    const int kmode = mode | (g.mdecl_par << 2);                           // this launch's count word of the declined list (zeroed by the
    g.mdecl_par ^= 1;                                                     // previous launch's k_move_fallback, or at allocation)
    // The moment path (mw_move_moments.hip.h): boxes staged in LDS, no self-images, and enough requests per box to pay for the
    // full-box pass that makes the moments (one pass costs what ~300 requests save; MW_MOVE_MOMENTS=0 | 1 overrides the count rule).
    // The moments must be those of the positions as they are NOW: they are taken from the last full-box launch only when nothing
    // that can move a molecule has run since (mw_step_launch: the full-box pass of the same step), else made here.
    const bool mom_ok = g.mlds && g.m_noself && model_geo(1).lds && g.m_boxhi >= g.m_boxlo;
    const bool fresh = g.d_mom && g.mom_count > 0 && g.mom_first - 1 <= g.m_boxlo && g.m_boxhi < g.mom_first - 1 + g.mom_count;
    // (a request saves ~0.3 ns of the launch; a box's moments cost 0.13 us as a by-product of the step's full-box pass, 0.32 us as a
    //  pass of their own: 512 / 1280 requests per box)
    const bool use_mom = mom_ok && (g.move_moments >= 0 ? g.move_moments != 0 : g.m_minreq >= (fresh ? 512 : 1280));
    const size_t shmem = g.mlds ? move_lds_bytes(g.N, g.ivcap, g.mchunk) : iv_bytes;
    auto launch = [&](auto kernel, const double* mom, unsigned int* tot, int bits = 0) { launch_move_kernel(kernel, shmem, kmode | bits, mom, tot); };
    if (use_mom) {
        if (!fresh && launch_model_energy(g.m_boxlo + 1, g.m_boxhi - g.m_boxlo + 1, true, false)) return 1;
        // the counts of the requests this kernel serves: made on demand (mw_moves_counts), by a pass of the same kernel with mode bits
        // 3 "count" and 4 "no energy output"; MW_MOVE_COUNTS=eager: by this launch, as before
        launch(mw::k_move_energy<true, mw::kLayoutSoA, false, true>, g.d_mom, g.d_mtot, (g.move_counts_eager ? 8 : 0) | (g.move_sort ? 32 : 0) | (g.move_masks ? 64 : 0) | (g.move_gate ? 128 : 0) | (g.move_pairs32 ? 256 : 0));
        if (g.move_counts_eager) g.mtot_n = g.mwork_n;
    } else if (g.mlds && g.m_noself) launch(mw::k_move_energy<true, mw::kLayoutSoA, false>, nullptr, nullptr);
    else if (g.mlds)                 launch(mw::k_move_energy<true>, nullptr, nullptr);
    else                             launch(mw::k_move_energy<false>, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    g.mcnt_state = use_mom && !g.move_counts_eager ? Ctx::kCountsPending : Ctx::kCountsThere;
    {
        int* d = g.disp[MW_DISPATCH_MOVES];
        d[0] = g.ivcap; d[1] = g.mn; d[2] = g.mlds; d[3] = g.m_noself; d[4] = use_mom; d[5] = use_mom && fresh; d[6] = g.mchunk;
        d[7] = g.mwork_n; d[8] = (int)shmem; d[9] = use_mom ? 3 : (g.mlds ? (g.m_noself ? 2 : 1) : 0);
        d[10] = g.mcnt_state; d[11] = g.mcnt_passes; d[12] = -1; d[13] = g.mwork_first;
    }
    // the requests the fused routine declined (a few hundred per million on thermal ice): batched routine, two wavefronts each (one per position)
    hipLaunchKernelGGL(mw::k_move_fallback, dim3(std::min(1024, (g.mn + 3) / 4)), dim3(256), 0, g.stream, g.d_pos, g.d_ivect, g.d_listm, g.d_nn,
                       g.d_mimol, g.d_mtrial, g.d_mperm, g.d_meold, g.d_menew, g.d_mcnt, g.d_mdecl, g.N, g.ivcap, kmode);
    HIPCHK(hipGetLastError());
    g.mmode = mode;
    return 0;
}

int mw_moves_launch(void)
{
    MW_LOCK;
    if (check_live()) return 1;
    return launch_moves(3);
}

int mw_step_launch(int first_ils, int count, int timer_slot)
{
    MW_LOCK;
    if (check_live() || check_range(first_ils, count)) return 1;
    Timers t;
    if (t.open("mw_step_launch", timer_slot, 2) || t.start(0)) return 1;
    // (the step's full-box pass leaves every molecule's moments behind when the step's move kernel will take the moment path)
    const bool want_mom = g.mn > 0 && g.mlds && g.m_noself && (g.move_moments >= 0 ? g.move_moments != 0 : g.m_minreq >= 512);
    if (launch_model_energy(first_ils, count, want_mom, true)) return 1;
    if (t.stop(0) || t.start(1) || launch_moves(3)) return 1;
    return t.stop(1);
}

int mw_moves_fetch(double* e_old, double* e_new)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (g.mn > 0) {
        if (e_old) HIPCHK(hipMemcpyAsync(e_old, g.d_meold, sizeof(double) * g.mn, hipMemcpyDeviceToHost, g.stream));
        if (e_new) HIPCHK(hipMemcpyAsync(e_new, g.d_menew, sizeof(double) * g.mn, hipMemcpyDeviceToHost, g.stream));
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_moves_counts(long long out[4])
{
    MW_LOCK;
    if (check_live()) return 1;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (g.mn == 0) return 0;
    if (g.mcnt_state == Ctx::kCountsDropped)
        return fail("mw_moves_counts: the counts of the last launch were not made, and the launch failed or the requests, positions, cells "
                    "or lists it saw have changed since: ask right after a launch (or run with MW_MOVE_COUNTS=eager)");
    if (g.mcnt_state == Ctx::kCountsPending) {
        // the launch's moment-path kernel once more, on the same work items, moments and positions: it counts what it serves (d_mtot,
        // zeros in d_mcnt), writes no energy and appends nothing to the declined list -- whose requests k_move_fallback counted at the launch
        launch_move_kernel(mw::k_move_energy<true, mw::kLayoutSoA, false, true>, move_lds_bytes(g.N, g.ivcap, g.mchunk), g.mmode | 8 | 16 | (g.move_sort ? 32 : 0) | (g.move_masks ? 64 : 0) | (g.move_gate ? 128 : 0) | (g.move_pairs32 ? 256 : 0), g.d_mom, g.d_mtot);
        HIPCHK(hipGetLastError());
        g.mtot_n = g.mwork_n;
        g.mcnt_state = Ctx::kCountsThere;
        g.disp[MW_DISPATCH_MOVES][10] = g.mcnt_state; g.disp[MW_DISPATCH_MOVES][11] = ++g.mcnt_passes;
    }
    std::vector<unsigned int> c((size_t)g.mn * 4);
    unsigned long long tot[4] = {0, 0, 0, 0};
    std::vector<unsigned int> it((size_t)g.mtot_n * 4);
    HIPCHK(hipMemcpyAsync(c.data(), g.d_mcnt, sizeof(unsigned int) * 4 * g.mn, hipMemcpyDeviceToHost, g.stream));
    if (g.mtot_n) HIPCHK(hipMemcpyAsync(it.data(), g.d_mtot, sizeof(unsigned int) * 4 * g.mtot_n, hipMemcpyDeviceToHost, g.stream));
    int ndecl = 0;                       // (the last launch's count word of the declined list: zeroed by the NEXT launch's k_move_fallback)
    HIPCHK(hipMemcpyAsync(&ndecl, g.d_mdecl + (g.mdecl_par ^ 1), sizeof(int), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    g.disp[MW_DISPATCH_MOVES][12] = ndecl;
    for (int k = 0; k < g.mtot_n; ++k) for (int q = 0; q < 4; ++q) tot[q] += it[4 * (size_t)k + q];
    for (int m = 0; m < g.mn; ++m) {
        if (g.mmode & 1) { out[0] += c[4 * (size_t)m]; out[1] += c[4 * (size_t)m + 1]; }
        if (g.mmode & 2) { out[2] += c[4 * (size_t)m + 2]; out[3] += c[4 * (size_t)m + 3]; }
    }
    if (g.mmode & 1) { out[0] += (long long)tot[0]; out[1] += (long long)tot[1]; }      // (the moment path's requests: summed on the device)
    if (g.mmode & 2) { out[2] += (long long)tot[2]; out[3] += (long long)tot[3]; }
    return 0;
}

int mw_local_energy_batch(int n, const int* ils, const int* imol, const double* trial_xyz, double* e_out)
{
    MW_LOCK;
    if (mw_moves_upload(n, ils, imol, trial_xyz)) return 1;
    if (launch_moves(trial_xyz ? 2 : 1)) return 1;
    return trial_xyz ? mw_moves_fetch(nullptr, e_out) : mw_moves_fetch(e_out, nullptr);
}

int mw_delta_energy_batch(int n, const int* ils, const int* imol, const double* trial_xyz, double* e_old, double* e_new)
{
    MW_LOCK;
    if (!trial_xyz) return fail("mw_delta_energy_batch: trial positions are required");
    if (mw_moves_upload(n, ils, imol, trial_xyz)) return 1;
    if (launch_moves(3)) return 1;
    return mw_moves_fetch(e_old, e_new);
}

}  // extern "C"
