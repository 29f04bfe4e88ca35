// mw_host_init.hip.h -- the life cycle of the context: mw_init, mw_finalize and what gives everything back.
#pragma once

namespace {

// Free everything the context holds (any subset may be allocated: mw_init's failure path comes here too).
void release_all()
{
    if (g.srv_running) (void)server_stop();
    if (g.stream) { (void)hipSetDevice(g.device); (void)hipStreamSynchronize(g.stream); }
    if (g.sstream) { (void)hipStreamSynchronize(g.sstream); (void)hipStreamDestroy(g.sstream); }
    if (g.h_head) (void)hipHostFree(g.h_head);
    if (g.h_slots) (void)hipHostFree(g.h_slots);
    if (g.req_dev_alloc) { (void)hipFree(g.req_dev_alloc); g.req_dev_alloc = nullptr; }
    dev_free_all();
    if (g.ev_srv) { (void)hipEventDestroy(g.ev_srv); g.ev_srv = nullptr; }
    if (g.h_pin) (void)hipHostFree(g.h_pin);
    if (g.h_stage) (void)hipHostFree(g.h_stage);
    for (int s = 0; s < kTimerSlots; ++s) {
        if (g.ev[s][0]) (void)hipEventDestroy(g.ev[s][0]);
        if (g.ev[s][1]) (void)hipEventDestroy(g.ev[s][1]);
    }
    if (g.stream) (void)hipStreamDestroy(g.stream);
    g = Ctx();
}

}  // namespace

extern "C" {

static int init_impl(int device, int nwater, int nboxes, int maxneigh);

int mw_init(int device, int nwater, int nboxes, int maxneigh)
{
    MW_LOCK;
    if (g.live) return fail("mw_init: already initialised (call mw_finalize first)");
    const int rc = init_impl(device, nwater, nboxes, maxneigh);
    if (rc != 0) {                       // a failed allocation half way: give back what was taken, keep the message
        const std::string msg = g_err;
        release_all();
        g_err = msg;
    }
    return rc;
}

static int init_impl(int device, int nwater, int nboxes, int maxneigh)
{
    if (nwater < 1 || nboxes < 1) return fail("mw_init: nwater = %d, nboxes = %d must be positive", nwater, nboxes);
    if (nwater > (1 << mw::kJBits)) return fail("mw_init: nwater = %d exceeds the %d-bit packed index", nwater, mw::kJBits);
    if (maxneigh < 1 || maxneigh > MW_MAXNEIGH_LIMIT)
        return fail("mw_init: maxneigh = %d outside 1..%d", maxneigh, MW_MAXNEIGH_LIMIT);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail("mw_init: no HIP device available (%s); this engine has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0) {
        // one process per GPU: take the local rank from the launcher's environment
        device = 0;
        const char* vars[] = {"MW_DEVICE", "LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", "MV2_COMM_WORLD_LOCAL_RANK",
                              "MPI_LOCALRANKID", "SLURM_LOCALID"};
        for (const char* v : vars) {
            const char* s = std::getenv(v);
            if (s && *s) { device = std::atoi(s) % ndev; if (device < 0) device = 0; break; }
        }
    }
    if (device >= ndev) return fail("mw_init: device %d outside 0..%d", device, ndev - 1);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("mw_init: device %d is %s; libmw_hip.so carries gfx950 code only", device, prop.gcnArchName);

    g = Ctx();
    g.device = device; g.N = nwater; g.nbox = nboxes; g.S = maxneigh; g.ivcap = 32;
    g.cu = prop.multiProcessorCount;
    g.nsplit_max = (nwater + 255) / 256;
    HIPCHK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    const size_t nb = (size_t)nboxes, N = (size_t)nwater;
    // (+ one staging ticket: k_model_energy reads whole tickets of the next box, the last of which may run past its end)
    if (dev_alloc_zeroed(g.d_pos, nb * N * 3 + mw::kStageTicket) || dev_alloc_zeroed(g.d_ivect, nb * g.ivcap * 3) ||
        dev_alloc_zeroed(g.d_nivect, nb) || dev_alloc_zeroed(g.d_hmat, nb * 9) || dev_alloc_zeroed(g.d_volume, nb) ||
        dev_alloc_zeroed(g.d_list, nb * N * (size_t)maxneigh) || dev_alloc_zeroed(g.d_listm, nb * N * (size_t)mw::kRow) ||
        dev_alloc_zeroed(g.d_nn, nb * N) || dev_alloc(g.d_stats, nb * 2)) return 1;
    {
        const size_t ngroups = (N + 63) / 64;
        if (dev_alloc(g.d_order, nb * N) || dev_alloc_zeroed(g.d_nns, nb * N) || dev_alloc_zeroed(g.d_cmax, nb * ngroups) ||
            dev_alloc_zeroed(g.d_cin, nb * N)) return 1;
        // identity order until the first list build (an energy call before any build sees empty rows anyway)
        std::vector<int> ident(nb * N);
        for (size_t b = 0; b < nb; ++b) for (size_t i = 0; i < N; ++i) ident[b * N + i] = (int)i;
        HIPCHK(hipMemcpy(g.d_order, ident.data(), ident.size() * sizeof(int), hipMemcpyHostToDevice));
        // Segments of k_list_order: the whole box when the full-box kernel stages its positions in LDS; when it gathers
        // them through the caches a wavefront keeps its 64 consecutive molecules (neighbours in index are neighbours in
        // space: measured on 64 x 32768 molecules, sorting over 256 / 1024 / 32768 molecules costs 16 / 80 / 95 % in
        // cache misses, more than the balance gains).  MW_ORDER_SEG overrides (a multiple of 64).
        // Sort key bits: the (key, group) table must fit kOrderSlots.
        const char* sg = std::getenv("MW_ORDER_SEG");
        order_plan(nwater, sg ? std::atoi(sg) : 0, g.order_seg, g.order_kbits);
    }
    g.cstride = cell_stride(nwater);
    if (dev_alloc_zeroed(g.d_grid, nb) || dev_alloc_zeroed(g.d_usegrid, nb) || dev_alloc(g.d_cellid, nb * N) ||
        dev_alloc(g.d_shift, nb * N) || dev_alloc(g.d_sorted, nb * N) || dev_alloc(g.d_wrel, nb * N) ||
        dev_alloc(g.d_wpos, nb * N) || dev_alloc(g.d_wsh, nb * N)) return 1;
    { const char* cs = std::getenv("MW_CELL_SEARCH"); g.legacy_search = cs && std::strcmp(cs, "legacy") == 0; }
    {
        const char* cs = std::getenv("MW_CELL_SORT");
        g.sort_in_lds = sort_fits(nwater) && !(cs && std::strcmp(cs, "global") == 0);
        if (g.sort_in_lds && raise_lds_limit(&mw::k_cell_sort_box, sort_lds_bytes(nwater))) return 1;
    }
    if (dev_alloc(g.d_ccount, nb * (size_t)g.cstride) || dev_alloc(g.d_cstart, nb * ((size_t)g.cstride + 1)) ||
        dev_alloc(g.d_ccursor, nb * (size_t)g.cstride)) return 1;
    g.h_grid.assign(nb, mw::GridDesc());
    for (auto& G : g.h_grid) std::memset(&G, 0, sizeof G);
    g.h_usegrid.assign(nb, 0);
    g.h_listbuilt.assign(nb, 0);
    { const char* fb = std::getenv("MW_FORCE_BRUTE_NEIGHBOURS"); g.force_brute = fb && *fb && *fb != '0'; }
    { const char* mm = std::getenv("MW_MOVE_MOMENTS"); g.move_moments = mm ? (mm[0] != '0' ? 1 : 0) : -1; }
    { const char* mc = std::getenv("MW_MOVE_COUNTS"); g.move_counts_eager = mc && std::strcmp(mc, "eager") == 0; }
    g.mcnt_state = Ctx::kCountsThere; g.mcnt_passes = 0;
    { const char* mp = std::getenv("MW_MODEL_PERSIST"); g.model_persist = !(mp && mp[0] == '0'); }
    { const char* cl = std::getenv("MW_ICE_CLUSTERS_LDS"); g.clusters_lds = !(cl && cl[0] == '0'); }
    if (dev_alloc(g.d_partial, nb * g.nsplit_max) || dev_alloc(g.d_cpartial, nb * g.nsplit_max * 2) ||
        dev_alloc_zeroed(g.d_energy, nb) || dev_alloc_zeroed(g.d_counts, nb * 2)) return 1;
    HIPCHK(hipHostMalloc(&g.h_pin, 4096, hipHostMallocMapped));
    std::memset(g.h_pin, 0, 4096);
    HIPCHK(hipHostGetDevicePointer((void**)&g.d_pin, g.h_pin, 0));
    g.stage_bytes = std::max((size_t)nwater * 3 * sizeof(double), sizeof(mw::CellRecord) + (size_t)MW_MAX_IVECT * 3 * sizeof(double));
    HIPCHK(hipHostMalloc((void**)&g.h_stage, g.stage_bytes, hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer((void**)&g.d_stage, g.h_stage, 0));
    {   // mail slots of the resident local-energy server: one per lattice, at most 8
        g.nslots = std::min(nboxes, 8);
        if (dev_alloc_zeroed(g.d_srvcounts, nb * 4)) return 1;
        HIPCHK(hipStreamCreateWithFlags(&g.sstream, hipStreamNonBlocking));
        HIPCHK(hipHostMalloc((void**)&g.h_head, sizeof(mw::MailHead), hipHostMallocMapped));
        HIPCHK(hipHostMalloc((void**)&g.h_slots, sizeof(mw::MailSlot) * 8, hipHostMallocMapped));
        std::memset(g.h_head, 0, sizeof(mw::MailHead));
        std::memset(g.h_slots, 0, sizeof(mw::MailSlot) * 8);
        HIPCHK(hipHostGetDevicePointer((void**)&g.d_head, g.h_head, 0));
        HIPCHK(hipHostGetDevicePointer((void**)&g.d_slots, g.h_slots, 0));
        const char* ev = std::getenv("MW_LOCAL_SERVER");
        g.srv_enabled = !(ev && *ev == '0');
        g_srv_enabled.store(g.srv_enabled, std::memory_order_release);
        g.req_slots = g.h_slots; g.d_req = g.d_slots;
        const char* rq = std::getenv("MW_SERVER_REQ");
        if (!(rq && std::strcmp(rq, "host") == 0)) {
            // Request lines in fine-grained DEVICE memory, written by the host through the PCIe BAR: the server polls
            // local memory (0.45 us a poll instead of a 1.3 us PCIe read, and an idle server puts no traffic on the
            // bus) and a request reaches it as one posted write.  Only where the host can address device memory (large
            // BAR): probed with a system call that reports EFAULT instead of faulting; otherwise, or with
            // MW_SERVER_REQ=host, the request lines stay in host-mapped memory next to the reply line (which the host
            // polls, so it stays there either way).
            void* p = nullptr;
            if (hipExtMallocWithFlags(&p, sizeof(mw::MailSlot) * 8, hipDeviceMallocFinegrained) == hipSuccess && p) {
                bool ok = hipMemset(p, 0, sizeof(mw::MailSlot) * 8) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
                int fds[2];
                if (ok && pipe(fds) == 0) {
                    ok = write(fds[1], p, 8) == 8;
                    close(fds[0]); close(fds[1]);
                } else ok = false;
                if (ok) { g.req_dev_alloc = p; g.req_slots = static_cast<mw::MailSlot*>(p); g.d_req = g.req_slots; }
                else { (void)hipGetLastError(); (void)hipFree(p); }
            } else (void)hipGetLastError();
            if (!g.req_dev_alloc && rq && std::strcmp(rq, "device") == 0)
                std::fprintf(stderr, "mw: MW_SERVER_REQ=device: device memory is not host-addressable here, requests stay in host memory\n");
        }
    }
    g.h_ivect.assign(nb * g.ivcap * 3, 0.0);
    g.h_nivect.assign(nb, 0);
    // the kernels that may ask for more than the default 64 KiB of dynamic LDS (the analysis kernels: when they first run)
    const size_t sweep_lds = 160 * 1024 - 8 * 1024;   // the driver's image vectors of small or sheared cells, staged positions and rows
    if (raise_lds_limit(&mw::k_model_energy<true, 1024, kFullLayout, false, true>, kLdsBudget) ||
        raise_lds_limit(&mw::k_model_energy<true, 1024, kFullLayout>, kLdsBudget) ||
        raise_lds_limit(&mw::k_list_order, mw::kOrderSlots * sizeof(int)) ||
        raise_lds_limit(&mw::k_cell_search, MW_MAXNEIGH_LIMIT * 256 * sizeof(uint32_t)) ||
        raise_lds_limit(&mw::k_move_energy<true>, kLdsBudget) ||
        raise_lds_limit(&mw::k_move_energy<true, mw::kLayoutSoA, false>, kLdsBudget) ||
        raise_lds_limit(&mw::k_move_energy<true, mw::kLayoutSoA, false, true>, kLdsBudget)) return 1;
    for (int v = 0; v < 12; ++v)
        if (raise_lds_limit(sweep_kernel(1 + (v & 1), (v >> 1) % 3, v >= 6, 1), sweep_lds)) return 1;
    for (int v = 0; v < 24; ++v)
        if (raise_lds_limit(sweep_kernel(1 + (v & 1), v >> 3, (v & 2) != 0, (v & 4) ? 4 : 2), sweep_lds)) return 1;
    for (int v = 0; v < 2; ++v)
        if (raise_lds_limit(sweep_kernel(1, 0, v != 0, 8), sweep_lds) || raise_lds_limit(sweep_kernel(2, 2, v != 0, 6), sweep_lds)) return 1;
    g.live = true;
    return 0;
}

int mw_finalize(void)
{
    MW_LOCK;
    if (!g.live) return 0;
    release_all();
    return 0;
}

}  // extern "C"
