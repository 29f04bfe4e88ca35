// mw_host_server.hip.h -- the resident server of the single local-energy call and the mw_local_energy* entry points.
#pragma once

extern "C" {

// Launch the resident server if it is not running (g_srv_mu held by the caller).
static int server_start_locked()
{
    if (g.srv_running) return 0;
    int prev = -1;
    const bool sw = hipGetDevice(&prev) == hipSuccess && prev != g.device && hipSetDevice(g.device) == hipSuccess;
    g.h_head->quit = 0; g.h_head->exited = 0;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    // a few tenths of a second of empty polls (one poll is a PCIe round trip, ~1 us) and the server leaves by itself
    static const bool stamps = std::getenv("MW_SERVER_STAMPS") != nullptr;
    static const bool plain = std::getenv("MW_SERVER_PLAIN_LOADS") != nullptr;      // experiment only: L1-cached position loads
    // The server's moment path (k_local_server): every molecule's moments of every box, from the full-box kernel, and the positions
    // they belong to -- made HERE, each time the server starts (every entry point that may move a molecule stops it first).  For the
    // drop-in's handful of boxes (a farm's thousands are not served one call at a time); MW_SERVER_MOMENTS=0: off.
    drop_driver_moments();               // (single calls patch positions)
    static const bool srvmom = !(std::getenv("MW_SERVER_MOMENTS") && std::getenv("MW_SERVER_MOMENTS")[0] == '0');
    double* mom = nullptr;
    bool allbuilt = true;                // (the full-box kernel over a box that never had a list would follow whatever its arrays hold)
    for (char c : g.h_listbuilt) allbuilt = allbuilt && c != 0;
    if (srvmom && g.nbox <= 64 && model_geo(g.nbox).lds && allbuilt) {
        bool okm = launch_model_energy(1, g.nbox, true, false) == 0 && g.d_mom != nullptr;
        if (okm && !g.d_pm) okm = dev_alloc(g.d_pm, (size_t)g.nbox * g.N * 3) == 0;
        if (okm && !g.d_srvmomok) okm = dev_alloc(g.d_srvmomok, (size_t)g.nbox) == 0;
        if (okm && !g.d_srvunc) okm = dev_alloc(g.d_srvunc, (size_t)g.nbox) == 0;
        if (okm) okm = ensure_event(g.ev_srv, hipEventDisableTiming) == 0;
        if (okm) {
            // (no host wait: the server's stream waits for the moments on the device -- 52 -> 20-odd us per server start, which a host
            //  with volume moves pays every few dozen calls; "still in step" = any non-zero word)
            okm = hipMemcpyAsync(g.d_pm, g.d_pos, (size_t)g.nbox * g.N * 3 * sizeof(double), hipMemcpyDeviceToDevice, g.stream) == hipSuccess
               && hipMemsetAsync(g.d_srvmomok, 1, (size_t)g.nbox * sizeof(int), g.stream) == hipSuccess
               && hipMemsetAsync(g.d_srvunc, 0xff, (size_t)g.nbox * sizeof(int), g.stream) == hipSuccess      // (-1: d_pm is d_pos)
               && hipEventRecord(g.ev_srv, g.stream) == hipSuccess
               && hipStreamWaitEvent(g.sstream, g.ev_srv, 0) == hipSuccess;
        }
        if (okm) mom = g.d_mom;
        else (void)hipGetLastError();
        g.mom_count = 0;                 // (the server will change them under the batch kernels' feet: not theirs to reuse)
    }
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(g.nslots), dim3(64), 0, g.sstream, g.d_head, g.d_slots, g.d_req, g.d_pos, g.d_ivect,
                           g.d_nivect, g.d_listm, g.d_nn, g.N, g.ivcap, 300000LL, stamps ? 1 : 0, mom, g.d_pm, g.d_srvmomok, g.d_srvunc, g.d_srvcounts);
    };
    if (plain) launch(mw::k_local_server<false>);
    else       launch(mw::k_local_server<true>);
    const hipError_t err = hipGetLastError();
    if (sw) (void)hipSetDevice(prev);
    if (err != hipSuccess) return fail("mw: launching the local-energy server failed: %s", hipGetErrorString(err));
    g.srv_running = true;
    ++g.srv_starts;
    return 0;
}

namespace {
// Stop the server and wait for it (called with g_gate held exclusively: no request is in flight).
int server_stop()
{
    std::lock_guard<std::mutex> lk(g_srv_mu);
    if (!g.srv_running) return 0;
    reinterpret_cast<volatile int*>(&g.h_head->quit)[0] = 1;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    int prev = -1;
    const bool sw = hipGetDevice(&prev) == hipSuccess && prev != g.device && hipSetDevice(g.device) == hipSuccess;
    const hipError_t err = hipStreamSynchronize(g.sstream);
    if (sw) (void)hipSetDevice(prev);
    g.srv_running = false;
    if (err != hipSuccess) return fail("mw: the local-energy server ended with %s", hipGetErrorString(err));
    return 0;
}
}  // namespace

// Wait for the reply to request `seq` of mail slot `sl` (the slot's mutex and g_gate shared are held by the caller).
static int server_wait(int sl, unsigned long long seq, double* e)
{
    volatile mw::MailSlot* m = g.h_slots + sl;
    // The reply normally shows within microseconds.  Every few thousand polls (a read of host memory that only changes when
    // a wavefront leaves): is the server still there?  It retires by itself after its idle limit, and a request posted just
    // then would otherwise wait for a restart nobody triggers.  The no-reply limit is wall-clock (MW_SERVER_TIMEOUT seconds,
    // default 20), not a poll count.
    static const double timeout_s = [] { const char* ev = std::getenv("MW_SERVER_TIMEOUT"); const double v = ev ? atof(ev) : 0.0; return v > 0.0 ? v : 20.0; }();
    std::chrono::steady_clock::time_point t_post{};
    for (long spin = 1;; ++spin) {
        if (m->rep_seq == seq) break;
        __builtin_ia32_pause();
        if ((spin & 0xfff) == 0 && reinterpret_cast<volatile int*>(&g.h_head->exited)[0] != 0) {
            std::lock_guard<std::mutex> lk(g_srv_mu);
            if (reinterpret_cast<volatile int*>(&g.h_head->exited)[0] != 0) {
                // it left (idle limit, racing with this request) -- or it faulted: the stream tells.  The slots' wavefronts
                // leave one by one: the others are told to go too (each finishes the request it has; a request posted
                // meanwhile is picked up by the server started below), or a slot kept busy by another thread would
                // hold this one up for as long as it stays busy.
                reinterpret_cast<volatile int*>(&g.h_head->quit)[0] = 1;
                std::atomic_thread_fence(std::memory_order_seq_cst);
                int prev = -1;
                const bool sw = hipGetDevice(&prev) == hipSuccess && prev != g.device && hipSetDevice(g.device) == hipSuccess;
                const hipError_t err = hipStreamSynchronize(g.sstream);
                if (sw) (void)hipSetDevice(prev);
                g.srv_running = false;
                if (err != hipSuccess) return fail("mw: the local-energy server ended with %s", hipGetErrorString(err));
                if (m->rep_seq == seq) break;
                if (server_start_locked()) return 1;          // it picks the pending request up: rep_seq != req_seq
            }
        }
        if ((spin & 0xffff) == 0) {
            const auto now = std::chrono::steady_clock::now();
            if (t_post == std::chrono::steady_clock::time_point{}) t_post = now;
            else if (std::chrono::duration<double>(now - t_post).count() > timeout_s)
                return fail("mw: no reply from the local-energy server within %.0f s", timeout_s);
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (e) *e = m->energy;
    return 0;
}

// Post one request to the resident server (g_gate shared + the slot's mutex held by the caller); returns its sequence number.
static int server_post(int sl, int ils, int imol, const mw::Override& o1, const mw::Override& o2, unsigned long long* seq_out)
{
    { std::lock_guard<std::mutex> lk(g_srv_mu); if (server_start_locked()) return 1; }
    volatile mw::MailSlot* q = g.req_slots + sl;
    q->box = ils - 1; q->imol = imol - 1;
    q->flags = 1 | (o1.idx >= 0 ? 2 : 0) | (o2.idx >= 0 ? 4 : 0);
    q->prev = o2.idx >= 0 ? o2.idx : 0;
    q->x1 = o1.x; q->y1 = o1.y; q->z1 = o1.z;
    q->x2 = o2.x; q->y2 = o2.y; q->z2 = o2.z;
    const unsigned long long seq = ++g.sseq[sl];
    // fields, then the sequence words: program order for write-back host memory; the store fence keeps it for a
    // write-combining mapping of device memory too
    // (the two sequence words need no order between themselves: the server acts when BOTH show the new number)
    std::atomic_thread_fence(std::memory_order_release); __builtin_ia32_sfence();
    q->seq_a = seq;
    q->seq_b = seq;
    __builtin_ia32_sfence();
    *seq_out = seq;
    return 0;
}

static int served_checks(int ils, int imol, const mw::Override& o2)
{
    if (!g.live) return fail("mw: engine not initialised (call mw_init / energy_init first)");
    if (ils < 1 || ils > g.nbox) return fail("mw: box index %d outside 1..%d", ils, g.nbox);
    if (imol < 1 || imol > g.N) return fail("mw: molecule index %d outside 1..%d", imol, g.N);
    if (o2.idx >= g.N) return fail("mw: molecule index %d outside 1..%d", o2.idx + 1, g.N);
    return 0;
}

// One request through the resident server: g_gate shared (no exclusive entry point is running; everything of the context is
// read under the gate: mw_finalize / mw_init rewrite it) + the slot's mutex.
static int local_energy_served(int ils, int imol, const mw::Override& o1, const mw::Override& o2, double* e)
{
    std::shared_lock<std::shared_mutex> gate(g_gate);
    if (served_checks(ils, imol, o2)) return 1;
    const int sl = (ils - 1) % g.nslots;
    std::lock_guard<std::mutex> slk(g_slot_mu[sl]);
    if (g.spend[sl]) {                                        // a posted request nobody collected: its reply first (the slot holds one request)
        const unsigned long long ps = g.spend[sl];
        g.spend[sl] = 0;
        if (server_wait(sl, ps, nullptr)) return 1;
    }
    unsigned long long seq = 0;
    if (server_post(sl, ils, imol, o1, o2, &seq)) return 1;
    return server_wait(sl, seq, e);
}

int mw_local_energy_patched(int ils, int imol, const double r_imol[3], int imol_prev, const double r_prev[3], double* e)
{
    mw::Override o1, o2;
    o1.idx = -1; o1.x = o1.y = o1.z = 0.0;
    o2 = o1;
    if (r_imol) { o1.idx = imol - 1; o1.x = r_imol[0]; o1.y = r_imol[1]; o1.z = r_imol[2]; }
    if (r_prev && imol_prev >= 1 && imol_prev != imol) {
        o2.idx = imol_prev - 1; o2.x = r_prev[0]; o2.y = r_prev[1]; o2.z = r_prev[2];
    }
    if (g_srv_enabled.load(std::memory_order_acquire)) return local_energy_served(ils, imol, o1, o2, e);

    // MW_LOCAL_SERVER=0: one launch per call (the path the server replaces; kept as its cross-check)
    MW_LOCK;
    if (check_live() || check_box(ils) || check_mol(imol)) return 1;
    if (o2.idx >= g.N) return fail("mw: molecule index %d outside 1..%d", o2.idx + 1, g.N);
    drop_driver_moments();               // (the call commits its positions)
    const unsigned long long seq = ++g.pin_seq;
    hipLaunchKernelGGL(mw::k_local_energy_single, dim3(1), dim3(64), 0, g.stream, g.d_pos, g.d_ivect, g.d_listm, g.d_nn,
                       ils - 1, imol - 1, o1, o2, 1, g.d_pin, g.N, g.ivcap,
                       reinterpret_cast<unsigned long long*>(g.d_pin + 8), seq);
    HIPCHK(hipGetLastError());
    // The kernel is the only thing in flight on this stream: wait for its completion word in host-visible memory
    // (a few microseconds less than a stream synchronisation); if it does not show up within a second, fall
    // back to the synchronisation, which also reports a fault.
    volatile unsigned long long* done = reinterpret_cast<volatile unsigned long long*>(g.h_pin + 8);
    bool seen = false;
    std::chrono::steady_clock::time_point t_first{};
    for (long spin = 1;; ++spin) {                       // (a wall clock, like the served path: one second, whatever the host's speed)
        if (*done == seq) { seen = true; break; }
        __builtin_ia32_pause();
        if ((spin & 0xffff) == 0) {
            const auto now = std::chrono::steady_clock::now();
            if (t_first == std::chrono::steady_clock::time_point{}) t_first = now;
            else if (std::chrono::duration<double>(now - t_first).count() > 1.0) break;
        }
    }
    if (!seen) HIPCHK(hipStreamSynchronize(g.stream));
    *e = g.h_pin[0];
    return 0;
}

int mw_local_energy(int ils, int imol, double* e) { return mw_local_energy_patched(ils, imol, nullptr, 0, nullptr, e); }

// The call split in two, for a host that knows its NEXT question while it still waits for the answer to this one (the two
// lattices of a move, mc_moves.F90:1006-1018): post does not wait, collect does.  One posted request per lattice at a time;
// any other single call on that lattice -- or on another lattice of its mail slot (lattices ils and ils + 8 share one) -- waits
// for it first and drops its reply.  Both return 2 -- not an error, no message -- when there is nothing to gain or to collect:
// the resident server is switched off (MW_LOCAL_SERVER=0), nothing was posted for THIS lattice (or its reply was dropped), or an
// entry point that changes device state ran in between (the reply may predate it: ask again).
int mw_local_energy_post(int ils, int imol, const double r_imol[3], int imol_prev, const double r_prev[3])
{
    if (!g_srv_enabled.load(std::memory_order_acquire)) return 2;
    mw::Override o1, o2;
    o1.idx = -1; o1.x = o1.y = o1.z = 0.0;
    o2 = o1;
    if (r_imol) { o1.idx = imol - 1; o1.x = r_imol[0]; o1.y = r_imol[1]; o1.z = r_imol[2]; }
    if (r_prev && imol_prev >= 1 && imol_prev != imol) { o2.idx = imol_prev - 1; o2.x = r_prev[0]; o2.y = r_prev[1]; o2.z = r_prev[2]; }
    std::shared_lock<std::shared_mutex> gate(g_gate);
    if (served_checks(ils, imol, o2)) return 1;
    const int sl = (ils - 1) % g.nslots;
    std::lock_guard<std::mutex> slk(g_slot_mu[sl]);
    if (g.spend[sl]) {
        const unsigned long long ps = g.spend[sl];
        g.spend[sl] = 0;
        if (server_wait(sl, ps, nullptr)) return 1;
    }
    unsigned long long seq = 0;
    if (server_post(sl, ils, imol, o1, o2, &seq)) return 1;
    g.spend[sl] = seq;
    g.spend_box[sl] = ils;
    g.spend_epoch[sl] = g_epoch.load(std::memory_order_relaxed);
    return 0;
}

int mw_local_energy_collect(int ils, double* e)
{
    std::shared_lock<std::shared_mutex> gate(g_gate);
    if (!g.live) return fail("mw: engine not initialised (call mw_init / energy_init first)");
    if (ils < 1 || ils > g.nbox) return fail("mw: box index %d outside 1..%d", ils, g.nbox);
    const int sl = (ils - 1) % g.nslots;
    std::lock_guard<std::mutex> slk(g_slot_mu[sl]);
    const unsigned long long ps = g.spend[sl];
    if (!ps || g.spend_box[sl] != ils) return 2;              // (nothing posted -- or what is pending belongs to another lattice of this slot,
                                                              //  whose post waited for and dropped this lattice's reply: ask again)
    g.spend[sl] = 0;
    if (server_wait(sl, ps, e)) return 1;
    return g.spend_epoch[sl] == g_epoch.load(std::memory_order_relaxed) ? 0 : 2;
}

// Which routine served the single calls of box ils since mw_init, for tests and tools: out = {moment path, scanning routine, plain
// routine, moment updates (of a prev, or of a molecule no request covered), server launches of the whole context}.  An exclusive
// entry point: the server is stopped first, so its counters are complete.  (MW_LOCAL_SERVER=0 serves nothing: zeros.)
int mw_server_counts(int ils, long long out[5])
{
    MW_LOCK;
    if (check_live() || check_box(ils)) return 1;
    if (!out) return fail("mw_server_counts: out is NULL");
    unsigned long long c[4];
    HIPCHK(hipMemcpy(c, g.d_srvcounts + 4 * (size_t)(ils - 1), sizeof c, hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; ++k) out[k] = (long long)c[k];
    out[4] = g.srv_starts;
    return 0;
}

}  // extern "C"
