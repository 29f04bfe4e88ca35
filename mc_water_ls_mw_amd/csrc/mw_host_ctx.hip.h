// mw_host_ctx.hip.h -- the context of libmw_hip.so and what every subsystem of its host code shares: errors, the locks and
// guards of the entry points, argument checks, the LDS size rules, device buffers, LDS limits and event timers.
#pragma once

namespace {

thread_local std::string g_err;
// Every entry point takes this lock: the engine is one context per process, calls from several host threads (the
// reference's dormant OpenMP would evaluate both lattices concurrently, mc_moves.F90:1006-1018) are serialised.
std::recursive_mutex g_mu;
// The single local-energy call (the drop-in compute_local_real_energy) does not take g_mu: it holds g_gate shared and
// its lattice's mail slot, so two host threads can evaluate the two lattices of a move at the same time
// (mc_moves.F90:1006-1018).  Every other entry point holds g_gate exclusively (outermost level only:
// entry points call each other) and first stops the resident server those calls talk to.
std::shared_mutex g_gate;
int g_depth = 0;                        // nesting of exclusive entry points on the thread that holds g_mu
struct DeviceGuard;
struct ExclusiveGuard;
#define MW_LOCK ExclusiveGuard mw_lock_; DeviceGuard mw_dev_; if (mw_lock_.rc) return 1

int fail(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

#define HIPCHK(call)                                                                             \
    do {                                                                                         \
        hipError_t err__ = (call);                                                               \
        if (err__ != hipSuccess)                                                                 \
            return fail("%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, __LINE__); \
    } while (0)

constexpr int kTimerSlots = 4096;
enum LazyLdsKernel { kLazyForces, kLazyIceQ, kLazyClusters, kLazyRdfSmall, kLazyLdsKernels };   // dynamic LDS limit raised on first use
constexpr int kLdsBudget = 160 * 1024 - 2048;   // leave room for the static reduction arrays

struct Ctx {
    bool live = false;
    int device = 0, N = 0, nbox = 0, S = 0, ivcap = 0;
    int cu = 0, nsplit_max = 0;
    hipStream_t stream = nullptr;
    int disp[MW_DISPATCH_FAMILIES][MW_DISPATCH_FIELDS] = {};   // what the last launch of each family did (mw_last_dispatch); field 0 is the ivcap, 0 before any launch
    // pinned, device-visible scratch for single results
    double* h_pin = nullptr;
    char* h_stage = nullptr; char* d_stage = nullptr; size_t stage_bytes = 0;   // pinned + mapped: one box's cell record / positions on their way in
    double* d_pin = nullptr;
    unsigned long long pin_seq = 0;   // completion word of the single-call kernel (h_pin + 8 doubles)
    hipEvent_t ev[kTimerSlots][2] = {};   // event timers: pairs created on first use (Timers)
    std::vector<void*> owned;             // every device buffer of the context (dev_alloc / dev_grow): release_all frees whatever exists
    bool lds_raised[kLazyLdsKernels] = {};   // raise_lds_limit has served the kernel that asks for its limit on first use
    // cells, positions and image vectors (mw_host_cells.hip.h)
    double* d_pos = nullptr;
    double* d_ivect = nullptr;
    int* d_nivect = nullptr;
    double* d_hmat = nullptr;                    // [box][9] hmatrix(:,:,ils), column-major
    double* d_volume = nullptr;                  // [box] |det hmatrix|
    std::vector<mw::GridDesc> h_grid;
    std::vector<int> h_usegrid;
    bool grid_on_device = false;   // some box of this context has (had) a cell grid: descriptors travel with mw_sweep_sync_cells
    bool force_brute = false;
    // host mirrors
    std::vector<double> h_ivect;   // nbox * ivcap * 3
    std::vector<int> h_nivect;     // nbox
    // neighbour lists (mw_host_lists.hip.h)
    uint32_t* d_list = nullptr;    // slot-major   [box][S][N]
    uint32_t* d_listm = nullptr;   // molecule-major [box][N][64]
    int* d_nn = nullptr;
    int* d_stats = nullptr;
    // sorted slot-major layout (k_list_order): column t of d_list belongs to molecule d_order[t]
    int* d_order = nullptr;        // [box][N]
    int* d_nns = nullptr;          // [box][N]   row length of column t
    int* d_cmax = nullptr;         // [box][ceil(N/64)] longest row of each group of 64 columns
    unsigned char* d_cin = nullptr;   // [box][N]   neighbours inside the energy cutoff when the list was built
    int order_kbits = -1, order_seg = 0;   // sort-key bits and segment length of k_list_order
    // cell-grid neighbour builder
    mw::GridDesc* d_grid = nullptr;
    int* d_usegrid = nullptr;
    int *d_cellid = nullptr, *d_shift = nullptr, *d_sorted = nullptr;
    float4 *d_wrel = nullptr, *d_wpos = nullptr;   // wrapped cell-relative positions (single precision) by molecule / by cell-sorted slot
    int* d_wsh = nullptr;                          // packed shifts by cell-sorted slot
    bool legacy_search = false;                    // MW_CELL_SEARCH=legacy: the one-thread-per-molecule search (cross-check)
    bool sort_in_lds = false;                      // bin + scan + scatter of a box in one workgroup (k_cell_sort_box); MW_CELL_SORT=global: the three kernels
    int *d_ccount = nullptr, *d_cstart = nullptr, *d_ccursor = nullptr;
    int cstride = 0;
    std::vector<char> h_listbuilt;     // per box: a neighbour list has been built (the full-box kernel may be run over it)
    unsigned long long list_version = 1, nnmax_version = 0;   // lists rebuilt <-> cached max row length
    int nnmax_cached = 0;
    // full-box energy (mw_host_energy.hip.h)
    bool model_persist = true;         // MW_MODEL_PERSIST at mw_init (0: one workgroup per box, A/B only)
    double* d_partial = nullptr;
    unsigned long long* d_cpartial = nullptr;
    double* d_energy = nullptr;
    unsigned long long* d_counts = nullptr;
    double* d_mom = nullptr;           // [box][N][kMomStride]: per-molecule moments (k_model_energy's by-product) for the single-move kernel's moment path
    int mom_first = 0, mom_count = 0;  // the boxes whose moments the LAST full-box launch left valid (cleared by everything that may move a molecule)
    // forces, ice classes, ice clusters, pair-distance histograms (mw_host_analysis.hip.h)
    double* d_force = nullptr;         // [box][N][3]: forces of the last mw_model_forces* call (allocated on first use)
    double* d_wpart = nullptr;         // [box][nsplit][9]: its per-workgroup virial partials
    double* d_virial = nullptr;        // [box][9]: its virials, column-major
    double* d_iceq = nullptr;          // [box][N][kIceQStride]: q^ of the last mw_ice_* call (allocated on first use)
    int4* d_icenb = nullptr;           // [box][N]: its first four neighbours of every molecule
    int* d_icen = nullptr;             // [box][N]: its neighbour counts n_i
    uint8_t* d_icecls = nullptr;       // [box][N]: its classes
    int* d_icecnt = nullptr;           // [box][kIceClasses]: its class counts
    double* d_icebond = nullptr;       // [N][S]: the bond values of mw_ice_bonds' box
    int* d_icelabel = nullptr;         // [box][N]: cluster labels of the last mw_ice_clusters* call (allocated on first use)
    int* d_icesize = nullptr;          // [box][N]: the global variant's per-root sizes (allocated when that variant first runs)
    int* d_icesum = nullptr;           // [box][4] summaries, then [box] hook / compress rounds
    bool clusters_lds = true;          // MW_ICE_CLUSTERS_LDS at mw_init (0: the global variant at any size)
    int clast[4] = {0, 0, 0, 0};       // the last cluster launch: first box (1-based), boxes, LDS variant, threads per workgroup
    unsigned long long* d_rdf = nullptr;   // [box][nbins of the last call]: pair-distance histograms of the last mw_rdf* call
    size_t rdf_bins = 0;               // ... allocated for nbox x rdf_bins counts (grown on demand)
    // device-resident translation driver, walker = nlat consecutive boxes (mw_host_sweep.hip.h)
    int swm_first = 0, swm_count = 0;  // the boxes (1-based first) whose moments in d_mom the Monte Carlo driver keeps current from launch to launch
                                       // (walkers in global memory): cleared by every entry point that writes positions or cells behind the driver's back
    int last_sweep[6] = {0, 0, 0, 0, 0, 0};   // what the last launch of the driver was: lattices, look-ahead, residency, volume moves, LDS bytes, row stride
    bool sweep_ready = false;
    mw::SweepParams sp;
    int nwalkers = 0;
    double *d_sw_mubin = nullptr, *d_sw_binwidth = nullptr;
    double *d_wweight = nullptr, *d_whist = nullptr, *d_wuhist = nullptr;   // [walker][nbins]
    unsigned long long* d_wswitch = nullptr;
    double* d_wshift = nullptr;      // per walker: sum of the minima mc_update_wl_bins subtracted since the last read-out
    double* d_tabscratch = nullptr;  // [3 nbins last | 3 nbins out | chunks x nbins partial] for mw_sweep_reduce_tables
    size_t tabscratch_n = 0;
    unsigned long long* d_wvol = nullptr;        // [walker][2] volume moves attempted / accepted
    int* d_wflag = nullptr;                      // [walker] bit 0: a volume move needed more image vectors than ivcap; bit 1: 'dd' walker outside its window at eq_mc_cycles
    double* d_wwin = nullptr;                    // [walker][4] start_bin, end_bin, mu_lo, mu_hi ('dd' windows); used when has_windows
    double *d_wfac = nullptr, *d_wsum = nullptr; // [walker] Wang-Landau increment, Swetnam's visit total
    int* d_winflag = nullptr;                    // [walker] walker_in_window
    double* d_wmom = nullptr; size_t wmom_cap = 0;   // the driver's moment scratch (doubles), grown on demand
    double* d_wstep = nullptr;                   // [walker][2] max_trans, dv_max (bohr) when the walkers' step sizes differ (mw_sweep_steps)
    bool has_steps = false;
    int sweep_log_ahead = 8;                     // look-ahead allowed when the move log is on (tests pin it to compare builds)
    bool has_windows = false;
    int* d_wls = nullptr;
    double* d_wmu = nullptr;
    unsigned long long* d_wacc = nullptr;
    double* d_swlog = nullptr;
    size_t swlog_cap = 0;
    // resident server of the single local-energy call, k_local_server: mail slots in host-mapped memory (mw_host_server.hip.h)
    hipStream_t sstream = nullptr;
    mw::MailHead* h_head = nullptr;  mw::MailHead* d_head = nullptr;
    mw::MailSlot* h_slots = nullptr; mw::MailSlot* d_slots = nullptr;
    mw::MailSlot* req_slots = nullptr;  // where requests are posted: h_slots, or device memory the host writes through the BAR
    mw::MailSlot* d_req = nullptr;      // the same lines as the server kernel addresses them
    void* req_dev_alloc = nullptr;
    int nslots = 0;
    bool srv_running = false, srv_enabled = true;
    unsigned long long sseq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long spend[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // per slot: sequence number of a posted, not yet collected request (0: none)
    unsigned long long spend_epoch[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int spend_box[8] = {0, 0, 0, 0, 0, 0, 0, 0};                // ... and the lattice it belongs to (a slot serves every nslots-th lattice)
    hipEvent_t ev_srv = nullptr;                     // the server's stream waits on it for the moments made on the main stream
    double* d_pm = nullptr; int* d_srvmomok = nullptr;   // the resident server's moment path: the positions its moments were made from [nbox][N][3]; per box, still in step
    int* d_srvunc = nullptr;                         // ... per box, the molecule whose committed position d_pm does not hold yet (-1: none)
    unsigned long long* d_srvcounts = nullptr;       // [nbox][4] since mw_init: requests by routine, moment updates (mw_server_counts)
    long long srv_starts = 0;                        // launches of the server since mw_init
    // staged moves (mw_host_moves.hip.h)
    int mcap = 0, mn = 0;
    int* d_mimol = nullptr;
    double *d_mtrial = nullptr, *d_meold = nullptr, *d_menew = nullptr;
    unsigned int* d_mcnt = nullptr;
    unsigned int* d_mtot = nullptr; int mtot_cap = 0, mtot_n = 0;   // [work item][4]: the counts of the requests the move kernel's moment path served (d_mcnt holds 0 for those)
    int* d_mperm = nullptr;        // sorted request -> caller's index
    int* d_mdecl = nullptr;        // [0], [1] counts (alternate launches), then {request, box} of the requests k_move_energy left to k_move_fallback
    int mdecl_par = 0;             // which count word the next launch uses (the fallback kernel zeroes the other)
    int4* d_mwork = nullptr;       // work items {box, begin, end, 0}
    int mwork_cap = 0, mwork_n = 0, mwork_first = -1;   // (mwork_first: the box the work list starts from, before the XCD dealing; for mw_last_dispatch)
    bool mlds = false;
    int mmode = 0;
    int m_boxlo = 0, m_boxhi = -1, m_minreq = 0;   // the uploaded requests: their boxes (0-based range) and the fewest requests any of them has
    // The moment path's launch does not count (mw_move_energy.hip.h, mode bit 3): mw_moves_counts makes the counts of the last launch
    // with one more pass of the same kernel over the same work items -- for as long as that pass would still count what the launch saw.
    enum { kCountsThere = 0, kCountsPending = 1, kCountsDropped = 2 };
    int mcnt_state = kCountsThere;     // There: d_mcnt / d_mtot hold them; Pending: to be made on demand; Dropped: a pending launch's requests,
                                       // positions, cells or lists have changed since -- they cannot be made any more
    int mcnt_passes = 0;               // on-demand count passes launched since mw_init
    bool move_sort = true;             // MW_MOVE_SORT != 0 at mw_moves_upload: the moment path sorts an item's requests by in-range neighbours
    bool move_masks = true;            // MW_MOVE_MASKS != 0 at mw_moves_upload: the sorted moment path rebuilds its queues from the count pass's row-slot masks
    bool move_gate = true;             // MW_MOVE_GATE != 0 at mw_moves_upload: the 0.99 rule's pair pass tests angles only behind the triangle-area gate
    bool move_pairs32 = true;          // MW_MOVE_PAIRS32 != 0 at mw_moves_upload: a walking group runs the f32 pair gate from its registers in front of that pass
    bool move_counts_eager = false;   // MW_MOVE_COUNTS=eager at mw_init: the launch itself counts, as it used to
    int move_moments = -1;             // MW_MOVE_MOMENTS at mw_init: -1 unset (the request-count rule), 0 scanning path, 1 moment path where admitted
    int mchunk = 16;                 // requests per work item of the uploaded batch
    bool m_noself = false;           // every box of the uploaded batch went through the cell grid: no molecule meets an image of itself
};

Ctx g;
std::mutex g_slot_mu[8];                // one per mail slot
std::mutex g_srv_mu;                    // start / stop of the server
std::atomic<unsigned long long> g_epoch{0};   // bumped by every exclusive entry point: a reply posted before, collected after, is stale
std::atomic<bool> g_srv_enabled{true};  // MW_LOCAL_SERVER != 0 (read by the single call before it holds any lock)

int server_stop();                      // defined below (needs the context)

struct ExclusiveGuard {
    int rc = 0;                         // a fault of the resident server surfaces HERE, at the entry point that stopped it
    ExclusiveGuard()
    {
        g_mu.lock();
        if (g_depth++ == 0) {
            g_gate.lock(); g_epoch.fetch_add(1, std::memory_order_relaxed);
            g.mom_count = 0;            // moments of an earlier entry point's full-box pass: positions may have moved since (only a pass
                                        // inside THIS entry point -- mw_step_launch -- makes them valid for its move kernel)
            if (g.srv_running) rc = server_stop();
            // A request posted ahead (mw_local_energy_post) that the server never got to -- it left between the post and this
            // entry point -- is CANCELLED: marked as answered, so that the server started by the next single call does not
            // replay it and commit its stale override positions over what this entry point is about to upload.  (Its collect
            // returns 2, "ask again", because of the epoch.)  The server is stopped: nobody else writes the reply lines.
            if (g.live && g.h_slots)
                for (int sl = 0; sl < g.nslots && sl < 8; ++sl)
                    if (g.spend[sl] && reinterpret_cast<volatile unsigned long long*>(&g.h_slots[sl].rep_seq)[0] != g.spend[sl]) {
                        reinterpret_cast<volatile unsigned long long*>(&g.h_slots[sl].rep_seq)[0] = g.spend[sl];
                        std::atomic_thread_fence(std::memory_order_seq_cst);
                    }
        }
    }
    ~ExclusiveGuard()
    {
        if (--g_depth == 0) g_gate.unlock();
        g_mu.unlock();
    }
};

// The current HIP device is per host thread: an entry point called from a thread other than the one that ran
// mw_init (the reference's OpenMP sections, a Python worker thread) would otherwise allocate and launch on
// device 0.  Every entry point makes the engine's device current and restores the caller's on return.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    DeviceGuard()
    {
        if (g.live && hipGetDevice(&prev) == hipSuccess && prev != g.device)
            switched = hipSetDevice(g.device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

constexpr size_t kQueue1024 = (size_t)(mw::kQCap + 1) * 1024 * sizeof(uint32_t);
constexpr size_t kQueue256 = (size_t)(mw::kQCap + 1) * 256 * sizeof(uint32_t);
constexpr int kFullLayout = mw::kLayoutPair;      // LDS layout of the full-box kernel's staged vectors (mw_full_energy.hip.h)
// Dynamic LDS of each LDS-staged build and the rules that admit it: the launches and mw_lds_plan use these and nothing else.
size_t model_lds_bytes(int N, int ivcap) { return kQueue1024 + mw::lds_vec_bytes((size_t)N) + mw::lds_vec_bytes((size_t)ivcap); }
bool lds_fits(int N, int ivcap)
{
    return model_lds_bytes(N, ivcap) <= (size_t)kLdsBudget;
}
size_t pos_lds_bytes(int N, int ivcap) { return mw::lds_vec_bytes((size_t)N) + mw::lds_vec_bytes((size_t)ivcap); }   // force pass, ice pass 1
constexpr size_t kMoveScratch = 16 * sizeof(mw::WaveScratch);
// (chunk: requests per work item, whose molecules an item keeps in LDS -- at most kMoveChunk)
size_t move_lds_bytes(int N, int ivcap, int chunk)
{
    return kMoveScratch + mw::lds_vec_bytes((size_t)ivcap) + mw::lds_vec_bytes((size_t)N) + (((size_t)N + 7) & ~(size_t)7) + (size_t)chunk * sizeof(int);
}
// (the moment path packs a molecule's index into kKeyMolBits bits of a request's key: every N that fits pays 25 bytes a molecule)
static_assert((size_t)kLdsBudget / 25 < ((size_t)1 << mw::kKeyMolBits), "a staged box's molecules fit the key of mw_move_energy.hip.h");
bool lds_fits_move(int N, int ivcap)
{
    return move_lds_bytes(N, ivcap, mw::kMoveChunk) <= (size_t)kLdsBudget;
}
int cell_stride(int N) { return N + 64; }
size_t sort_lds_bytes(int N) { return (size_t)N * 24 + ((size_t)cell_stride(N) + 1) * 4; }
bool sort_fits(int N) { return N <= mw::kSortBoxMax; }
// Segment length and sort-key bits of k_list_order: the whole box when the full-box kernel stages its positions in LDS (at the
// ivcap of mw_init), else the 64 molecules of a wavefront; the (key, group) table must fit kOrderSlots.
void order_plan(int N, int seg_override, int& seg, int& kbits)
{
    seg = lds_fits(N, 32) ? ((N + 63) & ~63) : 64;
    if (seg_override >= 64) seg = (seg_override + 63) & ~63;
    const size_t seg_groups = ((size_t)std::min(N, seg) + 63) / 64;
    kbits = -1;
    for (int kb = 8; kb >= 0; --kb)
        if ((seg_groups << kb) <= (size_t)mw::kOrderSlots) { kbits = kb; break; }
}
size_t order_lds_bytes(int N, int seg, int kbits)
{
    return kbits < 0 ? 0 : sizeof(int) * ((((size_t)std::min(N, seg) + 63) / 64) << kbits);
}

int check_live() { return g.live ? 0 : fail("mw: engine not initialised (call mw_init / energy_init first)"); }
int check_box(int ils) { return (ils >= 1 && ils <= g.nbox) ? 0 : fail("mw: box index %d outside 1..%d", ils, g.nbox); }
int check_range(int first, int count)
{
    return (first >= 1 && count >= 1 && first + count - 1 <= g.nbox)
               ? 0 : fail("mw: box range %d..%d outside 1..%d", first, first + count - 1, g.nbox);
}
int check_mol(int imol) { return (imol >= 1 && imol <= g.N) ? 0 : fail("mw: molecule index %d outside 1..%d", imol, g.N); }
// The forms an entry point comes in: the launch alone (results stay on the device), a range of boxes with its results
// fetched, and the one-box form, whose messages name a box, not a range.
enum Form { kLaunch, kBatch, kSingle };
int check_boxes(int first, int count, Form form) { return form == kSingle ? check_box(first) : check_range(first, count); }

// The Monte Carlo driver's moments (d_mom, swm_first / swm_count) describe positions and cells as the driver left them: every
// entry point that writes either behind its back calls this -- under its lock, or a launch of the driver on another thread
// could claim them again in between.
// The same entry points end a move launch's claim to counts it has not made yet (mw_moves_counts): a count pass after them would
// count another state than the launch evaluated.  `state_changed` = false: the full-box pass rewriting d_mom from unchanged positions.
void drop_move_counts() { if (g.mcnt_state == Ctx::kCountsPending) g.mcnt_state = Ctx::kCountsDropped; }
void drop_driver_moments(bool state_changed = true) { g.swm_count = 0; if (state_changed) drop_move_counts(); }

// Device buffers of the context.  Every one is taken and given back here, and g.owned knows them all: a buffer allocated on
// first use, or grown on demand, needs no entry anywhere for release_all to free it.  (Not for the single call's path, which
// allocates nothing; callers hold g_gate exclusively, or shared together with g_srv_mu.)
int dev_free_bytes(void** p)
{
    if (!*p) return 0;
    g.owned.erase(std::remove(g.owned.begin(), g.owned.end(), *p), g.owned.end());
    void* q = *p;
    *p = nullptr;
    HIPCHK(hipFree(q));
    return 0;
}
int dev_alloc_bytes(void** p, size_t bytes)
{
    if (*p) {                            // a buffer in use gives way to a new one: nothing on the stream may still read it
        HIPCHK(hipStreamSynchronize(g.stream));
        if (dev_free_bytes(p)) return 1;
    }
    HIPCHK(hipMalloc(p, bytes));
    g.owned.push_back(*p);
    return 0;
}
// n elements, uninitialised; an existing buffer is freed first (its contents are NOT kept)
template <class T> int dev_alloc(T*& p, size_t n) { return dev_alloc_bytes(reinterpret_cast<void**>(&p), n * sizeof(T)); }
template <class T> int dev_alloc_zeroed(T*& p, size_t n)
{
    if (dev_alloc(p, n)) return 1;
    HIPCHK(hipMemset(p, 0, n * sizeof(T)));
    return 0;
}
// Grown on demand: room for `need` units (of `per` elements each) in a buffer that holds `cap` of them; a new buffer takes `newcap`.
template <class T, class C> int dev_grow(T*& p, C& cap, size_t need, size_t newcap, size_t per = 1)
{
    if (need == 0 || (p && (size_t)cap >= need)) return 0;
    cap = 0;
    if (dev_alloc(p, newcap * per)) return 1;
    cap = (C)newcap;
    return 0;
}
void dev_free_all()
{
    for (void* p : g.owned) (void)hipFree(p);
    g.owned.clear();
}

// A kernel that asks for more than the default 64 KiB of dynamic LDS has its limit raised first: at mw_init, or -- with the
// kernel's flag in g.lds_raised -- when it is first launched.
int raise_lds_limit(const void* kernel, size_t bytes, int lazy = -1)
{
    if (lazy >= 0 && g.lds_raised[lazy]) return 0;
    HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (lazy >= 0) g.lds_raised[lazy] = true;
    return 0;
}
template <class K> int raise_lds_limit(K* kernel, size_t bytes, int lazy = -1)
{
    return raise_lds_limit(reinterpret_cast<const void*>(kernel), bytes, lazy);
}

int ensure_event(hipEvent_t& e, unsigned flags = hipEventDefault)
{
    if (!e) HIPCHK(hipEventCreateWithFlags(&e, flags));
    return 0;
}

// Event timers.  A launch that is timed takes n consecutive slots from `first` (slot k of them brackets its k-th part); open()
// checks the span for the entry point `who` and creates the event pairs -- before the launch allocates, reads back or launches
// anything.  A negative slot means untimed: open() admits it and start() / stop() do nothing.
int check_timer_span(const char* who, int slot, int n)
{
    return (slot >= 0 && slot + n <= kTimerSlots) ? 0 : fail("%s: timer slot %d outside 0..%d", who, slot, kTimerSlots - n);
}
struct Timers {
    int first = -1;
    int open(const char* who, int slot, int n)
    {
        if (slot < 0) return 0;
        if (check_timer_span(who, slot, n)) return 1;
        for (int s = slot; s < slot + n; ++s)
            if (ensure_event(g.ev[s][0]) || ensure_event(g.ev[s][1])) return 1;
        first = slot;
        return 0;
    }
    int record(int k, int end) const
    {
        if (first >= 0) HIPCHK(hipEventRecord(g.ev[first + k][end], g.stream));
        return 0;
    }
    int start(int k = 0) const { return record(k, 0); }
    int stop(int k = 0) const { return record(k, 1); }
};

}  // namespace
