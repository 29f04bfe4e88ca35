// mw_api.hip -- the C ABI of libmw_hip.so (include/mw_energy.h): context, device
// mirrors of the host's model::ljr / model::hmatrix, launch logic.
//
// Host-side state mirrors what the reference's `module energy` keeps
// (molint.F90:41-45,79-81): nivect/ivect per box, the neighbour list, and the
// energies of the last evaluation.  There is no CPU compute path here: every
// energy and every list comes from the gfx950 kernels in mw_kernels.hip.h.
#include "mw_kernels.hip.h"
#include "../../include/mw_energy.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <mutex>
#include <shared_mutex>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include <unistd.h>

// The host code lives in these headers, one per subsystem, included once and in this order.  The order is also the order in which
// the kernel templates are first named, and with it their order in the code object: a header that moves takes kernels with it.
#include "mw_host_ctx.hip.h"
#include "mw_host_cells.hip.h"
#include "mw_host_lists.hip.h"
#include "mw_host_energy.hip.h"
#include "mw_host_analysis.hip.h"
#include "mw_host_sweep.hip.h"
#include "mw_host_init.hip.h"
#include "mw_host_server.hip.h"
#include "mw_host_moves.hip.h"

extern "C" {

const char* mw_last_error(void) { return g_err.c_str(); }

int mw_is_initialised(void) { return g.live ? 1 : 0; }

int mw_constants(double out[8])
{
    MW_LOCK;
    out[0] = mw::kSigma; out[1] = mw::kEpsilon; out[2] = mw::kLambda; out[3] = mw::kBigA;
    out[4] = mw::kBigB;  out[5] = mw::kGamma;   out[6] = mw::kSmallA; out[7] = mw::kCos0;
    return 0;
}

int mw_device_info(char* name, int name_len, int* compute_units, long long* global_mem)
{
    MW_LOCK;
    if (check_live()) return 1;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, g.device));
    if (name && name_len > 0) { std::strncpy(name, prop.name, (size_t)name_len - 1); name[name_len - 1] = 0; }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (global_mem) *global_mem = (long long)prop.totalGlobalMem;
    return 0;
}

int mw_last_dispatch(int family, int* fields, int nfields)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (family < 0 || family >= MW_DISPATCH_FAMILIES) return fail("mw_last_dispatch: family %d outside 0..%d", family, MW_DISPATCH_FAMILIES - 1);
    if (g.disp[family][0] == 0) return fail("mw_last_dispatch: no launch of family %d yet", family);
    if (fields) for (int k = 0; k < nfields && k < MW_DISPATCH_FIELDS; ++k) fields[k] = g.disp[family][k];
    return 0;
}

int mw_lds_plan(int nwater, int image_capacity, int* out, int nout)
{
    if (nwater < 1 || nwater > (1 << mw::kJBits) || image_capacity < 1 || image_capacity > MW_MAX_IVECT) return -1;
    int seg = 0, kbits = 0;
    order_plan(nwater, 0, seg, kbits);
    const long long plan[MW_LDS_BUILDS][2] = {
        {lds_fits(nwater, image_capacity), (long long)model_lds_bytes(nwater, image_capacity)},
        {lds_fits(nwater, image_capacity), (long long)pos_lds_bytes(nwater, image_capacity)},
        {lds_fits(nwater, image_capacity), (long long)pos_lds_bytes(nwater, image_capacity)},
        {lds_fits_move(nwater, image_capacity), (long long)move_lds_bytes(nwater, image_capacity, mw::kMoveChunk)},
        {sort_fits(nwater), (long long)sort_lds_bytes(nwater)},
        {seg >= nwater, (long long)order_lds_bytes(nwater, seg, kbits)}};
    if (out) for (int k = 0; k < 2 * MW_LDS_BUILDS && k < nout; ++k) out[k] = (int)plan[k / 2][k % 2];
    return MW_LDS_BUILDS;
}

int mw_sync(void)
{
    MW_LOCK;
    if (check_live()) return 1;
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_timer_start(int slot)
{
    MW_LOCK;
    if (check_live()) return 1;
    Timers t;
    if (check_timer_span("mw_timer_start", slot, 1) || t.open("mw_timer_start", slot, 1)) return 1;
    return t.start();
}

int mw_timer_stop(int slot)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (check_timer_span("mw_timer_stop", slot, 1)) return 1;
    if (!g.ev[slot][1]) return fail("mw_timer_stop: slot %d was never started", slot);
    HIPCHK(hipEventRecord(g.ev[slot][1], g.stream));
    return 0;
}

int mw_timer_elapsed_ms(int slot, float* ms)
{
    MW_LOCK;
    if (check_live()) return 1;
    if (check_timer_span("mw_timer_elapsed_ms", slot, 1)) return 1;
    if (!g.ev[slot][1]) return fail("mw_timer_elapsed_ms: slot %d was never started", slot);
    HIPCHK(hipEventSynchronize(g.ev[slot][1]));
    HIPCHK(hipEventElapsedTime(ms, g.ev[slot][0], g.ev[slot][1]));
    return 0;
}

}  // extern "C"
