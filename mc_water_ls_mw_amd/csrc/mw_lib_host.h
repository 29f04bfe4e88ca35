// The host layer the stand-alone device libraries share (libmw_sk.so, libmw_boo.so, libmw_tet.so): the error buffer, growing device buffers,
// the device scope, the cell inverse and the life cycle of a library's stream, events and scratch budget.  Host code only, and
// all of it with internal linkage: every library that includes this keeps an error buffer and a state of its own and exports
// nothing from here.  (libmw_hip.so's host layer, mw_host_ctx.hip.h, is another contract and does not use this.)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

namespace {

char g_err[512] = "";

int fail(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return 1;
}

#define HIPOK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail("%s: %s", #call, hipGetErrorString(e_)); } while (0)

constexpr size_t kDefaultBudget = (size_t)256 << 20;

struct Buf {
    void* p = nullptr;
    size_t cap = 0;
};

int reserve(Buf& b, size_t bytes)
{
    if (bytes <= b.cap) return 0;
    if (b.p) { HIPOK(hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    HIPOK(hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return 0;
}

int release(std::initializer_list<Buf*> bufs)
{
    for (Buf* b : bufs)
        if (b->p) { HIPOK(hipFree(b->p)); *b = Buf{}; }
    return 0;
}

// Makes the library's device current and puts the caller's back when the call is over.
struct DeviceScope {
    int prev = -1;
    hipError_t enter(int device)
    {
        const hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) { prev = -1; return e; }
        return prev == device ? hipSuccess : hipSetDevice(device);
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// H^-1 (row-major) of the cell c (c[3 k + a] = H[a][k]); false if det is 0 or not finite
bool invert_cell(const double* c, double* I, double* det_out)
{
    double H[3][3], C[3][3];
    for (int a = 0; a < 3; ++a) for (int k = 0; k < 3; ++k) H[a][k] = c[3 * k + a];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            C[i][j] = std::fma(H[i1][j1], H[i2][j2], -(H[i1][j2] * H[i2][j1]));
        }
    const double det = std::fma(H[0][0], C[0][0], std::fma(H[0][1], C[0][1], H[0][2] * C[0][2]));
    *det_out = det;
    if (!(det != 0.0) || !std::isfinite(det)) return false;
    for (int a = 0; a < 3; ++a) for (int k = 0; k < 3; ++k) I[3 * a + k] = C[k][a] / det;
    for (int e = 0; e < 9; ++e) if (!std::isfinite(I[e])) return false;
    return true;
}

// What every library holds while it is live; NEV event timers.  A library's State derives from this and adds what is its own.
template <int NEV>
struct Runtime {
    bool live = false;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[NEV] = {};
    size_t budget = kDefaultBudget;
    bool have_last = false;
};

// `who` is the library's init entry, `env_name` its scratch budget variable (MiB).  A failed init leaves nothing behind.
template <int NEV>
int runtime_init(const char* who, const char* env_name, int device, Runtime<NEV>& rt)
{
    if (rt.live) return fail("%s: already initialised", who);
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail("%s: no HIP device available (%s); this library has no CPU fallback", who,
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0) device = 0;
    if (device >= ndev) return fail("%s: device = %d of %d", who, device, ndev);
    size_t budget = kDefaultBudget;
    const char* mb = getenv(env_name);
    if (mb && *mb) {
        char* end = nullptr;
        const long v = strtol(mb, &end, 10);
        if (end == mb || *end || v < 1 || v > (1L << 20)) return fail("%s: %s = '%s' is not a number of MiB in 1..%ld", who, env_name, mb, 1L << 20);
        budget = (size_t)v << 20;
    }
    DeviceScope scope;
    HIPOK(scope.enter(device));
    HIPOK(hipStreamCreateWithFlags(&rt.stream, hipStreamNonBlocking));
    for (auto& ev : rt.ev) {
        const hipError_t ee = hipEventCreate(&ev);
        if (ee != hipSuccess) {                              // give back what was made before failing
            for (auto& made : rt.ev) if (made) { (void)hipEventDestroy(made); made = nullptr; }
            (void)hipStreamDestroy(rt.stream);
            rt.stream = nullptr;
            return fail("%s: hipEventCreate: %s", who, hipGetErrorString(ee));
        }
    }
    rt.device = device;
    rt.budget = budget;
    rt.have_last = false;
    rt.live = true;
    return 0;
}

// Waits for the stream and frees `bufs`, the events and the stream; the caller then resets its State.  Not live: nothing to do.
template <int NEV>
int runtime_finalize(Runtime<NEV>& rt, std::initializer_list<Buf*> bufs)
{
    if (!rt.live) return 0;
    DeviceScope scope;
    HIPOK(scope.enter(rt.device));
    HIPOK(hipStreamSynchronize(rt.stream));
    if (release(bufs)) return 1;
    for (auto& ev : rt.ev) HIPOK(hipEventDestroy(ev));
    HIPOK(hipStreamDestroy(rt.stream));
    return 0;
}

template <int NEV>
int check_live(const char* who, const char* init_name, const Runtime<NEV>& rt)
{
    return rt.live ? 0 : fail("%s: not initialised (call %s first)", who, init_name);
}

void copy_fields(const int* src, int nfields, int* out, int nout) { for (int k = 0; k < nout && k < nfields; ++k) out[k] = src[k]; }

}  // namespace
