// libmw_sk.so -- the static structure factor of include/mw_sk.h: rho_b(n) = sum_j exp(-2 pi i n . s_j), S = |rho|^2 / N, for
// many boxes and one list of integer triples.  Two passes per chunk of boxes: k_sk_phasors writes the per-axis tables
// E_a(m) = exp(2 pi i m s_a) of every molecule to scratch, k_sk_sum walks them through LDS tiles with a few k-vectors per
// lane; k_sk_finish adds the segments' partial sums in segment order.  Boxes of <= 64 molecules make their tables in the sum
// kernel's LDS.  Every bit of rho depends on the box and n alone (mw_sk.h): the arithmetic below is spelled out in fma /
// mul / add with contraction off, and both geometries share it.
#include "../../include/mw_sk.h"

#include "mw_common.hip.h"

#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too

namespace mwsk {

constexpr int kThreads = 256;
constexpr int kVecPerLane = 2;
constexpr int kVecPerWg = kThreads * kVecPerLane;
constexpr int kSegment = 1024;                 // molecules per partial sum, times ceil(N / 8192): at most eight partial sums per
                                               // vector however large the box -- a function of N alone, like the order of the sum
constexpr int kSmallN = 64;
constexpr int kLdsCap = 64 * 1024;             // dynamic LDS a sum workgroup may ask for
constexpr int kMaxTile = 32;
constexpr int kMaxWater = 1 << 22;
constexpr int kMaxBoxes = 1 << 24;
constexpr int kMaxChunkBoxes = 65535;          // grid z

// s_a = (H^-1 r)_a reduced to [-1/2, 1/2]; I = H^-1, row-major
__device__ __forceinline__ double frac_coord(const double* __restrict__ I, int a, double x, double y, double z)
{
    const double s = __builtin_fma(I[3 * a], x, __builtin_fma(I[3 * a + 1], y, I[3 * a + 2] * z));
    return s - __builtin_rint(s);
}

// E(m) = exp(2 pi i m s) as (cos, sin)
__device__ __forceinline__ double2 phasor(double s, int m)
{
    double sn, cs;
    sincospi((2.0 * (double)m) * s, &sn, &cs);
    return make_double2(cs, sn);
}

__device__ __forceinline__ double flip(double v, int signbit) { return __hiloint2double(__double2hiint(v) ^ signbit, __double2loint(v)); }

// One lane per (box, molecule): s_j and the three tables, T[box][row][j] with row = (axis, m), j fastest.
__global__ __launch_bounds__(kThreads) void k_sk_phasors(int nb, int n, int nmax0, int nmax1, int nmax2, const double* __restrict__ inv,
                                                         const double* __restrict__ pos, double2* __restrict__ T)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)nb * n) return;
    const int b = (int)(t / n), j = (int)(t - (long long)b * n);
    const double* I = inv + 9 * (size_t)b;
    const double x = pos[3 * t], y = pos[3 * t + 1], z = pos[3 * t + 2];
    const int rows = nmax0 + nmax1 + nmax2 + 3;
    double2* out = T + (size_t)b * rows * n + j;
    const int nmax[3] = {nmax0, nmax1, nmax2};
    int row = 0;
    for (int a = 0; a < 3; ++a) {
        const double s = frac_coord(I, a, x, y, z);
        for (int m = 0; m <= nmax[a]; ++m, ++row) out[(size_t)row * n] = phasor(s, m);
    }
}

// Workgroup (k-tile, segment, box): lane l owns vectors tile * kVecPerWg + l + q * kThreads, q < kVecPerLane, and adds the
// molecules of its segment one after the other.  LDS tile[row][jj], row stride `stride` 16-byte slots (odd: lanes that read
// the same molecule at different m fall into different slots of the 256-byte bank row).  FUSED: the box has <= 64 molecules
// and the tile, the whole box, is computed here instead of copied from T.
template <bool FUSED>
__global__ __launch_bounds__(kThreads) void k_sk_sum(int n, int M, int nmax0, int nmax1, int nmax2, int jtlog, int stride,
                                                     int seglen, const int* __restrict__ nvec, const double2* __restrict__ T,
                                                     const double* __restrict__ inv, const double* __restrict__ pos,
                                                     double2* __restrict__ part)
{
    extern __shared__ double2 tile[];
    const int tid = threadIdx.x, seg = blockIdx.y, b = blockIdx.z, nseg = gridDim.y;
    const int off1 = nmax0 + 1, off2 = off1 + nmax1 + 1, rows = off2 + nmax2 + 1;
    int a0[kVecPerLane], a1[kVecPerLane], a2[kVecPerLane], f0[kVecPerLane], f1[kVecPerLane], f2[kVecPerLane];
    double re[kVecPerLane], im[kVecPerLane];
#pragma unroll
    for (int q = 0; q < kVecPerLane; ++q) {
        const int v = blockIdx.x * kVecPerWg + q * kThreads + tid;
        int c0 = 0, c1 = 0, c2 = 0;
        if (v < M) { c0 = nvec[3 * (size_t)v]; c1 = nvec[3 * (size_t)v + 1]; c2 = nvec[3 * (size_t)v + 2]; }
        a0[q] = abs(c0) * stride;           f0[q] = c0 < 0 ? (int)0x80000000 : 0;
        a1[q] = (off1 + abs(c1)) * stride;  f1[q] = c1 < 0 ? (int)0x80000000 : 0;
        a2[q] = (off2 + abs(c2)) * stride;  f2[q] = c2 < 0 ? (int)0x80000000 : 0;
        re[q] = 0.0; im[q] = 0.0;
    }
    const int jbeg = seg * seglen, jend = min(n, jbeg + seglen);
    const int jt = FUSED ? n : (1 << jtlog);
    const double2* Tb = FUSED ? nullptr : T + (size_t)b * rows * n;
    for (int j0 = jbeg; j0 < jend; j0 += jt) {
        const int cnt = min(jt, jend - j0);
        if constexpr (FUSED) {
            const double* I = inv + 9 * (size_t)b;
            const double* r = pos + 3 * (size_t)b * n;
            for (int idx = tid; idx < rows * n; idx += kThreads) {
                const int row = idx / n, jj = idx - row * n;
                const int a = (row >= off1) + (row >= off2);
                const int m = row - (a == 0 ? 0 : a == 1 ? off1 : off2);
                const double s = frac_coord(I, a, r[3 * jj], r[3 * jj + 1], r[3 * jj + 2]);
                tile[row * stride + jj] = phasor(s, m);
            }
        } else {
            for (int idx = tid; idx < (rows << jtlog); idx += kThreads) {
                const int row = idx >> jtlog, jj = idx & (jt - 1);
                if (jj < cnt) tile[row * stride + jj] = Tb[(size_t)row * n + j0 + jj];
            }
        }
        __syncthreads();
        for (int jj = 0; jj < cnt; ++jj) {
#pragma unroll
            for (int q = 0; q < kVecPerLane; ++q) {
                const double2 e0 = tile[a0[q] + jj], e1 = tile[a1[q] + jj], e2 = tile[a2[q] + jj];
                const double y0 = flip(e0.y, f0[q]), y1 = flip(e1.y, f1[q]), y2 = flip(e2.y, f2[q]);
                const double pr = __builtin_fma(e0.x, e1.x, -(y0 * y1));
                const double pi = __builtin_fma(e0.x, y1, y0 * e1.x);
                const double qr = __builtin_fma(pr, e2.x, -(pi * y2));
                const double qi = __builtin_fma(pr, y2, pi * e2.x);
                re[q] = re[q] + qr;
                im[q] = im[q] - qi;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < kVecPerLane; ++q) {
        const int v = blockIdx.x * kVecPerWg + q * kThreads + tid;
        if (v < M) part[((size_t)b * nseg + seg) * M + v] = make_double2(re[q], im[q]);
    }
}

// One lane per (box, vector): the segments' sums in segment order, then S.
__global__ __launch_bounds__(kThreads) void k_sk_finish(int nb, int n, int M, int nseg, const double2* __restrict__ part,
                                                        double* __restrict__ rho, double* __restrict__ S)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)nb * M) return;
    const int b = (int)(t / M), v = (int)(t - (long long)b * M);
    const double2* p = part + (size_t)b * nseg * M + v;
    double re = p[0].x, im = p[0].y;
    for (int s = 1; s < nseg; ++s) { const double2 w = p[(size_t)s * M]; re = re + w.x; im = im + w.y; }
    if (rho) { rho[2 * t] = re; rho[2 * t + 1] = im; }
    if (S) S[t] = __builtin_fma(re, re, im * im) / (double)n;
}

// One lane per (group, vector): the walkers' S in walker order.
__global__ __launch_bounds__(kThreads) void k_sk_mean(int ngroups, int nwalkers, int M, const double* __restrict__ S, double* __restrict__ mean)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)ngroups * M) return;
    const int g = (int)(t / M), v = (int)(t - (long long)g * M);
    double acc = 0.0;
    for (int w = 0; w < nwalkers; ++w) acc = acc + S[((size_t)w * ngroups + g) * M + v];
    mean[t] = acc / (double)nwalkers;
}

}  // namespace mwsk

namespace {

using namespace mwsk;

struct State : Runtime<3> {
    Buf scratch, inv, pos, nvec, rho, S, Sall, mean;
    int last[MW_SK_PLAN_FIELDS] = {0};
    float ms_phasors = 0.0f, ms_sums = 0.0f;
} g;

struct Plan {
    int small, rows, tile, jtlog, stride, nseg, seglen, bpc, chunks;
    size_t lds, per_box;
};

// The launch rules (mw_sk_plan reports them; the launches follow them).
int make_plan(const char* who, int n, const int nmax[3], int M, int nboxes, size_t budget, Plan& p)
{
    p.rows = nmax[0] + nmax[1] + nmax[2] + 3;
    const int small_stride = n | 1;
    p.small = n <= kSmallN && (size_t)p.rows * small_stride * 16 <= (size_t)kLdsCap;
    p.seglen = kSegment * ((n + 8 * kSegment - 1) / (8 * kSegment));
    if (p.small) {
        p.tile = n; p.jtlog = 0; p.stride = small_stride; p.nseg = 1;
    } else {
        p.tile = kMaxTile; p.jtlog = 5;
        while ((size_t)p.rows * (p.tile + 1) * 16 > (size_t)kLdsCap) { p.tile >>= 1; --p.jtlog; }    // 768 rows still admit 4
        p.stride = p.tile + 1;
        p.nseg = (n + p.seglen - 1) / p.seglen;
    }
    p.lds = (size_t)p.rows * p.stride * 16;
    p.per_box = (p.small ? 0 : (size_t)n * p.rows * 16) + (size_t)p.nseg * M * 16;
    const size_t fit = budget / p.per_box;
    if (fit < 1)
        return fail("%s: one box needs %zu bytes of scratch (nwater = %d, %d table rows, M = %d) and does not fit the budget of %zu bytes "
                    "(MW_SK_SCRATCH_MB)", who, p.per_box, n, p.rows, M, budget);
    p.bpc = (int)(fit < (size_t)kMaxChunkBoxes ? fit : (size_t)kMaxChunkBoxes);
    if (p.bpc > nboxes) p.bpc = nboxes;
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

void plan_fields(const Plan& p, int* f)
{
    f[0] = p.bpc; f[1] = p.chunks; f[2] = kVecPerLane; f[3] = p.nseg; f[4] = (int)p.lds; f[5] = p.small;
    f[6] = p.tile; f[7] = p.seglen; f[8] = kVecPerWg;
}

int check_sizes(const char* who, int nboxes, int n, int M)
{
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    if (M < 1 || M > MW_SK_MAX_VECTORS) return fail("%s: M = %d outside 1..%d", who, M, MW_SK_MAX_VECTORS);
    return 0;
}

int check_nvec(const char* who, int M, const int* nvec, int nmax[3])
{
    nmax[0] = nmax[1] = nmax[2] = 0;
    for (int v = 0; v < M; ++v)
        for (int a = 0; a < 3; ++a) {
            const int c = nvec[3 * (size_t)v + a];
            if (c > MW_SK_MAX_COMPONENT || c < -MW_SK_MAX_COMPONENT)
                return fail("%s: nvec: component %d of vector %d is %d, beyond %d", who, a, v, c, MW_SK_MAX_COMPONENT);
            const int m = c < 0 ? -c : c;
            if (m > nmax[a]) nmax[a] = m;
        }
    return 0;
}

int check_cells(const char* who, int nboxes, const double* cells, std::vector<double>& inv)
{
    inv.resize(9 * (size_t)nboxes);
    for (int b = 0; b < nboxes; ++b) {
        double det;
        if (!invert_cell(cells + 9 * (size_t)b, inv.data() + 9 * (size_t)b, &det))
            return fail("%s: cells: the determinant of box %d is %g (zero or not finite)", who, b, det);
    }
    return 0;
}

int check_live(const char* who) { return check_live(who, "mw_sk_init", g); }

// The work of every entry, arguments already checked.  `inv` is on the host; pos, nvec and the outputs are device pointers
// when `dev`, host pointers otherwise.  `keepS`: leave S of all boxes in g.Sall (for the mean) and copy nothing out.
int run(const char* who, int nboxes, int n, int M, const std::vector<double>& inv, const double* pos, const int* nvec,
        const int nmax[3], bool dev, double* rho, double* S, bool keepS)
{
    Plan p;
    if (make_plan(who, n, nmax, M, nboxes, g.budget, p)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (reserve(g.scratch, p.per_box * (size_t)p.bpc)) return 1;
    if (reserve(g.inv, inv.size() * sizeof(double))) return 1;
    HIPOK(hipMemcpyAsync(g.inv.p, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
    const int* d_nvec = nvec;
    if (!dev) {
        if (reserve(g.nvec, 12 * (size_t)M)) return 1;
        HIPOK(hipMemcpyAsync(g.nvec.p, nvec, 12 * (size_t)M, hipMemcpyHostToDevice, g.stream));
        d_nvec = (const int*)g.nvec.p;
        if (reserve(g.pos, 24 * (size_t)n * p.bpc)) return 1;
        if (rho && reserve(g.rho, 16 * (size_t)M * p.bpc)) return 1;
        if (S && !keepS && reserve(g.S, 8 * (size_t)M * p.bpc)) return 1;
    }
    if (keepS && reserve(g.Sall, 8 * (size_t)M * nboxes)) return 1;
    double2* T = (double2*)g.scratch.p;
    double2* part = T + (p.small ? 0 : (size_t)n * p.rows * p.bpc);
    float ms_ph = 0.0f, ms_sum = 0.0f;
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const double* d_pos = pos + 3 * (size_t)n * b0;
        if (!dev) {
            HIPOK(hipMemcpyAsync(g.pos.p, d_pos, 24 * (size_t)n * nb, hipMemcpyHostToDevice, g.stream));
            d_pos = (const double*)g.pos.p;
        }
        const double* d_inv = (const double*)g.inv.p + 9 * (size_t)b0;
        double* d_rho = !rho ? nullptr : dev ? rho + 2 * (size_t)M * b0 : (double*)g.rho.p;
        double* d_S = keepS ? (double*)g.Sall.p + (size_t)M * b0 : !S ? nullptr : dev ? S + (size_t)M * b0 : (double*)g.S.p;
        HIPOK(hipEventRecord(g.ev[0], g.stream));
        if (!p.small) {
            const long long lanes = (long long)nb * n;
            hipLaunchKernelGGL(k_sk_phasors, dim3((unsigned)((lanes + kThreads - 1) / kThreads)), dim3(kThreads), 0, g.stream,
                               nb, n, nmax[0], nmax[1], nmax[2], d_inv, d_pos, T);
            HIPOK(hipGetLastError());
        }
        HIPOK(hipEventRecord(g.ev[1], g.stream));
        const dim3 grid((unsigned)((M + kVecPerWg - 1) / kVecPerWg), (unsigned)p.nseg, (unsigned)nb);
        if (p.small)
            hipLaunchKernelGGL(k_sk_sum<true>, grid, dim3(kThreads), p.lds, g.stream, n, M, nmax[0], nmax[1], nmax[2], p.jtlog, p.stride, p.seglen,
                               d_nvec, (const double2*)nullptr, d_inv, d_pos, part);
        else
            hipLaunchKernelGGL(k_sk_sum<false>, grid, dim3(kThreads), p.lds, g.stream, n, M, nmax[0], nmax[1], nmax[2], p.jtlog, p.stride, p.seglen,
                               d_nvec, (const double2*)T, d_inv, d_pos, part);
        HIPOK(hipGetLastError());
        const long long outs = (long long)nb * M;
        hipLaunchKernelGGL(k_sk_finish, dim3((unsigned)((outs + kThreads - 1) / kThreads)), dim3(kThreads), 0, g.stream,
                           nb, n, M, p.nseg, (const double2*)part, d_rho, d_S);
        HIPOK(hipGetLastError());
        HIPOK(hipEventRecord(g.ev[2], g.stream));
        if (!dev) {
            if (rho) HIPOK(hipMemcpyAsync(rho + 2 * (size_t)M * b0, g.rho.p, 16 * (size_t)M * nb, hipMemcpyDeviceToHost, g.stream));
            if (S && !keepS) HIPOK(hipMemcpyAsync(S + (size_t)M * b0, g.S.p, 8 * (size_t)M * nb, hipMemcpyDeviceToHost, g.stream));
        }
        HIPOK(hipStreamSynchronize(g.stream));               // the next chunk reuses the scratch and the staging buffers
        float a = 0.0f, s = 0.0f;
        HIPOK(hipEventElapsedTime(&a, g.ev[0], g.ev[1]));
        HIPOK(hipEventElapsedTime(&s, g.ev[1], g.ev[2]));
        ms_ph += p.small ? 0.0f : a;
        ms_sum += s;
    }
    plan_fields(p, g.last);
    g.have_last = true;
    g.ms_phasors = ms_ph;
    g.ms_sums = ms_sum;
    return 0;
}

int check_common(const char* who, int nboxes, int n, const double* cells, const double* pos, int M, const int* nvec)
{
    if (check_sizes(who, nboxes, n, M)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (!nvec) return fail("%s: nvec is NULL", who);
    return 0;
}

}  // namespace

extern "C" {

const char* mw_sk_last_error(void) { return g_err; }
int mw_sk_is_initialised(void) { return g.live ? 1 : 0; }

int mw_sk_init(int device) { return runtime_init("mw_sk_init", "MW_SK_SCRATCH_MB", device, g); }

int mw_sk_finalize(void)
{
    if (runtime_finalize(g, {&g.scratch, &g.inv, &g.pos, &g.nvec, &g.rho, &g.S, &g.Sall, &g.mean})) return 1;
    g = State{};
    return 0;
}

int mw_sk_compute(int nboxes, int nwater, const double* cells, const double* pos, int M, const int* nvec, double* rho, double* S)
{
    const char* who = "mw_sk_compute";
    int nmax[3];
    std::vector<double> inv;
    if (check_common(who, nboxes, nwater, cells, pos, M, nvec)) return 1;
    if (check_nvec(who, M, nvec, nmax)) return 1;
    if (check_cells(who, nboxes, cells, inv)) return 1;
    if (check_live(who)) return 1;
    return run(who, nboxes, nwater, M, inv, pos, nvec, nmax, false, rho, S, false);
}

int mw_sk_compute_device(int nboxes, int nwater, const double* cells, const double* pos, int M, const int* nvec, double* rho, double* S)
{
    const char* who = "mw_sk_compute_device";
    int nmax[3];
    std::vector<double> inv;
    if (check_common(who, nboxes, nwater, cells, pos, M, nvec)) return 1;
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    HIPOK(hipDeviceSynchronize());                            // whoever made the inputs (another stream, PyTorch's) is done
    std::vector<double> h_cells(9 * (size_t)nboxes);
    std::vector<int> h_nvec(3 * (size_t)M);
    HIPOK(hipMemcpy(h_cells.data(), cells, h_cells.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(h_nvec.data(), nvec, h_nvec.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (check_nvec(who, M, h_nvec.data(), nmax)) return 1;
    if (check_cells(who, nboxes, h_cells.data(), inv)) return 1;
    return run(who, nboxes, nwater, M, inv, pos, nvec, nmax, true, rho, S, false);
}

int mw_sk_mean(int nboxes, int nwater, const double* cells, const double* pos, int M, const int* nvec, int ngroups, double* S_mean)
{
    const char* who = "mw_sk_mean";
    int nmax[3];
    std::vector<double> inv;
    if (check_common(who, nboxes, nwater, cells, pos, M, nvec)) return 1;
    if (ngroups < 1 || nboxes % ngroups != 0) return fail("%s: ngroups = %d does not divide nboxes = %d", who, ngroups, nboxes);
    if (!S_mean) return fail("%s: S_mean is NULL", who);
    if (check_nvec(who, M, nvec, nmax)) return 1;
    if (check_cells(who, nboxes, cells, inv)) return 1;
    if (check_live(who)) return 1;
    DeviceScope scope;                                        // over run() and the mean pass after it
    HIPOK(scope.enter(g.device));
    if (run(who, nboxes, nwater, M, inv, pos, nvec, nmax, false, nullptr, nullptr, true)) return 1;
    const size_t bytes = 8 * (size_t)M * ngroups;
    if (reserve(g.mean, bytes)) return 1;
    const long long outs = (long long)ngroups * M;
    hipLaunchKernelGGL(k_sk_mean, dim3((unsigned)((outs + kThreads - 1) / kThreads)), dim3(kThreads), 0, g.stream,
                       ngroups, nboxes / ngroups, M, (const double*)g.Sall.p, (double*)g.mean.p);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(S_mean, g.mean.p, bytes, hipMemcpyDeviceToHost, g.stream));
    HIPOK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_sk_plan(int nwater, const int nmax[3], int M, int nboxes, int* out, int nout)
{
    const char* who = "mw_sk_plan";
    if (check_sizes(who, nboxes, nwater, M)) return 1;
    if (!nmax) return fail("%s: nmax is NULL", who);
    for (int a = 0; a < 3; ++a)
        if (nmax[a] < 0 || nmax[a] > MW_SK_MAX_COMPONENT) return fail("%s: nmax[%d] = %d outside 0..%d", who, a, nmax[a], MW_SK_MAX_COMPONENT);
    if (!out || nout < 1) return fail("%s: out is NULL or nout < 1", who);
    Plan p;
    if (make_plan(who, nwater, nmax, M, nboxes, g.live ? g.budget : kDefaultBudget, p)) return 1;
    int f[MW_SK_PLAN_FIELDS];
    plan_fields(p, f);
    copy_fields(f, MW_SK_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_sk_last(int* out, int nout)
{
    if (check_live("mw_sk_last")) return 1;
    if (!out || nout < 1) return fail("mw_sk_last: out is NULL or nout < 1");
    if (!g.have_last) return fail("mw_sk_last: no call has launched yet");
    copy_fields(g.last, MW_SK_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_sk_elapsed_ms(float* phasors, float* sums)
{
    if (check_live("mw_sk_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_sk_elapsed_ms: no call has launched yet");
    if (phasors) *phasors = g.ms_phasors;
    if (sums) *sums = g.ms_sums;
    return 0;
}

}  // extern "C"
