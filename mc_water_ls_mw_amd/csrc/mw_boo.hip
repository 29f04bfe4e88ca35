// libmw_boo.so -- the Steinhardt bond-order parameters of include/mw_boo.h: q4, q6, their neighbour averages, the solid-like
// connection count of every molecule and the box summary (Q4, Q6, <qbar4>, <qbar6>), for many boxes.  General geometry
// (nwater > 64): a counting sort into a fractional cell grid (the sort of mw_lib_cells.h), then one
// lane per molecule in sorted order walks the 27 neighbouring cells twice -- k_boo_pass1 for n_i and the 22 harmonic sums,
// k_boo_pass2 for the neighbours' vectors -- and k_boo_summary adds the box up.  Small geometry (nwater <= 64): k_boo_small,
// one wavefront per box with the box in LDS.  Every bit of a box's results depends on the box, rc and the threshold alone
// (mw_boo.h): the arithmetic below is spelled out in fma / mul / add with contraction off, and the order of every sum is fixed.
// The grid rules, the sort and the two walks are mw_lib_cells.h's, shared with the other libraries that sort into a cell grid.
#include "../../include/mw_boo.h"

#include "mw_common.hip.h"

#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too
#include "mw_lib_cells.h"
#include "mw_lib_harmonics.h"                  // the 22 real harmonics, unit_harmonics and norm_of, shared with libmw_nuc.so

namespace mwboo {

using namespace mwcells;
using namespace mwharm;

constexpr int kSmallBoxesPerWg = kThreads / 64;   // one wavefront per box
constexpr int kRec = 24;                          // doubles per molecule in scratch: q_lm, |q_6|, n_i
constexpr int kSums = 25;                         // box sums: 22 of n_i q_lm, sum n_i, sum qbar4, sum qbar6
constexpr int kSmallLds = kSmallBoxesPerWg * (3 + kRec) * 64 * 8;

// ---- general geometry ----------------------------------------------------------------------------------------------------
// Per box in scratch after the sort's pieces (mw_lib_cells.h), in cell order: rec [n][kRec], qbar [n][2].

// Pass 1, one lane per molecule in sorted order: n_i and q_lm(i) into rec.
__global__ __launch_bounds__(kThreads) void k_boo_pass1(int n, int cap, double rc2, const double* __restrict__ par, const int* __restrict__ grid,
                                                        const int* __restrict__ start, const double* __restrict__ ss, double* __restrict__ rec)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    double acc[kNY];
#pragma unroll
    for (int k = 0; k < kNY; ++k) acc[k] = 0.0;
    int cnt = 0;
    const double* S = ss + 3 * (size_t)b * n;
    walk_cells(S[3 * (size_t)p], S[3 * (size_t)p + 1], S[3 * (size_t)p + 2], rc2, par + 18 * (size_t)b, grid + 4 * (size_t)b,
               start + (size_t)b * (cap + 1), S,
               [&](int, int, int, int, double r2, double dx, double dy, double dz) {
                   double Y[kNY];
                   unit_harmonics(r2, dx, dy, dz, Y);
#pragma unroll
                   for (int k = 0; k < kNY; ++k) acc[k] = acc[k] + Y[k];
                   ++cnt;
               });
    double* r = rec + kRec * ((size_t)b * n + p);
    const double m = (double)cnt;
#pragma unroll
    for (int k = 0; k < kNY; ++k) acc[k] = cnt ? acc[k] / m : 0.0;
    const double n6 = norm_of(acc, 9, 13);
#pragma unroll
    for (int k = 0; k < kNY; ++k) r[k] = acc[k];
    r[22] = n6;
    r[23] = m;
}

// Pass 2, the same walk: the neighbours' vectors for qbar and the connections; the outputs by molecule index.
__global__ __launch_bounds__(kThreads) void k_boo_pass2(int n, int cap, double rc2, double thr, const double* __restrict__ par,
                                                        const int* __restrict__ grid, const int* __restrict__ start, const double* __restrict__ ss,
                                                        const int* __restrict__ idx, const double* __restrict__ rec, double* __restrict__ qbar,
                                                        double* __restrict__ q, int* __restrict__ nn)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const double* R = rec + kRec * (size_t)b * n;
    double own[kRec], bar[kNY];
#pragma unroll
    for (int k = 0; k < kRec; ++k) own[k] = R[kRec * (size_t)p + k];
#pragma unroll
    for (int k = 0; k < kNY; ++k) bar[k] = own[k];
    int conn = 0;
    const double* S = ss + 3 * (size_t)b * n;
    walk_cells(S[3 * (size_t)p], S[3 * (size_t)p + 1], S[3 * (size_t)p + 2], rc2, par + 18 * (size_t)b, grid + 4 * (size_t)b,
               start + (size_t)b * (cap + 1), S,
               [&](int j, int, int, int, double, double, double, double) {
                   const double* rj = R + kRec * (size_t)j;
                   double dot = 0.0;
#pragma unroll
                   for (int k = 0; k < kNY; ++k) {
                       const double v = rj[k];
                       bar[k] = bar[k] + v;
                       if (k >= 9) dot = __builtin_fma(own[k], v, dot);
                   }
                   const double den = own[22] * rj[22];
                   if (den > 0.0 && dot / den > thr) ++conn;
               });
    const double m = own[23] + 1.0;
#pragma unroll
    for (int k = 0; k < kNY; ++k) bar[k] = bar[k] / m;
    const double b4 = norm_of(bar, 0, 9), b6 = norm_of(bar, 9, 13);
    const size_t o = (size_t)b * n;
    qbar[2 * (o + p)] = b4; qbar[2 * (o + p) + 1] = b6;
    const size_t i = o + idx[o + p];
    if (q) { q[4 * i] = norm_of(own, 0, 9); q[4 * i + 1] = own[22]; q[4 * i + 2] = b4; q[4 * i + 3] = b6; }
    if (nn) { nn[2 * i] = (int)own[23]; nn[2 * i + 1] = conn; }
}

// (Q4, Q6, <qbar4>, <qbar6>) from the box sums t[kSums]
__device__ __forceinline__ void write_summary(const double* t, int n, double* out)
{
    double Q[kNY];
    for (int k = 0; k < kNY; ++k) Q[k] = t[22] > 0.0 ? t[k] / t[22] : 0.0;
    out[0] = norm_of(Q, 0, 9); out[1] = norm_of(Q, 9, 13);
    out[2] = t[23] / (double)n; out[3] = t[24] / (double)n;
}

// One workgroup per box: lane t adds the sorted places t, t + 256, ... in that order, a fixed tree adds the lanes of a
// wavefront and thread 0 the four wavefronts in order.
__global__ __launch_bounds__(kThreads) void k_boo_summary(int n, const double* __restrict__ rec, const double* __restrict__ qbar, double* __restrict__ summary)
{
    __shared__ double part[kThreads / 64][kSums];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* R = rec + kRec * (size_t)b * n;
    const double* B = qbar + 2 * (size_t)b * n;
    double t[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) t[k] = 0.0;
    for (int p = tid; p < n; p += kThreads) {
        const double* r = R + kRec * (size_t)p;
        const double m = r[23];
#pragma unroll
        for (int k = 0; k < kNY; ++k) t[k] = t[k] + m * r[k];
        t[22] = t[22] + m;
        t[23] = t[23] + B[2 * (size_t)p];
        t[24] = t[24] + B[2 * (size_t)p + 1];
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
        const double w = mw::wave_sum(t[k]);
        if ((tid & 63) == 0) part[tid >> 6][k] = w;
    }
    __syncthreads();
    if (tid == 0) {
        double tot[kSums];
        for (int k = 0; k < kSums; ++k) {
            double a = part[0][k];
            for (int w = 1; w < kThreads / 64; ++w) a = a + part[w][k];
            tot[k] = a;
        }
        write_summary(tot, n, summary + 4 * (size_t)b);
    }
}

// ---- small geometry: one wavefront per box, lane i = molecule i, the box's fractional positions and records in LDS ---------
__global__ __launch_bounds__(kThreads) void k_boo_small(int nb, int n, double rc2, double thr, const double* __restrict__ par,
                                                        const double* __restrict__ pos, double* __restrict__ q, int* __restrict__ nn,
                                                        double* __restrict__ summary)
{
    __shared__ double lds[kSmallBoxesPerWg][(3 + kRec) * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * kSmallBoxesPerWg + wave;
    if (b >= nb) return;                                   // the whole wavefront; no workgroup barrier below
    double* S = lds[wave];
    double* R = S + 3 * 64;                                // R[k * 64 + j]
    const double* H = par + 18 * (size_t)b;
    const bool active = lane < n;
    const size_t m = (size_t)b * n + (active ? lane : 0);
    const double s0 = frac_coord(H + 9, 0, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s1 = frac_coord(H + 9, 1, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s2 = frac_coord(H + 9, 2, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    S[lane] = s0; S[64 + lane] = s1; S[128 + lane] = s2;
    mw::wave_fence();

    double own[kRec];
#pragma unroll
    for (int k = 0; k < kNY; ++k) own[k] = 0.0;
    int cnt = 0;
    walk_small(n, active, rc2, H, S, s0, s1, s2, [&](int, int, double r2, double dx, double dy, double dz) {
        double Y[kNY];
        unit_harmonics(r2, dx, dy, dz, Y);
#pragma unroll
        for (int k = 0; k < kNY; ++k) own[k] = own[k] + Y[k];
        ++cnt;
    });
    const double mi = (double)cnt;
#pragma unroll
    for (int k = 0; k < kNY; ++k) own[k] = cnt ? own[k] / mi : 0.0;
    own[22] = norm_of(own, 9, 13);
    own[23] = mi;
#pragma unroll
    for (int k = 0; k < kRec; ++k) R[k * 64 + lane] = own[k];
    mw::wave_fence();

    double bar[kNY];
#pragma unroll
    for (int k = 0; k < kNY; ++k) bar[k] = own[k];
    int conn = 0;
    walk_small(n, active, rc2, H, S, s0, s1, s2, [&](int j, int, double, double, double, double) {
        double dot = 0.0;
#pragma unroll
        for (int k = 0; k < kNY; ++k) {
            const double v = R[k * 64 + j];
            bar[k] = bar[k] + v;
            if (k >= 9) dot = __builtin_fma(own[k], v, dot);
        }
        const double den = own[22] * R[22 * 64 + j];
        if (den > 0.0 && dot / den > thr) ++conn;
    });
    const double m1 = mi + 1.0;
#pragma unroll
    for (int k = 0; k < kNY; ++k) bar[k] = bar[k] / m1;
    const double b4 = norm_of(bar, 0, 9), b6 = norm_of(bar, 9, 13);
    if (active) {
        if (q) { q[4 * m] = norm_of(own, 0, 9); q[4 * m + 1] = own[22]; q[4 * m + 2] = b4; q[4 * m + 3] = b6; }
        if (nn) { nn[2 * m] = cnt; nn[2 * m + 1] = conn; }
    }
    if (summary) {                                         // wave-uniform: lanes beyond n add +0.0
        double t[kSums];
#pragma unroll
        for (int k = 0; k < kNY; ++k) t[k] = mw::wave_sum(active ? mi * own[k] : 0.0);
        t[22] = mw::wave_sum(active ? mi : 0.0);
        t[23] = mw::wave_sum(active ? b4 : 0.0);
        t[24] = mw::wave_sum(active ? b6 : 0.0);
        if (lane == 0) write_summary(t, n, summary + 4 * (size_t)b);
    }
}

}  // namespace mwboo

namespace {

using namespace mwboo;

struct State : Runtime<5> {
    Buf scratch, par, grid, pos, q, nn, summary;
    int last[MW_BOO_PLAN_FIELDS] = {0};
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
} g;

// The scratch of one box of the general geometry: the sort's pieces, then rec and qbar.
struct Layout : SortLayout {
    size_t rec, qbar, per_box;
};

Layout make_layout(int n)
{
    Layout l;
    size_t o = 0;
    lay_sort(l, n, o);
    l.rec = o;   o += align16(8 * (size_t)kRec * n);
    l.qbar = o;  o += align16(16 * (size_t)n);
    l.per_box = o;
    return l;
}

struct Plan : PlanBase {
    Layout lay;
};

int make_plan(const char* who, int n, int nboxes, size_t budget, Plan& p)
{
    p.small = n <= kSmallN;
    p.lay = make_layout(n);
    if (p.small) {
        p.per_box = 0; p.lds = kSmallLds; p.boxes_per_wg = kSmallBoxesPerWg;
        p.bpc = nboxes < kSmallChunkBoxes ? nboxes : kSmallChunkBoxes;
    } else {
        p.per_box = p.lay.per_box; p.lds = (int)sizeof(double) * (kThreads / 64) * kSums; p.boxes_per_wg = 0;
        const size_t fit = budget / p.per_box;
        if (fit < 1)
            return fail("%s: one box needs %zu bytes of scratch (nwater = %d) and does not fit the budget of %zu bytes (MW_BOO_SCRATCH_MB)",
                        who, p.per_box, n, budget);
        p.bpc = (int)(fit < (size_t)kMaxChunkBoxes ? fit : (size_t)kMaxChunkBoxes);
        if (p.bpc > nboxes) p.bpc = nboxes;
    }
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

int check_scalars(const char* who, int nboxes, int n, double rc, double threshold)
{
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    if (!(rc > 0.0) || !std::isfinite(rc)) return fail("%s: rc = %g bohr is not a finite cutoff > 0 (box 0)", who, rc);
    if (!(threshold >= -1.0 && threshold <= 1.0)) return fail("%s: threshold = %g outside [-1, 1]", who, threshold);
    return 0;
}

const char kRadius[] = "rc";                  // the radius the cells are checked against, in the messages

int check_live(const char* who) { return check_live(who, "mw_boo_init", g); }

// The work of both entries, arguments already checked.  par and grid are on the host; pos and the outputs are device pointers
// when `dev`, host pointers otherwise.
int run(const char* who, int nboxes, int n, const std::vector<double>& par, const std::vector<int>& grid, const double* pos, double rc,
        double thr, bool dev, double* q, int* nn, double* summary)
{
    Plan p;
    if (make_plan(who, n, nboxes, g.budget, p)) return 1;
    const Layout& l = p.lay;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (!p.small && reserve(g.scratch, p.per_box * (size_t)p.bpc)) return 1;
    if (reserve(g.par, par.size() * sizeof(double))) return 1;
    if (reserve(g.grid, grid.size() * sizeof(int))) return 1;
    HIPOK(hipMemcpyAsync(g.par.p, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPOK(hipMemcpyAsync(g.grid.p, grid.data(), grid.size() * sizeof(int), hipMemcpyHostToDevice, g.stream));
    if (!dev) {
        if (reserve(g.pos, 24 * (size_t)n * p.bpc)) return 1;
        if (q && reserve(g.q, 32 * (size_t)n * p.bpc)) return 1;
        if (nn && reserve(g.nn, 8 * (size_t)n * p.bpc)) return 1;
        if (summary && reserve(g.summary, 32 * (size_t)p.bpc)) return 1;
    }
    if (!p.small && !summary && reserve(g.summary, 32 * (size_t)p.bpc)) return 1;          // the summary pass always runs
    const double rc2 = rc * rc;
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const double* d_pos = pos + 3 * (size_t)n * b0;
        if (!dev) {
            HIPOK(hipMemcpyAsync(g.pos.p, d_pos, 24 * (size_t)n * nb, hipMemcpyHostToDevice, g.stream));
            d_pos = (const double*)g.pos.p;
        }
        const double* d_par = (const double*)g.par.p + 18 * (size_t)b0;
        const int* d_grid = (const int*)g.grid.p + 4 * (size_t)b0;
        double* d_q = !q ? nullptr : dev ? q + 4 * (size_t)n * b0 : (double*)g.q.p;
        int* d_nn = !nn ? nullptr : dev ? nn + 2 * (size_t)n * b0 : (int*)g.nn.p;
        double* d_sum = !summary ? nullptr : dev ? summary + 4 * (size_t)b0 : (double*)g.summary.p;
        if (p.small) {
            HIPOK(hipEventRecord(g.ev[0], g.stream));
            hipLaunchKernelGGL(k_boo_small, dim3((unsigned)((nb + kSmallBoxesPerWg - 1) / kSmallBoxesPerWg)), dim3(kThreads), 0, g.stream,
                               nb, n, rc2, thr, d_par, d_pos, d_q, d_nn, d_sum);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[1], g.stream));
        } else {
            if (!d_sum) d_sum = (double*)g.summary.p;
            char* base = (char*)g.scratch.p;
            const size_t B = (size_t)p.bpc;
            double* rec = (double*)(base + l.rec * B);
            double* qbar = (double*)(base + l.qbar * B);
            const dim3 grid_m = per_molecule(n, nb);
            Sorted s;
            HIPOK(hipEventRecord(g.ev[0], g.stream));
            if (sort_into_cells(g.stream, n, nb, l, base, B, d_par, d_grid, d_pos, s)) return 1;
            HIPOK(hipEventRecord(g.ev[1], g.stream));
            hipLaunchKernelGGL(k_boo_pass1, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, rc2, d_par, d_grid, s.start, s.ss, rec);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[2], g.stream));
            hipLaunchKernelGGL(k_boo_pass2, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, rc2, thr, d_par, d_grid, s.start, s.ss, s.idx,
                               (const double*)rec, qbar, d_q, d_nn);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[3], g.stream));
            hipLaunchKernelGGL(k_boo_summary, dim3((unsigned)nb), dim3(kThreads), 0, g.stream, n, (const double*)rec, (const double*)qbar, d_sum);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[4], g.stream));
        }
        if (!dev) {
            if (q) HIPOK(hipMemcpyAsync(q + 4 * (size_t)n * b0, g.q.p, 32 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (nn) HIPOK(hipMemcpyAsync(nn + 2 * (size_t)n * b0, g.nn.p, 8 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (summary) HIPOK(hipMemcpyAsync(summary + 4 * (size_t)b0, g.summary.p, 32 * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
        }
        HIPOK(hipStreamSynchronize(g.stream));               // the next chunk reuses the scratch and the staging buffers
        if (p.small) {
            float t = 0.0f;
            HIPOK(hipEventElapsedTime(&t, g.ev[0], g.ev[1]));
            ms[1] += t;
        } else {
            for (int k = 0; k < 4; ++k) {
                float t = 0.0f;
                HIPOK(hipEventElapsedTime(&t, g.ev[k], g.ev[k + 1]));
                ms[k] += t;
            }
        }
    }
    plan_fields(p, grid.data(), g.last);
    g.have_last = true;
    for (int k = 0; k < 4; ++k) g.ms[k] = ms[k];
    return 0;
}

}  // namespace

extern "C" {

const char* mw_boo_last_error(void) { return g_err; }
int mw_boo_is_initialised(void) { return g.live ? 1 : 0; }

int mw_boo_init(int device) { return runtime_init("mw_boo_init", "MW_BOO_SCRATCH_MB", device, g); }

int mw_boo_finalize(void)
{
    if (runtime_finalize(g, {&g.scratch, &g.par, &g.grid, &g.pos, &g.q, &g.nn, &g.summary})) return 1;
    g = State{};
    return 0;
}

int mw_boo_compute(int nboxes, int nwater, const double* cells, const double* pos, double rc, double threshold, double* q, int* nn,
                   double* summary)
{
    const char* who = "mw_boo_compute";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, rc, threshold)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (check_cells(who, kRadius, nboxes, nwater, cells, rc, par, grid)) return 1;
    if (check_live(who)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, rc, threshold, false, q, nn, summary);
}

int mw_boo_compute_device(int nboxes, int nwater, const double* cells, const double* pos, double rc, double threshold, double* q, int* nn,
                          double* summary)
{
    const char* who = "mw_boo_compute_device";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, rc, threshold)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (fetch_cells(who, kRadius, nboxes, nwater, cells, rc, par, grid)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, rc, threshold, true, q, nn, summary);
}

int mw_boo_plan(int nwater, const double* cell, double rc, int nboxes, int* out, int nout)
{
    const char* who = "mw_boo_plan";
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, rc, 0.0)) return 1;
    if (plan_grid(who, kRadius, nwater, cell, rc, out, nout, grid)) return 1;
    Plan p;
    if (make_plan(who, nwater, nboxes, g.live ? g.budget : kDefaultBudget, p)) return 1;
    int f[MW_BOO_PLAN_FIELDS];
    plan_fields(p, grid.data(), f);
    copy_fields(f, MW_BOO_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_boo_last(int* out, int nout) { return last_fields("mw_boo_last", "mw_boo_init", g, g.last, MW_BOO_PLAN_FIELDS, out, nout); }

int mw_boo_elapsed_ms(float* binning, float* pass1, float* pass2, float* summary)
{
    if (check_live("mw_boo_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_boo_elapsed_ms: no call has launched yet");
    if (binning) *binning = g.ms[0];
    if (pass1) *pass1 = g.ms[1];
    if (pass2) *pass2 = g.ms[2];
    if (summary) *summary = g.ms[3];
    return 0;
}

}  // extern "C"
