// libmw_tet.so -- the nearest-neighbour order parameters of include/mw_tet.h: the tetrahedral order q, its translational
// companion s_k, the fifth-neighbour distance d5 and the local structure index of every molecule, the four nearest
// neighbours and the box means, for many boxes.  General geometry (nwater > 64): a counting sort into a fractional cell grid
// (the sort of mw_lib_cells.h), then k_tet_select, one lane per molecule in sorted order, walks the 27
// neighbouring cells and keeps the 16 nearest entries sorted in registers, and k_tet_summary adds the box up.  Small geometry
// (nwater <= 64): k_tet_small, one wavefront per box with the box in LDS.  Every bit of a box's results depends on the box and
// the two radii alone (mw_tet.h): the arithmetic below is spelled out in fma / mul / add with contraction off, and the order
// of every sum and of every ranking is fixed.  The grid rules, the sort and the two walks are mw_lib_cells.h's, shared with
// libmw_boo.so and the other libraries that sort into a cell grid.
#include "../../include/mw_tet.h"

#include "mw_common.hip.h"

#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too
#include "mw_lib_cells.h"

namespace mwtet {

using namespace mwcells;

constexpr int kSmallBoxesPerWg = kThreads / 64;   // one wavefront per box
constexpr int kKeep = MW_TET_KEEP;
constexpr int kOrd = 4;                           // doubles per molecule in scratch: q, s_k, d5, lsi
constexpr int kSums = 8;                          // box sums: the four values over the molecules where defined, and how many
constexpr int kSmallLds = kSmallBoxesPerWg * 3 * 64 * 8;
constexpr int kPlaceBits = 22;                    // an entry: the place (or index) of j in the low bits, its image above
constexpr int kPlaceMask = (1 << kPlaceBits) - 1;
static_assert(kMaxWater <= (1 << kPlaceBits), "an entry holds a molecule in kPlaceBits bits");

__device__ __forceinline__ double undefined() { return __longlong_as_double(0x7ff8000000000000LL); }

// ---- the 16 nearest, sorted in registers ---------------------------------------------------------------------------------
// k[a] / e[a]: r^2 and the entry of rank a + 1, +inf / -1 where there is none yet.  Every index below is a compile-time
// constant after unrolling, so both arrays live in registers.
struct Nearest {
    double k[kKeep];
    int e[kKeep];
    int n_search = 0, n_lsi = 0;
    __device__ __forceinline__ Nearest()
    {
#pragma unroll
        for (int a = 0; a < kKeep; ++a) { k[a] = __builtin_inf(); e[a] = -1; }
    }
    // An entry within r_search.  It goes in front of the first kept one with a larger r^2 -- behind its equals, which came
    // earlier in the walk -- and the chain is entered only when it beats the current 16th.
    __device__ __forceinline__ void add(double r2, double rl2, int entry)
    {
        ++n_search;
        if (r2 < rl2) ++n_lsi;
        if (!(r2 < k[kKeep - 1])) return;
#pragma unroll
        for (int a = kKeep - 1; a >= 1; --a) {
            const bool above = r2 < k[a - 1], here = r2 < k[a];
            k[a] = above ? k[a - 1] : here ? r2 : k[a];
            e[a] = above ? e[a - 1] : here ? entry : e[a];
        }
        const bool first = r2 < k[0];
        k[0] = first ? r2 : k[0];
        e[0] = first ? entry : e[0];
    }
};

// (q, s_k, d5, lsi) from the ranked r^2 and the vectors d[a] of ranks 1..4 (read only where the rank exists)
__device__ __forceinline__ void order_values(const Nearest& t, const double (&d)[4][3], double (&o)[kOrd])
{
    double r[kKeep];
#pragma unroll
    for (int a = 0; a < kKeep; ++a) r[a] = __builtin_sqrt(t.k[a]);
    o[0] = o[1] = o[2] = o[3] = undefined();
    if (t.n_search >= 4) {
        double u[4][3];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double rinv = 1.0 / r[a];
            u[a][0] = d[a][0] * rinv; u[a][1] = d[a][1] * rinv; u[a][2] = d[a][2] * rinv;
        }
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a + 1; b < 4; ++b) {
                const double c = __builtin_fma(u[a][0], u[b][0], __builtin_fma(u[a][1], u[b][1], u[a][2] * u[b][2]));
                const double v = c + 1.0 / 3.0;
                acc = __builtin_fma(v, v, acc);
            }
        o[0] = __builtin_fma(-0.375, acc, 1.0);
        const double rbar = 0.25 * (((r[0] + r[1]) + r[2]) + r[3]);
        double dev = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double v = r[a] - rbar;
            dev = __builtin_fma(v, v, dev);
        }
        o[1] = 1.0 - dev / (12.0 * (rbar * rbar));
    }
    if (t.n_search >= 5) o[2] = r[4];
    const int kept = t.n_search < kKeep ? t.n_search : kKeep, n = t.n_lsi;
    if (n >= 1 && n + 1 <= kept) {
        const double m = (double)n;
        double sum = 0.0;
#pragma unroll
        for (int a = 0; a + 1 < kKeep; ++a)
            if (a < n) sum = sum + (r[a + 1] - r[a]);
        const double mean = sum / m;
        double var = 0.0;
#pragma unroll
        for (int a = 0; a + 1 < kKeep; ++a)
            if (a < n) {
                const double v = (r[a + 1] - r[a]) - mean;
                var = __builtin_fma(v, v, var);
            }
        o[3] = var / m;
    }
}

// the means over the molecules where each value is defined, and their numbers, from the box sums t[kSums]
__device__ __forceinline__ void write_summary(const double* t, double* out)
{
    for (int k = 0; k < 4; ++k) {
        out[k] = t[4 + k] > 0.0 ? t[k] / t[4 + k] : undefined();
        out[4 + k] = t[4 + k];
    }
}

// ---- general geometry ----------------------------------------------------------------------------------------------------
// Per box in scratch after the sort's pieces (mw_lib_cells.h): ord [n][kOrd] in cell order.

// The selection pass, one lane per molecule in sorted order: the walk of the 27 cells in the contract's order, every entry
// within r_search offered to the lane's Nearest; then the values of the molecule.  An entry is the sorted place of j with the
// image shift (-1, 0, 1 per axis, base 3) above it, enough to form d again for the four that end up nearest.
__global__ __launch_bounds__(kThreads) void k_tet_select(int n, int cap, double rs2, double rl2, const double* __restrict__ par,
                                                         const int* __restrict__ grid, const int* __restrict__ start, const double* __restrict__ ss,
                                                         const int* __restrict__ idx, double* __restrict__ ord, double* __restrict__ order,
                                                         int* __restrict__ near_, int* __restrict__ counts)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const double* H = par + 18 * (size_t)b;
    const size_t o = (size_t)b * n;
    const double* S = ss + 3 * o;
    const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
    Nearest t;
    walk_cells(s0, s1, s2, rs2, H, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), S,
               [&](int q, int hx, int hy, int hz, double r2, double, double, double) {
                   t.add(r2, rl2, ((((hz + 1) * 3 + (hy + 1)) * 3 + (hx + 1)) << kPlaceBits) | q);
               });
    double d[4][3];
    int who[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        d[a][0] = d[a][1] = d[a][2] = 0.0;
        who[a] = -1;
        if (a < t.n_search) {                                  // (an entry is a place only where the rank exists)
            const int q = t.e[a] & kPlaceMask, image = t.e[a] >> kPlaceBits;
            const double fx = (double)(image % 3 - 1), fy = (double)(image / 3 % 3 - 1), fz = (double)(image / 9 - 1);
            (void)bond_vector(H, (S[3 * (size_t)q] - s0) + fx, (S[3 * (size_t)q + 1] - s1) + fy, (S[3 * (size_t)q + 2] - s2) + fz,
                              d[a][0], d[a][1], d[a][2]);
            who[a] = idx[o + q];
        }
    }
    double v[kOrd];
    order_values(t, d, v);
    double* w = ord + kOrd * (o + p);
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
    const size_t i = o + idx[o + p];
    if (order) { order[4 * i] = v[0]; order[4 * i + 1] = v[1]; order[4 * i + 2] = v[2]; order[4 * i + 3] = v[3]; }
    if (near_) { near_[4 * i] = who[0]; near_[4 * i + 1] = who[1]; near_[4 * i + 2] = who[2]; near_[4 * i + 3] = who[3]; }
    if (counts) { counts[2 * i] = t.n_search; counts[2 * i + 1] = t.n_lsi; }
}

// One workgroup per box: lane t adds the sorted places t, t + 256, ... in that order, a fixed tree adds the lanes of a
// wavefront and thread 0 the four wavefronts in order.
__global__ __launch_bounds__(kThreads) void k_tet_summary(int n, const double* __restrict__ ord, double* __restrict__ summary)
{
    __shared__ double part[kThreads / 64][kSums];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* O = ord + kOrd * (size_t)b * n;
    double t[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) t[k] = 0.0;
    for (int p = tid; p < n; p += kThreads) {
#pragma unroll
        for (int k = 0; k < kOrd; ++k) {
            const double v = O[kOrd * (size_t)p + k];
            const bool defined = v == v;
            t[k] = t[k] + (defined ? v : 0.0);
            t[4 + k] = t[4 + k] + (defined ? 1.0 : 0.0);
        }
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
        write_summary(tot, summary + kSums * (size_t)b);
    }
}

// ---- small geometry: one wavefront per box, lane i = molecule i, the box's fractional positions in LDS ----------------------
// The entries of i in walk_small's order; an entry is j with the image combination above it.
__global__ __launch_bounds__(kThreads) void k_tet_small(int nb, int n, double rs2, double rl2, const double* __restrict__ par,
                                                        const double* __restrict__ pos, double* __restrict__ order, int* __restrict__ near_,
                                                        int* __restrict__ counts, double* __restrict__ summary)
{
    __shared__ double lds[kSmallBoxesPerWg][3 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * kSmallBoxesPerWg + wave;
    if (b >= nb) return;                                   // the whole wavefront; no workgroup barrier below
    double* S = lds[wave];
    const double* H = par + 18 * (size_t)b;
    const bool active = lane < n;
    const size_t m = (size_t)b * n + (active ? lane : 0);
    const double s0 = frac_coord(H + 9, 0, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s1 = frac_coord(H + 9, 1, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s2 = frac_coord(H + 9, 2, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    S[lane] = s0; S[64 + lane] = s1; S[128 + lane] = s2;
    mw::wave_fence();

    Nearest t;
    walk_small(n, active, rs2, H, S, s0, s1, s2, [&](int j, int c, double r2, double, double, double) { t.add(r2, rl2, (c << kPlaceBits) | j); });
    double d[4][3];
    int who[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        d[a][0] = d[a][1] = d[a][2] = 0.0;
        who[a] = -1;
        if (a < t.n_search) {
            const int j = t.e[a] & kPlaceMask, c = t.e[a] >> kPlaceBits;
            const double e0 = S[j] - s0, e1 = S[64 + j] - s1, e2 = S[128 + j] - s2;
            const double f0 = e0 > 0.0 ? e0 - 1.0 : e0 + 1.0, f1 = e1 > 0.0 ? e1 - 1.0 : e1 + 1.0, f2 = e2 > 0.0 ? e2 - 1.0 : e2 + 1.0;
            (void)bond_vector(H, (c & 1) ? f0 : e0, (c & 2) ? f1 : e1, (c & 4) ? f2 : e2, d[a][0], d[a][1], d[a][2]);
            who[a] = j;
        }
    }
    double v[kOrd];
    order_values(t, d, v);
    if (active) {
        if (order) { order[4 * m] = v[0]; order[4 * m + 1] = v[1]; order[4 * m + 2] = v[2]; order[4 * m + 3] = v[3]; }
        if (near_) { near_[4 * m] = who[0]; near_[4 * m + 1] = who[1]; near_[4 * m + 2] = who[2]; near_[4 * m + 3] = who[3]; }
        if (counts) { counts[2 * m] = t.n_search; counts[2 * m + 1] = t.n_lsi; }
    }
    if (summary) {                                         // wave-uniform: lanes beyond n and undefined values add +0.0
        double tot[kSums];
#pragma unroll
        for (int k = 0; k < kOrd; ++k) {
            const bool defined = active && v[k] == v[k];
            tot[k] = mw::wave_sum(defined ? v[k] : 0.0);
            tot[4 + k] = mw::wave_sum(defined ? 1.0 : 0.0);
        }
        if (lane == 0) write_summary(tot, summary + kSums * (size_t)b);
    }
}

}  // namespace mwtet

namespace {

using namespace mwtet;

struct State : Runtime<4> {
    Buf scratch, par, grid, pos, order, near_, counts, summary;
    int last[MW_TET_PLAN_FIELDS] = {0};
    float ms[3] = {0.0f, 0.0f, 0.0f};
} g;

// The scratch of one box of the general geometry: the sort's pieces, then ord.
struct Layout : SortLayout {
    size_t ord, per_box;
};

Layout make_layout(int n)
{
    Layout l;
    size_t o = 0;
    lay_sort(l, n, o);
    l.ord = o;   o += align16(8 * (size_t)kOrd * n);
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
            return fail("%s: one box needs %zu bytes of scratch (nwater = %d) and does not fit the budget of %zu bytes (MW_TET_SCRATCH_MB)",
                        who, p.per_box, n, budget);
        p.bpc = (int)(fit < (size_t)kMaxChunkBoxes ? fit : (size_t)kMaxChunkBoxes);
        if (p.bpc > nboxes) p.bpc = nboxes;
    }
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

int check_scalars(const char* who, int nboxes, int n, double rs, double rl)
{
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    if (!(rs > 0.0) || !std::isfinite(rs)) return fail("%s: r_search = %g bohr is not a finite radius > 0", who, rs);
    if (!(rl > 0.0) || !std::isfinite(rl)) return fail("%s: r_lsi = %g bohr is not a finite radius > 0", who, rl);
    if (!(rl <= rs)) return fail("%s: r_lsi = %.17g bohr is beyond r_search = %.17g bohr (0 < r_lsi <= r_search is required)", who, rl, rs);
    return 0;
}

const char kRadius[] = "r_search";            // the radius the cells are checked against, in the messages

int check_live(const char* who) { return check_live(who, "mw_tet_init", g); }

// The work of both entries, arguments already checked.  par and grid are on the host; pos and the outputs are device pointers
// when `dev`, host pointers otherwise.
int run(const char* who, int nboxes, int n, const std::vector<double>& par, const std::vector<int>& grid, const double* pos, double rs,
        double rl, bool dev, double* order, int* near_, int* counts, double* summary)
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
        if (order && reserve(g.order, 32 * (size_t)n * p.bpc)) return 1;
        if (near_ && reserve(g.near_, 16 * (size_t)n * p.bpc)) return 1;
        if (counts && reserve(g.counts, 8 * (size_t)n * p.bpc)) return 1;
        if (summary && reserve(g.summary, 8 * (size_t)kSums * p.bpc)) return 1;
    }
    if (!p.small && !summary && reserve(g.summary, 8 * (size_t)kSums * p.bpc)) return 1;     // the summary pass always runs
    const double rs2 = rs * rs, rl2 = rl * rl;
    float ms[3] = {0.0f, 0.0f, 0.0f};
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const double* d_pos = pos + 3 * (size_t)n * b0;
        if (!dev) {
            HIPOK(hipMemcpyAsync(g.pos.p, d_pos, 24 * (size_t)n * nb, hipMemcpyHostToDevice, g.stream));
            d_pos = (const double*)g.pos.p;
        }
        const double* d_par = (const double*)g.par.p + 18 * (size_t)b0;
        const int* d_grid = (const int*)g.grid.p + 4 * (size_t)b0;
        double* d_order = !order ? nullptr : dev ? order + 4 * (size_t)n * b0 : (double*)g.order.p;
        int* d_near = !near_ ? nullptr : dev ? near_ + 4 * (size_t)n * b0 : (int*)g.near_.p;
        int* d_counts = !counts ? nullptr : dev ? counts + 2 * (size_t)n * b0 : (int*)g.counts.p;
        double* d_sum = !summary ? nullptr : dev ? summary + kSums * (size_t)b0 : (double*)g.summary.p;
        if (p.small) {
            HIPOK(hipEventRecord(g.ev[0], g.stream));
            hipLaunchKernelGGL(k_tet_small, dim3((unsigned)((nb + kSmallBoxesPerWg - 1) / kSmallBoxesPerWg)), dim3(kThreads), 0, g.stream,
                               nb, n, rs2, rl2, d_par, d_pos, d_order, d_near, d_counts, d_sum);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[1], g.stream));
        } else {
            if (!d_sum) d_sum = (double*)g.summary.p;
            char* base = (char*)g.scratch.p;
            const size_t B = (size_t)p.bpc;
            double* ord = (double*)(base + l.ord * B);
            const dim3 grid_m = per_molecule(n, nb);
            Sorted s;
            HIPOK(hipEventRecord(g.ev[0], g.stream));
            if (sort_into_cells(g.stream, n, nb, l, base, B, d_par, d_grid, d_pos, s)) return 1;
            HIPOK(hipEventRecord(g.ev[1], g.stream));
            hipLaunchKernelGGL(k_tet_select, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, rs2, rl2, d_par, d_grid, s.start, s.ss, s.idx, ord,
                               d_order, d_near, d_counts);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[2], g.stream));
            hipLaunchKernelGGL(k_tet_summary, dim3((unsigned)nb), dim3(kThreads), 0, g.stream, n, (const double*)ord, d_sum);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[3], g.stream));
        }
        if (!dev) {
            if (order) HIPOK(hipMemcpyAsync(order + 4 * (size_t)n * b0, g.order.p, 32 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (near_) HIPOK(hipMemcpyAsync(near_ + 4 * (size_t)n * b0, g.near_.p, 16 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (counts) HIPOK(hipMemcpyAsync(counts + 2 * (size_t)n * b0, g.counts.p, 8 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (summary) HIPOK(hipMemcpyAsync(summary + kSums * (size_t)b0, g.summary.p, 8 * (size_t)kSums * nb, hipMemcpyDeviceToHost, g.stream));
        }
        HIPOK(hipStreamSynchronize(g.stream));               // the next chunk reuses the scratch and the staging buffers
        if (p.small) {
            float t = 0.0f;
            HIPOK(hipEventElapsedTime(&t, g.ev[0], g.ev[1]));
            ms[1] += t;
        } else {
            for (int k = 0; k < 3; ++k) {
                float t = 0.0f;
                HIPOK(hipEventElapsedTime(&t, g.ev[k], g.ev[k + 1]));
                ms[k] += t;
            }
        }
    }
    plan_fields(p, grid.data(), g.last);
    g.have_last = true;
    for (int k = 0; k < 3; ++k) g.ms[k] = ms[k];
    return 0;
}

}  // namespace

extern "C" {

const char* mw_tet_last_error(void) { return g_err; }
int mw_tet_is_initialised(void) { return g.live ? 1 : 0; }

int mw_tet_init(int device) { return runtime_init("mw_tet_init", "MW_TET_SCRATCH_MB", device, g); }

int mw_tet_finalize(void)
{
    if (runtime_finalize(g, {&g.scratch, &g.par, &g.grid, &g.pos, &g.order, &g.near_, &g.counts, &g.summary})) return 1;
    g = State{};
    return 0;
}

int mw_tet_compute(int nboxes, int nwater, const double* cells, const double* pos, double r_search, double r_lsi, double* order, int* near_,
                   int* counts, double* summary)
{
    const char* who = "mw_tet_compute";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, r_search, r_lsi)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (check_cells(who, kRadius, nboxes, nwater, cells, r_search, par, grid)) return 1;
    if (check_live(who)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, r_search, r_lsi, false, order, near_, counts, summary);
}

int mw_tet_compute_device(int nboxes, int nwater, const double* cells, const double* pos, double r_search, double r_lsi, double* order,
                          int* near_, int* counts, double* summary)
{
    const char* who = "mw_tet_compute_device";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, r_search, r_lsi)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (fetch_cells(who, kRadius, nboxes, nwater, cells, r_search, par, grid)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, r_search, r_lsi, true, order, near_, counts, summary);
}

int mw_tet_plan(int nwater, const double* cell, double r_search, int nboxes, int* out, int nout)
{
    const char* who = "mw_tet_plan";
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, r_search, r_search)) return 1;
    if (plan_grid(who, kRadius, nwater, cell, r_search, out, nout, grid)) return 1;
    Plan p;
    if (make_plan(who, nwater, nboxes, g.live ? g.budget : kDefaultBudget, p)) return 1;
    int f[MW_TET_PLAN_FIELDS];
    plan_fields(p, grid.data(), f);
    copy_fields(f, MW_TET_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_tet_last(int* out, int nout) { return last_fields("mw_tet_last", "mw_tet_init", g, g.last, MW_TET_PLAN_FIELDS, out, nout); }

int mw_tet_elapsed_ms(float* binning, float* select, float* summary)
{
    if (check_live("mw_tet_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_tet_elapsed_ms: no call has launched yet");
    if (binning) *binning = g.ms[0];
    if (select) *select = g.ms[1];
    if (summary) *summary = g.ms[2];
    return 0;
}

}  // extern "C"
