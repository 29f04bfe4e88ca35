// libmw_adf.so -- the O-O-O angle distribution of include/mw_adf.h: for every centre molecule the angle between every two of
// its (at most 32 kept) neighbour entries, binned in cos(theta) over the caller's edges into one integer histogram per box and
// group, the entry counts of every molecule and four totals per box and group.  General geometry (nwater > 64): a counting
// sort into a fractional cell grid (the sort of mw_lib_cells.h), then k_adf_angles, one lane per molecule
// in sorted order, walks the 27 neighbouring cells.  Small geometry (nwater <= 64): k_adf_small, one wavefront per box with
// the box in LDS.  In both a lane keeps an entry as (j, image) in LDS and forms its unit vector again when it pairs: the
// first eight unit vectors of a lane live in registers, so a first-shell molecule (4 - 6 entries) forms each of its vectors
// once and never looks at the other 24 slots.  The histograms of a workgroup are 32-bit counters in LDS, flushed with 64-bit
// integer atomics; no floating-point number leaves the device.  The grid rules, the sort and the two walks are
// mw_lib_cells.h's, shared with libmw_boo.so, libmw_tet.so and the other libraries that sort into a cell grid.
#include "../../include/mw_adf.h"

#include "mw_common.hip.h"

#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too
#include "mw_lib_cells.h"

namespace mwadf {

using namespace mwcells;

constexpr int kPairThreads = 128;                 // k_adf_angles: 32 slots x 128 lanes x 4 bytes = 16 KiB of entries per workgroup
constexpr int kKeep = MW_ADF_KEEP;
constexpr int kRegs = 8;                          // unit vectors a lane holds in registers
constexpr int kMaxBins = MW_ADF_MAX_BINS;
constexpr int kMaxGroups = MW_ADF_MAX_GROUPS;
constexpr int kSums = 4;                          // per box and group: centres, pairs enumerated, pairs binned, centres over the cap
constexpr int kPlaceBits = 22;                    // an entry: the place (or index) of j in the low bits, its image above
constexpr int kPlaceMask = (1 << kPlaceBits) - 1;
static_assert(kMaxWater <= (1 << kPlaceBits), "an entry holds a molecule in kPlaceBits bits");
static_assert(kKeep * (kKeep - 1) / 2 * kThreads < (1LL << 31), "a workgroup's 32-bit counter holds every pair of its molecules");

// ---- the LDS of a workgroup ------------------------------------------------------------------------------------------------
// edges [nbins + 1] doubles | (small: the box, 3 x 64 doubles) | entries [kKeep][threads] ints | hist [ngroups][nbins] | sums [ngroups][4]
__host__ __device__ constexpr size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t lds_bytes(int threads, bool small, int nbins, int ngroups)
{
    return up16(8 * ((size_t)nbins + 1)) + (small ? 3 * 64 * 8 : 0) + 4 * (size_t)kKeep * threads + up16(4 * (size_t)ngroups * nbins) +
           4 * (size_t)kSums * ngroups;
}

struct Lds {
    double* edges;
    double* box;
    int* ent;
    unsigned* hist;
    unsigned* sums;
    __device__ __forceinline__ Lds(char* base, int threads, bool small, int nbins, int ngroups)
    {
        edges = (double*)base;          base += up16(8 * ((size_t)nbins + 1));
        box = (double*)base;            base += small ? 3 * 64 * 8 : 0;
        ent = (int*)base;               base += 4 * (size_t)kKeep * threads;
        hist = (unsigned*)base;         base += up16(4 * (size_t)ngroups * nbins);
        sums = (unsigned*)base;
    }
};

// The edges into LDS, the counters to zero.  Every thread of the workgroup calls this; it ends with a barrier.
__device__ __forceinline__ void lds_begin(const Lds& l, int threads, int tid, int nbins, int ngroups, const double* __restrict__ edges)
{
    for (int t = tid; t <= nbins; t += threads) l.edges[t] = edges[t];
    for (int t = tid; t < ngroups * nbins; t += threads) l.hist[t] = 0u;
    for (int t = tid; t < ngroups * kSums; t += threads) l.sums[t] = 0u;
    __syncthreads();
}

// The workgroup's counters into the box's, after a barrier: 64-bit integer adds, only where there is something to add.
__device__ __forceinline__ void lds_flush(const Lds& l, int threads, int tid, int nbins, int ngroups, long long* __restrict__ hist,
                                          long long* __restrict__ summary)
{
    __syncthreads();
    if (hist)
        for (int t = tid; t < ngroups * nbins; t += threads) {
            const unsigned v = l.hist[t];
            if (v) atomicAdd((unsigned long long*)hist + t, (unsigned long long)v);
        }
    if (summary)
        for (int t = tid; t < ngroups * kSums; t += threads) {
            const unsigned v = l.sums[t];
            if (v) atomicAdd((unsigned long long*)summary + t, (unsigned long long)v);
        }
}

// One pair: c clamped, its bin by bisection (at most 10 steps for 1024 bins) and the LDS counter of that bin.
__device__ __forceinline__ void bin_pair(double c, const double* E, int nbins, unsigned* h, unsigned& binned)
{
    c = c < -1.0 ? -1.0 : c > 1.0 ? 1.0 : c;
    if (!(c >= E[0] && c <= E[nbins])) return;
    int lo = 0, hi = nbins;                                  // E[lo] <= c, and c < E[hi] or hi == nbins
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (E[mid] <= c) lo = mid; else hi = mid;
    }
    atomicAdd(h + lo, 1u);
    ++binned;
}

__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3])
{
    return __builtin_fma(a[0], b[0], __builtin_fma(a[1], b[1], a[2] * b[2]));
}

// Every pair a < b of the lane's k kept entries (ent[a * stride], a < k; k = 0: the lane is no centre) into the counters h of its
// group; returns the pairs binned.  `unit(entry, u)` forms u = d (1 / r) of an entry.  kw = the largest k of the wavefront,
// the same in every lane: what is beyond it is skipped by a scalar branch.  The first kRegs unit vectors are formed once
// and held in registers (every index below is a compile-time constant after unrolling); an entry beyond them is formed
// again whenever it is paired, which a first-shell cutoff never reaches.
template <typename Unit>
__device__ __forceinline__ unsigned pair_up(const Unit& unit, const int* ent, int stride, int k, int kw, const double* E, int nbins, unsigned* h)
{
    unsigned binned = 0;
    double u[kRegs][3];
#pragma unroll
    for (int a = 0; a < kRegs; ++a) {
        u[a][0] = u[a][1] = u[a][2] = 0.0;
        if (a < kw) {
            if (a < k) unit(ent[a * stride], u[a]);
        }
    }
#pragma unroll
    for (int b = 1; b < kRegs; ++b) {
        if (b < kw) {
#pragma unroll
            for (int a = 0; a < b; ++a)
                if (b < k) bin_pair(dot3(u[a], u[b]), E, nbins, h, binned);
        }
    }
    for (int b = kRegs; b < kw; ++b) {
        if (b < k) {
            double ub[3];
            unit(ent[b * stride], ub);
#pragma unroll
            for (int a = 0; a < kRegs; ++a) bin_pair(dot3(u[a], ub), E, nbins, h, binned);
            for (int a = kRegs; a < b; ++a) {
                double ua[3];
                unit(ent[a * stride], ua);
                bin_pair(dot3(ua, ub), E, nbins, h, binned);
            }
        }
    }
    return binned;
}

// What a centre adds to the four totals of its group.
__device__ __forceinline__ void add_sums(unsigned* s, int n, int k, unsigned binned)
{
    atomicAdd(s, 1u);
    if (k > 1) atomicAdd(s + 1, (unsigned)(k * (k - 1) / 2));
    if (binned) atomicAdd(s + 2, binned);
    if (n > kKeep) atomicAdd(s + 3, 1u);
}

// ---- general geometry ----------------------------------------------------------------------------------------------------
// The unit vector of an entry of the general geometry: the sorted place of j with the image shift (-1, 0, 1 per axis, base 3) above it.
struct GeneralUnit {
    const double* H;
    const double* S;
    double s0, s1, s2;
    __device__ __forceinline__ void operator()(int entry, double (&u)[3]) const
    {
        const int q = entry & kPlaceMask, image = entry >> kPlaceBits;
        const double fx = (double)(image % 3 - 1), fy = (double)(image / 3 % 3 - 1), fz = (double)(image / 9 - 1);
        double dx, dy, dz;
        const double r2 = bond_vector(H, (S[3 * (size_t)q] - s0) + fx, (S[3 * (size_t)q + 1] - s1) + fy, (S[3 * (size_t)q + 2] - s2) + fz, dx, dy, dz);
        const double rinv = 1.0 / __builtin_sqrt(r2);
        u[0] = dx * rinv; u[1] = dy * rinv; u[2] = dz * rinv;
    }
};

// The angle pass, one lane per molecule in sorted order: the walk of the 27 cells in the contract's order, the first 32 entries
// within r_cut kept in LDS; then the pairs of a centre.  `pairs` = 0: only the counts are wanted.  `group` is NULL or [box][n].
__global__ __launch_bounds__(kPairThreads) void k_adf_angles(int n, int cap, double rc2, const double* __restrict__ par,
                                                             const int* __restrict__ grid, const int* __restrict__ start,
                                                             const double* __restrict__ ss, const int* __restrict__ idx,
                                                             const int* __restrict__ group, int ngroups, int nbins, int pairs,
                                                             const double* __restrict__ edges, long long* __restrict__ hist,
                                                             int* __restrict__ counts, long long* __restrict__ summary)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const Lds l(lds_raw, kPairThreads, false, nbins, ngroups);
    const int b = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * kPairThreads + tid;
    const bool active = p < n;
    lds_begin(l, kPairThreads, tid, nbins, ngroups, edges);
    const double* H = par + 18 * (size_t)b;
    const int* g = grid + 4 * (size_t)b;
    const int* st = start + (size_t)b * (cap + 1);
    const size_t o = (size_t)b * n;
    const double* S = ss + 3 * o;
    const size_t pp = active ? p : 0;
    const double s0 = S[3 * pp], s1 = S[3 * pp + 1], s2 = S[3 * pp + 2];
    const int g0 = g[0], g1 = g[1], g2 = g[2];
    const int c0 = cell_of(s0, g0), c1 = cell_of(s1, g1), c2 = cell_of(s2, g2);
    int* ent = l.ent + tid;
    int cnt = 0;
    if (active) {                                           // walk_cells' loops (mw_lib_cells.h), written out: on the template the pass was slower
        for (int oz = -1; oz <= 1; ++oz) {
            int wz, hz;
            wrap_cell(c2, oz, g2, wz, hz);
            for (int oy = -1; oy <= 1; ++oy) {
                int wy, hy;
                wrap_cell(c1, oy, g1, wy, hy);
                for (int ox = -1; ox <= 1; ++ox) {
                    int wx, hx;
                    wrap_cell(c0, ox, g0, wx, hx);
                    const int c = (wz * g1 + wy) * g0 + wx;
                    const int image = (((hz + 1) * 3 + (hy + 1)) * 3 + (hx + 1)) << kPlaceBits;
                    const double fx = (double)hx, fy = (double)hy, fz = (double)hz;
                    const int q1 = st[c + 1];
                    for (int q = st[c]; q < q1; ++q) {
                        const double a0 = (S[3 * (size_t)q] - s0) + fx, a1 = (S[3 * (size_t)q + 1] - s1) + fy, a2 = (S[3 * (size_t)q + 2] - s2) + fz;
                        double dx, dy, dz;
                        const double r2 = bond_vector(H, a0, a1, a2, dx, dy, dz);
                        if (r2 < rc2 && r2 > 0.0) {
                            if (cnt < kKeep) ent[cnt * kPairThreads] = image | q;
                            ++cnt;
                        }
                    }
                }
            }
        }
    }
    const int i = active ? idx[o + p] : 0;
    if (active && counts) counts[o + i] = cnt;
    if (pairs) {                                            // (the same in every thread)
        int gi = !active ? -1 : group ? group[o + i] : 0;
        if (gi >= ngroups) gi = -1;                         // (the host has rejected such a value; never index beyond the counters)
        const int k = gi < 0 ? 0 : cnt < kKeep ? cnt : kKeep;
        const int kw = __builtin_amdgcn_readfirstlane(mw::wave_max_i(k));
        const GeneralUnit unit{H, S, s0, s1, s2};
        const int gs = gi < 0 ? 0 : gi;
        const unsigned binned = pair_up(unit, ent, kPairThreads, k, kw, l.edges, nbins, l.hist + (size_t)gs * nbins);
        if (gi >= 0) add_sums(l.sums + kSums * gi, cnt, k, binned);
    }
    lds_flush(l, kPairThreads, tid, nbins, ngroups, hist ? hist + (size_t)b * ngroups * nbins : nullptr,
              summary ? summary + (size_t)b * ngroups * kSums : nullptr);
}

// ---- small geometry: one wavefront per box, lane i = molecule i, the box's fractional positions in LDS ----------------------
// The entries of i in walk_small's order; an entry is j with the image combination above it.
struct SmallUnit {
    const double* H;
    const double* S;
    double s0, s1, s2;
    __device__ __forceinline__ void operator()(int entry, double (&u)[3]) const
    {
        const int j = entry & kPlaceMask, c = entry >> kPlaceBits;
        const double e0 = S[j] - s0, e1 = S[64 + j] - s1, e2 = S[128 + j] - s2;
        const double f0 = e0 > 0.0 ? e0 - 1.0 : e0 + 1.0, f1 = e1 > 0.0 ? e1 - 1.0 : e1 + 1.0, f2 = e2 > 0.0 ? e2 - 1.0 : e2 + 1.0;
        double dx, dy, dz;
        const double r2 = bond_vector(H, (c & 1) ? f0 : e0, (c & 2) ? f1 : e1, (c & 4) ? f2 : e2, dx, dy, dz);
        const double rinv = 1.0 / __builtin_sqrt(r2);
        u[0] = dx * rinv; u[1] = dy * rinv; u[2] = dz * rinv;
    }
};

__global__ __launch_bounds__(64) void k_adf_small(int n, double rc2, const double* __restrict__ par, const double* __restrict__ pos,
                                                  const int* __restrict__ group, int ngroups, int nbins, int pairs,
                                                  const double* __restrict__ edges, long long* __restrict__ hist, int* __restrict__ counts,
                                                  long long* __restrict__ summary)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const Lds l(lds_raw, 64, true, nbins, ngroups);
    const int lane = threadIdx.x, b = blockIdx.x;
    double* S = l.box;
    const double* H = par + 18 * (size_t)b;
    const bool active = lane < n;
    const size_t m = (size_t)b * n + (active ? lane : 0);
    const double s0 = frac_coord(H + 9, 0, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s1 = frac_coord(H + 9, 1, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s2 = frac_coord(H + 9, 2, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    S[lane] = s0; S[64 + lane] = s1; S[128 + lane] = s2;
    lds_begin(l, 64, lane, nbins, ngroups, edges);          // (its barrier also publishes the box)

    int* ent = l.ent + lane;
    int cnt = 0;
    walk_small(n, active, rc2, H, S, s0, s1, s2, [&](int j, int c, double, double, double, double) {
        if (cnt < kKeep) ent[cnt * 64] = (c << kPlaceBits) | j;
        ++cnt;
    });
    if (active && counts) counts[m] = cnt;
    if (pairs) {
        int gi = !active ? -1 : group ? group[m] : 0;
        if (gi >= ngroups) gi = -1;
        const int k = gi < 0 ? 0 : cnt < kKeep ? cnt : kKeep;
        const int kw = __builtin_amdgcn_readfirstlane(mw::wave_max_i(k));
        const SmallUnit unit{H, S, s0, s1, s2};
        const int gs = gi < 0 ? 0 : gi;
        const unsigned binned = pair_up(unit, ent, 64, k, kw, l.edges, nbins, l.hist + (size_t)gs * nbins);
        if (gi >= 0) add_sums(l.sums + kSums * gi, cnt, k, binned);
    }
    lds_flush(l, 64, lane, nbins, ngroups, hist ? hist + (size_t)b * ngroups * nbins : nullptr,
              summary ? summary + (size_t)b * ngroups * kSums : nullptr);
}

}  // namespace mwadf

namespace {

using namespace mwadf;

struct State : Runtime<4> {
    Buf scratch, par, grid, edges, pos, group, hist, counts, summary;
    int last[MW_ADF_PLAN_FIELDS] = {0};
    float ms[3] = {0.0f, 0.0f, 0.0f};
} g;

// The scratch of one box of the general geometry: the sort's pieces and nothing more.
struct Layout : SortLayout {
    size_t per_box;
};

Layout make_layout(int n)
{
    Layout l;
    size_t o = 0;
    lay_sort(l, n, o);
    l.per_box = o;
    return l;
}

struct Plan : PlanBase {
    Layout lay;
};

// the histogram and the summary of a box
size_t result_bytes(int nbins, int ngroups) { return 8 * (size_t)ngroups * nbins + 8 * (size_t)kSums * ngroups; }

int make_plan(const char* who, int n, int nbins, int ngroups, int nboxes, size_t budget, Plan& p)
{
    p.small = n <= kSmallN;
    p.lay = make_layout(n);
    p.per_box = (p.small ? 0 : p.lay.per_box) + result_bytes(nbins, ngroups);
    p.lds = (int)lds_bytes(p.small ? 64 : kPairThreads, p.small, nbins, ngroups);
    p.boxes_per_wg = p.small ? 1 : 0;
    const size_t fit = budget / p.per_box;
    if (fit < 1)
        return fail("%s: one box needs %zu bytes of scratch (nwater = %d, nbins = %d, ngroups = %d) and does not fit the budget of %zu bytes "
                    "(MW_ADF_SCRATCH_MB)", who, p.per_box, n, nbins, ngroups, budget);
    const size_t most = (size_t)(p.small ? kSmallChunkBoxes : kMaxChunkBoxes);
    p.bpc = (int)(fit < most ? fit : most);
    if (p.bpc > nboxes) p.bpc = nboxes;
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

int check_scalars(const char* who, int nboxes, int n, double rc, int nbins, int ngroups)
{
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    if (!(rc > 0.0) || !std::isfinite(rc)) return fail("%s: r_cut = %g bohr is not a finite radius > 0", who, rc);
    if (nbins < 1 || nbins > kMaxBins) return fail("%s: nbins = %d outside 1..%d", who, nbins, kMaxBins);
    if (ngroups < 1 || ngroups > kMaxGroups) return fail("%s: ngroups = %d outside 1..%d", who, ngroups, kMaxGroups);
    return 0;
}

// finite, strictly ascending, inside [-1, 1]
int check_edges(const char* who, int nbins, const double* edges)
{
    if (!edges) return fail("%s: edges is NULL", who);
    for (int m = 0; m <= nbins; ++m)
        if (!std::isfinite(edges[m])) return fail("%s: edges[%d] = %g is not finite", who, m, edges[m]);
    for (int m = 0; m < nbins; ++m)
        if (!(edges[m] < edges[m + 1]))
            return fail("%s: edges[%d] = %.17g is not below edges[%d] = %.17g (strictly ascending edges are required)", who, m, edges[m], m + 1,
                        edges[m + 1]);
    if (edges[0] < -1.0) return fail("%s: edges[0] = %.17g is below -1 (edges in cos(theta), inside [-1, 1], are required)", who, edges[0]);
    if (edges[nbins] > 1.0)
        return fail("%s: edges[%d] = %.17g is above 1 (edges in cos(theta), inside [-1, 1], are required)", who, nbins, edges[nbins]);
    return 0;
}

int check_groups(const char* who, int nboxes, int n, int ngroups, const int* group)
{
    for (int b = 0; b < nboxes; ++b)
        for (int i = 0; i < n; ++i) {
            const int v = group[(size_t)b * n + i];
            if (v < -1 || v >= ngroups)
                return fail("%s: group = %d of molecule %d of box %d is neither -1 nor in 0..%d (ngroups = %d)", who, v, i, b, ngroups - 1, ngroups);
        }
    return 0;
}

const char kRadius[] = "r_cut";               // the radius the cells are checked against, in the messages

// what both compute entries can check on the host before they look at the library's state
int check_host_side(const char* who, int nboxes, int n, const double* cells, const double* pos, double rc, int nbins, const double* edges,
                    int ngroups, const int* group)
{
    if (check_scalars(who, nboxes, n, rc, nbins, ngroups)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (check_edges(who, nbins, edges)) return 1;
    if (!group && ngroups != 1) return fail("%s: group is NULL and ngroups = %d (without groups every molecule is a centre of group 0: ngroups = 1)", who, ngroups);
    return 0;
}

int check_live(const char* who) { return check_live(who, "mw_adf_init", g); }

// The work of both entries, arguments already checked.  par, grid and edges are on the host; pos, group and the outputs are
// device pointers when `dev`, host pointers otherwise.
int run(const char* who, int nboxes, int n, const std::vector<double>& par, const std::vector<int>& grid, const double* pos, double rc,
        int nbins, const double* edges, int ngroups, const int* group, bool dev, long long* hist, int* counts, long long* summary)
{
    Plan p;
    if (make_plan(who, n, nbins, ngroups, nboxes, g.budget, p)) return 1;
    const Layout& l = p.lay;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    const size_t hist_box = (size_t)ngroups * nbins, sum_box = (size_t)kSums * ngroups;
    if (!p.small && reserve(g.scratch, l.per_box * (size_t)p.bpc)) return 1;
    if (reserve(g.par, par.size() * sizeof(double))) return 1;
    if (reserve(g.grid, grid.size() * sizeof(int))) return 1;
    if (reserve(g.edges, 8 * ((size_t)nbins + 1))) return 1;
    HIPOK(hipMemcpyAsync(g.par.p, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPOK(hipMemcpyAsync(g.grid.p, grid.data(), grid.size() * sizeof(int), hipMemcpyHostToDevice, g.stream));
    HIPOK(hipMemcpyAsync(g.edges.p, edges, 8 * ((size_t)nbins + 1), hipMemcpyHostToDevice, g.stream));
    if (!dev) {
        if (reserve(g.pos, 24 * (size_t)n * p.bpc)) return 1;
        if (group && reserve(g.group, 4 * (size_t)n * p.bpc)) return 1;
        if (hist && reserve(g.hist, 8 * hist_box * p.bpc)) return 1;
        if (counts && reserve(g.counts, 4 * (size_t)n * p.bpc)) return 1;
        if (summary && reserve(g.summary, 8 * sum_box * p.bpc)) return 1;
    }
    const double rc2 = rc * rc;
    const int pairs = (hist || summary) ? 1 : 0;
    float ms[3] = {0.0f, 0.0f, 0.0f};
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const double* d_pos = pos + 3 * (size_t)n * b0;
        const int* d_group = group ? group + (size_t)n * b0 : nullptr;
        if (!dev) {
            HIPOK(hipMemcpyAsync(g.pos.p, d_pos, 24 * (size_t)n * nb, hipMemcpyHostToDevice, g.stream));
            d_pos = (const double*)g.pos.p;
            if (group) {
                HIPOK(hipMemcpyAsync(g.group.p, d_group, 4 * (size_t)n * nb, hipMemcpyHostToDevice, g.stream));
                d_group = (const int*)g.group.p;
            }
        }
        const double* d_par = (const double*)g.par.p + 18 * (size_t)b0;
        const int* d_grid = (const int*)g.grid.p + 4 * (size_t)b0;
        long long* d_hist = !hist ? nullptr : dev ? hist + hist_box * b0 : (long long*)g.hist.p;
        int* d_counts = !counts ? nullptr : dev ? counts + (size_t)n * b0 : (int*)g.counts.p;
        long long* d_sum = !summary ? nullptr : dev ? summary + sum_box * b0 : (long long*)g.summary.p;
        HIPOK(hipEventRecord(g.ev[0], g.stream));
        if (d_hist) HIPOK(hipMemsetAsync(d_hist, 0, 8 * hist_box * nb, g.stream));
        if (d_sum) HIPOK(hipMemsetAsync(d_sum, 0, 8 * sum_box * nb, g.stream));
        HIPOK(hipEventRecord(g.ev[1], g.stream));
        if (p.small) {
            HIPOK(hipEventRecord(g.ev[2], g.stream));
            hipLaunchKernelGGL(k_adf_small, dim3((unsigned)nb), dim3(64), (size_t)p.lds, g.stream, n, rc2, d_par, d_pos, d_group, ngroups, nbins,
                               pairs, (const double*)g.edges.p, d_hist, d_counts, d_sum);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[3], g.stream));
        } else {
            Sorted s;
            if (sort_into_cells(g.stream, n, nb, l, (char*)g.scratch.p, (size_t)p.bpc, d_par, d_grid, d_pos, s)) return 1;
            HIPOK(hipEventRecord(g.ev[2], g.stream));
            hipLaunchKernelGGL(k_adf_angles, per_molecule(n, nb, kPairThreads), dim3(kPairThreads), (size_t)p.lds, g.stream, n, l.cap, rc2, d_par,
                               d_grid, s.start, s.ss, s.idx, d_group, ngroups, nbins, pairs, (const double*)g.edges.p, d_hist, d_counts, d_sum);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[3], g.stream));
        }
        if (!dev) {
            if (hist) HIPOK(hipMemcpyAsync(hist + hist_box * b0, g.hist.p, 8 * hist_box * nb, hipMemcpyDeviceToHost, g.stream));
            if (counts) HIPOK(hipMemcpyAsync(counts + (size_t)n * b0, g.counts.p, 4 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (summary) HIPOK(hipMemcpyAsync(summary + sum_box * b0, g.summary.p, 8 * sum_box * nb, hipMemcpyDeviceToHost, g.stream));
        }
        HIPOK(hipStreamSynchronize(g.stream));               // the next chunk reuses the scratch and the staging buffers
        float t = 0.0f;
        HIPOK(hipEventElapsedTime(&t, g.ev[0], g.ev[1]));
        ms[2] += t;
        if (!p.small) {
            HIPOK(hipEventElapsedTime(&t, g.ev[1], g.ev[2]));
            ms[0] += t;
        }
        HIPOK(hipEventElapsedTime(&t, g.ev[2], g.ev[3]));
        ms[1] += t;
    }
    plan_fields(p, grid.data(), g.last);
    g.have_last = true;
    for (int k = 0; k < 3; ++k) g.ms[k] = ms[k];
    return 0;
}

}  // namespace

extern "C" {

const char* mw_adf_last_error(void) { return g_err; }
int mw_adf_is_initialised(void) { return g.live ? 1 : 0; }

int mw_adf_init(int device) { return runtime_init("mw_adf_init", "MW_ADF_SCRATCH_MB", device, g); }

int mw_adf_finalize(void)
{
    if (runtime_finalize(g, {&g.scratch, &g.par, &g.grid, &g.edges, &g.pos, &g.group, &g.hist, &g.counts, &g.summary})) return 1;
    g = State{};
    return 0;
}

int mw_adf_compute(int nboxes, int nwater, const double* cells, const double* pos, double r_cut, int nbins, const double* edges, int ngroups,
                   const int* group, long long* hist, int* counts, long long* summary)
{
    const char* who = "mw_adf_compute";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_host_side(who, nboxes, nwater, cells, pos, r_cut, nbins, edges, ngroups, group)) return 1;
    if (check_cells(who, kRadius, nboxes, nwater, cells, r_cut, par, grid)) return 1;
    if (group && check_groups(who, nboxes, nwater, ngroups, group)) return 1;
    if (check_live(who)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, r_cut, nbins, edges, ngroups, group, false, hist, counts, summary);
}

int mw_adf_compute_device(int nboxes, int nwater, const double* cells, const double* pos, double r_cut, int nbins, const double* edges,
                          int ngroups, const int* group, long long* hist, int* counts, long long* summary)
{
    const char* who = "mw_adf_compute_device";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_host_side(who, nboxes, nwater, cells, pos, r_cut, nbins, edges, ngroups, group)) return 1;
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (fetch_cells(who, kRadius, nboxes, nwater, cells, r_cut, par, grid)) return 1;
    if (group) {                                              // a value out of range must not reach the kernels
        std::vector<int> h_group((size_t)nboxes * nwater);
        HIPOK(hipMemcpy(h_group.data(), group, h_group.size() * sizeof(int), hipMemcpyDeviceToHost));
        if (check_groups(who, nboxes, nwater, ngroups, h_group.data())) return 1;
    }
    return run(who, nboxes, nwater, par, grid, pos, r_cut, nbins, edges, ngroups, group, true, hist, counts, summary);
}

int mw_adf_plan(int nwater, const double* cell, double r_cut, int nbins, int ngroups, int nboxes, int* out, int nout)
{
    const char* who = "mw_adf_plan";
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, r_cut, nbins, ngroups)) return 1;
    if (plan_grid(who, kRadius, nwater, cell, r_cut, out, nout, grid)) return 1;
    Plan p;
    if (make_plan(who, nwater, nbins, ngroups, nboxes, g.live ? g.budget : kDefaultBudget, p)) return 1;
    int f[MW_ADF_PLAN_FIELDS];
    plan_fields(p, grid.data(), f);
    copy_fields(f, MW_ADF_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_adf_last(int* out, int nout) { return last_fields("mw_adf_last", "mw_adf_init", g, g.last, MW_ADF_PLAN_FIELDS, out, nout); }

int mw_adf_elapsed_ms(float* binning, float* angles, float* reduce)
{
    if (check_live("mw_adf_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_adf_elapsed_ms: no call has launched yet");
    if (binning) *binning = g.ms[0];
    if (angles) *angles = g.ms[1];
    if (reduce) *reduce = g.ms[2];
    return 0;
}

}  // extern "C"
