// libmw_rings.so -- the primitive rings of include/mw_rings.h: for every box the closed paths of 3 to 7 nodes of the bond
// network over (molecule, image) nodes, counted once per cell at their smallest reading, and those of them that are shortest
// paths; per size the histogram, the membership of every molecule and, on request, the list.  The entries of a molecule are
// found as libmw_adf.so finds them -- general geometry (nwater > 64): a counting sort into a fractional cell grid (the sort
// of mw_lib_cells.h), then k_ring_adj, one lane per molecule over the 27 neighbouring cells; small geometry (nwater <= 64):
// k_ring_small, one wavefront per box with the box in LDS -- and go to scratch as n_i and the first 8 packed (molecule, image)
// codes.  k_ring_rows sorts every row and drops what touches a molecule over the cap.  k_ring_walk,
// one lane per (root, first edge), runs the depth-first walk on a stack in LDS, reads the rows of other molecules from
// scratch, applies the canonical and the shortest-path test at closure and keeps the workgroup's counters in LDS, flushed
// with 64-bit integer atomics.  The list takes k_ring_offsets (a scan of the per-lane ring counts) and the walk again.  No
// floating-point number leaves the device.  The grid rules, the sort and the device primitives are mw_lib_cells.h's, shared
// with libmw_boo.so, libmw_tet.so and libmw_adf.so.
#include "../../include/mw_rings.h"

#include "mw_common.hip.h"

#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too
#include "mw_lib_cells.h"

namespace mwrings {

using namespace mwcells;                          // kThreads: the sorting kernels, k_ring_adj, k_ring_rows, k_ring_offsets

constexpr int kWalkThreads = 128;                 // k_ring_walk: a stack of 7 levels x 2 ints per lane = 7 KiB of LDS
constexpr int kDeg = MW_RINGS_DEG;
constexpr int kSizes = MW_RINGS_SIZES;
constexpr int kMaxRing = MW_RINGS_MAX;
constexpr int kSums = 4;
// A code: the molecule j above six bits of image, (n_1 + 1) (n_2 + 1) (n_3 + 1) two bits each, so that codes ascend as
// (j, n_1, n_2, n_3) does.  kEmpty pads a row.
constexpr int kImageBits = 6;
constexpr int kEmpty = -1;
constexpr int kPad = 0x7fffffff;                  // sorts behind every code
static_assert((long long)kMaxWater << kImageBits <= (1LL << 30), "a code holds a molecule above its image");
static_assert(kDeg == 8, "a row is two int4");
// A node's translation m: (m_1 + 64) (m_2 + 64) (m_3 + 64), a byte each, m_1 highest, so that packed translations ascend as
// (m_1, m_2, m_3) does; |m_k| <= 6 along a walk of 7 nodes.  The byte above them is the cursor of the node's row in the walk.
constexpr int kOrigin = 0x404040;
constexpr int kImageMask = 0xffffff;

__device__ __forceinline__ int make_code(int j, int n1, int n2, int n3) { return (j << kImageBits) | ((n1 + 1) << 4) | ((n2 + 1) << 2) | (n3 + 1); }
__device__ __forceinline__ int code_mol(int code) { return code >> kImageBits; }
// what an edge adds to a packed translation
__device__ __forceinline__ int code_step(int code) { return ((((code >> 4) & 3) - 1) << 16) + ((((code >> 2) & 3) - 1) << 8) + ((code & 3) - 1); }

// |H a|^2: bond_vector without its components
__device__ __forceinline__ double bond_r2(const double* __restrict__ c, double a0, double a1, double a2)
{
    double dx, dy, dz;
    return bond_vector(c, a0, a1, a2, dx, dy, dz);
}

// ---- the adjacency pass --------------------------------------------------------------------------------------------------
// Per box in scratch: ncount [n] the entries of every molecule, raw [n][8] its first 8 codes in the order of the walk.  Both
// kernels write walk_cells' and walk_small's loops (mw_lib_cells.h) out: on the shared templates they took more registers.

// General geometry, one lane per molecule in sorted order: the walk of the 27 cells, every offset with its own image shift.
__global__ __launch_bounds__(kThreads) void k_ring_adj(int n, int cap, double rc2, const double* __restrict__ par, const int* __restrict__ grid,
                                                       const int* __restrict__ start, const double* __restrict__ ss,
                                                       const int* __restrict__ idx, int* __restrict__ ncount, int* __restrict__ raw,
                                                       int* __restrict__ counts)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const double* H = par + 18 * (size_t)b;
    const int* g = grid + 4 * (size_t)b;
    const int* st = start + (size_t)b * (cap + 1);
    const size_t o = (size_t)b * n;
    const double* S = ss + 3 * o;
    const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
    const int g0 = g[0], g1 = g[1], g2 = g[2];
    const int c0 = cell_of(s0, g0), c1 = cell_of(s1, g1), c2 = cell_of(s2, g2);
    const int i = idx[o + p];
    int* mine = raw + kDeg * (o + i);
    int cnt = 0;
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
                const double fx = (double)hx, fy = (double)hy, fz = (double)hz;
                const int q1 = st[c + 1];
                for (int q = st[c]; q < q1; ++q) {
                    const double r2 = bond_r2(H, (S[3 * (size_t)q] - s0) + fx, (S[3 * (size_t)q + 1] - s1) + fy, (S[3 * (size_t)q + 2] - s2) + fz);
                    if (r2 < rc2 && r2 > 0.0) {
                        if (cnt < kDeg) mine[cnt] = make_code(idx[o + q], hx, hy, hz);
                        ++cnt;
                    }
                }
            }
        }
    }
    ncount[o + i] = cnt;
    if (counts) counts[o + i] = cnt;
}

// Small geometry, one wavefront per box, lane i = molecule i: j in index order and for each j the eight combinations of ds_k
// and ds_k -/+ 1, the only two images per axis that can come within r_cut <= w_k -- walk_small's order and arithmetic.
__global__ __launch_bounds__(64) void k_ring_small(int n, double rc2, const double* __restrict__ par, const double* __restrict__ pos,
                                                   int* __restrict__ ncount, int* __restrict__ raw, int* __restrict__ counts)
{
    __shared__ double S[3 * 64];
    const int lane = threadIdx.x, b = blockIdx.x;
    const double* H = par + 18 * (size_t)b;
    const bool active = lane < n;
    const size_t m = (size_t)b * n + (active ? lane : 0);
    const double s0 = frac_coord(H + 9, 0, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s1 = frac_coord(H + 9, 1, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    const double s2 = frac_coord(H + 9, 2, pos[3 * m], pos[3 * m + 1], pos[3 * m + 2]);
    S[lane] = s0; S[64 + lane] = s1; S[128 + lane] = s2;
    __syncthreads();
    int* mine = raw + kDeg * m;
    int cnt = 0;
    for (int j = 0; j < n; ++j) {
        const double e0 = S[j] - s0, e1 = S[64 + j] - s1, e2 = S[128 + j] - s2;
        const int n0 = e0 > 0.0 ? -1 : 1, n1 = e1 > 0.0 ? -1 : 1, n2 = e2 > 0.0 ? -1 : 1;
        const double f0 = e0 + (double)n0, f1 = e1 + (double)n1, f2 = e2 + (double)n2;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const double r2 = bond_r2(H, (c & 1) ? f0 : e0, (c & 2) ? f1 : e1, (c & 4) ? f2 : e2);
            if (active && r2 < rc2 && r2 > 0.0) {
                if (cnt < kDeg) mine[cnt] = make_code(j, (c & 1) ? n0 : 0, (c & 2) ? n1 : 0, (c & 4) ? n2 : 0);
                ++cnt;
            }
        }
    }
    if (active) {
        ncount[m] = cnt;
        if (counts) counts[m] = cnt;
    }
}

__device__ __forceinline__ void order2(int& a, int& b)
{
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo; b = hi;
}

// One lane per molecule: its row of edges, ascending, padded with kEmpty -- the first 8 codes sorted (a network of 19
// exchanges over registers), without the ones to a molecule over the cap; no edges at all for a molecule over the cap.
// The molecules over the cap and the edges to a higher index (every undirected edge once) go to the box's summary.
__global__ __launch_bounds__(kThreads) void k_ring_rows(int n, const int* __restrict__ ncount, const int* __restrict__ raw, int* __restrict__ row,
                                                        long long* __restrict__ summary)
{
    __shared__ unsigned sums[2];
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (threadIdx.x < 2) sums[threadIdx.x] = 0u;
    __syncthreads();
    if (i < n) {
        const size_t o = (size_t)b * n;
        const int c = ncount[o + i];
        const int4* src = (const int4*)(raw + kDeg * (o + i));
        int* dst = row + kDeg * (o + i);
        int w = 0;
        if (c <= kDeg) {
            const int4 lo = src[0], hi = src[1];
            int v0 = 0 < c ? lo.x : kPad, v1 = 1 < c ? lo.y : kPad, v2 = 2 < c ? lo.z : kPad, v3 = 3 < c ? lo.w : kPad;
            int v4 = 4 < c ? hi.x : kPad, v5 = 5 < c ? hi.y : kPad, v6 = 6 < c ? hi.z : kPad, v7 = 7 < c ? hi.w : kPad;
            order2(v0, v1); order2(v2, v3); order2(v4, v5); order2(v6, v7);
            order2(v0, v2); order2(v1, v3); order2(v4, v6); order2(v5, v7);
            order2(v1, v2); order2(v5, v6); order2(v0, v4); order2(v3, v7);
            order2(v1, v5); order2(v2, v6);
            order2(v1, v4); order2(v3, v6);
            order2(v2, v4); order2(v3, v5);
            order2(v3, v4);
            unsigned up = 0;
            const int v[kDeg] = {v0, v1, v2, v3, v4, v5, v6, v7};
#pragma unroll
            for (int a = 0; a < kDeg; ++a)
                if (v[a] != kPad) {
                    const int j = code_mol(v[a]);
                    if (ncount[o + j] <= kDeg) {
                        dst[w++] = v[a];
                        up += j > i ? 1u : 0u;
                    }
                }
            if (up) atomicAdd(&sums[1], up);
        } else {
            atomicAdd(&sums[0], 1u);
        }
        for (; w < kDeg; ++w) dst[w] = kEmpty;
    }
    __syncthreads();
    if (summary && threadIdx.x < 2 && sums[threadIdx.x])
        atomicAdd((unsigned long long*)summary + (size_t)b * kSums + threadIdx.x, (unsigned long long)sums[threadIdx.x]);
}

// ---- the walk ------------------------------------------------------------------------------------------------------------
// The stack of a lane in LDS: level t holds node v_t of the path, its molecule in mol[t][lane] and in img[t][lane] its packed
// translation with the cursor of its row above.  Level 0 is the root at the origin, level 1 the lane's first edge.
struct Stack {
    int* mol;
    int* img;
    __device__ __forceinline__ int m(int t) const { return mol[t * kWalkThreads]; }
    __device__ __forceinline__ int t(int t_) const { return img[t_ * kWalkThreads] & kImageMask; }
};

// Is w = (wm, wt) joined to u = (um, ut)?  A scan of the row of u for the code of (wm, wt - ut).
__device__ __forceinline__ bool joined(const int* __restrict__ R, int um, int ut, int wm, int wt)
{
    const int d1 = ((wt >> 16) & 0xff) - ((ut >> 16) & 0xff), d2 = ((wt >> 8) & 0xff) - ((ut >> 8) & 0xff), d3 = (wt & 0xff) - (ut & 0xff);
    if (d1 < -1 || d1 > 1 || d2 < -1 || d2 > 1 || d3 < -1 || d3 > 1) return false;
    const int want = make_code(wm, d1, d2, d3);
    const int4* r = (const int4*)(R + kDeg * (size_t)um);
    const int4 lo = r[0], hi = r[1];
    return lo.x == want || lo.y == want || lo.z == want || lo.w == want || hi.x == want || hi.y == want || hi.z == want || hi.w == want;
}

// Is the reading v_0 v_1 ... of the closed path of L nodes on the stack the smallest of its 2 L readings?  `full` comes back
// true if that took the comparison of all readings.  Every other member's molecule is the root's or above it (the walk prunes
// below), so only readings rooted at an image of the root's molecule can be smaller.
__device__ __forceinline__ bool canonical(const Stack& s, int L, bool& full)
{
    const int r = s.m(0);
    full = s.m(1) == s.m(L - 1);
    for (int t = 1; t < L; ++t) full = full || s.m(t) == r;
    if (!full) return s.m(1) < s.m(L - 1);
    for (int root = 0; root < L; ++root) {
        if (s.m(root) != r) continue;
        const int shift = s.t(root) - kOrigin;              // (no byte borrows from its neighbour: every byte stays inside 64 +/- 12)
        for (int dir = -1; dir <= 1; dir += 2) {
            if (root == 0 && dir == 1) continue;             // (the reading itself)
            int at = root;
            for (int k = 1; k < L; ++k) {                    // (element 0 of both is the root's molecule at the origin)
                at += dir;
                at = at < 0 ? at + L : at >= L ? at - L : at;
                const int tm = s.m(at), om = s.m(k);
                if (tm != om) {
                    if (tm < om) return false;
                    break;
                }
                const int tt = s.t(at) - shift, ot = s.t(k);
                if (tt != ot) {
                    if (tt < ot) return false;
                    break;
                }
            }
        }
    }
    return true;
}

// No two nodes of the closed path closer in the graph than round the ring.
__device__ __forceinline__ bool primitive(const Stack& s, const int* __restrict__ R, int L)
{
    for (int a = 0; a < L; ++a) {
        const int am = s.m(a), at = s.t(a);
        for (int b = a + 2; b < L; ++b) {
            const int round = b - a < L - (b - a) ? b - a : L - (b - a);
            if (round < 2) continue;                         // (a = 0, b = L - 1)
            const int bm = s.m(b), bt = s.t(b);
            if (joined(R, am, at, bm, bt)) return false;
            if (round == 3)
                for (int k = 0; k < kDeg; ++k) {
                    const int code = R[kDeg * (size_t)am + k];
                    if (code < 0) break;
                    if (joined(R, bm, bt, code_mol(code), at + code_step(code))) return false;
                }
        }
    }
    return true;
}

// One lane per (root, slot of its row).  LIST false: the counts -- closed, hist, member, the two ring totals of the summary and
// the rings of every lane in lanes[box][8 n].  LIST true: lanes holds the rings of the lanes before each lane, and the lane
// writes its rings into the rows of `list` from there on, up to list_cap.
template <bool LIST>
__global__ __launch_bounds__(kWalkThreads) void k_ring_walk(int n, const int* __restrict__ row, int* __restrict__ lanes,
                                                            long long* __restrict__ hist, long long* __restrict__ closed,
                                                            int* __restrict__ member, long long* __restrict__ summary,
                                                            int* __restrict__ list, int list_cap)
{
    __shared__ int stack_mol[kMaxRing * kWalkThreads], stack_img[kMaxRing * kWalkThreads];
    __shared__ unsigned tally[2 * kSizes + 2];                // closed [5] | hist [5] | full | rings
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long gid = (long long)blockIdx.x * kWalkThreads + tid;
    const bool active = gid < (long long)kDeg * n;
    if (tid < 2 * kSizes + 2) tally[tid] = 0u;
    __syncthreads();
    const int* R = row + kDeg * (size_t)b * n;
    const Stack s{stack_mol + tid, stack_img + tid};
    const int r = (int)(gid >> 3);
    const int first = active ? R[gid] : kEmpty;
    unsigned found = 0;
    long long slot = LIST && active ? (long long)lanes[(size_t)b * kDeg * n + gid] : 0;
    if (first >= 0 && code_mol(first) >= r) {
        s.mol[0] = r;                           s.img[0] = kOrigin;
        s.mol[kWalkThreads] = code_mol(first);  s.img[kWalkThreads] = kOrigin + code_step(first);
        int depth = 1;
        while (depth >= 1) {
            const int um = s.mol[depth * kWalkThreads], ui = s.img[depth * kWalkThreads], k = (int)((unsigned)ui >> 24);
            if (k >= kDeg) { --depth; continue; }
            s.img[depth * kWalkThreads] = ui + (1 << 24);
            const int code = R[kDeg * (size_t)um + k];
            if (code < 0) { --depth; continue; }             // (the padding is behind the edges)
            const int j = code_mol(code);
            if (j < r) continue;                             // a ring is counted at its smallest molecule
            const int wt = (ui & kImageMask) + code_step(code);
            if (j == r && wt == kOrigin) {                   // back at the root itself
                const int L = depth + 1;
                if (L < 3) continue;
                bool full;
                if (!canonical(s, L, full)) continue;
                const bool prim = primitive(s, R, L);
                if (!LIST) {
                    atomicAdd(&tally[L - 3], 1u);
                    if (prim) {
                        atomicAdd(&tally[kSizes + L - 3], 1u);
                        if (full) atomicAdd(&tally[2 * kSizes], 1u);
                        if (member)
                            for (int t = 0; t < L; ++t) atomicAdd(member + ((size_t)b * n + s.m(t)) * kSizes + (L - 3), 1);
                        ++found;
                    }
                } else if (prim) {
                    if (slot < (long long)list_cap) {
                        int* out = list + ((size_t)b * list_cap + (size_t)slot) * 8;
                        out[0] = L;
                        for (int t = 0; t < kMaxRing; ++t) out[1 + t] = t < L ? s.m(t) : -1;
                    }
                    ++slot;
                }
                continue;
            }
            bool seen = false;
            for (int t = 1; t <= depth; ++t) seen = seen || (s.m(t) == j && s.t(t) == wt);
            if (seen || depth == kMaxRing - 1) continue;
            // from level depth + 1 the path has 6 - depth edges left to be back at the origin, one step per axis each
            const int room = kMaxRing - 1 - depth;
            const int a1 = ((wt >> 16) & 0xff) - 64, a2 = ((wt >> 8) & 0xff) - 64, a3 = (wt & 0xff) - 64;
            if (a1 > room || -a1 > room || a2 > room || -a2 > room || a3 > room || -a3 > room) continue;
            ++depth;
            s.mol[depth * kWalkThreads] = j;
            s.img[depth * kWalkThreads] = wt;                // (cursor 0)
        }
    }
    if (!LIST) {
        if (active) lanes[(size_t)b * kDeg * n + gid] = (int)found;
        if (found) atomicAdd(&tally[2 * kSizes + 1], found);
        __syncthreads();
        if (tid < kSizes) {
            if (closed && tally[tid]) atomicAdd((unsigned long long*)closed + (size_t)b * kSizes + tid, (unsigned long long)tally[tid]);
            if (hist && tally[kSizes + tid]) atomicAdd((unsigned long long*)hist + (size_t)b * kSizes + tid, (unsigned long long)tally[kSizes + tid]);
        } else if (tid < kSizes + 2) {
            const unsigned v = tally[kSizes + tid];
            if (summary && v) atomicAdd((unsigned long long*)summary + (size_t)b * kSums + (tid - kSizes + 2), (unsigned long long)v);
        }
    }
}

// One workgroup per box: lanes[t] = the rings of the lanes before t (an exclusive scan in place over 8 n counts).
__global__ __launch_bounds__(kThreads) void k_ring_offsets(int n, int* __restrict__ lanes)
{
    __shared__ int part[kThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long total = (long long)kDeg * n;
    int* v = lanes + (size_t)b * total;
    const long long per = (total + kThreads - 1) / kThreads;
    const long long t0 = tid * per < total ? tid * per : total, t1 = t0 + per < total ? t0 + per : total;
    int sum = 0;
    for (long long t = t0; t < t1; ++t) sum += v[t];
    part[tid] = sum;
    __syncthreads();
    int before = 0;
    for (int t = 0; t < tid; ++t) before += part[t];
    for (long long t = t0; t < t1; ++t) { const int c = v[t]; v[t] = before; before += c; }
}

}  // namespace mwrings

namespace {

using namespace mwrings;

struct State : Runtime<4> {
    Buf scratch, par, grid, pos, hist, closed, member, counts, summary, list;
    int last[MW_RINGS_PLAN_FIELDS] = {0};
    float ms[3] = {0.0f, 0.0f, 0.0f};
} g;

// The scratch of one box: the sort's pieces (the small geometry has none of them), then the adjacency and the walk's.
struct Layout : SortLayout {
    size_t ncount, raw, row, lanes, per_box;
};

Layout make_layout(int n, bool small)
{
    Layout l;
    size_t o = 0;
    if (!small) lay_sort(l, n, o);
    l.ncount = o; o += align16(4 * (size_t)n);
    l.raw = o;    o += 4 * (size_t)kDeg * n;
    l.row = o;    o += 4 * (size_t)kDeg * n;
    l.lanes = o;  o += 4 * (size_t)kDeg * n;
    l.per_box = o;
    return l;
}

struct Plan : PlanBase {
    Layout lay;
};

constexpr int kWalkLds = 2 * 4 * kMaxRing * kWalkThreads + 4 * (2 * kSizes + 2);

int make_plan(const char* who, int n, int nboxes, size_t budget, Plan& p)
{
    p.small = n <= kSmallN;
    p.lay = make_layout(n, p.small);
    p.per_box = p.lay.per_box;
    p.lds = kWalkLds;
    p.boxes_per_wg = p.small ? 1 : 0;
    const size_t fit = budget / p.per_box;
    if (fit < 1)
        return fail("%s: one box needs %zu bytes of scratch (nwater = %d) and does not fit the budget of %zu bytes (MW_RINGS_SCRATCH_MB)", who,
                    p.per_box, n, budget);
    p.bpc = (int)(fit < (size_t)kMaxChunkBoxes ? fit : (size_t)kMaxChunkBoxes);
    if (p.bpc > nboxes) p.bpc = nboxes;
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

int check_scalars(const char* who, int nboxes, int n, double rc)
{
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    if (!(rc > 0.0) || !std::isfinite(rc)) return fail("%s: r_cut = %g bohr is not a finite radius > 0", who, rc);
    return 0;
}

const char kRadius[] = "r_cut";               // the radius the cells are checked against, in the messages

// what both compute entries can check on the host before they look at the library's state
int check_host_side(const char* who, int nboxes, int n, const double* cells, const double* pos, double rc, int list_cap)
{
    if (check_scalars(who, nboxes, n, rc)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (list_cap < 0) return fail("%s: list_cap = %d is negative", who, list_cap);
    return 0;
}

int check_live(const char* who) { return check_live(who, "mw_rings_init", g); }

// The work of both entries, arguments already checked.  par and grid are on the host; pos and the outputs are device pointers
// when `dev`, host pointers otherwise.
int run(const char* who, int nboxes, int n, const std::vector<double>& par, const std::vector<int>& grid, const double* pos, double rc,
        int list_cap, bool dev, long long* hist, long long* closed, int* member, int* counts, long long* summary, int* list)
{
    Plan p;
    if (make_plan(who, n, nboxes, g.budget, p)) return 1;
    const Layout& l = p.lay;
    if (!list_cap) list = nullptr;
    const bool walk = hist || closed || member || summary || list;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    const size_t list_box = 8 * (size_t)list_cap, member_box = (size_t)kSizes * n;
    if (reserve(g.scratch, l.per_box * (size_t)p.bpc)) return 1;
    if (reserve(g.par, par.size() * sizeof(double))) return 1;
    if (reserve(g.grid, grid.size() * sizeof(int))) return 1;
    HIPOK(hipMemcpyAsync(g.par.p, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPOK(hipMemcpyAsync(g.grid.p, grid.data(), grid.size() * sizeof(int), hipMemcpyHostToDevice, g.stream));
    if (!dev) {
        if (reserve(g.pos, 24 * (size_t)n * p.bpc)) return 1;
        if (hist && reserve(g.hist, 8 * (size_t)kSizes * p.bpc)) return 1;
        if (closed && reserve(g.closed, 8 * (size_t)kSizes * p.bpc)) return 1;
        if (member && reserve(g.member, 4 * member_box * p.bpc)) return 1;
        if (counts && reserve(g.counts, 4 * (size_t)n * p.bpc)) return 1;
        if (summary && reserve(g.summary, 8 * (size_t)kSums * p.bpc)) return 1;
        if (list && reserve(g.list, 4 * list_box * p.bpc)) return 1;
    }
    const double rc2 = rc * rc;
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
        long long* d_hist = !hist ? nullptr : dev ? hist + (size_t)kSizes * b0 : (long long*)g.hist.p;
        long long* d_closed = !closed ? nullptr : dev ? closed + (size_t)kSizes * b0 : (long long*)g.closed.p;
        int* d_member = !member ? nullptr : dev ? member + member_box * b0 : (int*)g.member.p;
        int* d_counts = !counts ? nullptr : dev ? counts + (size_t)n * b0 : (int*)g.counts.p;
        long long* d_sum = !summary ? nullptr : dev ? summary + (size_t)kSums * b0 : (long long*)g.summary.p;
        int* d_list = !list ? nullptr : dev ? list + list_box * b0 : (int*)g.list.p;
        char* base = (char*)g.scratch.p;
        const size_t B = (size_t)p.bpc;
        int* ncount = (int*)(base + l.ncount * B);
        int* raw = (int*)(base + l.raw * B);
        int* row = (int*)(base + l.row * B);
        int* lanes = (int*)(base + l.lanes * B);
        HIPOK(hipEventRecord(g.ev[0], g.stream));
        if (p.small) {
            HIPOK(hipEventRecord(g.ev[1], g.stream));
            hipLaunchKernelGGL(k_ring_small, dim3((unsigned)nb), dim3(64), 0, g.stream, n, rc2, d_par, d_pos, ncount, raw, d_counts);
            HIPOK(hipGetLastError());
        } else {
            Sorted s;
            if (sort_into_cells(g.stream, n, nb, l, base, B, d_par, d_grid, d_pos, s)) return 1;
            HIPOK(hipEventRecord(g.ev[1], g.stream));
            hipLaunchKernelGGL(k_ring_adj, per_molecule(n, nb), dim3(kThreads), 0, g.stream, n, l.cap, rc2, d_par, d_grid, s.start, s.ss, s.idx,
                               ncount, raw, d_counts);
            HIPOK(hipGetLastError());
        }
        if (walk) {
            if (d_sum) HIPOK(hipMemsetAsync(d_sum, 0, 8 * (size_t)kSums * nb, g.stream));
            hipLaunchKernelGGL(k_ring_rows, per_molecule(n, nb), dim3(kThreads), 0, g.stream, n, (const int*)ncount, (const int*)raw, row,
                               d_sum);
            HIPOK(hipGetLastError());
        }
        HIPOK(hipEventRecord(g.ev[2], g.stream));
        if (walk) {
            if (d_hist) HIPOK(hipMemsetAsync(d_hist, 0, 8 * (size_t)kSizes * nb, g.stream));
            if (d_closed) HIPOK(hipMemsetAsync(d_closed, 0, 8 * (size_t)kSizes * nb, g.stream));
            if (d_member) HIPOK(hipMemsetAsync(d_member, 0, 4 * member_box * nb, g.stream));
            const dim3 grid_w((unsigned)(((size_t)kDeg * n + kWalkThreads - 1) / kWalkThreads), (unsigned)nb);
            hipLaunchKernelGGL(k_ring_walk<false>, grid_w, dim3(kWalkThreads), 0, g.stream, n, (const int*)row, lanes, d_hist, d_closed, d_member,
                               d_sum, (int*)nullptr, 0);
            HIPOK(hipGetLastError());
            if (d_list) {
                HIPOK(hipMemsetAsync(d_list, 0xff, 4 * list_box * nb, g.stream));
                hipLaunchKernelGGL(k_ring_offsets, dim3((unsigned)nb), dim3(kThreads), 0, g.stream, n, lanes);
                HIPOK(hipGetLastError());
                hipLaunchKernelGGL(k_ring_walk<true>, grid_w, dim3(kWalkThreads), 0, g.stream, n, (const int*)row, lanes, (long long*)nullptr,
                                   (long long*)nullptr, (int*)nullptr, (long long*)nullptr, d_list, list_cap);
                HIPOK(hipGetLastError());
            }
        }
        HIPOK(hipEventRecord(g.ev[3], g.stream));
        if (!dev) {
            if (hist) HIPOK(hipMemcpyAsync(hist + (size_t)kSizes * b0, g.hist.p, 8 * (size_t)kSizes * nb, hipMemcpyDeviceToHost, g.stream));
            if (closed) HIPOK(hipMemcpyAsync(closed + (size_t)kSizes * b0, g.closed.p, 8 * (size_t)kSizes * nb, hipMemcpyDeviceToHost, g.stream));
            if (member) HIPOK(hipMemcpyAsync(member + member_box * b0, g.member.p, 4 * member_box * nb, hipMemcpyDeviceToHost, g.stream));
            if (counts) HIPOK(hipMemcpyAsync(counts + (size_t)n * b0, g.counts.p, 4 * (size_t)n * nb, hipMemcpyDeviceToHost, g.stream));
            if (summary) HIPOK(hipMemcpyAsync(summary + (size_t)kSums * b0, g.summary.p, 8 * (size_t)kSums * nb, hipMemcpyDeviceToHost, g.stream));
            if (list) HIPOK(hipMemcpyAsync(list + list_box * b0, g.list.p, 4 * list_box * nb, hipMemcpyDeviceToHost, g.stream));
        }
        HIPOK(hipStreamSynchronize(g.stream));               // the next chunk reuses the scratch and the staging buffers
        float t = 0.0f;
        if (!p.small) {
            HIPOK(hipEventElapsedTime(&t, g.ev[0], g.ev[1]));
            ms[0] += t;
        }
        HIPOK(hipEventElapsedTime(&t, g.ev[1], g.ev[2]));
        ms[1] += t;
        HIPOK(hipEventElapsedTime(&t, g.ev[2], g.ev[3]));
        ms[2] += t;
    }
    plan_fields(p, grid.data(), g.last);
    g.have_last = true;
    for (int k = 0; k < 3; ++k) g.ms[k] = ms[k];
    return 0;
}

}  // namespace

extern "C" {

const char* mw_rings_last_error(void) { return g_err; }
int mw_rings_is_initialised(void) { return g.live ? 1 : 0; }

int mw_rings_init(int device) { return runtime_init("mw_rings_init", "MW_RINGS_SCRATCH_MB", device, g); }

int mw_rings_finalize(void)
{
    if (runtime_finalize(g, {&g.scratch, &g.par, &g.grid, &g.pos, &g.hist, &g.closed, &g.member, &g.counts, &g.summary, &g.list})) return 1;
    g = State{};
    return 0;
}

int mw_rings_compute(int nboxes, int nwater, const double* cells, const double* pos, double r_cut, int list_cap, long long* hist,
                     long long* closed, int* member, int* counts, long long* summary, int* list)
{
    const char* who = "mw_rings_compute";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_host_side(who, nboxes, nwater, cells, pos, r_cut, list_cap)) return 1;
    if (check_cells(who, kRadius, nboxes, nwater, cells, r_cut, par, grid)) return 1;
    if (check_live(who)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, r_cut, list_cap, false, hist, closed, member, counts, summary, list);
}

int mw_rings_compute_device(int nboxes, int nwater, const double* cells, const double* pos, double r_cut, int list_cap, long long* hist,
                            long long* closed, int* member, int* counts, long long* summary, int* list)
{
    const char* who = "mw_rings_compute_device";
    std::vector<double> par;
    std::vector<int> grid;
    if (check_host_side(who, nboxes, nwater, cells, pos, r_cut, list_cap)) return 1;
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (fetch_cells(who, kRadius, nboxes, nwater, cells, r_cut, par, grid)) return 1;
    return run(who, nboxes, nwater, par, grid, pos, r_cut, list_cap, true, hist, closed, member, counts, summary, list);
}

int mw_rings_plan(int nwater, const double* cell, double r_cut, int nboxes, int* out, int nout)
{
    const char* who = "mw_rings_plan";
    std::vector<int> grid;
    if (check_scalars(who, nboxes, nwater, r_cut)) return 1;
    if (plan_grid(who, kRadius, nwater, cell, r_cut, out, nout, grid)) return 1;
    Plan p;
    if (make_plan(who, nwater, nboxes, g.live ? g.budget : kDefaultBudget, p)) return 1;
    int f[MW_RINGS_PLAN_FIELDS];
    plan_fields(p, grid.data(), f);
    copy_fields(f, MW_RINGS_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_rings_last(int* out, int nout) { return last_fields("mw_rings_last", "mw_rings_init", g, g.last, MW_RINGS_PLAN_FIELDS, out, nout); }

int mw_rings_elapsed_ms(float* binning, float* adjacency, float* walk)
{
    if (check_live("mw_rings_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_rings_elapsed_ms: no call has launched yet");
    if (binning) *binning = g.ms[0];
    if (adjacency) *adjacency = g.ms[1];
    if (walk) *walk = g.ms[2];
    return 0;
}

}  // extern "C"
