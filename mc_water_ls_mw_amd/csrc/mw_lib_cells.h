// The cell layer ten libraries share: how a molecule's neighbour entries are found.  The four analysis libraries include it
// themselves (bond order, tetrahedral order, angle distribution, rings); the six force libraries reach it through
// mw_lib_forces.h (quench, dynamics at constant volume and at constant pressure with a scalar and a per-axis cell, the Hessian,
// thermodynamic integration).  General geometry (nwater > 64): a fractional cell grid, a counting sort into it (k_cells_bin, k_cells_scan,
// k_cells_place, k_cells_rank) and walk_cells, one lane per molecule in sorted order over the 27 neighbouring cells.  Small
// geometry (nwater <= 64): walk_small, one wavefront per box over the eight image combinations of every j.  Included after
// `#pragma clang fp contract(off)` and after mw_lib_host.h.  Like that header it exports nothing: the kernels live in the
// namespace mwcells and every library compiles a copy of its own into its own code object, the rest has internal linkage,
// and every text that names a library or its radius comes from the caller.  (libmw_sk.so has no cell grid and is not a user;
// libmw_hip.so's lists, mw_neighbours.hip.h and mw_host_cells.hip.h, are another contract.)
#pragma once

#include <cstring>
#include <vector>

namespace mwcells {

constexpr int kThreads = 256;                     // the sorting kernels
constexpr int kSmallN = 64;
constexpr int kMaxGrid = 1024;
constexpr int kMaxWater = 1 << 22;
constexpr int kMaxBoxes = 1 << 24;
constexpr int kMaxChunkBoxes = 65535;             // grid y
constexpr int kSmallChunkBoxes = 1 << 20;
constexpr double kGuard = 1.0 + 1e-9;

// s_a = (H^-1 r)_a reduced to [0, 1); I = H^-1, row-major
__device__ __forceinline__ double frac_coord(const double* __restrict__ I, int a, double x, double y, double z)
{
    double s = __builtin_fma(I[3 * a], x, __builtin_fma(I[3 * a + 1], y, I[3 * a + 2] * z));
    s = s - __builtin_floor(s);
    return s >= 1.0 ? 0.0 : s;                 // (-1e-17 - floor = 1.0 after rounding)
}

// the cell of s along an axis of g cells, inside the table whatever s is
__device__ __forceinline__ int cell_of(double s, int g)
{
    const int c = (int)(s * (double)g);
    return c < 0 ? 0 : c >= g ? g - 1 : c;
}

// d = H ds (c = the cell's 9 doubles: c[3 k + a] = component a of h_(k+1)); returns |d|^2
__device__ __forceinline__ double bond_vector(const double* __restrict__ c, double a0, double a1, double a2, double& dx, double& dy, double& dz)
{
    dx = __builtin_fma(c[0], a0, __builtin_fma(c[3], a1, c[6] * a2));
    dy = __builtin_fma(c[1], a0, __builtin_fma(c[4], a1, c[7] * a2));
    dz = __builtin_fma(c[2], a0, __builtin_fma(c[5], a1, c[8] * a2));
    return __builtin_fma(dx, dx, __builtin_fma(dy, dy, dz * dz));
}

// Offset o in {-1, 0, 1} from cell c of g: the cell it lands in and the image shift that goes with it.
__device__ __forceinline__ void wrap_cell(int c, int o, int g, int& cw, int& shift)
{
    cw = c + o; shift = 0;
    if (cw < 0) { cw += g; shift = -1; }
    if (cw >= g) { cw -= g; shift = 1; }
}

// ---- general geometry: the counting sort -----------------------------------------------------------------------------------
// par[box][18]: the cell (9) and its inverse (9).  grid[box][4]: g_1, g_2, g_3, cells.  Per box in scratch: su [n][3] fractional
// positions by index, cid [n], tmp [n] (members of the cells in arrival order), cnt / start [cap + 1]; then in cell order:
// idx [n] the molecule, ss [n][3].

// One lane per molecule: s, its cell, the cell's count.
__global__ __launch_bounds__(kThreads) void k_cells_bin(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                        const double* __restrict__ pos, double* __restrict__ su, int* __restrict__ cid,
                                                        int* __restrict__ cnt)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const double* I = par + 18 * (size_t)b + 9;
    const int* g = grid + 4 * (size_t)b;
    const size_t m = (size_t)b * n + i;
    const double x = pos[3 * m], y = pos[3 * m + 1], z = pos[3 * m + 2];
    const double s0 = frac_coord(I, 0, x, y, z), s1 = frac_coord(I, 1, x, y, z), s2 = frac_coord(I, 2, x, y, z);
    su[3 * m] = s0; su[3 * m + 1] = s1; su[3 * m + 2] = s2;
    const int c = (cell_of(s2, g[2]) * g[1] + cell_of(s1, g[1])) * g[0] + cell_of(s0, g[0]);
    cid[m] = c;
    atomicAdd(cnt + (size_t)b * (cap + 1) + c, 1);
}

// One workgroup per box: start[c] = the members of the cells before c, start[cells] = n.
__global__ __launch_bounds__(kThreads) void k_cells_scan(int cap, const int* __restrict__ grid, const int* __restrict__ cnt, int* __restrict__ start)
{
    __shared__ int part[kThreads];
    const int b = blockIdx.x, tid = threadIdx.x, cells = grid[4 * (size_t)b + 3];
    const int* cn = cnt + (size_t)b * (cap + 1);
    int* st = start + (size_t)b * (cap + 1);
    const int per = (cells + kThreads - 1) / kThreads, c0 = min(tid * per, cells), c1 = min(c0 + per, cells);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += cn[c];
    part[tid] = sum;
    __syncthreads();
    int before = 0;
    for (int t = 0; t < tid; ++t) before += part[t];
    for (int c = c0; c < c1; ++c) { st[c] = before; before += cn[c]; }
    if (tid == kThreads - 1) st[cells] = before;
}

// One lane per molecule: a place among its cell's members, in arrival order (k_cells_rank puts them in index order).
__global__ __launch_bounds__(kThreads) void k_cells_place(int n, int cap, const int* __restrict__ cid, const int* __restrict__ start,
                                                          int* __restrict__ cnt, int* __restrict__ tmp)
{
    const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const size_t m = (size_t)b * n + i, t = (size_t)b * (cap + 1);
    const int c = cid[m];
    const int slot = start[t + c] + atomicSub(cnt + t + c, 1) - 1;
    tmp[(size_t)b * n + slot] = i;
}

// One lane per member: its rank by molecule index among the members of its cell is its place in the sorted order.
__global__ __launch_bounds__(kThreads) void k_cells_rank(int n, int cap, const int* __restrict__ cid, const int* __restrict__ start,
                                                         const int* __restrict__ tmp, const double* __restrict__ su, int* __restrict__ idx,
                                                         double* __restrict__ ss)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const size_t o = (size_t)b * n, t = (size_t)b * (cap + 1);
    const int i = tmp[o + p], c = cid[o + i];
    const int q0 = start[t + c], q1 = start[t + c + 1];
    int rank = 0;
    for (int q = q0; q < q1; ++q) rank += tmp[o + q] < i ? 1 : 0;
    const size_t d = o + q0 + rank;
    idx[d] = i;
    ss[3 * d] = su[3 * (o + i)]; ss[3 * d + 1] = su[3 * (o + i) + 1]; ss[3 * d + 2] = su[3 * (o + i) + 2];
}

// ---- the two walks ---------------------------------------------------------------------------------------------------------
// General geometry: the entries of the molecule at s = (s0, s1, s2), in the contract's order -- the 27 cells around its own,
// z outermost, the members of a cell in sorted order.  Calls hit(q, hx, hy, hz, r2, dx, dy, dz): the sorted place of j, the image
// shift (-1, 0, 1 per axis) of the cell it was found in, |d|^2 and d.  g, st, S: the box's grid, start table and sorted s.
template <typename Hit>
__device__ __forceinline__ void walk_cells(double s0, double s1, double s2, double rc2, const double* __restrict__ H, const int* __restrict__ g,
                                           const int* __restrict__ st, const double* __restrict__ S, Hit hit)
{
    const int g0 = g[0], g1 = g[1], g2 = g[2];
    const int c0 = cell_of(s0, g0), c1 = cell_of(s1, g1), c2 = cell_of(s2, g2);
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
                    const double a0 = (S[3 * (size_t)q] - s0) + fx, a1 = (S[3 * (size_t)q + 1] - s1) + fy, a2 = (S[3 * (size_t)q + 2] - s2) + fz;
                    double dx, dy, dz;
                    const double r2 = bond_vector(H, a0, a1, a2, dx, dy, dz);
                    if (r2 < rc2 && r2 > 0.0) hit(q, hx, hy, hz, r2, dx, dy, dz);
                }
            }
        }
    }
}

// Small geometry, lane i = molecule i with the box's s in S (S[64 a + j] = s_a of j): j in index order, and for each j the eight
// combinations of ds_k and ds_k -/+ 1 (the only two images per axis that can come within a radius <= w_k), combination bit k
// choosing the second along axis k.  Calls hit(j, c, r2, dx, dy, dz) in the lanes that are `active`.
template <typename Hit>
__device__ __forceinline__ void walk_small(int n, bool active, double rc2, const double* __restrict__ H, const double* S, double s0, double s1,
                                           double s2, Hit hit)
{
    for (int j = 0; j < n; ++j) {
        const double e0 = S[j] - s0, e1 = S[64 + j] - s1, e2 = S[128 + j] - s2;
        const double f0 = e0 > 0.0 ? e0 - 1.0 : e0 + 1.0, f1 = e1 > 0.0 ? e1 - 1.0 : e1 + 1.0, f2 = e2 > 0.0 ? e2 - 1.0 : e2 + 1.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            double dx, dy, dz;
            const double r2 = bond_vector(H, (c & 1) ? f0 : e0, (c & 2) ? f1 : e1, (c & 4) ? f2 : e2, dx, dy, dz);
            if (active && r2 < rc2 && r2 > 0.0) hit(j, c, r2, dx, dy, dz);
        }
    }
}

}  // namespace mwcells

namespace {

using namespace mwcells;

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

int cell_cap(int n) { return 2 * n > 64 ? 2 * n : 64; }

// The sort's scratch of one box, piece by piece (byte offsets inside a chunk are these times boxes per chunk).  A library's
// Layout derives from this and continues with its own pieces.
struct SortLayout {
    int cap = 0;                                            // cells a box may have
    size_t su = 0, cid = 0, tmp = 0, cnt = 0, start = 0, idx = 0, ss = 0;
};

// the seven pieces from byte `o` on; `o` comes back behind them
void lay_sort(SortLayout& l, int n, size_t& o)
{
    l.cap = cell_cap(n);
    const size_t tab = align16(4 * ((size_t)l.cap + 1));
    l.su = o;    o += align16(24 * (size_t)n);
    l.cid = o;   o += align16(4 * (size_t)n);
    l.tmp = o;   o += align16(4 * (size_t)n);
    l.cnt = o;   o += tab;
    l.start = o; o += tab;
    l.idx = o;   o += align16(4 * (size_t)n);
    l.ss = o;    o += align16(24 * (size_t)n);
}

// What every library's Plan begins with, and the plan fields of its contract from it.
struct PlanBase {
    int small, bpc, chunks, lds, boxes_per_wg;
    size_t per_box;
};

void plan_fields(const PlanBase& p, const int grid[3], int* f)
{
    f[0] = p.bpc; f[1] = p.chunks; f[2] = p.small; f[3] = grid[0]; f[4] = grid[1]; f[5] = grid[2];
    f[6] = p.lds; f[7] = (int)p.per_box; f[8] = p.boxes_per_wg;
}

// w_k = |det| / |h_l x h_m|
void cell_widths(const double* c, double det, double w[3])
{
    for (int k = 0; k < 3; ++k) {
        const double* a = c + 3 * ((k + 1) % 3);
        const double* b = c + 3 * ((k + 2) % 3);
        const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
        w[k] = std::fabs(det) / std::sqrt(x * x + y * y + z * z);
    }
}

// g_k = max(1, floor(w_k / (r (1 + 1e-9)))), each at most kMaxGrid, the largest lowered until the product fits `cap` cells
void cell_grid(const double w[3], double r, int cap, int g[3])
{
    for (int k = 0; k < 3; ++k) {
        const double f = std::floor(w[k] / (r * kGuard));
        g[k] = f >= (double)kMaxGrid ? kMaxGrid : f >= 1.0 ? (int)f : 1;
    }
    while ((long long)g[0] * g[1] * g[2] > cap) {
        int k = 0;
        if (g[1] > g[k]) k = 1;
        if (g[2] > g[k]) k = 2;
        --g[k];
    }
}

// Every box's cell: invertible, and no narrower than r (1 + 1e-9); `radius` is the library's word for r.  Fills par [nboxes][18]
// and grid [nboxes][4].
int check_cells(const char* who, const char* radius, int nboxes, int n, const double* cells, double r, std::vector<double>& par,
                std::vector<int>& grid)
{
    par.resize(18 * (size_t)nboxes);
    grid.resize(4 * (size_t)nboxes);
    const int cap = cell_cap(n);
    for (int b = 0; b < nboxes; ++b) {
        const double* c = cells + 9 * (size_t)b;
        double* P = par.data() + 18 * (size_t)b;
        double det, w[3];
        if (!invert_cell(c, P + 9, &det))
            return fail("%s: cells: the determinant of box %d is %g (zero or not finite)", who, b, det);
        memcpy(P, c, 9 * sizeof(double));
        cell_widths(c, det, w);
        const double wmin = std::fmin(w[0], std::fmin(w[1], w[2]));
        if (!(r * kGuard <= wmin))
            return fail("%s: %s = %.17g bohr is beyond the narrowest width %.17g bohr of box %d (%s (1 + 1e-9) <= every cell width is required)",
                        who, radius, r, wmin, b, radius);
        int* G = grid.data() + 4 * (size_t)b;
        cell_grid(w, r, cap, G);
        G[3] = G[0] * G[1] * G[2];
    }
    return 0;
}

// The device-pointer entries' check_cells, the library's device current: waits for whoever made the inputs (another stream,
// PyTorch's) and looks at a host copy of the cells.
int fetch_cells(const char* who, const char* radius, int nboxes, int n, const double* d_cells, double r, std::vector<double>& par,
                std::vector<int>& grid)
{
    HIPOK(hipDeviceSynchronize());
    std::vector<double> h_cells(9 * (size_t)nboxes);
    HIPOK(hipMemcpy(h_cells.data(), d_cells, h_cells.size() * sizeof(double), hipMemcpyDeviceToHost));
    return check_cells(who, radius, nboxes, n, h_cells.data(), r, par, grid);
}

// What a plan entry checks once its scalars are good; grid [4] of the one cell.
int plan_grid(const char* who, const char* radius, int n, const double* cell, double r, const int* out, int nout, std::vector<int>& grid)
{
    std::vector<double> par;
    if (!cell) return fail("%s: cell is NULL", who);
    if (!out || nout < 1) return fail("%s: out is NULL or nout < 1", who);
    return check_cells(who, radius, 1, n, cell, r, par, grid);
}

// The body of a library's mw_*_last: the plan fields of the last call that launched.
template <int NEV>
int last_fields(const char* who, const char* init_name, const Runtime<NEV>& rt, const int* last, int nfields, int* out, int nout)
{
    if (check_live(who, init_name, rt)) return 1;
    if (!out || nout < 1) return fail("%s: out is NULL or nout < 1", who);
    if (!rt.have_last) return fail("%s: no call has launched yet", who);
    copy_fields(last, nfields, out, nout);
    return 0;
}

dim3 per_molecule(int n, int nb, int threads = kThreads) { return dim3((unsigned)((n + threads - 1) / threads), (unsigned)nb); }

// what the kernels after the sort read: per box start [cap + 1], and in cell order ss [n][3] and idx [n]
struct Sorted {
    const int* start;
    const double* ss;
    const int* idx;
};

// The counting sort of a chunk of nb boxes on `stream`; `base` is the chunk's scratch, laid out by `l` for bpc boxes.
int sort_into_cells(hipStream_t stream, int n, int nb, const SortLayout& l, char* base, size_t bpc, const double* d_par, const int* d_grid,
                    const double* d_pos, Sorted& s)
{
    double* su = (double*)(base + l.su * bpc);
    int* cid = (int*)(base + l.cid * bpc);
    int* tmp = (int*)(base + l.tmp * bpc);
    int* cnt = (int*)(base + l.cnt * bpc);
    int* start = (int*)(base + l.start * bpc);
    int* idx = (int*)(base + l.idx * bpc);
    double* ss = (double*)(base + l.ss * bpc);
    const dim3 grid_m = per_molecule(n, nb);
    HIPOK(hipMemsetAsync(cnt, 0, 4 * ((size_t)l.cap + 1) * nb, stream));
    hipLaunchKernelGGL(k_cells_bin, grid_m, dim3(kThreads), 0, stream, n, l.cap, d_par, d_grid, d_pos, su, cid, cnt);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_cells_scan, dim3((unsigned)nb), dim3(kThreads), 0, stream, l.cap, d_grid, (const int*)cnt, start);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_cells_place, grid_m, dim3(kThreads), 0, stream, n, l.cap, (const int*)cid, (const int*)start, cnt, tmp);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_cells_rank, grid_m, dim3(kThreads), 0, stream, n, l.cap, (const int*)cid, (const int*)start, (const int*)tmp,
                       (const double*)su, idx, ss);
    HIPOK(hipGetLastError());
    s = Sorted{start, ss, idx};
    return 0;
}

}  // namespace
