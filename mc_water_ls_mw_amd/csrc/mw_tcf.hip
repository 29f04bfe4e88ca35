// libmw_tcf.so -- the time correlation functions of include/mw_tcf.h: mean squared and quartic displacement, velocity
// autocorrelation, the self-intermediate scattering function and histograms of the squared displacement of every box of a
// frame-major trajectory, averaged over time origins and molecules.  k_tcf_check is the verdict-only look at device arrays,
// k_tcf_com forms the centre of every (frame, box), k_tcf_corr -- a workgroup per (box, tile of molecules, block of lags),
// lane = lag, frames staged in LDS as [molecule][component][frame] -- forms the partial sums of every (tile, lag) in registers,
// k_tcf_reduce adds the tiles in order and divides once, and k_tcf_hist counts the squared displacements of the selected lags
// in 32-bit LDS counters that it flushes with 64-bit integer atomics.  No floating-point atomic anywhere: every sum has the
// order the header states.
#include "../../include/mw_tcf.h"

#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too

namespace mwtcf {

constexpr int kTile = MW_TCF_TILE;
constexpr int kLagBlock = MW_TCF_LAG_BLOCK;       // = the threads of k_tcf_corr
constexpr int kChunk = MW_TCF_ORIGIN_CHUNK;
constexpr int kWindow = kLagBlock + kChunk - 1;   // target frames a chunk of origins reaches from one lag block
constexpr int kRows = 3 * kTile;                  // (molecule, component) rows of the LDS images
constexpr int kWO = kChunk + 1;                   // row lengths in doubles, odd: the rows of one frame fall on different banks when staged
constexpr int kWT = kWindow + 2;
static_assert(kWO % 2 == 1 && kWT % 2 == 1, "odd row lengths");
constexpr int kCorrLds = 8 * kRows * (kWO + kWT);
static_assert(2 * kCorrLds <= 160 * 1024, "at least two workgroups of k_tcf_corr per CU");
constexpr int kMaxQ = MW_TCF_MAX_Q;
constexpr int kMaxEdges = MW_TCF_MAX_EDGES;
constexpr int kMaxHistLags = MW_TCF_MAX_HIST_LAGS;
constexpr int kMaxFrames = MW_TCF_MAX_FRAMES;
constexpr int kMaxWater = 1 << 22;
constexpr int kMaxBoxes = 1 << 24;
constexpr int kMaxChunkBoxes = 65535;             // a chunk's boxes are a grid dimension
constexpr int kHistThreads = 256;
constexpr int kHistSlabItems = 1 << 16;           // terms a workgroup of k_tcf_hist takes at least, unless the slabs run out
constexpr int kMaxSlabs = 65535;
constexpr int kSums = 3;                          // msd, mqd, vacf; the nq sums of F_s follow
constexpr unsigned long long kNoVerdict = ~0ULL;

struct Waves {
    double v[kMaxQ];
};

__host__ __device__ constexpr size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// ---- the verdict-only check of device arrays: the smallest index of an element that is not finite -------------------------
__global__ __launch_bounds__(256) void k_tcf_check(size_t count, const double* __restrict__ a, unsigned long long* __restrict__ verdict)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const double v = a[i];
        if (!(v - v == 0.0)) atomicMin(verdict, (unsigned long long)i);
    }
}

// ---- the centre of every (frame, box of the chunk): one wavefront each, com[frame][nbc][3] ---------------------------------
__global__ __launch_bounds__(64) void k_tcf_com(int nbs, int nbc, int n, const double* __restrict__ src, double* __restrict__ com)
{
    const int f = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const double* x = src + ((size_t)f * nbs + b) * n * 3;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int j = lane; j < n; j += 64) {
        s0 += x[3 * (size_t)j];
        s1 += x[3 * (size_t)j + 1];
        s2 += x[3 * (size_t)j + 2];
    }
    for (int m = 32; m >= 1; m >>= 1) {
        s0 += __shfl_xor(s0, m, 64);
        s1 += __shfl_xor(s1, m, 64);
        s2 += __shfl_xor(s2, m, 64);
    }
    if (lane == 0) {
        const double dn = (double)n;
        double* c = com + ((size_t)f * nbc + b) * 3;
        c[0] = s0 / dn; c[1] = s1 / dn; c[2] = s2 / dn;
    }
}

// ---- the correlation pass -----------------------------------------------------------------------------------------------------
// `count` frames from `first` of the tile's rows into the LDS image `dst` (rows of `width` doubles), centred where `com` is
// given; a frame beyond the trajectory is zeros, which no valid lag reads.
__device__ __forceinline__ void stage(double* dst, int width, int first, int count, int nframes, int nbs, int nbc, int n, int b, int m0,
                                      int rows, const double* __restrict__ src, const double* __restrict__ com, int tid)
{
    const int total = count * rows;
    for (int t = tid; t < total; t += kLagBlock) {
        const int f = t / rows, e = t - f * rows, fa = first + f;
        double v = 0.0;
        if (fa < nframes) {
            v = src[(((size_t)fa * nbs + b) * n + m0) * 3 + e];
            if (com) v = v - com[((size_t)fa * nbc + b) * 3 + e % 3];
        }
        dst[e * width + f] = v;
    }
}

// part[box of the chunk][tile][3 + nq][nlags]; a sum nobody asked for is written as 0
template <int NQC>
__global__ __launch_bounds__(kLagBlock) void k_tcf_corr(int nframes, int nbs, int nbc, int n, int nlags, int every, int nq, Waves q, int ntiles,
                                                        const double* __restrict__ pos, const double* __restrict__ vel,
                                                        const double* __restrict__ cpos, const double* __restrict__ cvel,
                                                        double* __restrict__ part)
{
    __shared__ double lds[kRows * (kWO + kWT)];
    double* sO = lds;
    double* sT = lds + kRows * kWO;
    const int tile = blockIdx.x % ntiles, lb = blockIdx.x / ntiles, b = blockIdx.y, lane = threadIdx.x;
    const int m0 = tile * kTile, mt = n - m0 < kTile ? n - m0 : kTile;
    const int rows = 3 * mt;
    const int L0 = lb * kLagBlock, lag = L0 + lane;
    const int last = nframes - 1;
    double a_msd = 0.0, a_mqd = 0.0, a_vacf = 0.0;
    double a_fs[NQC > 0 ? NQC : 1];
#pragma unroll
    for (int a = 0; a < (NQC > 0 ? NQC : 1); ++a) a_fs[a] = 0.0;

    for (int t0 = 0; t0 + L0 <= last; t0 += kChunk) {
        const int o0 = (t0 + every - 1) / every * every;                 // the chunk's first origin
        const int oend = t0 + kChunk < nframes - L0 ? t0 + kChunk : nframes - L0;   // an origin o has a lag of this block: o + L0 <= last
        if (o0 >= oend) continue;                                         // (the same in every thread)
        if (pos) {
            stage(sO, kWO, t0, kChunk, nframes, nbs, nbc, n, b, m0, rows, pos, cpos, lane);
            stage(sT, kWT, t0 + L0, kWindow, nframes, nbs, nbc, n, b, m0, rows, pos, cpos, lane);
            __syncthreads();
            for (int o = o0; o < oend; o += every) {
                const int fo = o - t0;
                const bool valid = lag < nlags && o + lag <= last;
                for (int m = 0; m < mt; ++m) {
                    const double* O = sO + 3 * m * kWO + fo;
                    const double* T = sT + 3 * m * kWT + fo + lane;
                    const double dx = T[0] - O[0], dy = T[kWT] - O[kWO], dz = T[2 * kWT] - O[2 * kWO];
                    const double d2 = __builtin_fma(dx, dx, __builtin_fma(dy, dy, dz * dz));
                    if (valid) {
                        a_msd += d2;
                        a_mqd = __builtin_fma(d2, d2, a_mqd);
                        if (NQC > 0) {
                            const double r = __builtin_sqrt(d2);
#pragma unroll
                            for (int a = 0; a < NQC; ++a)
                                if (a < nq) {
                                    const double x = q.v[a] * r;
                                    a_fs[a] += x == 0.0 ? 1.0 : sin(x) / x;
                                }
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (vel) {
            stage(sO, kWO, t0, kChunk, nframes, nbs, nbc, n, b, m0, rows, vel, cvel, lane);
            stage(sT, kWT, t0 + L0, kWindow, nframes, nbs, nbc, n, b, m0, rows, vel, cvel, lane);
            __syncthreads();
            for (int o = o0; o < oend; o += every) {
                const int fo = o - t0;
                const bool valid = lag < nlags && o + lag <= last;
                for (int m = 0; m < mt; ++m) {
                    const double* O = sO + 3 * m * kWO + fo;
                    const double* T = sT + 3 * m * kWT + fo + lane;
                    const double dot = __builtin_fma(O[0], T[0], __builtin_fma(O[kWO], T[kWT], O[2 * kWO] * T[2 * kWT]));
                    if (valid) a_vacf += dot;
                }
            }
            __syncthreads();
        }
    }
    if (lag < nlags) {
        const int K = kSums + nq;
        double* p = part + ((size_t)b * ntiles + tile) * K * nlags + lag;
        p[0] = a_msd;
        p[(size_t)nlags] = a_mqd;
        p[2 * (size_t)nlags] = a_vacf;
#pragma unroll
        for (int a = 0; a < NQC; ++a)
            if (a < nq) p[(size_t)(kSums + a) * nlags] = a_fs[a];
    }
}

// One thread per (box of the chunk, sum, lag): the tiles in order onto 0, one division by n_l.
__global__ __launch_bounds__(256) void k_tcf_reduce(int nbc, int n, int nframes, int nlags, int every, int nq, int ntiles,
                                                    const double* __restrict__ part, double* __restrict__ msd, double* __restrict__ mqd,
                                                    double* __restrict__ vacf, double* __restrict__ fs)
{
    const int K = kSums + nq;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (size_t)nbc * K * nlags) return;
    const int lag = (int)(id % nlags), k = (int)(id / nlags % K), b = (int)(id / nlags / K);
    double* out = k == 0 ? msd : k == 1 ? mqd : k == 2 ? vacf : fs;
    if (!out) return;
    double s = 0.0;
    for (int t = 0; t < ntiles; ++t) s += part[(((size_t)b * ntiles + t) * K + k) * nlags + lag];
    const double nl = (double)((nframes - 1 - lag) / every + 1) * (double)n;
    const double r = s / nl;
    if (k < kSums) out[(size_t)b * nlags + lag] = r;
    else out[((size_t)b * nlags + lag) * nq + (k - kSums)] = r;
}

// ---- the histograms: a workgroup per (slab of terms, selected lag, box of the chunk) ------------------------------------------
// LDS: edges [nedges] doubles | counters [nedges + 1]
__host__ __device__ constexpr size_t hist_lds(int nedges) { return up16(8 * (size_t)nedges) + 4 * ((size_t)nedges + 1); }

__global__ __launch_bounds__(kHistThreads) void k_tcf_hist(int nframes, int nbs, int nbc, int n, int every, int nedges, int nh,
                                                           const double* __restrict__ edges2, const int* __restrict__ hist_lags,
                                                           const double* __restrict__ pos, const double* __restrict__ cpos,
                                                           long long* __restrict__ hist)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    double* E = (double*)lds_raw;
    unsigned* cnt = (unsigned*)(lds_raw + up16(8 * (size_t)nedges));
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    for (int t = tid; t < nedges; t += kHistThreads) E[t] = edges2[t];
    for (int t = tid; t <= nedges; t += kHistThreads) cnt[t] = 0u;
    __syncthreads();
    const int lag = hist_lags[h];
    if (lag >= 0 && lag < nframes) {                                      // (the host has rejected any other; never index beyond the frames)
        const size_t items = (size_t)((nframes - 1 - lag) / every + 1) * n;
        const size_t stride = (size_t)gridDim.x * kHistThreads;
        for (size_t i = (size_t)blockIdx.x * kHistThreads + tid; i < items; i += stride) {
            const int j = (int)(i % n), o = (int)(i / n) * every;
            const double* x0 = pos + (((size_t)o * nbs + b) * n + j) * 3;
            const double* x1 = pos + (((size_t)(o + lag) * nbs + b) * n + j) * 3;
            double a0 = x0[0], a1 = x0[1], a2 = x0[2], b0 = x1[0], b1 = x1[1], b2 = x1[2];
            if (cpos) {
                const double* c0 = cpos + ((size_t)o * nbc + b) * 3;
                const double* c1 = cpos + ((size_t)(o + lag) * nbc + b) * 3;
                a0 = a0 - c0[0]; a1 = a1 - c0[1]; a2 = a2 - c0[2];
                b0 = b0 - c1[0]; b1 = b1 - c1[1]; b2 = b2 - c1[2];
            }
            const double dx = b0 - a0, dy = b1 - a1, dz = b2 - a2;
            const double d2 = __builtin_fma(dx, dx, __builtin_fma(dy, dy, dz * dz));
            int slot;
            if (d2 < E[0]) slot = 0;
            else if (!(d2 < E[nedges - 1])) slot = nedges;
            else {
                int lo = 0, hi = nedges - 1;                              // E[lo] <= d2 < E[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (E[mid] <= d2) lo = mid; else hi = mid;
                }
                slot = 1 + lo;
            }
            atomicAdd(cnt + slot, 1u);
        }
    }
    __syncthreads();
    unsigned long long* out = (unsigned long long*)hist + ((size_t)b * nh + h) * ((size_t)nedges + 1);
    for (int t = tid; t <= nedges; t += kHistThreads) {
        const unsigned v = cnt[t];
        if (v) atomicAdd(out + t, (unsigned long long)v);
    }
}

}  // namespace mwtcf

namespace {

using namespace mwtcf;

struct State : Runtime<4> {
    Buf scratch, verdict, edges, lags, pos, vel, msd, mqd, vacf, fs, hist;
    int last[MW_TCF_PLAN_FIELDS] = {0};
    float ms[3] = {0.0f, 0.0f, 0.0f};
} g;

struct Plan {
    int bpc, chunks, ntiles, nlb, lds;
    size_t part_bytes, com_bytes, per_box;
};

void plan_fields(const Plan& p, int* f)
{
    f[0] = p.bpc; f[1] = p.chunks; f[2] = kTile; f[3] = kLagBlock; f[4] = kChunk; f[5] = kWindow; f[6] = p.lds;
    f[7] = (int)(p.per_box > 0x7fffffffu ? 0x7fffffffu : p.per_box); f[8] = p.ntiles; f[9] = p.nlb;
}

// The scratch of one box: the tiles' partial sums [tile][3 + nq][nlags] and, under MW_TCF_REMOVE_COM, the centres of its
// positions and of its velocities [frame][3] (both, whether or not the call brings velocities).
int make_plan(const char* who, int nframes, int n, int nlags, int nq, int nedges, unsigned flags, int nboxes, size_t budget, Plan& p)
{
    p.ntiles = (n + kTile - 1) / kTile;
    p.nlb = (nlags + kLagBlock - 1) / kLagBlock;
    if ((long long)p.ntiles * p.nlb > 0x7fffffffLL)
        return fail("%s: nwater = %d and nlags = %d make %d tiles x %d lag blocks, beyond 2^31 - 1 workgroups of a box", who, n, nlags, p.ntiles, p.nlb);
    p.part_bytes = up16(8 * (size_t)p.ntiles * (kSums + nq) * nlags);
    p.com_bytes = (flags & MW_TCF_REMOVE_COM) ? up16(24 * (size_t)nframes) : 0;
    p.per_box = p.part_bytes + 2 * p.com_bytes;
    const size_t hl = nedges ? hist_lds(nedges) : 0;
    p.lds = (int)(hl > (size_t)kCorrLds ? hl : (size_t)kCorrLds);
    const size_t fit = budget / p.per_box;
    if (fit < 1)
        return fail("%s: one box needs %zu bytes of scratch (nframes = %d, nwater = %d, nlags = %d, nq = %d) and does not fit the budget of %zu "
                    "bytes (MW_TCF_SCRATCH_MB)", who, p.per_box, nframes, n, nlags, nq, budget);
    p.bpc = (int)(fit < (size_t)kMaxChunkBoxes ? fit : (size_t)kMaxChunkBoxes);
    if (p.bpc > nboxes) p.bpc = nboxes;
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

int check_counts(const char* who, int nframes, int nboxes, int n, int nlags, int every, int nq, int nedges, int nh, unsigned flags)
{
    if (nframes < 1 || nframes > kMaxFrames) return fail("%s: nframes = %d outside 1..%d", who, nframes, kMaxFrames);
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    if (n < 1 || n > kMaxWater) return fail("%s: nwater = %d outside 1..%d", who, n, kMaxWater);
    if (nlags < 1 || nlags > nframes) return fail("%s: nlags = %d outside 1..nframes = %d", who, nlags, nframes);
    if (every < 1) return fail("%s: origin_every = %d is not >= 1", who, every);
    if (nq < 0 || nq > kMaxQ) return fail("%s: nq = %d outside 0..%d", who, nq, kMaxQ);
    if (nedges != 0 && (nedges < 2 || nedges > kMaxEdges)) return fail("%s: nedges = %d is neither 0 nor in 2..%d", who, nedges, kMaxEdges);
    if (nh < 0 || nh > kMaxHistLags) return fail("%s: nh = %d outside 0..%d", who, nh, kMaxHistLags);
    if (flags & ~MW_TCF_REMOVE_COM) return fail("%s: flags = 0x%x has bits other than MW_TCF_REMOVE_COM", who, flags);
    return 0;
}

// what both compute entries can check on the host before they look at the library's state
int check_host_side(const char* who, int nframes, int nboxes, int n, const double* pos, const double* vel, int nlags, int every, int nq,
                    const double* q, int nedges, const double* edges2, int nh, const int* hist_lags, unsigned flags, const double* vacf,
                    const double* fs, const long long* hist)
{
    if (check_counts(who, nframes, nboxes, n, nlags, every, nq, nedges, nh, flags)) return 1;
    if (!pos) return fail("%s: pos is NULL", who);
    if (vacf && !vel) return fail("%s: vacf is asked for and vel is NULL", who);
    if (nq > 0 && !q) return fail("%s: q is NULL and nq = %d", who, nq);
    for (int a = 0; a < nq; ++a)
        if (!(q[a] > 0.0) || !std::isfinite(q[a])) return fail("%s: q[%d] = %g is not a finite wave number > 0", who, a, q[a]);
    if (fs && nq == 0) return fail("%s: fs is asked for and nq = 0", who);
    if (nedges > 0 && !edges2) return fail("%s: edges2 is NULL and nedges = %d", who, nedges);
    for (int m = 0; m < nedges; ++m)
        if (!std::isfinite(edges2[m])) return fail("%s: edges2[%d] = %g is not finite", who, m, edges2[m]);
    for (int m = 0; m + 1 < nedges; ++m)
        if (!(edges2[m] < edges2[m + 1]))
            return fail("%s: edges2[%d] = %.17g is not below edges2[%d] = %.17g (strictly ascending edges are required)", who, m, edges2[m],
                        m + 1, edges2[m + 1]);
    if (nh > 0 && !hist_lags) return fail("%s: hist_lags is NULL and nh = %d", who, nh);
    for (int h = 0; h < nh; ++h)
        if (hist_lags[h] < 0 || hist_lags[h] >= nlags) return fail("%s: hist_lags[%d] = %d outside 0..nlags - 1 = %d", who, h, hist_lags[h], nlags - 1);
    if (hist && nedges == 0) return fail("%s: hist is asked for and nedges = 0", who);
    if (hist && nh == 0) return fail("%s: hist is asked for and nh = 0 (hist_lags selects its lags)", who);
    Plan p;
    return make_plan(who, nframes, n, nlags, nq, nedges, flags, nboxes, g.live ? g.budget : kDefaultBudget, p);
}

int check_finite(const char* who, const char* name, int nframes, int nboxes, int n, const double* a)
{
    const size_t per_box = 3 * (size_t)n, count = (size_t)nframes * nboxes * per_box;
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(a[i]))
            return fail("%s: %s of molecule %zu of frame %zu of box %zu is not finite", who, name, i % per_box / 3, i / per_box / nboxes, i / per_box % nboxes);
    return 0;
}

int check_live(const char* who) { return check_live(who, "mw_tcf_init", g); }

template <int NQC>
void launch_corr(dim3 grid, int nframes, int nbs, int nbc, int n, int nlags, int every, int nq, const Waves& q, int ntiles, const double* pos,
                 const double* vel, const double* cpos, const double* cvel, double* part)
{
    hipLaunchKernelGGL(k_tcf_corr<NQC>, grid, dim3(kLagBlock), 0, g.stream, nframes, nbs, nbc, n, nlags, every, nq, q, ntiles, pos, vel, cpos, cvel, part);
}

// The work of both entries, arguments already checked; pos, vel and the outputs are device pointers.
int run(const char* who, int nframes, int nboxes, int n, const double* pos, const double* vel, int nlags, int every, int nq, const double* q,
        int nedges, const double* edges2, int nh, const int* hist_lags, unsigned flags, double* msd, double* mqd, double* vacf, double* fs,
        long long* hist)
{
    Plan p;
    if (make_plan(who, nframes, n, nlags, nq, nedges, flags, nboxes, g.budget, p)) return 1;
    if (every > nframes) every = nframes;                                 // the same single origin, and no overflow in the kernels' arithmetic
    if (!fs) nq = 0;
    const bool want_pos = msd || mqd || fs, want_vel = vacf != nullptr, com = (flags & MW_TCF_REMOVE_COM) != 0;
    if (!hist) nh = 0;
    if (!want_vel) vel = nullptr;
    Waves w;
    for (int a = 0; a < kMaxQ; ++a) w.v[a] = a < nq ? q[a] : 0.0;
    // (with fs NULL the partial sums have 3 rows; the plan's scratch, sized for 3 + nq, holds them)
    if (reserve(g.scratch, p.per_box * (size_t)p.bpc)) return 1;
    if (nh) {
        if (reserve(g.edges, 8 * (size_t)nedges) || reserve(g.lags, 4 * (size_t)nh)) return 1;
        HIPOK(hipMemcpyAsync(g.edges.p, edges2, 8 * (size_t)nedges, hipMemcpyHostToDevice, g.stream));
        HIPOK(hipMemcpyAsync(g.lags.p, hist_lags, 4 * (size_t)nh, hipMemcpyHostToDevice, g.stream));
    }
    const size_t box_doubles = 3 * (size_t)n, hist_box = (size_t)nh * ((size_t)nedges + 1);
    float ms[3] = {0.0f, 0.0f, 0.0f};
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const double* d_pos = pos + box_doubles * b0;
        const double* d_vel = vel ? vel + box_doubles * b0 : nullptr;
        double* part = (double*)g.scratch.p;
        double* cpos = com ? (double*)((char*)g.scratch.p + p.part_bytes * (size_t)p.bpc) : nullptr;
        double* cvel = com && d_vel ? (double*)((char*)cpos + p.com_bytes * (size_t)p.bpc) : nullptr;
        HIPOK(hipEventRecord(g.ev[0], g.stream));
        if (com && (want_pos || nh)) {
            hipLaunchKernelGGL(k_tcf_com, dim3((unsigned)nframes, (unsigned)nb), dim3(64), 0, g.stream, nboxes, nb, n, d_pos, cpos);
            HIPOK(hipGetLastError());
        }
        if (cvel) {
            hipLaunchKernelGGL(k_tcf_com, dim3((unsigned)nframes, (unsigned)nb), dim3(64), 0, g.stream, nboxes, nb, n, d_vel, cvel);
            HIPOK(hipGetLastError());
        }
        HIPOK(hipEventRecord(g.ev[1], g.stream));
        if (want_pos || want_vel) {
            const dim3 grid((unsigned)(p.ntiles * p.nlb), (unsigned)nb);
            const double* kp = want_pos ? d_pos : nullptr;
            if (nq == 0) launch_corr<0>(grid, nframes, nboxes, nb, n, nlags, every, nq, w, p.ntiles, kp, d_vel, cpos, cvel, part);
            else if (nq <= 4) launch_corr<4>(grid, nframes, nboxes, nb, n, nlags, every, nq, w, p.ntiles, kp, d_vel, cpos, cvel, part);
            else launch_corr<kMaxQ>(grid, nframes, nboxes, nb, n, nlags, every, nq, w, p.ntiles, kp, d_vel, cpos, cvel, part);
            HIPOK(hipGetLastError());
        }
        if (nh) {
            long long* d_hist = hist + hist_box * b0;
            HIPOK(hipMemsetAsync(d_hist, 0, 8 * hist_box * nb, g.stream));
            const size_t items = (size_t)nframes * n;                     // (of lag 0 with every frame an origin: the most a lag has)
            size_t slabs = (items + kHistSlabItems - 1) / kHistSlabItems;
            if (slabs > (size_t)kMaxSlabs) slabs = kMaxSlabs;              // then a workgroup counts at most 2^42 / 65535 < 2^32 terms
            hipLaunchKernelGGL(k_tcf_hist, dim3((unsigned)slabs, (unsigned)nh, (unsigned)nb), dim3(kHistThreads), hist_lds(nedges), g.stream, nframes,
                               nboxes, nb, n, every, nedges, nh, (const double*)g.edges.p, (const int*)g.lags.p, d_pos, cpos, d_hist);
            HIPOK(hipGetLastError());
        }
        HIPOK(hipEventRecord(g.ev[2], g.stream));
        if (want_pos || want_vel) {
            const size_t threads = (size_t)nb * (kSums + nq) * nlags;
            hipLaunchKernelGGL(k_tcf_reduce, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, g.stream, nb, n, nframes, nlags, every, nq, p.ntiles,
                               part, msd ? msd + (size_t)nlags * b0 : nullptr, mqd ? mqd + (size_t)nlags * b0 : nullptr,
                               vacf ? vacf + (size_t)nlags * b0 : nullptr, fs ? fs + (size_t)nlags * nq * b0 : nullptr);
            HIPOK(hipGetLastError());
        }
        HIPOK(hipEventRecord(g.ev[3], g.stream));
        HIPOK(hipStreamSynchronize(g.stream));                              // the next chunk reuses the scratch
        for (int k = 0; k < 3; ++k) {
            float t = 0.0f;
            HIPOK(hipEventElapsedTime(&t, g.ev[k], g.ev[k + 1]));
            ms[k] += t;
        }
    }
    plan_fields(p, g.last);
    g.have_last = true;
    for (int k = 0; k < 3; ++k) g.ms[k] = ms[k];
    return 0;
}

// The first element of a device array that is not finite, by one kernel that writes nothing but its verdict.
int check_device_array(const char* who, const char* name, int nframes, int nboxes, int n, const double* a)
{
    const size_t per_box = 3 * (size_t)n, count = (size_t)nframes * nboxes * per_box;
    if (reserve(g.verdict, sizeof(unsigned long long))) return 1;
    unsigned long long v = kNoVerdict;
    HIPOK(hipMemcpyAsync(g.verdict.p, &v, sizeof v, hipMemcpyHostToDevice, g.stream));
    size_t blocks = (count + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_tcf_check, dim3((unsigned)blocks), dim3(256), 0, g.stream, count, a, (unsigned long long*)g.verdict.p);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(&v, g.verdict.p, sizeof v, hipMemcpyDeviceToHost, g.stream));
    HIPOK(hipStreamSynchronize(g.stream));
    if (v != kNoVerdict)
        return fail("%s: %s of molecule %zu of frame %zu of box %zu is not finite", who, name, (size_t)(v % per_box / 3), (size_t)(v / per_box / nboxes),
                    (size_t)(v / per_box % nboxes));
    return 0;
}

}  // namespace

extern "C" {

const char* mw_tcf_last_error(void) { return g_err; }
int mw_tcf_is_initialised(void) { return g.live ? 1 : 0; }

int mw_tcf_init(int device) { return runtime_init("mw_tcf_init", "MW_TCF_SCRATCH_MB", device, g); }

int mw_tcf_finalize(void)
{
    if (runtime_finalize(g, {&g.scratch, &g.verdict, &g.edges, &g.lags, &g.pos, &g.vel, &g.msd, &g.mqd, &g.vacf, &g.fs, &g.hist})) return 1;
    g = State{};
    return 0;
}

int mw_tcf_compute(int nframes, int nboxes, int nwater, const double* pos, const double* vel, int nlags, int origin_every, int nq, const double* q,
                   int nedges, const double* edges2, int nh, const int* hist_lags, unsigned flags, double* msd, double* mqd, double* vacf,
                   double* fs, long long* hist)
{
    const char* who = "mw_tcf_compute";
    if (check_host_side(who, nframes, nboxes, nwater, pos, vel, nlags, origin_every, nq, q, nedges, edges2, nh, hist_lags, flags, vacf, fs, hist)) return 1;
    if (check_finite(who, "pos", nframes, nboxes, nwater, pos)) return 1;
    if (vel && check_finite(who, "vel", nframes, nboxes, nwater, vel)) return 1;
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    const size_t traj = 24 * (size_t)nframes * nboxes * nwater, curve = 8 * (size_t)nboxes * nlags;
    const size_t hist_bytes = 8 * (size_t)nboxes * nh * ((size_t)nedges + 1);
    const bool use_vel = vel && vacf;
    if (reserve(g.pos, traj)) return 1;
    if (use_vel && reserve(g.vel, traj)) return 1;
    if (msd && reserve(g.msd, curve)) return 1;
    if (mqd && reserve(g.mqd, curve)) return 1;
    if (vacf && reserve(g.vacf, curve)) return 1;
    if (fs && reserve(g.fs, curve * nq)) return 1;
    if (hist && reserve(g.hist, hist_bytes)) return 1;
    HIPOK(hipMemcpyAsync(g.pos.p, pos, traj, hipMemcpyHostToDevice, g.stream));
    if (use_vel) HIPOK(hipMemcpyAsync(g.vel.p, vel, traj, hipMemcpyHostToDevice, g.stream));
    if (run(who, nframes, nboxes, nwater, (const double*)g.pos.p, use_vel ? (const double*)g.vel.p : nullptr, nlags, origin_every, nq, q, nedges, edges2,
            nh, hist_lags, flags, msd ? (double*)g.msd.p : nullptr, mqd ? (double*)g.mqd.p : nullptr, vacf ? (double*)g.vacf.p : nullptr,
            fs ? (double*)g.fs.p : nullptr, hist ? (long long*)g.hist.p : nullptr))
        return 1;
    if (msd) HIPOK(hipMemcpyAsync(msd, g.msd.p, curve, hipMemcpyDeviceToHost, g.stream));
    if (mqd) HIPOK(hipMemcpyAsync(mqd, g.mqd.p, curve, hipMemcpyDeviceToHost, g.stream));
    if (vacf) HIPOK(hipMemcpyAsync(vacf, g.vacf.p, curve, hipMemcpyDeviceToHost, g.stream));
    if (fs) HIPOK(hipMemcpyAsync(fs, g.fs.p, curve * nq, hipMemcpyDeviceToHost, g.stream));
    if (hist) HIPOK(hipMemcpyAsync(hist, g.hist.p, hist_bytes, hipMemcpyDeviceToHost, g.stream));
    HIPOK(hipStreamSynchronize(g.stream));
    return 0;
}

int mw_tcf_compute_device(int nframes, int nboxes, int nwater, const double* pos, const double* vel, int nlags, int origin_every, int nq,
                          const double* q, int nedges, const double* edges2, int nh, const int* hist_lags, unsigned flags, double* msd, double* mqd,
                          double* vacf, double* fs, long long* hist)
{
    const char* who = "mw_tcf_compute_device";
    if (check_host_side(who, nframes, nboxes, nwater, pos, vel, nlags, origin_every, nq, q, nedges, edges2, nh, hist_lags, flags, vacf, fs, hist)) return 1;
    if (check_live(who)) return 1;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    HIPOK(hipDeviceSynchronize());                                          // work queued before the call is waited for
    if (check_device_array(who, "pos", nframes, nboxes, nwater, pos)) return 1;
    if (vel && check_device_array(who, "vel", nframes, nboxes, nwater, vel)) return 1;
    return run(who, nframes, nboxes, nwater, pos, vel, nlags, origin_every, nq, q, nedges, edges2, nh, hist_lags, flags, msd, mqd, vacf, fs, hist);
}

int mw_tcf_plan(int nframes, int nwater, int nlags, int nq, int nedges, unsigned flags, int nboxes, int* out, int nout)
{
    const char* who = "mw_tcf_plan";
    if (check_counts(who, nframes, nboxes, nwater, nlags, 1, nq, nedges, 0, flags)) return 1;
    Plan p;
    if (make_plan(who, nframes, nwater, nlags, nq, nedges, flags, nboxes, g.live ? g.budget : kDefaultBudget, p)) return 1;
    int f[MW_TCF_PLAN_FIELDS];
    plan_fields(p, f);
    copy_fields(f, MW_TCF_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_tcf_last(int* out, int nout)
{
    if (check_live("mw_tcf_last")) return 1;
    if (!g.have_last) return fail("mw_tcf_last: no call has launched yet");
    copy_fields(g.last, MW_TCF_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_tcf_elapsed_ms(float* centre, float* correlate, float* reduce)
{
    if (check_live("mw_tcf_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_tcf_elapsed_ms: no call has launched yet");
    if (centre) *centre = g.ms[0];
    if (correlate) *correlate = g.ms[1];
    if (reduce) *reduce = g.ms[2];
    return 0;
}

}  // extern "C"
