// mom_gather.hip -- what a random 80-byte record read costs in fetched bytes and in time, at the plain 80-byte stride of the moment
// records (kMomStride, mw_common.hip.h) and packed three to 256 bytes (records at byte offsets 0, 80, 160 of their trio: one in three
// straddles a 128-byte line instead of four in eight): the calibration of FETCH_SIZE for the moment reads of k_move_energy, and the
// measurement behind profiles/r13_summary.md's account of the packed layout.  Stand-alone: nothing of the engine is linked.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/mom_gather tools/mom_gather.hip
//   tools/mom_gather plain|packed [reads in millions, default 16] [records in the table, default 2097152]
//   rocprofv3 --pmc FETCH_SIZE -d <dir> -- tools/mom_gather packed        (one counter run per layout, each a run of its own; two
//                                                                           dispatches show: a one-workgroup warm-up, then the launch)
//
// Every lane reads one record as five 16-byte loads (as load_moments does) at a random molecule of the table -- 2 097 152 records are
// 168 MB plain, 179 MB packed: far beyond L2 and most of the memory-side cache's reach for uniformly random reads -- and adds the ten
// doubles up; one launch, `reads` lanes.  Prints the launch's time and the bytes per read a line-granular fetch would need (lines
// touched x 128), to set beside FETCH_SIZE x 1024 / reads from the counter run.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// first double of record j, doubles of a table of n records
template <bool PACKED> __host__ __device__ constexpr size_t rec_offset(unsigned j) { return PACKED ? (size_t)(10u * j + 2u * (j / 3u)) : (size_t)(10u * j); }
template <bool PACKED> __host__ __device__ constexpr size_t table_doubles(size_t n) { return PACKED ? (n + 2) / 3 * 32 : n * 10; }

template <bool PACKED>
__global__ __launch_bounds__(256) void k_gather(const double* __restrict__ table, unsigned nrec, unsigned long long nreads, double* __restrict__ out)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    double s = 0.0;
    if (t < nreads) {
        unsigned long long h = (t + 1ull) * 0x9E3779B97F4A7C15ull;             // splitmix64: a molecule of the table, uniformly
        h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 27; h *= 0x94D049BB133111EBull; h ^= h >> 31;
        const unsigned j = (unsigned)(h % nrec);                                // < nrec: inside the table
        const double2* m2 = reinterpret_cast<const double2*>(table + rec_offset<PACKED>(j));
#pragma unroll
        for (int c = 0; c < 5; ++c) { const double2 v = m2[c]; s += v.x + v.y; }
    }
    if (s == 12345.678) out[0] = s;                                             // (never: the table holds ones)
}

int main(int argc, char** argv)
{
    if (argc < 2 || (std::strcmp(argv[1], "plain") != 0 && std::strcmp(argv[1], "packed") != 0)) {
        std::fprintf(stderr, "usage: mom_gather plain|packed [reads, millions] [records]\n");
        return 2;
    }
    const bool packed = std::strcmp(argv[1], "packed") == 0;
    const unsigned long long nreads = (unsigned long long)((argc > 2 ? std::atof(argv[2]) : 16.0) * 1e6);
    const unsigned nrec = argc > 3 ? (unsigned)std::atol(argv[3]) : 2097152u;
    if (nrec < 3u || nrec > (1u << 22) || nreads < 1ull || nreads > 4000000000ull) { std::fprintf(stderr, "mom_gather: arguments out of range\n"); return 2; }
    const size_t doubles = packed ? table_doubles<true>(nrec) : table_doubles<false>(nrec);
    double *table = nullptr, *out = nullptr;
    CHK(hipMalloc(&table, doubles * sizeof(double)));
    CHK(hipMalloc(&out, sizeof(double)));
    { std::vector<double> ones(doubles, 1.0); CHK(hipMemcpy(table, ones.data(), doubles * sizeof(double), hipMemcpyHostToDevice)); }
    // lines a read touches, on the host, over the same molecules
    double lines = 0.0;
    for (unsigned long long t = 0; t < nreads; t += 97ull) {
        unsigned long long h = (t + 1ull) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 27; h *= 0x94D049BB133111EBull; h ^= h >> 31;
        const size_t b = 8 * (packed ? rec_offset<true>((unsigned)(h % nrec)) : rec_offset<false>((unsigned)(h % nrec)));
        lines += (double)((b + 79) / 128 - b / 128 + 1);
    }
    lines /= (double)((nreads + 96ull) / 97ull);
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    const unsigned grid = (unsigned)((nreads + 255ull) / 256ull);
    auto launch = [&]() { if (packed) hipLaunchKernelGGL(k_gather<true>, dim3(grid), dim3(256), 0, 0, table, nrec, nreads, out);
                          else        hipLaunchKernelGGL(k_gather<false>, dim3(grid), dim3(256), 0, 0, table, nrec, nreads, out); };
    // warm-up (code object load): ONE workgroup, 256 reads -- it leaves nothing of the table in the memory-side cache, and under
    // --pmc its dispatch (grid 256) is the one to skip: read the counters of the second dispatch, the timed launch
    if (packed) hipLaunchKernelGGL(k_gather<true>, dim3(1), dim3(256), 0, 0, table, nrec, 256ull, out);
    else        hipLaunchKernelGGL(k_gather<false>, dim3(1), dim3(256), 0, 0, table, nrec, 256ull, out);
    CHK(hipDeviceSynchronize());
    CHK(hipEventRecord(e0, 0));
    launch();
    CHK(hipEventRecord(e1, 0));
    CHK(hipEventSynchronize(e1));
    CHK(hipGetLastError());
    float ms = 0.0f;
    CHK(hipEventElapsedTime(&ms, e0, e1));
    std::printf("{\"layout\": \"%s\", \"records\": %u, \"table_MB\": %.1f, \"reads\": %llu, \"ms\": %.4f, \"lines_per_read\": %.4f, \"line_bytes_per_read\": %.1f, \"Mreads_per_s\": %.0f}\n",
                argv[1], nrec, doubles * 8.0 / 1e6, nreads, ms, lines, 128.0 * lines, nreads / ms / 1e3);
    CHK(hipFree(table)); CHK(hipFree(out));
    return 0;
}
