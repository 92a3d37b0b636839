// sc_genie_bin.hip -- the genie construction for binary memoryless channels as one device pipeline
// (gfx950) + C-ABI: genieEncodeDecodeSimulation (BinaryPolarEncoderDecoder.py:390-491) with the
// untrusted statistic (trustXYProbs = False, :159-171) under a uniform prior, chunk by chunk on one
// stream:
//   pcub_mc_info (K = N)            the trial's u                                  (sc_mc.hip)
//   pcub_polar_encode_bin           x = polar transform of u (no frozen position)  (sc_util.hip)
//   pcub_mc_channel_norm_tiled      compact normalised rows, tile = 1: [B][N]      (sc_mc.hip)
//   k_sc_genie_bin                  breadth-first decode with u known, leaves classified and counted
//                                   in the kernel                                  (genie_bin_body.h)
// Trial g's draws depend only on (seed, g) (mc_rng.h) and the counts are integers, so any sharding
// or chunking of [offset, offset + count) gives the same counters.
//
// The kernel: a workgroup a trial, its work items over each level's N / 2 pairs, the level, the
// re-encoding bits and the wrong / tie counts in the workgroup's LDS (gb_lds_bytes).  Trials come
// from a static stride over a resident grid (every trial costs the same); the counts stay in LDS
// over all of a workgroup's trials and are flushed once, one 64-bit atomic a non-zero count.
// Root rows are per-trial rows, [B][N][2] raw pairs or [B][N] compact values: a trial's row is one
// contiguous run and pass 1 reads it in address order.
#include <hip/hip_runtime.h>

#include <cmath>

#include "genie_bin_body.h"
#include "polarcub_sc.h"

using namespace pcub;

namespace {

constexpr size_t kGbLdsPerCu = 160 * 1024;
constexpr long long kGbMaxLaunch = 1ll << 30;  // trials a launch: a workgroup's u32 counts cannot wrap

struct GbArgs {
    const double* rows;  // [B][N][2] raw pairs, or [B][N] compact
    const uint32_t* u;   // [ceil(N/32)][B]
    long long B;
    int n;
    unsigned long long* counters;  // [1 + 2N]
    double* leaf;                  // [N][B] or null
};

// run a phase on this work item, then make its LDS writes visible to the workgroup; a workgroup
// of one wave fences and meets only itself (sc_genie_prior.hip's GpWaveRun)
template <int BLOCK>
struct GbRun {
    int lane;
    template <class F>
    __device__ __forceinline__ void operator()(F&& f) const {
        f(lane);
        if (BLOCK == 64) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        } else {
            __syncthreads();
        }
    }
};

// Dynamic LDS: V [N] f64, cw [N] u32, ct [N] u32, E [2 nw] u32 (gb_lds_bytes(n) bytes).
template <bool COMPACT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_sc_genie_bin(GbArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gb_lds[];
    const int N = 1 << A.n;
    double* V = reinterpret_cast<double*>(gb_lds);
    uint32_t* cw = reinterpret_cast<uint32_t*>(V + N);
    uint32_t* ct = cw + N;
    uint32_t* E = ct + N;
    const int lane = (int)threadIdx.x;
    const GbRun<BLOCK> run{lane};
    run([&](int l) {
        for (int i = l; i < N; i += BLOCK) cw[i] = ct[i] = 0u;
    });
    const long long row = COMPACT ? (long long)N : 2ll * N;
    for (long long b = blockIdx.x; b < A.B; b += gridDim.x) {
        GbTrial T;
        T.row = A.rows + b * row;
        T.u = A.u + b;
        T.ustride = A.B;
        T.leaf = A.leaf ? A.leaf + b : nullptr;
        T.lstride = A.B;
        genie_bin_trial<COMPACT>(run, BLOCK, A.n, T, V, E, cw, ct);
    }
    // every phase ended with a barrier: the counts are visible to the whole workgroup
    for (int i = lane; i < N; i += BLOCK) {
        if (cw[i]) atomicAdd(&A.counters[1 + i], (unsigned long long)cw[i]);
        if (ct[i]) atomicAdd(&A.counters[1 + N + i], (unsigned long long)ct[i]);
    }
    if (blockIdx.x == 0 && lane == 0) atomicAdd(&A.counters[0], (unsigned long long)A.B);
}

// Work items a workgroup for length 2^n: a level has N / 2 pairs and a workgroup holds 16 N bytes
// of LDS, so the wave count follows N to keep the CU's SIMDs occupied by the few workgroups its
// LDS admits (DESIGN 3.3 has the measurement).
int gb_default_block(int n) { return n <= 8 ? 64 : (n <= 11 ? 256 : 1024); }

template <bool COMPACT, int BLOCK>
int gb_launch(GbArgs A, hipStream_t stream) {
    int dev = 0, cus = 0, occ = 0;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorNoDevice;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return (int)hipErrorNoDevice;
    const size_t lds = (size_t)gb_lds_bytes(A.n);
    if (lds > kGbLdsPerCu) return PCUB_EINVAL;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sc_genie_bin<COMPACT, BLOCK>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_sc_genie_bin<COMPACT, BLOCK>, BLOCK, lds) != hipSuccess ||
        occ < 1)
        return (int)hipErrorLaunchOutOfResources;  // no resident workgroup: nothing is launched
    const long long res = (long long)cus * occ;
    const long long grid = A.B < res ? A.B : res;
    hipLaunchKernelGGL((k_sc_genie_bin<COMPACT, BLOCK>), dim3((unsigned)grid), dim3(BLOCK), lds, stream, A);
    return (int)hipGetLastError();
}

template <bool COMPACT>
int gb_dispatch(const GbArgs& A, int block, hipStream_t stream) {
    switch (block) {
        case 64: return gb_launch<COMPACT, 64>(A, stream);
        case 256: return gb_launch<COMPACT, 256>(A, stream);
        case 1024: return gb_launch<COMPACT, 1024>(A, stream);
    }
    return PCUB_EINVAL;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// a chunk's buffers and the constant masks; past the kernel's lengths the composed route's pairs,
// leaves and leaf-kernel scratch as well
struct GbLayout {
    size_t u, x, rows, leaf, lws, lws_bytes, zeros, ones, total;
};

bool gb_sizable(int64_t chunk, int32_t n) {
    if (chunk <= 0 || n < 1 || n > 20) return false;
    return chunk <= (((int64_t)1 << 60) >> (n + 5));
}

// false when the composed route's scratch cannot be sized (no device)
bool gb_layout(int64_t chunk, int32_t n, GbLayout& L) {
    const size_t N = (size_t)1 << n, nw = (N + 31) / 32, c = (size_t)chunk;
    const bool fused = n <= kGbMaxLog2N;
    L.u = 0;
    L.x = L.u + align256(nw * c * 4);
    L.rows = L.x + align256(nw * c * 4);
    L.leaf = L.rows + align256(N * c * (fused ? 8 : 16));
    L.lws = L.leaf + (fused ? 0 : align256(N * c * 8));
    L.lws_bytes = fused ? 0 : pcub_sc_leaf_bin_workspace(chunk, n);
    if (!fused && L.lws_bytes == 0) return false;
    L.zeros = L.lws + align256(L.lws_bytes);
    L.ones = L.zeros + align256(nw * 4);
    L.total = L.ones + align256(nw * 4);
    return true;
}

bool gb_param_ok(int32_t channel, double param) {
    if (!std::isfinite(param)) return false;
    if (channel == 0) return param > 0.0;
    if (channel == 1) return param >= 0.0 && param <= 1.0;
    return false;
}

}  // namespace

extern "C" int pcub_sc_genie_bin_supported(int32_t log2N) { return log2N >= 1 && log2N <= kGbMaxLog2N ? 1 : 0; }

extern "C" int pcub_sc_genie_bin_geom(const double* rows, int32_t compact, const uint32_t* u_words, int64_t B,
                                      int32_t log2N, int32_t block, uint64_t* counters, double* leaf, void* stream) {
    if (log2N < 1 || log2N > kGbMaxLog2N || B < 0 || B > kGbMaxLaunch || !rows || !u_words || !counters)
        return PCUB_EINVAL;
    if (block != 0 && block != 64 && block != 256 && block != 1024) return PCUB_EINVAL;
    if (B == 0) return 0;
    GbArgs A;
    A.rows = rows;
    A.u = u_words;
    A.B = B;
    A.n = log2N;
    A.counters = (unsigned long long*)counters;
    A.leaf = leaf;
    if (block == 0) block = gb_default_block(log2N);
    return compact ? gb_dispatch<true>(A, block, (hipStream_t)stream) : gb_dispatch<false>(A, block, (hipStream_t)stream);
}

extern "C" int pcub_sc_genie_bin(const double* rows, int32_t compact, const uint32_t* u_words, int64_t B,
                                 int32_t log2N, uint64_t* counters, double* leaf, void* stream) {
    return pcub_sc_genie_bin_geom(rows, compact, u_words, B, log2N, 0, counters, leaf, stream);
}

extern "C" size_t pcub_mc_genie_bin_workspace(int64_t chunk, int32_t log2N) {
    GbLayout L;
    if (!gb_sizable(chunk, log2N) || !gb_layout(chunk, log2N, L)) return 0;
    return L.total;
}

extern "C" int pcub_mc_genie_bin(uint64_t seed, int64_t offset, int64_t count, int32_t log2N, int32_t channel,
                                 double param, int64_t chunk, uint64_t* counters, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (count < 0 || offset < 0 || !counters || !workspace || !gb_sizable(chunk, log2N)) return PCUB_EINVAL;
    if (!gb_param_ok(channel, param) || chunk > kGbMaxLaunch) return PCUB_EINVAL;
    GbLayout L;
    if (!gb_layout(chunk, log2N, L) || workspace_bytes < L.total) return PCUB_EINVAL;
    if (count == 0) return 0;
    const bool fused = log2N <= kGbMaxLog2N;
    char* ws = (char*)workspace;
    uint32_t* u = (uint32_t*)(ws + L.u);
    uint32_t* x = (uint32_t*)(ws + L.x);
    double* rows = (double*)(ws + L.rows);
    double* leaf = (double*)(ws + L.leaf);
    uint32_t* zeros = (uint32_t*)(ws + L.zeros);
    uint32_t* all = (uint32_t*)(ws + L.ones);
    const hipStream_t ms = (hipStream_t)stream;
    const int32_t N = 1 << log2N;
    const size_t nw = ((size_t)N + 31) / 32;
    // the encoder's mask (no position frozen; also every frozen value) and the leaf decode's (all of them)
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)zeros, 0, nw, ms);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetD32Async((hipDeviceptr_t)all, N >= 32 ? -1 : (int)((1u << N) - 1u), nw, ms);
    if (e != hipSuccess) return (int)e;
    int rc = 0;
    for (int64_t c0 = 0; !rc && c0 < count; c0 += chunk) {
        const int64_t B = (count - c0) < chunk ? (count - c0) : chunk;
        if ((rc = pcub_mc_info(seed, offset + c0, B, N, u, ms))) break;
        if ((rc = pcub_polar_encode_bin(u, B, log2N, zeros, zeros, N, x, ms))) break;
        if (fused) {
            if ((rc = pcub_mc_channel_norm_tiled(seed, offset + c0, B, log2N, channel, param, x, rows, 1, 1, ms))) break;
            rc = pcub_sc_genie_bin(rows, 1, u, B, log2N, counters, nullptr, ms);
        } else {
            if ((rc = pcub_mc_channel_norm(seed, offset + c0, B, log2N, channel, param, x, rows, 0, ms))) break;
            if ((rc = pcub_sc_leaf_bin(rows, B, log2N, all, nullptr, u, 0, nullptr, nullptr, leaf, ws + L.lws,
                                       L.lws_bytes, ms)))
                break;
            rc = pcub_genie_count(leaf, u, B, log2N, counters, ms);
        }
    }
    return rc;
}
