// sc_genie.hip -- the genie construction for the deletion channel as one device pipeline (gfx950)
// + C-ABI: genieEncodeDecodeSimulation (BinaryPolarEncoderDecoder.py:390-491) with the untrusted
// statistic (trustXYProbs = False, :159-171), chunk by chunk on one stream:
//   pcub_mc_info (K = N)        the trial's u                                    (sc_mc.hip)
//   pcub_polar_encode_bin       x = polar transform of u (no frozen position)    (sc_util.hip)
//   pcub_mc_deletion            guard bands + deletion channel                   (sc_mc.hip)
//   pcub_sc_leaf_deletion       every position frozen to the trial's u, every leaf exported (sc_del.hip)
//   pcub_genie_count            wrong / tie counts a position                    (genie_body.h)
// Trial g's draws depend only on (seed, g) (mc_rng.h) and the counts are integers, so any sharding
// or chunking of [offset, offset + count) gives the same counters.
#include <hip/hip_runtime.h>

#include "genie_body.h"
#include "polarcub_sc.h"

using namespace pcub;

namespace {

constexpr int kGenieBlock = 256;
constexpr int kGenieWave = 64;

// A workgroup takes the position rows blockIdx.x, + gridDim.x, .. and of each row the codeword
// sweeps blockIdx.y, + gridDim.y, .. (a sweep: blockDim.x consecutive codewords, a lane each; the
// leaf row and the u word row are codeword-minor, so a wave loads 512 and 256 contiguous bytes).
// A wave's classes are two ballots; their popcounts add up in wave-uniform integers over the
// sweeps, and lane 0 adds each non-zero sum to its counter with one 64-bit atomic.  The trip
// counts are wave-uniform (b0 does not depend on the lane), so every ballot sees the whole wave.
__global__ __launch_bounds__(kGenieBlock) void k_genie_count(const double* __restrict__ leaf,
                                                              const uint32_t* __restrict__ u_words, long long B,
                                                              long long N, unsigned long long* counters) {
    const int lane = threadIdx.x & (kGenieWave - 1);
    const long long first = (long long)blockIdx.y * blockDim.x + (threadIdx.x - lane);
    const long long step = (long long)gridDim.y * blockDim.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(&counters[0], (unsigned long long)B);
    for (long long i = blockIdx.x; i < N; i += gridDim.x) {
        unsigned long long wrong = 0, tie = 0;
        for (long long b0 = first; b0 < B; b0 += step) {
            const long long b = b0 + lane;
            const int c = b < B ? genie_class_at(leaf, u_words, B, i, b) : kGenieCorrect;
            wrong += (unsigned long long)__popcll(__ballot(c == kGenieWrong));
            tie += (unsigned long long)__popcll(__ballot(c == kGenieTie));
        }
        if (lane == 0) {
            if (wrong) atomicAdd(&counters[1 + i], wrong);
            if (tie) atomicAdd(&counters[1 + N + i], tie);
        }
    }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// a chunk's buffers and the two constant masks
struct GLayout {
    size_t u, x, rx, len, leaf, zeros, ones, total;
};

GLayout g_layout(int64_t chunk, int32_t n, int32_t W) {
    GLayout L;
    const size_t N = (size_t)1 << n, nw = (N + 31) / 32, c = (size_t)chunk;
    L.u = 0;
    L.x = L.u + align256(nw * c * 4);
    L.rx = L.x + align256(nw * c * 4);
    L.len = L.rx + align256((size_t)W * c);
    L.leaf = L.len + align256(c * 4);
    L.zeros = L.leaf + align256(N * c * 8);
    L.ones = L.zeros + align256(nw * 4);
    L.total = L.ones + align256(nw * 4);
    return L;
}

// sizes g_layout can add up without overflow: 16 N chunk and W chunk below 2^60 (W: at most the
// deletion decode's longest row, 2^24 symbols)
bool g_sizable(int64_t chunk, int32_t n, int32_t W) {
    if (chunk <= 0 || n < 1 || n > 24 || W <= 0 || W > (1 << 24)) return false;
    return chunk <= (((int64_t)1 << 60) >> (n + 4)) && chunk <= ((int64_t)1 << 60) / W;
}

}  // namespace

extern "C" int pcub_genie_count(const double* leaf, const uint32_t* u_words, int64_t B, int32_t log2N,
                                uint64_t* counters, void* stream) {
    if (!leaf || !u_words || !counters || B < 0 || log2N < 1 || log2N > 24) return PCUB_EINVAL;
    if (B == 0) return 0;
    const long long N = 1LL << log2N;
    const int block = B <= 64 ? 64 : (B <= 128 ? 128 : kGenieBlock);
    // sixteen sweeps a workgroup where the batch is long, and about 2^20 workgroups at the most
    const long long gx = N < 65536 ? N : 65536;
    long long gy = (B + 16LL * block - 1) / (16LL * block);
    if (gy > (1 << 20) / gx) gy = (1 << 20) / gx;
    if (gy > 65535) gy = 65535;
    if (gy < 1) gy = 1;
    hipLaunchKernelGGL(k_genie_count, dim3((unsigned)gx, (unsigned)gy), dim3(block), 0, (hipStream_t)stream, leaf,
                       u_words, (long long)B, N, (unsigned long long*)counters);
    return (int)hipGetLastError();
}

extern "C" size_t pcub_mc_genie_deletion_workspace(int64_t chunk, int32_t n, int32_t W) {
    if (!g_sizable(chunk, n, W)) return 0;
    return g_layout(chunk, n, W).total;
}

extern "C" int pcub_mc_genie_deletion(uint64_t seed, int64_t offset, int64_t count, int32_t n, int32_t n0,
                                      const int32_t* tmpl, int32_t W, int32_t ones, double pd, int64_t chunk,
                                      uint64_t* counters, void* workspace, size_t workspace_bytes, void* stream) {
    if (count < 0 || offset < 0 || !counters || !tmpl || !g_sizable(chunk, n, W)) return PCUB_EINVAL;
    if (!pcub_sc_leaf_deletion_supported(n, n0, ones) || !(pd >= 0.0 && pd <= 1.0)) return PCUB_EINVAL;
    const GLayout L = g_layout(chunk, n, W);
    if (!workspace || workspace_bytes < L.total) return PCUB_EINVAL;
    if (count == 0) return 0;
    char* ws = (char*)workspace;
    uint32_t* u = (uint32_t*)(ws + L.u);
    uint32_t* x = (uint32_t*)(ws + L.x);
    uint8_t* rx = (uint8_t*)(ws + L.rx);
    int32_t* len = (int32_t*)(ws + L.len);
    double* leaf = (double*)(ws + L.leaf);
    uint32_t* zeros = (uint32_t*)(ws + L.zeros);
    uint32_t* all = (uint32_t*)(ws + L.ones);
    const hipStream_t ms = (hipStream_t)stream;
    const int32_t N = 1 << n;
    const size_t nw = ((size_t)N + 31) / 32;
    // the encoder's mask (no position frozen; also every frozen value) and the decoder's (all of them)
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)zeros, 0, nw, ms);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetD32Async((hipDeviceptr_t)all, N >= 32 ? -1 : (int)((1u << N) - 1u), nw, ms);
    if (e != hipSuccess) return (int)e;
    int rc = 0;
    for (int64_t c0 = 0; !rc && c0 < count; c0 += chunk) {
        const int64_t B = (count - c0) < chunk ? (count - c0) : chunk;
        if ((rc = pcub_mc_info(seed, offset + c0, B, N, u, ms))) break;
        if ((rc = pcub_polar_encode_bin(u, B, n, zeros, zeros, N, x, ms))) break;
        if ((rc = pcub_mc_deletion(seed, offset + c0, B, n, tmpl, W, pd, x, rx, len, ms))) break;
        if ((rc = pcub_sc_leaf_deletion(rx, len, B, W, n, n0, ones, pd, all, zeros, u, 0, nullptr, nullptr, leaf, ms)))
            break;
        rc = pcub_genie_count(leaf, u, B, n, counters, ms);
    }
    return rc;
}
