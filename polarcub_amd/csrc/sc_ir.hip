// sc_ir.hip -- the information-reconciliation Monte-Carlo as one device pipeline (gfx950) + C-ABI:
// irSimulation (QaryPolarEncoderDecoder.py:887-930) over QSC(p), chunk by chunk on one stream:
//   pcub_ir_prepare   a, the channel rows, the key and the frozen values        (ir_body.h)
//   pcub_scl_qary / pcub_scl_qary_log with the actual path                       (scl.hip)
//   pcub_ir_classify  listDecode's verdict and irSimulation's counters           (ir_body.h)
// Codeword g's draws depend only on (seed, g) (mc_rng.h), so any sharding or chunking of
// [offset, offset + count) counts the same trials.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ir_body.h"
#include "polarcub_sc.h"

using namespace pcub;

namespace {

constexpr int kIrDrawBlock = 256;
constexpr int kIrSplitBlock = 64;
constexpr int kIrLanes = 64;   // codewords of a classify workgroup: one a lane
constexpr int kIrWaves = 16;   // its waves share the paths
constexpr int kIrBlock = kIrLanes * kIrWaves;

// grid: x over codewords, y strides over quads of positions (stores coalesce over the
// codeword-minor layouts)
__global__ __launch_bounds__(kIrDrawBlock) void k_ir_draw(IrPrepArgs A) {
    const long long b = (long long)blockIdx.x * kIrDrawBlock + threadIdx.x;
    if (b >= A.B) return;
    const long long quads = ((1LL << A.n) + 3) / 4;
    for (long long j = blockIdx.y; j < quads; j += gridDim.y) ir_draw_quad(A, b, j);
}

// a lane a codeword: N log2(N) / 2 byte butterflies on its column of work, then the split
__global__ __launch_bounds__(kIrSplitBlock) void k_ir_split(IrPrepArgs A) {
    const long long b = (long long)blockIdx.x * kIrSplitBlock + threadIdx.x;
    if (b >= A.B) return;
    ir_split_cw(A, b);
}

// Lanes over 64 consecutive codewords (out_info is codeword-minor: a wave's byte reads are one
// 64-byte line), the workgroup's sixteen waves over the paths: wave w compares paths w, w + 16, ..
// below its lane's list size, stops at its first match (its lowest), and the waves' matches meet
// in an integer min in LDS.  Wave 0 then takes the verdict and adds the group's counts.  Both
// barriers are unconditional; no thread returns before the second.
__global__ __launch_bounds__(kIrBlock) void k_ir_classify(IrClassArgs C) {
    __shared__ int best[kIrLanes];
    const int lane = threadIdx.x & (kIrLanes - 1), wave = threadIdx.x / kIrLanes;
    const long long b = (long long)blockIdx.x * kIrLanes + lane;
    const bool valid = b < C.B;
    const int size = valid ? ir_size(C, b) : 0;
    if (wave == 0) best[lane] = C.L;  // no match
    __syncthreads();
    for (int i = wave; i < size; i += kIrWaves) {
        if (ir_path_is_key(C, b, i)) {
            atomicMin(&best[lane], i);
            break;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    int outcome = -1;
    unsigned long long bad_symbols = 0, sizes = 0;
    if (valid) {
        const int match = best[lane] < size ? best[lane] : -1;
        outcome = ir_verdict(C, b, size, match);
        if (match < 0) bad_symbols = (unsigned long long)ir_distance_to_first(C, b);
        sizes = (unsigned long long)size;
        if (C.results) C.results[b] = (uint8_t)outcome;
    }
    for (int o = 32; o > 0; o >>= 1) {
        bad_symbols += __shfl_xor(bad_symbols, o);
        sizes += __shfl_xor(sizes, o);
    }
    unsigned long long per[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) per[r] = (unsigned long long)__popcll(__ballot(outcome == r));
    if (lane == 0) {
        atomicAdd(&C.counters[0], per[0] + per[1] + per[2] + per[3] + per[4] + per[5]);
        atomicAdd(&C.counters[1], per[2] + per[3] + per[4] + per[5]);
        atomicAdd(&C.counters[2], bad_symbols);
        atomicAdd(&C.counters[3], sizes);
#pragma unroll
        for (int r = 0; r < 6; ++r)
            if (per[r]) atomicAdd(&C.counters[4 + r], per[r]);
    }
}

bool ir_shape_ok(int32_t log2N, int32_t q, int32_t K) {
    return q >= 2 && q <= 8 && log2N >= 0 && log2N <= 12 && K >= 0 && K <= (1 << log2N);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// a chunk's buffers; the list decoder's slab follows at `scl`
struct IrLayout {
    size_t a, work, xy, actual, fvals, info, prob, size, aprob, scl;
};

IrLayout ir_layout(int64_t chunk, int32_t q, int32_t log2N, int32_t L, int32_t K) {
    IrLayout Y;
    const size_t N = (size_t)1 << log2N, c = (size_t)chunk;
    const size_t kk = (size_t)(K > 0 ? K : 1), ff = N - (size_t)K > 0 ? N - (size_t)K : 1;
    Y.a = 0;
    Y.work = Y.a + align256(N * c);
    Y.xy = Y.work + align256(N * c);
    Y.actual = Y.xy + align256(N * c * (size_t)q * 8);
    Y.fvals = Y.actual + align256(kk * c);
    Y.info = Y.fvals + align256(ff * c);
    Y.prob = Y.info + align256((size_t)L * kk * c);
    Y.size = Y.prob + align256((size_t)L * c * 8);
    Y.aprob = Y.size + align256(c * 4);
    Y.scl = Y.aprob + align256(c * 8);
    return Y;
}

}  // namespace

extern "C" int pcub_ir_prepare(uint64_t seed, int64_t offset, int64_t B, int32_t log2N, int32_t q, double p,
                               int32_t use_log, const uint8_t* frozen, int32_t K, uint8_t* a, double* xy,
                               uint8_t* actual, uint8_t* frozen_vals, uint8_t* work, void* stream) {
    if (B < 0 || offset < 0 || !ir_shape_ok(log2N, q, K) || !(p >= 0.0 && p <= 1.0) || !frozen) return PCUB_EINVAL;
    if (B == 0) return 0;
    const int N = 1 << log2N, nF = N - K;
    if (!a || !xy || !work || (K > 0 && !actual) || (nF > 0 && !frozen_vals)) return PCUB_EINVAL;
    const long long gx = (B + kIrDrawBlock - 1) / kIrDrawBlock;
    if (gx > 0x7fffffffLL) return PCUB_EINVAL;
    IrPrepArgs A;
    A.seed = seed;
    A.offset = offset;
    A.B = B;
    A.n = log2N;
    A.q = q;
    A.K = K;
    A.nF = nF;
    A.p = p;
    // makeQSC's row (ScalarDistributions/QaryMemorylessDistribution.py:780-784), as pcub_mc_channel_qsc
    A.hit = 1.0 - p;
    A.miss = p / (double)(q - 1);
    if (use_log) {
        A.hit = std::log(A.hit);
        A.miss = std::log(A.miss);
    }
    A.frozen = frozen;
    A.a = a;
    A.xy = xy;
    A.work = work;
    A.actual = actual;
    A.fvals = frozen_vals;
    const long long quads = ((long long)N + 3) / 4;
    long long gy = (16384 + gx - 1) / gx;
    if (gy > quads) gy = quads;
    if (gy > 65535) gy = 65535;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ir_draw, dim3((unsigned)gx, (unsigned)gy), dim3(kIrDrawBlock), 0, s, A);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(k_ir_split, dim3((unsigned)((B + kIrSplitBlock - 1) / kIrSplitBlock)), dim3(kIrSplitBlock), 0, s,
                       A);
    return (int)hipGetLastError();
}

extern "C" int pcub_ir_classify(const uint8_t* out_info, const double* out_prob, const int32_t* out_size,
                                const double* out_actual, const uint8_t* actual, int64_t B, int32_t L, int32_t K,
                                uint64_t* counters, uint8_t* results, void* stream) {
    if (B < 0 || L < 1 || L > PCUB_SCL_MAX_L || K < 0 || K > 4096 || !counters) return PCUB_EINVAL;
    if (B == 0) return 0;
    if (!out_prob || !out_size || !out_actual || (K > 0 && (!out_info || !actual))) return PCUB_EINVAL;
    const long long g = (B + kIrLanes - 1) / kIrLanes;
    if (g > 0x7fffffffLL) return PCUB_EINVAL;
    IrClassArgs C;
    C.out_info = out_info;
    C.out_prob = out_prob;
    C.out_size = (const int*)out_size;
    C.out_actual = out_actual;
    C.actual = actual;
    C.B = B;
    C.L = L;
    C.K = K;
    C.counters = (unsigned long long*)counters;
    C.results = results;
    hipLaunchKernelGGL(k_ir_classify, dim3((unsigned)g), dim3(kIrBlock), 0, (hipStream_t)stream, C);
    return (int)hipGetLastError();
}

extern "C" size_t pcub_mc_run_ir_workspace(int64_t chunk, int32_t q, int32_t log2N, int32_t L, int32_t K) {
    if (chunk <= 0 || !ir_shape_ok(log2N, q, K) || L < 1 || L > PCUB_SCL_MAX_L) return 0;
    return ir_layout(chunk, q, log2N, L, K).scl + align256(pcub_scl_qary_workspace(chunk, q, log2N, L, K));
}

extern "C" int pcub_mc_run_ir(uint64_t seed, int64_t offset, int64_t count, int32_t log2N, int32_t q, double p,
                              int32_t L, int32_t use_log, const uint8_t* frozen, int32_t K, int64_t chunk,
                              uint64_t* counters, uint8_t* results, void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (count < 0 || offset < 0 || chunk <= 0 || !counters || !frozen) return PCUB_EINVAL;
    if (!ir_shape_ok(log2N, q, K) || L < 1 || L > PCUB_SCL_MAX_L || !(p >= 0.0 && p <= 1.0)) return PCUB_EINVAL;
    const IrLayout Y = ir_layout(chunk, q, log2N, L, K);
    // the chunk's buffers and at least one workgroup's slots of the list decoder, which strides
    // fewer resident slots over the batch
    const size_t least = pcub_scl_qary_workspace(1, q, log2N, L, K);
    if (!workspace || least == 0 || workspace_bytes < Y.scl + least) return PCUB_EINVAL;
    char* ws = (char*)workspace;
    uint8_t* a = (uint8_t*)(ws + Y.a);
    uint8_t* work = (uint8_t*)(ws + Y.work);
    double* xy = (double*)(ws + Y.xy);
    uint8_t* actual = (uint8_t*)(ws + Y.actual);
    uint8_t* fvals = (uint8_t*)(ws + Y.fvals);
    uint8_t* info = (uint8_t*)(ws + Y.info);
    double* prob = (double*)(ws + Y.prob);
    int32_t* size = (int32_t*)(ws + Y.size);
    double* aprob = (double*)(ws + Y.aprob);
    const int32_t nF = (1 << log2N) - K;
    int rc = 0;
    for (int64_t c0 = 0; !rc && c0 < count; c0 += chunk) {
        const int64_t B = (count - c0) < chunk ? (count - c0) : chunk;
        if ((rc = pcub_ir_prepare(seed, offset + c0, B, log2N, q, p, use_log, frozen, K, a, xy, actual, fvals, work,
                                  stream)))
            break;
        rc = use_log ? pcub_scl_qary_log(xy, B, q, log2N, L, frozen, fvals, nF, actual, K, info, prob, size, aprob,
                                         ws + Y.scl, workspace_bytes - Y.scl, stream)
                     : pcub_scl_qary(xy, B, q, log2N, L, frozen, fvals, nF, actual, K, info, prob, size, aprob,
                                     ws + Y.scl, workspace_bytes - Y.scl, stream);
        if (rc) break;
        rc = pcub_ir_classify(info, prob, size, aprob, actual, B, L, K, counters, results ? results + c0 : nullptr,
                              stream);
    }
    return rc;
}
