// Test-only host build of the IR pipeline's per-codeword code (ir_body.h): the functions the
// kernels of sc_ir.hip call, one codeword after another.  tests/test_ir_pipeline.py checks the
// transform and the key / frozen split against coding_qary.polarTransformOfQudits and the verdict
// against QaryPolarEncoderDecoder._list_result.
#include <math.h>
#include <stdint.h>

#include <vector>

#include "ir_body.h"

namespace {

pcub::IrPrepArgs prep_args(uint64_t seed, long long offset, long long B, int n, int q, double p, int use_log,
                           const uint8_t* frozen, int K, uint8_t* a, double* xy, uint8_t* work, uint8_t* actual,
                           uint8_t* fvals) {
    pcub::IrPrepArgs A;
    A.seed = seed;
    A.offset = offset;
    A.B = B;
    A.n = n;
    A.q = q;
    A.K = K;
    A.nF = (1 << n) - K;
    A.p = p;
    A.hit = use_log ? log(1.0 - p) : 1.0 - p;
    A.miss = use_log ? log(p / (double)(q - 1)) : p / (double)(q - 1);
    A.frozen = frozen;
    A.a = a;
    A.xy = xy;
    A.work = work;
    A.actual = actual;
    A.fvals = fvals;
    return A;
}

}  // namespace

// the transform and the split alone on given words a [N][B]: u [N][B] in natural order, actual
// [K][B], fvals [nF][B]
extern "C" int emu_ir_split(const uint8_t* a, long long B, int n, int q, const uint8_t* frozen, int K, uint8_t* u,
                            uint8_t* actual, uint8_t* fvals) {
    const long long N = 1LL << n;
    std::vector<uint8_t> work(a, a + N * B);
    const pcub::IrPrepArgs A = prep_args(0, 0, B, n, q, 0.0, 0, frozen, K, nullptr, nullptr, work.data(), actual, fvals);
    for (long long b = 0; b < B; ++b) {
        pcub::ir_split_cw(A, b);
        for (long long i = 0; i < N; ++i) u[i * B + b] = work[(long long)pcub::bitrev((uint32_t)i, n) * B + b];
    }
    return 0;
}

// pcub_ir_prepare's outputs for global codewords [offset, offset + B)
extern "C" int emu_ir_prepare(uint64_t seed, long long offset, long long B, int n, int q, double p, int use_log,
                              const uint8_t* frozen, int K, uint8_t* a, double* xy, uint8_t* actual, uint8_t* fvals) {
    const long long N = 1LL << n;
    std::vector<uint8_t> work((size_t)(N * B));
    const pcub::IrPrepArgs A = prep_args(seed, offset, B, n, q, p, use_log, frozen, K, a, xy, work.data(), actual, fvals);
    for (long long b = 0; b < B; ++b) {
        for (long long j = 0; j < (N + 3) / 4; ++j) pcub::ir_draw_quad(A, b, j);
        pcub::ir_split_cw(A, b);
    }
    return 0;
}

// pcub_ir_classify's counters (accumulating) and results
extern "C" int emu_ir_classify(const uint8_t* out_info, const double* out_prob, const int* out_size,
                               const double* out_actual, const uint8_t* actual, long long B, int L, int K,
                               unsigned long long* counters, uint8_t* results) {
    pcub::IrClassArgs C;
    C.out_info = out_info;
    C.out_prob = out_prob;
    C.out_size = out_size;
    C.out_actual = out_actual;
    C.actual = actual;
    C.B = B;
    C.L = L;
    C.K = K;
    C.counters = counters;
    C.results = results;
    for (long long b = 0; b < B; ++b) {
        int size, bad_symbols;
        const int r = pcub::ir_classify_cw(C, b, &size, &bad_symbols);
        counters[0] += 1;
        counters[1] += r >= pcub::kIrFailAboveMax ? 1 : 0;
        counters[2] += (unsigned long long)bad_symbols;
        counters[3] += (unsigned long long)size;
        counters[4 + r] += 1;
        if (results) results[b] = (uint8_t)r;
    }
    return 0;
}
