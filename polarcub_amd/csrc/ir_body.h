// ir_body.h -- the information-reconciliation (IR) trial around the list decoder, per codeword
// (host + device): what irSimulation (QaryPolarEncoderDecoder.py:887-930) does before and after
// listDecode, restated over the batch layouts of the list decoder (codeword-minor, [..][B]).
//
//   prepare   a ~ uniform over [0, q)^N, b = QSC_p(a); u = polarTransformOfQudits(q, a)
//             (:1136-1154); a_key = u on the information set, frozen values on the frozen set,
//             both in ascending index order (the order pcub_scl_qary consumes)        (:822-855)
//   classify  listDecode's verdict with actualInformation (:172-213) and irSimulation's counting
//             (:905-909) from the decoder's final list
//
// Why the frozen values are u itself.  ir() forms the syndrome w = u (q - 1) mod q on the frozen
// set (calculate_syndrome_and_complement, :822-833) and hands listDecode
// frozen_values = w (q - 1) mod q (:846).  (q - 1)^2 = q (q - 2) + 1 is 1 mod q, so
// frozen_values = u (q - 1)^2 mod q = u on the frozen set: the two multiplications cancel and the
// decoder is given the transform's own symbols.
//
// The draws are those of pcub_mc_info_qary (K = N) and pcub_mc_channel_qsc (mc_rng.h): symbol i of
// global codeword g is below(q) of lane (i & 3) of counter (g, kStreamInfo, i >> 2), its channel
// output qsc_output of counter (g, kStreamChannel, i).
#pragma once
#include <stdint.h>

#include "mc_rng.h"
#include "sc_common.h"

namespace pcub {

// -- prepare ---------------------------------------------------------------------------------------

struct IrPrepArgs {
    uint64_t seed;
    long long offset;        // global index of codeword 0 of this batch
    long long B;
    int n, q, K, nF;         // log2 N, alphabet, information / frozen symbols (K + nF = N)
    double p;
    double hit, miss;        // the row's two values: 1 - p at y and p / (q - 1) elsewhere, or their
                             // logarithms (use_log; taken once on the host, so no device log)
    const uint8_t* frozen;   // [N] 1 = frozen
    uint8_t* a;              // [N][B] the drawn word
    double* xy;              // [N][B][q] channel rows
    uint8_t* work;           // [N][B] scratch: a copy of a, transformed in place
    uint8_t* actual;         // [K][B] u on the information set
    uint8_t* fvals;          // [nF][B] u on the frozen set
};

// symbols 4j .. 4j+3 of codeword b: the word a (and its copy in work) and the channel rows
PCUB_HD void ir_draw_quad(const IrPrepArgs& A, long long b, long long j) {
    const uint64_t g = (uint64_t)(A.offset + b);
    const long long N = 1LL << A.n;
    const P4 ri = mc_draw(A.seed, g, kStreamInfo, (uint32_t)j);
    for (int k = 0; k < 4; ++k) {
        const long long i = 4 * j + k;
        if (i >= N) break;
        const int xs = (int)below(ri.v[k], (uint32_t)A.q);
        A.a[i * A.B + b] = (uint8_t)xs;
        A.work[i * A.B + b] = (uint8_t)xs;
        const int y = qsc_output(mc_draw(A.seed, g, kStreamChannel, (uint32_t)i), A.q, A.p, xs);
        double* row = A.xy + (i * A.B + b) * A.q;
        for (int t = 0; t < A.q; ++t) row[t] = t == y ? A.hit : A.miss;
    }
}

// polarTransformOfQudits in place on v[0..N) (element i at v[i * stride]).  The reference splits a
// vector into [pair sums | negated odd elements] and recurses on each half (:1136-1154, as
// scl_polar).  Done in place on neighbours at distance 2^t (stage t pairs the positions whose bit
// t differs) the same butterflies leave the output in bit-reversed order: u[i] = v[bitrev(i)].
PCUB_HD void ir_transform(uint8_t* v, long long stride, int n, int q) {
    const int N = 1 << n;
    for (int t = 0; t < n; ++t) {
        const int h = 1 << t;
        for (int lo = 0; lo < N; lo += 2 * h) {
            for (int p = lo; p < lo + h; ++p) {
                const int x = v[p * stride], y = v[(p + h) * stride];
                const int s = x + y;
                v[p * stride] = (uint8_t)(s >= q ? s - q : s);
                v[(p + h) * stride] = (uint8_t)(y ? q - y : 0);
            }
        }
    }
}

// codeword b: transform its column of work, then deal u out in ascending index order
PCUB_HD void ir_split_cw(const IrPrepArgs& A, long long b) {
    const int N = 1 << A.n;
    uint8_t* v = A.work + b;
    ir_transform(v, A.B, A.n, A.q);
    int ki = 0, fi = 0;
    for (int i = 0; i < N; ++i) {
        const uint8_t u = v[(long long)bitrev((uint32_t)i, A.n) * A.B];
        if (A.frozen[i]) {
            if (fi < A.nF) A.fvals[(long long)fi * A.B + b] = u;
            ++fi;
        } else {
            if (ki < A.K) A.actual[(long long)ki * A.B + b] = u;
            ++ki;
        }
    }
}

// -- classify --------------------------------------------------------------------------------------

struct IrClassArgs {
    const uint8_t* out_info;   // [L][K][B] the decoder's final list
    const double* out_prob;    // [L][B]
    const int* out_size;       // [B]
    const double* out_actual;  // [B] actual_prob
    const uint8_t* actual;     // [K][B] the key
    long long B;
    int L, K;
    unsigned long long* counters;  // u64[10]
    uint8_t* results;              // [B] outcome codes, or null
};

// the ProbResult codes (QaryPolarEncoderDecoder.py:18-24)
constexpr int kIrSuccessMax = 0, kIrSuccessBelowMax = 1, kIrFailAboveMax = 2, kIrFailIsMax = 3, kIrFailInRange = 4,
              kIrFailBelowMin = 5;

// the list size as read: kept inside [1, L] so that no index below leaves the buffers
PCUB_HD int ir_size(const IrClassArgs& C, long long b) {
    const int s = C.out_size[b];
    return s < 1 ? 1 : (s > C.L ? C.L : s);
}

// whether path i of codeword b is the key (K = 0: it is).  Eight symbols a step, their loads
// independent of each other, and out at the first step with a mismatch: a symbol-by-symbol walk is
// one dependent byte load after another, and the paths of a list share long prefixes with the key.
PCUB_HD bool ir_path_is_key(const IrClassArgs& C, long long b, int i) {
    const uint8_t* row = C.out_info + (long long)i * C.K * C.B + b;
    const uint8_t* key = C.actual + b;
    int k = 0;
    for (; k + 8 <= C.K; k += 8) {
        unsigned diff = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) diff |= (unsigned)(row[(long long)(k + j) * C.B] ^ key[(long long)(k + j) * C.B]);
        if (diff) return false;
    }
    for (; k < C.K; ++k)
        if (row[(long long)k * C.B] != key[(long long)k * C.B]) return false;
    return true;
}

// symbols in which path 0 differs from the key (hamming(a_key, informationList[0]))
PCUB_HD int ir_distance_to_first(const IrClassArgs& C, long long b) {
    const uint8_t* row = C.out_info + b;
    const uint8_t* key = C.actual + b;
    int d = 0;
    for (int k = 0; k < C.K; ++k) d += row[(long long)k * C.B] != key[(long long)k * C.B] ? 1 : 0;
    return d;
}

// listDecode's ProbResult from the lowest matching index (`match` < size, or -1 for none).  max and
// min walk prob[:size] as Python's max / min do (the first element, replaced by a strictly larger /
// smaller one); the comparisons are the reference's in either domain (-inf compares as a number).
PCUB_HD int ir_verdict(const IrClassArgs& C, long long b, int size, int match) {
    double mx = C.out_prob[b], mn = mx;
    for (int i = 1; i < size; ++i) {
        const double v = C.out_prob[(long long)i * C.B + b];
        mx = v > mx ? v : mx;
        mn = v < mn ? v : mn;
    }
    if (match >= 0) return C.out_prob[(long long)match * C.B + b] == mx ? kIrSuccessMax : kIrSuccessBelowMax;
    const double ap = C.out_actual[b];
    if (ap > mx) return kIrFailAboveMax;
    if (ap == mx) return kIrFailIsMax;
    if (ap >= mn) return kIrFailInRange;
    return kIrFailBelowMin;
}

// One codeword start to end, serially: the reference for the kernel's mapping and the host build's
// entry.  Returns the outcome; *bad_symbols is 0 with a match.
PCUB_HD int ir_classify_cw(const IrClassArgs& C, long long b, int* size_out, int* bad_symbols) {
    const int size = ir_size(C, b);
    int match = -1;
    for (int i = 0; i < size && match < 0; ++i)
        if (ir_path_is_key(C, b, i)) match = i;
    *size_out = size;
    *bad_symbols = match >= 0 ? 0 : ir_distance_to_first(C, b);
    return ir_verdict(C, b, size, match);
}

}  // namespace pcub
