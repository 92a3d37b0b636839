// Test-only host build of the genie statistic (genie_body.h): the function the kernel of
// sc_genie.hip calls, one leaf after another.  tests/test_genie_pipeline.py checks it against
// coding._genie_stats on the marginals of the same leaves.
#include <stdint.h>

#include "genie_body.h"

// the class (0 correct, 1 tie, 2 wrong) of `count` single leaves with true bits u
extern "C" int emu_genie_classes(const double* leaf, const uint8_t* u, long long count, int32_t* cls) {
    for (long long k = 0; k < count; ++k) cls[k] = pcub::genie_class(leaf[k], u[k]);
    return 0;
}

// pcub_genie_count's counters (accumulating) for leaf [N][B] and u_words [ceil(N/32)][B]
extern "C" int emu_genie_count(const double* leaf, const uint32_t* u_words, long long B, int log2N,
                               unsigned long long* counters) {
    const long long N = 1LL << log2N;
    counters[0] += (unsigned long long)B;
    for (long long i = 0; i < N; ++i) {
        for (long long b = 0; b < B; ++b) {
            const int c = pcub::genie_class_at(leaf, u_words, B, i, b);
            counters[1 + i] += c == pcub::kGenieWrong ? 1 : 0;
            counters[1 + N + i] += c == pcub::kGenieTie ? 1 : 0;
        }
    }
    return 0;
}
