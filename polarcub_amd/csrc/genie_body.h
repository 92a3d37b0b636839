// genie_body.h -- the genie's per-leaf statistic (host + device): what one trial adds to Pe[i] when
// the channel probabilities are not trusted (genieSingleDecodeSimulatioan with trustXYProbs = False,
// BinaryPolarEncoderDecoder.py:159-171; coding._genie_stats(m, u, False)).
//
// With the true bit u and the leaf marginals m (calcMarginalizedProbabilities: s = p0 + p1,
// m = p / s, (0.5, 0.5) when s = 0) a trial is
//     correct  m[u] >  m[1 - u]    -> Pe[i] += 0
//     tie      m[u] == m[1 - u]    -> Pe[i] += 0.5
//     wrong    otherwise           -> Pe[i] += 1
// so N "wrong" and N "tie" counts are the whole result: integers, whatever the order they are
// added in.
//
// On the compact leaf v (sc_common.h: +r = (1, r), -r = (r, 1), r in [0, 1], NaN = (0, 0)) the
// class needs no division.  The pair is (1, r) up to its orientation, s = fl(1 + r) > 0 and
// m = (fl(1 / s), fl(r / s)).  For r < 1 the two stay strictly ordered, r / s < 1/2 <= 1 / s: the
// fact the leaf decisions of sc_common.h (leaf_v) rest on.  At the last value below 1,
// r = 1 - 2^-53, s rounds to 2 and the marginals are 1/2 and 1/2 - 2^-54, both exact.  So:
//     r == 1 or NaN   -> tie      ((1, 1) with either sign; (0, 0) gives (0.5, 0.5))
//     otherwise       -> the larger marginal is at bit s = sign(v); correct iff s == u
// -0.0 is (0, 1): the larger marginal is at 1.  tests/test_genie_pipeline.py holds this to the
// two divisions over crafted and random leaves.
#pragma once
#include <stdint.h>

#include "sc_common.h"

namespace pcub {

constexpr int kGenieCorrect = 0, kGenieTie = 1, kGenieWrong = 2;

// class of one leaf with true bit u (0 / 1)
PCUB_HD int genie_class(double v, uint32_t u) {
    const CV c = cv_load(v);
    if (!(c.r < 1.0)) return kGenieTie;  // r == 1, or the NaN of (0, 0)
    return c.s == u ? kGenieCorrect : kGenieWrong;
}

// leaf [N][B] compact leaves, u_words [ceil(N/32)][B]: the class of position i of codeword b
PCUB_HD int genie_class_at(const double* leaf, const uint32_t* u_words, long long B, long long i, long long b) {
    const uint32_t u = (u_words[(i >> 5) * B + b] >> (i & 31)) & 1u;
    return genie_class(leaf[i * B + b], u);
}

}  // namespace pcub
