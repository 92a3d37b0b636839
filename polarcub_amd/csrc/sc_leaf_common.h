// sc_leaf_common.h -- the two helpers the leaf-export kernels share (sc_leaf.hip's lane schedule,
// genie_prior_body.h's wave schedule): a bit of a packed word array, and the reference's leaf
// marginal m0 of a compact normalised leaf.
#pragma once
#include "sc_common.h"

namespace pcub {

PCUB_HD uint32_t word_bit(const uint32_t* w, int i) { return (w[i >> 5] >> (i & 31)) & 1u; }

// the reference's marginal m0 of a compact normalised leaf (calcMarginalizedProbabilities, :52-69)
PCUB_HD double leaf_m0(double v) {
    const CV c = cv_load(v);
    double p0 = c.s ? c.r : 1.0, p1 = c.s ? 1.0 : c.r;
    if (c.r != c.r) p0 = p1 = 0.0;
    double s = 0.0;
    s += p0;
    s += p1;
    return s > 0.0 ? p0 / s : 0.5;
}

}  // namespace pcub
