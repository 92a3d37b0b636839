// mc_rng.h -- the Monte-Carlo draws keyed by the GLOBAL codeword index (host + device), shared by
// the generators of sc_mc.hip and the IR pipeline of sc_ir.hip: the Philox4x32-10 block function,
// the counter streams inside one codeword, and the draw rules that more than one kernel uses.
#pragma once
#include <stdint.h>

#include "sc_common.h"

namespace pcub {

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1).
struct P4 {
    uint32_t v[4];
};

PCUB_HD P4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    return P4{{c0, c1, c2, c3}};
}

// streams inside one codeword's counter space
constexpr uint32_t kStreamInfo = 0, kStreamChannel = 1;

// counter `ctr` of stream `stream` of global codeword g under `seed`
PCUB_HD P4 mc_draw(uint64_t seed, uint64_t g, uint32_t stream, uint32_t ctr) {
    return philox((uint32_t)g, (uint32_t)(g >> 32), stream, ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// uniform double in (0, 1] from 53 random bits
PCUB_HD double u01(uint32_t hi, uint32_t lo) {
    const uint64_t m = (((uint64_t)hi << 32) | lo) >> 11;
    return ((double)m + 1.0) * (1.0 / 9007199254740992.0);
}

// uniform symbol in [0, m) from 32 random bits (multiply-shift)
PCUB_HD uint32_t below(uint32_t r, uint32_t m) { return (uint32_t)(((uint64_t)r * m) >> 32); }

// QSC(p) output of input symbol xs from position i's counter r = (g, kStreamChannel, i): words 0-1
// a 53-bit uniform u (error iff u <= p), word 2 the shift s in [1, q) of an erroneous symbol
PCUB_HD int qsc_output(const P4& r, int q, double p, int xs) {
    const bool err = u01(r.v[0], r.v[1]) <= p;
    return err ? (xs + 1 + (int)below(r.v[2], q - 1)) % q : xs;
}

}  // namespace pcub
