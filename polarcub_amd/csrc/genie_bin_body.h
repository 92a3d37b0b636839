// genie_bin_body.h -- one genie trial over a binary memoryless channel, breadth-first: host + device.
//
// The uniform-prior, every-position-frozen-to-u case of recursiveEncodeDecode
// (BinaryPolarEncoderDecoder.py:223-325, as genieSingleDecodeSimulatioan calls it, :114-178).  Every
// u_i is given, so no value of the SC tree waits for a decision and the tree is evaluated level by
// level: node (d, k) has N >> d values, node (d + 1, 2k) is f of node (d, k)'s pairs, node
// (d + 1, 2k + 1) is g of the same pairs with the bits of the minus sibling's re-encoding; every
// child is max-normalised, the root never is (op_f_raw / op_g_raw at the first level of raw rows).
// The per-value arithmetic is sc_common.h's, unchanged, so a leaf equals k_sc_leaf's bit for bit.
//
// Order.  The project's half-split order (k_sc_leaf): a node's pairs are (p, p + L/2).  With node
// (d, k) at [k (N >> d), (k + 1) (N >> d)) of one N-value array V, pass d (Lo = N >> d) takes the
// pairs (j, j + Lo), j with bit Lo clear, and writes f to j and g to j + Lo: in place, and after
// pass n position i holds the leaf of u_i.  The root in this order is root[bitrev(j)], so pass 1
// reads the natural-order pair (2q, 2q + 1) and writes to j = bitrev(q), j + N/2: the bit reversal
// is paid once, there, and the row is read in address order.
//
// Re-encodings ride along as one bit array E in the same order.  The encoding of a node of length L
// over its u's is the butterfly E[j] ^= E[j + s] (j with bit s clear) over the strides s < L, so
// applying every stride s < N to u gives the root's encoding, and undoing stride Lo in pass d gives
// the children's.  For a pair's bits (e0, e1) the g-bit is e0 ^ e1, the minus child inherits
// e0 ^ e1 and the plus child e1; at depth n the bit is u_i, which the classifier needs.  E is
// double-buffered words: a pass reads the old words and writes the new ones.
//
// A phase is one call of `run`: run(f) gives every lane f(lane) and then makes the phase's writes
// visible to all lanes (device: a barrier; the host emulation runs the lanes one after another).
// Within a phase no lane reads what another lane writes.
//
// Storage of a workgroup (N = 2^n, nw = max(1, N / 32)):
//   V        N doubles        the current level
//   cw, ct   N u32 each       wrong / tie counts over all the trials the workgroup takes; position
//                             2t, 2t + 1 belongs to lane t % lanes in every trial: plain increments
//   E        2 nw u32         the bits, two buffers
// Index bounds.  Pass d: t < N / 2, sh = n - d, j = (t >> sh) << (sh + 1) | (t & (Lo - 1)) has bit
// Lo clear and j + Lo < N (pass 1: j = bitrev(t, n - 1) < N / 2 = Lo).  Row reads are at 2t and
// 2t + 1 < N.  A word stage reads w and w + sw with bit sw clear in w and sw <= nw / 2.
#pragma once
#include "genie_body.h"

namespace pcub {

constexpr int kGbMaxLog2N = 13;

PCUB_HD int gb_bit_words(int n) { return n <= 5 ? 1 : 1 << (n - 5); }
// LDS bytes of a workgroup: V, cw, ct, E
PCUB_HD long long gb_lds_bytes(int n) { return (16ll << n) + 8ll * gb_bit_words(n); }

// one trial's rows
struct GbTrial {
    const double* row;     // COMPACT: [N] compact values; else [N][2] raw pairs
    const uint32_t* u;     // word w of the true bits at u[w * ustride]
    long long ustride;
    double* leaf;          // leaf i at leaf[i * lstride], or null
    long long lstride;
};

PCUB_HD uint32_t gb_stage_bits(uint32_t x, int s) {  // stride s < 32 inside a word
    const uint32_t m = s == 1 ? 0x55555555u : s == 2 ? 0x33333333u : s == 4 ? 0x0F0F0F0Fu : s == 8 ? 0x00FF00FFu : 0x0000FFFFu;
    return x ^ ((x >> s) & m);
}

// word w after the butterfly stage of stride s bits (its own inverse)
PCUB_HD uint32_t gb_stage_word(const uint32_t* src, int w, int s) {
    if (s < 32) return gb_stage_bits(src[w], s);
    const int sw = s >> 5;
    return (w & sw) ? src[w] : (src[w] ^ src[w + sw]);
}

PCUB_HD uint32_t gb_bit(const uint32_t* e, int j) { return (e[j >> 5] >> (j & 31)) & 1u; }

template <bool COMPACT, class Run>
PCUB_HD void genie_bin_trial(const Run& run, int lanes, int n, const GbTrial T, double* V, uint32_t* E, uint32_t* cw,
                             uint32_t* ct) {
    const int N = 1 << n, nw = gb_bit_words(n);
    int cur = 0;
    // the root's encoding: the strides inside a word on load, then the word strides
    run([&](int lane) {
        for (int w = lane; w < nw; w += lanes) {
            uint32_t x = T.u[(long long)w * T.ustride];
            if (N < 32) x &= (1u << N) - 1u;
            for (int s = 1; s < 32 && s < N; s <<= 1) x = gb_stage_bits(x, s);
            E[w] = x;
        }
    });
    for (int s = 32; s < N; s <<= 1) {
        const uint32_t* src = E + cur * nw;
        uint32_t* dst = E + (cur ^ 1) * nw;
        run([&](int lane) {
            for (int w = lane; w < nw; w += lanes) dst[w] = gb_stage_word(src, w, s);
        });
        cur ^= 1;
    }
    for (int d = 1; d <= n; ++d) {
        const int sh = n - d, Lo = 1 << sh;
        const uint32_t* src = E + cur * nw;
        uint32_t* dst = E + (cur ^ 1) * nw;
        run([&](int lane) {
            for (int w = lane; w < nw; w += lanes) dst[w] = gb_stage_word(src, w, Lo);
            for (int t = lane; t < N / 2; t += lanes) {
                int j;
                double f, g;
                uint32_t e, e1;
                if (d == 1) {  // t is the natural-order pair index
                    j = (int)bitrev((uint32_t)t, n - 1);
                    e1 = gb_bit(src, j + Lo);
                    e = gb_bit(src, j) ^ e1;
                    if (COMPACT) {
                        const double a = T.row[2 * t], b = T.row[2 * t + 1];
                        f = op_f(a, b);
                        g = op_g(a, b, e);
                    } else {
                        const double2* r2 = reinterpret_cast<const double2*>(T.row);
                        const double2 a = r2[2 * t], b = r2[2 * t + 1];
                        f = op_f_raw(a, b);
                        g = op_g_raw(a, b, e);
                    }
                } else {
                    j = ((t >> sh) << (sh + 1)) | (t & (Lo - 1));
                    e1 = gb_bit(src, j + Lo);
                    e = gb_bit(src, j) ^ e1;
                    const double a = V[j], b = V[j + Lo];
                    f = op_f(a, b);
                    g = op_g(a, b, e);
                }
                if (d == n) {  // Lo = 1: the leaves of u_j = e and u_{j+1} = e1
                    const int c0 = genie_class(f, e), c1 = genie_class(g, e1);
                    cw[j] += c0 == kGenieWrong ? 1u : 0u;
                    ct[j] += c0 == kGenieTie ? 1u : 0u;
                    cw[j + 1] += c1 == kGenieWrong ? 1u : 0u;
                    ct[j + 1] += c1 == kGenieTie ? 1u : 0u;
                    if (T.leaf) {
                        T.leaf[(long long)j * T.lstride] = f;
                        T.leaf[(long long)(j + 1) * T.lstride] = g;
                    }
                } else {
                    V[j] = f;
                    V[j + Lo] = g;
                }
            }
        });
        cur ^= 1;
    }
}

}  // namespace pcub
