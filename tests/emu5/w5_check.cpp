// Host check of trellis_wave5.h (the n0 = 5 wave-per-task trellises) against trellis_body.h's Trel
// walk at L = 32 (test-only): on random segments (length, received bits, deletion probability) and
// random 32-bit decision histories, the three rows of every depth-4 node -- minus, plus after 0, plus
// after 1 -- must be bit-identical to the DelBase / DelNode recursion's (the collapse values the
// memoryless subtree reads), and the re-encoding of the 32 decisions must equal the recursion's.
// Also checks w5_div against integer division over the whole range the phases (and trellis_wave.h's
// note) rely on.
//   w5_check <cases> <seed>    (exit status 0: all equal)
#include <cstdio>
#include <cstdlib>
#include <random>

#include "trellis_wave5.h"

using namespace pcub;

struct HostRun {
    template <class F>
    void operator()(F&& f) const {
        for (int l = 0; l < 64; ++l) f(l);
    }
};

static long long g_fail = 0, g_cmp = 0;

// the Trel walk, rows[k][0..2] per depth-4 node k; returns the root encoding
static uint32_t ref_rows(const BaseT<32>& b, uint32_t hist, double rows[16][3]) {
    using Cap = DelCap<32, 0>;
    auto* c1 = new Trel<16, Cap::V, Cap::E(1)>;
    auto* c2 = new Trel<8, Cap::V, Cap::E(2)>;
    auto* c3 = new Trel<4, Cap::V, Cap::E(3)>;
    auto* c4 = new Trel<2, Cap::V, Cap::E(4)>;
    uint32_t y1[2];
    for (int h1 = 0; h1 < 2; ++h1) {
        trellis_transform_base<32>(b, *c1, h1 ? &y1[0] : nullptr);
        trellis_normalize<16>(*c1);
        uint32_t y2[2];
        for (int h2 = 0; h2 < 2; ++h2) {
            trellis_transform<16>(*c1, *c2, h2 ? &y2[0] : nullptr);
            trellis_normalize<8>(*c2);
            uint32_t y3[2];
            for (int h3 = 0; h3 < 2; ++h3) {
                trellis_transform<8>(*c2, *c3, h3 ? &y3[0] : nullptr);
                trellis_normalize<4>(*c3);
                uint32_t y4[2];
                for (int h4 = 0; h4 < 2; ++h4) {
                    trellis_transform<4>(*c3, *c4, h4 ? &y4[0] : nullptr);
                    trellis_normalize<2>(*c4);
                    const int k = 8 * h1 + 4 * h2 + 2 * h3 + h4;
                    double m0, m1;
                    trellis_collapse(*c4, nullptr, m0, m1);
                    rows[k][0] = norm_pack(m0, m1);
                    for (uint32_t xm = 0; xm < 2; ++xm) {
                        trellis_collapse(*c4, &xm, m0, m1);
                        rows[k][1 + xm] = norm_pack(m0, m1);
                    }
                    const uint32_t xm = (hist >> (2 * k)) & 1u, xp = (hist >> (2 * k + 1)) & 1u;
                    y4[h4] = (xm ^ xp) | (xp << 1);
                }
                y3[h3] = w5_combine(y4[0], y4[1], 2);
            }
            y2[h2] = w5_combine(y3[0], y3[1], 4);
        }
        y1[h1] = w5_combine(y2[0], y2[1], 8);
    }
    delete c1;
    delete c2;
    delete c3;
    delete c4;
    return w5_combine(y1[0], y1[1], 16);
}

static bool same_bits(double a, double b) { return as_bits(a) == as_bits(b) || (a != a && b != b); }

// w5_div(n, w5_magic(d)) == n / d for n < 2^16, 0 < d < 512
static long long check_div() {
    long long bad = 0;
    for (int d = 1; d < 512; ++d) {
        const uint32_t mg = w5_magic(d);
        for (int n = 0; n < (1 << 16); ++n) bad += w5_div(n, mg) != n / d ? 1 : 0;
    }
    return bad;
}

int main(int argc, char** argv) {
    const long long n = argc > 1 ? std::atoll(argv[1]) : 2000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    const double pds[] = {0.0, 0.01, 0.1, 0.1, 0.2, 0.37, 0.5, 0.9, 1.0};
    const long long div_bad = check_div();
    if (div_bad) {
        std::printf("w5_div: %lld wrong quotients\n", div_bad);
        g_fail += div_bad;
    }
    auto* wb = new W5Buf;
    long long hist_m[34] = {};
    for (long long i = 0; i < n; ++i) {
        // lengths: near 32 (few deletions, the common case), uniform 0 .. 32, 32 itself, a few longer
        const int r = (int)(rng() % 16);
        const int m = r < 8    ? (int)(32 - (rng() % 10))
                      : r < 13 ? (int)(rng() % 33)
                      : r < 15 ? 32
                               : (int)(33 + rng() % 3);
        ++hist_m[m < 33 ? m : 33];
        const uint32_t y = (m <= 32) ? (uint32_t)rng() & w5_mask(m) : 0u;
        const double pd = pds[rng() % 9];
        const uint32_t hist = (uint32_t)rng();
        BaseT<32> b;
        b.m = m;
        b.d = 32 - m;
        b.y = y;
        b.pins = 0.5 * (1.0 - pd);
        b.pdel = 0.5 * pd;
        double rows[16][3];
        const uint32_t xr = ref_rows(b, hist, rows);
        W5Dims D;
        D.set(m, y, pd);
        for (int k = 0; k < 16; ++k) {
            w5_task(HostRun{}, *wb, D, k, hist);
            for (int o = 0; o < 3; ++o) {
                ++g_cmp;
                if (!same_bits(wb->out[o], rows[k][o])) {
                    if (g_fail++ < 12)
                        std::printf("case %lld (m=%d y=%#x pd=%g hist=%#x) node %d row %d: %.17g vs ref %.17g\n", i, m, y, pd,
                                    hist, k, o, wb->out[o], rows[k][o]);
                }
            }
        }
        ++g_cmp;
        if (w5_enc32(hist) != xr && g_fail++ < 12) std::printf("case %lld: encoding %#x vs %#x\n", i, w5_enc32(hist), xr);
    }
    delete wb;
    std::printf("w5_check: %lld cases, %lld comparisons, %lld mismatches; m histogram:", n, g_cmp, g_fail);
    for (int m = 0; m < 34; ++m) std::printf(" %lld", hist_m[m]);
    std::printf("\n");
    return g_fail ? 1 : 0;
}
