// Host run of genie_bin_body.h (the breadth-first genie trial), test-only: the workgroup's work
// items run one after another inside every phase, and the workgroup's LDS arrays are heap arrays of
// exactly the kernel's sizes (N doubles, 2 N + 2 nw words), one set for all trials as on the device,
// so an index out of range is an access outside an allocation.  The layouts are pcub_sc_genie_bin's:
// rows [B][N][2] or compact [B][N], u_words [ceil(N/32)][B], counters u64[1 + 2N] (accumulating),
// leaf [N][B] or null.
#include <cstdlib>

#include "genie_bin_body.h"

using namespace pcub;

namespace {

struct HostRun {
    int lanes;
    template <class F>
    void operator()(F&& f) const {
        for (int l = 0; l < lanes; ++l) f(l);
    }
};

}  // namespace

extern "C" int emu_genie_bin(const double* rows, int compact, const uint32_t* u_words, long long B, int n, int lanes,
                             uint64_t* counters, double* leaf) {
    if (n < 1 || n > kGbMaxLog2N || B < 0 || lanes < 1) return -1;
    const long long N = 1ll << n;
    const int nw = gb_bit_words(n);
    double* V = (double*)malloc((size_t)N * sizeof(double));
    uint32_t* cw = (uint32_t*)calloc((size_t)N, sizeof(uint32_t));
    uint32_t* ct = (uint32_t*)calloc((size_t)N, sizeof(uint32_t));
    uint32_t* E = (uint32_t*)malloc((size_t)(2 * nw) * sizeof(uint32_t));
    if ((long long)(N * 8 + N * 4 + N * 4 + 2 * nw * 4) != gb_lds_bytes(n)) return -2;
    const HostRun run{lanes};
    for (long long b = 0; b < B; ++b) {
        GbTrial T;
        T.row = rows + b * (compact ? N : 2 * N);
        T.u = u_words + b;
        T.ustride = B;
        T.leaf = leaf ? leaf + b : nullptr;
        T.lstride = B;
        if (compact) genie_bin_trial<true>(run, lanes, n, T, V, E, cw, ct);
        else genie_bin_trial<false>(run, lanes, n, T, V, E, cw, ct);
    }
    counters[0] += (uint64_t)B;
    for (long long i = 0; i < N; ++i) {
        counters[1 + i] += cw[i];
        counters[1 + N + i] += ct[i];
    }
    free(V);
    free(cw);
    free(ct);
    free(E);
    return 0;
}
