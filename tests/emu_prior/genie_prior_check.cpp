// Host run of genie_prior_body.h (the wave-a-trial genie walk under a non-uniform prior), test-only:
// the wave's 64 lanes run one after another inside every phase, and the wave's LDS arrays are heap
// arrays of exactly the kernel's sizes (N - 2 doubles a tree, N bytes), one set for all trials as on
// the device, so an index out of range is an access outside an allocation.
//   genie_prior_check <in> <out>    (exit status 0: ran)
// in:  int32 n, with_xy, B, PB; prior [PB][N][2] f64; xy [B][N][2] f64 (with_xy); r [B][N] f64
// out: leaf [B][N] f64 compact leaves; xhat [B][N] u8; u [B][N] u8
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "genie_prior_body.h"

using namespace pcub;

struct HostRun {
    template <class F>
    void operator()(F&& f) const {
        for (int l = 0; l < kGpLanes; ++l) f(l);
    }
};

template <class T>
static bool rd(FILE* f, T* p, size_t count) {
    return count == 0 || fread(p, sizeof(T), count, f) == count;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: genie_prior_check <in> <out>\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[4];
    if (!rd(f, hdr, 4)) return 2;
    const int n = hdr[0];
    const bool with_xy = hdr[1] != 0;
    const long long B = hdr[2], PB = hdr[3];
    if (n < 1 || n > 13 || B < 0 || (PB != 1 && PB != B)) return 2;
    const long long N = 1ll << n;
    std::vector<double> prior((size_t)(PB * N * 2)), xy((size_t)(with_xy ? B * N * 2 : 0)), r((size_t)(B * N));
    if (!rd(f, prior.data(), prior.size()) || !rd(f, xy.data(), xy.size()) || !rd(f, r.data(), r.size())) return 2;
    fclose(f);
    std::vector<double> leaf((size_t)(B * N));
    std::vector<uint8_t> xhat((size_t)(B * N)), u((size_t)(B * N));
    // the wave's LDS: exactly the kernel's sizes
    double* sx = (double*)malloc((size_t)gp_stage_doubles(n) * sizeof(double));
    double* sxy = with_xy ? (double*)malloc((size_t)gp_stage_doubles(n) * sizeof(double)) : nullptr;
    uint8_t* Y = (uint8_t*)malloc((size_t)N);
    for (long long b = 0; b < B; ++b) {
        GpTrial t;
        t.xy = with_xy ? reinterpret_cast<const double2*>(xy.data()) + b * N : nullptr;
        t.px = reinterpret_cast<const double2*>(prior.data()) + (PB == 1 ? 0 : b) * N;
        t.r = r.data() + b * N;
        t.leaf = leaf.data() + b * N;
        t.xhat = xhat.data() + b * N;
        t.u = u.data() + b * N;
        if (with_xy) genie_prior_trial<true>(HostRun{}, n, t, sx, sxy, Y);
        else genie_prior_trial<false>(HostRun{}, n, t, sx, sxy, Y);
    }
    free(sx);
    free(sxy);
    free(Y);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    bool ok = fwrite(leaf.data(), sizeof(double), leaf.size(), o) == leaf.size();
    ok = ok && fwrite(xhat.data(), 1, xhat.size(), o) == xhat.size();
    ok = ok && fwrite(u.data(), 1, u.size(), o) == u.size();
    ok = fclose(o) == 0 && ok;
    return ok ? 0 : 2;
}
