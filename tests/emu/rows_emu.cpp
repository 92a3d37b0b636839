// Host emulation of the binary decode schedule on the caller's [B][N][2] rows (TEST ONLY; see
// sc_emu.cpp).  Runs decode_small / decode_codeword of polarcub_amd/csrc/sc_bin_sched.h -- the code
// the kernels run -- at one lane a codeword on the layouts pcub_sc_decode_bin_rows uses:
//   layout 0: [N][B] rows (A.tile = 0), the untiled reference point;
//   layout 1: [B][N] rows through the generic path (A.tile = 1: the tiled layout of width 1);
//   layout 2: [B][N] rows through the rows twins' addressing (decode_codeword's RW: a uniform block
//             base and a 32-bit lane offset; at G = 1 a block is 64 codewords).
// Built as a shared library by tests/test_rows_layout_abi.py, and with -DROWS_EMU_MAIN as a stand-alone
// program (its own main, exactly sized heap buffers) that the same test compiles with
// -fsanitize=address,undefined and runs as a subprocess.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "sc_bin_sched.h"

using namespace pcub;

extern "C" int emu_decode_bin_rows(const double* xy, long long B, int n, const uint32_t* fmask, const uint32_t* fval,
                                   uint32_t* info, uint32_t* xhat, int S, int layout) {
    const int N = 1 << n;
    if (layout < 0 || layout > 2) return -1;
    BinArgs A;
    A.xy = (const double2*)xy;
    A.xc = nullptr;
    A.B = B;
    A.n = n;
    A.fmask = fmask;
    A.fval = fval;
    A.info = info;
    A.xhat = xhat;
    A.uout = nullptr;
    A.ef = nullptr;
    A.cmask = nullptr;
    A.scratch = nullptr;
    A.ybits = nullptr;
    A.nslots = 0;
    A.tile = layout == 0 ? 0 : 1;
    if (n <= 5) {
        for (long long b = 0; b < B; ++b) {
            switch (n) {
                case 0: decode_small<1>(A, b, true); break;
                case 1: decode_small<2>(A, b, true); break;
                case 2: decode_small<4>(A, b, true); break;
                case 3: decode_small<8>(A, b, true); break;
                case 4: decode_small<16>(A, b, true); break;
                case 5: decode_small<32>(A, b, true); break;
            }
        }
        return 0;
    }
    if (N < 2 * S || (S != 8 && S != 16 && S != 32)) return -1;
    const long long nslots = 2;
    std::vector<double2> scr((size_t)(N / 2 - S) * nslots + 1);  // + 1: never empty (N = 2 S stores no level)
    std::vector<uint32_t> yb((size_t)(N / 32) * nslots);
    const int D = n - (S == 8 ? 3 : S == 16 ? 4 : 5);
    std::vector<uint8_t> ef((size_t)1 << D);
    for (int k = 0; k < (1 << D); ++k) ef[k] = (uint8_t)first_frozen_depth(fmask, k, D, S);
    A.ef = ef.data();
    std::vector<uint32_t> cm((size_t)(N / 32) * 8);
    for (int i = 0; i < N / 32; ++i) compress_masks(fmask[i], cm.data() + 8 * i);
    A.cmask = cm.data();
    A.scratch = scr.data();
    A.ybits = yb.data();
    A.nslots = nslots;
    for (long long b = 0; b < B; ++b) {
        const long long slot = b % nslots;
        if (layout == 2) {
            if (S == 8) decode_codeword<8, 1, false, 1, false, false, 0, false, -1, true, true>(A, b, 0, 0, slot, true);
#ifndef ROWS_EMU_MAIN  // the stand-alone program runs S = 8 alone (a third of the sanitized compile)
            else if (S == 16) decode_codeword<16, 1, false, 1, false, false, 0, false, -1, true, true>(A, b, 0, 0, slot, true);
            else if (S == 32) decode_codeword<32, 1, false, 1, false, false, 0, false, -1, true, true>(A, b, 0, 0, slot, true);
#endif
            else return -1;
        } else {
            if (S == 8) decode_codeword<8, 1>(A, b, 0, 0, slot, true);
#ifndef ROWS_EMU_MAIN
            else if (S == 16) decode_codeword<16, 1>(A, b, 0, 0, slot, true);
            else if (S == 32) decode_codeword<32, 1>(A, b, 0, 0, slot, true);
#endif
            else return -1;
        }
    }
    return 0;
}

#ifdef ROWS_EMU_MAIN
// B = 3 codewords at N = 32, 64, 1024: the rows on the heap, exactly B N pairs, decoded through the
// rows layouts and through [N][B] rows; every output word must agree.  Exit status 0 when they do.
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) * 0x1p-53;
}

int main() {
    const long long B = 3;
    const int ns[3] = {5, 6, 10};
    for (int n : ns) {
        const int N = 1 << n, W = (N + 31) / 32;
        double* rows = (double*)malloc((size_t)B * N * 2 * sizeof(double));   // [B][N][2], exactly sized
        double* cols = (double*)malloc((size_t)B * N * 2 * sizeof(double));   // [N][B][2]
        uint32_t* fm = (uint32_t*)calloc((size_t)W, sizeof(uint32_t));
        uint32_t* fv = (uint32_t*)calloc((size_t)W, sizeof(uint32_t));
        int K = 0;
        for (int i = 0; i < N; ++i) {
            const bool frozen = i < N / 8 || rnd() < 0.4;
            if (frozen) fm[i >> 5] |= 1u << (i & 31);
            else ++K;
            if (frozen && rnd() < 0.5) fv[i >> 5] |= 1u << (i & 31);
        }
        for (long long b = 0; b < B; ++b)
            for (int i = 0; i < N; ++i)
                for (int x = 0; x < 2; ++x) {
                    const double v = rnd();
                    rows[((size_t)b * N + i) * 2 + x] = v;
                    cols[((size_t)i * B + b) * 2 + x] = v;
                }
        const size_t IW = (size_t)(K + 31) / 32 > 0 ? (size_t)(K + 31) / 32 : 1;
        uint32_t* out[3][2];
        for (int l = 0; l < 3; ++l) {
            out[l][0] = (uint32_t*)calloc(IW * B, sizeof(uint32_t));
            out[l][1] = (uint32_t*)calloc((size_t)W * B, sizeof(uint32_t));
            // the small-code kernels have one path for every [B][N] caller: layout 2 is layout 1 there
            if (emu_decode_bin_rows(l == 0 ? cols : rows, B, n, fm, fv, out[l][0], out[l][1], 8, l) != 0) {
                fprintf(stderr, "rows_emu: n=%d layout %d refused\n", n, l);
                return 2;
            }
        }
        for (int l = 1; l < 3; ++l)
            if (memcmp(out[l][0], out[0][0], IW * B * sizeof(uint32_t)) != 0 ||
                memcmp(out[l][1], out[0][1], (size_t)W * B * sizeof(uint32_t)) != 0) {
                fprintf(stderr, "rows_emu: n=%d layout %d differs from [N][B]\n", n, l);
                return 1;
            }
        for (int l = 0; l < 3; ++l) {
            free(out[l][0]);
            free(out[l][1]);
        }
        free(rows);
        free(cols);
        free(fm);
        free(fv);
    }
    printf("rows_emu: ok\n");
    return 0;
}
#endif
