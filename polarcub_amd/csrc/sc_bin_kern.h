// sc_bin_kern.h -- the binary SC decode kernel template, its variant table, and the list of the kernels
// the library builds (kBinBuilt: which variant in which root form, in which translation unit).
// sc_bin.hip owns the launch code.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "sc_bin_sched.h"

namespace pcub {

constexpr int kBinBlock = 256;

// Decode kernel variants: virtual register subtree S (values per lane), lanes
// per codeword G, and the minimum waves/SIMD the register allocation must allow.
// Variant fields: S = register subtree values per lane, G = lanes per codeword,
// W = minimum waves/SIMD for register allocation, L = deepest stage level in
// LDS, T = non-temporal loads for the (once-streamed) input rows, Y = the re-encoded bits
// in LDS (Nv/32 words per thread; only where W workgroups still fit a CU's LDS).
// H = the chain's last level has 2S values per lane, the first S in LDS (HL; hl_run).
// P = prefetch distance of the final passes, in column pairs (chain_final).
struct Variant {
    int S, G, W, L, T, Y, H, P;
};
constexpr int kNumVariants = 34;
constexpr Variant kVar[kNumVariants] = {
    {16, 1, 2, 0, 0}, {8, 1, 4, 0, 0}, {32, 1, 1, 0, 0}, {16, 4, 2, 0, 0}, {8, 4, 4, 0, 0}, {16, 2, 2, 0, 0},
    {32, 2, 1, 0, 0}, {8, 8, 4, 0, 0}, {16, 2, 2, 0, 1}, {8, 8, 4, 0, 1}, {16, 4, 2, 0, 1}, {8, 4, 4, 1, 0},
    {16, 2, 4, 0, 1}, {16, 4, 4, 0, 1}, {8, 4, 4, 0, 1}, {32, 4, 2, 0, 1}, {32, 2, 2, 0, 1},
    {32, 4, 3, 0, 1}, {32, 2, 3, 0, 1}, {32, 8, 2, 0, 1}, {32, 8, 3, 0, 1},
    {32, 16, 2, 0, 1}, {32, 16, 3, 0, 1}, {16, 16, 3, 0, 1},
    {32, 4, 3, 0, 1, 1}, {32, 8, 3, 0, 1, 1},
    {32, 4, 2, 0, 1, 1, 1, 2}, {32, 4, 2, 0, 1, 1, 1, 1}, {32, 4, 2, 0, 1, 1, 1, 3}, {32, 4, 3, 0, 1, 1, 0, 2},
    {32, 8, 2, 0, 1, 1, 1, 2}, {32, 4, 2, 0, 1, 0, 1, 2}, {16, 8, 3, 0, 1, 1, 1, 2},
    {32, 8, 2, 0, 1, 0, 1, 2},
};

// LDS bytes of the stage level (L: S pairs per thread) or of the split level's LDS half (H: S doubles)
inline size_t bin_lds_bytes(int v) {
    if (kVar[v].H) return (size_t)kVar[v].S * kBinBlock * sizeof(double);
    return kVar[v].L ? (size_t)kVar[v].S * kBinBlock * sizeof(double2) : 0;
}

// values per lane at the end of a chain (the register level; 2S for the split-level variants)
inline int bin_sr(int v) { return kVar[v].S << kVar[v].H; }

// LDS bytes of the re-encoded bits of variant v at code length 2^n (0 unless Y)
inline size_t bin_ylds_bytes(int v, int n) {
    return kVar[v].Y ? (size_t)kBinBlock * (((size_t)1 << n) / kVar[v].G / 32) * sizeof(uint32_t) : 0;
}

template <int S, int G, int W, bool LDS, int NT, bool YL = false, bool HL = false, int PF = 0, bool CR = false,
          bool TR = false, bool RW = false>
__global__ __launch_bounds__(kBinBlock, W) void k_sc_bin(BinArgs A) {
    // [S pairs][kBinBlock] when LDS (HL: [S doubles][kBinBlock]), then [Nv/32 words][kBinBlock]
    // when YL (plus occupancy padding)
    extern __shared__ double2 lds_last[];
    constexpr int LDS2 = LDS ? S * kBinBlock : HL ? S / 2 * kBinBlock : 0;  // double2 units before Y
    constexpr int CWB = kBinBlock / G;  // codewords per workgroup tile
    const long long slot = (long long)blockIdx.x * kBinBlock + threadIdx.x;
    const int j = threadIdx.x & (G - 1);
    const int lane = threadIdx.x & 63;
    const Lvl last = LDS ? Lvl{lds_last + threadIdx.x, kBinBlock} : Lvl{nullptr, 0};
    // wave tiles: a wave decodes 64 / G codewords at a time (its lanes' codewords are independent of the
    // other waves', whose LDS columns are their own), either the static stride of the workgroup tiles
    // (wave wv of workgroup b takes wave tiles (b + i * grid) * WPB + wv) or the next tile of a counter
    constexpr int WPB = kBinBlock / 64, CWW = 64 / G;
    static_assert(CWB == WPB * CWW, "workgroup tile = its waves' tiles");
    const long long nwt = (A.B + CWW - 1) / CWW;
    const int wv = threadIdx.x >> 6;
    long long wt = A.wtiles ? next_wave_tile(A.wtiles, lane) : (long long)blockIdx.x * WPB + wv;
    while (wt < nwt) {
        const long long cw = wt * CWW + lane / G;
        const bool valid = cw < A.B;
        decode_codeword<S, G, LDS, NT, YL, HL, PF, CR, -1, TR, RW>(A, valid ? cw : A.B - 1, j, lane, slot, valid, last,
                                               YL ? (uint32_t*)(lds_last + LDS2) + threadIdx.x : nullptr, kBinBlock,
                                               HL ? (double*)lds_last + threadIdx.x : nullptr);
        wt = A.wtiles ? next_wave_tile(A.wtiles, lane) : wt + (long long)gridDim.x * WPB;
    }
}

typedef void (*BinKernFn)(BinArgs);

// The root forms a variant can be built in: what the kernel reads at the root of the tree.
//   Compact      CR: the root rows as compact normalised doubles (the Monte-Carlo pipeline's rows, 8 bytes a
//                position instead of a 16-byte pair)
//   Tiled        TR: the rows in the wave's own tiles (tile = 64 / G codewords), addressed from a
//                wave-uniform base with 32-bit lane offsets; TiledCompact: the same over compact rows
//   Rows         RW: the caller's [B][N] rows read in place (a wave's 64 / G codewords are one block of
//                (64 / G) N rows; the same uniform base and lane offsets as Tiled), the root loads plain;
//                RowsNT: non-temporal as the other forms' (kVar's T)
enum BinForm { kPairs, kCompact, kTiled, kTiledCompact, kRows, kRowsNT, kNumBinForms };

// The one statement of a kernel's template arguments: variant V's row of kVar; the form decides CR, TR,
// RW and, for the rows forms, the load hint.
template <int V, BinForm F>
constexpr BinKernFn bin_instance() {
    constexpr Variant r = kVar[V];
    constexpr bool CR = F == kCompact || F == kTiledCompact, TR = F >= kTiled, RW = F == kRows || F == kRowsNT;
    return k_sc_bin<r.S, r.G, r.W, r.L != 0, RW ? int(F == kRowsNT) : r.T, r.Y != 0, r.H != 0, r.P, CR, TR, RW>;
}

// The kernels the library builds, each in the translation unit sc_bin_k<unit>.hip (several units so that
// the library builds in parallel).  The variants are those pick_variant can launch; the rest of kVar are
// the round 1-3 sweep's geometries, measured slower, kept as table rows so the variant
// numbers in profiles/ stay meaningful; pcub_sc_set_variant rejects them.
struct BinBuilt {
    int unit, v;
    BinForm form;
};
constexpr BinBuilt kBinBuilt[] = {
    {0, 0, kPairs}, {0, 24, kPairs},
    {1, 1, kPairs}, {1, 13, kPairs}, {1, 17, kPairs},
    {2, 10, kPairs}, {2, 14, kPairs},
    {4, 26, kPairs},  // the split-level default
    {5, 31, kPairs},  // the split level with the re-encoded bits in the slot scratch, N = 4096 and 8192
    // the split level at G = 8 lanes a codeword (S = 32: 64 values a lane, a node of 512 positions), the
    // re-encoded bits in LDS (30) or in the slot scratch (33).  At N = 4096 the split level is depth 3, so
    // only levels 1 and 2 are stored (variant 31, G = 4, stores three): the C3 shape's candidates
    {8, 30, kPairs}, {8, 33, kPairs},
    {6, 24, kCompact}, {6, 26, kCompact}, {6, 30, kCompact}, {6, 31, kCompact}, {6, 33, kCompact},
    {7, 26, kTiled}, {7, 26, kTiledCompact},
    // the N >= 4096 variants' tiled twins
    {9, 30, kTiled}, {9, 30, kTiledCompact}, {9, 31, kTiled}, {9, 31, kTiledCompact},
    {9, 33, kTiled}, {9, 33, kTiledCompact},
    // the default variant (N = 1024, 2048) with both load forms: a 128-byte line of the rows holds eight
    // rows of one codeword, fetched 16 bytes a load over a pass, and must stay cached until its other pieces
    // are used -- C2: 17.1 ms plain against 29.3 ms non-temporal (pcub_sc_set_rows_nt picks)
    {10, 26, kRows}, {10, 26, kRowsNT},
    // G = 8: a wave's block is 8 codewords; plain root loads only: the non-temporal hint of the tiled twins
    // costs the rows layout more than twice the decode
    {11, 30, kRows}, {11, 33, kRows},
};
constexpr int kNumBinBuilt = sizeof(kBinBuilt) / sizeof(kBinBuilt[0]);

// the rows of kBinBuilt that build (v, form): 1 where the library has the kernel, else 0
constexpr int bin_built(int v, BinForm f) {
    int c = 0;
    for (const BinBuilt& r : kBinBuilt) c += r.v == v && r.form == f;
    return c;
}
constexpr bool bin_list_sound() {
    for (const BinBuilt& r : kBinBuilt) {
        if (r.v < 0 || r.v >= kNumVariants || bin_built(r.v, r.form) != 1) return false;  // no pair twice
        if (!bin_built(r.v, kPairs)) return false;  // "variant v is built" = its Pairs form is
        // the launcher takes compact rows only where the variant's Compact form is built (compact_direct)
        if (r.form == kTiledCompact && !bin_built(r.v, kCompact)) return false;
    }
    return true;
}
static_assert(bin_list_sound(), "kBinBuilt: a pair twice, a variant without Pairs, or an unreachable compact form");

// Unit U's kernel of (v, form), or nullptr: defined by PCUB_BIN_UNIT(U) in sc_bin_k<U>.hip and nowhere
// else, so that each unit instantiates its own rows only.
template <int U>
BinKernFn bin_unit_kernel(int v, BinForm f);
// The built kernel of (v, form), or nullptr (sc_bin.hip).
BinKernFn bin_kernel(int v, BinForm f);

// row I where unit U builds it (the test on U is in a template, so the other units' rows are discarded
// uninstantiated)
template <int U, int I>
void bin_unit_row(int v, BinForm f, BinKernFn& k) {
    if constexpr (kBinBuilt[I].unit == U)
        if (kBinBuilt[I].v == v && kBinBuilt[I].form == f) k = bin_instance<kBinBuilt[I].v, kBinBuilt[I].form>();
}
template <int U, int... I>
BinKernFn bin_unit_rows(int v, BinForm f, std::integer_sequence<int, I...>) {
    BinKernFn k = nullptr;
    (bin_unit_row<U, I>(v, f, k), ...);
    return k;
}

}  // namespace pcub

#define PCUB_BIN_UNIT(U)                                                              \
    template <>                                                                       \
    pcub::BinKernFn pcub::bin_unit_kernel<U>(int v, BinForm f) {                      \
        return bin_unit_rows<U>(v, f, std::make_integer_sequence<int, kNumBinBuilt>{}); \
    }
