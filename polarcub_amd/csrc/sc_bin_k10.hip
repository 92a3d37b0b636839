// sc_bin_k10.hip -- the default variant (26: N = 1024, 2048) reading the caller's [B][N] rows in place
// (decode_codeword's RW: the tiled-root twin's uniform base over a wave's block of (64 / G) N rows),
// with plain (the default) and with non-temporal root loads: a 128-byte line of the rows holds eight rows
// of one codeword, fetched 16 bytes a load over a pass, and must stay cached until its other pieces are
// used -- C2: 17.1 ms plain against 29.3 ms non-temporal (pcub_sc_set_rows_nt picks).
#include "sc_bin_kern.h"

namespace pcub {

BinKernFn bin_kernel_rows(int v, bool nt) {
    switch (v) {
        case 26: return nt ? k_sc_bin<32, 4, 2, false, 1, true, true, 2, false, true, true>
                           : k_sc_bin<32, 4, 2, false, 0, true, true, 2, false, true, true>;
        default: return nullptr;
    }
}

}  // namespace pcub
