// sc_bin_k11.hip -- rows twins (RW: the caller's [B][N] rows read in place, see sc_bin_k10.hip) of the
// N >= 4096 variants 30 and 33 (G = 8: a wave's block is 8 codewords), with plain root loads: the
// non-temporal hint of the tiled twins costs the rows layout more than twice the decode.
#include "sc_bin_kern.h"

namespace pcub {

BinKernFn bin_kernel_rows2(int v, bool nt) {
    if (nt) return nullptr;
    switch (v) {
        case 30: return k_sc_bin<32, 8, 2, false, 0, true, true, 2, false, true, true>;
        case 33: return k_sc_bin<32, 8, 2, false, 0, false, true, 2, false, true, true>;
        default: return nullptr;
    }
}

}  // namespace pcub
