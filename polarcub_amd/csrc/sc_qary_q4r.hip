// sc_qary_q4r.hip -- the q = 4 split-level kernel reading the caller's [B][N][4] rows in place
// (decode_qary_cw's RW: the tiled-root twin's uniform base over a wave's block of 16 N rows; see
// sc_qary_q4.hip for the geometry).
#include "sc_qary_kern.h"

namespace pcub {

QKern qary_kernel_q4_h_rows(int S, int G) {
    if (S == 4 && G == 4) return k_sc_qary<4, 4, 4, 3, 1, true, true, true, -1, true>;
    return nullptr;
}

// ... specialised on the C4 code length (N = 256), as the tiled-root twin is
QKern qary_kernel_q4_h_rows_n(int S, int G, int n) {
    if (S == 4 && G == 4 && n == 8) return k_sc_qary<4, 4, 4, 3, 1, true, true, true, 8, true>;
    return nullptr;
}

}  // namespace pcub
