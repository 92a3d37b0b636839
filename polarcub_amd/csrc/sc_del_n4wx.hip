// sc_del_n4wx.hip -- leaf-export (genie) deletion kernels for 512 and 1024 trellises of 2^4
// inputs (n = 13, 14 at main_deletion's n0 = n // 3), no guard-band ones: the export twins of
// sc_del_n4w.hip, one codeword per workgroup of T threads (see sc_del_kern.h, export_wide).
#include "sc_del_kern.h"

namespace pcub {

DelKern del_kernel_n4_wide_x(int tb) {
    if (tb == 9) return k_sc_del<4, 9, true, 0>;
    if (tb == 10) return k_sc_del<4, 10, true, 0>;
    return nullptr;
}

}  // namespace pcub
