// sc_bin_k10.hip -- unit 10 of the binary SC decode kernels: its rows of kBinBuilt (sc_bin_kern.h).
#include "sc_bin_kern.h"

PCUB_BIN_UNIT(10)
