// sc_bin_k7.hip -- unit 7 of the binary SC decode kernels: its rows of kBinBuilt (sc_bin_kern.h).
#include "sc_bin_kern.h"

PCUB_BIN_UNIT(7)
