// sc_bin_k9.hip -- unit 9 of the binary SC decode kernels: its rows of kBinBuilt (sc_bin_kern.h).
#include "sc_bin_kern.h"

PCUB_BIN_UNIT(9)
