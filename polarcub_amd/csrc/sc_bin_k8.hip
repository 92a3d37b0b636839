// sc_bin_k8.hip -- unit 8 of the binary SC decode kernels: its rows of kBinBuilt (sc_bin_kern.h).
#include "sc_bin_kern.h"

PCUB_BIN_UNIT(8)
