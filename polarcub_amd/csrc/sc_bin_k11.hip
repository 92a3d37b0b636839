// sc_bin_k11.hip -- unit 11 of the binary SC decode kernels: its rows of kBinBuilt (sc_bin_kern.h).
#include "sc_bin_kern.h"

PCUB_BIN_UNIT(11)
