// scl_wg.h -- host interface of the workgroup-per-codeword list decoder (scl_wg.hip) for scl.hip.
#pragma once
#include <stddef.h>

#include "scl_body.h"

namespace pcub {

// bytes of one slab slot (one codeword in flight)
size_t scl_wg_slot_bytes(int q, int log2N, int L, int K);
// resident workgroups of a launch over B codewords (0: no device)
long long scl_wg_grid(long long B);
// launches k_scl_wg with `grid` workgroups over a workspace of grid slots; A.cells / A.bytes /
// A.ns are set here.  Returns the HIP error of the launch.
int scl_wg_launch(SclArgs A, long long grid, void* workspace, void* stream);

}  // namespace pcub
