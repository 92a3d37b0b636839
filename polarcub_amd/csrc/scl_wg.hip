// scl_wg.hip -- q-ary SCL / Fast-SSC list decoding on gfx950, one workgroup of 256 threads per
// codeword with the lanes over paths and candidates (scl_wg_body.h): the list decoder for
// L > 64, where the lane kernel's serial prune (keep x ncand steps a fork) and private arrays
// sized by L do not reach.
//
// The launch is persistent: workgroup b decodes codewords b, b + grid, ... in slab slot b.
// Static LDS only (SclWgShared); the recursion is scl_run's explicit frame stack, so the kernel has
// a fixed private segment and no dynamic stack.
//
// Barrier rule (scl_wg_body.h): every __syncthreads() sits under conditions that are the same for
// all 256 threads -- the frame state (a function of the frozen mask), Lin, ncand and kept counts
// read from LDS and made uniform; none depends on a thread's path, position or a candidate's
// value, and nothing returns early inside the codeword loop.
#include <hip/hip_runtime.h>

#include "scl_wg.h"
#include "scl_wg_body.h"

using namespace pcub;

namespace {

__global__ __launch_bounds__(kWg) void k_scl_wg(SclArgs A) {
    __shared__ SclWgShared sh;
    for (long long cw = blockIdx.x; cw < A.B; cw += gridDim.x) scl_wg_decode_cw(A, cw, (long long)blockIdx.x, sh);
}

}  // namespace

namespace pcub {

size_t scl_wg_slot_bytes(int q, int log2N, int L, int K) {
    SclWgLayout W;
    W.init(log2N, q, L, K);
    return W.slot_bytes();
}

// workgroups of a launch: 2 a CU (one codeword each)
long long scl_wg_grid(long long B) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    const long long g = (long long)cus * 2;
    return B < g ? B : g;
}

int scl_wg_launch(SclArgs A, long long grid, void* workspace, void* stream) {
    SclWgLayout W;
    W.init(A.n, A.q, A.L, A.K);
    A.ns = grid;
    A.cells = (double*)workspace;
    A.bytes = (uint8_t*)workspace + (size_t)W.ncells * 8 * (size_t)grid;
    hipLaunchKernelGGL(k_scl_wg, dim3((unsigned)grid), dim3(kWg), 0, (hipStream_t)stream, A);
    return (int)hipGetLastError();
}

}  // namespace pcub
