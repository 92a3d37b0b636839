// sc_genie_prior.hip -- genie trials under a non-uniform a-priori distribution, gfx950, + C-ABI
// launcher.
//
// Replaces genieSingleEncodeSimulatioan / genieSingleDecodeSimulatioan
// (BinaryPolarEncoderDecoder.py:114-221) over memoryless binary distributions for a batch of
// trials: every position frozen, a fresh common randomness r[b] for every trial (geniePreSteps,
// :101-107), the a-priori x tree deciding every u_i against it (:258-262).  XY = false is the genie
// encoder (x tree only, x leaves exported), XY = true the genie decoder (the xy tree beside the x
// tree, xy leaves exported).  The per-trial walk is genie_prior_body.h.
//
// Genie chunks are a few thousand trials, too few for a lane a trial (k_sc_prior), so the
// parallelism is inside the trial: one wave a trial, the lanes over each level's positions, the
// stage levels and the re-encoding bits in the wave's LDS.  Trials come from a static stride over a
// resident grid (every trial costs the same).  The waves of a workgroup share nothing: between
// phases a wave fences and meets only itself, and there is no workgroup barrier in the trial loop.
#include <hip/hip_runtime.h>

#include "genie_prior_body.h"
#include "polarcub_sc.h"

using namespace pcub;

namespace {

constexpr int kGpMaxLog2N = 13;          // 16 (N - 2) + N = 139,232 bytes a wave at N = 8192 with xy
constexpr size_t kGpLdsPerCu = 160 * 1024;

struct GpArgs {
    const double2* xy;     // [B][N] raw pairs, or null (XY = false)
    const double2* prior;  // [PB][N] raw prior pairs, PB = 1 or B
    long long PB;
    const double* r;       // [B][N]
    long long B;
    int n;
    uint8_t* xhat;         // [B][N] or null
    uint8_t* u;            // [B][N] or null
    double* leaf;          // [B][N]
};

// run a phase on this lane of the wave, then make its LDS writes visible to the wave's other lanes
// (sc_del_w5.hip's W5WaveRun)
struct GpWaveRun {
    int lane;
    template <class F>
    __device__ __forceinline__ void operator()(F&& f) const {
        f(lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
};

// Dynamic LDS of a workgroup of W waves: [W][T (N - 2)] doubles (T = 2 with XY: the x tree, then
// the xy tree), then [W][N] bytes.  W gp_wave_bytes(n, XY) bytes in all.
template <bool XY>
__global__ __launch_bounds__(256) void k_sc_genie_prior(GpArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gp_lds[];
    const int W = (int)blockDim.x >> 6;
    const int wv = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const long long N = 1ll << A.n;
    const long long sd = gp_stage_doubles(A.n);
    constexpr int T = XY ? 2 : 1;
    double* sx = reinterpret_cast<double*>(gp_lds) + (long long)wv * T * sd;
    double* sxy = sx + sd;  // used only with XY
    uint8_t* Y = gp_lds + (long long)W * T * sd * (long long)sizeof(double) + (long long)wv * N;
    const long long stride = (long long)gridDim.x * W;
    for (long long b = (long long)blockIdx.x * W + wv; b < A.B; b += stride) {
        GpTrial t;
        t.xy = XY ? A.xy + b * N : nullptr;
        t.px = A.prior + (A.PB == 1 ? 0 : b) * N;
        t.r = A.r + b * N;
        t.leaf = A.leaf + b * N;
        t.xhat = A.xhat ? A.xhat + b * N : nullptr;
        t.u = A.u ? A.u + b * N : nullptr;
        genie_prior_trial<XY>(GpWaveRun{lane}, A.n, t, sx, sxy, Y);
    }
}

// Waves a workgroup and workgroups for B trials: of 1, 2 and 4 waves a workgroup the one the
// occupancy query gives the most resident waves a CU (a tie goes to the larger workgroup), the grid
// capped at what is resident.  Dynamic LDS beyond 64 KB is asked for first (the sizes grow with the
// workgroup, so the last request covers the one chosen).  False when the query fits no workgroup.
template <bool XY>
bool gp_geometry(int n, long long B, int& waves, long long& grid, size_t& lds) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return false;
    const size_t per_wave = (size_t)gp_wave_bytes(n, XY);
    int best = 0, best_occ = 0;
    for (int w = 1; w <= 4; w <<= 1) {
        const size_t bytes = (size_t)w * per_wave;
        if (bytes > kGpLdsPerCu) break;
        if (bytes > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sc_genie_prior<XY>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
            break;
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_sc_genie_prior<XY>, w * 64, bytes) != hipSuccess)
            occ = 0;
        if (occ > 0 && w * occ >= best * best_occ) best = w, best_occ = occ;
    }
    if (best == 0) return false;
    waves = best;
    lds = (size_t)best * per_wave;
    const long long need = (B + best - 1) / best;
    const long long res = (long long)cus * best_occ;
    grid = need < res ? need : res;
    return true;
}

template <bool XY>
int gp_launch(const GpArgs& A, hipStream_t stream) {
    int waves = 0;
    long long grid = 0;
    size_t lds = 0;
    // no resident workgroup by the occupancy query: nothing is launched
    if (!gp_geometry<XY>(A.n, A.B, waves, grid, lds)) return (int)hipErrorLaunchOutOfResources;
    hipLaunchKernelGGL(k_sc_genie_prior<XY>, dim3((unsigned)grid), dim3((unsigned)(waves * 64)), lds, stream, A);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int pcub_sc_genie_prior_supported(int32_t log2N, int32_t with_xy) {
    (void)with_xy;  // both modes fit one wave's LDS over the whole range
    return log2N >= 1 && log2N <= kGpMaxLog2N ? 1 : 0;
}

extern "C" int pcub_sc_genie_prior_bin(const double* xy, const double* prior, int64_t prior_batch, const double* r,
                                       int64_t B, int32_t log2N, uint8_t* xhat, uint8_t* u, double* leaf,
                                       void* stream) {
    if (log2N < 1 || log2N > kGpMaxLog2N || B < 0) return PCUB_EINVAL;
    if (prior_batch != 1 && prior_batch != B) return PCUB_EINVAL;
    if (!prior || !r || !leaf) return PCUB_EINVAL;
    if (!xhat && !u && !leaf) return PCUB_EINVAL;
    if (B == 0) return 0;
    GpArgs A;
    A.xy = (const double2*)xy;
    A.prior = (const double2*)prior;
    A.PB = prior_batch;
    A.r = r;
    A.B = B;
    A.n = log2N;
    A.xhat = xhat;
    A.u = u;
    A.leaf = leaf;
    return xy ? gp_launch<true>(A, (hipStream_t)stream) : gp_launch<false>(A, (hipStream_t)stream);
}
