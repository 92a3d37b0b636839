// sc_del_w5.hip -- deletion-channel SC decode for 32-input trellises (n0 = 5, no guard-band ones):
// main_deletion.py's n0 = n // 3 at n = 15 (:100), and n = 11 .. 14 at the same n0: 64 .. 1024
// trellises a codeword.
//
// Replaces BinaryPolarEncoderDecoder.decode (BinaryPolarEncoderDecoder.py:71-99, recursion
// :223-325) over the CollectionOfBinaryTrellises of a received word
// (VectorDistributions/CollectionOfBinaryTrellises.py:55-82, 106-129) for those shapes, with the
// trellis levels of trellis_wave5.h: one wave a (trellis, depth-4 node) task, its trellises in the
// wave's LDS.  Not here: leaf export, guard-band ones, fewer than 64 trellises, and
// n = 16, 17 (2,048 / 4,096 rows a memoryless node need another subtree decode).
//
// Workgroup: WPB task waves, one codeword at a time (codewords from a per-launch counter, or a static
// stride).  For each of the 16 depth-4 nodes k, the waves take the codeword's trellises from an LDS
// counter and leave each one's three rows (minus; plus after decision 0 / 1) in LDS at its half-split
// position bitrev(t); wave 0 then decodes the memoryless node of the minus rows (16 lanes, T / 16
// values a lane, as sc_del_w4.hip), every trellis picks its plus row by its decision, and wave 0
// decodes that node.  A node whose two memoryless subtrees are both rate-0 skips its tasks (its
// decisions are the frozen values whatever the rows).  Every task rebuilds its path from the base:
// no device memory beyond the arguments.  The 32 decisions of a trellis re-encode to its 32 x_hat
// bits (w5_enc32).
#include <hip/hip_runtime.h>

#include "sc_del_kern.h"
#include "trellis_wave5.h"

namespace pcub {

namespace {

// run a phase on one lane of the wave, then make its LDS writes visible to the wave's other lanes
struct W5WaveRun {
    int lane;
    template <class F>
    __device__ __forceinline__ void operator()(F&& f) const {
        f(lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
};

template <int T>
__device__ __forceinline__ uint64_t w5_window(const uint32_t* w, int kk, int wi) {
    const int us = kk * T + 64 * wi;
    return (uint64_t)w[us >> 5] | ((uint64_t)w[(us >> 5) + 1] << 32);
}

// collapse point kk's memoryless node: all frozen?
template <int T>
__device__ __forceinline__ bool w5_rate0(const uint32_t* fmask, int kk) {
    bool r = true;
    for (int i = 0; i < T / 32; ++i) r = r && fmask[kk * (T / 32) + i] == 0xffffffffu;
    return r;
}

// SC over collapse point kk's memoryless node of the T rows vals[p] (half-split positions): wave 0,
// 16 lanes (the other groups decode copies); bits to xb[p / 16] bit p % 16, decisions to xub
template <int TB>
__device__ __forceinline__ void w5_subtree(const DelArgs& A, const double* vals, int kk, unsigned long long* xb,
                                           unsigned long long* xub) {
    constexpr int T = 1 << TB, NW = T / 64, LV = T / 16;
    const int lane = threadIdx.x & 63;
    if ((threadIdx.x >> 6) == 0) {
        uint64_t fm[NW], fv[NW], ubl[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            fm[w] = w5_window<T>(A.fmask, kk, w);
            fv[w] = w5_window<T>(A.fval, kk, w);
            ubl[w] = 0;
        }
        const int j = lane & 15;
        double vv[LV];
#pragma unroll
        for (int t = 0; t < LV; ++t) vv[t] = vals[j + 16 * t];
        typename DelWin<LV, NW>::Bits bits;
        if constexpr (NW == 1) bits = WinTree<LV, 16, 1>::run(vv, ubl, fm, fv, lane);
        else bits = DelWin<LV, NW>::run(vv, ubl, fm, fv, lane);
#pragma unroll
        for (int t = 0; t < LV; ++t) {
            const unsigned long long bal = __ballot((bits >> t) & 1u);
            if (lane == 0) xb[t] = bal;
        }
        if (lane == 0)
#pragma unroll
            for (int w = 0; w < NW; ++w) xub[w] = ubl[w];
    }
    __syncthreads();
}

// collapse point kk's information bits (its decisions at the unfrozen positions, in order) into the
// codeword's bit buffer at offset ib; returns the count
template <int T>
__device__ __forceinline__ int w5_info(const DelArgs& A, int kk, const unsigned long long* xub, uint32_t* infol, int ib) {
    constexpr int NW = T / 64;
    int total = 0, before = 0;
    const int w = (int)threadIdx.x;
    for (int i = 0; i < NW; ++i) {
        const int c = __builtin_popcountll(~w5_window<T>(A.fmask, kk, i));
        before += i < w ? c : 0;
        total += c;
    }
    if (w < NW) {
        const uint64_t ub = xub[w];
        int off = ib + before;
        for (uint64_t im = ~w5_window<T>(A.fmask, kk, w); im != 0ull; im &= im - 1ull, ++off)
            if ((ub >> __builtin_ctzll(im)) & 1ull) atomicOr(&infol[off >> 5], 1u << (off & 31));
    }
    return total;
}

// WPB task waves a workgroup, one workgroup a CU.  LDS sets WPB: a wave's trellises take
// sizeof(W5Buf) = 38,864 bytes and the codeword's rows, histories and segments ~38.6 T bytes, out of
// 160 KB, all of it static (w5_waves).
template <int TB, int WPB>
__global__ __launch_bounds__(WPB * 64, 1) void k_sc_del_w5(DelArgs A) {
    constexpr int BLK = WPB * 64;
    constexpr int T = 1 << TB;
    constexpr int LV = T / 16, NW = T / 64;
    constexpr int WPC = T;  // x_hat words a codeword (32 T bits)
    static_assert(NW <= BLK, "w5_info: a thread a 64-position window");
    __shared__ W5Buf wb[WPB];
    __shared__ double vm[T], vp0[T], vp1[T];
    __shared__ uint32_t hist[T], sy[T];
    __shared__ uint8_t sm[T];
    __shared__ uint8_t xmb[T];
    __shared__ unsigned long long xb[LV], xub[NW];
    __shared__ uint32_t infol[WPC];
    __shared__ long long s_next;
    __shared__ int s_task[16];  // node k's next task (the waves take the codeword's trellises in turn)
    // the packed received word is read only by the segment parse, before the codeword's first task: it
    // lies in the task waves' buffers (the launcher refuses rows longer than del_w5_rx_bytes)
    uint32_t* rxb = reinterpret_cast<uint32_t*>(wb);
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long it = 0;; ++it) {
        long long cw;
        if (A.wtiles) {
            if (threadIdx.x == 0) s_next = (long long)atomicAdd(A.wtiles, 1ull);
            __syncthreads();
            cw = s_next;
        } else {
            cw = (long long)blockIdx.x + it * (long long)gridDim.x;
        }
        if (cw >= A.B) break;
        // the received word, bit-packed; each trellis's segment (m > 32: no edges)
        pack_rows<1, BLK>(A, cw, rxb, lane);
        for (int i = threadIdx.x; i < WPC; i += BLK) infol[i] = 0u;
        __syncthreads();
        int len = A.rx_len[cw];
        len = len < 0 ? 0 : (len > A.stride ? A.stride : len);
        for (int t = threadIdx.x; t < T; t += BLK) {
            int s, m;
            segment_of_packed(rxb, len, TB, t, s, m);
            uint32_t y = 0;
            if (m > 0 && m <= kW5L) {
                const int w0 = s >> 5;
                const uint64_t lo = rxb[w0], hi = (w0 + 1 < A.rw) ? rxb[w0 + 1] : 0u;
                y = (uint32_t)(((hi << 32) | lo) >> (s & 31)) & w5_mask(m);
            }
            sm[t] = (uint8_t)(m <= kW5L ? m : kW5L + 1);
            sy[t] = y;
            hist[t] = 0u;
        }
        if (threadIdx.x < 16) s_task[threadIdx.x] = 0;
        __syncthreads();
        int ib = 0;  // information bits so far
#pragma unroll 1
        for (int k = 0; k < 16; ++k) {
            const int km = 2 * k, kp = 2 * k + 1;
            if (!(w5_rate0<T>(A.fmask, km) && w5_rate0<T>(A.fmask, kp))) {
                // the tasks come from a counter, not a fixed stride: their costs differ (segment
                // lengths), and the node's subtree waits for the slowest wave
#pragma unroll 1
                for (;;) {
                    int t = 0;
                    if (lane == 0) t = atomicAdd(&s_task[k], 1);
                    t = __builtin_amdgcn_readfirstlane(t);
                    if (t >= T) break;
                    // the task's segment and history are wave-uniform: scalar registers
                    W5Dims D;
                    D.set(__builtin_amdgcn_readfirstlane((int)sm[t]), (uint32_t)__builtin_amdgcn_readfirstlane((int)sy[t]),
                          A.pd);
                    w5_task(W5WaveRun{lane}, wb[wv], D, k, (uint32_t)__builtin_amdgcn_readfirstlane((int)hist[t]));
                    if (lane < 3) {
                        const int p = (int)bitrev((uint32_t)t, TB);
                        double* dst = lane == 0 ? vm : lane == 1 ? vp0 : vp1;
                        dst[p] = wb[wv].out[lane];
                    }
                }
            }
            __syncthreads();
            // the minus node, then every position's plus row by its decision, then the plus node
            w5_subtree<TB>(A, vm, km, xb, xub);
            ib += w5_info<T>(A, km, xub, infol, ib);
            for (int p = threadIdx.x; p < T; p += BLK) {
                const uint32_t x = (uint32_t)(xb[p >> 4] >> (p & 15)) & 1u;
                xmb[p] = (uint8_t)x;
                vm[p] = x ? vp1[p] : vp0[p];
            }
            __syncthreads();
            w5_subtree<TB>(A, vm, kp, xb, xub);
            ib += w5_info<T>(A, kp, xub, infol, ib);
            for (int t = threadIdx.x; t < T; t += BLK) {
                const int p = (int)bitrev((uint32_t)t, TB);
                const uint32_t xp = (uint32_t)(xb[p >> 4] >> (p & 15)) & 1u;
                hist[t] = hist[t] | ((uint32_t)xmb[p] << km) | (xp << kp);
            }
            __syncthreads();
        }
        // x_hat: trellis t's slice is natural positions [32 t, 32 t + 32)
        if (A.xhat)
            for (int i = threadIdx.x; i < WPC; i += BLK) A.xhat[(long long)i * A.B + cw] = w5_enc32(hist[i]);
        if (A.info)
            for (int i = threadIdx.x; i < (ib + 31) / 32; i += BLK) A.info[(long long)i * A.B + cw] = infol[i];
        __syncthreads();  // rxb / sm / hist / infol / s_next are rewritten by the next codeword
    }
}

}  // namespace

// task waves a workgroup for 2^tb trellises: four where the codeword's state leaves room (64, 128
// trellises), three beyond (DESIGN 3.2 has the sums)
constexpr int w5_waves(int tb) { return tb <= 7 ? 4 : 3; }

DelKern del_kernel_w5(int tb) {
    switch (tb) {
        case 6: return k_sc_del_w5<6, w5_waves(6)>;
        case 7: return k_sc_del_w5<7, w5_waves(7)>;
        case 8: return k_sc_del_w5<8, w5_waves(8)>;
        case 9: return k_sc_del_w5<9, w5_waves(9)>;
        case 10: return k_sc_del_w5<10, w5_waves(10)>;
        default: return nullptr;
    }
}

// threads a workgroup of del_kernel_w5(tb)
int del_w5_block(int tb) { return w5_waves(tb) * 64; }

// the longest packed received row, in bytes, that del_kernel_w5(tb) takes: its task waves' buffers
long long del_w5_rx_bytes(int tb) { return (long long)w5_waves(tb) * (long long)sizeof(W5Buf); }

}  // namespace pcub
