// genie_prior_body.h -- one genie trial under a non-uniform prior, run by one wave: host + device.
//
// genieSingleEncodeSimulatioan / genieSingleDecodeSimulatioan (BinaryPolarEncoderDecoder.py:114-221)
// make every position frozen and draw a fresh common randomness r for the trial (geniePreSteps,
// :101-107), so every u_i is decided by the a-priori x tree: u_i = 0 iff m0(x leaf i) >= r_i
// (:258-262).  The encoder records the x leaves; the decoder runs the xy tree beside the x tree
// through the same minus / plus / normalise steps with the x tree's decisions and records the xy
// leaves.
//
// The walk is prior_cw's (sc_leaf.hip): the same level-by-level half-split order, the same bitrev
// root access, the same leaf order and the same arithmetic (op_f / op_g / op_f_raw / op_g_raw,
// leaf_m0).  What differs is who does the work: the wave's 64 lanes split each level's position loop
// and each partial-sum combine, and the stage levels and re-encoding bits live in the wave's own
// LDS.  A phase is one call of `run`: run(f) gives every lane f(lane) and then makes the phase's LDS
// writes visible to the wave (device: fence + wave barrier; the host emulation runs the lanes one
// after another).  Within a phase no lane reads what another lane writes.
//
// Storage of one trial (N = 2^n):
//   sx, sxy   N - 2 doubles each (sxy only with XY): the stage levels d = 1 .. n - 1 of a tree,
//             level d's N >> d values at [N - 2 (N >> d), N - (N >> d))
//   Y         N bytes: the re-encoding bits, half-split order
// Index bounds.  Levels run d = 1 .. D = n - 1, so Lo = N >> d >= 2.  A level's reads are at
// N - 4 Lo + p and N - 4 Lo + p + Lo with p < Lo, below N - 2 Lo <= N - 4; its writes at
// N - 2 Lo + p < N - Lo <= N - 2.  Y is read at ystart + p with ystart a multiple of 2 Lo below N and
// p < Lo, and combined over [st, st + 2 Lc) with st a multiple of 2 Lc below N: all below N.  The
// leaf phase touches 2k, 2k + 1 (and, for odd k, 2k - 2, 2k - 1) with k < N / 2.
#pragma once
#include "sc_common.h"
#include "sc_leaf_common.h"

namespace pcub {

constexpr int kGpLanes = 64;  // a wave

// doubles of one tree's stage levels, bytes of the re-encoding bits
PCUB_HD long long gp_stage_doubles(int n) { return (1ll << n) - 2; }
PCUB_HD long long gp_wave_bytes(int n, bool with_xy) {
    return (with_xy ? 2 : 1) * gp_stage_doubles(n) * (long long)sizeof(double) + (1ll << n);
}

// one trial's rows
struct GpTrial {
    const double2* xy;  // [N] raw pairs, unused without XY
    const double2* px;  // [N] raw prior pairs
    const double* r;    // [N] common randomness
    double* leaf;       // [N] compact leaves of the exported tree (xy with XY, else x)
    uint8_t* xhat;      // [N] re-encoded bits, natural order, or null
    uint8_t* u;         // [N] decisions, or null
};

template <bool XY, class Run>
PCUB_HD void genie_prior_trial(const Run& run, int n, const GpTrial T, double* sx, double* sxy, uint8_t* Y) {
    const int N = 1 << n;
    const int D = n - 1;  // depth of the 2-value nodes
    for (int k = 0; k < (1 << D); ++k) {
        const int d0 = (k == 0) ? 1 : D - __builtin_ctz((unsigned)k);
        for (int d = d0; d <= D; ++d) {
            const bool gop = (d == d0) && (k != 0);
            const int Lo = N >> d;
            const int ystart = (k >> (D - d + 1)) * (N >> (d - 1));
            const int off = N - 4 * Lo, out = N - 2 * Lo;
            run([&](int lane) {
                for (int p = lane; p < Lo; p += kGpLanes) {
                    const uint32_t u = gop ? Y[ystart + p] : 0u;
                    if (d == 1) {
                        const int q = (int)bitrev((uint32_t)p, n - 1);
                        if (XY) {
                            const double2 a = T.xy[2 * q], b = T.xy[2 * q + 1];
                            sxy[out + p] = gop ? op_g_raw(a, b, u) : op_f_raw(a, b);
                        }
                        const double2 a = T.px[2 * q], b = T.px[2 * q + 1];
                        sx[out + p] = gop ? op_g_raw(a, b, u) : op_f_raw(a, b);
                    } else {
                        if (XY) {
                            const double a = sxy[off + p], b = sxy[off + p + Lo];
                            sxy[out + p] = gop ? op_g(a, b, u) : op_f(a, b);
                        }
                        const double a = sx[off + p], b = sx[off + p + Lo];
                        sx[out + p] = gop ? op_g(a, b, u) : op_f(a, b);
                    }
                }
            });
        }
        // the two leaves of this depth-D node, on one lane: the second needs the first's decision.
        // For odd k it also folds the pair into its sibling's (the combine at depth D).
        run([&](int lane) {
            if (lane != 0) return;
            const int i0 = 2 * k, i1 = 2 * k + 1;
            double c0 = 0.0, c1 = 0.0, x0, x1;
            uint32_t u0, u1;
            if (D == 0) {  // N = 2: the 2-value node is the (never normalised) root
                const double2 pa = T.px[0], pb = T.px[1];
                x0 = op_f_raw(pa, pb);
                u0 = leaf_m0(x0) >= T.r[i0] ? 0u : 1u;
                x1 = op_g_raw(pa, pb, u0);
                if (XY) {
                    const double2 ra = T.xy[0], rb = T.xy[1];
                    c0 = op_f_raw(ra, rb);
                    c1 = op_g_raw(ra, rb, u0);
                }
            } else {
                const double w0 = sx[N - 4], w1 = sx[N - 3];
                x0 = op_f(w0, w1);
                u0 = leaf_m0(x0) >= T.r[i0] ? 0u : 1u;
                x1 = op_g(w0, w1, u0);
                if (XY) {
                    const double v0 = sxy[N - 4], v1 = sxy[N - 3];
                    c0 = op_f(v0, v1);
                    c1 = op_g(v0, v1, u0);
                }
            }
            u1 = leaf_m0(x1) >= T.r[i1] ? 0u : 1u;
            T.leaf[i0] = XY ? c0 : x0;
            T.leaf[i1] = XY ? c1 : x1;
            if (T.u) {
                T.u[i0] = (uint8_t)u0;
                T.u[i1] = (uint8_t)u1;
            }
            const uint8_t y0 = (uint8_t)(u0 ^ u1), y1 = (uint8_t)u1;
            Y[i0] = y0;
            Y[i1] = y1;
            if (k & 1) {
                Y[i0 - 2] ^= y0;
                Y[i0 - 1] ^= y1;
            }
        });
        // the combines above depth D: a node's bits are [minus ^ plus | plus]
        for (int d = D - 1; d >= 1 && (k & 1) && ((k >> (D - d)) & 1); --d) {
            const int Lc = N >> d;
            const int st = (k >> (D - d + 1)) * 2 * Lc;
            run([&](int lane) {
                for (int p = lane; p < Lc; p += kGpLanes) Y[st + p] ^= Y[st + Lc + p];
            });
        }
    }
    if (T.xhat)
        run([&](int lane) {
            for (int i = lane; i < N; i += kGpLanes) T.xhat[i] = Y[bitrev((uint32_t)i, n)];
        });
}

}  // namespace pcub
