// scl_wg_body.h -- q-ary SCL / Fast-SSC list decoding of one codeword by one workgroup of 256
// threads, lanes over paths and candidates (host + device).
//
// The arithmetic is scl_body.h's: every rounded operation of a path is the one the lane kernel
// performs, in its order (the per-row helpers scl_marginal, scl_ratio, scl_argmax, scl_prod_enc,
// scl_np_sum_pow2, scl_polar, scl_logsumexp, scl_logaddexp are called as they are); only which
// thread performs it changes:
//   minus / plus transform + normalise, combine     threads over (path slot, position); slot L is
//                                                   the actual path
//   information / frozen leaf                       one path a thread (its q candidates)
//   rate-0, repetition                              (path) / (path, fork symbol); the product over
//                                                   the S positions sequential inside the thread
//   rate-1, SPC                                     one path a thread for the ratio scan, the least
//                                                   reliable pick and the product of maxima, then
//                                                   candidates f + q^2 i / q^3 i across threads
//   commit of information rows                      (kept path, information index)
//   normalise                                       max reduction (exact in any order), then one
//                                                   divide / subtract a path
//
// Slab.  Codeword-major: a slot's cells are contiguous (element e of slot s at
// cells[s * ncells + e]); SclLayout addresses it with ns = 1, so a depth's block runs
// (slot, position, symbol) with the pair (position, symbol) contiguous under the threads.  After
// SclLayout's cells come the per-path values the lane kernel keeps in registers or private arrays:
// the fork base metric (L cells), a marginal row a thread (256 x 8 cells), and integers: origin[]
// (L), the least reliable positions (4 L) and the parity delta (L).  After SclLayout's bytes: a
// transform scratch of 2 N bytes a thread.  All offsets are 64-bit.
//
// Prune: an exact parallel top-L equal to scl_prune + scl_commit (all kept when ncand <= L; else
// keep = max(1, min(#non-zero, L)) largest metrics, ties to the lower candidate, listed in
// ascending candidate order).  A most-significant-byte-first radix select over an order-preserving
// 64-bit key (sign-flip transform; -0.0 and +0.0 share a key) with a 256-bin LDS histogram a pass
// finds the keep-th largest key T and the count above it; then every thread takes a contiguous
// chunk of candidates, a workgroup prefix count in candidate order admits the first keep - above
// candidates equal to T, and the same prefix gives each thread its place in origin[].  Keys are
// totally ordered integers, so NaN metrics (after an all-zero list) cannot stall it.
//
// Barrier rule.  Every barrier (WG_SYNC) sits under conditions that are the same for all 256
// threads: the frame state (a function of the frozen mask alone), Lin, ncand, and kept counts that
// were written to LDS by one thread, read after a barrier and made wave-uniform (wg_uni).  No
// condition around a barrier depends on a thread's path, position or a candidate's value, and
// there is no early return inside the codeword loop.  Code between WG_EACH blocks is uniform:
// every thread executes it on identical values.
//
// Host build (tests/emu_scl_wg): WG_EACH runs the 256 threads one after another and WG_SYNC is
// empty, so anything a thread needs from another must have crossed a WG_SYNC through the slab or
// the shared block -- the same discipline the device needs.
#pragma once
#include "scl_body.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define WG_EACH(t) for (int t = (int)threadIdx.x, wg_once_ = 1; wg_once_; wg_once_ = 0)
#define WG_SYNC() __syncthreads()
#define WG_ATOMIC_ADD(x, v) atomicAdd(&(x), (v))
#else
#define WG_EACH(t) for (int t = 0; t < ::pcub::kWg; ++t)
#define WG_SYNC() ((void)0)
#define WG_ATOMIC_ADD(x, v) ((x) += (v))
#endif

namespace pcub {

constexpr int kWg = 256;

// what one slot holds beyond SclLayout (ns = 1)
struct SclWgLayout {
    SclLayout Y;
    long long c_base, c_marg, c_int, ncells;
    long long i_org, i_lr, i_dl;
    long long b_wtmp, nbytes;
    PCUB_HD void init(int n, int q, int L, int K) {
        Y.init(n, q, L, K);
        c_base = Y.ncells;                       // L fork base metrics
        c_marg = c_base + L;                     // a marginal row (8 cells) a thread
        c_int = c_marg + (long long)kWg * 8;     // 6 L ints
        i_org = 0;                               // origin[L]
        i_lr = L;                                // least reliable positions [L][4]
        i_dl = 5LL * L;                          // parity delta [L]
        ncells = c_int + (6LL * L + 1) / 2;
        b_wtmp = Y.nbytes;                       // 2 N bytes a thread: transform out + temp
        nbytes = (b_wtmp + 2LL * kWg * Y.N + 7) & ~7LL;
    }
    PCUB_HD size_t slot_bytes() const { return (size_t)ncells * 8 + (size_t)nbytes; }
};

// the workgroup's static LDS
struct SclWgShared {
    unsigned hist[256];
    int ca[kWg], cb[kWg];
    int ba[16], bb[16];
    double red[kWg];
    double red2[16];
    unsigned long long prefix;
    int rem, cnt;
    double w, ap;
};

struct SclWgCtx {
    SclCtx c;
    SclWgLayout W;
    SclWgShared* sh;
    int* ints;
};

// a value every thread read from the same LDS word, as a wave-uniform scalar
PCUB_HD int wg_uni(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}

// order-preserving key of a metric: a > b <=> key(a) > key(b) for non-NaN doubles, -0.0 == +0.0
PCUB_HD unsigned long long wg_key(double v) {
    unsigned long long b = (unsigned long long)as_bits(v);
    if ((b << 1) == 0) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

PCUB_HD int wg_fval(const SclCtx& c, int idx) { return (int)c.A->fvals[(long long)idx * c.A->B + c.cw]; }

// scl_normalize over the workgroup: returns the maximum
PCUB_HD double wg_normalize(SclWgCtx& g, int k) {
    SclCtx& c = g.c;
    SclWgShared& sh = *g.sh;
    const long long pr = c.Y.c_prob;
    WG_EACH(t) {
        double m = c.C(pr);
        for (int i = t; i < k; i += kWg) {
            const double v = c.C(pr + i);
            m = v > m ? v : m;
        }
        sh.red[t] = m;
    }
    WG_SYNC();
    WG_EACH(t) {
        if (t < 16) {
            double m = sh.red[16 * t];
            for (int j = 1; j < 16; ++j) {
                const double v = sh.red[16 * t + j];
                m = v > m ? v : m;
            }
            sh.red2[t] = m;
        }
    }
    WG_SYNC();
    WG_EACH(t) {
        double m = sh.red2[0];
        for (int j = 1; j < 16; ++j) {
            const double v = sh.red2[j];
            m = v > m ? v : m;
        }
        for (int i = t; i < k; i += kWg) c.C(pr + i) = c.lg ? c.C(pr + i) - m : c.C(pr + i) / m;
        if (t == 0) sh.w = m;
    }
    WG_SYNC();
    return sh.w;
}

// scl_prune + scl_commit over the workgroup: origin[] (ascending kept candidates) in the slab's
// ints, their metrics in c_prob, the information rows of the other buffer; returns the kept count
PCUB_HD int wg_prune_commit(SclWgCtx& g, int ncand, int ii, int div, int lin) {
    SclCtx& c = g.c;
    SclWgShared& sh = *g.sh;
    const int L = c.Y.L;
    int* org = g.ints + g.W.i_org;
    const long long cd = c.Y.c_cand;
    int k;
    if (ncand <= L) {
        k = ncand;
        WG_EACH(t) {
            for (int i = t; i < ncand; i += kWg) org[i] = i;
        }
        WG_SYNC();
    } else {
        const double zero = c.lg ? -INFINITY : 0.0;
        WG_EACH(t) {
            if (t == 0) sh.cnt = 0;
        }
        WG_SYNC();
        WG_EACH(t) {
            int nzt = 0;
            for (int i = t; i < ncand; i += kWg) nzt += c.C(cd + i) != zero;
            WG_ATOMIC_ADD(sh.cnt, nzt);
        }
        WG_SYNC();
        const int nz = wg_uni(sh.cnt);
        // (all candidates zero: the reference fails on the empty list; keep one)
        k = nz < L ? (nz > 0 ? nz : 1) : L;
        // the k-th largest key, a byte a pass: prefix = its decided high bytes, rem = its rank
        // among the candidates that share them
        for (int p = 7; p >= 0; --p) {
            const int sft = 8 * p;
            WG_EACH(t) {
                sh.hist[t] = 0;
                if (t == 0 && p == 7) {
                    sh.prefix = 0;
                    sh.rem = k;
                }
            }
            WG_SYNC();
            WG_EACH(t) {
                const unsigned long long pre = sh.prefix;
                for (int i = t; i < ncand; i += kWg) {
                    const unsigned long long key = wg_key(c.C(cd + i));
                    if (p == 7 || (key >> (sft + 8)) == (pre >> (sft + 8)))
                        WG_ATOMIC_ADD(sh.hist[(unsigned)(key >> sft) & 255u], 1u);
                }
            }
            WG_SYNC();
            WG_EACH(t) {
                if (t == 0) {
                    int rem = sh.rem, b = 255;
                    for (; b > 0; --b) {
                        const int h = (int)sh.hist[b];
                        if (rem <= h) break;
                        rem -= h;
                    }
                    sh.rem = rem;
                    sh.prefix |= (unsigned long long)b << sft;
                }
            }
            WG_SYNC();
        }
        // candidates above the threshold T, and the first rem equal to it in candidate order
        const int chunk = (ncand + kWg - 1) / kWg;
        WG_EACH(t) {
            const unsigned long long T = sh.prefix;
            const int lo = t * chunk < ncand ? t * chunk : ncand;
            const int hi = lo + chunk < ncand ? lo + chunk : ncand;
            int a = 0, e = 0;
            for (int i = lo; i < hi; ++i) {
                const unsigned long long key = wg_key(c.C(cd + i));
                a += key > T;
                e += key == T;
            }
            sh.ca[t] = a;
            sh.cb[t] = e;
        }
        WG_SYNC();
        WG_EACH(t) {
            if (t < 16) {
                int a = 0, e = 0;
                for (int j = 0; j < 16; ++j) {
                    a += sh.ca[16 * t + j];
                    e += sh.cb[16 * t + j];
                }
                sh.ba[t] = a;
                sh.bb[t] = e;
            }
        }
        WG_SYNC();
        WG_EACH(t) {
            const unsigned long long T = sh.prefix;
            const int need = sh.rem;
            int ga = 0, eb = 0;
            for (int j = 0; j < t / 16; ++j) {
                ga += sh.ba[j];
                eb += sh.bb[j];
            }
            for (int j = 16 * (t / 16); j < t; ++j) {
                ga += sh.ca[j];
                eb += sh.cb[j];
            }
            int off = ga + (eb < need ? eb : need);
            int seen = eb;
            const int lo = t * chunk < ncand ? t * chunk : ncand;
            const int hi = lo + chunk < ncand ? lo + chunk : ncand;
            for (int i = lo; i < hi; ++i) {
                const unsigned long long key = wg_key(c.C(cd + i));
                if (key > T) {
                    org[off++] = i;
                } else if (key == T) {
                    if (seen < need) org[off++] = i;
                    ++seen;
                }
            }
        }
        WG_SYNC();
    }
    const int nb = c.buf ^ 1;
    const int buf = c.buf;
    WG_EACH(t) {
        for (int r = t; r < k; r += kWg) c.C(c.Y.c_prob + r) = c.C(cd + org[r]);
        const long long tot = (long long)k * ii;
        for (long long e = t; e < tot; e += kWg) {
            const int r = (int)(e / ii), j = (int)(e % ii);
            const int from = div > 0 ? org[r] / div : org[r] % lin;
            c.Bt(c.Y.info(nb, r, j)) = c.Bt(c.Y.info(buf, from, j));
        }
    }
    WG_SYNC();
    c.buf = nb;
    return k;
}

// scl_least_reliable without the ratio scratch: the ratios are recomputed in every pass (the same
// rounded values), the picks and their tie rule are the lane kernel's
PCUB_HD void wg_least_reliable(SclCtx& c, int d, int slot, int S, int k, int* idx) {
    int taken = 0;
    for (int r = k - 1; r >= 0; --r) {
        int best = -1;
        double bv = 0.0;
        for (int p = 0; p < S; ++p) {
            bool used = false;
            for (int t = 0; t < taken; ++t) used = used || idx[k - 1 - t] == p;
            if (used) continue;
            const double v = scl_ratio(c, d, slot, p);
            if (best < 0 || v > bv) {
                best = p;
                bv = v;
            }
        }
        idx[r] = best;
        ++taken;
    }
}

// the actual path's metric update by one thread (actual_prob lives in LDS between barriers)
PCUB_HD void wg_scale_actual(SclWgCtx& g, double v, double w) {
    g.c.actual_prob = g.sh->ap;
    scl_scale_actual(g.c, v, w);
    g.sh->ap = g.c.actual_prob;
}

// scl_special over the workgroup
PCUB_HD int wg_special(SclWgCtx& g, int d, int u0, int ii, int side, int Lin, int nin) {
    SclCtx& c = g.c;
    const SclLayout& Y = c.Y;
    const int q = Y.q, L = Y.L, S = Y.N >> d;
    const long long mapo = Y.c_map + (long long)d * L;
    const long long pr = Y.c_prob;
    int* org = g.ints + g.W.i_org;
    const int ntr = c.track ? 1 : 0;
    if (S == 1) {
        if (nin == 1) {  // information leaf: q forks per path
            WG_EACH(t) {
                const long long mo = g.W.c_marg + 8LL * t;
                for (int i = t; i < Lin; i += kWg) {
                    scl_marginal(c, d, i, mo);
                    for (int s = 0; s < q; ++s) c.C(Y.c_cand + s * Lin + i) = scl_mul(c, c.C(pr + i), c.C(mo + s));
                }
            }
            WG_SYNC();
            const int k = wg_prune_commit(g, Lin * q, ii, 0, Lin);
            WG_EACH(t) {
                for (int r = t; r < k; r += kWg) {
                    const int i = org[r] % Lin, s = org[r] / Lin;
                    c.Bt(Y.info(c.buf, r, ii)) = (uint8_t)s;
                    c.Bt(Y.enc(d, side, r, 0)) = (uint8_t)s;
                    c.C(mapo + r) = (double)i;
                }
            }
            WG_SYNC();
            const double w = wg_normalize(g, k);
            if (c.track) {
                WG_EACH(t) {
                    if (t == 0) {
                        const int a = c.actual_sym(ii);
                        scl_marginal(c, d, L, g.W.c_marg);
                        wg_scale_actual(g, c.C(g.W.c_marg + a), w);
                        c.Bt(Y.enc(d, side, L, 0)) = (uint8_t)a;
                    }
                }
                WG_SYNC();
            }
            return k;
        }
        const int fv = wg_fval(c, c.fi);  // frozen leaf
        c.fi += 1;
        WG_EACH(t) {
            const long long mo = g.W.c_marg + 8LL * t;
            for (int i = t; i < Lin; i += kWg) {
                scl_marginal(c, d, i, mo);
                c.C(pr + i) = scl_mul(c, c.C(pr + i), c.C(mo + fv));
                c.Bt(Y.enc(d, side, i, 0)) = (uint8_t)fv;
                c.C(mapo + i) = (double)i;
            }
        }
        WG_SYNC();
        const double w = wg_normalize(g, Lin);
        if (c.track) {
            WG_EACH(t) {
                if (t == 0) {
                    scl_marginal(c, d, L, g.W.c_marg);
                    wg_scale_actual(g, c.C(g.W.c_marg + fv), w);
                    c.Bt(Y.enc(d, side, L, 0)) = (uint8_t)fv;
                }
            }
            WG_SYNC();
        }
        return Lin;
    }

    const long long tv = Y.b_tmp;                       // S bytes: a vector
    const long long tt = Y.b_tmp + (long long)q * Y.N;  // S bytes: transform temp
    const long long to = tt + Y.N;                      // S bytes: transform out
    if (nin == 0) {  // rate-0
        const int f0 = c.fi;
        c.fi += S;
        WG_EACH(t) {
            if (t == 0) {
                for (int j = 0; j < S; ++j) c.Bt(tv + j) = (uint8_t)wg_fval(c, f0 + j);
                scl_polar(c, tv, to, tt, S);
            }
        }
        WG_SYNC();
        WG_EACH(t) {
            for (int i = t; i < Lin; i += kWg) {
                c.C(pr + i) = scl_mul(c, c.C(pr + i), scl_prod_enc(c, d, i, S, to));
                c.C(mapo + i) = (double)i;
            }
            const long long tot = (long long)(Lin + ntr) * S;
            for (long long e = t; e < tot; e += kWg) {
                const int sl = (int)(e / S), j = (int)(e % S);
                c.Bt(Y.enc(d, side, sl < Lin ? sl : L, j)) = c.Bt(to + j);
            }
        }
        WG_SYNC();
        const double w = wg_normalize(g, Lin);
        if (c.track) {
            WG_EACH(t) {
                if (t == 0) wg_scale_actual(g, scl_prod_enc(c, d, L, S, to), w);
            }
            WG_SYNC();
        }
        return Lin;
    }
    if (nin == 1) {  // repetition: encodings of the q splits at b_tmp + s*N
        int kpos = 0;
        for (int j = 0; j < S; ++j)
            if (c.A->frozen[u0 + j] == 0) kpos = j;
        const int f0 = c.fi;
        c.fi += S - 1;
        WG_EACH(t) {
            if (t == 0) {
                int fi = f0;
                for (int j = 0; j < S; ++j) c.Bt(tv + j) = (uint8_t)(j == kpos ? 0 : wg_fval(c, fi++));
                for (int s = q - 1; s >= 0; --s) {  // split s at b_tmp + s*N (s = 0 last: tv is its input)
                    c.Bt(tv + kpos) = (uint8_t)s;
                    scl_polar(c, tv, to, tt, S);
                    for (int j = 0; j < S; ++j) c.Bt(Y.b_tmp + (long long)s * Y.N + j) = c.Bt(to + j);
                }
            }
        }
        WG_SYNC();
        const int nc = Lin * q;
        WG_EACH(t) {
            for (int e = t; e < nc; e += kWg) {
                const int i = e % Lin, s = e / Lin;
                c.C(Y.c_cand + e) = scl_mul(c, c.C(pr + i), scl_prod_enc(c, d, i, S, Y.b_tmp + (long long)s * Y.N));
            }
        }
        WG_SYNC();
        const int k = wg_prune_commit(g, nc, ii, 0, Lin);
        WG_EACH(t) {
            for (int r = t; r < k; r += kWg) {
                c.Bt(Y.info(c.buf, r, ii)) = (uint8_t)(org[r] / Lin);
                c.C(mapo + r) = (double)(org[r] % Lin);
            }
            const long long tot = (long long)k * S;
            for (long long e = t; e < tot; e += kWg) {
                const int r = (int)(e / S), j = (int)(e % S);
                c.Bt(Y.enc(d, side, r, j)) = c.Bt(Y.b_tmp + (long long)(org[r] / Lin) * Y.N + j);
            }
        }
        WG_SYNC();
        const double w = wg_normalize(g, k);
        if (c.track) {
            WG_EACH(t) {
                if (t == 0) {
                    const int a = c.actual_sym(ii);
                    wg_scale_actual(g, scl_prod_enc(c, d, L, S, Y.b_tmp + (long long)a * Y.N), w);
                    for (int j = 0; j < S; ++j) c.Bt(Y.enc(d, side, L, j)) = c.Bt(Y.b_tmp + (long long)a * Y.N + j);
                }
            }
            WG_SYNC();
        }
        return k;
    }
    // rate-1 (q^2 forks) / single parity check (q^3 forks)
    const bool spc = nin == S - 1;
    const int nfork_idx = spc ? 3 : 2;
    const int nsel = spc ? 4 : 2;
    int fork = q * q;
    if (spc) fork *= q;
    const int fv = spc ? wg_fval(c, c.fi) : 0;
    if (spc) c.fi += 1;
    int* lr = g.ints + g.W.i_lr;
    int* dl = g.ints + g.W.i_dl;
    WG_EACH(t) {
        for (int i = t; i < Lin; i += kWg) {
            int idx[4];
            wg_least_reliable(c, d, i, S, nsel, idx);
            // constant positions: argmax symbol and product of maxima, in position order
            double base = c.C(pr + i), pm = 1.0;
            bool first = true;
            int csum = 0;
            for (int j = 0; j < S; ++j) {
                bool sel = false;
                for (int u = 0; u < nsel; ++u) sel = sel || idx[u] == j;
                if (sel) continue;
                double mx;
                csum += scl_argmax(c, d, i, j, &mx);
                pm = first ? mx : (c.lg ? pm + mx : pm * mx);  // Python's sum from 0 / np.product
                first = false;
            }
            base = c.lg ? base + (first ? 0.0 : pm) : (first ? base * 1.0 : base * pm);
            c.C(g.W.c_base + i) = base;
            dl[i] = ((fv - csum) % q + q) % q;
            for (int u = 0; u < nsel; ++u) lr[4 * i + u] = idx[u];
        }
    }
    WG_SYNC();
    const int nc = Lin * fork;
    WG_EACH(t) {
        for (int e = t; e < nc; e += kWg) {
            const int i = e / fork, f = e % fork;
            const double base = c.C(g.W.c_base + i);
            int sym[4];
            int rem = f, ssum = 0;
            for (int u = nfork_idx - 1; u >= 0; --u) {
                sym[u] = rem % q;
                rem /= q;
                ssum += sym[u];
            }
            if (spc) sym[3] = ((dl[i] - ssum) % q + q) % q;
            double p = c.row(d, i, lr[4 * i], sym[0]);
            for (int u = 1; u < nsel; ++u) p = scl_mul(c, p, c.row(d, i, lr[4 * i + u], sym[u]));
            c.C(Y.c_cand + e) = c.lg ? p + base : p * base;
        }
    }
    WG_SYNC();
    const int k = wg_prune_commit(g, nc, ii, fork, Lin);
    WG_EACH(t) {
        const long long wo = g.W.b_wtmp + 2LL * Y.N * t;  // this thread's transform out, then temp
        for (int r = t; r < k; r += kWg) {
            const int i = org[r] / fork, f = org[r] % fork;
            const long long eo = Y.enc(d, side, r, 0);  // the fork's codeword part
            for (int j = 0; j < S; ++j) {
                double mx;
                c.Bt(eo + j) = (uint8_t)scl_argmax(c, d, i, j, &mx);
            }
            int rem = f, ssum = 0;
            for (int u = nfork_idx - 1; u >= 0; --u) {
                const int sv = rem % q;
                rem /= q;
                ssum += sv;
                c.Bt(eo + lr[4 * i + u]) = (uint8_t)sv;
            }
            if (spc) c.Bt(eo + lr[4 * i + 3]) = (uint8_t)(((dl[i] - ssum) % q + q) % q);
            scl_polar(c, eo, wo, wo + Y.N, S);
            const int off = spc ? 1 : 0;
            for (int j = 0; j + off < S; ++j) c.Bt(Y.info(c.buf, r, ii + j)) = c.Bt(wo + off + j);
            c.C(mapo + r) = (double)i;
        }
    }
    WG_SYNC();
    const double w = wg_normalize(g, k);
    if (c.track) {
        WG_EACH(t) {
            if (t == 0) {
                // T(actual information of the node) (T([frozen value] + information) for SPC)
                for (int j = 0; j < S; ++j) {
                    const int src = spc ? j - 1 : j;
                    c.Bt(tv + j) = (uint8_t)(src < 0 ? fv : c.actual_sym(ii + src));
                }
                scl_polar(c, tv, to, tt, S);
                wg_scale_actual(g, scl_prod_enc(c, d, L, S, to), w);
                for (int j = 0; j < S; ++j) c.Bt(Y.enc(d, side, L, j)) = c.Bt(to + j);
            }
        }
        WG_SYNC();
    }
    return k;
}

// one row of scl_minus: position h of path slot_in at depth d into slot_out at depth d + 1
PCUB_HD void wg_minus_pos(SclCtx& c, int d, int slot_in, int slot_out, int h) {
    const SclLayout& Y = c.Y;
    const int q = Y.q;
    double o[8];
    if (c.lg) {
        for (int u = 0; u < q; ++u) o[u] = -INFINITY;
        for (int x1 = 0; x1 < q; ++x1)
            for (int x2 = 0; x2 < q; ++x2) {
                const int u = (x1 + x2) % q;
                o[u] = scl_logaddexp(o[u], c.row(d, slot_in, 2 * h, x1) + c.row(d, slot_in, 2 * h + 1, x2));
            }
        scl_store_log(c, d + 1, slot_out, h, o);
        return;
    }
    for (int u = 0; u < q; ++u) o[u] = 0.0;
    for (int x1 = 0; x1 < q; ++x1)
        for (int x2 = 0; x2 < q; ++x2) {
            const int u = (x1 + x2) % q;
            o[u] = o[u] + c.row(d, slot_in, 2 * h, x1) * c.row(d, slot_in, 2 * h + 1, x2);
        }
    double s = 0.0;
    for (int u = 0; u < q; ++u) s = s + o[u];
    for (int u = 0; u < q; ++u) c.C(Y.dist(d + 1, slot_out, h, u)) = s != 0.0 ? o[u] / s : o[u];
}

// one row of scl_plus, given the minus child's symbol u1 at position h
PCUB_HD void wg_plus_pos(SclCtx& c, int d, int slot_in, int slot_out, int h, int u1) {
    const SclLayout& Y = c.Y;
    const int q = Y.q;
    double o[8];
    if (c.lg) {
        for (int u2 = 0; u2 < q; ++u2)
            o[u2] = scl_logaddexp(-INFINITY, c.row(d, slot_in, 2 * h, (u1 + u2) % q) +
                                                 c.row(d, slot_in, 2 * h + 1, (q - u2) % q));
        scl_store_log(c, d + 1, slot_out, h, o);
        return;
    }
    for (int u2 = 0; u2 < q; ++u2)
        o[u2] = 0.0 + c.row(d, slot_in, 2 * h, (u1 + u2) % q) * c.row(d, slot_in, 2 * h + 1, (q - u2) % q);
    double s = 0.0;
    for (int u = 0; u < q; ++u) s = s + o[u];
    for (int u = 0; u < q; ++u) c.C(Y.dist(d + 1, slot_out, h, u)) = s != 0.0 ? o[u] / s : o[u];
}

// scl_run over the workgroup: the same frame stack, every thread walking the same frames
PCUB_HD int wg_run(SclWgCtx& g) {
    SclCtx& c = g.c;
    const SclLayout& Y = c.Y;
    const int L = Y.L, q = Y.q;
    const int ntr = c.track ? 1 : 0;
    SclFrame st[kSclMaxDepth];
    int sp = 0, ret = 0;
    st[0] = SclFrame{0, 0, 0, 0, 1, 0};
    while (sp >= 0) {
        // the frame lives in private memory; its fields are the same in every thread
        SclFrame& fr = st[sp];
        SclFrame f{wg_uni(fr.d), wg_uni(fr.u0), wg_uni(fr.ii), wg_uni(fr.side), wg_uni(fr.Lin), wg_uni(fr.phase)};
        const int d = f.d, S = Y.N >> d, H = S / 2;
        const long long save = Y.c_save + (long long)d * L;
        const long long mapm = Y.c_map + (long long)(d + 1) * L;
        if (f.phase == 0) {
            const int nin = scl_nin(c, f.u0, S);
            if (scl_is_special(S, nin)) {
                ret = wg_special(g, d, f.u0, f.ii, f.side, f.Lin, nin);
                --sp;
                continue;
            }
            const long long tot = (long long)(f.Lin + ntr) * H;
            WG_EACH(t) {
                for (long long e = t; e < tot; e += kWg) {
                    const int sl = (int)(e / H), h = (int)(e % H);
                    const int so = sl < f.Lin ? sl : L;
                    wg_minus_pos(c, d, d == 0 ? 0 : so, so, h);
                }
            }
            WG_SYNC();
            fr.phase = 1;
            st[sp + 1] = SclFrame{d + 1, f.u0, f.ii, 0, f.Lin, 0};
            ++sp;
        } else if (f.phase == 1) {
            const int Lm = ret;
            WG_EACH(t) {
                for (int r = t; r < Lm; r += kWg) c.C(save + r) = c.C(mapm + r);
            }
            WG_SYNC();
            const int iim = f.ii + scl_nin(c, f.u0, H);
            const long long tot = (long long)(Lm + ntr) * H;
            WG_EACH(t) {
                for (long long e = t; e < tot; e += kWg) {
                    const int sl = (int)(e / H), h = (int)(e % H);
                    const int so = sl < Lm ? sl : L;
                    const int si = d == 0 ? 0 : (sl < Lm ? (int)c.C(save + sl) : L);
                    wg_plus_pos(c, d, si, so, h, c.Bt(Y.enc(d + 1, 0, so, h)));
                }
            }
            WG_SYNC();
            fr.phase = 2;
            st[sp + 1] = SclFrame{d + 1, f.u0 + H, iim, 1, Lm, 0};
            ++sp;
        } else {
            // scl_combine; ret = the plus child's list size = this node's
            const int Lp = ret;
            const long long mapo = Y.c_map + (long long)d * L;
            const long long tot = (long long)(Lp + ntr) * H;
            WG_EACH(t) {
                for (long long e = t; e < tot; e += kWg) {
                    const int sl = (int)(e / H), h = (int)(e % H);
                    const int r = sl < Lp ? sl : L;
                    const int mi = sl < Lp ? (int)c.C(mapm + sl) : L;
                    const int xm = c.Bt(Y.enc(d + 1, 0, mi, h)), xp = c.Bt(Y.enc(d + 1, 1, r, h));
                    c.Bt(Y.enc(d, f.side, r, 2 * h)) = (uint8_t)((xm + xp) % q);
                    c.Bt(Y.enc(d, f.side, r, 2 * h + 1)) = (uint8_t)((q - xp) % q);
                }
                for (int r = t; r < Lp; r += kWg) c.C(mapo + r) = (double)(int)c.C(save + (int)c.C(mapm + r));
            }
            WG_SYNC();
            --sp;
        }
    }
    return ret;
}

// decode codeword cw in slab slot `slot` (codeword-major) with the workgroup's shared block
PCUB_HD void scl_wg_decode_cw(const SclArgs& A, long long cw, long long slot, SclWgShared& sh) {
    SclWgCtx g;
    g.W.init(A.n, A.q, A.L, A.K);
    g.sh = &sh;
    SclCtx& c = g.c;
    c.A = &A;
    c.Y = g.W.Y;
    c.cw = cw;
    c.cells = A.cells + slot * g.W.ncells;
    c.bytes = A.bytes + slot * g.W.nbytes;
    c.ns = 1;
    c.fi = 0;
    c.buf = 0;
    c.track = A.actual != nullptr;
    c.lg = A.log != 0;
    c.actual_prob = c.lg ? 0.0 : 1.0;
    g.ints = (int*)(c.cells + g.W.c_int);
    WG_EACH(t) {
        if (t == 0) {
            sh.ap = c.lg ? 0.0 : 1.0;
            c.C(c.Y.c_prob) = c.lg ? 0.0 : 1.0;
        }
    }
    WG_SYNC();
    const int k = wg_run(g);
    const long long B = A.B;
    WG_EACH(t) {
        if (t == 0) {
            A.out_size[cw] = k;
            if (c.track && A.out_actual) A.out_actual[cw] = sh.ap;
        }
        for (int r = t; r < A.L; r += kWg) A.out_prob[(long long)r * B + cw] = r < k ? c.C(c.Y.c_prob + r) : 0.0;
        const long long tot = (long long)A.L * A.K;
        for (long long e = t; e < tot; e += kWg) {
            const int r = (int)(e / A.K), j = (int)(e % A.K);
            A.out_info[((long long)r * A.K + j) * B + cw] = r < k ? c.Bt(c.Y.info(c.buf, r, j)) : (uint8_t)0xff;
        }
    }
    WG_SYNC();  // the next codeword of this workgroup reuses the slab and the shared block
}

}  // namespace pcub
