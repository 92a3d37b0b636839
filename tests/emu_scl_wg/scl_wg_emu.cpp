// Test-only host build of the workgroup list decoder (scl_wg_body.h): the workgroup's 256 threads
// run one after another between barriers, one slab slot, one codeword at a time.  The same code
// runs on the GPU in k_scl_wg (scl_wg.hip); tests/test_scl_wide.py checks this build against the
// oracle's restatement (oracle/scl_oracle.py) and its selection against scl_prune / scl_commit.
#include <stdint.h>

#include <vector>

#include "scl_wg_body.h"

namespace {

struct Slab {
    pcub::SclWgLayout W;
    std::vector<double> cells;
    std::vector<uint8_t> bytes;
    Slab(int n, int q, int L, int K) {
        W.init(n, q, L, K);
        cells.assign((size_t)W.ncells, 0.0);
        bytes.assign((size_t)W.nbytes, 0);
    }
};

}  // namespace

extern "C" int emu_scl_wg(const double* xy, long long B, int q, int n, int L, const uint8_t* frozen,
                          const uint8_t* fvals, int nF, const uint8_t* actual, int K, uint8_t* out_info,
                          double* out_prob, int* out_size, double* out_actual, int use_log) {
    Slab s(n, q, L, K);
    pcub::SclWgShared sh;
    pcub::SclArgs A;
    A.xy = xy;
    A.B = B;
    A.n = n;
    A.q = q;
    A.L = L;
    A.K = K;
    A.frozen = frozen;
    A.fvals = fvals;
    A.nF = nF;
    A.actual = actual;
    A.out_info = out_info;
    A.out_prob = out_prob;
    A.out_size = out_size;
    A.out_actual = out_actual;
    A.log = use_log;
    A.cells = s.cells.data();
    A.bytes = s.bytes.data();
    A.ns = 1;
    for (long long cw = 0; cw < B; ++cw) pcub::scl_wg_decode_cw(A, cw, 0, sh);
    return 0;
}

// wg_prune_commit alone on ncand candidate metrics (ncand <= L q^3): the kept candidates in
// origin[] (ascending) and their metrics in prob[]; returns the kept count
extern "C" int emu_wg_select(const double* cand, int ncand, int q, int L, int use_log, int* origin, double* prob) {
    Slab s(0, q, L, 1);
    if ((long long)ncand > (long long)L * q * q * q) return -1;
    pcub::SclWgShared sh;
    pcub::SclArgs A = {};
    A.log = use_log;
    pcub::SclWgCtx g;
    g.W = s.W;
    g.sh = &sh;
    g.c.A = &A;
    g.c.Y = s.W.Y;
    g.c.cw = 0;
    g.c.cells = s.cells.data();
    g.c.bytes = s.bytes.data();
    g.c.ns = 1;
    g.c.fi = 0;
    g.c.buf = 0;
    g.c.track = false;
    g.c.lg = use_log != 0;
    g.c.actual_prob = 0.0;
    g.ints = (int*)(g.c.cells + g.W.c_int);
    for (int i = 0; i < ncand; ++i) g.c.C(g.c.Y.c_cand + i) = cand[i];
    const int k = pcub::wg_prune_commit(g, ncand, 0, 0, ncand);
    for (int r = 0; r < k; ++r) {
        origin[r] = g.ints[g.W.i_org + r];
        prob[r] = g.c.C(g.c.Y.c_prob + r);
    }
    return k;
}
