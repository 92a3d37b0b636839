"""The memoryless genie pipeline on the GPU: pcub_sc_genie_bin's leaves against the C oracle and
against pcub_sc_leaf_bin bit for bit, its counters against pcub_sc_leaf_bin + pcub_genie_count
integer for integer, pcub_mc_genie_bin against the composed generators, and the law of the counts
against closed forms and the degrading construction."""
import math

import numpy as np
import pytest

from tests.conftest import edge_long_cases
from tests.test_genie_bin import (bits, class_counts, compact_rows, expand, marginals, oracle_leaves, pack_u,
                                  raw_rows)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# N = 2: the root is the leaves' parent; 4, 8: fewer pairs than work items; 16, 32: a partial and a
# whole u word; 128 | 256: a work item first owns two pairs; 256 | 512 and 2048 | 4096: the
# workgroup grows to 256 and to 1024 work items; 1024; 8192: the largest.
LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.view(dtype)).to("cuda")


def words_dev(u):
    return dev(pack_u(u), torch.int32)


def all_frozen(N):
    from polarcub_amd import sc
    return sc.CodeSpec(N, np.ones(N, np.uint8), np.zeros(N, np.uint8), device="cuda")


def composed(xy_rows, u):
    """The parent's route: [B, N, 2] rows -> pcub_sc_leaf_bin with every position frozen to u ->
    pcub_genie_count.  Returns (counters [1 + 2N], leaf [N, B] numpy)."""
    from polarcub_amd import mc, sc
    B, N, _ = xy_rows.shape
    _, _, leaf = sc.LeafDecoder(all_frozen(N)).decode_native(sc.transpose_pairs(dev(xy_rows)), dev(u))
    t, w, ti = mc.genie_count(leaf, words_dev(u), N)
    return np.concatenate([[t], w, ti]).astype(np.int64), leaf.cpu().numpy()


def fused(rows, u, compact, want_leaf=True, block=0):
    from polarcub_amd import sc
    N = u.shape[1]
    out = sc.GenieBinCounter(N, "cuda").count(dev(rows), words_dev(u), compact=compact, want_leaf=want_leaf,
                                              block=block)
    c = np.concatenate([[out[0]], out[1], out[2]]).astype(np.int64)
    return c, (out[3].cpu().numpy() if want_leaf else None)


# -- leaves ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", LENGTHS)
def test_leaves_match_the_oracle(n):
    """Both root forms, random u, rows with one-sided zeros, (0, 0) pairs and exact ties: the leaf
    marginals are the C oracle's bit for bit, and the counters are genie_class's on the leaves."""
    N, B = 1 << n, 5 if n <= 10 else 3
    for compact in (False, True):
        rng = np.random.default_rng(40 * n + compact)
        u = rng.integers(0, 2, (B, N)).astype(np.uint8)
        rows = compact_rows("edge", B, N, rng) if compact else raw_rows("edge", B, N, rng)
        want = oracle_leaves(expand(rows) if compact else rows, u)
        c, leaf = fused(rows, u, compact)
        assert np.array_equal(bits(marginals(leaf.T)), bits(want)), (n, compact)
        assert np.array_equal(c, class_counts(leaf, u)), (n, compact)


def test_edge_long_rows_match_the_leaf_kernel():
    """The reference's edge families at N = 1024 / 4096 (subnormal, underflow, one-sided zeros, ties)
    with random u: leaves equal pcub_sc_leaf_bin's on the same rows and u bit for bit, counters equal
    pcub_genie_count's."""
    for i, c in enumerate(edge_long_cases()):
        xy = np.ascontiguousarray(c["xy"], np.float64)
        B, N, _ = xy.shape
        u = np.random.default_rng(900 + i).integers(0, 2, (B, N)).astype(np.uint8)
        cc, cleaf = composed(xy, u)
        fc, fleaf = fused(xy, u, False)
        assert np.array_equal(bits(fleaf), bits(cleaf)), (i, c["family_name"], N)
        assert np.array_equal(fc, cc), (i, c["family_name"], N)


# -- counters ----------------------------------------------------------------------------------------

_N64 = {}


def n64_case(B):
    """N = 64 rows and u of B trials with the composed route's counters, computed once."""
    if B not in _N64:
        rng = np.random.default_rng(B)
        u = rng.integers(0, 2, (B, 64)).astype(np.uint8)
        rows = raw_rows("edge", B, 64, rng)
        _N64[B] = (rows, u, composed(rows, u)[0])
    return _N64[B]


@pytest.mark.parametrize("B,block", [(1, 0), (100, 0), (20011, 0), (5003, 256), (5003, 1024)])
def test_counters_match_the_composed_route(B, block):
    """B = 1; B below the grid; B above resident workgroups x 1 with a remainder: 20,011 trials over
    at most 32 one-wave workgroups a CU, and 5,003 over the few 256- and 1024-item workgroups a CU
    holds, so a workgroup takes several trials and flushes once.  With and without the leaf output."""
    rows, u, want = n64_case(B)
    assert want[0] == B and want[1:].sum() > 0
    with_leaf, leaf = fused(rows, u, False, True, block)
    without, _ = fused(rows, u, False, False, block)
    assert np.array_equal(with_leaf, want) and np.array_equal(without, want)
    assert np.array_equal(with_leaf, class_counts(leaf, u))


def test_counters_accumulate():
    """Counters are added to, not overwritten: two calls into one buffer."""
    from polarcub_amd import _lib, sc
    rows, u, want = n64_case(100)
    counters = torch.zeros(1 + 2 * 64, dtype=torch.int64, device="cuda")
    r, w = dev(rows), words_dev(u)
    for _ in range(2):
        _lib.check(_lib.lib().pcub_sc_genie_bin(sc._p(r), 0, sc._p(w), 100, 6, sc._p(counters), None, sc._stream()),
                   "pcub_sc_genie_bin")
    assert np.array_equal(counters.cpu().numpy(), 2 * want)


# -- pipeline ----------------------------------------------------------------------------------------

def composed_pipeline(n, channel, param, seed, offset, count):
    """The existing generators, pcub_sc_leaf_bin and pcub_genie_count at the same (seed, offset)."""
    from polarcub_amd import mc, sc
    N = 1 << n
    rate1 = sc.CodeSpec(N, np.zeros(N, np.uint8), np.zeros(N, np.uint8), device="cuda")
    info, xy = mc.philox_norm_batch(rate1, seed, offset, count, channel, param, compact=False)
    _, _, leaf = sc.LeafDecoder(all_frozen(N)).decode_native(xy, sc.unpack(info, N))
    t, w, ti = mc.genie_count(leaf, info, N)
    return np.concatenate([[t], w, ti]).astype(np.int64)


def run(n, channel, param, seed, offset, count, chunk=None):
    from polarcub_amd import mc
    t, w, ti = mc.run_genie_bin(n, channel, param, seed, offset, count, chunk=chunk)
    return np.concatenate([[t], w, ti]).astype(np.int64)


@pytest.mark.parametrize("channel,param", [(0, 0.63), (1, 0.11)])
def test_pipeline_matches_the_composed_generators(channel, param):
    n, seed = 8, 77
    want = composed_pipeline(n, channel, param, seed, 0, 256)
    assert want[0] == 256 and want[1:1 + 256].sum() > 0
    assert np.array_equal(run(n, channel, param, seed, 0, 256), want)
    assert np.array_equal(run(n, channel, param, seed, 0, 100) + run(n, channel, param, seed, 100, 156), want)
    for chunk in (1, 7, 64):
        assert np.array_equal(run(n, channel, param, seed, 0, 256, chunk=chunk), want), chunk


def test_pipeline_past_the_kernel_lengths_composes_the_leaf_kernel():
    """N = 16384: the entry composes pcub_sc_leaf_bin + pcub_genie_count in its own workspace."""
    from polarcub_amd import sc
    assert not sc.genie_bin_supported(1 << 14) and sc.genie_bin_supported(1 << 13)
    want = composed_pipeline(14, 0, 0.63, 5, 3, 6)
    assert np.array_equal(run(14, 0, 0.63, 5, 3, 6, chunk=4), want)


# -- law ---------------------------------------------------------------------------------------------

def test_bsc_n2_closed_forms():
    """BSC(p), N = 2, T = 2^18.  u_0 sees the minus channel BSC(2p(1 - p)) and never ties; u_1 given
    u_0 sees two copies: wrong when both flipped (p^2), and a disagreeing pair gives fl(r * 1)
    against fl(1 * r), an exact tie (2p(1 - p)).  Each frequency is a binomial mean over T trials:
    within 5 standard deviations sqrt(q (1 - q) / T) of its closed form q."""
    p, T = 0.11, 1 << 18
    t, wrong, tie = (lambda c: (c[0], c[1:3], c[3:5]))(run(1, 1, p, 2024, 0, T))
    assert t == T and tie[0] == 0
    for got, q in [(wrong[0], 2 * p * (1 - p)), (wrong[1], p * p), (tie[1], 2 * p * (1 - p))]:
        sd = math.sqrt(q * (1 - q) / T)
        print("N=2 BSC: estimate %.6f closed form %.6f sd %.2e" % (got / T, q, sd))
        assert abs(got / T - q) <= 5 * sd


def test_genie_pe_is_below_the_degraded_construction():
    """BSC(0.11), n = 6: degrading only raises Pe, so the genie's Pe[i] is at most the degraded
    channel's Pe_d[i] of construction.tv_pe up to noise.  A trial's value is in [0, 1] with mean at
    most Pe_d <= 1/2, so its variance is at most Pe_d (1 - Pe_d): sigma = sqrt(Pe_d (1 - Pe_d) / T)."""
    from polarcub_amd import coding, construction, scalar
    T = 1 << 18
    _, pe_deg = construction.tv_pe(6, 16, None, scalar.makeBSC(0.11).probs)
    c = run(6, 1, 0.11, 31, 0, T)
    pe = np.array(coding.genie_pe_from_counts(c[0], c[1:65], c[65:]))
    sigma = np.sqrt(pe_deg * (1.0 - pe_deg) / T)
    print("max (Pe - Pe_d) / sigma:", float(np.max((pe - pe_deg) / np.maximum(sigma, 1e-300))))
    assert np.all(pe <= pe_deg + 5 * sigma)
    assert pe.min() < 1e-3 and pe.max() > 0.4  # polarised, and the counts are not all zero
