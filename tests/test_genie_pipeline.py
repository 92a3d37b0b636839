"""The genie pipeline's statistic on the CPU (tests/emu_genie/genie_emu.cpp over
polarcub_amd/csrc/genie_body.h, the function the kernel of sc_genie.hip calls): the class of crafted
and random compact leaves against coding._genie_stats on a numpy restatement of the leaf marginals,
the host-side argument checks of the loaded library (no GPU needed: every call made here returns
before a launch), the counts-to-frozen-set arithmetic and the CLI flag."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

P = ctypes.c_void_p
CORRECT, TIE, WRONG = 0, 1, 2
PE_OF_CLASS = {CORRECT: 0.0, TIE: 0.5, WRONG: 1.0}


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu_genie")], check=True)
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emu_genie", "build", "libgenieemu.so"))
    lib.emu_genie_classes.argtypes = [P, P, ctypes.c_longlong, P]
    lib.emu_genie_count.argtypes = [P, P, ctypes.c_longlong, ctypes.c_int, P]
    return lib


def _ptr(a):
    return a.ctypes.data_as(P)


# -- the host statistic ------------------------------------------------------------------------------
def np_leaf_marginals(v):
    """leaf_marginal (sc_leaf.hip) in numpy: +r = (1, r), -r = (r, 1), NaN = (0, 0); s = 0 + p0 + p1;
    m = p / s, or (0.5, 0.5) when s = 0.  [count] -> [count, 2]."""
    v = np.asarray(v, np.float64)
    r, neg = np.abs(v), np.signbit(v)
    p0, p1 = np.where(neg, r, 1.0), np.where(neg, 1.0, r)
    p0[np.isnan(r)] = 0.0
    p1[np.isnan(r)] = 0.0
    s = (0.0 + p0) + p1
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([np.where(s > 0.0, p0 / s, 0.5), np.where(s > 0.0, p1 / s, 0.5)], axis=1)


def host_classes(v, u):
    """coding._genie_stats(m, u, False) on the marginals of the leaves v, as class codes."""
    from polarcub_amd import coding
    pe, h = coding._genie_stats(np_leaf_marginals(v), np.asarray(u, np.int64), False)
    assert h == []
    back = {0.0: CORRECT, 0.5: TIE, 1.0: WRONG}
    return np.array([back[x] for x in pe], np.int32)


def crafted_leaves(rng, randoms):
    """Compact leaves at every edge of the representation, then `randoms` random ones (a quarter of
    them within a few ulps of 1), each listed once: the callers pair every one with u = 0 and u = 1."""
    edge = [0.0, -0.0, 1.0, -1.0, 1.0 - 2.0 ** -53, -(1.0 - 2.0 ** -53), 2.0 ** -1074, -(2.0 ** -1074), 0.5, -0.5,
            float("nan"), -float("nan"), 2.0 ** -1022, -(2.0 ** -1022), 1.0 - 2.0 ** -52, -(1.0 - 2.0 ** -52)]
    r = rng.random(randoms)
    near = np.ones(randoms // 4)
    for _ in range(4):  # 0 .. 4 ulps below 1
        near = np.where(rng.random(near.size) < 0.5, np.nextafter(near, 0.0), near)
    r[:near.size] = near
    r[near.size:near.size + 8] = [0.0, 1.0, 0.0, 1.0, 0.5, 0.5, 1.0, 0.0]
    sign = np.where(rng.random(randoms) < 0.5, -1.0, 1.0)
    return np.concatenate([np.array(edge), np.copysign(r, sign)])


def crafted_batch(N, B, seed):
    """leaf [N, B] f64, u [B, N] u8 and u_words [ceil(N/32), B] u32 with all three classes at both
    values of u in the batch: the edge leaves spread over the first rows, random ones elsewhere."""
    rng = np.random.default_rng(seed)
    v = crafted_leaves(rng, max(64, N * B))
    leaf = rng.permutation(v)[:N * B].reshape(N, B).copy()
    edge = v[:16]
    for k in range(min(N, 32)):  # row k carries edge value k // 2 in column k % B, u alternating
        leaf[k, k % B] = edge[k // 2]
    u = (rng.random((B, N)) < 0.5).astype(np.uint8)
    for k in range(min(N, 32)):
        u[k % B, k] = k & 1
    words = np.zeros(((N + 31) // 32, B), np.uint32)
    for i in range(N):
        words[i >> 5] |= u[:, i].astype(np.uint32) << np.uint32(i & 31)
    return np.ascontiguousarray(leaf), u, words


def host_counts(leaf, u):
    """[1 + 2N] counters of one batch through _genie_stats: trials, wrong a position, ties a position."""
    N, B = leaf.shape
    wrong, tie = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for b in range(B):
        c = host_classes(leaf[:, b], u[b])
        wrong += c == WRONG
        tie += c == TIE
    return np.concatenate([[B], wrong, tie]).astype(np.int64)


def test_classifier_matches_the_host_statistic(emu):
    rng = np.random.default_rng(7)
    v = crafted_leaves(rng, 4000)
    v = np.concatenate([v, v])
    u = np.concatenate([np.zeros(v.size // 2, np.uint8), np.ones(v.size // 2, np.uint8)])
    cls = np.full(v.size, -1, np.int32)
    assert emu.emu_genie_classes(_ptr(v), _ptr(u), v.size, _ptr(cls)) == 0
    want = host_classes(v, u)
    assert np.array_equal(cls, want), np.flatnonzero(cls != want)[:10]
    # every class occurs at both values of u
    for bit in (0, 1):
        assert set(cls[u == bit].tolist()) == {CORRECT, TIE, WRONG}
    half = v.size // 2
    for k in (10, 11):  # NaN of either sign: (0.5, 0.5)
        assert np.isnan(v[k]) and cls[k] == TIE and cls[half + k] == TIE


def test_edge_classes_by_hand(emu):
    """The ten finite edge leaves, their classes written out: (u = 0, u = 1)."""
    v = np.array([0.0, -0.0, 1.0, -1.0, 1.0 - 2.0 ** -53, -(1.0 - 2.0 ** -53), 2.0 ** -1074, -(2.0 ** -1074), 0.5, -0.5])
    plus, minus, tie = (CORRECT, WRONG), (WRONG, CORRECT), (TIE, TIE)
    want = [plus, minus, tie, tie, plus, minus, plus, minus, plus, minus]
    for bit in (0, 1):
        u = np.full(v.size, bit, np.uint8)
        cls = np.full(v.size, -1, np.int32)
        emu.emu_genie_classes(_ptr(v), _ptr(u), v.size, _ptr(cls))
        assert cls.tolist() == [w[bit] for w in want]
        assert np.array_equal(cls, host_classes(v, u))
    # the marginals at the last value below 1 are 1/2 and 1/2 - 2^-54: apart, as genie_body.h says
    m = np_leaf_marginals([1.0 - 2.0 ** -53])
    assert m[0, 0] == 0.5 and m[0, 1] == 0.5 - 2.0 ** -54


@pytest.mark.parametrize("N,B", [(64, 5), (2, 3), (32, 1)])
def test_counts_over_a_batch(emu, N, B):
    """The [N][B] / [ceil(N/32)][B] indexing of genie_class_at, and accumulation."""
    leaf, u, words = crafted_batch(N, B, 11 * N + B)
    counters = np.zeros(1 + 2 * N, np.uint64)
    assert emu.emu_genie_count(_ptr(leaf), _ptr(words), B, N.bit_length() - 1, _ptr(counters)) == 0
    want = host_counts(leaf, u)
    assert np.array_equal(counters.astype(np.int64), want)
    if N >= 32:
        assert want[1:1 + N].sum() > 0 and want[1 + N:].sum() > 0
    emu.emu_genie_count(_ptr(leaf), _ptr(words), B, N.bit_length() - 1, _ptr(counters))
    assert np.array_equal(counters.astype(np.int64), 2 * want)


# -- the loaded library, host side -------------------------------------------------------------------
def test_invalid_arguments_return_einval_before_any_launch():
    """Every rejected call: one argument wrong, the others valid (the pointers are never read on the
    host, and no call here gets as far as a launch)."""
    from polarcub_amd import _lib
    L = _lib.lib()
    fake = P(1 << 20)
    assert L.pcub_genie_count(None, fake, 4, 6, fake, None) == _lib.EINVAL
    assert L.pcub_genie_count(fake, None, 4, 6, fake, None) == _lib.EINVAL
    assert L.pcub_genie_count(fake, fake, 4, 6, None, None) == _lib.EINVAL
    assert L.pcub_genie_count(fake, fake, -1, 6, fake, None) == _lib.EINVAL
    assert L.pcub_genie_count(fake, fake, 4, 0, fake, None) == _lib.EINVAL
    assert L.pcub_genie_count(fake, fake, 4, 25, fake, None) == _lib.EINVAL
    assert L.pcub_genie_count(fake, fake, 0, 6, fake, None) == 0  # nothing to do is not an error

    W = 300
    need = L.pcub_mc_genie_deletion_workspace(10, 8, W)
    assert need >= 10 * (8 * 256 + 2 * 4 * 8 + W + 4)
    assert L.pcub_mc_genie_deletion_workspace(20, 8, W) > need
    ok = dict(seed=1, offset=0, count=10, n=8, n0=2, tmpl=fake, W=W, ones=0, pd=0.1, chunk=10, counters=fake,
              workspace=fake, workspace_bytes=need, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.pcub_mc_genie_deletion(a["seed"], a["offset"], a["count"], a["n"], a["n0"], a["tmpl"], a["W"],
                                        a["ones"], a["pd"], a["chunk"], a["counters"], a["workspace"],
                                        a["workspace_bytes"], a["stream"])
    assert L.pcub_sc_leaf_deletion_supported(8, 2, 0) == 1
    assert L.pcub_sc_deletion_supported(15, 5, 0) == 1 and L.pcub_sc_leaf_deletion_supported(15, 5, 0) == 0
    wrong = [dict(counters=None), dict(tmpl=None), dict(workspace=None), dict(n=15, n0=5, ones=0, workspace_bytes=1 << 50),
             dict(n=13, n0=4, ones=1, workspace_bytes=1 << 50), dict(n=8, n0=8), dict(n=8, n0=0), dict(pd=1.5),
             dict(pd=-0.1), dict(pd=float("nan")), dict(chunk=0), dict(chunk=-3), dict(workspace_bytes=need - 1),
             dict(workspace_bytes=0), dict(count=-1), dict(offset=-1), dict(W=0), dict(W=-1)]
    for kw in wrong:
        assert call(**kw) == _lib.EINVAL, kw
    assert call(count=0) == 0  # nothing to do: no launch either
    for bad in [(0, 8, W), (-1, 8, W), (10, 0, W), (10, 25, W), (10, 8, 0), (10, 8, -1), (1 << 62, 8, W)]:
        assert L.pcub_mc_genie_deletion_workspace(*bad) == 0, bad


def test_exports_are_declared_and_bound():
    from polarcub_amd import _lib
    L = _lib.lib()
    for name in ("pcub_genie_count", "pcub_mc_genie_deletion_workspace", "pcub_mc_genie_deletion"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes
    assert L.pcub_abi_version() == 4


# -- counts -> Pe -> frozen set ------------------------------------------------------------------------
def test_counts_to_frozen_set(capsys):
    from polarcub_amd import coding
    trials = 10
    wrong = np.array([0, 5, 0, 1, 0, 0, 10, 0], np.int64)
    tie = np.array([0, 0, 2, 0, 0, 1, 0, 0], np.int64)
    Pe = coding.genie_pe_from_counts(trials, wrong, tie)
    assert Pe == [0.0, 0.5, 0.1, 0.1, 0.0, 0.05, 1.0, 0.0]
    # what the trial-by-trial accumulation of _genie_stats' 0 / 0.5 / 1 gives, divided at the end
    assert Pe == [(w * 1.0 + t * 0.5) / trials for w, t in zip(wrong, tie)]
    # ascending TV + Pe (stable): 0, 4, 7 (0), 5 (0.05), 2 (0.1) add up to 0.15 <= 0.2; 3 (0.1) does not fit
    assert coding.frozenSetFromTVAndPe([0.0] * 8, Pe, 0.2) == {1, 3, 6}
    assert coding.frozenSetFromTVAndPe([0.0] * 8, Pe, 0.04) == {1, 2, 3, 5, 6}
    capsys.readouterr()


def test_device_genie_needs_n_above_n0():
    from polarcub_amd import coding
    with pytest.raises(ValueError):
        coding.genieEncodeDecodeSimulationDevice(3, 3, 0.1, 0.1, 8, 0.1, 300)


# -- the CLI flag --------------------------------------------------------------------------------------
def test_cli_flag_parses_and_defaults_to_off():
    from polarcub_amd.cli import main_deletion
    ap = main_deletion.parser()
    assert ap.parse_args(["-n", "8"]).device_genie is False
    assert ap.parse_args(["-n", "8", "-g"]).device_genie is False
    a = ap.parse_args(["-n", "8", "-n0", "2", "-g", "64", "--device-genie", "-gs", "300"])
    assert a.device_genie is True and a.genie_simulations == 64 and a.genie_seed == 300 and a.n0 == 2
