"""The memoryless genie pipeline on the CPU: the breadth-first kernel body
(polarcub_amd/csrc/genie_bin_body.h) compiled for the host with its work items run one after another
and its LDS arrays as exactly sized heap arrays (tests/emu_genie_bin/genie_bin_emu.cpp) against the C
oracle's leaves and against genie_class on them; the new symbols and their argument checks (every
call made here returns before a launch); the CLI parser and the counts -> file -> reader round trip."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import orc
from tests.conftest import ROOT, awgn_like

P = ctypes.c_void_p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(P)


# -- helpers shared with tests/test_gpu_genie_bin.py ---------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def marginals(leaf):
    """Compact leaves -> the reference's marginals, as pcub_leaf_marginals computes them:
    s = 0 + p0 + p1, m = p / s, (0.5, 0.5) for the (0, 0) leaf."""
    leaf = np.asarray(leaf, np.float64)
    s, r = np.signbit(leaf), np.abs(leaf)
    nan = np.isnan(r)
    p0 = np.where(nan, 0.0, np.where(s, r, 1.0))
    p1 = np.where(nan, 0.0, np.where(s, 1.0, r))
    tot = (0.0 + p0) + p1
    safe = np.where(tot > 0.0, tot, 1.0)
    return np.stack([np.where(tot > 0.0, p0 / safe, 0.5), np.where(tot > 0.0, p1 / safe, 0.5)], axis=-1)


def pack_u(u):
    """[B, N] 0/1 -> [ceil(N/32), B] uint32 words (bit t of word w = bit 32 w + t)."""
    B, N = u.shape
    words = np.zeros(((N + 31) // 32, B), np.uint32)
    for i in range(N):
        words[i >> 5] |= u[:, i].astype(np.uint32) << np.uint32(i & 31)
    return words


def expand(c):
    """Compact rows -> the pairs they stand for: +r = (1, r), -r = (r, 1), NaN = (0, 0)."""
    s, r = np.signbit(c), np.abs(c)
    nan = np.isnan(r)
    p0 = np.where(nan, 0.0, np.where(s, r, 1.0))
    p1 = np.where(nan, 0.0, np.where(s, 1.0, r))
    return np.ascontiguousarray(np.stack([p0, p1], axis=-1))


def oracle_leaves(xy, u):
    """The C oracle's leaf marginals [B, N, 2], all positions frozen to the trial's u, one call a trial."""
    B, N, _ = xy.shape
    out = np.empty((B, N, 2))
    ones = np.ones(N, np.uint8)
    for b in range(B):
        out[b] = orc.decode_bin(xy[b:b + 1], ones, u[b], leaf=True)[2][0]
    return out


def class_counts(leaf, u):
    """genie_class (genie_body.h) over compact leaves [N, B] and true bits [B, N]: tie when not
    r < 1 (r = 1 or the NaN of (0, 0)), else correct iff the sign is the true bit.
    Returns the [1 + 2N] counters."""
    N, B = leaf.shape
    r, s = np.abs(leaf), np.signbit(leaf)
    tie = ~(r < 1.0)
    wrong = ~tie & (s != (u.T != 0))
    return np.concatenate([[B], wrong.sum(axis=1), tie.sum(axis=1)]).astype(np.int64)


def raw_rows(kind, B, N, rng):
    """[B, N, 2] joint pairs: 'bsc' (makeBSC rows at p = 0.11), 'awgn' (likelihood pairs with one-sided
    zeros), 'edge' ((0, 0) pairs, exact ties, one-sided zeros and unnormalised scales)."""
    if kind == "bsc":
        y = rng.integers(0, 2, (B, N))
        hi, lo = 0.5 * (1.0 - 0.11), 0.5 * 0.11
        return np.ascontiguousarray(np.stack([np.where(y == 0, hi, lo), np.where(y == 0, lo, hi)], axis=-1))
    xy = awgn_like(B, N, rng, zeros=0.0)
    side = rng.integers(0, 2, (B, N))
    z = rng.random((B, N)) < 0.1
    xy[..., 0] = np.where(z & (side == 0), 0.0, xy[..., 0])
    xy[..., 1] = np.where(z & (side == 1), 0.0, xy[..., 1])
    if kind == "edge":
        xy *= rng.choice([1.0, 3.7, 1e-3, 250.0], size=(B, N, 1))
        xy[rng.random((B, N)) < 0.05] = 0.0
        t = rng.random((B, N)) < 0.25
        xy[..., 1] = np.where(t, xy[..., 0], xy[..., 1])
    return np.ascontiguousarray(xy)


def compact_rows(kind, B, N, rng):
    """[B, N] compact rows of the same families."""
    if kind == "bsc":
        r = 0.11 / 0.89
        return np.where(rng.integers(0, 2, (B, N)) == 0, r, -r)
    c = np.copysign(np.exp(-np.abs(rng.normal(2.0, 2.0, (B, N)))), rng.choice([-1.0, 1.0], size=(B, N)))
    c = np.where(rng.random((B, N)) < 0.1, np.copysign(0.0, c), c)
    if kind == "edge":
        c = np.where(rng.random((B, N)) < 0.05, np.nan, c)
        c = np.where(rng.random((B, N)) < 0.25, np.copysign(1.0, c), c)
    return np.ascontiguousarray(c)


KINDS = ("bsc", "awgn", "edge")


# -- host emulation of the kernel body ---------------------------------------------------------

@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu_genie_bin")], check=True)
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emu_genie_bin", "build", "libgeniebinemu.so"))
    lib.emu_genie_bin.argtypes = [P, ctypes.c_int, P, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, P, P]
    return lib


def emu_run(emu, rows, compact, u, lanes):
    B, N = u.shape
    counters = np.zeros(1 + 2 * N, np.uint64)
    leaf = np.zeros((N, B))
    words = pack_u(u)
    rows = np.ascontiguousarray(rows, np.float64)
    assert emu.emu_genie_bin(_ptr(rows), int(compact), _ptr(words), B, N.bit_length() - 1, lanes, _ptr(counters),
                             _ptr(leaf)) == 0
    return counters.astype(np.int64), leaf


@pytest.mark.parametrize("n", range(1, 11))
def test_emulated_level_pass_matches_oracle(emu, n):
    """Every N = 2 .. 1024, both root forms, the three row families, three trials with random u: the
    compact leaves give the C oracle's marginals bit for bit, and the counts are genie_class's on
    those leaves.  64 and 256 work items (fewer, as many and more pairs than work items)."""
    N, B = 1 << n, 3
    seen = np.zeros(3, np.int64)
    for ki, kind in enumerate(KINDS):
        for compact in (False, True):
            rng = np.random.default_rng(100 * n + 10 * ki + compact)
            u = rng.integers(0, 2, (B, N)).astype(np.uint8)
            rows = compact_rows(kind, B, N, rng) if compact else raw_rows(kind, B, N, rng)
            want = oracle_leaves(expand(rows) if compact else rows, u)
            for lanes in (64, 256):
                counters, leaf = emu_run(emu, rows, compact, u, lanes)
                assert np.array_equal(bits(marginals(leaf.T)), bits(want)), (n, kind, compact, lanes)
                ref = class_counts(leaf, u)
                assert np.array_equal(counters, ref), (n, kind, compact, lanes)
            seen += [B * N - ref[1:].sum(), ref[1:1 + N].sum(), ref[1 + N:].sum()]
    assert np.all(seen > 0)  # correct, wrong and tie leaves all occur


def test_emulated_counts_accumulate_over_calls_and_trials(emu):
    """The counts of 40 trials in one call equal those of two calls into the same counters."""
    N, B = 64, 40
    rng = np.random.default_rng(5)
    u = rng.integers(0, 2, (B, N)).astype(np.uint8)
    rows = raw_rows("edge", B, N, rng)
    whole, leaf = emu_run(emu, rows, False, u, 64)
    a, _ = emu_run(emu, rows[:13], False, u[:13], 64)
    b, _ = emu_run(emu, rows[13:], False, u[13:], 256)
    assert whole[0] == B and np.array_equal(whole, a + b)
    assert np.array_equal(whole, class_counts(leaf, u))


def test_class_counts_helper_matches_the_host_statistic():
    """The test's own numpy classifier against coding._genie_stats on edge leaves."""
    from polarcub_amd import coding
    v = np.array([0.0, -0.0, 1.0, -1.0, np.nan, 0.25, -0.25, 1.0 - 2.0 ** -53, -(1.0 - 2.0 ** -53)])
    for ub in (0, 1):
        u = np.full(v.size, ub, np.int64)
        pe, _ = coding._genie_stats(marginals(v), u, False)
        c = class_counts(v[:, None], np.full((1, v.size), ub, np.uint8))  # one trial, a position a leaf
        got = [1.0 if w else (0.5 if t else 0.0) for w, t in zip(c[1:1 + v.size], c[1 + v.size:])]
        assert list(pe) == got, ub


# -- ABI -------------------------------------------------------------------------------------------

NAMES = ("pcub_sc_genie_bin_supported", "pcub_sc_genie_bin", "pcub_sc_genie_bin_geom", "pcub_mc_genie_bin_workspace",
         "pcub_mc_genie_bin")


def test_symbols_are_exported_declared_and_bound():
    from polarcub_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "polarcub_sc.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert re.search(r"\b(int|size_t) %s\(" % name, header)
        assert getattr(L, name).argtypes
    assert L.pcub_abi_version() == _lib.ABI_VERSION == 4


def test_kernel_entry_refuses_invalid_arguments_before_any_hip_call():
    from polarcub_amd import _lib
    L = _lib.lib()
    fake = P(1 << 20)

    def call(**kw):
        a = dict(rows=fake, compact=0, u=fake, B=4, n=6, counters=fake, leaf=None)
        a.update(kw)
        return L.pcub_sc_genie_bin(a["rows"], a["compact"], a["u"], a["B"], a["n"], a["counters"], a["leaf"], None)

    for kw in [dict(rows=None), dict(u=None), dict(counters=None), dict(B=-1), dict(n=0), dict(n=14), dict(n=-2),
               dict(B=(1 << 30) + 1), dict(rows=None, compact=1)]:
        assert call(**kw) == _lib.EINVAL, kw
    assert call(B=0) == 0 and call(B=0, compact=1, leaf=fake) == 0  # an empty batch: nothing to launch
    assert L.pcub_sc_genie_bin_geom(fake, 0, fake, 4, 6, 128, fake, None, None) == _lib.EINVAL  # no such workgroup
    assert L.pcub_sc_genie_bin_geom(fake, 0, fake, 0, 6, 256, fake, None, None) == 0
    assert [L.pcub_sc_genie_bin_supported(n) for n in (-1, 0, 1, 2, 13, 14, 20)] == [0, 0, 1, 1, 1, 0, 0]


def test_pipeline_entry_refuses_invalid_arguments_before_any_launch():
    from polarcub_amd import _lib
    L = _lib.lib()
    fake = P(1 << 20)
    need = L.pcub_mc_genie_bin_workspace(10, 8)
    ok = dict(seed=1, offset=0, count=10, n=8, channel=0, param=0.5, chunk=10, counters=fake, workspace=fake,
              workspace_bytes=need)

    def call(**kw):
        a = dict(ok, **kw)
        return L.pcub_mc_genie_bin(a["seed"], a["offset"], a["count"], a["n"], a["channel"], a["param"], a["chunk"],
                                   a["counters"], a["workspace"], a["workspace_bytes"], None)

    wrong = [dict(counters=None), dict(workspace=None), dict(count=-1), dict(offset=-1), dict(chunk=0), dict(chunk=-3),
             dict(channel=2), dict(channel=-1), dict(param=float("nan")), dict(param=float("inf")), dict(param=0.0),
             dict(param=-1.0), dict(channel=1, param=1.5), dict(channel=1, param=-0.1),
             dict(channel=1, param=float("nan")), dict(n=0), dict(n=21), dict(workspace_bytes=need - 1),
             dict(workspace_bytes=0)]
    for kw in wrong:
        assert call(**kw) == _lib.EINVAL, kw
    assert call(count=0) == 0                        # nothing to do: no launch either
    assert call(count=0, channel=1, param=0.0) == 0  # BSC(0) and BSC(1) are in the domain
    assert call(count=0, channel=1, param=1.0) == 0


def test_workspace_sizes():
    from polarcub_amd import _lib
    L = _lib.lib()
    ws = L.pcub_mc_genie_bin_workspace
    # u, x and the chunk's compact rows at the least
    assert ws(10, 8) >= 10 * (8 * 256 + 2 * 4 * 8)
    for n in range(1, 14):
        sizes = [ws(c, n) for c in (1, 2, 7, 64, 1000, 1 << 18)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0], n
    for c in (1, 64, 1 << 12):
        sizes = [ws(c, n) for n in range(1, 14)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], c
    # no leaf buffer on the fused route: far less than the composed route's 8 N more bytes a trial
    assert ws(1 << 12, 12) < (1 << 12) * (8 * 4096 + 4096)
    for bad in [(0, 8), (-1, 8), (10, 0), (10, -1), (10, 21), (1 << 62, 8)]:
        assert ws(*bad) == 0, bad


# -- Python and CLI ----------------------------------------------------------------------------------

def test_cli_parser_and_channel():
    from polarcub_amd import construction, mc
    from polarcub_amd.cli import genie_bin
    ap = genie_bin.parser()
    a = vars(ap.parse_args(["--channel", "awgn", "--ebn0", "2", "--rate", "0.5", "-n", "10", "-g", "1000000", "-e",
                            "0.1", "-gs", "7", "-f", "F"]))
    assert (a["n"], a["genie_simulations"], a["error_probability"], a["genie_seed"], a["frozen_bits_file"]) == \
        (10, 1000000, 0.1, 7, "F")
    assert genie_bin.channel_of(a) == (mc.CHANNEL_AWGN, construction.awgn_sigma2(2.0, 0.5))
    a = vars(ap.parse_args(["--sigma2", "0.7", "-n", "4"]))
    assert genie_bin.channel_of(a) == (mc.CHANNEL_AWGN, 0.7) and a["genie_seed"] == 300
    a = vars(ap.parse_args(["--channel", "bsc", "-p", "0.2", "-n", "4"]))
    assert genie_bin.channel_of(a) == (mc.CHANNEL_BSC, 0.2)
    for bad in (["-n", "4"], ["--sigma2", "0.5", "--ebn0", "1", "-n", "4"], ["--sigma2", "-1", "-n", "4"],
                ["--channel", "bsc", "-p", "1.5", "-n", "4"], ["--ebn0", "1", "--rate", "0", "-n", "4"]):
        with pytest.raises(ValueError):
            genie_bin.channel_of(vars(ap.parse_args(bad)))
    with pytest.raises(SystemExit):
        ap.parse_args(["--channel", "bec", "-n", "4"])


def test_counts_to_file_round_trip(tmp_path, capsys):
    """Counts -> Pe -> frozen set -> the reference's file format -> the reader of main_deletion."""
    from polarcub_amd import coding
    trials = 10
    wrong = np.array([0, 5, 0, 1, 0, 0, 10, 0], np.int64)
    tie = np.array([0, 0, 2, 0, 0, 1, 0, 0], np.int64)
    f = str(tmp_path / "frozen.txt")
    frozen = coding._genie_bin_finish(8, trials, wrong, tie, trials, 0.2, f)
    out = capsys.readouterr().out
    assert frozen == {1, 3, 6} and coding.read_frozen_file(f) == frozen
    assert "pevec =  [0.0, 0.5, 0.1, 0.1, 0.0, 0.05, 1.0, 0.0]" in out
    assert "code rate =  0.625" in out and "codeword length =  8" in out
    text = open(f).read()
    assert "** number of trials = 10" in text and "*** 6 10.0" in text
