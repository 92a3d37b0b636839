"""The deletion channel's genie pipeline on the GPU (sc_genie.hip): pcub_genie_count against
sc.leaf_marginals + coding._genie_stats on the crafted leaves of tests/test_genie_pipeline.py, and
pcub_mc_genie_deletion against the composed path (mc.philox_deletion_batch of the rate-1 code ->
DeletionDecoder.decode_leaves with every position frozen to the trial's u -> _genie_stats on the
host), against the CPU trellis oracle, over shards and chunks, and through the facade and the CLI.
Counts are integers: every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from tests.test_genie_pipeline import crafted_batch

pytestmark = pytest.mark.gpu

XI = 0.1


def stats_counts(m, U):
    """(wrong int64[N], tie int64[N]) of marginals m [T, N, 2] and true bits U [T, N] through
    coding._genie_stats(..., trustXYProbs=False), trial by trial."""
    from polarcub_amd import coding
    T, N = U.shape
    wrong, tie = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for t in range(T):
        pe, _ = coding._genie_stats(m[t], U[t].astype(np.int64), False)
        pe = np.array(pe)
        assert np.isin(pe, (0.0, 0.5, 1.0)).all()
        wrong += pe == 1.0
        tie += pe == 0.5
    return wrong, tie


# -- pcub_genie_count alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_genie_count_on_crafted_leaves(B):
    """N = 64: two u words a codeword; B around one wave and past two."""
    from polarcub_amd import mc, sc
    N = 64
    leaf, u, words = crafted_batch(N, B, 100 + B)
    dl = torch.from_numpy(leaf).cuda()
    dw = torch.from_numpy(words.view(np.int32)).cuda()
    m = sc.leaf_marginals(dl).cpu().numpy()  # [B, N, 2]
    wrong, tie = stats_counts(m, u)
    # all three classes at both values of u
    mu = np.take_along_axis(m, u[:, :, None].astype(np.int64), 2)[:, :, 0]
    mo = np.take_along_axis(m, 1 - u[:, :, None].astype(np.int64), 2)[:, :, 0]
    cls = np.where(mu > mo, 0, np.where(mu == mo, 1, 2))
    for bit in (0, 1):
        assert set(cls[u == bit].tolist()) == {0, 1, 2}
    trials, gw, gt = mc.genie_count(dl, dw, N)
    assert trials == B and np.array_equal(gw, wrong) and np.array_equal(gt, tie)
    assert wrong.sum() > 0 and tie.sum() > 0


def test_genie_count_accumulates():
    from polarcub_amd import _lib, sc
    N, B = 64, 130
    leaf, u, words = crafted_batch(N, B, 5)
    dl, dw = torch.from_numpy(leaf).cuda(), torch.from_numpy(words.view(np.int32)).cuda()
    wrong, tie = stats_counts(sc.leaf_marginals(dl).cpu().numpy(), u)
    counters = torch.zeros(1 + 2 * N, dtype=torch.int64, device="cuda")
    for k in (1, 2):
        _lib.check(_lib.lib().pcub_genie_count(sc._p(dl), sc._p(dw), B, 6, sc._p(counters), sc._stream()),
                   "pcub_genie_count")
        c = counters.cpu().numpy()
        assert c[0] == k * B and np.array_equal(c[1:1 + N], k * wrong) and np.array_equal(c[1 + N:], k * tie)


# -- pcub_mc_genie_deletion against the composed path ----------------------------------------------------
SHAPES = {  # n, n0, ones, pd, trials, seed, offset
    "n5": (5, 2, 0, 0.1, 200, 20251101, 0),       # N = 32: one mask word
    "n7ones": (7, 1, 2, 0.1, 96, 20251102, 1000),  # guard-band ones
    "n10": (10, 3, 0, 0.1, 64, 20251103, 0),      # 128 trellises: the LDS export subtree across two waves
    "n13": (13, 4, 0, 0.1, 48, 20251104, 7),      # 512 trellises: a workgroup a codeword
    "n5noisy": (5, 2, 0, 0.4, 200, 20251105, 0),  # wrong and tied positions present
    "n8": (8, 2, 0, 0.1, 200, 20251106, 0),       # the shards / chunks / facade shape
    "n6": (6, 2, 0, 0.1, 8, 20251107, 3),         # the oracle's shape
}
_composed = {}


def composed(name):
    """(U [T, N] u8, rx, rx_len (numpy), wrong, tie): the rate-1 code's Philox batch, the export decode
    with every position frozen to the trial's u, _genie_stats on the host; computed once a shape."""
    if name not in _composed:
        from polarcub_amd import mc, sc
        n, n0, ones, pd, T, seed, offset = SHAPES[name]
        N = 1 << n
        rate1 = sc.CodeSpec(N, np.zeros(N, np.uint8), np.zeros(N, np.uint8), device="cuda")
        info, rx, ln = mc.philox_deletion_batch(rate1, seed, offset, T, n0, XI, pd, ones)
        U = sc.unpack(info, N)
        frozen = sc.CodeSpec(N, np.ones(N, np.uint8), np.zeros(N, np.uint8), device="cuda")
        m = sc.DeletionDecoder(frozen, n0, pd, ones).decode_leaves(rx, ln, U)[2].cpu().numpy()
        U = U.cpu().numpy()
        wrong, tie = stats_counts(m, U)
        _composed[name] = (U, rx.cpu().numpy(), ln.cpu().numpy(), wrong, tie)
    return _composed[name]


def run(name, lo=None, hi=None, chunk=None):
    from polarcub_amd import mc
    n, n0, ones, pd, T, seed, offset = SHAPES[name]
    lo, hi = 0 if lo is None else lo, T if hi is None else hi
    return mc.run_genie_deletion(n, n0, XI, pd, seed, offset + lo, hi - lo, ones=ones, chunk=chunk)


@pytest.mark.parametrize("name", ["n5", "n7ones", "n10", "n13", "n5noisy"])
def test_pipeline_equals_the_composed_path(name):
    T = SHAPES[name][4]
    _, _, _, wrong, tie = composed(name)
    print(name, "composed wrong", int(wrong.sum()), "tie", int(tie.sum()))
    if name == "n5noisy":
        assert wrong.sum() > 0 and tie.sum() > 0  # the comparison below is not between zeros
    trials, gw, gt = run(name)
    assert trials == T
    assert gw.dtype == np.int64 and gt.dtype == np.int64
    assert np.array_equal(gw, wrong) and np.array_equal(gt, tie)


def test_pipeline_equals_the_cpu_oracle():
    """Independent of the project's kernels: the leaves of oracle.trellis_oracle.decode_deletion on
    the downloaded received words, every position frozen to the trial's u."""
    from oracle import trellis_oracle as tro
    n, n0, ones, pd, T, seed, offset = SHAPES["n6"]
    N = 1 << n
    U, rx, ln, _, _ = composed("n6")
    m = np.empty((T, N, 2))
    for t in range(T):
        lm = []
        tro.decode_deletion(list(map(int, rx[t, :ln[t]])), n, n0, pd, np.ones(N, np.uint8), U[t], ones, leaf_m=lm)
        m[t] = np.array(lm)
    wrong, tie = stats_counts(m, U)
    trials, gw, gt = run("n6")
    assert trials == T and np.array_equal(gw, wrong) and np.array_equal(gt, tie)


def test_shards_and_chunks_add_up():
    T = SHAPES["n8"][4]
    _, _, _, wrong, tie = composed("n8")
    whole = run("n8")
    assert whole[0] == T and np.array_equal(whole[1], wrong) and np.array_equal(whole[2], tie)
    a, b = run("n8", 0, 77), run("n8", 77, T)
    assert a[0] + b[0] == T and np.array_equal(a[1] + b[1], wrong) and np.array_equal(a[2] + b[2], tie)
    for chunk in (64, 1):  # 64 does not divide 200
        c = run("n8", chunk=chunk)
        assert c[0] == T and np.array_equal(c[1], wrong) and np.array_equal(c[2], tie)


def test_short_workspace_is_refused_on_the_device_too():
    from polarcub_amd import _lib, mc, sc
    n, n0, ones, pd, T, seed, offset = SHAPES["n8"]
    t = mc.guard_template(n, n0, XI, ones, torch.device("cuda"))
    W = int(t.numel())
    need = int(_lib.lib().pcub_mc_genie_deletion_workspace(T, n, W))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(1 + 2 * (1 << n), dtype=torch.int64, device="cuda")
    rc = _lib.lib().pcub_mc_genie_deletion(seed, offset, T, n, n0, sc._p(t), W, ones, pd, T, sc._p(counters), sc._p(ws),
                                           need - 1, sc._stream())
    assert rc == _lib.EINVAL and counters.sum().item() == 0


# -- the facade and the CLI ------------------------------------------------------------------------------
def test_facade_and_cli(tmp_path, capsys):
    from polarcub_amd import coding, mc
    from polarcub_amd.cli import main_deletion
    n, n0, pd, T, seed, bound = 8, 2, 0.1, 64, 300, 0.1
    N = 1 << n
    trials, wrong, tie = mc.run_genie_deletion(n, n0, XI, pd, seed, 0, T)
    assert trials == T
    Pe = coding.genie_pe_from_counts(trials, wrong, tie)
    want = coding.frozenSetFromTVAndPe([0.0] * N, Pe, bound)
    capsys.readouterr()
    fn = os.path.join(str(tmp_path), "frozen.txt")
    got = coding.genieEncodeDecodeSimulationDevice(n, n0, XI, pd, T, bound, seed, filename=fn)
    out = capsys.readouterr().out.splitlines()
    assert got == want and 0 < len(got) < N
    assert coding.read_frozen_file(fn) == want
    pevec = "pevec =  %s" % (Pe,)
    assert out[0] == pevec
    W = int(mc.guard_template(n, n0, XI, 0, torch.device("cuda")).numel())
    assert "code rate =  %s" % ((N - len(want)) / W,) in out and "codeword length =  %d" % W in out
    assert not [line for line in out if line.startswith("H")]
    cli = main_deletion.main(["-n", "8", "-n0", "2", "-g", "64", "--device-genie", "-gs", "300"])
    out = capsys.readouterr().out.splitlines()
    assert cli == want and pevec in out
