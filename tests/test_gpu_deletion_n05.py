"""Deletion-channel SC decode of 32-input trellises (n0 = 5, main_deletion's n0 = n // 3 at n = 15) on
the GPU: the wave-per-task kernel of sc_del_w5.hip / trellis_wave5.h at 64 .. 1024 trellises a codeword
(n = 11 .. 15), bit-exact against the C oracle (oracle/trellis_oracle.c, pinned to the Python oracle at
n0 = 5 by tests/test_emulated_deletion_n05.py) and against the reference's own decodes
(tests/golden/deletion_wave.npz), through the decoder class, the persistent loop, the
facade, the launcher's length limit and the Monte-Carlo pipeline."""
import ctypes
import random

import numpy as np
import pytest
import torch

from oracle import orc
from oracle import trellis_oracle as tro

pytestmark = pytest.mark.gpu

N0 = 5


@pytest.fixture(scope="module")
def sc():
    from polarcub_amd import _lib, sc as m
    _lib.lib()
    return m


def _dec(sc, n, pd, frozen, fval, rx, rx_len):
    code = sc.CodeSpec(1 << n, frozen, fval, device="cuda")
    d = sc.DeletionDecoder(code, N0, pd, 0)
    assert d.table("cuda") is None
    info, xhat = d.decode(torch.from_numpy(np.ascontiguousarray(rx, np.uint8)).cuda(),
                          torch.from_numpy(np.asarray(rx_len, np.int32)).cuda())
    torch.cuda.synchronize()
    return info.cpu().numpy(), xhat.cpu().numpy()


def _padded(words):
    W = max([len(w) for w in words] + [1])
    rx = np.zeros((len(words), W), np.uint8)
    for i, w in enumerate(words):
        rx[i, :len(w)] = w
    return rx, np.array([len(w) for w in words], np.int32)


def _frozen(rng, n, rate0):
    """rate0: the first quarter frozen (the first four depth-4 nodes are rate-0: their tasks are
    skipped); else every one of the 32 collapse points keeps an information position."""
    N = 1 << n
    if rate0:
        frozen = (rng.random(N) < 0.5).astype(np.uint8)
        frozen[: N // 4] = 1
    else:
        frozen = (rng.random(N) < 0.3).astype(np.uint8)
        frozen[:: N // 32] = 0
    return frozen, (rng.random(N) < 0.5).astype(np.uint8)


def _channel_words(rng, prng, n, pds):
    N = 1 << n
    return [tro.deletion_channel(tro.add_guard_bands([int(b) for b in rng.integers(0, 2, N)], n, N0, 0.1, 0), p, prng)
            for p in pds]


def test_supported_range(sc):
    for n in range(11, 16):
        assert sc.deletion_supported(n, 5, 0), n
    assert not sc.deletion_supported(10, 5, 0)
    assert not sc.deletion_supported(16, 5, 0)
    assert not sc.deletion_supported(15, 5, 1)
    assert not sc.deletion_supported(15, 6, 0)
    for n in range(10, 17):
        assert not sc.leaf_deletion_supported(n, 5, 0), n
    code = sc.CodeSpec(1 << 11, np.zeros(1 << 11, np.uint8), np.zeros(1 << 11, np.uint8), device="cuda")
    with pytest.raises(ValueError):
        sc.DeletionDecoder(code, 5, 0.1, 0).decode_leaves(torch.zeros((1, 64), dtype=torch.uint8, device="cuda"),
                                                           torch.tensor([64], dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("n", [11, 12])
def test_small_shapes_vs_c_oracle(sc, n):
    """64 / 128 trellises: channel outputs at pd 0.05 .. 0.4 (segments from 0 to 32 symbols and overlong
    ones), an empty, a one-symbol, an all-zeros and an overlong random word; a frozen set with rate-0
    depth-4 nodes (their tasks skipped) and one with none.  Bit-exact."""
    N = 1 << n
    rng = np.random.default_rng(1500 + n)
    prng = random.Random(1900 + n)
    for fs in range(2):
        frozen, fval = _frozen(rng, n, fs == 0)
        pd = (0.05, 0.1, 0.25, 0.4)[(n + fs) % 4]
        words = _channel_words(rng, prng, n, (0.05, 0.1, 0.2, 0.3, 0.4, 0.1))
        words += [[], [1], [0] * 9, [int(b) for b in rng.integers(0, 2, N + N // 2)]]
        rx, ln = _padded(words)
        info, xhat = _dec(sc, n, pd, frozen, fval, rx, ln)
        i_ref, x_ref = orc.decode_deletion(rx, ln, n, N0, pd, frozen, fval)
        assert np.array_equal(info, i_ref), (n, fs)
        assert np.array_equal(xhat, x_ref), (n, fs)


@pytest.mark.parametrize("n,nch", [(13, 4), (14, 3), (15, 2)])
def test_wide_shapes_vs_c_oracle(sc, n, nch):
    """256 / 512 / 1024 trellises (n = 15: main_deletion's default shape): a few channel words, the empty
    word and an overlong random one, a frozen set without rate-0 nodes.  Bit-exact."""
    N = 1 << n
    rng = np.random.default_rng(2500 + n)
    prng = random.Random(2900 + n)
    frozen, fval = _frozen(rng, n, False)
    pd = 0.1
    words = _channel_words(rng, prng, n, (0.1, 0.3, 0.05, 0.2)[:nch])
    words += [[], [int(b) for b in rng.integers(0, 2, N + N // 2)]]
    rx, ln = _padded(words)
    info, xhat = _dec(sc, n, pd, frozen, fval, rx, ln)
    i_ref, x_ref = orc.decode_deletion(rx, ln, n, N0, pd, frozen, fval)
    assert np.array_equal(info, i_ref)
    assert np.array_equal(xhat, x_ref)


@pytest.mark.parametrize("n,pd", [(11, 0.1), (13, 0.2), (15, 0.1), (11, 0.05), (13, 0.1), (15, 0.05)])
def test_wave_fixture(sc, n, pd):
    """64, 256 and 1024 trellises of 32 inputs against the reference's own decodes
    (tests/golden/deletion_wave.npz: channel words, one at pd 0.4, the empty word and an overlong one;
    the first quarter frozen, so rate-0 depth-4 nodes; at rate 1/2, and at the rate 1/16 at which the
    reference decodes correctly and every leaf is live): info and x_hat bit-exact."""
    from tests.test_trellis_oracle import wave_case
    c = wave_case(n, N0, pd)
    info, xhat = _dec(sc, n, c["pd"], c["frozen"], c["fval"], c["rx"].copy(), c["rx_len"].copy())
    assert np.array_equal(info, c["info"])
    assert np.array_equal(xhat, c["xhat"])


def test_persistent_loop(sc):
    """n = 11, 1,280 codewords (several a resident workgroup): 40 distinct words of mixed lengths, each 32
    times in a shuffled order; every copy decodes as the oracle decodes its original, with the codewords
    taken from the per-launch counter and with the static stride."""
    n = 11
    N = 1 << n
    rng = np.random.default_rng(3511)
    prng = random.Random(3911)
    frozen, fval = _frozen(rng, n, True)
    pd = 0.1
    words = _channel_words(rng, prng, n, [(0.02, 0.1, 0.1, 0.2, 0.3, 0.45)[i % 6] for i in range(35)])
    words += [[], [1], [0] * 9, [int(b) for b in rng.integers(0, 2, N // 3)], [int(b) for b in rng.integers(0, 2, 2 * N)]]
    assert len(words) == 40
    rx, ln = _padded(words)
    i_ref, x_ref = orc.decode_deletion(rx, ln, n, N0, pd, frozen, fval)
    order = rng.permutation(np.repeat(np.arange(40), 32))
    old = sc.set_dynamic_tiles(1)
    try:
        for dyn in (1, 0):
            sc.set_dynamic_tiles(dyn)
            info, xhat = _dec(sc, n, pd, frozen, fval, rx[order], ln[order])
            assert np.array_equal(info, i_ref[order]), dyn
            assert np.array_equal(xhat, x_ref[order]), dyn
    finally:
        sc.set_dynamic_tiles(old)


def _facade(n, frozen):
    from polarcub_amd import coding, vectors
    N = 1 << n
    enc = coding.BinaryPolarEncoderDecoder(N, set(int(i) for i in np.nonzero(frozen)[0]), 77)
    xvd = vectors.BinaryMemorylessVectorDistribution(N)
    xvd.probs[:] = 0.5
    return enc, xvd


def test_facade_reaches_kernel(sc, monkeypatch):
    """BinaryPolarEncoderDecoder.decode over a received-word collection at n = 11, n0 = 5 runs the kernel
    (the host trellises are never built) and returns what the host recursion over the collection returns
    (the kernel reported missing)."""
    from polarcub_amd import deletion
    n, pd, xi = 11, 0.1, 0.1
    rng = np.random.default_rng(4511)
    prng = random.Random(4911)
    frozen, _ = _frozen(rng, n, True)
    enc, xvd = _facade(n, frozen)
    for w in _channel_words(rng, prng, n, (0.1, 0.25)):
        coll = deletion.buildCollectionOfBinaryTrellises_uniformInput_deletion(w, pd, xi, n, N0, 0)
        x, info = enc.decode(xvd, coll)
        assert coll._lazy is not None, "host trellises were built: the kernel path did not run"
        with monkeypatch.context() as mp:
            mp.setattr(sc, "deletion_supported", lambda n, n0, ones=0: False)
            coll2 = deletion.buildCollectionOfBinaryTrellises_uniformInput_deletion(w, pd, xi, n, N0, 0)
            x2, info2 = enc.decode(xvd, coll2)
        assert np.array_equal(np.asarray(x), np.asarray(x2)) and np.array_equal(np.asarray(info), np.asarray(info2))


def test_overlong_row_is_refused_and_facade_falls_back(sc):
    """A row stride past what the kernel's LDS takes returns PCUB_EINVAL from the C entry point (no launch,
    no fault); a word that long still decodes through the facade (the host recursion), as the oracle
    decodes it."""
    from polarcub_amd import _lib, deletion
    n, pd, xi = 11, 0.1, 0.1
    N = 1 << n
    rng = np.random.default_rng(5511)
    frozen, fval = _frozen(rng, n, True)
    code = sc.CodeSpec(N, frozen, fval, device="cuda")
    W = 1_300_000  # > 8 x 4 task waves x sizeof(W5Buf) = 1,243,648 symbols
    word = np.zeros(W, np.uint8)
    word[rng.integers(0, W, 4000)] = 1
    rx = torch.from_numpy(word[None, :]).cuda()
    ln = torch.tensor([W], dtype=torch.int32, device="cuda")
    info = torch.zeros((max(1, code.info_words), 1), dtype=torch.int32, device="cuda")
    xh = torch.zeros((code.n_words, 1), dtype=torch.int32, device="cuda")
    rc = _lib.lib().pcub_sc_decode_deletion(sc._p(rx), sc._p(ln), 1, W, n, N0, 0, ctypes.c_double(pd),
                                            sc._p(code.fmask_dev), sc._p(code.fval_dev), code.K, sc._p(info),
                                            sc._p(xh), sc._stream())
    torch.cuda.synchronize()
    assert rc == _lib.EINVAL
    # one symbol fewer than the limit is taken
    Wok = 1_243_648
    rc = _lib.lib().pcub_sc_decode_deletion(sc._p(rx), sc._p(ln), 1, Wok, n, N0, 0, ctypes.c_double(pd),
                                            sc._p(code.fmask_dev), sc._p(code.fval_dev), code.K, sc._p(info),
                                            sc._p(xh), sc._stream())
    torch.cuda.synchronize()
    assert rc == 0
    i_ok, x_ok = orc.decode_deletion(word[None, :Wok], np.array([Wok], np.int32), n, N0, pd, frozen, fval)
    assert np.array_equal(sc.unpack(info, code.K).cpu().numpy(), i_ok)
    assert np.array_equal(sc.unpack(xh, code.N).cpu().numpy(), x_ok)
    enc, xvd = _facade(n, frozen)
    # the facade's frozen values come from its common randomness: the oracle with the same
    fv = np.where(0.5 >= enc.randomlyGeneratedNumbers, 0, 1).astype(np.uint8)
    coll = deletion.buildCollectionOfBinaryTrellises_uniformInput_deletion([int(b) for b in word], pd, xi, n, N0, 0)
    x, inf = enc.decode(xvd, coll)
    i_ref, x_ref = orc.decode_deletion(word[None, :], np.array([W], np.int32), n, N0, pd, frozen, fv)
    assert np.array_equal(np.asarray(inf), i_ref[0]) and np.array_equal(np.asarray(x), x_ref[0])


def test_mc_run_shards_add_up(sc):
    """pcub_mc_run_deletion at (11, 5): one 256-codeword run counts what two 128-codeword shards count."""
    from polarcub_amd import construction, mc
    n = 11
    N = 1 << n
    fr = construction.bhattacharyya_frozen(n, N // 4, 0.5)
    code = sc.CodeSpec.from_frozen_set(N, set(np.nonzero(fr)[0].tolist()), 200, device="cuda")
    whole = mc.run_deletion(code, 31, 50, 256, N0, 0.1, 0.1)
    a = mc.run_deletion(code, 31, 50, 128, N0, 0.1, 0.1)
    b = mc.run_deletion(code, 31, 178, 128, N0, 0.1, 0.1)
    assert whole[0] == 256
    assert [p + q for p, q in zip(a, b)] == whole
