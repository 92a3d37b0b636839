"""Leaf export of the deletion channel at 512 and 1024 trellises a codeword (n0 = 4, n = 13, 14:
main_deletion's default n0 = n // 3; k_sc_del<4, 9|10, true, 0>, one codeword a workgroup of T
threads): the supported range, every leaf's marginal bit-exact against the Python oracle on
genie-mode inputs, decisions identical to the decode kernels, and leaves independent of the
batch a word is decoded in; and the export at 64, 256 and 512 trellises against the reference's own
decodes (tests/golden/deletion_wave.npz)."""
import random

import numpy as np
import pytest
import torch

from oracle import orc
from oracle import trellis_oracle as tro

pytestmark = pytest.mark.gpu

N0 = 4
PD = 0.1
XI = 0.1
SEEDS = {13: (1, 2), 14: (1,)}
TAIL = 64


@pytest.fixture(scope="module")
def sc():
    from polarcub_amd import _lib, sc as m
    _lib.lib()
    return m


def _channel_word(n, seed):
    """One genie trial's input: u drawn from the seed, its codeword with guard bands through the
    deletion channel.  Returns (u, received word)."""
    N = 1 << n
    u = np.random.default_rng(seed).integers(0, 2, N).astype(np.uint8)
    zeros = np.zeros(N, np.uint8)
    x = orc.encode_bin(u, zeros, fval=zeros)
    cw = tro.add_guard_bands([int(b) for b in x], n, N0, XI)
    return u, tro.deletion_channel(cw, PD, random.Random(seed))


def _pad(words, extra=0):
    W = max([len(w) for w in words] + [1]) + extra
    rx = np.zeros((len(words), W), np.uint8)
    for i, w in enumerate(words):
        rx[i, :len(w)] = w
    return torch.from_numpy(rx).cuda(), torch.tensor([len(w) for w in words], dtype=torch.int32).cuda()


_GENIE = {}


def _genie_case(n):
    """Genie-mode words of shape n (all positions frozen to the word's u) with the oracle's leaf
    marginals and x_hat, computed once a session: the channel words of SEEDS, then the empty word and
    a word whose every segment has 17 symbols (more than a 16-input trellis takes)."""
    if n not in _GENIE:
        N = 1 << n
        us, words = [], []
        for seed in SEEDS[n]:
            u, w = _channel_word(n, seed)
            us.append(u)
            words.append(w)
        rng = np.random.default_rng(1000 + n)
        overlong = [1] * (17 << (n - N0))
        assert len(tro.remove_guard_bands(overlong, n, N0)[0]) > 16
        for w in ([], overlong):
            us.append(rng.integers(0, 2, N).astype(np.uint8))
            words.append(w)
        ones = np.ones(N, np.uint8)
        ref_m, ref_x = [], []
        for u, w in zip(us, words):
            lm = []
            x, info = tro.decode_deletion(w, n, N0, PD, ones, u, leaf_m=lm)
            assert info == []
            ref_m.append(np.array(lm, np.float64))
            ref_x.append(np.array(x, np.uint8))
        for a in ref_m + ref_x:
            a.setflags(write=False)
        _GENIE[n] = dict(U=np.stack(us), words=words, m=ref_m, x=ref_x, nchan=len(SEEDS[n]))
    return _GENIE[n]


def _leaves(sc, n, words, U, extra=0):
    N = 1 << n
    code = sc.CodeSpec(N, np.ones(N, np.uint8), np.zeros(N, np.uint8), device="cuda")
    rx, ln = _pad(words, extra)
    info, xhat, m = sc.DeletionDecoder(code, N0, PD).decode_leaves(rx, ln, torch.from_numpy(U).cuda())
    torch.cuda.synchronize()
    assert info.shape == (len(words), 0)
    return xhat.cpu().numpy(), m.cpu().numpy()


def test_supported_range(sc):
    assert sc.leaf_deletion_supported(13, 4, 0)
    assert sc.leaf_deletion_supported(14, 4, 0)
    assert not sc.leaf_deletion_supported(13, 4, 1)
    assert not sc.leaf_deletion_supported(15, 4, 0)
    assert not sc.leaf_deletion_supported(15, 5, 0)
    for n0 in range(1, 5):
        for tb in range(1, 11):
            for ones in range(4):
                if sc.deletion_supported(n0 + tb, n0, ones):
                    assert sc.leaf_deletion_supported(n0 + tb, n0, ones), (n0, tb, ones)


@pytest.mark.parametrize("n", [13, 14])
def test_leaves_match_oracle(sc, n):
    """One batch a shape: marginals and x_hat of every word equal the oracle's, bit for bit.  Only
    the two added words may end in a run of (0.5, 0.5) leaves, so the channel words do compare
    live marginals down to the last leaf."""
    g = _genie_case(n)
    half = np.full((TAIL, 2), 0.5)
    collapsed = [np.array_equal(m[-TAIL:], half) for m in g["m"]]
    assert not any(collapsed[:g["nchan"]]) and sum(collapsed) <= 2
    for m, u, x in zip(g["m"][:g["nchan"]], g["U"], g["x"]):
        assert len(np.unique(m[:, 0])) > 1000  # a live decode: thousands of distinct leaf values
        assert np.array_equal(x, orc.encode_bin(u, np.zeros(1 << n, np.uint8), fval=np.zeros(1 << n, np.uint8)))
    xhat, m = _leaves(sc, n, g["words"], g["U"])
    for i in range(len(g["words"])):
        assert np.array_equal(m[i], g["m"][i]), i
        assert np.array_equal(xhat[i], g["x"][i]), i


@pytest.mark.parametrize("n,nwords", [(13, 6), (14, 3)])
def test_decisions_match_decode_kernels(sc, n, nwords):
    """A shared frozen set (about half the positions, whole frozen blocks of 512 and 1024 positions
    so that rate-0 nodes occur, random frozen values): the export kernel's info and x_hat equal the
    decode kernels', the wave-per-task one (default dispatch) and the lane-per-trellis one, and
    each information leaf's marginal decides its info bit."""
    N = 1 << n
    rng = np.random.default_rng(40 + n)
    frozen = (rng.random(N) < 0.5).astype(np.uint8)
    frozen[:1024] = 1
    frozen[2048:2560] = 1
    frozen[N - 3072:N - 2048] = 1
    frozen[N - 512:] = 1
    fval = (rng.random(N) < 0.5).astype(np.uint8)
    prng = random.Random(n)
    words = []
    for t in range(nwords):
        x = [int(b) for b in rng.integers(0, 2, N)]
        words.append(tro.deletion_channel(tro.add_guard_bands(x, n, N0, XI), PD, prng))
    rx, ln = _pad(words)
    code = sc.CodeSpec(N, frozen, fval, device="cuda")
    d = sc.DeletionDecoder(code, N0, PD)
    info_l, xhat_l, m = d.decode_leaves(rx, ln)
    torch.cuda.synchronize()
    info_l, xhat_l, m = info_l.cpu().numpy(), xhat_l.cpu().numpy(), m.cpu().numpy()
    old = sc.set_deletion_wave(1)
    try:
        for wave in (old, 0):
            sc.set_deletion_wave(wave)
            info, xhat = d.decode(rx, ln)
            torch.cuda.synchronize()
            assert np.array_equal(info_l, info.cpu().numpy()), wave
            assert np.array_equal(xhat_l, xhat.cpu().numpy()), wave
    finally:
        sc.set_deletion_wave(old)
    mi = m[:, frozen == 0]
    assert np.array_equal((mi[..., 0] < mi[..., 1]).astype(np.uint8), info_l)


@pytest.mark.parametrize("n,pd", [(10, 0.1), (12, 0.25), (13, 0.1), (10, 0.05), (12, 0.1), (13, 0.05)])
def test_leaves_match_reference_fixture(sc, n, pd):
    """Leaf export at 64, 256 and 512 trellises of 16 inputs against the reference's own decodes
    (tests/golden/deletion_wave.npz, both frozen sets of each shape): info and x_hat of every word
    bit-exact, and the marginals at the information leaves bit-exact for the words whose marginals the
    fixture stores (all eight at n = 10, the first two or the first at n = 12, 13)."""
    from tests.test_trellis_oracle import wave_case
    c = wave_case(n, N0, pd)
    assert c["nleaf"] >= 1
    code = sc.CodeSpec(1 << n, c["frozen"], c["fval"], device="cuda")
    info, xhat, m = sc.DeletionDecoder(code, N0, c["pd"]).decode_leaves(torch.from_numpy(c["rx"].copy()).cuda(),
                                                                         torch.from_numpy(c["rx_len"].copy()).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(info.cpu().numpy(), c["info"])
    assert np.array_equal(xhat.cpu().numpy(), c["xhat"])
    infopos = c["frozen"] == 0
    assert np.array_equal(m[:c["nleaf"]].cpu().numpy()[:, infopos], c["leaf_m"][:, infopos])


def test_ragged_batch(sc):
    """The n = 13 words as one batch and one by one, each in a row padded to another width: a
    word's leaves depend on neither its neighbours nor the row stride."""
    g = _genie_case(13)
    xhat, m = _leaves(sc, 13, g["words"], g["U"])
    for i, w in enumerate(g["words"]):
        x1, m1 = _leaves(sc, 13, [w], g["U"][i:i + 1], extra=(0, 1, 31, 1000)[i % 4])
        assert np.array_equal(m1[0], m[i]), i
        assert np.array_equal(x1[0], xhat[i]), i
