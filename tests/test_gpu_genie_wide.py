"""Genie construction at 512 trellises a codeword (main_deletion's n = 13, n0 = n // 3 = 4): the
facade sends every trial's leaves through the GPU export kernel and gets the frozen set of the
generic host recursion; sub-batched device calls return what one call returns."""
import contextlib
import io
import random

import numpy as np
import pytest

from oracle import orc
from oracle import trellis_oracle as tro

pytestmark = pytest.mark.gpu

N, N0, PD, XI = 13, 4, 0.1, 0.1


def _score_lines(path):
    with open(path) as f:
        return [l for l in f if l.startswith("***")]


def test_genie_facade_on_device(tmp_path, monkeypatch):
    """genieEncodeDecodeSimulation with main_deletion's closures, 2 trials: first with the host
    genie decode forbidden (the leaves must come from the device), then with the leaf kernel
    reported missing (the generic per-trial recursion).  Same frozen set, same scores."""
    from polarcub_amd import coding, sc
    from polarcub_amd.cli import main_deletion as md
    length = 1 << N

    def run(name):
        path = str(tmp_path / name)
        with contextlib.redirect_stdout(io.StringIO()):
            frozen = coding.genieEncodeDecodeSimulation(
                length, md.make_xVectorDistribuiton_deletion_uniform(length),
                md.make_codeword_addDeletionGuardBands(XI, N, N0, 0), md.make_simulateChannel_deletion(PD, seed=100),
                md.make_xyVectorDistribution_deletion(PD, XI, N, N0, 0), 2, 0.1, genieSeed=300, trustXYProbs=False,
                filename=path)
        return frozen, _score_lines(path)

    def forbidden(*a, **k):
        raise AssertionError("host genie decode used")

    with monkeypatch.context() as mp:
        mp.setattr(coding.BinaryPolarEncoderDecoder, "genieSingleDecodeSimulatioan", forbidden)
        dev_frozen, dev_lines = run("device.txt")
    with monkeypatch.context() as mp:
        mp.setattr(sc, "leaf_deletion_supported", lambda n, n0, ones=0: False)
        host_frozen, host_lines = run("host.txt")
    assert len(dev_lines) == length
    assert dev_frozen == host_frozen
    assert dev_lines == host_lines


def test_genie_sub_batches(monkeypatch):
    """_device_genie_deletion with the device bound so low that every trial is a call of its own
    returns the marginals of one call, in trial order."""
    from polarcub_amd import coding
    length = 1 << N
    zeros = np.zeros(length, np.uint8)
    U, words = [], []
    for seed in (11, 12, 13):
        u = np.random.default_rng(seed).integers(0, 2, length).astype(np.uint8)
        cw = tro.add_guard_bands([int(b) for b in orc.encode_bin(u, zeros, fval=zeros)], N, N0, XI)
        U.append(u)
        words.append(tro.deletion_channel(cw, PD, random.Random(seed)))
    U = np.stack(U)
    shape = (PD, N, N0, 0)
    assert len(words) < coding._GENIE_DEVICE_BYTES // (32 * length)
    whole = coding._device_genie_deletion(length, shape, words, U)
    monkeypatch.setattr(coding, "_GENIE_DEVICE_BYTES", 1)
    calls = []
    from polarcub_amd import sc
    orig = sc.DeletionDecoder.decode_leaves
    monkeypatch.setattr(sc.DeletionDecoder, "decode_leaves",
                        lambda self, rx, ln, fv=None: calls.append(rx.shape[0]) or orig(self, rx, ln, fv))
    split = coding._device_genie_deletion(length, shape, words, U)
    assert calls == [1, 1, 1]
    assert whole.shape == (3, length, 2) and len(np.unique(whole[:, :, 0])) > 1000
    assert np.array_equal(split, whole)
