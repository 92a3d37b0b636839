#!/usr/bin/env python3
"""tests/golden/genie_prior.npz: the reference's genie under a non-uniform a-priori distribution.

    python scripts/make_golden_genie_prior.py

Runs genieSingleEncodeSimulatioan / genieSingleDecodeSimulatioan (BinaryPolarEncoderDecoder.py:114-221)
trial by trial, and for cases a and b the whole genieEncodeDecodeSimulation (:390-491), on the
reference loaded by oracle.make_golden.load_reference (so only where the reference is present):

  a  N = 64    prior (0.7, 0.3)                     BSC(0.1) joint rows        24 trials  trust True, False
  b  N = 32    positional prior a_i in [0.05, 0.95]  Z channel, P(y=1|x=0) = 0  16 trials  trust True
  c  N = 1024  prior (0.89, 0.11)                   BSC(0.1) joint rows         3 trials  trust True

The joint row of position i for received symbol y is table[i][y] = (prior[i][0] W(y|0),
prior[i][1] W(y|1)).  Per trial the file holds the genie seed, the common randomness r, the encoder's
x_hat, TV and H, the received word, and the decoder's x_hat, Pe and H (case a: Pe of both statistics).
The per-trial seeds are those genieEncodeDecodeSimulation draws from genieSeed, and the channel
closure draws from its own random.Random(channel_seed), so the whole runs see the same trials; their
stdout and frozen sets are in `meta`.  Tests replay the stored received words.
"""
import contextlib
import io
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as mg  # noqa: E402


def bsc_table(prior, p):
    """table[i][y][x] = prior[i][x] * W(y|x) for the BSC(p)."""
    W = np.array([[1.0 - p, p], [p, 1.0 - p]])  # W[x][y]
    return np.stack([np.stack([prior[:, 0] * W[0][y], prior[:, 1] * W[1][y]], axis=-1) for y in range(2)], axis=1)


def z_table(prior, q):
    """Z channel: x = 0 is received as 0 always (exact zeros at y = 1), x = 1 as 0 with probability q."""
    W = np.array([[1.0, 0.0], [q, 1.0 - q]])
    return np.stack([np.stack([prior[:, 0] * W[0][y], prior[:, 1] * W[1][y]], axis=-1) for y in range(2)], axis=1)


def closures(R, N, prior, table, W, channel_seed, seen):
    BMVD = R["BMVD"]
    crng = random.Random(channel_seed)

    def make_x():
        xvd = BMVD.BinaryMemorylessVectorDistribution(N)
        xvd.probs[:] = prior
        return xvd

    def channel(codeword):
        out = []
        for x in codeword:
            out.append(0 if crng.random() < W[int(x)][0] else 1)
        seen.append(out)
        return out

    def make_xy(received):
        xyvd = BMVD.BinaryMemorylessVectorDistribution(N)
        xyvd.probs[:] = table[np.arange(N), np.asarray(received, np.int64)]
        return xyvd

    return make_x, channel, make_xy


def run_case(R, name, N, prior, table, W, T, genie_seed, channel_seed, bound, trusts, whole):
    BPED = R["BPED"]
    seen = []
    make_x, channel, make_xy = closures(R, N, prior, table, W, channel_seed, seen)
    xvd = make_x()
    encDec = BPED.BinaryPolarEncoderDecoder(N, set(), 0)
    srng = random.Random()
    srng.seed(genie_seed)
    out = dict(seeds=np.zeros(T, np.int64), r=np.zeros((T, N)), enc_x=np.zeros((T, N), np.uint8), TV=np.zeros((T, N)),
               HEnc=np.zeros((T, N)), rx=np.zeros((T, N), np.uint8), dec_x=np.zeros((T, N), np.uint8),
               Pe=np.zeros((T, N)), HDec=np.zeros((T, N)))
    if False in trusts:
        out["Pe_untrusted"] = np.zeros((T, N))
    for t in range(T):
        seed = srng.randint(1, 1000000)
        out["seeds"][t] = seed
        rr = random.Random()
        rr.seed(seed)
        out["r"][t] = [rr.random() for _ in range(N)]
        x, tv, henc = encDec.genieSingleEncodeSimulatioan(xvd, seed)
        out["enc_x"][t], out["TV"][t], out["HEnc"][t] = x, tv, henc
        received = channel(x)
        out["rx"][t] = received
        xd, pe, hdec = encDec.genieSingleDecodeSimulatioan(xvd, make_xy(received), seed, True)
        out["dec_x"][t], out["Pe"][t], out["HDec"][t] = xd, pe, hdec
        if False in trusts:
            xd2, pe2, h2 = encDec.genieSingleDecodeSimulatioan(xvd, make_xy(received), seed, False)
            assert list(xd2) == list(xd) and h2 == []
            out["Pe_untrusted"][t] = pe2
    meta = dict(N=N, trials=T, genie_seed=genie_seed, channel_seed=channel_seed, bound=bound, runs=[])
    if whole:
        for trust in trusts:
            again = []
            make_x, channel, make_xy = closures(R, N, prior, table, W, channel_seed, again)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                frozen = BPED.genieEncodeDecodeSimulation(N, make_x, lambda e: e, channel, make_xy, T, bound,
                                                          genieSeed=genie_seed, trustXYProbs=trust)
            assert again == seen[:T], "the whole run saw other received words"
            meta["runs"].append(dict(trust=trust, stdout=buf.getvalue(), frozen=sorted(int(i) for i in frozen)))
            print("  case %s trust=%s: %d frozen of %d" % (name, trust, len(frozen), N))
    out["prior"] = prior
    out["table"] = table
    return meta, {"%s_%s" % (name, k): v for k, v in out.items()}


def main():
    R = mg.load_reference()
    arrays, meta = {}, {}
    p64 = np.tile(np.array([0.7, 0.3]), (64, 1))
    W_bsc = [[0.9, 0.1], [0.1, 0.9]]
    meta["a"], arr = run_case(R, "a", 64, p64, bsc_table(p64, 0.1), W_bsc, 24, 11, 21, 0.1, (True, False), True)
    arrays.update(arr)
    a = 0.05 + 0.9 * np.random.default_rng(32).random(32)
    p32 = np.stack([a, 1.0 - a], axis=-1)
    meta["b"], arr = run_case(R, "b", 32, p32, z_table(p32, 0.3), [[1.0, 0.0], [0.3, 0.7]], 16, 12, 22, 0.2, (True,),
                              True)
    arrays.update(arr)
    p1024 = np.tile(np.array([0.89, 0.11]), (1024, 1))
    meta["c"], arr = run_case(R, "c", 1024, p1024, bsc_table(p1024, 0.1), W_bsc, 3, 13, 23, 0.1, (True,), False)
    arrays.update(arr)
    mg.save("genie_prior", dict(cases=meta, note="per case: seeds, r, enc_x, TV, HEnc, rx, dec_x, Pe, HDec "
                                                 "(a: Pe_untrusted), prior [N][2], table [N][y][x]"), **arrays)


if __name__ == "__main__":
    main()
