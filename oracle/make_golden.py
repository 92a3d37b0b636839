#!/usr/bin/env python3
"""Generate golden vectors by running the reference polarcub itself.

TEST INFRASTRUCTURE ONLY -- runs in the build container, never on the GPU box
(the reference tree does not exist there).  It imports /root/reference
in-process, with bytecode writing disabled, and applies two runtime shims
(no reference file is edited or copied):

  1. np.float / np.int / np.product aliases: the q-ary code still uses the
     NumPy < 1.24 names (VectorDistributions/QaryMemorylessVectorDistribution.py:16,72).
  2. normalizeDistList = normalize on the binary vector-distribution classes:
     BinaryPolarEncoderDecoder.py:279,285,299,305 call a method no class defines.

Outputs small .npz fixtures into tests/golden/ together with ref_timing.json.
Every fixture records its seeds and construction choices in a `meta` string.

Usage:  python oracle/make_golden.py [--only NAME ...]
"""
import argparse
import json
import math
import os
import random
import sys
import time

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")


def load_reference():
    if not os.path.isdir(REF):
        sys.exit("make_golden.py: /root/reference is not present (this script only runs in the build container)")
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    np.float = float  # noqa: shim 1
    np.int = int
    np.product = np.prod
    import BinaryPolarEncoderDecoder as BPED
    import QaryPolarEncoderDecoder as QPED
    from ScalarDistributions import BinaryMemorylessDistribution as BMD
    from ScalarDistributions import QaryMemorylessDistribution as QMD
    from VectorDistributions import BinaryMemorylessVectorDistribution as BMVD
    from VectorDistributions import BinaryTrellis as BT
    from VectorDistributions import CollectionOfBinaryTrellises as CBT
    from VectorDistributions import QaryMemorylessVectorDistribution as QMVD
    for cls in (BMVD.BinaryMemorylessVectorDistribution, BT.BinaryTrellis, CBT.CollectionOfBinaryTrellises):
        cls.normalizeDistList = cls.normalize  # shim 2
    return dict(BPED=BPED, QPED=QPED, BMD=BMD, QMD=QMD, BMVD=BMVD, BT=BT, CBT=CBT, QMVD=QMVD)


# ---------------------------------------------------------------------------
# helpers (build-side code, not reference code)
# ---------------------------------------------------------------------------

def bhattacharyya_frozen(n, K, sigma2):
    """Frozen set = the N-K least reliable indices by the Bhattacharyya recursion
    for BI-AWGN, in the adjacent-pair index convention (minus child = 2j, plus = 2j+1
    at each level, so u = path bits MSB first)."""
    z = np.array([math.exp(-1.0 / (2.0 * sigma2))])
    for _ in range(n):
        nz = np.empty(2 * len(z))
        nz[0::2] = 2 * z - z * z
        nz[1::2] = z * z
        z = nz
    order = sorted(range(len(z)), key=lambda i: (z[i], i))  # most reliable first
    info = set(order[:K])
    return set(i for i in range(len(z)) if i not in info), z


def awgn_pairs(x, sigma2, rng):
    """Joint P(x, y) for BPSK 0->+1, 1->-1 over AWGN with variance sigma2."""
    s = 1.0 - 2.0 * x.astype(np.float64)
    y = s + math.sqrt(sigma2) * rng.standard_normal(x.shape)
    c = 0.5 / math.sqrt(2.0 * math.pi * sigma2)
    p0 = c * np.exp(-((y - 1.0) ** 2) / (2.0 * sigma2))
    p1 = c * np.exp(-((y + 1.0) ** 2) / (2.0 * sigma2))
    return np.stack([p0, p1], axis=-1), y


class LeafRecorder:
    """Wraps BinaryMemorylessVectorDistribution.calcMarginalizedProbabilities to
    record the marginal the reference uses at each leaf (xy at information leaves,
    the a-priori tree at frozen leaves); one call per leaf during decode()."""

    def __init__(self, R):
        self.cls = R["BMVD"].BinaryMemorylessVectorDistribution
        self.orig = self.cls.calcMarginalizedProbabilities
        self.rec = []

    def __enter__(self):
        rec = self.rec
        orig = self.orig

        def wrapped(vd):
            m = orig(vd)
            rec.append((float(m[0]), float(m[1])))
            return m

        self.cls.calcMarginalizedProbabilities = wrapped
        return self

    def __exit__(self, *a):
        self.cls.calcMarginalizedProbabilities = self.orig


def ref_binary_decode_batch(R, N, frozen, crs, xy, prior=None, record_leaves=True):
    """Decode each codeword of xy [B][N][2] with the reference decoder."""
    BPED, BMVD = R["BPED"], R["BMVD"]
    enc = BPED.BinaryPolarEncoderDecoder(N, frozen, crs)
    xvd = BMVD.BinaryMemorylessVectorDistribution(N)
    xvd.probs[:] = np.array([0.5, 0.5]) if prior is None else prior
    B = xy.shape[0]
    info = np.zeros((B, enc.k), np.uint8)
    xhat = np.zeros((B, N), np.uint8)
    leaf = np.zeros((B, N, 2))
    t0 = time.perf_counter()
    for b in range(B):
        xyvd = BMVD.BinaryMemorylessVectorDistribution(N)
        xyvd.probs[:] = xy[b]
        with LeafRecorder(R) as lr:
            (xh, inf) = enc.decode(xvd, xyvd)
        assert len(lr.rec) == N
        leaf[b] = np.array(lr.rec)
        info[b] = inf
        xhat[b] = xh
    dt = (time.perf_counter() - t0) / max(B, 1)
    return enc, info, xhat, leaf, dt


def frozen_arrays(enc, N):
    mask = np.array([1 if i in enc.frozenSet else 0 for i in range(N)], np.uint8)
    r = np.array(enc.randomlyGeneratedNumbers, np.float64)
    fval = np.where(0.5 >= r, 0, 1).astype(np.uint8)
    return mask, r, fval


def ref_encode(R, N, enc, info_bits, prior=None):
    BMVD = R["BMVD"]
    xvd = BMVD.BinaryMemorylessVectorDistribution(N)
    xvd.probs[:] = np.array([0.5, 0.5]) if prior is None else prior
    return np.array(enc.encode(xvd, list(int(v) for v in info_bits)), np.uint8)


def save(name, meta, **arrays):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    print("wrote", path, "(%d bytes)" % os.path.getsize(path))


# ---------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------

def fx_bsc_n64(R, timing):
    """C1: N=64, K=32, BSC(0.11); frozen = 32 least reliable by the reference
    degrading construction (n=6, L=100), ranked by Pe; 1000 codewords."""
    BMD, BPED = R["BMD"], R["BPED"]
    n, N, K, L, p = 6, 64, 32, 100, 0.11
    bsc = BMD.makeBSC(p)
    dists = [bsc]
    for _ in range(n):
        nxt = []
        for d in dists:
            nxt.append(d.minusTransform().degrade(L))
            nxt.append(d.plusTransform().degrade(L))
        dists = nxt
    pe = [d.errorProb() for d in dists]
    order = sorted(range(N), key=lambda k: pe[k])
    frozen = set(order[K:])
    crs, irs, chs, T = 1, 1, 1, 1000
    info_rng = random.Random(irs)
    chan_rng = random.Random(chs)
    enc = BPED.BinaryPolarEncoderDecoder(N, frozen, crs)
    tx_info = np.zeros((T, K), np.uint8)
    y = np.zeros((T, N), np.uint8)
    for t in range(T):
        inf = [0 if info_rng.random() < 0.5 else 1 for _ in range(K)]
        tx_info[t] = inf
        x = ref_encode(R, N, enc, inf)
        for j in range(N):  # test2.py:29-50 channel, with an explicitly seeded RNG
            rnd = chan_rng.random()
            s = 0.0
            for yy in range(2):
                if s + bsc.probXGivenY(int(x[j]), yy) >= rnd:
                    y[t, j] = yy
                    break
                s += bsc.probXGivenY(int(x[j]), yy)
    table = np.array(bsc.probs, np.float64)  # [y][x]
    xy = table[y]
    enc, info, xhat, leaf, dt = ref_binary_decode_batch(R, N, frozen, crs, xy)
    mask, r, fval = frozen_arrays(enc, N)
    errs = int(np.sum(np.any(info != tx_info, axis=1)))
    timing["bsc_n64_decode_s_per_cw"] = dt
    save("bsc_n64", dict(config="C1", N=N, K=K, p=p, L=L, crs=crs, info_seed=irs, channel_seed=chs,
                         construction="reference degrade(L=100) ranked by Pe", frame_errors=errs, trials=T),
         frozen=mask, r=r, fval=fval, y=y, table=table, tx_info=tx_info, info=info, xhat=xhat, leaf_m=leaf)


def fx_awgn(R, timing, n, B, ebn0_db, seed, name, config):
    BPED = R["BPED"]
    N, K = 1 << n, 1 << (n - 1)
    sigma2 = 1.0 / (2.0 * 0.5 * 10 ** (ebn0_db / 10.0))
    frozen, _ = bhattacharyya_frozen(n, K, sigma2)
    crs = 7
    enc = BPED.BinaryPolarEncoderDecoder(N, frozen, crs)
    rng = np.random.default_rng(seed)
    tx_info = rng.integers(0, 2, size=(B, K)).astype(np.uint8)
    x = np.stack([ref_encode(R, N, enc, tx_info[b]) for b in range(B)])
    xy, _ = awgn_pairs(x, sigma2, rng)
    enc, info, xhat, leaf, dt = ref_binary_decode_batch(R, N, frozen, crs, xy)
    mask, r, fval = frozen_arrays(enc, N)
    errs = int(np.sum(np.any(info != tx_info, axis=1)))
    timing[name + "_decode_s_per_cw"] = dt
    save(name, dict(config=config, N=N, K=K, ebn0_db=ebn0_db, sigma2=sigma2, crs=crs, seed=seed,
                    construction="Bhattacharyya at design Eb/N0", frame_errors=errs, trials=B),
         frozen=mask, r=r, fval=fval, xy=xy, x=x, tx_info=tx_info, info=info, xhat=xhat, leaf_m=leaf)


def fx_edge(R, timing):
    """Hand-built inputs that exercise the tie / zero / subnormal rules:
    exact ties (p0 == p1), one-sided zeros (infinite LLR), (0,0) rows,
    subnormal and huge-ratio rows, at N = 2, 16 and 256."""
    rng = np.random.default_rng(1234)
    cases = []
    for n in (1, 2, 4, 8):
        N = 1 << n
        for variant in range(6):
            B = 24
            vals = np.array([0.0, 0.5, 0.25, 1.0, 0.125, 1e-300, 4.9e-324, 2.2e-308, 0.3, 0.7, 1e-5])
            if variant == 0:  # erasure-like: a few discrete levels, many ties and zeros
                xy = rng.choice(vals[:5], size=(B, N, 2))
            elif variant == 1:  # subnormal / tiny magnitudes
                xy = rng.choice(vals, size=(B, N, 2))
            elif variant == 2:  # random continuous
                xy = rng.random((B, N, 2))
            elif variant == 3:  # random with forced one-sided zeros
                xy = rng.random((B, N, 2))
                z = rng.random((B, N)) < 0.2
                side = rng.integers(0, 2, size=(B, N))
                xy[z, 0] *= side[z]
                xy[z, 1] *= 1 - side[z]
            elif variant == 4:  # ties everywhere
                v = rng.choice(vals[:5], size=(B, N, 1))
                xy = np.repeat(v, 2, axis=2)
                flip = rng.random((B, N)) < 0.3
                xy[flip, 1] = rng.random(int(flip.sum()))
            else:  # tiny scale: products underflow deep in the tree
                xy = rng.random((B, N, 2)) * 1e-120
            frozen = set(int(i) for i in np.nonzero(rng.random(N) < 0.5)[0])
            crs = int(rng.integers(-1, 50))
            enc, info, xhat, leaf, dt = ref_binary_decode_batch(R, N, frozen, crs, xy)
            mask, r, fval = frozen_arrays(enc, N)
            cases.append(dict(n=n, variant=variant, crs=crs, xy=xy, frozen=mask, r=r, fval=fval,
                              info=info, xhat=xhat, leaf_m=leaf))
    arrays = {}
    for i, c in enumerate(cases):
        for k, v in c.items():
            arrays["c%d_%s" % (i, k)] = np.asarray(v)
    save("edge_binary", dict(cases=len(cases), note="variants: 0 discrete 1 subnormal 2 random 3 one-sided zeros 4 ties 5 underflow"), **arrays)


def fx_prior(R, timing):
    """Non-uniform a-priori distribution: the x-tree decides frozen bits."""
    rng = np.random.default_rng(77)
    N, n = 64, 6
    frozen = set(int(i) for i in rng.permutation(N)[:28])
    xy = rng.random((40, N, 2))
    prior = np.array([0.7, 0.3])
    enc, info, xhat, leaf, dt = ref_binary_decode_batch(R, N, frozen, 11, xy, prior=prior)
    mask, r, fval = frozen_arrays(enc, N)
    tx = rng.integers(0, 2, size=(8, enc.k)).astype(np.uint8)
    xenc = np.stack([ref_encode(R, N, enc, tx[b], prior=prior) for b in range(8)])
    save("prior_n64", dict(N=N, crs=11, prior=prior.tolist()), frozen=mask, r=r, xy=xy, prior=prior,
         info=info, xhat=xhat, leaf_m=leaf, enc_info=tx, enc_x=xenc)


def fx_encode(R, timing):
    BPED = R["BPED"]
    rng = np.random.default_rng(5)
    out = {}
    for n in (1, 3, 5, 8, 10):
        N = 1 << n
        frozen = set(int(i) for i in np.nonzero(rng.random(N) < 0.4)[0])
        crs = int(rng.integers(-1, 100))
        enc = BPED.BinaryPolarEncoderDecoder(N, frozen, crs)
        B = 16
        tx = rng.integers(0, 2, size=(B, enc.k)).astype(np.uint8)
        x = np.stack([ref_encode(R, N, enc, tx[b]) for b in range(B)])
        u = np.stack([np.array(BPED.polarTransformOfBits([int(v) for v in x[b]]), np.uint8) for b in range(B)])
        mask, r, fval = frozen_arrays(enc, N)
        for k, v in dict(frozen=mask, r=r, fval=fval, info=tx, x=x, u=u).items():
            out["n%d_%s" % (n, k)] = v
    save("encode_binary", dict(ns=[1, 3, 5, 8, 10]), **out)


def fx_qsc(R, timing):
    """C4: q=4, N=256, QSC(0.11).  Frozen set: the binary Bhattacharyya ranking
    at z0 = 2*sqrt(p(1-p)) is used as a cheap stand-in (the reference q-ary
    degrading construction takes ~10 min); parity only needs SOME frozen set."""
    QPED, QMD = R["QPED"], R["QMD"]
    q, n, p = 4, 8, 0.11
    N, K = 1 << n, 128
    z = np.array([0.6])  # ranking proxy only
    for _ in range(n):
        nz = np.empty(2 * len(z))
        nz[0::2] = np.minimum(1.0, 2 * z - z * z)
        nz[1::2] = z * z
        z = nz
    order = sorted(range(N), key=lambda i: (z[i], i))
    frozen = set(order[K:])
    qsc = QMD.makeQSC(q, p)
    dec = QPED.QaryPolarEncoderDecoder(q, N, frozen, 1)
    xq = QMD.QaryMemorylessDistribution(q)
    xq.probs = [qsc.calcXMarginals()]
    xvd = xq.makeQaryMemorylessVectorDistribution(N, None)
    rng = random.Random(3)
    T = 160
    tx = np.zeros((T, K), np.uint8)
    y = np.zeros((T, N), np.uint8)
    xs = np.zeros((T, N), np.uint8)
    for t in range(T):
        inf = rng.choices(range(q), k=K)
        tx[t] = inf
        x = dec.encode(xvd, inf)
        xs[t] = x
        for j in range(N):
            rnd = rng.random()
            s = 0.0
            for yy in range(q):
                if s + qsc.probXGivenY(int(x[j]), yy) >= rnd:
                    y[t, j] = yy
                    break
                s += qsc.probXGivenY(int(x[j]), yy)
    table = np.array(qsc.probs, np.float64)
    info = np.zeros((T, K), np.uint8)
    t0 = time.perf_counter()
    for t in range(T):
        xyvd = qsc.makeQaryMemorylessVectorDistribution(N, [int(v) for v in y[t]])
        info[t] = dec.decode(xvd, xyvd)
    timing["qsc_q4_n256_decode_s_per_cw"] = (time.perf_counter() - t0) / T
    mask = np.array([1 if i in frozen else 0 for i in range(N)], np.uint8)
    errs = int(np.sum(np.any(info != tx, axis=1)))
    # extra: random continuous q-ary inputs (not channel-shaped), incl. zeros
    rs = np.random.default_rng(9)
    xr = rs.random((24, N, q))
    xr[rs.random((24, N)) < 0.1] = 0.0
    xr[:, :, 1][rs.random((24, N)) < 0.2] = 0.0
    info_r = np.zeros((24, K), np.uint8)
    for t in range(24):
        vd = R["QMVD"].QaryMemorylessVectorDistribution(q, N)
        vd.probs[:] = xr[t]
        info_r[t] = dec.decode(xvd, vd)
    save("qsc_q4_n256", dict(config="C4", q=q, N=N, K=K, p=p, seed=3, frame_errors=errs, trials=T,
                             construction="binary Bhattacharyya stand-in"),
         frozen=mask, y=y, table=table, tx_info=tx, x=xs, info=info, xy_rand=xr, info_rand=info_r)
    # q = 3 (non power of two) small case
    q3, n3 = 3, 5
    N3 = 1 << n3
    fr3 = set(int(i) for i in rs.permutation(N3)[:12])
    dec3 = QPED.QaryPolarEncoderDecoder(q3, N3, fr3, 1)
    x3 = rs.random((16, N3, q3))
    x3[rs.random((16, N3)) < 0.1] = 0.0
    xvd3 = R["QMVD"].QaryMemorylessVectorDistribution(q3, N3)
    xvd3.probs[:] = 1.0 / 3
    info3 = np.zeros((16, dec3.k), np.uint8)
    for t in range(16):
        vd = R["QMVD"].QaryMemorylessVectorDistribution(q3, N3)
        vd.probs[:] = x3[t]
        info3[t] = dec3.decode(xvd3, vd)
    tx3 = rs.integers(0, q3, size=(8, dec3.k))
    enc3 = np.stack([np.array(dec3.encode(xvd3, [int(v) for v in tx3[b]]), np.uint8) for b in range(8)])
    m3 = np.array([1 if i in fr3 else 0 for i in range(N3)], np.uint8)
    save("qary_q3_n32", dict(q=q3, N=N3), frozen=m3, xy=x3, info=info3, enc_info=tx3.astype(np.uint8), enc_x=enc3)


def fx_harness(R, timing):
    """The reference's own Monte-Carlo driver (encodeDecodeSimulation, BinaryPolarEncoderDecoder.py:328-387)
    with test2.py-style BSC closures and an explicitly seeded global RNG; records the printed line."""
    import contextlib
    import io
    BMD, BPED = R["BMD"], R["BPED"]
    g = np.load(os.path.join(OUT, "bsc_n64.npz"))
    frozen = set(int(i) for i in np.nonzero(g["frozen"])[0])
    N, T, seed = 64, 400, 5
    xy_dist = BMD.makeBSC(0.11)

    def make_x():
        xd = BMD.BinaryMemorylessDistribution()
        xd.probs.append([xy_dist.calcXMarginal(0), xy_dist.calcXMarginal(1)])
        return xd.makeBinaryMemorylessVectorDistribution(N, None)

    def channel(codeword):  # test2.py:29-50
        out = []
        for x in codeword:
            rnd = random.random()
            s = 0.0
            for y in range(len(xy_dist.probs)):
                if s + xy_dist.probXGivenY(x, y) >= rnd:
                    out.append(y)
                    break
                s += xy_dist.probXGivenY(x, y)
        return out

    def make_xy(received):
        return xy_dist.makeBinaryMemorylessVectorDistribution(len(received), received)

    random.seed(seed)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        BPED.encodeDecodeSimulation(N, make_x, lambda e: e, channel, make_xy, T, frozen)
    line = buf.getvalue().strip().splitlines()[-1]
    print("  reference printed:", line)
    save("harness_bsc_n64", dict(N=N, trials=T, global_seed=seed, p=0.11, line=line), frozen=g["frozen"])


def fx_harness_verbose(R, timing):
    """encodeDecodeSimulation with verbosity=1 (BinaryPolarEncoderDecoder.py:374-385): the
    per-error printout (information as a Python list, decoded/encoded as numpy arrays)."""
    import contextlib
    import io
    BMD, BPED = R["BMD"], R["BPED"]
    g = np.load(os.path.join(OUT, "bsc_n64.npz"))
    frozen = set(int(i) for i in np.nonzero(g["frozen"])[0])
    N, T, seed = 64, 40, 9
    xy_dist = BMD.makeBSC(0.11)

    def make_x():
        xd = BMD.BinaryMemorylessDistribution()
        xd.probs.append([xy_dist.calcXMarginal(0), xy_dist.calcXMarginal(1)])
        return xd.makeBinaryMemorylessVectorDistribution(N, None)

    def channel(codeword):
        out = []
        for x in codeword:
            rnd = random.random()
            s = 0.0
            for y in range(len(xy_dist.probs)):
                if s + xy_dist.probXGivenY(x, y) >= rnd:
                    out.append(y)
                    break
                s += xy_dist.probXGivenY(x, y)
        return out

    def make_xy(received):
        return xy_dist.makeBinaryMemorylessVectorDistribution(len(received), received)

    random.seed(seed)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        BPED.encodeDecodeSimulation(N, make_x, lambda e: e, channel, make_xy, T, frozen, verbosity=1)
    out = buf.getvalue()
    print("  reference verbose run: %d lines" % len(out.splitlines()))
    save("harness_verbose", dict(N=N, trials=T, global_seed=seed, p=0.11, stdout=out), frozen=g["frozen"])


def deletion_closures(R, n, n0, pd, xi, ones, channel_seed):
    """The main_deletion.py:17-59 closures, rebuilt from the reference modules (main_deletion.py
    itself runs main() on import)."""
    import Guardbands as GB
    BMD, BT, CBT = R["BMD"], R["BT"], R["CBT"]
    N = 1 << n

    def make_x():
        xd = BMD.BinaryMemorylessDistribution()
        xd.probs.append([0.5, 0.5])
        return xd.makeBinaryMemorylessVectorDistribution(N, None)

    def make_codeword(enc):
        return GB.addDeletionGuardBands(enc, n, n0, xi, ones)

    rng = random.Random()
    rng.seed(channel_seed)

    def channel(cw):
        return BT.deletionChannelSimulation(cw, pd, seed=None, randomNumberGenerator=rng)

    def make_xy(received, verbosity=0):
        return CBT.buildCollectionOfBinaryTrellises_uniformInput_deletion(received, pd, xi, n, n0, ones, verbosity)

    return make_x, make_codeword, channel, make_xy


def ref_deletion_trials(R, n, n0, pd, xi, ones, frozen, crs, info_seed, channel_seed, T, rx_override=None):
    """encodeDecodeSimulation (BinaryPolarEncoderDecoder.py:328-387) unrolled so that every
    received word, transmitted/decoded information, x_hat and leaf marginal is recorded."""
    BPED = R["BPED"]
    N = 1 << n
    make_x, make_codeword, channel, make_xy = deletion_closures(R, n, n0, pd, xi, ones, channel_seed)
    xvd = make_x()
    enc = BPED.BinaryPolarEncoderDecoder(N, frozen, crs)
    irng = random.Random()
    irng.seed(info_seed)
    words, tx, info, xhat, leaf = [], [], [], [], []
    t0 = time.perf_counter()
    for t in range(T):
        inf = [0 if irng.random() < 0.5 else 1 for _ in range(enc.k)]
        cw = make_codeword(enc.encode(xvd, inf))
        rx = channel(cw) if rx_override is None else list(rx_override[t])
        with LeafRecorder(R) as lr:
            xh, di = enc.decode(xvd, make_xy(rx))
        assert len(lr.rec) == N
        words.append(rx)
        tx.append(inf)
        info.append(list(di))
        xhat.append(list(xh))
        leaf.append(lr.rec)
    dt = (time.perf_counter() - t0) / max(T, 1)
    W = max([len(w) for w in words] + [1])
    rx = np.zeros((T, W), np.uint8)
    for t, w in enumerate(words):
        rx[t, :len(w)] = w
    lens = np.array([len(w) for w in words], np.int32)
    mask, r, fval = frozen_arrays(enc, N)
    return dict(rx=rx, rx_len=lens, tx_info=np.array(tx, np.uint8).reshape(T, enc.k),
                info=np.array(info, np.uint8).reshape(T, enc.k), xhat=np.array(xhat, np.uint8),
                leaf_m=np.array(leaf), frozen=mask, r=r, fval=fval, cw_len=len(cw)), dt


def fx_deletion(R, timing):
    """C5: main_deletion.py defaults (pd=0.1, xi=0.1, n0=n//3, ones=0, seeds cs=100 crs=200
    gs=300 is=400) at n=8; frozen set from the reference's own genie
    (genieEncodeDecodeSimulation, 100 trials, Pe bound 0.1, trustXYProbs=False)."""
    import contextlib
    import io
    BPED = R["BPED"]
    n, n0, pd, xi, ones = 8, 2, 0.1, 0.1, 0
    N = 1 << n
    make_x, make_codeword, channel, make_xy = deletion_closures(R, n, n0, pd, xi, ones, 100)
    G = 100
    buf = io.StringIO()
    captured = {}
    orig = BPED.frozenSetFromTVAndPe

    def capture(TV, Pe, bound):
        captured["score"] = [a + b for a, b in zip(TV, Pe)]
        return orig(TV, Pe, bound)

    BPED.frozenSetFromTVAndPe = capture
    try:
        with contextlib.redirect_stdout(buf):
            frozen = BPED.genieEncodeDecodeSimulation(N, make_x, make_codeword, channel, make_xy, G, 0.1,
                                                      genieSeed=300, trustXYProbs=False, filename=None)
    finally:
        BPED.frozenSetFromTVAndPe = orig
    # The genie set at this trial count keeps very few information bits; the decode
    # fixture uses the K = N/4 indices of smallest genie TV+Pe so that decisions matter.
    score = captured["score"]
    order = sorted(range(N), key=lambda i: (score[i], i))
    frozen_dec = set(order[N // 4:])
    T = 48
    d, dt = ref_deletion_trials(R, n, n0, pd, xi, ones, frozen_dec, 200, 400, 100, T)
    timing["deletion_n8_decode_s_per_cw"] = dt
    errs = int(np.sum(np.any(d["info"] != d["tx_info"], axis=1)))
    # the reference's own MC driver on the same closures: the printed line
    make_x, make_codeword, channel, make_xy = deletion_closures(R, n, n0, pd, xi, ones, 100)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        BPED.encodeDecodeSimulation(N, make_x, make_codeword, channel, make_xy, 24, frozen,
                                    commonRandomnessSeed=200, randomInformationSeed=400)
    line = buf.getvalue().strip().splitlines()[-1]
    print("  reference printed:", line, "| codeword length", d["cw_len"], "| K", N - len(frozen))
    save("deletion_n8", dict(config="C5", n=n, n0=n0, pd=pd, xi=xi, ones=ones, crs=200, info_seed=400,
                             channel_seed=100, genie_seed=300, genie_trials=G, trials=T, frame_errors=errs,
                             mc_trials=24, line=line, cw_len=d.pop("cw_len"), genie_K=N - len(frozen),
                             decode_frozen="K=N/4 smallest genie TV+Pe"),
         genie_frozen=np.array([1 if i in frozen else 0 for i in range(N)], np.uint8),
         genie_score=np.array(score), **d)


def fx_deletion_edge(R, timing):
    """Other (n, n0, pd) shapes, random frozen sets, and received words that break the
    guard-band parse (segments longer than the trellis, empty, all-zero, raw random words)."""
    rng = np.random.default_rng(42)
    out = {}
    cases = [(4, 1, 0.1, 0), (5, 2, 0.2, 0), (6, 2, 0.1, 0), (6, 3, 0.05, 0), (7, 2, 0.3, 0), (8, 2, 0.1, 0),
             (9, 3, 0.1, 0), (5, 4, 0.1, 0), (4, 2, 0.1, 0), (6, 2, 0.1, 1), (5, 1, 0.15, 2)]
    for ci, (n, n0, pd, ones) in enumerate(cases):
        N = 1 << n
        frozen = set(int(i) for i in np.nonzero(rng.random(N) < 0.5)[0])
        T = 12 if n <= 8 else 6
        crs = int(rng.integers(-1, 500))
        d, _ = ref_deletion_trials(R, n, n0, pd, 0.1, ones, frozen, crs, int(rng.integers(1, 999)),
                                   int(rng.integers(1, 999)), T)
        # replace a few received words by adversarial ones (decoded by the reference again)
        import Guardbands as GB
        cwl = len(GB.addDeletionGuardBands([0] * N, n, n0, 0.1, ones))
        adv = [list(w[:l]) for w, l in zip(d["rx"], d["rx_len"])]
        adv[0] = []
        adv[1] = [0] * (cwl // 2)
        adv[2] = [int(b) for b in rng.integers(0, 2, cwl)]
        adv[3] = [1] * (cwl - 3)
        adv[4] = [int(b) for b in rng.integers(0, 2, max(1, cwl // 3))]
        d, _ = ref_deletion_trials(R, n, n0, pd, 0.1, ones, frozen, crs, 1, 1, T, rx_override=adv)
        d.pop("cw_len")
        for k, v in d.items():
            out["c%d_%s" % (ci, k)] = v
        out["c%d_shape" % ci] = np.array([n, n0, ones], np.int32)
        out["c%d_pd" % ci] = np.array([pd])
    save("deletion_edge", dict(cases=len(cases), note="(n, n0, pd, ones) per case; words 0-4 adversarial"), **out)


def fx_genie_bsc(R, timing):
    """The reference's genie construction (genieEncodeDecodeSimulation, BinaryPolarEncoderDecoder.py:390-491)
    on BSC(0.11), n=6, 300 trials, trustXYProbs=True, with a seeded channel RNG; records the
    TV and Pe vectors it hands to frozenSetFromTVAndPe and the frozen set it returns."""
    import contextlib
    import io
    BMD, BPED = R["BMD"], R["BPED"]
    N, T, p, gseed, cseed, bound = 64, 300, 0.11, 77, 5, 0.05
    bsc = BMD.makeBSC(p)
    crng = random.Random(cseed)

    def make_x():
        xd = BMD.BinaryMemorylessDistribution()
        xd.probs.append([bsc.calcXMarginal(0), bsc.calcXMarginal(1)])
        return xd.makeBinaryMemorylessVectorDistribution(N, None)

    def channel(codeword):  # test2.py:29-50 with an explicit RNG instance
        out = []
        for x in codeword:
            rnd = crng.random()
            acc = 0.0
            for y in range(2):
                if acc + bsc.probXGivenY(int(x), y) >= rnd:
                    out.append(y)
                    break
                acc += bsc.probXGivenY(int(x), y)
        return out

    def make_xy(received):
        return bsc.makeBinaryMemorylessVectorDistribution(len(received), received)

    cap = {}
    orig = BPED.frozenSetFromTVAndPe

    def capture(TV, Pe, b):
        cap["TV"], cap["Pe"] = [float(v) for v in TV], [float(v) for v in Pe]
        return orig(TV, Pe, b)

    BPED.frozenSetFromTVAndPe = capture
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            frozen = BPED.genieEncodeDecodeSimulation(N, make_x, lambda e: e, channel, make_xy, T, bound,
                                                      genieSeed=gseed, trustXYProbs=True)
    finally:
        BPED.frozenSetFromTVAndPe = orig
    save("genie_bsc_n64", dict(N=N, trials=T, p=p, genie_seed=gseed, channel_seed=cseed, bound=bound,
                               trust=True),
         TV=np.array(cap["TV"]), Pe=np.array(cap["Pe"]),
         frozen=np.array([1 if i in frozen else 0 for i in range(N)], np.uint8))


def fx_main_deletion(R, timing):
    """The reference's main_deletion.py itself (runpy, its own argv parsing) with
    -n 8 -g 100 -e 40 and default seeds; records its stdout lines."""
    import contextlib
    import io
    import runpy
    argv = ["main_deletion.py", "-n", "8", "-g", "100", "-e", "40"]
    old = sys.argv
    sys.argv = argv
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            runpy.run_path(os.path.join(REF, "main_deletion.py"), run_name="__main__")
    finally:
        sys.argv = old
    lines = buf.getvalue().strip().splitlines()
    keep = [l for l in lines if not l.startswith(("TVVec", "pevec", "HEncvec", "HDecvec"))]
    print("  reference main_deletion:", keep[-1])
    save("main_deletion_n8", dict(argv=argv[1:], lines=keep))


def fx_test2(R, timing):
    """The reference's test2.py itself (runpy): Tal-Vardy construction for BSC(0.11),
    n=7, L=100, bound 0.1, then 4000 encode/decode trials.  Its channel draws from the
    global `random` (unseeded in the script, test2.py:37); it is seeded with 7 here.
    Records the stdout lines."""
    import contextlib
    import io
    import runpy
    buf = io.StringIO()
    t0 = time.time()
    random.seed(7)
    with contextlib.redirect_stdout(buf):
        runpy.run_path(os.path.join(REF, "test2.py"), run_name="__main__")
    timing["test2_full_run_s"] = time.time() - t0
    lines = buf.getvalue().strip().splitlines()
    print("  reference test2:", lines[-1])
    save("test2_run", dict(global_random_seed=7, lines=lines))


def _construct_sources(R):
    """Scalar channels for the construction fixtures (build-side choices)."""
    BMD = R["BMD"]
    rng = np.random.default_rng(2024)
    out = {"bsc": BMD.makeBSC(0.11), "bec": BMD.makeBEC(0.3)}
    rnd = BMD.BinaryMemorylessDistribution()
    for _ in range(10):
        a, b = rng.random(2)
        rnd.append([float(a), float(b)])
    rnd.append(list(rnd.probs[3]))                                  # exact duplicate letter
    rnd.append([rnd.probs[5][0] * (1 + 3e-10), rnd.probs[5][1]])  # within math.isclose
    rnd.append([0.0, 0.0])                                          # zero-probability letter
    rnd.append([0.2, 0.2])                                          # LLR 0
    out["random"] = rnd
    awgn = BMD.BinaryMemorylessDistribution()                       # BI-AWGN quantised to 48 letters
    s2 = 0.63
    edges = np.linspace(-4, 4, 47)
    grid = np.concatenate([[-np.inf], edges, [np.inf]])
    from math import erf, sqrt

    def cdf(v, m):
        return 0.5 * (1 + erf((v - m) / sqrt(2 * s2))) if np.isfinite(v) else (0.0 if v < 0 else 1.0)
    for lo, hi in zip(grid[:-1], grid[1:]):
        awgn.append([0.5 * (cdf(hi, 1.0) - cdf(lo, 1.0)), 0.5 * (cdf(hi, -1.0) - cdf(lo, -1.0))])
    out["awgn48"] = awgn
    return out


def fx_construct_bin(R, timing):
    """Tal-Vardy construction (section 8(f) rank 3): the reference's own
    mergeEquivalentSymbols / degrade / upgrade on several channels and their polar
    transforms (auxiliary letter sets included), and calcFrozenSet_degradingUpgrading's
    Pe vectors + frozen sets (TV = 0: the reference crashes with an x distribution)."""
    import copy
    BMD = R["BMD"]
    arrays, cases = {}, []

    def dist(pairs):
        d = BMD.BinaryMemorylessDistribution()
        for p in pairs:
            d.append([float(p[0]), float(p[1])])
        return d

    for sname, src in _construct_sources(R).items():
        variants = {"": src, "m": src.minusTransform(), "p": src.plusTransform()}
        variants["pm"] = variants["m"].plusTransform() if len(src.probs) <= 4 else None
        for vname, d0 in variants.items():
            if d0 is None:
                continue
            case = sname + ("_" + vname if vname else "")
            pairs = [list(p) for p in d0.probs]
            arrays[case + "_in"] = np.array(pairs, np.float64)
            d = dist(pairs)
            d.auxiliary = [{i} for i in range(len(pairs))]
            d.mergeEquivalentSymbols()
            arrays[case + "_merged"] = np.array(d.probs, np.float64)
            arrays[case + "_merged_aux"] = _aux_groups(d.auxiliary, len(pairs))
            rec = {"case": case, "deg": [], "up": [], "up_err": []}
            for L in (1, 2, 3, 8, 32):
                d = dist(pairs)
                d.auxiliary = [{i} for i in range(len(pairs))]
                o = d.degrade(L)
                arrays["%s_deg%d" % (case, L)] = np.array(o.probs, np.float64)
                arrays["%s_deg%d_aux" % (case, L)] = _aux_groups(o.auxiliary, len(pairs))
                rec["deg"].append(L)
            for L in (1, 2, 3, 8, 32):
                d = dist(pairs)
                try:
                    o = d.upgrade(L)
                except Exception as e:  # the reference's own failure, recorded as expected
                    rec["up_err"].append([L, type(e).__name__])
                    continue
                arrays["%s_up%d" % (case, L)] = np.array(o.probs, np.float64)
                rec["up"].append(L)
            cases.append(rec)
    trees = []
    for tname, n, L, bound, src in (("bsc_test2", 7, 100, 0.1, BMD.makeBSC(0.11)), ("bec", 6, 16, 0.05, BMD.makeBEC(0.4)),
                                     ("random", 5, 8, 0.2, None)):
        if src is None:
            src = dist(_construct_sources(R)["random"].probs[:6])
        pairs = [list(p) for p in src.probs]
        t0 = time.time()
        Pe = []
        orig = R["BPED"].frozenSetFromTVAndPe

        def capture(TV, Pe_, b, _orig=orig):
            Pe.extend(Pe_)
            return _orig(TV, Pe_, b)
        R["BPED"].frozenSetFromTVAndPe = capture
        try:
            fz = BMD.calcFrozenSet_degradingUpgrading(n, L, bound, None, copy.deepcopy(src))
        finally:
            R["BPED"].frozenSetFromTVAndPe = orig
        timing["construct_%s_n%d_L%d_s" % (tname, n, L)] = time.time() - t0
        arrays[tname + "_tree_in"] = np.array(pairs, np.float64)
        arrays[tname + "_tree_pe"] = np.array(Pe, np.float64)
        mask = np.zeros(1 << n, np.uint8)
        mask[sorted(fz)] = 1
        arrays[tname + "_tree_frozen"] = mask
        trees.append({"name": tname, "n": n, "L": L, "bound": bound})
    # LinkedListHeap with tied keys: extraction order, neighbour key updates, final list
    sys.path.insert(0, os.path.join(REF, "ScalarDistributions", "UpgradingDegrading"))
    from ScalarDistributions.UpgradingDegrading import LinkedListHeap as LLH
    hr = np.random.default_rng(11)
    keys = hr.integers(0, 6, 40).astype(np.float64)
    upd = hr.integers(0, 6, 2 * 30).astype(np.float64)
    h = LLH.LinkedListHeap(list(keys), list(range(40)))
    order, ui = [], 0
    for _ in range(30):
        e = h.extractHeapMin()
        order.append(e.data)
        for nb in (e.leftElementInList, e.rightElementInList):
            if nb is not None:
                h.updateKey(nb, float(upd[ui]))
            ui += 1
    arrays["heap_keys"] = keys
    arrays["heap_updates"] = upd
    arrays["heap_order"] = np.array(order, np.int64)
    arrays["heap_final_list"] = np.array(h.returnData(), np.int64)
    arrays["heap_final_array"] = np.array([el.data for el in h._heapArray], np.int64)
    save("construct_bin", {"cases": cases, "trees": trees,
                           "note": "reference BinaryMemorylessDistribution merge/degrade/upgrade/calcFrozenSet_degradingUpgrading"},
         **arrays)


def _qsc_channel_closure(qsc):
    """test3.py:35-55 channel: one global random.random() per symbol, cumulative P(y|x)."""
    def channel(codeword):
        out = []
        for x in codeword:
            rnd = random.random()
            s = 0.0
            for y in range(len(qsc.probs)):
                if s + qsc.probXGivenY(int(x), y) >= rnd:
                    out.append(y)
                    break
                s += qsc.probXGivenY(int(x), y)
        return out
    return channel


def _qary_tv_pe(R, n, L, xy_dist, x_dist=None):
    """calcTVAndPe_degradingUpgrading (ScalarDistributions/QaryMemorylessDistribution.py:934-991)
    through its own .npy cache in a temporary directory (it returns None without one)."""
    import tempfile
    QMD = R["QMD"]
    with tempfile.TemporaryDirectory() as d:
        tv, pe = QMD.calcTVAndPe_degradingUpgrading(n, L, x_dist, xy_dist, d + "/")
    return np.asarray(tv, np.float64), np.asarray(pe, np.float64)


def fx_construct_qary(R, timing):
    """q-ary degrading construction (section 8(f) rank 3): the reference's own
    QaryMemorylessDistribution.degrade (dynamic: one-hot binary channels degraded to
    M = floor(L^(1/(q-1))) letters, product re-indexing) on polar-transformed QSC/QEC
    channels, whole-tree Pe vectors (calcTVAndPe_degradingUpgrading) and the frozen sets of
    frozenSetFromTVAndPe, including the C4 code: q=4, n=8, L=64, QSC(0.11),
    numInfoIndices=127 (K=128, QaryPolarEncoderDecoder.py:1173-1176 off-by-one)."""
    QMD, QPED = R["QMD"], R["QPED"]
    arrays, cases, trees = {}, [], []
    chans = {"qsc3": QMD.makeQSC(3, 0.2), "qsc4": QMD.makeQSC(4, 0.11), "qec3": QMD.makeQEC(3, 0.3),
             "qsc5": QMD.makeQSC(5, 0.15)}
    for cname, ch in chans.items():
        variants = {"": ch, "m": ch.minusTransform(), "p": ch.plusTransform()}
        if ch.q <= 3:
            variants["mp"] = variants["m"].plusTransform()
        for vname, d0 in variants.items():
            case = cname + ("_" + vname if vname else "")
            arrays[case + "_in"] = np.array(d0.probs, np.float64)
            for L in (4, 9, 16, 64):
                import copy
                o = copy.deepcopy(d0).degrade(L)
                arrays["%s_deg%d" % (case, L)] = np.array(o.probs, np.float64).reshape(-1, ch.q)
            cases.append(case)
    for tname, q, n, L, p, kinfo in (("qsc3_n4_L16", 3, 4, 16, 0.2, None), ("qsc4_n3_L27", 4, 3, 27, 0.11, None),
                                     ("qsc4_n5_L64", 4, 5, 64, 0.11, 15), ("qsc2_n6_L16", 2, 6, 16, 0.11, None),
                                     ("qsc4_n8_L64", 4, 8, 64, 0.11, 127)):
        t0 = time.time()
        ch = QMD.makeQSC(q, p)
        tv, pe = _qary_tv_pe(R, n, L, ch)
        timing["construct_qary_%s_s" % tname] = time.time() - t0
        bound = 0.1
        fz = QPED.frozenSetFromTVAndPe(tv, pe, None if kinfo is not None else bound, kinfo)
        mask = np.zeros(1 << n, np.uint8)
        mask[sorted(fz)] = 1
        arrays[tname + "_tv"] = tv
        arrays[tname + "_pe"] = pe
        arrays[tname + "_frozen"] = mask
        trees.append({"name": tname, "q": q, "n": n, "L": L, "p": p, "numInfoIndices": kinfo,
                      "bound": None if kinfo is not None else bound, "K": int((1 << n) - mask.sum()),
                      "seconds": round(time.time() - t0, 1)})
        print("  tree %s: K=%d (%.1f s)" % (tname, (1 << n) - mask.sum(), time.time() - t0))
    save("construct_qary", {"cases": cases, "trees": trees,
                            "note": "reference QaryMemorylessDistribution.degrade / calcTVAndPe_degradingUpgrading / "
                                    "QaryPolarEncoderDecoder.frozenSetFromTVAndPe; xDistribution=None (TV=0)"},
         **arrays)


def fx_qary_harness(R, timing):
    """The reference's q-ary Monte-Carlo driver (QaryPolarEncoderDecoder.encodeDecodeSimulation,
    QaryPolarEncoderDecoder.py:935-982) with the test3.py:21-70 closures and a seeded global
    channel RNG; records the printed line and the per-trial words to replay it."""
    import contextlib
    import io
    QMD, QPED = R["QMD"], R["QPED"]
    g = np.load(os.path.join(OUT, "construct_qary.npz"))
    out, runs = {}, []
    for name, q, n, p, T, seed, fkey in (("q4_n5", 4, 5, 0.11, 300, 11, "qsc4_n5_L64_frozen"),
                                         ("q3_n4", 3, 4, 0.2, 400, 12, "qsc3_n4_L16_frozen")):
        N = 1 << n
        frozen = set(int(i) for i in np.nonzero(g[fkey])[0])
        qsc = QMD.makeQSC(q, p)

        def make_x(q=q, qsc=qsc, N=N):
            xd = QMD.QaryMemorylessDistribution(q)
            xd.probs = [qsc.calcXMarginals()]
            return xd.makeQaryMemorylessVectorDistribution(N, None)

        def make_xy(rx, qsc=qsc):
            return qsc.makeQaryMemorylessVectorDistribution(len(rx), rx)

        random.seed(seed)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            QPED.encodeDecodeSimulation(q, N, make_x, lambda e: e, _qsc_channel_closure(qsc), make_xy, T, frozen)
        line = buf.getvalue().strip().splitlines()[-1]
        print("  reference q-ary printed:", line)
        runs.append(dict(name=name, q=q, n=n, p=p, trials=T, global_seed=seed, frozen_key=fkey, line=line))
        out[name + "_frozen"] = g[fkey]
    save("qary_harness", dict(runs=runs), **out)


def _joint(QMD, prior, W):
    """Joint q-ary distribution probs[y][x] = prior[x] * W[x][y] (build-side choice)."""
    q = len(prior)
    d = QMD.QaryMemorylessDistribution(q)
    for y in range(len(W[0])):
        d.append([prior[x] * W[x][y] for x in range(q)])
    return d


def fx_construct_qary_up(R, timing):
    """q-ary upgrading (QaryMemorylessDistribution.upgrade_dynamic, :329-475: one-hot binary
    channels upgraded with left/centre/right auxiliary sets, then recombined letter by letter)
    on a-priori distributions (makeInputDistribution) and joint channels and their polar
    transforms, and whole trees with an a-priori distribution (TV from the upgraded x tree,
    calcTVAndPe_degradingUpgrading :934-991) and their frozen sets."""
    import copy
    QMD, QPED = R["QMD"], R["QPED"]
    arrays, cases, trees, errors = {}, [], [], {}
    W3 = [[0.7, 0.2, 0.1], [0.15, 0.7, 0.15], [0.1, 0.2, 0.7]]
    srcs = {"x3": QMD.makeInputDistribution([0.5, 0.3, 0.2]), "x4": QMD.makeInputDistribution([0.4, 0.3, 0.2, 0.1]),
            "x5": QMD.makeInputDistribution([0.3, 0.25, 0.2, 0.15, 0.1]),
            "j3": _joint(QMD, [0.5, 0.3, 0.2], W3), "qsc4": QMD.makeQSC(4, 0.11), "qec3": QMD.makeQEC(3, 0.3)}
    for cname, ch in srcs.items():
        variants = {"": ch, "m": ch.minusTransform(), "p": ch.plusTransform()}
        if ch.q <= 4:
            variants["mp"] = variants["m"].plusTransform()
            variants["pm"] = variants["p"].minusTransform()
        for vname, d0 in variants.items():
            case = cname + ("_" + vname if vname else "")
            arrays[case + "_in"] = np.array(d0.probs, np.float64)
            for L in (4, 9, 16, 64):
                for op in ("up", "deg"):
                    try:
                        o = getattr(copy.deepcopy(d0), "upgrade" if op == "up" else "degrade")(L)
                        arrays["%s_%s%d" % (case, op, L)] = np.array(o.probs, np.float64).reshape(-1, ch.q)
                    except Exception as e:  # the reference's own failure, recorded as the expected outcome
                        errors["%s_%s%d" % (case, op, L)] = type(e).__name__
            cases.append(case)
    for tname, q, n, L, prior, kinfo in (("j3_n4_L16", 3, 4, 16, [0.5, 0.3, 0.2], 5),
                                         ("j3_n5_L9", 3, 5, 9, [0.5, 0.3, 0.2], 10),
                                         ("j4_n3_L27", 4, 3, 27, [0.4, 0.3, 0.2, 0.1], 3)):
        t0 = time.time()
        if q == 3:
            xy = _joint(QMD, prior, W3)
        else:
            W4 = [[0.85 if x == y else 0.05 for y in range(4)] for x in range(4)]
            xy = _joint(QMD, prior, W4)
        xd = QMD.makeInputDistribution(prior)
        tv, pe = _qary_tv_pe(R, n, L, xy, xd)
        bound = 0.2
        fz = QPED.frozenSetFromTVAndPe(tv, pe, None if kinfo is not None else bound, kinfo)
        mask = np.zeros(1 << n, np.uint8)
        mask[sorted(fz)] = 1
        arrays[tname + "_xy"] = np.array(xy.probs, np.float64)
        arrays[tname + "_x"] = np.array(xd.probs, np.float64)
        arrays[tname + "_tv"] = tv
        arrays[tname + "_pe"] = pe
        arrays[tname + "_frozen"] = mask
        trees.append({"name": tname, "q": q, "n": n, "L": L, "prior": prior, "numInfoIndices": kinfo,
                      "bound": None if kinfo is not None else bound, "K": int((1 << n) - mask.sum()),
                      "seconds": round(time.time() - t0, 1)})
        print("  tree %s: K=%d (%.1f s)" % (tname, (1 << n) - mask.sum(), time.time() - t0))
    save("construct_qary_up", {"cases": cases, "trees": trees, "errors": errors,
                               "note": "reference QaryMemorylessDistribution.upgrade/degrade and "
                                       "calcTVAndPe_degradingUpgrading with an a-priori distribution"}, **arrays)


def fx_combine_codes(R, timing):
    """The reference's combine_codes.py itself (runpy, its own argv) on two frozen-set files in
    BinaryPolarEncoderDecoder's genie format (build-side synthetic contents): printed line and
    the 'out' file it writes."""
    import contextlib
    import io
    import runpy
    import tempfile
    rng = np.random.default_rng(77)
    files, texts = [], []
    with tempfile.TemporaryDirectory() as d:
        for k, (N, M) in enumerate(((64, 100), (64, 250))):
            v = rng.random(N) * rng.choice([0.0, 1.0, 30.0], N)
            lines = ["* main_deletion.py -n 6 -g %d" % M]
            lines += [str(i) for i in range(0, N, 3)]
            lines += ["** number of trials = %d" % M, "* (TotalVariation+errorProbability) * (number of trials)"]
            lines += ["*** %d %s" % (i, repr(float(v[i]))) for i in range(N)]
            path = os.path.join(d, "frozen%d.txt" % k)
            with open(path, "w") as f:
                f.write("\n".join(lines) + "\n")
            files.append(path)
            texts.append("\n".join(lines) + "\n")
        cwd, argv = os.getcwd(), sys.argv
        buf = io.StringIO()
        try:
            os.chdir(d)
            sys.argv = ["combine_codes.py"] + files
            with contextlib.redirect_stdout(buf):
                runpy.run_path(os.path.join(REF, "combine_codes.py"), run_name="__main__")
        finally:
            os.chdir(cwd)
            sys.argv = argv
        out = open(os.path.join(d, "out")).read()
    save("combine_codes", {"argv_files": 2}, inputs=np.array(texts), stdout=np.array(buf.getvalue()),
         out=np.array(out))


def fx_scl(R, timing, use_log=False):
    """The reference's q-ary list decoder (QaryPolarEncoderDecoder.listDecode / recursiveListDecode,
    :118-227, 403-820) on tie-free inputs (continuous random rows, no zeros), with an actual
    information word: the final list (informationList[:finalListSize], captured from the
    outermost recursiveListDecode return), prob_list, actual_prob and the returned ProbResult.
    The list ORDER is numpy-argpartition-dependent; tests compare it as a set.
    use_log=True: the same cases in the log domain (QaryPolarEncoderDecoder(..., use_log=True), rows
    np.log of the linear ones, log-domain vector distributions) -> scl_log.npz."""
    QPED = R["QPED"]
    rs = np.random.default_rng(404)
    lg = np.log if use_log else (lambda a: a)
    out, cases = {}, []
    specs = [(2, 3, 2, 0.5), (2, 4, 4, 0.5), (3, 3, 2, 0.4), (3, 4, 4, 0.5), (4, 3, 4, 0.5), (4, 4, 8, 0.5),
             (2, 5, 8, 0.6), (3, 5, 3, 0.5), (4, 5, 4, 0.6), (2, 4, 1, 0.5), (4, 4, 16, 0.3), (3, 3, 8, 0.2)]
    for ci, (q, n, L, fr) in enumerate(specs):
        N = 1 << n
        frozen = set(int(i) for i in np.nonzero(rs.random(N) < fr)[0])
        dec = QPED.QaryPolarEncoderDecoder(q, N, frozen, 1, use_log=use_log)
        T = 12
        K = dec.k
        xy = lg(rs.random((T, N, q)) * 0.98 + 0.02)
        fv = rs.integers(0, q, (T, len(frozen)))
        act = rs.integers(0, q, (T, K))
        infos = np.full((T, L, K), -1, np.int64)
        probs = np.full((T, L), np.nan)
        sizes = np.zeros(T, np.int64)
        aprob = np.zeros(T)
        ret = np.zeros((T, K), np.int64)
        pres = []
        for t in range(T):
            vd = R["QMVD"].QaryMemorylessVectorDistribution(q, N, use_log=use_log)
            vd.probs[:] = xy[t]
            orig = dec.recursiveListDecode
            depth = [0]
            top = {}

            def wrapped(*a, _orig=orig, **k):
                depth[0] += 1
                try:
                    r = _orig(*a, **k)
                finally:
                    depth[0] -= 1
                if depth[0] == 0:
                    top["r"] = r
                return r
            dec.recursiveListDecode = wrapped
            try:
                info, pr = dec.listDecode(vd, fv[t], L, np.zeros((K, 0), np.int64), np.zeros(0, np.int64),
                                          actualInformation=act[t])
            finally:
                del dec.recursiveListDecode
            il, _, _, _, fls, _, _ = top["r"]
            sizes[t] = fls
            infos[t, :fls] = il[:fls]
            probs[t, :fls] = dec.prob_list[:fls]
            aprob[t] = dec.actual_prob
            ret[t] = info
            pres.append(pr.name)
        tag = "c%d" % ci
        out.update({tag + "_xy": xy, tag + "_frozen": np.array([1 if i in frozen else 0 for i in range(N)], np.uint8),
                    tag + "_fv": fv.astype(np.uint8), tag + "_actual": act.astype(np.uint8), tag + "_info": infos,
                    tag + "_prob": probs, tag + "_size": sizes, tag + "_aprob": aprob, tag + "_ret": ret})
        cases.append(dict(tag=tag, q=q, n=n, L=L, K=K, prob_result=pres))
    # the reference's irSimulation (:887-930) over a continuous channel (no ties): a q-ary symbol
    # plus Gaussian noise, likelihood rows exp(-(b - x)^2 / 2 s^2) (build-side closures)
    import contextlib
    import io
    import random as _random
    irs = []
    for name, q, n, L, T, sig, cs in (("ir_q3_n4", 3, 4, 4, 60, 0.45, 2), ("ir_q2_n5", 2, 5, 8, 60, 0.6, 1)):
        N = 1 << n
        frozen = set(int(i) for i in np.nonzero(np.random.default_rng(9 + q).random(N) < 0.5)[0])
        chan = _random.Random(1234 + q)

        def simulate(a, _c=chan, _s=sig):
            return [float(x) + _c.gauss(0.0, _s) for x in a]

        def make_xy(b, _q=q, _s=sig, _N=N):
            vd = R["QMVD"].QaryMemorylessVectorDistribution(_q, _N, use_log=use_log)
            for i, y in enumerate(b):
                if use_log:  # log-likelihood rows
                    vd.probs[i] = [-((y - x) ** 2) / (2 * _s * _s) for x in range(_q)]
                else:
                    vd.probs[i] = [math.exp(-((y - x) ** 2) / (2 * _s * _s)) for x in range(_q)]
            return vd
        np.random.seed(77)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            fe, se, rate, prl = QPED.irSimulation(q, N, simulate, make_xy, T, frozen, L, cs, use_log=use_log,
                                                  verbosity=1)
        out[name + "_frozen"] = np.array([1 if i in frozen else 0 for i in range(N)], np.uint8)
        irs.append(dict(name=name, q=q, n=n, L=L, trials=T, sigma=sig, check_size=cs, chan_seed=1234 + q,
                        np_seed=77, frame_error_prob=fe, symbol_error_prob=float(se), rate=rate,
                        prob_results=[p.name for p in prl], printed=buf.getvalue()))
    save("scl_log" if use_log else "scl", dict(cases=cases, ir=irs, use_log=use_log,
                                               note="listDecode with actualInformation; list order is argpartition's"),
         **out)


def fx_qary_log(R, timing):
    """use_log=True q-ary decodes (VectorDistributions/QaryMemorylessVectorDistribution.py:40,92-118:
    logaddexp transforms, logsumexp normalisation, log-domain marginals): QSC received words and
    random log-domain rows incl. -inf entries; info decisions and every leaf marginal."""
    QMD, QPED, QMVD = R["QMD"], R["QPED"], R["QMVD"]
    cls = QMVD.QaryMemorylessVectorDistribution
    orig = cls.calcMarginalizedProbabilities
    out, meta = {}, []
    rs = np.random.default_rng(31)
    cq = np.load(os.path.join(OUT, "construct_qary.npz"))
    for name, q, n, p, T in (("q4_n6", 4, 6, 0.11, 40), ("q3_n5", 3, 5, 0.2, 40), ("q2_n4", 2, 4, 0.11, 24),
                             ("q4_n5_good", 4, 5, 0.11, 40)):
        N = 1 << n
        if name.endswith("_good"):  # the reference construction's frozen set (qsc4_n5_L64, K=16)
            frozen = set(int(i) for i in np.nonzero(cq["qsc4_n5_L64_frozen"])[0])
        else:
            frozen = set(int(i) for i in rs.permutation(N)[:N // 2])
        dec = QPED.QaryPolarEncoderDecoder(q, N, frozen, 1, use_log=True)
        qsc = QMD.makeQSC(q, p)
        xd = QMD.QaryMemorylessDistribution(q)
        xd.probs = [qsc.calcXMarginals()]
        xvd = xd.makeQaryMemorylessVectorDistribution(N, None, use_log=True)
        y = rs.integers(0, q, size=(T, N))
        xr = np.log(rs.random((T, N, q)))
        xr[rs.random((T, N, q)) < 0.05] = -np.inf
        xr[0, 0, :] = -np.inf
        rows = [("chan", None), ("rand", xr)]
        for kind, data in rows:
            info = np.zeros((T, dec.k), np.uint8)
            leaves = np.zeros((T, N, q))
            xy_in = np.zeros((T, N, q))
            for t in range(T):
                if data is None:
                    vd = qsc.makeQaryMemorylessVectorDistribution(N, [int(v) for v in y[t]], use_log=True)
                else:
                    vd = cls(q, N, use_log=True)
                    vd.probs[:] = data[t]
                xy_in[t] = vd.probs
                rec = []

                def wrapped(self, _rec=rec):
                    m = orig(self)
                    _rec.append(np.array(m, np.float64))
                    return m
                cls.calcMarginalizedProbabilities = wrapped
                try:
                    info[t] = dec.decode(xvd, vd)
                finally:
                    cls.calcMarginalizedProbabilities = orig
                ii = [i for i in range(N) if i not in frozen]
                assert len(rec) == len(ii)
                for j, i in enumerate(ii):
                    leaves[t, i] = rec[j]
            out["%s_%s_xy" % (name, kind)] = xy_in
            out["%s_%s_info" % (name, kind)] = info
            out["%s_%s_leaf" % (name, kind)] = leaves
        out[name + "_frozen"] = np.array([1 if i in frozen else 0 for i in range(N)], np.uint8)
        meta.append(dict(name=name, q=q, n=n, p=p, trials=T))
    save("qary_log", dict(sets=meta, note="leaf = log marginal at information leaves (0 elsewhere)"), **out)


def _aux_groups(aux, n):
    """auxiliary (one set of input-letter indices per output letter) -> group[n], -1 = dropped"""
    g = np.full(n, -1, np.int64)
    for j, sset in enumerate(aux):
        for i in sset:
            assert g[i] == -1
            g[i] = j
    return g


FIXTURES = {
    "bsc_n64": fx_bsc_n64,
    "awgn_n1024": lambda R, t: fx_awgn(R, t, 10, 64, 2.0, 20250204, "awgn_n1024", "C2"),
    "awgn_n4096": lambda R, t: fx_awgn(R, t, 12, 12, 2.0, 4096, "awgn_n4096", "C3"),
    "awgn_n256_lowsnr": lambda R, t: fx_awgn(R, t, 8, 64, 0.0, 256, "awgn_n256_lowsnr", "low-SNR"),
    "edge_binary": fx_edge,
    "prior_n64": fx_prior,
    "encode_binary": fx_encode,
    "qsc_q4_n256": fx_qsc,
    "harness_bsc_n64": fx_harness,
    "harness_verbose": fx_harness_verbose,
    "deletion_n8": fx_deletion,
    "deletion_edge": fx_deletion_edge,
    "genie_bsc_n64": fx_genie_bsc,
    "main_deletion_n8": fx_main_deletion,
    "construct_bin": fx_construct_bin,
    "test2_run": fx_test2,
    "construct_qary": fx_construct_qary,
    "qary_harness": fx_qary_harness,
    "qary_log": fx_qary_log,
    "construct_qary_up": fx_construct_qary_up,
    "combine_codes": fx_combine_codes,
    "scl": fx_scl,
}



HARNESSES = ("test.py", "test2.py", "test3.py", "main_deletion.py", "combine_codes.py")


def _harness_module_attrs(path):
    """{reference module: sorted attribute names} that a harness script binds: `import M` /
    `from P import M` aliases followed by `M.attr`, and `from M import name` (an AST scan of the
    harness text; nothing is executed)."""
    import ast
    tree = ast.parse(open(path).read())
    alias = {}
    out = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                alias[a.asname or a.name] = a.name
        elif isinstance(node, ast.ImportFrom) and node.module:
            for a in node.names:
                full = node.module + "." + a.name
                if os.path.exists(os.path.join(REF, *full.split(".")) + ".py"):
                    alias[a.asname or a.name] = full  # a reference module imported from its package
                elif os.path.exists(os.path.join(REF, *node.module.split(".")) + ".py"):
                    out.setdefault(node.module, set()).add(a.name)  # a name imported from a module
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in alias:
            mod = alias[node.value.id]
            if os.path.exists(os.path.join(REF, *mod.split(".")) + ".py"):
                out.setdefault(mod, set()).add(node.attr)
    return {m: sorted(v) for m, v in sorted(out.items())}


def _outcome(fn):
    import contextlib
    import io
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            r = fn()
        return {"ok": True, "value": r, "stdout": buf.getvalue()}
    except Exception as e:  # the reference's own failure modes are part of its behaviour
        return {"ok": False, "error": type(e).__name__, "message": str(e), "stdout": buf.getvalue()}


def fx_harness_names(R, timing):
    """Which module attributes the reference harnesses bind (test.py, test2.py, test3.py,
    main_deletion.py, combine_codes.py; an AST scan), whether the reference module defines each
    one, and the observed behaviour of the entry points whose reference behaviour is a stub or a
    failure (makeAWGN, encodeListDecodeSimulation, the q-ary genie) plus a few
    small helper values (the binary upgrade split, the q-ary cost bounds, makeQuantizedUniform)."""
    import importlib
    QMD, QPED, BMD = R["QMD"], R["QPED"], R["BMD"]
    names = {}
    for h in HARNESSES:
        mods = _harness_module_attrs(os.path.join(REF, h))
        names[h] = {}
        for mod, attrs in mods.items():
            m = importlib.import_module(mod)
            names[h][mod] = {a: hasattr(m, a) for a in attrs}
    beh = {}
    beh["makeAWGN_q2"] = _outcome(lambda: {"q": QMD.makeAWGN(2, 1.0, 0.5).q, "probs": QMD.makeAWGN(2, 1.0, 0.5).probs})
    beh["makeAWGN_q3"] = _outcome(lambda: QMD.makeAWGN(3, 1.0, 0.5))
    qsc = QMD.makeQSC(2, 0.05)

    def make_x(qsc=qsc):
        xd = QMD.QaryMemorylessDistribution(2)
        xd.probs = [qsc.calcXMarginals()]
        return xd.makeQaryMemorylessVectorDistribution(8, None)

    def make_xy(rx, qsc=qsc):
        return qsc.makeQaryMemorylessVectorDistribution(len(rx), rx)

    random.seed(5)
    np.random.seed(5)
    beh["encodeListDecodeSimulation"] = _outcome(lambda: QPED.encodeListDecodeSimulation(
        2, 8, make_x, lambda e: e, _qsc_channel_closure(qsc), make_xy, 3, {0, 1, 2, 4}, 2, 1))
    beh["qary_genieEncodeDecodeSimulation"] = _outcome(lambda: QPED.genieEncodeDecodeSimulation(
        8, make_x, lambda e: e, _qsc_channel_closure(qsc), make_xy, 2, 0.1, 7))
    beh["normalize"] = _outcome(lambda: [np.asarray(QPED.normalize(np.array([0.5, 2.0, 1.0]))[0]).tolist(),
                                         float(QPED.normalize(np.array([0.5, 2.0, 1.0]))[1])])
    beh["normalize_log"] = _outcome(lambda: [np.asarray(QPED.normalize(np.array([-3.0, -1.0]), True)[0]).tolist(),
                                             float(QPED.normalize(np.array([-3.0, -1.0]), True)[1])])
    beh["makeQuantizedUniform_3_4"] = _outcome(lambda: QMD.makeQuantizedUniform(3, 4).probs)
    beh["cost_bounds"] = _outcome(lambda: [QMD.degrade_cost_lower_bound(q, L) for q in (2, 3, 4) for L in (16, 100)]
                                  + [QMD.upgrade_cost_lower_bound(q, L) for q in (2, 3, 4) for L in (16, 100)]
                                  + [QMD.degrade_dynamic_upper_bound(q, L) for q in (2, 3, 4) for L in (16, 100)]
                                  + [QMD.upgrade_dynamic_upper_bound(q, L) for q in (2, 3, 4) for L in (16, 100)])
    rng = np.random.default_rng(9)
    splits = []
    for _ in range(40):
        # three letters ordered by posterior P(x=0|y), left > centre > right (the upgrade's order)
        post = sorted(rng.uniform(0.01, 0.99, 3), reverse=True)
        pis = rng.uniform(0.05, 1.0, 3)
        data = [([pis[i] * post[i], pis[i] * (1.0 - post[i])],) for i in range(3)]
        left, right = BMD.upgradedLeftRightProbs(*data)
        splits.append({"in": [d[0] for d in data], "left": left, "right": right,
                       "key_up": BMD._calcKey_upgrade(*data), "key_deg": BMD._calcKey_degrade(data[0], data[1])})
    beh["binary_upgrade_split"] = {"ok": True, "value": splits}
    beh["binary_use_fast"] = {"ok": True, "value": BMD.use_fast}
    with open(os.path.join(OUT, "harness_names.json"), "w") as f:
        json.dump({"note": "written by oracle/make_golden.py fx_harness_names from an AST scan of the reference "
                           "harnesses and calls into the reference modules",
                   "names": names, "behaviour": beh}, f, indent=1, sort_keys=True, default=str)
    print("  harness names:", sum(len(v) for h in names.values() for v in h.values()), "bindings")


def fx_test3_body(R, timing):
    """The body of test3.test() (test3.py:118-150) with its getFrozenSet call repaired: the
    reference passes upperBoundOnErrorProbability and numInfoIndices positionally into the
    snr / rate slots of getFrozenSet (test3.py:130 vs :81), so the construction is called with
    no bound and frozenSetFromTVAndPe compares a float with None (TypeError).  Here the frozen set
    comes from calcFrozenSet_degradingUpgrading(n=8, L=100, None, QSC(q, 0.99), bound 0.1) and the
    reference's encodeDecodeSimulation runs with test3.py's own closures (:21-70) and a seeded
    global channel RNG (test3.py:43 is unseeded); records the frozen set and the printed line."""
    import contextlib
    import io
    import tempfile
    sys.path.insert(0, REF)
    import test3 as T3
    QMD, QPED = R["QMD"], R["QPED"]
    runs, arrays = [], {}
    for q in (2,):
        p, L, n, N, bound, trials, seed = 0.99, 100, 8, 256, 0.1, 200, 31
        xy = QMD.makeQSC(q, p)
        t0 = time.time()
        with tempfile.TemporaryDirectory() as d:
            frozen = QMD.calcFrozenSet_degradingUpgrading(n, L, None, xy, d + "/", bound, None, False)
        timing["test3_body_q%d_construction_s" % q] = time.time() - t0
        random.seed(seed)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            QPED.encodeDecodeSimulation(q, N, T3.make_xVectorDistribution_fromQaryMemorylessDistribution(q, xy, N),
                                        T3.make_codeword_noprocessing,
                                        T3.simulateChannel_fromQaryMemorylessDistribution(xy),
                                        T3.make_xyVectorDistribution_fromQaryMemorylessDistribution(xy),
                                        trials, frozen)
        line = buf.getvalue().strip().splitlines()[-1]
        print("  test3 body q=%d: %s" % (q, line))
        mask = np.zeros(N, np.uint8)
        mask[sorted(frozen)] = 1
        arrays["q%d_frozen" % q] = mask
        runs.append(dict(q=q, p=p, L=L, n=n, bound=bound, trials=trials, global_seed=seed, line=line,
                         K=int(N - mask.sum())))
    save("test3_body", dict(runs=runs), **arrays)


FIXTURES["harness_names"] = fx_harness_names
FIXTURES["test3_body"] = fx_test3_body


def fx_deletion_genie_wide(R, timing):
    """The reference's genie construction (genieEncodeDecodeSimulation, BinaryPolarEncoderDecoder.py:390-491)
    over the deletion channel at shapes past 64 trellises and with guard-band ones
    (main_deletion.py:122-133 closures, trustXYProbs = n > n0): main_deletion's own default n0 = n//3
    at n = 10 (128 trellises), n0 = 1 at n = 8 / 9 (128 / 256 trellises), and ones = 1, 2, 3.
    Records the TV + Pe score vector handed to frozenSetFromTVAndPe and the returned frozen set;
    plus the reference main_deletion.py itself at -n 10 -g 6 -e 4 (runpy), its printed lines."""
    import contextlib
    import io
    import runpy
    BPED = R["BPED"]
    cases = [(10, 3, 0.1, 0, 6), (8, 1, 0.1, 0, 8), (9, 1, 0.05, 0, 4), (8, 2, 0.1, 1, 8), (9, 1, 0.1, 2, 3),
             (7, 1, 0.2, 3, 8)]
    out = {}
    for ci, (n, n0, pd, ones, G) in enumerate(cases):
        N = 1 << n
        make_x, make_codeword, channel, make_xy = deletion_closures(R, n, n0, pd, 0.1, ones, 100 + ci)
        cap = {}
        orig = BPED.frozenSetFromTVAndPe

        def capture(TV, Pe, bound, _orig=orig):
            cap["score"] = [float(a) + float(b) for a, b in zip(TV, Pe)]
            return _orig(TV, Pe, bound)

        BPED.frozenSetFromTVAndPe = capture
        t0 = time.time()
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                frozen = BPED.genieEncodeDecodeSimulation(N, make_x, make_codeword, channel, make_xy, G, 0.1,
                                                          genieSeed=300 + ci, trustXYProbs=n <= n0, filename=None)
        finally:
            BPED.frozenSetFromTVAndPe = orig
        print("  genie n=%d n0=%d ones=%d: %d trials, %.1f s" % (n, n0, ones, G, time.time() - t0))
        out["c%d_score" % ci] = np.array(cap["score"])
        out["c%d_frozen" % ci] = np.array([1 if i in frozen else 0 for i in range(N)], np.uint8)
        out["c%d_shape" % ci] = np.array([n, n0, ones, G], np.int32)
        out["c%d_pd" % ci] = np.array([pd])
    argv = ["main_deletion.py", "-n", "10", "-g", "6", "-e", "4"]
    old = sys.argv
    sys.argv = argv
    buf = io.StringIO()
    t0 = time.time()
    try:
        with contextlib.redirect_stdout(buf):
            runpy.run_path(os.path.join(REF, "main_deletion.py"), run_name="__main__")
    finally:
        sys.argv = old
    print("  main_deletion -n 10: %.1f s" % (time.time() - t0))
    lines = buf.getvalue().strip().splitlines()
    keep = [l for l in lines if not l.startswith(("TVVec", "pevec", "HEncvec", "HDecvec"))]
    save("deletion_genie_wide", dict(cases=len(cases), xi=0.1, channel_seed="100 + case", genie_seed="300 + case",
                                     bound=0.1, note="(n, n0, ones, trials) per case", main_argv=argv[1:],
                                     main_lines=keep), **out)


FIXTURES["deletion_genie_wide"] = fx_deletion_genie_wide
FIXTURES["scl_log"] = lambda R, t: fx_scl(R, t, use_log=True)


# ---------------------------------------------------------------------------
# edge families at the BASELINE code lengths (N = 1024, 4096)
# ---------------------------------------------------------------------------

EDGE_LONG_FAMILIES = ("discrete", "subnormal", "random", "one_sided_zeros", "ties", "underflow",
                      "awgn_2db", "awgn_2db_subnormal_scale", "awgn_high_snr", "awgn_mixed_defects")


def _awgn_table(sigma2, levels, scale=1.0):
    """256-letter quantised BI-AWGN output alphabet: the joint P(x, y) rows at the level centres."""
    c = 0.5 / math.sqrt(2.0 * math.pi * sigma2)
    p0 = c * np.exp(-((levels - 1.0) ** 2) / (2.0 * sigma2))
    p1 = c * np.exp(-((levels + 1.0) ** 2) / (2.0 * sigma2))
    return np.stack([p0, p1], axis=-1) * scale


def _edge_long_inputs(family, N, B, x, rng):
    """(table [256][2] f64, idx [B][N] u8) for one edge family; xy = table[idx].  x [B][N] is a
    codeword batch of the case's code (used by the channel-like families)."""
    vals = np.array([0.0, 0.5, 0.25, 1.0, 0.125, 1e-300, 4.9e-324, 2.2e-308, 0.3, 0.7, 1e-5])
    idx = rng.integers(0, 256, size=(B, N)).astype(np.uint8)
    levels = np.linspace(-5.0, 5.0, 256)

    def channel_idx(sigma2):
        s = 1.0 - 2.0 * x.astype(np.float64)
        y = s + math.sqrt(sigma2) * rng.standard_normal(x.shape)
        return np.clip(np.rint((y + 5.0) * 25.5), 0, 255).astype(np.uint8)

    if family == "discrete":        # a few discrete levels: many ties and zeros
        table = rng.choice(vals[:5], size=(256, 2))
    elif family == "subnormal":     # subnormal / tiny magnitudes
        table = rng.choice(vals, size=(256, 2))
    elif family == "random":
        table = rng.random((256, 2))
    elif family == "one_sided_zeros":
        table = rng.random((256, 2))
        z = rng.random(256) < 0.3
        side = rng.integers(0, 2, size=256)
        table[z, 0] *= side[z]
        table[z, 1] *= 1 - side[z]
    elif family == "ties":
        table = np.repeat(rng.choice(vals[:5], size=(256, 1)), 2, axis=1)
        flip = rng.random(256) < 0.3
        table[flip, 1] = rng.random(int(flip.sum()))
    elif family == "underflow":     # products underflow deep in the tree
        table = rng.random((256, 2)) * 1e-120
    elif family == "awgn_2db":      # the C2/C3 channel: the rate-1 shortcut's common case
        table = _awgn_table(0.630957, levels)
        idx = channel_idx(0.630957)
    elif family == "awgn_2db_subnormal_scale":  # root products subnormal (scale 1e-160)
        table = _awgn_table(0.630957, levels, 1e-160)
        idx = channel_idx(0.630957)
    elif family == "awgn_high_snr":  # |LLR| up to ~200 at the levels: ratios underflow to subnormals / 0
        table = _awgn_table(0.05, levels)
        idx = channel_idx(0.05)
    else:                           # awgn_mixed_defects: 2 dB rows with 1 % subnormal / tie / zero letters
        table = _awgn_table(0.630957, levels)
        table[0] = (4.9e-324, 0.0)
        table[1] = (0.0, 4.9e-324)
        table[2] = (0.0, 0.0)
        table[3] = (0.25, 0.25)
        table[4] = (1e-300, 2.2e-308)
        table[5] = (1.0, 1e-310)
        idx = channel_idx(0.630957)
        bad = rng.random((B, N)) < 0.01
        idx[bad] = rng.integers(0, 6, size=int(bad.sum()))
    return np.ascontiguousarray(table, np.float64), idx


def _edge_long_case(args):
    """One (N, frozen kind, family) case, decoded by the reference in a worker process."""
    n, fkind, fam_i, B, seed = args
    R = _EDGE_R
    BPED, BMVD = R["BPED"], R["BMVD"]
    N = 1 << n
    rng = np.random.default_rng(seed)
    if fkind == "bhattacharyya":   # the C2 / C3 code: K = N/2 at 2 dB
        frozen, _ = bhattacharyya_frozen(n, N // 2, 0.630957)
    else:
        frozen = set(int(i) for i in np.nonzero(rng.random(N) < 0.5)[0])
    crs = int(rng.integers(-1, 50))
    enc = BPED.BinaryPolarEncoderDecoder(N, frozen, crs)
    u = rng.integers(0, 2, size=(B, enc.k)).astype(np.uint8)
    x = np.stack([ref_encode(R, N, enc, u[b]) for b in range(B)])
    table, idx = _edge_long_inputs(EDGE_LONG_FAMILIES[fam_i], N, B, x, rng)
    xvd = BMVD.BinaryMemorylessVectorDistribution(N)
    xvd.probs[:] = np.array([0.5, 0.5])
    info = np.zeros((B, enc.k), np.uint8)
    xhat = np.zeros((B, N), np.uint8)
    for b in range(B):
        xyvd = BMVD.BinaryMemorylessVectorDistribution(N)
        xyvd.probs[:] = table[idx[b]]
        xh, inf = enc.decode(xvd, xyvd)
        info[b] = inf
        xhat[b] = xh
    mask, r, fval = frozen_arrays(enc, N)
    return dict(n=n, family=fam_i, crs=crs, table=table, idx=idx, frozen=mask, fval=fval,
                info_bits=np.packbits(info, axis=1), xhat_bits=np.packbits(xhat, axis=1), K=enc.k)


_EDGE_R = None


def fx_edge_long(R, timing):
    """The six edge families of fx_edge (discrete, subnormal, random, one-sided zeros, ties,
    underflow) plus four channel-shaped ones (quantised BI-AWGN at 2 dB, the same scaled by 1e-160,
    a high-SNR channel whose ratios underflow, 2 dB with 1 % defect letters) at N = 1024 and 4096,
    with the C2 / C3 Bhattacharyya frozen sets and random frozen sets, decoded by the reference
    (BinaryPolarEncoderDecoder.decode, :71-99).  Inputs are stored as a 256-letter table and u8
    letter indices (xy = table[idx]); decisions bit-packed along the codeword (np.packbits)."""
    import multiprocessing as mp
    global _EDGE_R
    _EDGE_R = R
    jobs = []
    for n, B in ((10, 32), (12, 16)):
        for fk in ("bhattacharyya", "random"):
            for fi in range(len(EDGE_LONG_FAMILIES)):
                jobs.append((n, fk, fi, B, 9000 + 100 * n + 10 * fi + (fk == "random")))
    t0 = time.time()
    with mp.get_context("fork").Pool(8) as pool:
        cases = pool.map(_edge_long_case, jobs, chunksize=1)
    timing["edge_long_wall_s_8proc"] = time.time() - t0
    arrays = {}
    for i, c in enumerate(cases):
        for k, v in c.items():
            arrays["c%d_%s" % (i, k)] = np.asarray(v)
    save("edge_long", dict(cases=len(cases), families=list(EDGE_LONG_FAMILIES),
                           frozen_kinds=["bhattacharyya (2 dB, K = N/2)", "random 50 %"],
                           note="xy = table[idx]; info / xhat np.packbits(axis=1); seeds 9000 + 100 n + 10 family "
                                "+ (random frozen)"), **arrays)


FIXTURES["edge_long"] = fx_edge_long


# ---------------------------------------------------------------------------
# the shapes the wave-per-task deletion kernels serve (n0 = 4 at n >= 10, n0 = 5)
# ---------------------------------------------------------------------------

def ref_deletion_words(R, n, n0, pds, xi, ones, frozen, crs, info_seed, channel_seed):
    """Received words only: the reference's encode -> guard bands -> deletionChannelSimulation, word t at
    deletion rate pds[t].  The information of word t is the one ref_deletion_trials draws for its
    word t from the same info_seed, so a later rx_override run keeps tx_info aligned with the words."""
    BPED = R["BPED"]
    make_x, make_codeword, _, _ = deletion_closures(R, n, n0, pds[0], xi, ones, channel_seed)
    channels = {pd: deletion_closures(R, n, n0, pd, xi, ones, channel_seed + k)[2]
                for k, pd in enumerate(sorted(set(pds)))}
    xvd = make_x()
    enc = BPED.BinaryPolarEncoderDecoder(1 << n, frozen, crs)
    irng = random.Random()
    irng.seed(info_seed)
    words = []
    for pd in pds:
        inf = [0 if irng.random() < 0.5 else 1 for _ in range(enc.k)]
        cw = make_codeword(enc.encode(xvd, inf))
        words.append([int(b) for b in channels[pd](cw)])
    return words, len(cw)


# (n, n0, pd, words in total, words whose leaf marginals are stored, frozen set).  Frozen set "half":
# rate about 1/2 at random; at that rate the reference's decode of a channel word goes wrong early and
# most of its later leaves are ties, so each shape of a kernel also has a "low" case: rate 1/16 on the
# positions of largest index weight (the Reed-Muller rule), which the reference decodes correctly, every
# leaf live to the end.
DELETION_WAVE_CASES = [(6, 5, 0.1, 8, 8, "half"), (6, 5, 0.25, 8, 8, "half"), (7, 5, 0.1, 8, 8, "half"),
                       (7, 5, 0.25, 8, 8, "half"), (10, 4, 0.1, 8, 8, "half"), (11, 5, 0.1, 8, 8, "half"),
                       (12, 4, 0.25, 8, 2, "half"), (13, 4, 0.1, 5, 2, "half"), (14, 4, 0.1, 4, 0, "half"),
                       (13, 5, 0.2, 4, 0, "half"), (15, 5, 0.1, 3, 0, "half"),
                       (10, 4, 0.05, 8, 8, "low"), (11, 5, 0.05, 8, 4, "low"), (12, 4, 0.1, 5, 1, "low"),
                       (13, 4, 0.05, 4, 1, "low"), (14, 4, 0.05, 3, 0, "low"), (13, 5, 0.1, 3, 0, "low"),
                       (15, 5, 0.05, 3, 0, "low")]


def fx_deletion_wave(R, timing):
    """The shapes of the wave-per-task deletion kernels (16-input trellises at n = 10, 12, 13, 14 and
    32-input trellises at n = 6, 7, 11, 13, 15; ones = 0, xi = 0.1): channel words at the case's pd, one
    channel word drawn at pd 0.4 (segments from empty to overlong), the empty word, an all-zero word
    of half the codeword length and a random word 1.5 x the codeword length (every segment past
    2^n0), each decoded by the reference at the case's pd.  Frozen sets: the first quarter frozen
    (rate-0 nodes down to depth 2), then a third of the rest at random, so the rate is about 1/2
    ("half"), or all but the N / 16 positions of largest index weight ("low", see
    DELETION_WAVE_CASES); crs >= 0, so the frozen values are mixed."""
    import trellis_oracle as tro
    rng = np.random.default_rng(4511)
    out = {}
    for ci, (n, n0, pd, T, nleaf, kind) in enumerate(DELETION_WAVE_CASES):
        N = 1 << n
        mask = rng.random(N) < 1.0 / 3.0
        if kind == "low":
            mask[:] = True
            mask[sorted(range(N // 4, N), key=lambda i: (bin(i).count("1"), i))[-(N // 16):]] = False
        mask[: N // 4] = True
        frozen = set(int(i) for i in np.nonzero(mask)[0])
        crs = int(rng.integers(0, 500))
        info_seed, channel_seed = int(rng.integers(1, 999)), int(rng.integers(1, 999))
        # 8 words: 4 at pd, 1 at 0.4, empty, zeros, overlong; 5: 2, 1, empty, overlong;
        # 4: 1, 1, empty, overlong; 3: 1 at pd, empty, overlong
        nch = {8: 5, 5: 3, 4: 2, 3: 1}[T]
        pds = [pd] * (nch - 1) + [0.4] if nch > 1 else [pd]
        t0 = time.perf_counter()
        words, cwl = ref_deletion_words(R, n, n0, pds, 0.1, 0, frozen, crs, info_seed, channel_seed)
        words.append([])
        if T == 8:
            words.append([0] * (cwl // 2))
        words.append([int(b) for b in rng.integers(0, 2, cwl + cwl // 2)])
        assert len(words) == T
        d, _ = ref_deletion_trials(R, n, n0, pd, 0.1, 0, frozen, crs, info_seed, channel_seed, T, rx_override=words)
        dt = (time.perf_counter() - t0) / T
        timing["deletion_wave_n%d_n0%d_pd%g_s_per_cw" % (n, n0, pd)] = dt
        # conditions that keep the case from being vacuous
        K = d["info"].shape[1]
        assert K > 0, (n, n0)
        assert any(not np.array_equal(d["info"][t], d["info"][u]) for t in range(nch) for u in range(T)), (n, n0)
        seglens = set(len(s) for w in words for s in tro.remove_guard_bands(w, n, n0))
        if kind == "low":  # a live decode: a channel word at the case's pd is decoded correctly
            assert any(np.array_equal(d["info"][t], d["tx_info"][t]) for t in range(max(1, nch - 1))), (n, n0)
        if T >= 5:
            assert 0 in seglens and any(1 <= l <= 1 << n0 for l in seglens) and max(seglens) > 1 << n0, (n, n0)
        print("  (%d, %d) pd %g %s: K %d, %d words, %.1f s a word, segment lengths %d..%d, words decoded correctly %s"
              % (n, n0, pd, kind, K, T, dt, min(seglens), max(seglens),
                 [t for t in range(T) if np.array_equal(d["info"][t], d["tx_info"][t])]))
        d.pop("cw_len")
        d.pop("r")  # N doubles a case: fval is what the decoders take, and crs regenerates r
        d["crs"] = np.array([crs], np.int32)
        # the marginals at the information leaves only (what the tests compare), first words only
        d["leaf_mi"] = np.ascontiguousarray(d.pop("leaf_m")[:nleaf][:, d["frozen"] == 0])
        for k, v in d.items():
            out["c%d_%s" % (ci, k)] = v
        out["c%d_shape" % ci] = np.array([n, n0, 0, nch, kind == "low"], np.int32)
        out["c%d_pd" % ci] = np.array([pd])
    save("deletion_wave", dict(cases=len(DELETION_WAVE_CASES), xi=0.1,
                               note="shape = (n, n0, ones, channel words, low-rate frozen set); the last channel word of a case "
                                    "with two or more is drawn at pd 0.4; then the empty word, (8-word cases) "
                                    "zeros of half the codeword length, a random word 1.5 x the codeword "
                                    "length; leaf_mi holds the marginals at the information leaves of the first words"), **out)
    size = os.path.getsize(os.path.join(OUT, "deletion_wave.npz"))
    assert size <= 1 << 20, "deletion_wave.npz is %d bytes: store fewer leaf_m words" % size


FIXTURES["deletion_wave"] = fx_deletion_wave


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    R = load_reference()
    tpath = os.path.join(OUT, "ref_timing.json")
    timing = json.load(open(tpath)) if os.path.exists(tpath) else {}
    for name, fn in FIXTURES.items():
        if args.only and name not in args.only:
            continue
        t0 = time.time()
        fn(R, timing)
        print("  %s: %.1f s" % (name, time.time() - t0))
    timing["host"] = "build container, 1 thread, shimmed reference Python (decode only)"
    os.makedirs(OUT, exist_ok=True)
    with open(tpath, "w") as f:
        json.dump(timing, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
