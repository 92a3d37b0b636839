#!/usr/bin/env python3
"""The memoryless genie construction as one device pipeline (the breadth-first kernel with in-kernel
counting) against the composed route through the export decode, and the host facade.

    python scripts/ab_genie_bin.py [--n 10 --n 12 ...] [--trials T] [--host-trials H] [--reps R]
                                   [--ebn0 2.0] [--rate 0.5] [--blocks]

For each length, on one GPU, BI-AWGN at the given Eb/N0 and rate (construction.awgn_sigma2), device
events, one warm-up and R timed calls (median, min, max):
  * mc.run_genie_bin (pcub_mc_genie_bin) over `trials` trials at its default chunk;
  * its stages alone over one chunk on preallocated buffers: generate (pcub_mc_info +
    pcub_polar_encode_bin + pcub_mc_channel_norm_tiled, compact, tile = 1), the same generate with
    tile = 0 (what per-trial rows cost the generator), and the kernel (pcub_sc_genie_bin);
  * the composed route to the same counters at the same chunk, chunk by chunk: the same info and
    encode, pcub_mc_channel_norm (pairs), pcub_sc_leaf_bin with every position frozen to u,
    pcub_genie_count -- through the existing wrappers' entries; its counters must equal the
    pipeline's;
  * with --blocks, the kernel at 64, 256 and 1024 work items a workgroup;
  * coding.genieEncodeDecodeSimulation (trustXYProbs = False) with host closures over `host-trials`
    trials on the wall clock, for context.
Prints one JSON line a length, with the kernel's achieved fraction of the fp64 vector and HBM
ceilings (157.3 TFLOP/s counted as 78.6 T multiply-adds/s, 8 TB/s; the kernel is counted at two
divisions of ~12 fp64 operations and ~10 more a pair, an estimate).
"""
import argparse
import contextlib
import io
import json
import math
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from polarcub_amd import _lib, coding, construction, mc, sc, vectors  # noqa: E402

FP64_OPS_S = 78.6e12  # fp64 vector instructions x lanes a second (FMA counted once)
HBM_B_S = 8.0e12
OPS_A_PAIR = 34      # f: product, two sums, compare / select, division (~12); g: product or division


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def stats(secs, trials):
    r = [trials / s for s in secs]
    return dict(median_trials_s=statistics.median(r), min_trials_s=min(r), max_trials_s=max(r),
                seconds=[round(s, 6) for s in secs])


def repeat(fn, reps):
    timed(fn)  # warm-up
    return [timed(fn)[0] for _ in range(reps)]


class Stages:
    """One chunk's buffers and the entries on them."""

    def __init__(self, n, sigma2, seed, B):
        self.lib = _lib.lib()
        dev = torch.device("cuda:0")
        self.n, self.N, self.B, self.sigma2, self.seed = n, 1 << n, B, sigma2, seed
        N, nw = self.N, ((1 << n) + 31) // 32
        i32 = dict(dtype=torch.int32, device=dev)
        self.u, self.x = torch.empty((nw, B), **i32), torch.empty((nw, B), **i32)
        self.zeros = torch.zeros(nw, **i32)
        self.ones = torch.full((nw,), -1 if N >= 32 else (1 << N) - 1, **i32)
        self.rows = torch.empty((B, N), dtype=torch.float64, device=dev)
        self.pairs = torch.empty((N, B, 2), dtype=torch.float64, device=dev)
        self.leaf = torch.empty((N, B), dtype=torch.float64, device=dev)
        need = int(self.lib.pcub_sc_leaf_bin_workspace(B, n))
        self.lws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        self.counters = torch.zeros(1 + 2 * N, dtype=torch.int64, device=dev)

    def info_encode(self, offset, B):
        L, st = self.lib, sc._stream()
        _lib.check(L.pcub_mc_info(self.seed, offset, B, self.N, sc._p(self.u), st), "pcub_mc_info")
        _lib.check(L.pcub_polar_encode_bin(sc._p(self.u), B, self.n, sc._p(self.zeros), sc._p(self.zeros), self.N,
                                           sc._p(self.x), st), "pcub_polar_encode_bin")

    def generate(self, tile, offset=0, B=None):
        B = self.B if B is None else B
        self.info_encode(offset, B)
        _lib.check(self.lib.pcub_mc_channel_norm_tiled(self.seed, offset, B, self.n, 0, self.sigma2, sc._p(self.x),
                                                       sc._p(self.rows), 1, tile, sc._stream()),
                   "pcub_mc_channel_norm_tiled")

    def kernel(self, block=0):
        _lib.check(self.lib.pcub_sc_genie_bin_geom(sc._p(self.rows), 1, sc._p(self.u), self.B, self.n, block,
                                                   sc._p(self.counters), None, sc._stream()), "pcub_sc_genie_bin")

    def composed_chunk(self, offset, B):
        """The parent's route: the strides of u, pairs and leaf are B, so a short last chunk is its own
        batch on the same buffers."""
        L, st = self.lib, sc._stream()
        self.info_encode(offset, B)
        _lib.check(L.pcub_mc_channel_norm(self.seed, offset, B, self.n, 0, self.sigma2, sc._p(self.x),
                                          sc._p(self.pairs), 0, st), "pcub_mc_channel_norm")
        _lib.check(L.pcub_sc_leaf_bin(sc._p(self.pairs), B, self.n, sc._p(self.ones), None, sc._p(self.u), 0, None,
                                      None, sc._p(self.leaf), sc._p(self.lws), self.lws.numel(), st),
                   "pcub_sc_leaf_bin")
        _lib.check(L.pcub_genie_count(sc._p(self.leaf), sc._p(self.u), B, self.n, sc._p(self.counters), st),
                   "pcub_genie_count")

    def composed(self, trials):
        self.counters.zero_()
        for c0 in range(0, trials, self.B):
            self.composed_chunk(c0, min(self.B, trials - c0))
        return self.counters.cpu().numpy().copy()


def host_genie(n, sigma2, trials, seed):
    """coding.genieEncodeDecodeSimulation over BI-AWGN with host closures; its printout is dropped."""
    N = 1 << n
    rng = random.Random(100)
    sigma = math.sqrt(sigma2)

    def make_x():
        v = vectors.BinaryMemorylessVectorDistribution(N)
        v.probs[:] = 0.5
        return v

    def channel(codeword):
        return [(1.0 - 2.0 * int(b)) + sigma * rng.gauss(0.0, 1.0) for b in codeword]

    def make_xy(received):
        y = np.asarray(received)
        v = vectors.BinaryMemorylessVectorDistribution(N)
        c = 0.5 / math.sqrt(2.0 * math.pi * sigma2)
        v.probs[:, 0] = c * np.exp(-(y - 1.0) ** 2 / (2.0 * sigma2))
        v.probs[:, 1] = c * np.exp(-(y + 1.0) ** 2 / (2.0 * sigma2))
        return v

    with contextlib.redirect_stdout(io.StringIO()):
        return coding.genieEncodeDecodeSimulation(N, make_x, lambda e: e, channel, make_xy, trials, 0.1,
                                                  genieSeed=seed, trustXYProbs=False)


def run_length(n, trials, host_trials, reps, sigma2, seed, blocks):
    N = 1 << n
    chunk = int(min(trials, mc.genie_bin_default_chunk(n)))
    pipe = repeat(lambda: mc.run_genie_bin(n, mc.CHANNEL_AWGN, sigma2, seed, 0, trials, chunk=chunk), reps)
    t, wrong, tie = mc.run_genie_bin(n, mc.CHANNEL_AWGN, sigma2, seed, 0, trials, chunk=chunk)
    S = Stages(n, sigma2, seed, chunk)
    comp = repeat(lambda: S.composed(trials), reps)
    cc = S.composed(trials)
    same = bool(cc[0] == t and np.array_equal(cc[1:1 + N], wrong) and np.array_equal(cc[1 + N:], tie))
    gen1 = repeat(lambda: S.generate(1), reps)
    gen0 = repeat(lambda: S.generate(0), reps)
    S.generate(1)
    kern = repeat(lambda: S.kernel(0), reps)
    out = dict(n=n, N=N, trials=trials, chunk=chunk, reps=reps, sigma2=sigma2, counters_equal=same,
               pipeline=stats(pipe, trials), composed=stats(comp, trials),
               generate_tile1=stats(gen1, chunk), generate_tile0=stats(gen0, chunk), kernel=stats(kern, chunk),
               mean_pe=float(np.mean(coding.genie_pe_from_counts(t, wrong, tie))))
    out["speedup_over_composed"] = out["pipeline"]["median_trials_s"] / out["composed"]["median_trials_s"]
    k = out["kernel"]["median_trials_s"]
    out["kernel_fp64_fraction"] = k * (N // 2) * n * OPS_A_PAIR / FP64_OPS_S
    out["kernel_hbm_fraction"] = k * (8 * N + 4 * ((N + 31) // 32)) / HBM_B_S
    if blocks:
        out["kernel_by_block"] = {str(b): stats(repeat(lambda: S.kernel(b), reps), chunk)["median_trials_s"]
                                  for b in (64, 256, 1024)}
    if host_trials:
        host_genie(n, sigma2, min(4, host_trials), 300)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_genie(n, sigma2, host_trials, 300)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        out["host"] = dict(trials=host_trials, trials_s=host_trials / s, seconds=round(s, 6))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, action="append", default=None)
    ap.add_argument("--trials", type=int, default=1 << 18)
    ap.add_argument("--host-trials", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ebn0", type=float, default=2.0)
    ap.add_argument("--rate", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--blocks", action="store_true")
    a = ap.parse_args()
    sigma2 = construction.awgn_sigma2(a.ebn0, a.rate)
    for n in (a.n or [10, 12]):
        print(json.dumps(run_length(n, a.trials, a.host_trials, a.reps, sigma2, a.seed, a.blocks)), flush=True)


if __name__ == "__main__":
    main()
