#!/usr/bin/env python3
"""The IR Monte-Carlo as one device pipeline against the host loop around the list decoder.

    python scripts/ab_ir_pipeline.py [--shape q,n,L,trials,host_trials ...] [--reps R] [--p P]

For each shape, on one GPU:
  * mc.run_ir (pcub_mc_run_ir: prepare -> list decode -> classify, no host synchronisation) over
    `trials` trials, timed with device events after one warm-up call, R repeats (median, spread);
  * coding_qary.irSimulation on the same law (QSC(p) closures: random.Random channel, makeQSC's rows)
    over `host_trials` trials in one chunk, on the wall clock after one warm-up call;
  * the three stages of the pipeline alone through their own entries on preallocated buffers
    (pcub_ir_prepare, pcub_scl_qary, pcub_ir_classify over the same `trials` codewords), device
    events around each, median of R: their shares of the sum.
Frozen set: the K = N / 2 most reliable indices of construction.bhattacharyya_frozen(n, K, 0.5).
Prints one JSON line a shape.  Default shapes: q = 3 at (N 256, L 9), (N 1024, L 81), (N 1024, L 729).
"""
import argparse
import json
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

from polarcub_amd import _lib, coding_qary, construction, mc, sc, vectors  # noqa: E402

DEFAULT_SHAPES = [(3, 8, 9, 16384, 512), (3, 10, 81, 2048, 128), (3, 10, 729, 512, 64)]


def qsc_closures(q, N, p, chan_seed):
    chan = random.Random(chan_seed)

    def simulate(a):
        return [(x + chan.randrange(1, q)) % q if chan.random() < p else x for x in a]

    def make_xy(b):
        vd = vectors.QaryMemorylessVectorDistribution(q, N)
        for i, y in enumerate(b):
            vd.probs[i] = [1.0 - p if x == y else p / (q - 1) for x in range(q)]
        return vd
    return simulate, make_xy


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def stage_split(code, mask, seed, B, p, L, reps):
    """Seconds of pcub_ir_prepare, pcub_scl_qary and pcub_ir_classify over B codewords, each through
    its own entry on buffers allocated beforehand (median of reps after one warm-up round)."""
    lib = _lib.lib()
    dev, N, K, q = code.device, code.N, code.K, code.q
    nF = N - K
    u8 = dict(dtype=torch.uint8, device=dev)
    a, work = torch.empty((N, B), **u8), torch.empty((N, B), **u8)
    xy = torch.empty((N, B, q), dtype=torch.float64, device=dev)
    act, fv = torch.empty((max(1, K), B), **u8), torch.empty((max(1, nF), B), **u8)
    info = torch.empty((L, max(1, K), B), **u8)
    prob = torch.empty((L, B), dtype=torch.float64, device=dev)
    size = torch.empty(B, dtype=torch.int32, device=dev)
    ap = torch.empty(B, dtype=torch.float64, device=dev)
    counters = torch.zeros(10, dtype=torch.int64, device=dev)
    need = int(lib.pcub_scl_qary_workspace(B, q, code.n, L, K))
    block = int(lib.pcub_scl_qary_workspace(1, q, code.n, L, K))
    ws = torch.empty(min(need, max(block, torch.cuda.mem_get_info(dev)[0] // 2)), **u8)
    st = sc._stream()

    def prepare():
        _lib.check(lib.pcub_ir_prepare(seed, 0, B, code.n, q, p, 0, sc._p(code.frozen_dev), K, sc._p(a), sc._p(xy),
                                       sc._p(act), sc._p(fv), sc._p(work), st), "pcub_ir_prepare")

    def decode():
        _lib.check(lib.pcub_scl_qary(sc._p(xy), B, q, code.n, L, sc._p(code.frozen_dev), sc._p(fv), nF, sc._p(act), K,
                                     sc._p(info), sc._p(prob), sc._p(size), sc._p(ap), sc._p(ws), ws.numel(), st),
                   "pcub_scl_qary")

    def classify():
        _lib.check(lib.pcub_ir_classify(sc._p(info), sc._p(prob), sc._p(size), sc._p(ap), sc._p(act), B, L, K,
                                        sc._p(counters), None, st), "pcub_ir_classify")
    t = {"prepare": [], "list_decode": [], "classify": []}
    for it in range(reps + 1):
        for name, fn in (("prepare", prepare), ("list_decode", decode), ("classify", classify)):
            s, _ = timed(fn)
            if it:
                t[name].append(s)
    return {k: statistics.median(v) for k, v in t.items()}


def run_shape(q, n, L, trials, host_trials, p, reps, seed):
    N = 1 << n
    K = N // 2
    mask = construction.bhattacharyya_frozen(n, K, 0.5)
    code = sc.QaryCode(q, N, mask, device=torch.device("cuda:0"))
    frozen = np.nonzero(mask)[0].tolist()
    mc.run_ir(code, seed, 0, trials, p, L)  # warm-up
    secs, counters = [], None
    for _ in range(reps):
        s, counters = timed(lambda: mc.run_ir(code, seed, 0, trials, p, L))
        secs.append(s)
    rate = [trials / s for s in secs]
    # the host loop: one warm-up call (decoder construction, first launches), then the timed run
    simulate, make_xy = qsc_closures(q, N, p, 5)
    coding_qary.irSimulation(q, N, simulate, make_xy, min(8, host_trials), frozen, maxListSize=L)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hfe, _, _, _ = coding_qary.irSimulation(q, N, simulate, make_xy, host_trials, frozen, maxListSize=L,
                                            chunk=host_trials)
    torch.cuda.synchronize()
    host_s = time.perf_counter() - t0
    split = stage_split(code, mask, seed, trials, p, L, reps)
    total = sum(split.values())
    return dict(q=q, N=N, L=L, K=K, p=p, reps=reps,
                pipeline=dict(trials=trials, median_trials_s=statistics.median(rate), min_trials_s=min(rate),
                              max_trials_s=max(rate), seconds=[round(s, 6) for s in secs], counters=counters),
                host=dict(trials=host_trials, trials_s=host_trials / host_s, seconds=round(host_s, 6),
                          frame_error_prob=hfe),
                speedup=statistics.median(rate) / (host_trials / host_s),
                split_seconds={k: round(v, 6) for k, v in split.items()},
                split_share={k: round(v / total, 5) for k, v in split.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None, help="q,n,L,trials,host_trials (repeatable)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=20251020)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else DEFAULT_SHAPES
    for q, n, L, trials, host_trials in shapes:
        print(json.dumps(run_shape(q, n, L, trials, host_trials, a.p, a.reps, a.seed)), flush=True)


if __name__ == "__main__":
    main()
