#!/usr/bin/env python3
"""The deletion channel's genie construction as one device pipeline against the host loop around the
export decode.

    python scripts/ab_genie_pipeline.py [--shape n,n0,trials,host_trials ...] [--reps R] [--pd P] [--xi X]

For each shape, on one GPU:
  * mc.run_genie_deletion (pcub_mc_genie_deletion: info -> encode -> guard bands + channel -> export
    decode -> count, no host synchronisation) over `trials` trials, timed with device events after one
    warm-up call, R repeats (median, spread);
  * coding.genieEncodeDecodeSimulation with main_deletion's closures (trustXYProbs = False) over
    `host_trials` trials on the wall clock after one warm-up call of a few trials: the parent path
    (MT19937 draws, guard bands and channel as Python closures, padded upload, export decode on the
    device, marginals downloaded, _genie_stats and the accumulation in Python);
  * the stages of one chunk alone through their own entries on preallocated buffers (generate:
    pcub_mc_info + pcub_polar_encode_bin + pcub_mc_deletion; export decode: pcub_sc_leaf_deletion;
    count: pcub_genie_count, over min(trials, the default chunk) trials), device events around each,
    median of R: their shares of the sum.
Prints one JSON line a shape.  Default shapes: (n, n0) = (10, 3), (13, 4), (14, 4).
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from polarcub_amd import _lib, coding, mc, sc  # noqa: E402
from polarcub_amd.cli import main_deletion  # noqa: E402

DEFAULT_SHAPES = [(10, 3, 8000, 1024), (13, 4, 4096, 256), (14, 4, 4096, 128)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def stage_split(n, n0, xi, pd, seed, B, reps):
    """Seconds of the generators, pcub_sc_leaf_deletion and pcub_genie_count over B trials, each through
    its own entry on buffers allocated beforehand (median of reps after one warm-up round)."""
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    N = 1 << n
    nw = (N + 31) // 32
    t = mc.guard_template(n, n0, xi, 0, dev)
    W = int(t.numel())
    i32 = dict(dtype=torch.int32, device=dev)
    u, x = torch.empty((nw, B), **i32), torch.empty((nw, B), **i32)
    rx = torch.empty((B, W), dtype=torch.uint8, device=dev)
    ln = torch.empty(B, **i32)
    leaf = torch.empty((N, B), dtype=torch.float64, device=dev)
    zeros, ones = torch.zeros(nw, **i32), torch.full((nw,), -1, **i32)
    counters = torch.zeros(1 + 2 * N, dtype=torch.int64, device=dev)
    st = sc._stream()

    def generate():
        _lib.check(lib.pcub_mc_info(seed, 0, B, N, sc._p(u), st), "pcub_mc_info")
        _lib.check(lib.pcub_polar_encode_bin(sc._p(u), B, n, sc._p(zeros), sc._p(zeros), N, sc._p(x), st),
                   "pcub_polar_encode_bin")
        _lib.check(lib.pcub_mc_deletion(seed, 0, B, n, sc._p(t), W, pd, sc._p(x), sc._p(rx), sc._p(ln), st),
                   "pcub_mc_deletion")

    def decode():
        _lib.check(lib.pcub_sc_leaf_deletion(sc._p(rx), sc._p(ln), B, W, n, n0, 0, pd, sc._p(ones), sc._p(zeros),
                                             sc._p(u), 0, None, None, sc._p(leaf), st), "pcub_sc_leaf_deletion")

    def count():
        _lib.check(lib.pcub_genie_count(sc._p(leaf), sc._p(u), B, n, sc._p(counters), st), "pcub_genie_count")
    sec = {"generate": [], "export_decode": [], "count": []}
    for it in range(reps + 1):
        for name, fn in (("generate", generate), ("export_decode", decode), ("count", count)):
            s, _ = timed(fn)
            if it:
                sec[name].append(s)
    return {k: statistics.median(v) for k, v in sec.items()}, N * B * 8 + nw * B * 4


def host_genie(n, n0, xi, pd, trials, seed):
    """main_deletion -g through the parent path; its printout (vectors of N floats) is dropped."""
    N = 1 << n
    make_x = main_deletion.make_xVectorDistribuiton_deletion_uniform(N)
    make_codeword = main_deletion.make_codeword_addDeletionGuardBands(xi, n, n0, 0)
    channel = main_deletion.make_simulateChannel_deletion(pd, seed=100)
    make_xy = main_deletion.make_xyVectorDistribution_deletion(pd, xi, n, n0, 0)
    with contextlib.redirect_stdout(io.StringIO()):
        return coding.genieEncodeDecodeSimulation(N, make_x, make_codeword, channel, make_xy, trials, 0.1,
                                                  genieSeed=seed, trustXYProbs=False)


def run_shape(n, n0, trials, host_trials, pd, xi, reps, seed):
    N = 1 << n
    mc.run_genie_deletion(n, n0, xi, pd, seed, 0, trials)  # warm-up
    secs, out = [], None
    for _ in range(reps):
        s, out = timed(lambda: mc.run_genie_deletion(n, n0, xi, pd, seed, 0, trials))
        secs.append(s)
    rate = [trials / s for s in secs]
    done, wrong, tie = out
    pe = np.array(coding.genie_pe_from_counts(done, wrong, tie))
    host_genie(n, n0, xi, pd, min(4, host_trials), 300)  # warm-up: first launches, templates
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_genie(n, n0, xi, pd, host_trials, 300)
    torch.cuda.synchronize()
    host_s = time.perf_counter() - t0
    W = int(mc.guard_template(n, n0, xi, 0, torch.device("cuda:0")).numel())
    B = int(min(trials, mc.genie_default_chunk(n, W)))
    split, count_bytes = stage_split(n, n0, xi, pd, seed, B, reps)
    total = sum(split.values())
    return dict(n=n, n0=n0, N=N, pd=pd, xi=xi, reps=reps,
                pipeline=dict(trials=trials, median_trials_s=statistics.median(rate), min_trials_s=min(rate),
                              max_trials_s=max(rate), seconds=[round(s, 6) for s in secs], counted=done,
                              wrong=int(wrong.sum()), tie=int(tie.sum()), mean_pe=float(pe.mean())),
                host=dict(trials=host_trials, trials_s=host_trials / host_s, seconds=round(host_s, 6)),
                speedup=statistics.median(rate) / (host_trials / host_s),
                split_trials=B, split_seconds={k: round(v, 6) for k, v in split.items()},
                split_share={k: round(v / total, 5) for k, v in split.items()},
                count_over_export_decode=round(split["count"] / split["export_decode"], 6),
                count_read_gb_s=round(count_bytes / split["count"] * 1e-9, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None, help="n,n0,trials,host_trials (repeatable)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pd", type=float, default=0.1)
    ap.add_argument("--xi", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=20251101)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else DEFAULT_SHAPES
    for n, n0, trials, host_trials in shapes:
        print(json.dumps(run_shape(n, n0, trials, host_trials, a.pd, a.xi, a.reps, a.seed)), flush=True)


if __name__ == "__main__":
    main()
