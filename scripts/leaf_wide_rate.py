"""Genie-mode leaf export of the deletion channel at 512 / 1024 trellises a codeword (n0 = 4,
n = 13, 14: k_sc_del<4, 9|10, true, 0>): DeletionDecoder.decode_leaves on B codewords, all positions
frozen to each codeword's own u, timed with device events after a warm-up; then the generic host
recursion the genie used before (genieEncodeDecodeSimulation with the leaf kernel reported missing)
over a few trials.  Diagnostic, not a test.

    python scripts/leaf_wide_rate.py [--n 13 14] [--B 1024] [--reps 5] [--host-trials 2]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polarcub_amd import coding, mc, sc  # noqa: E402
from polarcub_amd.cli import main_deletion as md  # noqa: E402

N0, PD, XI = 4, 0.1, 0.1


def device_rate(n, B, reps, warmup=2):
    dev = torch.device("cuda", 0)
    N = 1 << n
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    full = sc.CodeSpec(N, np.zeros(N, np.uint8), np.zeros(N, np.uint8), device=dev)  # K = N: info = u
    rx, ln, U = mc.deletion_batch(full, B, N0, XI, PD, gen)
    genie = sc.CodeSpec(N, np.ones(N, np.uint8), np.zeros(N, np.uint8), device=dev)
    d = sc.DeletionDecoder(genie, N0, PD)
    ms = []
    for r in range(warmup + reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _, xhat, m = d.decode_leaves(rx, ln, U)
        t1.record()
        t1.synchronize()
        if r >= warmup:
            ms.append(t0.elapsed_time(t1))
    # the genie's decode re-encodes to the sent codeword, and the leaves are live
    assert torch.equal(xhat, sc.encode(full, U))
    live = float((m[:, :, 0] != 0.5).double().mean())
    ms.sort()
    return {"n": n, "B": B, "reps": reps, "ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1],
            "cw_per_s": B / (ms[len(ms) // 2] * 1e-3), "leaves_not_half": live}


def host_rate(n, trials):
    N = 1 << n
    orig = sc.leaf_deletion_supported
    sc.leaf_deletion_supported = lambda n, n0, ones=0: False
    try:
        t = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            coding.genieEncodeDecodeSimulation(
                N, md.make_xVectorDistribuiton_deletion_uniform(N), md.make_codeword_addDeletionGuardBands(XI, n, N0, 0),
                md.make_simulateChannel_deletion(PD, seed=100), md.make_xyVectorDistribution_deletion(PD, XI, n, N0, 0),
                trials, 0.1, genieSeed=300, trustXYProbs=False)
        dt = time.perf_counter() - t
    finally:
        sc.leaf_deletion_supported = orig
    return {"n": n, "host_trials": trials, "s_per_trial": dt / trials, "cw_per_s": trials / dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[13, 14])
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-trials", type=int, default=2)
    a = ap.parse_args()
    for n in a.n:
        print(json.dumps(device_rate(n, a.B, a.reps)), flush=True)
    for n in a.n:
        if a.host_trials > 0:
            print(json.dumps(host_rate(n, a.host_trials)), flush=True)


if __name__ == "__main__":
    main()
