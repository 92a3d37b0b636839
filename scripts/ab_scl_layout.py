#!/usr/bin/env python3
"""A/B of the list decoder's two layouts at L <= 64 on the bench's inputs.

    python scripts/ab_scl_layout.py [--shape q,n,L,B ...] [--reps R] [--warmup W]

Times sc.set_scl_layout(1) (k_scl: a lane a codeword) against sc.set_scl_layout(2) (k_scl_wg: a
workgroup a codeword) on the inputs of `bench.py --workload scl` (the same frozen set, Philox QSC(0.11)
batch, frozen values 0): device events around each decode_native call, warm-up calls first, the two
layouts interleaved in one process, R repeats each.  Prints one JSON line a shape with each
layout's median codewords/s and the spread (min .. max) of its repeats, and whether the outputs
are identical.  Default shapes: (q 4, N 256, L 8), (q 4, N 4096, L 32), (q 4, N 1024, L 64).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from polarcub_amd import construction, mc, sc  # noqa: E402

DEFAULT_SHAPES = [(4, 8, 8, 1 << 16), (4, 12, 32, 1 << 12), (4, 10, 64, 1 << 12)]


def bench_code(q, n, device):
    """The frozen set bench.py's q-ary workloads use."""
    N = 1 << n
    if q == 4 and n == 8:
        g = np.load(os.path.join(ROOT, "tests", "golden", "construct_qary.npz"), allow_pickle=False)
        mask = g["qsc4_n8_L64_frozen"].astype(np.uint8)
    else:
        z = construction.bhattacharyya_z(n, 0.5)
        order = sorted(range(N), key=lambda i: (z[i], i))
        mask = np.ones(N, np.uint8)
        mask[order[:N // 2]] = 0
    return sc.QaryCode(q, N, mask, device=device), mask


def run_shape(q, n, L, B, reps, warmup, seed, device):
    code, mask = bench_code(q, n, device)
    N = 1 << n
    _, xy = mc.philox_qsc_batch(code, seed, 0, B, 0.11, tile=0)
    fv = torch.zeros((int(mask.sum()), B), dtype=torch.uint8, device=device)
    decs, times, outs = {}, {1: [], 2: []}, {}
    try:
        for mode in (1, 2):
            sc.set_scl_layout(mode)
            decs[mode] = sc.QaryListDecoder(q, N, mask, L, device=device)
        for it in range(warmup + reps):
            for mode in (1, 2):
                sc.set_scl_layout(mode)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs[mode] = decs[mode].decode_native(xy, fv)
                e1.record()
                e1.synchronize()
                if it >= warmup:
                    times[mode].append(e0.elapsed_time(e1) * 1e-3)
    finally:
        sc.set_scl_layout(0)
    same = all(torch.equal(a, b) for a, b in zip(outs[1][:3], outs[2][:3]))
    res = dict(q=q, N=N, L=L, batch=B, reps=reps, warmup=warmup, identical=bool(same))
    for mode, name in ((1, "lane"), (2, "workgroup")):
        cw = [B / t for t in times[mode]]
        res[name] = dict(median_cw_s=statistics.median(cw), min_cw_s=min(cw), max_cw_s=max(cw),
                         seconds=[round(t, 6) for t in times[mode]])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=None, help="q,n,L,B (repeatable)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20250204)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else DEFAULT_SHAPES
    device = torch.device("cuda:0")
    for q, n, L, B in shapes:
        print(json.dumps(run_shape(q, n, L, B, a.reps, a.warmup, a.seed, device)), flush=True)


if __name__ == "__main__":
    main()
