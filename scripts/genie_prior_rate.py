"""Genie passes under a non-uniform prior at N = 1024: the wave-a-trial kernel
(pcub_sc_genie_prior_bin, sc.GeniePriorCoder) against the lane-a-codeword two-tree kernel
(pcub_sc_prior_bin, sc.PriorCoder) on the same prior with one r for all trials and every position
frozen -- the same trees and the same arithmetic -- in encode mode (K = 0, prior tree only) and in
decode mode.  The two alternate in one process after a warm-up, each call timed with device events;
the median of the repetitions is reported with min and max, and x_hat and the compact leaves of the
timed inputs are compared.  The inputs are staged in each kernel's own layout beforehand (rows for
the wave kernel, [N][B] for the lane kernel): only the kernels are timed.  Diagnostic, not a test.

    python scripts/genie_prior_rate.py [--n 10] [--B 4096 65536] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polarcub_amd import sc  # noqa: E402


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}


def rate(n, B, reps, warmup):
    dev = torch.device("cuda", 0)
    N = 1 << n
    rng = np.random.default_rng(1000 * n + B % 997)
    prior = np.tile(np.array([0.89, 0.11]), (N, 1))
    r = rng.random(N)
    gen = torch.Generator(device=dev)
    gen.manual_seed(B)
    # BSC(0.1) joint rows of random received symbols
    y = torch.randint(0, 2, (B, N), generator=gen, device=dev)
    table = torch.tensor([[0.89 * 0.9, 0.11 * 0.1], [0.89 * 0.1, 0.11 * 0.9]], dtype=torch.float64, device=dev)
    xy_rows = torch.where(y[:, :, None] != 0, table[1], table[0]).contiguous()  # [B, N, 2]
    xy_lane = sc.transpose_pairs(xy_rows)                # [N, B, 2]
    p_dev = torch.from_numpy(prior).to(dev)
    R = torch.from_numpy(r).to(dev)[None, :].expand(B, N).contiguous()
    code = sc.CodeSpec(N, np.ones(N, np.uint8), device=dev)
    lane = sc.PriorCoder(code, r)
    wave = sc.GeniePriorCoder(N, device=dev)
    out = []
    for mode, xr, xl in (("encode", None, None), ("decode", xy_rows, xy_lane)):
        ms = {"wave": [], "lane": []}
        for i in range(warmup + reps):
            tw, (xh_w, _, leaf_w) = timed(lambda: wave.run_native(p_dev, R, xy=xr))
            tl, (_, xw_l, leaf_l) = timed(lambda: lane.run_native(p_dev, xy=xl, B=B, want_leaf=True))
            if i >= warmup:
                ms["wave"].append(tw)
                ms["lane"].append(tl)
        same_x = bool(torch.equal(sc.unpack(xw_l, N), xh_w))
        same_leaf = bool(torch.equal(leaf_l.t().contiguous().view(torch.int64), leaf_w.view(torch.int64)))
        w, l = stats(ms["wave"]), stats(ms["lane"])
        out.append({"n": n, "B": B, "mode": mode, "reps": reps, "wave": w, "lane": l,
                    "wave_trials_per_s": B / (w["ms_median"] * 1e-3), "lane_trials_per_s": B / (l["ms_median"] * 1e-3),
                    "lane_over_wave": l["ms_median"] / w["ms_median"], "same_xhat": same_x, "same_leaves": same_leaf})
        del xh_w, leaf_w, xw_l, leaf_l
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--B", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "genie_prior_rate.py needs a GPU"
    for B in a.B:
        for row in rate(a.n, B, a.reps, a.warmup):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
