#!/usr/bin/env python3
"""tests/golden/scl_wide.npz: the reference's q-ary list decoder above L = 64.

    python scripts/make_scl_wide_golden.py

Runs QaryPolarEncoderDecoder.listDecode with actualInformation (the reference loaded by
oracle.make_golden.load_reference, so only where the reference is present) on tie-free rows
(rs.random * 0.98 + 0.02) with a random frozen set, and records what oracle.make_golden.fx_scl
records: the final list captured from the outermost recursiveListDecode return
(informationList[:finalListSize] as uint8), prob_list, the list size, actual_prob and the returned
ProbResult's name.  The list ORDER is numpy-argpartition-dependent; tests compare it as a set.

Cases (q, n, L, words): (3,5,81,8) (2,6,128,6) (3,4,243,6) (3,6,243,3) (4,5,256,3) (2,7,1024,2),
(2,5,4096,2) at a frozen rate of about 0.7 (the list is every q^K word, never pruned), and the
first three again with use_log=True (rows np.log of the linear ones).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as mg  # noqa: E402

# (q, n, L, words, frozen rate)
SPECS = [(3, 5, 81, 8, 0.35), (2, 6, 128, 6, 0.4), (3, 4, 243, 6, 0.45), (3, 6, 243, 3, 0.4), (4, 5, 256, 3, 0.55),
         (2, 7, 1024, 2, 0.5), (2, 5, 4096, 2, 0.7)]
LOG_CASES = 3


def run_case(R, rs, q, n, L, T, fr, use_log):
    QPED = R["QPED"]
    N = 1 << n
    frozen = set(int(i) for i in np.nonzero(rs.random(N) < fr)[0])
    dec = QPED.QaryPolarEncoderDecoder(q, N, frozen, 1, use_log=use_log)
    K = dec.k
    xy = rs.random((T, N, q)) * 0.98 + 0.02
    if use_log:
        xy = np.log(xy)
    fv = rs.integers(0, q, (T, len(frozen)))
    act = rs.integers(0, q, (T, K))
    rows = min(L, q ** K)
    infos = np.full((T, rows, K), 0xff, np.uint8)
    probs = np.full((T, rows), np.nan)
    sizes = np.zeros(T, np.int64)
    aprob = np.zeros(T)
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
            _, pr = dec.listDecode(vd, fv[t], L, np.zeros((K, 0), np.int64), np.zeros(0, np.int64),
                                   actualInformation=act[t])
        finally:
            del dec.recursiveListDecode
        il, _, _, _, fls, _, _ = top["r"]
        sizes[t] = fls
        infos[t, :fls] = np.asarray(il[:fls], np.uint8)
        probs[t, :fls] = dec.prob_list[:fls]
        aprob[t] = dec.actual_prob
        pres.append(pr.name)
    mask = np.array([1 if i in frozen else 0 for i in range(N)], np.uint8)
    arrays = dict(xy=xy, frozen=mask, fv=fv.astype(np.uint8), actual=act.astype(np.uint8), info=infos, prob=probs,
                  size=sizes, aprob=aprob)
    return K, pres, arrays


def main():
    R = mg.load_reference()
    out, cases = {}, []
    for use_log in (False, True):
        rs = np.random.default_rng(4096)  # the log cases repeat the linear ones' draws
        for ci, (q, n, L, T, fr) in enumerate(SPECS[:LOG_CASES] if use_log else SPECS):
            K, pres, arrays = run_case(R, rs, q, n, L, T, fr, use_log)
            tag = ("g%d" if use_log else "c%d") % ci
            out.update({tag + "_" + k: v for k, v in arrays.items()})
            cases.append(dict(tag=tag, q=q, n=n, L=L, K=K, use_log=use_log, prob_result=pres))
            print(tag, q, n, L, "K=%d" % K, "sizes", arrays["size"].tolist(), pres, flush=True)
    mg.save("scl_wide", dict(cases=cases, note="listDecode with actualInformation above L = 64; list order is "
                                               "argpartition's; info rows past a list's size are 0xff"), **out)


if __name__ == "__main__":
    main()
