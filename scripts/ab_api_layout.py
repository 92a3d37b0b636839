"""A/B of the API layout: decoding a [B, N, 2] / [B, N, q] batch (the reference's layout, what
BinaryDecoder.decode, QaryDecoder.decode and torch.ops.polarcub.* take) on one GPU,
  (a) rows     the rows entry points (pcub_sc_decode_bin_rows / _qary_rows): the rows read in place;
  (b) staged   pcub_tile_pairs into a second buffer, then the tiled decode (the path before them);
  (c) tiled    the tiled decode alone on rows already in the kernel's tiles (what bench.py times);
and, where the launcher has more than one kernel for the rows, (a) with the rows twins switched off
(rows_generic: the generic path) and with non-temporal instead of plain root loads (rows_nt).

Device events around `--inner` back-to-back calls, `--warmup` untimed rounds, then `--reps` rounds with
the candidates interleaved in one process; min / median / max of the per-call times; every candidate's
outputs compared bit for bit.  One JSON line a shape, appended to --out.  Diagnostic, not a test.

    python scripts/ab_api_layout.py --out profiles/api_layout/ab_api_layout.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polarcub_amd import _lib, construction, mc, sc  # noqa: E402

SEED = 20250204


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def stats(ms, B):
    v = np.asarray(ms)
    return {"ms_min": float(v.min()), "ms_median": float(np.median(v)), "ms_max": float(v.max()),
            "mcw_s_median": float(B / np.median(v) / 1e3)}


def run_shape(name, cands, same, B, a):
    """cands: {label: fn}; same(): True when every candidate's last outputs are identical."""
    for _ in range(a.warmup):
        for fn in cands.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(a.reps):
        for k, fn in cands.items():
            times[k].append(timed(fn, a.inner))
    ok = bool(same())
    rec = {"shape": name, "B": B, "reps": a.reps, "inner": a.inner, "identical_outputs": ok,
           "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        rec[k] = stats(v, B)
    rec["a_over_b"] = rec["rows"]["ms_median"] / rec["staged"]["ms_median"]
    rec["a_over_c"] = rec["rows"]["ms_median"] / rec["tiled"]["ms_median"]
    rec["a_faster_than_b_ranges_disjoint"] = rec["rows"]["ms_max"] < rec["staged"]["ms_min"]
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert ok, "outputs differ at " + name
    return rec


def binary(name, n, K, B, a):
    L = _lib.lib()
    N = 1 << n
    s2 = construction.awgn_sigma2(2.0, K / N)
    fr = construction.bhattacharyya_frozen(n, K, s2)
    code = sc.CodeSpec.from_frozen_set(N, set(np.nonzero(fr)[0].tolist()), 1)
    dec = sc.BinaryDecoder(code)
    T = sc.bin_tile(n)
    assert B % T == 0
    _, xt = mc.philox_batch(code, SEED, 0, B, mc.CHANNEL_AWGN, s2, tile=T)        # [B/T, N, T, 2]
    rows = xt.permute(0, 2, 1, 3).reshape(B, N, 2).contiguous()                    # [B, N, 2]
    dec.workspace(B)

    def outs():
        return (torch.empty((code.info_words, B), dtype=torch.int32, device="cuda"),
                torch.empty((code.n_words, B), dtype=torch.int32, device="cuda"), None)

    o = {k: outs() for k in ("rows", "staged", "tiled", "rows_generic", "rows_nt")}

    def generic():
        old = L.pcub_sc_set_tiled_root(0)
        dec.decode_rows_native(rows, out=o["rows_generic"])
        L.pcub_sc_set_tiled_root(old)

    def nontemporal():
        old = L.pcub_sc_set_rows_nt(1)
        dec.decode_rows_native(rows, out=o["rows_nt"])
        L.pcub_sc_set_rows_nt(old)

    cands = {"rows": lambda: dec.decode_rows_native(rows, out=o["rows"]),
             "staged": lambda: dec.decode_tiled_native(sc.tile_pairs(rows, T), B, out=o["staged"]),
             "tiled": lambda: dec.decode_tiled_native(xt, B, out=o["tiled"])}
    v = sc.variant_for(n)
    if v in (26, 30, 33):
        cands["rows_generic"] = generic
    if v == 26:
        cands["rows_nt"] = nontemporal

    def same():
        return all(torch.equal(o[k][0], o["tiled"][0]) and torch.equal(o[k][1], o["tiled"][1]) for k in cands)

    rec = run_shape("%s (binary N=%d K=%d, %s, callers use %s)" % (
        name, N, K, "variant %d" % v if n > 5 else "small-code kernel", "rows" if sc.rows_preferred(n) else "staged"),
        cands, same, B, a)
    del xt, rows, o
    torch.cuda.empty_cache()
    return rec


def qary(name, q, n, p, B, a):
    L = _lib.lib()
    N = 1 << n
    if q == 4 and n == 8:   # the C4 code: the reference's own degrading construction (bench.py's)
        g = np.load(os.path.join(ROOT, "tests", "golden", "construct_qary.npz"), allow_pickle=False)
        mask = g["qsc4_n8_L64_frozen"].astype(np.uint8)
    else:                   # rate 1/2 by the binary Bhattacharyya ranking (bench.py's stand-in)
        z = construction.bhattacharyya_z(n, 0.5)
        mask = np.ones(N, np.uint8)
        mask[sorted(range(N), key=lambda i: (z[i], i))[:N // 2]] = 0
    code = sc.QaryCode(q, N, mask)
    dec = sc.QaryDecoder(code)
    T = dec.tile()
    assert B % T == 0
    _, xt = mc.philox_qsc_batch(code, SEED, 0, B, p, tile=T)
    rows = xt.permute(0, 2, 1, 3).reshape(B, N, q).contiguous()
    dec.workspace(B)
    o = {}

    def put(k, v):
        o[k] = v

    def generic():
        old = L.pcub_sc_set_qary_tiled_root(0)
        put("rows_generic", dec.decode_rows_native(rows))
        L.pcub_sc_set_qary_tiled_root(old)

    cands = {"rows": lambda: put("rows", dec.decode_rows_native(rows)),
             "staged": lambda: put("staged", dec.decode_tiled_native(sc.tile_pairs(rows, T), B)),
             "tiled": lambda: put("tiled", dec.decode_tiled_native(xt, B)),
             "rows_generic": generic}

    def same():
        return all(torch.equal(o[k][0], o["tiled"][0]) and torch.equal(o[k][1], o["tiled"][1]) for k in cands)

    rec = run_shape("%s (q=%d N=%d K=%d QSC(%g))" % (name, q, N, code.K, p), cands, same, B, a)
    del xt, rows
    o.clear()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=0, help="shift every batch right by this many bits (smoke runs)")
    ap.add_argument("--shapes", default="C2,N4096,C4,N256,N64,N32",
                    help="comma-separated shapes to run (also Q2, Q3, Q5, Q8: the generic q-ary kernels at N = 256)")
    a = ap.parse_args()
    s = a.scale
    table = {"C2": lambda: binary("C2", 10, 512, (1 << 20) >> s, a),
             "N4096": lambda: binary("N4096", 12, 2048, (1 << 18) >> s, a),
             "C4": lambda: qary("C4", 4, 8, 0.11, (1 << 20) >> s, a),
             "N256": lambda: binary("N256", 8, 128, (1 << 20) >> s, a),
             "N64": lambda: binary("N64", 6, 32, (1 << 20) >> s, a),
             "N32": lambda: binary("N32", 5, 16, (1 << 20) >> s, a),
             "Q2": lambda: qary("Q2", 2, 8, 0.11, (1 << 19) >> s, a),
             "Q3": lambda: qary("Q3", 3, 8, 0.11, (1 << 19) >> s, a),
             "Q5": lambda: qary("Q5", 5, 8, 0.11, (1 << 18) >> s, a),
             "Q8": lambda: qary("Q8", 8, 8, 0.11, (1 << 18) >> s, a)}
    recs = [table[k]() for k in a.shapes.split(",")]
    print("%-72s %10s %10s %10s %8s %8s" % ("shape", "(a) rows", "(b) staged", "(c) tiled", "a/b", "a/c"))
    for r in recs:
        print("%-72s %10.3f %10.3f %10.3f %8.3f %8.3f" % (r["shape"], r["rows"]["ms_median"], r["staged"]["ms_median"],
                                                          r["tiled"]["ms_median"], r["a_over_b"], r["a_over_c"]))


if __name__ == "__main__":
    main()
