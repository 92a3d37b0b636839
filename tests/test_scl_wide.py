"""q-ary list decoding above L = 64 on CPU: the oracle's restatement (oracle/scl_oracle.py) against
runs of the reference itself at L = 81 .. 4096 (tests/golden/scl_wide.npz, made by
scripts/make_scl_wide_golden.py; until now the oracle was reference-pinned only up to L = 16), and
the host build of the workgroup kernel's code (tests/emu_scl_wg/scl_wg_emu.cpp over
polarcub_amd/csrc/scl_wg_body.h, the workgroup's 256 threads one after another between barriers)
against the oracle and, for its parallel top-L selection alone, against a direct restatement of
scl_prune / scl_commit (polarcub_amd/csrc/scl_body.h)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import scl_oracle as so
from tests.conftest import ROOT, load_golden
from tests.test_scl import _as_set, _close_log, _oracle_log_with_gap, _random_inputs, emu_decode


def wide_cases():
    return load_golden("scl_wide")["meta"]["cases"]


WIDE_SPECS = [(3, 5, 81, 8), (2, 6, 128, 6), (3, 4, 243, 6), (3, 6, 243, 3), (4, 5, 256, 3), (2, 7, 1024, 2),
              (2, 5, 4096, 2)]


def test_fixture_holds_the_cases():
    """The seven linear-domain cases and the first three again in the log domain, with their word
    counts; the last case's list is every q^K word."""
    g = load_golden("scl_wide")
    cases = g["meta"]["cases"]
    lin = [c for c in cases if not c["use_log"]]
    log = [c for c in cases if c["use_log"]]
    assert [(c["q"], c["n"], c["L"], g[c["tag"] + "_xy"].shape[0]) for c in lin] == WIDE_SPECS
    assert [(c["q"], c["n"], c["L"], g[c["tag"] + "_xy"].shape[0]) for c in log] == WIDE_SPECS[:3]
    last = lin[-1]
    assert (g[last["tag"] + "_size"] == last["q"] ** last["K"]).all() and last["q"] ** last["K"] <= last["L"]
    for c in cases:
        assert g[c["tag"] + "_info"].dtype == np.uint8 and len(c["prob_result"]) == g[c["tag"] + "_xy"].shape[0]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "scl_wide.npz")) < 1 << 20


def check_against_fixture(g, c, t, k, info, probs, ap):
    """One decoded word (list size, rows, metrics, actual_prob) against the reference's run: the
    path set, and the metrics bit for bit (linear domain) or within _close_log (log domain)."""
    t_ = c["tag"]
    rk = int(g[t_ + "_size"][t])
    assert k == rk
    ours = _as_set(np.asarray(info)[:rk].tolist(), np.asarray(probs)[:rk].tolist())
    ref = _as_set(g[t_ + "_info"][t][:rk].tolist(), g[t_ + "_prob"][t][:rk].tolist())
    assert [a for a, _ in ours] == [a for a, _ in ref]
    if c["use_log"]:
        assert _close_log([p for _, p in ours], [p for _, p in ref])
        assert _close_log(ap, g[t_ + "_aprob"][t])
    else:
        assert [p for _, p in ours] == [p for _, p in ref]
        assert ap == g[t_ + "_aprob"][t]


# (2, 7, 1024) is left to the GPU test (tests/test_gpu_scl_wide.py): the Python oracle takes about
# 14 s a word there, past the 30 s this file allows a case
ORACLE_CASES = [0, 1, 2, 3, 4, 6, 7, 8, 9]


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_oracle_matches_reference_wide(case):
    """oracle/scl_oracle.py against the reference at L = 81 .. 4096: linear domain, the path set,
    the metrics and actual_prob bit-equal; log domain, _close_log's tolerance.  The (2, 7, 1024) case
    (index 5) is skipped here: the oracle needs about 30 s for its two words; the GPU decoder meets
    that case in tests/test_gpu_scl_wide.py."""
    g = load_golden("scl_wide")
    c = g["meta"]["cases"][case]
    t_ = c["tag"]
    for t in range(g[t_ + "_xy"].shape[0]):
        k, info, probs, ap = so.list_decode(c["q"], g[t_ + "_frozen"], c["L"], g[t_ + "_xy"][t], g[t_ + "_fv"][t],
                                            g[t_ + "_actual"][t], use_log=c["use_log"])
        check_against_fixture(g, c, t, k, info, probs, ap)


# -- host build of the workgroup kernel's code ---------------------------------------------------
@pytest.fixture(scope="module")
def wg():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu_scl_wg")], check=True)
    return ctypes.CDLL(os.path.join(ROOT, "tests", "emu_scl_wg", "build", "libsclwgemu.so"))


class _AsEmu:
    """emu_scl_wg under the name tests.test_scl.emu_decode calls."""

    def __init__(self, lib):
        self.emu_scl = lib.emu_scl_wg


def _inputs(rng, q, n, B, kind):
    """tie-free rows; QSC rows (exact ties); QSC rows with one zero entry in a fifth of the rows
    (paths with a zero metric, which a prune does not count).  A zero never falls on the symbol of
    the codeword that the actual information and the frozen values encode, so that word's path keeps
    a non-zero metric and no list is all zero."""
    frozen, xy, fv, act = _random_inputs(rng, q, n, B, kind != "free")
    if kind == "zeros":
        x = np.array([so.polar_qudits(q, so.merge_info_and_frozen(frozen, act[b], fv[b])) for b in range(B)])
        hit = rng.random(xy.shape[:2]) < 0.2
        col = (x + rng.integers(1, q, xy.shape[:2])) % q
        xy = np.where(hit[:, :, None] & (np.arange(q)[None, None, :] == col[:, :, None]), 0.0, xy)
    return frozen, xy, fv, act


@pytest.mark.parametrize("kind", ["free", "ties", "zeros"])
@pytest.mark.parametrize("q,n,L", [(3, 4, 81), (2, 5, 128), (3, 5, 243)])
def test_workgroup_code_matches_oracle(wg, q, n, L, kind):
    """Linear domain, bit for bit: list size, rows in order, metrics, actual_prob."""
    rng = np.random.default_rng(1000 * q + 10 * n + L + len(kind))
    B = 3
    frozen, xy, fv, act = _inputs(rng, q, n, B, kind)
    size, info, prob, ap = emu_decode(_AsEmu(wg), xy, q, L, frozen, fv, act)
    for b in range(B):
        k, oinfo, oprob, oap = so.list_decode(q, frozen, L, xy[b], fv[b], act[b])
        assert np.isfinite(oprob).all()  # no all-zero list (its 0/0 metrics are unspecified)
        assert size[b] == k
        assert info[b][:k].tolist() == oinfo
        assert np.array_equal(prob[b][:k], np.array(oprob))
        assert ap[b] == oap


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("q,n,L", [(3, 4, 81), (2, 5, 128), (3, 5, 243)])
def test_workgroup_code_log_matches_oracle(wg, monkeypatch, q, n, L, ties):
    """Log domain, by the rules of tests/test_scl.py::test_kernel_code_log_matches_oracle: the same
    lists in the same order and metrics within the log tolerance, except for codewords with a prune
    whose kept / dropped metrics are within 1e-9 (exact ties among them), where only the list size
    and the normalisation are checked."""
    rng = np.random.default_rng(3000 * q + 10 * n + L + ties)
    B = 3
    frozen, xy, fv, act = _random_inputs(rng, q, n, B, ties)
    xy = np.log(xy)
    size, info, prob, ap = emu_decode(_AsEmu(wg), xy, q, L, frozen, fv, act, use_log=True)
    compared = 0
    for b in range(B):
        (k, oinfo, oprob, oap), gap = _oracle_log_with_gap(monkeypatch, q, frozen, L, xy[b], fv[b], act[b])
        if gap < 1e-9:
            assert size[b] == k and prob[b][:k].max() == 0.0
            continue
        compared += 1
        assert size[b] == k
        assert info[b][:k].tolist() == oinfo
        assert _close_log(prob[b][:k], np.array(oprob))
        assert _close_log(ap[b], oap)
    assert ties or compared >= (B + 1) // 2


@pytest.mark.parametrize("use_log", [False, True])
def test_workgroup_code_equals_lane_code(wg, use_log):
    """The two host builds (scl_body.h's lane walk, scl_wg_body.h's workgroup walk) agree bit for bit
    in both domains, ties and list sizes on either side of 64 included: they perform the same
    rounded operations."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "build/libsclemu.so"], check=True)
    lane = ctypes.CDLL(os.path.join(ROOT, "tests", "emu", "build", "libsclemu.so"))
    for q, n, L, ties in [(2, 3, 2, False), (4, 5, 8, True), (3, 4, 64, True), (2, 8, 8, False), (8, 3, 5, False),
                          (2, 0, 2, False), (3, 5, 1, False), (4, 6, 32, True)]:
        rng = np.random.default_rng(100 * q + 10 * n + L)
        frozen, xy, fv, act = _random_inputs(rng, q, n, 4, ties)
        if use_log:
            xy = np.log(xy)
        a = emu_decode(lane, xy, q, L, frozen, fv, act, use_log=use_log)
        b = emu_decode(_AsEmu(wg), xy, q, L, frozen, fv, act, use_log=use_log)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (q, n, L, ties)


# -- the selection alone -------------------------------------------------------------------------
def prune_commit(cand, L, use_log):
    """scl_prune + scl_commit restated: all kept when ncand <= L; else the keep = max(1,
    min(count of non-zero, L)) largest, ties to the lower candidate, in ascending candidate order."""
    cand = np.asarray(cand, np.float64)
    n = len(cand)
    if n <= L:
        return np.arange(n)
    nz = int((cand != (-np.inf if use_log else 0.0)).sum())
    keep = max(1, min(nz, L))
    order = np.argsort(-cand, kind="stable")  # descending metric, equal metrics by ascending index
    return np.sort(order[:keep])


def wg_select(lib, cand, q, L, use_log):
    cand = np.ascontiguousarray(cand, np.float64)
    org = np.zeros(max(L, len(cand)), np.int32)
    prob = np.zeros(max(L, len(cand)))
    P = ctypes.c_void_p
    k = lib.emu_wg_select(cand.ctypes.data_as(P), len(cand), q, L, int(use_log), org.ctypes.data_as(P),
                          prob.ctypes.data_as(P))
    assert k >= 0
    return org[:k], prob[:k]


def _selection_arrays(rng, n, L, use_log):
    """Random and adversarial candidate arrays of length n for a list of L."""
    base = rng.random(n)
    out = {"random": base.copy()}
    srt = np.sort(base)[::-1]
    tied = base.copy()
    if n > L:  # the threshold value repeated on both sides of the cut
        thr = srt[L - 1]
        tied[rng.random(n) < 0.3] = thr
    out["ties_at_threshold"] = tied
    out["all_equal"] = np.full(n, 0.25)
    out["all_zero"] = np.zeros(n)
    few = np.zeros(n)
    few[rng.permutation(n)[: max(1, min(n, L) // 3)]] = rng.random(max(1, min(n, L) // 3)) + 0.1
    out["few_nonzero"] = few
    out["two_values"] = rng.integers(0, 2, n).astype(np.float64)
    out["tiny"] = base * 5e-324 * 4  # denormals and zeros
    out["close"] = 1.0 + rng.integers(0, 4, n) * 2.0 ** -52
    if use_log:
        with np.errstate(divide="ignore"):
            lg = {k: np.log(v) for k, v in out.items()}  # zeros become -inf
        lg["mixed_signs"] = rng.standard_normal(n) * 3.0
        mixed = rng.standard_normal(n)
        mixed[rng.random(n) < 0.4] = -np.inf
        mixed[rng.random(n) < 0.1] = 0.0
        mixed[rng.random(n) < 0.05] = -0.0
        lg["mixed_with_inf_and_zeros"] = mixed
        return lg
    signed_zero = base.copy()
    signed_zero[rng.random(n) < 0.5] = 0.0
    signed_zero[rng.random(n) < 0.2] = -0.0  # -0.0 and +0.0 are one value
    out["signed_zeros"] = signed_zero
    return out


@pytest.mark.parametrize("use_log", [False, True])
@pytest.mark.parametrize("q,L,ncand", [(2, 1, 8), (2, 3, 24), (3, 81, 81), (3, 81, 243), (2, 100, 255), (2, 100, 257),
                                       (4, 256, 1000), (3, 243, 6561), (2, 1024, 8192), (3, 4096, 4096),
                                       (3, 4096, 4097), (3, 4096, 4096 * 27)])
def test_selection_equals_prune_and_commit(wg, use_log, q, L, ncand):
    """wg_prune_commit (radix select, prefix count in candidate order, compaction) against scl_prune
    / scl_commit restated: the kept candidates, their order and their metrics, on random and
    adversarial arrays up to ncand = 4096 x 27, ncand <= L included."""
    rng = np.random.default_rng(ncand * 7 + L + use_log)
    for name, cand in _selection_arrays(rng, ncand, L, use_log).items():
        org, prob = wg_select(wg, cand, q, L, use_log)
        want = prune_commit(cand, L, use_log)
        assert np.array_equal(org, want), name
        assert np.array_equal(prob, cand[want]), name
