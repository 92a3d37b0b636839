"""The IR pipeline's per-codeword code on the CPU (tests/emu_ir/ir_emu.cpp over
polarcub_amd/csrc/ir_body.h, the functions the kernels of sc_ir.hip call): the verdict on crafted
final lists against QaryPolarEncoderDecoder._list_result, the transform and the key / frozen split
against coding_qary.polarTransformOfQudits, and the host-side argument checks of the loaded library
(no GPU needed: every call made here returns before a launch)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

P = ctypes.c_void_p


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu_ir")], check=True)
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emu_ir", "build", "libiremu.so"))
    lib.emu_ir_prepare.argtypes = [ctypes.c_uint64, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_double, ctypes.c_int, P, ctypes.c_int, P, P, P, P]
    lib.emu_ir_split.argtypes = [P, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, P, ctypes.c_int, P, P, P]
    lib.emu_ir_classify.argtypes = [P, P, P, P, P, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, P, P]
    return lib


def _ptr(a):
    return a.ctypes.data_as(P)


# -- crafted final lists -----------------------------------------------------------------------------
def _case(q, K, L, size, rows, probs, key, ap):
    """One codeword: rows {index: symbols} (any index < L, also past size), the rest random non-key
    rows; probs for [0, size)."""
    return dict(size=size, rows=rows, probs=list(probs), key=list(key), ap=ap)


def crafted_cases(q, K, L, use_log):
    """Codewords that hit every branch of listDecode's verdict (QaryPolarEncoderDecoder.py:172-213)
    exactly.  Metrics are the decoder's kind: the largest is 1 (0 in the log domain)."""
    assert L >= 6 and K >= 1
    key = [(3 * k + 1) % q for k in range(K)]
    other = [list(key) for _ in range(4)]
    for j, o in enumerate(other):  # non-key rows: differ from the key in the last, first, .. symbol
        o[(K - 1 - j) % K] = (o[(K - 1 - j) % K] + 1 + j % (q - 1)) % q
    if use_log:
        top, mid, low, tiny = 0.0, -0.75, -3.5, -np.inf
    else:
        top, mid, low, tiny = 1.0, 0.5, 0.125, 0.0
    above = 0.25 if use_log else 1.5
    between = (mid + low) / 2
    below = -9.0 if use_log else 0.0625
    c = []
    # 0: the key's metric is the maximum (alone, and tied with another path)
    c.append(_case(q, K, L, 4, {2: key}, [mid, low, top, low], key, top))
    c.append(_case(q, K, L, 4, {1: key}, [top, top, mid, low], key, top))
    # 1: the key is listed below the maximum
    c.append(_case(q, K, L, 5, {4: key}, [top, mid, low, mid, low], key, low))
    # the key at two indices: the lower one (below the maximum) decides, not the one at the maximum
    c.append(_case(q, K, L, 5, {1: key, 3: key}, [mid, low, mid, top, low], key, low))
    c.append(_case(q, K, L, 5, {0: key, 2: key}, [top, low, mid, mid, low], key, top))
    # 2 .. 5: no match; actual_prob above / at the maximum, inside the range (strictly, and exactly at
    # the minimum), below the minimum
    c.append(_case(q, K, L, 3, {}, [mid, top, low], key, above))
    c.append(_case(q, K, L, 3, {}, [mid, top, low], key, top))
    c.append(_case(q, K, L, 3, {}, [mid, top, low], key, between))
    c.append(_case(q, K, L, 3, {}, [mid, top, low], key, low))
    c.append(_case(q, K, L, 3, {}, [mid, top, low], key, below))
    # the key only at an index past the list's size: no match
    c.append(_case(q, K, L, 3, {4: key}, [top, mid, low], key, mid))
    c.append(_case(q, K, L, 1, {1: key}, [top], key, below))
    # size 1: match, no match (maximum == minimum: actual_prob at it is FailActualIsMax)
    c.append(_case(q, K, L, 1, {0: key}, [top], key, top))
    c.append(_case(q, K, L, 1, {}, [top], key, top))
    c.append(_case(q, K, L, 1, {}, [top], key, below))
    # a full list, the key last
    c.append(_case(q, K, L, L, {L - 1: key}, [top] + [mid] * (L - 2) + [low], key, low))
    # zero metrics (-inf in the log domain): a key of metric zero, an actual_prob of zero at the
    # minimum and below it
    c.append(_case(q, K, L, 3, {1: key}, [top, tiny, low], key, tiny))
    c.append(_case(q, K, L, 3, {}, [top, tiny, low], key, tiny))
    c.append(_case(q, K, L, 3, {}, [top, mid, low], key, tiny))
    return c, other


def build_lists(q, K, L, B, use_log, seed):
    """B codewords in the list decoder's output layout: the crafted cases, then random lists (random
    size, the key listed with probability 1/2, metrics from a few values so that ties occur).  Rows
    past a list's size are 0xff and their metrics NaN, unless a case plants the key there."""
    rng = np.random.default_rng(seed)
    info = np.full((L, max(K, 1), B), 0xff, np.uint8)
    prob = np.full((L, B), np.nan)
    size = np.zeros(B, np.int32)
    ap = np.zeros(B)
    actual = np.zeros((max(K, 1), B), np.uint8)
    cases, other = crafted_cases(q, K, L, use_log) if K else ([], [])
    values = [0.0, -0.75, -3.5, -np.inf, -1.25] if use_log else [1.0, 0.5, 0.125, 0.0, 0.25]
    for b in range(B):
        if b < len(cases):
            c = cases[b]
        else:
            key = rng.integers(0, q, K).tolist()
            sz = int(rng.integers(1, L + 1))
            probs = [values[0]] + [values[int(rng.integers(0, len(values)))] for _ in range(sz - 1)]
            probs = [probs[i] for i in rng.permutation(sz)]
            rows = {int(rng.integers(0, sz)): key} if rng.random() < 0.5 else {}
            c = _case(q, K, L, sz, rows, probs, key, values[int(rng.integers(0, len(values)))])
        size[b] = c["size"]
        ap[b] = c["ap"]
        actual[:K, b] = c["key"]
        prob[:c["size"], b] = c["probs"]
        for i in range(c["size"]):
            row = other[i % 4] if b < len(cases) else rng.integers(0, q, K).tolist()
            if K and row == c["key"]:
                row = list(row)
                row[0] = (row[0] + 1) % q
            info[i, :K, b] = row
        for i, row in c["rows"].items():
            info[i, :K, b] = row
    return dict(q=q, K=K, L=L, B=B, info=info[:, :K], prob=prob, size=size, ap=ap, actual=actual[:K])


def host_verdicts(d):
    """QaryPolarEncoderDecoder._list_result and irSimulation's counting (coding_qary.py, the
    reference's :172-213 and :905-909) on the lists as list_decode_batch hands them over (rows past
    the size -1): the ten counters and the outcome codes."""
    from polarcub_amd import coding_qary
    counters = [0] * 10
    codes = np.zeros(d["B"], np.uint8)
    for b in range(d["B"]):
        sz = int(d["size"][b])
        infos = d["info"][:, :, b].astype(np.int64)
        infos[sz:] = -1
        key = d["actual"][:, b].astype(np.int64)
        b_key, pr = coding_qary.QaryPolarEncoderDecoder._list_result(None, infos, d["prob"][:, b], sz,
                                                                      float(d["ap"][b]), d["L"], None, None, key)
        codes[b] = pr.value
        counters[0] += 1
        counters[3] += sz
        counters[4 + pr.value] += 1
        if not np.array_equal(key, b_key):
            counters[1] += 1
            counters[2] += int(coding_qary.hamming(key, b_key))
    return counters, codes


def emu_verdicts(emu, d):
    counters = np.zeros(10, np.uint64)
    res = np.zeros(d["B"], np.uint8)
    info, actual = np.ascontiguousarray(d["info"]), np.ascontiguousarray(d["actual"])
    emu.emu_ir_classify(_ptr(info), _ptr(d["prob"]), _ptr(d["size"]), _ptr(d["ap"]), _ptr(actual), d["B"], d["L"],
                        d["K"], _ptr(counters), _ptr(res))
    return [int(v) for v in counters], res


CLASSIFY_SHAPES = [(2, 5, 6), (3, 7, 9), (8, 4, 7), (3, 19, 6)]  # q, K, L (K = 19: two steps of eight symbols and a tail)


@pytest.mark.parametrize("use_log", [False, True])
@pytest.mark.parametrize("q,K,L", CLASSIFY_SHAPES)
def test_classify_matches_list_result(emu, q, K, L, use_log):
    """Every branch of the verdict, hit exactly (see crafted_cases), and random lists with ties, at
    q = 2, 3 and 8, with linear metrics that include 0 and log metrics that include -inf."""
    d = build_lists(q, K, L, 130, use_log, 17 * q + L)
    want, codes = host_verdicts(d)
    crafted = codes[:19].tolist()
    assert crafted == [0, 0, 1, 1, 0, 2, 3, 4, 4, 5, 4, 5, 0, 3, 5, 1, 1, 4, 5]
    assert all(want[4 + r] > 0 for r in range(6)) and want[0] == 130 and 0 < want[1] < 130
    got, res = emu_verdicts(emu, d)
    assert got == want
    assert np.array_equal(res, codes)


def test_classify_without_information_symbols(emu):
    """K = 0: the empty key is path 0 of every list; the outcome only says whether its metric is
    the maximum."""
    d = build_lists(3, 0, 6, 40, False, 5)
    want, codes = host_verdicts(d)
    assert want[1] == 0 and want[2] == 0 and want[4] + want[5] == 40 and want[4] > 0 and want[5] > 0
    got, res = emu_verdicts(emu, d)
    assert got == want and np.array_equal(res, codes)


def test_classify_accumulates(emu):
    d = build_lists(3, 7, 9, 50, False, 3)
    want, _ = host_verdicts(d)
    counters = np.arange(10).astype(np.uint64)
    info, actual = np.ascontiguousarray(d["info"]), np.ascontiguousarray(d["actual"])
    emu.emu_ir_classify(_ptr(info), _ptr(d["prob"]), _ptr(d["size"]), _ptr(d["ap"]), _ptr(actual), 50, 9, 7,
                        _ptr(counters), None)
    assert [int(v) for v in counters] == [w + i for i, w in enumerate(want)]


# -- the transform and the split -------------------------------------------------------------------
def masks(N):
    alt = np.zeros(N, np.uint8)
    alt[0::2] = 1
    return {"all": np.ones(N, np.uint8), "none": np.zeros(N, np.uint8), "alternating": alt}


def host_split(q, a, frozen):
    """(u, key, frozen values) of the words a [N, B] by the facade's transform."""
    from polarcub_amd import coding_qary
    u = np.stack([coding_qary.polarTransformOfQudits(q, a[:, b]) for b in range(a.shape[1])], axis=1).astype(np.uint8)
    return u, u[frozen == 0], u[frozen != 0]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("q", [2, 3, 5, 8])
def test_transform_and_split(emu, q, n):
    N, B = 1 << n, 5
    rng = np.random.default_rng(100 * q + n)
    a = rng.integers(0, q, (N, B)).astype(np.uint8)
    a[:, 0] = q - 1
    for name, frozen in masks(N).items():
        K = int(N - frozen.sum())
        u = np.zeros((N, B), np.uint8)
        actual = np.full((max(1, K), B), 0xee, np.uint8)
        fv = np.full((max(1, N - K), B), 0xee, np.uint8)
        emu.emu_ir_split(_ptr(a), B, n, q, _ptr(frozen), K, _ptr(u), _ptr(actual), _ptr(fv))
        hu, hkey, hfv = host_split(q, a, frozen)
        assert np.array_equal(u, hu), name
        assert np.array_equal(actual[:K], hkey), name
        assert np.array_equal(fv[:N - K], hfv), name
        if K == 0:
            assert (actual == 0xee).all()
        if K == N:
            assert (fv == 0xee).all()


def test_frozen_values_are_the_transform():
    """ir() hands listDecode (w (q - 1)) % q with w = (u (q - 1)) % q on the frozen set: u itself."""
    from polarcub_amd import coding_qary
    rng = np.random.default_rng(8)
    for q in (2, 3, 5, 8):
        N = 16
        frozen = sorted(rng.permutation(N)[:7].tolist())
        ed = coding_qary.QaryPolarEncoderDecoder(q, N, frozen, -1)
        a = rng.integers(0, q, N)
        u = coding_qary.polarTransformOfQudits(q, a)
        state = np.random.get_state()  # _ir_inputs draws its check matrix from the global numpy RNG
        key, fvals, _, _, _ = ed._ir_inputs(a, None, lambda b: None, 0)
        np.random.set_state(state)
        assert np.array_equal(fvals, u[frozen]) and np.array_equal(key, np.delete(u, frozen))


@pytest.mark.parametrize("use_log", [False, True])
def test_host_build_of_prepare(emu, use_log):
    """The draws feed the split: the rows take the two QSC values with one hit a row (their math.log
    in the log domain), key and frozen values are the transform of the drawn word, and two half
    batches at their offsets are the whole batch."""
    q, n, p, B, off = 5, 5, 0.3, 12, 1000
    N = 1 << n
    frozen = masks(N)["alternating"]
    K = N // 2

    def run(o, b):
        a = np.zeros((N, b), np.uint8)
        xy = np.zeros((N, b, q))
        act = np.zeros((K, b), np.uint8)
        fv = np.zeros((N - K, b), np.uint8)
        emu.emu_ir_prepare(77, o, b, n, q, p, int(use_log), _ptr(frozen), K, _ptr(a), _ptr(xy), _ptr(act), _ptr(fv))
        return a, xy, act, fv
    a, xy, act, fv = run(off, B)
    assert a.max() < q and len(np.unique(a)) == q
    hit, miss = 1.0 - p, p / (q - 1)
    if use_log:
        hit, miss = math.log(hit), math.log(miss)
    assert set(np.unique(xy).tolist()) == {hit, miss}
    assert ((xy == hit).sum(axis=2) == 1).all()
    y = (xy == hit).argmax(axis=2)
    assert 0.1 < (y != a).mean() < 0.5  # p = 0.3 over 384 symbols
    _, hkey, hfv = host_split(q, a, frozen)
    assert np.array_equal(act, hkey) and np.array_equal(fv, hfv)
    first, second = run(off, B // 2), run(off + B // 2, B // 2)
    for whole, x0, x1 in zip((a, xy, act, fv), first, second):
        assert np.array_equal(whole, np.concatenate([x0, x1], axis=1))


# -- the loaded library, host side -------------------------------------------------------------------
def test_workspace_grows_with_chunk_and_list_size():
    from polarcub_amd import _lib
    L = _lib.lib()
    base = L.pcub_mc_run_ir_workspace(64, 3, 6, 9, 34)
    assert base > 64 * (9 * 34 + 64 * 3 * 8)
    assert L.pcub_mc_run_ir_workspace(128, 3, 6, 9, 34) > base
    assert L.pcub_mc_run_ir_workspace(64, 3, 6, 81, 34) > base
    assert L.pcub_mc_run_ir_workspace(64, 3, 6, 4096, 34) > L.pcub_mc_run_ir_workspace(64, 3, 6, 81, 34)
    for bad in [(0, 3, 6, 9, 34), (64, 1, 6, 9, 34), (64, 9, 6, 9, 34), (64, 3, 13, 9, 34), (64, 3, 6, 0, 34),
                (64, 3, 6, 4097, 34), (64, 3, 6, 9, 65), (64, 3, 6, 9, -1)]:
        assert L.pcub_mc_run_ir_workspace(*bad) == 0


def test_invalid_arguments_return_einval_before_any_launch():
    """Every rejected call: one argument wrong, the others valid (the pointers are never read on the
    host, and no call here gets as far as a launch)."""
    from polarcub_amd import _lib
    L = _lib.lib()
    fake = P(1 << 20)
    big = 1 << 40
    ok = dict(seed=1, offset=0, count=10, log2N=6, q=3, p=0.1, L=9, use_log=0, frozen=fake, K=34, chunk=10,
              counters=fake, results=None, workspace=fake, workspace_bytes=big, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.pcub_mc_run_ir(a["seed"], a["offset"], a["count"], a["log2N"], a["q"], a["p"], a["L"], a["use_log"],
                                a["frozen"], a["K"], a["chunk"], a["counters"], a["results"], a["workspace"],
                                a["workspace_bytes"], a["stream"])
    least = L.pcub_mc_run_ir_workspace(10, 3, 6, 9, 34) - ((L.pcub_scl_qary_workspace(10, 3, 6, 9, 34) + 255) & ~255) \
        + L.pcub_scl_qary_workspace(1, 3, 6, 9, 34)
    assert least > 0
    wrong = [dict(counters=None), dict(frozen=None), dict(q=1), dict(q=9), dict(L=0), dict(L=4097), dict(log2N=13),
             dict(p=-0.01), dict(p=1.01), dict(p=float("nan")), dict(count=-1), dict(offset=-1), dict(chunk=0),
             dict(chunk=-5), dict(workspace=None), dict(workspace_bytes=least - 1), dict(workspace_bytes=0),
             dict(K=65), dict(K=-1)]
    for kw in wrong:
        assert call(**kw) == _lib.EINVAL, kw
    # the stages' own checks
    assert L.pcub_ir_prepare(1, 0, 4, 6, 9, 0.1, 0, fake, 34, fake, fake, fake, fake, fake, None) == _lib.EINVAL
    assert L.pcub_ir_prepare(1, 0, 4, 6, 3, 1.5, 0, fake, 34, fake, fake, fake, fake, fake, None) == _lib.EINVAL
    assert L.pcub_ir_prepare(1, 0, 4, 6, 3, 0.1, 0, None, 34, fake, fake, fake, fake, fake, None) == _lib.EINVAL
    assert L.pcub_ir_prepare(1, -1, 4, 6, 3, 0.1, 0, fake, 34, fake, fake, fake, fake, fake, None) == _lib.EINVAL
    assert L.pcub_ir_prepare(1, 0, 4, 6, 3, 0.1, 0, fake, 34, None, fake, fake, fake, fake, None) == _lib.EINVAL
    assert L.pcub_ir_classify(fake, fake, fake, fake, fake, 4, 9, 34, None, None, None) == _lib.EINVAL
    assert L.pcub_ir_classify(fake, fake, fake, fake, fake, 4, 0, 34, fake, None, None) == _lib.EINVAL
    assert L.pcub_ir_classify(fake, fake, fake, fake, fake, 4, 4097, 34, fake, None, None) == _lib.EINVAL
    assert L.pcub_ir_classify(None, fake, fake, fake, fake, 4, 9, 34, fake, None, None) == _lib.EINVAL
    # nothing to do is not an error
    assert call(count=0) == 0
    assert L.pcub_ir_classify(fake, fake, fake, fake, fake, 0, 9, 34, fake, None, None) == 0
