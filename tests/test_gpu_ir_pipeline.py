"""The IR Monte-Carlo pipeline on the GPU (sc_ir.hip): pcub_ir_prepare against the generators it
restates and the host transform, pcub_ir_classify against QaryPolarEncoderDecoder._list_result on the
crafted lists of tests/test_ir_pipeline.py, and pcub_mc_run_ir against the composed path (the prepare
stage's buffers -> QaryListDecoder.decode_native -> _list_result on the host), over shards, chunks
and workspace sizes.  All shapes are N <= 128."""
import math
import random

import numpy as np
import pytest
import torch

from tests.test_ir_pipeline import CLASSIFY_SHAPES, build_lists, host_split, host_verdicts

pytestmark = pytest.mark.gpu


def make_code(q, n, K):
    from polarcub_amd import construction, sc
    mask = construction.bhattacharyya_frozen(n, K, 0.5)
    return sc.QaryCode(q, 1 << n, mask, device="cuda"), mask


# -- pcub_ir_prepare -----------------------------------------------------------------------------------
def generators(code, seed, offset, B, p):
    """a and the linear rows through the entries pcub_ir_prepare restates."""
    from polarcub_amd import _lib, sc
    L = _lib.lib()
    a = torch.empty((code.N, B), dtype=torch.uint8, device=code.device)
    _lib.check(L.pcub_mc_info_qary(seed, offset, B, code.N, code.q, sc._p(a), sc._stream()), "pcub_mc_info_qary")
    xy = torch.empty((code.N, B, code.q), dtype=torch.float64, device=code.device)
    _lib.check(L.pcub_mc_channel_qsc(seed, offset, B, code.n, code.q, p, sc._p(a), sc._p(xy), sc._stream()),
               "pcub_mc_channel_qsc")
    return a, xy


@pytest.mark.parametrize("q,n,K,p", [(3, 6, 34, 0.10), (8, 7, 50, 0.3), (2, 2, 1, 0.5), (5, 5, 32, 0.0), (4, 4, 0, 0.2)])
def test_prepare_restates_the_generators_and_the_transform(q, n, K, p):
    from polarcub_amd import mc
    code, mask = make_code(q, n, K)
    B, off, seed = 130, 100000, 31
    a, xy, act, fv = mc.ir_prepare(code, seed, off, B, p)
    ga, gxy = generators(code, seed, off, B, p)
    assert torch.equal(a, ga) and torch.equal(xy, gxy)  # bit for bit
    _, hkey, hfv = host_split(q, a.cpu().numpy(), mask)
    assert np.array_equal(act.cpu().numpy(), hkey) and np.array_equal(fv.cpu().numpy(), hfv)
    # the log rows: math.log of the two row values, and nothing else
    if p > 0:
        la, lxy, lact, lfv = mc.ir_prepare(code, seed, off, B, p, use_log=True)
        hit, miss = 1.0 - p, p / (q - 1)
        lin, lg = xy.cpu().numpy(), lxy.cpu().numpy()
        assert set(np.unique(lg).tolist()) <= {math.log(hit), math.log(miss)}
        assert np.array_equal(lg == math.log(hit), lin == hit) or hit == miss
        assert np.array_equal(lg, np.where(lin == hit, math.log(hit), math.log(miss)))
        assert torch.equal(la, a) and torch.equal(lact, act) and torch.equal(lfv, fv)
    # two half batches at their offsets are the batch
    h = B // 2
    first, second = mc.ir_prepare(code, seed, off, h, p), mc.ir_prepare(code, seed, off + h, B - h, p)
    for whole, x0, x1 in zip((a, xy, act, fv), first, second):
        assert torch.equal(whole, torch.cat([x0, x1], dim=1))
    other = mc.ir_prepare(code, seed + 1, off, B, p)
    assert not torch.equal(other[0], a)


# -- pcub_ir_classify ----------------------------------------------------------------------------------
def device_verdicts(d):
    from polarcub_amd import mc
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("info", "prob", "size", "ap", "actual")}
    return mc.ir_classify(t["info"], t["prob"], t["size"], t["ap"], t["actual"], d["L"], results=True)


@pytest.mark.parametrize("use_log", [False, True])
@pytest.mark.parametrize("q,K,L", CLASSIFY_SHAPES)
def test_classify_on_crafted_lists(q, K, L, use_log):
    """The CPU test's lists (every branch of the verdict hit exactly, the key at two indices and past
    the size, size 1, metrics with 0 / -inf), B = 130: three groups of lanes, the last partial."""
    d = build_lists(q, K, L, 130, use_log, 17 * q + L)
    want, codes = host_verdicts(d)
    got, res = device_verdicts(d)
    assert got == want
    assert np.array_equal(res, codes)


def test_classify_without_information_symbols_and_long_lists():
    d = build_lists(3, 0, 6, 40, False, 5)
    want, codes = host_verdicts(d)
    got, res = device_verdicts(d)
    assert got == want and np.array_equal(res, codes)
    d = build_lists(4, 3, 70, 67, True, 9)  # lists longer than the workgroup's lanes, B = 64 + 3
    want, codes = host_verdicts(d)
    got, res = device_verdicts(d)
    assert got == want and np.array_equal(res, codes)


# -- pcub_mc_run_ir against the composed path -------------------------------------------------------
SHAPES = {  # q, n, L, p, K, trials, use_log
    "A": (3, 6, 9, 0.10, 34, 300, False),
    "B": (3, 6, 81, 0.12, 36, 120, False),
    "C": (2, 7, 8, 0.08, 70, 300, False),
    "Alog": (3, 6, 9, 0.10, 34, 300, True),
}
SEED = 20251020
_composed = {}


def composed(name):
    """prepare's buffers -> QaryListDecoder.decode_native -> _list_result and irSimulation's counting
    on the host; computed once a shape."""
    if name not in _composed:
        from polarcub_amd import mc, sc
        q, n, L, p, K, T, use_log = SHAPES[name]
        code, mask = make_code(q, n, K)
        _, xy, act, fv = mc.ir_prepare(code, SEED, 0, T, p, use_log=use_log)
        dec = sc.QaryListDecoder(q, 1 << n, mask, L, device="cuda", use_log=use_log)
        info, prob, size, ap = dec.decode_native(xy, fv, act)
        d = dict(B=T, L=L, info=info.cpu().numpy(), prob=prob.cpu().numpy(), size=size.cpu().numpy(),
                 ap=ap.cpu().numpy(), actual=act.cpu().numpy())
        _composed[name] = (code, host_verdicts(d))
    return _composed[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_run_ir_equals_the_composed_path(name):
    from polarcub_amd import mc
    q, n, L, p, K, T, use_log = SHAPES[name]
    code, (want, codes) = composed(name)
    got, res = mc.run_ir(code, SEED, 0, T, p, L, use_log=use_log, results=True)
    print(name, "counters", got)
    assert got == want
    assert np.array_equal(res, codes)
    assert got[0] == T and sum(got[4:]) == T and got[1] == sum(got[6:])
    bad, good = got[1], T - got[1]
    # the floors the shapes were chosen for (numpy-drawn trials of the same law on the CPU oracle gave
    # A: 231 / 41 / 0 / 0 / 5 / 22, B: 64 / 37 / 0 / 0 / 3 / 16, C: 209 / 13 / 13 / 8 / 8 / 49,
    # A in the log domain: 246 / 29 / 0 / 0 / 8 / 17)
    if name in ("A", "Alog"):
        assert bad >= 8 and good >= 100 and got[5] >= 10
    elif name == "B":
        assert bad >= 5 and got[5] >= 10
    else:
        assert bad >= 25 and sum(1 for r in range(6) if got[4 + r] > 0) >= 5


def test_shards_and_chunks_add_up():
    from polarcub_amd import mc
    q, n, L, p, K, T, _ = SHAPES["A"]
    code, (want, codes) = composed("A")
    c0, r0 = mc.run_ir(code, SEED, 0, 130, p, L, results=True)
    c1, r1 = mc.run_ir(code, SEED, 130, T - 130, p, L, results=True)
    assert [x + y for x, y in zip(c0, c1)] == want
    assert np.array_equal(np.concatenate([r0, r1]), codes)
    small, rs = mc.run_ir(code, SEED, 0, T, p, L, chunk=37, results=True)
    whole, rw = mc.run_ir(code, SEED, 0, T, p, L, chunk=300, results=True)
    assert small == whole == want
    assert np.array_equal(rs, codes) and np.array_equal(rw, codes)
    assert mc.run_ir(code, SEED, 0, T, p, L) == want  # no per-trial codes asked for


@pytest.mark.parametrize("name", ["A", "B"])
def test_smallest_workspace_gives_the_same_counters(name):
    """The chunk's buffers and one workgroup's slots of the list decoder (lane kernel: A, workgroup
    kernel: B): accepted, same counters; one byte less: refused."""
    from polarcub_amd import _lib, mc, sc
    q, n, L, p, K, T, _ = SHAPES[name]
    code, (want, codes) = composed(name)
    full, least = mc.ir_workspace_bytes(code, L, T)
    assert least < full
    got, res = mc.run_ir(code, SEED, 0, T, p, L, results=True, max_workspace_bytes=least)
    assert got == want and np.array_equal(res, codes)
    ws = torch.empty(least, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(10, dtype=torch.int64, device="cuda")
    rc = _lib.lib().pcub_mc_run_ir(SEED, 0, T, n, q, p, L, 0, sc._p(code.frozen_dev), K, T, sc._p(counters), None,
                                   sc._p(ws), least - 1, sc._stream())
    assert rc == _lib.EINVAL and counters.sum().item() == 0


# -- irSimulationDevice ------------------------------------------------------------------------------
def qsc_closures(q, N, p, chan_seed):
    """irSimulation's two closures for QSC(p): the channel and makeQSC's rows."""
    from polarcub_amd import vectors
    chan = random.Random(chan_seed)

    def simulate(a):
        return [(x + chan.randrange(1, q)) % q if chan.random() < p else x for x in a]

    def make_xy(b):
        vd = vectors.QaryMemorylessVectorDistribution(q, N)
        for i, y in enumerate(b):
            vd.probs[i] = [1.0 - p if x == y else p / (q - 1) for x in range(q)]
        return vd
    return simulate, make_xy


def test_ir_simulation_device(capsys):
    from polarcub_amd import coding_qary, mc
    q, n, L, p, K, T, _ = SHAPES["A"]
    N = 1 << n
    code, _ = composed("A")
    frozen = np.nonzero(code.frozen_mask)[0].tolist()
    fe, se, rate, prs = coding_qary.irSimulationDevice(q, N, p, T, frozen, maxListSize=L, seed=SEED, verbosity=1)
    c, codes = mc.run_ir(code, SEED, 0, T, p, L, results=True)
    assert fe == c[1] / T and se == c[2] / (T * N)
    assert rate == (math.log2(q) * K - math.log2(L)) / N
    assert prs == [coding_qary.ProbResult(int(v)) for v in codes]
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "Rate:  %s" % rate
    assert out[1] == "Frame error probability =  %d / %d  =  %s" % (c[1], T, fe)
    assert out[2] == "Symbol error probability =  %d / ( %d  *  %d ) =  %s" % (c[2], T, N, se)
    # the host irSimulation on the same law, shape and number of trials.  Both frame error counts are
    # binomial(T, r); their difference has variance 2 r (1 - r) / T, with r taken as the pooled rate.
    # At T = 300 and r near 0.09 the 4 sigma band is about +-0.09: it catches a wrong law (a pipeline
    # that never or nearly always fails), not a small bias.
    simulate, make_xy = qsc_closures(q, N, p, 5)
    hfe, _, hrate, hprs = coding_qary.irSimulation(q, N, simulate, make_xy, T, frozen, maxListSize=L)
    assert hrate == rate and len(hprs) == T
    r = (fe + hfe) / 2
    sigma = math.sqrt(2 * r * (1 - r) / T)
    print("device", fe, "host", hfe, "4 sigma", 4 * sigma)
    assert 0 < r < 1 and abs(fe - hfe) <= 4 * sigma
