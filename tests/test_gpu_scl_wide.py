"""q-ary list decoding above L = 64 on the GPU (k_scl_wg: a workgroup a codeword, lanes over paths
and candidates): the reference's own runs at L = 81 .. 4096 (tests/golden/scl_wide.npz) bit for bit in
the linear domain, the workgroup kernel against the lane kernel at L <= 64 (pcub_scl_set_layout),
the persistent loop, the argument edges and the irSimulation facade."""
import numpy as np
import pytest

from oracle import scl_oracle as so
from tests.conftest import load_golden
from tests.test_scl import _random_inputs, ir_closures
from tests.test_scl_wide import check_against_fixture, wide_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    from polarcub_amd import _lib, sc as m
    _lib.lib()
    return m


@pytest.mark.parametrize("case", range(10))
def test_gpu_wide_list_decoder_matches_reference(sc, case):
    """Every fixture case through QaryListDecoder.decode under the default dispatch: linear domain,
    the path set, the metrics and actual_prob equal the reference's bit for bit; log domain within
    _close_log.  The ProbResult of coding_qary's listDecode equals the recorded one."""
    from polarcub_amd import coding_qary, vectors
    g = load_golden("scl_wide")
    c = wide_cases()[case]
    t_, q, L, N = c["tag"], c["q"], c["L"], 1 << c["n"]
    assert L > 64
    info, prob, size, ap = sc.QaryListDecoder(q, N, g[t_ + "_frozen"], L, use_log=c["use_log"]).decode(
        g[t_ + "_xy"], g[t_ + "_fv"], g[t_ + "_actual"])
    T = g[t_ + "_xy"].shape[0]
    for t in range(T):
        check_against_fixture(g, c, t, int(size[t]), info[t], prob[t], ap[t])
    frozen = set(int(i) for i in np.nonzero(g[t_ + "_frozen"])[0])
    enc = coding_qary.QaryPolarEncoderDecoder(q, N, frozen, 1, use_log=c["use_log"])
    for t in range(T):
        vd = vectors.QaryMemorylessVectorDistribution(q, N, use_log=c["use_log"])
        vd.probs[:] = g[t_ + "_xy"][t]
        word, pr = enc.listDecode(vd, g[t_ + "_fv"][t], L, np.zeros((enc.k, 0), np.int64), np.zeros(0, np.int64),
                                  actualInformation=g[t_ + "_actual"][t])
        assert pr.name == c["prob_result"][t]
        if pr.name.startswith("Success"):
            assert np.array_equal(word, g[t_ + "_actual"][t])


@pytest.mark.parametrize("L", [1, 2, 8, 64])
@pytest.mark.parametrize("n", [3, 5, 8])
@pytest.mark.parametrize("q", [2, 3, 4, 8])
def test_gpu_workgroup_layout_equals_lane_layout(sc, q, n, L):
    """set_scl_layout(2) (the workgroup kernel) against set_scl_layout(1) (the lane kernel) at
    L <= 64, B = 5 with an actual path, tie-free and tied (QSC) rows, linear and log domain: info,
    prob, size and actual_prob identical (torch.equal) -- both kernels call the same device functions
    in the same order per path, ties included.
    Inputs as tests/test_scl.py::_random_inputs, a random frozen set of rate 1/2 at n = 3, 5 and of
    rate 3/4 at n = 8: the lane kernel's serial prune costs L^2 q^3 steps a single-parity-check
    fork, and a rate-1/2 set at N = 256 has 17 such nodes (10 s a call at q = 8, L = 64) where the
    rate-3/4 set has one or two beside its rate-1, repetition and rate-0 nodes (3.5 s a lane call
    there, 14 s for that case's four; the workgroup kernel's calls take milliseconds)."""
    import torch
    N = 1 << n
    try:
        for ties in (False, True):
            rng = np.random.default_rng(1000 * q + 10 * n + L + ties)
            frozen, xy, fv, act = _random_inputs(rng, q, n, 5, ties)
            if n == 8:
                frozen = (rng.random(N) < 0.75).astype(np.uint8)
                K = int((frozen == 0).sum())
                fv, act = rng.integers(0, q, (5, N - K)), rng.integers(0, q, (5, K))
            for use_log in (False, True):
                x = torch.from_numpy(np.ascontiguousarray((np.log(xy) if use_log else xy).transpose(1, 0, 2))).cuda()
                f = torch.from_numpy(np.ascontiguousarray(fv.astype(np.uint8).T)).cuda()
                a = torch.from_numpy(np.ascontiguousarray(act.astype(np.uint8).T)).cuda()
                if f.shape[0] == 0:
                    f = torch.zeros((1, 5), dtype=torch.uint8, device="cuda")
                out = []
                for mode in (1, 2):
                    sc.set_scl_layout(mode)
                    dec = sc.QaryListDecoder(q, N, frozen, L, use_log=use_log)
                    out.append(dec.decode_native(x, f, a))
                    torch.cuda.synchronize()
                (i1, p1, s1, a1), (i2, p2, s2, a2) = out
                assert torch.equal(s1, s2), (ties, use_log)
                assert torch.equal(i1, i2), (ties, use_log)
                assert torch.equal(p1.view(torch.int64), p2.view(torch.int64)), (ties, use_log)
                assert torch.equal(a1.view(torch.int64), a2.view(torch.int64)), (ties, use_log)
    finally:
        sc.set_scl_layout(0)


def test_gpu_set_layout_modes(sc):
    """The hook returns the previous mode, rejects other values, and mode 1 refuses L > 64."""
    from polarcub_amd import _lib
    try:
        assert sc.set_scl_layout(2) == 0
        assert sc.set_scl_layout(1) == 2
        with pytest.raises(ValueError):
            sc.set_scl_layout(3)
        assert _lib.lib().pcub_scl_set_layout(-1) == -1
        assert _lib.lib().pcub_scl_qary_workspace(4, 3, 4, 81, 8) == 0  # the lane kernel cannot take L = 81
        assert sc.set_scl_layout(0) == 1
    finally:
        sc.set_scl_layout(0)


def test_gpu_wide_persistent_loop(sc):
    """(3, 5, 81), B = 7 with the workspace capped to two slots: two workgroups stride over the seven
    codewords, and every codeword equals its single decode."""
    import torch
    from polarcub_amd import _lib
    q, n, L, B = 3, 5, 81, 7
    N = 1 << n
    rng = np.random.default_rng(81)
    frozen, xy, fv, act = _random_inputs(rng, q, n, B, False)
    K = N - int(frozen.sum())
    one = int(_lib.lib().pcub_scl_qary_workspace(1, q, n, L, K))
    two = int(_lib.lib().pcub_scl_qary_workspace(2, q, n, L, K))
    assert one < two < 2 * one
    x = torch.from_numpy(np.ascontiguousarray(xy.transpose(1, 0, 2))).cuda()
    f = torch.from_numpy(np.ascontiguousarray(fv.astype(np.uint8).T)).cuda()
    a = torch.from_numpy(np.ascontiguousarray(act.astype(np.uint8).T)).cuda()
    dec = sc.QaryListDecoder(q, N, frozen, L)
    info, prob, size, ap = dec.decode_native(x, f, a, max_workspace_bytes=two)
    torch.cuda.synchronize()
    assert dec._ws.numel() <= two
    for b in range(B):
        i1, p1, s1, a1 = sc.QaryListDecoder(q, N, frozen, L).decode_native(
            x[:, b:b + 1].contiguous(), f[:, b:b + 1].contiguous(), a[:, b:b + 1].contiguous())
        assert torch.equal(size[b:b + 1], s1) and torch.equal(info[:, :, b:b + 1], i1)
        assert torch.equal(prob[:, b:b + 1], p1) and torch.equal(ap[b:b + 1], a1)
    k, oinfo, oprob, oap = so.list_decode(q, frozen, L, xy[B - 1], fv[B - 1], act[B - 1])
    assert int(size[B - 1]) == k and info[:k, :, B - 1].cpu().numpy().tolist() == oinfo
    assert np.array_equal(prob[:k, B - 1].cpu().numpy(), np.array(oprob)) and float(ap[B - 1]) == oap


def test_gpu_wide_argument_edges(sc):
    """L = 65 and L = 4096 are accepted, L = 4097 is not; K = 0 and K = N decode above L = 64; no
    workspace that holds a slot is PCUB_EINVAL."""
    import torch
    from polarcub_amd import _lib
    L_ = _lib.lib()
    rng = np.random.default_rng(65)
    q, n = 2, 4
    N = 1 << n
    frozen, xy, fv, act = _random_inputs(rng, q, n, 3, False)
    for L in (65, 4096):
        info, prob, size, ap = sc.QaryListDecoder(q, N, frozen, L).decode(xy, fv, act)
        for b in range(3):
            k, oinfo, oprob, oap = so.list_decode(q, frozen, L, xy[b], fv[b], act[b])
            assert size[b] == k and info[b][:k].tolist() == oinfo
            assert np.array_equal(prob[b][:k], np.array(oprob)) and ap[b] == oap
    with pytest.raises(ValueError, match="4096"):
        sc.QaryListDecoder(q, N, frozen, 4097)
    assert L_.pcub_scl_qary_workspace(3, q, n, 4097, 8) == 0
    assert L_.pcub_scl_qary_workspace(3, q, n, 4096, 8) > 0
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    rc = L_.pcub_scl_qary(None, 3, q, n, 4097, None, None, 8, None, 8, None, None, None, None, ws.data_ptr(),
                          ws.numel(), None)
    assert rc == _lib.EINVAL
    # K = 0 (one rate-0 node) and K = N (one rate-1 node) at L = 100
    for mask in (np.ones(N, np.uint8), np.zeros(N, np.uint8)):
        K = N - int(mask.sum())
        f0 = rng.integers(0, q, (3, N - K))
        a0 = rng.integers(0, q, (3, K)) if K else None  # no information: no actual word to follow
        info, prob, size, ap = sc.QaryListDecoder(q, N, mask, 100).decode(xy, f0, a0)
        for b in range(3):
            k, oinfo, oprob, oap = so.list_decode(q, mask, 100, xy[b], f0[b], None if a0 is None else a0[b])
            assert size[b] == k and info[b][:k].tolist() == oinfo
            assert np.array_equal(prob[b][:k], np.array(oprob))
            assert a0 is None or ap[b] == oap
    # a workspace smaller than one slot
    dec = sc.QaryListDecoder(q, N, frozen, 128)
    x = torch.from_numpy(np.ascontiguousarray(xy.transpose(1, 0, 2))).cuda()
    f = torch.from_numpy(np.ascontiguousarray(fv.astype(np.uint8).T)).cuda()
    info = torch.empty((128, dec.K, 3), dtype=torch.uint8, device="cuda")
    prob = torch.empty((128, 3), dtype=torch.float64, device="cuda")
    size = torch.empty(3, dtype=torch.int32, device="cuda")
    rc = L_.pcub_scl_qary(x.data_ptr(), 3, q, n, 128, dec.frozen_dev.data_ptr(), f.data_ptr(), dec.nF, None, dec.K,
                          info.data_ptr(), prob.data_ptr(), size.data_ptr(), None, ws.data_ptr(), 4096, None)
    assert rc == _lib.EINVAL


def test_gpu_lane_workspace_unchanged(sc):
    """pcub_scl_qary_workspace at L <= 64 under mode 0: the values of the lane kernel's slot-minor
    slab before the workgroup kernel existed (64 slots a workgroup; batches of one and two
    workgroups, so the values do not depend on the device's CU count)."""
    from polarcub_amd import _lib
    L_ = _lib.lib()
    assert sc.set_scl_layout(0) == 0
    for args, want in (((1, 4, 8, 8, 128), 6410768), ((64, 2, 5, 64, 16), 3789328), ((100, 3, 4, 16, 9), 2133008),
                       ((1, 8, 3, 1, 0), 628880), ((128, 4, 12, 32, 2048), 656262160)):
        assert L_.pcub_scl_qary_workspace(*args) == want, args


def test_gpu_wide_ir_simulation_matches_oracle(sc, monkeypatch, capsys):
    """irSimulation at q = 3, N = 16, maxListSize = 81 on the device equals the same call with
    list_decode_batch replaced by the Python oracle (frame errors, symbol errors, rate, ProbResults,
    printed lines): the inputs are tie-free, so the lists agree in order too."""
    from polarcub_amd import coding_qary
    g = load_golden("scl")
    r = dict(g["meta"]["ir"][0])
    assert r["q"] == 3 and r["n"] == 4
    frozen = set(int(i) for i in np.nonzero(g[r["name"] + "_frozen"])[0])
    trials = 12

    def run():
        simulate, make_xy = ir_closures(r)
        np.random.seed(r["np_seed"])
        out = coding_qary.irSimulation(3, 16, simulate, make_xy, trials, frozen, 81, r["check_size"], verbosity=1)
        return out, capsys.readouterr().out

    (fe, se, rate, prl), printed = run()

    def oracle_batch(self, xy, fvals, L, actual):
        B = xy.shape[0]
        info = np.full((B, L, self.k), -1, np.int64)
        prob = np.zeros((B, L))
        size = np.zeros(B, np.int64)
        ap = np.zeros(B)
        for b in range(B):
            k, inf, p, a = so.list_decode(self.q, self._mask, L, xy[b], fvals[b], actual[b])
            size[b], ap[b] = k, a
            info[b, :k] = inf
            prob[b, :k] = p
        return info, prob, size, ap
    monkeypatch.setattr(coding_qary.QaryPolarEncoderDecoder, "list_decode_batch", oracle_batch)
    (ofe, ose, orate, oprl), oprinted = run()
    assert (fe, se, rate) == (ofe, ose, orate)
    assert [p.name for p in prl] == [p.name for p in oprl]
    assert printed == oprinted
