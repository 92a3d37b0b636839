"""q-ary SC on the GPU against the reference's golden vectors (bit-exact symbols)."""
import numpy as np
import pytest

from tests.conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LANES = [1, 2, 4, 8, 16]  # lanes per codeword of the q-ary kernel (8, 16: q = 4 only, else 4)


@pytest.fixture(params=LANES)
def lanes(request):
    from polarcub_amd import sc
    old = sc.set_qary_lanes(request.param)
    yield request.param
    sc.set_qary_lanes(old)


@pytest.mark.parametrize("lds,hl", [(True, True), (True, False), (False, False)])
def test_qsc_q4_n256_matches_reference(lanes, lds, hl):
    """lds: the re-encoded symbols in LDS (the C4 kernel's default) or in the workspace; hl: the
    split last level (default with the symbols in LDS at G = 4) or not."""
    from polarcub_amd import sc
    old_lds = sc.set_qary_lds(lds)
    old_hl = sc.set_qary_hl(hl)
    g = load_golden("qsc_q4_n256")
    code = sc.QaryCode(4, 256, g["frozen"])
    dec = sc.QaryDecoder(code)
    info, xhat = dec.decode(torch.from_numpy(g["table"][g["y"]]).cuda())
    assert np.array_equal(info.cpu().numpy(), g["info"])
    info_r, _ = dec.decode(torch.from_numpy(g["xy_rand"]).cuda())
    assert np.array_equal(info_r.cpu().numpy(), g["info_rand"])
    # x_hat re-encodes the decoded symbols
    enc = sc.encode_qary(code, info)
    assert torch.equal(enc, xhat)
    sc.set_qary_lds(old_lds)
    sc.set_qary_hl(old_hl)


def test_qary_q3_matches_reference(lanes):
    from polarcub_amd import sc
    g = load_golden("qary_q3_n32")
    code = sc.QaryCode(3, 32, g["frozen"])
    info, _ = sc.QaryDecoder(code).decode(torch.from_numpy(g["xy"]).cuda())
    assert np.array_equal(info.cpu().numpy(), g["info"])
    x = sc.encode_qary(code, torch.from_numpy(g["enc_info"]).cuda())
    assert np.array_equal(x.cpu().numpy(), g["enc_x"])


def test_qary_encode_matches_reference():
    from polarcub_amd import sc
    g = load_golden("qsc_q4_n256")
    code = sc.QaryCode(4, 256, g["frozen"])
    x = sc.encode_qary(code, torch.from_numpy(g["tx_info"]).cuda())
    assert np.array_equal(x.cpu().numpy(), g["x"])


@pytest.mark.parametrize("q", [2, 3, 4, 5, 6, 7, 8])
def test_qary_random_vs_oracle(q, lanes):
    from oracle import orc
    from polarcub_amd import sc
    rng = np.random.default_rng(q)
    for N, B in [(4, 7), (16, 33), (64, 300), (512, 1000)]:
        frozen = (rng.random(N) < 0.4).astype(np.uint8)
        frozen[N // 2: N // 2 + N // 8] = 1  # an aligned rate-0 block
        xy = rng.random((B, N, q))
        xy[rng.random((B, N)) < 0.05] = 0.0
        code = sc.QaryCode(q, N, frozen)
        info, xhat = sc.QaryDecoder(code).decode(torch.from_numpy(xy).cuda())
        ri, rx = orc.decode_qary(q, xy, frozen)
        assert np.array_equal(info.cpu().numpy(), ri), (q, N)
        assert np.array_equal(xhat.cpu().numpy(), rx), (q, N)


def test_qary_facade_decode():
    from polarcub_amd import coding_qary, scalar_qary
    g = load_golden("qsc_q4_n256")
    fs = set(int(i) for i in np.nonzero(g["frozen"])[0])
    encdec = coding_qary.QaryPolarEncoderDecoder(4, 256, fs, 1)
    qsc = scalar_qary.makeQSC(4, 0.11)
    xq = scalar_qary.QaryMemorylessDistribution(4)
    xq.probs = [qsc.calcXMarginals()]
    xvd = xq.makeQaryMemorylessVectorDistribution(256, None)
    for t in range(0, 160, 20):
        yvd = qsc.makeQaryMemorylessVectorDistribution(256, [int(v) for v in g["y"][t]])
        info = encdec.decode(xvd, yvd)
        assert info.dtype == np.int64 and np.array_equal(info, g["info"][t])
    assert np.array_equal(encdec.encode(xvd, list(g["tx_info"][0])), g["x"][0])


@pytest.mark.parametrize("q", [2, 3, 4, 8])
def test_tiled_root_layout_qary(q):
    """pcub_sc_decode_qary_tiled: the rows in tiles of T codewords (the native width, 1, 5) decode
    exactly as the [N, B, q] rows, ragged last tiles included."""
    import torch
    from polarcub_amd import sc
    rng = np.random.default_rng(40 + q)
    for N, B in [(16, 50), (256, 333)]:
        frozen = (rng.random(N) < 0.5).astype(np.uint8)
        code = sc.QaryCode(q, N, frozen, device="cuda")
        dec = sc.QaryDecoder(code)
        xy = rng.random((N, B, q))
        native = torch.from_numpy(xy).cuda()
        ri, rx = dec.decode_native(native)
        for T in sorted({dec.tile(), 1, 5}):
            ti, tx = dec.decode_tiled_native(sc.tile_rows(native, T), B)
            assert torch.equal(ti, ri) and torch.equal(tx, rx), (N, T)


def test_qary_rate1_blocks(lanes):
    """q = 4 codes with aligned all-information (rate-1) blocks of 4..64 positions: QSC-like rows
    from near-certain to noisy, exact ties, near ties, zero and uniform rows in the same waves,
    against the oracle.  (A rate-1 shortcut like the binary kernel's measured 90.0 -> 86.3 M cw/s at
    C4 and is not built; this pins the recursion on the inputs it would have taken.)"""
    from oracle import orc
    from polarcub_amd import sc
    q = 4
    rng = np.random.default_rng(77 + lanes)
    for N, B in [(16, 200), (64, 400), (256, 700), (1024, 150)]:
        frozen = (rng.random(N) < 0.5).astype(np.uint8)
        w = max(N // 4, 4)
        while w >= 4:
            s = int(rng.integers(N // (2 * w), N // w)) * w
            frozen[s:s + w] = 0
            w //= 2
        frozen[: N // 8] = 1
        p = rng.choice([0.0005, 0.01, 0.11, 0.4], size=(B, 1, 1), p=[0.3, 0.3, 0.3, 0.1])
        sym = rng.integers(0, q, (B, N))
        xy = np.broadcast_to(p / (q - 1), (B, N, q)).copy()
        np.put_along_axis(xy, sym[..., None], np.broadcast_to(1.0 - p, (B, N, 1)), axis=-1)
        flip = rng.random((B, N)) < 0.05
        xy[flip] = rng.random((int(flip.sum()), q))
        tie = rng.random((B, N)) < 0.003
        xy[tie, 1] = xy[tie, 0] = 0.45
        near = rng.random((B, N)) < 0.003
        xy[near, 2] = np.nextafter(xy[near, 3], 2.0)
        xy[rng.random((B, N)) < 0.002] = 0.0
        xy[rng.random((B, N)) < 0.002] = 0.25
        code = sc.QaryCode(q, N, frozen)
        info, xhat = sc.QaryDecoder(code).decode(torch.from_numpy(xy).cuda())
        ri, rx = orc.decode_qary(q, xy, frozen)
        assert np.array_equal(info.cpu().numpy(), ri), (N, lanes)
        assert np.array_equal(xhat.cpu().numpy(), rx), (N, lanes)


def _decode_qary_c(sc, code, native, ws_bytes):
    """pcub_sc_decode_qary on [N, B, q] rows with a workspace of exactly ws_bytes bytes."""
    from polarcub_amd import _lib
    B = native.shape[1]
    info = torch.zeros((max(1, code.K), B), dtype=torch.uint8, device="cuda")
    xh = torch.zeros((code.N, B), dtype=torch.uint8, device="cuda")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rc = _lib.lib().pcub_sc_decode_qary(sc._p(native), B, code.n, code.q, sc._p(code.frozen_dev), code.K, sc._p(info),
                                        sc._p(xh), sc._p(ws), ws.numel(), sc._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return info[:code.K].t().contiguous(), xh.t().contiguous()


@pytest.mark.parametrize("q,N", [(4, 256), (3, 64)])
def test_qary_tile_loop_both_schedulers(q, N):
    """1,007 codewords with the workspace for one codeword (the launcher clamps the grid to one workgroup,
    which goes over every wave tile, the last one ragged) and with the workspace for all of them, the
    tiles from the per-launch counter and on the static stride: all four equal the oracle.  At q = 4,
    N = 256 (the C4 kernel) also three rounds of the full grid plus five codewords, 256 distinct rows
    repeated in a shuffled order."""
    from oracle import orc
    from polarcub_amd import _lib, sc
    n = N.bit_length() - 1
    B = 1000 + 7
    rng = np.random.default_rng(900 + q)
    frozen = (rng.random(N) < 0.4).astype(np.uint8)
    frozen[N // 2: N // 2 + N // 8] = 1
    xy = rng.random((B, N, q))
    xy[rng.random((B, N)) < 0.05] = 0.0
    ri, rx = orc.decode_qary(q, xy, frozen)
    code = sc.QaryCode(q, N, frozen, device="cuda")
    native = torch.from_numpy(np.ascontiguousarray(xy.transpose(1, 0, 2))).cuda()
    L = _lib.lib()
    one, full = int(L.pcub_sc_decode_qary_workspace(1, n, q)), int(L.pcub_sc_decode_qary_workspace(B, n, q))
    assert 0 < one < full
    old = sc.set_dynamic_tiles(1)
    try:
        for dyn in (1, 0):
            sc.set_dynamic_tiles(dyn)
            for ws in (one, full):
                info, xhat = _decode_qary_c(sc, code, native, ws)
                assert np.array_equal(info.cpu().numpy(), ri), (dyn, ws)
                assert np.array_equal(xhat.cpu().numpy(), rx), (dyn, ws)
            if (q, N) == (4, 256):
                dec = sc.QaryDecoder(code)
                cwb = 4 * dec.tile()  # codewords a workgroup of four waves
                # the grid the launcher saturates at, from its workspace: one workgroup's slots are what a
                # second tile adds
                per_wg = int(L.pcub_sc_decode_qary_workspace(cwb + 1, n, q)) - one
                grid = (int(L.pcub_sc_decode_qary_workspace(1 << 22, n, q)) - one) // per_wg + 1
                assert grid >= torch.cuda.get_device_properties(0).multi_processor_count
                Bg = 3 * grid * cwb + 5
                order = np.concatenate([rng.permutation(256) for _ in range(Bg // 256 + 1)])[:Bg]
                idx = torch.from_numpy(order).cuda()
                gi, gx = dec.decode_native(native[:, :256].index_select(1, idx))
                torch.cuda.synchronize()
                assert torch.equal(gi.t(), torch.from_numpy(ri[:256]).cuda().index_select(0, idx)), dyn
                assert torch.equal(gx.t(), torch.from_numpy(rx[:256]).cuda().index_select(0, idx)), dyn
    finally:
        sc.set_dynamic_tiles(old)
