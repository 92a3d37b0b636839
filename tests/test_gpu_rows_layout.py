"""The rows root layout on the GPU: pcub_sc_decode_bin_rows / pcub_sc_decode_qary_rows read the caller's
[B, N, 2] / [B, N, q] rows in place (BinaryDecoder.decode_rows_native, QaryDecoder.decode_rows_native).
Every output is compared word for word with the untiled kernels on the transposed rows, or with the
reference's stored decodes; the facade and the torch operators call the same entry points and hold no
second buffer of the batch's size."""
import numpy as np
import pytest

from tests.conftest import edge_long_cases, load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

VARIANTS = [0, 1, 10, 13, 14, 17, 24, 26, 30, 31, 33]


@pytest.fixture(scope="module")
def sc():
    from polarcub_amd import sc as _sc
    yield _sc
    _sc.set_variant()


_CODES = {}


def rate_half_code(sc, n):
    """The Bhattacharyya rate-1/2 code of test_batch_decode_through_tiles_matches_native (N = 1: the one
    position is information)."""
    if n not in _CODES:
        from polarcub_amd import construction
        N = 1 << n
        if n == 0:
            fr = np.zeros(1, np.uint8)
        else:
            fr = construction.bhattacharyya_frozen(n, N // 2, construction.awgn_sigma2(2.0, 0.5))
        _CODES[n] = sc.CodeSpec.from_frozen_set(N, set(np.nonzero(fr)[0].tolist()), 1, device="cuda")
    return _CODES[n]


def rand_rows(B, N, q, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.rand((B, N, q), dtype=torch.float64, device="cuda", generator=g)


def same_words(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def batches(sc, n):
    T = sc.bin_tile(n)
    Bs = {1, T - 1, T, T + 1, 197}
    if n <= 10:
        Bs.add(1000)
    if n == 13:
        Bs = {b for b in Bs if b <= 77} | {77}   # 10 MB of rows at the most
    return sorted(b for b in Bs if b > 0)


@pytest.mark.parametrize("n", [0, 1, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13])
def test_binary_rows_equal_untiled_kernel(sc, n):
    """The small kernels (n <= 5), the fallback variants (6..9) and the default variants with their rows
    twins (26 at n = 10, 11; 30 at 12; 33 at 13), at batches around the wave tile."""
    sc.set_variant()
    if n >= 10:
        assert sc.variant_for(n) == {10: 26, 11: 26, 12: 30, 13: 33}[n]
    code = rate_half_code(sc, n)
    dec = sc.BinaryDecoder(code)
    for B in batches(sc, n):
        xy = rand_rows(B, 1 << n, 2, n * 1000 + B)
        got = dec.decode_rows_native(xy, want_u=True)
        ref = dec.decode_native(sc.transpose_pairs(xy), want_u=True)
        assert same_words(got, ref), (n, B)


def smallest_n(sc, v):
    for n in range(6, 15):
        if sc.variant_for(n) == v:
            return n
    raise AssertionError("variant %d fits no code length up to 2^14" % v)


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_built_variant_reads_rows(sc, variant):
    from polarcub_amd import _lib
    L = _lib.lib()
    sc.set_variant(variant)
    old_tr, old_dyn = L.pcub_sc_set_tiled_root(1), sc.set_dynamic_tiles(1)
    try:
        n = smallest_n(sc, variant)
        code = rate_half_code(sc, n)
        dec = sc.BinaryDecoder(code)
        xy = rand_rows(37, 1 << n, 2, 7000 + variant)
        ref = dec.decode_native(sc.transpose_pairs(xy))
        for tr in (1, 0):
            for dyn in (1, 0):
                L.pcub_sc_set_tiled_root(tr)
                sc.set_dynamic_tiles(dyn)
                assert same_words(dec.decode_rows_native(xy), ref), (variant, n, tr, dyn)
    finally:
        L.pcub_sc_set_tiled_root(old_tr)
        sc.set_dynamic_tiles(old_dyn)
        sc.set_variant()


def test_rows_twin_load_forms_agree(sc):
    """Variant 26's rows twin with plain (the default) and with non-temporal root loads
    (pcub_sc_set_rows_nt)."""
    from polarcub_amd import _lib
    L = _lib.lib()
    sc.set_variant()
    code = rate_half_code(sc, 10)
    dec = sc.BinaryDecoder(code)
    xy = rand_rows(333, 1024, 2, 26)
    ref = dec.decode_native(sc.transpose_pairs(xy))
    old = L.pcub_sc_set_rows_nt(0)
    try:
        for nt in (0, 1):
            L.pcub_sc_set_rows_nt(nt)
            assert same_words(dec.decode_rows_native(xy), ref), nt
    finally:
        L.pcub_sc_set_rows_nt(old)


def test_persistent_loop_over_many_wave_tiles(sc):
    """N = 1024, B = 2000 in a workspace sized for two workgroups: the launcher clips the grid, so each
    workgroup strides over (or draws) many wave tiles."""
    from polarcub_amd import _lib
    from polarcub_amd.sc import _p, _stream
    L = _lib.lib()
    sc.set_variant()
    n, B = 10, 2000
    code = rate_half_code(sc, n)
    dec = sc.BinaryDecoder(code)
    xy = rand_rows(B, 1 << n, 2, 99)
    ref = dec.decode_native(sc.transpose_pairs(xy))
    per_wg = 256 // sc.variants()[sc.variant_for(n)][1]            # codewords a workgroup tile
    small = int(L.pcub_sc_decode_bin_workspace(2 * per_wg, n))     # two workgroups' slots
    assert 0 < small < int(L.pcub_sc_decode_bin_workspace(B, n))
    ws = torch.empty(small, dtype=torch.uint8, device="cuda")
    old_dyn = sc.set_dynamic_tiles(1)
    try:
        for dyn in (1, 0):
            sc.set_dynamic_tiles(dyn)
            info = torch.zeros_like(ref[0])
            xh = torch.zeros_like(ref[1])
            rc = L.pcub_sc_decode_bin_rows(_p(xy), B, n, _p(code.fmask_dev), _p(code.fval_dev), code.K, _p(info),
                                           _p(xh), None, _p(ws), ws.numel(), _stream())
            assert rc == 0
            assert torch.equal(info, ref[0]) and torch.equal(xh, ref[1]), dyn
    finally:
        sc.set_dynamic_tiles(old_dyn)


@pytest.mark.parametrize("n", [6, 10, 12])
def test_nothing_outside_the_rows_reaches_a_result(sc, n):
    """The batch in the middle of a (B + 2, N, 2) tensor whose first and last blocks are NaN: the decode
    of the view equals the decode of a tight copy (B = 17: the last wave tile is mostly padding lanes)."""
    sc.set_variant()
    B, N = 17, 1 << n
    big = torch.full((B + 2, N, 2), float("nan"), dtype=torch.float64, device="cuda")
    big[1:B + 1] = rand_rows(B, N, 2, 500 + n)
    view = big[1:B + 1]
    assert view.is_contiguous() and view.data_ptr() != big.data_ptr()
    dec = sc.BinaryDecoder(rate_half_code(sc, n))
    assert same_words(dec.decode_rows_native(view), dec.decode_rows_native(view.clone()))
    assert same_words(dec.decode_rows_native(view), dec.decode_native(sc.transpose_pairs(view)))


@pytest.mark.parametrize("name", ["bsc_n64", "awgn_n256_lowsnr", "awgn_n1024", "awgn_n4096"])
def test_reference_vectors_through_rows(sc, name):
    sc.set_variant()
    g = load_golden(name)
    xy = g["xy"] if "xy" in g else g["table"][g["y"]]
    N = g["frozen"].shape[0]
    code = sc.CodeSpec(N, g["frozen"], g["fval"])
    iw, xw, _ = sc.BinaryDecoder(code).decode_rows_native(torch.from_numpy(np.ascontiguousarray(xy)).cuda())
    assert np.array_equal(sc.unpack(iw, code.K).cpu().numpy(), g["info"])
    assert np.array_equal(sc.unpack(xw, N).cpu().numpy(), g["xhat"])


def test_edge_long_through_rows(sc):
    """All 40 cases of tests/golden/edge_long.npz (N = 1024, 4096) through the rows entry point."""
    sc.set_variant()
    cases = edge_long_cases()
    assert len(cases) == 40
    for c in cases:
        N = 1 << int(c["n"])
        code = sc.CodeSpec(N, c["frozen"], c["fval"])
        iw, xw, _ = sc.BinaryDecoder(code).decode_rows_native(torch.from_numpy(np.ascontiguousarray(c["xy"])).cuda())
        assert np.array_equal(sc.unpack(iw, code.K).cpu().numpy(), c["info"]), (N, c["family_name"])
        assert np.array_equal(sc.unpack(xw, N).cpu().numpy(), c["xhat"]), (N, c["family_name"])


# -- q-ary ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [2, 3, 4, 5, 8])
def test_qary_rows_equal_untiled_kernel(sc, q):
    for n in (2, 6, 8):
        rng = np.random.default_rng(10 * q + n)
        mask = (rng.random(1 << n) < 0.5).astype(np.uint8)
        dec = sc.QaryDecoder(sc.QaryCode(q, 1 << n, mask, device="cuda"))
        for B in (1, 15, 17, 333):
            xy = rand_rows(B, 1 << n, q, 100 * q + 10 * n + B)
            info, xh = dec.decode_rows_native(xy)
            i2, x2 = dec.decode_native(sc.transpose_pairs(xy))
            assert torch.equal(info, i2) and torch.equal(xh, x2), (q, n, B)


def test_qary_rows_twin_switch(sc):
    """The q = 4, N = 256 rows twin on and off (pcub_sc_set_qary_tiled_root), and generic in the code
    length (pcub_sc_set_fixed_n(0)): identical outputs."""
    from polarcub_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(4)
    mask = (rng.random(256) < 0.5).astype(np.uint8)
    dec = sc.QaryDecoder(sc.QaryCode(4, 256, mask, device="cuda"))
    xy = rand_rows(333, 256, 4, 44)
    ref = dec.decode_native(sc.transpose_pairs(xy))
    old_tr, old_fn = L.pcub_sc_set_qary_tiled_root(1), L.pcub_sc_set_fixed_n(1)
    try:
        for tr, fn in ((1, 1), (1, 0), (0, 1)):
            L.pcub_sc_set_qary_tiled_root(tr)
            L.pcub_sc_set_fixed_n(fn)
            got = dec.decode_rows_native(xy)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (tr, fn)
    finally:
        L.pcub_sc_set_qary_tiled_root(old_tr)
        L.pcub_sc_set_fixed_n(old_fn)


def test_qary_reference_vectors_through_rows(sc):
    g = load_golden("qsc_q4_n256")
    dec = sc.QaryDecoder(sc.QaryCode(4, 256, g["frozen"], device="cuda"))
    info, xh = dec.decode_rows_native(torch.from_numpy(np.ascontiguousarray(g["table"][g["y"]])).cuda())
    assert np.array_equal(info.t().cpu().numpy(), g["info"])
    assert xh.shape == (256, g["info"].shape[0])
    info_r, _ = dec.decode_rows_native(torch.from_numpy(g["xy_rand"]).cuda())
    assert np.array_equal(info_r.t().cpu().numpy(), g["info_rand"])


def test_qary_nothing_outside_the_rows_reaches_a_result(sc):
    q, n, B = 4, 8, 17
    rng = np.random.default_rng(8)
    mask = (rng.random(1 << n) < 0.5).astype(np.uint8)
    dec = sc.QaryDecoder(sc.QaryCode(q, 1 << n, mask, device="cuda"))
    big = torch.full((B + 2, 1 << n, q), float("nan"), dtype=torch.float64, device="cuda")
    big[1:B + 1] = rand_rows(B, 1 << n, q, 48)
    view = big[1:B + 1]
    a, b = dec.decode_rows_native(view), dec.decode_rows_native(view.clone())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = dec.decode_native(sc.transpose_pairs(view))
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


# -- callers -------------------------------------------------------------------------------------------
def sc_pack(bits):
    """[N] 0/1 -> int32 [ceil(N/32)] words (bit i of word i // 32)"""
    from polarcub_amd.sc import pack_rows
    return pack_rows(np.asarray(bits, np.uint8)).reshape(-1).view(np.int32).copy()


def test_callers_run_the_rows_entry_points(sc):
    """BinaryDecoder.decode, QaryDecoder.decode and the four torch operators against the rows entry
    points called directly."""
    from polarcub_amd import ops
    sc.set_variant()
    rng = np.random.default_rng(12)
    N, B = 1024, 300
    frozen = (rng.random(N) < 0.5).astype(np.uint8)
    fval = (rng.random(N) < 0.5).astype(np.uint8) & frozen
    code = sc.CodeSpec(N, frozen, fval)
    dec = sc.BinaryDecoder(code)
    xy = rand_rows(B, N, 2, 1212)
    iw, xw, _ = dec.decode_rows_native(xy)
    info, xhat = sc.unpack(iw, code.K), sc.unpack(xw, N)
    fi, fx = dec.decode(xy)
    assert torch.equal(fi, info) and torch.equal(fx, xhat)
    oi, ox = ops.sc_decode_bin_f64(xy, frozen, fval)
    assert torch.equal(oi, info) and torch.equal(ox, xhat)
    li, lx, lm = ops.sc_decode_bin_f64(xy, frozen, fval, leaf_m=True)
    assert torch.equal(li, info) and torch.equal(lx, xhat) and lm.shape == xy.shape
    wi, wx = ops.sc_decode_bin_words(xy, torch.from_numpy(sc_pack(frozen)).cuda(),
                                     torch.from_numpy(sc_pack(fval)).cuda(), code.K)
    assert torch.equal(wi, info) and torch.equal(wx, xhat)
    q, Nq = 4, 256
    mask = (rng.random(Nq) < 0.5).astype(np.uint8)
    qdec = sc.QaryDecoder(sc.QaryCode(q, Nq, mask, device="cuda"))
    xq = rand_rows(B, Nq, q, 1313)
    qi, qx = qdec.decode_rows_native(xq)
    di, dx = qdec.decode(xq)
    assert torch.equal(di, qi.t().contiguous()) and torch.equal(dx, qx.t().contiguous())
    pi, px = ops.sc_decode_qary_f64(q, xq, mask)
    assert torch.equal(pi, di) and torch.equal(px, dx)


def test_words_op_still_replays_from_a_graph(sc):
    """tests/test_torch_ops.py's capture pattern on the rows path."""
    from polarcub_amd import ops
    g = load_golden("awgn_n1024")
    xy = torch.from_numpy(g["xy"]).cuda()
    K = int((g["frozen"] == 0).sum())
    fw, vw = torch.from_numpy(sc_pack(g["frozen"])).cuda(), torch.from_numpy(sc_pack(g["fval"])).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sc_decode_bin_words(xy, fw, vw, K)  # warm the caching allocator on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gi, gx = ops.sc_decode_bin_words(xy, fw, vw, K)
    xy.copy_(torch.from_numpy(g["xy"][::-1].copy()).cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(gi.cpu().numpy(), g["info"][::-1])
    assert np.array_equal(gx.cpu().numpy(), g["xhat"][::-1])


def test_no_second_buffer_of_the_batch(sc):
    """N = 1024, K = 512, B = 4096: a contiguous input of 64 MiB (16 KiB a codeword).  After a warm-up
    call of the same B, one call may raise the peak of allocated device memory by
      * BinaryDecoder.decode: the packed outputs (16 + 32 words = 192 B a codeword) and the unpacked ones
        (512 + 1024 B), 1728 B a codeword = 6.75 MiB, the workspace being cached in the decoder:
        less than half the input's bytes (a staging buffer alone is all of them);
      * sc_decode_bin_f64: the same outputs, the two mask word tensors, and its workspace, allocated per
        call -- 64 resident workgroups x 256 slots x 1 KiB of stored levels + tables = 16 MiB and a
        little: 23 MiB, less than the input's bytes (with a staging buffer: 64 MiB more)."""
    from polarcub_amd import ops
    sc.set_variant()
    n, B = 10, 4096
    code = rate_half_code(sc, n)
    assert code.K == 512
    xy = rand_rows(B, 1 << n, 2, 4096)
    nbytes = xy.numel() * xy.element_size()
    assert nbytes == 64 << 20
    dec = sc.BinaryDecoder(code)
    fm, fv = code.frozen_mask, code.frozen_values

    def rise(fn):
        out = fn()  # warm-up: the decoder's workspace, the allocator's pools
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out
        return peak

    r_facade = rise(lambda: dec.decode(xy))
    r_op = rise(lambda: ops.sc_decode_bin_f64(xy, fm, fv))
    print("peak rise: facade %d B, op %d B, input %d B" % (r_facade, r_op, nbytes))
    assert r_facade < nbytes // 2
    assert r_op < nbytes


def test_edge_arguments(sc):
    from polarcub_amd import _lib
    from polarcub_amd.sc import _p, _stream
    L = _lib.lib()
    sc.set_variant()
    n = 10
    code = rate_half_code(sc, n)
    xy = rand_rows(1, 1 << n, 2, 1)
    need = int(L.pcub_sc_decode_bin_workspace(1, n))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    info = torch.full((code.info_words, 1), -1, dtype=torch.int32, device="cuda")

    def call(xy_p, B, log2N, wsb):
        return L.pcub_sc_decode_bin_rows(xy_p, B, log2N, _p(code.fmask_dev), _p(code.fval_dev), code.K, _p(info),
                                         None, None, _p(ws), wsb, _stream())

    assert call(_p(xy), 0, n, need) == 0
    torch.cuda.synchronize()
    assert bool((info == -1).all())                 # B = 0: nothing launched, nothing written
    assert call(None, 1, n, need) == _lib.EINVAL
    assert call(_p(xy), 1, 25, need) == _lib.EINVAL
    assert call(_p(xy), 1, n, need - 1) == _lib.EINVAL
    assert call(_p(xy), 1, n, need) == 0
    torch.cuda.synchronize()
    assert not bool((info == -1).all())
    q = sc.QaryCode(4, 256, np.zeros(256, np.uint8), device="cuda")
    qneed = int(L.pcub_sc_decode_qary_workspace(1, 8, 4))
    qws = torch.empty(qneed, dtype=torch.uint8, device="cuda")
    qxy = rand_rows(1, 256, 4, 2)
    qinfo = torch.empty((256, 1), dtype=torch.uint8, device="cuda")

    def qcall(xy_p, B, log2N, wsb):
        return L.pcub_sc_decode_qary_rows(xy_p, B, log2N, 4, _p(q.frozen_dev), q.K, _p(qinfo), None, _p(qws), wsb,
                                          _stream())

    assert qcall(_p(qxy), 0, 8, qneed) == 0
    assert qcall(None, 1, 8, qneed) == _lib.EINVAL
    assert qcall(_p(qxy), 1, 21, qneed) == _lib.EINVAL
    assert qcall(_p(qxy), 1, 8, qneed - 1) == _lib.EINVAL
    assert qcall(_p(qxy), 1, 8, qneed) == 0
    torch.cuda.synchronize()
