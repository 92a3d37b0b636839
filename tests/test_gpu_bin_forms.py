"""Every kernel of the library's list of built binary decode kernels (sc_bin_kern.h's kBinBuilt, walked
through pcub_sc_bin_form_built) launched once through its entry point: each form decodes exactly what
the same variant's Pairs kernel decodes on the same codewords, and the Pairs kernel what the oracle
decodes."""
import numpy as np
import pytest

from tests.test_bin_forms import BUILT, COMPACT, FORMS, PAIRS, ROWS, ROWS_NT, TILED, TILED_COMPACT
from tests.test_gpu_rows_layout import rate_half_code, same_words, smallest_n

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B = 37  # no multiple of a wave tile (64, 16 or 8 codewords): the padding lanes of the last tile run
SMALLEST_N = {0: 6, 13: 7, 24: 8, 26: 9, 31: 9, 30: 10, 33: 10}


@pytest.fixture()
def sc():
    from polarcub_amd import _lib, sc as _sc
    L = _lib.lib()
    old_tr, old_nt = L.pcub_sc_set_tiled_root(1), L.pcub_sc_set_rows_nt(0)
    yield _sc
    L.pcub_sc_set_tiled_root(old_tr)
    L.pcub_sc_set_rows_nt(old_nt)
    _sc.set_variant()


def compact_tiled(sc, L, dec, xct, T):
    """pcub_sc_decode_bin_compact_tiled on the [N, B] compact rows in tiles of T codewords."""
    code, n = dec.code, dec.code.n
    tiled = sc.tile_rows(xct, T)
    ws = torch.empty(int(L.pcub_sc_decode_bin_compact_workspace(tiled.shape[0] * T, n)), dtype=torch.uint8,
                     device="cuda")
    info = torch.empty((max(1, code.info_words), B), dtype=torch.int32, device="cuda")
    xh = torch.empty((code.n_words, B), dtype=torch.int32, device="cuda")
    rc = L.pcub_sc_decode_bin_compact_tiled(sc._p(tiled), B, n, T, sc._p(code.fmask_dev), sc._p(code.fval_dev),
                                            code.K, sc._p(info), sc._p(xh), None, sc._p(ws), ws.numel(), sc._stream())
    assert rc == 0
    return info, xh, None


@pytest.mark.parametrize("variant", sorted(BUILT))
def test_every_built_kernel_decodes_as_its_pairs_form(sc, variant):
    from oracle import orc
    from polarcub_amd import _lib
    L = _lib.lib()
    built = [f for f in FORMS if L.pcub_sc_bin_form_built(variant, f) == 1]
    assert built == BUILT[variant]
    sc.set_variant(variant)
    n = smallest_n(sc, variant)
    assert n == SMALLEST_N.get(variant, n)
    N, T = 1 << n, sc.bin_tile(n)
    code = rate_half_code(sc, n)
    dec = sc.BinaryDecoder(code)
    # normalised codewords, so that the compact rows and the pairs are the same codewords exactly: the
    # Monte-Carlo pipeline's rows, +r for the pair (1, r) and -r for (r, 1)
    rng = np.random.default_rng(9000 + variant)
    r = rng.random((B, N))
    neg = rng.random((B, N)) < 0.5
    xy = np.stack([np.where(neg, r, 1.0), np.where(neg, 1.0, r)], axis=-1)
    rows = torch.from_numpy(xy).cuda()                                               # [B, N, 2]
    native = sc.transpose_pairs(rows)                                                # [N, B, 2]
    xct = torch.from_numpy(np.ascontiguousarray(np.where(neg, -r, r).T)).cuda()      # [N, B]

    def run(form):
        """(form the hook says this entry point launches, its packed info and x_hat words)"""
        if form == PAIRS:
            return L.pcub_sc_bin_form_for(n, 0, 0, 0), dec.decode_native(native)
        if form == TILED:
            return L.pcub_sc_bin_form_for(n, T, 0, 0), dec.decode_tiled_native(sc.tile_rows(native, T), B)
        if form in (ROWS, ROWS_NT):
            L.pcub_sc_set_rows_nt(int(form == ROWS_NT))
            return L.pcub_sc_bin_form_for(n, 0, 1, 0), dec.decode_rows_native(rows)
        if form == COMPACT:
            return L.pcub_sc_bin_form_for(n, 0, 0, 1), dec.decode_compact_native(xct)
        assert form == TILED_COMPACT
        return L.pcub_sc_bin_form_for(n, T, 0, 1), compact_tiled(sc, L, dec, xct, T)

    launched, ref = run(PAIRS)
    assert launched == PAIRS
    ri, rx = orc.decode_bin(xy, code.frozen_mask, code.frozen_values)
    assert np.array_equal(sc.unpack(ref[0], code.K).cpu().numpy(), ri)
    assert np.array_equal(sc.unpack(ref[1], code.N).cpu().numpy(), rx)
    for form in built[1:]:
        launched, got = run(form)
        assert launched == form, (variant, FORMS[form])
        assert same_words(got, ref), (variant, FORMS[form])
