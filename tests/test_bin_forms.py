"""The binary decode launcher's choice of kernel, on the CPU: pcub_sc_bin_form_for answers which root
form (sc_bin_kern.h's BinForm) a decode at 2^n launches under the current switches, and
pcub_sc_bin_form_built walks the library's own list of built kernels (kBinBuilt).  Host-only calls; no
GPU, no compute call."""
import pytest

PAIRS, COMPACT, TILED, TILED_COMPACT, ROWS, ROWS_NT, SMALL = range(7)
FORMS = {PAIRS: "Pairs", COMPACT: "Compact", TILED: "Tiled", TILED_COMPACT: "TiledCompact", ROWS: "Rows",
         ROWS_NT: "RowsNT"}
# what the library builds: variant -> forms
BUILT = {0: [PAIRS], 1: [PAIRS], 10: [PAIRS], 13: [PAIRS], 14: [PAIRS], 17: [PAIRS],
         24: [PAIRS, COMPACT],
         26: [PAIRS, COMPACT, TILED, TILED_COMPACT, ROWS, ROWS_NT],
         30: [PAIRS, COMPACT, TILED, TILED_COMPACT, ROWS],
         31: [PAIRS, COMPACT, TILED, TILED_COMPACT],
         33: [PAIRS, COMPACT, TILED, TILED_COMPACT, ROWS]}
# the variant a decode at n = 6 .. 16 launches with the default selected
DEFAULT_VARIANT = [0, 13, 24, 26, 26, 26, 30, 33, 33, 17, 17]
NS = range(6, 17)


@pytest.fixture()
def L():
    """The library with its switches at their defaults, put back whatever the test changed."""
    from polarcub_amd import _lib
    lib = _lib.lib()
    lib.pcub_sc_set_variant(lib.pcub_sc_default_variant())
    old_tr, old_nt = lib.pcub_sc_set_tiled_root(1), lib.pcub_sc_set_rows_nt(0)
    yield lib
    lib.pcub_sc_set_variant(lib.pcub_sc_default_variant())
    lib.pcub_sc_set_tiled_root(old_tr)
    lib.pcub_sc_set_rows_nt(old_nt)


def forms(L, tile=0, rows=0, compact=0):
    """The form at n = 6 .. 16; tile "wave": the launched variant's own 64 / G."""
    return [L.pcub_sc_bin_form_for(n, L.pcub_sc_bin_tile(n) if tile == "wave" else tile, rows, compact) for n in NS]


def by_variant(table, default=PAIRS):
    return [table.get(v, default) for v in DEFAULT_VARIANT]


def test_built_set_is_the_list(L):
    built = {v: [f for f in FORMS if L.pcub_sc_bin_form_built(v, f) == 1] for v in range(L.pcub_sc_num_variants())}
    assert {v: fs for v, fs in built.items() if fs} == BUILT
    assert sum(len(fs) for fs in built.values()) == 28
    # "variant v is built" is "its Pairs form is built": what pcub_sc_set_variant accepts
    accepted = [v for v in range(L.pcub_sc_num_variants()) if L.pcub_sc_set_variant(v) == 0]
    assert accepted == sorted(BUILT)


def test_default_state(L):
    assert [L.pcub_sc_variant_for(n) for n in NS] == DEFAULT_VARIANT
    assert forms(L) == [PAIRS] * 11
    assert forms(L, tile="wave") == by_variant({26: TILED, 30: TILED, 33: TILED})
    assert forms(L, tile=5) == [PAIRS] * 11            # not the wave's own width
    assert forms(L, rows=1) == by_variant({26: ROWS, 30: ROWS, 33: ROWS})
    direct = {24: COMPACT, 26: COMPACT, 30: COMPACT, 33: COMPACT}   # elsewhere expanded into pairs first
    assert forms(L, compact=1) == by_variant(direct)
    assert forms(L, tile="wave", compact=1) == by_variant({24: COMPACT, 26: TILED_COMPACT, 30: TILED_COMPACT,
                                                           33: TILED_COMPACT})
    assert [L.pcub_sc_decode_bin_compact_direct(n) for n in NS] == [int(v in direct) for v in DEFAULT_VARIANT]
    # the rows-preferred vector of tests/test_rows_layout_abi.py: a rows twin, or plain root loads (variant 0)
    assert [L.pcub_sc_bin_rows_preferred(n) for n in NS] == [int(v in (0, 26, 30, 33)) for v in DEFAULT_VARIANT]


def test_rows_nt_switch(L):
    L.pcub_sc_set_rows_nt(1)
    assert forms(L, rows=1) == by_variant({26: ROWS_NT, 30: ROWS, 33: ROWS})   # 30, 33: only Rows is built
    assert forms(L, tile="wave") == by_variant({26: TILED, 30: TILED, 33: TILED})


def test_tiled_root_switch_off(L):
    L.pcub_sc_set_tiled_root(0)
    compact = by_variant({24: COMPACT, 26: COMPACT, 30: COMPACT, 33: COMPACT})
    for nt in (0, 1):
        L.pcub_sc_set_rows_nt(nt)
        assert forms(L) == forms(L, tile="wave") == forms(L, rows=1) == [PAIRS] * 11
        assert forms(L, compact=1) == forms(L, tile="wave", compact=1) == compact


def test_variant_31_has_no_rows_twin(L):
    assert L.pcub_sc_set_variant(31) == 0
    assert L.pcub_sc_variant_for(12) == 31 and L.pcub_sc_bin_tile(12) == 16
    assert L.pcub_sc_bin_form_for(12, 16, 0, 0) == TILED
    assert L.pcub_sc_bin_form_for(12, 16, 0, 1) == TILED_COMPACT
    assert L.pcub_sc_bin_form_for(12, 0, 1, 0) == PAIRS
    assert L.pcub_sc_bin_rows_preferred(12) == 0       # non-temporal root loads (T = 1) and no rows twin


def test_small_codes_and_bad_arguments(L):
    from polarcub_amd import _lib
    for n in range(0, 6):
        assert L.pcub_sc_bin_form_for(n, 0, 0, 0) == L.pcub_sc_bin_form_for(n, 64, 0, 1) == SMALL
        assert L.pcub_sc_bin_form_for(n, 0, 1, 0) == SMALL
    for args in [(-1, 0, 0, 0), (25, 0, 0, 0), (10, -1, 0, 0), (10, 4097, 0, 0), (10, 0, 1, 1)]:
        assert L.pcub_sc_bin_form_for(*args) == _lib.EINVAL, args
    for args in [(-1, PAIRS), (34, PAIRS), (26, -1), (26, SMALL)]:
        assert L.pcub_sc_bin_form_built(*args) == _lib.EINVAL, args
