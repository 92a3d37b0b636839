"""The rows root layout ([B, N, 2] / [B, N, q] read in place: pcub_sc_decode_bin_rows,
pcub_sc_decode_qary_rows) on the CPU: the symbols and their argument checks, and the decode schedule of
polarcub_amd/csrc/sc_bin_sched.h compiled for the host (tests/emu/rows_emu.cpp) on exactly sized
[B][N][2] buffers -- through the generic path (the tiled layout of width 1) and through the rows
twins' addressing -- against the reference's golden vectors, against the [N][B] emulation, and as a
stand-alone program under AddressSanitizer and UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from polarcub_amd.sc import pack_rows, unpack_rows
from tests.conftest import ROOT, load_golden

EMU = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(EMU, "build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOST = [HIPCC, "--offload-host-only", "-ffp-contract=off", "-std=c++17",
        "-I" + os.path.join(ROOT, "polarcub_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
SRC = os.path.join(EMU, "rows_emu.cpp")

_L = None


def emu():
    """tests/emu/rows_emu.cpp as a shared library (this test's own compile command)."""
    global _L
    if _L is None:
        os.makedirs(BUILD, exist_ok=True)
        lib = os.path.join(BUILD, "librowsemu.so")
        subprocess.run(HOST + ["-O2", "-fPIC", "-shared", "-o", lib, SRC], check=True)
        _L = ctypes.CDLL(lib)
    return _L


def run(xy, frozen, fval, S, layout):
    """xy [B, N, 2]; layout 0 hands the emulator the transposed [N, B, 2] rows, 1 and 2 the rows as
    they are, in a buffer of exactly B N pairs."""
    B, N, _ = xy.shape
    n = N.bit_length() - 1
    K = int(N - frozen.sum())
    fm = pack_rows(frozen).reshape(-1).copy()
    fv = pack_rows(fval).reshape(-1).copy()
    src = np.ascontiguousarray(np.transpose(xy, (1, 0, 2))) if layout == 0 else np.ascontiguousarray(xy).copy()
    info = np.zeros((max(1, (K + 31) // 32), B), np.uint32)
    xh = np.zeros((max(1, (N + 31) // 32), B), np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = emu().emu_decode_bin_rows(P(src), ctypes.c_longlong(B), n, P(fm), P(fv), P(info), P(xh), S, layout)
    assert rc == 0
    return unpack_rows(info, K), unpack_rows(xh, N)


def test_symbols_resolve_and_abi_version():
    from polarcub_amd import _lib
    L = _lib.lib()
    for name in ("pcub_sc_decode_bin_rows", "pcub_sc_decode_qary_rows", "pcub_sc_bin_rows_preferred"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes
    assert L.pcub_abi_version() == _lib.ABI_VERSION == 4


def test_callers_policy_follows_the_kernels_root_loads():
    """pcub_sc_bin_rows_preferred: the small-code kernels, variant 0 (plain root loads, N = 64) and the
    default variants with rows twins (N = 512 .. 16384) read the rows in place; the generic kernels with
    non-temporal root loads (N = 128, 256, N >= 32768) keep the staging pass."""
    from polarcub_amd import _lib, sc
    L = _lib.lib()
    sc.set_variant()
    assert [sc.rows_preferred(n) for n in range(0, 17)] == [True] * 7 + [False, False] + [True] * 6 + [False, False]
    assert L.pcub_sc_bin_rows_preferred(25) == _lib.EINVAL and L.pcub_sc_bin_rows_preferred(-1) == _lib.EINVAL


def test_invalid_arguments_are_refused_before_any_launch():
    from polarcub_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    fake = ctypes.cast(buf, ctypes.c_void_p)

    def bin_call(**kw):
        a = dict(xy=fake, B=4, log2N=6, fm=fake, fv=fake, K=32, info=fake, xhat=fake, u=None, ws=fake, wsb=4096)
        a.update(kw)
        return L.pcub_sc_decode_bin_rows(a["xy"], a["B"], a["log2N"], a["fm"], a["fv"], a["K"], a["info"], a["xhat"],
                                         a["u"], a["ws"], a["wsb"], None)

    for kw in [dict(xy=None), dict(B=-1), dict(log2N=-1), dict(log2N=25), dict(fm=None), dict(fv=None), dict(K=-1),
               dict(K=65), dict(info=None)]:
        assert bin_call(**kw) == _lib.EINVAL, kw
    assert bin_call(B=0) == 0          # an empty batch: nothing to launch
    assert bin_call(B=0, xy=None) == 0

    def q_call(**kw):
        a = dict(xy=fake, B=4, log2N=6, q=4, frozen=fake, K=32, info=fake, xhat=fake, ws=fake, wsb=4096)
        a.update(kw)
        return L.pcub_sc_decode_qary_rows(a["xy"], a["B"], a["log2N"], a["q"], a["frozen"], a["K"], a["info"],
                                          a["xhat"], a["ws"], a["wsb"], None)

    for kw in [dict(xy=None), dict(B=-1), dict(log2N=1), dict(log2N=21), dict(q=1), dict(q=9), dict(frozen=None),
               dict(K=-1), dict(K=65), dict(info=None)]:
        assert q_call(**kw) == _lib.EINVAL, kw
    assert q_call(B=0) == 0


@pytest.mark.parametrize("layout", [1, 2])
@pytest.mark.parametrize("S", [8, 16, 32])
@pytest.mark.parametrize("name", ["bsc_n64", "awgn_n1024", "awgn_n4096"])
def test_rows_schedule_matches_reference(name, S, layout):
    g = load_golden(name)
    xy = g["xy"] if "xy" in g else g["table"][g["y"]]
    info, xhat = run(xy, g["frozen"], g["fval"], S, layout)
    assert np.array_equal(info, g["info"])
    assert np.array_equal(xhat, g["xhat"])


@pytest.mark.parametrize("n", [4, 6, 10])
def test_rows_schedule_equals_codeword_minor_rows(n):
    """Random rows, B = 3: both rows forms decode what the [N][B] emulation decodes."""
    rng = np.random.default_rng(40 + n)
    N, B = 1 << n, 3
    frozen = (rng.random(N) < 0.5).astype(np.uint8)
    frozen[: N // 8] = 1
    fval = (rng.random(N) < 0.5).astype(np.uint8)
    xy = rng.random((B, N, 2))
    for S in (8, 16, 32):
        if n > 5 and N < 2 * S:
            continue
        ref = run(xy, frozen, fval, S, 0)
        for layout in (1, 2):
            got = run(xy, frozen, fval, S, layout)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (S, layout)


def test_rows_schedule_stand_alone_under_sanitizers():
    """The same host code as a program with its own main (B = 3 at N = 32, 64, 1024; input buffers of
    exactly B N pairs on the heap), built with -fsanitize=address,undefined and run as a child
    process: a read outside the rows, or undefined behaviour in the addressing, ends it non-zero."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "rows_emu_san")
    subprocess.run(HOST + ["-O1", "-DROWS_EMU_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rows_emu: ok" in r.stdout
