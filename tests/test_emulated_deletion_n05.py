"""The n0 = 5 wave-per-task trellises (polarcub_amd/csrc/trellis_wave5.h) compiled for the host and run
with their lanes one after another (tests/emu5/w5_check.cpp) against trellis_body.h's Trel walk at
L = 32; and the C oracle against the Python oracle at n0 = 5, which the GPU tests of those shapes
rest on."""
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import trellis_oracle as tro
from tests.conftest import ROOT


def test_wave5_trellises_match_trel():
    """Random segments (lengths near 32, 0 .. 32, 32 itself and a few longer; pd from 0 to 1) and random
    32-bit decision histories: every depth-4 node's three collapsed rows bit-identical to the
    recursion's, the re-encoding of the 32 decisions equal to the recursion's, and the phases'
    multiply-shift division exact over its stated range.  6,000 cases, two seeds."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu5")], check=True)
    exe = os.path.join(ROOT, "tests", "emu5", "build", "w5_check")
    for seed in (51, 52):
        r = subprocess.run([exe, "3000", str(seed)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "3000 cases" in r.stdout and " 0 mismatches" in r.stdout


@pytest.mark.parametrize("n,n0", [(6, 5), (7, 5)])
def test_c_oracle_matches_python_oracle_n05(n, n0):
    """oracle/trellis_oracle.c equals oracle/trellis_oracle.py on 32-input trellises (two and four a
    codeword): channel words at two deletion rates plus an empty, a one-symbol, a short and an
    overlong word."""
    from oracle import orc
    rng = np.random.default_rng(100 * n + n0)
    prng = random.Random(7 * n + n0)
    N = 1 << n
    frozen = (rng.random(N) < 0.5).astype(np.uint8)
    fval = (rng.random(N) < 0.5).astype(np.uint8)
    pd = 0.1
    words = [tro.deletion_channel(tro.add_guard_bands([int(b) for b in rng.integers(0, 2, N)], n, n0, 0.1, 0),
                                  (0.05, 0.1, 0.1, 0.3)[t], prng) for t in range(4)]
    words += [[], [1], [0, 0, 1], [1] * (N + 3)]
    W = max(len(w) for w in words)
    rx = np.zeros((len(words), W), np.uint8)
    for i, w in enumerate(words):
        rx[i, :len(w)] = w
    ln = np.array([len(w) for w in words], np.int32)
    info, xhat = orc.decode_deletion(rx, ln, n, n0, pd, frozen, fval, 0)
    for i, w in enumerate(words):
        x, inf = tro.decode_deletion(w, n, n0, pd, frozen, fval, 0)
        assert list(info[i]) == inf and list(xhat[i]) == x, i
