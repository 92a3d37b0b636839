"""The n0 = 5 wave-per-task trellises (polarcub_amd/csrc/trellis_wave5.h) compiled for the host and run
with their lanes one after another (tests/emu5/w5_check.cpp) against trellis_body.h's Trel walk at
L = 32; the C oracle against the Python oracle at n0 = 5, which the GPU tests of those shapes
rest on; and the Python oracle against the reference's own decodes at n0 = 5
(tests/golden/deletion_wave.npz; the C oracle meets them in tests/test_trellis_oracle.py)."""
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import trellis_oracle as tro
from tests.conftest import ROOT
from tests.test_trellis_oracle import _check, _words, wave_case


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


@pytest.mark.parametrize("n,pd,nwords", [(6, 0.1, 8), (6, 0.25, 8), (7, 0.1, 8), (7, 0.25, 8), (11, 0.1, 8),
                                         (11, 0.05, 4)])
def test_python_oracle_matches_wave_fixture_n05(n, pd, nwords):
    """oracle/trellis_oracle.py against the reference at 32-input trellises (two, four and 64 a codeword):
    info, x_hat and the marginals at information leaves bit-exact, every word whose marginals the
    fixture stores (channel words at the case's pd and at 0.4, the empty word, an all-zeros and an
    overlong one; (11, 5, 0.05), the frozen set the reference decodes correctly: the channel words).
    (13, 5) and (15, 5) are left to the C oracle: the Python restatement takes seconds a word there."""
    c = wave_case(n, 5, pd)
    assert c["nleaf"] == nwords
    _check(_words(c)[:nwords], n, 5, pd, 0, c["frozen"], c["fval"], c["info"], c["xhat"], c["leaf_m"])
