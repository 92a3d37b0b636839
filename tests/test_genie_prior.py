"""The genie under a non-uniform a-priori distribution on the CPU: the wave-a-trial kernel body
(polarcub_amd/csrc/genie_prior_body.h) compiled for the host with its lanes run one after another
and its LDS arrays as exactly sized heap arrays (tests/emu_prior/genie_prior_check.cpp) against the C
oracle's two-tree recursion; the two new symbols and their argument checks; and the host path of the
facade against the reference's own genie runs (tests/golden/genie_prior.npz,
scripts/make_golden_genie_prior.py)."""
import contextlib
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import orc
from tests.conftest import ROOT, load_golden

EMU_SIZES = [1, 2, 3, 6, 7, 8, 10]  # n = 1: the raw-root leaf pair; 6 / 7 / 8: a level below, at, above 64 positions


# -- helpers shared with tests/test_gpu_genie_prior.py ----------------------------------------

def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def marginals(leaf):
    """Compact leaves -> the reference's marginals, as pcub_leaf_marginals computes them."""
    leaf = np.asarray(leaf, np.float64)
    s, r = np.signbit(leaf), np.abs(leaf)
    nan = np.isnan(r)
    p0 = np.where(nan, 0.0, np.where(s, r, 1.0))
    p1 = np.where(nan, 0.0, np.where(s, 1.0, r))
    tot = (0.0 + p0) + p1
    safe = np.where(tot > 0.0, tot, 1.0)
    return np.stack([np.where(tot > 0.0, p0 / safe, 0.5), np.where(tot > 0.0, p1 / safe, 0.5)], axis=-1)


def oracle_trial(prior, r, xy=None):
    """One genie pass by the C oracle: every position frozen, u decided by the x tree against r.
    xy = None is the encoder: with xy = prior the two trees are equal, so the leaf marginals are the
    x tree's.  Returns (xhat [N], u [N], m [N, 2])."""
    N = r.shape[0]
    _, xhat, m = orc.decode_bin_general(prior if xy is None else xy, np.ones(N, np.uint8), r, prior=prior)
    return xhat, orc.polar_transform_bits(xhat), m


def make_case(n, B, kind, per_trial_prior, with_xy, seed):
    """Inputs of B trials at N = 2^n: prior [1 or B, N, 2], xy [B, N, 2] or None, R [B, N].
    kind: 'iid' (one pair for every position), 'positional', 'edge' (rows with exact zeros and
    unnormalised rows).  xy has one-sided zeros and (0, 0) rows.  R has entries of exactly 0.0 and
    1.0, and R[b, 0] is leaf 0's own m0 (a tie, which decides 0)."""
    rng = np.random.default_rng(seed)
    N = 1 << n
    PB = B if per_trial_prior else 1
    if kind == "iid":
        a = 0.05 + 0.9 * rng.random((PB, 1))
        prior = np.repeat(np.stack([a, 1.0 - a], axis=-1), N, axis=1)
    elif kind == "positional":
        a = 0.05 + 0.9 * rng.random((PB, N))
        prior = np.stack([a, 1.0 - a], axis=-1)
    else:
        prior = rng.random((PB, N, 2)) * rng.choice([1.0, 3.7, 1e-3, 250.0], size=(PB, N, 1))
        z = rng.random((PB, N)) < 0.15
        side = rng.integers(0, 2, (PB, N))
        prior[..., 0] = np.where(z & (side == 0), 0.0, prior[..., 0])
        prior[..., 1] = np.where(z & (side == 1), 0.0, prior[..., 1])
    prior = np.ascontiguousarray(prior)
    xy = None
    if with_xy:
        xy = rng.random((B, N, 2))
        z = rng.random((B, N)) < 0.15
        side = rng.integers(0, 2, (B, N))
        xy[..., 0] = np.where(z & (side == 0), 0.0, xy[..., 0])
        xy[..., 1] = np.where(z & (side == 1), 0.0, xy[..., 1])
        xy[rng.random((B, N)) < 0.03] = 0.0
    R = rng.random((B, N))
    R[rng.random((B, N)) < 0.05] = 0.0
    R[rng.random((B, N)) < 0.05] = 1.0
    for b in range(B):
        pr = prior[b if per_trial_prior else 0]
        R[b, 0] = oracle_trial(pr, R[b])[2][0, 0]  # leaf 0 does not depend on r
    return prior, xy, R


def case_matrix(B):
    """(n, kind, per_trial_prior, with_xy, seed) of every emulated / device case at batch size B."""
    out = []
    for n in EMU_SIZES:
        for ki, kind in enumerate(("iid", "positional", "edge")):
            for per_trial in (False, True):
                for with_xy in (False, True):
                    out.append((n, kind, per_trial, with_xy, 1000 * n + 10 * ki + 2 * per_trial + with_xy + 7 * B))
    return out


def check_against_oracle(prior, xy, R, xhat, u, m, what=""):
    B = R.shape[0]
    for b in range(B):
        pr = prior[b if prior.shape[0] > 1 else 0]
        rx, ru, rm = oracle_trial(pr, R[b], None if xy is None else xy[b])
        assert np.array_equal(xhat[b], rx), (what, b, "xhat")
        assert np.array_equal(u[b], ru), (what, b, "u")
        assert np.array_equal(bits(m[b]), bits(rm)), (what, b, "marginals")


# -- host emulation of the kernel body ---------------------------------------------------------

_EXE = None


def emu_exe():
    global _EXE
    if _EXE is None:
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu_prior")], check=True)
        _EXE = os.path.join(ROOT, "tests", "emu_prior", "build", "genie_prior_check")
    return _EXE


def emu_run(tmp, prior, xy, R):
    B, N = R.shape
    n = N.bit_length() - 1
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([n, 0 if xy is None else 1, B, prior.shape[0]], np.int32).tobytes())
        f.write(np.ascontiguousarray(prior, np.float64).tobytes())
        if xy is not None:
            f.write(np.ascontiguousarray(xy, np.float64).tobytes())
        f.write(np.ascontiguousarray(R, np.float64).tobytes())
    r = subprocess.run([emu_exe(), src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(dst, "rb").read()
    assert len(raw) == B * N * 10
    leaf = np.frombuffer(raw[:B * N * 8], np.float64).reshape(B, N)
    xhat = np.frombuffer(raw[B * N * 8:B * N * 9], np.uint8).reshape(B, N)
    u = np.frombuffer(raw[B * N * 9:], np.uint8).reshape(B, N)
    return xhat, u, leaf


@pytest.mark.parametrize("n", EMU_SIZES)
def test_emulated_body_matches_oracle(n, tmp_path):
    """Both modes, shared and per-trial priors of the three kinds, three trials each: x_hat, u and the
    leaf marginals bit-equal to the C oracle's two-tree recursion."""
    ones = zeros = 0
    for (cn, kind, per_trial, with_xy, seed) in case_matrix(3):
        if cn != n:
            continue
        prior, xy, R = make_case(n, 3, kind, per_trial, with_xy, seed)
        xhat, u, leaf = emu_run(str(tmp_path), prior, xy, R)
        check_against_oracle(prior, xy, R, xhat, u, marginals(leaf), (n, kind, per_trial, with_xy))
        assert np.all(u[:, 0] == 0)  # the tie at leaf 0 decides 0
        ones += int(u.sum())
        zeros += int((1 - u).sum())
    assert ones > 0 and zeros > 0


def test_numpy_marginals_match_the_oracle_on_edge_leaves():
    """The test's own leaf -> marginal helper on the sentinel and boundary leaves."""
    leaf = np.array([0.0, -0.0, 1.0, -1.0, np.nan, 0.25, -0.25])
    want = [[1.0, 0.0], [0.0, 1.0], [0.5, 0.5], [0.5, 0.5], [0.5, 0.5], [1.0 / 1.25, 0.25 / 1.25], [0.25 / 1.25, 1.0 / 1.25]]
    assert np.array_equal(bits(marginals(leaf)), bits(np.array(want)))


# -- ABI -------------------------------------------------------------------------------------------

NAMES = ("pcub_sc_genie_prior_supported", "pcub_sc_genie_prior_bin")


def test_symbols_are_exported_declared_and_bound():
    from polarcub_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "polarcub_sc.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint %s\(" % name, header)
        assert getattr(L, name).argtypes
    assert L.pcub_abi_version() == _lib.ABI_VERSION == 4


def test_invalid_arguments_are_refused_before_any_hip_call():
    from polarcub_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    fake = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        a = dict(xy=fake, prior=fake, pb=1, r=fake, B=4, log2N=6, xhat=fake, u=fake, leaf=fake)
        a.update(kw)
        return L.pcub_sc_genie_prior_bin(a["xy"], a["prior"], a["pb"], a["r"], a["B"], a["log2N"], a["xhat"], a["u"],
                                         a["leaf"], None)

    for kw in [dict(log2N=0), dict(log2N=14), dict(log2N=-3), dict(B=-1), dict(pb=0), dict(pb=2), dict(pb=5),
               dict(prior=None), dict(r=None), dict(leaf=None), dict(xhat=None, u=None, leaf=None),
               dict(xy=None, prior=None)]:
        assert call(**kw) == _lib.EINVAL, kw
    assert call(B=0) == 0            # an empty batch: nothing to launch
    assert call(B=0, pb=0) == 0      # prior_batch = B
    assert call(B=0, xy=None) == 0
    assert [L.pcub_sc_genie_prior_supported(n, w) for w in (0, 1) for n in (0, 1, 13, 14, -1)] == [0, 1, 1, 0, 0] * 2


# -- the host path against the reference -----------------------------------------------------------

def golden_case(g, name):
    c = {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "_")}
    c["meta"] = g["meta"]["cases"][name]
    return c


def xvd_of(prior):
    from polarcub_amd import vectors
    xvd = vectors.BinaryMemorylessVectorDistribution(prior.shape[0])
    xvd.probs[:] = prior
    return xvd


def xyvd_of(c, received):
    N = c["prior"].shape[0]
    return xvd_of(c["table"][np.arange(N), np.asarray(received, np.int64)])


def whole_run(c, run, check_codeword=True):
    """coding.genieEncodeDecodeSimulation on the fixture's trials: the channel closure replays the
    stored received words (and checks the codeword it is handed).  Returns (frozen set, stdout)."""
    from polarcub_amd import coding
    N, T = c["prior"].shape[0], c["meta"]["trials"]
    state = {"t": 0}

    def channel(codeword):
        t = state["t"]
        state["t"] += 1
        if check_codeword:
            assert np.array_equal(np.asarray(codeword, np.int64), c["enc_x"][t].astype(np.int64)), t
        return [int(v) for v in c["rx"][t]]

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        frozen = coding.genieEncodeDecodeSimulation(N, lambda: xvd_of(c["prior"]), lambda e: e, channel,
                                                    lambda rx: xyvd_of(c, rx), T, c["meta"]["bound"],
                                                    genieSeed=c["meta"]["genie_seed"], trustXYProbs=run["trust"])
    assert state["t"] == T
    return frozen, buf.getvalue()


def check_per_trial(c, enc, dec, dec_untrusted=None):
    """enc / dec: per trial (x, TV, H) and (x, Pe, H) as the genieSingle* methods return them."""
    T = c["meta"]["trials"]
    assert len(enc) == len(dec) == T
    for t in range(T):
        assert np.array_equal(np.asarray(enc[t][0], np.int64), c["enc_x"][t].astype(np.int64)), t
        assert np.array_equal(bits(enc[t][1]), bits(c["TV"][t])), t
        assert np.array_equal(bits(enc[t][2]), bits(c["HEnc"][t])), t
        assert np.array_equal(np.asarray(dec[t][0], np.int64), c["dec_x"][t].astype(np.int64)), t
        assert np.array_equal(bits(dec[t][1]), bits(c["Pe"][t])), t
        assert np.array_equal(bits(dec[t][2]), bits(c["HDec"][t])), t
        if dec_untrusted is not None:
            assert np.array_equal(np.asarray(dec_untrusted[t][0], np.int64), c["dec_x"][t].astype(np.int64)), t
            assert np.array_equal(bits(dec_untrusted[t][1]), bits(c["Pe_untrusted"][t])), t
            assert list(dec_untrusted[t][2]) == []


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_host_genie_singles_match_reference(name):
    """genieSingleEncodeSimulatioan / genieSingleDecodeSimulatioan on the host reproduce the
    reference's per-trial vectors bit for bit (the first reference pin of this path)."""
    from polarcub_amd import coding
    c = golden_case(load_golden("genie_prior"), name)
    N, T = c["prior"].shape[0], c["meta"]["trials"]
    encDec = coding.BinaryPolarEncoderDecoder(N, set(), 0)
    xvd = xvd_of(c["prior"])
    seeds = [int(s) for s in c["seeds"]]
    enc = [encDec.genieSingleEncodeSimulatioan(xvd, s) for s in seeds]
    dec = [encDec.genieSingleDecodeSimulatioan(xvd, xyvd_of(c, c["rx"][t]), seeds[t], True) for t in range(T)]
    unt = None
    if "Pe_untrusted" in c:
        unt = [encDec.genieSingleDecodeSimulatioan(xvd, xyvd_of(c, c["rx"][t]), seeds[t], False) for t in range(T)]
    check_per_trial(c, enc, dec, unt)


@pytest.mark.parametrize("name,run", [("a", 0), ("a", 1), ("b", 0)])
def test_batched_branch_with_the_emulated_kernel_matches_reference(name, run, monkeypatch, tmp_path):
    """The facade's batched branch on the CPU: sc.GeniePriorCoder replaced by a stand-in that runs the
    host-compiled kernel body, the per-trial host genie forbidden.  The statistics, their
    accumulation and the printout (element types included) are the reference's."""
    import torch

    from polarcub_amd import coding, sc

    class EmulatedCoder:
        def __init__(self, N, device=None):
            self.N = N

        def encode(self, prior, R):
            return self.decode(prior, None, R)

        def decode(self, prior, xy, R):
            p = prior.numpy()
            xhat, u, leaf = emu_run(str(tmp_path), p[None] if p.ndim == 2 else p, None if xy is None else xy.numpy(),
                                    R.numpy())
            return torch.from_numpy(xhat.copy()), torch.from_numpy(u.copy()), torch.from_numpy(marginals(leaf))

    def forbidden(*a, **k):
        raise AssertionError("host genie used")

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(sc, "genie_prior_supported", lambda N, with_xy=True: True)
    monkeypatch.setattr(sc, "GeniePriorCoder", EmulatedCoder)
    monkeypatch.setattr(coding.BinaryPolarEncoderDecoder, "genieSingleEncodeSimulatioan", forbidden)
    monkeypatch.setattr(coding.BinaryPolarEncoderDecoder, "genieSingleDecodeSimulatioan", forbidden)
    c = golden_case(load_golden("genie_prior"), name)
    r = c["meta"]["runs"][run]
    frozen, out = whole_run(c, r)
    assert sorted(frozen) == r["frozen"]
    assert out == r["stdout"]


def test_batch_common_randomness_is_the_reference_draw():
    """The [T, N] common randomness the batched genie hands the device is Random(seed).random() per
    position, trial by trial (the reference's randomlyGeneratedNumbers after geniePreSteps)."""
    from polarcub_amd import coding
    g = load_golden("genie_prior")
    for name in ("a", "b", "c"):
        c = golden_case(g, name)
        R = coding._genie_r(c["prior"].shape[0], [int(s) for s in c["seeds"]])
        assert np.array_equal(bits(R), bits(c["r"]))
    assert np.array_equal(coding._genie_r(4, [-1]), np.ones((1, 4)))


@pytest.mark.parametrize("name,run", [("a", 0), ("a", 1), ("b", 0)])
def test_host_fallback_whole_run_matches_reference(name, run, monkeypatch):
    """Without a usable GPU genieEncodeDecodeSimulation under a non-uniform prior takes the host
    path, as before, and reproduces the reference's stdout and frozen set."""
    import torch

    from polarcub_amd import coding
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    def forbidden(*a, **k):
        raise AssertionError("device genie used without a GPU")

    monkeypatch.setattr(coding.BinaryPolarEncoderDecoder, "genie_encode_prior_batch", forbidden)
    monkeypatch.setattr(coding.BinaryPolarEncoderDecoder, "genie_decode_prior_batch", forbidden)
    c = golden_case(load_golden("genie_prior"), name)
    r = c["meta"]["runs"][run]
    frozen, out = whole_run(c, r)
    assert sorted(frozen) == r["frozen"]
    assert out == r["stdout"]
