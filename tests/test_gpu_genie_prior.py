"""The genie under a non-uniform a-priori distribution on the GPU (pcub_sc_genie_prior_bin, one wave
a trial): against the reference's own genie runs (tests/golden/genie_prior.npz), per trial and as
whole genieEncodeDecodeSimulation runs with the host genie forbidden; against the C oracle on the
emulation's case matrix and on a batch larger than any resident grid; and against the lane-a-codeword
two-tree kernel (pcub_sc_prior_bin) where the two compute the same thing."""
import numpy as np
import pytest

from tests.conftest import load_golden
from tests.test_genie_prior import (EMU_SIZES, bits, case_matrix, check_against_oracle, check_per_trial, golden_case,
                                    make_case, whole_run)

pytestmark = pytest.mark.gpu


def device_run(prior, xy, R):
    import torch

    from polarcub_amd import sc
    gp = sc.GeniePriorCoder(R.shape[1])
    p = torch.from_numpy(prior)
    r = torch.from_numpy(R)
    if xy is None:
        xhat, u, m = gp.encode(p, r)
    else:
        xhat, u, m = gp.decode(p, torch.from_numpy(xy), r)
    return xhat.cpu().numpy(), u.cpu().numpy(), m.cpu().numpy()


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fixture_per_trial(name):
    """Both passes as device batches: x_hat, TV, HEnc, Pe (trusted, and untrusted where the fixture
    has it) and HDec bit-equal to the reference's per-trial vectors; N = 1024 included."""
    from polarcub_amd import coding
    c = golden_case(load_golden("genie_prior"), name)
    N, T = c["prior"].shape[0], c["meta"]["trials"]
    encDec = coding.BinaryPolarEncoderDecoder(N, set(), 0)
    seeds = [int(s) for s in c["seeds"]]
    xy = c["table"][np.arange(N)[None, :], c["rx"].astype(np.int64)]
    assert xy.shape == (T, N, 2)
    enc = encDec.genie_encode_prior_batch(c["prior"], seeds)
    dec = encDec.genie_decode_prior_batch(c["prior"], xy, seeds, True)
    unt = encDec.genie_decode_prior_batch(c["prior"], xy, seeds, False) if "Pe_untrusted" in c else None
    check_per_trial(c, enc, dec, unt)


@pytest.mark.parametrize("name,run", [("a", 0), ("a", 1), ("b", 0)])
def test_fixture_whole_run_on_device(name, run, monkeypatch):
    """coding.genieEncodeDecodeSimulation with the per-trial host genie forbidden reproduces the
    reference's stdout and frozen set."""
    from polarcub_amd import coding

    def forbidden(*a, **k):
        raise AssertionError("host genie used")

    monkeypatch.setattr(coding.BinaryPolarEncoderDecoder, "genieSingleEncodeSimulatioan", forbidden)
    monkeypatch.setattr(coding.BinaryPolarEncoderDecoder, "genieSingleDecodeSimulatioan", forbidden)
    c = golden_case(load_golden("genie_prior"), name)
    r = c["meta"]["runs"][run]
    frozen, out = whole_run(c, r)
    assert sorted(frozen) == r["frozen"]
    assert out == r["stdout"]


@pytest.mark.parametrize("n", EMU_SIZES)
@pytest.mark.parametrize("B", [1, 5, 33, 257])
def test_random_cases_match_oracle(B, n):
    """The emulation's matrix (iid / positional / edge priors, shared and per trial, both modes; zeros,
    (0, 0) rows, r of exactly 0 and 1, the tie at leaf 0) at four batch sizes."""
    for (cn, kind, per_trial, with_xy, seed) in case_matrix(B):
        if cn != n:
            continue
        prior, xy, R = make_case(n, B, kind, per_trial, with_xy, seed)
        xhat, u, m = device_run(prior, xy, R)
        check_against_oracle(prior, xy, R, xhat, u, m, (n, B, kind, per_trial, with_xy))
        assert np.all(u[:, 0] == 0)


@pytest.mark.parametrize("n", [12, 13])
def test_largest_lengths_match_oracle(n):
    """N = 4096 and 8192: with xy a wave's LDS passes 64 KB (69,600 and 139,232 bytes), so the
    launcher asks for the larger dynamic size; at N = 8192 one wave is a whole workgroup."""
    for with_xy in (False, True):
        prior, xy, R = make_case(n, 3, "positional", False, with_xy, 77 + n)
        xhat, u, m = device_run(prior, xy, R)
        check_against_oracle(prior, xy, R, xhat, u, m, (n, with_xy))


@pytest.mark.parametrize("with_xy", [False, True])
def test_persistent_grid_strides_over_a_large_batch(with_xy):
    """B = 20,000 at N = 16: more trials than the 256 x 4 x 8 = 8,192 waves an MI355X can hold, so
    every wave runs its trial loop at least twice; every trial checked."""
    prior, xy, R = make_case(4, 20000, "positional", False, with_xy, 99)
    xhat, u, m = device_run(prior, xy, R)
    check_against_oracle(prior, xy, R, xhat, u, m, ("persistent", with_xy))


def test_matches_the_lane_kernel_with_one_shared_r():
    """n = 9, one r repeated for all trials, every position frozen: x_hat and the compact leaves equal
    pcub_sc_prior_bin's, for the encoder (K = 0) and the decoder."""
    import torch

    from polarcub_amd import sc
    n, B = 9, 70
    N = 1 << n
    prior, xy, R = make_case(n, B, "positional", True, True, 4242)
    R[:] = R[0]
    code = sc.CodeSpec(N, np.ones(N, np.uint8))
    pc = sc.PriorCoder(code, R[0])
    gp = sc.GeniePriorCoder(N)
    dev = code.device
    p_rows = torch.from_numpy(prior).to(dev)              # [B, N, 2]
    p_lane = p_rows.transpose(0, 1).contiguous()          # [N, B, 2]
    r_dev = torch.from_numpy(R).to(dev)
    xy_dev = torch.from_numpy(xy).to(dev)
    for mode_xy in (None, xy_dev):
        if mode_xy is None:
            _, xw, leaf_lane = pc.run_native(p_lane, B=B, want_leaf=True)
        else:
            _, xw, leaf_lane = pc.run_native(p_lane, xy=sc.transpose_pairs(mode_xy), want_leaf=True)
        xhat, _, leaf = gp.run_native(p_rows, r_dev, xy=mode_xy)
        assert torch.equal(sc.unpack(xw, N), xhat)
        assert np.array_equal(bits(leaf_lane.t().contiguous().cpu().numpy()), bits(leaf.cpu().numpy()))


def test_supported_range():
    from polarcub_amd import _lib, sc
    L = _lib.lib()
    for w in (0, 1):
        assert [L.pcub_sc_genie_prior_supported(n, w) for n in range(0, 15)] == [0] + [1] * 13 + [0]
    assert sc.genie_prior_supported(8192) and not sc.genie_prior_supported(16384) and not sc.genie_prior_supported(1)
    assert not sc.genie_prior_supported(48)
