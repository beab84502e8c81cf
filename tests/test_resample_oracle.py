"""CPU: the float64 restatement of the resampler (tests/resample_cases.py) against scipy's polyphase filter, the product's
bank against the restatement's, and the output lengths."""
import numpy as np
import pytest
import scipy.signal
import torch

from lookoncetohear_amd.resample import resample_bank, resampled_length
from tests import resample_cases as C


def upfirdn_restated(x, bank, width, o, n):
    """The same sum through scipy.signal.upfirdn: the interleaved prototype filter h[p o - k n + c n o] = bank[p][k] applied
    to xpad at up = n, down = o, read c blocks late (c o >= K - 1 makes every index of h non-negative)."""
    K = bank.shape[1]
    c = -(-(K - 1) // o)
    h = np.zeros(c * n * o + (n - 1) * o + 1)
    for p in range(n):
        for k in range(K):
            h[p * o - k * n + c * n * o] = bank[p][k]
    N = len(x)
    xpad = np.concatenate([np.zeros(width), x, np.zeros(width + o)])
    y = scipy.signal.upfirdn(h, xpad, up=n, down=o)
    L = C.out_len(N, o, n)
    return y[c * n:c * n + L]


@pytest.mark.parametrize("orig,new", C.ORACLE_PAIRS)
def test_restatement_matches_scipy_upfirdn(orig, new):
    bank, width, o, n = C.bank64(orig, new)
    rng = np.random.default_rng(orig + new)
    for N in (1, o, 1000):
        x = rng.standard_normal(N)
        y, _ = C.resample64(x[None], bank, width, o, n)
        want = upfirdn_restated(x, bank, width, o, n)
        assert y.shape == (1, len(want)) and np.abs(y[0] - want).max() <= 1e-12, (orig, new, N)
    l1 = np.abs(bank).sum(1)
    assert 1.0 < l1.min() and l1.max() < 2.0                      # rows are low-pass interpolators of unit gain


@pytest.mark.parametrize("orig,new", C.ORACLE_PAIRS)
def test_bank_is_the_float64_bank_cast_to_fp32(orig, new):
    bank, width, o, n = C.bank64(orig, new)
    got, w, oo, nn = resample_bank(orig, new)
    assert (w, oo, nn) == (width, o, n) and got.dtype == torch.float32 and tuple(got.shape) == bank.shape
    assert np.array_equal(got.numpy(), bank.astype(np.float32))
    assert got.shape[1] == 2 * width + o


def test_geometry_of_the_table():
    geo = {p: C.bank64(*p)[1:] for p in C.ORACLE_PAIRS}
    assert geo[(48000, 16000)] == (19, 3, 1) and geo[(16000, 48000)] == (7, 1, 3) and geo[(44100, 16000)] == (17, 441, 160)
    assert geo[(24000, 16000)] == (10, 3, 2) and geo[(8000, 16000)] == (7, 1, 2) and geo[(32000, 16000)] == (13, 2, 1)


@pytest.mark.parametrize("orig,new", C.ORACLE_PAIRS)
def test_output_lengths(orig, new):
    bank, width, o, n = C.bank64(orig, new)
    for N in (0, 1, o - 1, o, o + 1, 1000):
        y, _ = C.resample64(np.ones((2, N)), bank, width, o, n)
        want = -(-n * N // o)
        assert y.shape == (2, want) and resampled_length(N, o, n) == want, (orig, new, N)
