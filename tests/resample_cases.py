"""The float64 restatement of the resampling arithmetic and the case tables of tests/test_resample_oracle.py,
tests/test_emu_resample.py and tests/test_gpu_resample.py.

The oracle is torchaudio's published `sinc_interp_hann` algorithm written out in numpy float64, cross-checked against
`scipy.signal.upfirdn` (tests/test_resample_oracle.py) — pinned to the formula and to scipy, not to torchaudio itself."""
import math

import numpy as np

LPW, ROLLOFF = 6, 0.99
# (orig, new): the pairs the oracle is checked on against scipy
ORACLE_PAIRS = [(48000, 16000), (16000, 48000), (44100, 16000), (24000, 16000), (8000, 16000), (32000, 16000)]
# the pairs lh_resample runs on: o/n = 3/1, 1/3, 3/2, 1/2, 441/160
KERNEL_PAIRS = [(48000, 16000), (16000, 48000), (24000, 16000), (8000, 16000), (44100, 16000)]
ROWS = (1, 3)
TILE_OUT, SPAN = 1024, 8192                    # k_resample: outputs per tile, staged input samples (lh_render.hip)


def ratio(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def bank64(orig, new, lpw=LPW, rolloff=ROLLOFF):
    """-> (bank float64 [n, K], width, o, n)"""
    o, n = ratio(orig, new)
    base = min(o, n) * rolloff
    width = int(math.ceil(lpw * o / base))
    K = 2 * width + o
    bank = np.zeros((n, K), dtype=np.float64)
    for p in range(n):
        t = np.clip(((np.arange(K, dtype=np.float64) - width) / o - p / n) * base, -lpw, lpw)
        bank[p] = np.sinc(t) * np.cos(np.pi * t / (2 * lpw)) ** 2 * (base / o)       # np.sinc(t) = sin(pi t) / (pi t)
    return bank, width, o, n


def out_len(N, o, n):
    return -(-N * n // o)


def windows(x, width, o, K):
    """x [rows, N] -> the tap windows [rows, blocks, K] of xpad = width zeros, x, width + o zeros."""
    rows, N = x.shape
    blocks = -(-N // o) if N else 0
    xpad = np.zeros((rows, max(blocks, 1) * o + K), dtype=np.float64)
    xpad[:, width:width + N] = x
    return np.lib.stride_tricks.sliding_window_view(xpad, K, axis=1)[:, ::o][:, :blocks]


def resample64(x, bank, width, o, n):
    """x [rows, N] (any float dtype) with `bank` [n, K] -> (y float64 [rows, ceil(N n / o)], sum_k |bank| |x| per sample)."""
    x = np.asarray(x, dtype=np.float64)
    K = bank.shape[1]
    w = windows(x, width, o, K)                                  # [rows, blocks, K]
    L = out_len(x.shape[1], o, n)
    y = np.einsum("rbk,pk->rbp", w, bank).reshape(x.shape[0], -1)[:, :L]
    mag = np.einsum("rbk,pk->rbp", np.abs(w), np.abs(bank)).reshape(x.shape[0], -1)[:, :L]
    return y, mag


def bound(mag, K):
    """The fp32 dot product of K terms (one rounding per fmaf, <= K 2^-24 relative to the sum of magnitudes, first order)
    plus the bank's own rounding to fp32 (2^-24 relative per entry) and one spare: derived, not measured."""
    return (K + 2) * 2.0 ** -24 * mag


def tile_blocks(o, n, width):
    """Output blocks per workgroup of k_resample (lh_resample's choice): the size at which a second tile starts."""
    return min(max(1, TILE_OUT // n), (SPAN - 2 * width - 8) // o)


def kernel_lengths(orig, new):
    """Input lengths at the edges: 1, width, width + 1, one tile of blocks - 1 / exactly / + 1 block and one sample more."""
    _, width, o, n = bank64(orig, new)
    if o > 64:                                                   # 441/160
        return [1, width, width + 1, 900]
    tb = tile_blocks(o, n, width)
    return sorted({1, width, width + 1, (tb - 1) * o, tb * o, tb * o + 1, (tb + 1) * o})
