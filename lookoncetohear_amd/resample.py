"""Sample-rate conversion on the MI355X — the last step of every reference dataset
(`torchaudio.transforms.Resample(sr, resample_rate)`, reference src/datasets/MixLibriSpeechNoisyEnrollNorm.py:69-73, 345-347)
and what its simulators do to every impulse response (`torchaudio.functional.resample`, src/datasets/multi_ch_simulator.py:49,
169, 248, 345: CIPIC and ASH responses are 44.1 / 48 kHz).

The arithmetic is torchaudio's published `sinc_interp_hann` algorithm, restated — pinned to the formula (and, in the tests, to
scipy's polyphase filter), not to torchaudio itself.  With g = gcd(orig, new), o = orig / g, n = new / g:

    base  = min(o, n) * rolloff
    width = ceil(lowpass_filter_width * o / base)
    K     = 2 width + o
    t[p][k]    = clamp(((k - width) / o - p / n) * base, -lpw, lpw)
    bank[p][k] = sinc(pi t) * cos(pi t / (2 lpw))^2 * base / o                    fp64, then cast to fp32
    y[q n + p] = sum_k xpad[q o + k] * bank[p][k]                                 xpad = width zeros, x, width + o zeros
    len(y)     = ceil(n len(x) / o)

The same bank and the same inner product serve `SessionStreamer(..., client_rate=)` per slot (net.py).  No CPU fallback: CUDA
tensors only.
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np
import torch

from . import _cabi


def resample_ratio(orig_freq: int, new_freq: int) -> Tuple[int, int]:
    """(o, n): the two rates over their greatest common divisor."""
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq < 1 or new_freq < 1:
        raise ValueError(f"sample rates are positive integers, got {orig_freq} and {new_freq}")
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def resample_bank(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99
                  ) -> Tuple[torch.Tensor, int, int, int]:
    """-> (bank fp32 [n, K] on the host, width, o, n); computed in fp64."""
    o, n = resample_ratio(orig_freq, new_freq)
    if lowpass_filter_width < 1:
        raise ValueError("lowpass_filter_width must be positive")
    lpw = float(lowpass_filter_width)
    base = min(o, n) * float(rolloff)
    width = int(math.ceil(lpw * o / base))
    k = np.arange(2 * width + o, dtype=np.float64)[None, :]
    p = np.arange(n, dtype=np.float64)[:, None]
    t = np.clip(((k - width) / o - p / n) * base, -lpw, lpw)
    window = np.cos(np.pi * t / (2.0 * lpw)) ** 2
    pt = np.pi * t
    sinc = np.where(pt == 0.0, 1.0, np.sin(pt) / np.where(pt == 0.0, 1.0, pt))
    bank = sinc * window * (base / o)
    return torch.from_numpy(bank.astype(np.float32)), width, o, n


def resampled_length(n_samples: int, o: int, n: int) -> int:
    return (n_samples * n + o - 1) // o


class Resampler(_cabi.HipHost):
    """`torchaudio.transforms.Resample(orig_freq, new_freq)` call semantics: x [..., N] -> [..., ceil(N n / o)], one launch
    (`lh_resample`), fp32 on the device, nothing waits.  Equal rates return the input itself."""
    _host_name = "Resampler"

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.bank, self.width, self.o, self.n = resample_bank(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self._banks = {}                                    # device -> the bank there

    def _bank_on(self, device) -> torch.Tensor:
        b = self._banks.get(device)
        if b is None:
            b = self._banks[device] = self.bank.to(device)
        return b

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if self.o == self.n:
            return x
        lib = self._lib(x)
        if x.dtype != torch.float32 or x.dim() < 1:
            raise ValueError(f"Resampler takes float32 [..., N], got {x.dtype} {tuple(x.shape)}")
        N = x.shape[-1]
        n_out = resampled_length(N, self.o, self.n)
        y = torch.empty(*x.shape[:-1], n_out, dtype=torch.float32, device=x.device)
        rows = y.numel() // n_out if n_out else 0
        if rows == 0:
            return y
        x = x.contiguous()
        if x.data_ptr() % 16:                               # a view into a larger tensor: the kernel loads 16 bytes at a time
            x = x.clone()
        if N >= 1 << 31 or n_out >= 1 << 31:
            raise ValueError("rows of 2^31 samples or more are not supported")
        bank, st = self._bank_on(x.device), self._stream(x.device)
        xr, yr = x.view(rows, N), y.view(rows, n_out)
        with self._device_ctx(x):
            for r0 in range(0, rows, 65532):                # rows ride the grid's second dimension; a multiple of 4 keeps 16 bytes
                r = min(65532, rows - r0)
                lib.call("lh_resample", xr[r0:].data_ptr(), yr[r0:].data_ptr(), bank.data_ptr(), r, N, n_out, self.o, self.n,
                         self.width, st)
        return y
