"""Binaural rendering on the MI355X — the data-pipeline step in front of the separator.

Host-side mirror of the arithmetic in the reference's simulators and dataset:
`SOFASimulator._convolve(src, hrtf, idx)` / `ASHSimulator._convolve(src, hrtf_file)` (reference
src/datasets/multi_ch_simulator.py:40-61, :166-174) and `MixLibriSpeechNoisyEnrollNorm.__getitem__` lines 176-202,
batched over utterances.  Choosing WHICH impulse responses (SOFA / BRIR files by `random.Random(seed)`) stays with
the caller — that is data selection, and the `sofa` / `scaper` packages it needs are not part of this path.
No CPU fallback: CUDA tensors only.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _cabi


# ---- render_moving(method="fft"): the partitioning of include/lookonce_hip.h (lh_bank_spectra, lh_render_moving_fft)
FFT_Z = 1024                  # transform size
FFT_FRAME_MAX = 512           # 2 * frame - 1 must fit the transform
FFT_LH_MAX = 16384            # taps: a 1 s room response at 16 kHz
FFT_LDS_RING = 16             # block spectra a workgroup keeps in LDS; beyond that they live in the call's scratch
# method="auto": "fft" from this length on.  profiles/render_moving_fft_cost.txt (32 x 4 rows x 5 s, frame 400): the FFT form is
# faster than the direct one by more than three times the run's scatter at every measured Lh from 512 on, on both kinds of path —
# "Lh = 512: fft, every frame 0.4850 against 0.8217 ms (1.69 x); fft, arcs 0.4196 against 0.5303 ms (1.26 x)" — and slower on arcs at
# 256 (0.4065 against 0.3131 ms).  512 is the first such row; the constant is not set below 1024, whose row reads
# "Lh = 1024: fft, every frame 0.5056 against 1.5390 ms (3.04 x); fft, arcs 0.4359 against 0.9692 ms (2.22 x)".
AUTO_FFT_MIN_LH = 1024


def fft_partition(Lh: int, frame: int) -> Tuple[int, int, int, int, int]:
    """(m, Lp, Q, RING, RUN) of the partitioned path for responses of Lh taps at this frame; ValueError where it is refused."""
    if frame <= 0 or frame % 8 or frame > FFT_FRAME_MAX:
        raise ValueError(f"method 'fft' needs a frame that is a multiple of 8 and at most {FFT_FRAME_MAX}; got {frame}")
    if not 0 < Lh <= FFT_LH_MAX:
        raise ValueError(f"method 'fft' renders responses of at most {FFT_LH_MAX} taps; got {Lh}")
    m = max(1, (FFT_Z + 1 - frame) // frame)
    Lp = m * frame
    Q = -(-Lh // Lp)
    ring = (Q - 1) * m + 1
    return m, Lp, Q, ring, max(25, 2 * (ring - 1))


class BinauralRenderer(_cabi.HipHost):
    _host_name = "BinauralRenderer"

    def convolve(self, src: torch.Tensor, rir: torch.Tensor) -> torch.Tensor:
        """`_convolve`, batched: src [R, N] mono rows, rir [R, 2, Lh] -> [R, 2, N] (`convolve(...)[:len(src)]` per ear)."""
        R = src.shape[0]
        ones = torch.ones(1, R, device=src.device)
        tgt = torch.zeros(1, dtype=torch.int32, device=src.device)
        ev = self.render(src[None], rir[None], ones, tgt)[3]
        return ev[0]

    def render(self, srcs: torch.Tensor, rirs: torch.Tensor, gains: torch.Tensor, tgt_idx: torch.Tensor
               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """srcs [B, S1, N] (noise bed LAST), rirs [B, S1, 2, Lh], gains [B, S1] (1 for sources, noise_scale for the
        noise row), tgt_idx [B] -> mixture [B, 2, N], target [B, 2, N], norm_factor [B], events [B, S1, 2, N]."""
        lib = self._lib(srcs)
        if srcs.dim() != 3 or rirs.dim() != 4 or rirs.shape[:2] != srcs.shape[:2] or rirs.shape[2] != 2:
            raise ValueError(f"expected srcs [B,S1,N] and rirs [B,S1,2,Lh]; got {tuple(srcs.shape)} and {tuple(rirs.shape)}")
        B, S1, N = srcs.shape
        Lh = rirs.shape[3]
        if tuple(gains.shape) != (B, S1) or tuple(tgt_idx.shape) != (B,):
            raise ValueError("gains must be [B,S1] and tgt_idx [B]")
        if int(tgt_idx.max()) >= S1 or int(tgt_idx.min()) < 0:
            raise IndexError("tgt_idx out of range")
        dev = srcs.device
        srcs, rirs, gains = srcs.contiguous().float(), rirs.contiguous().float(), gains.contiguous().float()
        tgt_idx = tgt_idx.to(torch.int32).contiguous()
        events = torch.empty(B, S1, 2, N, device=dev)
        mixture, target = torch.empty(B, 2, N, device=dev), torch.empty(B, 2, N, device=dev)
        peak = torch.empty(B, dtype=torch.int32, device=dev)
        st = self._stream(dev)
        P = lambda t: t.data_ptr()
        with self._device_ctx(srcs):
            lib.call("lh_render_binaural", P(srcs), P(rirs), P(gains), P(tgt_idx), P(events), P(peak), P(mixture),
                     P(target), B, S1, N, Lh, st)
        return mixture, target, peak.view(torch.float32), events

    # ---- moving sources (ABI 24).  The interface follows the reference's binding of its native simulator
    # (src/datasets/motion_simulator.py: set_hrtf -> `bank`, add_source(audio, path) -> `nearest`, simulate ->
    # `render_moving`); the arithmetic is this project's own definition (include/lookonce_hip.h), the native code is absent.
    def nearest(self, paths: torch.Tensor, positions: torch.Tensor, bank_of: torch.Tensor) -> torch.Tensor:
        """paths [B, S1, F, 3] (one point per frame, any scale), positions [K, P, 3] (unit vectors), bank_of [B] ->
        idx [B, S1, F] int32: per point the bank entry with the largest dot product, the lowest index among equals."""
        lib = self._lib(paths)
        if paths.dim() != 4 or paths.shape[3] != 3 or positions.dim() != 3 or positions.shape[2] != 3:
            raise ValueError(f"expected paths [B,S1,F,3] and positions [K,P,3]; got {tuple(paths.shape)} and {tuple(positions.shape)}")
        B, S1, F, _ = paths.shape
        K, P, _ = positions.shape
        if tuple(bank_of.shape) != (B,):
            raise ValueError("bank_of must be [B]")
        if int(bank_of.max()) >= K or int(bank_of.min()) < 0:
            raise IndexError("bank_of out of range")
        dev = paths.device
        paths, positions = paths.contiguous().float(), positions.contiguous().float()
        bank_of = bank_of.to(torch.int32).contiguous()
        idx = torch.empty(B, S1, F, dtype=torch.int32, device=dev)
        D = lambda t: t.data_ptr()
        with self._device_ctx(paths):
            lib.call("lh_path_nearest", D(paths), D(positions), D(bank_of), D(idx), B, S1, F, P, K, self._stream(dev))
        return idx

    def bank_spectra(self, bank: torch.Tensor, frame: int = 400) -> torch.Tensor:
        """The partition spectra of a response bank [K, P, 2, Lh] for `render_moving(method="fft", spectra=...)` at this
        `frame`: an opaque image [K, P, Q, FFT_Z, 2] on the bank's device.  It depends on the bank and the frame only."""
        lib = self._lib(bank)
        if bank.dim() != 4 or bank.shape[2] != 2:
            raise ValueError(f"expected bank [K,P,2,Lh]; got {tuple(bank.shape)}")
        K, P, _, Lh = bank.shape
        Q = fft_partition(Lh, int(frame))[2]
        bank = bank.contiguous().float()
        spec = torch.empty(K, P, Q, FFT_Z, 2, device=bank.device)
        with self._device_ctx(bank):
            lib.call("lh_bank_spectra", bank.data_ptr(), spec.data_ptr(), K, P, Lh, int(frame), self._stream(bank.device))
        return spec

    def render_moving(self, srcs: torch.Tensor, bank: torch.Tensor, bank_of: torch.Tensor, idx: torch.Tensor, gains: torch.Tensor,
                      tgt_idx: torch.Tensor, frame: int = 400, method: str = "direct", spectra: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """`render` for sources that move: srcs [B, S1, N] (noise bed LAST), bank [K, P, 2, Lh], bank_of [B], idx [B, S1, F]
        with F >= ceil(N / frame) + 1 (row s passes through bank entry idx[b, s, f] at sample f * frame and is cross-faded
        towards idx[b, s, f + 1] over the frame), gains [B, S1], tgt_idx [B] -> mixture [B, 2, N], target [B, 2, N],
        norm_factor [B], events [B, S1, 2, N].  frame % 8 == 0.
        method: "direct" (one fmaf chain per response, any length), "fft" (the same definition by partitioned overlap-save:
        frame <= 512, Lh <= 16384; for room-length responses) or "auto" ("fft" from AUTO_FFT_MIN_LH taps on where it is
        supported).  spectra: `bank_spectra(bank, frame)` computed before, for "fft" / "auto"; computed in the call when None."""
        lib = self._lib(srcs)
        if srcs.dim() != 3 or bank.dim() != 4 or bank.shape[2] != 2:
            raise ValueError(f"expected srcs [B,S1,N] and bank [K,P,2,Lh]; got {tuple(srcs.shape)} and {tuple(bank.shape)}")
        B, S1, N = srcs.shape
        K, P, _, Lh = bank.shape
        frame = int(frame)
        if frame <= 0 or frame % 8:
            raise ValueError(f"frame must be a positive multiple of 8; got {frame}")
        if method not in ("direct", "fft", "auto"):
            raise ValueError(f"method must be 'direct', 'fft' or 'auto'; got {method!r}")
        if method == "auto":
            method = "fft" if Lh >= AUTO_FFT_MIN_LH and frame <= FFT_FRAME_MAX and Lh <= FFT_LH_MAX else "direct"
        if method == "fft":
            _, _, Q, ring, run = fft_partition(Lh, frame)                # ValueError for an unsupported frame or length
            if spectra is not None and (tuple(spectra.shape) != (K, P, Q, FFT_Z, 2) or spectra.dtype != torch.float32 or
                                        spectra.device != bank.device or not spectra.is_contiguous()):
                raise ValueError(f"spectra must be bank_spectra(bank, frame): contiguous float32 [{K},{P},{Q},{FFT_Z},2] on the "
                                 f"bank's device; got {tuple(spectra.shape)}")
        if idx.dim() != 3 or idx.shape[:2] != srcs.shape[:2] or idx.shape[2] < -(-N // frame) + 1:
            raise ValueError(f"idx must be [B,S1,F] with F >= ceil(N / frame) + 1 = {-(-N // frame) + 1}; got {tuple(idx.shape)}")
        if tuple(gains.shape) != (B, S1) or tuple(tgt_idx.shape) != (B,) or tuple(bank_of.shape) != (B,):
            raise ValueError("gains must be [B,S1], tgt_idx [B] and bank_of [B]")
        # one host read each, before anything is launched (`render` pays the same for tgt_idx)
        if int(tgt_idx.max()) >= S1 or int(tgt_idx.min()) < 0:
            raise IndexError("tgt_idx out of range")
        if int(bank_of.max()) >= K or int(bank_of.min()) < 0:
            raise IndexError("bank_of out of range")
        if int(idx.max()) >= P or int(idx.min()) < 0:
            raise IndexError("idx out of range")
        F = idx.shape[2]
        dev = srcs.device
        srcs, bank, gains = srcs.contiguous().float(), bank.contiguous().float(), gains.contiguous().float()
        bank_of, idx, tgt_idx = (t.to(torch.int32).contiguous() for t in (bank_of, idx, tgt_idx))
        events = torch.empty(B, S1, 2, N, device=dev)
        mixture, target = torch.empty(B, 2, N, device=dev), torch.empty(B, 2, N, device=dev)
        peak = torch.empty(B, dtype=torch.int32, device=dev)
        D = lambda t: t.data_ptr()
        if method == "fft":
            if spectra is None:
                spectra = self.bank_spectra(bank, frame)
            runs = -(-(-(-N // frame)) // run)
            work = torch.empty(B * S1 * runs * ring * FFT_Z, 2, device=dev) if ring > FFT_LDS_RING else None
            with self._device_ctx(srcs):
                lib.call("lh_render_moving_fft", D(srcs), D(spectra), D(bank_of), D(idx), D(gains), D(tgt_idx), D(events), D(peak),
                         D(mixture), D(target), None if work is None else D(work), B, S1, N, Lh, P, K, F, frame, self._stream(dev))
            return mixture, target, peak.view(torch.float32), events
        with self._device_ctx(srcs):
            lib.call("lh_render_moving", D(srcs), D(bank), D(bank_of), D(idx), D(gains), D(tgt_idx), D(events), D(peak), D(mixture),
                     D(target), B, S1, N, Lh, P, K, F, frame, self._stream(dev))
        return mixture, target, peak.view(torch.float32), events
