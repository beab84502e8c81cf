"""`Net` — MI355X-native drop-in for the reference separator `src.models.tfgridnet_realtime.net.Net`.

Installation = changing one string in the reference config (configs/tsh.json:4):

    "model": "lookoncetohear_amd.net.Net"

because the reference builds its model with `utils.import_attr(model)(**model_params)`
(reference src/ts_hear_embed_pl_module.py:25).  This class therefore mirrors, exactly:

  * the constructor keywords and defaults of reference net.py:21-24 (configs/tsh.json:5-19 pass unchanged);
  * `forward(x, embeds, input_state=None, pad=True)`, `predict(x, embed, input_state, pad=True)`,
    `init_buffers(batch_size, device)` (reference net.py:51-76) with the same state-dict-of-tensors layout
    (reference tfgridnet_causal.py:173-186, 408-427), mutated and returned like the reference does;
  * the parameter / buffer names and shapes of the reference module tree (`tfgridnet.blocks.0.intra_rnn.
    weight_ih_l0`, ... SURVEY.md §8b), so a reference Lightning checkpoint loads with strict=True, and the same
    construction order, so `torch.manual_seed(s); Net(**params)` draws the same initial weights.

The torch modules below are parameter containers only: they are never called.  All arithmetic runs in the
hand-written gfx950 kernels behind the C ABI of include/lookonce_hip.h; there is no CPU fallback (the product
path raises if the HIP library is missing or the tensors are not on the GPU).
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _cabi
from .weights import KV_PAD_ROWS, QK_PAD, pack_all, unsplit_qk, unsplit_v


def mod_pad(x: torch.Tensor, chunk_size: int, pad: Tuple[int, int]):
    """Right-pad to a multiple of `chunk_size`, then apply `pad` (reference net.py:8-18)."""
    mod = 0
    if x.shape[-1] % chunk_size != 0:
        mod = chunk_size - (x.shape[-1] % chunk_size)
    # one zero-filled copy for both pads (the reference's two F.pad calls cost two copies of the batch; with nothing to pad,
    # none: the kernels only read x)
    if mod or pad[0] or pad[1]:
        x = F.pad(x, (pad[0], mod + pad[1]))
    return x, mod


def stft_filterbank(n_fft: int, hop: int) -> torch.Tensor:
    """Analysis/synthesis filterbank buffer `[n_fft + 2, 1, n_fft]` (asteroid-filterbanks STFTFB as called at
    reference tfgridnet_causal.py:131-135): sqrt-periodic-Hann windowed real-DFT rows, 97 cosine rows then 97
    negative-sine rows, DC/Nyquist cosine rows scaled by 1/sqrt(2), overall 1/(0.5*sqrt(n_fft^2/hop))."""
    nbin = n_fft // 2 + 1
    n = np.arange(n_fft)
    window = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft))
    ang = 2 * np.pi * np.arange(nbin)[:, None] * n[None, :] / n_fft
    re, im = np.cos(ang), -np.sin(ang)
    re[0] /= np.sqrt(2)
    re[n_fft // 2] /= np.sqrt(2)
    rows = np.vstack([re, im]) * window[None, :] / (0.5 * np.sqrt(n_fft * n_fft / hop))
    return torch.from_numpy(rows).float().unsqueeze(1)


class _FilterBank(nn.Module):
    def __init__(self, n_fft, hop):
        super().__init__()
        self.register_buffer("_filters", stft_filterbank(n_fft, hop))


class _Coder(nn.Module):          # name holder for `enc.filterbank._filters` / `dec.filterbank._filters`
    def __init__(self, n_fft, hop):
        super().__init__()
        self.filterbank = _FilterBank(n_fft, hop)


class _Norm(nn.Module):           # name holder for `*.norm.{weight,bias}`
    def __init__(self, n, eps):
        super().__init__()
        self.norm = nn.LayerNorm(n, eps=eps)


def _proj(n_in, n_out, n_norm, eps):
    # Linear, PReLU (single slope, espnet2 get_layer("prelu")()), [reshape], joint LayerNorm -> indices 0,1,3
    return nn.Sequential(nn.Linear(n_in, n_out), nn.PReLU(), nn.Identity(), _Norm(n_norm, eps))


class _GridNetBlockParams(nn.Module):
    """Parameters of one causal GridNet block, created in the reference order (tfgridnet_causal.py:334-396)."""

    def __init__(self, emb_dim, n_freqs, hidden, n_head, eps):
        super().__init__()
        E = math.ceil(512 * 1.0 / n_freqs)
        self.intra_norm = _Norm(emb_dim, eps)
        self.intra_rnn = nn.LSTM(emb_dim, hidden, 1, batch_first=True, bidirectional=True)
        self.intra_linear = nn.Linear(hidden * 2, emb_dim)
        self.inter_norm = _Norm(emb_dim, eps)
        self.inter_rnn = nn.LSTM(emb_dim, hidden, 1, batch_first=True, bidirectional=False)
        self.inter_linear = nn.Linear(hidden, emb_dim)
        self.attn_conv_Q = _proj(emb_dim, E * n_head, n_freqs * E, eps)
        self.attn_conv_K = _proj(emb_dim, E * n_head, n_freqs * E, eps)
        self.attn_conv_V = _proj(emb_dim, (emb_dim // n_head) * n_head, n_freqs * (emb_dim // n_head), eps)
        self.attn_concat_proj = _proj(emb_dim, emb_dim, n_freqs * emb_dim, eps)


class _TFGridNetParams(nn.Module):
    """Parameter tree of the reference causal TFGridNet (tfgridnet_causal.py:113-171), same names/order."""

    def __init__(self, n_fft, stride, n_imics, n_srcs, emb_dim, n_layers, hidden, n_head, spk_emb_dim, eps=1.0e-5):
        super().__init__()
        n_freqs = n_fft // 2 + 1
        self.enc = _Coder(n_fft, stride)
        self.dec = _Coder(n_fft, stride)
        self.conv = nn.Sequential(nn.Conv2d(2 * n_imics, emb_dim, (3, 3), padding=(0, 1)))
        self.blocks = nn.ModuleList(
            [_GridNetBlockParams(emb_dim, n_freqs, hidden, n_head, eps) for _ in range(n_layers)])
        self.embed_to_feats_proj = nn.Sequential(nn.Linear(spk_emb_dim, emb_dim * n_freqs),
                                                 nn.LayerNorm(emb_dim * n_freqs))
        self.deconv = nn.ConvTranspose2d(emb_dim, n_srcs * 2, (3, 3), padding=(2, 1))


class _Lanes:
    """K HIP streams forked from and joined to the current stream of `dev` (the windows of `Net.time_chunks`).  The only
    stream / event calls of the chunked block loop live here; tests/hipemu/hosts.py substitutes a serial stand-in."""
    serial = False

    def __init__(self, dev, side_streams):
        # lane 0 is the CURRENT stream (the chip has four hardware queues per process by default: a fifth stream would share
        # one and serialise behind it — profiles/r06e: the fourth side stream's first kernel started 300 us late)
        self.dev = dev
        self.main = torch.cuda.current_stream(dev)
        self.streams = [self.main] + list(side_streams)

    def fork(self):
        ev = torch.cuda.Event()
        ev.record(self.main)
        for s_ in self.streams[1:]:
            s_.wait_event(ev)

    def on(self, k):
        return torch.cuda.stream(self.streams[k])

    def signal(self, k):
        ev = torch.cuda.Event()
        ev.record(self.streams[k])
        return ev

    def wait(self, k, ev):
        self.streams[k].wait_event(ev)

    def join(self):
        for s_ in self.streams[1:]:
            self.main.wait_stream(s_)


class _EnrollSide:
    """The ONE side stream a `SessionStreamer` runs the enrollment embedder on, with the two events of a call and the "is it
    done" query (one stream only: the process has four hardware queues and `time_chunks` uses lanes of its own).  The only
    stream / event calls of enrollment live here; the emulator tests substitute a synchronous stand-in, as for `_Lanes`."""

    def __init__(self, dev, low_priority: bool = False):
        self.dev = dev
        self._hip, self._raw = None, None
        if low_priority:
            # torch hands out default- and high-priority streams only: the lowest priority comes from the HIP runtime itself
            # (dlsym on the library's handle searches its dependencies, i.e. the runtime that owns torch's streams too)
            hip = self._hip = _cabi.load()._dll
            least, greatest, raw = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_void_p()
            with torch.cuda.device(dev):
                if (hip.hipDeviceGetStreamPriorityRange(ctypes.byref(least), ctypes.byref(greatest)) != 0 or
                        hip.hipStreamCreateWithPriority(ctypes.byref(raw), 1, least.value) != 0):     # 1: non-blocking
                    raise RuntimeError("could not create a low-priority HIP stream")
            self._raw = raw
            self.stream = torch.cuda.ExternalStream(raw.value, device=dev)
        else:
            self.stream = torch.cuda.Stream(device=dev)

    def __del__(self):
        if self._raw is not None:
            self._hip.hipStreamDestroy(self._raw)      # asynchronous: the runtime frees it once its work has drained

    def run(self, fn):
        """fn() on the side stream, after everything enqueued so far on the loop's (current) stream -> (result, done event)."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self.stream.wait_event(ev)
        with torch.cuda.stream(self.stream):
            out = fn()
        done = torch.cuda.Event()
        done.record(self.stream)
        return out, done

    def finished(self, done) -> bool:
        return done.query()

    def hand_over(self, done, out: torch.Tensor):
        """The loop's stream may read `out` from here on (`done` has completed: the wait costs the device nothing)."""
        main = torch.cuda.current_stream(self.dev)
        main.wait_event(done)
        out.record_stream(main)


class Net(_cabi.HipHost, nn.Module):
    _host_name = "Net"
    enroll_low_priority = False      # priority of a SessionStreamer's embedder stream: see `_EnrollSide`, DESIGN.md

    def __init__(self, stft_chunk_size=160, stft_pad_size=120, embed_dim=256,
                 num_ch=2, D=64, B=6, I=1, J=1, L=0, H=128,
                 use_attn=False, lookahead=True, local_atten_len=100,
                 chunk_causal=False, num_src=2):
        super().__init__()
        self.ctor_params = dict(stft_chunk_size=stft_chunk_size, stft_pad_size=stft_pad_size, embed_dim=embed_dim,
                                num_ch=num_ch, D=D, B=B, I=I, J=J, L=L, H=H, use_attn=use_attn, lookahead=lookahead,
                                local_atten_len=local_atten_len, chunk_causal=chunk_causal, num_src=num_src)
        self.stft_chunk_size = stft_chunk_size
        self.stft_pad_size = stft_pad_size
        self.num_ch = num_ch
        self.lookahead = lookahead
        self.nfft = stft_chunk_size + stft_pad_size
        # I, J (emb_ks / emb_hs) are accepted and unused, like the reference causal block (:399-400)
        self.n_blocks, self.emb_dim, self.hidden, self.n_head = B, D, H, L
        self.n_freqs = self.nfft // 2 + 1
        self.local_atten_len = local_atten_len
        self.n_srcs = num_src
        self.spk_emb_dim = embed_dim
        if not (use_attn and chunk_causal):
            raise NotImplementedError("only the chunk-causal attention mode of configs/tsh.json is implemented")
        shape = (self.nfft, stft_chunk_size, num_ch, D, H, L, local_atten_len, num_src, embed_dim)
        if shape != (192, 128, 2, 64, 64, 4, 50, 2, 256):
            raise NotImplementedError(
                f"the gfx950 kernels are specialised on the configs/tsh.json shapes; got (nfft, hop, mics, D, H, L, "
                f"window, srcs, embed_dim) = {shape}")
        self.E = math.ceil(512 * 1.0 / self.n_freqs)
        self.V_dim = D // L
        self.tfgridnet = _TFGridNetParams(self.nfft, stft_chunk_size, num_ch, num_src, D, B, H, L, embed_dim)
        # contraction arithmetic of the two RECURRENCES: "f16x3" = split-precision fp16 MFMA (hi/lo operands, ~22 mantissa
        # bits, ~5x the fp32-MFMA rate), "f32rec" = exact fp32 MFMA in the intra / inter LSTMs (the name says what it
        # covers: the frame kernels — STFT / conv, Q/K/V, attention, projection, deconv / iSTFT — are split-precision in
        # every mode); "f32all" = additionally the frame kernels on plain-fp32 reference kernels (lh_ref32.hip: slow,
        # test-only — the all-fp32 run that separates "split-precision error" from "kernel bug" on a real checkpoint).
        # LOOKONCE_GEMM overrides.
        self.gemm_mode = os.environ.get("LOOKONCE_GEMM", "f16x3")
        self._check_gemm_mode()                 # a stale LOOKONCE_GEMM=f32 (the spelling removed in round 5) fails HERE
        # range guard of the split-precision kernels (include/lookonce_hip.h): the frame kernels scale every row / tile by
        # a power of two before they split it, so any finite input is in range; non-finite output samples (inf / NaN in
        # the input, a true fp32 overflow) reach the caller AS THEY ARE, like from the reference's plain-fp32 forward
        # (`keep_nonfinite`, ABI 13: nothing is hidden even when nobody looks at the flag — a `Streamer` stores 0 instead,
        # silence for a listener) and raise THIS Net's flag word (`_range_flag`: pinned host memory the kernel stores to
        # directly, one per device, never shared with another Net or a Streamer).
        #   range_check = True / "deferred" (default): the forward stays asynchronous; the word is looked at when the NEXT
        #       forward starts and in `range_status()`, and a set word raises LH_ERR_RANGE there.  (Round 3 ended every
        #       forward with a host wait: 7.58 -> 7.36 ms per batch-32 step without it, profiles/r04e_range_check_sync_cost.txt.)
        #   range_check = "sync": wait for the stream at the end of every forward and raise from the forward that
        #       produced the samples (LOOKONCE_RANGE_CHECK=sync); False / LOOKONCE_RANGE_CHECK=0: never look.
        rc = os.environ.get("LOOKONCE_RANGE_CHECK", "1")
        self.range_check = False if rc == "0" else ("sync" if rc == "sync" else True)
        self._range_flags: Dict[str, torch.Tensor] = {}
        # fused LSTM + Linear + residual kernels (f16x3 mode only); LOOKONCE_FUSE=0 selects the unfused pair
        self.fuse_linear = os.environ.get("LOOKONCE_FUSE", "1") != "0"
        # An offline forward (zero state in, no state out) lets the LAST block's closing stage emit the 36 deconv tap products
        # per (frame, bin) instead of the 64-channel frame, and the back end start from them (lh_proj_ln_res_taps ->
        # lh_taps_istft: the same waveform bits, 0.875 frame passes over HBM less; profiles/taps_fusion_ab.txt).
        # LOOKONCE_FUSE_TAPS=0 keeps lh_proj_ln_res -> lh_deconv_istft.
        self.fuse_taps = os.environ.get("LOOKONCE_FUSE_TAPS", "1") != "0"
        # fused intra kernel (two launches, one per direction) from here on, the unfused pair (both directions concurrently) below:
        # 8192 frames in rounds 1-5; with time windows the crossover is lower (profiles/r06h: B = 13 x 625 frames 3.40 -> 3.08 ms,
        # B = 10 2.66 -> 2.60, B = 8 2.32 -> 2.36)
        self.fuse_intra_min_frames = int(os.environ.get("LOOKONCE_FUSE_INTRA_MIN_FRAMES", "6000"))
        # inter LSTM: one workgroup per sequence (mat-vec recurrence, 0.39 us per step) while the sequences fit ONE round of CUs
        # (batch <= 2); above, the 16-sequence tile kernel in time windows wins (round 6, profiles/r06h: B = 4 2.27 -> 1.67 ms;
        # rounds 3-5 used the per-sequence kernel up to two rounds = batch 5).  LOOKONCE_MATVEC_MAX_SEQS overrides.
        self.inter_matvec_max_seqs = int(os.environ.get("LOOKONCE_MATVEC_MAX_SEQS", "256"))
        self.stream_intra_max_frames = 128      # up to here one workgroup per (frame, direction) still finds its own CU
        # time-axis pipelining of the three blocks (round 6; include/lookonce_hip.h "time windows"): every stage is causal in
        # t, so the frames can be cut into K windows, window k on its own HIP stream, and block i on window k + 1 runs beside
        # block i + 1 on window k.  State is handed over on the device: (h, c) per window, the K / V history = the previous
        # window's rows of the history-extended buffers (one pair per block, so a window that runs ahead cannot overwrite rows a
        # slower one still reads); the output is bit-identical to the whole-clip forward.  What it buys depends on how much of
        # the chip one launch fills (profiles/r06b, r06e, r06h): the inter LSTM is a 625-step dependent chain on ceil(97 B / 16)
        # CUs, and every small-batch launch is latency-bound —
        #   time_chunks        batches on the fused kernels (B T >= 6000 frames: B >= 10 at 5 s).  0 = automatic: 2 windows while
        #                      the inter launch leaves more than ~30 % of the 256 CUs dark (B <= 29: -19 % at B = 14, -15 % at 16,
        #                      -11 % at 20, -5 % at 24, -1 % at 28), one from there on (B = 32: +-0, and the per-launch figures of
        #                      bench.py's roofline object stay those of kernels that run alone); K >= 1 forces K.
        #   time_chunks_small  smaller batches (unfused intra pair; per-sequence inter kernel up to B = 5, tiled one above),
        #                      windows on multiples of the attention tile / of 64 frames.  0 = automatic: 3 windows (B = 6 … 13:
        #                      -21 … -27 %), 2 for one utterance (1.31 -> 1.12 ms per 5 s clip; every hand-over between windows is
        #                      a cross-stream event of 10-20 us on this runtime), 1 where the per-sequence kernel's last round of
        #                      workgroups already fills the chip (B = 2, 5); K >= 1 forces K.
        # LOOKONCE_TIME_CHUNKS / LOOKONCE_TIME_CHUNKS_SMALL override.
        self.n_cus = 256                        # MI355X (the library is gfx950-only)
        self.time_chunks = int(os.environ.get("LOOKONCE_TIME_CHUNKS", "0"))
        self.time_chunks_small = int(os.environ.get("LOOKONCE_TIME_CHUNKS_SMALL", "0"))
        self.chunk_min_frames = 64              # >= the 49 frames of attention history: a window then depends on ONE predecessor
        self._chunk_streams: Dict[str, list] = {}
        self._pack_key = None
        self._packed = None
        self._ws: Dict[tuple, dict] = {}
        self._zeros: Dict[tuple, dict] = {}
        self._blob = None                  # (device, packed tree) when built by `from_packed`
        self._debug_taps: Optional[dict] = None
        self._prof: Optional[list] = None  # bench.py: list of (kernel tag, start event, end event) per launch
        self._prof_only: Optional[set] = None
        self._prof_stride: int = 1              # bench.py: bracket every n-th call of the selected names only (see bench.py)
        self._prof_count: dict = {}
        # asteroid-filterbanks' STFTFB may register a second buffer (`torch_window`) next to `_filters` (un-vendored,
        # version unpinned: could not be checked here).  The kernels only need `_filters`, so such keys of a reference
        # checkpoint are dropped before the strict key check instead of failing it.
        self._register_load_state_dict_pre_hook(self._drop_foreign_filterbank_keys)

    @staticmethod
    def _drop_foreign_filterbank_keys(state_dict, prefix, *_):
        for k in [k for k in state_dict if k.startswith(prefix) and ".filterbank." in k and not k.endswith("._filters")]:
            state_dict.pop(k)

    # ------------------------------------------------------------------------------------------------
    # reference API
    # ------------------------------------------------------------------------------------------------
    def init_buffers(self, batch_size, device):
        """Zero streaming state, reference shapes (tfgridnet_causal.py:173-186, 408-427)."""
        z = lambda *s: torch.zeros(*s, device=device)
        F_, C_, L_ = self.n_freqs, self.emb_dim, self.local_atten_len
        bufs = {}
        for i in range(self.n_blocks):
            bufs[f"buf{i}"] = dict(K_buf=z(batch_size * self.n_head, L_ - 1, self.E * F_),
                                   V_buf=z(batch_size * self.n_head, L_ - 1, self.V_dim * F_),
                                   c0=z(1, batch_size * F_, self.hidden),
                                   h0=z(1, batch_size * F_, self.hidden))
        return dict(conv_buf=z(batch_size, self.num_ch * 2, 2, F_), deconv_buf=z(batch_size, C_, 2, F_),
                    istft_buf=z(batch_size, self.n_srcs, F_ * 2, 1), gridnet_bufs=bufs)

    def predict(self, x, embed, input_state, pad=True, want_state=True):
        """Reference signature (net.py:54-66) plus `want_state`: False (only used by `forward` when it starts from the
        zero state) skips materialising the next state, which `forward` discards anyway."""
        mod = 0
        if pad:
            pad_size = (0, self.stft_pad_size) if self.lookahead else (0, 0)
            x, mod = mod_pad(x, chunk_size=self.stft_chunk_size, pad=pad_size)
        x, next_state = self._separate(x, embed, input_state, want_state)
        # the kernels already leave out the stft_pad_size look-ahead tail the reference trims at net.py:61
        if mod != 0:
            x = x[:, :, :-mod]
        return x, next_state

    def forward(self, x, embeds, input_state=None, pad=True):
        embeds = embeds[:, 0]  # [B, E]
        # zero initial state and the next state is dropped (reference net.py:68-76): no per-call state tensors
        x, next_state = self.predict(x, embeds, input_state, pad, want_state=input_state is not None)
        return x

    def forward_many(self, x, embeds, pad=True):
        """Every enrolled speaker of a mixture in one call: x [B, 2, N], embeds [B, K, 256] -> y [B, K, 2, N], where
        y[b, k] is `forward(x[b:b+1], embeds[b:b+1, k:k+1])`.  The reference multiplies the embedding in only in front of
        block 1 (tfgridnet_causal.py:247-251), so the STFT, the input convolution and block 0 run once per MIXTURE (B rows,
        with the kernels and windows `forward` picks for batch B) and block 0's last kernel stores its frame once per
        target (`lh_proj_ln_res_fan`); blocks 1 ... and the back end run on the B K rows as `forward` would for that batch.
        Starts from the zero state and keeps none.  `gemm_mode = "f32all"` (the test-only reference kernels) shares
        nothing: it runs the K-times-repeated mixtures through `forward`'s path.  A ragged K is the caller's to pad (any
        embedding, drop the row)."""
        if embeds.dim() != 3:
            raise ValueError(f"embeds must be [B, K, {self.spk_emb_dim}], got {tuple(embeds.shape)}")
        if x.dim() != 3 or embeds.shape[0] != x.shape[0]:
            raise ValueError(f"x [B, {self.num_ch}, N] and embeds [B, K, {self.spk_emb_dim}] must agree in B, got "
                             f"{tuple(x.shape)} and {tuple(embeds.shape)}")
        if embeds.shape[1] < 1:
            raise ValueError("embeds must hold at least one speaker per mixture (K >= 1)")
        if self._debug_taps is not None:
            raise ValueError("forward_many has no stage taps: tap `forward` on one (mixture, speaker) pair")
        mod = 0
        if pad:
            pad_size = (0, self.stft_pad_size) if self.lookahead else (0, 0)
            x, mod = mod_pad(x, chunk_size=self.stft_chunk_size, pad=pad_size)
        y = self._separate_many(x, embeds)
        if mod != 0:
            y = y[..., :-mod]
        return y

    def make_streamer(self, batch_size: int, device, use_graph: bool = True):
        """Chunked real-time front end (BASELINE configs[1]): see `Streamer`."""
        return Streamer(self, batch_size, device, use_graph)

    def make_session_streamer(self, n_slots: int, device, use_graph: bool = True, enroll_chunks: int = 0,
                              compact: bool = False, row_buckets=None, pace: bool = False, packets: bool = False,
                              fifo_samples: int = 2048, pcm16: bool = False, client_rate: int = 16000, monitor: bool = False,
                              monitor_ramp: int = 256):
        """The batched streamer with per-listener sessions (slots open, close and fail one at a time): see `SessionStreamer`.
        `enroll_chunks` = n >= 2: slots can also `enroll()` — the device records a slot's next n chunks (128 n samples), the
        enrollment embedder runs beside the chunk loop and the slot opens itself on the result.
        `compact`: open listeners are kept in the leading rows and a chunk is launched for the smallest of `row_buckets`
        (ascending launch sizes ending in n_slots; default: the powers of two below n_slots, and n_slots) that holds them.
        `pace`: `step(chunks, present=...)` holds the listeners whose chunk is late; every row owns its K / V ring position.
        `packets` (with `pace`): `push({slot: samples [2, n]})` takes the clients' packets at any size and `step()` takes no
        input — a device FIFO of `fifo_samples` (a power of two >= 256) per slot is re-framed into windows on the device;
        `pcm16`: packets and output are int16.
        `client_rate` (with `packets`): the clients' sample rate, a multiple of 125 Hz; `push` takes and `step` returns PCM at
        that rate, resampled on the device on the way in and on the way out.
        `monitor`: every slot has a wet / dry mix (`set_mix`), ramped on the device over `monitor_ramp` 16 kHz samples per
        full swing; `enroll(slot, embedder, passthrough=True)` lets the listener hear the room while they look."""
        return SessionStreamer(self, n_slots, device, use_graph, enroll_chunks, compact, row_buckets, pace, packets,
                               fifo_samples, pcm16, client_rate, monitor, monitor_ramp)

    def _enroll_side(self, dev) -> _EnrollSide:
        return _EnrollSide(dev, self.enroll_low_priority)

    # ------------------------------------------------------------------------------------------------
    # host-side plumbing
    # ------------------------------------------------------------------------------------------------
    @classmethod
    def from_packed(cls, path: str, device) -> "Net":
        """A separator whose weights come ONLY from a packed blob (`checkpoint.export_packed`, format in
        include/lookonce_weights.h): the blob's payload is uploaded in one copy and its tensors are handed to the C ABI
        as they are.  The parameter tree is dropped (nothing to pack, nothing to load) — this is the host a Python-free
        caller of the C ABI would write, with the launch sequence of `_separate`."""
        from . import checkpoint
        meta, flat = checkpoint.import_packed(path, device)
        if meta["model"] != "separator":
            raise ValueError(f"{path}: holds a {meta['model']!r} blob")
        if meta["abi_version"] != _cabi.ABI_VERSION:
            raise ValueError(f"{path}: packed for ABI v{meta['abi_version']}, library is v{_cabi.ABI_VERSION}")
        net = cls(**meta["params"]).eval()
        net.tfgridnet = None                                     # no parameters: the blob is the only weight source
        tree: dict = {"blocks": [dict() for _ in range(net.n_blocks)]}
        for name, t in flat.items():
            if name.startswith("blocks."):
                _, i, key = name.split(".", 2)
                tree["blocks"][int(i)][key] = t
            else:
                tree[name] = t
        net._blob = (next(iter(flat.values())).device, tree)
        return net

    def _weights(self, device) -> dict:
        if self._blob is not None:
            if torch.device(device) != self._blob[0]:
                raise RuntimeError(f"packed weights live on {self._blob[0]}, input on {device}")
            return self._blob[1]
        tensors = list(self.parameters()) + list(self.buffers())
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in tensors)
        if key != self._pack_key:
            sd = {k: v for k, v in self.state_dict(keep_vars=True).items()}
            for k, v in sd.items():
                if v.device != device:
                    raise RuntimeError(f"parameter {k} lives on {v.device}, input on {device}")
            with torch.no_grad():
                self._packed = pack_all(sd, self.n_blocks)
            self._pack_key = key
        return self._packed

    def _workspace(self, B, T, device) -> dict:
        key = (B, T, str(device))
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) > 4:
                self._ws.clear()
            F_, C_, nh = self.n_freqs, self.emb_dim, self.n_head
            e = lambda *s: torch.empty(*s, device=device, dtype=torch.float32)
            hist = self.local_atten_len - 1
            # q / kx / vx: split-precision fp16 rows (include/lookonce_hip.h); kx / vx carry KV_PAD_ROWS zero rows that
            # only this allocation ever writes
            z16 = lambda *s: torch.zeros(*s, device=device, dtype=torch.float16)
            ws = dict(xa=e(B, T, F_, C_), xb=e(B, T, F_, C_), xc=e(B, T, F_, C_), hbuf=e(B * T * F_, 2 * self.hidden),
                      q=z16(B * nh, T, 2 * QK_PAD), kx=z16(B * nh, T + hist + KV_PAD_ROWS, 2 * QK_PAD),
                      vx=z16(B * nh, T + hist + KV_PAD_ROWS, 2 * self.V_dim * F_), gain=e(B, F_, C_),
                      gain_raw=e(B, F_ * C_), hist_dirty=False)
            self._ws[key] = ws
        return ws

    @staticmethod
    def _dev_key(device) -> str:
        """'cuda' / torch.device('cuda') and 'cuda:N' of the current device are ONE key (`range_status('cuda')`
        must find the flag the forward keyed by `x.device` = 'cuda:0')."""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return str(dev)

    def _range_flag(self, device) -> torch.Tensor:
        """This Net's two-word range flag for `device` (include/lookonce_hip.h: [0] sticky, [1] unused here): pinned host
        memory — device-accessible, and readable by the host without a copy or a launch."""
        key = self._dev_key(device)
        if key not in self._range_flags:
            self._range_flags[key] = self._flag_words(torch.device(key))
        return self._range_flags[key]

    def range_status(self, device=None) -> bool:
        """Waits for the current stream of `device`, then reads and clears this Net's range flag: True when a forward since
        the last look produced non-finite samples.  Call it after the last forward of a loop (a set flag otherwise raises at
        the start of the next forward).  `device=None`: EVERY device this Net has run on (it used to look at the
        first one only)."""
        if device is None:
            keys = list(self._range_flags)
        else:
            keys = [self._dev_key(device)]
        bad = False
        for key in keys:
            dev = torch.device(key)
            flag = self._range_flag(dev)
            self._sync(dev)
            if int(flag[0]) != 0:
                flag.zero_()
                bad = True
        return bad

    def _sync(self, dev):
        torch.cuda.current_stream(dev).synchronize()

    _RANGE_MSG = ("LH_ERR_RANGE: {} produced non-finite samples. The frame kernels scale every row by a power of "
                  "two before the fp16 hi + lo split, so this means inf / NaN in the input or the state, or an activation "
                  "beyond the fp32 range itself (include/lookonce_hip.h, range contract).")

    def _zero_state(self, B, device) -> dict:
        key = (B, str(device))
        if key not in self._zeros:
            if len(self._zeros) > 4:
                self._zeros.clear()
            self._zeros[key] = self.init_buffers(B, device)        # read-only: the kernels write state to separate tensors
        return self._zeros[key]

    def _separate(self, x: torch.Tensor, embed: torch.Tensor, state: Optional[dict], want_state: bool = True):
        """TFGridNet.forward (reference tfgridnet_causal.py:188-283) on the HIP kernels."""
        if self.training and torch.is_grad_enabled():
            raise RuntimeError("lookoncetohear_amd.Net is an inference-only drop-in (forward kernels, no autograd): call "
                               ".eval() and/or run under torch.no_grad(); training stays on the reference model")
        self._check_gemm_mode()                 # before the first launch, not mid-forward
        if self.gemm_mode == "f32all":
            return self._separate_ref32(x, embed, state, want_state)
        lib = self._lib(x)
        dev = x.device
        if self.range_check and int(self._range_flag(dev)[0]) != 0:       # deferred look at the previous forwards' flag: a host read
            self._range_flag(dev).zero_()
            raise RuntimeError(self._RANGE_MSG.format("an earlier forward of this Net"))
        hop, nfft = self.stft_chunk_size, self.nfft
        assert x.dim() == 3 and x.shape[1] == self.num_ch, "input must be [B, num_ch, N]"
        Bn, _, n = x.shape
        from_zero = state is None and not want_state
        if state is None:
            state = self._zero_state(Bn, dev) if from_zero else self.init_buffers(Bn, dev)
        T = (n - nfft) // hop + 1
        if T < 1:
            raise ValueError(f"need at least {nfft} samples, got {n}")
        ns = (T - 1) * hop + nfft
        x = x[..., :ns].contiguous().float()
        embed = embed.contiguous().float()
        F_, C_, nh, H_ = self.n_freqs, self.emb_dim, self.n_head, self.hidden
        hist = self.local_atten_len - 1
        # raw launches go to the CURRENT HIP device: make it the tensors' device (the reference eval driver builds
        # `cuda:N` tensors without torch.cuda.set_device, src/ts_hear_test.py:175)
        with torch.no_grad(), self._device_ctx(x):
            pk = self._weights(dev)
            ws = self._workspace(Bn, T, dev)
            st = self._stream(dev)
            P = lambda t: t.data_ptr()
            new = lambda t: torch.empty_like(t, dtype=torch.float32)
            c32 = lambda t: t.contiguous().float()
            taps = self._debug_taps
            xa, xb, xc, hbuf = ws["xa"], ws["xb"], ws["xc"], ws["hbuf"]
            prof = self._prof
            only = self._prof_only                   # bench.py: restrict the event pairs to these C-ABI calls
            stride, count = self._prof_stride, self._prof_count

            class _Timed:                       # HIP events on the launch stream around each C-ABI call
                @staticmethod
                def call(fn, *args):
                    name = fn[:-4] if fn.endswith("_win") else fn       # a windowed call counts as its stage
                    if prof is None or (only is not None and name not in only):
                        return lib_.call(fn, *args)
                    if stride > 1:                  # sampled bracket: an event record costs ~6 us of stream time
                        n = count.get(name, 0)
                        count[name] = n + 1
                        if n % stride:
                            return lib_.call(fn, *args)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    lib_.call(fn, *args)
                    e1.record()
                    prof.append((name, e0, e1))

            lib_, lib = lib, _Timed

            conv_in = c32(state["conv_buf"]); conv_out = new(conv_in)
            lib.call("lh_stft_conv_in", P(x), P(conv_in), P(conv_out), P(pk["wfb_t"]), P(pk["conv_w"]),
                     P(pk["conv_b"]), P(xa), Bn, T, ns, st)
            lib.call("lh_embed_proj_ln", P(embed), P(pk["emb_w"]), P(pk["emb_b"]), P(pk["emb_ln_w"]),
                     P(pk["emb_ln_b"]), P(ws["gain_raw"]), P(ws["gain"]), Bn, st)
            if taps is not None:
                taps["Z0"], taps["G"] = xa.clone(), ws["gain"].clone()

            mode = 1 if self.gemm_mode == "f16x3" else 0
            K = self._n_time_chunks(Bn, T, mode)
            # tap products instead of the last block's frame: zero state in, nothing out, no stage taps (the last block has no
            # gain: only block 0 applies one, and with a single block nobody does)
            ptaps = None
            if self.fuse_taps and from_zero and taps is None:
                ptaps = self._tap_buffers(ws, Bn, T, dev, own=K > 1)
            if K > 1:
                self._blocks_chunked(lib, pk, ws, state, Bn, T, dev, from_zero, want_state, K, ptaps=ptaps)
            else:
                self._blocks_whole(lib, pk, ws, state, Bn, T, dev, from_zero, want_state, mode, ptaps=ptaps)

            y = torch.empty(Bn, self.n_srcs, hop * T, device=dev, dtype=torch.float32)
            flag = self._range_flag(dev)
            if ptaps is not None:
                lib.call("lh_taps_istft", P(ptaps[0]), P(ptaps[1]), P(pk["deconv_w"]), P(pk["deconv_b"]), P(pk["wfb_dec"]),
                         P(y), P(flag), 1, Bn, T, st)
            else:
                dec_in, ist_in = c32(state["deconv_buf"]), c32(state["istft_buf"])
                dec_out, ist_out = new(dec_in), new(ist_in)
                lib.call("lh_deconv_istft", P(xa), P(dec_in), P(dec_out), P(ist_in), P(ist_out), P(pk["deconv_w"]),
                         P(pk["deconv_b"]), P(pk["wfb_dec"]), P(y), P(flag), 1, Bn, T, st)
            if want_state:
                state["conv_buf"], state["deconv_buf"], state["istft_buf"] = conv_out, dec_out, ist_out
            if self.range_check == "sync" and not self._capturing():
                if self.range_status(dev):
                    raise RuntimeError(self._RANGE_MSG.format("this forward"))
        return y, (state if want_state else None)

    def _tap_buffers(self, ws, Bn, T, dev, own):
        """(P [B][T][97][36], fmax [B][T]) of `lh_proj_ln_res_taps` / `lh_taps_istft`.  On whole clips P lives in the storage of
        `xa`: the last block's closing stage is the only writer of `xa` and nothing reads it afterwards.  With time windows
        (`own`) a later window's intra stage still reads ITS frames of `xa` while an earlier window writes P — frame t of P is
        not where frame t of `xa` is — so P gets storage of its own, allocated on first use."""
        n = Bn * T * self.n_freqs * 36
        if "fmax" not in ws:
            ws["fmax"] = torch.empty(Bn * T, device=dev, dtype=torch.float32)
        if not own:
            return ws["xa"].view(-1)[:n], ws["fmax"]
        if "ptaps" not in ws:
            ws["ptaps"] = torch.empty(n, device=dev, dtype=torch.float32)
        return ws["ptaps"], ws["fmax"]

    def _separate_many(self, x: torch.Tensor, embeds: torch.Tensor) -> torch.Tensor:
        """`_separate` from the zero state for Kt speakers per mixture (`forward_many`): front end and block 0 on the Bn
        mixtures, blocks 1 ... and the back end on Bn * Kt rows (row b * Kt + j = mixture b, speaker j), each part with the
        kernels and windows `_separate` picks for its batch.  `fan` = (gain [Bn * Kt][97][64], out [Bn * Kt][T][97][64], Kt)
        is what block 0's last stage writes instead of its own batch's `xa`: no stage of block 0 reads that buffer, so its
        windows may run ahead of each other; the window streams join before block 1 starts."""
        if self.training and torch.is_grad_enabled():
            raise RuntimeError("lookoncetohear_amd.Net is an inference-only drop-in (forward kernels, no autograd): call "
                               ".eval() and/or run under torch.no_grad(); training stays on the reference model")
        self._check_gemm_mode()
        assert x.shape[1] == self.num_ch, "input must be [B, num_ch, N]"
        Bn, _, n = x.shape
        Kt = embeds.shape[1]
        Bk = Bn * Kt
        embed = embeds.reshape(Bk, -1)
        if self.gemm_mode == "f32all" or self.n_blocks < 2:       # nothing to share (one block: no gain at all)
            y, _ = self._separate(x.repeat_interleave(Kt, 0), embed, None, False)
            return y.view(Bn, Kt, *y.shape[1:])
        lib = self._lib(x)
        dev = x.device
        if self.range_check and int(self._range_flag(dev)[0]) != 0:       # as in `_separate`
            self._range_flag(dev).zero_()
            raise RuntimeError(self._RANGE_MSG.format("an earlier forward of this Net"))
        hop, nfft = self.stft_chunk_size, self.nfft
        T = (n - nfft) // hop + 1
        if T < 1:
            raise ValueError(f"need at least {nfft} samples, got {n}")
        ns = (T - 1) * hop + nfft
        x = x[..., :ns].contiguous().float()
        embed = embed.contiguous().float()
        with torch.no_grad(), self._device_ctx(x):
            pk = self._weights(dev)
            ws, wsk = self._workspace(Bn, T, dev), self._workspace(Bk, T, dev)
            s0, sk = self._zero_state(Bn, dev), self._zero_state(Bk, dev)
            st = self._stream(dev)
            P = lambda t: t.data_ptr()
            new = lambda t: torch.empty_like(t, dtype=torch.float32)
            c32 = lambda t: t.contiguous().float()
            conv_in = c32(s0["conv_buf"]); conv_out = new(conv_in)
            lib.call("lh_stft_conv_in", P(x), P(conv_in), P(conv_out), P(pk["wfb_t"]), P(pk["conv_w"]),
                     P(pk["conv_b"]), P(ws["xa"]), Bn, T, ns, st)
            lib.call("lh_embed_proj_ln", P(embed), P(pk["emb_w"]), P(pk["emb_b"]), P(pk["emb_ln_w"]),
                     P(pk["emb_ln_b"]), P(wsk["gain_raw"]), P(wsk["gain"]), Bk, st)
            mode = 1 if self.gemm_mode == "f16x3" else 0
            fan = (wsk["gain"], wsk["xa"], Kt)
            for w, s, rows, blocks, f in ((ws, s0, Bn, range(0, 1), fan), (wsk, sk, Bk, range(1, self.n_blocks), None)):
                K = self._n_time_chunks(rows, T, mode)
                if K > 1:
                    self._blocks_chunked(lib, pk, w, s, rows, T, dev, True, False, K, blocks, f)
                else:
                    self._blocks_whole(lib, pk, w, s, rows, T, dev, True, False, mode, blocks, f)
            dec_in, ist_in = c32(sk["deconv_buf"]), c32(sk["istft_buf"])
            dec_out, ist_out = new(dec_in), new(ist_in)
            y = torch.empty(Bn, Kt, self.n_srcs, hop * T, device=dev, dtype=torch.float32)
            lib.call("lh_deconv_istft", P(wsk["xa"]), P(dec_in), P(dec_out), P(ist_in), P(ist_out), P(pk["deconv_w"]),
                     P(pk["deconv_b"]), P(pk["wfb_dec"]), P(y), P(self._range_flag(dev)), 1, Bk, T, st)
            if self.range_check == "sync" and not self._capturing():
                if self.range_status(dev):
                    raise RuntimeError(self._RANGE_MSG.format("this forward"))
        return y

    def _blocks_whole(self, lib, pk, ws, state, Bn, T, dev, from_zero, want_state, mode, blocks=None, fan=None, ptaps=None):
        """The GridNet blocks (tfgridnet_causal.py:489-590) on whole clips: five stage launches per block on the current stream.
        `blocks`: the block indices to run (all of them by default); `fan`: see `_separate_many`; `ptaps`: (P, fmax) the last
        block's closing stage writes instead of its frame (`_separate`, `fuse_taps`)."""
        F_, nh, H_, hist = self.n_freqs, self.n_head, self.hidden, self.local_atten_len - 1
        P = lambda t: t.data_ptr()
        new = lambda t: torch.empty_like(t, dtype=torch.float32)
        c32 = lambda t: t.contiguous().float()
        xa, xb, xc, hbuf = ws["xa"], ws["xb"], ws["xc"], ws["hbuf"]
        st = self._stream(dev)
        taps = self._debug_taps
        rows = Bn * T * F_
        wkey, bkey = ("_w16", "_b16") if mode else ("_w", "_b")
        for i in (range(self.n_blocks) if blocks is None else blocks):
            bp = pk["blocks"][i]
            bs = state["gridnet_bufs"][f"buf{i}"]
            h0, c0 = c32(bs["h0"]), c32(bs["c0"])
            hN, cN = new(h0), new(c0)
            fuse = mode == 1 and self.fuse_linear
            # the fused intra path runs the two directions as consecutive launches (the reverse one accumulates into
            # the forward one's rows): worth it once a single direction fills the GPU, otherwise the unfused kernel
            # (both directions concurrently) has half the latency (streaming, batch 1)
            if fuse and Bn * T >= self.fuse_intra_min_frames:
                lib.call("lh_intra_block", P(xa), P(bp["intra_w16"]), P(bp["intra_b16"]), P(bp["intra_lin_w2"]),
                         P(bp["intra_lin_b"]), P(xb), Bn * T, st)
            elif mode == 1 and Bn * T <= self.stream_intra_max_frames:
                # a handful of frames (streaming): one workgroup per (frame, direction), mat-vec recurrence
                lib.call("lh_intra_stream", P(xa), P(bp["intra_s_wih"]), P(bp["intra_s_b"]), P(bp["intra_s_whh"]),
                         P(hbuf), Bn * T, st)
                lib.call("lh_linear_res", P(hbuf), P(bp["intra_lin_w"]), P(bp["intra_lin_b"]), P(xa), P(xb), rows,
                         2 * H_, st)
            else:
                # intra: LN + BiLSTM over frequency -> Linear(128->64) + residual
                lib.call("lh_ln_lstm_intra", P(xa), P(bp["intra_ln_w"]), P(bp["intra_ln_b"]), P(bp["intra" + wkey]),
                         P(bp["intra" + bkey]), P(hbuf), Bn * T, mode, st)
                lib.call("lh_linear_res", P(hbuf), P(bp["intra_lin_w"]), P(bp["intra_lin_b"]), P(xa), P(xb), rows,
                         2 * H_, st)
            if fuse and Bn * F_ <= self.inter_matvec_max_seqs and T >= 32:
                # few sequences, many steps (batch 1 offline): one workgroup per sequence, mat-vec recurrence
                lib.call("lh_inter_matvec", P(xb), P(bp["inter_s_wih"]), P(bp["inter_s_b"]), P(bp["inter_s_whh"]),
                         P(bp["inter_lin_w"]), P(bp["inter_lin_b"]), P(h0), P(c0), P(hN), P(cN), P(xc), Bn, T, st)
            elif fuse:
                lib.call("lh_inter_block", P(xb), P(bp["inter_w8"]), P(bp["inter_b16"]), P(bp["inter_lin_wu"]),
                         P(bp["inter_lin_b"]), P(h0), P(c0), P(hN), P(cN), P(xc), Bn, T, st)
            else:
                # inter: LN + causal LSTM over time with carried state -> Linear(64->64) + residual
                lib.call("lh_ln_lstm_inter", P(xb), P(bp["inter_ln_w"]), P(bp["inter_ln_b"]), P(bp["inter" + wkey]),
                         P(bp["inter" + bkey]), P(h0), P(c0), P(hN), P(cN), P(hbuf), Bn, T, mode, st)
                lib.call("lh_linear_res", P(hbuf), P(bp["inter_lin_w"]), P(bp["inter_lin_b"]), P(xb), P(xc), rows,
                         H_, st)
            # attention: history rows in, Q/K/V, local attention (head merge fused), projection + LN + residual
            if not from_zero:
                lib.call("lh_ring_pack", P(c32(bs["K_buf"])), P(c32(bs["V_buf"])), P(ws["kx"]), P(ws["vx"]), Bn, T, st)
                ws["hist_dirty"] = True
            elif ws["hist_dirty"]:                      # history rows of the window-extended buffers back to zero
                ws["kx"][:, :hist].zero_()
                ws["vx"][:, :hist].zero_()
                ws["hist_dirty"] = False
            lib.call("lh_qkv_proj_ln", P(xc), P(bp["qkv_w"]), P(bp["qkv_b"]), P(bp["qkv_slopes"]), P(bp["lnq_w"]),
                     P(bp["lnq_b"]), P(bp["lnk_w"]), P(bp["lnk_b"]), P(bp["lnv_w"]), P(bp["lnv_b"]), P(ws["q"]),
                     P(ws["kx"]), P(ws["vx"]), None, Bn, T, st)
            lib.call("lh_local_attn", P(ws["q"]), P(ws["kx"]), P(ws["vx"]), P(xb), Bn, T, st)
            if taps is not None:
                taps[f"blocks.{i}.attn"] = xb.clone()          # head-major [B][T][4][97][16]
            gain = ws["gain"] if (i == 0 and self.n_blocks > 1) else None   # `batch * embed` before block 1
            if fan is not None and i == 0:
                lib.call("lh_proj_ln_res_fan", P(xb), P(bp["proj_w"]), P(bp["proj_b"]), P(bp["proj_slope"]),
                         P(bp["proj_ln_w"]), P(bp["proj_ln_b"]), P(xc), P(fan[0]), P(fan[1]), Bn, T, fan[2], st)
            elif ptaps is not None and i == self.n_blocks - 1 and gain is None:
                lib.call("lh_proj_ln_res_taps", P(xb), P(bp["proj_w"]), P(bp["proj_b"]), P(bp["proj_slope"]),
                         P(bp["proj_ln_w"]), P(bp["proj_ln_b"]), P(xc), P(pk["deconv_w"]), P(ptaps[0]), P(ptaps[1]), Bn, T, st)
            else:
                lib.call("lh_proj_ln_res", P(xb), P(bp["proj_w"]), P(bp["proj_b"]), P(bp["proj_slope"]),
                         P(bp["proj_ln_w"]), P(bp["proj_ln_b"]), P(xc), P(gain) if gain is not None else None, P(xa),
                         Bn, T, st)
            if want_state:
                bs["h0"], bs["c0"] = hN, cN
                bs["K_buf"] = torch.empty(Bn * nh, hist, self.E * F_, device=dev, dtype=torch.float32)
                bs["V_buf"] = torch.empty(Bn * nh, hist, self.V_dim * F_, device=dev, dtype=torch.float32)
                lib.call("lh_ring_unpack", P(ws["kx"]), P(ws["vx"]), P(bs["K_buf"]), P(bs["V_buf"]), Bn, T, st)
            if taps is not None:
                taps[f"blocks.{i}.Y2"] = xc.clone()
                taps[f"blocks.{i}.Q"] = unsplit_qk(ws["q"], self.E * F_)
                taps[f"blocks.{i}.K"] = unsplit_qk(ws["kx"][:, hist:hist + T], self.E * F_)
                taps[f"blocks.{i}.V"] = unsplit_v(ws["vx"][:, hist:hist + T])
                taps[f"blocks.{i}.out"] = xa.clone()

    def _n_time_chunks(self, Bn: int, T: int, mode: int) -> int:
        """Windows the block loop is cut into (see `time_chunks` / `time_chunks_small` in __init__); 1 for streaming-size
        inputs, stage taps and the exact-fp32 modes.  Every window keeps at least `chunk_min_frames` (>= the 49 frames of
        attention history: a window then depends on ONE predecessor)."""
        if mode != 1 or not self.fuse_linear or self._debug_taps is not None:
            return 1
        if Bn * self.n_freqs <= self.inter_matvec_max_seqs and T < 32:
            return 1                                             # (the per-sequence inter kernel serves T >= 32, `_separate`)
        if Bn * T < self.fuse_intra_min_frames:                  # small batches: unfused intra pair
            if Bn * T <= self.stream_intra_max_frames:
                return 1                                         # a handful of frames: the streaming intra kernel
            K = int(self.time_chunks_small)
            if K == 0:                                           # automatic (profiles/r06h_batch_sweep_windows.txt)
                nseq = Bn * self.n_freqs
                K = 3
                if nseq <= self.inter_matvec_max_seqs:
                    # per-sequence inter kernel (one workgroup per sequence, B <= 2): windows only pay while its workgroups leave
                    # CUs dark (B = 1: 97 of 256 -> -14 %; B = 2: 194 -> +5 %); one utterance is best in two (three: 1.18 against
                    # 1.12 ms)
                    tail = nseq % self.n_cus or self.n_cus
                    K = 1 if tail >= 0.6 * self.n_cus else (2 if nseq <= self.n_cus else 3)
        else:
            K = int(self.time_chunks)
            if K == 0:                                           # automatic
                tiles = (Bn * self.n_freqs + 15) // 16           # workgroups (= CUs) of the inter launch
                K = 2 if tiles < 0.7 * self.n_cus else 1
            while K > 1 and Bn * (T // K) < self.fuse_intra_min_frames // 2:
                K -= 1
        return max(min(K, T // max(self.chunk_min_frames, 1)), 1)

    def _window_bounds(self, Bn: int, T: int, K: int) -> list:
        """Window boundaries [0, ..., T]: even cuts, moved to multiples of the attention kernel's query-tile length (the library
        says which it uses for this batch and clip: `lh_attn_tile_frames`) when the windows are long enough — the windows then
        cut the time axis into exactly the tiles of the whole-clip launch and the forward is bit-identical to the unchunked one
        (every other stage is per frame or per sequence)."""
        frames = ctypes.c_int(0)
        self._lib(next(self.parameters())).call("lh_attn_tile_frames", Bn, T, ctypes.addressof(frames))
        align = max(frames.value, 32)                         # (clips of one 16-frame tile are never cut)
        if Bn * self.n_freqs <= self.inter_matvec_max_seqs:
            align = 64                                        # lh_inter_matvec's chunk of steps (a multiple of the 32-frame tile)
        cuts = [(k * T) // K for k in range(K + 1)]
        moved = [0] + [int(round(k * T / K / align)) * align for k in range(1, K)] + [T]
        # long enough: two tiles per window, or (79-frame tiles at K = 4: 156 frames) every moved window still holds a whole
        # tile and the frames a window must keep
        whole = min(b - a for a, b in zip(moved, moved[1:])) >= max(align, self.chunk_min_frames)
        if T // K >= 2 * align or (align == 64 and T // K >= 64) or whole:
            cuts = moved
        return cuts

    def _lanes(self, dev, K) -> _Lanes:
        # ONE pool of side streams per device, grown on demand and shared by every window count: the process has four hardware
        # queues, and every further stream shares one with somebody (a bench run that had left six window streams behind slowed
        # the EMBEDDER's two-stream forward from 59.7 to 68.4 ms: its side stream had landed on a busy queue)
        pool = self._chunk_streams.setdefault(str(dev), [])
        while len(pool) < K - 1:
            pool.append(torch.cuda.Stream(device=dev))
        if self.chunk_min_frames < self.local_atten_len - 1:
            raise ValueError("chunk_min_frames must cover the attention history (49 frames) on concurrent streams")
        return _Lanes(dev, pool[:K - 1])

    def _blocks_chunked(self, lib, pk, ws, state, Bn, T, dev, from_zero, want_state, K, blocks=None, fan=None, ptaps=None):
        """The three GridNet blocks (tfgridnet_causal.py:489-590) with the time axis cut into K windows, window k on stream k:
        for block i and window k the five stage launches of `_separate` through the `_win` entry points, with two cross-stream
        dependences per (block, window) — the inter LSTM's (h, c) and the K / V rows of the previous window.
        `blocks`: the block indices to run (all of them by default); `fan`: see `_separate_many`; `ptaps`: see `_blocks_whole`."""
        blocks = range(self.n_blocks) if blocks is None else blocks
        F_, nh, hist = self.n_freqs, self.n_head, self.local_atten_len - 1
        P = lambda t: t.data_ptr()
        c32 = lambda t: t.contiguous().float()
        xa, xb, xc = ws["xa"], ws["xb"], ws["xc"]
        lanes = self._lanes(dev, K)
        # the whole-clip rules of `_separate`, per batch: which intra / inter kernels the windows run
        unfused_intra = Bn * T < self.fuse_intra_min_frames
        matvec_inter = Bn * F_ <= self.inter_matvec_max_seqs
        if "kxb" not in ws:                                   # one history-extended K / V pair per block
            z16 = lambda *s_: torch.zeros(*s_, device=dev, dtype=torch.float16)
            ws["kxb"] = [ws["kx"]] + [z16(*ws["kx"].shape) for _ in range(self.n_blocks - 1)]
            ws["vxb"] = [ws["vx"]] + [z16(*ws["vx"].shape) for _ in range(self.n_blocks - 1)]
            ws["hist_dirty_b"] = [False] * self.n_blocks
        bounds = self._window_bounds(Bn, T, K)
        # per block: (h, c) of every window boundary; history rows in place (on the current stream, before the fork)
        hs, cs = {}, {}
        for i in blocks:
            bs = state["gridnet_bufs"][f"buf{i}"]
            h0, c0 = c32(bs["h0"]).reshape(-1, self.hidden), c32(bs["c0"]).reshape(-1, self.hidden)
            hs[i] = [h0] + [torch.empty_like(h0) for _ in range(K)]
            cs[i] = [c0] + [torch.empty_like(c0) for _ in range(K)]
            kx, vx = ws["kxb"][i], ws["vxb"][i]
            if not from_zero:
                lib.call("lh_ring_pack", P(c32(bs["K_buf"])), P(c32(bs["V_buf"])), P(kx), P(vx), Bn, T, self._stream(dev))
                ws["hist_dirty_b"][i] = True
                if i == 0:
                    ws["hist_dirty"] = True                   # block 0's pair is the unchunked path's one pair
            elif ws["hist_dirty_b"][i] or (i == 0 and ws["hist_dirty"]):
                kx[:, :hist].zero_()
                vx[:, :hist].zero_()
                ws["hist_dirty_b"][i] = False
                if i == 0:
                    ws["hist_dirty"] = False
        lanes.fork()
        for i in blocks:
            bp = pk["blocks"][i]
            kx, vx = ws["kxb"][i], ws["vxb"][i]
            gain = ws["gain"] if (i == 0 and self.n_blocks > 1) else None
            ev_r = ev_q = None                                # the previous window's (h, c) / K, V rows of THIS block
            for k in range(K):
                t0, Tc = bounds[k], bounds[k + 1] - bounds[k]
                carry = (1 if k > 0 else 0) | (2 if k + 1 < K else 0)     # inner boundaries: internal cell-state form
                with lanes.on(k):
                    st = self._stream(dev)
                    if unfused_intra:
                        lib.call("lh_ln_lstm_intra_win", P(xa), P(bp["intra_ln_w"]), P(bp["intra_ln_b"]), P(bp["intra_w16"]),
                                 P(bp["intra_b16"]), P(ws["hbuf"]), Bn, T, t0, Tc, st)
                        lib.call("lh_linear_res_win", P(ws["hbuf"]), P(bp["intra_lin_w"]), P(bp["intra_lin_b"]), P(xa), P(xb),
                                 Bn, T, t0, Tc, 2 * self.hidden, st)
                    else:
                        lib.call("lh_intra_block_win", P(xa), P(bp["intra_w16"]), P(bp["intra_b16"]), P(bp["intra_lin_w2"]),
                                 P(bp["intra_lin_b"]), P(xb), Bn, T, t0, Tc, st)
                    if k > 0:
                        lanes.wait(k, ev_r)
                    if matvec_inter:
                        lib.call("lh_inter_matvec_win", P(xb), P(bp["inter_s_wih"]), P(bp["inter_s_b"]), P(bp["inter_s_whh"]),
                                 P(bp["inter_lin_w"]), P(bp["inter_lin_b"]), P(hs[i][k]), P(cs[i][k]), P(hs[i][k + 1]),
                                 P(cs[i][k + 1]), P(xc), Bn, T, t0, Tc, carry, st)
                    else:
                        lib.call("lh_inter_block_win", P(xb), P(bp["inter_w8"]), P(bp["inter_b16"]), P(bp["inter_lin_wu"]),
                                 P(bp["inter_lin_b"]), P(hs[i][k]), P(cs[i][k]), P(hs[i][k + 1]), P(cs[i][k + 1]), P(xc), Bn, T,
                                 t0, Tc, carry, st)
                    if k + 1 < K:
                        ev_r = lanes.signal(k)
                    lib.call("lh_qkv_proj_ln_win", P(xc), P(bp["qkv_w"]), P(bp["qkv_b"]), P(bp["qkv_slopes"]), P(bp["lnq_w"]),
                             P(bp["lnq_b"]), P(bp["lnk_w"]), P(bp["lnk_b"]), P(bp["lnv_w"]), P(bp["lnv_b"]), P(ws["q"]),
                             P(kx), P(vx), None, Bn, T, t0, Tc, st)
                    ev_prev = ev_q
                    if k + 1 < K:
                        ev_q = lanes.signal(k)
                    if k > 0:
                        lanes.wait(k, ev_prev)
                    lib.call("lh_local_attn_win", P(ws["q"]), P(kx), P(vx), P(xb), Bn, T, t0, Tc, st)
                    if fan is not None and i == 0:
                        lib.call("lh_proj_ln_res_fan_win", P(xb), P(bp["proj_w"]), P(bp["proj_b"]), P(bp["proj_slope"]),
                                 P(bp["proj_ln_w"]), P(bp["proj_ln_b"]), P(xc), P(fan[0]), P(fan[1]), Bn, T, t0, Tc, fan[2], st)
                    elif ptaps is not None and i == self.n_blocks - 1 and gain is None:
                        lib.call("lh_proj_ln_res_taps_win", P(xb), P(bp["proj_w"]), P(bp["proj_b"]), P(bp["proj_slope"]),
                                 P(bp["proj_ln_w"]), P(bp["proj_ln_b"]), P(xc), P(pk["deconv_w"]), P(ptaps[0]), P(ptaps[1]), Bn, T,
                                 t0, Tc, st)
                    else:
                        lib.call("lh_proj_ln_res_win", P(xb), P(bp["proj_w"]), P(bp["proj_b"]), P(bp["proj_slope"]),
                                 P(bp["proj_ln_w"]), P(bp["proj_ln_b"]), P(xc), P(gain) if gain is not None else None, P(xa),
                                 Bn, T, t0, Tc, st)
        lanes.join()
        if want_state:
            for i in blocks:
                bs = state["gridnet_bufs"][f"buf{i}"]
                bs["h0"], bs["c0"] = hs[i][K].reshape(1, -1, self.hidden), cs[i][K].reshape(1, -1, self.hidden)
                bs["K_buf"] = torch.empty(Bn * nh, hist, self.E * F_, device=dev, dtype=torch.float32)
                bs["V_buf"] = torch.empty(Bn * nh, hist, self.V_dim * F_, device=dev, dtype=torch.float32)
                lib.call("lh_ring_unpack", P(ws["kxb"][i]), P(ws["vxb"][i]), P(bs["K_buf"]), P(bs["V_buf"]), Bn, T,
                         self._stream(dev))

    def _check_gemm_mode(self):
        if self.gemm_mode not in ("f32rec", "f32all", "f16x3"):
            raise ValueError(f"gemm_mode / LOOKONCE_GEMM must be 'f16x3', 'f32rec' or 'f32all', got {self.gemm_mode!r}"
                             + (" ('f32' was the pre-round-5 spelling of 'f32rec')" if self.gemm_mode == "f32" else ""))

    def _capturing(self) -> bool:
        return torch.cuda.is_current_stream_capturing()

    def _separate_ref32(self, x: torch.Tensor, embed: torch.Tensor, state: Optional[dict], want_state: bool = True):
        """`gemm_mode = "f32all"`: the same forward with EVERY contraction in plain fp32 — the exact fp32-MFMA recurrences
        (`lh_ln_lstm_intra / _inter`, LH_GEMM_F32) between the plain-fp32 reference kernels of lh_ref32.hip for the frame
        stages (weights straight from the state dict, Q / K / V as fp32 rows).  Slow (~50x), allocation-happy, test /
        diagnosis only: the in-tree A/B that tells split-precision error from a kernel bug (reference arithmetic:
        tfgridnet_causal.py:188-283 is fp32 end to end)."""
        if self._blob is not None:
            raise RuntimeError("gemm_mode='f32all' reads the parameter tree; a `from_packed` Net has none")
        lib = self._lib(x)
        dev = x.device
        hop, nfft = self.stft_chunk_size, self.nfft
        assert x.dim() == 3 and x.shape[1] == self.num_ch, "input must be [B, num_ch, N]"
        Bn, _, n = x.shape
        if state is None:
            state = self.init_buffers(Bn, dev)
        T = (n - nfft) // hop + 1
        if T < 1:
            raise ValueError(f"need at least {nfft} samples, got {n}")
        ns = (T - 1) * hop + nfft
        x = x[..., :ns].contiguous().float()
        embed = embed.contiguous().float()
        F_, C_, nh, H_ = self.n_freqs, self.emb_dim, self.n_head, self.hidden
        hist = self.local_atten_len - 1
        rows = Bn * T * F_
        with torch.no_grad(), self._device_ctx(x):
            pk = self._weights(dev)                    # only the fp32-MFMA LSTM images and the speaker-gain tensors
            sd = {k: v.detach().float().contiguous() for k, v in self.tfgridnet.state_dict().items()}
            st = self._stream(dev)
            P = lambda t: t.data_ptr()
            e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
            c32 = lambda t: t.contiguous().float()
            xa, xb, xc, hbuf = e(Bn, T, F_, C_), e(Bn, T, F_, C_), e(Bn, T, F_, C_), e(rows, 2 * H_)
            gain_raw, gain = e(Bn, F_ * C_), e(Bn, F_, C_)
            conv_in = c32(state["conv_buf"]); conv_out = torch.empty_like(conv_in)
            spec_s, sx_s = e(Bn, 2 * self.num_ch, T + 2, F_), e(Bn, self.n_srcs, T + 1, 2 * F_)   # scratch: named, so they outlive the calls
            lib.call("lh_ref32_stft_conv_in", P(x), P(conv_in), P(conv_out), P(sd["enc.filterbank._filters"]),
                     P(sd["conv.0.weight"]), P(sd["conv.0.bias"]), P(spec_s), P(xa), Bn, T, ns, st)
            lib.call("lh_embed_proj_ln", P(embed), P(pk["emb_w"]), P(pk["emb_b"]), P(pk["emb_ln_w"]), P(pk["emb_ln_b"]),
                     P(gain_raw), P(gain), Bn, st)                                   # plain fp32 in every mode
            taps = self._debug_taps
            if taps is not None:
                taps["Z0"], taps["G"] = xa.clone(), gain.clone()
            pre, rows_s, pre_s = e(rows, 112), e(rows, C_), e(rows, C_)
            q = e(Bn * nh, T, self.E * F_)
            for i in range(self.n_blocks):
                bp, bs, g = pk["blocks"][i], state["gridnet_bufs"][f"buf{i}"], f"blocks.{i}."
                h0, c0 = c32(bs["h0"]), c32(bs["c0"])
                hN, cN = torch.empty_like(h0), torch.empty_like(c0)
                lib.call("lh_ln_lstm_intra", P(xa), P(bp["intra_ln_w"]), P(bp["intra_ln_b"]), P(bp["intra_w"]), P(bp["intra_b"]),
                         P(hbuf), Bn * T, 0, st)
                lib.call("lh_ref32_linear", P(hbuf), P(sd[g + "intra_linear.weight"]), P(sd[g + "intra_linear.bias"]), None,
                         P(xa), P(xb), rows, 2 * H_, C_, st)
                lib.call("lh_ln_lstm_inter", P(xb), P(bp["inter_ln_w"]), P(bp["inter_ln_b"]), P(bp["inter_w"]), P(bp["inter_b"]),
                         P(h0), P(c0), P(hN), P(cN), P(hbuf), Bn, T, 0, st)
                lib.call("lh_ref32_linear", P(hbuf), P(sd[g + "inter_linear.weight"]), P(sd[g + "inter_linear.bias"]), None,
                         P(xb), P(xc), rows, H_, C_, st)
                # Q | K | V: Linear + PReLU (one launch per projection: each has its own slope), head split + LayerNorm
                kx, vx = e(Bn * nh, T + hist, self.E * F_), e(Bn * nh, T + hist, self.V_dim * F_)
                kx[:, :hist] = bs["K_buf"].float()
                vx[:, :hist] = bs["V_buf"].float()
                for nm, D, dst, row0, rpb in (("Q", self.E, q, 0, T), ("K", self.E, kx, hist, T + hist),
                                              ("V", self.V_dim, vx, hist, T + hist)):
                    a = g + f"attn_conv_{nm}."
                    ncol = nh * D
                    lib.call("lh_ref32_linear", P(xc), P(sd[a + "0.weight"]), P(sd[a + "0.bias"]), P(sd[a + "1.weight"]), None,
                             P(pre), rows, C_, ncol, st)
                    lib.call("lh_ref32_head_ln", P(pre), ncol, 0, D, P(sd[a + "3.norm.weight"]), P(sd[a + "3.norm.bias"]),
                             P(dst), row0, rpb, Bn, T, st)
                lib.call("lh_ref32_local_attn", P(q), P(kx), P(vx), P(xb), Bn, T, st)
                a = g + "attn_concat_proj."
                gn = gain if (i == 0 and self.n_blocks > 1) else None
                lib.call("lh_ref32_proj_ln_res", P(xb), P(sd[a + "0.weight"]), P(sd[a + "0.bias"]), P(sd[a + "1.weight"]),
                         P(sd[a + "3.norm.weight"]), P(sd[a + "3.norm.bias"]), P(xc), P(gn) if gn is not None else None,
                         P(rows_s), P(pre_s), P(xa), Bn, T, st)
                if want_state:
                    bs["h0"], bs["c0"] = hN, cN
                    bs["K_buf"], bs["V_buf"] = kx[:, T:T + hist].clone(), vx[:, T:T + hist].clone()
                if taps is not None:
                    taps[f"blocks.{i}.Y2"], taps[f"blocks.{i}.Q"] = xc.clone(), q.clone()
                    taps[f"blocks.{i}.K"], taps[f"blocks.{i}.V"] = kx[:, hist:].clone(), vx[:, hist:].clone()
                    taps[f"blocks.{i}.out"] = xa.clone()
            dec_in, ist_in = c32(state["deconv_buf"]), c32(state["istft_buf"])
            dec_out, ist_out = torch.empty_like(dec_in), torch.empty_like(ist_in)
            y = e(Bn, self.n_srcs, hop * T)
            lib.call("lh_ref32_deconv_istft", P(xa), P(dec_in), P(dec_out), P(ist_in), P(ist_out), P(sd["deconv.weight"]),
                     P(sd["deconv.bias"]), P(sd["dec.filterbank._filters"]), P(sx_s), P(y), Bn, T, st)
            if want_state:
                state["conv_buf"], state["deconv_buf"], state["istft_buf"] = conv_out, dec_out, ist_out
        return y, (state if want_state else None)

    # ------------------------------------------------------------------------------------------------
    # streaming fast path (Streamer)
    # ------------------------------------------------------------------------------------------------
    def _speaker_gain(self, embed: torch.Tensor, gain_raw: torch.Tensor, gain: torch.Tensor):
        """gain[b][f][c] = LayerNorm(Linear(embed)) (reference tfgridnet_causal.py:247-248) into preallocated tensors."""
        lib = self._lib(embed)
        pk = self._weights(embed.device)
        st = self._stream(embed.device)
        P = lambda t: t.data_ptr()
        with self._device_ctx(embed):
            lib.call("lh_embed_proj_ln", P(embed), P(pk["emb_w"]), P(pk["emb_b"]), P(pk["emb_ln_w"]), P(pk["emb_ln_b"]),
                     P(gain_raw), P(gain), embed.shape[0], st)

    def _speaker_gain_rows(self, embed: torch.Tensor, gain_raw: torch.Tensor, gain: torch.Tensor, items: torch.Tensor):
        """`_speaker_gain` for the rows of an item table [k, 4] on the device (lh_snap_item_t): gain[row] from embed[slot],
        every tensor whole, [S, ...].  The same two kernels whatever k is; a row's bits are those of the per-row call."""
        lib = self._lib(embed)
        pk = self._weights(embed.device)
        st = self._stream(embed.device)
        P = lambda t: t.data_ptr()
        with self._device_ctx(embed):
            lib.call("lh_embed_proj_ln_rows", P(embed), P(pk["emb_w"]), P(pk["emb_b"]), P(pk["emb_ln_w"]), P(pk["emb_ln_b"]),
                     P(gain_raw), P(gain), P(items), items.shape[0], embed.shape[0], st)

    def _stream_chunk(self, x, gain, sin: dict, sout: dict, rings, pos, y, pk: dict, ws: dict, flag=None,
                      keep_nonfinite: int = 0, write_pos=None):
        """One chunk of ONE frame for `Streamer`: the launches of `_separate` with every state tensor read from `sin` and
        written to `sout` (preallocated), the K / V history in per-block persistent rings, the speaker gain given.
        `pk` / `ws`: the packed weights and the T=1 workspace, OWNED by the caller — a captured graph holds raw pointers
        into them, so they must not be the entries `_weights` / `_workspace` may replace or evict later.
        `keep_nonfinite`: lh_deconv_istft's switch — 0 for `Streamer` (silence, not NaN, reaches a listener), 1 for
        `SessionStreamer`, whose own last kernel looks at the samples and silences the slot.
        `write_pos` [B] (a paced `SessionStreamer`): every row's own ring slot, negative = the row writes no K / V row
        (`lh_qkv_proj_ln_rows`); `pos` is then not looked at."""
        lib = self._lib(x)
        dev = x.device
        hop, nfft = self.stft_chunk_size, self.nfft
        Bn, _, n = x.shape
        T = (n - nfft) // hop + 1
        assert T == 1 and n == nfft, "the streaming path takes chunks of stft_chunk_size + stft_pad_size samples"
        F_, H_ = self.n_freqs, self.hidden
        st = self._stream(dev)
        P = lambda t: t.data_ptr()
        xa, xb, xc, hbuf = ws["xa"], ws["xb"], ws["xc"], ws["hbuf"]
        lib.call("lh_stft_conv_in", P(x), P(sin["conv_buf"]), P(sout["conv_buf"]), P(pk["wfb_t"]), P(pk["conv_w"]),
                 P(pk["conv_b"]), P(xa), Bn, T, n, st)
        for i in range(self.n_blocks):
            bp = pk["blocks"][i]
            kx, vx = rings[i]
            lib.call("lh_intra_stream", P(xa), P(bp["intra_s_wih"]), P(bp["intra_s_b"]), P(bp["intra_s_whh"]), P(hbuf),
                     Bn * T, st)
            lib.call("lh_linear_res", P(hbuf), P(bp["intra_lin_w"]), P(bp["intra_lin_b"]), P(xa), P(xb), Bn * T * F_,
                     2 * H_, st)
            lib.call("lh_inter_block", P(xb), P(bp["inter_w8"]), P(bp["inter_b16"]), P(bp["inter_lin_wu"]),
                     P(bp["inter_lin_b"]), P(sin["h"][i]), P(sin["c"][i]), P(sout["h"][i]), P(sout["c"][i]), P(xc), Bn, T, st)
            if write_pos is None:
                lib.call("lh_qkv_proj_ln", P(xc), P(bp["qkv_w"]), P(bp["qkv_b"]), P(bp["qkv_slopes"]), P(bp["lnq_w"]),
                         P(bp["lnq_b"]), P(bp["lnk_w"]), P(bp["lnk_b"]), P(bp["lnv_w"]), P(bp["lnv_b"]), P(ws["q"]),
                         P(kx), P(vx), P(pos), Bn, T, st)
            else:
                lib.call("lh_qkv_proj_ln_rows", P(xc), P(bp["qkv_w"]), P(bp["qkv_b"]), P(bp["qkv_slopes"]), P(bp["lnq_w"]),
                         P(bp["lnq_b"]), P(bp["lnk_w"]), P(bp["lnk_b"]), P(bp["lnv_w"]), P(bp["lnv_b"]), P(ws["q"]),
                         P(kx), P(vx), P(write_pos), Bn, st)
            lib.call("lh_local_attn", P(ws["q"]), P(kx), P(vx), P(xb), Bn, T, st)
            g = gain if (i == 0 and self.n_blocks > 1) else None
            lib.call("lh_proj_ln_res", P(xb), P(bp["proj_w"]), P(bp["proj_b"]), P(bp["proj_slope"]),
                     P(bp["proj_ln_w"]), P(bp["proj_ln_b"]), P(xc), P(g) if g is not None else None, P(xa), Bn, T, st)
        lib.call("lh_deconv_istft", P(xa), P(sin["deconv_buf"]), P(sout["deconv_buf"]), P(sin["istft_buf"]),
                 P(sout["istft_buf"]), P(pk["deconv_w"]), P(pk["deconv_b"]), P(pk["wfb_dec"]), P(y),
                 P(flag) if flag is not None else None, keep_nonfinite, Bn, T, st)



class Streamer:
    """8 ms-chunk streaming driver (reference usage: `Net.predict(chunk[B,2,192], embed[B,256], state, pad=False)`
    in a loop) with the per-chunk launch sequence captured once into HIP graphs.

    One chunk = 128 new samples + 64 look-ahead samples -> 128 output samples.  Everything the chunk loop touches is
    static device memory, and nothing is copied that a kernel can write in place:
      * conv / deconv / iSTFT tails and the inter-LSTM (h, c) exist twice; even chunks read set 0 and write set 1, odd
        chunks the other way round (two captured graphs, replayed alternately);
      * the K / V history of each block is a persistent 50-row ring in the attention kernel's own split-precision
        layout: the new row goes to slot (chunk mod 50) (`lh_qkv_proj_ln` ring_pos, a device counter the graph
        increments), and as the 50 rows are exactly the window of the chunk's one frame, nothing is ever moved;
      * the speaker gain LayerNorm(Linear(embedding)) is computed once in `set_embedding`.
    `step()` is: copy the chunk in, replay a graph, hand back the output buffer (a view that the next `step`
    overwrites).  `use_graph=False` runs the same launches eagerly (also what the capture warm-up does).
    Measured (MI355X, batch 1): 0.68 ms per chunk with the generic `predict` path captured in one graph, see DESIGN.md.
    """

    def __init__(self, net: Net, batch_size: int, device, use_graph: bool = True):
        if net.gemm_mode != "f16x3" or not net.fuse_linear:
            raise ValueError("Streamer runs the split-precision fused kernels (LOOKONCE_GEMM=f16x3, LOOKONCE_FUSE=1)")
        self.net = net
        self.B = B = batch_size
        self.device = dev = torch.device(device)
        n = net.stft_chunk_size + net.stft_pad_size
        z = lambda *s, **k: torch.zeros(*s, device=dev, **k)
        self.chunk = z(B, net.num_ch, n)
        self.embed = z(B, net.spk_emb_dim)
        self.out = z(B, net.n_srcs, net.stft_chunk_size)
        F_, C_, nh, H_ = net.n_freqs, net.emb_dim, net.n_head, net.hidden
        mk = lambda: dict(conv_buf=z(B, net.num_ch * 2, 2, F_), deconv_buf=z(B, C_, 2, F_),
                          istft_buf=z(B, net.n_srcs, F_ * 2, 1),
                          h=[z(1, B * F_, H_) for _ in range(net.n_blocks)], c=[z(1, B * F_, H_) for _ in range(net.n_blocks)])
        self.sets = [mk(), mk()]
        rows = 1 + net.local_atten_len - 1 + KV_PAD_ROWS
        self.rings = [(z(B * nh, rows, 2 * QK_PAD, dtype=torch.float16), z(B * nh, rows, 2 * net.V_dim * F_, dtype=torch.float16))
                      for _ in range(net.n_blocks)]
        self.pos = z(1, dtype=torch.int32)
        self.gain = z(B, F_, C_)
        self.gain_raw = z(B, F_ * C_)
        # range guard: THIS streamer's own two-word flag (never shared with the Net's offline forwards or another streamer);
        # a non-finite chunk (output: zeros) raises at the first `step` after that chunk has finished on the device.
        # On the GPU the flag lives in PINNED HOST memory (device-accessible under unified addressing): the back end stores
        # to it directly in the rare chunk that needs it and `step` just reads the word — no exchange kernel, no copy, no
        # extra launches in the chunk loop (round 3 polled with a kernel + copy every 64th chunk: +0.15 ms on that chunk,
        # which was the p99 of the latency distribution).
        self.range_flag = net._flag_words(dev)
        self.parity = 0
        self.graphs = None
        self.graph = None
        # strong references: the captured graphs bake in pointers into the packed weights and the T=1 workspace.
        # `Net._workspace` evicts its cache after a few shapes and `Net._weights` re-packs after any parameter change;
        # holding the objects here keeps the memory alive, and `step` refuses to replay once the weights were re-packed.
        with torch.no_grad(), net._device_ctx(self.chunk):
            self._pk = net._weights(dev)
            self._pack_key = net._pack_key
            self._n_steps = 0
            # (tensor, version at build time) of every parameter / buffer: `step` re-checks a few per chunk, round robin
            self._versions = [] if net._blob is not None else [(t, t._version) for t in list(net.parameters()) + list(net.buffers())]
            self._vpos = 0
            self._ws = net._workspace(B, 1, dev)
            net._ws.pop((B, 1, str(dev)), None)          # private to this streamer from now on
        if use_graph:
            self.graphs = self._capture(self._body, dev)
            self.graph = self.graphs[0]
            self.reset()

    @staticmethod
    def _capture(body, dev) -> list:
        """The two alternating per-chunk graphs of `body(k)`, k = 0, 1 (after one eager pass of each on a side stream)."""
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for k in (0, 1):                    # warm-up: packs weights, allocates the T=1 workspace
                body(k)
        torch.cuda.current_stream(dev).wait_stream(side)
        graphs = []
        for k in (0, 1):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body(k)
            graphs.append(g)
        return graphs

    def _body(self, k: int):
        with self.net._device_ctx(self.chunk):
            self.net._stream_chunk(self.chunk, self.gain, self.sets[k], self.sets[k ^ 1], self.rings, self.pos, self.out,
                                   self._pk, self._ws, self.range_flag)
            # ring slot counter, kept in [0, window): an ever-growing int32 would go negative after 2^31 chunks and C's
            # `%` would then index before the ring.  One 1-thread kernel (two torch elementwise launches cost 9 us of the chunk)
            st = self.net._stream(self.device)
            self.net._lib(self.pos).call("lh_ring_advance", self.pos.data_ptr(), self.net.local_atten_len, st)

    def reset(self):
        for st in self.sets:
            for t in [st["conv_buf"], st["deconv_buf"], st["istft_buf"]] + st["h"] + st["c"]:
                t.zero_()
        for kx, vx in self.rings:
            kx.zero_()
            vx.zero_()
        self.pos.zero_()
        self.range_flag.zero_()
        self.parity = 0

    def set_embedding(self, embed: torch.Tensor):
        self.embed.copy_(embed.reshape(self.B, -1))
        with torch.no_grad():
            self.net._speaker_gain(self.embed, self.gain_raw, self.gain)

    def step(self, chunk: torch.Tensor) -> torch.Tensor:
        """chunk [B, 2, 192] (128 new + 64 look-ahead samples) -> [B, 2, 128]."""
        self._check_repacked()
        if self.net.range_check and int(self.range_flag[0]) != 0:     # host read of the pinned word: free
            self.range_flag.zero_()
            raise RuntimeError("LH_ERR_RANGE: an earlier chunk produced non-finite samples, emitted as zeros (inf / NaN in "
                               "the input or in the carried state); reset() the streamer")
        self._check_versions()
        self.chunk.copy_(chunk)
        with torch.no_grad():
            if self.graphs is not None:
                self.graphs[self.parity].replay()
            else:
                self._body(self.parity)
        self.parity ^= 1
        return self.out

    def _check_repacked(self):
        # O(1) staleness check (re-deriving the pack key walks all 130 parameters: ~0.1 ms of host time per 8 ms chunk):
        # any `Net` call after a parameter change re-packs and replaces `net._packed`.  The streamer owns references to
        # the images its graphs point into, so a stale streamer is never unsafe, only out of date.
        net = self.net
        cur = net._blob[1] if net._blob is not None else net._packed      # blob-only hosts (`from_packed`) never re-pack
        if cur is not self._pk:
            raise RuntimeError("the Net's parameters changed after this Streamer was built (its HIP graphs hold pointers "
                               "into the old packed weights): create a new streamer with net.make_streamer(...)")

    def _check_versions(self):
        # ... and a parameter updated IN PLACE (optimizer step, load_state_dict) without any other `Net` call in between
        # would replay silently on the old images: the tensors' version counters are re-checked three per chunk, round
        # robin (all ~130 within 0.4 s of audio).  Round 3 summed all of them every 64th chunk: ~0.13 ms of host time on
        # that chunk — exactly the p99 of the chunk latency (0.40 ms against a p50 of 0.26).
        self._n_steps += 1
        for _ in range(3 if self._versions else 0):
            t, v = self._versions[self._vpos]
            self._vpos = (self._vpos + 1) % len(self._versions)
            if t._version != v:
                raise RuntimeError("a parameter of the Net was modified in place after this Streamer was built: create a new "
                                   "streamer with net.make_streamer(...)")


class _Span(ctypes.Structure):
    """`lh_span_t` (include/lookonce_hip.h): one tensor of per-slot streaming state."""
    _fields_ = [("base", ctypes.c_void_p), ("bytes", ctypes.c_ulonglong)]


def _cuda_device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _copy_behind(data: torch.Tensor, event, dev: torch.device):
    """`data` copied into the memory of GPU `dev` behind `event`, without waiting: (the copy, an event behind it)."""
    if data.is_cuda:                                        # the copy is issued on the source's current stream
        cur = torch.cuda.current_stream(data.device)
        if event is not None:
            cur.wait_event(event)
        data.record_stream(cur)
    data = data.to(dev, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    return data, ev


class SessionSnapshot:
    """One listener's streaming state as a value: what `SessionStreamer.suspend` takes out and `resume` puts back, into any
    slot of any `SessionStreamer` of the same model — after a minute, on another GPU, in another process.
    `data`: ONE contiguous uint8 tensor in the layout of include/lookonce_hip.h ("suspend / resume"): header, the words, the
    speaker embedding, the tails and (h, c) of the live ping-pong set, the 50 window rows per head of every K / V ring.
    `event`: recorded behind the kernel that filled `data` (None for host memory, or where nothing is in flight); a resume on
    another stream orders itself behind it with a stream wait.  `layout`: the header's sizes on the host, so that `resume`
    can refuse a snapshot of another model without reading device memory.
    A snapshot is never written after it was filled: it can be resumed any number of times.  The state is only meaningful
    under the weights it was computed with; nothing checks that.  `to` never waits for the device; `cpu`, `save` and `load`
    may: they are not for the chunk loop."""
    MAGIC, VERSION, HEADER_BYTES = 0x5353484c, 1, 256       # LH_SNAPSHOT_*
    batch, index = None, 0                                  # a view of a `SessionSnapshotBatch`: the batch and the row

    def __init__(self, data: torch.Tensor, layout: tuple, event=None):
        self.data, self.layout, self.event = data, tuple(layout), event

    @staticmethod
    def layout_bytes(layout: tuple) -> int:
        """Size of a snapshot with these header sizes: (n_flat, n_rings, heads, window, embed_bytes, *flat, *ring rows)."""
        n_flat, n_rings, heads, window, embed_bytes = layout[:5]
        sizes = layout[5:]
        return SessionSnapshot.HEADER_BYTES + 16 + embed_bytes + sum(sizes[:n_flat]) + heads * window * sum(sizes[n_flat:])

    @property
    def device(self) -> torch.device:
        return self.data.device

    def to(self, device) -> "SessionSnapshot":
        """The snapshot in the memory of `device`: this object if it is there already, else a copy enqueued behind the event.
        From device memory or pinned host memory (what `cpu` and `load` return where a GPU is present) the copy is asynchronous;
        from pageable host memory it is staged and the host may wait for it."""
        dev = _cuda_device(device)
        if dev == self.data.device:
            return self
        if dev.type != "cuda":
            return self.cpu()
        data, ev = _copy_behind(self.data, self.event, dev)
        return SessionSnapshot(data, self.layout, ev)

    def cpu(self) -> "SessionSnapshot":
        """In host memory.  Waits for the kernel that fills the snapshot."""
        if not self.data.is_cuda:
            return self
        if self.event is not None:
            self.event.synchronize()
        return SessionSnapshot(self._pinned(self.data.cpu()), self.layout, None)

    @staticmethod
    def _pinned(host: torch.Tensor) -> torch.Tensor:
        """`host` in pinned memory where a GPU is present, so that a later `to(device)` does not stage the copy."""
        return host.pin_memory() if torch.cuda.is_available() else host

    def save(self, path: str):
        """The bytes of `data` as a file: the header makes it self-describing."""
        self.cpu().data.numpy().tofile(path)

    @classmethod
    def load(cls, path: str, device=None) -> "SessionSnapshot":
        """A snapshot from `save`'s file, in host memory or on `device`.  ValueError: not a snapshot, another layout version, or
        a size that does not match the header."""
        raw = np.fromfile(path, dtype=np.uint8)
        layout, total = cls._header(raw, path)
        if cls.layout_bytes(layout) != raw.size or total != raw.size:
            raise ValueError(f"{path}: {raw.size} bytes, the header's sizes make {cls.layout_bytes(layout)} (total word {total})")
        snap = cls(cls._pinned(torch.from_numpy(raw)), layout, None)
        return snap if device is None else snap.to(device)

    @classmethod
    def _header(cls, raw: np.ndarray, path: str):
        """(layout, total bytes) as the header at the start of `raw` states them.  ValueError: not a snapshot's header."""
        if raw.size < cls.HEADER_BYTES + 16:
            raise ValueError(f"{path}: {raw.size} bytes, not a session snapshot")
        head = raw[:cls.HEADER_BYTES].view("<u4").astype(np.int64)
        if head[0] != cls.MAGIC or head[1] != cls.VERSION:
            raise ValueError(f"{path}: magic {int(head[0]):#x} version {int(head[1])}, expected {cls.MAGIC:#x} version {cls.VERSION}")
        n_flat, n_rings = int(head[3]), int(head[4])
        if n_flat < 1 or n_rings < 1 or 8 + n_flat + n_rings > cls.HEADER_BYTES // 4:
            raise ValueError(f"{path}: header names {n_flat} state tensors and {n_rings} rings")
        return tuple(int(v) for v in head[3:8 + n_flat + n_rings]), int(head[2])


class SessionSnapshotBatch:
    """k listeners' snapshots as ONE value: what `SessionStreamer.suspend_many` / `drain` take out and `resume_many` puts back
    — a whole streamer moves in one launch and one copy.
    `data`: ONE uint8 tensor [k, stride]; row i holds snapshot i in its leading `nbytes` = `SessionSnapshot.layout_bytes(layout)`
    bytes (stride >= nbytes, a multiple of 16; what lies behind is padding nobody writes).  `layout` and `event` as for a
    `SessionSnapshot`: one layout, and ONE event behind the launch or copy that filled all of `data`.
    `batch[i]` is a `SessionSnapshot` whose `data` is a view of row i — same memory, same event — so `resume(slot, batch[i])`
    works, and `resume_many` recognises views of one batch and uses the batch in place.  `to` never waits for the device;
    `cpu`, `save` and `load` may."""

    def __init__(self, data: torch.Tensor, layout: tuple, event=None):
        self.data, self.layout, self.event = data, tuple(layout), event
        self.nbytes = SessionSnapshot.layout_bytes(self.layout)
        if data.dim() != 2 or data.dtype != torch.uint8 or data.stride(1) != 1 or data.shape[1] < self.nbytes or \
                data.shape[1] % 16 or (data.shape[0] > 1 and data.stride(0) != data.shape[1]):
            raise ValueError(f"a batch is a contiguous uint8 [k, stride >= {self.nbytes}, a multiple of 16], got "
                             f"{tuple(data.shape)} {data.dtype}")

    def __len__(self) -> int:
        return self.data.shape[0]

    def __getitem__(self, i: int) -> SessionSnapshot:
        i = range(len(self))[i]                             # negative indexes; IndexError ends an iteration
        snap = SessionSnapshot(self.data[i, :self.nbytes], self.layout, self.event)
        snap.batch, snap.index = self, i
        return snap

    @property
    def device(self) -> torch.device:
        return self.data.device

    def to(self, device) -> "SessionSnapshotBatch":
        """The batch in the memory of `device`: this object if it is there already, else ONE copy enqueued behind the event."""
        dev = _cuda_device(device)
        if dev == self.data.device:
            return self
        if dev.type != "cuda":
            return self.cpu()
        data, ev = _copy_behind(self.data, self.event, dev)
        return SessionSnapshotBatch(data, self.layout, ev)

    def cpu(self) -> "SessionSnapshotBatch":
        """In host memory.  Waits for the launch that fills the batch."""
        if not self.data.is_cuda:
            return self
        if self.event is not None:
            self.event.synchronize()
        return SessionSnapshotBatch(SessionSnapshot._pinned(self.data.cpu()), self.layout, None)

    @classmethod
    def stack(cls, snapshots, device=None) -> "SessionSnapshotBatch":
        """A batch of single snapshots of one layout, on `device` (default: where the first one lies).  One copy per snapshot,
        each ordered behind that snapshot's event on the device's current stream; the host does not wait for device memory."""
        snaps = list(snapshots)
        if not snaps:
            raise ValueError("no snapshots to stack")
        layout = snaps[0].layout
        for sn in snaps:
            if sn.layout != layout or sn.data.numel() != SessionSnapshot.layout_bytes(layout):
                raise ValueError(f"snapshots of different layouts: {sn.layout} ({sn.data.numel()} bytes) and {layout}")
        dev = _cuda_device(snaps[0].data.device if device is None else device)
        if dev.type != "cuda":
            return cls(SessionSnapshot._pinned(torch.stack([sn.cpu().data for sn in snaps])), layout, None)
        data = torch.empty(len(snaps), SessionSnapshot.layout_bytes(layout), dtype=torch.uint8, device=dev)
        cur = torch.cuda.current_stream(dev)
        for i, sn in enumerate(snaps):
            sn = sn.to(dev)
            if sn.event is not None:
                cur.wait_event(sn.event)
            sn.data.record_stream(cur)
            data[i].copy_(sn.data, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(cur)
        return cls(data, layout, ev)

    def save(self, path: str):
        """The k snapshots back to back, unpadded, each in `SessionSnapshot.save`'s format: a header's total word says where the
        next one starts."""
        self.cpu().data[:, :self.nbytes].contiguous().numpy().tofile(path)

    @classmethod
    def load(cls, path: str, device=None) -> "SessionSnapshotBatch":
        """A batch from `save`'s file, in host memory or on `device`.  ValueError: not snapshots back to back, sizes that do not
        add up, or snapshots of more than one layout."""
        raw = np.fromfile(path, dtype=np.uint8)
        layout, total = SessionSnapshot._header(raw, path)
        n = SessionSnapshot.layout_bytes(layout)
        if total != n or raw.size % n:
            raise ValueError(f"{path}: {raw.size} bytes, the first header's sizes make {n} (total word {total})")
        rows = raw.reshape(-1, n)
        for i in range(1, rows.shape[0]):
            if SessionSnapshot._header(rows[i], path) != (layout, total):
                raise ValueError(f"{path}: snapshot {i} has another layout than snapshot 0")
        batch = cls(SessionSnapshot._pinned(torch.from_numpy(rows)), layout, None)
        return batch if device is None else batch.to(device)


class SessionStreamer:
    """A batched `Streamer` whose rows are listener SLOTS that open, close and fail one at a time.

    The chunk loop stays what `Streamer` runs — same buffers, same launches, all slots advance together, one chunk per
    `step` — between two more graph nodes (include/lookonce_hip.h, "streaming sessions"): `lh_session_begin` zeroes the
    state of a slot that was just opened or closed and hands only live slots' samples to the separator; `lh_session_end`
    silences idle slots and closes a slot whose chunk was, or came out, non-finite.  A fault therefore costs ONE listener
    their session: `step` never raises for it, the other rows keep their bits, and the slot can be opened again at once.
      * `open(slot, embed)`: from the next `step` on the slot is a fresh stream (zero tails, (h, c) and K / V history — the
        zero history is the same in every rotation of the ring, so the shared ring position needs no per-slot copy) with
        its own speaker gain;  `close(slot)`: from the next `step` on its output rows are exact zeros;
      * `set_embedding(slot, embed)` re-targets an open slot, its carried state is kept;
      * `faults()`: slots the device closed since they were opened;  `active`: the open slots that have not faulted.
    Nothing here waits for the device: commands travel as one asynchronous copy of a pinned array ahead of the replay
    (only when something is pending), the fault words are pinned host memory the last kernel stores to.
    Enrollment (`enroll_chunks` = n >= 2; 0, the default, builds exactly the object above): "look once" from the listener's
    own stream.  `enroll(slot, embedder)` arms an idle slot: one more graph node (`lh_session_capture`, after
    `lh_session_begin`) records the slot's next n chunks — the 128 n contiguous samples from the next `step` on — into a
    device buffer and posts a word in pinned host memory when the clip is complete.  `poll()` (the first thing `step` does;
    public, cheap, idempotent) reads those words: the clips completed since the last poll go through ONE `embedder` call, a
    batch in ascending slot order, on the streamer's one side stream behind an event of the loop's stream; a call whose
    second event reports complete hands its rows to the `open` path, and the slot is in `active` and a fresh stream from that
    `step` on.  `enrolling`: the slots capturing or embedding;  `embedding_of(slot)`: the [256] device tensor enrollment
    opened the slot with (keep it to `open` the listener again later).  Meanwhile the slot is idle to the separator: its
    output rows are exact zeros — or their own input, with `passthrough=True` in a monitor streamer (below).  An inf / NaN among
    the recorded samples aborts the capture: the slot is listed by `faults()` and is idle again, to be enrolled or opened at
    once.  `close(slot)` cancels a capture or a running embedding (a result that arrives later is dropped by its
    generation), `reset()` cancels all of them.  Call the embedder once on a clip of this length before the loop starts:
    its first call packs weights.
    Compaction (`compact=True`; False, the default, builds exactly the object above): a chunk costs what its listeners cost.
    Slots keep their numbers towards the caller — every method above, the rows of `step`'s input and output, the fault
    words — while the open listeners live in the leading ROWS of the same state buffers, and `step` runs the chunk's kernels
    for `last_rows` = the smallest of `row_buckets` that holds the `rows_in_use` rows (one alternating graph pair per
    bucket, over the leading rows of the same buffers and workspace).  An opening takes the first free row.  When a
    listener leaves — `close`, or a fault word `step` sees — the survivors in the rows at and above the new row count move
    into the holes below it, highest row first: every move has src >= the new count > dst, so the moves of one step are
    disjoint and run in one launch (`lh_session_move`, the chunk's first node: the row's slice of every state tensor, its
    speaker gain, its `active` and pending device command word — bytes, the listener keeps their bits).  An opening of the
    same step takes the uppermost of the holes, which saves that move.  `lh_session_begin_rows` / `lh_session_end_rows` gather
    the row's input from, and scatter its output to, the slot; rows without a listener are idle on the device whatever they
    still hold, and a slot without a row is written zeros in every chunk.  Moves, the row <-> slot maps and the commands travel
    in the one asynchronous copy, only when something is pending.  A slot that is capturing or embedding owns no row.
    Pacing (`pace=True`; False, the default, builds exactly the object above, launch for launch): listeners do not arrive in
    lock-step.  `step(chunks, present)` HOLDS every slot whose `present[s]` is false: its input row is ignored (it may be NaN
    and is never judged for a fault), its output row is exact zeros, and every bit of its carried state — tails, (h, c), K / V
    rings and ring position — is after the step what it was before.  A listener's output stream is the concatenation of the
    output rows of the steps they were present for.  Every ROW owns its ring position: the chunk that serves an OPEN sets it
    to 0 and only a chunk the row consumed advances it (`lh_qkv_proj_ln_rows`, `lh_ring_advance_rows`), so in a paced streamer
    a listener's bits depend on their own chunks only — not on when they were opened, not on who else was held.  Commands are
    served whether or not the slot is held: a slot opened and held in the same step is reset and active, and its first chunk
    is the first one it is present for; a capturing slot that is held records nothing, its clip is the samples of the chunks
    it was present for.  With `compact=True` the position word moves with the row, and the hold words stay addressed by slot.
    The hold words travel like the commands, a fresh pinned array copied asynchronously, and only in a step whose mask differs
    from the one on the device: a steady all-present loop copies nothing.  A held row costs what a live row costs — its
    kernels run on a zero-gated input and `lh_session_end_paced` puts the row's state back, about 0.2 MB of copies — so
    pacing buys correctness under jitter, not time; a compacting streamer does not skip held rows.
    Suspend / resume (every flavour above, as source and as target, in any combination): `suspend(slot)` takes an open
    listener's state, as of the last `step`, out as a `SessionSnapshot` — one launch (`lh_session_save`) into a fresh device
    tensor: the tails and (h, c) of the ping-pong set the next chunk would read, the 50 window rows per head of every ring, the
    ring position (the row's own, or the shared counter), the speaker embedding and the row's two device words — and closes the
    slot.  `resume(slot, snapshot)` makes an idle slot that listener again from the next `step` on: `step` enqueues
    `lh_session_restore` behind its copy of the command words and ahead of the chunk (eager launches between two replays,
    like `set_embedding`'s; the graphs are what they were), and the slot opens WITHOUT a reset.  Into a paced streamer the ring
    rows and the position go back as they were, and the listener's output continues bit for bit; into a lock-step streamer the
    ring rows are rotated so that the listener's oldest row is the next one the shared counter overwrites — bit for bit when
    the shared position equals the saved one, within the tolerance of a listener opened at an arbitrary position otherwise.
    A compacting streamer plans a resume as an opening: it takes a hole, which no move of that step reads or writes; a slot
    closed or suspended and resumed between two steps gives its previous listener's row up first, like any listener that left.  A
    listener the device had closed in the chunk before `suspend` (the fault word not yet seen) makes a dead snapshot: resuming
    it leaves the slot idle on the device and lists it in `faults()` after that `step`.  Neither call waits for the device.
    Many at once: `suspend_many(slots)` / `drain()` / `resume_many(slots, snapshots)` are those calls in order for any number of
    listeners with a number of launches that does not depend on it — one `lh_session_save_rows` into one `SessionSnapshotBatch`
    tensor; in `step` one `lh_session_restore_rows` and one `lh_embed_proj_ln_rows` per batch, behind one copy of an item table.
    `suspend`, `resume` and a streamer that never calls the batched methods enqueue what they always did.
    Packets (`pace=True, packets=True`; False, the default, builds exactly the object above, launch for launch): clients do not
    send windows, they send contiguous PCM in packets of 10 or 20 ms that arrive with jitter.  `push({slot: samples [2, n]})`
    takes one tick's packets at any size — one fresh pinned buffer (an item table, then the samples), one asynchronous copy,
    one launch (`lh_session_feed`) that scatters them into a device FIFO of `fifo_samples` per slot — and `step()` takes no
    input: the chunk's first node (`lh_session_frame`) cuts a 192-sample window for every slot that holds one, writes the hold
    words of the others itself, and everything behind `chunk_in` and `hold` is the paced streamer.  The FIFO's two sample
    counters per slot wrap modulo 2^32 and are mirrored on the host in the same arithmetic: the host knows what every launch
    will find (`buffered(slot)`, `ready()`, `last_present` — a tuple of S bools, the slots the last `step` consumed a chunk
    of), the device follows, nothing is read back and no hold word travels.  A listener's output is the concatenation of
    their rows over the steps with `last_present[slot]`, whatever the packet sizes were; a slot with two chunks buffered is
    stepped twice (`while ss.ready(): ss.step()` catches up), a slot without one is held.  `push` raises `BufferError`, before
    anything is enqueued for any slot, when a slot would hold more than `fifo_samples`: the device FIFO cannot overflow.
    `flush(slot)` drops a slot's buffered input (with its next packet, or in a push of its own that `step` issues); `reset()`
    flushes everyone.  The FIFO is transport, not listener state: `open`, `close`, `enroll`, `suspend` and `resume` do not touch
    it and it is in no snapshot — a host that gives a slot to another client flushes it.  An idle slot is framed like any
    other, as lock-step gates an idle slot's row.  The last chunk of a stream needs its 64 look-ahead samples: push 64 zeros
    for the tail.  `pcm16=True`: packets are int16 (scaled by 2^-15 on the device, exact) and `step` returns int16 rows
    (`lh_session_emit_s16`, round half even, saturating) — the bits of the fp32 path fed `pcm.float() / 32768`.
    Client rate (`packets=True, client_rate=48000`; 16000, the default, builds exactly the object above, launch for launch):
    headsets and WebRTC stacks capture and play at 48 kHz, some at 32, 24 or 8.  `push` takes `[2, n]` at the client's rate and
    `step()` returns `[S, 2, hop_client]`, `hop_client = 128 * client_rate / 16000` samples at that rate (fp32, or int16 with
    `pcm16`) — resampled on the device with the arithmetic of `resample.Resampler` (torchaudio's `sinc_interp_hann`, one fp32
    inner product that every kernel shares): the packets land through `lh_session_feed` in a second per-slot ring at the client
    rate, `lh_session_resample_in` (one more launch of the same `push`, its items in the same copy) turns whole blocks of it into
    16 kHz samples of the FIFO, and `lh_session_resample_out`, the chunk's last node, turns the 16 kHz rows into client rows.
    What a listener hears equals `Resampler(client_rate, 16000)` of their whole stream, served by a 16 kHz packet streamer, then
    `Resampler(16000, client_rate)` of `delay_out` zeros followed by the rows — bit for bit, whatever the packet sizes.  Rates
    are multiples of 125 Hz (a chunk is then a whole number of client samples): 8000, 24000, 32000, 40000, 48000, 96000 ...;
    44100 is refused — resample such a stream with `Resampler` first.  `fifo_samples`, `buffered`, `ready`, `last_present` and
    `BufferError` keep their meaning in 16 kHz samples: the host mirrors the resampler's block arithmetic in integers.
    Added latency: a 16 kHz block is made when its `lookahead_in = width + o - 1` later client samples have been pushed (48 kHz:
    21 samples, 0.44 ms), and the output is `delay_out` 16 kHz samples late (toward 48 kHz: 8 samples, 0.5 ms); the tail of a
    stream needs `lookahead_in` zeros pushed behind it (and the 64 look-ahead samples of the last chunk, at the client's rate).
    The raw ring and the output tail are transport like the FIFO: in no snapshot, untouched by `open`, `close`, `suspend` and
    `resume`; `flush(slot)` and `reset()` clear them, so a flushed slot's stream starts from silence, as torchaudio's left pad
    does.  Enrollment keeps recording the 16 kHz `chunk_in`.
    Monitor (`monitor=True`; False, the default, builds exactly the object above, launch for launch): what a listener hears is
    `wet` x their separated rows + `dry` x their own input.  `set_mix(slot, wet, dry)` (finite, in [0, 1]; any slot, idle ones
    included) holds from the next `step`, `mix_of(slot)` returns the targets.  One more graph node after the end node and ahead of
    the resample / 16-bit node (`lh_session_mix`, by slot in every flavour) ramps the slot's two gains towards the targets on the
    device — linear, `monitor_ramp` 16 kHz samples per full swing, exactly on target at the end, re-targetable in mid-ramp — and
    mixes in place: output row j covers samples [128 j, 128 j + 128) of the slot's stream, the first 128 samples of input row j, so
    the dry path needs no delay line and is aligned to the sample behind any framing and resampling.  A slot settled at the
    defaults (1, 0) keeps the bits of a streamer without the node; a held slot's row stays zeros and its ramp waits; a non-finite
    sample among the row's own 128 silences that row without a fault.  The targets travel like the hold words (a fresh pinned
    array, one asynchronous copy, only in a step where one changed).  The mix is transport, like the FIFO: in no snapshot,
    untouched by `open`, `close`, `suspend`, `resume` and row moves; `reset()` puts it back to (1, 0).  `enroll(slot, embedder,
    passthrough=True)` posts (0, 1) with the arming and (1, 0) in the step that opens the slot: the room, then a click-free
    cross-fade into the target from the slot's first live chunk.  A slot the device closed for a fault is idle and sounds as an
    idle slot with its dry gain sounds: fail-open.
    Re-look (`relook(slot, embedder)`; needs `enroll_chunks`, not `monitor`): the capture runs on an OPEN slot while the separator
    goes on with the current embedding — the slot is in `active` and in `enrolling`, keeps its row in a compacting streamer, and
    its output is bit for bit what it would be without the capture — and the finished embedding takes the `set_embedding` path:
    state kept, `embedding_of(slot)` updated.  `close` cancels the look and closes the session, `suspend` is refused meanwhile.
        ss = net.make_session_streamer(64, "cuda:0", pace=True, packets=True)
        ss.open(0, emb_a); ss.open(1, emb_b)
        while serving:                                       # one tick: whatever arrived, then the chunks that are ready
            ss.push({0: a.recv(160), 1: b.recv(320)})        # a 10 ms and a 20 ms client, [2, n] float32 each
            while ss.ready():
                y = ss.step()
                for slot, took in enumerate(ss.last_present):
                    if took:
                        send(slot, y[slot])                  # [2, 128], the next 8 ms of that listener
    A snapshot is only meaningful under the weights it was taken with: that is the caller's to keep."""
    RESET, OPEN, CLOSE, GEN_SHIFT, MAX_SPANS, GEN_MASK = 1, 2, 4, 8, 32, 0x7fffff      # LH_SESSION_*
    ARM, CANCEL, ENROLL_FAULT = 1, 2, 0x80000000                                       # LH_ENROLL_*
    FEED_F32, FEED_S16, FEED_FLUSH, FEED_ITEM_WORDS = 0, 1, 1, 5                       # LH_FEED_*, lh_feed_item_t
    HOP, WINDOW, COUNTER_MASK = 128, 192, 0xffffffff                                   # samples a chunk consumes / needs
    RATE, RESAMPLE_ITEM_WORDS = 16000, 4                                               # the model's rate; lh_resample_item_t

    def __init__(self, net: Net, n_slots: int, device, use_graph: bool = True, enroll_chunks: int = 0, compact: bool = False,
                 row_buckets=None, pace: bool = False, packets: bool = False, fifo_samples: int = 2048, pcm16: bool = False,
                 client_rate: int = 16000, monitor: bool = False, monitor_ramp: int = 256):
        if n_slots < 1:
            raise ValueError("n_slots must be positive")
        if client_rate != self.RATE:
            if not packets:
                raise ValueError("client_rate is the sample rate of a packet streamer's clients: packets=True")
            if int(client_rate) != client_rate or client_rate % 125 or not 1000 <= client_rate <= 384000:
                raise ValueError(f"client_rate must be a multiple of 125 Hz in [1000, 384000] — a 128-sample chunk at 16 kHz is "
                                 f"then a whole number of client samples (8000, 24000, 32000, 48000 ...); {client_rate} is not "
                                 "(44100 is not either): resample such a stream with resample.Resampler first")
        if packets and not pace:
            raise ValueError("packets are the input of a paced streamer (the device decides who is present): pace=True")
        if pcm16 and not packets:
            raise ValueError("pcm16 is the sample format of a packet streamer: packets=True")
        if packets and (fifo_samples < 256 or fifo_samples & (fifo_samples - 1) or fifo_samples > 1 << 24):
            raise ValueError(f"fifo_samples must be a power of two in [256, 2^24] (a 192-sample window while 128 more "
                             f"arrive; the ring index is a mask), got {fifo_samples}")
        if row_buckets is not None and not compact:
            raise ValueError("row_buckets are the launch sizes of a compacting streamer: compact=True")
        if compact:
            if row_buckets is None:
                row_buckets = [1 << i for i in range(n_slots.bit_length()) if 1 << i < n_slots] + [n_slots]
            row_buckets = tuple(int(b) for b in row_buckets)
            if not row_buckets or row_buckets[0] < 1 or row_buckets[-1] != n_slots or \
                    any(a >= b for a, b in zip(row_buckets, row_buckets[1:])):
                raise ValueError(f"row_buckets must ascend from >= 1 to n_slots = {n_slots}, got {row_buckets}")
        if isinstance(monitor_ramp, bool) or not isinstance(monitor_ramp, int) or monitor_ramp < 1:
            raise ValueError(f"monitor_ramp is the number of 16 kHz samples of a full 0 -> 1 swing, an int >= 1, got "
                             f"{monitor_ramp!r}")
        if enroll_chunks < 0 or enroll_chunks == 1:
            raise ValueError("enroll_chunks must be 0 (no enrollment) or >= 2: the embedder needs 4 STFT frames at stride 64, "
                             "192 samples, and a chunk records 128")
        # buffers, packed weights, workspace and staleness checks are a Streamer's; its graphs are not captured
        self._st = st = Streamer(net, n_slots, device, use_graph=False)
        self.net, self.S, self.device = net, n_slots, st.device
        S, dev = n_slots, st.device
        self.chunk_in = torch.zeros_like(st.chunk)          # as the clients sent it; `st.chunk` is the gated copy
        self.out = st.out
        self.compact, self.row_buckets = bool(compact), row_buckets
        if compact:
            # rows of words: move table | row -> slot | slot -> row | cmd from the host || cmd from the device | active.
            # The first four are the host's (one copy), the last three the [2][S] cmd and the [S] active of the kernels
            self.out = torch.zeros_like(st.out)             # by SLOT; `st.out` is by row
            self._tables = torch.zeros(6, S, dtype=torch.int32, device=dev)
            self._tables[1:3].fill_(-1)
            self._words = self._tables[3:]
            self._row_of, self._slot_of = [-1] * S, [-1] * S                 # as of the last `step`
            self._n_rows = 0
            self._last_rows = row_buckets[0]
            # slot and generation of the listener in each row: one vector compare per `step` finds a fault word
            self._slot_np, self._rgen_np = np.zeros(S, dtype=np.int64), np.full(S, -1, dtype=np.int64)
        else:
            self._words = torch.zeros(3, S, dtype=torch.int32, device=dev)   # cmd from the host | cmd from the device | active
        self._fault = net._host_words(S, dev)
        self._fault_np = self._fault.numpy()                # the same memory, read without a tensor op per slot
        span = lambda t: _Span(t.data_ptr(), t.numel() * t.element_size() // S)
        state = [t for x in st.sets for t in [x["conv_buf"], x["deconv_buf"], x["istft_buf"]] + x["h"] + x["c"]]
        state += [t for kv in st.rings for t in kv]
        if len(state) + compact > self.MAX_SPANS:
            raise ValueError(f"{len(state) + compact} state tensors, lh_session_begin / lh_session_move take {self.MAX_SPANS}")
        self._spans = (_Span * len(state))(*[span(t) for t in state])
        if compact:                                         # what a row owns: its state and its speaker gain
            self._spans_move = (_Span * (len(state) + 1))(*[span(t) for t in state + [st.gain]])
        # what chunk k WRITES: the (h, c) of the other ping-pong set
        self._spans_end = [(_Span * (2 * net.n_blocks))(*[span(t) for t in st.sets[k ^ 1]["h"] + st.sets[k ^ 1]["c"]])
                           for k in (0, 1)]
        # suspend / resume: the tails and (h, c) of each ping-pong set, the rings with their geometry, the snapshot's sizes
        tails = lambda x: [x["conv_buf"], x["deconv_buf"], x["istft_buf"]] + x["h"] + x["c"]
        rings = [t for kv in st.rings for t in kv]
        self._spans_live = [(_Span * len(tails(x)))(*[span(t) for t in tails(x)]) for x in st.sets]
        self._spans_rings = (_Span * len(rings))(*[_Span(t.data_ptr(), t.shape[-1] * t.element_size()) for t in rings])
        self._ring_geom = (net.n_head, rings[0].shape[1], net.local_atten_len)      # heads per slot, rows per head, window
        self._snap_layout = (len(self._spans_live[0]), len(rings), net.n_head, net.local_atten_len,
                             st.embed.shape[1] * st.embed.element_size(), *[sp.bytes for sp in self._spans_live[0]],
                             *[sp.bytes for sp in self._spans_rings])
        self._snap_bytes = SessionSnapshot.layout_bytes(self._snap_layout)
        self._resumes = {}                                  # slot -> [snapshot, embedding set since `resume` or None]
        self._resume_batches = []                           # `resume_many`: (batch, {slot: (index, the slot's entry above)})
        self.pace = bool(pace)
        if pace:
            self._ring = torch.zeros(2, S, dtype=torch.int32, device=dev)    # per row: ring position | the chunk's write slot
            self._hold = torch.zeros(S, dtype=torch.int32, device=dev)       # per slot, as of the last copy: `_held`
            self._none_held = self._held = (False,) * S
            # what a held row gets back: (read, written) of every tail and (h, c), for chunk k
            carry = lambda x: [x["conv_buf"], x["deconv_buf"], x["istft_buf"]] + x["h"] + x["c"]
            pairs = [[t for rw in zip(carry(st.sets[k]), carry(st.sets[k ^ 1])) for t in rw] for k in (0, 1)]
            if len(pairs[0]) > self.MAX_SPANS:
                raise ValueError(f"{len(pairs[0]) // 2} state pairs, lh_session_end_paced takes {self.MAX_SPANS // 2}")
            self._spans_carry = [(_Span * len(p))(*[span(t) for t in p]) for p in pairs]
        self.packets, self.pcm16, self.fifo_samples = bool(packets), bool(pcm16), int(fifo_samples)
        if packets:
            R = self.fifo_samples
            self._fifo = torch.zeros(S, net.num_ch, R, device=dev)           # a ring per slot and channel
            self._fifo_words = torch.zeros(2, S, dtype=torch.int32, device=dev)      # wr | rd: sample counters mod 2^32
            self._wr, self._rd = [0] * S, [0] * S                             # the host's mirror of both: the device follows
            self._flush = set()                                              # slots whose next item carries FLUSH
            # one tick's item table and samples: at most a full ring per slot (`push` refuses more)
            self._item_words = (self.FEED_ITEM_WORDS * S + 3) // 4 * 4
            self._stage = torch.zeros(self._item_words + S * net.num_ch * R // (2 if pcm16 else 1), dtype=torch.int32, device=dev)
            self.last_present = (False,) * S
            if pcm16 and client_rate == self.RATE:
                self.out16 = torch.zeros(S, net.n_srcs, net.stft_chunk_size, dtype=torch.int16, device=dev)
        self.client_rate, self.hop_client, self._resampling = int(client_rate), self.HOP, client_rate != self.RATE
        if self._resampling:
            from .resample import resample_bank
            bank_in, self._w_in, self._o_in, self._n_in = resample_bank(self.client_rate, self.RATE)
            bank_out, self._w_out, self._o_out, self._n_out = resample_bank(self.RATE, self.client_rate)
            self._k_in = 2 * self._w_in + self._o_in
            self.hop_client = self.HOP * self._o_in // self._n_in
            self.lookahead_in = self._w_in + self._o_in - 1                  # client samples behind a block's first one
            self.delay_out = (self._w_out + 2 * self._o_out - 1) // self._o_out * self._o_out       # 16 kHz samples, D o
            # a full FIFO's worth of input plus one block's taps: what `push` can leave unconsumed
            self.raw_samples = 256
            while self.raw_samples < self.fifo_samples * self._o_in // self._n_in + self._k_in:
                self.raw_samples *= 2
            Rin = self.raw_samples
            self._raw = torch.zeros(S, net.num_ch, Rin, device=dev)          # a ring per slot and channel, at the client rate
            self._raw_words = torch.zeros(2, S, dtype=torch.int32, device=dev)       # its wr | rd (rd: only FLUSH writes it)
            self._tap0 = -self._w_in & self.COUNTER_MASK                     # a stream's first tap: the left pad lies below 0
            self._raw_wr, self._tap = [0] * S, [self._tap0] * S              # mirrors: raw samples pushed | next block's first tap
            self._tail = torch.zeros(S, net.n_srcs, self._w_out + self.delay_out, device=dev)
            self.out_client = torch.zeros(S, net.n_srcs, self.hop_client, dtype=torch.int16 if pcm16 else torch.float32,
                                          device=dev)
            self._bank_in, self._bank_out = bank_in.to(dev), bank_out.to(dev)
            self._ritem_off = self.FEED_ITEM_WORDS * S                       # the resample items follow the feed items
            self._item_words = ((self.FEED_ITEM_WORDS + self.RESAMPLE_ITEM_WORDS) * S + 3) // 4 * 4
            self._stage = torch.zeros(self._item_words + S * net.num_ch * Rin // (2 if pcm16 else 1), dtype=torch.int32, device=dev)
        self._gen = [0] * S                                 # generation of the slot's current opening, 0 = idle
        self._next_gen = 1
        self._pending = {}                                  # slot -> command word for the next step
        self.enroll_chunks = n = enroll_chunks
        self._capturing = {}                                # slot -> (generation, embedder) of a capture in progress
        self._embedding = {}                                # slot -> generation of a clip the embedder is running on
        self._jobs = []                                     # embedder calls in flight, oldest first: (event, slots, gens, out)
        self._enroll_faults = set()                         # idle slots whose last capture the device aborted
        self._enrolled = {}                                 # slot -> the embedding enrollment opened it with
        self._epending = {}                                 # slot -> LH_ENROLL_* word for the next step
        self._relook = set()                                # capturing / embedding slots whose session stays open: `relook`
        self.monitor, self.monitor_ramp = bool(monitor), monitor_ramp
        self._passthrough = set()                           # enrolling slots whose mix goes back to (1, 0) with their OPEN
        if monitor:
            self._mix = torch.zeros(2, 2, S, device=dev)    # targets [2][S] | gains [2][S]: wet, then dry
            self._mix[:, 0].fill_(1.0)
            self._mix_step = float(np.float32(1.0) / np.float32(monitor_ramp))
            self._targets = [(1.0, 0.0)] * S                # the host's copy of the targets, as fp32 values
            self._mix_posted = True                         # false: a target changed since the last copy
        if n:
            self._clips = torch.zeros(S, net.num_ch, net.stft_chunk_size * n, device=dev)
            self._ewords = torch.zeros(3, S, dtype=torch.int32, device=dev)      # ecmd | estate: generation, chunks recorded
            self._edone = net._host_words(S, dev)
            self._edone_np = self._edone.numpy()
            self._side = net._enroll_side(dev)
        self.graphs = None
        if use_graph:
            with torch.no_grad():
                if compact:                                 # one alternating pair per launch size
                    self.graphs = {n: Streamer._capture(lambda k, n=n: self._body(k, n), dev) for n in row_buckets}
                else:
                    self.graphs = Streamer._capture(self._body, dev)
            self.reset()

    def _body(self, k: int, n_rows: int = 0):
        if self.pace:
            return self._body_paced(k, n_rows)
        if self.compact:
            return self._body_rows(k, n_rows)
        st, net, S = self._st, self.net, self.S
        P = lambda t: t.data_ptr()
        with net._device_ctx(st.chunk):
            lib, stream = net._lib(st.chunk), net._stream(self.device)
            cmd, active = self._words.data_ptr(), self._words[2].data_ptr()
            lib.call("lh_session_begin", ctypes.addressof(self._spans), len(self._spans), P(self.chunk_in), P(st.chunk), cmd,
                     active, S, stream)
            if self.enroll_chunks:
                lib.call("lh_session_capture", P(self.chunk_in), P(self._clips), P(self._ewords), P(self._ewords[1]),
                         P(self._edone), self.enroll_chunks, S, stream)
            net._stream_chunk(st.chunk, st.gain, st.sets[k], st.sets[k ^ 1], st.rings, st.pos, st.out, st._pk, st._ws, None,
                              keep_nonfinite=1)
            lib.call("lh_ring_advance", P(st.pos), net.local_atten_len, stream)
            lib.call("lh_session_end", ctypes.addressof(self._spans_end[k]), len(self._spans_end[k]), P(self.chunk_in),
                     P(st.out), cmd, active, P(self._fault), S, stream)
            if self.monitor:
                self._mix_node(lib, None, stream)

    def _mix_node(self, lib, hold, stream):
        """The wet / dry mix of a monitor streamer, by slot, on the rows the end node left (`hold`: a paced streamer's)."""
        P = lambda t: t.data_ptr()
        lib.call("lh_session_mix", P(self.chunk_in), P(self.out), P(self._mix[0]), P(self._mix[1]), hold, self._mix_step,
                 self.S, stream)

    def _body_rows(self, k: int, n: int):
        """The chunk of a compacting streamer for its leading `n` rows: move -> begin -> (capture) -> chunk -> ring advance ->
        end.  Every per-row tensor is row-major in the batch index, so the leading rows of the same buffers are a batch of n."""
        st, net, S = self._st, self.net, self.S
        P = lambda t: t.data_ptr()
        with net._device_ctx(st.chunk):
            lib, stream = net._lib(st.chunk), net._stream(self.device)
            t = self._tables
            frm, slot_of, row_of, cmd, active = P(t[0]), P(t[1]), P(t[2]), P(t[3]), P(t[5])
            lib.call("lh_session_move", ctypes.addressof(self._spans_move), len(self._spans_move), frm, cmd, active, n, S, stream)
            lib.call("lh_session_begin_rows", ctypes.addressof(self._spans), len(self._spans), P(self.chunk_in), P(st.chunk), cmd,
                     active, slot_of, n, S, stream)
            if self.enroll_chunks:                          # by slot: a capturing slot owns no row
                lib.call("lh_session_capture", P(self.chunk_in), P(self._clips), P(self._ewords), P(self._ewords[1]),
                         P(self._edone), self.enroll_chunks, S, stream)
            net._stream_chunk(st.chunk[:n], st.gain, st.sets[k], st.sets[k ^ 1], st.rings, st.pos, st.out, st._pk, st._ws, None,
                              keep_nonfinite=1)
            lib.call("lh_ring_advance", P(st.pos), net.local_atten_len, stream)
            lib.call("lh_session_end_rows", ctypes.addressof(self._spans_end[k]), len(self._spans_end[k]), P(self.chunk_in),
                     P(st.out), P(self.out), cmd, active, P(self._fault), slot_of, row_of, frm, n, S, stream)
            if self.monitor:
                self._mix_node(lib, None, stream)

    def _body_paced(self, k: int, n: int):
        """The chunk of a paced streamer, lock-step rows (n = 0: every slot is a row) or the leading `n` rows of a compacting
        one: (move ->) begin -> (capture) -> chunk with per-row ring slots -> per-row ring advance -> end."""
        st, net, S = self._st, self.net, self.S
        P, A = (lambda t: t.data_ptr()), ctypes.addressof
        with net._device_ctx(st.chunk):
            lib, stream = net._lib(st.chunk), net._stream(self.device)
            hold, pos, wpos = P(self._hold), P(self._ring[0]), P(self._ring[1])
            end, carry = self._spans_end[k], self._spans_carry[k]
            if self.packets:                                # the windows and the hold words of this chunk, made on the device
                lib.call("lh_session_frame", P(self._fifo), P(self._fifo_words[0]), P(self._fifo_words[1]), P(self.chunk_in),
                         hold, self.fifo_samples, S, stream)
            if self.compact:
                t = self._tables
                frm, slot_of, row_of, cmd, active = P(t[0]), P(t[1]), P(t[2]), P(t[3]), P(t[5])
                lib.call("lh_session_move_paced", A(self._spans_move), len(self._spans_move), frm, cmd, active, pos, n, S, stream)
                lib.call("lh_session_begin_rows_paced", A(self._spans), len(self._spans), P(self.chunk_in), P(st.chunk), cmd,
                         active, slot_of, hold, pos, wpos, n, S, stream)
            else:
                n, cmd, active = S, P(self._words), P(self._words[2])
                lib.call("lh_session_begin_paced", A(self._spans), len(self._spans), P(self.chunk_in), P(st.chunk), cmd, active,
                         hold, pos, wpos, S, stream)
            if self.enroll_chunks:                          # by slot, like the hold words
                lib.call("lh_session_capture_paced", P(self.chunk_in), P(self._clips), P(self._ewords), P(self._ewords[1]),
                         P(self._edone), hold, self.enroll_chunks, S, stream)
            net._stream_chunk(st.chunk[:n], st.gain, st.sets[k], st.sets[k ^ 1], st.rings, st.pos, st.out, st._pk, st._ws, None,
                              keep_nonfinite=1, write_pos=self._ring[1])
            lib.call("lh_ring_advance_rows", pos, wpos, net.local_atten_len, n, stream)
            if self.compact:
                lib.call("lh_session_end_rows_paced", A(end), len(end), A(carry), len(carry) // 2, P(self.chunk_in), P(st.out),
                         P(self.out), cmd, active, P(self._fault), hold, slot_of, row_of, frm, n, S, stream)
            else:
                lib.call("lh_session_end_paced", A(end), len(end), A(carry), len(carry) // 2, P(self.chunk_in), P(st.out), cmd,
                         active, P(self._fault), hold, S, stream)
            if self.monitor:
                self._mix_node(lib, hold, stream)
            if self._resampling:                            # the rows at the client's rate, fp32 or 16-bit
                lib.call("lh_session_resample_out", P(self.out), P(self._tail), hold, P(self.out_client),
                         self.FEED_S16 if self.pcm16 else self.FEED_F32, S, P(self._bank_out), self._o_out, self._n_out,
                         self._w_out, stream)
            elif self.pcm16:
                lib.call("lh_session_emit_s16", P(self.out), P(self.out16), S, stream)

    def reset(self):
        """Every slot idle, all state zero (what a new SessionStreamer starts from).  Captures and embeddings are cancelled."""
        self._st.reset()
        if self.pace:
            self._ring.zero_()
            self._hold.zero_()
            self._held = self._none_held
        if self.packets:                                    # every slot flushed
            self._fifo_words.zero_()
            self._wr, self._rd = [0] * self.S, [0] * self.S
            self._flush.clear()
            self.last_present = (False,) * self.S
        if self._resampling:
            for t in (self._raw, self._raw_words, self._tail, self.out_client):
                t.zero_()
            self._raw_wr, self._tap = [0] * self.S, [self._tap0] * self.S
        if self.compact:
            self._tables.zero_()
            self._tables[1:3].fill_(-1)
            self.out.zero_()
            self._row_of, self._slot_of = [-1] * self.S, [-1] * self.S
            self._n_rows = 0
            self._last_rows = self.row_buckets[0]
            self._rgen_np.fill(-1)
        self._words.zero_()
        self._fault.zero_()
        self._gen = [0] * self.S
        self._pending.clear()
        self._resumes.clear()
        self._resume_batches.clear()
        if self.enroll_chunks:
            self._ewords.zero_()
            self._edone.zero_()
        self._capturing.clear()
        self._embedding.clear()                             # calls in flight finish; their rows are dropped by generation
        self._enroll_faults.clear()
        self._enrolled.clear()
        self._epending.clear()
        self._relook.clear()
        self._passthrough.clear()
        if self.monitor:                                    # gains and targets: wet 1, dry 0
            self._mix.zero_()
            self._mix[:, 0].fill_(1.0)
            self._targets = [(1.0, 0.0)] * self.S
            self._mix_posted = True

    def set_mix(self, slot: int, wet: float, dry: float):
        """From the next `step` on `slot` sounds `wet` x its separated rows + `dry` x its own input samples (a monitor
        streamer: `monitor=True`), each gain ramped on the device from where it stands, `monitor_ramp` samples per full
        swing.  Any slot, idle ones included: an idle slot's separated rows are zeros, so it sounds `dry` x the room."""
        self._slot(slot)
        if not self.monitor:
            raise ValueError("this SessionStreamer was built without a monitor: make_session_streamer(..., monitor=True)")
        wet, dry = float(wet), float(dry)
        if not (math.isfinite(wet) and math.isfinite(dry) and 0.0 <= wet <= 1.0 and 0.0 <= dry <= 1.0):
            raise ValueError(f"wet and dry are finite gains in [0, 1], got ({wet}, {dry})")
        target = (float(np.float32(wet)), float(np.float32(dry)))
        if target != self._targets[slot]:
            self._targets[slot] = target
            self._mix_posted = False

    def mix_of(self, slot: int) -> tuple:
        """(wet, dry): the targets of `slot`'s mix, as the device gets them (fp32 values)."""
        self._slot(slot)
        if not self.monitor:
            raise ValueError("this SessionStreamer was built without a monitor: make_session_streamer(..., monitor=True)")
        return self._targets[slot]

    def _slot(self, slot: int) -> int:
        if not 0 <= slot < self.S:
            raise IndexError(f"slot {slot} out of range for {self.S} slots")
        return slot

    def _new_gen(self) -> int:
        gen = self._next_gen
        self._next_gen = gen % self.GEN_MASK + 1
        return gen

    def _aborted(self) -> list:
        """Capturing slots whose done word reports the abort of their current generation."""
        d = self._edone_np
        return [s for s, (g, _) in self._capturing.items() if int(d[s]) & 0xffffffff == g | self.ENROLL_FAULT]

    def faults(self) -> list:
        """Slots the device closed (non-finite input, or an fp32 overflow inside the separator) since their last `open`, and
        idle slots whose enrollment capture it aborted (a non-finite recorded sample) since their last `enroll`."""
        f = self._fault_np
        out = [s for s, g in enumerate(self._gen) if g and int(f[s]) == g]
        if self._capturing or self._enroll_faults:
            out = sorted(set(out) | self._enroll_faults | set(self._aborted()))
        return out

    @property
    def active(self) -> list:
        """The host's view of the open slots: opened, not closed, no fault reported so far."""
        f = self._fault_np
        return [s for s, g in enumerate(self._gen) if g and int(f[s]) != g]

    @property
    def enrolling(self) -> list:
        """The slots whose clip is being recorded or embedded."""
        bad = set(self._aborted()) if self._capturing else ()
        return sorted(s for s in list(self._capturing) + list(self._embedding) if s not in bad)

    def embedding_of(self, slot: int) -> torch.Tensor:
        """The [256] device tensor `slot` was opened with by enrollment."""
        self._slot(slot)
        if slot not in self._enrolled:
            raise ValueError(f"slot {slot} was not opened by enrollment")
        return self._enrolled[slot]

    @property
    def rows_in_use(self) -> int:
        """Rows that held a listener in the last `step` (a lock-step streamer: every slot is a row)."""
        return self._n_rows if self.compact else self.S

    @property
    def last_rows(self) -> int:
        """The batch the last `step` launched its kernels for: the bucket of `rows_in_use`."""
        return self._last_rows if self.compact else self.S

    def _set_gain(self, slot: int, embed: torch.Tensor):
        st = self._st
        st.embed[slot].copy_(embed.reshape(-1), non_blocking=True)
        row = self._row_of[slot] if self.compact else slot
        if row >= 0:                                        # else: `_plan` does it once the slot has a row
            self._row_gain(slot, row)

    def _row_gain(self, slot: int, row: int):
        st = self._st
        with torch.no_grad():                               # this row only, eager, stream-ordered before the next replay
            self.net._speaker_gain(st.embed[slot:slot + 1], st.gain_raw[row:row + 1], st.gain[row:row + 1])

    def _plan(self):
        """The rows of the next chunk, from the rows of the last one: listeners that left give their rows up, survivors above
        the new row count move into the holes below it, openings take the holes that are left — and the tables that tell the
        device, in one asynchronous copy."""
        S, f, gen, pend = self.S, self._fault_np, self._gen, self._pending
        row_of, slot_of, n_old = self._row_of, self._slot_of, self._n_rows
        for r in range(n_old):                              # closed by the host, or by the device and seen now
            s = slot_of[r]
            # ... or closed / suspended and resumed since the last step: the row is the PREVIOUS listener's.  It is given up
            # like theirs, so that the resume is an opening and takes a hole — a row kept here could be a mover of this step,
            # and the move would copy the previous listener over what `_restore` has written
            if not gen[s] or int(f[s]) == gen[s] or s in self._resumes:
                slot_of[r], row_of[s] = -1, -1
        opens = [s for s, w in pend.items() if w & self.OPEN and row_of[s] < 0]
        keep = [r for r in range(n_old) if slot_of[r] >= 0]
        n = len(keep) + len(opens)
        holes = [r for r in range(n) if r >= n_old or slot_of[r] < 0]
        movers = [r for r in reversed(keep) if r >= n]     # src >= n > dst: disjoint, one launch
        src = self.net._host_words(4 * S, self.device)      # a FRESH pinned array per batch, as for the commands alone
        words = src.numpy().reshape(4, S)
        for dst, r in zip(holes, movers):
            s = slot_of[r]
            slot_of[dst], row_of[s], slot_of[r] = s, dst, -1
            words[0, dst] = r + 1
        for s, dst in zip(opens, holes[len(movers):]):
            slot_of[dst], row_of[s] = s, dst
            if s not in self._resumes:                      # a resumed listener's gain follows their embedding: `_restore`
                self._row_gain(s, dst)                      # a hole or a new row: never the source of a move
        words[1], words[2] = slot_of, row_of
        for s, w in pend.items():
            if w & self.OPEN:                               # a row whose listener left needs no word: it has no slot
                words[3, row_of[s]] = w
        pend.clear()
        self._tables[:4].copy_(src.view(4, S), non_blocking=True)
        self._n_rows = n
        self._slot_np[:n] = slot_of[:n]
        self._rgen_np[:n] = [gen[s] for s in slot_of[:n]]
        self._rgen_np[n:] = -1

    def _open(self, slot: int, embed: torch.Tensor):
        gen = self._new_gen()
        # the fault word of the previous listener holds an older generation: cleared for the host as of now, and on the
        # device by the chunk that opens the slot
        self._gen[slot] = gen
        self._pending[slot] = self.RESET | self.OPEN | (gen << self.GEN_SHIFT)
        self._set_gain(slot, embed)

    def open(self, slot: int, embed: torch.Tensor):
        """From the next `step` on `slot` is a fresh stream that listens for `embed` [256]."""
        self._slot(slot)
        if slot in self.active:
            raise ValueError(f"slot {slot} is open: close() it first")
        if slot in self._capturing or slot in self._embedding:
            self.poll()                                     # an aborted capture has left the slot idle
            if slot in self._capturing or slot in self._embedding:
                raise ValueError(f"slot {slot} is enrolling: close() it first")
        self._enroll_faults.discard(slot)
        self._enrolled.pop(slot, None)
        self._open(slot, embed)

    def enroll(self, slot: int, embedder, passthrough: bool = False):
        """From the next `step` on the rows of idle `slot` are recorded, `enroll_chunks` of them; then
        `embedder(clips [k, 2, 128 enroll_chunks]) -> [k, 256]` (an `EmbedTFGridNet` on this device) runs beside the chunk
        loop and the slot opens on its row.  Until then the slot's output rows are zeros — or, with `passthrough` (a monitor
        streamer), the listener's own input: the slot's mix goes to (0, 1) with the arming and back to (1, 0) in the step
        that opens the slot, so the room cross-fades into the target on the slot's first live chunk.  A capture that is
        aborted or cancelled leaves the mix where it is: the listener keeps the room until `set_mix` says otherwise."""
        self._slot(slot)
        if not self.enroll_chunks:
            raise ValueError("this SessionStreamer was built without enrollment: make_session_streamer(..., enroll_chunks=n)")
        if passthrough and not self.monitor:
            raise ValueError("passthrough is the dry path of a monitor streamer: make_session_streamer(..., monitor=True)")
        self.poll()
        if slot in self.active:
            raise ValueError(f"slot {slot} is open: close() it first")
        if slot in self._capturing or slot in self._embedding:
            raise ValueError(f"slot {slot} is enrolling already")
        self._gen[slot] = 0                                 # a slot the device closed for a fault is idle there already
        gen = self._new_gen()
        self._enroll_faults.discard(slot)
        self._enrolled.pop(slot, None)
        self._capturing[slot] = (gen, embedder)
        self._epending[slot] = self.ARM | (gen << self.GEN_SHIFT)
        self._passthrough.discard(slot)
        if passthrough:
            self.set_mix(slot, 0.0, 1.0)
            self._passthrough.add(slot)

    def relook(self, slot: int, embedder):
        """"Look once" at another speaker without leaving the session: from the next `step` on the rows of OPEN `slot` are
        recorded as `enroll` records an idle slot's, while the separator goes on with the current embedding — the slot stays
        in `active` (and is listed by `enrolling` too), keeps its row in a compacting streamer, and its output is bit for bit
        what it would be without the capture.  The finished embedding takes the `set_embedding` path: the carried state is
        kept, `embedding_of(slot)` is the new one.  `close` cancels the look and closes the session; an aborted capture leaves
        the old target in place (the non-finite input faults the session anyway); `suspend` is refused meanwhile."""
        self._slot(slot)
        if not self.enroll_chunks:
            raise ValueError("this SessionStreamer was built without enrollment: make_session_streamer(..., enroll_chunks=n)")
        self.poll()
        if slot in self._capturing or slot in self._embedding:
            raise ValueError(f"slot {slot} is enrolling already")
        if slot not in self.active:
            raise ValueError(f"slot {slot} is not open: enroll() it")
        gen = self._new_gen()
        self._capturing[slot] = (gen, embedder)
        self._epending[slot] = self.ARM | (gen << self.GEN_SHIFT)
        self._relook.add(slot)

    def close(self, slot: int):
        """From the next `step` on `slot` is idle: its output rows are exact zeros.  Also acknowledges a fault, and cancels an
        enrollment in progress: nothing opens later.  A `relook` is cancelled and its session closed."""
        self._slot(slot)
        if slot in self._capturing or slot in self._embedding:
            if self._capturing.pop(slot, None) is not None:
                self._epending[slot] = self.CANCEL
            self._embedding.pop(slot, None)                 # the call goes on; its row is dropped by generation
            self._passthrough.discard(slot)
            if slot not in self._relook:
                return
            self._relook.discard(slot)                      # ... and the session it ran beside is closed below
        if slot in self._enroll_faults:
            self._enroll_faults.discard(slot)
            return
        if not self._gen[slot]:
            raise ValueError(f"slot {slot} is not open")
        self._gen[slot] = 0
        self._enrolled.pop(slot, None)
        self._resumes.pop(slot, None)                       # resumed and closed before a `step`: nothing is restored
        self._pending[slot] = self.RESET | self.CLOSE

    def _snap_args(self, k: int, slot=None):
        """The leading arguments of lh_session_save / lh_session_restore up to the embedding: ping-pong set k, `slot`; of the
        *_rows forms without a slot: the embeddings of all slots."""
        live, rings, emb = self._spans_live[k], self._spans_rings, self._st.embed
        return (ctypes.addressof(live), len(live), ctypes.addressof(rings), len(rings), *self._ring_geom,
                (emb if slot is None else emb[slot]).data_ptr(), emb.shape[1] * emb.element_size())

    def _suspendable(self, slot: int):
        self._slot(slot)
        if slot in self._capturing or slot in self._embedding:
            raise ValueError(f"slot {slot} is enrolling: it has no session yet")
        if slot not in self.active:
            raise ValueError(f"slot {slot} is not open")
        if slot in self._pending:
            raise ValueError(f"slot {slot} was opened or resumed and no step has served it yet: it has no state on the device")

    def suspend(self, slot: int) -> SessionSnapshot:
        """The listener of open `slot` as a `SessionSnapshot`: their state as of the last `step`.  From the next `step` on the
        slot is idle exactly as after `close(slot)`.  Enqueues one launch and returns; never waits for the device."""
        self._suspendable(slot)
        st, net, S = self._st, self.net, self.S
        row = self._row_of[slot] if self.compact else slot
        words = self._tables[3:] if self.compact else self._words       # cmd from the host | cmd from the device | active
        pos = self._ring[0, row:row + 1] if self.pace else st.pos       # the word that holds this row's ring position
        data = torch.empty(self._snap_bytes, dtype=torch.uint8, device=self.device)
        with torch.no_grad(), net._device_ctx(st.chunk):
            # the set the next chunk reads is the one the last chunk wrote: sets[parity]
            net._lib(st.chunk).call("lh_session_save", *self._snap_args(st.parity, slot), data.data_ptr(), self._snap_bytes,
                                    words.data_ptr(), words[2].data_ptr(), pos.data_ptr(), row, S, net._stream(self.device))
            event = net._record_event(self.device)
        self._gen[slot] = 0
        self._enrolled.pop(slot, None)
        self._pending[slot] = self.RESET | self.CLOSE
        return SessionSnapshot(data, self._snap_layout, event)

    def _items(self, items: list) -> torch.Tensor:
        """A table of lh_snap_item_t (row, slot, generation, index) on the device: a FRESH pinned array and one asynchronous
        copy, as the command words travel."""
        src = self.net._host_words(4 * len(items), self.device)
        src.numpy().reshape(-1, 4)[:] = items
        table = torch.empty(len(items), 4, dtype=torch.int32, device=self.device)
        table.copy_(src.view(-1, 4), non_blocking=True)
        return table

    def suspend_many(self, slots) -> "SessionSnapshotBatch":
        """`suspend(s)` for every s of `slots`, in order, between the same two steps — the same snapshot bytes, the same slots idle
        afterwards — as ONE launch (`lh_session_save_rows`) into one fresh [k, snapshot bytes] tensor, behind one asynchronous
        copy of the item table.  Every ValueError of `suspend` applies, a slot named twice is one more; everything is checked
        before anything is enqueued or changed.  Never waits for the device."""
        slots = [int(s) for s in slots]
        for slot in slots:
            self._suspendable(slot)
        if len(set(slots)) != len(slots):
            raise ValueError(f"a slot is named twice: {slots}")
        st, net, S, k = self._st, self.net, self.S, len(slots)
        data = torch.empty(k, self._snap_bytes, dtype=torch.uint8, device=self.device)
        event = None
        if k:
            words = self._tables[3:] if self.compact else self._words   # cmd from the host | cmd from the device | active
            pos_rows, pos_shared = (self._ring[0].data_ptr(), None) if self.pace else (None, st.pos.data_ptr())
            items = self._items([(self._row_of[s] if self.compact else s, s, 0, i) for i, s in enumerate(slots)])
            with torch.no_grad(), net._device_ctx(st.chunk):
                net._lib(st.chunk).call("lh_session_save_rows", *self._snap_args(st.parity), data.data_ptr(), data.stride(0),
                                        words.data_ptr(), words[2].data_ptr(), pos_rows, pos_shared, items.data_ptr(), k, S,
                                        net._stream(self.device))
                event = net._record_event(self.device)
        for slot in slots:
            self._gen[slot] = 0
            self._enrolled.pop(slot, None)
            self._pending[slot] = self.RESET | self.CLOSE
        return SessionSnapshotBatch(data, self._snap_layout, event)

    def drain(self):
        """Everyone leaves: (the active slots in ascending order, `suspend_many` of them)."""
        slots = self.active
        return slots, self.suspend_many(slots)

    def _resumable(self, slot: int, layout: tuple, nbytes: int):
        self._slot(slot)
        if slot in self.active:
            raise ValueError(f"slot {slot} is open: close() it first")
        if slot in self._capturing or slot in self._embedding:
            self.poll()                                     # an aborted capture has left the slot idle
            if slot in self._capturing or slot in self._embedding:
                raise ValueError(f"slot {slot} is enrolling: close() it first")
        if layout != self._snap_layout or nbytes != self._snap_bytes:
            raise ValueError(f"the snapshot's layout {layout} ({nbytes} bytes) is not this Net's "
                             f"{self._snap_layout} ({self._snap_bytes} bytes)")

    def _resumed(self, slot: int, snapshot: SessionSnapshot) -> list:
        self._enroll_faults.discard(slot)
        self._enrolled.pop(slot, None)
        gen = self._new_gen()
        self._gen[slot] = gen
        # no RESET: lh_session_restore writes every byte a RESET would zero, apart from what the chunk rewrites itself
        self._pending[slot] = self.OPEN | (gen << self.GEN_SHIFT)
        self._resumes[slot] = entry = [snapshot, None]
        return entry

    def resume(self, slot: int, snapshot: SessionSnapshot):
        """From the next `step` on idle `slot` is the listener of `snapshot`: carried state, ring history, ring position and
        speaker embedding are theirs (there is no embedding argument).  ValueError for a snapshot of another model layout.
        Never waits for the device: a snapshot in another GPU's memory is copied over behind its event."""
        self._resumable(slot, snapshot.layout, snapshot.data.numel())
        self._resumed(slot, snapshot.to(self.device))

    def resume_many(self, slots, snapshots):
        """`resume(slots[i], snapshots[i])` for every i, in order — the generations handed out, `set_embedding` and `close`
        afterwards, dead snapshots, a compacting streamer's holes: all as there — but `step` restores them in ONE launch
        (`lh_session_restore_rows`) and computes their gains in one call.  `snapshots`: a `SessionSnapshotBatch`, or a sequence
        of `SessionSnapshot`; views of one batch use that batch in place (any subset, any order), anything else is stacked
        first.  A batch in another GPU's memory comes over in one copy behind its event.  Everything is checked before anything
        changes: a slot named twice, an open or enrolling slot and another model's layout are ValueErrors.  Never waits."""
        slots = [int(s) for s in slots]
        if isinstance(snapshots, SessionSnapshotBatch):
            batch, index = snapshots, list(range(len(snapshots)))
            layouts = [(batch.layout, batch.nbytes)] * len(index)
        else:
            snaps = list(snapshots)
            batch = snaps[0].batch if snaps and all(sn.batch is snaps[0].batch for sn in snaps) else None
            index = [sn.index for sn in snaps] if batch is not None else list(range(len(snaps)))
            layouts = [(sn.layout, sn.data.numel()) for sn in snaps]
        if len(slots) != len(index):
            raise ValueError(f"{len(slots)} slots for {len(index)} snapshots")
        if len(set(slots)) != len(slots):
            raise ValueError(f"a slot is named twice: {slots}")
        for slot, (layout, nbytes) in zip(slots, layouts):
            self._resumable(slot, layout, nbytes)
        if not slots:
            return
        batch = SessionSnapshotBatch.stack(snaps, self.device) if batch is None else batch.to(self.device)
        self._resume_batches.append((batch, {slot: (i, self._resumed(slot, batch[i])) for slot, i in zip(slots, index)}))

    def _restore(self):
        """The resumes of this step, behind the copy of the command words (a dead snapshot takes its OPEN back) and ahead of
        the chunk.  The rows are idle, and in a compacting streamer holes: no move of the step reads or writes them."""
        st, net, S = self._st, self.net, self.S
        words = self._tables[3:] if self.compact else self._words
        with torch.no_grad(), net._device_ctx(st.chunk):
            lib, stream = net._lib(st.chunk), net._stream(self.device)
            # `resume_many`: the slots of a batch that still hold that resume (not closed, or closed and resumed again, since)
            groups = [(batch, [(slot, i) for slot, (i, entry) in group.items() if self._resumes.get(slot) is entry])
                      for batch, group in self._resume_batches]
            batched = {slot for _, live in groups for slot, _ in live}
            for slot, (snap, embed) in self._resumes.items():
                if slot in batched:
                    continue
                row = self._row_of[slot] if self.compact else slot
                net._wait_event(self.device, snap.event, snap.data)
                pos_row, pos_shared = (self._ring[0, row:row + 1].data_ptr(), None) if self.pace else (None, st.pos.data_ptr())
                lib.call("lh_session_restore", *self._snap_args(st.parity, slot), snap.data.data_ptr(), snap.data.numel(),
                         words.data_ptr(), pos_row, pos_shared, self._fault[slot:slot + 1].data_ptr(), self._gen[slot], row, S,
                         stream)
                if embed is not None:                       # `set_embedding` after `resume`
                    st.embed[slot].copy_(embed.reshape(-1), non_blocking=True)
                self._row_gain(slot, row)
            for batch, live in groups:                      # one table, one restore launch, one gain call per batch
                if not live:
                    continue
                net._wait_event(self.device, batch.event, batch.data)
                items = self._items([(self._row_of[slot] if self.compact else slot, slot, self._gen[slot], i)
                                     for slot, i in live])
                pos_rows, pos_shared = (self._ring[0].data_ptr(), None) if self.pace else (None, st.pos.data_ptr())
                lib.call("lh_session_restore_rows", *self._snap_args(st.parity), batch.data.data_ptr(), batch.data.stride(0),
                         words.data_ptr(), pos_rows, pos_shared, self._fault.data_ptr(), items.data_ptr(), len(live), S, stream)
                for slot, _ in live:
                    embed = self._resumes[slot][1]
                    if embed is not None:                   # `set_embedding` after `resume_many`
                        st.embed[slot].copy_(embed.reshape(-1), non_blocking=True)
                net._speaker_gain_rows(st.embed, st.gain_raw, st.gain, items)
        self._resumes.clear()
        self._resume_batches.clear()

    def _packet_streamer(self):
        if not self.packets:
            raise ValueError("this SessionStreamer takes windows: make_session_streamer(..., pace=True, packets=True)")

    def buffered(self, slot: int) -> int:
        """Samples pushed for `slot` and not yet consumed by a `step` (host arithmetic; a pending `flush` counts as done)."""
        self._packet_streamer()
        slot = self._slot(slot)
        return 0 if slot in self._flush else (self._wr[slot] - self._rd[slot]) & self.COUNTER_MASK

    def ready(self) -> list:
        """The slots that hold a whole window, 192 samples: the next `step` consumes a chunk of each (host arithmetic)."""
        self._packet_streamer()
        return [s for s in range(self.S) if self.buffered(s) >= self.WINDOW]

    def flush(self, slot: int):
        """Drops what `slot` has buffered: a host that gives the slot to another client does this.  Travels with the slot's
        item of the next `push`, or in a push of its own that the next `step` issues."""
        self._packet_streamer()
        self._flush.add(self._slot(slot))

    def push(self, packets: dict):
        """packets {slot: CPU tensor [2, n]}, float32 (int16 in a `pcm16` streamer), any n >= 0: the clients' contiguous PCM
        as it arrived since the last call.  One fresh pinned buffer (item table, then the samples), one asynchronous copy
        and one `lh_session_feed` launch, whatever the number of packets; never waits for the device.  BufferError, before
        anything is enqueued or changed for any slot, when a slot would hold more than `fifo_samples`.
        A `client_rate` streamer takes the samples at the client's rate: they go to the slot's raw ring, and a second launch
        (`lh_session_resample_in`) makes the 16 kHz blocks whose taps are now complete — `fifo_samples` bounds those."""
        self._packet_streamer()
        S, R, M, dtype = self.S, self.fifo_samples, self.COUNTER_MASK, torch.int16 if self.pcm16 else torch.float32
        nch, wr, rd, flushed = self.chunk_in.shape[1], self._wr, self._rd, self._flush
        resamp, blocks = self._resampling, {}
        if resamp:                                          # the feed serves the raw ring; wr16 / rd stay the FIFO's
            wr16, wr, tap = self._wr, self._raw_wr, self._tap
            o, nn, K = self._o_in, self._n_in, self._k_in
        todo = []
        for slot, x in packets.items():
            slot = self._slot(int(slot))
            if not isinstance(x, torch.Tensor) or x.is_cuda or x.dtype != dtype or x.dim() != 2 or x.shape[0] != nch:
                raise ValueError(f"slot {slot}: a packet is a CPU {dtype} tensor [{nch}, n]")
            n = x.shape[1]
            if resamp:
                # the resampler's block arithmetic: a block is made once all K of its samples are there
                fl = slot in flushed
                have = 0 if fl else (wr16[slot] - rd[slot]) & M
                fill = ((0 if fl else wr[slot]) + n - (self._tap0 if fl else tap[slot])) & M
                nb = 0 if fill < K else (fill - K) // o + 1
                if have + nb * nn > R:
                    raise BufferError(f"slot {slot}: {have} samples buffered + {nb * nn} made of the {n} pushed > fifo_samples = "
                                      f"{R} (at 16 kHz): step() first (while ss.ready(): ss.step()), or flush(slot)")
                blocks[slot] = nb
                if n or fl:
                    todo.append((slot, x, n))
                continue
            have = 0 if slot in flushed else (wr[slot] - rd[slot]) & M
            if have + n > R:
                raise BufferError(f"slot {slot}: {have} samples buffered + {n} pushed > fifo_samples = {R}: "
                                  "step() first (while ss.ready(): ss.step()), or flush(slot)")
            if n or slot in flushed:
                todo.append((slot, x, n))
        if flushed:
            todo += [(slot, None, 0) for slot in sorted(flushed - {t[0] for t in todo})]
        if not todo:
            return
        net, st = self.net, self._st
        per = 2 if self.pcm16 else 1                        # samples per 32-bit word
        total = sum(nch * n for _, _, n in todo)
        used = self._item_words + (total + per - 1) // per
        src = net._host_words(used, self.device)            # FRESH, for the reason `step` gives for its command words
        buf = src.numpy()
        table = buf[:self.FEED_ITEM_WORDS * len(todo)].reshape(-1, self.FEED_ITEM_WORDS)
        samples = buf[self._item_words:].view(np.int16 if self.pcm16 else np.float32)
        i32 = lambda v: v - (1 << 32) if v >> 31 else v       # a 32-bit pattern as an int32 table holds it
        off, ritems = 0, []
        for i, (slot, x, n) in enumerate(todo):
            flush = slot in flushed
            if flush:
                wr[slot] = rd[slot] = 0
                if resamp:                                  # the stream restarts from silence: zero history, phase 0
                    wr16[slot], tap[slot] = 0, self._tap0
                    for t in (self._raw[slot], self._tail[slot], self._fifo_words[:, slot]):
                        t.zero_()
            at = wr[slot]
            table[i] = (slot, off, n, i32(at), self.FEED_FLUSH if flush else 0)
            if n:
                samples[off:off + nch * n].reshape(nch, n)[...] = x.numpy()
            wr[slot] = (at + n) & M
            off += nch * n
            nb = blocks.get(slot, 0)
            if nb:
                ritems.append((slot, nb, i32(wr16[slot]), i32(tap[slot])))
                wr16[slot], tap[slot] = (wr16[slot] + nb * nn) & M, (tap[slot] + nb * o) & M
        flushed.clear()
        if ritems:
            buf[self._ritem_off:self._ritem_off + self.RESAMPLE_ITEM_WORDS * len(ritems)].reshape(-1, self.RESAMPLE_ITEM_WORDS)[...] = ritems
        self._stage[:used].copy_(src, non_blocking=True)
        ring, words, Rr = (self._raw, self._raw_words, self.raw_samples) if resamp else (self._fifo, self._fifo_words, R)
        with torch.no_grad(), net._device_ctx(st.chunk):
            lib, stream = net._lib(st.chunk), net._stream(self.device)
            lib.call("lh_session_feed", self._stage[self._item_words:].data_ptr(), total * (4 // per),
                     self.FEED_S16 if self.pcm16 else self.FEED_F32, self._stage.data_ptr(), len(todo), ring.data_ptr(),
                     words[0].data_ptr(), words[1].data_ptr(), Rr, S, stream)
            if ritems:
                lib.call("lh_session_resample_in", ring.data_ptr(), Rr, self._stage[self._ritem_off:].data_ptr(), len(ritems),
                         self._fifo.data_ptr(), self._fifo_words[0].data_ptr(), R, S, self._bank_in.data_ptr(), o, nn,
                         self._w_in, stream)

    def set_embedding(self, slot: int, embed: torch.Tensor):
        """Re-target an open slot ("look once" at another speaker): the carried state is kept."""
        self._slot(slot)
        if not self._gen[slot]:
            raise ValueError(f"slot {slot} is not open")
        if slot in self._resumes:                           # the snapshot's embedding is not there yet: after the restore
            self._resumes[slot][1] = embed
            return
        self._set_gain(slot, embed)

    def poll(self):
        """Moves enrollments on, without waiting for the device: clips the device has completed go to the embedder on the side
        stream, finished embeddings open their slots.  `step` calls it first; call it more often if you like."""
        if not self._capturing and not self._jobs:
            return
        d, ready = self._edone_np, {}
        for s in sorted(self._capturing):
            g, embedder = self._capturing[s]
            w = int(d[s]) & 0xffffffff
            if w == g:
                ready.setdefault(embedder, []).append(s)
            elif w == g | self.ENROLL_FAULT:
                del self._capturing[s]
                self._passthrough.discard(s)                # the mix stays: the listener keeps the room
                if s in self._relook:                       # the session has its own fault word; the old target stays
                    self._relook.discard(s)
                else:
                    self._enroll_faults.add(s)
        for embedder, slots in ready.items():               # one call per embedder: a batch in ascending slot order
            gens = [self._capturing.pop(s)[0] for s in slots]
            # views and a copy on the side stream: nothing here moves host memory, so nothing waits
            clips = lambda: self._clips[slots[0]:slots[0] + 1] if len(slots) == 1 else torch.stack([self._clips[s] for s in slots])
            with torch.no_grad():
                out, done = self._side.run(lambda: embedder(clips()))
            self._embedding.update(zip(slots, gens))
            self._jobs.append((done, slots, gens, out))
        while self._jobs and self._side.finished(self._jobs[0][0]):      # one stream: the calls finish in order
            done, slots, gens, out = self._jobs.pop(0)
            self._side.hand_over(done, out)
            for i, s in enumerate(slots):
                if self._embedding.get(s) == gens[i]:       # else: cancelled (and perhaps enrolling again) meanwhile
                    del self._embedding[s]
                    if s in self._relook:                   # the session goes on: `set_embedding`, state kept
                        self._relook.discard(s)
                        if s in self.active:                # else the device closed it meanwhile: nothing to re-target
                            self._enrolled[s] = out[i]
                            self.set_embedding(s, out[i])
                        continue
                    self._enrolled[s] = out[i]
                    self._open(s, out[i])
                    if s in self._passthrough:              # with the OPEN: the cross-fade starts on the first live chunk
                        self._passthrough.discard(s)
                        self.set_mix(s, 1.0, 0.0)

    def step(self, chunks: Optional[torch.Tensor] = None, present=None) -> torch.Tensor:
        """chunks [S, 2, 192] (rows of idle slots are ignored) -> [S, 2, 128] (rows of idle slots are zeros); a view the next
        `step` overwrites.  Never raises for a slot's fault: see `faults()`.
        `present` (a paced streamer only): a length-S sequence or CPU bool tensor, false = the slot is held for this step —
        its row of `chunks` is ignored, its output row is zeros, its state stays.  None: everyone is present.
        A packet streamer takes neither: `step()` consumes one window of every slot that has 192 samples buffered, holds the
        others, and says which in `last_present`; the output is int16 when the streamer was built with `pcm16`."""
        st = self._st
        if self.packets:
            if chunks is not None or present is not None:
                raise ValueError("a packet streamer gets its samples through push(): step() takes no chunks and no `present`")
        elif chunks is None:
            raise ValueError("step() without chunks needs a packet streamer: make_session_streamer(..., pace=True, packets=True)")
        if present is not None and not self.pace:
            raise ValueError("`present` needs a paced streamer: make_session_streamer(..., pace=True)")
        st._check_repacked()
        st._check_versions()
        self.poll()
        if self.packets:
            if self._flush:                                 # a flush nobody pushed behind travels on its own
                self.push({})
            # what lh_session_frame will find and do, in the same arithmetic: nothing travels, nothing is read back
            wr, rd, M = self._wr, self._rd, self.COUNTER_MASK
            self.last_present = took = tuple((w - r) & M >= self.WINDOW for w, r in zip(wr, rd))
            for s, t in enumerate(took):
                if t:
                    rd[s] = (rd[s] + self.HOP) & M
        elif self.pace:
            held = self._none_held
            if present is not None:
                held = tuple(not p for p in (present.tolist() if isinstance(present, torch.Tensor) else present))
                if len(held) != self.S:
                    raise ValueError(f"`present` has {len(held)} entries for {self.S} slots")
            if held != self._held:                          # a steady loop copies nothing; a FRESH pinned array, as below
                src = self.net._host_words(self.S, self.device)
                src.numpy()[:] = held
                self._hold.copy_(src, non_blocking=True)
                self._held = held
        if self.compact:
            n = self._n_rows
            if self._pending or (n and (self._fault_np[self._slot_np[:n]] == self._rgen_np[:n]).any()):
                self._plan()
            self._last_rows = next(b for b in self.row_buckets if b >= self._n_rows)
        elif self._pending:
            # a FRESH pinned array per batch of commands: the host allocator hands its memory out again only after the
            # copy below has run, so a host that runs ahead of the device cannot overwrite commands in flight
            src = self.net._host_words(self.S, self.device)
            words = src.numpy()
            for slot, w in self._pending.items():
                words[slot] = w
            self._pending.clear()
            self._words[0].copy_(src, non_blocking=True)
        if self._epending:                                  # the LH_ENROLL_* words travel the same way
            src = self.net._host_words(self.S, self.device)
            words = src.numpy()
            for slot, w in self._epending.items():
                words[slot] = w
            self._epending.clear()
            self._ewords[0].copy_(src, non_blocking=True)
        if self.monitor and not self._mix_posted:           # the mix targets too: bit patterns of fp32, [2][S]
            src = self.net._host_words(2 * self.S, self.device)
            src.numpy().view(np.float32).reshape(2, self.S)[:] = np.asarray(self._targets, dtype=np.float32).T
            self._mix[0].view(torch.int32).copy_(src.view(2, self.S), non_blocking=True)
            self._mix_posted = True
        if self._resumes:
            self._restore()
        if not self.packets:
            self.chunk_in.copy_(chunks)
        with torch.no_grad():
            if self.graphs is None:
                self._body(st.parity, self.last_rows)
            elif self.compact:
                self.graphs[self._last_rows][st.parity].replay()
            else:
                self.graphs[st.parity].replay()
        st.parity ^= 1
        if self._resampling:
            return self.out_client
        return self.out16 if self.pcm16 else self.out
