"""Harness shared by tests/test_gpu_data_stages.py (MI355X) and tests/test_emu_data_stages.py (hipemu, CPU) for the two kernel
families around the model: the binaural renderer (lh_render_binaural: k_fir_causal, k_fft_conv, k_mix_peak, k_mix_apply) and the
eval metrics (lh_metric_sums: k_metric_moments, k_metric_finish, k_metric_total).

`DataRig` calls the two C-ABI entry points of include/lookonce_hip.h directly.  Every output lives in a `Guarded` buffer
(tests/stage_cases.py) of exactly the documented size, pre-filled with the guard's bit pattern, and every call asserts that the
guards are unchanged.  Inputs are made on the host from seeded generators and the references run on the host in float64.

Renderer.  White inputs: sources N(0, 0.1^2), responses N(0, 1) / sqrt(Lh) — the last tap weighs as much as the first, so a
dropped or misplaced tap anywhere moves the result by percents — a gain from [0.5, 3] on EVERY row and a target row drawn from
all S1 rows (the last utterance of a batch takes the noise row).  Per case:
  * each events row [2][N] within 4e-6 * amp * max(1, sqrt(Lh / 256)) of `render_oracle.convolve_trunc(exact=True)` * gain,
    amp = max |float64 row| of THAT row (tests/test_render.py's bound, which takes amp over the whole utterance);
  * peak within twice that bound, amp = the utterance's largest row (every row's error adds into the mixture), of the float64
    peak max |sum of rows|;
  * mixture, target and peak equal to `render_oracle.mix` applied to the device's own events (fp32 torch, reference order);
  * a second call gives equal bits, and so does utterance b rendered alone (B = 1).

Metric sums.  The reference is the float64 restatement below with eps FIXED at the fp32 value 1.1920928955078125e-07 (what
torchmetrics uses on the fp32 tensors of the reference's eval and what the kernel uses): the centred definition — subtract the
means, alpha, scaled, noise, 10 log10((|scaled|^2 + eps) / (|noise|^2 + eps)) — and the cosine with each norm clamped at 1e-8.
Per case:
  * rows [B][3] fp32 = (output_sisnr, si_snr_i, embedding_sim): the dB columns within 1e-4 dB (tests/test_gpu_parity.py's
    bound), the cosine within 2^-23 (fp64 arithmetic rounded to fp32 once: one fp32 ulp at 1);
  * sums[3] == B, sums[2] within 1e-12 * B;
  * sums[0], sums[1]: a second host value in the KERNEL's algebra (raw moments added sample by sample, pt = sum pt - n mp mt,
    ...) lies at distance d from the centred definition — the conditioning of that algebra on these signals; the bound is
    min(1e-4, max(1e-9, 16 d)) dB per utterance, summed over B (16: the kernel's summation tree is not numpy's; the 1e-4 cap is
    a requirement, not a measurement);
  * rows of utterance b alone (B = 1) have the bits of row b of the batch, and its sums those of the batch's fp64 row b (the
    [B][3] tail of the scratch: si_snr_i, output_sisnr, embedding_sim); a second call gives equal bits.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import render_oracle as R
from tests.stage_cases import GUARD, Guarded

EPS32 = 1.1920928955078125e-07                             # torch.finfo(torch.float32).eps
LH_ERR_ARG = 1
MT_PART = 2 * 16 * 8                                       # fp64 partials per utterance in lh_metric_sums' scratch
F32, F64 = torch.float32, torch.float64


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def check(results: dict, case: str):
    """results {name: (value, bound)}: print every value next to its bound (None: information only), then assert all of them."""
    bad = []
    for k, (v, b) in results.items():
        print(f"{case:>34} {k:<22} {v:.3e}" + ("" if b is None else f"  (bound {b:.3e})"))
        if b is not None and not v <= b:
            bad.append((k, v, b))
    assert not bad, f"{case}: {bad}"


# ---- renderer: inputs and float64 reference
def render_scene(seed: int, B: int, S1: int, N: int, Lh: int, gains=(0.5, 3.0)):
    g = torch.Generator().manual_seed(seed)
    src = (0.1 * torch.randn(B, S1, N, generator=g, dtype=F64)).float()
    rir = (torch.randn(B, S1, 2, Lh, generator=g, dtype=F64) / math.sqrt(Lh)).float()
    gain = (gains[0] + (gains[1] - gains[0]) * torch.rand(B, S1, generator=g, dtype=F64)).float()
    tgt = torch.randint(0, S1, (B,), generator=g).to(torch.int32)
    if B > 1:
        tgt[-1] = S1 - 1                                   # the noise row as the target
    return src, rir, gain, tgt


def render_ref(src, rir, gain) -> torch.Tensor:
    """float64 events [B][S1][2][N]: convolve(src, rir[ear])[:N] * gain per row."""
    B, S1, _ = src.shape
    rows = [[torch.from_numpy(R.convolve_trunc(src[b, s].numpy(), rir[b, s].numpy(), exact=True)) * float(gain[b, s])
             for s in range(S1)] for b in range(B)]
    return torch.stack([torch.stack(r) for r in rows])


# ---- metric sums: inputs and float64 references
SIGNALS = ("plain", "dc", "close", "equal", "silent_target", "const_target", "silent_output", "x1e4", "x1e-6")


def metric_signals(seed: int, B: int, n: int, E: int, kind: str = "plain"):
    """(outputs, target, mixture [B][2][n], emb, emb_gt [B][E]) fp32.  plain: target N(0, 0.1^2), output 6 dB above its error,
    mixture 6 dB below; the other classes of SIGNALS change that as their name says."""
    assert kind in SIGNALS
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    t = 0.1 * rn(B, 2, n)
    o = t + 0.05 * rn(B, 2, n)
    m = t + 0.2 * rn(B, 2, n)
    e = rn(B, E)
    eg = e + 0.5 * rn(B, E)
    if kind == "dc":                                       # offsets of 3 .. 5, AC part 0.1: 30 dB above it
        off = lambda: (3.0 + 2.0 * torch.rand(B, 2, 1, generator=g, dtype=F64)) * (1 - 2 * torch.randint(0, 2, (B, 2, 1), generator=g))
        t, o, m = t + off(), o + off(), m + off()
    elif kind == "close":                                  # about 80 dB
        o = t + 1e-5 * rn(B, 2, n)
    elif kind == "equal":
        o = t.clone()
    elif kind == "silent_target":
        t = torch.zeros_like(t)
        e[0] = 0.0                                         # a zero embedding row on either side of the cosine
        eg[B - 1] = 0.0
    elif kind == "const_target":
        c = torch.tensor([0.7, -1.3, 0.3, 0.9, -0.6, 1.1], dtype=F64)   # inexact in binary: the raw moments round
        t = c[torch.arange(B * 2) % 6].reshape(B, 2, 1).expand(B, 2, n).clone()
    elif kind == "silent_output":
        o = torch.zeros_like(o)
    elif kind in ("x1e4", "x1e-6"):
        k = float(kind[1:])
        t, o, m = t * k, o * k, m * k
    return tuple(x.float().contiguous() for x in (o, t, m, e, eg))


def si_snr_centred(p: np.ndarray, t: np.ndarray) -> np.ndarray:
    """The definition, float64 over the last axis, eps = fp32 eps."""
    p = p - p.mean(-1, keepdims=True)
    t = t - t.mean(-1, keepdims=True)
    alpha = ((p * t).sum(-1, keepdims=True) + EPS32) / ((t * t).sum(-1, keepdims=True) + EPS32)
    scaled = alpha * t
    noise = scaled - p
    return 10.0 * np.log10(((scaled * scaled).sum(-1) + EPS32) / ((noise * noise).sum(-1) + EPS32))


def si_snr_moments(p: np.ndarray, t: np.ndarray) -> np.ndarray:
    """The same quantity in the algebra of lh_metrics.hip (si_snr_from_moments): raw float64 moments, centred afterwards.
    The moments are added one sample after the other (cumsum): the order whose rounding error no summation tree exceeds on
    average, and one that is not exact by construction on a constant signal, as numpy's pairwise `sum` of equal terms is."""
    n = float(p.shape[-1])
    seq = lambda x: np.cumsum(x, -1)[..., -1]
    sp, st, spp, stt, spt = seq(p), seq(t), seq(p * p), seq(t * t), seq(p * t)
    mp, mt = sp / n, st / n
    pt, tt, pp = spt - n * mp * mt, stt - n * mt * mt, spp - n * mp * mp
    alpha = (pt + EPS32) / (tt + EPS32)
    sig = alpha * alpha * tt
    noise = sig - 2.0 * alpha * pt + pp
    return 10.0 * np.log10((sig + EPS32) / (np.maximum(noise, 0.0) + EPS32))


def metric_ref(o, t, m, e, eg):
    """float64 [B][3] = (output_sisnr, si_snr_i, embedding_sim) by the centred definition, and [B][2] = the two dB columns in
    the kernel's algebra."""
    o, t, m, e, eg = (x.double().numpy() for x in (o, t, m, e, eg))
    cols = []
    for f in (si_snr_centred, si_snr_moments):
        so, sm = f(o, t), f(m, t)                          # [B][2]
        cols.append((so.mean(1), (so - sm).mean(1)))
    cos = (e * eg).sum(1) / (np.maximum(np.sqrt((e * e).sum(1)), 1e-8) * np.maximum(np.sqrt((eg * eg).sum(1)), 1e-8))
    return np.stack([cols[0][0], cols[0][1], cos], 1), np.stack([cols[1][0], cols[1][1]], 1)


class DataRig:
    """A `Lib`, a device, a stream and a way to wait for it."""

    def __init__(self, lib, device, stream, sync=lambda: None):
        self.lib, self.dev, self.st, self.sync = lib, torch.device(device), stream, sync

    def g(self, shape, dtype=F32):
        return Guarded(shape, dtype, self.dev)

    # ---- lh_render_binaural
    def render_call(self, src, rir, gain, tgt):
        """One call on host tensors -> host tensors (events [B][S1][2][N], peak [B] fp32, mixture, target [B][2][N])."""
        B, S1, N = src.shape
        Lh = rir.shape[3]
        ins = [x.contiguous().to(self.dev) for x in (src, rir, gain, tgt)]
        ev, pk, mx, tg = self.g((B, S1, 2, N)), self.g((B,)), self.g((B, 2, N)), self.g((B, 2, N))
        self.lib.call("lh_render_binaural", *[x.data_ptr() for x in ins], ev.t.data_ptr(), pk.t.data_ptr(), mx.t.data_ptr(),
                      tg.t.data_ptr(), B, S1, N, Lh, self.st)
        self.sync()
        for n, x in (("events", ev), ("peak", pk), ("mixture", mx), ("target", tg)):
            x.check(f"lh_render_binaural {n} B={B} S1={S1} N={N} Lh={Lh}")
        return tuple(x.t.cpu().clone() for x in (ev, pk, mx, tg))

    @staticmethod
    def _mix_of(ev, tgt):
        """`render_oracle.mix` per utterance on rendered rows [B][S1][2][N] -> (mixture, target, peak)."""
        out = [R.mix([ev[b, i] for i in range(ev.shape[1] - 1)], ev[b, -1], 1.0, int(tgt[b])) for b in range(ev.shape[0])]
        return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out]), torch.stack([o[2] for o in out])

    def render_case(self, B, S1, N, Lh, seed=0, gains=(0.5, 3.0)):
        src, rir, gain, tgt = render_scene(seed, B, S1, N, Lh, gains)
        ev, pk, mx, tg = self.render_call(src, rir, gain, tgt)
        ref = render_ref(src, rir, gain)
        what = f"B={B} S1={S1} N={N} Lh={Lh}"
        k = 4e-6 * max(1.0, math.sqrt(Lh / 256))
        amp = ref.abs().amax((2, 3))                                         # [B][S1]
        err = (ev.double() - ref).abs().amax((2, 3))
        i = int((err / (k * amp)).argmax())                                  # the row that uses most of its bound
        res = {"events": (float(err.flatten()[i]), float(k * amp.flatten()[i]))}
        pk64 = ref.sum(1).abs().amax((1, 2))                                 # [B]
        perr, pbound = (pk.double() - pk64).abs(), 2 * k * amp.amax(1)
        i = int((perr / pbound).argmax())
        res["peak"] = (float(perr[i]), float(pbound[i]))
        res["peak.value"] = (float(pk.max()), None)
        mm, tt, nn = self._mix_of(ev, tgt)
        assert torch.equal(mm, mx), f"{what}: mixture is not the reference's mix of the device's events"
        assert torch.equal(tt, tg), f"{what}: target is not row tgt_idx of the device's events (normalised)"
        assert torch.equal(nn, pk), f"{what}: peak is not max |mixture| of the device's events"
        again = self.render_call(src, rir, gain, tgt)
        assert all(same_bits(a, b) for a, b in zip((ev, pk, mx, tg), again)), f"{what}: a second call differs"
        if B > 1:
            for b in range(B):
                alone = self.render_call(src[b:b + 1], rir[b:b + 1], gain[b:b + 1], tgt[b:b + 1])
                assert all(same_bits(a[b:b + 1], x) for a, x in zip((ev, pk, mx, tg), alone)), f"{what}: utterance {b} alone differs"
        return res

    def render_threshold(self, top: float, Lh: int):
        """Unit-impulse responses and a source whose largest |sample| is exactly `top`: the peak is `top`; at 1.0 nothing is
        divided, one ulp above everything is (IEEE division) and 0.25 becomes 0.2499999702."""
        N = 301
        g = torch.Generator().manual_seed(5)
        src = torch.zeros(1, 2, N)
        src[0, 0] = torch.rand(N, generator=g) - 0.5
        src[0, 0, 17], src[0, 0, 200] = 0.25, -top                           # the peak is an absolute value
        rir = torch.zeros(1, 2, 2, Lh)
        rir[:, :, :, 0] = 1.0
        ev, pk, mx, tg = self.render_call(src, rir, torch.ones(1, 2), torch.zeros(1, dtype=torch.int32))
        want = src[:, :1].expand(1, 2, N)
        assert torch.equal(ev[0, 0], want[0]) and not bool(ev[0, 1].any()), "unit impulse: events != source"
        assert float(pk[0]) == top, (float(pk[0]), top)
        if top > 1.0:
            want = want / torch.tensor(top, dtype=F32)
            assert float(mx[0, 0, 17]) == float(np.float32(0.2499999702)) != 0.25
        assert same_bits(mx, want) and same_bits(tg, want), f"top={top!r}: wrong side of the normalisation threshold"

    def render_refusals(self):
        """A null pointer or B, S1, N, Lh <= 0: LH_ERR_ARG, and nothing is written."""
        B, S1, N, Lh = 1, 2, 16, 4
        src, rir, gain, tgt = (x.to(self.dev) for x in render_scene(0, B, S1, N, Lh))
        outs = [self.g((B, S1, 2, N)), self.g((B,)), self.g((B, 2, N)), self.g((B, 2, N))]
        good = [x.data_ptr() for x in (src, rir, gain, tgt)] + [x.t.data_ptr() for x in outs] + [B, S1, N, Lh, self.st]
        fn = self.lib.raw("lh_render_binaural")
        self._refusals(fn, good, 8, 4, outs)

    # ---- lh_metric_sums
    def metric_call(self, o, t, m, e, eg):
        """One call on host tensors -> host tensors (rows [B][3] fp32, sums [4] fp64, fp64 rows [B][3] of the scratch tail)."""
        B, _, n = o.shape
        E = e.shape[1]
        ins = [x.contiguous().to(self.dev) for x in (o, t, m, e, eg)]
        scratch, rows, sums = self.g((B * MT_PART + B * 3,), F64), self.g((B, 3)), self.g((4,), F64)
        self.lib.call("lh_metric_sums", *[x.data_ptr() for x in ins], scratch.t.data_ptr(), rows.t.data_ptr(), sums.t.data_ptr(),
                      B, n, E, self.st)
        self.sync()
        for nm, x in (("scratch", scratch), ("rows", rows), ("sums", sums)):
            x.check(f"lh_metric_sums {nm} B={B} n={n} emb_dim={E}")
        return rows.t.cpu().clone(), sums.t.cpu().clone(), scratch.t[B * MT_PART:].view(B, 3).cpu().clone()

    def metric_case(self, B, n, E=256, kind="plain", seed=0):
        sig = metric_signals(seed, B, n, E, kind)
        rows, sums, rows64 = self.metric_call(*sig)
        ref, mom = metric_ref(*sig)
        what = f"B={B} n={n} emb_dim={E} {kind}"
        assert np.isfinite(ref).all() and np.isfinite(mom).all(), what
        r = rows.double().numpy()
        res = {"rows.output_sisnr": (float(np.abs(r[:, 0] - ref[:, 0]).max()), 1e-4),
               "rows.si_snr_i": (float(np.abs(r[:, 1] - ref[:, 1]).max()), 1e-4),
               "rows.embedding_sim": (float(np.abs(r[:, 2] - ref[:, 2]).max()), 2.0 ** -23)}
        s = sums.numpy()
        assert s[3] == float(B), f"{what}: sums[3] = {s[3]}"
        for i, col, nm in ((0, 1, "si_snr_i"), (1, 0, "output_sisnr")):      # sums = (sum si_snr_i, sum output_sisnr, ...)
            d = np.abs(mom[:, col] - ref[:, col])
            res[f"sums[{i}].d"] = (float(d.sum()), None)
            res[f"sums[{i}] {nm}"] = (abs(float(s[i]) - float(ref[:, col].sum())), float(np.minimum(1e-4, np.maximum(1e-9, 16 * d)).sum()))
        res["sums[2] embedding_sim"] = (abs(float(s[2]) - float(ref[:, 2].sum())), 1e-12 * B)
        again = self.metric_call(*sig)
        assert all(same_bits(a, b) for a, b in zip((rows, sums, rows64), again)), f"{what}: a second call differs"
        for b in range(B if B > 1 else 0):
            rb, sb, _ = self.metric_call(*[x[b:b + 1] for x in sig])
            assert same_bits(rb[0], rows[b]), f"{what}: rows of utterance {b} alone differ"
            assert same_bits(sb[:3], rows64[b]) and float(sb[3]) == 1.0, f"{what}: sums of utterance {b} alone differ"
        return res

    def metric_refusals(self):
        B, n, E = 2, 16, 8
        ins = [x.to(self.dev) for x in metric_signals(0, B, n, E)]
        outs = [self.g((B * MT_PART + B * 3,), F64), self.g((B, 3)), self.g((4,), F64)]
        good = [x.data_ptr() for x in ins] + [x.t.data_ptr() for x in outs] + [B, n, E, self.st]
        self._refusals(self.lib.raw("lh_metric_sums"), good, 8, 3, outs)

    def _refusals(self, fn, good, n_ptr, n_int, outs):
        for i in range(n_ptr):
            a = list(good)
            a[i] = None
            assert fn(*a) == LH_ERR_ARG, f"null pointer in argument {i} accepted"
        for i in range(n_ptr, n_ptr + n_int):
            for v in (0, -1):
                a = list(good)
                a[i] = v
                assert fn(*a) == LH_ERR_ARG, f"argument {i} = {v} accepted"
        self.sync()
        for x in outs:
            assert bool((x.ibuf == x.pat).all()), "a refused call wrote to an output"
        assert fn(*good) == 0
        self.sync()
        for x in outs:
            x.check("call after the refusals")
            assert not bool((x.ibuf[GUARD:GUARD + x.n] == x.pat).any()), "an accepted call left an output element unwritten"


# ---- case tables, shared by both back ends (every case takes well under a second on either)
# (B, S1, N, Lh); direct form: Lh < 1024 or Lh > 4097.  FIR_TILE = 2048 outputs per workgroup, 8 per thread; 8-tap chunks, two
# per loop trip; FIR_KT = 2048 taps per stage
RENDER_DIRECT = [
    (1, 1, 1, 1),
    (2, 3, 513, 1), (2, 3, 2047, 7), (2, 3, 2048, 8), (3, 5, 2049, 9), (2, 3, 2052, 15), (2, 2, 4100, 16), (2, 3, 300, 17),
    (2, 3, 700, 24), (2, 3, 700, 72), (1, 2, 2100, 1000),    # 3, 9 and 125 chunks: the odd trip of the two-chunk loop
    (1, 3, 1100, 1023), (1, 2, 1100, 1017),                  # ragged tail (7 taps, 1 tap) at chunk 127
    (1, 2, 4400, 4101), (1, 2, 6200, 4101),                  # ragged tail in the third stage; workgroups skip to 1, 2, 3 stages
    (1, 2, 2052, 4104), (1, 2, 4400, 4098),                  # just past the FFT range: a multiple of 8, and 2 taps in stage 3
    (1, 1, 6400, 6151),                                      # four stages with a 7-tap tail
    (2, 3, 300, 1000), (1, 2, 2049, 4104),                   # N < Lh
]
# FC_L = 4096 outputs per block, 5 blocks per workgroup, 1024 <= Lh <= 4097
RENDER_FFT = [
    (2, 3, 9000, 1024), (1, 2, 4096, 1025), (1, 2, 4097, 4096), (3, 5, 1, 4097), (1, 1, 4097, 4097),
    (1, 2, 20481, 1024),                                     # 6 blocks: the second workgroup has one block of one sample
    (1, 1, 24577, 1025),                                     # 7 blocks
    (1, 2, 1500, 3001),                                      # N < Lh
]
# gains of about 20: a peak far above 1, on both paths
RENDER_LOUD = [(2, 3, 2052, 33), (1, 2, 4100, 1024)]

METRIC_N = [1, 2, 3, 5, 63, 64, 65, 1023, 1024, 1025, 1026, 4099, 16384, 16385, 65537]      # at B = 3: every row alignment
METRIC_B = [1, 4, 5, 9]                                                                       # at n = 1001
METRIC_E = [1, 63, 64, 65, 256, 300]                                                          # at B = 3, n = 1001
