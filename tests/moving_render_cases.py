"""Harness shared by tests/test_gpu_moving_render.py (MI355X) and tests/test_emu_moving_render.py (hipemu, CPU) for the
moving-source renderer: lh_render_moving (k_fir_moving, then lh_render_binaural's k_mix_peak / k_mix_apply) and lh_path_nearest
(k_path_nearest).  `MovingRig` extends tests/data_stage_cases.DataRig: the C-ABI entry points are called directly, every output
lives in a `Guarded` buffer (tests/stage_cases.py) and every call asserts that the guards are unchanged.

The renderer's arithmetic is the project's own definition (include/lookonce_hip.h), so the reference here is that definition
in float64, not a restatement of the reference project's absent native simulator:
    y64 = (a64 + w (b64 - a64)) gain,  a64 / b64 = float64 convolutions of the fp32 inputs with the responses of path points
    f and f + 1 (f = n // frame),  w = the fp32 value (float)(n % frame) / (float)frame.
Inputs follow `render_scene`'s recipe: sources N(0, 0.1^2), taps N(0, 1) / sqrt(Lh), a gain from [0.5, 3] on every row, a target
drawn from all S1 rows (the last utterance of a batch takes the noise row).  Per case:
  * each events row [2][N] within (4e-6 max(1, sqrt(Lh / 256)) + 2^-21) amp gain of y64, amp = max over n and ears of
    max(|a64|, |b64|) of THAT row: the first term is the static renderer's bound (tests/data_stage_cases.py), which applies to
    each chain, the second covers the three roundings of the blend (b - a, the fmaf, the gain);
  * peak, mixture and target equal to `render_oracle.mix` applied to the device's own events;
  * a second call gives equal bits, and so does utterance b rendered alone (B = 1, the whole bank).
`const_case`: a path that stays on one bank entry has the bits of lh_render_binaural with that response (events, peak,
mixture, target) outside the static FFT range; inside it (1024 <= Lh <= 4097) the two agree within the static bound.
`blend_exact`: the blend weight itself, to the bit (a silent entry and a unit impulse under a constant source).
`delay_case`: what the frame index and the ear order MEAN, measured by code the renderer's author did not write — bank entry p
delays the left ear by p samples; the host's moving-mode cue metric must find p in every 250 ms segment.
`nearest_case`: float64 argmax of the dot products; a point whose best and second-best dots are closer in float64 than
4 * 2^-24 * sum_i |v_i| |p_i| is ambiguous (each fp32 dot carries at most 3 roundings of relative size 2^-24 on terms bounded
by that sum) — there the device's choice must be within that margin of the best, elsewhere it must be the argmax; at most 1 % of
the points may be ambiguous.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.data_stage_cases import F32, F64, LH_ERR_ARG, DataRig, same_bits

LH_ERR_UNSUPPORTED = 2
I32 = torch.int32


def fir_bound(Lh: int) -> float:
    return 4e-6 * max(1.0, math.sqrt(Lh / 256)) + 2.0 ** -21


def static_bound(Lh: int) -> float:
    return 4e-6 * max(1.0, math.sqrt(Lh / 256))


def n_points(N: int, frame: int) -> int:
    return -(-N // frame) + 1


def make_idx(g, pattern: str, B: int, S1: int, F: int, P: int) -> torch.Tensor:
    """[B][S1][F] int32.  distinct: consecutive entries all differ (all F differ when P >= F); alt: 0 and P - 1 in turn;
    mixed: runs of 1 .. 3 equal entries, entries 0 and P - 1 among them; const: one entry per row."""
    idx = torch.zeros(B, S1, F, dtype=torch.int64)
    for b in range(B):
        for s in range(S1):
            if pattern == "distinct":
                idx[b, s] = (torch.arange(F) + 3 * s + 5 * b) % P
            elif pattern == "alt":
                idx[b, s] = torch.where((torch.arange(F) + s) % 2 == 0, 0, P - 1)
            elif pattern == "const":
                idx[b, s] = int(torch.randint(0, P, (1,), generator=g))
            elif pattern == "mixed":
                vals, runs = [], 0
                while len(vals) < F:
                    v = (0, P - 1)[runs] if runs < 2 else int(torch.randint(0, P, (1,), generator=g))
                    vals += [v] * int(torch.randint(1, 4, (1,), generator=g))
                    runs += 1
                idx[b, s] = torch.tensor(vals[:F])
            else:
                raise KeyError(pattern)
    return idx.to(I32)


def moving_inputs(seed, B, S1, N, Lh, frame, P, K, pattern, extra=0, gains=(0.5, 3.0)):
    g = torch.Generator().manual_seed(seed)
    src = (0.1 * torch.randn(B, S1, N, generator=g, dtype=F64)).float()
    bank = (torch.randn(K, P, 2, Lh, generator=g, dtype=F64) / math.sqrt(Lh)).float()
    gain = (gains[0] + (gains[1] - gains[0]) * torch.rand(B, S1, generator=g, dtype=F64)).float()
    tgt = torch.randint(0, S1, (B,), generator=g).to(I32)
    if B > 1:
        tgt[-1] = S1 - 1                                   # the noise row as the target
    bank_of = ((K - 1 - torch.arange(B)) % K).to(I32)      # K = 3, B = 3: (2, 1, 0); B > K wraps
    if K > 2 and B > 2:
        bank_of[:3] = torch.tensor([1, 2, 0], dtype=I32)   # a permutation that is no reversal
    idx = make_idx(g, pattern, B, S1, n_points(N, frame) + extra, P)
    return src, bank, bank_of, idx, gain, tgt


def blend_weights(N: int, frame: int) -> np.ndarray:
    """The definition's w: fp32 IEEE division of the fp32 values of n % frame and frame."""
    return (np.arange(N) % frame).astype(np.float32) / np.float32(frame)


def moving_ref(src, bank, bank_of, idx, gain, frame):
    """float64 (events [B][S1][2][N], amp [B][S1]): the definition with a, b_ and the blend in float64."""
    B, S1, N = src.shape
    f = np.arange(N) // frame
    w = blend_weights(N, frame).astype(np.float64)
    ev = np.zeros((B, S1, 2, N))
    amp = np.zeros((B, S1))
    for b in range(B):
        bk = bank[int(bank_of[b])].double().numpy()
        for s in range(S1):
            x = src[b, s].double().numpy()
            row = idx[b, s].numpy()
            ia, ib = row[f], row[f + 1]
            conv = {int(p): np.stack([np.convolve(x, bk[p, e])[:N] for e in range(2)]) for p in np.unique(np.concatenate([ia, ib]))}
            a, c = _gather(conv, ia), _gather(conv, ib)
            ev[b, s] = (a + w * (c - a)) * float(gain[b, s])
            amp[b, s] = max(np.abs(a).max(), np.abs(c).max())
    return torch.from_numpy(ev), torch.from_numpy(amp)


def _gather(conv: dict, which: np.ndarray) -> np.ndarray:
    out = np.zeros((2, which.shape[0]))
    for p, c in conv.items():
        m = which == p
        out[:, m] = c[:, m]
    return out


class MovingRig(DataRig):
    """`DataRig` plus a host object (`BinauralRenderer`, or tests/hipemu/hosts.EmuRenderer) for the end-to-end case."""

    def __init__(self, lib, device, stream, sync=lambda: None, renderer=None):
        super().__init__(lib, device, stream, sync)
        self.renderer = renderer

    # ---- lh_render_moving
    def moving_call(self, src, bank, bank_of, idx, gain, tgt, frame):
        """One call on host tensors -> host tensors (events [B][S1][2][N], peak [B] fp32, mixture, target [B][2][N])."""
        B, S1, N = src.shape
        K, P, _, Lh = bank.shape
        F = idx.shape[2]
        ins = [x.contiguous().to(self.dev) for x in (src, bank, bank_of, idx, gain, tgt)]
        ev, pk, mx, tg = self.g((B, S1, 2, N)), self.g((B,)), self.g((B, 2, N)), self.g((B, 2, N))
        self.lib.call("lh_render_moving", *[x.data_ptr() for x in ins], ev.t.data_ptr(), pk.t.data_ptr(), mx.t.data_ptr(),
                      tg.t.data_ptr(), B, S1, N, Lh, P, K, F, frame, self.st)
        self.sync()
        for n, x in (("events", ev), ("peak", pk), ("mixture", mx), ("target", tg)):
            x.check(f"lh_render_moving {n} B={B} S1={S1} N={N} Lh={Lh} frame={frame} P={P} K={K} F={F}")
        return tuple(x.t.cpu().clone() for x in (ev, pk, mx, tg))

    def _events_vs_ref(self, ev, ref, amp, gain, Lh, bound=fir_bound):
        k = bound(Lh)
        lim = k * amp * gain.double()                                        # [B][S1]
        err = (ev.double() - ref).abs().amax((2, 3))
        use = torch.where(lim > 0, err / lim, torch.where(err > 0, math.inf, 0.0).double())       # a silent row must stay silent
        i = int(use.argmax())                                                # the row that uses most of its bound
        return float(err.flatten()[i]), float(lim.flatten()[i])

    def moving_case(self, B, S1, N, Lh, frame, P, K, pattern, extra=0, seed=0, gains=(0.5, 3.0)):
        ins = moving_inputs(seed, B, S1, N, Lh, frame, P, K, pattern, extra, gains)
        src, bank, bank_of, idx, gain, tgt = ins
        ev, pk, mx, tg = self.moving_call(*ins, frame)
        ref, amp = moving_ref(src, bank, bank_of, idx, gain, frame)
        what = f"B={B} S1={S1} N={N} Lh={Lh} frame={frame} P={P} K={K} {pattern}"
        res = {"events": self._events_vs_ref(ev, ref, amp, gain, Lh), "peak.value": (float(pk.max()), None)}
        mm, tt, nn = self._mix_of(ev, tgt)
        assert torch.equal(mm, mx), f"{what}: mixture is not the reference's mix of the device's events"
        assert torch.equal(tt, tg), f"{what}: target is not row tgt_idx of the device's events (normalised)"
        assert torch.equal(nn, pk), f"{what}: peak is not max |mixture| of the device's events"
        again = self.moving_call(*ins, frame)
        assert all(same_bits(a, b) for a, b in zip((ev, pk, mx, tg), again)), f"{what}: a second call differs"
        if B > 1:
            for b in range(B):
                alone = self.moving_call(src[b:b + 1], bank, bank_of[b:b + 1], idx[b:b + 1], gain[b:b + 1], tgt[b:b + 1], frame)
                assert all(same_bits(a[b:b + 1], x) for a, x in zip((ev, pk, mx, tg), alone)), f"{what}: utterance {b} alone differs"
        return res

    def const_case(self, B, S1, N, Lh, frame, P=3, K=2, seed=0):
        """A constant path against lh_render_binaural with that entry's response: equal bits outside the static FFT range."""
        src, bank, bank_of, idx, gain, tgt = moving_inputs(seed, B, S1, N, Lh, frame, P, K, "const", 1)
        rir = torch.stack([torch.stack([bank[int(bank_of[b]), int(idx[b, s, 0])] for s in range(S1)]) for b in range(B)])
        mov = self.moving_call(src, bank, bank_of, idx, gain, tgt, frame)
        sta = self.render_call(src, rir, gain, tgt)
        what = f"B={B} S1={S1} N={N} Lh={Lh} frame={frame} const"
        if Lh < 1024 or Lh > 4097:
            for nm, a, b in zip(("events", "peak", "mixture", "target"), mov, sta):
                assert same_bits(a, b), f"{what}: {nm} differs from lh_render_binaural"
            return {}
        ref, amp = moving_ref(src, bank, bank_of, idx, gain, frame)
        lim = static_bound(Lh) * amp * gain.double()
        d = (mov[0].double() - sta[0].double()).abs().amax((2, 3))
        i = int((d / lim).argmax())
        return {"events vs static (FFT)": (float(d.flatten()[i]), float(lim.flatten()[i])),
                "events vs float64": self._events_vs_ref(mov[0], ref, amp, gain, Lh)}

    def delay_case(self, delays=(3, 11, 0, 16, 7), sr=16000, frame=400):
        """Bank entry p: the left ear delayed by p samples, the right ear a unit impulse.  A white source rests on entry
        delays[c] for the whole of 250 ms segment c; the host's moving-mode metric reports ITD = p / sr seconds there."""
        from lookoncetohear_amd import metrics
        P = Lh = 17
        seg = sr // 4
        C = len(delays)
        N = C * seg
        bank = torch.zeros(1, P, 2, Lh)
        for p in range(P):
            bank[0, p, 0, p] = 1.0
            bank[0, p, 1, 0] = 1.0
        g = torch.Generator().manual_seed(11)
        src = 0.1 * torch.randn(1, 1, N, generator=g)
        F = n_points(N, frame)
        idx = torch.tensor([delays[min(f * frame // seg, C - 1)] for f in range(F)], dtype=I32).reshape(1, 1, F)
        ev = self.moving_call(src, bank, torch.zeros(1, dtype=I32), idx, torch.ones(1, 1), torch.zeros(1, dtype=I32), frame)[0]
        _, segs = metrics.binaural_errors(ev[:, 0], ev[:, 0], sr=sr, moving=True, return_segments=True)
        want = torch.tensor(delays, dtype=F64)[None]
        assert bool(segs["counted"].all())
        assert torch.equal(segs["tau_est"], want), (segs["tau_est"], want)
        assert torch.equal(segs["itd_est"], want / sr * 1e6), (segs["itd_est"], want / sr * 1e6)

    def blend_exact(self, frame, N):
        """The blend weight to the bit: entry 0 is silence, entry 1 a unit impulse, the source is 1 everywhere and the path
        alternates, so even frames give w and odd frames fmaf(w, -1, 1) = 1 - w rounded once, w the fp32 quotient."""
        bank = torch.zeros(1, 2, 2, 3)
        bank[0, 1, :, 0] = 1.0
        F = n_points(N, frame)
        idx = (torch.arange(F) % 2).to(I32).reshape(1, 1, F)
        ev = self.moving_call(torch.ones(1, 1, N), bank, torch.zeros(1, dtype=I32), idx, torch.ones(1, 1), torch.zeros(1, dtype=I32),
                              frame)[0]
        w = blend_weights(N, frame)
        odd = (np.arange(N) // frame) % 2 == 1
        want = torch.from_numpy(np.where(odd, (1.0 - w.astype(np.float64)).astype(np.float32), w))
        assert same_bits(ev[0, 0, 0], want) and same_bits(ev[0, 0, 1], want), f"frame={frame} N={N}: blend weights differ"

    def moving_refusals(self):
        """A null pointer, a dimension <= 0 or F one short: LH_ERR_ARG; frame of 4 and 12: LH_ERR_UNSUPPORTED; nothing is written."""
        B, S1, N, Lh, P, K, frame = 1, 2, 40, 4, 3, 2, 16
        F = n_points(N, frame)
        ins = [x.to(self.dev) for x in moving_inputs(0, B, S1, N, Lh, frame, P, K, "mixed")]
        outs = [self.g((B, S1, 2, N)), self.g((B,)), self.g((B, 2, N)), self.g((B, 2, N))]
        good = [x.data_ptr() for x in ins] + [x.t.data_ptr() for x in outs] + [B, S1, N, Lh, P, K, F, frame, self.st]
        fn = self.lib.raw("lh_render_moving")
        short = list(good)
        short[16] = F - 1
        assert fn(*short) == LH_ERR_ARG, "F one short accepted"
        for fr in (4, 12):
            a = list(good)
            a[17] = fr                                                       # (F is large enough for these frames too)
            a[12] = 8
            assert fn(*a) == LH_ERR_UNSUPPORTED, f"frame {fr}: not LH_ERR_UNSUPPORTED"
        self._refusals(fn, good, 10, 8, outs)

    # ---- lh_path_nearest
    def nearest_call(self, paths, positions, bank_of):
        B, S1, F, _ = paths.shape
        K, P, _ = positions.shape
        ins = [x.contiguous().to(self.dev) for x in (paths, positions, bank_of)]
        out = self.g((B, S1, F))                                             # int32 words behind a float32 view
        self.lib.call("lh_path_nearest", *[x.data_ptr() for x in ins], out.t.data_ptr(), B, S1, F, P, K, self.st)
        self.sync()
        out.check(f"lh_path_nearest B={B} S1={S1} F={F} P={P} K={K}")
        return out.t.view(I32).cpu().clone()

    def nearest_case(self, B, S1, F, P, K, seed=0, scale=1.5):
        g = torch.Generator().manual_seed(seed)
        unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, 3, generator=g, dtype=F64), dim=-1)
        positions = unit(K, P).float()
        paths = (scale * unit(B, S1, F)).float()
        paths[0, 0, F // 2] = 0.0                                            # a zero vector gives 0
        bank_of = ((K - 1 - torch.arange(B)) % K).to(I32)
        idx = self.nearest_call(paths, positions, bank_of)
        assert int(idx.min()) >= 0 and int(idx.max()) < P
        assert int(idx[0, 0, F // 2]) == 0, "zero vector"
        assert same_bits(idx, self.nearest_call(paths, positions, bank_of)), "a second call differs"
        n_amb = n_pts = 0
        worst = 0.0
        for b in range(B):
            p64 = positions[int(bank_of[b])].double()                        # [P][3]
            v64 = paths[b].double().reshape(-1, 3)                           # [S1 F][3]
            D = v64 @ p64.t()
            mag = v64.abs() @ p64.abs().t()
            dev = idx[b].reshape(-1).long()
            best = D.argmax(1)
            top = D.gather(1, best[:, None])[:, 0]
            D2 = D.clone()
            D2.scatter_(1, best[:, None], -math.inf)
            gap = top - D2.amax(1) if P > 1 else torch.full_like(top, math.inf)
            margin = 4 * 2.0 ** -24 * torch.maximum(mag.gather(1, best[:, None])[:, 0], mag.gather(1, dev[:, None])[:, 0])
            amb = gap < margin
            zero = v64.abs().amax(1) == 0
            assert torch.equal(dev[~amb & ~zero], best[~amb & ~zero]), f"B={B} S1={S1} F={F} P={P}: not the float64 argmax"
            short = top - D.gather(1, dev[:, None])[:, 0]
            assert bool((short[amb] <= margin[amb]).all()), "an ambiguous point's choice is outside the margin"
            n_amb += int((amb & ~zero).sum())
            n_pts += dev.numel()
            worst = max([worst] + (short / margin.clamp_min(1e-300))[~zero].tolist())
        return {"nearest.ambiguous share": (n_amb / n_pts, 0.01), "nearest.shortfall / margin": (worst, None)}

    def nearest_ties(self):
        """Exactly representable coordinates, duplicated positions: the lowest index wins, exactly."""
        positions = torch.tensor([[[0, 1, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 0, 1], [-1, 0, 0]]], dtype=F32)
        paths = torch.tensor([[1.5, 0, 0], [0, 1.5, 0], [0, 0, 1.5], [1, 1, 0], [1, 1, 1], [0.5, 1, 1], [-1.5, 0, 0], [0, 0, 0],
                              [0, -2, 0], [0, 0.25, 0.25]], dtype=F32).reshape(1, 1, -1, 3)
        idx = self.nearest_call(paths, positions, torch.zeros(1, dtype=I32))
        # (0, -2, 0): the dots are -2, 0 (or -0), -2, 0, 0, 0, 0: the first 0 is entry 1
        assert idx.flatten().tolist() == [1, 0, 4, 0, 0, 0, 6, 0, 1, 0], idx.flatten().tolist()

    def nearest_refusals(self):
        B, S1, F, P, K = 2, 2, 5, 4, 2
        g = torch.Generator().manual_seed(3)
        ins = [torch.randn(B, S1, F, 3, generator=g).to(self.dev), torch.randn(K, P, 3, generator=g).to(self.dev),
               torch.tensor([1, 0], dtype=I32).to(self.dev)]
        outs = [self.g((B, S1, F))]
        good = [x.data_ptr() for x in ins] + [outs[0].t.data_ptr(), B, S1, F, P, K, self.st]
        self._refusals(self.lib.raw("lh_path_nearest"), good, 4, 5, outs)

    # ---- nearest -> render_moving through the host class, on a synth.moving_scene clip
    def scene_case(self, scene_idx=2, n=8000, frame=400):
        from lookoncetohear_amd import synth
        sc = synth.moving_scene(scene_idx, n=n, frame=frame)
        to = lambda t: t.to(self.dev)
        srcs, bank, pos, paths, gains = (torch.from_numpy(sc[k])[None] for k in ("srcs", "bank", "positions", "paths", "gains"))
        tgt = torch.tensor([sc["tgt_idx"]], dtype=I32)
        bank_of = torch.zeros(1, dtype=I32)
        r = self.renderer
        idx = r.nearest(to(paths), to(pos), to(bank_of))
        mx, tg, pk, ev = (t.cpu() for t in r.render_moving(to(srcs), to(bank), to(bank_of), idx, to(gains), to(tgt), frame=frame))
        self.sync()
        idx = idx.cpu()
        assert bool((idx[..., 1:] != idx[..., :-1]).any(-1).sum() >= 2), "the scene's sources do not move"
        ref, amp = moving_ref(srcs, bank, bank_of, idx, gains, frame)
        assert int((amp > 0).sum()) >= 3, "the scene is silent"
        mm, tt, nn = self._mix_of(ev, tgt)
        assert torch.equal(mm, mx) and torch.equal(tt, tg) and torch.equal(nn, pk)
        return {"scene.events": self._events_vs_ref(ev, ref, amp, gains, bank.shape[3])}


# ---- case tables, shared by both back ends (every case takes well under a second on either)
# (B, S1, N, Lh, frame, P, K, pattern, extra path points).  k_fir_moving: 8 outputs per lane, a wave = one ear of one segment of
# at most MV_SEG = 512 outputs of ONE frame, a workgroup = two consecutive segments x two ears, MV_KT = 1024 taps per LDS stage,
# 8-tap chunks, two per loop trip; the vector store needs N % 4 == 0 and 8 outputs inside N
MOVING = [
    (1, 1, 1, 1, 8, 1, 1, "const", 0),                       # N = 1, P = 1
    (2, 3, 7, 1, 8, 2, 1, "alt", 0), (2, 3, 8, 7, 8, 3, 1, "alt", 0), (2, 3, 9, 8, 8, 3, 1, "distinct", 2),      # frame 8: -1, 0, +1
    (2, 2, 15, 9, 16, 4, 1, "distinct", 0), (1, 5, 16, 17, 16, 4, 2, "mixed", 0), (2, 2, 17, 9, 16, 4, 2, "alt", 1),
    (3, 5, 100, 17, 16, 5, 3, "mixed", 0),                   # ragged last frame, N % 8 == 4, K = 3 with a permuted bank_of
    (2, 3, 300, 72, 16, 19, 1, "distinct", 0),               # Lh > frame: the history spans frames that used other filters
    (1, 2, 50, 64, 16, 3, 1, "alt", 0),                      # Lh > N
    (2, 3, 2100, 9, 8, 264, 1, "distinct", 0),               # 263 frames, every path point another entry (P = F)
    (2, 3, 399, 9, 400, 3, 2, "alt", 0), (2, 3, 400, 17, 400, 3, 2, "alt", 3), (2, 3, 401, 8, 400, 3, 2, "distinct", 0),
    (2, 2, 1204, 16, 400, 4, 1, "mixed", 0),                 # N % 8 == 4: vector store and scalar tail in one wave; an idle wave pair
    (2, 3, 3000, 200, 400, 6, 2, "mixed", 0),                # equal and unequal neighbours side by side in one workgroup
    (2, 3, 300, 1000, 400, 3, 1, "alt", 0),                  # Lh > N, N < frame
    (1, 2, 2100, 1000, 400, 3, 1, "alt", 0), (1, 2, 2100, 1024, 400, 3, 1, "mixed", 0),      # direct where the static path turns to FFT
    (1, 2, 2500, 1025, 400, 3, 1, "alt", 0),                 # one tap in the second stage
    (1, 2, 2600, 2100, 400, 3, 1, "mixed", 0),               # three stages; workgroups skip to 1, 2 and 3 of them
    (1, 1, 4400, 4101, 400, 2, 1, "alt", 0),                 # five stages with a 5-tap tail
    (1, 2, 1700, 33, 520, 3, 1, "mixed", 0),                 # frame > MV_SEG: segments of 512 and 8 outputs
    (1, 2, 2100, 24, 1024, 3, 1, "alt", 0),                  # two full segments per frame
    (1, 3, 1100, 40, 1000, 2, 1, "alt", 0),                  # 512 + 488, the second frame cut by N
]
MOVING_LOUD = [(2, 3, 2052, 33, 400, 4, 2, "mixed", 0)]      # gains of about 20: a peak far above 1
# (B, S1, N, Lh, frame): N on both sides of a frame and of the static kernel's 2048-sample tile
CONST = [(2, 3, 399, 1, 400), (2, 3, 401, 17, 400), (2, 2, 2047, 17, 400), (2, 2, 2049, 200, 400), (1, 2, 2052, 200, 16),
         (1, 2, 2047, 1000, 400), (1, 2, 2049, 1000, 400), (1, 1, 2500, 4101, 400)]
CONST_FFT = [(1, 2, 2500, 2048, 400)]
# (B, S1, F, P, K)
NEAREST = [(1, 1, 1, 1, 1), (2, 2, 201, 63, 2), (2, 3, 201, 64, 1), (3, 2, 201, 65, 3), (2, 5, 201, 1250, 2), (1, 2, 1, 1250, 1),
           (1, 3, 300, 1025, 1)]
# (frame, N): every position of a frame, of two segments of one frame, and a ragged last frame
BLEND = [(8, 30), (16, 50), (200, 500), (400, 1204), (520, 1100), (1024, 2100)]
