"""Harness shared by tests/test_gpu_moving_fft.py (MI355X) and tests/test_emu_moving_fft.py (hipemu, CPU) for the moving-source
renderer's partitioned overlap-save path: lh_bank_spectra (k_bank_spectra) and lh_render_moving_fft (k_moving_fft, then
lh_render_binaural's k_mix_peak / k_mix_apply).  `MovingFftRig` extends tests/moving_render_cases.MovingRig: the entry points are
called directly, every output — events, peak, mixture, target, the spectra image and the scratch — lives in a `Guarded` buffer
of exactly the size include/lookonce_hip.h states, and every call asserts that the guards are unchanged.  The partitioning
(`partition`) is restated here from the header, not imported from the host code.

The definition is lh_render_moving's, so the reference and the bound are tests/moving_render_cases.py's: `moving_ref` (float64)
and `fir_bound(Lh)` = 4e-6 max(1, sqrt(Lh / 256)) + 2^-21 relative to amp gain — each chain gets the static renderer's bound,
whose range includes its own FFT path, plus the blend's three roundings.  A float32 model of exactly this scheme stays below
0.07 of that bound on these cases, so a miss is a bug, not a tolerance to widen.  Per case (`fft_case`):
  * each events row within fir_bound(Lh) amp gain of `moving_ref`;
  * peak, mixture and target `torch.equal` to `_mix_of` of the device's own events;
  * a second call gives equal bits, and so does utterance b rendered alone (B = 1, the whole bank);
  * against lh_render_moving on the same inputs: within 2 fir_bound(Lh) amp gain (both sit inside one bound of float64; a
    separate look at the frame index and the ear order).
`const_case`: a constant path against lh_render_binaural with that response, within static_bound(Lh) amp gain, where the static
renderer is direct and where it takes its own FFT path.
`resting_case`: a frame of a `mixed` path whose two path points name one entry e has the bits of the same frame in a run that
stays on e for the whole clip (the history of inputs is the row's own, so it is the same): the one-chain branch changes time,
not bits, and the frames around it that used other entries leave nothing behind.
"""
from __future__ import annotations

import math

import torch

from tests.data_stage_cases import LH_ERR_ARG, same_bits
from tests.moving_render_cases import I32, LH_ERR_UNSUPPORTED, MovingRig, fir_bound, moving_inputs, moving_ref, n_points, static_bound

FZ = 1024
LDS_RING = 16                                              # block spectra a workgroup keeps in LDS: no scratch up to here
LH_MAX = 16384
RUN_MIN = 25


def partition(Lh: int, frame: int):
    """(m, Lp, Q, RING, RUN) as include/lookonce_hip.h states them."""
    m = max(1, (FZ + 1 - frame) // frame)
    Lp = m * frame
    Q = -(-Lh // Lp)
    ring = (Q - 1) * m + 1
    return m, Lp, Q, ring, max(RUN_MIN, 2 * (ring - 1))


def work_floats(B: int, S1: int, N: int, Lh: int, frame: int) -> int:
    """fp32 elements of lh_render_moving_fft's scratch; 0: not needed."""
    _, _, _, ring, run = partition(Lh, frame)
    if ring <= LDS_RING:
        return 0
    runs = -(-(-(-N // frame)) // run)
    return B * S1 * runs * ring * FZ * 2


class MovingFftRig(MovingRig):
    # ---- lh_bank_spectra
    def spectra_call(self, bank, frame):
        """The image [K][P][Q][FZ][2] of a host bank, left on the device inside its guarded buffer."""
        K, P, _, Lh = bank.shape
        Q = partition(Lh, frame)[2]
        spec = self.g((K, P, Q, FZ, 2))
        bank = bank.contiguous().to(self.dev)
        self.lib.call("lh_bank_spectra", bank.data_ptr(), spec.t.data_ptr(), K, P, Lh, frame, self.st)
        self.sync()
        spec.check(f"lh_bank_spectra K={K} P={P} Lh={Lh} frame={frame}")
        return spec

    # ---- lh_render_moving_fft
    def fft_call(self, src, bank, bank_of, idx, gain, tgt, frame, spec=None):
        """One call on host tensors -> host tensors (events [B][S1][2][N], peak [B] fp32, mixture, target [B][2][N])."""
        B, S1, N = src.shape
        K, P, _, Lh = bank.shape
        F = idx.shape[2]
        spec = self.spectra_call(bank, frame) if spec is None else spec
        ins = [x.contiguous().to(self.dev) for x in (src, bank_of, idx, gain, tgt)]
        ev, pk, mx, tg = self.g((B, S1, 2, N)), self.g((B,)), self.g((B, 2, N)), self.g((B, 2, N))
        nw = work_floats(B, S1, N, Lh, frame)
        work = self.g((nw,)) if nw else None
        self.lib.call("lh_render_moving_fft", ins[0].data_ptr(), spec.t.data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(),
                      ins[3].data_ptr(), ins[4].data_ptr(), ev.t.data_ptr(), pk.t.data_ptr(), mx.t.data_ptr(), tg.t.data_ptr(),
                      work.t.data_ptr() if nw else None, B, S1, N, Lh, P, K, F, frame, self.st)
        self.sync()
        what = f"B={B} S1={S1} N={N} Lh={Lh} frame={frame} P={P} K={K} F={F}"
        for n, x in (("events", ev), ("peak", pk), ("mixture", mx), ("target", tg), ("spec", spec)) + ((("work", work),) if nw else ()):
            x.check(f"lh_render_moving_fft {n} {what}")
        return tuple(x.t.cpu().clone() for x in (ev, pk, mx, tg))

    def fft_case(self, B, S1, N, Lh, frame, P, K, pattern, extra=0, seed=0, gains=(0.5, 3.0)):
        ins = moving_inputs(seed, B, S1, N, Lh, frame, P, K, pattern, extra, gains)
        src, bank, bank_of, idx, gain, tgt = ins
        ev, pk, mx, tg = self.fft_call(*ins, frame)
        ref, amp = moving_ref(src, bank, bank_of, idx, gain, frame)
        what = f"fft B={B} S1={S1} N={N} Lh={Lh} frame={frame} P={P} K={K} {pattern}"
        res = {"events": self._events_vs_ref(ev, ref, amp, gain, Lh), "peak.value": (float(pk.max()), None)}
        mm, tt, nn = self._mix_of(ev, tgt)
        assert torch.equal(mm, mx), f"{what}: mixture is not the reference's mix of the device's events"
        assert torch.equal(tt, tg), f"{what}: target is not row tgt_idx of the device's events (normalised)"
        assert torch.equal(nn, pk), f"{what}: peak is not max |mixture| of the device's events"
        again = self.fft_call(*ins, frame)
        assert all(same_bits(a, b) for a, b in zip((ev, pk, mx, tg), again)), f"{what}: a second call differs"
        if B > 1:
            for b in range(B):
                alone = self.fft_call(src[b:b + 1], bank, bank_of[b:b + 1], idx[b:b + 1], gain[b:b + 1], tgt[b:b + 1], frame)
                assert all(same_bits(a[b:b + 1], x) for a, x in zip((ev, pk, mx, tg), alone)), f"{what}: utterance {b} alone differs"
        direct = self.moving_call(*ins, frame)[0]
        lim = 2 * fir_bound(Lh) * amp * gain.double()
        d = (ev.double() - direct.double()).abs().amax((2, 3))
        i = int((d / lim).argmax())
        res["events vs direct"] = (float(d.flatten()[i]), float(lim.flatten()[i]))
        return res

    def const_case(self, B, S1, N, Lh, frame, P=3, K=2, seed=0):
        """A constant path against lh_render_binaural with that entry's response: within the static bound of it and of float64."""
        src, bank, bank_of, idx, gain, tgt = moving_inputs(seed, B, S1, N, Lh, frame, P, K, "const", 1)
        rir = torch.stack([torch.stack([bank[int(bank_of[b]), int(idx[b, s, 0])] for s in range(S1)]) for b in range(B)])
        mov = self.fft_call(src, bank, bank_of, idx, gain, tgt, frame)
        sta = self.render_call(src, rir, gain, tgt)
        ref, amp = moving_ref(src, bank, bank_of, idx, gain, frame)
        lim = static_bound(Lh) * amp * gain.double()
        d = (mov[0].double() - sta[0].double()).abs().amax((2, 3))
        i = int((d / lim).argmax())
        return {"events vs static": (float(d.flatten()[i]), float(lim.flatten()[i])),
                "events vs float64": self._events_vs_ref(mov[0], ref, amp, gain, Lh)}

    def resting_case(self, B, S1, N, Lh, frame, P, K, seed=0):
        """Resting frames of a `mixed` path have the bits of the same frames of a run that never leaves their entry."""
        src, bank, bank_of, idx, gain, tgt = moving_inputs(seed, B, S1, N, Lh, frame, P, K, "mixed")
        spec = self.spectra_call(bank, frame)
        ev = self.fft_call(src, bank, bank_of, idx, gain, tgt, frame, spec)[0]
        nf = -(-N // frame)
        rest = idx[:, :, :nf] == idx[:, :, 1:nf + 1]                          # [B][S1][nf]
        assert bool(rest.any()) and not bool(rest.all()), "the path has no resting frame next to a moving one"
        n_checked = 0
        for e in range(P):
            on_e = rest & (idx[:, :, :nf] == e)
            if not bool(on_e.any()):
                continue
            ce = self.fft_call(src, bank, bank_of, torch.full_like(idx, e), gain, tgt, frame, spec)[0]
            for b, s, f in on_e.nonzero().tolist():
                lo, hi = f * frame, min((f + 1) * frame, N)
                assert same_bits(ev[b, s, :, lo:hi], ce[b, s, :, lo:hi]), f"Lh={Lh} frame={frame}: row {b},{s} frame {f} at rest on {e} differs"
                n_checked += 1
        return n_checked

    def silent_row(self, frame=400, Lh=900):
        """A silent source renders to exact zeros on both chains (no rounding noise out of the transforms)."""
        src, bank, bank_of, idx, gain, tgt = moving_inputs(9, 1, 3, 1000, Lh, frame, 3, 1, "alt")
        src[0, 1] = 0.0
        ev = self.fft_call(src, bank, bank_of, idx, gain, tgt, frame)[0]
        assert not bool(ev[0, 1].any()), "a silent row is not silent"
        assert bool(ev[0, 0].any()) and bool(ev[0, 2].any())

    def fft_refusals(self):
        """Null pointers (spec and a needed work among them), dimensions <= 0, F one short: LH_ERR_ARG; frame of 4, 12 and 520 and
        Lh past the limit: LH_ERR_UNSUPPORTED; nothing is written.  frame 16 with Lh 1100: RING = 64, so the scratch is needed."""
        B, S1, N, Lh, P, K, frame = 1, 2, 40, 1100, 3, 2, 16
        assert partition(Lh, frame)[3] > LDS_RING
        F = n_points(N, frame)
        src, bank, bank_of, idx, gain, tgt = moving_inputs(0, B, S1, N, Lh, frame, P, K, "mixed")
        spec = self.spectra_call(bank, frame)
        ins = [x.to(self.dev) for x in (src, bank_of, idx, gain, tgt)]
        outs = [self.g((B, S1, 2, N)), self.g((B,)), self.g((B, 2, N)), self.g((B, 2, N))]
        work = self.g((work_floats(B, S1, N, Lh, frame),))
        good = ([ins[0].data_ptr(), spec.t.data_ptr()] + [x.data_ptr() for x in ins[1:]] + [x.t.data_ptr() for x in outs] +
                [work.t.data_ptr(), B, S1, N, Lh, P, K, F, frame, self.st])
        fn = self.lib.raw("lh_render_moving_fft")
        short = list(good)
        short[17] = F - 1
        assert fn(*short) == LH_ERR_ARG, "F one short accepted"
        for fr in (4, 12, 520):
            a = list(good)
            a[18] = fr
            a[13] = 8                                                        # N: F is large enough for these frames too
            assert fn(*a) == LH_ERR_UNSUPPORTED, f"frame {fr}: not LH_ERR_UNSUPPORTED"
        a = list(good)
        a[14] = LH_MAX + 1
        assert fn(*a) == LH_ERR_UNSUPPORTED, "Lh one past the limit accepted"
        self._refusals(fn, good, 11, 8, outs)
        spec.check("refusals: spec")
        work.check("refusals: work")
        # lh_bank_spectra
        img = self.g((K, P, partition(Lh, frame)[2], FZ, 2))
        bk = bank.to(self.dev)
        fs = self.lib.raw("lh_bank_spectra")
        good = [bk.data_ptr(), img.t.data_ptr(), K, P, Lh, frame, self.st]
        for fr in (4, 12, 520):
            assert fs(*(good[:5] + [fr, self.st])) == LH_ERR_UNSUPPORTED, f"lh_bank_spectra frame {fr}"
        assert fs(*(good[:4] + [LH_MAX + 1, frame, self.st])) == LH_ERR_UNSUPPORTED, "lh_bank_spectra Lh one past the limit"
        self._refusals(fs, good, 2, 4, [img])
        assert same_bits(img.t, spec.t), "lh_bank_spectra: a second image differs"

    # ---- nearest -> render_moving(method="fft") through the host class, on a synth.moving_scene clip
    def scene_fft_case(self, scene_idx=2, n=8000, lh=1100, frame=400):
        from lookoncetohear_amd import synth
        sc = synth.moving_scene(scene_idx, n=n, lh=lh, frame=frame)
        to = lambda t: t.to(self.dev)
        srcs, bank, pos, paths, gains = (torch.from_numpy(sc[k])[None] for k in ("srcs", "bank", "positions", "paths", "gains"))
        tgt = torch.tensor([sc["tgt_idx"]], dtype=I32)
        bank_of = torch.zeros(1, dtype=I32)
        r = self.renderer
        idx = r.nearest(to(paths), to(pos), to(bank_of))
        args = (to(srcs), to(bank), to(bank_of), idx, to(gains), to(tgt))
        mx, tg, pk, ev = (t.cpu() for t in r.render_moving(*args, frame=frame, method="fft"))
        cached = r.render_moving(*args, frame=frame, method="fft", spectra=r.bank_spectra(to(bank), frame))
        self.sync()
        assert all(same_bits(a, b.cpu()) for a, b in zip((mx, tg, pk, ev), cached)), "a precomputed image changes the bits"
        idx = idx.cpu()
        assert bool((idx[..., 1:] != idx[..., :-1]).any(-1).sum() >= 2), "the scene's sources do not move"
        ref, amp = moving_ref(srcs, bank, bank_of, idx, gains, frame)
        assert int((amp > 0).sum()) >= 3, "the scene is silent"
        mm, tt, nn = self._mix_of(ev, tgt)
        assert torch.equal(mm, mx) and torch.equal(tt, tg) and torch.equal(nn, pk)
        return {"scene.events": self._events_vs_ref(ev, ref, amp, gains, bank.shape[3])}


# ---- case tables, shared by both back ends.  (B, S1, N, Lh, frame, P, K, pattern, extra path points)
# frame 400: m = 1, Lp = 400; frame 200: m = 4, Lp = 800; frame 104: m = 8, Lp = 832; frame 512: m = 1; frame 8: m = 127, Lp = 1016;
# frame 16: m = 63, Lp = 1008.  The block spectra live in LDS up to RING = 16 and in the scratch beyond.
_R1025 = partition(1025, 400)                              # Q = 3, RING = 3, RUN = 25
FFT_MOVING = [
    (1, 1, 1, 1, 8, 1, 1, "const", 0),                       # N = 1, P = 1
    (2, 3, 399, 9, 400, 3, 2, "alt", 0), (2, 3, 400, 17, 400, 3, 2, "alt", 3), (2, 3, 401, 8, 400, 3, 2, "distinct", 0),
    (1, 2, 900, 400, 400, 3, 1, "alt", 0),                   # exactly one full partition
    (1, 2, 900, 401, 400, 3, 1, "alt", 0),                   # one tap in the second partition
    (1, 2, 900, 700, 400, 3, 1, "alt", 1),                   # a partial second partition
    (1, 2, 2500, 1025, 400, 3, 1, "alt", 0),
    (1, 2, 2600, 2100, 400, 3, 1, "mixed", 0),               # six partitions; resting and moving frames side by side
    (1, 1, 4400, 4101, 400, 2, 1, "alt", 0),                 # eleven partitions
    (1, 1, 4400, 4001, 400, 2, 1, "alt", 0),                 # a one-tap last partition
    (1, 1, 6000, 8192, 400, 2, 1, "alt", 0),                 # beyond the static FFT range; RING = 21: the ring in the scratch
    (1, 1, 801, LH_MAX, 400, 2, 1, "alt", 0),                # the length limit, N = 2 frame + 1
    (2, 3, 1300, 2048, 200, 5, 2, "distinct", 0),            # m = 4: a partition delay of several blocks
    (1, 2, 1704, 1000, 104, 6, 1, "mixed", 0),               # m = 8, frame not a divisor of anything convenient
    (1, 2, 1500, 1024, 512, 3, 1, "alt", 0),                 # the largest frame, 2 frame - 1 = FZ - 1
    (2, 2, 300, 64, 8, 4, 1, "distinct", 0),                 # the smallest frame, m = 127
    (1, 1, 200, 1017, 8, 2, 1, "alt", 0),                    # frame 8, one tap in the second partition (RING = 128: scratch)
    (1, 2, 50, 64, 16, 3, 1, "alt", 0),                      # Lh > N
    (2, 3, 300, 1000, 400, 3, 1, "alt", 0),                  # Lh > N, N < frame
    (3, 5, 900, 500, 400, 5, 3, "mixed", 0),                 # K = 3 with the permuted bank_of, S1 = 5, the noise row as target
    (2, 3, 2100, 9, 8, 264, 1, "distinct", 0),               # 263 frames, every path point another entry
    # two workgroup time runs: the blocks in front of the second run are real input, not zeros
    (1, 1, 400 * (_R1025[4] + _R1025[2] * _R1025[0]) + 4, 1025, 400, 3, 1, "alt", 0),
    (1, 1, 16 * 130 + 4, 1100, 16, 3, 1, "mixed", 0),        # the same with the ring in the scratch: RING = 64, RUN = 126
]
FFT_LOUD = [(2, 3, 2052, 1100, 400, 4, 2, "mixed", 0)]       # MOVING_LOUD's gains of 15 to 25: a peak far above 1
# (B, S1, N, Lh, frame): the static renderer direct (Lh < 1024, Lh > 4097) and on its own FFT path
FFT_CONST = [(2, 2, 1300, 700, 400), (1, 2, 2500, 2048, 400), (1, 1, 4400, 4101, 400), (1, 2, 1300, 1030, 200)]
# (B, S1, N, Lh, frame, P, K)
FFT_RESTING = [(1, 2, 2600, 2100, 400, 3, 1), (1, 2, 1704, 1000, 104, 3, 1), (1, 1, 700, 1100, 16, 3, 1)]
