"""Cases shared by tests/test_emu_taps.py (hipemu, CPU) and tests/test_gpu_taps.py (MI355X): the last block's closing stage
emitting the deconv tap products and the back end that starts from them (`lh_proj_ln_res_taps` -> `lh_taps_istft`, ABI 26)
against the pair they replace from the zero state (`lh_proj_ln_res` without gain -> `lh_deconv_istft` on zero state buffers).

The contract is BITS: every power-of-two scale is taken over the same elements, every accumulator chain and sum keeps its
order, so `torch.equal` on the waveforms — for random data, for frames whose rows are 2^+-20 apart, for rows far below their
scale group's maximum, for an all-zero frame, and when the frame's last four channels (which the back end's clamped staging
loads put into seven of its eight scale groups) are the largest values of the frame.  `Rig` is tests/stage_cases.py's."""
from __future__ import annotations

import torch

from oracle import tfgridnet_oracle as O
from tests.stage_cases import C, F, NH, PRE, VD, VF, rel_err

NP = 36                                                    # tap columns (kt, kf, o) per (frame, bin)
# (B, T, lh_set_tuning key 6): one and two frames; the 15-frame tile edges; three utterances on one run each (a 3-frame halo never
# occurs, a persistent workgroup of the emulator / a small grid crosses utterances) and on three runs each (run starts at
# frames 15 and 30 take the 3-frame halo)
SHAPES = [(1, 1, 0), (1, 2, 0), (1, 15, 0), (1, 16, 0), (2, 31, 0), (3, 46, 1), (3, 46, 3)]


def _flag(rig):
    return torch.zeros(2, dtype=torch.int32, device=rig.dev)


def _proj_args(rig, mg, y2, ln=None):
    bp = rig.bp
    lw, lb = (bp["proj_ln_w"], bp["proj_ln_b"]) if ln is None else ln
    return [mg, bp["proj_w"], bp["proj_b"], bp["proj_slope"], lw, lb, y2]


def old_pair(rig, mg, y2, runs=0, keep=1, ln=None):
    """lh_proj_ln_res (no gain) -> lh_deconv_istft on zero state buffers: (wave, flag word, frame Y)."""
    B, T = y2.shape[:2]
    y = rig.g((B, T, F, C))
    rig.call("lh_proj_ln_res", *_proj_args(rig, mg, y2, ln), None, y.t, B, T, rig.st)
    db, ib = torch.zeros(B, C, 2, F, device=rig.dev), torch.zeros(B, 2, 2 * F, 1, device=rig.dev)
    dbo, ibo, wave, flag = rig.g((B, C, 2, F)), rig.g((B, 2, 2 * F, 1)), rig.g((B, 2, 128 * T)), _flag(rig)
    with rig.tuning(6, runs):
        rig.call("lh_deconv_istft", y.t, db, dbo.t, ib, ibo.t, rig.pk["deconv_w"], rig.pk["deconv_b"], rig.pk["wfb_dec"], wave.t,
                 flag, keep, B, T, rig.st)
    rig.sync()
    for n, t in (("y", y), ("deconv_buf_out", dbo), ("istft_buf_out", ibo), ("wave", wave)):
        t.check("old pair " + n)
    return wave.t, int(flag[0]), y.t


def new_pair(rig, mg, y2, runs=0, keep=1, ln=None, wins=None):
    """lh_proj_ln_res_taps (whole clip, or one `_win` call per (t0, Tc) of `wins`) -> lh_taps_istft: (wave, flag word, P, fmax)."""
    B, T = y2.shape[:2]
    p, fm = rig.g((B, T, F, NP)).fill_pattern(), rig.g((B, T)).fill_pattern()
    args = _proj_args(rig, mg, y2, ln) + [rig.pk["deconv_w"], p.t, fm.t, B, T]
    if wins is None:
        rig.call("lh_proj_ln_res_taps", *args, rig.st)
    else:
        for t0, Tc in wins:                                # each call leaves the frames outside its window alone
            p0, f0 = p.t.clone(), fm.t.clone()
            rig.call("lh_proj_ln_res_taps_win", *args, t0, Tc, rig.st)
            rig.sync()
            p.frames_untouched(p0, 1, t0, Tc, "taps_win P")
            fm.frames_untouched(f0, 1, t0, Tc, "taps_win fmax")
    wave, flag = rig.g((B, 2, 128 * T)), _flag(rig)
    with rig.tuning(6, runs):
        rig.call("lh_taps_istft", p.t, fm.t, rig.pk["deconv_w"], rig.pk["deconv_b"], rig.pk["wfb_dec"], wave.t, flag, keep, B, T,
                 rig.st)
    rig.sync()
    for n, t in (("P", p), ("fmax", fm), ("wave", wave)):
        t.check("new pair " + n)
    return wave.t, int(flag[0]), p.t, fm.t


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def inputs(rig, B, T, scales=None):
    return rig.randn(B, T, NH, F, VD), rig.randn(B, T, F, C, scales=scales)


def pair_bits(rig, B, T, runs, wins=None):
    mg, y2 = inputs(rig, B, T)
    w0, f0, y = old_pair(rig, mg, y2, runs)
    w1, f1, _, fm = new_pair(rig, mg, y2, runs, wins=wins)
    assert same_bits(w1, w0), f"B={B} T={T} runs={runs} wins={wins}: {int((w1 != w0).sum())} samples differ, max {float((w1 - w0).abs().max()):.3e}"
    assert f0 == 0 and f1 == 0
    assert torch.equal(fm, y.abs().amax((2, 3))), "fmax is max |Y| of the frame"


def _zero_ln(rig):
    z = torch.zeros(F * C, device=rig.dev)
    return z, z.clone()


def range_bits(rig):
    """Frames under the stage's own LayerNorm affine whose residual rows are 2^+-20 apart, and — with a ZERO affine, which makes
    the frame exactly y2 — rows 2^+-20 apart, rows at 1e-6 of their scale group's maximum, an all-zero frame, and frames whose
    last four channels of bin 96 carry the frame maximum (see the module text).  B = 2, T = 17: two tiles, one run each."""
    B, T = 2, 17
    mg, y2 = inputs(rig, B, T)
    e = torch.randint(-20, 21, (B, T, F, 1), generator=rig.gen).float().to(rig.dev)
    cases = {"ln affine, rows 2^+-20": (y2 * torch.exp2(e), None)}
    z = y2 * torch.exp2(e)
    z[0, 3] = 0.0                                          # an all-zero frame
    z[1, 5, :, :] *= 1e-6                                  # group g = rows with (r & 31) >> 2 == g: one row of each at full scale
    z[1, 5, 0::4] *= 1e6
    z[0, 7] = y2[0, 7] * 1e-6                              # the clamped float4 (bin 96, channels 60..63) above everything else
    z[0, 7, 96, 60:] = torch.tensor([3.0e4, -2.0, 1.0, 0.5], device=rig.dev)
    z[1, 9] = y2[1, 9]
    z[1, 9, 96, 60:] *= 2.0 ** 18
    cases["zero affine, controlled frames"] = (z, _zero_ln(rig))
    for name, (yy, ln) in cases.items():
        w0, f0, y = old_pair(rig, mg, yy, 0, ln=ln)
        w1, f1, _, fm = new_pair(rig, mg, yy, 0, ln=ln)
        if ln is not None:
            assert torch.equal(y, yy), "zero affine: the frame is the residual"
        assert same_bits(w1, w0), f"{name}: {int((w1 != w0).sum())} samples differ, max {float((w1 - w0).abs().max()):.3e}"
        assert f0 == 0 and f1 == 0 and torch.equal(fm, y.abs().amax((2, 3))), name


def against_float64(rig, B, T, scales, runs=0):
    """P against Y . Wd and the waveform against the back end, both in float64 from the projection's own float64 output."""
    mg, y2 = inputs(rig, B, T, scales)
    wave, _, p, _ = new_pair(rig, mg, y2, runs)
    Ob = mg.double().permute(0, 2, 1, 3, 4).reshape(B * NH, T, VF)
    Y = O.concat_proj_ln_res(rig.cfg, rig.p, PRE, Ob, y2.double())
    Wd = rig.p["deconv.weight"].permute(0, 2, 3, 1).reshape(C, NP)          # [c][(kt, kf, o)]
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=rig.dev)
    wr, _, _ = O.back_end(rig.cfg, rig.p, Y, z(B, C, 2, F), z(B, 2, 2 * F, 1))
    return {"proj_ln_res_taps.P": rel_err(p, Y @ Wd, B), f"deconv_istft.taps.k6={runs}": rel_err(wave, wr[..., :-64], B)}


def nonfinite(rig):
    """One inf in `merged`: both pairs raise the flag and agree on which samples are non-finite, kept (1) or stored as 0 (0)."""
    B, T = 2, 17
    mg, y2 = inputs(rig, B, T)
    mg[1, 4, 2, 40, 7] = float("inf")
    out = {}
    for keep in (1, 0):
        w0, f0, _ = old_pair(rig, mg, y2, 0, keep)
        w1, f1, _, _ = new_pair(rig, mg, y2, 0, keep)
        assert f0 == 1 and f1 == 1, (keep, f0, f1)
        out[keep] = (w0, w1)
    (k0, k1), (s0, s1) = out[1], out[0]
    bad = ~torch.isfinite(k0)
    assert bool(bad.any()) and not bool(bad[0].any()), "utterance 1 only"
    assert torch.equal(~torch.isfinite(k1), bad)
    assert same_bits(k1[~bad], k0[~bad])
    assert bool(torch.isfinite(s0).all()) and bool(torch.isfinite(s1).all())
    assert bool((s0[bad] == 0).all()) and bool((s1[bad] == 0).all()) and same_bits(s1, s0)


def arg_errors(rig):
    """Null pointers, B <= 0, T <= 0 and a window outside the clip: LH_ERR_ARG (1), nothing launched."""
    B, T = 1, 4
    mg, y2 = inputs(rig, B, T)
    p, fm, wave = rig.g((B, T, F, NP)).fill_pattern(), rig.g((B, T)).fill_pattern(), rig.g((B, 2, 128 * T)).fill_pattern()
    snap = [t.t.clone() for t in (p, fm, wave)]
    ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a
    good = _proj_args(rig, mg, y2) + [rig.pk["deconv_w"], p.t, fm.t]
    raw = rig.lib.raw
    for i in range(len(good)):
        a = [ptr(x) for x in good]
        a[i] = None
        assert raw("lh_proj_ln_res_taps")(*a, B, T, rig.st) == 1, i
        assert raw("lh_proj_ln_res_taps_win")(*a, B, T, 0, T, rig.st) == 1, i
    a = [ptr(x) for x in good]
    for b, t in ((0, T), (-1, T), (B, 0), (B, -3)):
        assert raw("lh_proj_ln_res_taps")(*a, b, t, rig.st) == 1
    for t0, Tc in ((-1, 2), (0, 0), (0, T + 1), (T, 1), (2, T - 1)):
        assert raw("lh_proj_ln_res_taps_win")(*a, B, T, t0, Tc, rig.st) == 1, (t0, Tc)
    back = [p.t, fm.t, rig.pk["deconv_w"], rig.pk["deconv_b"], rig.pk["wfb_dec"], wave.t]
    for i in range(len(back)):
        a = [ptr(x) for x in back]
        a[i] = None
        assert raw("lh_taps_istft")(*a, None, 1, B, T, rig.st) == 1, i
    a = [ptr(x) for x in back]
    for b, t in ((0, T), (-1, T), (B, 0), (B, -3)):
        assert raw("lh_taps_istft")(*a, None, 1, b, t, rig.st) == 1
    rig.sync()
    for t, s in zip((p, fm, wave), snap):
        assert same_bits(t.t, s)
    assert raw("lh_taps_istft")(*a, None, 1, B, T, rig.st) == 0          # the flag word itself may be NULL
    rig.sync()


NEW_ENTRY_POINTS = {"lh_proj_ln_res_taps", "lh_proj_ln_res_taps_win", "lh_taps_istft"}
