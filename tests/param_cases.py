"""Cases shared by tests/test_emu_param_stages.py (hipemu, CPU) and tests/test_gpu_param_stages.py (MI355X): the stage kernels
under PARAMETERS the synthetic state dict never takes.  Every other stage test sweeps shapes, windows and activation scale on
one parameter set (weights U(+-1/sqrt(fan_in)), PReLU slopes in [0.15, 0.35], norm weights in [0.75, 1.25], gate biases in
+-1/8); here the shapes are the smallest (B = 2, T = 3; T = 1 for the ring forms) and the parameters move:

  A  PReLU slopes above 1, exactly 1, exactly 0 and below 0 in the Q/K/V and the projection frame kernels (the compare + select
     epilogue of k_qkv_proj_ln / k_proj_ln_res runs only for a slope above 1), through every entry point built on the two
     kernel bodies, at the existing bounds of stage_cases.TOL;
  B  a layer's weight and bias multiplied together by 2^-3, 2^-6, 2^-9.  The bound of a case is
     max(existing bound, 4 x the fp32 yardstick), the yardstick being the same oracle function evaluated in torch float32 on
     the same inputs and parameters (the `yard` argument of the rigs).  Where a LayerNorm follows the Linear the float64 result
     and the yardstick do not depend on the scale, so these cases hold the kernels to scale invariance;
  C  the recurrences under LayerNorm weights of 2^-6, gate biases U(+-6), and gate biases of +-80 (beyond the +-100 clamp of the
     fused kernels' 2^b bias factors once the -log2e / -2 log2e prescale is applied), at the existing bounds.

A case builds a `Net` / `EmbedTFGridNet` from an edited copy of the synthetic state dict (`rig_with`) and a `stage_cases.Rig` /
`embed_stage_cases.EmbedRig` on it: the packed images come from `net._weights`, the float64 parameters from the same dict."""
from __future__ import annotations

import math

import torch

from lookoncetohear_amd.weights import KV_PAD_ROWS, unsplit_qk, unsplit_v
from oracle import embedder_oracle as E
from oracle import tfgridnet_oracle as O
from tests import taps_cases as TC
from tests.embed_stage_cases import ETOL, EmbedRig
from tests.forward_many_cases import proj_ln_res_fan
from tests.stage_cases import C, F, H, NH, PRE, TOL, Rig, bound, check, rel_err

SD = "tfgridnet." + PRE                                    # block 0 of the separator's state dict
ACT = [1e-6, 1e3]                                          # per-utterance activation scales of the slope cases (B = 2)
# A: (Q, K, V slopes, projection slope) of the edited net
SLOPES = [((1.5, 0.25, 0.25), 1.5), ((0.25, 0.25, 1.5), 1.0), ((1.0, 1.0, 1.0), 0.0), ((0.0, -0.5, 0.25), -0.5)]
UNIT = [1.0, 1.0]                                          # ... of the weight-scale cases
LOG2S = [-3, -6, -9]                                       # B: weight and bias times 2^k


class Maker:
    """What a runner supplies: the library, device, stream and sync of its rigs, the two host classes, the separator's
    synthetic state dict."""

    def __init__(self, lib, dev, stream, sync, net_cls, emb_cls, sd):
        self.lib, self.dev, self.stream, self.sync, self.net_cls, self.emb_cls, self.sd = lib, dev, stream, sync, net_cls, emb_cls, sd


def rig_with(mk: Maker, edit, embed=False):
    """A rig on a net whose state dict is the synthetic one after `edit(sd)` (which changes it in place)."""
    if embed:
        sd, cls, kw, rig = E.synthetic_state_dict(E.ECfg(**E.EMBED_PARAMS), 0), mk.emb_cls, E.EMBED_PARAMS, EmbedRig
    else:
        sd, cls, kw, rig = {k: v.clone() for k, v in mk.sd.items()}, mk.net_cls, O.TSH_PARAMS, Rig
    edit(sd)
    net = cls(**kw).eval()
    net.load_state_dict(sd, strict=True)
    return rig(mk.lib, net.to(mk.dev), mk.dev, mk.stream, mk.sync)


def scale_layers(names, s):
    """An edit: weight and bias of every layer in `names` times s."""
    def edit(sd):
        for n in names:
            sd[n + ".weight"] *= s
            sd[n + ".bias"] *= s
    return edit


# ---- A. slopes -------------------------------------------------------------------------------------------------------------
def qkv_rows(rig, B):
    """`lh_qkv_proj_ln_rows` (one frame per row, each row its own ring slot) against float64: Q, and the K / V rows at
    write_pos[b]; every other ring row stays zero."""
    y = rig.randn(B, 1, F, C, scales=ACT[:B])
    q, kx, vx = rig._kv_bufs(B, 1, rows=50 + KV_PAD_ROWS)
    wp = torch.tensor([(49 + 7 * b) % 50 for b in range(B)], dtype=torch.int32, device=rig.dev)
    bp = rig.bp
    rig.call("lh_qkv_proj_ln_rows", y, bp["qkv_w"], bp["qkv_b"], bp["qkv_slopes"], bp["lnq_w"], bp["lnq_b"], bp["lnk_w"], bp["lnk_b"],
             bp["lnv_w"], bp["lnv_b"], q.t, kx.t, vx.t, wp, B, rig.st)
    rig.sync()
    for n, t in (("q", q), ("kx", kx), ("vx", vx)):
        t.check("qkv_rows " + n)
    Qr, Kr, Vr = O.qkv_proj_ln(rig.cfg, rig.p, PRE, y.double())
    slot = wp.long().repeat_interleave(NH)
    row = torch.arange(B * NH, device=rig.dev)
    krow, vrow = kx.t[row, slot].clone(), vx.t[row, slot].clone()
    kx.t[row, slot], vx.t[row, slot] = 0, 0
    assert not bool(kx.t.any()) and not bool(vx.t.any()), "qkv_rows: a ring row other than write_pos[b] written"
    return {"qkv_proj_ln_rows.Q": rel_err(unsplit_qk(q.t), Qr, B), "qkv_proj_ln_rows.K": rel_err(unsplit_qk(krow), Kr, B),
            "qkv_proj_ln_rows.V": rel_err(unsplit_v(vrow), Vr, B)}


def slope_case(mk, qkv, proj):
    def edit(sd):
        for nm, a in zip("QKV", qkv):
            sd[SD + f"attn_conv_{nm}.1.weight"].fill_(a)
        sd[SD + "attn_concat_proj.1.weight"].fill_(proj)
    rig = rig_with(mk, edit)
    case = f"qkv {qkv} proj {proj}"
    B, T, win = 2, 3, (1, 2)
    check(rig.qkv_ring(B, T, ACT), case)
    check(rig.qkv_attn_win(B, T, *win), case)
    check(rig.stream_ring(B, 3), case)
    check(qkv_rows(rig, B), case)
    for gain in (True, False):
        check(rig.proj_ln_res(B, T, ACT, gain), case)
    check(rig.proj_ln_res(B, T, ACT, True, win=win), case)
    check(proj_ln_res_fan(rig, B, T, 2, ACT), case)
    check(TC.against_float64(rig, B, T, ACT), case)
    TC.pair_bits(rig, B, T, 0)
    TC.pair_bits(rig, B, T, 0, wins=((0, 1), (1, 2)))


# ---- B. weight scale ---------------------------------------------------------------------------------------------------------
def linear_res(rig, yard):
    """`lh_linear_res` of the intra and the inter projection on a ZERO residual, so that the branch alone is measured."""
    B, T, out = 2, 3, {}
    for nm, K in (("intra", 2 * H), ("inter", H)):
        h = rig.randn(B, T * F, K) * 0.5
        x = torch.zeros(B, T * F, C, device=rig.dev)
        y = rig.g((B, T * F, C))
        rig.call("lh_linear_res", h, rig.bp[nm + "_lin_w"], rig.bp[nm + "_lin_b"], x, y.t, B * T * F, K, rig.st)
        rig.sync()
        y.check(nm + " linear_res")
        w, b = PRE + nm + "_linear.weight", PRE + nm + "_linear.bias"
        ref = h.double() @ rig.p[w].t() + rig.p[b]
        out[f"linear_res.{nm}"] = rel_err(y.t, ref, B)
        yard[f"linear_res.{nm}"] = rel_err(h @ rig.p32[w].t() + rig.p32[b], ref, B)
    return out


def _embed_names():
    heads = [f"blocks.0.attn_conv_{nm}_{h}.0" for nm in "QKV" for h in range(4)]
    return heads + ["blocks.0.attn_concat_proj.0", "embed_proj.0"]


def _embed_run(rig, yard):
    res = rig.attn_block(1, 5, 1, yard=yard)
    res.update(rig.head(3, 1, yard=yard))
    return res


def _proj_run(rig, yard):
    res = rig.proj_ln_res(2, 3, UNIT, False, yard=yard)
    res.update(rig.proj_ln_res(2, 3, UNIT, True, yard=yard))
    return res


# layer -> (the layers whose weight and bias are scaled, embedder?, the run: (rig, yard) -> results, the table of bounds)
LAYERS = {
    "qkv": ([SD + f"attn_conv_{nm}.0" for nm in "QKV"], False, lambda r, y: r.qkv_ring(2, 3, UNIT, yard=y), TOL),
    "k_alone": ([SD + "attn_conv_K.0"], False, lambda r, y: r.qkv_ring(2, 3, UNIT, yard=y), TOL),
    "proj": ([SD + "attn_concat_proj.0"], False, _proj_run, TOL),
    "embedder": (_embed_names(), True, _embed_run, ETOL),
    "deconv": (["tfgridnet.deconv"], False, lambda r, y: r.deconv_istft(2, 3, UNIT, 0, yard=y), TOL),
    "conv": (["tfgridnet.conv.0"], False, lambda r, y: r.stft_conv_in(2, 3, UNIT, yard=y), TOL),
    "linear": ([SD + "intra_linear", SD + "inter_linear"], False, linear_res, TOL),
}
# Measured on the MI355X (profiles/weight_scale.json: worst of the three scales | the fp32 yardstick there | the bound that holds).
# A LayerNorm follows the first four, so the packers scale each LayerNorm group by a power of two (weights.ln_group) and the
# error is flat in the scale; before that the emulator gave 2.3e-6 / 2.0e-5 / 1.5e-4 for qkv at 2^-3 / 2^-6 / 2^-9.
#   qkv        .Q 4.79e-7  .K 3.19e-7  .V 4.16e-7                                         | 2.8e-7 .. 3.8e-7 | 1.5e-6
#   k_alone    .K 3.19e-7 (Q and V as at scale 1: 3.75e-7, 4.17e-7)                       | 3.8e-7           | 1.5e-6
#   proj       2.77e-7, with gain 2.48e-7                                                 | 3.2e-7           | 2e-6
#   embedder   q 3.32e-7  k 3.47e-7  v 3.43e-7  sc 1.24e-6  p 3.88e-7  merged 4.10e-7
#              out 4.37e-7  xsplit 5.12e-7  head 9.25e-7                                  | 1e-7 .. 9.5e-7   | ETOL
# No norm follows the last three and their images keep the un-rescaled split's absolute floor of 2^-25 per weight: the error
# relative to the layer's own output grows as 1 / scale while the yardstick stays flat.  OPEN lists the results that are outside
# max(bound, 4 x yardstick): measured, printed and recorded, not asserted (DESIGN.md section 3 states the floor); every other
# result of these layers is asserted at every scale.        2^-3      2^-6      2^-9   | yardstick | bound
#   conv     stft_conv_in                                  1.69e-6   1.25e-5   1.12e-4 | 3.0e-7    | 1.5e-6
#   deconv   deconv_istft.k6=0.istft_buf                   7.31e-6   5.14e-5   3.97e-4 | 2.7e-7    | 4e-6
#            (the waveform itself stays inside its 1e-5: 2.97e-6, 2.76e-6, 3.16e-6)
#   linear   linear_res.intra                              2.75e-6   2.15e-5   1.80e-4 | 3.5e-7    | 1.40e-6
#            linear_res.inter                              1.92e-6   1.36e-5   1.21e-4 | 3.3e-7    | 1.31e-6
NORMALISED = ("qkv", "k_alone", "proj", "embedder")        # a LayerNorm follows: the yardstick is flat in the scale
OPEN = {(layer, k, name) for layer, name in (("conv", "stft_conv_in"), ("deconv", "deconv_istft.k6=0.istft_buf"),
                                             ("linear", "linear_res.intra"), ("linear", "linear_res.inter")) for k in LOG2S}
assert not any(layer in NORMALISED for layer, _, _ in OPEN)

CURVE = []                                                 # one record per (layer, scale, result) measured in this process


def weight_scale_case(mk, layer, k, open_items=OPEN):
    """Measure `layer` at scale 2^k, print hip error, yardstick and bound per result, record them in CURVE, assert the bounds.
    A result whose (layer, k, name) is in `open_items` is measured, printed and recorded, and not asserted."""
    names, embed, run, table = LAYERS[layer]
    rig = rig_with(mk, scale_layers(names, 2.0 ** k), embed)
    yard = {}
    res = run(rig, yard)
    bad = []
    for name, v in res.items():
        y = yard.get(name)
        b = max(bound(name, table), 4.0 * y) if y is not None else bound(name, table)
        is_open = (layer, k, name) in open_items
        ys = f"{y:.3e}" if y is not None else "    -    "
        print(f"{layer:>10} 2^{k:<3} {name:<32} hip {v:.3e}  fp32 {ys}  bound {b:.3e}{'  (open item)' if is_open else ''}")
        CURVE.append({"layer": layer, "log2_scale": k, "result": name, "hip": v, "fp32": y, "bound": b, "asserted": not is_open})
        if not is_open and not v <= b:
            bad.append((name, v, b))
    assert not bad, f"{layer} x 2^{k}: {bad}"


# ---- C. recurrence parameters ----------------------------------------------------------------------------------------------------
GATE_BIASES = [f"{rnn}.bias_ih_l0{sfx}" for rnn, sfx in (("intra_rnn", ""), ("intra_rnn", "_reverse"), ("inter_rnn", ""))]


def _norm_weights(sd):
    for nm in ("intra_norm", "inter_norm"):
        sd[SD + nm + ".norm.weight"] *= 2.0 ** -6


def _wide_biases(sd):
    g = torch.Generator().manual_seed(77)
    for n in GATE_BIASES:
        sd[SD + n].copy_((torch.rand(4 * H, generator=g, dtype=torch.float64) * 12 - 6).float())


def _saturated_gates(sd):
    for n in GATE_BIASES:
        for gate in range(4):
            for unit, b in ((0, 80.0), (1, -80.0)):
                sd[SD + n][gate * H + unit] = b
                sd[SD + n.replace("bias_ih", "bias_hh")][gate * H + unit] = 0.0


RECURRENCE = {"norm_weights_2^-6": _norm_weights, "gate_biases_U6": _wide_biases, "gate_biases_+-80": _saturated_gates}


def recurrence_case(mk, which):
    rig = rig_with(mk, RECURRENCE[which])
    for res in (rig.intra(2, 3), rig.inter(2, 3), rig.intra_win(2, 3, 1, 2), rig.inter_win(2, 3, 1, 2)):
        assert all(math.isfinite(v) for v in res.values()), (which, res)
        check(res, which)
