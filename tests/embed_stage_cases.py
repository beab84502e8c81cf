"""Stage harness of the enrollment embedder, shared by tests/test_gpu_embed_stages.py (MI355X) and
tests/test_emu_embed_stages.py (hipemu, CPU): tests/stage_cases.py for the lh_emb_* entry points.

Each `EmbedRig` method calls ONE C-ABI entry point (lh_emb_frontend, lh_emb_axis_fused, lh_emb_axis_mv, lh_emb_attn_block,
lh_emb_head; lh_emb_axis in -DLH_LEGACY builds) directly, with the packed images of `EmbedTFGridNet._weights(dev)` for
`embedder_oracle.synthetic_state_dict(cfg, 0)`, block 0, and compares it with the float64 stage function of
oracle/embedder_oracle.py on the rig's device.  Metric: max|hip - ref| / max|ref| per utterance; a method returns
{name: worst utterance's value}.

Every buffer the call may write sits in a guard region that is checked bitwise.  Every output and every scratch buffer
(gn_part, xsplit, hsplit, q, k, v, vt, sc, p, merged, part) holds a NaN bit pattern before the call (fp32 0x7FC00000, fp16
0x7E00, fp64 NaN), so a read of scratch that the call did not write first, or an output element it did not write, makes an
output non-finite: all outputs are asserted finite.  The pads the GEMMs rely on (features 520..543 of the Q/K rows, keys
T..Tp-1 of P and of V^T) are asserted exactly zero.  Split fp16 images are built and decoded here with the project's
un-rescaled rule (weights.split_f16_unscaled; value = hi + lo).
"""
from __future__ import annotations

import zlib

import torch

from lookoncetohear_amd.weights import split_f16_unscaled
from oracle import embedder_oracle as E
from tests.stage_cases import Guarded, Rig, check as _check, rel_err

F, C, NH, EQ, VD = 65, 64, 4, 8, 16
DQK, DV, QKP = F * EQ, F * VD, 544                       # 520, 1040; Q/K rows padded to 17 k-steps of 32
PRE = "blocks.0."
FRONT_SCALES = [1e-6, 1e4, 1.0, 3e-3, 250.0]             # per-utterance input scales of the front end (std-normalised away)
ACT_SCALES = [0.1, 1.0, 10.0]                            # ... of the activations (every entry starts with a LayerNorm)
NAN32, NAN16 = 0x7FC00000, 0x7E00


def cl(x):
    """[B, C, T, F] (oracle) -> [B, T, F, C] (kernels)."""
    return x.permute(0, 2, 3, 1)


def cf(x):
    """[B, T, F, C] -> [B, C, T, F]."""
    return x.permute(0, 3, 1, 2)


def nan_fill(t: torch.Tensor) -> torch.Tensor:
    if t.dtype == torch.float64:
        t.fill_(float("nan"))
    elif t.dtype == torch.float32:
        t.view(torch.int32).fill_(NAN32)
    else:
        t.view(torch.int16).fill_(NAN16)
    return t


def split_image(v: torch.Tensor) -> torch.Tensor:
    """[...] -> fp16 [2, ...]: hi image, lo image (lo = fp16(v - hi), un-rescaled)."""
    return torch.stack(split_f16_unscaled(v.float()))


def unsplit(img: torch.Tensor) -> torch.Tensor:
    """fp16 [2, ...] -> float64 hi + lo."""
    return img[0].double() + img[1].double()


def all_zero(t: torch.Tensor) -> bool:
    return not bool((t.view(torch.int16) & 0x7FFF).any()) if t.dtype == torch.float16 else not bool((t != 0).any())


class EmbedRig(Rig):
    """A `Lib`, a device, a stream, the packed images of `EmbedTFGridNet._weights(dev)` and the float64 parameters."""

    def __init__(self, lib, net, dev, stream, sync=lambda: None):
        self.lib, self.dev, self.st, self.sync = lib, torch.device(dev), stream, sync
        self.cfg = E.ECfg(**E.EMBED_PARAMS)
        self.pk = net._weights(self.dev)
        self.bp = self.pk["blocks"][0]
        self.p = {k: v.detach().double().to(self.dev) for k, v in net.state_dict().items()}
        self.p32 = {k: v.float() for k, v in self.p.items()}      # the fp32 yardstick's parameters (`yard`: see stage_cases.Rig)
        self.gen = torch.Generator().manual_seed(4321)

    # ---- helpers
    def seed(self, *key):
        """Inputs are a function of the case alone, not of the cases that ran before it: a case measures the same error
        whether it runs alone or in the sweep the bounds were set from."""
        self.gen.manual_seed(zlib.crc32(repr(key).encode()))

    def out(self, shape, dtype=torch.float32):
        """An output or scratch buffer: guard pattern around it, NaN inside."""
        g = Guarded(shape, dtype, self.dev)
        nan_fill(g.t)
        return g

    def act(self, B, T):
        return self.randn(B, T, F, C, scales=[ACT_SCALES[b % 3] for b in range(B)])

    @staticmethod
    def finite(**tensors):
        for n, t in tensors.items():
            assert bool(torch.isfinite(t).all()), f"{n}: non-finite values (unwritten output, or scratch read before it was written)"

    # ---- front end
    def frontend(self, B, N, scales, emit_split):
        T = N // 64 + 1
        self.seed("frontend", B, N, emit_split)
        x = self.randn(B, 2, N, scales=scales)
        pk = self.pk
        z, inv = self.out((B, T, F, C)), self.out((B,))
        gn_part = self.out((B * ((T + 13) // 14) * 2,), torch.float64)
        xs = self.out((2, B, T, F, C), torch.float16) if emit_split else None
        self.call("lh_emb_frontend", x, inv.t, pk["wfb"], pk["conv_w"], pk["conv_b"], pk["gn_w"], pk["gn_b"], gn_part.t, z.t,
                  xs.t if emit_split else None, B, T, N, self.st)
        self.sync()
        z.check("z"), inv.check("inv_std"), gn_part.check("gn_part")
        zr, ir = E.front_end(self.cfg, self.p, x.double())
        sd = torch.std(x.double(), dim=(1, 2))                                      # the reference's figure is 1 / unbiased std
        assert bool(((ir * sd - 1.0).abs() < 1e-12).all())
        self.finite(z=z.t, inv_std=inv.t, gn_part=gn_part.t)
        res = {"frontend.z": rel_err(z.t, cl(zr), B), "frontend.inv_std": rel_err(inv.t, ir, B)}
        if emit_split:
            xs.check("xsplit_next")
            self.finite(xsplit_next=xs.t)
            res["frontend.xsplit"] = rel_err(unsplit(xs.t), E.ln_channels(cl(zr)), B)
        return res

    # ---- axis paths
    def _axis(self, name, B, T, ax, have_xsplit, emit_split, launch, nseq_p, h_dtype=torch.float16):
        self.seed(name, B, T, have_xsplit, emit_split)
        x = self.act(B, T)
        xs, out = self.out((2, B, T, F, C), torch.float16), self.out((B, T, F, C))
        hs = self.out((2, nseq_p, 128), h_dtype) if h_dtype == torch.float16 else self.out((nseq_p, 128), h_dtype)
        if have_xsplit:
            xs.t.copy_(split_image(E.ln_channels(x.double())))
        xs0 = xs.t.clone()
        launch(x, xs, hs, out)
        self.sync()
        xs.check(name + " xsplit"), hs.check(name + " hsplit"), out.check(name)
        ref = cl(E.axis(self.cfg, self.p, PRE, ax, cf(x.double())))
        self.finite(out=out.t, xsplit=xs.t)
        res = {name: rel_err(out.t, ref, B)}
        if emit_split:
            res[name + ".xsplit"] = rel_err(unsplit(xs.t), E.ln_channels(ref), B)
        elif have_xsplit:
            assert torch.equal(xs.t.view(torch.int16), xs0.view(torch.int16)), f"{name}: xsplit written without emit_split"
        else:
            res["lnsplit"] = rel_err(unsplit(xs.t), E.ln_channels(x.double()), B)      # k_emb_lnsplit's own image
        return res

    def axis_fused(self, B, T, inter, have_xsplit, emit_split, prio=0):
        ax = "inter" if inter else "intra"
        bp = self.bp

        def launch(x, xs, hs, out):
            with self.tuning(16, prio):
                self.call("lh_emb_axis_fused", x, bp[ax + "_wrec"], bp[ax + "_brec"], bp[ax + "_wct"], bp[ax + "_bct"], xs.t, hs.t,
                          out.t, B, T, inter, have_xsplit, emit_split, self.st)
        nseq_p = B * F * (T - 3) if inter else B * T * (F - 3)
        return self._axis(f"axis_fused.{ax}" + (".prio" if prio else ""), B, T, ax, have_xsplit, emit_split, launch, nseq_p)

    def axis_mv(self, B, T, have_xsplit, emit_split):
        bp = self.bp

        def launch(x, xs, hs, out):
            self.call("lh_emb_axis_mv", x, bp["inter_wih"], bp["inter_bih"], bp["inter_whh_mv"], bp["inter_wct"], bp["inter_bct"],
                      xs.t, hs.t, out.t, B, T, have_xsplit, emit_split, self.st)
        return self._axis("axis_mv", B, T, "inter", have_xsplit, emit_split, launch, B * F * (T - 3))

    def axis_legacy(self, B, T, inter):
        """lh_emb_axis (-DLH_LEGACY builds: the emulator's): the three-launch form of the same path, gate pre-activations and
        hidden states in fp32."""
        ax = "inter" if inter else "intra"
        bp = self.bp
        nseq_p = B * F * (T - 3) if inter else B * T * (F - 3)
        gx = self.out((nseq_p, 512))

        def launch(x, xs, hs, out):
            self.call("lh_emb_axis", x, bp[ax + "_wih"], bp[ax + "_bih"], bp[ax + "_whh"], bp[ax + "_wct"], bp[ax + "_bct"], xs.t, gx.t,
                      hs.t, out.t, B, T, inter, self.st)
        res = self._axis(f"axis_legacy.{ax}", B, T, ax, 0, 0, launch, nseq_p, torch.float32)      # hbuf: fp32 [nseq * P][128]
        gx.check("gx")
        return res

    # ---- attention block
    def _peaked(self, x2):
        """The smallest Q LayerNorm gain factor at which the reference's median row maximum of the softmax exceeds 0.5, the
        float32 gains (packed order) and the reference parameters that carry it."""
        for g in (2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0, 24.0, 32.0, 48.0, 64.0):
            p = dict(self.p)
            for h in range(NH):
                k = PRE + f"attn_conv_Q_{h}.2.gamma"
                p[k] = (self.p[k].float() * g).double()
            Qh, Kh, Vh = E.qkv_heads(self.cfg, p, PRE, x2)
            sc, att, O = E.attention(self.cfg, Qh, Kh, Vh)
            if float(att.amax(2).median()) > 0.5:
                return self.bp["lnq_w"] * g, p, (Qh, Kh, Vh, sc, att, O)
        raise AssertionError("no gain factor makes the reference softmax peaked")

    def attn_block(self, B, T, emit_split, peaked=False, yard=None):
        self.seed("attn", B, T, emit_split, peaked)
        y2 = self.act(B, T)
        x2 = cf(y2.double())
        bp, p, nb, Tp = self.bp, self.p, NH * B, (T + 63) // 64 * 64
        if peaked:
            lnq_w, p, (Qh, Kh, Vh, scr, att, Or) = self._peaked(x2)
            assert float(att.amax(2).median()) > 0.5
        else:
            lnq_w = bp["lnq_w"]
            Qh, Kh, Vh = E.qkv_heads(self.cfg, p, PRE, x2)
            scr, att, Or = E.attention(self.cfg, Qh, Kh, Vh)
        outr = cl(E.concat_proj_ln_res(self.cfg, p, PRE, Or, x2))
        h16 = torch.float16
        q, k, v = self.out((2, nb, T, QKP), h16), self.out((2, nb, T, QKP), h16), self.out((nb, T, DV))
        vt, sc, pp = self.out((2, nb, DV, Tp), h16), self.out((nb, T, Tp)), self.out((2, nb, T, Tp), h16)
        merged, out = self.out((B, T, F, C)), self.out((B, T, F, C))
        xs = self.out((2, B, T, F, C), h16) if emit_split else None
        self.call("lh_emb_attn_block", y2, bp["wqkv"], bp["bqkv"], bp["slopes"], lnq_w, bp["lnq_b"], bp["lnk_w"], bp["lnk_b"],
                  bp["lnv_w"], bp["lnv_b"], bp["wproj"], bp["bproj"], bp["slope_p"], bp["lnp_w"], bp["lnp_b"], q.t, k.t, v.t, vt.t,
                  sc.t, pp.t, merged.t, out.t, xs.t if emit_split else None, B, T, self.st)
        self.sync()
        for n, t in (("q", q), ("k", k), ("v", v), ("vt", vt), ("sc", sc), ("p", pp), ("merged", merged), ("out", out)):
            t.check(n)
        self.finite(q=q.t, k=k.t, v=v.t, vt=vt.t, sc=sc.t[:, :, :T], p=pp.t, merged=merged.t, out=out.t)
        assert all_zero(q.t[..., DQK:]) and all_zero(k.t[..., DQK:]), "features 520..543 of the Q / K rows are not zero"
        assert all_zero(pp.t[..., T:]), "keys T..Tp-1 of P are not zero"
        assert all_zero(vt.t[..., T:]), "keys T..Tp-1 of V^T are not zero"
        rows = lambda h: h.permute(0, 2, 3, 1).reshape(nb, T, -1)                   # [nb, d, T, F] -> [nb, T, f*d + c]
        sfx = ".peaked" if peaked else ""
        res = {"attn.q" + sfx: rel_err(unsplit(q.t)[..., :DQK], rows(Qh), nb), "attn.k": rel_err(unsplit(k.t)[..., :DQK], rows(Kh), nb),
               "attn.v": rel_err(v.t, rows(Vh), nb), "attn.vt": rel_err(unsplit(vt.t)[..., :T], rows(Vh).transpose(1, 2), nb),
               "attn.sc" + sfx: rel_err(sc.t[:, :, :T], scr, nb), "attn.p" + sfx: rel_err(unsplit(pp.t)[..., :T], att, nb),
               "attn.merged" + sfx: rel_err(merged.t, cl(Or), B), "attn.out" + sfx: rel_err(out.t, outr, B)}
        if emit_split:
            xs.check("xsplit_next")
            self.finite(xsplit_next=xs.t)
            res["attn.xsplit" + sfx] = rel_err(unsplit(xs.t), E.ln_channels(outr), B)
        if yard is not None:
            assert not peaked
            x32 = cf(y2)
            Q32, K32, V32 = E.qkv_heads(self.cfg, self.p32, PRE, x32)
            sc32, att32, O32 = E.attention(self.cfg, Q32, K32, V32)
            out32 = cl(E.concat_proj_ln_res(self.cfg, self.p32, PRE, O32, x32))
            yard.update({"attn.q": rel_err(rows(Q32), rows(Qh), nb), "attn.k": rel_err(rows(K32), rows(Kh), nb),
                         "attn.v": rel_err(rows(V32), rows(Vh), nb), "attn.vt": rel_err(rows(V32), rows(Vh), nb),
                         "attn.sc": rel_err(sc32, scr, nb), "attn.p": rel_err(att32, att, nb),
                         "attn.merged": rel_err(cl(O32), cl(Or), B), "attn.out": rel_err(out32, outr, B)})
            if emit_split:
                yard["attn.xsplit"] = rel_err(E.ln_channels(out32), E.ln_channels(outr), B)
        return res

    # ---- head
    def head(self, B, T, yard=None):
        self.seed("head", B, T)
        z = self.act(B, T)
        pk = self.pk
        part, emb = self.out((B * ((T + 63) // 64) * 256,)), self.out((B, 256))
        self.call("lh_emb_head", z, pk["head_w"], pk["head_b"], pk["head_ln_w"], pk["head_ln_b"], part.t, emb.t, B, T, self.st)
        self.sync()
        part.check("part"), emb.check("emb")
        self.finite(part=part.t, emb=emb.t)
        ref = E.head(self.cfg, self.p, cf(z.double()))
        if yard is not None:
            yard["head"] = rel_err(E.head(self.cfg, self.p32, cf(z)), ref, B)
        return {"head": rel_err(emb.t, ref, B)}


# Bounds on max|hip - ref| / max|ref| per utterance, first matching rule wins (a result without a rule is an error).  Set from
# the MI355X run of tests/test_gpu_embed_stages.py whose whole printed table is profiles/embed_stage_errors.txt (worst case over
# that sweep in the comment) with at most 4x margin, never above 1e-5; where 4x the measured value is above 1e-5 the bound is the
# cap.  Inputs are seeded per case (EmbedRig.seed), so a case measures the same value alone or in the sweep.  The decoded split
# images (.xsplit, lnsplit, q, k, vt, p) carry the split's own error on top of the kernel's: hi + lo keeps 22 bits of the value,
# 2.4e-7 of it, and a lo below the fp16 subnormal spacing adds 2^-25 = 3.0e-8 absolute; the measured values are of that size
# plus the fp32 arithmetic in front, and none needs a bound above the cap either.
ETOL = [
    (r"^frontend\.inv_std$", 2e-7),                               # 5.86e-8
    (r"^frontend\.z$", 1.8e-6),                                   # 4.53e-7
    (r"^frontend\.xsplit$", 1.8e-6),                              # 4.63e-7
    (r"^lnsplit$", 7e-7),                                         # 2.06e-7
    (r"^axis_(fused|mv|legacy)\S*\.xsplit$", 2.8e-6),             # 7.68e-7 (axis_mv, B = 7, T = 34)
    (r"^axis_(fused|mv|legacy)", 2.6e-6),                         # 7.10e-7 (axis_mv, B = 3, T = 36)
    (r"^attn\.(q|k|v|vt)(\.peaked)?$", 2e-6),                     # 5.23e-7
    (r"^attn\.sc", 4e-6),                                         # 1.00e-6
    (r"^attn\.p", 1e-5),                                          # 3.62e-6 flat rows, 7.60e-6 peaked at T = 2049: the cap
    (r"^attn\.merged", 1e-5),                                     # 6.73e-6 (B = 4, T = 1251): the cap
    (r"^attn\.out", 1e-5),                                        # 3.97e-6 (peaked, T = 2049): the cap
    (r"^attn\.xsplit", 1e-5),                                     # 4.35e-6 (B = 4, T = 1251): the cap
    (r"^head$", 8e-6),                                            # 2.95e-6 (B = 3, T = 2)
    (r"^tap\.(z0|blocks\.0\.x[12])$", 1.6e-6),                    # 4.31e-7
    (r"^tap\.emb$", 8e-6),                                        # 2.04e-6
    (r"^tap\.blocks\.", 6.4e-6),                                  # 1.61e-6 (blocks.0.O, B = 8)
]


def check(results: dict, case: str):
    _check(results, case, ETOL)
