"""Stage harness shared by tests/test_gpu_stages.py (MI355X) and tests/test_emu_stages.py (hipemu, CPU).

Each `Rig` method calls one C-ABI entry point of include/lookonce_hip.h directly on random inputs and compares it with the
float64 restatement of the same operation in oracle/tfgridnet_oracle.py (front_end, speaker_gain, qkv_proj_ln,
history_concat, local_attention, concat_proj_ln_res, back_end, and torch's float64 LayerNorm + LSTM).  The metric is
max|hip - ref| / max|ref| per utterance; a method returns {name: worst utterance's value}.

Every output lives inside a guard region filled with a bit pattern, and window calls pre-fill the frames outside
[t0, t0 + Tc): a method asserts that all of them are bitwise unchanged.  Split rows (q / kx / vx) are made and decoded here
(`split_qk` / `split_v` and weights.unsplit_qk / unsplit_v), so the attention kernel is checked on exactly the values it
reads.  The references run in float64 on the rig's device.
"""
from __future__ import annotations

import contextlib
import math
import re

import torch

from lookoncetohear_amd.weights import KV_PAD_ROWS, QK_PAD, unsplit_qk, unsplit_v
from oracle import tfgridnet_oracle as O

F, C, H, NH, E, VD, HIST = 97, 64, 64, 4, 6, 16, 49
QKF, VF = F * E, F * VD                                    # 582, 1552 features per head row
GUARD = 1024                                               # elements of guard before and after every output
PAT32, PAT16 = 0x5A5A5A5A, 0x5A5A                          # finite bit patterns (fp32 1.5e16, fp16 203)
PAT64 = 0x5A5A5A5A5A5A5A5A                                 # (fp64 4.8e127: the embedder's GroupNorm partial sums)
_BITS = {torch.float32: (torch.int32, PAT32), torch.float16: (torch.int16, PAT16), torch.float64: (torch.int64, PAT64)}
PRE = "blocks.0."


def split_qk(v: torch.Tensor) -> torch.Tensor:
    """fp32 [..., 582] -> split-precision q / kx rows [..., 1216] fp16 ([76 blocks][hi 8 | lo 8], pad features 0)."""
    v = torch.nn.functional.pad(v.float(), (0, QK_PAD - v.shape[-1]))
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.stack([hi.reshape(*v.shape[:-1], QK_PAD // 8, 8), lo.reshape(*v.shape[:-1], QK_PAD // 8, 8)],
                       -2).reshape(*v.shape[:-1], 2 * QK_PAD)


def split_v(v: torch.Tensor) -> torch.Tensor:
    """fp32 [..., 1552] -> split-precision vx rows [..., 3104] fp16 ([388 quads][hi 4 | lo 4])."""
    v = v.float()
    hi = v.half()
    lo = (v - hi.float()).half()
    n = v.shape[-1] // 4
    return torch.stack([hi.reshape(*v.shape[:-1], n, 4), lo.reshape(*v.shape[:-1], n, 4)], -2).reshape(*v.shape[:-1], 2 * v.shape[-1])


def rel_err(hip: torch.Tensor, ref: torch.Tensor, B: int) -> float:
    """max over utterances of max|hip - ref| / max|ref| (leading axis = utterance, or utterance * heads)."""
    h = hip.detach().double().reshape(B, -1)
    r = ref.detach().double().reshape(B, -1)
    return float(((h - r).abs().amax(1) / r.abs().amax(1).clamp_min(1e-300)).max())


class Guarded:
    """A tensor of `shape` inside a flat buffer whose GUARD elements before and after hold a bit pattern."""

    def __init__(self, shape, dtype, dev, init=None):
        self.n = math.prod(shape)
        self.buf = torch.empty(self.n + 2 * GUARD, dtype=dtype, device=dev)
        self.itype, self.pat = _BITS[dtype]
        self.ibuf = self.buf.view(self.itype)
        self.ibuf.fill_(self.pat)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def fill_pattern(self):
        self.ibuf[GUARD:GUARD + self.n].fill_(self.pat)
        return self

    def check(self, what: str):
        pat = self.pat
        assert bool((self.ibuf[:GUARD] == pat).all()), f"{what}: write before the buffer"
        assert bool((self.ibuf[GUARD + self.n:] == pat).all()), f"{what}: write past the buffer"

    def frames_untouched(self, before: torch.Tensor, axis_t: int, t0: int, Tc: int, what: str):
        """Frames outside [t0, t0 + Tc) along `axis_t` bitwise equal to `before`."""
        a = self.t.view(self.itype)
        b = before.view(a.dtype)
        T = a.shape[axis_t]
        for lo, hi in ((0, t0), (t0 + Tc, T)):
            if hi > lo:
                assert torch.equal(a.narrow(axis_t, lo, hi - lo), b.narrow(axis_t, lo, hi - lo)), f"{what}: frames [{lo}, {hi}) written"


class Rig:
    """A `Lib`, a device, a stream, the packed weight images of `Net._weights(dev)` and the float64 parameters."""

    def __init__(self, lib, net, dev, stream, sync=lambda: None):
        self.lib, self.dev, self.st, self.sync = lib, torch.device(dev), stream, sync
        self.pk = net._weights(self.dev)
        self.bp = self.pk["blocks"][0]
        sd = {k: v for k, v in net.state_dict().items()}
        self.p = {k: v.to(self.dev) for k, v in O.strip_prefix(sd, torch.float64).items()}
        self.p32 = {k: v.float() for k, v in self.p.items()}      # the fp32 yardstick's parameters (`yard`, below)
        self.cfg = O.Cfg(**O.TSH_PARAMS)
        self.gen = torch.Generator().manual_seed(1234)

    # ---- helpers
    def call(self, name, *args):
        self.lib.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])

    @contextlib.contextmanager
    def tuning(self, key, value):
        self.lib.call("lh_set_tuning", key, value)
        try:
            yield
        finally:
            self.lib.call("lh_set_tuning", key, 0)

    def randn(self, *shape, scales=None):
        """float32 N(0, 1) on the device; `scales` [B]: utterance b (leading axis) multiplied by scales[b]."""
        x = torch.randn(*shape, generator=self.gen, dtype=torch.float64)
        if scales is not None:
            x = x * torch.tensor(scales, dtype=torch.float64).reshape(-1, *([1] * (len(shape) - 1)))
        return x.float().to(self.dev)

    def g(self, shape, dtype=torch.float32, init=None):
        return Guarded(shape, dtype, self.dev, init)

    # `yard` (a dict, optional argument of some methods): filled with the error of the SAME oracle function evaluated in torch
    # float32 on the same inputs and parameters, under the names of the returned results — what plain fp32 arithmetic loses
    # on this case, the yardstick of tests/param_cases.py
    def _ln(self, x, nm):
        return torch.nn.functional.layer_norm(x.double(), (C,), self.p[PRE + nm + ".norm.weight"], self.p[PRE + nm + ".norm.bias"], 1e-5)

    def _lstm(self, x, nm, h0=None, c0=None, bidirectional=False):
        return O._lstm_fast(x, self.p, PRE + nm + ".", h0, c0, bidirectional)

    # ---- A.1 front end
    def stft_conv_in(self, B, T, scales, yard=None):
        ns = 128 * T + 64
        x = self.randn(B, 2, ns, scales=scales)
        cb = self.randn(B, 4, 2, F, scales=[0.5 * s for s in scales])
        z, cbo = self.g((B, T, F, C)), self.g((B, 4, 2, F))
        self.call("lh_stft_conv_in", x, cb, cbo.t, self.pk["wfb_t"], self.pk["conv_w"], self.pk["conv_b"], z.t, B, T, ns, self.st)
        self.sync()
        zr, nb, _ = O.front_end(self.cfg, self.p, x.double(), cb.double())
        z.check("z"), cbo.check("conv_buf_out")
        if yard is not None:
            z32, nb32, _ = O.front_end(self.cfg, self.p32, x, cb)
            yard.update({"stft_conv_in": rel_err(z32, zr, B), "stft_conv_in.conv_buf": rel_err(nb32, nb, B)})
        return {"stft_conv_in": rel_err(z.t, zr, B), "stft_conv_in.conv_buf": rel_err(cbo.t, nb, B)}

    # ---- A.2 speaker gain
    def embed_proj_ln(self, B):
        e = self.randn(B, 256)
        scratch, gain = self.g((B, F * C)), self.g((B, F, C))
        self.call("lh_embed_proj_ln", e, self.pk["emb_w"], self.pk["emb_b"], self.pk["emb_ln_w"], self.pk["emb_ln_b"], scratch.t,
                  gain.t, B, self.st)
        self.sync()
        gr = O.speaker_gain(self.cfg, self.p, e.double())[:, 0]
        scratch.check("scratch"), gain.check("gain")
        return {"embed_proj_ln": rel_err(gain.t, gr, B)}

    # ---- A.3.1 intra: every kernel behind the intra stage, and its window form
    def _intra_ref(self, x):
        B, T = x.shape[:2]
        hs, _, _ = self._lstm(self._ln(x, "intra_norm").reshape(B * T, F, C), "intra_rnn", bidirectional=True)
        y = x.double() + (hs @ self.p[PRE + "intra_linear.weight"].t() + self.p[PRE + "intra_linear.bias"]).reshape(B, T, F, C)
        return hs.reshape(B, T, F, 2 * H), y

    def intra(self, B, T, fused=True, stream=True):
        x = self.randn(B, T, F, C)
        hr, yr = self._intra_ref(x)
        bp, out = self.bp, {}
        runs = [("ln_lstm_intra.f16x3", "lh_ln_lstm_intra", 1), ("ln_lstm_intra.f32", "lh_ln_lstm_intra", 0)]
        if stream:
            runs.append(("intra_stream", "lh_intra_stream", None))
        for name, fn, mode in runs:
            h, y = self.g((B * T * F, 2 * H)), self.g((B, T, F, C))
            if fn == "lh_intra_stream":
                self.call(fn, x, bp["intra_s_wih"], bp["intra_s_b"], bp["intra_s_whh"], h.t, B * T, self.st)
            else:
                w, b = (bp["intra_w16"], bp["intra_b16"]) if mode else (bp["intra_w"], bp["intra_b"])
                self.call(fn, x, bp["intra_ln_w"], bp["intra_ln_b"], w, b, h.t, B * T, mode, self.st)
            self.call("lh_linear_res", h.t, bp["intra_lin_w"], bp["intra_lin_b"], x, y.t, B * T * F, 2 * H, self.st)
            self.sync()
            h.check(name), y.check(name + " + linear_res")
            out[name + ".h"] = rel_err(h.t, hr, B)
            out[name + "+linear_res"] = rel_err(y.t, yr, B)
        if fused:
            y = self.g((B, T, F, C))
            self.call("lh_intra_block", x, bp["intra_w16"], bp["intra_b16"], bp["intra_lin_w2"], bp["intra_lin_b"], y.t, B * T, self.st)
            self.sync()
            y.check("intra_block")
            out["intra_block"] = rel_err(y.t, yr, B)
        return out

    def intra_win(self, B, T, t0, Tc):
        x = self.randn(B, T, F, C)
        hr, yr = self._intra_ref(x)
        bp, out = self.bp, {}
        w = slice(t0, t0 + Tc)
        h = self.g((B, T, F, 2 * H)).fill_pattern()
        y = self.g((B, T, F, C)).fill_pattern()
        h0, y0 = h.t.clone(), y.t.clone()
        self.call("lh_ln_lstm_intra_win", x, bp["intra_ln_w"], bp["intra_ln_b"], bp["intra_w16"], bp["intra_b16"], h.t, B, T, t0, Tc,
                  self.st)
        self.call("lh_linear_res_win", h.t, bp["intra_lin_w"], bp["intra_lin_b"], x, y.t, B, T, t0, Tc, 2 * H, self.st)
        self.sync()
        h.check("ln_lstm_intra_win"), y.check("linear_res_win")
        h.frames_untouched(h0, 1, t0, Tc, "ln_lstm_intra_win"), y.frames_untouched(y0, 1, t0, Tc, "linear_res_win")
        out["ln_lstm_intra_win.h"] = rel_err(h.t[:, w], hr[:, w], B)
        out["ln_lstm_intra_win+linear_res_win"] = rel_err(y.t[:, w], yr[:, w], B)
        y = self.g((B, T, F, C)).fill_pattern()
        self.call("lh_intra_block_win", x, bp["intra_w16"], bp["intra_b16"], bp["intra_lin_w2"], bp["intra_lin_b"], y.t, B, T, t0, Tc,
                  self.st)
        self.sync()
        y.check("intra_block_win"), y.frames_untouched(y0, 1, t0, Tc, "intra_block_win")
        out["intra_block_win"] = rel_err(y.t[:, w], yr[:, w], B)
        return out

    # ---- A.3.2 inter: every kernel behind the inter stage with a carried state, and the window forms (carry = 0)
    def _inter_ref(self, x, h0, c0):
        B, T = x.shape[:2]
        v = self._ln(x, "inter_norm").transpose(1, 2).reshape(B * F, T, C)
        hs, h, c = self._lstm(v, "inter_rnn", h0.double()[None], c0.double()[None])
        lin = (hs @ self.p[PRE + "inter_linear.weight"].t() + self.p[PRE + "inter_linear.bias"]).reshape(B, F, T, C).transpose(1, 2)
        return hs.reshape(B, F, T, H).transpose(1, 2), x.double() + lin, h[0], c[0]

    def _inter_state(self, B):
        return self.randn(B * F, H) * 0.3, self.randn(B * F, H) * 0.3

    def inter(self, B, T, matvec=True):
        x = self.randn(B, T, F, C)
        h0, c0 = self._inter_state(B)
        hr, yr, hnr, cnr = self._inter_ref(x, h0, c0)
        bp, out = self.bp, {}
        runs = [("ln_lstm_inter.f16x3", 1), ("ln_lstm_inter.f32", 0), ("inter_block.k5=0", "b0"), ("inter_block.k5=2", "b2")]
        if matvec:
            runs.append(("inter_matvec", "mv"))
        for name, mode in runs:
            y, hN, cN = self.g((B, T, F, C)), self.g((B * F, H)), self.g((B * F, H))
            if mode in (0, 1):
                h = self.g((B, T, F, H))
                w, b = (bp["inter_w16"], bp["inter_b16"]) if mode else (bp["inter_w"], bp["inter_b"])
                self.call("lh_ln_lstm_inter", x, bp["inter_ln_w"], bp["inter_ln_b"], w, b, h0, c0, hN.t, cN.t, h.t, B, T, mode, self.st)
                self.call("lh_linear_res", h.t, bp["inter_lin_w"], bp["inter_lin_b"], x, y.t, B * T * F, H, self.st)
                self.sync()
                h.check(name)
                out[name + ".h"] = rel_err(h.t, hr, B)
                name += "+linear_res"
            elif mode == "mv":
                self.call("lh_inter_matvec", x, bp["inter_s_wih"], bp["inter_s_b"], bp["inter_s_whh"], bp["inter_lin_w"], bp["inter_lin_b"],
                          h0, c0, hN.t, cN.t, y.t, B, T, self.st)
            else:
                with self.tuning(5, int(mode[1])):
                    self.call("lh_inter_block", x, bp["inter_w8"], bp["inter_b16"], bp["inter_lin_wu"], bp["inter_lin_b"], h0, c0, hN.t,
                              cN.t, y.t, B, T, self.st)
            self.sync()
            y.check(name), hN.check(name + " hN"), cN.check(name + " cN")
            out[name] = rel_err(y.t, yr, B)
            out[name + ".hN"] = rel_err(hN.t, hnr, B)
            out[name + ".cN"] = rel_err(cN.t, cnr, B)
        return out

    def inter_win(self, B, T, t0, Tc):
        x = self.randn(B, T, F, C)
        h0, c0 = self._inter_state(B)
        _, yr, hnr, cnr = self._inter_ref(x[:, t0:t0 + Tc], h0, c0)
        bp, out = self.bp, {}
        for name in ("inter_block_win", "inter_matvec_win"):
            y = self.g((B, T, F, C)).fill_pattern()
            y0 = y.t.clone()
            hN, cN = self.g((B * F, H)), self.g((B * F, H))
            if name == "inter_block_win":
                self.call("lh_inter_block_win", x, bp["inter_w8"], bp["inter_b16"], bp["inter_lin_wu"], bp["inter_lin_b"], h0, c0, hN.t,
                          cN.t, y.t, B, T, t0, Tc, 0, self.st)
            else:
                self.call("lh_inter_matvec_win", x, bp["inter_s_wih"], bp["inter_s_b"], bp["inter_s_whh"], bp["inter_lin_w"],
                          bp["inter_lin_b"], h0, c0, hN.t, cN.t, y.t, B, T, t0, Tc, 0, self.st)
            self.sync()
            y.check(name), hN.check(name + " hN"), cN.check(name + " cN")
            y.frames_untouched(y0, 1, t0, Tc, name)
            out[name] = rel_err(y.t[:, t0:t0 + Tc], yr, B)
            out[name + ".hN"] = rel_err(hN.t, hnr, B)
            out[name + ".cN"] = rel_err(cN.t, cnr, B)
        return out

    # ---- A.3.3 - A.3.5 attention: Q/K/V rows, history rows in / out, local attention
    def _kv_bufs(self, B, T, rows=None):
        rows = T + HIST + KV_PAD_ROWS if rows is None else rows
        q = self.g((B * NH, T, 2 * QK_PAD), torch.float16, torch.zeros(B * NH, T, 2 * QK_PAD))
        kx = self.g((B * NH, rows, 2 * QK_PAD), torch.float16, torch.zeros(B * NH, rows, 2 * QK_PAD))
        vx = self.g((B * NH, rows, 2 * VF), torch.float16, torch.zeros(B * NH, rows, 2 * VF))
        return q, kx, vx

    def _qkv_call(self, y, q, kx, vx, B, T, win=None, ring_pos=None):
        bp = self.bp
        args = [y, bp["qkv_w"], bp["qkv_b"], bp["qkv_slopes"], bp["lnq_w"], bp["lnq_b"], bp["lnk_w"], bp["lnk_b"], bp["lnv_w"],
                bp["lnv_b"], q.t, kx.t, vx.t, ring_pos, B, T]
        if win is None:
            self.call("lh_qkv_proj_ln", *args, self.st)
        else:
            self.call("lh_qkv_proj_ln_win", *args, *win, self.st)

    def qkv_ring(self, B, T, scales, yard=None):
        """K_buf / V_buf -> lh_ring_pack -> lh_qkv_proj_ln -> lh_ring_unpack against Q, K, V and the new history."""
        y = self.randn(B, T, F, C, scales=scales)
        kb, vb = self.randn(B * NH, HIST, QKF), self.randn(B * NH, HIST, VF)
        q, kx, vx = self._kv_bufs(B, T)
        self.call("lh_ring_pack", kb, vb, kx.t, vx.t, B, T, self.st)
        self._qkv_call(y, q, kx, vx, B, T)
        kb2, vb2 = self.g((B * NH, HIST, QKF)), self.g((B * NH, HIST, VF))
        self.call("lh_ring_unpack", kx.t, vx.t, kb2.t, vb2.t, B, T, self.st)
        self.sync()
        for n, t in (("q", q), ("kx", kx), ("vx", vx), ("k_buf", kb2), ("v_buf", vb2)):
            t.check(n)
        assert not bool(kx.t[:, T + HIST:].any()) and not bool(vx.t[:, T + HIST:].any()), "pad rows of kx / vx written"
        Qr, Kr, Vr = O.qkv_proj_ln(self.cfg, self.p, PRE, y.double())
        _, _, kbr, vbr = O.history_concat(self.cfg, kb.double(), vb.double(), Kr, Vr)
        if yard is not None:
            Q32, K32, V32 = O.qkv_proj_ln(self.cfg, self.p32, PRE, y)
            yard.update({"qkv_proj_ln.Q": rel_err(Q32, Qr, B), "qkv_proj_ln.K": rel_err(K32, Kr, B), "qkv_proj_ln.V": rel_err(V32, Vr, B)})
        return {"qkv_proj_ln.Q": rel_err(unsplit_qk(q.t), Qr, B),
                "qkv_proj_ln.K": rel_err(unsplit_qk(kx.t[:, HIST:HIST + T]), Kr, B),
                "qkv_proj_ln.V": rel_err(unsplit_v(vx.t[:, HIST:HIST + T]), Vr, B),
                "ring_pack": max(rel_err(unsplit_qk(kx.t[:, :HIST]), kb, B), rel_err(unsplit_v(vx.t[:, :HIST]), vb, B)),
                "ring_unpack.K_buf": rel_err(kb2.t, kbr, B), "ring_unpack.V_buf": rel_err(vb2.t, vbr, B)}

    def local_attn(self, B, T, mq=0):
        """Attention on split rows made here (history rows included), against local_attention on the decoded rows."""
        q, kx, vx = self._kv_bufs(B, T)
        Qd = self._split_rows(q.t, self.randn(B * NH, T, QKF), split_qk)
        Kd = self._split_rows(kx.t[:, :T + HIST], self.randn(B * NH, T + HIST, QKF), split_qk)
        Vd = self._split_rows(vx.t[:, :T + HIST], self.randn(B * NH, T + HIST, VF), split_v)
        m = self.g((B, T, NH, F, VD))
        with self.tuning(4, mq):
            self.call("lh_local_attn", q.t, kx.t, vx.t, m.t, B, T, self.st)
        self.sync()
        m.check(f"local_attn mq={mq}")
        Or = O.local_attention(self.cfg, Qd, Kd, Vd)
        return {f"local_attn.k4={mq}": rel_err(m.t, self._merge(Or, B, T), B)}

    def _split_rows(self, dst, v, split):
        dst.copy_(split(v))
        return (unsplit_qk(dst) if split is split_qk else unsplit_v(dst)).double()

    @staticmethod
    def _merge(Ob, B, T):
        """O [B*4, T, 97*16] -> merged [B][T][4][97][16]."""
        return Ob.reshape(B, NH, T, F, VD).permute(0, 2, 1, 3, 4)

    def qkv_attn_win(self, B, T, t0, Tc, mq=0):
        """Window forms: rows past the window filled with an unrelated input's rows first (read, never used), frames outside the
        window bitwise unchanged, Q / K / V and the attention of the window against float64."""
        y, other = self.randn(B, T, F, C), self.randn(B, T, F, C) * 1e3
        q, kx, vx = self._kv_bufs(B, T)
        kb, vb = self.randn(B * NH, HIST, QKF), self.randn(B * NH, HIST, VF)
        self.call("lh_ring_pack", kb, vb, kx.t, vx.t, B, T, self.st)
        self._qkv_call(other, q, kx, vx, B, T)                          # unrelated rows everywhere
        self._qkv_call(y, q, kx, vx, B, T, win=(0, t0))                 # the true history rows ...
        self.sync()
        snap = [t.t.clone() for t in (q, kx, vx)]
        self._qkv_call(y, q, kx, vx, B, T, win=(t0, Tc))                # ... and the window
        self.sync()
        for n, t, s, ax_off in (("q", q, snap[0], 0), ("kx", kx, snap[1], HIST), ("vx", vx, snap[2], HIST)):
            t.check(n + "_win")
            a, b = t.t.view(torch.int16), s.view(torch.int16)
            assert torch.equal(a[:, :ax_off + t0], b[:, :ax_off + t0]) and torch.equal(a[:, ax_off + t0 + Tc:], b[:, ax_off + t0 + Tc:]), \
                f"qkv_proj_ln_win: {n} rows outside the window written"
        Qr, Kr, Vr = O.qkv_proj_ln(self.cfg, self.p, PRE, y.double())
        w = slice(t0, t0 + Tc)
        out = {"qkv_proj_ln_win.Q": rel_err(unsplit_qk(q.t[:, w]), Qr[:, w], B),
               "qkv_proj_ln_win.K": rel_err(unsplit_qk(kx.t[:, HIST + t0:HIST + t0 + Tc]), Kr[:, w], B),
               "qkv_proj_ln_win.V": rel_err(unsplit_v(vx.t[:, HIST + t0:HIST + t0 + Tc]), Vr[:, w], B)}
        m = self.g((B, T, NH, F, VD)).fill_pattern()
        m0 = m.t.clone()
        with self.tuning(4, mq):
            self.call("lh_local_attn_win", q.t, kx.t, vx.t, m.t, B, T, t0, Tc, self.st)
        self.sync()
        m.check("local_attn_win"), m.frames_untouched(m0, 1, t0, Tc, "local_attn_win")
        Qd = unsplit_qk(q.t[:, w]).double()
        Kd = unsplit_qk(kx.t[:, t0:t0 + Tc + HIST]).double()
        Vd = unsplit_v(vx.t[:, t0:t0 + Tc + HIST]).double()
        out[f"local_attn_win.k4={mq}"] = rel_err(m.t[:, w], self._merge(O.local_attention(self.cfg, Qd, Kd, Vd), B, Tc), B)
        return out

    def stream_ring(self, B, steps):
        """T = 1 steps through lh_qkv_proj_ln(ring_pos) + lh_local_attn + lh_ring_advance over a 50-row ring that starts with
        history, against the reference shifting K_buf / V_buf by one row per chunk.  Returns the worst error over all steps."""
        q, kx, vx = self._kv_bufs(B, 1, rows=1 + HIST + KV_PAD_ROWS)
        kb = self._split_rows(kx.t[:, 1:HIST + 1], self.randn(B * NH, HIST, QKF), split_qk)      # slots 1..49: the history
        vb = self._split_rows(vx.t[:, 1:HIST + 1], self.randn(B * NH, HIST, VF), split_v)
        pos = torch.zeros(1, dtype=torch.int32, device=self.dev)
        m = self.g((B, 1, NH, F, VD))
        worst = {}
        for s in range(steps):
            y = self.randn(B, 1, F, C)
            self._qkv_call(y, q, kx, vx, B, 1, ring_pos=pos)
            self.call("lh_local_attn", q.t, kx.t, vx.t, m.t, B, 1, self.st)
            self.call("lh_ring_advance", pos, 50, self.st)
            self.sync()
            Qr, Kr, Vr = O.qkv_proj_ln(self.cfg, self.p, PRE, y.double())
            Kxr, Vxr, kb, vb = O.history_concat(self.cfg, kb, vb, Kr, Vr)
            Or = O.local_attention(self.cfg, Qr, Kxr, Vxr)
            # the ring holds the window in rotated order: slot (s + 1 + j) mod 50 = window row j
            order = [(s + 1 + j) % 50 for j in range(50)]
            e = {"stream_ring.attn": rel_err(m.t, self._merge(Or, B, 1), B),
                 "stream_ring.K": rel_err(unsplit_qk(kx.t[:, order]), Kxr, B),
                 "stream_ring.V": rel_err(unsplit_v(vx.t[:, order]), Vxr, B)}
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert int(pos.item()) == (s + 1) % 50, "lh_ring_advance"
        for n, t in (("q", q), ("ring k", kx), ("ring v", vx), ("merged", m)):
            t.check(n)
        return worst

    # ---- A.3.6 projection + LayerNorm + residual (+ gain)
    def proj_ln_res(self, B, T, scales, gain=True, win=None, yard=None):
        mg = self.randn(B, T, NH, F, VD)
        y2 = self.randn(B, T, F, C, scales=scales)
        g = self.randn(B, F, C) if gain else None
        out = self.g((B, T, F, C)).fill_pattern()
        o0 = out.t.clone()
        bp = self.bp
        args = [mg, bp["proj_w"], bp["proj_b"], bp["proj_slope"], bp["proj_ln_w"], bp["proj_ln_b"], y2, g, out.t, B, T]
        name = "proj_ln_res" + ("_win" if win else "") + (".gain" if gain else "")
        if win:
            self.call("lh_proj_ln_res_win", *args, *win, self.st)
        else:
            self.call("lh_proj_ln_res", *args, self.st)
        self.sync()
        out.check(name)
        Ob = mg.double().permute(0, 2, 1, 3, 4).reshape(B * NH, T, VF)
        ref = O.concat_proj_ln_res(self.cfg, self.p, PRE, Ob, y2.double())
        if gain:
            ref = ref * g.double()[:, None]
        t0, Tc = win if win else (0, T)
        if win:
            out.frames_untouched(o0, 1, t0, Tc, name)
        if yard is not None:
            r32 = O.concat_proj_ln_res(self.cfg, self.p32, PRE, Ob.float(), y2)
            yard[name] = rel_err((r32 * g[:, None] if gain else r32)[:, t0:t0 + Tc], ref[:, t0:t0 + Tc], B)
        return {name: rel_err(out.t[:, t0:t0 + Tc], ref[:, t0:t0 + Tc], B)}

    # ---- A.4 back end
    def deconv_istft(self, B, T, scales, runs=0, yard=None):
        y = self.randn(B, T, F, C, scales=scales)
        db = self.randn(B, C, 2, F, scales=scales)
        ib = self.randn(B, 2, 2 * F, 1, scales=[0.3 * s for s in scales])
        dbo, ibo, wave = self.g((B, C, 2, F)), self.g((B, 2, 2 * F, 1)), self.g((B, 2, 128 * T))
        with self.tuning(6, runs):
            self.call("lh_deconv_istft", y, db, dbo.t, ib, ibo.t, self.pk["deconv_w"], self.pk["deconv_b"], self.pk["wfb_dec"], wave.t,
                      None, 1, B, T, self.st)
        self.sync()
        for n, t in (("deconv_buf_out", dbo), ("istft_buf_out", ibo), ("wave", wave)):
            t.check(n)
        wr, dr, ir = O.back_end(self.cfg, self.p, y.double(), db.double(), ib.double())
        k = f"deconv_istft.k6={runs}"
        if yard is not None:
            w32, d32, i32 = O.back_end(self.cfg, self.p32, y, db, ib)
            yard.update({k: rel_err(w32[..., :-64], wr[..., :-64], B), k + ".deconv_buf": rel_err(d32, dr, B),
                         k + ".istft_buf": rel_err(i32, ir, B)})
        return {k: rel_err(wave.t, wr[..., :-64], B), k + ".deconv_buf": rel_err(dbo.t, dr, B),
                k + ".istft_buf": rel_err(ibo.t, ir, B)}


# Bounds on max|hip - ref| / max|ref| per utterance, first matching rule wins (a result without a rule is an error).  Set from
# the first MI355X run of tests/test_gpu_stages.py (worst case over the sweep in the comment) with at most 4x margin, never
# above 1e-5.
TOL = [
    (r"\.deconv_buf$", 0.0),                                      # a copy of the last two input frames: exact
    (r"\.istft_buf$", 4e-6),                                      # 1.24e-6
    (r"^deconv_istft", 1e-5),                                     # 6.65e-6: the 1e-6-scale utterance, whose output is the bias
    (r"\.(hN|cN)$", 3e-6),                                        # 9.54e-7
    (r"\.h$", 2.5e-6),                                            # 7.39e-7
    (r"^(intra_block|inter_block|inter_matvec)|linear_res", 4e-7),  # 1.18e-7
    (r"^stft_conv_in", 1.5e-6),                                   # 4.77e-7
    (r"^embed_proj_ln", 8e-7),                                    # 2.20e-7
    (r"^ring_pack", 4e-7),                                        # 1.19e-7
    (r"^(qkv_proj_ln|ring_unpack|stream_ring\.[KV]$)", 1.5e-6),    # 4.49e-7
    (r"^stream_ring\.attn$", 5e-6),                               # 1.46e-6
    (r"^local_attn", 4e-6),                                       # 1.08e-6
    (r"^proj_ln_res", 2e-6),                                      # 5.78e-7
]


def bound(name: str, table=None) -> float:
    for pat, b in (TOL if table is None else table):
        if re.search(pat, name):
            return b
    raise KeyError(f"no bound for {name}")


def check(results: dict, case: str, table=None):
    """Print every measured error next to its bound (of `table`, default TOL), then assert all of them."""
    bad = []
    for k, v in results.items():
        b = bound(k, table)
        print(f"{case:>24} {k:<44} {v:.3e}  (bound {b:.0e})")
        if not v <= b:
            bad.append((k, v, b))
    assert not bad, f"{case}: {bad}"
