"""Cases of the 79-frame attention tile (k_local_attn<5, 2, 79>, lh_set_tuning(4, 5)) shared by tests/test_gpu_attn_wide.py
(MI355X) and tests/test_emu_attn_wide.py (hipemu): the rig and the float64 reference of tests/stage_cases.py, with the history
rows either zero or written by lh_ring_pack.

`forced_digests` is the record of what the forced forms 1..3 compute: SHA-256 of `merged` for fixed inputs.  The file
tests/golden/attn_forced_forms.json holds the digests of the library BEFORE the 79-frame form existed (same function, MI355X);
the kernels behind keys 1..3 must go on producing exactly those bits."""
import hashlib

import torch

from lookoncetohear_amd.weights import KV_PAD_ROWS, QK_PAD
from tests.stage_cases import F, HIST, NH, QKF, VD, VF, split_qk, split_v

WIDE = 5                                                   # lh_set_tuning(4, WIDE): 79 query frames per workgroup
TQ = 79
SHAPES = [50, 79, 80, 128, 159]      # one partial tile; one full; full + one row; a second tile shorter than the history; two + one row


def wide_case(rig, B, T, hist, mq=WIDE, win=None, nt=None):
    """lh_local_attn (or `win` = (t0, Tc): lh_local_attn_win) under key 4 = mq (and key 19 = nt) on random split rows; `hist`:
    the 49 history rows come from random K_buf / V_buf through lh_ring_pack, else they stay zero.  Returns (Guarded merged,
    float64 reference in merged order): the reference is computed from the decoded rows the kernel reads."""
    from lookoncetohear_amd.weights import unsplit_qk, unsplit_v
    from oracle import tfgridnet_oracle as O
    q, kx, vx = rig._kv_bufs(B, T)
    Qd = rig._split_rows(q.t, rig.randn(B * NH, T, QKF), split_qk)
    if hist:
        kb, vb = rig.randn(B * NH, HIST, QKF), rig.randn(B * NH, HIST, VF)
        rig.call("lh_ring_pack", kb, vb, kx.t, vx.t, B, T, rig.st)
    rig._split_rows(kx.t[:, HIST:HIST + T], rig.randn(B * NH, T, QKF), split_qk)
    rig._split_rows(vx.t[:, HIST:HIST + T], rig.randn(B * NH, T, VF), split_v)
    m = rig.g((B, T, NH, F, VD)).fill_pattern()
    m0 = m.t.clone()
    rig.lib.call("lh_set_tuning", 4, mq)
    if nt is not None:
        rig.lib.call("lh_set_tuning", 19, nt)
    try:
        if win is None:
            rig.call("lh_local_attn", q.t, kx.t, vx.t, m.t, B, T, rig.st)
        else:
            rig.call("lh_local_attn_win", q.t, kx.t, vx.t, m.t, B, T, win[0], win[1], rig.st)
        rig.sync()
    finally:
        rig.lib.call("lh_set_tuning", 4, 0)
        rig.lib.call("lh_set_tuning", 19, 1)
    what = f"local_attn k4={mq} B={B} T={T} hist={hist} win={win}"
    m.check(what), q.check(what + " q"), kx.check(what + " kx"), vx.check(what + " vx")
    if win is not None:
        m.frames_untouched(m0, 1, win[0], win[1], what)
    assert not bool(kx.t[:, T + HIST:].any()) and not bool(vx.t[:, T + HIST:].any()), "pad rows of kx / vx written"
    Kd, Vd = unsplit_qk(kx.t[:, :T + HIST]).double(), unsplit_v(vx.t[:, :T + HIST]).double()
    assert hist == bool(Kd[:, :HIST].any()) and hist == bool(Vd[:, :HIST].any())
    return m, rig._merge(O.local_attention(rig.cfg, Qd, Kd, Vd), B, T)


def forced_digests(lib, dev, stream, sync, B=3, T=159):
    """{str(mq): sha256 of merged} for mq = 1, 2, 3 on inputs from a generator of this function's own (seed 79)."""
    gen = torch.Generator().manual_seed(79)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).float()
    rows = T + HIST + KV_PAD_ROWS
    q = split_qk(rn(B * NH, T, QKF)).to(dev)
    kx = torch.zeros(B * NH, rows, 2 * QK_PAD, dtype=torch.float16)
    vx = torch.zeros(B * NH, rows, 2 * VF, dtype=torch.float16)
    kx[:, :T + HIST] = split_qk(rn(B * NH, T + HIST, QKF))
    vx[:, :T + HIST] = split_v(rn(B * NH, T + HIST, VF))
    kx, vx = kx.to(dev), vx.to(dev)
    out = {}
    try:
        for mq in (1, 2, 3):
            m = torch.zeros(B, T, NH, F, VD, device=dev)
            lib.call("lh_set_tuning", 4, mq)
            lib.call("lh_local_attn", q.data_ptr(), kx.data_ptr(), vx.data_ptr(), m.data_ptr(), B, T, stream)
            sync()
            out[str(mq)] = hashlib.sha256(m.cpu().numpy().tobytes()).hexdigest()
    finally:
        lib.call("lh_set_tuning", 4, 0)
    return out
