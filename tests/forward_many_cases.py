"""Cases shared by tests/test_emu_forward_many.py (hipemu, CPU) and tests/test_gpu_forward_many.py (MI355X): the fan-out form
of block 0's closing stage (`lh_proj_ln_res_fan` / `_win`, include/lookonce_hip.h A.3.6) on a `stage_cases.Rig`, and the scenes
of the `Net.forward_many` tests — mixtures with several enrolled speakers each."""
from __future__ import annotations

import torch

from lookoncetohear_amd import synth
from oracle import tfgridnet_oracle as O
from tests.stage_cases import C, F, NH, PRE, VD, VF, rel_err


def proj_ln_res_fan(rig, B, T, K, scales, win=None):
    """One fan-out call on random inputs (utterance b of y2 scaled by scales[b]) into a guarded, pattern-filled
    out [B * K][T][97][64].  Asserts: guards intact, frames outside the window bitwise untouched, and row b * K + j bitwise
    equal to `lh_proj_ln_res` / `_win` on the same inputs with gain[b * K + j].  Returns the float64 error of all B * K rows
    (per row: max|hip - ref| / max|ref|) under a `proj_ln_res...` name of stage_cases.TOL."""
    mg = rig.randn(B, T, NH, F, VD)
    y2 = rig.randn(B, T, F, C, scales=scales)
    g = rig.randn(B * K, F, C)
    out = rig.g((B * K, T, F, C)).fill_pattern()
    o0 = out.t.clone()
    bp = rig.bp
    head = [mg, bp["proj_w"], bp["proj_b"], bp["proj_slope"], bp["proj_ln_w"], bp["proj_ln_b"], y2]
    t0, Tc = win if win else (0, T)
    name = "proj_ln_res_fan" + ("_win" if win else "") + f".K={K}"
    if win:
        rig.call("lh_proj_ln_res_fan_win", *head, g, out.t, B, T, t0, Tc, K, rig.st)
    else:
        rig.call("lh_proj_ln_res_fan", *head, g, out.t, B, T, K, rig.st)
    rig.sync()
    out.check(name)
    out.frames_untouched(o0, 1, t0, Tc, name)
    w = slice(t0, t0 + Tc)
    rows = out.t.view(B, K, T, F, C)
    for j in range(K):
        gj = g.view(B, K, F, C)[:, j].contiguous()
        one = rig.g((B, T, F, C)).fill_pattern()
        if win:
            rig.call("lh_proj_ln_res_win", *head, gj, one.t, B, T, t0, Tc, rig.st)
        else:
            rig.call("lh_proj_ln_res", *head, gj, one.t, B, T, rig.st)
        rig.sync()
        one.check(name + " single gain")
        assert torch.equal(rows[:, j, w].view(torch.int32), one.t[:, w].view(torch.int32)), f"{name}: target {j} differs in bits"
    Ob = mg.double().permute(0, 2, 1, 3, 4).reshape(B * NH, T, VF)
    ref = O.concat_proj_ln_res(rig.cfg, rig.p, PRE, Ob, y2.double())                      # [B, T, 97, 64], un-gained
    ref = ref[:, None] * g.double().view(B, K, 1, F, C)
    return {name: rel_err(rows[:, :, w], ref[:, :, w], B * K)}


def fan_arg_errors(lib):
    """The C-ABI argument checks of the two entry points: every call below must return LH_ERR_ARG (1) before any launch."""
    p = 4096                                                   # a non-null pointer value: never dereferenced by a refused call
    ok = [p] * 9 + [2, 8]
    bad = []
    for i in range(9):                                         # each pointer null in turn, gain (index 7) included
        a = list(ok)
        a[i] = None
        bad.append(("lh_proj_ln_res_fan", a + [3, None]))
        bad.append(("lh_proj_ln_res_fan_win", a + [1, 4, 3, None]))
    for K in (0, -1):
        bad.append(("lh_proj_ln_res_fan", ok + [K, None]))
        bad.append(("lh_proj_ln_res_fan_win", ok + [0, 8, K, None]))
    for t0, Tc in ((-1, 4), (0, 0), (5, 4), (0, 9)):           # windows outside [0, T = 8)
        bad.append(("lh_proj_ln_res_fan_win", ok + [t0, Tc, 3, None]))
        bad.append(("lh_proj_ln_res_fan_win", ok + [t0, Tc, 1, None]))
    for B, T in ((0, 8), (2, 0)):
        bad.append(("lh_proj_ln_res_fan", [p] * 9 + [B, T, 3, None]))
    for name, args in bad:
        assert lib.raw(name)(*args) == 1, (name, args)


def scene(B, K, n, first=300):
    """B mixtures of n samples with K enrolled speakers each: x [B, 2, n], E [B, K, 256].  E[b, 0] is the embedding of the
    mixture's own target, the others those of unrelated utterances; a smaller scene is the leading part of a larger one."""
    d = synth.batch(list(range(first, first + B)), n)
    rows = [d["embedding_gt"]]
    for k in range(1, K):
        rows.append(synth.batch(list(range(first + 1000 * k, first + 1000 * k + B)), 256)["embedding_gt"])
    return d["mixture"], torch.cat(rows, 1)
