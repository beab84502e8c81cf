"""GPU: the cache policy of the activation streams (csrc/lh_cachepol.h) changes the replacement hint of individual loads and
stores and nothing else, so every output with the policy forced on (lh_set_tuning(19, 2)) must equal, bit for bit, the output
with it off (19 = 0): the stage entry points whose kernels carry a policy at B = 1, T = 17 (one ragged attention tile, one
frame-kernel iteration past a tile) and B = 2, T = 41, one windowed call per stage with a window that starts mid-clip, and a
whole forward on 2 x 0.5 s from the zero state and with state in and out (which also runs every kernel the policy does not
touch).  The attention kernel's tile shape is chosen from the launch's size: at these sizes it is the 32-frame one
(k_local_attn<2, 2, 32>), so the B = 2 cases also run with lh_set_tuning(4, 3), the 40-frame tile of the batch-32 launch
(k_local_attn<3, 2, 40>: at T = 41 a 40-frame tile plus one frame, its masked third row tile and ragged tail included)."""
import pytest
import torch

from lookoncetohear_amd import _cabi
from lookoncetohear_amd.net import Net
from oracle import tfgridnet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NF, C = 97, 64


@pytest.fixture(scope="module")
def net(oracle_cfg_sd):
    _, sd = oracle_cfg_sd
    n = Net(**O.TSH_PARAMS).eval()
    n.load_state_dict(sd, strict=True)
    n = n.to(DEV)
    _cabi.selftest_device(_cabi.load(), 0)
    return n


def _both(run, mq=0):
    """`run()` -> dict of output tensors, once with the policy off and once forced on, under attention tile shape `mq`
    (lh_set_tuning key 4; 0 = by size); keys 19 and 4 go back to their defaults either way"""
    lib = _cabi.load()
    try:
        lib.call("lh_set_tuning", 4, mq)
        lib.call("lh_set_tuning", 19, 0)
        off = {k: v.clone() for k, v in run().items()}
        torch.cuda.synchronize()
        lib.call("lh_set_tuning", 19, 2)
        on = {k: v.clone() for k, v in run().items()}
        torch.cuda.synchronize()
    finally:
        lib.call("lh_set_tuning", 19, 1)
        lib.call("lh_set_tuning", 4, 0)
    assert off.keys() == on.keys()
    for k in off:
        assert torch.isfinite(off[k].float()).all(), k
        assert torch.equal(off[k], on[k]), k


def _stages(net, B, T, win=None):
    """The three policy stages of block 0 on random frames, whole clip or the window (t0, Tc); fresh zeroed outputs per run"""
    lib = _cabi.load()
    pk = net._weights(torch.device(DEV))
    bp = pk["blocks"][0]
    ws = net._workspace(B, T, torch.device(DEV))
    st = torch.cuda.current_stream(DEV).cuda_stream
    P = lambda t: t.data_ptr()
    g = torch.Generator().manual_seed(100 * B + T)
    x = (torch.randn(B, T, NF, C, generator=g) * 3.0).to(DEV)
    gain = torch.randn(2 * B, NF, C, generator=g).to(DEV)
    t0, Tc = win if win else (0, T)
    sfx = "_win" if win else ""
    wargs = (t0, Tc) if win else ()

    def run():
        q, kx, vx = torch.zeros_like(ws["q"]), torch.zeros_like(ws["kx"]), torch.zeros_like(ws["vx"])
        m, out, fan = torch.zeros_like(x), torch.zeros_like(x), torch.zeros(2 * B, T, NF, C, device=DEV)
        ptaps, fmax = torch.zeros(B * T * NF * 36, device=DEV), torch.zeros(B * T, device=DEV)
        lib.call("lh_qkv_proj_ln" + sfx, P(x), P(bp["qkv_w"]), P(bp["qkv_b"]), P(bp["qkv_slopes"]), P(bp["lnq_w"]), P(bp["lnq_b"]),
                 P(bp["lnk_w"]), P(bp["lnk_b"]), P(bp["lnv_w"]), P(bp["lnv_b"]), P(q), P(kx), P(vx), None, B, T, *wargs, st)
        lib.call("lh_local_attn" + sfx, P(q), P(kx), P(vx), P(m), B, T, *wargs, st)
        proj = (P(m), P(bp["proj_w"]), P(bp["proj_b"]), P(bp["proj_slope"]), P(bp["proj_ln_w"]), P(bp["proj_ln_b"]), P(x))
        lib.call("lh_proj_ln_res" + sfx, *proj, P(gain), P(out), B, T, *wargs, st)
        lib.call("lh_proj_ln_res_fan" + sfx, *proj, P(gain), P(fan), B, T, *wargs, 2, st)
        lib.call("lh_proj_ln_res_taps" + sfx, *proj, P(pk["deconv_w"]), P(ptaps), P(fmax), B, T, *wargs, st)
        return dict(q=q, kx=kx, vx=vx, merged=m, out=out, fan=fan, ptaps=ptaps, fmax=fmax)

    return run


@pytest.mark.parametrize("B,T,mq", [(1, 17, 0), (2, 41, 0), (2, 41, 3)])
def test_stage_outputs_do_not_depend_on_the_policy(net, B, T, mq):
    _both(_stages(net, B, T), mq)


@pytest.mark.parametrize("mq", [0, 3])
def test_windowed_stage_outputs_do_not_depend_on_the_policy(net, mq):
    _both(_stages(net, 2, 41, win=(17, 13)), mq)


def test_forward_does_not_depend_on_the_policy(net):
    g = torch.Generator().manual_seed(7)
    mix = (torch.randn(2, 2, 8000, generator=g) * 0.1).to(DEV)
    emb = torch.randn(2, 1, 256, generator=g).to(DEV)

    def from_zero():
        with torch.no_grad():
            return dict(y=net(mix, emb))

    def with_state():
        gs = torch.Generator().manual_seed(8)
        state = net.init_buffers(2, DEV)
        leaves = lambda d: [t for v in d.values() for t in (leaves(v) if isinstance(v, dict) else [v])]
        for t in leaves(state):
            t.copy_((torch.randn(t.shape, generator=gs) * 0.3).to(DEV))
        with torch.no_grad():
            y, nxt = net.predict(mix, emb[:, 0], state)
        return dict(y=y, **{f"state{i}": t for i, t in enumerate(leaves(nxt))})

    _both(from_zero)
    _both(with_state)
