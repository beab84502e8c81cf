"""CPU: `Net.forward_many` and the fan-out form of block 0's closing stage (`lh_proj_ln_res_fan` / `_win`, ABI 25) on the hipemu
emulator — the stage against the single-gain kernel (bits) and float64, the forward against the oracle pair by pair and
against `forward`, the launches it makes, and the argument checks of the C ABI and of the method."""
from unittest import mock

import pytest
import torch

from lookoncetohear_amd import _cabi
from oracle import tfgridnet_oracle as O
from tests.forward_many_cases import fan_arg_errors, proj_ln_res_fan, scene
from tests.hipemu.hosts import EmuNet
from tests.stage_cases import Rig, check

TOL = 5e-5                                                     # the bound of tests/test_emu_kernels.py for emulated kernels against the oracle
RANGE = [1e-6, 1e4, 1.0]
FORCED = ("fuse_intra_min_frames", "stream_intra_max_frames", "inter_matvec_max_seqs", "time_chunks", "time_chunks_small",
          "chunk_min_frames")


@pytest.fixture(scope="module")
def emu_net(oracle_cfg_sd):
    from tests.hipemu.build_emu import build_emu
    _, sd = oracle_cfg_sd
    net = EmuNet(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net.emu_lib = _cabi.Lib(build_emu())
    return net


@pytest.fixture(scope="module")
def rig(emu_net):
    return Rig(emu_net.emu_lib, emu_net, "cpu", 0)


@pytest.mark.parametrize("K", [1, 3])
def test_fan_stage_whole_clip(rig, K):
    check(proj_ln_res_fan(rig, 3, 2, K, RANGE), f"B=3 T=2 K={K}")


def test_fan_stage_window(rig):
    check(proj_ln_res_fan(rig, 3, 41, 2, RANGE, win=(17, 23)), "B=3 T=41 t0=17 Tc=23 K=2")


def test_fan_argument_errors(rig):
    fan_arg_errors(rig.lib)


def _forced(net, **kw):
    saved = {k: getattr(net, k) for k in FORCED}
    for k, v in kw.items():
        assert k in saved
        setattr(net, k, v)
    return saved


def test_forward_many_whole_clip_windows_and_oracle(emu_net, oracle_cfg_sd):
    """B = 2 mixtures, K = 3 speakers each, T = 7 frames.  Whole clip, then block 0 (2 rows: the unfused intra pair) in 3 windows of
    2 / 2 / 3 frames and blocks 1, 2 (6 rows: the fused kernels, forced at this size) in 2 windows of 3 / 4 — the fan-out call
    once per window of block 0, into the buffer the 6-row part reads."""
    cfg, sd = oracle_cfg_sd
    B, K, T = 2, 3, 7
    x, E = scene(B, K, 128 * T + 64)
    # 14 frames below and 42 frames above the fused / unfused crossing; no per-sequence inter kernel, no streaming intra kernel
    saved = _forced(emu_net, fuse_intra_min_frames=20, stream_intra_max_frames=0, inter_matvec_max_seqs=0, time_chunks=1,
                    time_chunks_small=1)
    try:
        assert emu_net._n_time_chunks(B, T, 1) == 1 and emu_net._n_time_chunks(B * K, T, 1) == 1
        y1 = emu_net.forward_many(x, E, pad=False)
        y_one = emu_net.forward_many(x, E[:, :1], pad=False)
        y_fwd = emu_net(x, E[:, :1], pad=False)
        emu_net.time_chunks, emu_net.time_chunks_small, emu_net.chunk_min_frames = 2, 3, 2
        assert emu_net._n_time_chunks(B, T, 1) == 3 and emu_net._n_time_chunks(B * K, T, 1) == 2
        yw = emu_net.forward_many(x, E, pad=False)
    finally:
        for k, v in saved.items():
            setattr(emu_net, k, v)
    assert y1.shape == (B, K, 2, 128 * T)
    for b in range(B):
        for k in range(K):
            yo = O.forward(cfg, sd, x[b:b + 1], E[b:b + 1, k:k + 1], pad=False)
            e = float((y1[b, k] - yo[0]).abs().max())
            print(f"[{b}, {k}] max|hip - oracle| = {e:.3e}, windowed - whole = {float((yw[b, k] - y1[b, k]).abs().max()):.3e}")
            assert e < TOL, (b, k)
    assert y_one.shape == (B, 1, 2, 128 * T) and torch.equal(y_one[:, 0], y_fwd)
    assert torch.equal(yw, y1)


def test_forward_many_launches(emu_net):
    """K = 3: the front end once on the B mixtures, one gain call for the B K embeddings, the fan-out entry once per window of
    block 0, the single-gain stage never with a gain; a plain `forward` calls neither new entry point."""
    B, K, T = 2, 3, 7
    x, E = scene(B, K, 128 * T + 64)
    lib, call = emu_net.emu_lib, emu_net.emu_lib.call
    gain_arg = {"lh_proj_ln_res": 7, "lh_proj_ln_res_win": 7}
    saved = _forced(emu_net, fuse_intra_min_frames=20, stream_intra_max_frames=0, inter_matvec_max_seqs=0, time_chunks=2,
                    time_chunks_small=3, chunk_min_frames=2)
    try:
        for n_win in (3, 1):
            if n_win == 1:
                emu_net.time_chunks_small = 1
            calls = []
            with mock.patch.object(lib, "call", lambda name, *a: (calls.append((name, a)), call(name, *a))[1]):
                emu_net.forward_many(x, E, pad=False)
            names = [c[0] for c in calls]
            front = [a for n, a in calls if n == "lh_stft_conv_in"]
            assert len(front) == 1 and front[0][7] == B
            gains = [a for n, a in calls if n == "lh_embed_proj_ln"]
            assert len(gains) == 1 and gains[0][7] == B * K
            fan = "lh_proj_ln_res_fan_win" if n_win > 1 else "lh_proj_ln_res_fan"
            assert names.count(fan) == n_win and names.count("lh_proj_ln_res_fan") + names.count("lh_proj_ln_res_fan_win") == n_win
            assert all(a[9] == B and a[-2] == K for n, a in calls if n == fan)
            single = [a for n, a in calls if n in gain_arg]
            assert single and all(a[7] is None for a in single)
            back = [a for n, a in calls if n == "lh_deconv_istft"]
            assert len(back) == 1 and back[0][11] == B * K
        calls = []
        with mock.patch.object(lib, "call", lambda name, *a: (calls.append((name, a)), call(name, *a))[1]):
            emu_net(x, E[:, :1], pad=False)
        assert not {"lh_proj_ln_res_fan", "lh_proj_ln_res_fan_win"} & {c[0] for c in calls}
        assert sum(a[7] is not None for n, a in calls if n in gain_arg) == 1          # block 0, with its gain
    finally:
        for k, v in saved.items():
            setattr(emu_net, k, v)


def test_forward_many_modes(emu_net, oracle_cfg_sd):
    """`f32rec` (exact-fp32 recurrences) shares block 0 like the default mode; `f32all` runs the repeated mixtures through the
    reference kernels and calls neither fan-out entry point."""
    cfg, sd = oracle_cfg_sd
    x, E = scene(1, 2, 128 * 2 + 64)
    lib, call = emu_net.emu_lib, emu_net.emu_lib.call
    try:
        for mode, shared in (("f32rec", True), ("f32all", False)):
            emu_net.gemm_mode = mode
            names = []
            with mock.patch.object(lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1]):
                y = emu_net.forward_many(x, E, pad=False)
            assert (names.count("lh_proj_ln_res_fan") == 1) == shared, mode
            assert names.count("lh_stft_conv_in") + names.count("lh_ref32_stft_conv_in") == 1
            for k in range(2):
                yo = O.forward(cfg, sd, x, E[:, k:k + 1], pad=False)
                assert (y[0, k] - yo[0]).abs().max() < TOL, (mode, k)
    finally:
        emu_net.gemm_mode = "f16x3"


def test_forward_many_argument_errors(emu_net):
    x, E = scene(2, 2, 128 * 3 + 64)
    for bad in (E[:, 0], E[:1], E[:, :0]):
        with pytest.raises(ValueError):
            emu_net.forward_many(x, bad)
    emu_net._debug_taps = {}
    try:
        with pytest.raises(ValueError, match="taps"):
            emu_net.forward_many(x, E)
    finally:
        emu_net._debug_taps = None
