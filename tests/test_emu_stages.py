"""CPU: the stage cases of tests/test_gpu_stages.py (tests/stage_cases.py) on the hipemu emulator at tiny shapes — the same
entry points, variants, state, ring, range, window and guard checks against float64, with the same bounds."""
import pytest

from lookoncetohear_amd import _cabi
from oracle import tfgridnet_oracle as O
from tests.hipemu.hosts import EmuNet
from tests.stage_cases import Rig, check

RANGE = [1e-6, 1e4, 1.0]


@pytest.fixture(scope="module")
def rig(oracle_cfg_sd):
    from tests.hipemu.build_emu import build_emu
    _, sd = oracle_cfg_sd
    net = EmuNet(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    return Rig(_cabi.Lib(build_emu()), net, "cpu", 0)


def test_front_end_and_speaker_gain(rig):
    for T in (1, 17):
        check(rig.stft_conv_in(3, T, RANGE), f"B=3 T={T}")
    check(rig.embed_proj_ln(3), "B=3")


def test_intra_kernels(rig):
    check(rig.intra(1, 2), "B=1 T=2")


def test_inter_kernels(rig):
    check(rig.inter(1, 3), "B=1 T=3")


def test_qkv_ring_pack_unpack(rig):
    check(rig.qkv_ring(3, 2, RANGE), "B=3 T=2")


def test_local_attention_every_query_tile(rig):
    for mq in (0, 1, 2, 3):
        check(rig.local_attn(1, 17, mq), "B=1 T=17")
    check(rig.local_attn(3, 1, 0), "B=3 T=1")


def test_proj_ln_res_with_and_without_gain(rig):
    for gain in (True, False):
        check(rig.proj_ln_res(3, 2, RANGE, gain), "B=3 T=2")


def test_deconv_istft_state_and_runs(rig):
    for runs in (0, 1):
        check(rig.deconv_istft(3, 17, RANGE, runs), "B=3 T=17")


def test_windows_at_non_tile_offsets(rig):
    check(rig.intra_win(1, 20, 17, 3), "B=1 T=20 t0=17 Tc=3")
    check(rig.inter_win(1, 24, 17, 5), "B=1 T=24 t0=17 Tc=5")
    check(rig.qkv_attn_win(1, 41, 17, 23, 2), "B=1 T=41 t0=17 Tc=23")
    check(rig.proj_ln_res(3, 41, RANGE, True, win=(17, 23)), "B=3 T=41 t0=17 Tc=23")


def test_streaming_ring_wraps(rig):
    check(rig.stream_ring(1, 55), "B=1 55 steps")
