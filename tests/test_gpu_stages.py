"""GPU: every separator stage entry point of include/lookonce_hip.h against its float64 restatement (tests/stage_cases.py) over
the batch / frame counts where the launch shape changes, every `lh_set_tuning` variant of those stages, non-zero state in and
out, the T = 1 streaming ring over several wraps, utterances of far-apart scale in one call, windows at non-tile offsets, and
guard regions around every output.  Run: pytest -m gpu tests/test_gpu_stages.py -s (prints each error next to its bound)."""
import pytest
import torch

from lookoncetohear_amd import _cabi
from lookoncetohear_amd.net import Net
from oracle import tfgridnet_oracle as O
from tests.stage_cases import Rig, check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BS = [1, 2, 3, 5, 8]
TS = [1, 2, 15, 16, 17, 31, 32, 33, 39, 40, 41, 49, 50, 51, 97]
RANGE = [1e-6, 1e4, 1.0, 3e-3, 250.0, 0.5, 1e-2, 7.0]          # per-utterance input scales: B utterances take the first B


@pytest.fixture(scope="module")
def rig(oracle_cfg_sd):
    _, sd = oracle_cfg_sd
    net = Net(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    return Rig(lib, net, DEV, torch.cuda.current_stream(DEV).cuda_stream, torch.cuda.synchronize)


@pytest.mark.parametrize("B", BS)
def test_front_end_and_speaker_gain(rig, B):
    for T in TS:
        check(rig.stft_conv_in(B, T, RANGE[:B]), f"B={B} T={T}")
    check(rig.embed_proj_ln(B), f"B={B}")


@pytest.mark.parametrize("B", BS)
def test_intra_kernels(rig, B):
    for T in TS:
        check(rig.intra(B, T, stream=B * T <= 128), f"B={B} T={T}")


@pytest.mark.parametrize("B", BS)
def test_inter_kernels(rig, B):
    for T in TS:
        check(rig.inter(B, T), f"B={B} T={T}")


@pytest.mark.parametrize("B", BS)
def test_qkv_ring_pack_unpack(rig, B):
    for T in TS:
        check(rig.qkv_ring(B, T, RANGE[:B]), f"B={B} T={T}")


@pytest.mark.parametrize("B", BS)
def test_local_attention_every_query_tile(rig, B):
    for T in TS:
        for mq in (0, 1, 2, 3):
            check(rig.local_attn(B, T, mq), f"B={B} T={T}")


@pytest.mark.parametrize("B", BS)
def test_proj_ln_res_with_and_without_gain(rig, B):
    for T in TS:
        for gain in (True, False):
            check(rig.proj_ln_res(B, T, RANGE[:B], gain), f"B={B} T={T}")


@pytest.mark.parametrize("B", BS)
def test_deconv_istft_state_and_runs(rig, B):
    for T in TS:
        for runs in (0, 1):
            check(rig.deconv_istft(B, T, RANGE[:B], runs), f"B={B} T={T}")


def test_deconv_istft_oversubscribed_grid(rig):
    """B > 256: more runs than the 256 workgroups of the grid."""
    scales = (RANGE * 38)[:300]
    for T in (1, 2, 17):
        for runs in (0, 1):
            check(rig.deconv_istft(300, T, scales, runs), f"B=300 T={T}")


def test_realistic_size(rig):
    """B = 32, T = 625: the automatic choices of the big launches (attention mq = 3, deconv runs 256 / B)."""
    B, T = 32, 625
    scales = (RANGE * 4)[:B]
    check(rig.stft_conv_in(B, T, scales), "B=32 T=625")
    check(rig.intra(B, T, stream=False), "B=32 T=625")
    check(rig.inter(B, T, matvec=False), "B=32 T=625")
    check(rig.qkv_ring(B, T, scales), "B=32 T=625")
    for mq in (0, 2, 3):
        check(rig.local_attn(B, T, mq), "B=32 T=625")
    check(rig.proj_ln_res(B, T, scales, True), "B=32 T=625")
    check(rig.deconv_istft(B, T, scales, 0), "B=32 T=625")


@pytest.mark.parametrize("B", [1, 3])
def test_windows_at_non_tile_offsets(rig, B):
    for T, t0, Tc in ((64, 17, 23), (97, 33, 41)):
        case = f"B={B} T={T} t0={t0} Tc={Tc}"
        check(rig.intra_win(B, T, t0, Tc), case)
        check(rig.inter_win(B, T, t0, Tc), case)
        for mq in (0, 1, 2, 3):
            check(rig.qkv_attn_win(B, T, t0, Tc, mq), case)
        check(rig.proj_ln_res(B, T, RANGE[:B], True, win=(t0, Tc)), case)
        check(rig.proj_ln_res(B, T, RANGE[:B], False, win=(t0, Tc)), case)


@pytest.mark.parametrize("B", [1, 3])
def test_streaming_ring_wraps(rig, B):
    check(rig.stream_ring(B, 125), f"B={B} 125 steps")
