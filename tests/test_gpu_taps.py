"""GPU: the tap-product pair (`lh_proj_ln_res_taps` -> `lh_taps_istft`, ABI 26) on the MI355X — tests/taps_cases.py: the waveform
bits of `lh_proj_ln_res` -> `lh_deconv_istft` from the zero state at the tile, run, window and grid edges and over far-apart
ranges, P and the waveform against float64, the non-finite flag, the argument checks, and `Net.fuse_taps` on against off.
Run: pytest -m gpu tests/test_gpu_taps.py -s"""
import pytest
import torch

from lookoncetohear_amd import _cabi
from lookoncetohear_amd.net import Net
from oracle import tfgridnet_oracle as O
from tests import taps_cases as TC
from tests.forward_many_cases import scene
from tests.stage_cases import Rig, check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RANGE = [1e-6, 1e4, 1.0, 3e-3, 250.0, 0.5, 1e-2, 7.0]          # per-utterance input scales, as in tests/test_gpu_stages.py
# beyond the shared shapes: 513 and 1025 frames on the projection's grid of min(B T, 512) persistent workgroups, and more runs
# than the back end's 256 workgroups (a workgroup walks runs of several utterances, one tile and two tiles long)
GRID_SHAPES = [(3, 171, 0), (5, 205, 0), (300, 2, 0), (300, 17, 1)]


@pytest.fixture(scope="module")
def net(oracle_cfg_sd):
    assert torch.cuda.is_available()
    n = Net(**O.TSH_PARAMS).eval()
    n.load_state_dict(oracle_cfg_sd[1], strict=True)
    return n.to(DEV)


@pytest.fixture(scope="module")
def rig(net):
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    return Rig(lib, net, DEV, torch.cuda.current_stream(DEV).cuda_stream, torch.cuda.synchronize)


@pytest.mark.parametrize("B,T,runs", TC.SHAPES + GRID_SHAPES)
def test_pair_bits(rig, B, T, runs):
    TC.pair_bits(rig, B, T, runs)


def test_pair_bits_windows(rig):
    TC.pair_bits(rig, 2, 20, 0, wins=((0, 8), (8, 12)))


def test_range_bits(rig):
    TC.range_bits(rig)


def test_against_float64(rig):
    for B, T in ((3, 17), (8, 46)):
        for runs in (0, 1):
            check(TC.against_float64(rig, B, T, RANGE[:B], runs), f"B={B} T={T}")


def test_nonfinite_flag(rig):
    TC.nonfinite(rig)


def test_argument_errors(rig):
    TC.arg_errors(rig)


def test_net_fuse_taps_on_against_off(net):
    """B = 2: 1 s clips (124 frames, one window) and 2 s clips cut into two windows on two streams — `fuse_taps` on gives the bits
    of off."""
    for n, chunks in ((16000, 0), (32000, 2)):
        x, E = scene(2, 1, n)
        x, E = x.to(DEV), E.to(DEV)
        keep = net.time_chunks_small
        try:
            net.time_chunks_small = chunks
            assert net._n_time_chunks(2, (n - 192) // 128 + 1, 1) == max(chunks, 1)
            net.fuse_taps = True
            y_on = net(x, E, pad=False)
            net.fuse_taps = False
            y_off = net(x, E, pad=False)
        finally:
            net.fuse_taps, net.time_chunks_small = True, keep
        torch.cuda.synchronize()
        assert net.range_status(DEV) == 0
        assert TC.same_bits(y_on, y_off), (n, float((y_on - y_off).abs().max()))
