"""CPU: the tap-product pair (`lh_proj_ln_res_taps` -> `lh_taps_istft`, ABI 26) on the hipemu emulator — tests/taps_cases.py:
the waveform bits of the pair it replaces at the tile / run / window edges and over far-apart ranges, P and the waveform
against float64, the non-finite flag, the argument checks, and `Net.fuse_taps` on the host class: the same bits as the
unfused forward (whole clip and time windows), `forward_many(K = 1) == forward`, and no new entry point when stage taps are set
or a state is passed."""
from unittest import mock

import pytest
import torch

from lookoncetohear_amd import _cabi
from oracle import tfgridnet_oracle as O
from tests import taps_cases as TC
from tests.forward_many_cases import scene
from tests.hipemu.hosts import EmuNet
from tests.stage_cases import Rig, check

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


@pytest.mark.parametrize("B,T,runs", TC.SHAPES)
def test_pair_bits(rig, B, T, runs):
    TC.pair_bits(rig, B, T, runs)


def test_pair_bits_windows(rig):
    TC.pair_bits(rig, 2, 20, 0, wins=((0, 8), (8, 12)))


def test_range_bits(rig):
    TC.range_bits(rig)


def test_against_float64(rig):
    for runs in (0, 1):
        check(TC.against_float64(rig, 3, 17, RANGE, runs), "B=3 T=17")


def test_nonfinite_flag(rig):
    TC.nonfinite(rig)


def test_argument_errors(rig):
    TC.arg_errors(rig)


def _calls(net, fn):
    lib, call = net.emu_lib, net.emu_lib.call
    names = []
    with mock.patch.object(lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1]):
        out = fn()
    return out, names


def test_net_fuse_taps_whole_and_windows(emu_net):
    """B = 2, T = 7 on the fused block kernels (forced at this size): `fuse_taps` on against off, whole clip and in two windows of
    3 / 4 frames, and `forward_many` with one speaker against `forward`."""
    B, T = 2, 7
    x, E = scene(B, 1, 128 * T + 64)
    saved = {k: getattr(emu_net, k) for k in FORCED}
    try:
        emu_net.fuse_intra_min_frames, emu_net.stream_intra_max_frames, emu_net.inter_matvec_max_seqs = 8, 0, 0
        emu_net.time_chunks, emu_net.time_chunks_small, emu_net.chunk_min_frames = 1, 1, 64
        assert emu_net._n_time_chunks(B, T, 1) == 1
        y_on, n_on = _calls(emu_net, lambda: emu_net(x, E, pad=False))
        y_many = emu_net.forward_many(x, E, pad=False)
        emu_net.fuse_taps = False
        y_off, n_off = _calls(emu_net, lambda: emu_net(x, E, pad=False))
        emu_net.fuse_taps = True
        emu_net.time_chunks, emu_net.chunk_min_frames = 2, 2
        assert emu_net._n_time_chunks(B, T, 1) == 2
        y_win, n_win = _calls(emu_net, lambda: emu_net(x, E, pad=False))
    finally:
        emu_net.fuse_taps = True
        for k, v in saved.items():
            setattr(emu_net, k, v)
    assert n_on.count("lh_proj_ln_res_taps") == 1 and n_on.count("lh_taps_istft") == 1 and "lh_deconv_istft" not in n_on
    assert n_on.count("lh_proj_ln_res") == emu_net.n_blocks - 1
    assert not TC.NEW_ENTRY_POINTS & set(n_off) and n_off.count("lh_deconv_istft") == 1
    assert n_win.count("lh_proj_ln_res_taps_win") == 2 and n_win.count("lh_taps_istft") == 1 and "lh_deconv_istft" not in n_win
    assert TC.same_bits(y_on, y_off)
    assert TC.same_bits(y_win, y_off)
    assert TC.same_bits(y_many[:, 0], y_on)


def test_net_keeps_the_frame_for_taps_and_state(emu_net):
    """Stage taps want the last block's frame and a carried state wants the back end's state out: neither calls a new entry point."""
    x, E = scene(1, 1, 128 * 3 + 64)
    emu_net._debug_taps = {}
    try:
        _, names = _calls(emu_net, lambda: emu_net(x, E, pad=False))
    finally:
        emu_net._debug_taps = None
    assert not TC.NEW_ENTRY_POINTS & set(names) and names.count("lh_deconv_istft") == 1
    state = emu_net.init_buffers(1, "cpu")
    _, names = _calls(emu_net, lambda: emu_net.predict(x, E, state, pad=False))
    assert not TC.NEW_ENTRY_POINTS & set(names) and names.count("lh_deconv_istft") == 1
    _, names = _calls(emu_net, lambda: emu_net.predict(x, E, None, pad=False))          # zero state in, state out
    assert not TC.NEW_ENTRY_POINTS & set(names) and names.count("lh_deconv_istft") == 1
