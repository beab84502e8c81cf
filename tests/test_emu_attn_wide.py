"""CPU: the 79-frame attention tile (lh_set_tuning(4, 5)) on the hipemu emulator — the cases of tests/test_gpu_attn_wide.py
(tests/attn_wide_cases.py) at B = 1: T = 80 (a full tile and a one-row tail) and T = 50 (one partial tile), zero and packed
history, against float64 at the `local_attn` bound of tests/stage_cases.py; the tile-length query; and the time windows of a batch-32
forward, which must fall on the boundaries of the tile the library says it uses."""
import ctypes

import pytest

from lookoncetohear_amd import _cabi
from oracle import tfgridnet_oracle as O
from tests.attn_wide_cases import TQ, WIDE, wide_case
from tests.hipemu.hosts import EmuNet
from tests.stage_cases import Rig, check, rel_err


@pytest.fixture(scope="module")
def rig(oracle_cfg_sd):
    from tests.hipemu.build_emu import build_emu
    _, sd = oracle_cfg_sd
    net = EmuNet(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net.emu_lib = _cabi.Lib(build_emu())
    rig = Rig(net.emu_lib, net, "cpu", 0)
    rig.net = net
    return rig


@pytest.mark.parametrize("T,hist", [(80, True), (50, False)])
def test_wide_tile_against_float64(rig, T, hist):
    m, ref = wide_case(rig, 1, T, hist)
    check({f"local_attn.k4={WIDE}": rel_err(m.t, ref, 1)}, f"B=1 T={T} hist={hist}")


def test_tile_length_query(rig):
    lib = rig.lib

    def frames(B, T):
        f = ctypes.c_int(-1)
        lib.call("lh_attn_tile_frames", B, T, ctypes.addressof(f))
        return f.value

    assert [frames(1, 16), frames(1, 80), frames(14, 625), frames(30, 625), frames(32, 625)] == [16, 32, 40, 40, TQ]
    lib.call("lh_set_tuning", 4, WIDE)
    try:
        assert frames(1, 80) == TQ and frames(1, 16) == 16
    finally:
        lib.call("lh_set_tuning", 4, 0)
    assert lib.raw("lh_attn_tile_frames")(1, 0, None) == 1          # LH_ERR_ARG


def test_windows_fall_on_the_tiles_the_library_uses(rig):
    net = rig.net
    assert net._window_bounds(32, 625, 2) == [0, 4 * TQ, 625]
    assert net._window_bounds(32, 625, 3) == [0, 3 * TQ, 5 * TQ, 625]
    assert net._window_bounds(32, 625, 4) == [0, 2 * TQ, 4 * TQ, 6 * TQ, 625]
    assert net._window_bounds(14, 625, 2) == [0, 320, 625] and net._window_bounds(4, 625, 3) == [0, 224, 416, 625]
    rig.lib.call("lh_set_tuning", 4, 3)
    try:
        assert net._window_bounds(32, 625, 4) == [0, 160, 320, 480, 625]
    finally:
        rig.lib.call("lh_set_tuning", 4, 0)
