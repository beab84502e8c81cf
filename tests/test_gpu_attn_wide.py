"""GPU: the 79-frame attention tile (k_local_attn<5, 2, 79>: five MFMA row tiles, 128 key rows, whole tile products per wave),
forced with lh_set_tuning(4, 5) at shapes far below its automatic threshold — tests/attn_wide_cases.py.  Against the float64
reference at the `local_attn` bound of tests/stage_cases.py; a window on a tile boundary, both cache-policy instantiations and a
rerun bit for bit; the forced forms 1..3 against the digests recorded before this form existed; and the tile-length query.
Run: pytest -m gpu tests/test_gpu_attn_wide.py -s (prints each error next to its bound)."""
import json
import os

import pytest
import torch

from lookoncetohear_amd import _cabi
from lookoncetohear_amd.net import Net
from oracle import tfgridnet_oracle as O
from tests.attn_wide_cases import SHAPES, TQ, WIDE, forced_digests, wide_case
from tests.stage_cases import Rig, check, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_forced_forms.json")


@pytest.fixture(scope="module")
def rig(oracle_cfg_sd):
    _, sd = oracle_cfg_sd
    net = Net(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    return Rig(lib, net, DEV, torch.cuda.current_stream(DEV).cuda_stream, torch.cuda.synchronize)


@pytest.mark.parametrize("B", [1, 3])            # 4 heads; 12 heads: the grid is padded to 16 and four workgroups leave at once
@pytest.mark.parametrize("hist", [False, True])
def test_wide_tile_against_float64(rig, B, hist):
    for T in SHAPES:
        m, ref = wide_case(rig, B, T, hist)
        check({f"local_attn.k4={WIDE}": rel_err(m.t, ref, B)}, f"B={B} T={T} hist={hist}")


def test_window_on_a_tile_boundary_is_the_whole_clip(rig):
    B, T = 3, 159
    gen = rig.gen.get_state()
    whole, _ = wide_case(rig, B, T, True)
    rig.gen.set_state(gen)                       # the same inputs again
    part, ref = wide_case(rig, B, T, True, win=(TQ, T - TQ))
    assert torch.equal(part.t[:, TQ:], whole.t[:, TQ:])
    check({f"local_attn_win.k4={WIDE}": rel_err(part.t[:, TQ:], ref[:, TQ:], B)}, f"B={B} T={T} t0={TQ} Tc={T - TQ}")


@pytest.mark.parametrize("B", [1, 3])
def test_cache_policy_and_rerun_bit_identical(rig, B):
    T = 159
    gen = rig.gen.get_state()
    outs = []
    for nt in (0, 2, 2):
        rig.gen.set_state(gen)
        outs.append(wide_case(rig, B, T, True, nt=nt)[0].t.clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


def test_forced_forms_1_to_3_give_what_they_gave(rig):
    want = json.load(open(GOLDEN))
    got = forced_digests(rig.lib, DEV, rig.st, rig.sync)
    assert got == want["digests"], (got, want)
    # and they still meet the reference at these shapes (B = 3, T = 159: ten, five and four tiles)
    for mq in (1, 2, 3):
        m, ref = wide_case(rig, 3, 159, True, mq=mq)
        check({f"local_attn.k4={mq}": rel_err(m.t, ref, 3)}, "B=3 T=159")


def test_tile_length_query_and_automatic_choice(rig):
    import ctypes
    lib = rig.lib

    def frames(B, T):
        f = ctypes.c_int(-1)
        lib.call("lh_attn_tile_frames", B, T, ctypes.addressof(f))
        return f.value

    # automatic: one tile up to 16 frames; 32; 40 above 512 workgroups of 32; 79 from two full rounds (1024) of those
    assert [frames(1, 1), frames(1, 16), frames(1, 17), frames(3, 625), frames(8, 625)] == [16, 16, 32, 32, 40]
    assert [frames(24, 625), frames(30, 625), frames(32, 625), frames(32, 553), frames(64, 300)] == [40, 40, 79, 40, 79]
    for v, f in ((1, 16), (2, 32), (3, 40), (WIDE, TQ)):
        lib.call("lh_set_tuning", 4, v)
        try:
            assert frames(3, 159) == f and frames(3, 16) == 16
        finally:
            lib.call("lh_set_tuning", 4, 0)
    assert lib.raw("lh_attn_tile_frames")(0, 5, None) == 1 and lib.raw("lh_set_tuning")(4, 4) == 1 and lib.raw("lh_set_tuning")(4, 6) == 1      # LH_ERR_ARG
    # below the threshold the automatic launch IS the 32-frame form's
    gen = rig.gen.get_state()
    a = wide_case(rig, 3, 159, True, mq=0)[0].t.clone()
    rig.gen.set_state(gen)
    assert torch.equal(a, wide_case(rig, 3, 159, True, mq=2)[0].t)
