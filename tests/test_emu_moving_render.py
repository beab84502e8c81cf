"""CPU: the moving-source renderer (lh_render_moving, lh_path_nearest; tests/moving_render_cases.py) on the hipemu emulator — the
full tables of tests/test_gpu_moving_render.py with the same float64 references, bounds, guard regions and bit-equality checks —
and what only runs here: an out-of-range path index handed straight to the C ABI (clamped, never read outside the bank), and the
Python surface (`BinauralRenderer.nearest` / `render_moving` shape and range errors before any launch, `synth.moving_scene`)."""
import hashlib

import numpy as np
import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from tests import moving_render_cases as M
from tests.data_stage_cases import check, same_bits


@pytest.fixture(scope="module")
def rig():
    from tests.hipemu.build_emu import build_emu
    from tests.hipemu.hosts import EmuRenderer
    lib = _cabi.Lib(build_emu())
    r = EmuRenderer()
    r.emu_lib = lib
    return M.MovingRig(lib, "cpu", 0, renderer=r)


def _id(c):
    return "-".join(str(v) for v in c)


# ---- lh_render_moving
@pytest.mark.parametrize("case", M.MOVING, ids=_id)
def test_moving_against_float64(rig, case):
    check(rig.moving_case(*case, seed=sum(v for v in case if isinstance(v, int))), _id(case))


@pytest.mark.parametrize("case", M.MOVING_LOUD, ids=_id)
def test_moving_peak_far_above_one(rig, case):
    res = rig.moving_case(*case, seed=7, gains=(15.0, 25.0))
    check(res, _id(case) + " loud")
    assert res["peak.value"][0] > 4.0


@pytest.mark.parametrize("case", M.CONST, ids=_id)
def test_constant_path_has_the_static_renderers_bits(rig, case):
    assert rig.const_case(*case, seed=sum(case)) == {}


@pytest.mark.parametrize("case", M.CONST_FFT, ids=_id)
def test_constant_path_in_the_static_fft_range(rig, case):
    check(rig.const_case(*case, seed=sum(case)), _id(case) + " const")


@pytest.mark.parametrize("case", M.BLEND, ids=_id)
def test_blend_weight_is_the_fp32_quotient(rig, case):
    rig.blend_exact(*case)


def test_delays_found_by_the_cue_metric(rig):
    rig.delay_case()


def test_moving_refusals(rig):
    rig.moving_refusals()


def test_out_of_range_index_is_clamped(rig):
    """Emulator only: the C ABI clamps idx (and bank_of) into range where it reads them."""
    src, bank, bank_of, idx, gain, tgt = M.moving_inputs(3, 2, 2, 100, 9, 16, 4, 2, "mixed")
    bad, clamped = idx.clone(), idx.clone()
    for (b, s, f), v in (((0, 0, 1), -5), ((0, 1, 3), 4), ((1, 0, 0), 2 ** 31 - 1), ((1, 1, 7), -2 ** 31)):
        bad[b, s, f] = v
        clamped[b, s, f] = min(max(v, 0), 3)
    a = rig.moving_call(src, bank, bank_of, bad, gain, tgt, 16)
    b = rig.moving_call(src, bank, bank_of, clamped, gain, tgt, 16)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    a = rig.moving_call(src, bank, torch.tensor([-3, 9], dtype=torch.int32), idx, gain, tgt, 16)
    b = rig.moving_call(src, bank, torch.tensor([0, 1], dtype=torch.int32), idx, gain, tgt, 16)
    assert all(same_bits(x, y) for x, y in zip(a, b))


# ---- lh_path_nearest
@pytest.mark.parametrize("case", M.NEAREST, ids=_id)
def test_nearest_against_float64(rig, case):
    check(rig.nearest_case(*case, seed=sum(case)), _id(case))


def test_nearest_unscaled_paths(rig):
    check(rig.nearest_case(2, 2, 201, 64, 2, seed=5, scale=1.0), "scale 1")


def test_nearest_lowest_index_wins(rig):
    rig.nearest_ties()


def test_nearest_refusals(rig):
    rig.nearest_refusals()


def test_scene_end_to_end(rig):
    check(rig.scene_case(), "moving_scene(2)")


# ---- Python surface
class _NoLaunch:
    def call(self, *a):
        raise AssertionError("launched: " + a[0])


def _args():
    src, bank, bank_of, idx, gain, tgt = M.moving_inputs(1, 2, 3, 100, 9, 16, 4, 2, "mixed")
    return dict(srcs=src, bank=bank, bank_of=bank_of, idx=idx, gains=gain, tgt_idx=tgt, frame=16)


def test_render_moving_refuses_before_launching(rig):
    from tests.hipemu.hosts import EmuRenderer
    r = EmuRenderer()
    r.emu_lib = _NoLaunch()
    good = _args()
    bad_shapes = [("srcs", good["srcs"][0]), ("bank", good["bank"][0]), ("bank", good["bank"][:, :, :1]),
                  ("idx", good["idx"][:, :, :-1]), ("idx", good["idx"][:, :2]), ("idx", good["idx"][0]),
                  ("gains", good["gains"][:, :2]), ("tgt_idx", good["tgt_idx"][:1]), ("bank_of", good["bank_of"][:1]),
                  ("frame", 12), ("frame", 0)]
    for k, v in bad_shapes:
        with pytest.raises(ValueError):
            r.render_moving(**{**good, k: v})
    for k, pos, v in (("idx", (1, 2, 3), 4), ("idx", (0, 0, 0), -1), ("bank_of", (1,), 2), ("bank_of", (0,), -1),
                      ("tgt_idx", (0,), 3), ("tgt_idx", (1,), -1)):
        t = good[k].clone()
        t[pos] = v
        with pytest.raises(IndexError):
            r.render_moving(**{**good, k: t})
    paths, positions = torch.randn(2, 3, 5, 3), torch.randn(2, 4, 3)
    for p, q, bo in ((paths[0], positions, good["bank_of"]), (paths[..., :2], positions, good["bank_of"]),
                     (paths, positions[0], good["bank_of"]), (paths, positions, good["bank_of"][:1])):
        with pytest.raises(ValueError):
            r.nearest(p, q, bo)
    with pytest.raises(IndexError):
        r.nearest(paths, positions, torch.tensor([0, 2], dtype=torch.int32))
    with pytest.raises(AssertionError, match="launched: lh_render_moving"):       # the good call does reach the library
        r.render_moving(**good)


def test_render_moving_matches_the_c_abi(rig):
    good = _args()
    mx, tg, pk, ev = rig.renderer.render_moving(**good)
    want = rig.moving_call(good["srcs"], good["bank"], good["bank_of"], good["idx"], good["gains"], good["tgt_idx"], 16)
    assert all(same_bits(a, b) for a, b in zip((ev, pk, mx, tg), want))


def test_product_class_refuses_host_tensors():
    from lookoncetohear_amd.render import BinauralRenderer
    good = _args()
    with pytest.raises(RuntimeError, match="no CPU"):
        BinauralRenderer().render_moving(**good)
    with pytest.raises(RuntimeError, match="no CPU"):
        BinauralRenderer().nearest(torch.randn(2, 3, 5, 3), torch.randn(2, 4, 3), good["bank_of"])


def _digest(arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_moving_scene_is_deterministic_and_in_contract():
    a, b, c = synth.moving_scene(4, n=8000), synth.moving_scene(4, n=8000), synth.moving_scene(5, n=8000)
    keys = ("srcs", "bank", "positions", "paths", "gains")
    assert _digest(a[k] for k in keys) == _digest(b[k] for k in keys) != _digest(c[k] for k in keys)
    assert a["tgt_idx"] == b["tgt_idx"] and 0 <= a["tgt_idx"] < 3
    assert a["srcs"].shape == (4, 8000) and a["bank"].shape == (72, 2, 64) and a["positions"].shape == (72, 3)
    assert a["paths"].shape == (4, 21, 3) and a["gains"].shape == (4,) and all(v.dtype == np.float32 for v in (a[k] for k in keys))
    assert np.allclose(np.linalg.norm(a["positions"], axis=1), 1.0, atol=1e-6)
    assert np.allclose(np.linalg.norm(a["paths"], axis=2), synth.PATH_RADIUS, atol=1e-5)
    # the inter-aural delay (first tap above half the largest, per ear) stays at or below 16 samples and follows the azimuth
    onset = (np.abs(a["bank"]) > 0.5 * np.abs(a["bank"]).max(2, keepdims=True)).argmax(2)          # [P][2]
    itd = onset[:, 1] - onset[:, 0]
    assert np.abs(itd).max() <= 16 and itd[18] >= 15 and itd[54] <= -15 and abs(itd[0]) <= 1 and abs(itd[36]) <= 1
    assert np.abs(np.diff(itd)).max() <= 3
    # the three laws of motion: steady, rests and moves, jitter straight ahead; the bed stands still
    s = synth.moving_scene(5)
    az = np.unwrap(np.arctan2(s["paths"][..., 1], s["paths"][..., 0]).astype(np.float64), axis=1)
    v = np.diff(az, axis=1) / 0.025
    assert np.pi / 6 - 1e-3 <= abs(v[0]).min() and abs(v[0]).max() <= np.pi / 2 + 1e-3 and np.ptp(v[0]) < 1e-3
    assert (np.abs(v[1]) < 1e-4).any() and (np.abs(v[1]) > np.pi / 6 - 1e-3).any() and np.abs(v[1]).max() <= np.pi / 2 + 1e-3
    assert np.abs(az[2]).max() < np.radians(20) and np.abs(v[2]).max() > 0
    assert np.abs(v[3]).max() < 1e-4


def test_utterance_is_unchanged():
    """synth.utterance feeds bench.py: the bytes of utterance 3 as the commit before moving_scene made them."""
    assert _digest(synth.utterance(3)) == "a635ea1ef41e6047a54086bb7a353eb413df7466a9366ec256607b61804fc886"
