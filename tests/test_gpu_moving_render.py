"""GPU: the moving-source renderer — lh_render_moving (k_fir_moving, then lh_render_binaural's k_mix_peak / k_mix_apply) and
lh_path_nearest (k_path_nearest) — called directly against the float64 form of the project's own definition
(tests/moving_render_cases.py; the reference project's native simulator is absent, nothing here is pinned to it), at the smallest
shapes that reach each edge of the launch code, with guard regions around every output, bit-equality from call to call and for
an utterance alone, and the C ABI's refusals.  No case passes an out-of-range index (tests/test_emu_moving_render.py does).
Run: pytest -m gpu tests/test_gpu_moving_render.py -s (prints each error next to its bound).

k_fir_moving (MV_R = 8 outputs per lane; a wave = one ear of one segment of at most MV_SEG = 512 outputs of ONE frame; a workgroup
= two consecutive segments x two ears; MV_KT = 1024 taps per LDS stage; 8-tap chunks, two per loop trip): frame 8, 16 and 400 with
N of 1, frame - 1, frame, frame + 1, several frames with a ragged last one and N % 8 == 4 (vector store and scalar tail in one
wave); an odd number of segments (an idle wave pair); frame 520, 1000 and 1024 (two segments per frame, whole and ragged); Lh of
1, 7, 8, 9, 16, 17 around one and two chunks, Lh > frame (the history spans frames that used other filters), Lh > N, Lh of 1000,
1024 and 1025 (direct where the static path turns to FFT; one tap in the second stage), 2100 and 4101 (three and five stages,
workgroups that skip to fewer); paths whose every point names another entry, that alternate between entries 0 and P - 1, that mix
equal and unequal neighbours inside one workgroup (the one-chain branch beside the two-chain one), more points than needed,
P = 1, K = 3 with a permuted bank_of, B of 1 .. 3, S1 of 1, 2, 3, 5, the noise row as a target, gains of about 20.
A constant path has the bits of lh_render_binaural at Lh of 1, 17, 200, 1000 and 4101 with N on both sides of a frame and of the
static kernel's 2048-sample tile, and agrees with its FFT path (Lh = 2048) within the static bound.
The blend weight is checked to the bit at frame 8, 16, 200, 400, 520 and 1024, and the frame-to-sample mapping and the ear order
by the host's moving-mode cue metric on a bank of pure delays.
k_path_nearest (one thread per point, PN_TILE = 1024 positions per LDS tile): P of 1, 63, 64, 65, 1025 and 1250, F of 1, 201
and 300 (a second workgroup), paths scaled by 1.5 and unscaled, a zero vector, duplicated positions.

Measured on the first MI355X run: the events rows use at most 0.14 of their bound (B=1 S1=2 N=2500 Lh=1025: 1.10e-6 of 7.90e-6), a
constant path differs from the static FFT path by 0.13 of the static bound, and no `nearest` case has an ambiguous point.  The
whole output of that run: profiles/moving_render_errors.txt.
"""
import pytest
import torch

from lookoncetohear_amd import _cabi
from tests import moving_render_cases as M
from tests.data_stage_cases import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rig():
    from lookoncetohear_amd.render import BinauralRenderer
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    return M.MovingRig(lib, DEV, torch.cuda.current_stream(DEV).cuda_stream, torch.cuda.synchronize, BinauralRenderer())


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
