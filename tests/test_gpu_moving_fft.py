"""GPU: the moving-source renderer's partitioned overlap-save path — lh_bank_spectra (k_bank_spectra) and lh_render_moving_fft
(k_moving_fft, then lh_render_binaural's k_mix_peak / k_mix_apply) — called directly against the float64 form of the project's
own definition (tests/moving_fft_cases.py, tests/moving_render_cases.py), with guard regions around every output, the spectra
image and the scratch, bit-equality from call to call and for an utterance alone, and the C ABI's refusals.  No case passes an
out-of-range index (tests/test_emu_moving_fft.py does).
Run: pytest -m gpu tests/test_gpu_moving_fft.py -s (prints each error next to its bound).

k_moving_fft (1024-point transforms, a workgroup = one row and a run of RUN >= 25 frames, the last RING = (Q - 1) m + 1 block
spectra in LDS up to 16 and in the scratch beyond): frame 400 with N of frame - 1, frame, frame + 1 and N < frame under Lh > N; Lh
of 400, 401 and 700 (one full partition, one tap and a part of the second), 1025, 2100, 4001 and 4101 (a one-tap and a 101-tap
eleventh partition), 8192 (RING = 21: the scratch) and the limit 16384; frame 200 (m = 4), 104 (m = 8), 512 (the largest), 16
(m = 63) and 8 (m = 127; Lh 1017: one tap in the second partition, RING = 128); 263 frames whose every path point names another
entry; an N that spans two runs with the ring in LDS and with the ring in the scratch (the blocks in front of the second run are
real input); paths that alternate, that mix equal and unequal neighbours (the one-chain branch beside the two-chain one), more
points than needed, P = 1, K = 3 with a permuted bank_of, B of 1 .. 3, S1 of 1 .. 5, the noise row as a target, gains of about 20.
Every case is also held against lh_render_moving on the same inputs.  A constant path agrees with lh_render_binaural where that
is direct (Lh 700, 4101) and where it takes its own FFT path (Lh 1030, 2048); resting frames inside a moving path have the bits
of a run that never leaves their entry; a silent row stays exactly silent.

Measured on the first MI355X run: the events rows use at most 0.050 of their bound (B=3 S1=5 N=900 Lh=500: 1.88e-7 of 3.73e-6), the
two forms differ by at most 0.11 of twice the bound, a constant path differs from the static renderer by at most 0.15 of the
static bound (Lh = 700, where that one is direct) and the scene uses 0.032.  The whole output of that run:
profiles/moving_fft_errors.txt.
"""
import pytest
import torch

from lookoncetohear_amd import _cabi
from tests import moving_fft_cases as C
from tests.data_stage_cases import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rig():
    from lookoncetohear_amd.render import BinauralRenderer
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    return C.MovingFftRig(lib, DEV, torch.cuda.current_stream(DEV).cuda_stream, torch.cuda.synchronize, BinauralRenderer())


def _id(c):
    return "-".join(str(v) for v in c)


@pytest.mark.parametrize("case", C.FFT_MOVING, ids=_id)
def test_fft_against_float64(rig, case):
    check(rig.fft_case(*case, seed=sum(v for v in case if isinstance(v, int))), _id(case))


@pytest.mark.parametrize("case", C.FFT_LOUD, ids=_id)
def test_fft_peak_far_above_one(rig, case):
    res = rig.fft_case(*case, seed=7, gains=(15.0, 25.0))
    check(res, _id(case) + " loud")
    assert res["peak.value"][0] > 4.0


@pytest.mark.parametrize("case", C.FFT_CONST, ids=_id)
def test_constant_path_against_the_static_renderer(rig, case):
    check(rig.const_case(*case, seed=sum(case)), _id(case) + " const")


@pytest.mark.parametrize("case", C.FFT_RESTING, ids=_id)
def test_resting_frames_have_the_bits_of_a_constant_path(rig, case):
    assert rig.resting_case(*case, seed=sum(case)) >= 1


def test_silent_row_stays_silent(rig):
    rig.silent_row()


def test_fft_refusals(rig):
    rig.fft_refusals()


def test_scene_end_to_end(rig):
    check(rig.scene_fft_case(), "moving_scene(2, lh=1100) fft")
