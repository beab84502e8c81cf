"""CPU: the moving-source renderer's partitioned overlap-save path (lh_bank_spectra, lh_render_moving_fft;
tests/moving_fft_cases.py) on the hipemu emulator — the full tables of tests/test_gpu_moving_fft.py with the same float64
reference, bounds, guard regions and bit-equality checks — and what only runs here: an out-of-range path index handed straight to
the C ABI (clamped, never read outside the image), and the Python surface (`BinauralRenderer.bank_spectra`,
`render_moving(method=..., spectra=...)`: errors before any launch, "direct" unchanged, a cached image to the bit)."""
import pytest
import torch

from lookoncetohear_amd import _cabi, render
from tests import moving_fft_cases as C
from tests import moving_render_cases as M
from tests.data_stage_cases import check, same_bits


@pytest.fixture(scope="module")
def rig():
    from tests.hipemu.build_emu import build_emu
    from tests.hipemu.hosts import EmuRenderer
    lib = _cabi.Lib(build_emu())
    r = EmuRenderer()
    r.emu_lib = lib
    return C.MovingFftRig(lib, "cpu", 0, renderer=r)


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


def test_partition_formulas_match_the_host_code():
    for Lh in (1, 400, 401, 1016, 1017, 4096, 8192, C.LH_MAX):
        for frame in (8, 16, 104, 200, 400, 512):
            assert render.fft_partition(Lh, frame) == C.partition(Lh, frame), (Lh, frame)
            assert frame + C.partition(Lh, frame)[1] - 1 <= C.FZ
    assert (render.FFT_Z, render.FFT_LDS_RING, render.FFT_LH_MAX) == (C.FZ, C.LDS_RING, C.LH_MAX)
    assert C.partition(4096, 400)[2:4] == (11, 11) and C.partition(64, 8)[0] == 127 and C.partition(2048, 200)[0] == 4


def test_out_of_range_index_is_clamped(rig):
    """Emulator only: the C ABI clamps idx (and bank_of) into range where it reads them."""
    src, bank, bank_of, idx, gain, tgt = M.moving_inputs(3, 2, 2, 100, 1100, 16, 4, 2, "mixed")
    bad, clamped = idx.clone(), idx.clone()
    for (b, s, f), v in (((0, 0, 1), -5), ((0, 1, 3), 4), ((1, 0, 0), 2 ** 31 - 1), ((1, 1, 7), -2 ** 31)):
        bad[b, s, f] = v
        clamped[b, s, f] = min(max(v, 0), 3)
    a = rig.fft_call(src, bank, bank_of, bad, gain, tgt, 16)
    b = rig.fft_call(src, bank, bank_of, clamped, gain, tgt, 16)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    a = rig.fft_call(src, bank, torch.tensor([-3, 9], dtype=torch.int32), idx, gain, tgt, 16)
    b = rig.fft_call(src, bank, torch.tensor([0, 1], dtype=torch.int32), idx, gain, tgt, 16)
    assert all(same_bits(x, y) for x, y in zip(a, b))


# ---- Python surface
class _NoLaunch:
    def call(self, *a):
        raise AssertionError("launched: " + a[0])


def _args(Lh=9):
    src, bank, bank_of, idx, gain, tgt = M.moving_inputs(1, 2, 3, 100, Lh, 16, 4, 2, "mixed")
    return dict(srcs=src, bank=bank, bank_of=bank_of, idx=idx, gains=gain, tgt_idx=tgt, frame=16)


def test_method_and_spectra_errors_before_launching(rig):
    from tests.hipemu.hosts import EmuRenderer
    r = EmuRenderer()
    r.emu_lib = _NoLaunch()
    good = _args()
    spec = rig.renderer.bank_spectra(good["bank"], 16)
    assert tuple(spec.shape) == (2, 4, 1, C.FZ, 2)
    for m in ("FFT", "overlap", "", None):
        with pytest.raises(ValueError, match="method"):
            r.render_moving(**good, method=m)
    for bad in (spec[:1], spec[:, :, :, :512], spec.double(), spec.transpose(0, 1), rig.renderer.bank_spectra(good["bank"][..., :5], 16)[..., :1]):
        with pytest.raises(ValueError, match="spectra"):
            r.render_moving(**good, method="fft", spectra=bad)
    long = _args(Lh=1100)
    with pytest.raises(ValueError, match="spectra"):                     # the image of another frame: another Q
        r.render_moving(**long, method="fft", spectra=rig.renderer.bank_spectra(long["bank"], 400))
    with pytest.raises(ValueError, match="frame"):
        r.render_moving(**{**good, "frame": 520, "idx": good["idx"]}, method="fft")
    with pytest.raises(ValueError, match="frame"):
        r.bank_spectra(good["bank"], 12)
    with pytest.raises(ValueError, match="taps"):
        r.bank_spectra(torch.zeros(1, 1, 2, C.LH_MAX + 1), 400)
    with pytest.raises(ValueError, match="taps"):
        r.render_moving(torch.zeros(1, 1, 8), torch.zeros(1, 1, 2, C.LH_MAX + 1), torch.zeros(1, dtype=torch.int32),
                        torch.zeros(1, 1, 2, dtype=torch.int32), torch.ones(1, 1), torch.zeros(1, dtype=torch.int32), frame=8, method="fft")
    with pytest.raises(ValueError):
        r.bank_spectra(good["bank"][0], 16)
    with pytest.raises(AssertionError, match="launched: lh_render_moving_fft"):   # the good call does reach the library
        r.render_moving(**good, method="fft", spectra=spec)
    with pytest.raises(AssertionError, match="launched: lh_bank_spectra"):
        r.render_moving(**good, method="fft")
    with pytest.raises(AssertionError, match="launched: lh_render_moving$"):
        r.render_moving(**good, method="direct")


def test_direct_is_the_default_and_unchanged(rig):
    good = _args()
    want = rig.moving_call(good["srcs"], good["bank"], good["bank_of"], good["idx"], good["gains"], good["tgt_idx"], 16)
    for kw in ({}, {"method": "direct"}, {"method": "auto"}):          # (9 taps: far below the threshold of "auto")
        mx, tg, pk, ev = rig.renderer.render_moving(**good, **kw)
        assert all(same_bits(a, b) for a, b in zip((ev, pk, mx, tg), want)), kw


def test_fft_method_matches_the_c_abi_and_a_cached_image(rig):
    good = _args(Lh=1100)                                               # frame 16: RING = 64, the host allocates the scratch
    want = rig.fft_call(good["srcs"], good["bank"], good["bank_of"], good["idx"], good["gains"], good["tgt_idx"], 16)
    spec = rig.renderer.bank_spectra(good["bank"], 16)
    for kw in ({}, {"spectra": spec}):
        mx, tg, pk, ev = rig.renderer.render_moving(**good, method="fft", **kw)
        assert all(same_bits(a, b) for a, b in zip((ev, pk, mx, tg), want)), kw
    assert render.AUTO_FFT_MIN_LH >= 1024
    big = _args(Lh=max(render.AUTO_FFT_MIN_LH, 1100))                   # "auto" takes the FFT form from the threshold on
    a = rig.renderer.render_moving(**big, method="auto")
    b = rig.renderer.render_moving(**big, method="fft")
    assert all(same_bits(x, y) for x, y in zip(a, b))
    r = type(rig.renderer)()
    r.emu_lib = _NoLaunch()
    with pytest.raises(AssertionError, match="launched: lh_render_moving$"):      # ... and the direct one below it
        r.render_moving(**_args(Lh=render.AUTO_FFT_MIN_LH - 1), method="auto")
    with pytest.raises(AssertionError, match="launched: lh_bank_spectra"):
        r.render_moving(**_args(Lh=render.AUTO_FFT_MIN_LH), method="auto")


def test_product_class_refuses_host_tensors():
    from lookoncetohear_amd.render import BinauralRenderer
    good = _args()
    with pytest.raises(RuntimeError, match="no CPU"):
        BinauralRenderer().render_moving(**good, method="fft")
    with pytest.raises(RuntimeError, match="no CPU"):
        BinauralRenderer().bank_spectra(good["bank"], 16)
