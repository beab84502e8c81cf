"""CPU: the renderer and metric-sum cases of tests/test_gpu_data_stages.py (tests/data_stage_cases.py) on the hipemu emulator —
the full tables (every case takes under a second here), the same float64 references, bounds, guard regions and bit-equality
checks."""
import numpy as np
import pytest

from lookoncetohear_amd import _cabi
from tests import data_stage_cases as D


@pytest.fixture(scope="module")
def rig():
    from tests.hipemu.build_emu import build_emu
    return D.DataRig(_cabi.Lib(build_emu()), "cpu", 0)


def _id(c):
    return "-".join(str(v) for v in c)


# ---- lh_render_binaural
@pytest.mark.parametrize("case", D.RENDER_DIRECT, ids=_id)
def test_render_direct_form(rig, case):
    D.check(rig.render_case(*case, seed=sum(case)), "B=%d S1=%d N=%d Lh=%d" % case)


@pytest.mark.parametrize("case", D.RENDER_FFT, ids=_id)
def test_render_fft_path(rig, case):
    D.check(rig.render_case(*case, seed=sum(case)), "B=%d S1=%d N=%d Lh=%d" % case)


@pytest.mark.parametrize("case", D.RENDER_LOUD, ids=_id)
def test_render_peak_far_above_one(rig, case):
    res = rig.render_case(*case, seed=sum(case), gains=(15.0, 25.0))
    D.check(res, "B=%d S1=%d N=%d Lh=%d loud" % case)
    assert res["peak.value"][0] > 4.0


@pytest.mark.parametrize("Lh", [1, 8])
def test_render_normalisation_threshold(rig, Lh):
    rig.render_threshold(1.0, Lh)
    rig.render_threshold(float(np.nextafter(np.float32(1), np.float32(2))), Lh)


def test_render_refusals(rig):
    rig.render_refusals()


# ---- lh_metric_sums
@pytest.mark.parametrize("n", D.METRIC_N)
def test_metric_lengths_and_row_alignments(rig, n):
    D.check(rig.metric_case(3, n, seed=n), f"B=3 n={n}")


@pytest.mark.parametrize("B", D.METRIC_B)
def test_metric_batch_sizes(rig, B):
    D.check(rig.metric_case(B, 1001, seed=B), f"B={B} n=1001")


@pytest.mark.parametrize("E", D.METRIC_E)
def test_metric_embedding_widths(rig, E):
    D.check(rig.metric_case(3, 1001, E, seed=E), f"B=3 n=1001 emb_dim={E}")


@pytest.mark.parametrize("kind", D.SIGNALS)
def test_metric_signal_classes(rig, kind):
    D.check(rig.metric_case(3, 4099, kind=kind, seed=7), f"B=3 n=4099 {kind}")


def test_metric_refusals(rig):
    rig.metric_refusals()
