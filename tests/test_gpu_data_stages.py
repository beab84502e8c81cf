"""GPU: lh_render_binaural (k_fir_causal, k_fft_conv, k_mix_peak, k_mix_apply) and lh_metric_sums (k_metric_moments,
k_metric_finish, k_metric_total) called directly against float64 (tests/data_stage_cases.py) at the smallest shapes that reach each
edge of their launch code, with guard regions around every output, bit-equality from call to call and for an utterance alone, and
the C ABI's refusals.  Full-size shapes stay with tests/test_render.py and tests/test_gpu_parity.py.
Run: pytest -m gpu tests/test_gpu_data_stages.py -s (prints each error next to its bound).

Renderer, direct form (FIR_TILE = 2048 outputs per workgroup, 8 per thread; 8-tap chunks, two per loop trip; FIR_KT = 2048 taps
per stage): Lh 1 .. 17 around one and two chunks, odd chunk counts, ragged tails at a late chunk and in the third and fourth
stage, the `lh_eff` skip with 1, 2 and 3 stages in one launch, N around one tile and N % 8 == 4 (vector store and scalar tail in
one workgroup), N < Lh.  FFT path (1024 <= Lh <= 4097, 4096 outputs per block, 5 blocks per workgroup): both ends of the range,
N of 1, 4096, 4097, a second workgroup holding one sample, 7 blocks, N < Lh.  S1 of 1, 2, 3, 5 and B of 1, 2, 3, every row with
its own gain, the noise row as a target, peaks below, at, one ulp above and far above 1.

Metric sums: n of 1 .. 65537 at B = 3, where the row bases take every alignment (the scalar loads of k_metric_moments run for
every n that is not a multiple of 4), B of 1, 4, 5, 9 (a wave of k_metric_finish that leaves beside waves that stay), emb_dim
around the 64 lanes, and nine signal classes.  Measured on the first MI355X run, B = 3, n = 4099 — d (distance of the kernel's
algebra, evaluated on the host, from the centred definition), the bound it gives and the device's error, each summed over the
three utterances, worse of sums[0] and sums[1]:
    class            d          bound      device error
    plain            6.0e-13    3.0e-09    1.8e-14
    dc               1.6e-09    2.6e-08    4.1e-12
    close            1.1e-05    1.8e-04    3.9e-07      (80 dB; rows within 3.6e-6 dB)
    equal            2.7e-13    3.0e-09    5.7e-14
    silent_target    7.1e-14    3.0e-09    0
    const_target     1.7e-02    3.0e-04    5.0e-05      (the cap; rows within 3.7e-5 dB: tt = sum tt - n mt^2 cancels to a few ulps of
                                                         n c^2 = 7e-13 next to eps = 1.2e-7)
    silent_output    1.7e-13    3.0e-09    7.1e-15
    x1e4             5.0e-13    3.0e-09    7.1e-15
    x1e-6            0          3.0e-09    0
Every other metric case (n, B, emb_dim sweeps on plain signals) has d below 2.1e-10 and a device error below 3.1e-11 over
its utterances.  The renderer's rows use at most 0.15 of their bound (B=1 S1=2 N=1100 Lh=1017).  The whole output of that run:
profiles/data_stage_errors.txt.
"""
import numpy as np
import pytest
import torch

from lookoncetohear_amd import _cabi
from tests import data_stage_cases as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rig():
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    return D.DataRig(lib, DEV, torch.cuda.current_stream(DEV).cuda_stream, torch.cuda.synchronize)


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
