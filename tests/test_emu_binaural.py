"""CPU: lh_binaural_cues (lookoncetohear_amd/csrc/lh_metrics.hip) on the hipemu emulator, driven through
`metrics.binaural_errors_device` with an `EmuHost`, against the FFT restatement `metrics.binaural_errors` on small shapes:
every segment's lag equal, ILDs and rows within 1e-9.  The GPU version is tests/test_gpu_binaural.py."""
import numpy as np
import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.metrics import binaural_errors, binaural_errors_device, binaural_sums
from tests.hipemu.hosts import EmuMetricHost


@pytest.fixture(scope="module")
def host():
    from tests.hipemu.build_emu import build_emu
    return EmuMetricHost(_cabi.Lib(build_emu()))


def _pair(n, seed, silent=False):
    gt = torch.stack([torch.from_numpy(synth.utterance(i, n)[1]) for i in (seed, seed + 1)])
    g = torch.Generator().manual_seed(seed)
    est = gt.clone()
    est[:, 1] = 0.7 * torch.roll(gt[:, 1], 3, dims=-1)
    est += 0.01 * torch.randn(est.shape, generator=g)
    if silent:
        est[0, :, 2000:4000] = 0.0                    # a silent estimate frame (counted: NaN ILD)
        est[1, 1] = 0.0                               # a silent right channel: inf ILD, cc = 0, tau = -t_max
    return est, gt


def _check(host, est, gt, sr, moving):
    rows, segs = binaural_errors(est, gt, sr, moving, return_segments=True)
    sums, rows_d, segs_d = binaural_errors_device(est, gt, sr, moving, host=host, return_segments=True)
    for k in ("tau_est", "tau_gt", "itd_est", "itd_gt", "counted"):
        assert torch.equal(segs_d[k], segs[k]), k
    for k in ("ild_est", "ild_gt"):
        np.testing.assert_allclose(segs_d[k].numpy(), segs[k].numpy(), rtol=0, atol=1e-9, equal_nan=True)
    np.testing.assert_allclose(rows_d.numpy(), rows.numpy(), rtol=0, atol=1e-9, equal_nan=True)
    bs = binaural_sums(rows_d)
    assert torch.equal(sums[1::2], bs[1::2]) and torch.allclose(sums[0::2], bs[0::2], rtol=0, atol=1e-9)
    return rows_d, segs_d


@pytest.mark.parametrize("n,moving,silent", [(8000, False, False), (8000, True, False), (8617, True, False),
                                             (8000, True, True), (8000, False, True), (12, False, False)])
def test_emulated_kernel_matches_restatement(host, n, moving, silent):
    est, gt = _pair(n, 20 + n % 7, silent)
    _check(host, est, gt, 8000, moving)


def test_row_does_not_depend_on_the_batch(host):
    est, gt = _pair(8617, 30)
    _, rows, segs = binaural_errors_device(est, gt, 8000, True, host=host, return_segments=True)
    _, r1, s1 = binaural_errors_device(est[1:], gt[1:], 8000, True, host=host, return_segments=True)
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t      # NaN ILDs of silent frames compare too
    assert torch.equal(bits(rows[1:]), bits(r1))
    assert all(torch.equal(bits(segs[k][1:]), bits(s1[k])) for k in segs)


def test_refused_lengths(host):
    x = torch.zeros(1, 2, 8001)
    with pytest.raises(ValueError):
        binaural_errors_device(x, x, 8000, moving=False, host=host)
    with pytest.raises(ValueError):
        binaural_errors_device(x, x, 17000, moving=True, host=host)
    # the C ABI refuses them by itself (LH_ERR_UNSUPPORTED = 2)
    raw = host.emu_lib.raw("lh_binaural_cues")
    scratch, rows, sums = torch.zeros(4096, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    p = (x.data_ptr(), x.data_ptr(), scratch.data_ptr(), rows.data_ptr(), sums.data_ptr())
    assert raw(*p, 1, 8001, 8000, 0, 1e-3, None) == 2            # odd clip, static
    assert raw(*p, 1, 8001, 8004, 2001, 1e-3, None) == 2         # odd frame
    assert raw(*p, 1, 8000, 17000, 0, 1e-3, None) == 2           # t_max 17
    assert raw(*p, 1, 8000, 400, 0, 1e-3, None) == 2             # t_max 0
