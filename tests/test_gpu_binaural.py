"""GPU: lh_binaural_cues (`metrics.binaural_errors_device`) against the FFT restatement `metrics.binaural_errors` on the
separator's outputs of a 32 x 5 s synthetic batch (est = output, gt = target), in both modes, and on the committed fixture
cases (tests/golden/binaural_golden.npz); bit-identical from call to call and for a row alone vs inside the batch; and
`eval.evaluate(net, ..., binaural="moving")` on the device path against the host restatement."""
import os

import numpy as np
import pytest
import torch

from lookoncetohear_amd import _cabi, config, synth
from lookoncetohear_amd.eval import evaluate
from lookoncetohear_amd.metrics import binaural_errors, binaural_errors_device, binaural_lengths, binaural_sums
from lookoncetohear_amd.net import Net
from tests.binaural_cases import CASES, inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = 16000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    t = t.cpu()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


@pytest.fixture(scope="module")
def net():
    assert torch.cuda.is_available()
    _cabi.load()
    m = Net(**config.TSH_PARAMS).eval()
    m.load_state_dict(config.separator_weights(0), strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def batch32(net):
    d = synth.batch(range(32), 80000)
    with torch.no_grad():
        y = net(d["mixture"].to(DEV), d["embedding_gt"].to(DEV))
    torch.cuda.synchronize()
    return y.contiguous(), d["target"].to(DEV)


def _near_tie(x, b, c, sr, frame, t_max):
    """True when the restatement's two largest |cc| of segment (b, c) of x [B, 2, N] lie within 1e-9 relative."""
    seg = x[b].double().cpu()
    if frame:
        seg = torch.nn.functional.pad(seg, (0, frame * (c + 1) - seg.shape[-1]))[:, c * frame:(c + 1) * frame]
    L = seg.shape[-1]
    corr = torch.fft.irfft(torch.fft.rfft(seg[0]) * torch.fft.rfft(seg[1]).conj(), n=L)
    t = min(t_max, L // 2)
    top = torch.cat([corr[L - t:], corr[:t + 1]]).abs().topk(2).values
    return bool(top[0] - top[1] <= 1e-9 * top[0])


def _compare(est, gt, sr, moving):
    """Device vs restatement; returns the number of segments whose lag differs at a near-tie of the restatement."""
    rows, segs = binaural_errors(est.cpu(), gt.cpu(), sr, moving, return_segments=True)
    sums, rows_d, segs_d = binaural_errors_device(est, gt, sr, moving, return_segments=True)
    t_max, frame = binaural_lengths(est.shape[-1], sr, moving)
    ties = 0
    for sig, x in (("est", est), ("gt", gt)):
        diff = (segs_d["tau_" + sig].cpu() != segs[f"tau_{sig}"]).nonzero().tolist()
        for b, c in diff:
            assert _near_tie(x, b, c, sr, frame, t_max), (sig, b, c)
        ties += len(diff)
    assert torch.equal(segs_d["counted"].cpu(), segs["counted"])
    for k in ("ild_est", "ild_gt"):
        np.testing.assert_allclose(segs_d[k].cpu().numpy(), segs[k].numpy(), rtol=0, atol=1e-9, equal_nan=True)
    if ties == 0:
        np.testing.assert_allclose(rows_d.cpu().numpy(), rows.numpy(), rtol=0, atol=1e-9, equal_nan=True)
    bs = binaural_sums(rows_d.cpu())
    assert torch.equal(sums.cpu()[1::2], bs[1::2]) and torch.allclose(sums.cpu()[0::2], bs[0::2], rtol=0, atol=1e-6)
    return ties, rows_d, segs_d


@pytest.mark.parametrize("moving", [False, True], ids=["static", "moving"])
def test_device_matches_restatement_on_separator_outputs(batch32, moving):
    est, gt = batch32
    ties, rows, _ = _compare(est, gt, SR, moving)
    assert ties == 0                       # lags that differ only where the restatement's top two |cc| tie within 1e-9
    assert torch.isfinite(rows[:, 0]).all()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_reproduces_golden(case):
    z = np.load(os.path.join(ROOT, "tests", "golden", "binaural_golden.npz"))
    g = lambda k: z[case["name"] + "/" + k]
    est, gt = (torch.from_numpy(a).to(DEV) for a in inputs(case))
    ties, rows, segs = _compare(est, gt, case["sr"], case["moving"])
    assert ties == 0
    assert np.array_equal(segs["itd_est"].cpu().numpy(), g("itd_est")) and np.array_equal(segs["itd_gt"].cpu().numpy(), g("itd_gt"))
    assert np.array_equal(segs["counted"].cpu().numpy(), g("counted"))
    np.testing.assert_allclose(rows[:, 0].cpu().numpy(), g("delta_itd"), rtol=0, atol=1e-9, equal_nan=True)
    np.testing.assert_allclose(rows[:, 1].cpu().numpy(), g("delta_ild"), rtol=0, atol=1e-9, equal_nan=True)


@pytest.mark.parametrize("moving", [False, True], ids=["static", "moving"])
def test_bit_identical_across_calls_and_batch_positions(batch32, moving):
    est, gt = batch32
    s1, r1, g1 = binaural_errors_device(est, gt, SR, moving, return_segments=True)
    s2, r2, g2 = binaural_errors_device(est, gt, SR, moving, return_segments=True)
    assert torch.equal(_bits(s1), _bits(s2)) and torch.equal(_bits(r1), _bits(r2))
    assert all(torch.equal(_bits(g1[k]), _bits(g2[k])) for k in g1)
    for b in range(est.shape[0]):
        _, rb, gb = binaural_errors_device(est[b:b + 1], gt[b:b + 1], SR, moving, return_segments=True)
        assert torch.equal(_bits(rb[0]), _bits(r1[b])), b
        assert all(torch.equal(_bits(gb[k][0]), _bits(g1[k][b])) for k in g1), b


def test_evaluate_binaural_on_device_matches_host_path(net):
    data_fn = lambda idx: synth.batch(idx, 80000)
    outs = []

    def model(m, e):
        y = net(m, e)
        outs.append(y.cpu())
        return y

    res, rows = evaluate(model, data_fn, n_utts=6, batch_size=4, device=DEV, binaural="moving")
    d = data_fn(range(6))
    want = binaural_errors(torch.cat(outs), d["target"], SR, moving=True)
    got = torch.tensor([[r["delta_itd_us"], r["delta_ild_db"]] for r in rows], dtype=torch.float64)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-9, equal_nan=True)
    s = binaural_sums(want)
    assert res["n_itd"] == int(s[1]) and res["n_ild"] == int(s[3]) and res["n"] == 6
    assert abs(res["delta_itd_us"] - float(s[0] / s[1])) < 1e-9 and abs(res["delta_ild_db"] - float(s[2] / s[3])) < 1e-9
