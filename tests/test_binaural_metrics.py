"""CPU: the binaural cue errors (reference src/eval/binaural.py: itd_diff, ild_diff) — the torch fp64 restatement
`metrics.binaural_errors` against the committed fixture (tests/golden/binaural_golden.npz, scripts/make_binaural_golden.py)
and, where the reference checkout is importable, against the reference functions themselves; the lengths it refuses; and
`eval.evaluate(binaural=...)`: the extra row columns, the 64-byte all-reduce over a world-2 gloo group, and the unchanged
result of `binaural=None`."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from lookoncetohear_amd import synth
from lookoncetohear_amd.metrics import binaural_errors, binaural_lengths, binaural_sums
from tests.binaural_cases import CASES, inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "binaural_golden.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _close(a, b, tol):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=0, atol=tol,
                               equal_nan=True)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_golden(golden, case):
    assert json.loads(str(golden[case["name"] + "/params"])) == case      # the fixture was written for these inputs
    est, gt = inputs(case)
    rows, segs = binaural_errors(torch.from_numpy(est), torch.from_numpy(gt), case["sr"], case["moving"],
                                 return_segments=True)
    g = lambda k: golden[case["name"] + "/" + k]
    assert np.array_equal(segs["counted"].numpy(), g("counted"))
    assert np.array_equal(segs["itd_est"].numpy(), g("itd_est"))              # ITD of every segment: exact
    assert np.array_equal(segs["itd_gt"].numpy(), g("itd_gt"))
    _close(segs["ild_est"], g("ild_est"), 1e-9)
    _close(segs["ild_gt"], g("ild_gt"), 1e-9)
    _close(rows[:, 0], g("delta_itd"), 1e-9)
    _close(rows[:, 1], g("delta_ild"), 1e-9)


def test_golden_covers_masks_silence_and_ragged_frames(golden):
    assert not golden["synth_moving/counted"].all()                          # gated bursts: masked frames
    assert golden["synth_ragged_moving/counted"].shape[1] == 21              # ceil(81234 / 4000), last frame padded
    assert np.isnan(golden["silent_moving/delta_ild"]).all()                 # a counted silent estimate frame: NaN ILD
    assert np.isnan(golden["silent_static/delta_ild"][1])
    assert (golden["silent_static/itd_est"][1] == -1e3).all()               # all-zero cc: tau = -t_max (first maximum)
    assert (golden["synth_static/delta_itd"] != 0).sum() == 3                # the delayed right channels


def _reference():
    from oracle.ref_stubs import REFERENCE_ROOT
    path = os.path.join(REFERENCE_ROOT, "src", "eval", "binaural.py")
    if not os.path.exists(path):
        pytest.skip("the reference checkout is not on this machine")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        from make_binaural_golden import load_reference
    finally:
        sys.path.pop(0)
    return load_reference(REFERENCE_ROOT)


@pytest.mark.parametrize("sr,n,moving", [(16000, 20, False), (8000, 12, False), (16000, 6000, False), (8000, 8000, True),
                                         (8000, 9001, True), (16000, 13000, True), (12000, 7000, True)])
def test_restatement_matches_reference_functions(sr, n, moving):
    ref = _reference()
    g = torch.Generator().manual_seed(n + sr)
    gt = torch.randn(3, 2, n, generator=g, dtype=torch.float64) * torch.rand(3, 1, 1, generator=g, dtype=torch.float64)
    gt[1, :, : n // 2] *= 1e-5                                               # a quiet half: masked frames in moving mode
    est = gt.roll(2, dims=-1) * 0.7 + 0.05 * torch.randn(3, 2, n, generator=g, dtype=torch.float64)
    rows = binaural_errors(est, gt, sr, moving)
    e, t = est.numpy(), gt.numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        _close(rows[:, 0], ref.itd_diff(e, t, sr, moving=moving), 1e-9)
        _close(rows[:, 1], ref.ild_diff(e, t, sr, moving=moving), 1e-9)


def test_refused_lengths():
    x = torch.zeros(1, 2, 8001)
    with pytest.raises(ValueError):
        binaural_errors(x, x, 16000, moving=False)                           # odd clip, static
    binaural_errors(x, x, 16000, moving=True)                                # ... is fine in moving mode
    with pytest.raises(ValueError):
        binaural_errors(x, x, 8004, moving=True)                             # frame round(0.25 * 8004) = 2001
    with pytest.raises(ValueError):
        binaural_errors(x[..., :8000], x[..., :8000], 20000)                 # t_max 20 > 16
    with pytest.raises(ValueError):
        binaural_errors(x[..., :8000], x[..., :8000], 400)                   # t_max 0
    assert binaural_lengths(80000, 16000, True) == (16, 4000)
    assert binaural_lengths(40000, 8000, False) == (8, 0)


def test_binaural_sums_skip_non_finite_rows():
    rows = torch.tensor([[125.0, 1.5], [62.5, float("nan")], [0.0, float("inf")]], dtype=torch.float64)
    assert binaural_sums(rows).tolist() == [187.5, 3.0, 1.5, 1.0]


def _stand_in(m, e):
    return 0.6 * m


def test_evaluate_binaural_none_keeps_todays_keys():
    from lookoncetohear_amd.eval import evaluate
    res, rows = evaluate(_stand_in, lambda idx: synth.batch(idx, 1500), n_utts=3, batch_size=2)
    assert list(res) == ["si_snr_i", "output_sisnr", "embedding_sim", "n"]
    assert all(list(r) == ["idx", "output_sisnr", "si_snr_i", "embedding_sim"] for r in rows)
    res_b, rows_b = evaluate(_stand_in, lambda idx: synth.batch(idx, 1500), n_utts=3, batch_size=2, binaural="static")
    assert list(res_b) == list(res) + ["delta_itd_us", "delta_ild_db", "n_itd", "n_ild"]
    for k in res:                                                            # the SI-SNR half is unchanged
        assert res_b[k] == res[k]
    with pytest.raises(ValueError):
        evaluate(_stand_in, lambda idx: synth.batch(idx, 1500), n_utts=3, binaural="dynamic")


def test_evaluate_binaural_rows_and_silent_utterance():
    """Rows carry the restatement's values; a silent output (NaN ILD) is a metric value, not LH_ERR_RANGE."""
    from lookoncetohear_amd.eval import evaluate
    data_fn = lambda idx: synth.batch(idx, 9000)

    def model(m, e):
        y = 0.6 * m
        y[0, 1] = 0.0                                                        # first utterance of each batch: right channel off
        return y

    res, rows = evaluate(model, data_fn, n_utts=3, batch_size=2, binaural="moving")
    d = data_fn([0, 1, 2])
    want = torch.cat([binaural_errors(model(d["mixture"][:2], None), d["target"][:2], 16000, True),
                      binaural_errors(model(d["mixture"][2:], None), d["target"][2:], 16000, True)])
    got = torch.tensor([[r["delta_itd_us"], r["delta_ild_db"]] for r in rows], dtype=torch.float64)
    assert torch.equal(got.isfinite(), want.isfinite()) and torch.allclose(got.nan_to_num(), want.nan_to_num(), atol=0)
    assert torch.isinf(got[[0, 2], 1]).all()                                 # 10 log10(L^2 / 0) = inf: not finite
    assert res["n_itd"] == 3 and res["n_ild"] == 1
    assert res["delta_ild_db"] == float(want[1, 1])
    assert abs(res["delta_itd_us"] - float(want[:, 0].mean())) < 1e-9


WORKER = r"""
import os, sys, json, torch
sys.path.insert(0, %r)
import torch.distributed as dist
from lookoncetohear_amd import synth
from lookoncetohear_amd.eval import evaluate
torch.set_num_threads(2)
dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
agg, rows = evaluate(lambda m, e: 0.6 * m, lambda idx: synth.batch(idx, 9000), n_utts=5, batch_size=2, rank=rank,
                     world=world, dist=dist, all_rows=True, binaural="moving")
if rank == 0:
    print("RESULT " + json.dumps(agg))
print("ROWS%%d " %% rank + json.dumps(rows))
dist.destroy_process_group()
""" % ROOT


def test_world2_binaural_matches_world1(tmp_path):
    from lookoncetohear_amd.eval import evaluate
    ref, rows = evaluate(lambda m, e: 0.6 * m, lambda idx: synth.batch(idx, 9000), n_utts=5, batch_size=2,
                         binaural="moving")
    assert ref["n"] == 5 and ref["n_itd"] == 5 and len(rows) == 5
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29541", str(script)],
                         capture_output=True, text=True, env=dict(os.environ, MASTER_ADDR="127.0.0.1"), timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(re.search(r"RESULT (\{.*?\})", out.stdout).group(1))
    assert set(got) == set(ref)
    for k in ("n", "n_itd", "n_ild"):
        assert got[k] == ref[k], k
    for k in ("si_snr_i", "output_sisnr", "embedding_sim", "delta_itd_us", "delta_ild_db"):
        assert abs(got[k] - ref[k]) < 1e-9, (k, got[k], ref[k])
    for r in (0, 1):                                                         # the gathered table on every rank
        table = json.loads(re.search(r"ROWS%d (\[.*?\])" % r, out.stdout).group(1))
        assert [t["idx"] for t in table] == [0, 1, 2, 3, 4]
        for t, q in zip(table, sorted(rows, key=lambda q: q["idx"])):
            assert list(t) == list(q)
            for k in ("delta_itd_us", "delta_ild_db"):
                assert t[k] == q[k], (r, k, t, q)
