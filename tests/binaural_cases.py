"""Inputs of the binaural cue fixture (tests/golden/binaural_golden.npz, written by scripts/make_binaural_golden.py).

No waveform is stored: each case is a small parameter dict, saved in the fixture next to the expected outputs, and
`inputs(case)` regenerates its (est, gt) float32 arrays [B, 2, N] from it.
  kind "synth"  targets `synth.utterance(idx, n)[1]` (their gated bursts give silent, masked frames); the estimate is the
                target with its right channel delayed by `delay` samples (zero-filled; negative = advanced), scaled by `gain`,
                plus seeded white noise of std `noise`.  `silence`: [utterance, start, stop) spans of the estimate set to 0.
  kind "chirp"  the reference's own demo (src/eval/binaural.py `test`): 8 kHz, 5 s chirp, right channel = left rolled by
                -shift and halved, shifts -4 .. 4, estimate = target + N(0, 0.1^2) from np.random.seed(0).
"""
import numpy as np

CASES = [
    dict(name="synth_static", kind="synth", sr=16000, n=80000, moving=False, idx=[0, 1, 2, 3], delay=[0, 2, -3, 5],
         gain=[1.0, 0.8, 1.25, 0.5], noise=0.01, seed=7),
    dict(name="synth_moving", kind="synth", sr=16000, n=80000, moving=True, idx=[0, 1, 2, 3], delay=[0, 2, -3, 5],
         gain=[1.0, 0.8, 1.25, 0.5], noise=0.01, seed=7),
    dict(name="synth_ragged_moving", kind="synth", sr=16000, n=81234, moving=True, idx=[4, 5], delay=[1, -7],
         gain=[0.9, 1.1], noise=0.003, seed=11),
    dict(name="chirp_static", kind="chirp", sr=8000, n=40000, moving=False),
    dict(name="chirp_moving", kind="chirp", sr=8000, n=40000, moving=True),
    # utterance 0: one silent estimate frame (a counted frame whose ILD is NaN); utterance 1: an all-silent estimate
    dict(name="silent_moving", kind="synth", sr=16000, n=32000, moving=True, idx=[6, 7], delay=[3, 0], gain=[1.0, 1.0],
         noise=0.0, seed=3, silence=[[0, 8000, 12000], [1, 0, 32000]]),
    dict(name="silent_static", kind="synth", sr=16000, n=32000, moving=False, idx=[6, 7], delay=[3, 0], gain=[1.0, 1.0],
         noise=0.0, seed=3, silence=[[0, 8000, 12000], [1, 0, 32000]]),
]


def _delay(x: np.ndarray, k: int) -> np.ndarray:
    y = np.zeros_like(x)
    if k >= 0:
        y[k:] = x[:len(x) - k]
    else:
        y[:k] = x[-k:]
    return y


def inputs(case: dict):
    """(est, gt) float32 [B, 2, N] of one case."""
    if case["kind"] == "chirp":
        sr, T = case["sr"], case["n"] // case["sr"]
        np.random.seed(0)
        gts, ests = [], []
        for shift in range(-4, 5):
            t = np.arange(0, T, 1 / sr)
            x = np.cos(2 * np.pi * (100 + 250 * t) * t)[None]
            g = np.concatenate([x, np.roll(x, -shift) * 0.5], axis=0) * 0.1
            gts.append(g)
            ests.append(g + np.random.normal(0, 1, size=g.shape) * 0.1)
        return np.array(ests).astype(np.float32), np.array(gts).astype(np.float32)
    from lookoncetohear_amd import synth
    gt = np.stack([synth.utterance(i, case["n"])[1] for i in case["idx"]]).astype(np.float32)
    rs = np.random.RandomState(case["seed"])
    est = np.empty_like(gt)
    for b in range(len(gt)):
        est[b, 0] = gt[b, 0]
        est[b, 1] = case["gain"][b] * _delay(gt[b, 1], case["delay"][b])
        est[b] += (case["noise"] * rs.standard_normal(gt[b].shape)).astype(np.float32)
    for b, lo, hi in case.get("silence", []):
        est[b, :, lo:hi] = 0.0
    return est, gt
