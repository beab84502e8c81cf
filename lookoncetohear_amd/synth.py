"""Deterministic synthetic binaural mixtures with the reference dataset's I/O contract.

The reference eval loop (reference `src/ts_hear_test.py:124-146`) consumes, per utterance,
`mixture [2, 80000]` (16 kHz, 5 s, peak <= 1), `target [2, 80000]` and a unit-L2 non-negative
d-vector `embedding_gt [1, 256]`, produced by `MixLibriSpeechNoisyEnroll.__getitem__`
(reference `src/datasets/MixLibriSpeechNoisyEnrollNorm.py:152-376`).  Neither the dataset nor a
checkpoint exists in this environment, so `bench.py`, the eval driver and the tests use this
generator instead: per-utterance seed = utterance index (the reference seeds
val/test samples by index too, `MixLibriSpeechNoisyEnrollNorm.py:164-168`), three pseudo-speech
sources (AM harmonic stacks, f0 100-250 Hz, random on/off bursts) each rendered through a random
2-channel 64-tap FIR (pseudo-HRIR, interaural delay <= 16 samples, cf. `max_shift: 16`
`configs/tsh.json:87`), plus 2-channel coloured noise, peak-normalised when above 1.
"""
from __future__ import annotations

import numpy as np
import torch

SR = 16000


def _source(rs: np.random.RandomState, n: int) -> np.ndarray:
    t = np.arange(n) / SR
    f0 = rs.uniform(100.0, 250.0) * (1.0 + 0.03 * np.sin(2 * np.pi * rs.uniform(2, 6) * t + rs.uniform(0, 6.28)))
    phase = 2 * np.pi * np.cumsum(f0) / SR
    sig = np.zeros(n)
    for h in range(1, 13):
        sig += rs.uniform(0.2, 1.0) / h * np.sin(h * phase + rs.uniform(0, 6.28))
    # syllable-rate envelope with random pauses
    env = 0.5 * (1 + np.sin(2 * np.pi * rs.uniform(3, 5) * t + rs.uniform(0, 6.28)))
    gate = (rs.rand(int(np.ceil(n / 4000)) + 1) > 0.25).astype(np.float64)
    gate = np.repeat(gate, 4000)[:n]
    gate = np.convolve(gate, np.ones(400) / 400, mode="same")[:n]
    return sig * env * gate


def _hrir(rs: np.random.RandomState) -> np.ndarray:
    h = np.zeros((2, 64))
    itd = rs.randint(0, 17)
    near = rs.randint(0, 2)
    decay = np.exp(-np.arange(64) / rs.uniform(3, 9))
    for ch in range(2):
        d = itd if ch != near else 0
        taps = rs.randn(64 - d) * decay[: 64 - d]
        taps[0] += 1.0
        h[ch, d:] = taps * (rs.uniform(0.4, 0.9) if ch != near else 1.0)
    return h


def utterance(idx: int, n: int = 80000):
    """Returns (mixture [2,n], target [2,n], embedding [1,256]) float32 numpy arrays for utterance `idx`."""
    rs = np.random.RandomState(idx)
    srcs = []
    for _ in range(3):
        s = _source(rs, n)
        h = _hrir(rs)
        srcs.append(np.stack([np.convolve(s, h[c])[:n] for c in range(2)]))
    srcs = np.stack(srcs)                                   # [3,2,n]
    srcs *= 0.12 / (srcs.std() + 1e-9)
    noise = rs.randn(2, n + 8)
    noise = np.stack([np.convolve(noise[c], [0.4, 0.3, 0.15, 0.08, 0.04, 0.02, 0.01, 0.005], mode="valid")[:n]
                      for c in range(2)])
    noise *= 0.004 * rs.uniform(3.0, 10.0)                  # noise_scale U(3,10), configs/tsh.json:86
    mix = srcs.sum(0) + noise
    peak = np.abs(mix).max()
    if peak > 1.0:                                          # peak-normalise (MixLibriSpeechNoisyEnrollNorm.py:196-202)
        mix, srcs = mix / peak, srcs / peak
    tgt = srcs[rs.randint(0, 3)]
    emb = np.abs(rs.randn(256))
    emb = emb / np.linalg.norm(emb)
    return mix.astype(np.float32), tgt.astype(np.float32), emb[None].astype(np.float32)


ENROLL_SEED_OFFSET = 1_000_003          # the enrollment recording of utterance i is synthetic utterance i + this


def enrollment(idx: int, n: int = 80000) -> np.ndarray:
    """[1, 2, n] float32: the noisy binaural enrollment recording the reference dataset returns as `inputs['enrollments']`
    (`num_enroll` = 1 recordings of `enroll_len` = 5 s: MixLibriSpeechNoisyEnrollNorm.py:118, 259-303 — another scene
    with the target speaker in it, rendered like a mixture).  Synthetic stand-in: the mixture of an unrelated synthetic
    utterance, seeded by the utterance index like everything else here."""
    return utterance(ENROLL_SEED_OFFSET + int(idx), n)[0][None]


def batch(indices, n: int = 80000, enroll_n: int = 0):
    """Stack utterances -> dict of torch CPU tensors: mixture [B,2,n], target [B,2,n], embedding_gt [B,1,256] and, with
    `enroll_n` > 0, enrollments [B,1,2,enroll_n] (the eval loop squeezes dim 1, reference src/ts_hear_test.py:133)."""
    m, t, e = zip(*(utterance(int(i), n) for i in indices))
    out = dict(mixture=torch.from_numpy(np.stack(m)), target=torch.from_numpy(np.stack(t)),
               embedding_gt=torch.from_numpy(np.stack(e)))
    if enroll_n:
        out["enrollments"] = torch.from_numpy(np.stack([enrollment(int(i), enroll_n) for i in indices]))
    return out


# ---- moving scenes: the input side of BinauralRenderer.nearest / render_moving -------------------------------------------------
MOVING_SEED_OFFSET = 2_000_003          # moving scene i draws from RandomState(i + this): unrelated to utterance i
PATH_RADIUS = 1.5                       # metres; the reference's RRBRIR paths use r = 1.5 (the lookup ignores the scale)


def _ring_bank(rs: np.random.RandomState, P: int, lh: int):
    """Pseudo-HRIR bank [P, 2, lh] on a ring of P azimuths (0 = ahead, +pi/2 = the left ear's side) and the unit vectors
    [P, 3] of its entries.  One decaying random tail per ear is shared by every entry, so a response changes smoothly with
    the azimuth: the far ear is delayed by 16 |sin az| samples (a fractional delay, split linearly over two taps: the
    inter-aural delay stays at or below 16 samples, as in `_hrir`) and attenuated by up to 0.5."""
    az = 2 * np.pi * np.arange(P) / P
    decay = np.exp(-np.arange(lh) / rs.uniform(3, 9))
    base = 0.3 * rs.randn(2, lh) * decay
    base[:, 0] += 1.0
    bank = np.zeros((P, 2, lh))
    for p in range(P):
        s = np.sin(az[p])
        for ear in range(2):                                    # ear 0 = left: far when the source is on the right (s < 0)
            far = (s < 0) if ear == 0 else (s > 0)
            d = 16.0 * abs(s) if far else 0.0
            g = 1.0 - 0.5 * abs(s) if far else 1.0
            d0, fr = int(np.floor(d)), d - np.floor(d)
            h = np.zeros(lh + 17)
            h[d0:d0 + lh] += (1.0 - fr) * base[ear]
            h[d0 + 1:d0 + 1 + lh] += fr * base[ear]
            bank[p, ear] = g * h[:lh]
    positions = np.stack([np.cos(az), np.sin(az), np.zeros(P)], 1)
    return bank, positions


def _path_azimuths(rs: np.random.RandomState, law: int, F: int, dt: float) -> np.ndarray:
    """F azimuths, one per `dt` seconds, by one of the three laws of motion the reference's moving dataset describes:
    0: a constant angular velocity (pi/6 .. pi/2 rad/s, either way) from a random start;
    1: piecewise arcs — rest, then a move of 0.1 .. 1 s at pi/6 .. pi/2 rad/s either way, again and again;
    2: face to face — small jitter round straight ahead (a mean-reverting random walk), the enrollment posture."""
    t = np.arange(F) * dt
    if law == 0:
        return rs.uniform(0, 2 * np.pi) + rs.choice([-1.0, 1.0]) * rs.uniform(np.pi / 6, np.pi / 2) * t
    if law == 1:
        az, out, k = rs.uniform(0, 2 * np.pi), np.zeros(F), 0
        while k < F:
            rest = int(round(rs.uniform(0.2, 1.5) / dt))
            out[k:k + rest] = az
            k += rest
            move, vel = int(round(rs.uniform(0.1, 1.0) / dt)), rs.choice([-1.0, 1.0]) * rs.uniform(np.pi / 6, np.pi / 2)
            steps = az + vel * dt * np.arange(1, move + 1)
            m = max(0, min(move, F - k))
            out[k:k + m] = steps[:m]
            az, k = steps[-1], k + move
        return out
    out, steps = np.zeros(F), rs.randn(F) * np.radians(1.0)
    for k in range(1, F):                                       # mean-reverting: a few degrees either side of straight ahead
        out[k] = 0.95 * out[k - 1] + steps[k]
    return out


def moving_scene(idx: int, n: int = 80000, n_src: int = 3, P: int = 72, lh: int = 64, frame: int = 400):
    """Seeded moving scene for `BinauralRenderer.nearest` / `render_moving`: a dict of float32 numpy arrays
        srcs [n_src + 1, n]          pseudo-speech sources, then the noise bed (LAST)
        bank [P, 2, lh]              pseudo-HRIRs on a ring of P azimuths, positions [P, 3] their unit vectors
        paths [n_src + 1, F, 3]      one point per `frame` samples at radius PATH_RADIUS, F = ceil(n / frame) + 1: source i moves
                                     by law i % 3 of `_path_azimuths`; the noise bed stands still
        gains [n_src + 1]            1 for sources, noise_scale U(3, 10) for the bed
    and `tgt_idx` (int, a source).  Host code, like `utterance`; the rendering itself is the device's."""
    rs = np.random.RandomState(MOVING_SEED_OFFSET + int(idx))
    F = -(-n // frame) + 1
    srcs = np.stack([_source(rs, n) for _ in range(n_src)])
    srcs *= 0.12 / (srcs.std() + 1e-9)
    noise = np.convolve(rs.randn(n + 7), [0.4, 0.3, 0.15, 0.08, 0.04, 0.02, 0.01, 0.005], mode="valid")[:n] * 0.004
    bank, positions = _ring_bank(rs, P, lh)
    az = [_path_azimuths(rs, i % 3, F, frame / SR) for i in range(n_src)] + [np.full(F, rs.uniform(0, 2 * np.pi))]
    paths = np.stack([PATH_RADIUS * np.stack([np.cos(a), np.sin(a), np.zeros(F)], 1) for a in az])
    gains = np.array([1.0] * n_src + [rs.uniform(3.0, 10.0)])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(srcs=f32(np.concatenate([srcs, noise[None]])), bank=f32(bank), positions=f32(positions), paths=f32(paths),
                gains=f32(gains), tgt_idx=int(rs.randint(n_src)))
