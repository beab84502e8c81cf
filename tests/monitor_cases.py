"""Shared by tests/test_emu_monitor.py and tests/test_gpu_monitor.py: the numpy-fp32 restatement of `lh_session_mix`
(include/lookonce_hip.h, "Monitor mix") — the ramp, the five rules and the fused multiply-add — the target trajectories of the
direct-call cases, and a driver of the entry point on hand-made buffers that runs on host tensors over the emulated library
and on device tensors over the product library alike.  Every comparison made with these is bit for bit."""
import ctypes

import numpy as np
import torch

HOP, NFFT = 128, 192
ERR_ARG = 1
F32 = np.float32

RAMPS = (1, 100, 128, 256, 1000)
# chunk -> (wet, dry) posted ahead of that chunk; gains start at (1, 0)
TRAJECTORIES = {
    "up": {0: (1.0, 1.0)},                                  # the dry path comes in beside the target
    "down": {0: (0.0, 0.0), 9: (0.3, 0.0)},                 # the wet path alone (rule 3), down to silence and part of the way back
    "reversed": {0: (0.25, 0.75), 1: (1.0, 0.0), 4: (0.0, 1.0), 5: (0.5, 0.5)},        # re-targeted in mid-ramp (ramp 256, 1000)
    "settled": {3: (1.0, 0.0)},                             # never leaves the defaults
}
N_CHUNKS = 12


def step_of(ramp: int) -> np.float32:
    return F32(1.0) / F32(ramp)


def ramp_gains(g0, t, step, n: int = HOP) -> np.ndarray:
    """g(0 .. n - 1) of one gain from its value g0 at the chunk's start towards t, all fp32."""
    g0, t, step = F32(g0), F32(t), F32(step)
    d = F32(t - g0)
    lim = (np.arange(1, n + 1, dtype=F32) * step).astype(F32)         # (float)(n + 1) * step: one fp32 multiply
    moved = (g0 + np.copysign(lim, d)).astype(F32)
    return np.where(np.abs(d) <= lim, t, moved).astype(F32)


def fma32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fmaf(a, b, c) on fp32 arrays, correctly rounded.  a * b is exact in fp64 (48 bits); the fp64 sum with c is made exact
    by TwoSum and rounded TO ODD, after which the rounding to fp32 cannot be a double rounding (53 >= 2 * 24 + 2)."""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                                      # s + e == p + c exactly
    even = (s.view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def mix_row(x: np.ndarray, y: np.ndarray, gain, target, step, held: bool = False):
    """One slot, one chunk.  x [2, 192] the input row, y [2, 128] the row the end node left, gain / target (wet, dry) ->
    (the row after the node, the gains after the node)."""
    (w0, d0), (wt, dt) = (F32(gain[0]), F32(gain[1])), (F32(target[0]), F32(target[1]))
    if held:
        return y.copy(), (w0, d0)
    if w0 == 1 and wt == 1 and d0 == 0 and dt == 0:
        return y.copy(), (w0, d0)
    w, d = ramp_gains(w0, wt, step), ramp_gains(d0, dt, step)
    after = (w[-1], d[-1])
    if d0 == 0 and dt == 0:
        return (w * y).astype(F32), after
    dry = x[:, :HOP]
    if not np.isfinite(dry).all():
        return np.zeros_like(y), after
    return fma32(np.broadcast_to(w, y.shape), y, (d * dry).astype(F32)), after


def rows_with_zeros(gen: torch.Generator, *shape) -> torch.Tensor:
    """Random rows in which some samples are +0 and some -0."""
    t = torch.randn(*shape, generator=gen)
    t[..., 5::17] = 0.0
    t[..., 9::23] = -0.0
    return t


def same_bits(a: torch.Tensor, b) -> bool:
    b = torch.as_tensor(np.ascontiguousarray(b)) if isinstance(b, np.ndarray) else b
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))


class Mix:
    """`lh_session_mix` on hand-made buffers of S slots; `device` "cpu" (the emulated library) or a GPU (the product one)."""

    def __init__(self, lib, S: int, ramp: int, device="cpu", paced: bool = False, seed: int = 0):
        self.lib, self.S, self.dev = lib, S, torch.device(device)
        self.step = float(step_of(ramp))
        self.gen = torch.Generator().manual_seed(seed)
        self.x = torch.zeros(S, 2, NFFT, device=self.dev)
        self.out = torch.zeros(S, 2, HOP, device=self.dev)
        self.target = torch.tensor([[1.0] * S, [0.0] * S], device=self.dev)
        self.gain = self.target.clone()
        self.hold = torch.zeros(S, dtype=torch.int32, device=self.dev) if paced else None
        # the restatement's side
        self.ref_gain = [(F32(1), F32(0))] * S
        self.ref_target = [(F32(1), F32(0))] * S

    def args(self):
        P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream(self.dev).cuda_stream if self.dev.type == "cuda" else None
        return [P(self.x), P(self.out), P(self.target), P(self.gain), P(self.hold), ctypes.c_float(self.step), self.S, stream]

    def post(self, slot: int, wet: float, dry: float):
        self.target[0, slot], self.target[1, slot] = wet, dry
        self.ref_target[slot] = (F32(wet), F32(dry))

    def call(self, x: torch.Tensor = None, y: torch.Tensor = None, held=()):
        """One chunk on rows x [S, 2, 192], y [S, 2, 128] (random by default) -> (what the node left, what the restatement
        says), and the gains of both sides have advanced."""
        S = self.S
        x = rows_with_zeros(self.gen, S, 2, NFFT) if x is None else x
        y = rows_with_zeros(self.gen, S, 2, HOP) if y is None else y
        self.x.copy_(x), self.out.copy_(y)
        if self.hold is not None:
            self.hold.copy_(torch.tensor([1 if s in held else 0 for s in range(S)], dtype=torch.int32))
        with torch.cuda.device(self.dev) if self.dev.type == "cuda" else _nothing():
            assert self.lib.raw("lh_session_mix")(*self.args()) == 0
        want = np.zeros((S, 2, HOP), dtype=F32)
        for s in range(S):
            want[s], self.ref_gain[s] = mix_row(x[s].numpy(), y[s].numpy(), self.ref_gain[s], self.ref_target[s], F32(self.step),
                                                held=s in held)
        return self.out.cpu().clone(), want

    def gains_match(self) -> bool:
        want = np.array(self.ref_gain, dtype=F32).T                  # [2][S]
        return same_bits(self.gain, want)


class _nothing:
    def __enter__(self): return None
    def __exit__(self, *a): return False


def run_trajectory(lib, S: int, ramp: int, names, device="cpu", seed: int = 0):
    """N_CHUNKS chunks with slot s following TRAJECTORIES[names[s]]: asserts every output sample and every gain word against
    the restatement, bit for bit; returns the `Mix`."""
    m = Mix(lib, S, ramp, device, seed=seed)
    for j in range(N_CHUNKS):
        for s, name in enumerate(names):
            if j in TRAJECTORIES[name]:
                m.post(s, *TRAJECTORIES[name][j])
        got, want = m.call()
        assert same_bits(got, want), (S, ramp, names, j, float(np.abs(got.numpy() - want).max()))
        assert m.gains_match(), (S, ramp, names, j, m.gain.cpu().tolist(), m.ref_gain)
    return m
