"""The fractional hop of `lh_session_resample_out_any` (include/lookonce_hip.h, "any rate") restated in plain integers, and the
helpers tests/test_emu_any_rate.py and tests/test_gpu_any_rate.py share: the node driven step by step through the C ABI on host
or device tensors, and the tick loop of a packet streamer whose rows carry a count.

Nothing here is taken from the code under test: width, o and n come from tests/resample_cases.py (the float64 restatement of
torchaudio's `sinc_interp_hann`), d, P, T and c(r) from the definition."""
import ctypes
import math

import torch

from tests import resample_cases as C

HOP, NFFT, RATE = 128, 192, 16000
STAGE = 1427                                     # samples per channel the node stages: T + 128 of 11 025 Hz
ARG = 1
F32, S16 = 0, 1
V = lambda t: ctypes.c_void_p(t.data_ptr())


class Geometry:
    """16 kHz -> `rate`: width, o, n, K of the bank; the delay d, the period P, the carried samples T, the widest row."""

    def __init__(self, rate):
        _, self.width, self.o, self.n = C.bank64(RATE, rate)
        w, o, n = self.width, self.o, self.n
        self.rate, self.K = rate, 2 * w + o
        self.d = w + o - 1
        self.P = o // math.gcd(HOP, o)
        self.T = self.K + o + -(-o // n) - 1
        self.hop_max = -(-HOP * n // o)

    def c(self, r):
        return HOP * r * self.n // self.o

    def count(self, live_steps_before):
        r = live_steps_before % self.P
        return self.c(r + 1) - self.c(r)

    def counts(self, steps):
        return [self.count(t) for t in range(steps)]


def s16_of(y32):
    """lh_session_emit_s16 on fp32 bits: round half even, saturating, NaN -> 0."""
    return torch.nan_to_num(torch.clamp(torch.round(y32 * 32768), -32768, 32767), nan=0.0).to(torch.int16)


def held_pattern(steps, S):
    """held[t][s]: slot 0 is always live; slot s > 0 is held at the steps t with (t + 2 s) % (s + 2) == 0 — slot 1 at 1, 4, 7,
    10, slot 2 at 0, 4, 8 ... — so that the slots sit at different phases of the period."""
    return [[bool(s) and (t + 2 * s) % (s + 2) == 0 for s in range(S)] for t in range(steps)]


def node_args(out, tail, phase, hold, y, count, fmt, bank_t, g):
    return [V(out), V(tail), V(phase), V(hold), V(y), V(count), fmt, out.shape[0], V(bank_t), g.o, g.n, g.width]


def run_node(raw, stream, dev, rate, S, steps, bank, up):
    """`raw` = the entry point, `bank` = resample_bank(16000, rate)[0] [n][K], `up(x)` = the offline resampler 16 kHz -> rate on
    `dev`.  Drives fp32 and int16 side by side through `steps` steps with holds and asserts, per step: the count, the zero columns
    behind it, the tail and the phase word, a held slot's zero row and untouched words, the int16 rounding; at the end: every
    slot's concatenated valid samples equal `up` of d zeros followed by its live rows."""
    g = Geometry(rate)
    assert tuple(bank.shape) == (g.n, g.K) and g.T + HOP <= STAGE
    bank_t = bank.t().contiguous().to(dev)
    torch.manual_seed(rate)
    rows = (torch.randn(steps, S, 2, HOP) * 0.4).to(dev)
    held = held_pattern(steps, S)
    z = lambda *s, **k: torch.zeros(*s, device=dev, **k)
    tail, tail16 = z(S, 2, g.T), z(S, 2, g.T)
    phase, phase16 = z(S, dtype=torch.int32), z(S, dtype=torch.int32)
    cnt, cnt16 = torch.full((S,), -1, dtype=torch.int32, device=dev), torch.full((S,), -1, dtype=torch.int32, device=dev)
    y32 = torch.full((S, 2, g.hop_max), 9.0, device=dev)
    y16 = torch.full((S, 2, g.hop_max), 9, dtype=torch.int16, device=dev)
    got, live = [[] for _ in range(S)], [0] * S
    for t in range(steps):
        hold = torch.tensor(held[t], dtype=torch.int32).to(dev)
        before, ph0 = tail.clone(), phase.clone()
        assert raw(*node_args(rows[t], tail, phase, hold, y32, cnt, F32, bank_t, g), stream) == 0
        assert raw(*node_args(rows[t], tail16, phase16, hold, y16, cnt16, S16, bank_t, g), stream) == 0
        assert torch.equal(tail, tail16) and torch.equal(phase, phase16) and torch.equal(cnt, cnt16)
        assert torch.equal(y16, s16_of(y32))
        want = [0 if held[t][s] else g.count(live[s]) for s in range(S)]
        assert cnt.tolist() == want, (t, cnt.tolist(), want)
        for s in range(S):
            assert not y32[s, :, want[s]:].any(), (t, s)         # at and beyond the count: zeros
            if held[t][s]:
                assert torch.equal(tail[s], before[s]) and phase[s] == ph0[s], (t, s)
            else:
                got[s].append(y32[s, :, :want[s]].clone())
                live[s] += 1
                assert torch.equal(tail[s], torch.cat([before[s], rows[t, s]], -1)[:, -g.T:])
                assert phase[s].item() == live[s] % g.P
    for s in range(S):
        x = torch.cat([rows[t, s] for t in range(steps) if not held[t][s]], -1)
        whole = up(torch.cat([z(2, g.d), x], -1))
        mine = torch.cat(got[s], -1)
        assert mine.shape[-1] == sum(g.counts(live[s])) == (live[s] // g.P) * g.c(g.P) + g.c(live[s] % g.P)
        assert torch.equal(mine, whole[:, :mine.shape[-1]]) and mine.abs().max() > 0.1, s
    return live


def client_len(rate, n16):
    """Client samples that make at least n16 samples at 16 kHz, the last block's taps ending with the stream; and what they make."""
    _, width, o, n = C.bank64(rate, RATE)
    blocks = -(-n16 // n)
    return (blocks - 1) * o + width + o, blocks * n


def drive(ss, x, sizes, total):
    """The tick loop of a packet streamer: one packet per slot (`sizes(slot, tick)` client samples of x[slot], up to `total`),
    then ONE `step` — so a listener whose stream is there at once and one whose packets trickle in share steps, and whoever has
    no window yet is held — until the streams are pushed and nobody is ready.  Reads nothing back.  -> (rows [steps, S, 2,
    hop_client] on the streamer's device, [(last_present, last_counts)] per step)."""
    pos, outs, log, t = [0] * ss.S, [], [], 0
    while any(p < total for p in pos) or ss.ready():
        packets = {}
        for s in range(ss.S):
            n = min(sizes(s, t), total - pos[s])
            packets[s] = x[s][:, pos[s]:pos[s] + n]
            pos[s] += n
        ss.push(packets)
        ready = ss.ready()
        y = ss.step()
        assert [s for s in range(ss.S) if ss.last_present[s]] == ready
        outs.append(y.clone())
        log.append((ss.last_present, ss.last_counts))
        t += 1
    return torch.stack(outs), log


def listener(y, log, s, g):
    """Slot s's stream out of `drive`'s rows: the valid samples of the steps it was present for, after checking that its counts
    follow the pattern, that a held step has count 0 and that everything behind a count is zero."""
    parts, live = [], 0
    for i, (present, counts) in enumerate(log):
        want = g.count(live) if present[s] else 0
        assert counts[s] == want, (i, s, counts[s], want)
        assert not y[i, s, :, want:].any(), (i, s)
        if present[s]:
            parts.append(y[i, s, :, :want])
            live += 1
    return torch.cat(parts, -1), live
