"""CPU: the monitor mix (ABI 30) — `lh_session_mix` (lh_stream.hip) by direct C-ABI calls on hand-made buffers, and
`SessionStreamer(monitor=True)`: `set_mix`, `enroll(..., passthrough=True)` and `relook` (sessions.py) over the emulated library,
eager.  No claim here is about the separator's arithmetic: the mix is held to the numpy-fp32 restatement of
tests/monitor_cases.py and everything else to a twin streamer, all bit for bit.  Small on purpose: the emulator runs a chunk
row in ~0.5 s, so the host cases share one reference run and stay at S = 2 and a handful of chunks."""
import ctypes

import numpy as np
import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.resample import Resampler
from tests import monitor_cases as C
from tests.hipemu.hosts import EmuHost, EmuNet
from oracle import tfgridnet_oracle as O

HOP, NFFT = C.HOP, C.NFFT
F32 = np.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def emu_lib():
    from tests.hipemu.build_emu import build_emu
    return _cabi.Lib(build_emu())


# ---- the entry point on hand-made buffers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ramp", C.RAMPS)
@pytest.mark.parametrize("name", sorted(C.TRAJECTORIES))
def test_mix_one_slot_equals_the_restatement(emu_lib, name, ramp):
    C.run_trajectory(emu_lib, 1, ramp, [name], seed=ramp)


@pytest.mark.parametrize("ramp", C.RAMPS)
@pytest.mark.parametrize("first", range(4))
def test_mix_three_slots_equal_the_restatement(emu_lib, first, ramp):
    """Three slots on three different trajectories at once: a slot's row and gains are its own."""
    names = sorted(C.TRAJECTORIES)
    C.run_trajectory(emu_lib, 3, ramp, [names[(first + s) % 4] for s in range(3)], seed=10 * ramp + first)


def test_ramp_reaches_its_target_exactly_and_is_monotone():
    """The restatement itself: 0 -> 1 in `ramp` samples, exactly 1 from then on, never decreasing; and the fused
    multiply-add is the correctly rounded one where a plain fp32 multiply and add is not."""
    for ramp in C.RAMPS:
        g, g0, seen = [], F32(0), 0
        while seen < ramp + HOP:
            r = C.ramp_gains(g0, 1.0, C.step_of(ramp))
            g.append(r)
            g0, seen = r[-1], seen + HOP
        g = np.concatenate(g)
        # (100 and 1000 are not powers of two: `step` is rounded, and the last step may come one sample late)
        assert (np.diff(g) >= 0).all() and (g[ramp:] == 1).all() and (g[:ramp - 1] < 1).all() and g[0] == C.step_of(ramp), ramp
    a, b, c = F32(1 + 2 ** -12), F32(1 + 2 ** -12), F32(-1)
    exact = (1 + 2 ** -12) ** 2 - 1                                  # 2^-11 + 2^-24: representable
    assert C.fma32(np.array([a]), np.array([b]), np.array([c]))[0] == F32(exact) != F32(F32(a * b) + c)


def test_settled_default_rows_keep_their_bytes(emu_lib):
    """Gains and targets at (1, 0): the row is not touched — a sentinel pattern with -0.0, NaN and inf in it stays byte for
    byte, whatever the input row holds."""
    m = C.Mix(emu_lib, 3, 256)
    y = torch.tensor([-0.0, 0.0, NAN, float("inf"), -7.0, 1e-42, -1e38, 3.0]).repeat(3, 2, HOP // 8)
    x = torch.full((3, 2, NFFT), NAN)
    for _ in range(2):
        got, _ = m.call(x, y)
        assert C.same_bits(got, y) and C.same_bits(m.gain, torch.tensor([[1.0] * 3, [0.0] * 3]))


def test_held_slot_is_untouched_and_the_ramp_resumes(emu_lib):
    m = C.Mix(emu_lib, 3, 1000, paced=True)
    for s in range(3):
        m.post(s, 0.0, 1.0)
    got, want = m.call()
    assert C.same_bits(got, want) and m.gains_match()
    before = m.gain.clone()
    y = torch.full((3, 2, HOP), -0.0)
    y[0] = torch.randn(2, HOP)
    got, want = m.call(torch.full((3, 2, NFFT), NAN), y, held=(0, 1, 2))       # all held: the input may be anything
    assert C.same_bits(got, y) and C.same_bits(m.gain, before)
    got, want = m.call(held=(1,))                                   # slots 0 and 2 go on, slot 1 waits
    assert C.same_bits(got, want) and m.gains_match() and C.same_bits(m.gain[:, 1], before[:, 1])
    assert not C.same_bits(m.gain[:, 0], before[:, 0])
    for _ in range(9):                                              # ... and everyone arrives: 1000 samples from where they were
        got, want = m.call()
        assert C.same_bits(got, want) and m.gains_match()
    assert m.gain.tolist() == [[0.0] * 3, [1.0] * 3]


@pytest.mark.parametrize("bad", [NAN, float("inf"), float("-inf")])
def test_nonfinite_dry_input_silences_the_row_and_the_gains_advance(emu_lib, bad):
    m = C.Mix(emu_lib, 3, 256)
    for s in range(3):
        m.post(s, 0.5, 1.0)
    m.call()
    x = C.rows_with_zeros(m.gen, 3, 2, NFFT)
    x[0, 1, 127] = bad                                              # the last sample of the row's own 128: slot 0 is silenced
    x[1, 0, 128] = bad                                              # look-ahead only: slot 1 is mixed as ever
    x[2, 0, 191] = bad
    before = m.gain.clone()
    got, want = m.call(x)
    assert not got[0].any() and C.same_bits(got[0], torch.zeros(2, HOP))
    assert C.same_bits(got, want) and got[1].abs().max() > 0.1 and torch.isfinite(got).all()
    assert m.gains_match() and not C.same_bits(m.gain[:, 0], before[:, 0])     # slot 0's ramp went on underneath
    got, want = m.call()
    assert C.same_bits(got, want) and got[0].abs().max() > 0.1


def test_dry_path_absent_never_reads_the_input_into_the_result(emu_lib):
    """dry g0 == t == 0 and the wet gain on its way down: wet * y, finite, although the whole input row is NaN."""
    m = C.Mix(emu_lib, 3, 256)
    for s in range(3):
        m.post(s, 0.25, 0.0)
    got, want = m.call(torch.full((3, 2, NFFT), NAN))
    assert C.same_bits(got, want) and torch.isfinite(got).all() and got.abs().max() > 0.1 and m.gains_match()
    assert m.gain[0].tolist() == [0.5] * 3


def test_mix_validates_arguments(emu_lib):
    m = C.Mix(emu_lib, 3, 256, paced=True)
    for s in range(3):
        m.post(s, 0.0, 1.0)
    m.x.copy_(torch.randn(3, 2, NFFT)), m.out.fill_(-7.0)
    f, ok = emu_lib.raw("lh_session_mix"), m.args()
    off = lambda a, i, n: a[:i] + [ctypes.c_void_p(a[i].value + n)] + a[i + 1:]
    bad = [ok[:i] + [None] + ok[i + 1:] for i in range(4)]          # a null pointer; hold may be null
    bad += [off(ok, 0, 4), off(ok, 1, 8), off(ok, 2, 2), off(ok, 3, 1), off(ok, 4, 2)]          # misaligned
    bad += [ok[:6] + [S] + ok[7:] for S in (0, -1)]
    bad += [ok[:5] + [ctypes.c_float(v)] + ok[6:] for v in (0.0, -0.5, 1.0000001, 2.0, NAN, float("inf"))]
    for i, a in enumerate(bad):
        assert f(*a) == C.ERR_ARG, i
    assert bool(m.out.eq(-7.0).all()) and m.gain.tolist() == [[1.0] * 3, [0.0] * 3]         # nothing was written
    assert f(*ok) == 0 and not m.out.eq(-7.0).any()
    assert f(*(ok[:4] + [None] + ok[5:])) == 0                      # the lock-step form
    assert f(*(ok[:5] + [ctypes.c_float(1.0)] + ok[6:])) == 0       # monitor_ramp = 1


# ---- the host over the emulated device ----------------------------------------------------------------------------------------
class SyncSide:
    """Stand-in for `net._EnrollSide`, as in tests/test_emu_enroll.py: the embedder call has finished when `run` returns."""

    def run(self, fn):
        return fn(), None

    def finished(self, done):
        return True

    def hand_over(self, done, out):
        pass


class EmuMonitorNet(EmuNet):
    def _host_words(self, n, device):               # the pinned words of the GPU host: plain host memory here
        return torch.zeros(n, dtype=torch.int32)

    def _enroll_side(self, dev):
        return SyncSide()


class EmuResampler(EmuHost, Resampler):
    """The product `Resampler` over the emulated library and host tensors."""


class NoEmbed:
    def __call__(self, x):
        raise AssertionError("the embedder ran")


class FakeEmbed:
    """The first 256 samples of the clip's left channel: cheap, and shows which clip it was called on."""

    def __init__(self):
        self.calls = []

    def __call__(self, x):
        self.calls.append(x.clone())
        return x[:, 0, :256].contiguous()


S, N_REF = 2, 5


@pytest.fixture(scope="module")
def emu_net(oracle_cfg_sd, emu_lib):
    cfg, sd = oracle_cfg_sd
    net = EmuMonitorNet(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net.emu_lib = emu_lib
    return net


@pytest.fixture(scope="module")
def clips():
    d = synth.batch([20, 21], HOP * 8 + NFFT - HOP)
    return d["mixture"], d["embedding_gt"][:, 0]


def chunk_of(mix_row, j):
    return mix_row[:, j * HOP:j * HOP + NFFT]


def feed_both(mix):
    return lambda i: torch.stack([chunk_of(mix[0], i), chunk_of(mix[1], i)])


def run(ss, n, feed, events=None, start=0):
    """Steps start .. start + n - 1 on feed(i) [S, 2, 192]; events {i: fn} run before step i -> [n][S, 2, 128]."""
    outs = []
    for i in range(start, start + n):
        if events and i in events:
            events[i]()
        outs.append(ss.step(feed(i)).clone())
    return outs


@pytest.fixture(scope="module")
def plain(emu_net, clips):
    """The reference of the lock-step cases: a streamer WITHOUT the feature, slot 0 open on its own stream, slot 1 idle."""
    mix, emb = clips
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=2)
    assert not ss.monitor and not hasattr(ss, "_mix") and not hasattr(ss, "_targets")      # exactly today's object
    ss.open(0, emb[0])
    return run(ss, N_REF, feed_both(mix))


def restated(x_row, y_row, gain, target, ramp):
    row, gain = C.mix_row(x_row.numpy(), y_row.numpy(), gain, target, C.step_of(ramp))
    return torch.from_numpy(row), gain


def test_monitor_defaults_equal_a_streamer_without_it(emu_net, clips, plain):
    mix, emb = clips
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=2, monitor=True)
    assert ss.monitor and ss.monitor_ramp == 256 and ss.mix_of(0) == ss.mix_of(1) == (1.0, 0.0)
    ss.open(0, emb[0])
    y = run(ss, 3, feed_both(mix))
    for j in range(3):
        assert C.same_bits(y[j], plain[j]), j
    assert y[2][0].abs().max() > 1e-4 and not y[2][1].any()
    assert ss._mix.tolist() == [[[1.0, 1.0], [0.0, 0.0]]] * 2


def test_monitor_defaults_equal_a_paced_streamer_without_it(emu_net, clips):
    mix, emb = clips
    pair = [emu_net.make_session_streamer(S, "cpu", use_graph=False, pace=True, monitor=m) for m in (False, True)]
    ys = []
    for ss in pair:
        ss.open(0, emb[0]), ss.open(1, emb[1])
        ys.append([ss.step(feed_both(mix)(0), present=[True, True]).clone(),
                   ss.step(feed_both(mix)(1), present=[True, False]).clone()])
    for j in range(2):
        assert C.same_bits(ys[1][j], ys[0][j]), j
    assert ys[1][0].abs().max() > 1e-4 and not ys[1][1][1].any()


def test_monitor_defaults_equal_a_pcm16_packet_streamer_without_it(emu_net, clips):
    mix, emb = clips
    pcm = (mix[:, :, :2 * HOP + NFFT - HOP] * 32768).round().clamp(-32768, 32767).to(torch.int16)
    ys = []
    for m in (False, True):
        ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, pace=True, packets=True, pcm16=True, monitor=m)
        ss.open(0, emb[0])
        ss.push({0: pcm[0], 1: pcm[1, :, :NFFT]})
        rows = []
        while ss.ready():
            rows.append(ss.step().clone())
        ys.append(rows)
    assert len(ys[0]) == len(ys[1]) == 2 and ys[1][0].dtype == torch.int16
    for j in range(2):
        assert torch.equal(ys[1][j], ys[0][j]), j
    assert ys[1][1][0].abs().max() > 0


def test_set_mix_idle_and_open_slots_and_faults_fail_open(emu_net, clips, plain):
    """ramp 128.  Slot 0 is open at (1, 0.5): target and room together, on the reference's separated rows.  Slot 1 is idle at
    (0, 1): the ramp, then its own input, sample for sample.  NaN on the idle slot: a zero row, no fault.  NaN on the open
    slot: a zero row, the slot in `faults()`, and from the next chunk on it sounds as the idle slot with its dry gain does."""
    mix, emb = clips
    ramp = 128
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=2, monitor=True, monitor_ramp=ramp)
    ss.open(0, emb[0])
    ss.set_mix(0, 1.0, 0.5), ss.set_mix(1, 0.0, 1.0)
    assert ss.mix_of(0) == (1.0, 0.5) and ss.mix_of(1) == (0.0, 1.0)
    gains = [(1.0, 0.0), (1.0, 0.0)]
    feed = feed_both(mix)
    x = [feed(i).clone() for i in range(5)]
    x[2][1, 0, 5] = NAN                                             # the idle slot
    x[3][0, 1, 100] = float("inf")                                  # the open slot
    zero = torch.zeros(2, HOP)
    for i in range(5):
        y = ss.step(x[i]).clone()
        sep0 = plain[i][0] if i < 3 else zero                       # what the end node leaves: the session dies in chunk 3
        want0, gains[0] = restated(x[i][0], sep0, gains[0], (1.0, 0.5), ramp)
        want1, gains[1] = restated(x[i][1], zero, gains[1], (0.0, 1.0), ramp)
        assert C.same_bits(y[0], want0) and C.same_bits(y[1], want1), i
        assert ss.faults() == ([] if i < 3 else [0]) and ss.active == ([0] if i < 3 else [])
        if i == 1:
            assert C.same_bits(y[1], x[i][1, :, :HOP] + 0.0)        # settled at (0, 1): the room itself (0 y + x: a -0 is +0)
        if i == 2:
            assert C.same_bits(y[1], zero)
        if i == 3:
            assert C.same_bits(y[0], zero) and C.same_bits(y[1], x[i][1, :, :HOP] + 0.0)
        if i == 4:
            assert C.same_bits(y[0], (x[i][0, :, :HOP] * 0.5) + 0.0) and y[0].abs().max() > 1e-3     # fail-open
    assert C.same_bits(ss._mix[1], torch.tensor([[1.0, 0.0], [0.5, 1.0]]))
    ss.reset()
    assert ss.mix_of(0) == ss.mix_of(1) == (1.0, 0.0) and ss._mix.tolist() == [[[1.0, 1.0], [0.0, 0.0]]] * 2
    assert not ss.step(x[0]).any()


def test_enroll_with_passthrough_cross_fades_into_the_target(emu_net, clips):
    """Slot 1 enrolls at step 0 over two chunks and opens at step 2; ramp 256.  While capturing the listener hears their own
    input, from the opening step on fmaf(w, y, d x) on the rows of a twin WITHOUT the feature enrolling the same way, and
    after the ramp the twin's rows, bit for bit."""
    mix, emb = clips
    ramp, n, opened = 256, 5, 2
    feed = feed_both(mix)
    twin = emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=2)
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=2, monitor=True, monitor_ramp=ramp)
    with pytest.raises(ValueError, match="monitor"):
        twin.enroll(1, NoEmbed(), passthrough=True)
    e_twin, e = FakeEmbed(), FakeEmbed()
    twin.enroll(1, e_twin)
    yt = run(twin, n, feed)
    ss.enroll(1, e, passthrough=True)
    assert ss.mix_of(1) == (0.0, 1.0) and ss.mix_of(0) == (1.0, 0.0)
    gain, seen = (1.0, 0.0), []
    for i in range(n):
        y = ss.step(feed(i)).clone()
        seen.append((ss.active, ss.enrolling, ss.mix_of(1)))
        want, gain = restated(feed(i)[1], yt[i][1], gain, (0.0, 1.0) if i < opened else (1.0, 0.0), ramp)
        assert C.same_bits(y[1], want) and not y[0].any(), i
        if i == 0:
            # the ramp of a monitor_ramp of two chunks has not arrived; ramp 256 from (1, 0) to (0, 1) on a zero row
            assert not C.same_bits(y[1], feed(i)[1, :, :HOP])
        if i == 1:
            assert not yt[i][1].any()
        if i >= opened + 2:
            assert C.same_bits(y[1], yt[i][1]) and y[1].abs().max() > 1e-4
    assert seen[1] == ([], [1], (0.0, 1.0)) and seen[2] == ([1], [], (1.0, 0.0)) and twin.active == [1]
    assert len(e.calls) == 1 and torch.equal(e.calls[0], e_twin.calls[0]) and torch.equal(e.calls[0], mix[1][None, :, :2 * HOP])
    assert ss._mix.tolist() == [[[1.0, 1.0], [0.0, 0.0]]] * 2


def test_passthrough_rows_during_capture_are_the_input(emu_net, clips):
    """ramp 1: the swing is over with the first sample, so every row of the capture is the slot's own input.  The second
    recorded chunk holds an inf: its row is zeros, the capture is a fault, the slot stays idle and keeps sounding dry."""
    mix, emb = clips
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=3, monitor=True, monitor_ramp=1)
    ss.enroll(1, NoEmbed(), passthrough=True)
    feed = feed_both(mix)
    x = [feed(i).clone() for i in range(4)]
    x[1][1, 0, 3] = float("inf")
    for i in range(4):
        y = ss.step(x[i])
        assert C.same_bits(y[1], torch.zeros(2, HOP) if i == 1 else x[i][1, :, :HOP] + 0.0) and not y[0].any(), i
    assert ss.faults() == [1] and ss.enrolling == [] and ss.active == [] and ss.mix_of(1) == (0.0, 1.0)
    ss.close(1)                                                     # acknowledges; the mix is the caller's
    assert ss.faults() == [] and ss.mix_of(1) == (0.0, 1.0)


def test_paced_held_slot_is_silent_and_its_gains_wait(emu_net, clips):
    mix, emb = clips
    ramp = 256
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, pace=True, monitor=True, monitor_ramp=ramp)
    ss.set_mix(1, 0.0, 1.0)
    feed, zero, gain = feed_both(mix), torch.zeros(2, HOP), (1.0, 0.0)
    y = ss.step(feed(0), present=[True, True]).clone()
    want, gain = restated(feed(0)[1], zero, gain, (0.0, 1.0), ramp)
    assert C.same_bits(y[1], want) and ss._mix[1, :, 1].tolist() == [0.5, 0.5]
    late = feed(1).clone()
    late[1] = NAN
    y = ss.step(late, present=[True, False])
    assert C.same_bits(y[1], zero) and ss._mix[1, :, 1].tolist() == [0.5, 0.5] and ss.faults() == []
    y = ss.step(feed(1), present=[True, True])
    want, gain = restated(feed(1)[1], zero, gain, (0.0, 1.0), ramp)
    assert C.same_bits(y[1], want) and ss._mix[1, :, 1].tolist() == [0.0, 1.0] and not y[0].any()


def test_client_rate_rows_are_the_resampled_mix(emu_net, emu_lib):
    """48 kHz clients, slot 0 idle at (0, 1), slot 1 at the defaults: the client rows are what `lh_session_resample_out`
    makes of the MIXED 16 kHz rows — `Resampler(16000, 48000)` of `delay_out` zeros followed by them."""
    ramp, n_chunks = 100, 3
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, pace=True, packets=True, client_rate=48000, monitor=True,
                                       monitor_ramp=ramp)
    ss.set_mix(0, 0.0, 1.0)
    torch.manual_seed(5)
    x48 = torch.randn(2, 3 * (HOP * n_chunks + NFFT - HOP) + ss.lookahead_in) * 0.1
    ss.push({0: x48, 1: x48})
    rows16, rows48, gain, zero = [], [], (1.0, 0.0), torch.zeros(2, HOP)
    while ss.ready():
        y = ss.step().clone()
        assert ss.last_present == (True, True) and tuple(y.shape) == (S, 2, 384)
        want, gain = restated(ss.chunk_in[0], zero, gain, (0.0, 1.0), ramp)
        assert C.same_bits(ss.out[0], want) and not ss.out[1].any() and not y[1].any()
        rows16.append(ss.out[0].clone()), rows48.append(y[0])
    assert len(rows16) == n_chunks and C.same_bits(rows16[-1], ss.chunk_in[0, :, :HOP] + 0.0)
    up = EmuResampler(16000, 48000)
    up.emu_lib = emu_lib
    mine = torch.cat(rows48, -1)
    want = up(torch.cat([torch.zeros(2, ss.delay_out)] + rows16, -1))[:, :mine.shape[-1]]
    assert torch.equal(mine, want) and mine.abs().max() > 1e-2


def test_relook_keeps_the_session_and_retargets_it(emu_net, clips, plain):
    """Slot 0 is open; `relook` before step 1 records chunks 1 and 2 beside the running session; the poll of step 3 embeds
    and re-targets.  Until then the rows are those of a streamer that never relooked; from then on those of a twin on which
    `set_embedding(0, that embedding)` was called before the same step."""
    mix, emb = clips
    feed, e = feed_both(mix), FakeEmbed()
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=2)
    with pytest.raises(ValueError, match="not open"):
        ss.relook(0, NoEmbed())
    ss.open(0, emb[0])
    seen = []

    def look():
        ss.relook(0, e)
        assert ss.active == [0] and ss.enrolling == [0]
        for refused in (lambda: ss.suspend(0), lambda: ss.suspend_many([0]), lambda: ss.enroll(0, NoEmbed()),
                        lambda: ss.relook(0, NoEmbed()), lambda: ss.open(0, emb[1]), lambda: ss.embedding_of(0)):
            with pytest.raises(ValueError):
                refused()
    y = []
    for i in range(5):
        if i == 1:
            look()
        seen.append((ss.active, ss.enrolling))
        y.append(ss.step(feed(i)).clone())
    assert seen == [([0], []), ([0], [0]), ([0], [0]), ([0], [0]), ([0], [])] and ss.faults() == []
    for i in range(3):
        assert C.same_bits(y[i], plain[i]), i
    clip = mix[0][:, HOP:3 * HOP]
    assert len(e.calls) == 1 and torch.equal(e.calls[0], clip[None])                # once, on exactly the recorded samples
    new = clip[0, :256]
    assert torch.equal(ss.embedding_of(0), new)
    twin = emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=2)
    twin.open(0, emb[0])
    yt = run(twin, 5, feed, {3: lambda: twin.set_embedding(0, new)})
    for i in range(5):
        assert C.same_bits(y[i], yt[i]), i
    assert not C.same_bits(y[4], plain[4])                          # the new target is heard
    assert not ss._ewords.any() and ss._relook == set()
    plain_ss = emu_net.make_session_streamer(S, "cpu", use_graph=False)
    with pytest.raises(ValueError, match="enroll_chunks"):
        plain_ss.relook(0, NoEmbed())


def test_close_in_mid_look_cancels_it_and_closes_the_session(emu_net, clips):
    mix, emb = clips
    feed = feed_both(mix)
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=3)
    ss.open(0, emb[0])
    ss.step(feed(0))
    ss.relook(0, NoEmbed())
    assert ss.step(feed(1))[0].abs().max() > 1e-5 and ss._ewords[1:].tolist() == [[ss._next_gen - 1, 0], [1, 0]]
    ss.close(0)
    assert ss.active == [] and ss.enrolling == [] and ss._relook == set()
    for i in (2, 3):
        assert not ss.step(feed(i)).any()
    assert not ss._ewords.any() and not ss._edone.any() and not ss._words.any()
    assert ss.active == [] and ss.enrolling == [] and ss.faults() == [] and not ss._capturing and not ss._epending


def test_relook_in_a_compacting_streamer_keeps_the_row(emu_net, clips):
    """Slot 1 lives in row 0 of a compacting streamer and stays there while it looks again; its rows during the capture are
    those of a twin that does not."""
    mix, emb = clips
    feed, e = feed_both(mix), FakeEmbed()
    pair = [emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=2, compact=True) for _ in range(2)]
    ys = []
    for ss, looks in zip(pair, (False, True)):
        ss.open(1, emb[1])
        rows = []
        for i in range(4):
            if looks and i == 1:
                ss.relook(1, e)
            rows.append(ss.step(feed(i)).clone())
            assert ss._row_of == [-1, 0] and ss.rows_in_use == 1 and ss.last_rows == 1 and ss.active == [1], i
            if looks:
                assert ss.enrolling == ([1] if i in (1, 2) else []), i
        ys.append(rows)
    for i in range(3):
        assert C.same_bits(ys[1][i], ys[0][i]), i
    assert len(e.calls) == 1 and torch.equal(pair[1].embedding_of(1), mix[1][0, HOP:HOP + 256])
    assert not C.same_bits(ys[1][3], ys[0][3]) and ys[1][3][1].abs().max() > 1e-5


def test_monitor_api_errors(emu_net):
    mk = emu_net.make_session_streamer
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="monitor_ramp"):
            mk(S, "cpu", use_graph=False, monitor=True, monitor_ramp=bad)
    plain_ss = mk(S, "cpu", use_graph=False)
    for call in (lambda: plain_ss.set_mix(0, 1.0, 0.0), lambda: plain_ss.mix_of(0)):
        with pytest.raises(ValueError, match="monitor"):
            call()
    ss = mk(S, "cpu", use_graph=False, monitor=True, monitor_ramp=1)
    with pytest.raises(ValueError, match="enroll_chunks"):
        ss.enroll(0, NoEmbed(), passthrough=True)
    for wet, dry in ((NAN, 0.0), (0.0, float("inf")), (-0.1, 0.0), (0.0, 1.5), (1.0000001, 0.0)):
        with pytest.raises(ValueError, match="finite"):
            ss.set_mix(0, wet, dry)
    for slot in (S, -1):
        with pytest.raises(IndexError):
            ss.set_mix(slot, 1.0, 0.0)
        with pytest.raises(IndexError):
            ss.mix_of(slot)
    assert ss.mix_of(0) == (1.0, 0.0) and ss._mix_posted
    ss.set_mix(0, 1.0, 0.0)                                         # no change: nothing to copy
    assert ss._mix_posted
    ss.set_mix(0, 0.1, 0.7)
    assert not ss._mix_posted and ss.mix_of(0) == (float(F32(0.1)), float(F32(0.7)))
