"""CPU: enrollment from a listener's own stream — `lh_session_capture` (lh_stream.hip) by direct C-ABI calls, and
`SessionStreamer.enroll / poll` (sessions.py) over the emulated library, eager.  The side stream of the GPU host is replaced by a
synchronous stand-in here (as `SerialLanes` replaces `_Lanes`): every other host line is the one the GPU runs.  Copies and
isolation claims are `torch.equal`; a session's reference is the oracle's fresh stream within the emulator tolerance of
tests/test_emu_kernels.py.  Small on purpose: the emulator runs a chunk row in ~0.5 s."""
import ctypes

import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from tests.hipemu.hosts import EmuEmbed, EmuNet
from oracle import embedder_oracle as E
from oracle import tfgridnet_oracle as O

TOL = 5e-5          # tests/test_emu_kernels.py
HOP, NFFT = 128, 192
ARM, CANCEL, SHIFT, FAULT, ERR_ARG = 1, 2, 8, 0x80000000, 1


class SyncSide:
    """Stand-in for `net._EnrollSide`: the emulator executes every launch at once, so the embedder call has finished when
    `run` returns.  `hold` keeps "is it done" false, to look at a slot while its embedding is in flight."""
    hold = False

    def run(self, fn):
        return fn(), None

    def finished(self, done):
        return not self.hold

    def hand_over(self, done, out):
        pass


class EmuEnrollNet(EmuNet):
    def _host_words(self, n, device):               # the pinned words of the GPU host: plain host memory here
        return torch.zeros(n, dtype=torch.int32)

    def _enroll_side(self, dev):
        return SyncSide()


class RecordingEmbed(EmuEmbed):
    """Keeps what it was called with."""
    calls = None

    def forward(self, input):
        if self.calls is not None:
            self.calls.append(input.clone())
        return super().forward(input)


@pytest.fixture(scope="module")
def emu_lib():
    from tests.hipemu.build_emu import build_emu
    return _cabi.Lib(build_emu())


@pytest.fixture(scope="module")
def emu_net(oracle_cfg_sd, emu_lib):
    cfg, sd = oracle_cfg_sd
    net = EmuEnrollNet(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net.emu_lib = emu_lib
    return net


@pytest.fixture(scope="module")
def embedder(emu_lib):
    net = RecordingEmbed(**E.EMBED_PARAMS).eval()
    net.load_state_dict(E.synthetic_state_dict(E.ECfg(**E.EMBED_PARAMS), 0), strict=True)
    net.emu_lib = emu_lib
    return net


@pytest.fixture(scope="module")
def clips():
    """Two 12-chunk binaural mixtures with their speaker embeddings."""
    d = synth.batch([20, 21], HOP * 12 + NFFT - HOP)
    return d["mixture"], d["embedding_gt"][:, 0]


def chunk_of(mix_row, j):
    return mix_row[:, j * HOP:j * HOP + NFFT]


# ---- the entry point on hand-made buffers ----------------------------------------------------------------------------------
class Capture:
    S, N = 3, 3

    def __init__(self, lib):
        S, N = self.S, self.N
        self.lib = lib
        self.enroll = torch.full((S, 2, HOP * N), -7.0)             # sentinel
        self.words = torch.zeros(3, S, dtype=torch.int32)           # ecmd | estate[2]
        self.edone = torch.zeros(S, dtype=torch.int32)
        self.rows = []                                              # slot 1's rows as fed
        self.gen = torch.Generator().manual_seed(3)

    def call(self, row=None):
        """One chunk: slot 1's row is random (or `row`), the rows of slots 0 and 2 are NaN."""
        x = torch.full((self.S, 2, NFFT), float("nan"))
        x[1] = torch.randn(2, NFFT, generator=self.gen) if row is None else row
        self.rows.append(x[1].clone())
        keep = x.clone()
        self.lib.call("lh_session_capture", x.data_ptr(), self.enroll.data_ptr(), self.words.data_ptr(),
                      self.words[1].data_ptr(), self.edone.data_ptr(), self.N, self.S, None)
        assert torch.equal(torch.nan_to_num(x, nan=5.0), torch.nan_to_num(keep, nan=5.0))      # the input is never written
        return x[1]

    def post(self, slot, word):
        self.words[0, slot] = word

    def state(self):
        return self.words[1:].tolist()

    def done(self, slot):
        return int(self.edone[slot]) & 0xffffffff


def sentinel(t):
    return bool(t.eq(-7.0).all())


def test_capture_word_protocol(emu_lib):
    k = Capture(emu_lib)
    k.call()                                                        # nobody armed: nothing happens
    assert sentinel(k.enroll) and not k.words.any() and not k.edone.any()
    k.post(1, ARM | (5 << SHIFT))
    k.call()
    assert k.words[0].tolist() == [0, 0, 0]                         # consumed
    assert k.state() == [[0, 5, 0], [0, 1, 0]] and k.done(1) == 0
    k.call()
    assert k.state() == [[0, 5, 0], [0, 2, 0]] and k.done(1) == 0
    k.call()
    assert k.state() == [[0, 0, 0], [0, 0, 0]] and k.edone.tolist() == [0, 5, 0]
    clip = torch.cat([r[:, :HOP] for r in k.rows[1:4]], -1)         # the first 128 samples of the three armed rows
    assert torch.equal(k.enroll[1], clip)
    k.call()                                                        # disarmed: a fourth call changes nothing
    assert torch.equal(k.enroll[1], clip) and k.state() == [[0, 0, 0], [0, 0, 0]] and k.edone.tolist() == [0, 5, 0]
    assert sentinel(k.enroll[0]) and sentinel(k.enroll[2]) and not k.words.any()


def test_capture_is_the_contiguous_stream(emu_lib):
    """Rows cut from one stream (64 samples of look-ahead shared with the next row): the clip is the stream itself."""
    k = Capture(emu_lib)
    stream = torch.randn(2, HOP * 3 + NFFT - HOP, generator=k.gen)
    k.post(1, ARM | (9 << SHIFT))
    for j in range(3):
        k.call(chunk_of(stream, j))
    assert torch.equal(k.enroll[1], stream[:, :HOP * 3]) and k.done(1) == 9


def test_capture_cancel(emu_lib):
    k = Capture(emu_lib)
    k.post(1, ARM | (5 << SHIFT))
    k.call(), k.call()
    k.post(1, CANCEL)
    k.call()
    assert not k.words.any() and not k.edone.any()
    third = k.enroll[1, :, 2 * HOP:].clone()
    k.call()
    assert sentinel(third) and torch.equal(k.enroll[1, :, 2 * HOP:], third) and not k.edone.any()


def test_capture_nonfinite_recorded_sample_aborts(emu_lib):
    k = Capture(emu_lib)
    k.post(1, ARM | (5 << SHIFT))
    k.call(), k.call()
    bad = torch.randn(2, NFFT, generator=k.gen)
    bad[1, 127] = float("nan")                                      # the last recorded sample of chunk 2
    k.call(bad)
    assert k.done(1) == 5 | FAULT and k.state() == [[0, 0, 0], [0, 0, 0]] and k.edone[0] == 0 and k.edone[2] == 0
    before = k.enroll.clone()
    k.call()
    assert torch.equal(k.enroll, before) and k.done(1) == 5 | FAULT and not k.words.any()
    assert sentinel(k.enroll[1, :, 2 * HOP:])                       # the bad row was not stored


def test_capture_nonfinite_lookahead_alone_does_not_abort(emu_lib):
    k = Capture(emu_lib)
    k.post(1, ARM | (5 << SHIFT))
    k.call(), k.call()
    last = torch.randn(2, NFFT, generator=k.gen)
    last[0, 130] = float("nan")                                     # look-ahead: a recorded sample of the NEXT chunk only
    k.call(last)
    assert k.done(1) == 5 and torch.equal(k.enroll[1], torch.cat([r[:, :HOP] for r in k.rows], -1))
    assert torch.isfinite(k.enroll[1]).all()


def test_capture_arm_during_a_capture_restarts_it(emu_lib):
    k = Capture(emu_lib)
    k.post(1, ARM | (5 << SHIFT))
    k.call(), k.call()
    k.post(1, ARM | (6 << SHIFT))
    k.call()
    assert k.state() == [[0, 6, 0], [0, 1, 0]] and not k.edone.any()
    k.call(), k.call()
    assert k.edone.tolist() == [0, 6, 0] and k.state() == [[0, 0, 0], [0, 0, 0]]
    assert torch.equal(k.enroll[1], torch.cat([r[:, :HOP] for r in k.rows[2:5]], -1))


def test_capture_validates_arguments(emu_lib):
    k = Capture(emu_lib)
    f = emu_lib.raw("lh_session_capture")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    x = torch.zeros(k.S, 2, NFFT)
    ok = [P(x), P(k.enroll), P(k.words), P(k.words[1]), P(k.edone), k.N, k.S, None]
    assert f(*ok) == 0
    for i in range(5):                                              # a null pointer
        a = list(ok)
        a[i] = None
        assert f(*a) == ERR_ARG, i
    for S in (0, -1):
        assert f(*ok[:6], S, None) == ERR_ARG
    for n in (0, -3):
        assert f(*ok[:5], n, k.S, None) == ERR_ARG
    a = list(ok)
    a[1] = ctypes.c_void_p(k.enroll.data_ptr() + 4)                 # enroll not 16-byte aligned
    assert f(*a) == ERR_ARG
    assert sentinel(k.enroll) and not k.words.any() and not k.edone.any()


# ---- the host ------------------------------------------------------------------------------------------------------------
def run(ss, S, n, feed, events=None):
    """n steps; feed(i) -> {slot: chunk [2, 192]} (rows not named are NaN), events {i: fn} run before step i -> [S, 2, 128 n]."""
    outs = []
    for i in range(n):
        if events and i in events:
            events[i]()
        x = torch.full((S, 2, NFFT), float("nan"))
        for slot, c in feed(i).items():
            x[slot] = c
        outs.append(ss.step(x).clone())
    return torch.cat(outs, -1)


def test_enroll_opens_the_slot_on_its_own_stream(emu_net, embedder, clips, oracle_cfg_sd):
    """S = 2, four chunks = 512 samples = 9 embedder frames.  Slot 0 is open from chunk 0; slot 1 enrolls at chunk 1 (odd: the
    capture starts in the second of the two alternating bodies) on its own stream, whose chunks 0..3 are the clip."""
    cfg, sd = oracle_cfg_sd
    mix, emb = clips
    S, n, at, N = 2, 8, 1, 4
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=N)
    ss.open(0, emb[0])
    seen = {}
    embedder.calls = []

    def feed(i):
        seen[i] = (ss.active, ss.enrolling)
        return {0: chunk_of(mix[0], i), **({1: chunk_of(mix[1], i - at)} if i >= at else {})}
    y = run(ss, S, n, feed, {at: lambda: ss.enroll(1, embedder)})
    calls, embedder.calls = embedder.calls, None
    opened = at + N                                                 # the step whose poll sees the fourth chunk recorded
    for i in range(n):                                              # looked at BEFORE step i, whose poll is what moves things
        assert seen[i] == (([0], []) if i < at else ([0], [1]) if i <= opened else ([0, 1], [])), (i, seen[i])
    assert ss.active == [0, 1] and ss.enrolling == [] and ss.faults() == []
    clip = mix[1][:, :HOP * N]
    assert len(calls) == 1 and torch.equal(calls[0], clip[None])
    e1 = ss.embedding_of(1)
    assert e1.shape == (256,) and torch.equal(e1, embedder(clip[None])[0])
    # before its opening: exact zeros; from then on: the oracle's fresh stream of its own samples with that embedding
    assert torch.equal(y[1, :, :opened * HOP], torch.zeros(2, opened * HOP))
    own = mix[1][:, (opened - at) * HOP:]
    ref, _ = O.predict(cfg, sd, own[None, :, :HOP * (n - opened) + NFFT - HOP], e1[None], None, pad=False)
    err = float((y[1, :, opened * HOP:] - ref[0]).abs().max())
    print("slot 1 opened by enrollment at chunk", opened, ": max|emu - oracle fresh stream| =", err)
    assert err < TOL
    # slot 0 is bit-identical to a run in which slot 1 never enrolls
    alone = emu_net.make_session_streamer(S, "cpu", use_graph=False, enroll_chunks=N)
    alone.open(0, emb[0])
    ya = run(alone, S, n, lambda i: {0: chunk_of(mix[0], i)})
    assert torch.equal(ya[0], y[0]) and torch.equal(ya[1], torch.zeros(2, n * HOP))
    with pytest.raises(ValueError):
        ss.embedding_of(0)                                          # opened by hand


class NoEmbed:
    """An embedder that must not be called."""
    def __call__(self, x):
        raise AssertionError("the embedder ran")


class FakeEmbed:
    """The first 256 samples of the clip's left channel: enough to see which clip opened a slot."""
    def __call__(self, x):
        return x[:, 0, :256].contiguous()


def zeros_in(S):
    return torch.zeros(S, 2, NFFT)


def test_enroll_api_errors(emu_net, clips):
    mix, emb = clips
    with pytest.raises(ValueError):
        emu_net.make_session_streamer(2, "cpu", use_graph=False, enroll_chunks=1)
    with pytest.raises(ValueError):
        emu_net.make_session_streamer(2, "cpu", use_graph=False, enroll_chunks=-2)
    plain = emu_net.make_session_streamer(2, "cpu", use_graph=False)
    assert plain.enrolling == []
    with pytest.raises(ValueError):
        plain.enroll(0, NoEmbed())
    ss = emu_net.make_session_streamer(2, "cpu", use_graph=False, enroll_chunks=2)
    for bad in (2, -1):
        with pytest.raises(IndexError):
            ss.enroll(bad, NoEmbed())
        with pytest.raises(IndexError):
            ss.embedding_of(bad)
    ss.open(0, emb[0])
    with pytest.raises(ValueError):
        ss.enroll(0, NoEmbed())                                     # open
    ss.enroll(1, NoEmbed())
    assert ss.enrolling == [1]
    with pytest.raises(ValueError):
        ss.enroll(1, NoEmbed())                                     # twice
    with pytest.raises(ValueError):
        ss.open(1, emb[1])                                          # enrolling: close() it first
    with pytest.raises(ValueError):
        ss.embedding_of(1)


def test_close_during_capture_cancels(emu_net):
    ss = emu_net.make_session_streamer(2, "cpu", use_graph=False, enroll_chunks=3)
    ss.enroll(1, NoEmbed())
    ss.step(zeros_in(2)), ss.step(zeros_in(2))
    assert ss._ewords[1:].tolist() == [[0, ss._next_gen - 1], [0, 2]]
    ss.close(1)
    assert ss.enrolling == []
    for _ in range(3):
        assert not ss.step(zeros_in(2)).any()
    assert not ss._ewords.any() and not ss._edone.any() and ss.active == [] and ss.enrolling == [] and ss.faults() == []


def test_close_during_embedding_cancels_and_a_stale_result_is_dropped(emu_net):
    """The embedder call is held "in flight" by the stand-in: close() then enroll() again — the first call's row must not open
    the slot, the second one's does."""
    ss = emu_net.make_session_streamer(2, "cpu", use_graph=False, enroll_chunks=2)
    ss._side.hold = True
    ss.enroll(0, FakeEmbed())
    a = torch.randn(3, 2, 2, NFFT)
    ss.step(a[0]), ss.step(a[1])
    ss.poll()
    assert ss.enrolling == [0] and len(ss._jobs) == 1 and ss.active == []
    ss.poll()                                                       # idempotent
    assert len(ss._jobs) == 1
    ss.close(0)
    assert ss.enrolling == []
    ss.enroll(0, FakeEmbed())                                       # at once, while the first call is still "running"
    b = torch.randn(2, 2, 2, NFFT)
    ss.step(b[0])
    ss._side.hold = False
    ss.poll()                                                       # the stale call completes: dropped by its generation
    assert ss.active == [] and ss.enrolling == [0] and ss._jobs == []
    ss.step(b[1])
    ss.poll()
    assert ss.active == [0] and ss.enrolling == []
    assert torch.equal(ss.embedding_of(0), torch.cat([b[0, 0, 0, :HOP], b[1, 0, 0, :HOP]]))
    # ... and a close() while embedding with nothing after it: the slot never opens
    ss._side.hold = True
    ss.enroll(1, FakeEmbed())
    ss.step(a[0]), ss.step(a[1]), ss.step(a[2])
    assert ss.enrolling == [1]
    ss.close(1)
    ss._side.hold = False
    for _ in range(2):
        ss.step(a[2])
    assert ss.active == [0] and ss.enrolling == [] and ss._jobs == []


def test_reset_cancels(emu_net):
    ss = emu_net.make_session_streamer(2, "cpu", use_graph=False, enroll_chunks=2)
    ss._side.hold = True
    ss.enroll(0, FakeEmbed()), ss.enroll(1, NoEmbed())
    ss.step(zeros_in(2))
    ss.close(1), ss.step(zeros_in(2)), ss.poll()                    # slot 0 embedding
    ss.enroll(1, NoEmbed())
    ss.step(zeros_in(2))                                            # slot 1 capturing
    assert ss.enrolling == [0, 1]
    ss.reset()
    ss._side.hold = False
    assert ss.enrolling == [] and not ss._ewords.any() and not ss._edone.any()
    for _ in range(3):
        assert not ss.step(zeros_in(2)).any()
    assert ss.active == [] and ss.enrolling == [] and ss.faults() == [] and ss._jobs == []


def test_aborted_capture_is_a_fault_and_the_slot_enrolls_again(emu_net):
    ss = emu_net.make_session_streamer(2, "cpu", use_graph=False, enroll_chunks=2)
    ss.enroll(1, NoEmbed())
    x = torch.randn(2, 2, NFFT)
    ss.step(x)
    bad = x.clone()
    bad[1, 0, 3] = float("inf")
    assert not ss.step(bad).any()                                   # never raises
    assert ss.faults() == [1] and ss.enrolling == [] and ss.active == []
    ss.step(x)
    assert ss.faults() == [1] and ss.active == []
    ss.enroll(1, FakeEmbed())                                       # at once
    assert ss.faults() == [] and ss.enrolling == [1]
    ss.step(x), ss.step(x), ss.step(x)
    assert ss.active == [1] and ss.faults() == []


def test_captures_completed_in_one_poll_share_one_embedder_call(emu_net):
    """Slots 2 and 0 (armed in that order) finish in the same step, slot 1 a step later: one call with the batch in ascending
    slot order, then a call of its own."""
    calls = []

    class Embed(FakeEmbed):
        def __call__(self, x):
            calls.append(x.clone())
            return super().__call__(x)
    e = Embed()
    ss = emu_net.make_session_streamer(3, "cpu", use_graph=False, enroll_chunks=2)
    x = torch.randn(4, 3, 2, NFFT)
    ss.enroll(2, e), ss.enroll(0, e)
    ss.step(x[0])
    ss.enroll(1, e)
    ss.step(x[1]), ss.step(x[2])
    assert ss.active == [0, 2] and ss.enrolling == [1]
    ss.step(x[3])
    assert ss.active == [0, 1, 2] and [tuple(c.shape) for c in calls] == [(2, 2, 2 * HOP), (1, 2, 2 * HOP)]
    clip = lambda s, i: torch.cat([x[i, s, :, :HOP], x[i + 1, s, :, :HOP]], -1)
    assert torch.equal(calls[0], torch.stack([clip(0, 0), clip(2, 0)])) and torch.equal(calls[1], clip(1, 1)[None])
    for s, i in ((0, 0), (2, 0), (1, 1)):
        assert torch.equal(ss.embedding_of(s), clip(s, i)[0, :256])
