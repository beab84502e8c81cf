"""CPU: any client rate (ABI 31) — `lh_session_resample_out_any` (lh_stream.hip) by direct C-ABI calls, `lh_session_resample_in` at
the 441 / 160 ratio, and `SessionStreamer(pace=True, packets=True, client_rate=44100, any_rate=True)` (sessions.py) over the
emulated library, eager.  The node shares `lh_resample`'s inner product, so everything it makes is `torch.equal` to `lh_resample`
of the whole stream behind d zeros; the counts are held to the integers of tests/any_rate_cases.py."""
import ctypes

import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.resample import Resampler, resample_bank
from tests import any_rate_cases as A
from tests.any_rate_cases import ARG, F32, HOP, NFFT, S16, V
from tests.hipemu.hosts import EmuHost, EmuNet
from oracle import tfgridnet_oracle as O

M32 = 0xffffffff
i32 = lambda v: v - (1 << 32) if v >> 31 else v


class EmuResampler(EmuHost, Resampler):
    """The product `Resampler` over the emulated library and host tensors."""


class EmuSessionNet(EmuNet):
    def _host_words(self, n, device):
        return torch.zeros(n, dtype=torch.int32)

    def _enroll_side(self, dev):
        return None


@pytest.fixture(scope="module")
def emu_lib():
    from tests.hipemu.build_emu import build_emu
    return _cabi.Lib(build_emu())


def resampler(lib, orig, new):
    r = EmuResampler(orig, new)
    r.emu_lib = lib
    return r


def test_the_restated_geometry():
    g = A.Geometry(44100)
    assert (g.width, g.o, g.n, g.K, g.d, g.P, g.T, g.hop_max) == (7, 160, 441, 174, 166, 5, 334, 353)
    assert g.counts(7) == [352, 353, 353, 353, 353, 352, 353] and g.c(g.P) == 4 * 441
    g = A.Geometry(11025)
    assert (g.o, g.n, g.P, g.T, g.T + HOP, g.hop_max) == (640, 441, 5, 1299, A.STAGE, 89)
    assert [A.Geometry(r).P for r in (22050, 88200, 48000, 24000, 8000, 12000)] == [5, 5, 1, 1, 1, 1]


# ---- the node against the whole stream ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [44100, 11025, 88200, 48000])
def test_node_is_the_delayed_whole_stream(emu_lib, rate):
    """Three slots, 12 steps (more than two periods): slot 0 always live, slots 1 and 2 held at steps of their own."""
    bank = resample_bank(16000, rate)[0]
    live = A.run_node(emu_lib.raw("lh_session_resample_out_any"), None, "cpu", rate, 3, 12, bank, resampler(emu_lib, 16000, rate))
    assert live == [12, 8, 9]


# ---- the phase word -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [44100, 11025])
def test_a_phase_word_out_of_range_behaves_as_its_value_mod_p(emu_lib, rate):
    raw = emu_lib.raw("lh_session_resample_out_any")
    g = A.Geometry(rate)
    bank_t = resample_bank(16000, rate)[0].t().contiguous()
    torch.manual_seed(5)
    out, tail0, hold = torch.randn(2, 2, HOP) * 0.4, torch.randn(2, 2, g.T) * 0.4, torch.zeros(2, dtype=torch.int32)

    def run(words):
        tail, phase = tail0.clone(), torch.tensor([i32(w) for w in words], dtype=torch.int32)
        y, cnt = torch.full((2, 2, g.hop_max), 9.0), torch.full((2,), -1, dtype=torch.int32)
        assert raw(*A.node_args(out, tail, phase, hold, y, cnt, F32, bank_t, g), None) == 0
        return y, tail, cnt.tolist(), phase.tolist()

    wild, p = M32 % g.P, g.P
    assert wild == 0 and g.P == 5                                # 2^32 - 1 is a multiple of 5
    for words in ((M32, p), (M32 - 1, p + 3)):
        want = [w % g.P for w in words]
        ya, ta, ca, pa = run(words)
        yb, tb, cb, pb = run(want)
        assert torch.equal(ya, yb) and torch.equal(ta, tb) and ca == cb and pa == pb == [(r + 1) % g.P for r in want]
        assert ca == [g.c(r + 1) - g.c(r) for r in want] and ya.abs().max() > 0.1


# ---- argument validation ------------------------------------------------------------------------------------------------------
def test_node_validates_arguments(emu_lib):
    raw = emu_lib.raw("lh_session_resample_out_any")
    g = A.Geometry(44100)
    bank_t = resample_bank(16000, 44100)[0].t().contiguous()
    out, tail, hold = torch.randn(2, 2, HOP), torch.zeros(2, 2, g.T), torch.zeros(2, dtype=torch.int32)
    phase, cnt = torch.full((2,), 3, dtype=torch.int32), torch.full((2,), -1, dtype=torch.int32)
    y = torch.full((2, 2, g.hop_max), 9.0)
    a = A.node_args(out, tail, phase, hold, y, cnt, F32, bank_t, g) + [None]
    for i in (0, 1, 2, 3, 4, 5, 8):                              # every pointer
        assert raw(*(a[:i] + [None] + a[i + 1:])) == ARG, i
    for i in (0, 1, 4):                                          # the 16-byte base pointers
        assert raw(*(a[:i] + [ctypes.c_void_p(a[i].value + 4)] + a[i + 1:])) == ARG, i
    for i in (2, 3, 5):                                          # the words
        assert raw(*(a[:i] + [ctypes.c_void_p(a[i].value + 2)] + a[i + 1:])) == ARG, i
    for i, j in ((4, 0), (1, 0), (4, 1), (5, 2), (3, 2), (5, 3)):                # aliased buffers
        assert raw(*(a[:i] + [a[j]] + a[i + 1:])) == ARG, (i, j)
    for i, vals in ((6, (2, -1)), (7, (0, -1)), (9, (0, -1, 4097)), (10, (0, -1, 4097)), (11, (0, -3))):
        for bad in vals:
            assert raw(*(a[:i] + [bad] + a[i + 1:])) == ARG, (i, bad)
    # T + 128 beyond the staging: 11 025 Hz's ratio fits to the sample with its own width 9, not with 10
    big = A.Geometry(11025)
    assert raw(*(a[:9] + [big.o, big.n, big.width + 1] + a[12:])) == ARG
    assert raw(*(a[:9] + [4096, 1, 7] + a[12:])) == ARG
    assert (y == 9.0).all() and not tail.any() and phase.tolist() == [3, 3] and cnt.tolist() == [-1, -1]
    assert raw(*a) == 0 and not (y == 9.0).any() and phase.tolist() == [4, 4] and cnt.tolist() == [353, 353]
    tail11, y11 = torch.zeros(2, 2, big.T), torch.full((2, 2, big.hop_max), 9.0)
    bank11 = resample_bank(16000, 11025)[0].t().contiguous()
    assert raw(*A.node_args(out, tail11, phase, hold, y11, cnt, F32, bank11, big), None) == 0
    assert cnt.tolist() == [big.c(5) - big.c(4)] * 2 == [89, 89] and phase.tolist() == [0, 0]


# ---- the input side at 441 / 160 ----------------------------------------------------------------------------------------------
R, R_IN, S = 1024, 1024, 2
AT = 0xFFFFFF80                                                  # both counters start here: the ring's end and 2^32 are crossed
PACKETS = (1, 441, 457, 2, 3, 40, 41, 63, 480, 160, 441, 457, 1, 300, 7, 441, 441, 441, 457, 1, 1, 339)


def test_resample_in_at_441_over_160_equals_the_whole_stream(emu_lib):
    """Slot 1 of 2, as tests/test_emu_resample.py drives the 3 / 1 ratio: feed, then resample_in, with the host's integers."""
    bank, width, o, n = resample_bank(44100, 16000)
    K = 2 * width + o
    assert (width, o, n, K, width + o - 1) == (17, 441, 160, 475, 457)
    torch.manual_seed(3)
    x = torch.randint(-20000, 20000, (2, sum(PACKETS)), dtype=torch.int64).float() / 32768
    whole = resampler(emu_lib, 44100, 16000)(x)
    raw_ring, raw_words = torch.zeros(S, 2, R_IN), torch.tensor([[5, i32(AT)], [9, 0]], dtype=torch.int32)
    raw_ring[0] = 3.0
    fifo, wr = torch.full((S, 2, R), -5.0), torch.tensor([77, i32(AT)], dtype=torch.int32)
    raw_wr, tap, wr16, made, pos = AT, (AT - width) & M32, AT, 0, 0
    for size in PACKETS:
        st = x[:, pos:pos + size].contiguous().view(-1)
        items = torch.tensor([[1, 0, size, i32(raw_wr), 0]], dtype=torch.int32)
        assert emu_lib.raw("lh_session_feed")(V(st), st.numel() * 4, F32, V(items), 1, V(raw_ring), V(raw_words[0]),
                                              V(raw_words[1]), R_IN, S, None) == 0
        raw_wr, pos = (raw_wr + size) & M32, pos + size
        fill = (raw_wr - tap) & M32
        nb = 0 if fill < K else (fill - K) // o + 1
        if nb:
            rit = torch.tensor([[1, nb, i32(wr16), i32(tap)]], dtype=torch.int32)
            assert emu_lib.raw("lh_session_resample_in")(V(raw_ring), R_IN, V(rit), 1, V(fifo), V(wr), R, S, V(bank), o, n, width,
                                                         None) == 0
            wr16, tap = (wr16 + nb * n) & M32, (tap + nb * o) & M32
        got = nb * n
        assert made + got == (0 if pos + width < K else (pos + width - K) // o + 1) * n      # a block exists once its K samples do
        idx = (AT + made + torch.arange(got)) & (R - 1)
        assert torch.equal(fifo[1][:, idx], whole[:, made:made + got]), (size, pos)
        made += got
        assert wr.tolist() == [77, i32(wr16)] and (fifo[0] == -5.0).all() and (raw_ring[0] == 3.0).all()
    assert made > R and pos > 4 * R_IN and raw_wr < AT and wr16 < AT             # the rings' ends and the counters' wrap were crossed


# ---- the host over the emulated device ----------------------------------------------------------------------------------------
N_CHUNKS, RATE = 6, 44100


@pytest.fixture(scope="module")
def emu_net(oracle_cfg_sd, emu_lib):
    cfg, sd = oracle_cfg_sd
    net = EmuSessionNet(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net.emu_lib = emu_lib
    return net


def test_any_rate_streamer_end_to_end(emu_net, emu_lib):
    """S = 2 at 44.1 kHz, the same stream for both slots: slot 0 in 441-sample packets, one a tick, slot 1 in one packet.  A
    listener's valid samples equal: the stream resampled offline, through a 16 kHz packet streamer, resampled offline behind
    `delay_out` zeros.  Then flush: that slot's tail and phase only, and its next rows start from silence at phase 0."""
    mk = emu_net.make_session_streamer
    g = A.Geometry(RATE)
    ss = mk(2, "cpu", use_graph=False, pace=True, packets=True, client_rate=RATE, any_rate=True)
    ref = mk(2, "cpu", use_graph=False, pace=True, packets=True)
    assert (ss.client_rate, ss.hop_client, ss.lookahead_in, ss.delay_out) == (RATE, 353, 457, 166)
    assert tuple(ss._tail.shape) == (2, 2, g.T) and ss.last_counts == (0, 0) and ref.last_counts == (0, 0)
    n16 = HOP * N_CHUNKS + NFFT - HOP
    total, made = A.client_len(RATE, n16)
    emb = synth.batch([30], n16)["embedding_gt"][0, 0]
    torch.manual_seed(30)
    x = torch.randn(2, total) * 0.1
    x16 = resampler(emu_lib, RATE, 16000)(x)[:, :n16]
    for s in (0, 1):
        ss.open(s, emb), ref.open(s, emb)
    ref.push({0: x16, 1: x16})
    ss.push({1: x})
    assert ss.buffered(1) == made and ss.buffered(0) == 0 and ss.ready() == [1]
    rows, log, theirs, pos = [], [], [], 0
    while pos < total or ss.ready():
        if pos < total:
            ss.push({0: x[:, pos:pos + 441]})
            pos += 441
            done = HOP * sum(p[0] for p, _ in log)
            assert ss.buffered(0) + done == (0 if pos + 17 < 475 else (min(pos, total) + 17 - 475) // 441 + 1) * 160
        y = ss.step().clone()
        assert tuple(y.shape) == (2, 2, 353)
        rows.append(y), log.append((ss.last_present, ss.last_counts))
        if len(theirs) < N_CHUNKS:
            theirs.append(ref.step().clone()[0])
            assert ref.last_counts == (HOP, HOP)
    y = torch.stack(rows)
    assert ss.faults() == []
    want = resampler(emu_lib, 16000, RATE)(torch.cat([torch.zeros(2, ss.delay_out), torch.cat(theirs, -1)], -1))
    n_out = g.c(g.P) + g.c(N_CHUNKS - g.P)                       # one period and a step: 1764 + 352
    for s in (0, 1):
        mine, live = A.listener(y, log, s, g)
        assert live >= N_CHUNKS and sum(c[s] for _, c in log) == mine.shape[-1] >= n_out
        assert torch.equal(mine[:, :n_out], want[:, :n_out]) and mine.abs().max() > 1e-4, s
    assert any(not p[0] for p, _ in log) and ss._phase.tolist() == ss._phase_of and ss._count.tolist() == list(ss.last_counts)
    # flush: slot 0's tail and phase, the host's and the device's; slot 1 keeps its own
    tail1, phase1 = ss._tail[1].clone(), ss._phase_of[1]
    assert ss._tail[0].any() and tail1.any() and ss._phase_of[0] and phase1      # both somewhere inside a period
    ss.flush(0)
    ss.push({0: x[:, :1400]})
    assert not ss._tail[0].any() and ss._phase.tolist() == ss._phase_of == [0, phase1] and torch.equal(ss._tail[1], tail1)
    assert ss.buffered(0) == 480 and torch.equal(ss._fifo[0, :, :480], x16[:, :480])
    got, rows16 = [], []                                         # two steps: the first lies inside the delay almost whole
    for want_count in (352, 353):
        y = ss.step().clone()
        assert ss.last_present == (True, False) and ss.last_counts == (want_count, 0) and not y[1].any()
        assert not y[0, :, want_count:].any()
        got.append(y[0, :, :want_count]), rows16.append(ss.out[0].clone())
    assert ss._phase.tolist() == ss._phase_of == [2, phase1] and torch.equal(ss._tail[1], tail1)
    fresh = resampler(emu_lib, 16000, RATE)(torch.cat([torch.zeros(2, ss.delay_out)] + rows16, -1))
    assert torch.equal(torch.cat(got, -1), fresh[:, :705]) and got[1].abs().max() > 1e-5
    ss.reset()
    assert not ss._tail.any() and ss._phase.tolist() == ss._phase_of == [0, 0] and ss.last_counts == (0, 0)


def test_any_rate_at_a_multiple_of_125_is_the_fixed_hop_streamer(emu_net):
    """`any_rate=True` at 48 kHz: the outputs of `any_rate=False`, through `lh_session_resample_out`."""
    mk = emu_net.make_session_streamer
    a = mk(2, "cpu", use_graph=False, pace=True, packets=True, client_rate=48000, any_rate=True)
    b = mk(2, "cpu", use_graph=False, pace=True, packets=True, client_rate=48000)
    assert not a._fractional and not hasattr(a, "_phase") and (a.hop_client, a.delay_out) == (b.hop_client, b.delay_out) == (384, 8)
    emb = synth.batch([31], 400)["embedding_gt"][0, 0]
    torch.manual_seed(31)
    x = torch.randn(2, 1400) * 0.1
    calls = []

    class Spy:
        def __init__(self, lib):
            self.lib = lib

        def call(self, name, *args):
            calls.append(name)
            return self.lib.call(name, *args)

        def __getattr__(self, name):
            return getattr(self.lib, name)

    lib, outs = emu_net.emu_lib, []
    emu_net.emu_lib = Spy(lib)
    try:
        for ss in (a, b):
            ss.open(0, emb)
            ss.push({0: x})
            ys = []
            while ss.ready():
                ys.append(ss.step().clone())
                assert ss.last_counts == (384, 0)
            outs.append(torch.stack(ys))
    finally:
        emu_net.emu_lib = lib
    assert outs[0].shape[0] == 3 and torch.equal(outs[0], outs[1]) and outs[0].abs().max() > 1e-4
    assert calls.count("lh_session_resample_out") == 6 and "lh_session_resample_out_any" not in calls
    half = len(calls) // 2
    assert calls[:half] == calls[half:]                          # launch for launch


def test_what_any_rate_refuses(emu_net):
    mk = emu_net.make_session_streamer
    with pytest.raises(ValueError, match="125") as e:
        mk(2, "cpu", use_graph=False, pace=True, packets=True, client_rate=44100)
    assert "any_rate=True" in str(e.value)
    with pytest.raises(ValueError, match="packets"):
        mk(2, "cpu", use_graph=False, pace=True, client_rate=44100, any_rate=True)
    for bad in (0, 500, 16001, 44101, 1 << 20):                  # out of range, or more to carry than 11 025 Hz
        with pytest.raises(ValueError):
            mk(2, "cpu", use_graph=False, pace=True, packets=True, client_rate=bad, any_rate=True)
    low = mk(2, "cpu", use_graph=False, pace=True, packets=True, pcm16=True, client_rate=11025, any_rate=True, fifo_samples=256)
    assert (low.hop_client, low.delay_out, low._period) == (89, 648, 5) and low.out_client.dtype == torch.int16
    assert tuple(low._tail.shape) == (2, 2, 1299)
