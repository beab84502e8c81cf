"""CPU: client-rate resampling (ABI 23) — `lh_resample` (lh_render.hip), `lh_session_resample_in`, `lh_session_resample_out`
(lh_stream.hip) and `SessionStreamer(pace=True, packets=True, client_rate=...)` (sessions.py) over the emulated library, eager.
`lh_resample` is held to the float64 restatement of tests/resample_cases.py within the derived fp32 dot-product bound; the
session nodes share its inner product, so everything they make is `torch.equal` to `lh_resample` of the whole stream."""
import ctypes

import numpy as np
import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.resample import Resampler, resample_bank
from tests import resample_cases as C
from tests.hipemu.hosts import EmuHost, EmuNet
from oracle import tfgridnet_oracle as O

HOP, NFFT = 128, 192
ARG = 1
F32, S16 = 0, 1
M32 = 0xffffffff
V = lambda v: ctypes.c_void_p(v.data_ptr())
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


# ---- lh_resample against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", C.KERNEL_PAIRS)
def test_resample_matches_float64_within_the_dot_product_bound(emu_lib, orig, new):
    bank, width, o, n = C.bank64(orig, new)
    K = bank.shape[1]
    rs = resampler(emu_lib, orig, new)
    assert (rs.width, rs.o, rs.n) == (width, o, n)
    worst = 0.0
    for rows in C.ROWS:
        for N in C.kernel_lengths(orig, new):
            torch.manual_seed(N + rows)
            x = torch.randn(rows, N) * 0.5
            y = rs(x)
            want, mag = C.resample64(x.numpy(), bank, width, o, n)
            assert tuple(y.shape) == want.shape == (rows, C.out_len(N, o, n))
            err, lim = np.abs(y.numpy().astype(np.float64) - want), C.bound(mag, K)
            worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
            print(f"{orig}->{new} rows {rows} N {N}: max err {err.max():.3e}, largest err / bound {(err / np.maximum(lim, 1e-300)).max():.4f}")
            assert (err <= lim).all(), (orig, new, rows, N, float(err.max()))
    assert 0.0 < worst <= 1.0


def test_resampler_call_semantics(emu_lib):
    rs = resampler(emu_lib, 48000, 16000)
    x = torch.randn(2, 3, 100)
    y = rs(x)
    assert tuple(y.shape) == (2, 3, 34) and torch.equal(y[1, 2], rs(x[1, 2]))        # leading dimensions are rows
    assert torch.equal(rs(x[0, :, 1:]), rs(x[0, :, 1:].clone()))                     # a view that is not 16-byte aligned
    assert tuple(rs(torch.zeros(2, 0)).shape) == (2, 0)
    same = resampler(emu_lib, 16000, 16000)
    assert same(x) is x
    with pytest.raises(ValueError):
        rs(x.double())
    with pytest.raises(RuntimeError, match="no CPU path"):
        Resampler(48000, 16000)(x)                                                   # the product class refuses host tensors
    import lookoncetohear_amd
    assert lookoncetohear_amd.Resampler is Resampler and lookoncetohear_amd.resample_bank is resample_bank


def test_resample_validates_arguments(emu_lib):
    raw = emu_lib.raw("lh_resample")
    bank, width, o, n = resample_bank(48000, 16000)
    x, y = torch.randn(2, 90), torch.full((2, 30), 7.0)
    a = [V(x), V(y), V(bank), 2, 90, 30, o, n, width, None]
    for i in range(3):
        assert raw(*(a[:i] + [None] + a[i + 1:])) == ARG, i
    odd = ctypes.c_void_p(x.data_ptr() + 4)
    assert raw(*([odd] + a[1:])) == ARG
    for i, bad in ((3, 0), (3, 65536), (4, 0), (5, 29), (5, 31), (6, 0), (6, 4097), (7, 0), (7, 4097), (8, 0), (8, 4100)):
        assert raw(*(a[:i] + [bad] + a[i + 1:])) == ARG, (i, bad)
    assert (y == 7.0).all()                                      # nothing was written
    assert raw(*a) == 0 and not (y == 7.0).any()


# ---- lh_session_resample_in on hand-made rings --------------------------------------------------------------------------------
R, R_IN, S = 1024, 1024, 2
PACKETS = (1, 2, 3, 40, 41, 63, 480, 961)
AT = 0xFFFFFF80                                                  # both counters start here: the ring's end and 2^32 are crossed


class Rings:
    """Slot 1 of 2: the raw ring with a zeroed history below counter AT, the 16 kHz FIFO full of a marker."""

    def __init__(self, lib, rate, fmt):
        self.lib, self.fmt = lib, fmt
        self.bank, self.width, self.o, self.n = resample_bank(rate, 16000)
        self.K = 2 * self.width + self.o
        self.raw = torch.zeros(S, 2, R_IN)
        self.raw[0] = 3.0
        self.raw_words = torch.tensor([[5, i32(AT)], [9, 0]], dtype=torch.int32)
        self.fifo = torch.full((S, 2, R), -5.0)
        self.wr = torch.tensor([77, i32(AT)], dtype=torch.int32)
        self.raw_wr, self.tap, self.wr16 = AT, (AT - self.width) & M32, AT      # the host's mirrors
        self.made = 0                                            # 16 kHz samples made so far

    def push(self, x):
        """x [2, n] float32 (or int16) -> the number of new 16 kHz samples; feed, then resample_in, as `push` does."""
        n = x.shape[1]
        st = x.contiguous().view(-1)
        items = torch.tensor([[1, 0, n, i32(self.raw_wr), 0]], dtype=torch.int32)
        assert self.lib.raw("lh_session_feed")(V(st), st.numel() * st.element_size(), self.fmt, V(items), 1, V(self.raw),
                                               V(self.raw_words[0]), V(self.raw_words[1]), R_IN, S, None) == 0
        self.raw_wr = (self.raw_wr + n) & M32
        fill = (self.raw_wr - self.tap) & M32
        nb = 0 if fill < self.K else (fill - self.K) // self.o + 1
        if nb:
            rit = torch.tensor([[1, nb, i32(self.wr16), i32(self.tap)]], dtype=torch.int32)
            assert self.lib.raw("lh_session_resample_in")(*self.args(rit)) == 0
            self.wr16, self.tap = (self.wr16 + nb * self.n) & M32, (self.tap + nb * self.o) & M32
        return nb * self.n

    def args(self, rit, n_items=None):
        return [V(self.raw), R_IN, V(rit), rit.shape[0] if n_items is None else n_items, V(self.fifo), V(self.wr), R, S,
                V(self.bank), self.o, self.n, self.width, None]


def stream_of(n, seed):
    torch.manual_seed(seed)
    pcm = torch.randint(-20000, 20000, (2, n), dtype=torch.int64).to(torch.int16)
    return pcm, pcm.float() / 32768


@pytest.mark.parametrize("rate", [48000, 24000])
def test_resample_in_any_packets_equal_the_whole_stream(emu_lib, rate):
    sizes = PACKETS + PACKETS[::-1]
    pcm, x = stream_of(sum(sizes), 3)
    whole = resampler(emu_lib, rate, 16000)(x)                   # lh_resample of the whole stream
    a, b = Rings(emu_lib, rate, F32), Rings(emu_lib, rate, S16)
    pos = 0
    for n in sizes:
        got = a.push(x[:, pos:pos + n])
        assert b.push(pcm[:, pos:pos + n]) == got
        pos += n
        # a block exists exactly when all K of its samples have been pushed
        assert a.made + got == (0 if pos + a.width < a.K else (pos + a.width - a.K) // a.o + 1) * a.n
        idx = (AT + a.made + torch.arange(got)) & (R - 1)
        assert torch.equal(a.fifo[1][:, idx], whole[:, a.made:a.made + got]), (n, pos)
        a.made += got
        assert a.wr.tolist() == [77, i32(a.wr16)] and a.wr16 == (AT + a.made) & M32
        assert torch.equal(a.fifo, b.fifo) and torch.equal(a.wr, b.wr)               # s16 carries the bits of the fp32 path
        assert (a.fifo[0] == -5.0).all() and (a.raw[0] == 3.0).all()                 # slot 0 is nobody's
    assert a.made > R and pos > 3 * R_IN and a.raw_wr < AT and a.wr16 < AT      # the ring's end and the counter's wrap were crossed
    assert a.raw_words.tolist() == [[5, i32(a.raw_wr)], [9, 0]]


def test_resample_in_skips_bad_items_and_validates(emu_lib):
    r = Rings(emu_lib, 48000, F32)
    _, x = stream_of(600, 4)
    assert r.push(x[:, :100]) == 27
    raw = emu_lib.raw("lh_session_resample_in")
    before, wr0 = r.fifo.clone(), r.wr.clone()
    good = [0, 2, 40, 0]
    for bad in ([-1, 2, 0, 0], [S, 2, 0, 0], [1, -1, 0, 0], [1, R + 1, 0, 0], [1, R_IN, 0, 0]):
        rit = torch.tensor([bad], dtype=torch.int32)
        assert raw(*r.args(rit)) == 0 and torch.equal(r.fifo, before) and torch.equal(r.wr, wr0), bad
    rit = torch.tensor([[1, R + 1, 0, 0], good], dtype=torch.int32)              # a good neighbour is served
    assert raw(*r.args(rit)) == 0 and r.wr.tolist() == [42, wr0[1].item()] and torch.equal(r.fifo[1], before[1])
    assert not torch.equal(r.fifo[0, :, 40:42], before[0, :, 40:42])
    before, wr0 = r.fifo.clone(), r.wr.clone()
    rit = torch.tensor([good], dtype=torch.int32)
    a = r.args(rit)
    for i in (0, 2, 4, 5, 8):                                    # every pointer
        assert raw(*(a[:i] + [None] + a[i + 1:])) == ARG, i
    assert raw(*([ctypes.c_void_p(r.raw.data_ptr() + 4)] + a[1:])) == ARG
    for i, vals in ((1, (0, 128, 768, 1 << 25)), (6, (0, 128, 768, 1 << 25)), (3, (0, -1, 65536)), (7, (0, -1)), (9, (0, 4097)),
                    (10, (0, 4097)), (11, (0, 4100, 600))):      # width 600: K = 1203 > R_in, too few samples for one block
        for bad in vals:
            assert raw(*(a[:i] + [bad] + a[i + 1:])) == ARG, (i, bad)
    assert torch.equal(r.fifo, before) and torch.equal(r.wr, wr0)


# ---- lh_session_resample_out --------------------------------------------------------------------------------------------------
def out_args(out, tail, hold, out_client, fmt, bank, o, n, width):
    return [V(out), V(tail), V(hold), V(out_client), fmt, out.shape[0], V(bank), o, n, width, None]


@pytest.mark.parametrize("rate", [48000, 24000, 8000])
def test_resample_out_is_the_delayed_whole_stream(emu_lib, rate):
    """Three slots, five steps: slot 0 always present, slot 1 held at step 2, slot 2 held at steps 0 and 4."""
    lib = emu_lib
    bank, width, o, n = resample_bank(16000, rate)
    D = -(-(width + o) // o)
    T, hop_c, steps = width + D * o, HOP // o * n, 5
    assert hop_c == HOP * rate // 16000
    torch.manual_seed(rate)
    rows = torch.randn(steps, 3, 2, HOP) * 0.4
    held = [(0, 0, 1), (0, 0, 0), (0, 1, 0), (0, 0, 0), (0, 0, 1)]
    tail, tail16 = torch.zeros(3, 2, T), torch.zeros(3, 2, T)
    y32, y16 = torch.full((3, 2, hop_c), 9.0), torch.full((3, 2, hop_c), 9, dtype=torch.int16)
    raw = lib.raw("lh_session_resample_out")
    got = [[] for _ in range(3)]
    for t in range(steps):
        hold = torch.tensor(held[t], dtype=torch.int32)
        before = tail.clone()
        assert raw(*out_args(rows[t], tail, hold, y32, F32, bank, o, n, width)) == 0
        assert raw(*out_args(rows[t], tail16, hold, y16, S16, bank, o, n, width)) == 0
        assert torch.equal(tail, tail16)
        want16 = torch.nan_to_num(torch.clamp(torch.round(y32 * 32768), -32768, 32767), nan=0.0).to(torch.int16)
        assert torch.equal(y16, want16)                           # the rounding of lh_session_emit_s16, on the fp32 bits
        for s in range(3):
            if held[t][s]:
                assert not y32[s].any() and torch.equal(tail[s], before[s]), (t, s)      # a zero row, the tail stays
            else:
                got[s].append(y32[s].clone())
                assert torch.equal(tail[s], torch.cat([before[s], rows[t, s]], -1)[:, -T:])
    up = resampler(lib, 16000, rate)
    for s in range(3):
        x = torch.cat([rows[t, s] for t in range(steps) if not held[t][s]], -1)
        whole = up(torch.cat([torch.zeros(2, D * o), x], -1))     # lh_resample of D o zeros, then the rows
        mine = torch.cat(got[s], -1)
        assert torch.equal(mine, whole[:, :mine.shape[-1]]) and mine.abs().max() > 0.1, s


def test_resample_out_validates_arguments(emu_lib):
    raw = emu_lib.raw("lh_session_resample_out")
    bank, width, o, n = resample_bank(16000, 48000)
    out, tail, hold = torch.randn(2, 2, HOP), torch.zeros(2, 2, width + 8), torch.zeros(2, dtype=torch.int32)
    y = torch.full((2, 2, 3 * HOP), 9.0)
    a = out_args(out, tail, hold, y, F32, bank, o, n, width)
    for i in (0, 1, 2, 3, 6):
        assert raw(*(a[:i] + [None] + a[i + 1:])) == ARG, i
    assert raw(*(a[:3] + [a[0]] + a[4:])) == ARG                 # out_client == out
    for i, vals in ((4, (2, -1)), (5, (0, -1)), (7, (0, 3, 5, 256)), (8, (0, 4097)), (9, (0, 900))):
        for bad in vals:
            assert raw(*(a[:i] + [bad] + a[i + 1:])) == ARG, (i, bad)
    assert (y == 9.0).all() and not tail.any()
    assert raw(*a) == 0 and not (y == 9.0).any()


# ---- the host over the emulated device ----------------------------------------------------------------------------------------
N_CHUNKS, RATE = 3, 48000


@pytest.fixture(scope="module")
def emu_net(oracle_cfg_sd, emu_lib):
    cfg, sd = oracle_cfg_sd
    net = EmuSessionNet(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net.emu_lib = emu_lib
    return net


def test_client_rate_streamer_end_to_end(emu_net, emu_lib):
    """S = 2 at 48 kHz, the same stream for both slots: slot 0 in 480-sample packets, one a tick, slot 1 in one packet.  A
    listener's rows equal: the stream resampled offline, through a 16 kHz packet streamer, resampled offline with the zero
    prefix."""
    mk = emu_net.make_session_streamer
    ss = mk(2, "cpu", use_graph=False, pace=True, packets=True, client_rate=RATE)
    ref = mk(2, "cpu", use_graph=False, pace=True, packets=True)
    assert ss.client_rate == RATE and ss.hop_client == 384 and ss.fifo_samples == 2048 and ss.raw_samples == 8192
    assert (ss.lookahead_in, ss.delay_out) == (21, 8) and ref.hop_client == HOP and not hasattr(ref, "_raw")
    n16 = HOP * N_CHUNKS + NFFT - HOP
    n48 = 3 * n16 + ss.lookahead_in - 2                          # the last block's taps end with the stream
    emb = synth.batch([30], n16)["embedding_gt"][0, 0]
    torch.manual_seed(30)
    x48 = torch.randn(2, n48) * 0.1
    x16 = resampler(emu_lib, RATE, 16000)(x48)[:, :n16]
    for s in (0, 1):
        ss.open(s, emb), ref.open(s, emb)
    ref.push({0: x16, 1: x16})
    ss.push({1: x48})
    assert ss.buffered(1) == n16 and ss.buffered(0) == 0 and ss.ready() == [1]
    mine, theirs, pos = [[], []], [], 0
    while pos < n48 or ss.ready():
        if pos < n48:
            ss.push({0: x48[:, pos:pos + 480]})
            pos += 480
            assert ss.buffered(0) + HOP * len(mine[0]) == (0 if pos + 19 < 41 else (min(pos, n48) + 19 - 41) // 3 + 1)
        y = ss.step().clone()
        assert tuple(y.shape) == (2, 2, 384)
        for s in (0, 1):
            if ss.last_present[s]:
                mine[s].append(y[s])
            else:
                assert not y[s].any()
        if len(theirs) < N_CHUNKS:
            theirs.append(ref.step().clone()[0])
    assert len(mine[0]) == len(mine[1]) == N_CHUNKS and ss.faults() == []
    a, b = torch.cat(mine[0], -1), torch.cat(mine[1], -1)
    rows16 = torch.cat(theirs, -1)
    want = resampler(emu_lib, 16000, RATE)(torch.cat([torch.zeros(2, ss.delay_out), rows16], -1))[:, :a.shape[-1]]
    assert torch.equal(a, b) and torch.equal(a, want) and a.abs().max() > 1e-4
    assert torch.equal(ss._fifo[:, :, :n16], ref._fifo[:, :, :n16])                 # the 16 kHz FIFO is the offline stream
    # BufferError in 16 kHz samples, before anything changes; flush restarts the slot from silence
    wr0 = list(ss._wr)
    with pytest.raises(BufferError):
        ss.push({0: torch.zeros(2, 3 * 2048)})
    assert ss._wr == wr0
    ss.flush(0)
    ss.push({0: x48[:, :100]})
    assert ss.buffered(0) == 27 and torch.equal(ss._fifo[0, :, :27], x16[:, :27]) and not ss._tail[0].any()
    assert ss._tail[1].any() and ss._fifo_words.tolist()[0][0] == 27
    ss.reset()
    assert not ss._raw.any() and not ss._tail.any() and ss._raw_wr == [0, 0] and ss.buffered(0) == 0


def test_client_rate_streamer_refuses_what_it_cannot_serve(emu_net):
    mk = emu_net.make_session_streamer
    with pytest.raises(ValueError, match="125"):
        mk(2, "cpu", use_graph=False, pace=True, packets=True, client_rate=44100)
    with pytest.raises(ValueError, match="packets"):
        mk(2, "cpu", use_graph=False, pace=True, client_rate=48000)
    for bad in (0, 500, 16001, 1 << 20):
        with pytest.raises(ValueError):
            mk(2, "cpu", use_graph=False, pace=True, packets=True, client_rate=bad)
    p16 = mk(2, "cpu", use_graph=False, pace=True, packets=True, pcm16=True, client_rate=8000, fifo_samples=256)
    assert p16.hop_client == 64 and p16.out_client.dtype == torch.int16 and p16.raw_samples == 256
    with pytest.raises(ValueError):
        p16.push({0: torch.zeros(2, 8)})
