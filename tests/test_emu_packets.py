"""CPU: packets (ABI 22) — `lh_session_feed`, `lh_session_frame`, `lh_session_emit_s16` (lh_stream.hip) and
`SessionStreamer(pace=True, packets=True)` (sessions.py) over the emulated library, eager.  The feature moves bytes and derives
presence from two counters, so every claim is `torch.equal`: FIFO contents as 32-bit patterns (NaN and inf among them), the
counters across the ring's end and across 2^32, and a listener's output rows against `step(windows, present)` of a second paced
streamer.  Small on purpose: the emulator runs a chunk row in ~0.5 s."""
import ctypes

import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from tests.hipemu.hosts import EmuNet
from oracle import tfgridnet_oracle as O

HOP, NFFT = 128, 192
ARG = 1
F32, S16, FLUSH = 0, 1, 1
M32 = 0xffffffff
V = lambda v: ctypes.c_void_p(v.data_ptr())
i32 = lambda v: v - (1 << 32) if v >> 31 else v          # a 32-bit pattern as torch.int32 holds it


class EmuSessionNet(EmuNet):
    def _host_words(self, n, device):               # the pinned words of the GPU host: plain host memory here
        return torch.zeros(n, dtype=torch.int32)

    def _enroll_side(self, dev):                    # no embedder runs here
        return None


@pytest.fixture(scope="module")
def emu_net(oracle_cfg_sd):
    from tests.hipemu.build_emu import build_emu
    cfg, sd = oracle_cfg_sd
    net = EmuSessionNet(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net.emu_lib = _cabi.Lib(build_emu())
    return net


def patterns(*shape):
    """Random 32-bit patterns, NaN and inf patterns among them: the FIFO carries bytes, not numbers."""
    t = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int64).to(torch.int32)
    flat = t.view(-1)
    special = torch.tensor([0x7fc00000, 0x7f800000, -0x800000, 0x7f800001, -1, 0x7fffffff], dtype=torch.int64).to(torch.int32)
    idx = torch.randperm(flat.numel())[:max(6, flat.numel() // 50)]
    flat[idx] = special[torch.arange(idx.numel()) % special.numel()]
    return t


# ---- lh_session_feed on hand-made buffers ------------------------------------------------------------------------------------
R, S = 256, 3
SIZES = (0, 1, 63, 64, 65, 255, 256)
ATS = (0, 200, 0xFFFFFF80)              # plain, the ring wraps, the counter wraps


class Fifo:
    def __init__(self, lib, seed):
        torch.manual_seed(seed)
        self.lib = lib
        self.fifo = patterns(S, 2, R)
        self.words = torch.tensor([[7, 0x80, 300], [0, 0x80, 128]], dtype=torch.int32)      # wr | rd, whatever lay there

    def args(self, staging, fmt, items, n_items=None, nbytes=None):
        nbytes = staging.numel() * staging.element_size() if nbytes is None else nbytes
        return [V(staging), nbytes, fmt, V(items), items.shape[0] if n_items is None else n_items, V(self.fifo), V(self.words[0]),
                V(self.words[1]), R, S, None]

    def feed(self, staging, fmt, items):
        """items: rows (slot, offset, n, at, flags)"""
        table = torch.tensor([[a, b, c, i32(d), e] for a, b, c, d, e in items], dtype=torch.int32)
        assert self.lib.raw("lh_session_feed")(*self.args(staging, fmt, table)) == 0


def served(fifo, words, staging32, items):
    """What the feed of `items` (all of them legal) leaves, from `staging32`: the samples as the 32-bit patterns they become."""
    fifo, words = fifo.clone(), words.clone()
    for slot, off, n, at, flags in items:
        if flags & FLUSH:
            at = 0
            words[1, slot] = 0
        for ch in range(2):
            for i in range(n):
                fifo[slot, ch, (at + i) & (R - 1)] = staging32[off + ch * n + i]
        words[0, slot] = i32((at + n) & M32)
    return fifo, words


def s16_staging(n):
    x = torch.randint(-32768, 32768, (n,), dtype=torch.int64).to(torch.int16)
    x[:5] = torch.tensor([-32768, -1, 0, 1, 32767], dtype=torch.int16)
    return x[torch.randperm(n)] if n > 5 else x


def as_bits(staging, fmt):
    if fmt == F32:
        return staging
    want = staging.to(torch.float64) / 32768.0                   # exact in fp32: 16 significant bits times a power of two
    assert torch.equal(want.float().double(), want)
    return want.float().view(torch.int32)


@pytest.mark.parametrize("fmt", [F32, S16], ids=["fp32", "s16"])
def test_feed_scatters_packets_into_the_rings(emu_net, fmt):
    """Every size at every position, three packets (one per slot) a launch: the written samples, and nothing else, change."""
    cases = [(at, n) for at in ATS for n in SIZES]
    f = Fifo(emu_net.emu_lib, 5)
    for k in range(0, len(cases), 2):
        batch = cases[k:k + 2]
        # slot 1 is nobody's in this launch; the two packets lie back to back behind 3 unused elements
        slots, items, off = (0, 2) if (k // 2) % 2 == 0 else (2, 0), [], 3
        for slot, (at, n) in zip(slots, batch):
            items.append((slot, off, n, at, 0))
            off += 2 * n
        staging = patterns(off + 5) if fmt == F32 else s16_staging(off + 5)
        want_fifo, want_words = served(f.fifo, f.words, as_bits(staging, fmt), items)
        before = f.fifo.clone()
        f.feed(staging, fmt, items)
        assert torch.equal(f.fifo, want_fifo) and torch.equal(f.words, want_words), (batch, f.words.tolist())
        assert torch.equal(f.fifo[1], before[1])
        for slot, _, n, at, _ in items:                          # exactly n ring cells of each channel may differ
            assert int((f.fifo[slot] != before[slot]).sum()) <= 2 * n
            assert f.words[0, slot].item() == i32((at + n) & M32)
    assert f.words[1].tolist() == [0, 0x80, 128]                 # rd is not feed's without FLUSH
    if fmt == S16:                                               # the five corner values, by value
        st = torch.tensor([-32768, -1, 0, 1, 32767] * 2, dtype=torch.int16)
        f.feed(st, S16, [(1, 0, 5, 0, 0)])
        assert f.fifo[1, 0, :5].view(torch.float32).tolist() == [-1.0, -1 / 32768, 0.0, 1 / 32768, 32767 / 32768]
    else:                                                        # NaN and inf patterns arrive as they were sent
        st = torch.tensor([0x7fc00001, 0x7f800000, i32(0xff800000), i32(0xffc12345)] * 2, dtype=torch.int64).to(torch.int32)
        f.feed(st, F32, [(1, 0, 4, 254, 0)])
        assert f.fifo[1, 1, [254, 255, 0, 1]].tolist() == st[:4].tolist()


def test_feed_flush_restarts_the_slot(emu_net):
    f = Fifo(emu_net.emu_lib, 6)
    staging = patterns(2 * 70)
    before = f.fifo.clone()
    f.feed(staging, F32, [(1, 0, 70, 0x12345, FLUSH), (2, 0, 0, 999, FLUSH)])       # `at` is taken as 0; n = 0 is legal
    assert f.words.tolist() == [[7, 70, 0], [0, 0, 0]]
    assert torch.equal(f.fifo[1, :, :70], staging.view(2, 70)) and torch.equal(f.fifo[1, :, 70:], before[1, :, 70:])
    assert torch.equal(f.fifo[0], before[0]) and torch.equal(f.fifo[2], before[2])


def test_feed_skips_a_bad_item_whole(emu_net):
    """Between two good neighbours: slot -1, slot S, n = -1, n = R + 1, samples that reach past the staging buffer."""
    n_st = 2 * (R + 1) + 40
    for bad in ((-1, 0, 8, 0, 0), (S, 0, 8, 0, 0), (1, 0, -1, 0, 0), (1, 0, R + 1, 0, 0), (1, n_st - 15, 8, 0, 0),
                (1, -4, 8, 0, 0), (1, 0x7fffffff, 8, 0, 0)):
        f = Fifo(emu_net.emu_lib, 7)
        staging = patterns(n_st)
        good = [(0, 2, 9, 250, 0), (2, 20, 10, 0xFFFFFFFB, 0)]
        want_fifo, want_words = served(f.fifo, f.words, staging, good)
        f.feed(staging, F32, [good[0], bad, good[1]])
        assert torch.equal(f.fifo, want_fifo) and torch.equal(f.words, want_words), bad
    # the last samples of the staging buffer are reachable
    f = Fifo(emu_net.emu_lib, 8)
    staging = patterns(64)
    f.feed(staging, F32, [(1, 64 - 16, 8, 0, 0)])
    assert torch.equal(f.fifo[1, :, :8], staging[48:].view(2, 8)) and f.words[0, 1].item() == 8


def test_feed_validates_arguments(emu_net):
    f = Fifo(emu_net.emu_lib, 9)
    raw = f.lib.raw("lh_session_feed")
    staging = patterns(64)
    items = torch.tensor([[0, 0, 4, 0, 0]], dtype=torch.int32)
    a = f.args(staging, F32, items)
    assert raw(*a) == 0
    for i in (0, 3, 5, 6, 7):                                    # every pointer
        assert raw(*(a[:i] + [None] + a[i + 1:])) == ARG, i
    for r in (192, 384, 128, 0, -256):                           # too small, not a power of two
        assert raw(*(a[:8] + [r] + a[9:])) == ARG, r
    for s in (0, -1):
        assert raw(*(a[:9] + [s] + a[10:])) == ARG
    for n in (0, -1):
        assert raw(*(a[:4] + [n] + a[5:])) == ARG
    assert raw(*(a[:2] + [2] + a[3:])) == ARG                    # an unknown sample format
    assert raw(*(a[:6] + [a[7]] + a[7:])) == ARG                 # wr == rd
    odd = ctypes.c_void_p(f.fifo.data_ptr() + 4)
    assert raw(*(a[:5] + [odd] + a[6:])) == ARG                  # the rings move 16 bytes at a time


# ---- lh_session_frame ----------------------------------------------------------------------------------------------------------
def frame(lib, fifo, words, chunk_in, hold, r=R, s=None):
    return lib.raw("lh_session_frame")(V(fifo), V(words[0]), V(words[1]), V(chunk_in), V(hold), r, fifo.shape[0] if s is None else s,
                                       None)


def window(fifo, slot, rd, r=R):
    idx = (rd + torch.arange(NFFT)) & (r - 1)
    return fifo[slot][:, idx]


def test_frame_cuts_windows_and_decides_presence(emu_net):
    """Six slots, one launch: 191 samples hold, 192 frame, 64 (the state right after a frame) hold, a window across the ring's
    end, a window across the counter's wrap, a slot nobody fed."""
    lib = emu_net.emu_lib
    torch.manual_seed(12)
    n = 6
    fifo, chunk_in = patterns(n, 2, R), patterns(n, 2, NFFT)
    hold = torch.full((n,), 7, dtype=torch.int32)
    rd = [0, 256, 128, 128, 0xFFFFFF80, 0]
    wr = [191, 256 + 192, 128 + 64, 128 + 192, 0x40, 0]
    words = torch.tensor([[i32(v) for v in wr], [i32(v) for v in rd]], dtype=torch.int32)
    rows0 = chunk_in.clone()
    assert frame(lib, fifo, words, chunk_in, hold) == 0
    assert hold.tolist() == [1, 0, 1, 0, 0, 1]
    assert words[0].tolist() == [i32(v) for v in wr]             # wr is never frame's
    assert words[1].tolist() == [0, 384, 128, 256, 0, 0]         # += 128, and 0xFFFFFF80 + 128 = 2^32 = 0
    for s in (0, 2, 5):
        assert torch.equal(chunk_in[s], rows0[s]), s             # a held row is not touched
    for s in (1, 3, 4):
        assert torch.equal(chunk_in[s], window(fifo, s, rd[s])), s
    assert torch.equal(chunk_in[3, :, 128:], fifo[3, :, :64])    # rd & 255 = 128: the look-ahead comes from the ring's start
    assert torch.equal(chunk_in[4, :, :128], fifo[4, :, 128:]) and torch.equal(chunk_in[4, :, 128:], fifo[4, :, :64])
    # the next chunk: slot 1 has 64 left and holds, the unfed slot holds for ever
    rows1 = chunk_in.clone()
    assert frame(lib, fifo, words, chunk_in, hold) == 0
    assert hold.tolist() == [1] * n and torch.equal(chunk_in, rows1) and words[1].tolist() == [0, 384, 128, 256, 0, 0]
    # a larger ring, fed by lh_session_feed: 320 samples are two windows, the second one overlaps the first by 64
    R2 = 1024
    fifo2, words2 = torch.zeros(1, 2, R2, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32)
    st = patterns(2 * 320)
    at = 0xFFFFFF00
    words2[1, 0] = i32(at)
    items = torch.tensor([[0, 0, 320, i32(at), 0]], dtype=torch.int32)
    assert lib.raw("lh_session_feed")(V(st), st.numel() * 4, F32, V(items), 1, V(fifo2), V(words2[0]), V(words2[1]), R2, 1, None) == 0
    row, h = torch.zeros(1, 2, NFFT, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    got = []
    for _ in range(3):
        assert frame(lib, fifo2, words2, row, h, R2) == 0
        got.append((h.item(), row.clone()))
    assert [g[0] for g in got] == [0, 0, 1] and words2.tolist() == [[i32((at + 320) & M32)], [0]]
    assert torch.equal(got[0][1][0], st.view(2, 320)[:, :192]) and torch.equal(got[1][1][0], st.view(2, 320)[:, 128:320])


def test_frame_validates_arguments(emu_net):
    lib = emu_net.emu_lib
    fifo, chunk_in = patterns(S, 2, R), patterns(S, 2, NFFT)
    words, hold = torch.zeros(2, S, dtype=torch.int32), torch.zeros(S, dtype=torch.int32)
    raw = lib.raw("lh_session_frame")
    a = [V(fifo), V(words[0]), V(words[1]), V(chunk_in), V(hold), R, S, None]
    assert raw(*a) == 0
    for i in range(5):
        assert raw(*(a[:i] + [None] + a[i + 1:])) == ARG, i
    for r in (192, 384, 0):
        assert raw(*(a[:5] + [r] + a[6:])) == ARG
    assert raw(*(a[:6] + [0, None])) == ARG and raw(*(a[:1] + [a[2]] + a[2:])) == ARG


# ---- lh_session_emit_s16 -------------------------------------------------------------------------------------------------------
def test_emit_rounds_half_even_and_saturates(emu_net):
    lib = emu_net.emu_lib
    torch.manual_seed(13)
    inf, nan = float("inf"), float("nan")
    corner = [1.0, -1.0, 1 - 2.0 ** -16, -(1 - 2.0 ** -16), 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768,
              7.0, -7.0, inf, -inf, nan, 32767.5 / 32768, -32768.5 / 32768, 0.0, -0.0]
    x = torch.randn(3, 2, HOP) * 0.6
    x.view(-1)[:len(corner)] = torch.tensor(corner)
    x.view(-1)[300:300 + len(corner)] = torch.tensor(corner)
    out = torch.full((3, 2, HOP), 1234, dtype=torch.int16)
    assert lib.raw("lh_session_emit_s16")(V(x), V(out), 3, None) == 0
    want = torch.nan_to_num(torch.clamp(torch.round(x * 32768), -32768, 32767), nan=0.0).to(torch.int16)
    assert torch.equal(out, want)
    assert out.view(-1)[:14].tolist() == [32767, -32768, 32767, -32768, 0, 2, 2, 0, -2, 32767, -32768, 32767, -32768, 0]
    raw = lib.raw("lh_session_emit_s16")
    assert raw(None, V(out), 3, None) == ARG and raw(V(x), None, 3, None) == ARG and raw(V(x), V(out), 0, None) == ARG
    assert raw(V(x), V(x), 3, None) == ARG


# ---- the host over the emulated device ------------------------------------------------------------------------------------
N_CHUNKS = 6
N_STREAM = HOP * N_CHUNKS + NFFT - HOP


@pytest.fixture(scope="module")
def clip():
    d = synth.batch([30], N_STREAM)
    return d["mixture"][0], d["embedding_gt"][0, 0]


def words_of(ss):
    return [[v & M32 for v in row] for row in ss._fifo_words.tolist()]


def test_packet_streamer_end_to_end(emu_net, clip):
    """S = 2, the same 6-chunk stream for both slots: slot 0 gets it in 160-sample packets, one a tick; slot 1 in one packet.
    Every step's output equals that of a second paced streamer stepped with explicit windows and the same presence."""
    mix, emb = clip
    ss = emu_net.make_session_streamer(2, "cpu", use_graph=False, pace=True, packets=True)
    ref = emu_net.make_session_streamer(2, "cpu", use_graph=False, pace=True)
    assert ss.packets and not ref.packets and ss.fifo_samples == 2048 and ss.last_present == (False, False)
    for s in (0, 1):
        ss.open(s, emb), ref.open(s, emb)
    # hand arithmetic: 160 a tick against 128 a chunk and 192 to start
    present = [(False, True)] + [(True, True)] * 5 + [(True, False)]
    left = [(160, 704), (192, 576), (224, 448), (256, 320), (288, 192), (192, 64), (64, 64)]
    ready = [[1], [0, 1], [0, 1], [0, 1], [0, 1], [0, 1], [0]]
    took, mine = [0, 0], [[], []]
    for t in range(7):
        pk = {0: mix[:, 160 * t:160 * (t + 1)]} if 160 * t < N_STREAM else {}
        if t == 0:
            pk[1] = mix
        ss.push(pk)
        assert ss.ready() == ready[t], t
        y = ss.step().clone()
        assert ss.last_present == present[t] and (ss.buffered(0), ss.buffered(1)) == left[t], t
        x = torch.full((2, 2, NFFT), float("nan"))
        for s in (0, 1):
            if present[t][s]:
                x[s] = mix[:, took[s] * HOP:took[s] * HOP + NFFT]
                took[s] += 1
                mine[s].append(y[s])
        assert torch.equal(y, ref.step(x, present[t])), t
        assert ss._hold.tolist() == [int(not p) for p in present[t]]
    assert took == [N_CHUNKS, N_CHUNKS] and ss.faults() == [] and ss.active == [0, 1]
    a, b = torch.cat(mine[0], -1), torch.cat(mine[1], -1)
    assert torch.equal(a, b) and a.abs().max() > 1e-3            # any packetisation, the same listener
    assert words_of(ss) == [[N_STREAM, N_STREAM], [HOP * N_CHUNKS, HOP * N_CHUNKS]]
    assert ss._wr == [N_STREAM] * 2 and ss._rd == [HOP * N_CHUNKS] * 2

    # BufferError at fifo_samples + 1: nothing of the call happens, for either slot
    fifo0 = ss._fifo.clone()
    with pytest.raises(BufferError):
        ss.push({0: torch.ones(2, 10), 1: torch.ones(2, 2048 - 64 + 1)})
    assert words_of(ss) == [[N_STREAM] * 2, [HOP * N_CHUNKS] * 2] and ss._wr == [N_STREAM] * 2 and ss._rd == [HOP * N_CHUNKS] * 2
    assert torch.equal(ss._fifo, fifo0) and (ss.buffered(0), ss.buffered(1)) == (64, 64)
    ss.push({1: torch.ones(2, 2048 - 64)})                       # exactly full is fine
    assert ss.buffered(1) == 2048 and words_of(ss)[0] == [N_STREAM, N_STREAM + 2048 - 64]

    # flush: with the slot's next packet ...
    ss.flush(1)
    assert ss.buffered(1) == 0 and ss.ready() == []
    ss.push({1: mix[:, :10]})
    assert words_of(ss) == [[N_STREAM, 10], [HOP * N_CHUNKS, 0]] and ss.buffered(1) == 10
    assert torch.equal(ss._fifo[1, :, :10], mix[:, :10])
    # ... or in a push of its own that `step` issues
    ss.flush(0)
    assert ss.buffered(0) == 0
    y = ss.step()
    assert ss.last_present == (False, False) and not y.any() and words_of(ss) == [[0, 10], [0, 0]]
    assert ss._hold.tolist() == [1, 1] and ss.active == [0, 1]
    # reset flushes everyone
    ss.reset()
    assert words_of(ss) == [[0, 0], [0, 0]] and ss.buffered(1) == 0 and ss._wr == [0, 0]


def test_packet_streamer_refuses_what_it_cannot_serve(emu_net):
    mk = emu_net.make_session_streamer
    with pytest.raises(ValueError, match="pace"):
        mk(2, "cpu", use_graph=False, packets=True)
    for bad in (192, 300, 128, 0):
        with pytest.raises(ValueError, match="fifo_samples"):
            mk(2, "cpu", use_graph=False, pace=True, packets=True, fifo_samples=bad)
    with pytest.raises(ValueError, match="pcm16"):
        mk(2, "cpu", use_graph=False, pace=True, pcm16=True)
    ss = mk(2, "cpu", use_graph=False, pace=True, packets=True, fifo_samples=256)
    paced = mk(2, "cpu", use_graph=False, pace=True)
    with pytest.raises(ValueError):
        ss.step(torch.zeros(2, 2, NFFT))
    with pytest.raises(ValueError):
        ss.step(present=[True, True])
    with pytest.raises(ValueError):
        paced.step()
    for call in (lambda: paced.push({}), lambda: paced.flush(0), lambda: paced.buffered(0), paced.ready):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        ss.push({0: torch.zeros(2, 8, dtype=torch.int16)})       # an fp32 streamer
    with pytest.raises(ValueError):
        ss.push({0: torch.zeros(8)})
    with pytest.raises(IndexError):
        ss.push({2: torch.zeros(2, 8)})
    with pytest.raises(BufferError):
        ss.push({0: torch.zeros(2, 257)})
    assert ss._wr == [0, 0] and ss.buffered(0) == 0
    p16 = mk(2, "cpu", use_graph=False, pace=True, packets=True, pcm16=True, fifo_samples=256)
    with pytest.raises(ValueError):
        p16.push({0: torch.zeros(2, 8)})
    pcm = torch.tensor([[-32768, -1, 0], [1, 32767, 5]], dtype=torch.int16)
    p16.push({1: pcm})
    assert torch.equal(p16._fifo[1, :, :3], pcm.float() / 32768) and p16.buffered(1) == 3 and p16.out16.dtype == torch.int16
