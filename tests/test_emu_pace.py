"""CPU: `SessionStreamer(pace=True)` (sessions.py) and its entry points (`lh_qkv_proj_ln_rows`, `lh_ring_advance_rows`,
`lh_session_{begin,end,move,capture}_paced` and the row forms; lh_pointwise.hip, lh_attn.hip, lh_stream.hip) over the emulated
library, eager.  A listener whose chunk is late is HELD for the step: nothing of theirs is judged, their output row is zeros
and every bit of their state is afterwards what it was before — a hold copies bytes, so those claims are `torch.equal` on
integers, NaN and inf patterns among them.  A session is compared with the oracle's forward over its OWN samples from the zero
state within the emulator tolerance of tests/test_emu_kernels.py.  Small on purpose: the emulator runs a chunk row in ~0.5 s."""
import ctypes
from unittest import mock

import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.net import _Span
from lookoncetohear_amd.weights import KV_PAD_ROWS, QK_PAD
from tests.hipemu.hosts import EmuNet
from oracle import tfgridnet_oracle as O

TOL = 5e-5          # tests/test_emu_kernels.py
HOP, NFFT = 128, 192
RESET, OPEN, CLOSE, SHIFT = 1, 2, 4, 8
ARM = 1
ARG = 1
NEW = ("lh_qkv_proj_ln_rows", "lh_ring_advance_rows", "lh_session_begin_paced", "lh_session_end_paced",
       "lh_session_move_paced", "lh_session_begin_rows_paced", "lh_session_end_rows_paced", "lh_session_capture_paced")
P = lambda v: v.data_ptr()
V = lambda v: ctypes.c_void_p(v.data_ptr())


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
    """Random 32-bit patterns, NaN and inf patterns among them: a hold must copy bytes, not numbers."""
    t = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int64).to(torch.int32)
    flat = t.view(-1)
    special = torch.tensor([0x7fc00000, 0x7f800000, -0x800000, 0x7f800001, -1, 0x7fffffff], dtype=torch.int64).to(torch.int32)
    idx = torch.randperm(flat.numel())[:max(6, flat.numel() // 50)]
    flat[idx] = special[torch.arange(idx.numel()) % special.numel()]
    return t


# ---- lh_qkv_proj_ln_rows / lh_ring_advance_rows -----------------------------------------------------------------------------
def test_qkv_rows_write_their_own_ring_slot(emu_net):
    """B = 3, write_pos = [0, 49, -1]: rows 0 and 1 are, bit for bit, what lh_qkv_proj_ln writes for that row alone with the
    shared position at 0 and 49; row 2's rings are untouched; so is every pad row."""
    lib = emu_net.emu_lib
    torch.manual_seed(3)
    bp = emu_net._weights(torch.device("cpu"))["blocks"][0]
    B, NH, rows = 3, 4, 50 + KV_PAD_ROWS
    y = torch.randn(B, 1, 97, 64) * 3.0
    w = [bp[k] for k in ("qkv_w", "qkv_b", "qkv_slopes", "lnq_w", "lnq_b", "lnk_w", "lnk_b", "lnv_w", "lnv_b")]
    i16 = lambda *s: patterns(*s[:-1], s[-1] // 2).view(torch.int16).view(*s)      # fp16 rings as bit patterns
    kx0, vx0 = i16(B * NH, rows, 2 * QK_PAD), i16(B * NH, rows, 2 * 1552)
    q0 = torch.zeros(B * NH, 1, 2 * QK_PAD, dtype=torch.int16)
    kx, vx, q = kx0.clone(), vx0.clone(), q0.clone()
    wp = torch.tensor([0, 49, -1], dtype=torch.int32)
    lib.call("lh_qkv_proj_ln_rows", P(y), *[P(t) for t in w], P(q), P(kx), P(vx), P(wp), B, None)
    for b, pos in ((0, 0), (1, 49)):
        sl = slice(b * NH, (b + 1) * NH)
        kr, vr, qr = kx0[sl].clone(), vx0[sl].clone(), q0[sl].clone()
        yb = y[b:b + 1].clone()
        shared = torch.tensor([pos], dtype=torch.int32)
        lib.call("lh_qkv_proj_ln", P(yb), *[P(t) for t in w], P(qr), P(kr), P(vr), P(shared), 1, 1, None)
        assert torch.equal(kx[sl], kr) and torch.equal(vx[sl], vr) and torch.equal(q[sl], qr), b
        assert not torch.equal(kr[:, pos], kx0[sl][:, pos])                         # ... and that row was written
        keep = [r for r in range(rows) if r != pos]
        assert torch.equal(kx[sl][:, keep], kx0[sl][:, keep]) and torch.equal(vx[sl][:, keep], vx0[sl][:, keep])
    assert torch.equal(kx[2 * NH:], kx0[2 * NH:]) and torch.equal(vx[2 * NH:], vx0[2 * NH:])
    assert torch.isfinite(q[2 * NH:].view(torch.float16).float()).all()             # a held row's Q row: anything finite
    assert torch.equal(kx[:, 50:], kx0[:, 50:]) and torch.equal(vx[:, 50:], vx0[:, 50:])
    raw = lib.raw("lh_qkv_proj_ln_rows")
    args = [V(y)] + [V(t) for t in w] + [V(q), V(kx), V(vx)]
    assert raw(*args, None, B, None) == ARG and raw(*args, V(wp), 0, None) == ARG
    assert raw(*args[:-1], None, V(wp), B, None) == ARG


def test_ring_advance_rows(emu_net):
    lib = emu_net.emu_lib
    pos = torch.tensor([0, 49, 7, 11], dtype=torch.int32)
    wp = torch.tensor([0, 49, -1, 3], dtype=torch.int32)
    lib.call("lh_ring_advance_rows", P(pos), P(wp), 50, 3, None)
    assert pos.tolist() == [1, 0, 7, 11]                        # the fourth row was not launched
    raw = lib.raw("lh_ring_advance_rows")
    assert raw(None, V(wp), 50, 3, None) == ARG and raw(V(pos), None, 50, 3, None) == ARG
    assert raw(V(pos), V(pos), 50, 3, None) == ARG and raw(V(pos), V(wp), 0, 3, None) == ARG
    assert raw(V(pos), V(wp), 50, 0, None) == ARG and raw(V(pos), V(wp), 50, 3, None) == 0


# ---- the paced bracket kernels on hand-made buffers -----------------------------------------------------------------------
class Paced:
    """S rows of two ping-pong sets of three state tensors (the third longer than one pass of the carry loop: 1024 threads x
    4 loads x 16 bytes), one `ring` tensor outside the sets, the words and the chunk's buffers."""
    BYTES = [112, 16000, 80000]

    def __init__(self, lib, S):
        torch.manual_seed(11)
        self.lib, self.S = lib, S
        self.sets = [[patterns(S, b // 4) for b in self.BYTES] for _ in (0, 1)]
        self.ring = patterns(S, 4000)
        for st in self.sets:                                    # what lh_session_end scans of row 0: finite
            st[0][0] = torch.arange(28, dtype=torch.int32)
        sp = lambda t: _Span(t.data_ptr(), t.shape[1] * 4)
        every = self.sets[0] + self.sets[1] + [self.ring]
        self.spans = (_Span * len(every))(*[sp(t) for t in every])
        self.scan = [(_Span * 1)(sp(self.sets[k ^ 1][0])) for k in (0, 1)]
        self.carry = [(_Span * 6)(*[sp(t) for pair in zip(self.sets[k], self.sets[k ^ 1]) for t in pair]) for k in (0, 1)]
        self.words = torch.zeros(3, S, dtype=torch.int32)       # cmd host | cmd device | active
        self.hold = torch.zeros(S, dtype=torch.int32)
        self.ringpos = torch.zeros(2, S, dtype=torch.int32)     # pos | write_pos
        self.fault = torch.zeros(S, dtype=torch.int32)
        self.x, self.gated = torch.randn(S, 2, NFFT), torch.full((S, 2, NFFT), 9.0)
        self.out = torch.randn(S, 2, HOP)

    def begin_args(self, spans=None, n_spans=None):
        return (ctypes.c_void_p(ctypes.addressof(self.spans if spans is None else spans)),
                len(self.spans) if n_spans is None else n_spans, V(self.x), V(self.gated), V(self.words), V(self.words[2]),
                V(self.hold), V(self.ringpos[0]), V(self.ringpos[1]), self.S, None)

    def end_args(self, k):
        return (ctypes.c_void_p(ctypes.addressof(self.scan[k])), 1, ctypes.c_void_p(ctypes.addressof(self.carry[k])), 3,
                V(self.x), V(self.out), V(self.words), V(self.words[2]), V(self.fault), V(self.hold), self.S, None)

    def begin(self):
        assert self.lib.raw("lh_session_begin_paced")(*self.begin_args()) == 0

    def end(self, k):
        assert self.lib.raw("lh_session_end_paced")(*self.end_args(k)) == 0

    def state(self):
        return [[t.clone() for t in st] for st in self.sets], self.ring.clone()


@pytest.mark.parametrize("k", [0, 1], ids=["even_chunk", "odd_chunk"])
def test_held_row_is_carried_byte_for_byte(emu_net, k):
    """Rows 0 and 1 active (generations 5, 6), row 2 idle; row 1 is held and its input row is NaN.  begin -> end with no
    separator launch in between: what the chunk `wrote` (set k ^ 1) is whatever lay there."""
    S = 3
    p = Paced(emu_net.emu_lib, S)
    p.words[2] = torch.tensor([5, 6, 0], dtype=torch.int32)
    p.hold[1] = 1
    p.ringpos[0] = torch.tensor([3, 7, 9], dtype=torch.int32)
    p.x[1] = float("nan")
    p.x[2] = float("nan")                                       # idle: ignored as ever
    sets0, ring0 = p.state()
    out0 = p.out.clone()
    p.begin()
    assert torch.equal(p.gated[0], p.x[0]) and not p.gated[1].any() and not p.gated[2].any()
    assert p.ringpos.tolist() == [[3, 7, 9], [3, -1, -1]]
    now, ring = p.state()
    assert all(torch.equal(a, b) for s in (0, 1) for a, b in zip(now[s], sets0[s])) and torch.equal(ring, ring0)
    p.end(k)
    now, ring = p.state()
    for i in range(3):                                          # every pair: set k over set k ^ 1, row 1 only
        assert torch.equal(now[k][i], sets0[k][i]), i
        assert torch.equal(now[k ^ 1][i][1], sets0[k][i][1]), i
        assert torch.equal(now[k ^ 1][i][0], sets0[k ^ 1][i][0]) and torch.equal(now[k ^ 1][i][2], sets0[k ^ 1][i][2]), i
        assert not torch.equal(sets0[k][i][1], sets0[k ^ 1][i][1])
    assert torch.equal(ring, ring0)
    assert torch.equal(p.out[0], out0[0]) and not p.out[1].any() and not p.out[2].any()
    assert p.words.tolist() == [[0, 0, 0], [0, 0, 0], [5, 6, 0]] and p.fault.tolist() == [0, 0, 0]
    assert p.ringpos[0].tolist() == [3, 7, 9]                   # lh_ring_advance_rows is the only writer
    # the same row present: its NaN input is a fault again
    p.hold[1] = 0
    p.begin()
    p.end(k ^ 1)
    assert p.fault.tolist() == [0, 6, 0] and p.words[2].tolist() == [5, 0, 0] and p.ringpos[1].tolist() == [3, -1, -1]


def test_held_row_with_a_pending_open(emu_net):
    """OPEN (with RESET) on a held row: zeroed, active, no ring slot — and the first chunk it is present for starts at 0."""
    S, gen = 3, 9
    p = Paced(emu_net.emu_lib, S)
    p.words[0, 1] = RESET | OPEN | (gen << SHIFT)
    p.words[2] = torch.tensor([5, 4, 0], dtype=torch.int32)     # row 1: the previous listener's word
    p.fault[1] = 4
    p.hold[1] = 1
    p.ringpos[0] = torch.tensor([3, 17, 9], dtype=torch.int32)
    p.x[1] = float("nan")
    sets0, ring0 = p.state()
    p.begin()
    now, ring = p.state()
    assert all(not t[1].any() for st in now for t in st) and not ring[1].any()
    assert all(torch.equal(t[0], u[0]) and torch.equal(t[2], u[2]) for s in (0, 1) for t, u in zip(now[s], sets0[s]))
    assert p.ringpos[1].tolist() == [3, -1, -1] and not p.gated[1].any()
    p.sets[1][2][1] = 7                                         # what the chunk's kernels leave in the set they write
    p.lib.call("lh_ring_advance_rows", P(p.ringpos[0]), P(p.ringpos[1]), 50, S, None)
    p.end(0)
    assert not p.sets[1][2][1].any()                            # the carried state is the zeros
    assert p.words.tolist() == [[0, 0, 0], [0, RESET, 0], [5, gen, 0]] and p.fault.tolist() == [0, 0, 0]
    assert p.ringpos[0].tolist() == [4, 17, 9] and not p.out[1].any()
    # still held: nothing changes, the RESET stays posted
    p.begin()
    p.end(1)
    assert p.words.tolist() == [[0, 0, 0], [0, RESET, 0], [5, gen, 0]] and p.ringpos[1].tolist() == [4, -1, -1]
    # present: the row's first chunk
    p.hold[1] = 0
    p.x[1] = torch.randn(2, NFFT)
    p.sets[0][1][1] = 3
    out = p.out.clone()
    p.begin()
    assert p.ringpos[1].tolist() == [4, 0, -1] and torch.equal(p.gated[1], p.x[1]) and not p.sets[0][1][1].any()
    p.lib.call("lh_ring_advance_rows", P(p.ringpos[0]), P(p.ringpos[1]), 50, S, None)
    p.end(0)
    assert p.ringpos[0].tolist() == [5, 1, 9] and torch.equal(p.out[1], out[1])
    assert p.words.tolist() == [[0, 0, 0], [0, 0, 0], [5, gen, 0]] and p.fault.tolist() == [0, 0, 0]
    # CLOSE is served on a held row
    p.words[0, 1] = RESET | CLOSE
    p.hold[1] = 1
    p.begin()
    p.end(1)
    assert p.words.tolist() == [[0, 0, 0], [0, 0, 0], [5, 0, 0]] and p.ringpos[1].tolist() == [5, -1, -1]


def test_paced_row_forms_look_the_hold_up_by_slot(emu_net):
    """Rows 0, 1 hold slots 2 and 0 of S = 3; slot 2 is held: row 0 is gated and carried, slot 0 in row 1 plays."""
    lib, S, n = emu_net.emu_lib, 3, 2
    p = Paced(lib, S)
    t = torch.zeros(3, S, dtype=torch.int32)                    # from | slot_of | row_of
    t[1] = torch.tensor([2, 0, -1], dtype=torch.int32)
    t[2] = torch.tensor([1, -1, 0], dtype=torch.int32)
    p.words[2] = torch.tensor([5, 6, 0], dtype=torch.int32)
    p.hold[2] = 1
    p.x[2] = float("nan")
    p.sets[1][0][1] = torch.arange(28, dtype=torch.int32)       # row 1 plays: what end scans of it is finite
    p.ringpos[0] = torch.tensor([3, 7, 9], dtype=torch.int32)
    rows_out, out = torch.randn(S, 2, HOP), torch.full((S, 2, HOP), 9.0)
    sets0, _ = p.state()
    sp, ca, en = (ctypes.addressof(x) for x in (p.spans, p.carry[0], p.scan[0]))
    b_args = [sp, len(p.spans), P(p.x), P(p.gated), P(p.words), P(p.words[2]), P(t[1]), P(p.hold), P(p.ringpos[0]),
              P(p.ringpos[1]), n, S, None]
    e_args = [en, 1, ca, 3, P(p.x), P(rows_out), P(out), P(p.words), P(p.words[2]), P(p.fault), P(p.hold), P(t[1]), P(t[2]),
              P(t[0]), n, S, None]
    lib.call("lh_session_begin_rows_paced", *b_args)
    assert not p.gated[0].any() and torch.equal(p.gated[1], p.x[0]) and p.ringpos[1].tolist() == [-1, 7, 0]
    lib.call("lh_session_end_rows_paced", *e_args)
    assert not out[2].any() and torch.equal(out[0], rows_out[1]) and not out[1].any()
    assert all(torch.equal(p.sets[1][i][0], sets0[0][i][0]) and torch.equal(p.sets[1][i][1], sets0[1][i][1]) for i in range(3))
    assert p.words[2].tolist() == [5, 6, 0] and p.fault.tolist() == [0, 0, 0]
    # the position word moves with the row: 1 -> 2 over the three rows
    t[0, 2] = 2
    lib.call("lh_session_move_paced", sp, len(p.spans), P(t[0]), P(p.words), P(p.words[2]), P(p.ringpos[0]), S, S, None)
    assert p.ringpos[0].tolist() == [3, 7, 7] and p.words[2].tolist() == [5, 6, 6]
    assert all(torch.equal(x[2], x[1]) for st in p.sets for x in st) and torch.equal(p.ring[2], p.ring[1])
    raw_b, raw_e, raw_m = (lib.raw(x) for x in ("lh_session_begin_rows_paced", "lh_session_end_rows_paced",
                                                "lh_session_move_paced"))
    c = lambda a: [ctypes.c_void_p(v) if isinstance(v, int) and v > 4096 else v for v in a]
    bad = lambda a, i, v: c(a[:i] + [v] + a[i + 1:])
    assert raw_b(*c(b_args)) == 0 and raw_b(*bad(b_args, 7, None)) == ARG and raw_b(*bad(b_args, 10, S + 1)) == ARG
    assert raw_b(*bad(b_args, 9, None)) == ARG and raw_b(*bad(b_args, 6, None)) == ARG
    assert raw_e(*c(e_args)) == 0 and raw_e(*bad(e_args, 10, None)) == ARG and raw_e(*bad(e_args, 14, S + 1)) == ARG
    assert raw_e(*bad(e_args, 3, 0)) == ARG and raw_e(*bad(e_args, 2, None)) == ARG
    m_args = [sp, len(p.spans), P(t[0]), P(p.words), P(p.words[2]), P(p.ringpos[0]), S, S, None]
    assert raw_m(*bad(m_args, 5, None)) == ARG and raw_m(*bad(m_args, 6, S + 1)) == ARG


def test_paced_entry_points_validate_arguments(emu_net):
    S = 3
    p = Paced(emu_net.emu_lib, S)
    raw_b, raw_e = p.lib.raw("lh_session_begin_paced"), p.lib.raw("lh_session_end_paced")
    a = list(p.begin_args())
    assert raw_b(*a) == 0
    for i in (0, 2, 3, 4, 5, 6, 7, 8):                          # every pointer
        assert raw_b(*(a[:i] + [None] + a[i + 1:])) == ARG, i
    assert raw_b(*(a[:8] + [a[7]] + a[9:])) == ARG              # pos == write_pos
    assert raw_b(*(a[:9] + [0] + a[10:])) == ARG
    odd = (_Span * 1)(_Span(p.ring.data_ptr(), 24))             # a span that is not a multiple of 16 bytes
    assert raw_b(*p.begin_args(odd, 1)) == ARG
    e = list(p.end_args(0))
    assert raw_e(*e) == 0
    for i in (0, 2, 4, 5, 6, 7, 8, 9):
        assert raw_e(*(e[:i] + [None] + e[i + 1:])) == ARG, i
    assert raw_e(*(e[:3] + [0] + e[4:])) == ARG and raw_e(*(e[:3] + [17] + e[4:])) == ARG and raw_e(*(e[:10] + [0, None])) == ARG
    sp = lambda t, b: _Span(t.data_ptr(), b)
    uneven = (_Span * 2)(sp(p.sets[0][0], 112), sp(p.sets[1][0], 96))
    twice = (_Span * 2)(sp(p.sets[0][0], 112), sp(p.sets[0][0], 112))
    ragged = (_Span * 2)(sp(p.sets[0][0], 24), sp(p.sets[1][0], 24))
    for bad in (uneven, twice, ragged):
        assert raw_e(*(e[:2] + [ctypes.c_void_p(ctypes.addressof(bad)), 1] + e[4:])) == ARG


def test_capture_paced_records_present_chunks_only(emu_net):
    """n_chunks = 2, slot 0 armed and held in the second of three steps with a NaN row: the clip is the samples of steps 0 and
    2, nothing is judged in between, and the done word comes with the third step."""
    lib, S, gen = emu_net.emu_lib, 2, 3
    x = [torch.randn(S, 2, NFFT) for _ in range(3)]
    x[1][0] = float("nan")
    clip, ew, done = torch.zeros(S, 2, 2 * HOP), torch.zeros(3, S, dtype=torch.int32), torch.zeros(S, dtype=torch.int32)
    hold = torch.zeros(S, dtype=torch.int32)
    ew[0, 0] = ARM | (gen << SHIFT)
    seen = []
    for i in range(3):
        hold[0] = int(i == 1)
        lib.call("lh_session_capture_paced", P(x[i]), P(clip), P(ew), P(ew[1]), P(done), P(hold), 2, S, None)
        seen.append((ew.tolist(), done.tolist()))
    assert seen[0] == ([[0, 0], [gen, 0], [1, 0]], [0, 0]) and seen[1] == seen[0] and seen[2] == ([[0, 0]] * 3, [gen, 0])
    assert torch.equal(clip[0], torch.cat([x[0][0, :, :HOP], x[2][0, :, :HOP]], -1)) and not clip[1].any()
    # ARM is served on a held slot: armed, nothing recorded
    ew[0, 1], hold[1] = ARM | (5 << SHIFT), 1
    lib.call("lh_session_capture_paced", P(x[1]), P(clip), P(ew), P(ew[1]), P(done), P(hold), 2, S, None)
    assert ew.tolist() == [[0, 0], [0, 5], [0, 0]] and not clip[1].any() and done.tolist() == [gen, 0]
    raw = lib.raw("lh_session_capture_paced")
    assert raw(V(x[0]), V(clip), V(ew), V(ew[1]), V(done), None, 2, S, None) == ARG
    assert raw(V(x[0]), V(clip), V(ew), V(ew[1]), V(done), V(hold), 0, S, None) == ARG


# ---- the host over the emulated device ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clips():
    d = synth.batch([20, 21, 22], HOP * 10 + NFFT - HOP)
    return d["mixture"], d["embedding_gt"][:, 0]


def chunk_of(mix_row, j):
    return mix_row[:, j * HOP:j * HOP + NFFT]


def fresh_stream(oracle_cfg_sd, mix_row, emb_row, n):
    cfg, sd = oracle_cfg_sd
    y, _ = O.predict(cfg, sd, mix_row[None, :, :HOP * n + NFFT - HOP], emb_row[None], None, pad=False)
    return y[0]


def test_held_listener_end_to_end(emu_net, clips, oracle_cfg_sd):
    """S = 3, 9 steps.  Listener A (slot 0) is held at steps 1, 2 and 5, B (slot 1) opens at step 3, C (slot 2) is never held.
    Held and idle input rows are NaN."""
    mix, emb = clips
    S, n = 3, 9
    held = {0: (1, 2, 5)}
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, pace=True)
    ss.open(0, emb[0]), ss.open(2, emb[2])
    took, outs = [0] * S, [[] for _ in range(S)]
    for i in range(n):
        if i == 3:
            ss.open(1, emb[1])
        x = torch.full((S, 2, NFFT), float("nan"))
        present = [True] * S
        for s in ss.active:
            if i in held.get(s, ()):
                present[s] = False
            else:
                x[s] = chunk_of(mix[s], took[s])
        y = ss.step(x, present if i % 2 else torch.tensor(present))
        for s in range(S):
            if s in ss.active and present[s]:
                outs[s].append(y[s].clone())
                took[s] += 1
            else:
                assert not y[s].any(), (i, s)                   # held, or idle: exact zeros
    assert took == [6, 6, 9] and ss.faults() == [] and ss.active == [0, 1, 2]
    assert ss._ring[0].tolist() == took                         # every row's own position
    y = [torch.cat(o, -1) for o in outs]
    for s in range(S):
        e = float((y[s] - fresh_stream(oracle_cfg_sd, mix[s], emb[s], took[s])).abs().max())
        print(f"slot {s}, {took[s]} chunks: max|emu - oracle fresh stream| =", e)
        assert e < TOL, s
    # A without holds, in the same object
    ss.reset()
    ss.open(0, emb[0])
    x = torch.full((S, 2, NFFT), float("nan"))
    plain = []
    for j in range(6):
        x[0] = chunk_of(mix[0], j)
        plain.append(ss.step(x)[0].clone())
    assert torch.equal(torch.cat(plain, -1), y[0])


def test_lock_step_object_is_unchanged(emu_net):
    """pace=False: `_body` calls none of the new entry points, and `present` is refused."""
    S, lib = 2, emu_net.emu_lib
    for kw in ({}, {"compact": True}, {"enroll_chunks": 2}):
        ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, **kw)
        assert not ss.pace
        names, call = [], lib.call
        with mock.patch.object(lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1]):
            ss._body(0, S)
        assert "lh_qkv_proj_ln" in names and "lh_ring_advance" in names and not set(names) & set(NEW), kw
        with pytest.raises(ValueError):
            ss.step(torch.zeros(S, 2, NFFT), present=[True] * S)
    ss = emu_net.make_session_streamer(S, "cpu", use_graph=False, pace=True, compact=True, enroll_chunks=2)
    names = []
    with mock.patch.object(lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1]):
        ss._body(0, S)
    assert set(NEW) - set(names) == {"lh_session_begin_paced", "lh_session_end_paced"}
    assert "lh_qkv_proj_ln" not in names and "lh_ring_advance" not in names
    with pytest.raises(ValueError):
        ss.step(torch.zeros(S, 2, NFFT), present=[True])
