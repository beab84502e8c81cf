"""CPU: `SessionStreamer.suspend` / `resume`, `SessionSnapshot` (sessions.py) and their entry points `lh_session_save` /
`lh_session_restore` (lh_stream.hip) over the emulated library, eager.  A snapshot is bytes: what a listener owns is copied out
of one set of buffers and into another, so every claim about state is `torch.equal` on integers, NaN and inf patterns among
them; a resumed listener's output is `torch.equal` to the uninterrupted run.  Small on purpose: the emulator runs a chunk row
in ~0.5 s."""
import contextlib
import ctypes
from unittest import mock

import numpy as np
import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.net import SessionSnapshot, _Span
from tests.hipemu.hosts import EmuNet
from oracle import tfgridnet_oracle as O

HOP, NFFT = 128, 192
RESET, OPEN, CLOSE, SHIFT = 1, 2, 4, 8
ARG = 1
MAGIC, VERSION, HEADER = 0x5353484c, 1, 256
V = lambda v: ctypes.c_void_p(v.data_ptr())
A = lambda t: ctypes.c_void_p(ctypes.addressof(t))


class EmuSessionNet(EmuNet):
    def _host_words(self, n, device):               # the pinned words of the GPU host: plain host memory here
        return torch.zeros(n, dtype=torch.int32)

    def _enroll_side(self, dev):                    # no embedder runs here
        return None

    def _record_event(self, device):                # every launch has finished when it returns: nothing to order
        return None

    def _wait_event(self, device, ev, tensor=None):
        assert ev is None


@pytest.fixture(scope="module")
def emu_net(oracle_cfg_sd):
    from tests.hipemu.build_emu import build_emu
    cfg, sd = oracle_cfg_sd
    net = EmuSessionNet(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net.emu_lib = _cabi.Lib(build_emu())
    return net


def patterns(*shape):
    """Random 32-bit patterns, NaN and inf patterns among them (tests/test_emu_pace.py): a snapshot copies bytes, not numbers."""
    t = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int64).to(torch.int32)
    flat = t.view(-1)
    special = torch.tensor([0x7fc00000, 0x7f800000, -0x800000, 0x7f800001, -1, 0x7fffffff], dtype=torch.int64).to(torch.int32)
    idx = torch.randperm(flat.numel())[:max(6, flat.numel() // 50)]
    flat[idx] = special[torch.arange(idx.numel()) % special.numel()]
    return t


# ---- the two kernels on hand-made buffers ---------------------------------------------------------------------------------
class Bufs:
    """S rows of two ping-pong sets of three state tensors — 112 bytes, 16000, and one that gives every one of the copy's 32
    tiles more than one pass of its loop (256 threads x 4 loads x 16 bytes) and a ragged end — two rings of 2 heads x
    (50 + 48) rows x 32 bytes, an embedding of 256 bytes per row, the words and the buffers of a chunk's two bracket kernels."""
    BYTES = [112, 16000, 32 * 16384 + 16 * 37]
    HEADS, ROWS, WIN, RB, EMB = 2, 98, 50, 32, 256
    SNAP = HEADER + 16 + EMB + sum(BYTES) + 2 * HEADS * WIN * RB

    def __init__(self, lib, S, seed):
        torch.manual_seed(seed)
        self.lib, self.S = lib, S
        self.sets = [[patterns(S, b // 4) for b in self.BYTES] for _ in (0, 1)]
        self.rings = [patterns(S * self.HEADS, self.ROWS, self.RB // 4) for _ in (0, 1)]
        self.embed = patterns(S, self.EMB // 4)
        self.words = torch.zeros(3, S, dtype=torch.int32)       # cmd host | cmd device | active
        self.pos = torch.zeros(2, S, dtype=torch.int32)         # a paced host's pos | write_pos
        self.shared = torch.zeros(1, dtype=torch.int32)         # a lock-step host's counter
        self.hold = torch.zeros(S, dtype=torch.int32)
        self.fault = torch.zeros(S, dtype=torch.int32)
        self.x, self.gated, self.out = torch.randn(S, 2, NFFT), torch.full((S, 2, NFFT), 9.0), torch.randn(S, 2, HOP)
        sp = lambda t: _Span(t.data_ptr(), t.shape[1] * 4)
        self.live = [(_Span * 3)(*[sp(t) for t in st]) for st in self.sets]
        self.ring_tab = (_Span * 2)(*[_Span(t.data_ptr(), self.RB) for t in self.rings])
        every = self.sets[0] + self.sets[1]
        per_slot = self.HEADS * self.ROWS * self.RB
        self.spans = (_Span * 8)(*[sp(t) for t in every], *[_Span(t.data_ptr(), per_slot) for t in self.rings])
        self.scan = [(_Span * 1)(sp(self.sets[k ^ 1][0])) for k in (0, 1)]
        self.carry = [(_Span * 6)(*[sp(t) for pair in zip(self.sets[k], self.sets[k ^ 1]) for t in pair]) for k in (0, 1)]

    def head(self, k, row):
        """lh_session_save / lh_session_restore up to the embedding: the live set is set k."""
        return [A(self.live[k]), 3, A(self.ring_tab), 2, self.HEADS, self.ROWS, self.WIN, V(self.embed[row]), self.EMB]

    def save_args(self, k, row, snap, paced=True):
        pos = self.pos[0, row:row + 1] if paced else self.shared
        return self.head(k, row) + [V(snap), snap.numel(), V(self.words), V(self.words[2]), V(pos), row, self.S, None]

    def restore_args(self, k, row, snap, gen, paced=True):
        pos = [V(self.pos[0, row:row + 1]), None] if paced else [None, V(self.shared)]
        return self.head(k, row) + [V(snap), snap.numel(), V(self.words)] + pos + [V(self.fault[row:row + 1]), gen, row, self.S,
                                                                                  None]

    def save(self, k, row, paced=True):
        snap = torch.full((self.SNAP,), 0x5a, dtype=torch.uint8)
        assert self.lib.raw("lh_session_save")(*self.save_args(k, row, snap, paced)) == 0
        return snap

    def restore(self, k, row, snap, gen, paced=True):
        assert self.lib.raw("lh_session_restore")(*self.restore_args(k, row, snap, gen, paced)) == 0

    def bracket(self, k):
        """One chunk's lh_session_begin_paced -> lh_ring_advance_rows -> lh_session_end_paced, no separator in between."""
        lib, S = self.lib, self.S
        lib.call("lh_session_begin_paced", ctypes.addressof(self.spans), 8, self.x.data_ptr(), self.gated.data_ptr(),
                 self.words.data_ptr(), self.words[2].data_ptr(), self.hold.data_ptr(), self.pos[0].data_ptr(),
                 self.pos[1].data_ptr(), S, None)
        wrote = self.pos[1].tolist()
        lib.call("lh_ring_advance_rows", self.pos[0].data_ptr(), self.pos[1].data_ptr(), self.WIN, S, None)
        lib.call("lh_session_end_paced", ctypes.addressof(self.scan[k]), 1, ctypes.addressof(self.carry[k]), 3,
                 self.x.data_ptr(), self.out.data_ptr(), self.words.data_ptr(), self.words[2].data_ptr(), self.fault.data_ptr(),
                 self.hold.data_ptr(), S, None)
        return wrote

    def everything(self):
        return [t.clone() for st in self.sets for t in st] + [t.clone() for t in self.rings] + \
               [self.embed.clone(), self.words.clone(), self.pos.clone(), self.shared.clone(), self.fault.clone()]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def source(lib, pos=13, active=7, cmd1=0):
    """Three rows; row 1 is the listener: their own ring position, their words."""
    src = Bufs(lib, 3, seed=1)
    src.words[2] = torch.tensor([3, active, 4], dtype=torch.int32)
    src.words[1] = torch.tensor([0, cmd1, RESET], dtype=torch.int32)
    src.pos[0] = torch.tensor([21, pos, 22], dtype=torch.int32)
    src.shared[0] = 41
    return src


def test_snapshot_layout_and_paced_round_trip(emu_net):
    """Save row 1 of a source whose live set is set 0, restore into row 2 of a differently filled paced target whose live set
    is set 1."""
    lib, H, W = emu_net.emu_lib, Bufs.HEADS, Bufs.WIN
    src = source(lib, pos=13, active=7, cmd1=RESET)
    before = src.everything()
    snap = src.save(0, 1)
    assert same(src.everything(), before)                       # save writes the snapshot only
    # the layout of include/lookonce_hip.h
    head = snap[:HEADER].view(torch.int32).tolist()
    assert head[:8] == [MAGIC, VERSION, Bufs.SNAP, 3, 2, H, W, Bufs.EMB] and head[8:13] == Bufs.BYTES + [Bufs.RB] * 2
    assert not any(head[13:])
    assert snap[HEADER:HEADER + 16].view(torch.int32).tolist() == [7, RESET, 13, 0]
    o = HEADER + 16
    assert torch.equal(snap[o:o + Bufs.EMB].view(torch.int32), src.embed[1])
    o += Bufs.EMB
    for i, b in enumerate(Bufs.BYTES):
        assert torch.equal(snap[o:o + b].view(torch.int32), src.sets[0][i][1]), i
        o += b
    for r in src.rings:
        n = H * W * Bufs.RB
        assert torch.equal(snap[o:o + n].view(torch.int32).view(H, W, -1), r[H:2 * H, :W])
        o += n
    assert o == snap.numel() == Bufs.SNAP
    # a lock-step source saves the shared counter
    assert src.save(0, 1, paced=False)[HEADER:HEADER + 16].view(torch.int32).tolist() == [7, RESET, 41, 0]
    assert torch.equal(src.save(0, 1, paced=False)[HEADER + 16:], snap[HEADER + 16:])

    dst = Bufs(lib, 3, seed=2)
    dst.words[0, 2] = OPEN | (9 << SHIFT)                       # what the host has posted for the row
    dst.words[2] = torch.tensor([5, 6, 8], dtype=torch.int32)
    dst.pos[0] = torch.tensor([1, 2, 3], dtype=torch.int32)
    was = dst.everything()
    keep = snap.clone()
    dst.restore(1, 2, snap, gen=9)
    assert torch.equal(snap, keep) and same(src.everything(), before)
    for i in range(3):
        assert torch.equal(dst.sets[1][i][2], src.sets[0][i][1]), i                         # the live set's slices
        assert torch.equal(dst.sets[1][i][:2], was[3 + i][:2]), i                           # rows 0 and 1
        assert torch.equal(dst.sets[0][i], was[i]), i                                       # the dead set
        assert not torch.equal(src.sets[0][i][1], was[3 + i][2])
    for i in range(2):
        assert torch.equal(dst.rings[i][2 * H:, :W], src.rings[i][H:2 * H, :W]), i          # the window rows, raw order
        assert torch.equal(dst.rings[i][2 * H:, W:], was[6 + i][2 * H:, W:]), i             # the pad rows
        assert torch.equal(dst.rings[i][:2 * H], was[6 + i][:2 * H]), i
    assert torch.equal(dst.embed[2], src.embed[1]) and torch.equal(dst.embed[:2], was[8][:2])
    assert dst.pos.tolist() == [[1, 2, 13], [0, 0, 0]] and dst.shared.tolist() == [0]
    # cmd[1][2] is the saved word; the host's OPEN stands (the snapshot is alive); nobody else's word, no fault word
    assert dst.words.tolist() == [[0, 0, OPEN | (9 << SHIFT)], [0, 0, RESET], [5, 6, 8]] and dst.fault.tolist() == [0, 0, 0]


@pytest.mark.parametrize("saved,shared", [(49, 0), (7, 7), (3, 30)])
def test_lock_step_target_rotates_the_ring(emu_net, saved, shared):
    """Ring row j lands at (j + delta) % 50, delta = (shared position now - saved position) % 50, in each head: the row at the
    saved position — the listener's oldest — is the next one the shared counter overwrites."""
    lib, H, W = emu_net.emu_lib, Bufs.HEADS, Bufs.WIN
    src = source(lib, pos=saved)
    snap = src.save(1, 1)
    dst = Bufs(lib, 3, seed=2)
    dst.shared[0] = shared
    dst.words[0, 2] = OPEN | (9 << SHIFT)
    was = dst.everything()
    dst.restore(0, 2, snap, gen=9, paced=False)
    delta = (shared - saved) % W
    to = [(j + delta) % W for j in range(W)]
    for i in range(2):
        assert torch.equal(dst.rings[i][2 * H:, to], src.rings[i][H:2 * H, :W]), i
        assert torch.equal(dst.rings[i][2 * H:, shared], src.rings[i][H:2 * H, saved]), i
        assert torch.equal(dst.rings[i][2 * H:, W:], was[6 + i][2 * H:, W:]) and torch.equal(dst.rings[i][:2 * H], was[6 + i][:2 * H])
    for i in range(3):
        assert torch.equal(dst.sets[0][i][2], src.sets[1][i][1]) and torch.equal(dst.sets[1][i], was[3 + i]), i
    assert dst.shared.tolist() == [shared] and torch.equal(dst.pos, was[10])          # read, never written; no row position
    # the same snapshot into a paced target: raw order, the row's position is the saved one
    dst.restore(0, 0, snap, gen=9)
    assert all(torch.equal(dst.rings[i][:H, :W], src.rings[i][H:2 * H, :W]) for i in range(2)) and int(dst.pos[0, 0]) == saved


@pytest.mark.parametrize("cmd1", [0, RESET], ids=["input_fault", "overflow"])
def test_dead_snapshot_stays_dead(emu_net, cmd1):
    """active = 0: the device had closed the listener in the chunk before the save.  After restore and one chunk's bracket the
    row is idle and zeroed, its output is zeros and its fault word is the generation of the opening the host had posted."""
    lib, gen = emu_net.emu_lib, 9
    snap = source(lib, active=0, cmd1=cmd1).save(0, 1)
    dst = Bufs(lib, 3, seed=2)
    dst.words[0, 2] = OPEN | (gen << SHIFT)
    dst.words[2] = torch.tensor([0, 0, 8], dtype=torch.int32)   # rows 0, 1 idle; row 2: the previous listener's word
    dst.fault[2] = 8
    dst.restore(1, 2, snap, gen)
    assert dst.words.tolist() == [[0, 0, CLOSE | RESET], [0, 0, cmd1], [0, 0, 8]] and dst.fault.tolist() == [0, 0, gen]
    was = dst.everything()
    assert dst.bracket(1) == [-1, -1, -1]
    assert dst.words.tolist() == [[0, 0, 0]] * 3 and dst.fault.tolist() == [0, 0, gen] and not dst.out[2].any()
    assert not dst.gated.any()
    assert all(not t[2].any() for st in dst.sets for t in st) and not dst.rings[0][4:].any() and not dst.rings[1][4:].any()
    now = dst.everything()
    for a, b in zip(now[:6], was[:6]):                          # no other row changes a bit
        assert torch.equal(a[:2], b[:2])
    assert torch.equal(now[6][:4], was[6][:4]) and torch.equal(now[7][:4], was[7][:4])


def test_held_unconsumed_listener_is_alive(emu_net):
    """active != 0 with RESET pending: a paced listener opened and held who has consumed nothing.  The row comes alive and the
    RESET is served: zero state, ring slot 0."""
    lib, gen = emu_net.emu_lib, 9
    snap = source(lib, pos=17, active=5, cmd1=RESET).save(0, 1)
    dst = Bufs(lib, 3, seed=2)
    dst.words[0, 2] = OPEN | (gen << SHIFT)
    dst.fault[2] = 3
    dst.restore(1, 2, snap, gen)
    assert dst.words.tolist() == [[0, 0, OPEN | (gen << SHIFT)], [0, 0, RESET], [0, 0, 0]] and dst.fault.tolist() == [0, 0, 3]
    out = dst.out.clone()
    assert dst.bracket(1) == [-1, -1, 0]
    assert dst.words.tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, gen]] and dst.fault.tolist() == [0, 0, 0]
    assert torch.equal(dst.gated[2], dst.x[2]) and torch.equal(dst.out[2], out[2]) and dst.pos[0].tolist() == [0, 0, 1]
    assert all(not t[2].any() for st in dst.sets for t in st) and not dst.rings[0][4:].any()


def test_entry_points_validate_arguments(emu_net):
    lib = emu_net.emu_lib
    b = Bufs(lib, 3, seed=3)
    snap = torch.zeros(Bufs.SNAP + 16, dtype=torch.uint8)
    save, restore = lib.raw("lh_session_save"), lib.raw("lh_session_restore")
    s, r = b.save_args(0, 1, snap), b.restore_args(0, 1, snap, 9)
    assert save(*s) == 0 and restore(*r) == 0
    sub = lambda a, i, v: a[:i] + [v] + a[i + 1:]
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    for i in (0, 2, 7, 9, 11, 12, 13):                          # every pointer of save
        assert save(*sub(s, i, None)) == ARG, i
    for i in (0, 2, 7, 9, 11, 14):                              # ... of restore; 12 / 13 are the two positions
        assert restore(*sub(r, i, None)) == ARG, i
    assert restore(*sub(r, 12, None)) == ARG                                        # neither position
    assert restore(*sub(r, 13, V(b.shared))) == ARG                                 # both
    assert restore(*sub(sub(r, 12, None), 13, V(b.shared))) == 0
    for fn, a in ((save, s), (restore, r)):
        assert fn(*sub(a, 9, off(snap, 4))) == ARG and fn(*sub(a, 7, off(b.embed, 8))) == ARG       # unaligned
        assert fn(*sub(a, 9, off(snap, 16))) == 0
        for i, bad in ((1, 0), (1, 33), (3, 0), (3, 9), (4, 0), (6, 0), (6, Bufs.ROWS + 1), (8, 0), (8, 24)):
            assert fn(*sub(a, i, bad)) == ARG, (i, bad)                             # counts, geometry, embedding size
        assert fn(*sub(a, 10, Bufs.SNAP - 1)) == ARG and fn(*sub(a, 10, Bufs.SNAP)) == 0            # smaller than the layout
    assert save(*sub(s, 14, -1)) == ARG and save(*sub(s, 14, 3)) == ARG and save(*sub(s, 15, 0)) == ARG
    assert restore(*sub(r, 16, -1)) == ARG and restore(*sub(r, 16, 3)) == ARG and restore(*sub(r, 17, 0)) == ARG
    assert restore(*sub(r, 15, 0)) == ARG and restore(*sub(r, 15, 1 << 23)) == ARG                  # the generation
    ragged = (_Span * 3)(_Span(b.sets[0][0].data_ptr(), 24), *list(b.live[0])[1:])
    odd_ring = (_Span * 2)(_Span(b.rings[0].data_ptr(), 40), _Span(b.rings[1].data_ptr(), Bufs.RB))
    low = (_Span * 3)(_Span(b.sets[0][0].data_ptr() + 4, 112), *list(b.live[0])[1:])
    for fn, a in ((save, s), (restore, r)):
        assert fn(*sub(a, 0, A(ragged))) == ARG and fn(*sub(a, 2, A(odd_ring))) == ARG and fn(*sub(a, 0, A(low))) == ARG


# ---- the host over the emulated device ------------------------------------------------------------------------------------
@contextlib.contextmanager
def no_host_wait():
    def refuse(*a, **k):
        raise AssertionError("the host waited for the device inside the chunk loop")
    with mock.patch.object(torch.cuda, "synchronize", refuse), mock.patch.object(torch.cuda.Stream, "synchronize", refuse), \
            mock.patch.object(torch.cuda.Event, "synchronize", refuse):
        yield


def chunk_of(mix_row, j):
    return mix_row[:, j * HOP:j * HOP + NFFT]


@pytest.fixture(scope="module")
def moved(emu_net):
    """Listener A runs 3 chunks in slot 0 of the paced streamer X next to B in slot 1, is suspended, and after two more steps
    of X resumes in slot 1 of the compacting paced streamer Y for 3 more chunks; and both listeners' uninterrupted runs."""
    d = synth.batch([20, 21], HOP * 6 + NFFT - HOP)
    mix, emb = d["mixture"], d["embedding_gt"][:, 0]
    nan = lambda: torch.full((2, 2, NFFT), float("nan"))
    r = dict(mix=mix, emb=emb)
    with no_host_wait():
        X = emu_net.make_session_streamer(2, "cpu", use_graph=False, pace=True)
        Y = emu_net.make_session_streamer(2, "cpu", use_graph=False, pace=True, compact=True)
        X.open(0, emb[0]), X.open(1, emb[1])
        with pytest.raises(ValueError):
            X.suspend(0)                                        # opened, not served yet: no device state
        xs = []
        for i in range(5):
            if i == 3:
                r["snap"], r["x_parity"] = X.suspend(0), X._st.parity      # X's live set after 3 chunks
                assert X.active == [1]
            x = nan()
            x[1] = chunk_of(mix[1], i)
            if i < 3:
                x[0] = chunk_of(mix[0], i)
            xs.append(X.step(x).clone())
        r["y_parity"] = Y._st.parity
        Y.resume(1, r["snap"])
        assert Y.active == [1]
        ys = []
        for i in range(3, 6):
            x = nan()
            x[1] = chunk_of(mix[0], i)
            ys.append(Y.step(x).clone())
        r["y_rows"] = (list(Y._row_of), Y.last_rows)
        ref = emu_net.make_session_streamer(2, "cpu", use_graph=False, pace=True, compact=True)
        ref.open(0, emb[0]), ref.open(1, emb[1])
        rs = []
        for i in range(6):
            x = nan()
            x[0] = chunk_of(mix[0], i)
            if i < 5:
                x[1] = chunk_of(mix[1], i)
            rs.append(ref.step(x, [True, i < 5]).clone())
    r["end"] = (X.faults(), Y.faults(), X.active, Y.active)
    r.update(X=X, Y=Y, xs=torch.stack(xs), ys=torch.stack(ys), ref=torch.stack(rs))
    return r


def test_listener_moves_between_streamers_bit_for_bit(emu_net, moved):
    m = moved
    assert m["x_parity"] != m["y_parity"] and m["y_rows"] == ([-1, 0], 1)      # another parity, another row, another slot
    got = torch.cat([m["xs"][:3, 0], m["ys"][:, 1]])
    assert torch.equal(got, m["ref"][:, 0]) and got.abs().max() > 1e-3          # A: 6 chunks as if nothing had happened
    assert torch.equal(m["xs"][:, 1], m["ref"][:5, 1])                          # B: as without the traffic
    assert not m["xs"][3:, 0].any() and not m["ys"][:, 0].any()                 # X's slot 0 after the suspend: zeros
    assert m["end"] == ([], [], [1], [1])
    snap = m["snap"]
    assert isinstance(snap, SessionSnapshot) and snap.data.dtype == torch.uint8 and snap.data.is_contiguous()
    assert snap.data.numel() == SessionSnapshot.layout_bytes(snap.layout) and 5.3e6 < snap.data.numel() < 5.5e6
    assert snap.data[:8].view(torch.int32).tolist() == [MAGIC, VERSION]
    assert torch.equal(snap.data[HEADER + 16:HEADER + 16 + 1024].view(torch.float32), m["emb"][0])
    assert snap.to("cpu") is snap and snap.cpu() is snap and snap.event is None


def test_resumed_slot_is_an_open_slot(emu_net, moved):
    """What `open` refuses `resume` refuses; `close`, `set_embedding` and `suspend` work on a resumed slot."""
    Y, snap = moved["Y"], moved["snap"]
    with pytest.raises(ValueError):
        Y.resume(1, snap)                                       # open
    with pytest.raises(IndexError):
        Y.resume(2, snap)
    with pytest.raises(IndexError):
        Y.suspend(2)
    with pytest.raises(ValueError):
        Y.suspend(0)                                            # idle
    with pytest.raises(ValueError):
        Y.embedding_of(1)                                       # for enrolled slots only
    Y.resume(0, snap)                                           # a snapshot is a value: the same one again
    with pytest.raises(ValueError):
        Y.suspend(0)                                            # no step has served the resume yet
    Y.set_embedding(0, moved["emb"][1])
    Y.close(0)
    assert Y.active == [1] and not Y._resumes
    again = Y.suspend(1)                                        # Y's listener, 6 chunks in
    assert Y.active == [] and again.layout == snap.layout and not torch.equal(again.data, snap.data)
    assert again.data[HEADER:HEADER + 16].view(torch.int32).tolist()[2] == 6


def test_snapshot_survives_a_file(emu_net, moved, tmp_path):
    """save -> load -> resume gives the bits of resuming the object itself; a changed header size is refused."""
    m, path = moved, str(tmp_path / "listener.lhss")
    m["snap"].save(path)
    back = SessionSnapshot.load(path)
    assert back.layout == m["snap"].layout and torch.equal(back.data, m["snap"].data) and back.event is None
    Z = emu_net.make_session_streamer(2, "cpu", use_graph=False, pace=True, compact=True)
    Z.resume(1, back)
    for i in range(3, 6):
        x = torch.full((2, 2, NFFT), float("nan"))
        x[1] = chunk_of(m["mix"][0], i)
        assert torch.equal(Z.step(x), m["ys"][i - 3]), i
    raw = np.fromfile(path, dtype=np.uint8)
    words = raw[:HEADER].view("<u4")
    words[8] += 16                                              # the first tensor's size: the file no longer adds up
    raw.tofile(path)
    with pytest.raises(ValueError):
        SessionSnapshot.load(path)
    words[8] -= 32                                              # ... and one that adds up with the next: another layout
    words[9] += 16
    raw.tofile(path)
    other = SessionSnapshot.load(path)
    assert other.layout != back.layout
    with pytest.raises(ValueError):
        Z.resume(0, other)
    words[0] ^= 1
    raw.tofile(path)
    with pytest.raises(ValueError):
        SessionSnapshot.load(path)
    assert Z.active == [1]


def test_same_slot_resume_in_a_step_that_moves_rows(emu_net, moved):
    """S = 4, paced and compacting: slots 0 and 1 are fillers, slot 2 plays clip 1, slot 3 — the top row — plays clip 0 for one
    chunk, is suspended and opened for somebody else.  Then ONE step closes the fillers, suspends slot 3's second listener and
    resumes the first one in the same slot: the previous listener's row is given up and not moved over the restored one, the
    survivor of row 2 moves to row 0, the resume takes the hole at row 1.  Both keep the bits of the uninterrupted run."""
    mix, emb, ref = moved["mix"], moved["emb"], moved["ref"]
    ss = emu_net.make_session_streamer(4, "cpu", use_graph=False, pace=True, compact=True)
    ss.open(0, emb[1]), ss.open(1, emb[1]), ss.open(2, emb[1]), ss.open(3, emb[0])
    plays = [[(1, 0), (1, 0), (1, 0), (0, 0)], [(1, 1), (1, 1), (1, 1), (1, 0)], [None, None, (1, 2), (0, 1)]]   # (clip, chunk)
    ys, snap = [], None
    for i, row in enumerate(plays):
        if i == 1:
            snap = ss.suspend(3)
            ss.open(3, emb[1])
        if i == 2:
            ss.close(0), ss.close(1)
            ss.suspend(3)
            ss.resume(3, snap)
        x = torch.full((4, 2, NFFT), float("nan"))
        for s, p in enumerate(row):
            if p is not None:
                x[s] = chunk_of(mix[p[0]], p[1])
        ys.append(ss.step(x).clone())
        if i == 1:
            assert ss._row_of == [0, 1, 2, 3]
    assert ss._row_of == [-1, -1, 0, 1] and ss.rows_in_use == 2 and ss.last_rows == 2 and ss.faults() == [] and ss.active == [2, 3]
    assert torch.equal(torch.stack([ys[0][3], ys[2][3]]), ref[:2, 0]) and ys[2][3].abs().max() > 1e-3
    assert torch.equal(torch.stack([y[2] for y in ys]), ref[:3, 1])
    assert torch.equal(ys[1][3], ref[0, 1]) and not ys[2][:2].any()


def test_streamer_without_suspends_is_unchanged(emu_net, moved):
    """Nobody suspends or resumes: `_body` and a `step` with open and close traffic call neither new entry point, in any flavour."""
    lib, call = emu_net.emu_lib, emu_net.emu_lib.call
    x = torch.full((2, 2, NFFT), float("nan"))
    x[0] = chunk_of(moved["mix"][0], 0)
    for kw in ({}, {"compact": True}, {"pace": True}, {"pace": True, "compact": True}):
        ss = emu_net.make_session_streamer(2, "cpu", use_graph=False, **kw)
        names = []
        with mock.patch.object(lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1]):
            ss._body(0, 2)
            ss.open(0, moved["emb"][0])
            ss.step(x)
            ss.close(0), ss.open(1, moved["emb"][1])
            ss.step(x.flip(0))                                  # slot 1 gets the samples, slot 0's row is NaN
        assert names.count("lh_embed_proj_ln") == 2 and not {"lh_session_save", "lh_session_restore"} & set(names), kw
        assert not ss._resumes and ss.active == [1]
