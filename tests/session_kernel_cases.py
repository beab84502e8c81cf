"""Shared by tests/test_emu_session_kernels.py (hipemu, CPU) and tests/test_gpu_session_kernels.py (MI355X): the session
kernels of lh_stream.hip — begin, end, move, capture, save / restore and `lh_ring_advance_rows`, in all their ROWS / PACED
forms — called directly on hand-made buffers and held to an integer restatement of include/lookonce_hip.h.

The restatement (`ref_*`) is written from the header's text alone, in numpy on uint32 words: it takes a dict of every buffer
of the call and returns a dict of every buffer after it, so a buffer the header says is not written comes back as it went in.
The runner (`Dev`, `check`) puts every buffer into a `stage_cases.Guarded` region on the device ("cpu": the emulated library),
calls the entry point once and compares every buffer, word for word, and every guard.  `fault` and `edone` live in pinned host
memory on a GPU and are read in place after one synchronize.  Nothing here has a tolerance: these kernels move bytes and words.

Span contents are a running counter below 2^30: distinct per (span, row, element), so a float4 that lands in the wrong row,
span or tile shows, and finite as fp32 bits, so `lh_session_end` may scan them."""
from __future__ import annotations

import ctypes
import itertools

import numpy as np
import torch

from tests.stage_cases import GUARD, Guarded

U32, I32 = np.uint32, np.int32
IN_W, OUT_W, HOP = 384, 256, 128                      # words of an input row [2][192], of an output row [2][128]
RESET, OPEN, CLOSE, GEN_SHIFT, GEN_MASK = 1, 2, 4, 8, 0x7FFFFF
MAX_SPANS, MAX_END_SPANS = 32, 8
ARM, CANCEL, EFAULT = 1, 2, 0x80000000
MAGIC, VERSION, HEADER_W, MAX_RINGS = 0x5353484C, 1, 64, 8
ERR_ARG = 1
EXP = 0x7F800000
NAN, INF, NINF = 0x7FC00000, 0x7F800000, 0xFF800000
PINNED = ("fault", "edone")


class Span(ctypes.Structure):                          # lh_span_t
    _fields_ = [("base", ctypes.c_void_p), ("bytes", ctypes.c_ulonglong)]


def nonfinite(words) -> bool:
    w = np.asarray(words, dtype=U32)
    return bool(((w & U32(EXP)) == U32(EXP)).any())


def s32(v) -> int:
    """A stored word as the signed int the header's `int` arrays hold."""
    return int(np.array(v, dtype=U32).view(I32))


class Counter:
    """Distinct finite words: 1, 2, 3, .. below 2^30."""

    def __init__(self, start=1):
        self.at = start

    def take(self, *shape) -> np.ndarray:
        n = int(np.prod(shape))
        a = np.arange(self.at, self.at + n, dtype=np.int64)
        self.at += n
        assert self.at < 1 << 30
        return a.astype(U32).reshape(shape)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def decide(host, dev, act, x, owned=True, held=False):
    """'Per slot, with c = cmd[0][s] | cmd[1][s]' -> (c, generation or 0, bad_in, live).  A row without a listener decides as
    if the host's word were CLOSE; a held row is open to the words and its input is not looked at."""
    host, dev, act = int(host), int(dev), int(act)
    if not owned:
        host = CLOSE
    c = host | dev
    if c & OPEN:
        gen = ((host >> GEN_SHIFT) & GEN_MASK) or 1
    elif c & CLOSE:
        gen = 0
    else:
        gen = act
    if held:
        return c, gen, False, gen != 0
    bad_in = gen != 0 and owned and nonfinite(x)
    return c, gen, bad_in, gen != 0 and not bad_in


def _row(b, r, S, rows):
    if not rows:
        return r, True
    slot = s32(b["slot_of"][r])
    return (slot, True) if 0 <= slot < S else (0, False)


def _copy(b):
    return {k: v.copy() for k, v in b.items()}


def ref_begin(b, spans, S, n_rows=None, rows=False, paced=False):
    b0, b = b, _copy(b)
    for r in range(n_rows if rows else S):
        slot, owned = _row(b0, r, S, rows)
        held = paced and owned and b0["hold"][slot] != 0
        c, gen, bad_in, live = decide(b0["cmd"][0, r], b0["cmd"][1, r], b0["active"][r], b0["chunk_in"][slot], owned, held)
        takes = live and not held
        b["chunk"][r] = b0["chunk_in"][slot] if takes else 0
        if paced:
            b["write_pos"][r] = U32(0xFFFFFFFF) if not takes else (0 if c & RESET else b0["pos"][r])
        if (c & RESET) or bad_in:
            for s in spans:
                b[s][r] = 0
    return b


def ref_end(b, spans, S, n_rows=None, rows=False, paced=False, carry=()):
    b0, b = b, _copy(b)
    n = n_rows if rows else S
    src = "out_rows" if rows else "out"
    for r in range(n):
        slot, owned = _row(b0, r, S, rows)
        held = paced and owned and b0["hold"][slot] != 0
        c, gen, bad_in, live = decide(b0["cmd"][0, r], b0["cmd"][1, r], b0["active"][r], b0["chunk_in"][slot], owned, held)
        scan = nonfinite(b0[src][r]) or any(nonfinite(b0[s][r]) for s in spans)
        overflow = live and not held and scan
        on = live and not overflow
        if held:
            for i in range(0, len(carry), 2):
                b[carry[i + 1]][r] = b0[carry[i]][r]
        if owned:
            b["out"][slot] = b0[src][r] if on and not held else 0
            if bad_in or overflow:
                b["fault"][slot] = gen
            elif c & OPEN:
                b["fault"][slot] = 0
        b["active"][r] = gen if on else 0
        b["cmd"][0, r] = 0
        b["cmd"][1, r] = RESET if overflow or (held and on and (c & RESET)) else 0
        if rows and "from" in b:
            b["from"][r] = 0
    if rows:
        for s in range(S):
            if not 0 <= s32(b0["row_of"][s]) < n:
                b["out"][s] = 0
    return b


def ref_move(b, spans, S, n_rows, paced=False):
    b0, b = b, _copy(b)
    for d in range(n_rows):
        src = s32(b0["from"][d]) - 1
        if not 0 <= src < S or src == d:
            continue
        for s in spans:
            b[s][d] = b0[s][src]
        b["active"][d] = b0["active"][src]
        b["cmd"][1, d] = b0["cmd"][1, src]
        if paced:
            b["pos"][d] = b0["pos"][src]
    return b


def ref_capture(b, S, n_chunks, paced=False):
    b0, b = b, _copy(b)
    for s in range(S):
        cmd, gen, k = int(b0["ecmd"][s]), int(b0["estate"][0, s]), int(b0["estate"][1, s])
        held = paced and b0["hold"][s] != 0
        if cmd & CANCEL:
            gen = 0
        if cmd & ARM:
            gen, k = ((cmd >> GEN_SHIFT) & GEN_MASK) or 1, 0
        done = 0
        if gen and not held:
            rec = b0["chunk_in"][s].reshape(2, 192)[:, :HOP]
            if nonfinite(rec):
                done = gen | EFAULT
            else:
                b["enroll"][s].reshape(2, n_chunks, HOP)[:, k] = rec
                k += 1
                if k == n_chunks:
                    done = gen
        if done or not gen:
            gen = k = 0
        if cmd:
            b["ecmd"][s] = 0
        b["estate"][0, s], b["estate"][1, s] = gen, k
        if done:
            b["edone"][s] = done
    return b


def ref_ring_advance_rows(b, modulo, n_rows):
    b = _copy(b)
    for r in range(n_rows):
        w = s32(b["write_pos"][r])
        if w >= 0:
            b["pos"][r] = (w + 1) % modulo
    return b


class Layout:
    """The snapshot layout of one geometry, in words.  Flat span f is b[flat[f]] [S][words]; ring g is b[rings[g]]
    [S][heads][ring_rows][row words]; the embedding has `embed_w` words."""

    def __init__(self, flat, flat_w, rings, ring_w, heads, ring_rows, window, embed_w):
        self.flat, self.flat_w, self.rings, self.ring_w = list(flat), list(flat_w), list(rings), list(ring_w)
        self.heads, self.ring_rows, self.window, self.embed_w = heads, ring_rows, window, embed_w
        self.words_at = HEADER_W
        self.embed_at = HEADER_W + 4
        at = self.embed_at + embed_w
        self.flat_at, self.ring_at = [], []
        for w in self.flat_w:
            self.flat_at.append(at)
            at += w
        for w in self.ring_w:
            self.ring_at.append(at)
            at += heads * window * w
        self.total = at

    def header(self) -> np.ndarray:
        h = np.zeros(HEADER_W, dtype=U32)
        h[:8] = [MAGIC, VERSION, self.total * 4, len(self.flat), len(self.rings), self.heads, self.window, self.embed_w * 4]
        sizes = [4 * w for w in self.flat_w + self.ring_w]
        h[8:8 + len(sizes)] = sizes
        return h


def ref_save(b, L: Layout, row, index, embed_row, pos_word):
    """b["snaps"][index] = the snapshot of row `row`; pos_word the value of the position word the call reads."""
    b = _copy(b)
    snap = b["snaps"][index]
    snap[:HEADER_W] = L.header()
    snap[L.words_at:L.words_at + 4] = [b["active"][row], b["cmd"][1, row], s32(pos_word) % L.window, 0]
    snap[L.embed_at:L.embed_at + L.embed_w] = b["embed"][embed_row]
    for name, w, at in zip(L.flat, L.flat_w, L.flat_at):
        snap[at:at + w] = b[name][row]
    for name, w, at in zip(L.rings, L.ring_w, L.ring_at):
        snap[at:at + L.heads * L.window * w] = b[name][row][:, :L.window].reshape(-1)
    return b


def ref_restore(b, L: Layout, row, index, embed_row, fault_at, gen, pos_row=None, shared=False):
    """Row `row` from b["snaps"][index].  pos_row: the index of the row's own position word in b["pos"], or `shared`: the
    rings are rotated to the counter b["pos_shared"][0]."""
    b = _copy(b)
    snap = b["snaps"][index]
    was_active, was_cmd, saved = (int(v) for v in snap[L.words_at:L.words_at + 3])
    saved = s32(saved) % L.window
    delta = (s32(b["pos_shared"][0]) - saved) % L.window if shared else 0
    b["embed"][embed_row] = snap[L.embed_at:L.embed_at + L.embed_w]
    for name, w, at in zip(L.flat, L.flat_w, L.flat_at):
        b[name][row] = snap[at:at + w]
    for name, w, at in zip(L.rings, L.ring_w, L.ring_at):
        dense = snap[at:at + L.heads * L.window * w].reshape(L.heads, L.window, w)
        for j in range(L.window):
            b[name][row][:, (j + delta) % L.window] = dense[:, j]
    b["cmd"][1, row] = was_cmd
    if pos_row is not None:
        b["pos"][pos_row] = saved
    if was_active == 0:
        b["cmd"][0, row] = CLOSE | RESET
        b["fault"][fault_at] = gen
    return b


def item_ok(it, S):
    row, slot, gen, index = (s32(v) for v in it)
    return 0 <= row < S and 0 <= slot < S and index >= 0


def ref_save_rows(b, L, S, shared=False):
    for it in b["items"]:
        if item_ok(it, S):
            row, slot, index = s32(it[0]), s32(it[1]), s32(it[3])
            b = ref_save(b, L, row, index, slot, b["pos_shared"][0] if shared else b["pos"][row])
    return b


def ref_restore_rows(b, L, S, shared=False):
    for it in b["items"]:
        if item_ok(it, S):
            row, slot, index = s32(it[0]), s32(it[1]), s32(it[3])
            b = ref_restore(b, L, row, index, slot, slot, int(it[2]), None if shared else row, shared)
    return b


# ---- the runner ----------------------------------------------------------------------------------------------------------------
class Dev:
    """The buffers of one case on `device`, each inside a guard region; name -> Guarded of fp32 viewed as words."""

    def __init__(self, lib, device, bufs):
        self.lib, self.dev = lib, torch.device(device)
        self.g, self.keep = {}, []
        for name, a in bufs.items():
            self.g[name] = self._guarded(name, a)
            self.set(name, a)

    def _guarded(self, name, a):
        g = Guarded(a.shape, torch.float32, "cpu" if name in PINNED else self.dev)
        if name in PINNED and self.dev.type == "cuda":
            g.buf = g.buf.pin_memory()
            g.ibuf = g.buf.view(g.itype)
            g.t = g.buf[GUARD:GUARD + g.n].view(a.shape)
        return g

    def set(self, name, a):
        self.g[name].t.view(torch.int32).copy_(torch.from_numpy(np.ascontiguousarray(a).view(I32)))

    def get(self, name) -> np.ndarray:
        return self.g[name].t.view(torch.int32).cpu().numpy().view(U32)

    def p(self, name, word=0):
        return ctypes.c_void_p(self.g[name].t.data_ptr() + 4 * word)

    def table(self, names, row_bytes=None):
        """lh_span_t[len(names)] of the named buffers: `bytes` is one row's (dim 0) size, or row_bytes[i]."""
        t = (Span * max(len(names), 1))()
        for i, n in enumerate(names):
            a = self.g[n].t
            t[i] = Span(a.data_ptr(), row_bytes[i] if row_bytes else 4 * a[0].numel())
        self.keep.append(t)
        return ctypes.c_void_p(ctypes.addressof(t))

    def stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream if self.dev.type == "cuda" else None

    def call(self, name, args):
        if self.dev.type == "cuda":
            with torch.cuda.device(self.dev):
                return self.lib.raw(name)(*args, self.stream())
        return self.lib.raw(name)(*args, None)

    def sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    def compare(self, want, label):
        self.sync()
        for name, g in self.g.items():
            got = self.get(name)
            if not np.array_equal(got, want[name]):
                at = np.argwhere(got != want[name])
                raise AssertionError(f"{label}: {name} differs in {len(at)} words, first at {at[0].tolist()}: "
                                     f"got {got[tuple(at[0])]:#x}, restated {want[name][tuple(at[0])]:#x}")
            g.check(f"{label}: {name}")


def check(lib, device, entry, bufs, make_args, want, label, unwritten=()):
    """One call of `entry` on `bufs`; every buffer afterwards equals `want`, every guard holds, and the buffers the header
    says are not written equal their copy from before the call."""
    print(label)
    before = _copy(bufs)
    d = Dev(lib, device, bufs)
    rc = d.call(entry, make_args(d))
    assert rc == 0, f"{label}: {entry} returned {rc}"
    d.compare(want, label)
    for name in unwritten:
        assert np.array_equal(d.get(name), before[name]), f"{label}: {name} was written"
    return d


# ---- argument lists, in the order of the header -------------------------------------------------------------------------------
def begin_entry(rows, paced):
    return "lh_session_begin" + ("_rows" if rows else "") + ("_paced" if paced else "")


def end_entry(rows, paced):
    return "lh_session_end" + ("_rows" if rows else "") + ("_paced" if paced else "")


def begin_args(d, spans, S, n_rows, rows, paced):
    a = [d.table(spans), len(spans), d.p("chunk_in"), d.p("chunk"), d.p("cmd"), d.p("active")]
    if rows:
        a.append(d.p("slot_of"))
    if paced:
        a += [d.p("hold"), d.p("pos"), d.p("write_pos")]
    return a + ([n_rows, S] if rows else [S])


def end_args(d, spans, S, n_rows, rows, paced, carry=(), with_from=True):
    a = [d.table(spans), len(spans)]
    if paced:
        a += [d.table(carry), len(carry) // 2]
    a.append(d.p("chunk_in"))
    if rows:
        a.append(d.p("out_rows"))
    a += [d.p("out"), d.p("cmd"), d.p("active"), d.p("fault")]
    if paced:
        a.append(d.p("hold"))
    if rows:
        a += [d.p("slot_of"), d.p("row_of"), d.p("from") if with_from else None, n_rows]
    return a + [S]


def move_args(d, spans, S, n_rows, paced):
    a = [d.table(spans), len(spans), d.p("from"), d.p("cmd"), d.p("active")]
    if paced:
        a.append(d.p("pos"))
    return a + [n_rows, S]


def capture_args(d, S, n_chunks, paced):
    a = [d.p("chunk_in"), d.p("enroll"), d.p("ecmd"), d.p("estate"), d.p("edone")]
    if paced:
        a.append(d.p("hold"))
    return a + [n_chunks, S]


def snap_geometry(d, L: Layout):
    return [d.table(L.flat), len(L.flat), d.table(L.rings, [4 * w for w in L.ring_w]), len(L.rings), L.heads, L.ring_rows,
            L.window]


def save_args(d, L, S, row, index, embed_row, pos):
    """pos: (buffer name, word) of the position word the call reads."""
    stride = d.g["snaps"].t.shape[1]
    return snap_geometry(d, L) + [d.p("embed", embed_row * L.embed_w), 4 * L.embed_w, d.p("snaps", index * stride),
                                  ctypes.c_ulonglong(4 * stride), d.p("cmd"), d.p("active"), d.p(*pos), row, S]


def restore_args(d, L, S, row, index, embed_row, fault_at, gen, pos_row=None, shared=False):
    stride = d.g["snaps"].t.shape[1]
    return snap_geometry(d, L) + [d.p("embed", embed_row * L.embed_w), 4 * L.embed_w, d.p("snaps", index * stride),
                                  ctypes.c_ulonglong(4 * stride), d.p("cmd"), None if shared else d.p("pos", pos_row),
                                  d.p("pos_shared") if shared else None, d.p("fault", fault_at), gen, row, S]


def save_rows_args(d, L, S, n_items, shared):
    stride = d.g["snaps"].t.shape[1]
    return snap_geometry(d, L) + [d.p("embed"), 4 * L.embed_w, d.p("snaps"), ctypes.c_ulonglong(4 * stride), d.p("cmd"),
                                  d.p("active"), None if shared else d.p("pos"), d.p("pos_shared") if shared else None,
                                  d.p("items"), n_items, S]


def restore_rows_args(d, L, S, n_items, shared):
    stride = d.g["snaps"].t.shape[1]
    return snap_geometry(d, L) + [d.p("embed"), 4 * L.embed_w, d.p("snaps"), ctypes.c_ulonglong(4 * stride), d.p("cmd"),
                                  None if shared else d.p("pos"), d.p("pos_shared") if shared else None, d.p("fault"),
                                  d.p("items"), n_items, S]


# ---- the cases -----------------------------------------------------------------------------------------------------------------
ROW_COUNTS = (1, 3, 16, 17, 33, 63, 64, 65)            # the three branches of the tile count and their borders
ROWS_OF_S = ((1, 1), (1, 3), (3, 16), (16, 17), (17, 33), (33, 63), (63, 64), (64, 65), (65, 65))      # (n_rows, S)
COPY_SIZES = (1, 3, 15, 17, 255, 256, 257, 1023, 1025, 4097)       # float4 per row: begin / move / save / restore
END_SIZES = (1, 2047, 2048, 2049, 4095, 4096, 4097, 6145)          # ... end and its carry pairs
COPY_TABLES = ((4097,), (1, 1025), (3, 15, 17, 255, 256, 257, 1023, 1), tuple(COPY_SIZES[i % 10] for i in range(32)))
END_TABLES = ((6145,), END_SIZES, (2047, 4097), (2049,), (4096, 1), (2048,), (4095,), (6145, 1, 2049))

HOSTS = ("0", "reset", "open", "close", "close_reset")
INPUTS = ("finite", "nan", "inf_lookahead", "inf_last")
OPEN_GENS = (1, GEN_MASK, 0, 5)                        # an OPEN whose generation field is 0 opens generation 1
ACTIVE_GENS = (7, GEN_MASK, 1)


def word_table(paced):
    """Every combination host word x device word x active x input (x hold): 80, or 160."""
    return list(itertools.product(HOSTS, (0, RESET), (0, 1), INPUTS, (0, 1) if paced else (0,)))


def host_word(kind, i):
    return {"0": 0, "reset": RESET, "open": OPEN | RESET | (OPEN_GENS[i % 4] << GEN_SHIFT), "close": CLOSE,
            "close_reset": CLOSE | RESET}[kind]


def input_row(cnt, kind):
    x = cnt.take(IN_W)
    if kind == "nan":
        x[77] = NAN
    elif kind == "inf_lookahead":
        x[150] = INF                                   # channel 0, sample 150: one of the 64 look-ahead samples
    elif kind == "inf_last":
        x[IN_W - 1] = NINF                             # channel 1, sample 191
    return x


def slot_tables(n_rows, S):
    """slot_of: a permutation of the slots that is not the identity, with -1 in row 1 and S + 3 in row 2 where those rows
    exist; row_of: its inverse over the rows launched, -1 elsewhere and (one slot) a row beyond those launched."""
    slot_of = np.array([(S - 1 - r + S // 2) % S for r in range(S)], dtype=I32)
    if S > 1 and (slot_of == np.arange(S)).all():
        slot_of = np.roll(slot_of, 1)
    if S > 3:
        slot_of[1], slot_of[2] = -1, S + 3
    row_of = np.full(S, -1, dtype=I32)
    for r in range(n_rows):
        if 0 <= slot_of[r] < S:
            row_of[slot_of[r]] = r
    free = [s for s in range(S) if row_of[s] < 0]
    if free and n_rows < S:
        row_of[free[-1]] = n_rows
    return slot_of.view(U32), row_of.view(U32)


def session_bufs(S, sizes, rows, paced, first=0, n_rows=None, prefix="span", cnt=None, combos=None, slots=None):
    """Buffers of a begin / end / move call on S slots with one span of sizes[i] float4 per row each, the word table spread
    over the rows from combination `first` on.  -> (bufs, span names, counter)."""
    cnt = cnt or Counter()
    b = {}
    spans = [f"{prefix}{i}" for i in range(len(sizes))]
    for name, n16 in zip(spans, sizes):
        b[name] = cnt.take(S, 4 * n16)
    table = combos or word_table(paced)
    b["chunk_in"] = np.zeros((S, IN_W), dtype=U32)
    b["cmd"], b["active"] = np.zeros((2, S), dtype=U32), np.zeros(S, dtype=U32)
    if paced:
        b["hold"] = np.zeros(S, dtype=U32)
        b["pos"] = (np.arange(S, dtype=U32) * 7 + 3) % 50
        b["write_pos"] = np.full(S, 0x77, dtype=U32)
    if rows:
        b["slot_of"], b["row_of"] = slots or slot_tables(n_rows, S)
    for r in range(S):
        host, dev, act, inp, hold = table[(first + r) % len(table)]
        slot, owned = _row(b, r, S, rows)
        b["cmd"][0, r], b["cmd"][1, r] = host_word(host, first + r), dev
        b["active"][r] = ACTIVE_GENS[(first + r) % 3] if act else 0
        if owned:
            b["chunk_in"][slot] = input_row(cnt, inp)
            if paced:
                b["hold"][slot] = hold
    for s in range(S):                                 # the slots no row owns: finite rows nobody may read into a verdict
        if not b["chunk_in"][s].any():
            b["chunk_in"][s] = cnt.take(IN_W)
    return b, spans, cnt


def run_begin(lib, device, S, sizes, rows=False, paced=False, n_rows=None, first=0):
    n_rows = n_rows or S
    b, spans, cnt = session_bufs(S, sizes, rows, paced, first, n_rows)
    b["chunk"] = cnt.take(S, IN_W)
    want = ref_begin(b, spans, S, n_rows, rows, paced)
    check(lib, device, begin_entry(rows, paced), b, lambda d: begin_args(d, spans, S, n_rows, rows, paced), want,
          f"begin rows={rows} paced={paced} n_rows={n_rows} S={S} spans={sizes} first={first}",
          unwritten=["chunk_in", "cmd", "active"] + [k for k in ("slot_of", "row_of", "hold", "pos") if k in b])
    return b, want


def end_bufs(S, sizes, rows, paced, n_rows, first=0, carry_sizes=None, combos=None, slots=None):
    b, spans, cnt = session_bufs(S, sizes, rows, paced, first, n_rows, combos=combos, slots=slots)
    b["out"] = cnt.take(S, OUT_W)
    b["fault"] = np.arange(100, 100 + S, dtype=U32)
    carry = []
    if rows:
        b["out_rows"] = cnt.take(S, OUT_W)
        b["from"] = np.arange(1, S + 1, dtype=U32)[::-1].copy()
    if paced:
        for i, n16 in enumerate(carry_sizes if carry_sizes is not None else sizes):
            b[f"read{i}"], b[f"wrote{i}"] = cnt.take(S, 4 * n16), cnt.take(S, 4 * n16)
            carry += [f"read{i}", f"wrote{i}"]
    return b, spans, carry


def run_end(lib, device, S, sizes, rows=False, paced=False, n_rows=None, first=0, plant=None, alias=False, with_from=True,
            combos=None, label=""):
    """plant: [(buffer, row, word, value)] written into the buffers before the call.  alias: the first scanned span IS the
    first written tensor of the carry table, as (h, c) are in a streamer."""
    n_rows = n_rows or S
    b, spans, carry = end_bufs(S, sizes, rows, paced, n_rows, first, combos=combos)
    if alias and paced:
        del b["wrote0"]
        carry[1] = spans[0]
    if not with_from:
        b.pop("from", None)
    for name, r, w, v in plant or ():
        b[name][r, w] = v
    want = ref_end(b, spans, S, n_rows, rows, paced, carry)
    ro = ["chunk_in"] + [k for k in ("out_rows", "slot_of", "row_of", "hold") if k in b] + carry[::2]
    ro += [s for s in spans if s not in carry]
    check(lib, device, end_entry(rows, paced), b, lambda d: end_args(d, spans, S, n_rows, rows, paced, carry, with_from), want,
          f"end rows={rows} paced={paced} n_rows={n_rows} S={S} spans={sizes} first={first} {label}", unwritten=ro)
    return b, want


def run_move(lib, device, S, n_rows, sizes, paced=False, first=0):
    """Disjoint pairs: the destinations are even rows below n_rows, the sources odd rows or rows at and above n_rows; and
    the entries that move nothing: 0, d + 1, a negative one, S + 1 and beyond."""
    b, spans, cnt = session_bufs(S, sizes, False, paced, first)
    frm = np.zeros(S, dtype=I32)
    sources = [r for r in range(S - 1, -1, -1) if r >= n_rows or r % 2 == 1]
    nothing = itertools.cycle((0, None, -3, S + 1, S + 40))
    for d in range(S):
        if d % 2 == 0 and d % 3 != 2 and sources and sources[0] > d:
            frm[d] = sources.pop(0) + 1
        else:
            v = next(nothing)
            frm[d] = d + 1 if v is None else v
    frm[n_rows:] = np.arange(S - n_rows) + 1           # entries at and beyond n_rows are not read: they would move rows
    b["from"] = frm.view(U32)
    want = ref_move(b, spans, S, n_rows, paced)
    assert n_rows < 2 or S < 2 or any(not np.array_equal(want[s], b[s]) for s in spans)
    check(lib, device, "lh_session_move" + ("_paced" if paced else ""), b, lambda d: move_args(d, spans, S, n_rows, paced),
          want, f"move paced={paced} n_rows={n_rows} S={S} spans={sizes} from={frm.tolist()[:8]}..", unwritten=["from", "chunk_in"])
    assert np.array_equal(want["cmd"][0], b["cmd"][0])            # the host's word does not travel
    return b, want


# capture: what each slot does, by s % 8, over CAPTURE_STEPS chunks of a stream
def capture_script(s, j, n_chunks):
    """-> (ecmd word posted ahead of chunk j, hold, kind of input row)."""
    gen = (1, GEN_MASK, 9, 300)[s % 4]
    role = s % 8
    arm = ARM | (gen << GEN_SHIFT)
    if role == 0:                                      # armed at chunk 0, runs to the done word
        return (arm if j == 0 else 0), 0, "finite"
    if role == 1:                                      # armed again in mid-capture (n_chunks > 1) under another generation
        return (arm if j == 0 else ARM | ((gen ^ 6) << GEN_SHIFT) if j == 1 else 0), 0, "finite"
    if role == 2:                                      # cancelled after one chunk
        return (arm if j == 0 else CANCEL if j == 1 else 0), 0, "finite"
    if role == 3:                                      # a fault in a recorded sample of chunk 1
        return (arm if j == 0 else 0), 0, ("bad_recorded" if j == 1 else "finite")
    if role == 4:                                      # a fault in the look-ahead of chunk 0 only: not judged
        return (arm if j == 0 else 0), 0, ("inf_lookahead" if j == 0 else "finite")
    if role == 5:                                      # held at chunk 1 (paced), with a NaN row nobody may look at
        return (arm if j == 0 else 0), (1 if j == 1 else 0), ("nan" if j == 1 else "finite")
    if role == 6:                                      # never armed; a non-finite row
        return 0, 0, "nan"
    return (arm if j == 2 else 0), 0, "finite"         # armed late


CAPTURE_STEPS = 5


def run_capture(lib, device, S, n_chunks, paced=False):
    cnt = Counter()
    b = {"chunk_in": np.zeros((S, IN_W), dtype=U32), "enroll": cnt.take(S, 2 * HOP * n_chunks), "ecmd": np.zeros(S, dtype=U32),
         "estate": np.zeros((2, S), dtype=U32), "edone": np.zeros(S, dtype=U32)}
    if paced:
        b["hold"] = np.zeros(S, dtype=U32)
    d = Dev(lib, device, b)
    args = capture_args(d, S, n_chunks, paced)
    done_seen = set()
    for j in range(CAPTURE_STEPS):
        for s in range(S):
            word, hold, kind = capture_script(s, j, n_chunks)
            x = input_row(cnt, kind if kind != "bad_recorded" else "finite")
            if kind == "bad_recorded":
                x[192 + 127] = INF                     # channel 1, sample 127: the last recorded sample
            b["chunk_in"][s] = x
            if word:
                b["ecmd"][s] = word
            if paced:
                b["hold"][s] = hold
        for k in ("chunk_in", "ecmd") + (("hold",) if paced else ()):
            d.set(k, b[k])
        before = b["chunk_in"].copy()
        want = ref_capture(b, S, n_chunks, paced)
        label = f"capture paced={paced} S={S} n_chunks={n_chunks} chunk {j}"
        print(label)
        assert d.call("lh_session_capture" + ("_paced" if paced else ""), args) == 0
        d.compare(want, label)
        assert np.array_equal(d.get("chunk_in"), before)
        done_seen |= {s for s in range(S) if want["edone"][s] != b["edone"][s]}
        b = want
    assert 0 in done_seen                              # slot 0 completed its clip
    return b


def snapshot_bufs(S, L: Layout, n_snaps, stride_w, cnt=None, pos=None, shared_pos=0):
    cnt = cnt or Counter()
    b = {}
    for name, w in zip(L.flat, L.flat_w):
        b[name] = cnt.take(S, w)
    for name, w in zip(L.rings, L.ring_w):
        b[name] = cnt.take(S, L.heads, L.ring_rows, w)
    b["embed"] = cnt.take(S, L.embed_w)
    b["snaps"] = cnt.take(n_snaps, stride_w)
    b["cmd"], b["active"] = cnt.take(2, S), cnt.take(S)
    b["pos"] = np.array(pos if pos is not None else [(17 * r) % L.window for r in range(S)], dtype=I32).view(U32)
    b["pos_shared"] = np.array([shared_pos], dtype=I32).view(U32)
    b["fault"] = np.arange(100, 100 + S, dtype=U32)
    return b, cnt


def make_layout(n_flat, flat_sizes, n_rings, ring_bytes, heads, window, ring_rows=50, embed_w=256):
    """flat span f has flat_sizes[f % len] float4 per row, ring g rows of ring_bytes[g % len] bytes."""
    return Layout([f"flat{i}" for i in range(n_flat)], [4 * flat_sizes[i % len(flat_sizes)] for i in range(n_flat)],
                  [f"ring{i}" for i in range(n_rings)], [ring_bytes[i % len(ring_bytes)] // 4 for i in range(n_rings)],
                  heads, ring_rows, window, embed_w)


def run_save_restore(lib, device, L: Layout, S=3, row=1, to_row=2, saved_pos=17, delta=None, dead=False, pad_w=8):
    """`lh_session_save` of row `row` (position saved_pos), then `lh_session_restore` into row `to_row` of OTHER buffers:
    delta None -> a paced target (pos_row), else a lock-step one whose shared counter gives that delta."""
    stride = L.total + pad_w
    pos = [0] * S
    pos[row] = saved_pos
    b, cnt = snapshot_bufs(S, L, 1, stride, pos=pos)
    if dead:
        b["active"][row] = 0
    ro = [k for k in b if k != "snaps"]
    before_pad = b["snaps"][0, L.total:].copy()
    want = ref_save(b, L, row, 0, row, b["pos"][row])
    label = (f"flat={len(L.flat)}x{[w // 4 for w in L.flat_w[:4]]} rings={len(L.rings)}x{[4 * w for w in L.ring_w[:3]]} "
             f"heads={L.heads} window={L.window} pos={saved_pos} delta={delta} dead={dead}")
    check(lib, device, "lh_session_save", b, lambda d: save_args(d, L, S, row, 0, row, ("pos", row)), want, "save " + label,
          unwritten=ro)
    snap = want["snaps"]
    assert np.array_equal(snap[0, L.total:], before_pad)                    # the padding behind the layout
    assert np.array_equal(snap[0, :HEADER_W], L.header()) and snap[0, 2] == 4 * L.total
    # the target: other buffers with other contents, the snapshot carried over
    shared = delta is not None
    t, _ = snapshot_bufs(S, L, 1, stride, cnt=cnt, shared_pos=((saved_pos % L.window) + (delta or 0)) % L.window + 3 * L.window)
    t["snaps"] = snap.copy()
    gen = 0x123456
    want_t = ref_restore(t, L, to_row, 0, to_row, to_row, gen, None if shared else to_row, shared)
    check(lib, device, "lh_session_restore", t,
          lambda d: restore_args(d, L, S, to_row, 0, to_row, to_row, gen, None if shared else to_row, shared), want_t,
          "restore " + label, unwritten=["snaps", "active", "pos_shared"] + (["pos"] if shared else []))
    # the row is reproduced: flat slices byte for byte, ring rows where they were or rotated by delta
    for name in L.flat:
        assert np.array_equal(want_t[name][to_row], b[name][row])
    for name in L.rings:
        for j in range(L.window):
            assert np.array_equal(want_t[name][to_row][:, (j + (delta or 0)) % L.window], b[name][row][:, j])
        assert np.array_equal(want_t[name][to_row][:, L.window:], t[name][to_row][:, L.window:])
    assert np.array_equal(want_t["embed"][to_row], b["embed"][row])
    if dead:
        assert want_t["cmd"][0, to_row] == (CLOSE | RESET) and want_t["fault"][to_row] == gen
    else:
        assert want_t["cmd"][0, to_row] == t["cmd"][0, to_row] and want_t["fault"][to_row] == t["fault"][to_row]
    return want, want_t


def run_snapshot_rows(lib, device, L: Layout, S, n_items, shared=False, with_bad=True):
    """`lh_session_save_rows` over n_items items equals the restatement — the single form per item — and the single form
    itself on the first item; then `lh_session_restore_rows` of the same snapshots into other buffers, rows permuted."""
    stride = L.total + 12
    rows = [(3 * i + 1) % S for i in range(n_items)] if S % 3 else list(range(n_items))
    assert len(set(rows)) == n_items
    items = np.array([(rows[i], (rows[i] + 1) % S, 40 + i, n_items - 1 - i) for i in range(n_items)], dtype=I32)
    if with_bad and n_items >= 3:                      # skipped whole: a row outside [0, S), a negative index
        items[1, 0] = S
        items[2, 3] = -1
    b, cnt = snapshot_bufs(S, L, n_items, stride, shared_pos=L.window + 5)
    b["items"] = items.view(U32)
    b["active"][rows[0]] = 0                           # the first item is a dead snapshot
    label = f"rows n_items={n_items} S={S} shared={shared} window={L.window} heads={L.heads}"
    want = ref_save_rows(b, L, S, shared)
    check(lib, device, "lh_session_save_rows", b, lambda d: save_rows_args(d, L, S, n_items, shared), want, "save_" + label,
          unwritten=[k for k in b if k != "snaps"])
    it = items[0]
    one = ref_save(b, L, int(it[0]), int(it[3]), int(it[1]), b["pos_shared"][0] if shared else b["pos"][it[0]])
    check(lib, device, "lh_session_save", b,
          lambda d: save_args(d, L, S, int(it[0]), int(it[3]), int(it[1]), ("pos_shared", 0) if shared else ("pos", int(it[0]))),
          one, "save, item 0 alone, " + label)
    assert np.array_equal(one["snaps"][it[3]], want["snaps"][it[3]])
    t, _ = snapshot_bufs(S, L, n_items, stride, cnt=cnt, shared_pos=2 * L.window + 11)
    t["snaps"] = want["snaps"].copy()
    back = items.copy()
    back[:, 0] = S - 1 - back[:, 0]                    # every listener comes back in another row (the middle one excepted)
    if with_bad and n_items >= 3:
        back[1, 0], back[2, 3] = -2, -7
    assert len(set(back[:, 0].tolist())) == n_items
    t["items"] = back.view(U32)
    want_t = ref_restore_rows(t, L, S, shared)
    check(lib, device, "lh_session_restore_rows", t, lambda d: restore_rows_args(d, L, S, n_items, shared), want_t,
          "restore_" + label, unwritten=["snaps", "items", "active", "pos_shared"] + (["pos"] if shared else []))
    assert want_t["fault"][back[0, 1]] == 40 and want_t["cmd"][0, back[0, 0]] == (CLOSE | RESET)
    return want, want_t


def run_ring_advance(lib, device, n_rows, modulo=50, extra=3):
    S = n_rows + extra
    wp = np.array([(-1, 0, modulo - 1, 17, -5, modulo)[r % 6] for r in range(S)], dtype=I32)
    b = {"pos": (np.arange(S, dtype=U32) * 11 + 2) % modulo, "write_pos": wp.view(U32)}
    want = ref_ring_advance_rows(b, modulo, n_rows)
    assert np.array_equal(want["pos"][n_rows:], b["pos"][n_rows:])
    check(lib, device, "lh_ring_advance_rows", b, lambda d: [d.p("pos"), d.p("write_pos"), modulo, n_rows], want,
          f"ring_advance_rows n_rows={n_rows} modulo={modulo}", unwritten=["write_pos"])


# ---- non-finite probes for the end kernels -------------------------------------------------------------------------------------
PROBE_N16 = 2055                                       # float4 of a probed span: 0, 2047, 2048, 2049 and n16 - 1 are five places
PROBE_TABLES = ((PROBE_N16,), (PROBE_N16, PROBE_N16), (PROBE_N16, 1, 7, 300, 2048, 3, 64, PROBE_N16))
PROBE_AT = (0, 2047, 2048, 2049, PROBE_N16 - 1)
PROBE_VALUES = (INF, NAN, NINF, 0x7F800001)            # the last one a signalling NaN


def probe_list(tables=PROBE_TABLES, at=PROBE_AT):
    """(table, buffer or None = the output row, float4 index) of every probe."""
    out = []
    for sizes in tables:
        for span in sorted({0, len(sizes) - 1}):
            out += [(sizes, span, j) for j in at]
        out.append((sizes, None, 63))
    out.append((tables[0], None, 0))
    return out


def run_end_probe(lib, device, rows, paced, sizes, span, j4, k):
    """Five rows: 0 and 1 live, 2 idle, 3 held (PACED; else idle), 4 unowned (ROWS; else idle).  Probe k plants one value in
    component k % 4 of float4 j4 (span None: of the output row): in row 0 (closes it, row 1 goes on), in row 1 (the other way
    round), and in rows 2, 3 and 4 at once (no word, fault or output row differs from the launch without the plant)."""
    S = n_rows = 5
    combos = [("0", 0, 1, "finite", 0)] * 2 + [("0", 0, 0, "finite", 0), ("0", 0, 1 if paced else 0, "finite", 1 if paced else 0),
                                               ("0", 0, 1 if rows else 0, "finite", 0)]
    slots = (np.array([2, 0, 4, 1, -1], dtype=I32).view(U32), np.array([1, 3, 0, -1, 2], dtype=I32).view(U32)) if rows else None
    slot = [2, 0] if rows else [0, 1]
    value, comp = PROBE_VALUES[k % 4], k % 4
    name = ("out_rows" if rows else "out") if span is None else f"span{span}"

    def launch(planted_rows, tag, run=True):
        b, spans, carry = end_bufs(S, sizes, rows, paced, n_rows, combos=combos, slots=slots)
        for r in planted_rows:
            b[name][r, 4 * j4 + comp] = value
        want = ref_end(b, spans, S, n_rows, rows, paced, carry)
        if run:
            check(lib, device, end_entry(rows, paced), b, lambda d: end_args(d, spans, S, n_rows, rows, paced, carry), want,
                  f"end probe rows={rows} paced={paced} spans={sizes} {name}[{tag}] float4 {j4}.{comp} = {value:#x}")
        return want
    clean = launch([], "", run=False)                  # the restatement alone
    gens = [int(clean["active"][0]), int(clean["active"][1])]
    assert gens[0] and gens[1] and not clean["cmd"].any() and clean["out"][slot[0]].any() and clean["out"][slot[1]].any()
    for me, other in ((0, 1), (1, 0)):
        w = launch([me], f"row {me}")
        assert w["active"][me] == 0 and w["cmd"][1, me] == RESET and w["fault"][slot[me]] == gens[me] and not w["out"][slot[me]].any()
        assert w["active"][other] == gens[other] and w["cmd"][1, other] == 0 and w["fault"][slot[other]] == clean["fault"][slot[other]]
        assert np.array_equal(w["out"][slot[other]], clean["out"][slot[other]])
    w = launch([2, 3, 4], "rows 2, 3, 4")
    for key in ("cmd", "active", "fault", "out"):
        assert np.array_equal(w[key], clean[key]), key


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def sub(args, i, v):
    return args[:i] + [v] + args[i + 1:]


def bad_tables(d, ok, i, name):
    """The table at argument i with one entry spoiled: a null base, an unaligned one, no bytes, bytes not a multiple of 16."""
    a = d.g[name].t
    good = Span(a.data_ptr(), 4 * a[0].numel())
    out = []
    for what, bad in (("null base", Span(None, good.bytes)), ("unaligned base", Span(good.base + 4, good.bytes)),
                      ("no bytes", Span(good.base, 0)), ("bytes % 16", Span(good.base, good.bytes + 8))):
        t = (Span * 2)(good, bad)
        d.keep.append(t)
        out.append((f"table {i}: {what}", sub(sub(ok, i, ctypes.c_void_p(ctypes.addressof(t))), i + 1, 2)))
    return out


def run_refusals(lib, device, entry, bufs, make_args, extra=None, optional=()):
    """Every pointer null, every count -1, every byte count 0, and what `extra(d, ok)` adds: LH_ERR_ARG each, and afterwards
    every buffer holds what it held and every guard its pattern; the unspoiled call then succeeds."""
    d = Dev(lib, device, bufs)
    ok = make_args(d)
    bad = []
    for i, a in enumerate(ok):
        if isinstance(a, ctypes.c_void_p) and i not in optional:
            bad.append((f"argument {i} null", sub(ok, i, None)))
        elif isinstance(a, int):
            bad.append((f"argument {i} = -1", sub(ok, i, -1)))
        elif isinstance(a, ctypes.c_ulonglong):
            bad.append((f"argument {i} = 0", sub(ok, i, ctypes.c_ulonglong(0))))
    bad += extra(d, ok) if extra else []
    for what, a in bad:
        assert d.call(entry, a) == ERR_ARG, f"{entry}: {what} was not refused"
    d.compare(bufs, f"{entry} after {len(bad)} refusals")
    assert d.call(entry, ok) == 0, entry
    d.sync()
    print(entry, "refused", len(bad))
    return len(bad)


def refusal_cases(lib, device):
    """Every entry point of the file with the header's LH_ERR_ARG list."""
    S, n = 4, 3
    total = 0
    for rows, paced in itertools.product((False, True), repeat=2):
        b, spans, cnt = session_bufs(S, (3, 5), rows, paced, 0, n)
        b["chunk"] = cnt.take(S, IN_W)

        def more(d, ok, rows=rows, paced=paced):
            e = bad_tables(d, ok, 0, "span0") + [("n_spans 0", sub(ok, 1, 0)), ("n_spans 33", sub(ok, 1, MAX_SPANS + 1)),
                                                 ("S 0", sub(ok, len(ok) - 1, 0))]
            if rows:
                e += [("n_rows 0", sub(ok, len(ok) - 2, 0)), ("n_rows S + 1", sub(ok, len(ok) - 2, S + 1))]
            if paced:
                i = 7 + rows                           # pos, then write_pos
                e.append(("pos == write_pos", sub(ok, i + 1, ok[i])))
            return e
        total += run_refusals(lib, device, begin_entry(rows, paced), b, lambda d: begin_args(d, spans, S, n, rows, paced), more)
        b, spans, carry = end_bufs(S, (3, 5), rows, paced, n)

        def more(d, ok, rows=rows, paced=paced):
            e = bad_tables(d, ok, 0, "span0") + [("n_spans 0", sub(ok, 1, 0)), ("n_spans 9", sub(ok, 1, MAX_END_SPANS + 1)),
                                                 ("S 0", sub(ok, len(ok) - 1, 0))]
            at = 4 if paced else 2                     # chunk_in
            if rows:
                e += [("n_rows 0", sub(ok, len(ok) - 2, 0)), ("n_rows S + 1", sub(ok, len(ok) - 2, S + 1)),
                      ("out_rows == out", sub(ok, at + 1, ok[at + 2]))]
            if paced:
                e += bad_tables(d, ok, 2, "read0")
                uneq = (Span * 2)(Span(d.g["read0"].t.data_ptr(), 48), Span(d.g["wrote1"].t.data_ptr(), 80))
                twice = (Span * 2)(Span(d.g["read0"].t.data_ptr(), 48), Span(d.g["read0"].t.data_ptr(), 48))
                d.keep += [uneq, twice]
                e += [("n_pairs 0", sub(ok, 3, 0)), ("n_pairs 17", sub(ok, 3, MAX_SPANS // 2 + 1)),
                      ("a pair of unequal sizes", sub(sub(ok, 2, ctypes.c_void_p(ctypes.addressof(uneq))), 3, 1)),
                      ("one tensor twice", sub(sub(ok, 2, ctypes.c_void_p(ctypes.addressof(twice))), 3, 1))]
            return e
        n_args = len(end_args(Dev(lib, device, b), spans, S, n, rows, paced, carry))
        total += run_refusals(lib, device, end_entry(rows, paced), b, lambda d: end_args(d, spans, S, n, rows, paced, carry), more,
                              optional=(n_args - 3,) if rows else ())
    for paced in (False, True):
        b, spans, cnt = session_bufs(S, (3, 5), False, paced)
        b["from"] = np.array([3, 0, 0, 0], dtype=U32)
        total += run_refusals(lib, device, "lh_session_move" + ("_paced" if paced else ""), b,
                              lambda d: move_args(d, spans, S, n, paced),
                              lambda d, ok: bad_tables(d, ok, 0, "span0") + [
                                  ("n_spans 0", sub(ok, 1, 0)), ("n_spans 33", sub(ok, 1, MAX_SPANS + 1)), ("S 0", sub(ok, len(ok) - 1, 0)),
                                  ("n_rows 0", sub(ok, len(ok) - 2, 0)), ("n_rows S + 1", sub(ok, len(ok) - 2, S + 1))])
        cnt = Counter()
        b = {"chunk_in": cnt.take(S, IN_W), "enroll": cnt.take(S, 2 * HOP * 2), "ecmd": np.full(S, ARM | (5 << GEN_SHIFT), dtype=U32),
             "estate": np.zeros((2, S), dtype=U32), "edone": np.zeros(S, dtype=U32)}
        if paced:
            b["hold"] = np.zeros(S, dtype=U32)
        total += run_refusals(lib, device, "lh_session_capture" + ("_paced" if paced else ""), b,
                              lambda d: capture_args(d, S, 2, paced),
                              lambda d, ok: [("n_chunks 0", sub(ok, len(ok) - 2, 0)), ("S 0", sub(ok, len(ok) - 1, 0)),
                                             ("chunk_in unaligned", sub(ok, 0, d.p("chunk_in", 1))),
                                             ("enroll unaligned", sub(ok, 1, d.p("enroll", 2)))])
    # snapshots: arguments 0 .. 6 the geometry, 7 embed, 8 embed_bytes, 9 snap, 10 snap bytes / stride
    L = make_layout(2, (3, 5), 2, (48, 16), 2, 7, ring_rows=9, embed_w=8)
    b, cnt = snapshot_bufs(S, L, 2, L.total + 4)
    b["items"] = np.array([(0, 1, 5, 1), (2, 0, 6, 0)], dtype=I32).view(U32)

    def geometry(d, ok, rows_form):
        e = bad_tables(d, ok, 0, "flat0") + [("n_flat 0", sub(ok, 1, 0)), ("n_flat 33", sub(ok, 1, MAX_SPANS + 1)), ("n_rings 0", sub(ok, 3, 0)),
                                             ("n_rings 9", sub(ok, 3, MAX_RINGS + 1)), ("heads 0", sub(ok, 4, 0)), ("window 0", sub(ok, 6, 0)),
                                             ("window > ring_rows", sub(ok, 6, L.ring_rows + 1)), ("embed_bytes 0", sub(ok, 8, 0)),
                                             ("embed_bytes 24", sub(ok, 8, 24)), ("embed unaligned", sub(ok, 7, d.p("embed", 1))),
                                             ("snap unaligned", sub(ok, 9, d.p("snaps", 2))),
                                             ("snapshot too small", sub(ok, 10, ctypes.c_ulonglong(4 * L.total - 16))),
                                             ("S 0", sub(ok, len(ok) - 1, 0))]
        if rows_form:
            e += [("n_items 0", sub(ok, len(ok) - 2, 0)), ("n_items S + 1", sub(ok, len(ok) - 2, S + 1)),
                  ("items misaligned", sub(ok, len(ok) - 3, ctypes.c_void_p(d.p("items").value + 2))),
                  ("stride % 16", sub(ok, 10, ctypes.c_ulonglong(4 * L.total + 8)))]
        else:
            e += [("row S", sub(ok, len(ok) - 2, S))]
        return e
    total += run_refusals(lib, device, "lh_session_save", b, lambda d: save_args(d, L, S, 1, 0, 1, ("pos", 1)),
                          lambda d, ok: geometry(d, ok, False))
    total += run_refusals(lib, device, "lh_session_restore", b, lambda d: restore_args(d, L, S, 1, 0, 1, 1, 9, 1, False),
                          lambda d, ok: geometry(d, ok, False) + [("pos_row and pos_shared", sub(ok, 13, d.p("pos_shared"))),
                                                                  ("gen 0", sub(ok, 15, 0)), ("gen 2^23", sub(ok, 15, 1 << 23))])
    for shared in (False, True):
        both = lambda d, ok, i: [("pos_rows and pos_shared", sub(sub(ok, i, d.p("pos")), i + 1, d.p("pos_shared")))]
        total += run_refusals(lib, device, "lh_session_save_rows", b, lambda d: save_rows_args(d, L, S, 2, shared),
                              lambda d, ok: geometry(d, ok, True) + both(d, ok, 13))
        total += run_refusals(lib, device, "lh_session_restore_rows", b, lambda d: restore_rows_args(d, L, S, 2, shared),
                              lambda d, ok: geometry(d, ok, True) + both(d, ok, 12))
    b = {"pos": np.arange(S, dtype=U32), "write_pos": np.arange(S, dtype=U32)}
    total += run_refusals(lib, device, "lh_ring_advance_rows", b, lambda d: [d.p("pos"), d.p("write_pos"), 50, S],
                          lambda d, ok: [("pos == write_pos", sub(ok, 1, ok[0])), ("n_rows 0", sub(ok, 3, 0)), ("modulo 0", sub(ok, 2, 0))])
    return total
