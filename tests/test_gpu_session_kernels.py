"""GPU: the session kernels of lh_stream.hip — begin, end, move, capture, save / restore in their ROWS / PACED forms, and
`lh_ring_advance_rows` — called directly through the C ABI on hand-made device buffers and held, word for word, to the integer
restatement of include/lookonce_hip.h in tests/session_kernel_cases.py.  The shapes are the smallest that reach each edge: 1 to
65 rows (the three tile counts of begin / move and their borders, one to five passes of the silencing workgroup), spans of 1 to
6145 float4 (the tile split, the unrolled copies, the 2048 float4 the end kernel scans from registers and the loop behind
them), tables of 1 to 32 spans.  `fault` and `edone` are pinned host words read in place.  The replay cases capture a chunk's
session nodes once and replay them with nothing but new words.  Every claim is exact equality; every case prints its label."""
import ctypes

import numpy as np
import pytest
import torch

from lookoncetohear_amd import _cabi
from tests import session_kernel_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = [(False, False), (True, False), (False, True), (True, True)]
FORM_IDS = ["slots", "rows", "paced", "rows_paced"]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _cabi.load()


def shapes(rows):
    """(rows launched, S) over the row counts of the issue; the row forms launch fewer rows than S where they can."""
    return C.ROWS_OF_S if rows else tuple((n, n) for n in C.ROW_COUNTS)


@pytest.mark.parametrize("rows,paced", FORMS, ids=FORM_IDS)
def test_begin_equals_the_restatement(lib, rows, paced):
    for i, (n, S) in enumerate(shapes(rows)):
        sizes = C.COPY_TABLES[3] if S == 3 else C.COPY_TABLES[i % 3]
        C.run_begin(lib, DEV, S, sizes, rows, paced, n_rows=n, first=7 * i)


@pytest.mark.parametrize("rows,paced", FORMS, ids=FORM_IDS)
def test_end_equals_the_restatement(lib, rows, paced):
    for i, (n, S) in enumerate(shapes(rows)):
        C.run_end(lib, DEV, S, C.END_TABLES[i % 8], rows, paced, n_rows=n, first=11 * i, alias=i % 2 == 1, with_from=i % 3 != 2)


@pytest.mark.parametrize("rows,paced", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("role", ["begin", "end"])
def test_word_table(lib, role, rows, paced):
    """Every host word x device word x active x input (x hold), 65 rows per launch."""
    S, n = 65, len(C.word_table(paced))
    for first in range(0, n, S):
        if role == "begin":
            C.run_begin(lib, DEV, S, (3, 257), rows, paced, n_rows=S, first=first)
        else:
            C.run_end(lib, DEV, S, (1, 2049), rows, paced, n_rows=S, first=first)


@pytest.mark.parametrize("rows,paced", FORMS, ids=FORM_IDS)
def test_end_nonfinite_probes(lib, rows, paced):
    """One inf / NaN per launch, in each component of a float4 in turn, at float4 0, 2047, 2048, 2049 and n16 - 1 of the first
    and the last span of tables of 1, 2 and 8 spans and in the output row; and the same value in the neighbour's, an idle, a
    held and an unowned row."""
    for k, (sizes, span, j4) in enumerate(C.probe_list()):
        C.run_end_probe(lib, DEV, rows, paced, sizes, span, j4, k)


@pytest.mark.parametrize("paced", [False, True], ids=["slots", "paced"])
def test_move_equals_the_restatement(lib, paced):
    for i, (n, S) in enumerate(C.ROWS_OF_S + ((3, 3), (17, 17))):
        sizes = C.COPY_TABLES[3] if S == 16 else C.COPY_TABLES[i % 3]
        C.run_move(lib, DEV, S, n, sizes, paced, first=5 * i)


@pytest.mark.parametrize("paced", [False, True], ids=["slots", "paced"])
def test_capture_equals_the_restatement(lib, paced):
    for S in (1, 17, 65):
        for n_chunks in (1, 3):
            C.run_capture(lib, DEV, S, n_chunks, paced)


@pytest.mark.parametrize("heads", [1, 4])
def test_save_restore_rotations(lib, heads):
    """window 1, 49 and 50 of 50 ring rows; ring rows of 16, 48 and 4864 bytes (the K row of the model); saved positions 0, 17
    and 49; a paced target and lock-step targets at delta 0, 1 and window - 1; dead snapshots."""
    for window, rb, pos, delta, dead in ((50, (16, 48, 4864), 17, None, False), (50, (48,), 49, 1, False), (50, (16,), 0, 49, True),
                                         (49, (48, 16), 17, 48, False), (49, (4864,), 0, 0, False), (1, (48, 16), 0, 0, False),
                                         (50, (4864, 16), 49, 0, False), (49, (16,), 48, 1, True), (50, (4864,), 0, None, True),
                                         (50, (48, 4864), 17, 49, False), (49, (16, 4864), 48, None, False)):
        L = C.make_layout(2, (3, 257), len(rb), rb, heads, window)
        C.run_save_restore(lib, DEV, L, saved_pos=pos, delta=delta, dead=dead)


def test_save_restore_table_sizes(lib):
    """n_flat + n_rings at 2 and at 40, the most the two tables hold; flat spans of 1 .. 4097 float4."""
    for n16 in (4097, 1025, 15):
        C.run_save_restore(lib, DEV, C.make_layout(1, (n16,), 1, (48,), 4, 50), saved_pos=17, delta=1)
    C.run_save_restore(lib, DEV, C.make_layout(32, C.COPY_SIZES, 8, (16, 48, 4864), 4, 49), saved_pos=17, delta=None)
    C.run_save_restore(lib, DEV, C.make_layout(32, C.COPY_SIZES, 8, (4864, 16), 1, 50), saved_pos=49, delta=1)


@pytest.mark.parametrize("shared", [False, True], ids=["pos_rows", "pos_shared"])
def test_snapshot_rows_equal_the_single_form(lib, shared):
    for S, n_items, heads, window in ((3, 1, 4, 50), (8, 5, 1, 49), (5, 5, 4, 1), (17, 17, 4, 50)):
        L = C.make_layout(3, (3, 257, 1), 2, (48, 4864), heads, window)
        C.run_snapshot_rows(lib, DEV, L, S, n_items, shared)


@pytest.mark.parametrize("n_items", [1, 5, 8])
def test_embed_proj_ln_rows_is_the_single_form_per_row(lib, n_items):
    """gain[items[i].row] from embed[items[i].slot] holds the bits of `lh_embed_proj_ln` on that embedding alone; rows nobody
    names, and the rows of items outside [0, S), are not written."""
    S, N = 8, 6208
    g = torch.Generator().manual_seed(n_items)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    embed, w, bias, ln_w, ln_b = r(S, 256), r(N, 256) * 0.06, r(N) * 0.1, 1 + 0.1 * r(N), 0.1 * r(N)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rows = [(3 * i + 2) % S for i in range(n_items)]
    items = [(rows[i], (rows[i] + 3) % S, 0, -5) for i in range(n_items)]      # `index` and `gen` are not looked at
    if n_items == 5:
        items[3] = (S, 1, 0, 0)
        items[4] = (rows[4], -1, 0, 0)
    table = torch.tensor(items, dtype=torch.int32, device=DEV)
    scratch, gain = C.Guarded((S, N), torch.float32, DEV), C.Guarded((S, 97, 64), torch.float32, DEV)
    scratch.fill_pattern(), gain.fill_pattern()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    with torch.cuda.device(DEV):
        assert lib.raw("lh_embed_proj_ln_rows")(P(embed), P(w), P(bias), P(ln_w), P(ln_b), P(scratch.t), P(gain.t), P(table),
                                                n_items, S, stream) == 0
        torch.cuda.synchronize()
        scratch.check("scratch"), gain.check("gain")
        got = gain.t.view(torch.int32).cpu()
        named = set()
        for row, slot, _, _ in items:
            if not (0 <= row < S and 0 <= slot < S):
                continue
            named.add(row)
            s1, g1 = torch.empty(1, N, device=DEV), torch.empty(1, 97, 64, device=DEV)
            assert lib.raw("lh_embed_proj_ln")(P(embed[slot]), P(w), P(bias), P(ln_w), P(ln_b), P(s1), P(g1), 1, stream) == 0
            assert torch.equal(got[row], g1[0].view(torch.int32).cpu()), (n_items, row, slot)
        for row in set(range(S)) - named:
            assert bool((got[row] == gain.pat).all()), (n_items, row)
    assert len(named) == (3 if n_items == 5 else n_items)


def test_ring_advance_rows(lib):
    for n in (1, 17, 65):
        C.run_ring_advance(lib, DEV, n)
    C.run_ring_advance(lib, DEV, 3, modulo=1)


def test_refusals_write_nothing(lib):
    """The header's LH_ERR_ARG list of every entry point above returns 1 and leaves every buffer and guard as it was."""
    assert C.refusal_cases(lib, DEV) > 250


# ---- replay ----------------------------------------------------------------------------------------------------------------------
def capture_graph(d, launches):
    """The launches captured once on a side stream; the span tables they were given are wiped afterwards: they travelled in the
    launch arguments."""
    side = torch.cuda.Stream(DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        for entry, args in launches(d):
            assert d.call(entry, args) == 0, entry
    for t in d.keep:
        ctypes.memset(ctypes.addressof(t), 0, ctypes.sizeof(t))
    return graph


def replay(d, graph):
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()


def repost(b, cnt, S, first, paced=False):
    """What a host posts between two chunks: its command words, new input rows, new output rows."""
    table = C.word_table(paced)
    for r in range(S):
        host, _, _, inp, _ = table[(first + r) % len(table)]
        b["cmd"][0, r] = C.host_word(host, first + r)
        b["chunk_in"][r] = C.input_row(cnt, inp)
    for k in ("out", "out_rows"):
        if k in b:
            b[k] = cnt.take(*b[k].shape)
    return b


def test_replay_begin_end(lib):
    """begin -> end captured once, replayed twice with words posted in between: each replay is the restatement applied once
    more."""
    S, sizes = 17, (3, 2049)
    b, spans, carry = C.end_bufs(S, sizes, False, False, S, first=2)
    cnt = C.Counter(1 << 24)
    b["chunk"] = cnt.take(S, C.IN_W)
    d = C.Dev(lib, DEV, b)
    graph = capture_graph(d, lambda d: [("lh_session_begin", C.begin_args(d, spans, S, S, False, False)),
                                        ("lh_session_end", C.end_args(d, spans, S, S, False, False))])
    d.compare(b, "capture launches nothing")
    for i in range(2):
        b = C.ref_end(C.ref_begin(b, spans, S), spans, S)
        replay(d, graph)
        d.compare(b, f"replay {i} of begin -> end")
        b = repost(b, cnt, S, 31 + 40 * i)
        for k in ("cmd", "chunk_in", "out"):
            d.set(k, b[k])
        if i == 0:                                     # the next chunk's (h, c): one overflow in a live row's slice
            b["span1"] = cnt.take(S, 4 * sizes[1])
            live = [r for r in range(S) if b["active"][r]]
            assert live
            b["span1"][live[0], 4 * 2048 + 1] = C.INF
            d.set("span1", b["span1"])


def test_replay_move_begin_rows_end_rows(lib):
    """move -> begin_rows -> end_rows captured once.  The first replay moves two rows and zeroes the table; the second, with
    new words and no new table, moves nothing."""
    S, n, sizes = 8, 5, (3, 257, 2049)
    b, spans, carry = C.end_bufs(S, sizes, True, False, n, first=4)
    cnt = C.Counter(1 << 24)
    b["chunk"] = cnt.take(S, C.IN_W)
    b["from"] = np.array([6, 0, 8, 0, 0, 0, 0, 0], dtype=C.U32)      # row 5 -> row 0, row 7 -> row 2
    b["active"][5], b["active"][7] = 77, 0
    d = C.Dev(lib, DEV, b)
    graph = capture_graph(d, lambda d: [("lh_session_move", C.move_args(d, spans, S, n, False)),
                                        ("lh_session_begin_rows", C.begin_args(d, spans[:2], S, n, True, False)),
                                        ("lh_session_end_rows", C.end_args(d, spans[2:], S, n, True, False))])
    for i in range(2):
        moved = C.ref_move(b, spans, S, n)
        assert any(not np.array_equal(moved[s], b[s]) for s in spans) == (i == 0)
        b = C.ref_end(C.ref_begin(moved, spans[:2], S, n, True), spans[2:], S, n, True)
        assert not b["from"][:n].any()
        replay(d, graph)
        d.compare(b, f"replay {i} of move -> begin_rows -> end_rows")
        b = repost(b, cnt, S, 9)
        for k in ("cmd", "chunk_in", "out", "out_rows"):
            d.set(k, b[k])
