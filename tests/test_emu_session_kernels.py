"""CPU: the session kernels of lh_stream.hip — begin, end, move, capture, save / restore in their ROWS / PACED forms, and
`lh_ring_advance_rows` — called directly over the emulated library and held, word for word, to the integer restatement of
include/lookonce_hip.h in tests/session_kernel_cases.py.  The subset of tests/test_gpu_session_kernels.py that is cheap here:
1, 3 and 17 rows, spans of 1, 3, 257, 2047, 2049 and 4097 float4, the full word table, the non-finite probes and the snapshot
rotations.  This is where the end kernel's loop over spans longer than 2048 float4 runs, which no streamer reaches.  What the
emulator cannot stand in for — the 64-lane reduction of sixteen waves, the system-scope stores to pinned memory, graph replay —
is the device file's."""
import ctypes
import mmap

import numpy as np
import pytest

from lookoncetohear_amd import _cabi
from tests import session_kernel_cases as C

FORMS = [(False, False), (True, False), (False, True), (True, True)]
FORM_IDS = ["slots", "rows", "paced", "rows_paced"]
SIZES = (1, 3, 257, 2047, 2049, 4097)
LOCKSTEP = ((1, 1), (3, 3), (17, 17))                  # (rows launched, S)
COMPACT = ((1, 3), (3, 17), (17, 17))
TABLES = ((4097,), SIZES, (257, 1))
END_TABLES = ((4097,), SIZES, (2049,))


@pytest.fixture(scope="module")
def emu_lib():
    from tests.hipemu.build_emu import build_emu
    return _cabi.Lib(build_emu())


@pytest.mark.parametrize("rows,paced", FORMS, ids=FORM_IDS)
def test_begin_equals_the_restatement(emu_lib, rows, paced):
    for (n, S), sizes in zip(COMPACT if rows else LOCKSTEP, TABLES):
        C.run_begin(emu_lib, "cpu", S, sizes, rows, paced, n_rows=n, first=3 * n)


@pytest.mark.parametrize("rows,paced", FORMS, ids=FORM_IDS)
def test_end_equals_the_restatement(emu_lib, rows, paced):
    for i, ((n, S), sizes) in enumerate(zip(COMPACT if rows else LOCKSTEP, END_TABLES)):
        C.run_end(emu_lib, "cpu", S, sizes, rows, paced, n_rows=n, first=5 * n, alias=i == 1, with_from=i != 2)


@pytest.mark.parametrize("rows,paced", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("role", ["begin", "end"])
def test_word_table(emu_lib, role, rows, paced):
    """Every host word x device word x active x input (x hold), 17 rows per launch."""
    S, n = 17, len(C.word_table(paced))
    for first in range(0, n, S):
        if role == "begin":
            C.run_begin(emu_lib, "cpu", S, (3,), rows, paced, n_rows=S, first=first)
        else:
            C.run_end(emu_lib, "cpu", S, (1, 3), rows, paced, n_rows=S, first=first)


@pytest.mark.parametrize("rows,paced", FORMS, ids=FORM_IDS)
def test_end_nonfinite_probes(emu_lib, rows, paced):
    """One inf / NaN per launch at float4 0, 2047, 2048, 2049 and n16 - 1 of the first and the last span and in the output row:
    the lock-step form takes every probe, the other forms the table of two spans."""
    probes = C.probe_list() if not (rows or paced) else C.probe_list(C.PROBE_TABLES[1:2])
    for k, (sizes, span, j4) in enumerate(probes):
        C.run_end_probe(emu_lib, "cpu", rows, paced, sizes, span, j4, k)


@pytest.mark.parametrize("paced", [False, True], ids=["slots", "paced"])
def test_move_equals_the_restatement(emu_lib, paced):
    for (n, S), sizes in zip(((1, 3), (3, 3), (3, 17), (17, 17)), ((4097,), (1, 3, 257), (2047, 2049), (3, 257))):
        C.run_move(emu_lib, "cpu", S, n, sizes, paced, first=2 * n)


@pytest.mark.parametrize("paced", [False, True], ids=["slots", "paced"])
def test_capture_equals_the_restatement(emu_lib, paced):
    for S, n_chunks in ((1, 1), (17, 3), (3, 1)):
        C.run_capture(emu_lib, "cpu", S, n_chunks, paced)


@pytest.mark.parametrize("heads", [1, 4])
def test_save_restore_rotations(emu_lib, heads):
    """window 1, 49 and 50 of 50 ring rows; ring rows of 16, 48 and 4864 bytes; saved positions 0, 17 and 49; a paced target
    and lock-step targets at delta 0, 1 and window - 1; a dead snapshot."""
    for window, rb, pos, delta, dead in ((50, (16, 48, 4864), 17, None, False), (50, (48,), 49, 1, False), (50, (16,), 0, 49, True),
                                         (49, (48, 16), 17, 48, False), (49, (4864,), 0, 0, False), (1, (48, 16), 0, 0, False),
                                         (50, (4864, 16), 49, 0, False), (49, (16,), 48, 1, True)):
        L = C.make_layout(2, (3, 257), len(rb), rb, heads, window)
        C.run_save_restore(emu_lib, "cpu", L, saved_pos=pos, delta=delta, dead=dead)


def test_save_restore_table_sizes(emu_lib):
    """n_flat + n_rings at 2 and at 40, the most the two tables hold; flat spans of 1 .. 4097 float4."""
    C.run_save_restore(emu_lib, "cpu", C.make_layout(1, (4097,), 1, (48,), 4, 50), saved_pos=17, delta=1)
    C.run_save_restore(emu_lib, "cpu", C.make_layout(32, (1, 3, 257, 2047, 2049), 8, (16, 48), 1, 49), saved_pos=17, delta=None)


@pytest.mark.parametrize("shared", [False, True], ids=["pos_rows", "pos_shared"])
def test_snapshot_rows_equal_the_single_form(emu_lib, shared):
    for S, n_items, heads, window in ((3, 1, 4, 50), (8, 5, 1, 49), (5, 5, 4, 1)):
        L = C.make_layout(3, (3, 257, 1), 2, (48, 16), heads, window)
        C.run_snapshot_rows(emu_lib, "cpu", L, S, n_items, shared)


def test_ring_advance_rows(emu_lib):
    for n in (1, 17, 65):
        C.run_ring_advance(emu_lib, "cpu", n)
    C.run_ring_advance(emu_lib, "cpu", 3, modulo=1)


def test_refusals_write_nothing(emu_lib):
    """The header's LH_ERR_ARG list of every entry point above returns 1 and leaves every buffer and guard as it was."""
    assert C.refusal_cases(emu_lib, "cpu") > 250


@pytest.mark.parametrize("paced", [False, True], ids=["slots", "paced"])
def test_move_reads_nothing_behind_the_source_row(emu_lib, paced):
    """The move's clamped loads (`min(j + u * NT, hi - 1)`) never leave the tile: the span's last row, the source, ends where
    an unreadable page begins.  A load of the float4 behind it changes no byte that is stored, so no comparison can see it;
    here it ends the process."""
    S, n16, page = 3, 5, mmap.PAGESIZE
    m = mmap.mmap(-1, 2 * page)
    hold = ctypes.c_char.from_buffer(m)
    base = ctypes.addressof(hold)
    assert ctypes.CDLL(None, use_errno=True).mprotect(ctypes.c_void_p(base + page), ctypes.c_size_t(page), 0) == 0
    span = np.frombuffer(m, dtype=C.U32, count=page // 4)[page // 4 - S * 4 * n16:].reshape(S, 4 * n16)
    span[:] = C.Counter(1000).take(S, 4 * n16)
    b, _, _ = C.session_bufs(S, (), False, paced, first=8)
    b["from"] = np.array([S, 0, 0], dtype=C.U32)       # the last row over row 0
    want = C.ref_move(dict(b, span=span), ["span"], S, 1, paced)
    d = C.Dev(emu_lib, "cpu", b)
    table = (C.Span * 1)(C.Span(span.ctypes.data, 16 * n16))
    args = C.move_args(d, [], S, 1, paced)
    args[0], args[1] = ctypes.c_void_p(ctypes.addressof(table)), 1
    assert span.ctypes.data + span.nbytes == base + page
    assert d.call("lh_session_move" + ("_paced" if paced else ""), args) == 0
    assert np.array_equal(span, want.pop("span")) and np.array_equal(span[0], span[2])
    d.compare(want, "move from the last row of a span that ends at an unreadable page")
    del span, hold
