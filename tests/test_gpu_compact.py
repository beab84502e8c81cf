"""GPU: `SessionStreamer(compact=True)` under graph replay — open listeners live in the leading rows, a listener that leaves
makes the survivors above move down (`lh_session_move`), and a chunk is launched for the bucket of the rows in use (one
alternating graph pair per bucket).  S = 8 throughout.  A session's reference is the float64 oracle over the session's OWN
samples from the zero state, tolerance as in tests/test_gpu_sessions.py; isolation, placement and equality claims are
`torch.equal`.  The 3e38 burst of the fault test is ordinary data for the range guard and runs once."""
import contextlib
from unittest import mock

import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.net import Net
from oracle import tfgridnet_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_gpu_sessions.py
DEV = "cuda:0"
HOP, NFFT = 128, 192
S = 8


@pytest.fixture(scope="module")
def net(oracle_cfg_sd):
    assert torch.cuda.is_available()
    _cabi.load()
    cfg, sd = oracle_cfg_sd
    n = Net(**O.TSH_PARAMS).eval()
    n.load_state_dict(sd, strict=True)
    return n.to(DEV)


def clips(idx, n_chunks):
    d = synth.batch(idx, HOP * n_chunks + NFFT - HOP)
    return d["mixture"], d["embedding_gt"][:, 0]


def fresh_stream64(oracle_cfg_sd, mix_row, emb_row, n):
    """float64 oracle output of the first n chunks of a stream that starts from the zero state: [2, 128 n]."""
    cfg, sd = oracle_cfg_sd
    y, _ = O.predict(cfg, sd, mix_row[None, :, :HOP * n + NFFT - HOP], emb_row[None], None, pad=False, dtype=torch.float64,
                     fast_lstm=True)
    return y[0]


def run_schedule(ss, sessions, n, mix, emb, each=None):
    """sessions: (slot, first chunk, end chunk (exclusive), clip).  Closings before openings, rows of idle slots are NaN: they
    must be ignored.  each(i) runs after step i.  [S, 2, 128 n] on the host."""
    outs = []
    for i in range(n):
        for slot, t0, t1, c in sessions:
            if t1 == i:
                ss.close(slot)
        for slot, t0, t1, c in sessions:
            if t0 == i:
                ss.open(slot, emb[c])
        x = torch.full((S, 2, NFFT), float("nan"), device=DEV)
        for slot, t0, t1, c in sessions:
            if t0 <= i < t1:
                x[slot] = mix[c, :, (i - t0) * HOP:(i - t0) * HOP + NFFT]
        outs.append(ss.step(x).clone())
        if each:
            each(i)
    torch.cuda.synchronize()
    return torch.cat(outs, -1).cpu()


# Openings at chunks 0, 3, 5, 7, 20, 49, 50 and 63 — before, at and after the 50-slot ring wraps.  Rows in use and the bucket
# launched: 1, 2, 3 (4), 4, 5 (8); slot 1 closes at 40 out of row 1 with rows 2..4 in use (row 4 moves down), 4 (4); at 49 slot 7
# closes and slot 4 opens into its row; 5 (8) at 50; slots 3 and 4 close together at 60: 3 (4); slot 1 re-used at 63: 4; 3 at
# 100; 2 (2) at 110.  Slot 6 is never opened.
SESSIONS = [(0, 0, 120, 0), (1, 3, 40, 1), (7, 5, 49, 2), (2, 7, 100, 3), (3, 20, 60, 4), (4, 49, 60, 5), (5, 50, 110, 6),
            (1, 63, 120, 7)]
N_CHUNKS = 120


def test_schedule_across_buckets(net, oracle_cfg_sd):
    mix, emb = clips(list(range(40, 48)), N_CHUNKS)
    mixd, embd = mix.to(DEV), emb.to(DEV)
    ss = net.make_session_streamer(S, DEV, compact=True)
    assert ss.graphs is not None and ss.row_buckets == (1, 2, 4, 8)
    launched = []
    y = run_schedule(ss, SESSIONS, N_CHUNKS, mixd, embd, lambda i: launched.append((ss.rows_in_use, ss.last_rows)))
    assert ss.faults() == [] and ss.active == [0, 1] and ss.rows_in_use == 2
    assert torch.isfinite(y).all()
    rows = {0: 1, 3: 2, 5: 3, 7: 4, 20: 5, 40: 4, 49: 4, 50: 5, 60: 3, 63: 4, 100: 3, 110: 2}
    want = [rows[max(t for t in rows if t <= i)] for i in range(N_CHUNKS)]
    assert [r for r, _ in launched] == want
    assert [b for _, b in launched] == [min(b for b in (1, 2, 4, 8) if b >= r) for r in want]
    took = [b for _, b in launched]
    assert set(took) == {1, 2, 4, 8} and took[-1] == 2 and took.index(8) < took.index(4, 40)       # ... and shrank again
    busy = torch.zeros(S, N_CHUNKS, dtype=torch.bool)
    for slot, t0, t1, c in SESSIONS:
        ref = fresh_stream64(oracle_cfg_sd, mix[c], emb[c], t1 - t0)
        e = float((y[slot, :, t0 * HOP:t1 * HOP].double() - ref).abs().max())
        print(f"slot {slot} chunks {t0}..{t1}: max|hip - fp64 fresh stream| = {e:.2e}")
        assert e <= TOL, (slot, t0, e)
        busy[slot, t0:t1] = True
    idle = ~busy.repeat_interleave(HOP, 1)[:, None, :].expand(-1, 2, -1)
    assert idle.any() and not y[idle].any()                  # idle slots are exact zeros
    # the same bits from a second run of the same streamer, and from the eager launches
    ss.reset()
    assert ss.rows_in_use == 0
    assert torch.equal(run_schedule(ss, SESSIONS, N_CHUNKS, mixd, embd), y)
    eager = net.make_session_streamer(S, DEV, use_graph=False, compact=True)
    assert eager.graphs is None
    assert torch.equal(run_schedule(eager, SESSIONS, N_CHUNKS, mixd, embd), y)


def test_row_placement_does_not_change_bits(net):
    """One launch size (8, as in the lock-step streamer), so only the ROW of a listener differs between the two objects: slot
    6's listener lives in rows 6 -> 4 -> 2 -> 0 here and in row 6 there, slot 1's in row 1 in both."""
    n = 24
    sessions = [(0, 0, 12, 0), (1, 0, n, 1), (2, 0, 8, 2), (3, 0, 12, 3), (4, 0, 4, 4), (5, 0, 8, 5), (6, 0, n, 6)]
    mix, emb = clips(list(range(60, 67)), n)
    mixd, embd = mix.to(DEV), emb.to(DEV)
    ss = net.make_session_streamer(S, DEV, compact=True, row_buckets=(S,))
    lock = net.make_session_streamer(S, DEV)
    seen = []
    y = run_schedule(ss, sessions, n, mixd, embd, lambda i: seen.append((ss._row_of[6], ss._row_of[1], ss.last_rows)))
    assert seen[0] == (6, 1, S) and seen[4] == (4, 1, S) and seen[8] == (2, 1, S) and seen[12] == (0, 1, S)
    assert [r for r, _, _ in seen] == [6] * 4 + [4] * 4 + [2] * 4 + [0] * 12
    yl = run_schedule(lock, sessions, n, mixd, embd)
    for slot in range(S):
        assert torch.equal(y[slot], yl[slot]), slot
    assert y[6].any() and ss.faults() == [] and ss.active == [1, 6]


def test_fault_in_a_moved_row(net, oracle_cfg_sd):
    """All 8 open; slot 0 closes at chunk 3, so slot 7's listener moves to row 0; its chunk 8 is a finite 3e38 burst that
    overflows fp32 inside the separator (caught by lh_session_end_rows, reported under slot 7)."""
    n, close_at, bad_at, reopen_at = 24, 3, 8, 14
    mix, emb = clips(list(range(50, 59)), n)
    mixd, embd = mix.to(DEV), emb.to(DEV)

    def run(fault):
        ss = net.make_session_streamer(S, DEV, compact=True)
        for s in range(S):
            ss.open(s, embd[s])
        outs, seen = [], {}
        for i in range(n):
            if i == close_at:
                ss.close(0)
            x = mixd[:S, :, i * HOP:i * HOP + NFFT].clone()
            if i >= close_at:
                x[0] = float("nan")
            if fault:
                if i == bad_at:
                    assert ss._row_of[7] == 0
                    x[7] = 3e38
                if i == reopen_at:
                    ss.open(7, embd[8])
                if i >= reopen_at:
                    x[7] = mixd[8, :, (i - reopen_at) * HOP:(i - reopen_at) * HOP + NFFT]
            outs.append(ss.step(x).clone())                  # never raises
            if fault and i in (bad_at - 1, bad_at, bad_at + 1, bad_at + 2):
                torch.cuda.synchronize()
                seen[i] = (ss.faults(), ss.active, ss.rows_in_use)
        torch.cuda.synchronize()
        return torch.cat(outs, -1).cpu(), seen, ss

    clean, _, _ = run(False)
    y, seen, ss = run(True)
    others = list(range(1, 7))
    assert seen[bad_at - 1] == ([], list(range(1, 8)), 7)
    assert seen[bad_at] == ([7], others, 7)                  # the device's word; the host's rows are as of this step
    assert seen[bad_at + 1] == seen[bad_at + 2] == ([7], others, 6)
    assert torch.equal(y[others], clean[others])
    assert torch.equal(y[7, :, :bad_at * HOP], clean[7, :, :bad_at * HOP])
    assert not y[7, :, bad_at * HOP:reopen_at * HOP].any() and not y[0, :, close_at * HOP:].any()
    assert torch.isfinite(y).all()
    ref = fresh_stream64(oracle_cfg_sd, mix[8], emb[8], n - reopen_at)
    e = float((y[7, :, reopen_at * HOP:].double() - ref).abs().max())
    print(f"slot 7 re-opened after the fault in its moved row: max|hip - fp64 fresh stream| = {e:.2e}")
    assert e <= TOL
    assert ss.faults() == [] and ss.active == list(range(1, 8)) and ss.rows_in_use == 7 and ss._row_of[7] == 6


@contextlib.contextmanager
def no_host_wait():
    def refuse(*a, **k):
        raise AssertionError("the host waited for the device inside the chunk loop")
    with mock.patch.object(torch.cuda, "synchronize", refuse), mock.patch.object(torch.cuda.Stream, "synchronize", refuse), \
            mock.patch.object(torch.cuda.Event, "synchronize", refuse):
        yield


def test_enrollment_with_compaction(net, oracle_cfg_sd):
    """Slots 0 and 1 open (rows 0, 1); slot 5 enrolls at step 2 with a stand-in embedder; slot 0 closes at step 4, during the
    capture: slot 1's listener moves to row 0.  The enrolled slot opens into the last row as a fresh stream of the samples
    it goes on sending.  The loop ends when it has; its cap is a condition (the host runs ahead of the device), not a
    measurement."""
    n_enroll, cap, tail = 4, 2000, 10
    mix, emb = clips([70, 71, 72], 32)
    mixd, embd = mix.to(DEV), emb.to(DEV)
    own = clips([72], cap + tail)[0][0]                      # slot 5's own stream, one chunk per step from step 0 on
    ownd = own.to(DEV)
    calls = []

    def stand_in(x):                                         # the embedding the listener's reference is computed with
        calls.append(tuple(x.shape))
        return embd[2][None].expand(x.shape[0], -1).clone()
    ss = net.make_session_streamer(S, DEV, enroll_chunks=n_enroll, compact=True)
    ss.open(0, embd[0]), ss.open(1, embd[1])
    outs, opened, rows = [], None, {}
    with no_host_wait():
        for i in range(cap):
            if i == 2:
                ss.enroll(5, stand_in)
            if i == 4:
                ss.close(0)
            x = torch.full((S, 2, NFFT), float("nan"), device=DEV)
            j = i % 30
            x[1] = mixd[1, :, j * HOP:j * HOP + NFFT]
            if i < 4:
                x[0] = mixd[0, :, j * HOP:j * HOP + NFFT]
            x[5] = ownd[:, i * HOP:i * HOP + NFFT]
            outs.append(ss.step(x).clone())
            if opened is None and 5 in ss.active:
                opened = i                                   # the step whose poll opened it: a fresh stream from this step on
            rows[i] = (list(ss._slot_of), ss.rows_in_use, ss.enrolling)
            assert ss.faults() == []
            if opened is not None and i == opened + tail - 1:
                break
        else:
            raise AssertionError("the enrolling slot did not open within the cap")
    torch.cuda.synchronize()
    print("enrolled slot opened at step", opened, "of", len(outs), "; embedder calls:", calls)
    assert opened is not None and opened >= 2 + n_enroll and calls == [(1, 2, HOP * n_enroll)]
    assert rows[3] == ([0, 1] + [-1] * 6, 2, [5]) and rows[4][:2] == ([1] + [-1] * 7, 1)      # a capturing slot owns no row
    assert rows[opened - 1][:2] == ([1] + [-1] * 7, 1) and rows[opened] == ([1, 5] + [-1] * 6, 2, [])
    assert ss.active == [1, 5] and ss._row_of[5] == ss.rows_in_use - 1 == 1
    y = torch.cat(outs, -1).cpu()
    assert not y[5, :, :opened * HOP].any() and not y[0, :, 4 * HOP:].any() and torch.isfinite(y).all()
    ref = fresh_stream64(oracle_cfg_sd, own[:, opened * HOP:], emb[2], tail)
    e = float((y[5, :, opened * HOP:].double() - ref).abs().max())
    print(f"enrolled slot in row 1: max|hip - fp64 fresh stream| = {e:.2e}")
    assert e <= TOL


def test_default_is_unchanged(net):
    """Without the new keywords: the lock-step object, bit-identical to `Streamer(4)` over 60 chunks (the ring wraps)."""
    B, n = 4, 60
    mix, emb = clips([31, 32, 33, 34], n)
    mix, emb = mix.to(DEV), emb.to(DEV)
    st = net.make_streamer(B, DEV)
    st.set_embedding(emb)
    ss = net.make_session_streamer(B, DEV)
    assert not ss.compact and ss.row_buckets is None and isinstance(ss.graphs, list) and len(ss.graphs) == 2
    assert ss._words.shape == (3, B) and ss.out is ss._st.out
    for s in range(B):
        ss.open(s, emb[s])
    for i in range(n):
        x = mix[:, :, i * HOP:i * HOP + NFFT]
        assert torch.equal(ss.step(x).clone(), st.step(x).clone()), i
    torch.cuda.synchronize()
    assert ss.active == [0, 1, 2, 3] and ss.faults() == [] and ss.rows_in_use == ss.last_rows == B
