"""GPU: `SessionStreamer(pace=True)` under graph replay — a listener whose chunk is late is HELD for the step (`step(chunks,
present)`): their input row is ignored, their output row is zeros and their state, K / V rings and ring position included, is
afterwards what it was before; every row owns its ring position, so a listener's bits depend on their own chunks only.
Equality claims are `torch.equal`; a listener's reference is the float64 oracle over their OWN samples from the zero state,
tolerance as in tests/test_gpu_parity.py.  Held and idle input rows are NaN throughout.  The NaN of the fault case is ordinary
input data for lh_session_begin_paced and runs once."""
import contextlib
from unittest import mock

import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.net import Net
from oracle import tfgridnet_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_gpu_parity.py
DEV = "cuda:0"
HOP, NFFT = 128, 192
S, N_CLIP = 4, 120


@pytest.fixture(scope="module")
def net(oracle_cfg_sd):
    assert torch.cuda.is_available()
    _cabi.load()
    cfg, sd = oracle_cfg_sd
    n = Net(**O.TSH_PARAMS).eval()
    n.load_state_dict(sd, strict=True)
    return n.to(DEV)


@pytest.fixture(scope="module")
def clips():
    """Four listeners: mix [4, 2, 128 * 120 + 64] and emb [4, 256], on the host and on the device."""
    d = synth.batch([80, 81, 82, 83], HOP * N_CLIP + NFFT - HOP)
    mix, emb = d["mixture"], d["embedding_gt"][:, 0]
    return mix, emb, mix.to(DEV), emb.to(DEV)


@pytest.fixture(scope="module")
def plain(net, clips):
    """Every listener's clip without a hold: all four opened before the first chunk of one paced streamer.  [4, 2, 128 * 120]"""
    _, _, mixd, embd = clips
    ss = net.make_session_streamer(S, DEV, pace=True)
    for s in range(S):
        ss.open(s, embd[s])
    outs = [ss.step(mixd[:, :, i * HOP:i * HOP + NFFT]).clone() for i in range(N_CLIP)]
    torch.cuda.synchronize()
    assert ss.faults() == []
    return torch.cat(outs, -1).cpu()


@pytest.fixture(scope="module")
def fresh64(oracle_cfg_sd, clips):
    """float64 oracle output of each clip as a stream that starts from the zero state (tests/test_gpu_sessions.py:
    fresh_stream64), computed once; the model is causal, so a listener's first n chunks are its first 128 n samples."""
    cfg, sd = oracle_cfg_sd
    mix, emb, _, _ = clips
    return [O.predict(cfg, sd, mix[c][None], emb[c][None], None, pad=False, dtype=torch.float64, fast_lstm=True)[0][0]
            for c in range(S)]


@contextlib.contextmanager
def no_host_wait():
    def refuse(*a, **k):
        raise AssertionError("the host waited for the device inside the chunk loop")
    with mock.patch.object(torch.cuda, "synchronize", refuse), mock.patch.object(torch.cuda.Stream, "synchronize", refuse), \
            mock.patch.object(torch.cuda.Event, "synchronize", refuse):
        yield


def test_all_present_equals_lock_step(net, clips):
    """S = 4, every slot opened before the first chunk, 60 chunks (the ring wraps): without `present` and with an all-true
    one, chunk by chunk the bits of the lock-step `make_session_streamer(4)`."""
    n = 60
    _, _, mixd, embd = clips
    lock = net.make_session_streamer(S, DEV)
    a, b = net.make_session_streamer(S, DEV, pace=True), net.make_session_streamer(S, DEV, pace=True)
    assert a.pace and not lock.pace and a.graphs is not None
    for ss in (lock, a, b):
        for s in range(S):
            ss.open(s, embd[s])
    everyone = torch.ones(S, dtype=torch.bool)
    for i in range(n):
        x = mixd[:, :, i * HOP:i * HOP + NFFT]
        want = lock.step(x).clone()
        assert torch.equal(a.step(x), want), i
        assert torch.equal(b.step(x, everyone if i % 2 else [True] * S), want), i
    torch.cuda.synchronize()
    assert a.active == b.active == [0, 1, 2, 3] and a.faults() == b.faults() == []
    assert a._ring[0].tolist() == [n % 50] * S and int(lock._st.pos) == n % 50
    with pytest.raises(ValueError):
        lock.step(x, [True] * S)


# ---- the fixed hold schedule: slot s plays clip s ---------------------------------------------------------------------------
N_STEPS = 130
OPEN_AT, CLOSE_AT = {0: 0, 1: 0, 2: 0, 3: 10}, {2: 100}
# by step: slot 0 is held in the step that opens it, once at 5, twice in a row at 8, 9 (both ping-pong parities carry), and
# during slot 3's opening (10); slot 1 is held for 55 steps (30..84: longer than the ring) and during slot 2's closing (100);
# slot 2 twice in a row at 20, 21; slot 3 in the step that opens it; steps 20 and 60 hold everyone
STEP_HOLDS = {0: {0, 5, 8, 9, 10, 20, 60}, 1: {20, 60, 100} | set(range(30, 85)), 2: {3, 20, 21, 60}, 3: {10, 20, 60, 100}}
# by the listener's own count: one held step right before their own chunk k — before, at and after the 50th (k = 49)
OWN_HOLDS = {0: {48, 49, 50, 51}, 3: {49, 50}}


def schedule():
    """[(active, present)] per step and slot, and the chunks each listener consumed."""
    took, used, table = [0] * S, set(), []
    for i in range(N_STEPS):
        row = []
        for s in range(S):
            active = OPEN_AT[s] <= i < CLOSE_AT.get(s, N_STEPS)
            hold = i in STEP_HOLDS[s]
            if active and not hold and took[s] in OWN_HOLDS.get(s, ()) and (s, took[s]) not in used:
                used.add((s, took[s]))
                hold = True
            row.append((active, not hold))
            took[s] += active and not hold
        table.append(row)
    return table, took


def run_held(ss, table, mixd, embd):
    """[N_STEPS, S, 2, 128] on the device; nothing here waits for it."""
    took, outs = [0] * S, []
    for i, row in enumerate(table):
        for s in range(S):
            if CLOSE_AT.get(s) == i:
                ss.close(s)
            if OPEN_AT[s] == i:
                ss.open(s, embd[s])
        x = torch.full((S, 2, NFFT), float("nan"), device=DEV)
        for s, (active, present) in enumerate(row):
            if active and present:
                x[s] = mixd[s, :, took[s] * HOP:took[s] * HOP + NFFT]
                took[s] += 1
        outs.append(ss.step(x, [p for _, p in row]).clone())
    return torch.stack(outs)


def per_listener(y, table):
    """y [N_STEPS, S, 2, 128] on the host -> the concatenated present-step rows of each listener; every other row is zeros."""
    mine = [[] for _ in range(S)]
    for i, row in enumerate(table):
        for s, (active, present) in enumerate(row):
            if active and present:
                mine[s].append(y[i, s])
            else:
                assert not y[i, s].any(), (i, s)
    return [torch.cat(m, -1) for m in mine]


def test_held_listener_keeps_their_bits(net, clips, plain, fresh64):
    _, _, mixd, embd = clips
    table, took = schedule()
    assert took[0] > 52 and took[3] > 51 and max(took) <= N_CLIP and N_STEPS <= 130
    assert any(all(not p for a, p in row if a) for row in table[1:])            # a step in which every slot is held
    assert not table[0][0][1] and not table[10][3][1] and not table[10][0][1] and not table[100][1][1]
    ss = net.make_session_streamer(S, DEV, pace=True)
    y = run_held(ss, table, mixd, embd)
    torch.cuda.synchronize()
    assert ss.faults() == [] and ss.active == [0, 1, 3]
    assert ss._ring[0].tolist() == [t % 50 for t in took]
    y = y.cpu()
    mine = per_listener(y, table)
    for s in range(S):
        n = took[s] * HOP
        assert mine[s].shape[-1] == n and torch.equal(mine[s], plain[s, :, :n]), s
        e = float((mine[s].double() - fresh64[s][:, :n]).abs().max())
        print(f"listener {s}, {took[s]} chunks in {N_STEPS} steps: max|hip - fp64 fresh stream| = {e:.2e}")
        assert e <= TOL, (s, e)
    # the same bits from a second run of the same streamer, and from the eager launches
    ss.reset()
    y2 = run_held(ss, table, mixd, embd)
    eager = net.make_session_streamer(S, DEV, use_graph=False, pace=True)
    assert eager.graphs is None
    y3 = run_held(eager, table, mixd, embd)
    torch.cuda.synchronize()
    assert torch.equal(y2.cpu(), y) and torch.equal(y3.cpu(), y)


def test_opening_time_does_not_matter(net, clips, plain):
    """Slots 0..2 busy from step 0; slot 3 opens at step 63 — its ring position starts at 0, whatever the others' are."""
    at, n = 63, 30
    _, _, mixd, embd = clips
    ss = net.make_session_streamer(S, DEV, pace=True)
    for s in range(3):
        ss.open(s, embd[s])
    outs = []
    for i in range(at + n):
        if i == at:
            ss.open(3, embd[3])
        x = torch.full((S, 2, NFFT), float("nan"), device=DEV)
        x[:3] = mixd[:3, :, i * HOP:i * HOP + NFFT]
        if i >= at:
            x[3] = mixd[3, :, (i - at) * HOP:(i - at) * HOP + NFFT]
        outs.append(ss.step(x, [True, i % 7 != 3, True, True]).clone())
    torch.cuda.synchronize()
    y = torch.cat(outs, -1).cpu()
    assert ss.faults() == [] and not y[3, :, :at * HOP].any()
    assert torch.equal(y[3, :, at * HOP:], plain[3, :, :n * HOP])
    assert torch.equal(y[0], plain[0, :, :(at + n) * HOP])


def test_fault_next_to_a_held_row(net, clips, plain):
    """All four open.  Slot 1's chunk 10 holds a NaN while slot 2 is held (steps 9..11): slot 1 alone is closed, and opens
    again at step 16 as a fresh stream — its ring position is back at 0."""
    n, bad_at, reopen_at = 24, 10, 16
    _, _, mixd, embd = clips
    ss = net.make_session_streamer(S, DEV, pace=True)
    for s in range(S):
        ss.open(s, embd[s])
    took, outs, seen = [0] * S, [], {}
    for i in range(n):
        if i == reopen_at:
            ss.open(1, embd[1])
            took[1] = 0
        present = [True, True, i not in (9, 10, 11), True]
        x = torch.full((S, 2, NFFT), float("nan"), device=DEV)
        for s in range(S):
            if present[s] and not (s == 1 and bad_at < i < reopen_at):
                x[s] = mixd[s, :, took[s] * HOP:took[s] * HOP + NFFT]
                took[s] += 1
        if i == bad_at:
            x[1, 0, 5] = float("nan")
        outs.append(ss.step(x, present).clone())                 # never raises
        if i in (bad_at, bad_at + 1):
            torch.cuda.synchronize()
            seen[i] = (ss.faults(), ss.active)
    torch.cuda.synchronize()
    y = torch.stack(outs).cpu()                                  # [n, S, 2, 128]
    assert seen[bad_at] == ([1], [0, 2, 3]) and seen[bad_at + 1] == ([1], [0, 2, 3])
    assert ss.faults() == [] and ss.active == [0, 1, 2, 3] and torch.isfinite(y).all()
    cat = lambda s, steps: torch.cat([y[i, s] for i in steps], -1)
    for s in (0, 3):
        assert torch.equal(cat(s, range(n)), plain[s, :, :n * HOP]), s
    assert not y[9:12, 2].any()
    assert torch.equal(cat(2, [i for i in range(n) if i not in (9, 10, 11)]), plain[2, :, :(n - 3) * HOP])
    assert torch.equal(cat(1, range(bad_at)), plain[1, :, :bad_at * HOP]) and not y[bad_at:reopen_at, 1].any()
    assert torch.equal(cat(1, range(reopen_at, n)), plain[1, :, :(n - reopen_at) * HOP])


def test_held_rows_move_with_compaction(net, clips):
    """compact=True, pace=True, S = 6 (clips 0..3, 0, 1), all open.  Slot 0 closes at step 3 (odd chunk): slot 5's listener
    moves from row 5 to row 0 in a step it is held; slot 1 closes at step 6 (even chunk): slot 4's moves from row 4 to row 1,
    held as well.  Every listener keeps the bits of the streamer that does not compact."""
    S6, n = 6, 14
    _, _, mixd, embd = clips
    clip = [0, 1, 2, 3, 0, 1]
    close_at = {0: 3, 1: 6}
    holds = {5: {3, 4, 9}, 4: {1, 6}, 2: {6, 7}, 3: {3}}

    def run(compact):
        ss = net.make_session_streamer(S6, DEV, pace=True, compact=compact)
        for s in range(S6):
            ss.open(s, embd[clip[s]])
        took, outs, rows = [0] * S6, [], []
        for i in range(n):
            for s, t in close_at.items():
                if t == i:
                    ss.close(s)
            present = [i not in holds.get(s, ()) for s in range(S6)]
            x = torch.full((S6, 2, NFFT), float("nan"), device=DEV)
            for s in range(S6):
                if present[s] and i < close_at.get(s, n):
                    x[s] = mixd[clip[s], :, took[s] * HOP:took[s] * HOP + NFFT]
                    took[s] += 1
            outs.append(ss.step(x, present).clone())
            rows.append((list(ss._row_of), ss._st.parity ^ 1) if compact else None)
        torch.cuda.synchronize()
        assert ss.faults() == [] and ss.active == [2, 3, 4, 5]
        return torch.stack(outs).cpu(), rows, took

    y, rows, took = run(True)
    assert rows[2] == ([0, 1, 2, 3, 4, 5], 0) and rows[3] == ([-1, 1, 2, 3, 4, 0], 1)       # moved while held, odd chunk
    assert rows[5][0] == rows[3][0] and rows[6] == ([-1, -1, 2, 3, 1, 0], 0)                # ... and even chunk
    lock, _, took2 = run(False)
    assert took == took2 and torch.equal(y, lock)
    assert y[5:, 5].any() and y[7:, 4].any() and not y[3, 5].any() and not y[6, 4].any() and not y[3:, 0].any()


def test_enrollment_records_present_chunks(net, clips):
    """enroll_chunks = 4, pace=True: slot 1 enrolls at step 2 and is held at steps 3 and 5, mid-capture, with NaN rows.  The
    stand-in embedder gets the 512 contiguous samples of the four chunks the slot was present for; then the slot opens.  The
    loop's cap is a condition (the host runs ahead of the device), not a measurement."""
    n_enroll, cap = 4, 2000
    mix, _, mixd, embd = clips
    got = []

    def stand_in(x):
        got.append(x.clone())
        return embd[1][None].expand(x.shape[0], -1).clone()
    ss = net.make_session_streamer(S, DEV, enroll_chunks=n_enroll, pace=True)
    ss.open(0, embd[0])
    took, opened = 0, None
    with no_host_wait():
        for i in range(cap):
            if i == 2:
                ss.enroll(1, stand_in)
            present = [True, i not in (3, 5), True, True]
            x = torch.full((S, 2, NFFT), float("nan"), device=DEV)
            x[0] = mixd[0, :, (i % 100) * HOP:(i % 100) * HOP + NFFT]
            if i >= 2 and present[1]:
                x[1] = mixd[1, :, (took % 100) * HOP:(took % 100) * HOP + NFFT]
                took += 1
            ss.step(x, present)
            if 1 in ss.active:
                opened = i
                break
        else:
            raise AssertionError("the enrolling slot did not open within the cap")
    torch.cuda.synchronize()
    assert opened >= 2 + n_enroll + 2 and ss.faults() == [] and ss.enrolling == [] and ss.active == [0, 1]
    assert len(got) == 1 and torch.equal(got[0].cpu(), mix[1][None, :, :HOP * n_enroll])


def test_host_never_waits(net, clips):
    """The loop of the hold schedule with every `synchronize` refusing: the hold words travel as the commands do."""
    _, _, mixd, embd = clips
    table, _ = schedule()
    ss = net.make_session_streamer(S, DEV, pace=True)
    with no_host_wait():
        y = run_held(ss, table, mixd, embd)
    torch.cuda.synchronize()
    assert ss.faults() == [] and torch.isfinite(y).all()
