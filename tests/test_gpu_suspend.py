"""GPU: `SessionStreamer.suspend` / `resume` under graph replay — a listener's state leaves the streamer as a `SessionSnapshot`
and enters another slot, another streamer, or comes back from host memory.  In a paced streamer the listener's output goes on
bit for bit (`torch.equal` against the run without the traffic, across the 50-row ring wrap); a lock-step target rotates the
ring, which is bit-identical when the shared position equals the saved one and otherwise within the tolerance of a listener
opened at an arbitrary shared position: the float64 oracle over their OWN samples from the zero state, TOL as in
tests/test_gpu_pace.py / tests/test_gpu_sessions.py.  Idle and held input rows are NaN throughout.  The NaN of the fault case
is ordinary input data for lh_session_begin_paced and runs once."""
import contextlib
from unittest import mock

import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.net import Net, SessionSnapshot
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
    """Four listeners: mix [4, 2, 128 * 120 + 64], target alike and emb [4, 256] on the host; mix and emb on the device."""
    d = synth.batch([80, 81, 82, 83], HOP * N_CLIP + NFFT - HOP)
    mix, emb = d["mixture"], d["embedding_gt"][:, 0]
    return dict(mix=mix, emb=emb, tgt=d["target"], mixd=mix.to(DEV), embd=emb.to(DEV))


@pytest.fixture(scope="module")
def plain(net, clips):
    """Every listener's clip without any traffic: all four opened before the first chunk of one paced streamer.
    [4, 2, 128 * 120]"""
    ss = net.make_session_streamer(S, DEV, pace=True)
    for s in range(S):
        ss.open(s, clips["embd"][s])
    outs = [ss.step(clips["mixd"][:, :, i * HOP:i * HOP + NFFT]).clone() for i in range(N_CLIP)]
    torch.cuda.synchronize()
    assert ss.faults() == []
    return torch.cat(outs, -1).cpu()


@pytest.fixture(scope="module")
def lock_plain(net, clips):
    """The uninterrupted lock-step run of clips 0..2, all opened before the first chunk.  [3, 2, 128 * 120]"""
    ss = net.make_session_streamer(3, DEV)
    for s in range(3):
        ss.open(s, clips["embd"][s])
    outs = [ss.step(clips["mixd"][:3, :, i * HOP:i * HOP + NFFT]).clone() for i in range(N_CLIP)]
    torch.cuda.synchronize()
    assert ss.faults() == []
    return torch.cat(outs, -1).cpu()


@pytest.fixture(scope="module")
def fresh64(oracle_cfg_sd, clips):
    """float64 oracle output of each clip as a stream that starts from the zero state (tests/test_gpu_pace.py), computed once."""
    cfg, sd = oracle_cfg_sd
    return [O.predict(cfg, sd, clips["mix"][c][None], clips["emb"][c][None], None, pad=False, dtype=torch.float64,
                      fast_lstm=True)[0][0] for c in range(S)]


@contextlib.contextmanager
def no_host_wait():
    def refuse(*a, **k):
        raise AssertionError("the host waited for the device inside the chunk loop")
    with mock.patch.object(torch.cuda, "synchronize", refuse), mock.patch.object(torch.cuda.Stream, "synchronize", refuse), \
            mock.patch.object(torch.cuda.Event, "synchronize", refuse):
        yield


def chunk(clips, c, k):
    return clips["mixd"][c, :, k * HOP:k * HOP + NFFT]


def nan_rows(n):
    return torch.full((n, 2, NFFT), float("nan"), device=DEV)


# ---- paced: bit for bit across the ring wrap and across objects ----------------------------------------------------------
SUSPEND_AFTER = (24, 56)        # listener 0 has consumed chunks 0..23 / 0..55: before and past the 50-row wrap (position 6)
AWAY = 3                        # steps between a suspend and the resume
HELD = {0: {30, 64}, 1: {24, 27, 40, 59, 65}, 3: {62, 63}}      # by step, while the listener is in a streamer


def run_moves(net, clips, via, guard=contextlib.nullcontext):
    """Listener c plays clip c.  A (S = 4, paced): listeners 0 and 1 from step 0, listener 2 from step 5 to step 70.
    B (S = 2, paced and compacting): listener 3 from step 0.  Listener 0 is suspended twice and resumes AWAY steps later, first
    in A's slot 3, then in B's slot 1; `via` is what happens to the snapshot in between.  The loop runs under `guard()` and
    waits for the device only where `via` does.  -> every listener's concatenated rows, every output row of A and of B by
    step, the chunks consumed"""
    A, B = net.make_session_streamer(S, DEV, pace=True), net.make_session_streamer(2, DEV, pace=True, compact=True)
    assert A.graphs is not None and B.graphs is not None
    embd = clips["embd"]
    A.open(0, embd[0]), A.open(1, embd[1]), B.open(0, embd[3])
    where = {0: (A, 0), 1: (A, 1), 3: (B, 0)}
    took, mine, rows_a, rows_b, done, snap, back_at = [0] * S, [[] for _ in range(S)], [], [], [], None, -1
    with guard():
        for i in range(400):
            if 0 in where and took[0] in SUSPEND_AFTER and took[0] not in done:
                ss, slot = where.pop(0)
                snap, back_at = ss.suspend(slot), i + AWAY
                done.append(took[0])
                assert slot not in ss.active
            elif 0 not in where and i == back_at:
                where[0] = (A, 3) if len(done) == 1 else (B, 1)
                where[0][0].resume(where[0][1], via(snap))
            if i == 5:
                A.open(2, embd[2])
                where[2] = (A, 2)
            if i == 70:
                A.close(2)
                del where[2]
            x, present, plays = {A: nan_rows(S), B: nan_rows(2)}, {A: [True] * S, B: [True] * 2}, []
            for c, (ss, slot) in where.items():
                if i in HELD.get(c, ()) or took[c] == N_CLIP:
                    present[ss][slot] = False
                else:
                    x[ss][slot] = chunk(clips, c, took[c])
                    took[c] += 1
                    plays.append((c, ss, slot))
            y = {A: A.step(x[A], present[A]).clone(), B: B.step(x[B], present[B]).clone()}
            for c, ss, slot in plays:
                mine[c].append(y[ss][slot])
            rows_a.append(y[A]), rows_b.append(y[B])
            if took[0] == N_CLIP:
                break
    return dict(A=A, B=B, mine=[torch.cat(m, -1) for m in mine], rows_a=torch.stack(rows_a), rows_b=torch.stack(rows_b),
                took=took, steps=i + 1, done=done)


def check_moves(r, plain):
    A, B, took = r["A"], r["B"], r["took"]
    assert A.faults() == [] and B.faults() == [] and A.active == [1] and B.active == [0, 1]
    assert r["done"] == list(SUSPEND_AFTER) and took[0] == N_CLIP and took[2] == 65 and r["steps"] == N_CLIP + 2 * AWAY + 2
    assert B._ring[0].tolist() == [took[3] % 50, took[0] % 50] and B.rows_in_use == 2
    for c in range(S):
        got = r["mine"][c].cpu()
        assert got.shape[-1] == took[c] * HOP and torch.equal(got, plain[c, :, :took[c] * HOP]), c
    ra, rb = r["rows_a"].cpu(), r["rows_b"].cpu()
    assert not ra[SUSPEND_AFTER[0]:, 0].any()                   # A's slot 0 from the suspend on: idle as after close
    first_back = SUSPEND_AFTER[0] + AWAY
    assert not ra[:first_back, 3].any() and ra[first_back, 3].any() and not ra[-50:, 3].any() and not rb[:50, 1].any()


def test_paced_listener_moves_bit_for_bit(net, clips, plain):
    r = run_moves(net, clips, lambda snap: snap, no_host_wait)
    torch.cuda.synchronize()
    check_moves(r, plain)


def test_snapshot_through_host_memory(net, clips, plain):
    """snapshot.cpu() -> .to(DEV) -> resume: the same bits."""
    seen = []

    def via(snap):
        host = snap.cpu()
        assert not host.data.is_cuda and host.event is None and host.layout == snap.layout
        back = host.to(DEV)
        assert back.data.is_cuda and back.event is not None and back.to(DEV) is back
        seen.append(torch.equal(back.data, snap.data))
        return back
    r = run_moves(net, clips, via)
    torch.cuda.synchronize()
    assert seen == [True, True]
    check_moves(r, plain)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs 2 GPUs")
def test_snapshot_through_another_gpu(net, clips, plain):
    """Device to device and back, every copy ordered by events: the host never waits."""
    r = run_moves(net, clips, lambda snap: snap.to("cuda:1").to(DEV), no_host_wait)
    torch.cuda.synchronize()
    check_moves(r, plain)


# ---- lock-step targets: the ring is rotated ---------------------------------------------------------------------------------
N_LOCK = 70                     # chunks of the moved listener


def lock_step_run(net, clips, resume_at):
    """S = 3, pace=False: clips 0 and 1 in slots 0 and 1 from step 0; slot 1's listener is suspended when 30 steps are done and
    resumes in slot 2 when `resume_at` are.  -> the listener's N_LOCK chunks, slot 0's rows"""
    ss = net.make_session_streamer(3, DEV)
    ss.open(0, clips["embd"][0]), ss.open(1, clips["embd"][1])
    where, took, mine, other, snap = 1, 0, [], [], None
    with no_host_wait():
        for i in range(resume_at + N_LOCK - 30):
            if i == 30:
                snap, where = ss.suspend(1), None
            if i == resume_at:
                ss.resume(2, snap)
                where = 2
            x = nan_rows(3)
            x[0] = chunk(clips, 0, i)
            if where is not None:
                x[where] = chunk(clips, 1, took)
            y = ss.step(x).clone()
            other.append(y[0])
            if where is not None:
                mine.append(y[where])
                took += 1
            else:
                assert ss.active == [0]
    torch.cuda.synchronize()
    assert took == N_LOCK and ss.faults() == [] and ss.active == [0, 2] and int(ss._st.pos) == (resume_at + N_LOCK - 30) % 50
    return torch.cat(mine, -1).cpu(), torch.cat(other, -1).cpu()


def check_against_oracle(name, got, clips, fresh64, c, n):
    ref = fresh64[c][:, :n * HOP]
    e = float((got.double() - ref).abs().max())
    mix, tgt = clips["mix"][c][None, :, :n * HOP].double(), clips["tgt"][c][None, :, :n * HOP].double()
    dsi = float((O.si_snr_i(got[None].double(), mix, tgt) - O.si_snr_i(ref[None], mix, tgt)).abs())
    print(f"{name}: max|hip - fp64 fresh stream| = {e:.2e}, |dSI-SNRi| = {dsi:.2e} dB over {n} chunks")
    return e, dsi


def test_lock_step_same_position_is_bit_identical(net, clips, lock_plain):
    """Suspended with 30 steps done, resumed with 80: delta = 50 = 0 (mod 50), the ring rows go back where they were."""
    mine, other = lock_step_run(net, clips, 80)
    assert torch.equal(mine, lock_plain[1, :, :N_LOCK * HOP])
    assert torch.equal(other, lock_plain[0, :, :other.shape[-1]])


def test_lock_step_other_position_is_within_tolerance(net, clips, lock_plain, fresh64):
    """Resumed with 67 steps done: the ring rows are rotated by 37, the listener's oldest row is the next one overwritten."""
    mine, other = lock_step_run(net, clips, 67)
    assert torch.equal(other, lock_plain[0, :, :other.shape[-1]])
    e, dsi = check_against_oracle("lock-step, delta 37", mine, clips, fresh64, 1, N_LOCK)
    assert e <= TOL and dsi < 0.05, (e, dsi)


def test_transfers_between_paced_and_lock_step(net, clips, fresh64):
    """P (S = 2, paced) and L (S = 3, lock-step, clip 0 in slot 0 throughout) step together.  Clip 2's listener starts in P and
    moves to L (saved position 30, shared position 41: rotated by 11); clip 3's starts in L and moves to P, which takes the
    rows as they are with position 30.  Both are suspended with 30 steps done."""
    P, L = net.make_session_streamer(2, DEV, pace=True), net.make_session_streamer(3, DEV)
    embd = clips["embd"]
    P.open(0, embd[2]), L.open(0, embd[0]), L.open(2, embd[3])
    where, took, mine, snaps = {2: (P, 0), 3: (L, 2)}, {2: 0, 3: 0}, {2: [], 3: []}, {}
    with no_host_wait():
        for i in range(41 + N_LOCK - 30):
            if i == 30:
                for c in (2, 3):
                    ss, slot = where.pop(c)
                    snaps[c] = ss.suspend(slot)
            if i == 37:
                P.resume(1, snaps[3])
                where[3] = (P, 1)
            if i == 41:
                L.resume(1, snaps[2])
                where[2] = (L, 1)
            x, present, plays = {P: nan_rows(2), L: nan_rows(3)}, [True, True], []
            x[L][0] = chunk(clips, 0, i)
            for c, (ss, slot) in where.items():
                if took[c] < N_LOCK:
                    x[ss][slot] = chunk(clips, c, took[c])
                    took[c] += 1
                    plays.append((c, ss, slot))
                else:                                           # the listener in P is through: held, not fed NaN
                    assert ss is P
                    present[slot] = False
            y = {P: P.step(x[P], present).clone(), L: L.step(x[L]).clone()}
            for c, ss, slot in plays:
                mine[c].append(y[ss][slot])
    torch.cuda.synchronize()
    assert P.faults() == [] and L.faults() == [] and took == {2: N_LOCK, 3: N_LOCK}
    assert P.active == [1] and L.active == [0, 1] and int(P._ring[0, 1]) == N_LOCK % 50
    for c, name in ((2, "paced -> lock-step"), (3, "lock-step -> paced")):
        e, dsi = check_against_oracle(name, torch.cat(mine[c], -1).cpu(), clips, fresh64, c, N_LOCK)
        assert e <= TOL, (name, e)


# ---- compaction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pace", [True, False], ids=["paced", "lock_step"])
def test_suspend_and_resume_under_compaction(net, clips, plain, fresh64, pace):
    """S = 8, compact=True.  Slots 0..4 play clips 0, 1, 2, 3, 0 from step 0.  Step 10 suspends slots 1 and 3: three rows are
    left and the survivor of row 4 moves down.  Step 15 opens slots 5, 6, 7 (clips 1, 2, 3).  Step 20 closes slots 0, 2 and 4
    and resumes the two listeners in each other's slots: the survivor of row 5 moves into one hole, the resumes take the
    others, in one step.  Paced, everyone's bits are those without the traffic; lock-step, a listener that was opened late or
    resumed at another shared position is within the oracle tolerance instead."""
    S8, n = 8, 36
    ss = net.make_session_streamer(S8, DEV, compact=True, pace=pace)
    assert ss.row_buckets == (1, 2, 4, 8)
    embd = clips["embd"]
    sessions = {s: [c, 0, 0, True] for s, c in enumerate([0, 1, 2, 3, 0])}      # slot -> clip, first own chunk, took, exact
    streams, snaps, seen = [], {}, {}
    with no_host_wait():
        for s, (c, *_) in sessions.items():
            ss.open(s, embd[c])
        for i in range(n):
            if i == 10:
                for s in (1, 3):
                    snaps[s] = ss.suspend(s)
                    streams.append(sessions.pop(s))
            if i == 15:
                for s, c in ((5, 1), (6, 2), (7, 3)):
                    ss.open(s, embd[c])
                    sessions[s] = [c, 0, 0, pace]
            if i == 20:
                for s in (0, 2, 4):
                    ss.close(s)
                    streams.append(sessions.pop(s))
                for s, was in ((1, 3), (3, 1)):
                    ss.resume(s, snaps[was])
                    sessions[s] = [was, 10, 10, pace]             # slots 1 and 3 played clips 1 and 3
            x = nan_rows(S8)
            for s, v in sessions.items():
                x[s] = chunk(clips, v[0], v[2])
                v[2] += 1
            y = ss.step(x).clone()
            for s, v in sessions.items():
                v.append(y[s])
            idle = [s for s in range(S8) if s not in sessions]
            seen[i] = (ss.rows_in_use, ss.last_rows, list(ss._row_of), y[idle])
    torch.cuda.synchronize()
    assert ss.faults() == [] and ss.active == [1, 3, 5, 6, 7]
    assert seen[9][:3] == (5, 8, [0, 1, 2, 3, 4, -1, -1, -1])
    assert seen[10][:3] == (3, 4, [0, -1, 2, -1, 1, -1, -1, -1])                # rows_in_use drops, last_rows follows the bucket
    assert seen[15][:3] == (6, 8, [0, -1, 2, -1, 1, 3, 4, 5])
    assert seen[20][:3] == (5, 8, [-1, 1, -1, 2, -1, 3, 4, 0])                  # row 5 -> 0 and two resumes in one step
    assert all(not v[3].any() for v in seen.values())
    # the suspended listeners' first ten chunks, then everyone who was there at the end or left on the way
    rows = [(v[:4], v[4:]) for v in sessions.values()] + [(v[:4], v[4:]) for v in streams]
    assert len(rows) == 10
    for (c, k0, k1, exact), ys in rows:
        got = torch.cat(ys, -1).cpu()
        assert got.shape[-1] == (k1 - k0) * HOP
        if exact:
            assert torch.equal(got, plain[c, :, k0 * HOP:k1 * HOP]), (c, k0, k1)
        elif k0 == 0:
            e = float((got.double() - fresh64[c][:, :k1 * HOP]).abs().max())
            print(f"lock-step, clip {c} opened at step 15: max|hip - fp64 fresh stream| = {e:.2e}")
            assert e <= TOL, (c, e)
        else:                                                   # resumed at shared position 20 with position 10 saved
            head = plain[c, :, :k0 * HOP]                       # their first ten chunks were checked bit for bit above
            e = float((torch.cat([head, got], -1).double() - fresh64[c][:, :k1 * HOP]).abs().max())
            print(f"lock-step, clip {c} resumed with delta 10: max|hip - fp64 fresh stream| = {e:.2e}")
            assert e <= TOL, (c, e)


@pytest.mark.parametrize("leave", ["suspend", "close"])
def test_same_slot_resume_in_a_step_that_moves_rows(net, clips, plain, leave):
    """S = 4, paced and compacting, rows 0..3 = slots 0..3: clip 1 twice as fillers, clip 2 in slot 2, clip 0 in slot 3 — the top
    row.  Clip 0's listener is suspended with 30 chunks done and slot 3 serves clip 3's for five steps.  Then ONE step closes
    both fillers, takes clip 3's listener out of slot 3 (`leave`) and resumes clip 0's in the same slot.  The previous
    listener's row is given up, not moved over the restored one; the survivor of row 2 moves to row 0 and the resume takes
    the hole at row 1.  Everyone has the bits of the run without the traffic."""
    n, away = 60, 5
    ss = net.make_session_streamer(S, DEV, pace=True, compact=True)
    embd = clips["embd"]
    for s, c in enumerate([1, 1, 2, 0]):
        ss.open(s, embd[c])
    outs, rows = [], {}
    with no_host_wait():
        for i in range(n + away):
            if i == 30:
                snap = ss.suspend(3)
                ss.open(3, embd[3])
            if i == 30 + away:
                ss.close(0), ss.close(1)
                ss.suspend(3) if leave == "suspend" else ss.close(3)
                ss.resume(3, snap)
            x = nan_rows(S)
            x[2] = chunk(clips, 2, i)
            if i < 30 + away:
                x[0] = x[1] = chunk(clips, 1, i)
            x[3] = chunk(clips, 0, i) if i < 30 else chunk(clips, 3, i - 30) if i < 30 + away else chunk(clips, 0, i - away)
            outs.append(ss.step(x).clone())
            rows[i] = (list(ss._row_of), ss.rows_in_use, ss.last_rows)
    torch.cuda.synchronize()
    y = torch.stack(outs).cpu()
    assert ss.faults() == [] and ss.active == [2, 3]
    assert rows[30 + away - 1] == ([0, 1, 2, 3], 4, 4) and rows[30 + away] == ([-1, -1, 0, 1], 2, 2)
    cat = lambda s, steps: torch.cat([y[i, s] for i in steps], -1)
    mine = [i for i in range(n + away) if not 30 <= i < 30 + away]
    assert torch.equal(cat(3, mine), plain[0, :, :n * HOP])
    assert torch.equal(cat(3, range(30, 30 + away)), plain[3, :, :away * HOP])
    assert torch.equal(cat(2, range(n + away)), plain[2, :, :(n + away) * HOP])
    assert torch.equal(cat(0, range(30 + away)), plain[1, :, :(30 + away) * HOP]) and not y[30 + away:, :2].any()


# ---- a fault in flight ----------------------------------------------------------------------------------------------------
def test_fault_in_flight_makes_a_dead_snapshot(net, clips, plain):
    """Slots 0..2 of a paced S = 4 streamer play clips 0..2.  Slot 1's chunk 20 holds a NaN and `suspend(1)` follows at once,
    with no poll in between: the device closes the listener, the host has not seen it.  Resumed in slot 3, the snapshot stays
    dead: slot 3 is in `faults()` after that step with zero output, nobody else changes a bit, and `open(3)` works at once."""
    n, bad_at, reopen_at = 40, 20, 22
    ss = net.make_session_streamer(S, DEV, pace=True)
    embd = clips["embd"]
    for s in range(3):
        ss.open(s, embd[s])
    outs = []

    def steps(lo, hi):
        for i in range(lo, hi):
            if i == bad_at + 1:
                # The scenario needs the host NOT to have seen step 20's fault word yet (`suspend` wants a slot in `active`,
                # which reads the pinned word in place).  That word is the last store of the last node of step 20's graph,
                # 0.26 ms of device work after the replay was enqueued a few host instructions ago, behind whatever is still
                # queued; a host stalled for that long right here would make `suspend` raise ValueError instead.
                snap = ss.suspend(1)
                ss.resume(3, snap)
                assert ss.active == [0, 2, 3]
            x = nan_rows(S)
            x[0], x[2] = chunk(clips, 0, i), chunk(clips, 2, i)
            if i <= bad_at:
                x[1] = chunk(clips, 1, i)
            if i == bad_at:
                x[1, 1, 100] = float("nan")
            if i == bad_at + 1:
                x[3] = chunk(clips, 1, i)                       # what the moved listener's client goes on sending
            if i >= reopen_at:
                x[3] = chunk(clips, 3, i - reopen_at)
            outs.append(ss.step(x).clone())
    with no_host_wait():
        steps(0, reopen_at)
    torch.cuda.synchronize()
    assert ss.faults() == [3] and ss.active == [0, 2] and not outs[-1][3].any() and not outs[-1][1].any()
    ss.open(3, embd[3])                                         # no close, no poll
    with no_host_wait():
        steps(reopen_at, n)
    torch.cuda.synchronize()
    y = torch.stack(outs).cpu()
    assert ss.faults() == [] and ss.active == [0, 2, 3] and torch.isfinite(y).all()
    cat = lambda s, rows: torch.cat([y[i, s] for i in rows], -1)
    assert torch.equal(cat(0, range(n)), plain[0, :, :n * HOP]) and torch.equal(cat(2, range(n)), plain[2, :, :n * HOP])
    assert torch.equal(cat(1, range(bad_at)), plain[1, :, :bad_at * HOP]) and not y[bad_at:, 1].any()
    assert not y[:reopen_at, 3].any()                           # the dead snapshot never sounds
    assert torch.equal(cat(3, range(reopen_at, n)), plain[3, :, :(n - reopen_at) * HOP])


def test_dead_snapshot_is_reported(net, clips):
    """The same, looked at after the step that served the resume: the slot is listed by `faults()`, `close` acknowledges it."""
    ss = net.make_session_streamer(S, DEV, pace=True)
    ss.open(1, clips["embd"][1])
    for i in range(12):
        x = nan_rows(S)
        x[1] = chunk(clips, 1, i)
        if i == 11:
            x[1, 0, 0] = float("inf")
        ss.step(x)
    snap = ss.suspend(1)
    assert isinstance(snap, SessionSnapshot) and snap.data.numel() == ss._snap_bytes and 5.3e6 < ss._snap_bytes < 5.5e6
    ss.resume(2, snap)
    y = ss.step(nan_rows(S)).clone()
    torch.cuda.synchronize()
    assert ss.faults() == [2] and ss.active == [] and not y.any()
    assert snap.cpu().data[256:268].view(torch.int32).tolist()[:2] == [0, 0]                # active, cmd[1]: dead, nothing pending
    ss.close(2)
    ss.resume(2, snap)                                          # a value: again, with the same end
    ss.step(nan_rows(S))
    torch.cuda.synchronize()
    assert ss.faults() == [2]
