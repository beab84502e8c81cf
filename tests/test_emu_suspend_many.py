"""CPU: `SessionStreamer.suspend_many` / `resume_many` / `drain`, `SessionSnapshotBatch` (sessions.py) and their entry points
`lh_session_save_rows` / `lh_session_restore_rows` / `lh_embed_proj_ln_rows` over the emulated library, eager.  The batched forms
claim to be the single forms, many at once: every check here is `torch.equal` against `lh_session_save` / `lh_session_restore` /
`suspend` / `resume` on a twin — bytes, NaN and inf patterns among them.  The hand-made buffers are those of
tests/test_emu_suspend.py; the emulator runs a chunk row in ~0.5 s, so the streamers are small and compacting where they can be."""
import ctypes
from unittest import mock

import pytest
import torch

from lookoncetohear_amd import synth
from lookoncetohear_amd.net import SessionSnapshot, SessionSnapshotBatch
from tests.test_emu_suspend import (A, ARG, CLOSE, HOP, NFFT, OPEN, RESET, SHIFT, V, Bufs, chunk_of, emu_net,  # noqa: F401
                                    no_host_wait, same)

S5 = 5
PAD = 256                                                       # bytes between the layout and the stride


def head(b, k, embed):
    return [A(b.live[k]), 3, A(b.ring_tab), 2, b.HEADS, b.ROWS, b.WIN, embed, b.EMB]


def table(items):
    """[(row, slot, gen, index)] -> lh_snap_item_t[k]"""
    return torch.tensor(items, dtype=torch.int32).reshape(-1, 4)


def blank(k, pad=PAD):
    return torch.full((k, Bufs.SNAP + pad), 0x5a, dtype=torch.uint8)


def save_rows_args(b, k, items, snaps, paced=True):
    pos = [V(b.pos[0]), None] if paced else [None, V(b.shared)]
    return head(b, k, V(b.embed)) + [V(snaps), snaps.stride(0), V(b.words), V(b.words[2])] + pos + \
        [V(items), items.shape[0], b.S, None]


def restore_rows_args(b, k, items, snaps, paced=True):
    pos = [V(b.pos[0]), None] if paced else [None, V(b.shared)]
    return head(b, k, V(b.embed)) + [V(snaps), snaps.stride(0), V(b.words)] + pos + [V(b.fault), V(items), items.shape[0], b.S, None]


def save_rows(b, k, items, snaps, paced=True):
    assert b.lib.raw("lh_session_save_rows")(*save_rows_args(b, k, items, snaps, paced)) == 0


def restore_rows(b, k, items, snaps, paced=True):
    assert b.lib.raw("lh_session_restore_rows")(*restore_rows_args(b, k, items, snaps, paced)) == 0


def save_one(b, k, row, slot, paced=True):
    """lh_session_save of `row`, whose listener's embedding is that of `slot`."""
    snap = torch.full((Bufs.SNAP,), 0x5a, dtype=torch.uint8)
    pos = b.pos[0, row:row + 1] if paced else b.shared
    args = head(b, k, V(b.embed[slot])) + [V(snap), snap.numel(), V(b.words), V(b.words[2]), V(pos), row, b.S, None]
    assert b.lib.raw("lh_session_save")(*args) == 0
    return snap


def restore_one(b, k, row, slot, snap, gen, paced=True):
    pos = [V(b.pos[0, row:row + 1]), None] if paced else [None, V(b.shared)]
    args = head(b, k, V(b.embed[slot])) + [V(snap), snap.numel(), V(b.words)] + pos + \
        [V(b.fault[slot:slot + 1]), gen, row, b.S, None]
    assert b.lib.raw("lh_session_restore")(*args) == 0


def source(lib, positions=(21, 13, 22, 49, 3), active=(3, 7, 4, 9, 6)):
    src = Bufs(lib, S5, seed=1)
    src.words[2] = torch.tensor(active, dtype=torch.int32)
    src.words[1] = torch.tensor([0, RESET, 0, 0, RESET], dtype=torch.int32)
    src.pos[0] = torch.tensor(positions, dtype=torch.int32)
    src.shared[0] = 41
    return src


def target(lib, opens):
    """A differently filled target; `opens`: [(row, gen)] the host has posted an OPEN for."""
    dst = Bufs(lib, S5, seed=2)
    for row, gen in opens:
        dst.words[0, row] = OPEN | (gen << SHIFT)
    dst.words[2] = torch.tensor([5, 6, 8, 2, 1], dtype=torch.int32)
    dst.pos[0] = torch.tensor([1, 2, 3, 4, 5], dtype=torch.int32)
    dst.fault[:] = torch.tensor([90, 91, 92, 93, 94], dtype=torch.int32)
    return dst


# ---- the kernels on hand-made buffers --------------------------------------------------------------------------------------
@pytest.mark.parametrize("paced", [True, False], ids=["paced", "lock_step"])
def test_save_rows_is_save_per_row(emu_net, paced):
    """Rows (3, 1) -> snapshots (0, 1), and all five rows under a slot and an index permutation, stride = layout + 256 into a
    buffer of 0x5a: each snapshot is lh_session_save of that row, the padding is untouched, the source is unchanged."""
    src = source(emu_net.emu_lib)
    before = src.everything()
    for rows, slots, index in (((3, 1), (4, 0), (0, 1)), ((0, 1, 2, 3, 4), (2, 4, 0, 1, 3), (4, 2, 0, 3, 1))):
        snaps = blank(len(rows))
        save_rows(src, 0, table([(r, s, 0, i) for r, s, i in zip(rows, slots, index)]), snaps, paced)
        for r, s, i in zip(rows, slots, index):
            assert torch.equal(snaps[i, :Bufs.SNAP], save_one(src, 0, r, s, paced)), (r, s, i)
        assert (snaps[:, Bufs.SNAP:] == 0x5a).all()
        assert same(src.everything(), before)
    # the words are the row's, the embedding is the slot's, the position the row's own or the shared counter
    words = snaps[1, 256:272].view(torch.int32).tolist()                    # index 1 = row 4, slot 3
    assert words == [6, RESET, 3 if paced else 41, 0]
    assert torch.equal(snaps[1, 272:272 + Bufs.EMB].view(torch.int32), src.embed[3])


def test_restore_rows_paced_is_restore_per_row(emu_net):
    """Two snapshots of a source whose live set is set 0 into rows (0, 4) — slots (3, 1) — of a target whose live set is set
    1, in one launch: everything equals a twin restored by two lh_session_restore calls; rows 1-3, the dead set and the pad rows
    are what they were."""
    lib, H, W = emu_net.emu_lib, Bufs.HEADS, Bufs.WIN
    src = source(lib)
    snaps = blank(2)
    save_rows(src, 0, table([(3, 4, 0, 1), (1, 0, 0, 0)]), snaps)           # snapshot 1 = row 3 (pos 49), 0 = row 1 (pos 13)
    keep = snaps.clone()
    dst, twin = target(lib, [(0, 9), (4, 10)]), target(lib, [(0, 9), (4, 10)])
    was = dst.everything()
    assert same(was, twin.everything())
    restore_rows(dst, 1, table([(0, 3, 9, 1), (4, 1, 10, 0)]), snaps)
    restore_one(twin, 1, 0, 3, snaps[1, :Bufs.SNAP], 9)
    restore_one(twin, 1, 4, 1, snaps[0, :Bufs.SNAP], 10)
    now = dst.everything()
    assert same(now, twin.everything()) and torch.equal(snaps, keep)
    for i in range(3):
        assert torch.equal(dst.sets[1][i][0], src.sets[0][i][3]) and torch.equal(dst.sets[1][i][4], src.sets[0][i][1]), i
        assert torch.equal(dst.sets[1][i][1:4], was[3 + i][1:4]) and torch.equal(dst.sets[0][i], was[i]), i
    for i in range(2):
        assert torch.equal(dst.rings[i][:H, :W], src.rings[i][3 * H:4 * H, :W]), i
        assert torch.equal(dst.rings[i][4 * H:, :W], src.rings[i][H:2 * H, :W]), i
        assert torch.equal(dst.rings[i][:, W:], was[6 + i][:, W:]) and torch.equal(dst.rings[i][H:4 * H], was[6 + i][H:4 * H]), i
    assert torch.equal(dst.embed[3], src.embed[4]) and torch.equal(dst.embed[1], src.embed[0])
    assert torch.equal(dst.embed[[0, 2, 4]], was[8][[0, 2, 4]])
    assert dst.pos.tolist() == [[49, 2, 3, 4, 13], [0] * 5] and dst.shared.tolist() == [0]
    assert dst.words[1].tolist() == [0, 0, 0, 0, RESET] and torch.equal(dst.words[0], was[9][0])
    assert torch.equal(dst.words[2], was[9][2]) and torch.equal(dst.fault, was[12])


@pytest.mark.parametrize("shared", [0, 7, 30])
def test_restore_rows_lock_step_rotates_each_item_by_its_own_delta(emu_net, shared):
    """Saved positions 49 and 3 against one shared position, one launch: item i lands rotated by (shared - saved_i) % 50."""
    lib, H, W = emu_net.emu_lib, Bufs.HEADS, Bufs.WIN
    src = source(lib)
    snaps = blank(2, pad=0)
    save_rows(src, 1, table([(3, 3, 0, 0), (4, 4, 0, 1)]), snaps)           # rows 3 and 4: positions 49 and 3
    dst, twin = target(lib, [(1, 9), (2, 10)]), target(lib, [(1, 9), (2, 10)])
    dst.shared[0] = twin.shared[0] = shared
    was = dst.everything()
    restore_rows(dst, 0, table([(2, 0, 10, 1), (1, 4, 9, 0)]), snaps, paced=False)
    restore_one(twin, 0, 2, 0, snaps[1], 10, paced=False)
    restore_one(twin, 0, 1, 4, snaps[0], 9, paced=False)
    assert same(dst.everything(), twin.everything())
    for row, src_row, saved in ((1, 3, 49), (2, 4, 3)):
        to = [(j + (shared - saved)) % W for j in range(W)]
        for i in range(2):
            assert torch.equal(dst.rings[i][row * H:(row + 1) * H, to], src.rings[i][src_row * H:(src_row + 1) * H, :W]), (row, i)
            assert torch.equal(dst.rings[i][row * H:(row + 1) * H, shared], src.rings[i][src_row * H:(src_row + 1) * H, saved])
    assert dst.shared.tolist() == [shared] and torch.equal(dst.pos, was[10])            # read, never written; no row position


def test_restore_rows_dead_snapshot_between_two_live_ones(emu_net):
    """Only the dead snapshot's row gets CLOSE | RESET, only its slot the fault word — the generation of ITS item."""
    lib = emu_net.emu_lib
    src = source(lib, active=(3, 0, 4, 9, 6))                               # row 1: the device had closed the listener
    snaps = blank(3)
    save_rows(src, 0, table([(0, 0, 0, 0), (1, 1, 0, 1), (2, 2, 0, 2)]), snaps)
    opens = [(0, 11), (2, 12), (4, 13)]
    dst = target(lib, opens)
    was = dst.everything()
    restore_rows(dst, 1, table([(0, 1, 11, 0), (2, 3, 12, 1), (4, 0, 13, 2)]), snaps)
    w = lambda row, gen: OPEN | (gen << SHIFT)
    assert dst.words[0].tolist() == [w(0, 11), 0, CLOSE | RESET, 0, w(4, 13)]
    assert dst.fault.tolist() == [90, 91, 92, 12, 94]
    assert dst.words[1].tolist() == [0, 0, RESET, 0, 0] and torch.equal(dst.words[2], was[9][2])


def test_items_out_of_range_are_skipped_whole(emu_net):
    """CPU only.  Row -1, row S, slot S and index -1 between served neighbours: nothing is read or written for them — the
    result is that of the two valid items alone."""
    lib = emu_net.emu_lib
    src = source(lib)
    before = src.everything()
    for bad in ([(-1, 0, 7, 1), (S5, 1, 7, 1), (2, S5, 7, 1)], [(2, 2, 7, -1), (2, -1, 7, 1), (1 << 30, 2, 7, 1)]):
        snaps = blank(3)
        save_rows(src, 0, table([(3, 4, 0, 0)] + bad + [(1, 0, 0, 2)]), snaps)
        assert torch.equal(snaps[0, :Bufs.SNAP], save_one(src, 0, 3, 4)) and torch.equal(snaps[2, :Bufs.SNAP], save_one(src, 0, 1, 0))
        assert (snaps[1] == 0x5a).all() and (snaps[:, Bufs.SNAP:] == 0x5a).all() and same(src.everything(), before)
        dst, twin = target(lib, [(0, 9), (4, 10)]), target(lib, [(0, 9), (4, 10)])
        restore_rows(dst, 1, table([(0, 3, 9, 0)] + bad + [(4, 1, 10, 2)]), snaps)
        restore_one(twin, 1, 0, 3, snaps[0, :Bufs.SNAP], 9)
        restore_one(twin, 1, 4, 1, snaps[2, :Bufs.SNAP], 10)
        assert same(dst.everything(), twin.everything())


def test_rows_entry_points_validate_arguments(emu_net):
    lib = emu_net.emu_lib
    b = Bufs(lib, S5, seed=3)
    snaps = blank(3)
    items = table([(0, 1, 9, 0), (2, 3, 10, 2)])
    save, restore = lib.raw("lh_session_save_rows"), lib.raw("lh_session_restore_rows")
    s, r = save_rows_args(b, 0, items, snaps), restore_rows_args(b, 0, items, snaps)
    assert save(*s) == 0 and restore(*r) == 0
    sub = lambda a, i, v: a[:i] + [v] + a[i + 1:]
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    for i in (0, 2, 7, 9, 11, 12, 15):                          # every pointer of save but the two positions
        assert save(*sub(s, i, None)) == ARG, i
    for i in (0, 2, 7, 9, 11, 14, 15):                          # ... of restore
        assert restore(*sub(r, i, None)) == ARG, i
    for fn, a, p in ((save, s, 13), (restore, r, 12)):          # p: pos_rows; p + 1: pos_shared
        assert fn(*sub(a, p, None)) == ARG                                              # neither position
        assert fn(*sub(a, p + 1, V(b.shared))) == ARG                                   # both
        assert fn(*sub(sub(a, p, None), p + 1, V(b.shared))) == 0
        n = len(a) - 3                                                                  # n_items
        assert fn(*sub(a, n, 0)) == ARG and fn(*sub(a, n, -1)) == ARG and fn(*sub(a, n, S5 + 1)) == ARG
        assert fn(*sub(a, n + 1, 0)) == ARG and fn(*sub(a, n + 1, 1)) == ARG            # S; n_items = 2 > S = 1
        assert fn(*sub(a, n - 1, off(items, 2))) == ARG                                 # a misaligned table
        assert fn(*sub(a, 10, Bufs.SNAP - 16)) == ARG and fn(*sub(a, 10, Bufs.SNAP + 8)) == ARG     # the stride
        assert fn(*sub(a, 10, Bufs.SNAP)) == 0 and fn(*sub(a, 10, Bufs.SNAP + 16)) == 0
        assert fn(*sub(a, 9, off(snaps, 4))) == ARG and fn(*sub(a, 7, off(b.embed, 8))) == ARG      # unaligned
        for i, wrong in ((1, 0), (1, 33), (3, 0), (3, 9), (4, 0), (6, 0), (6, Bufs.ROWS + 1), (8, 0), (8, 24)):
            assert fn(*sub(a, i, wrong)) == ARG, (i, wrong)                             # what the single forms refuse
    gains = lib.raw("lh_embed_proj_ln_rows")
    f = torch.zeros(8)
    g = [V(f)] * 5 + [V(f), V(torch.zeros(8)), V(items), 2, S5, None]
    for i in range(8):
        assert gains(*sub(g, i, None)) == ARG, i
    assert gains(*sub(g, 6, V(f))) == ARG                                               # scratch == gain
    assert gains(*sub(g, 8, 0)) == ARG and gains(*sub(g, 8, S5 + 1)) == ARG and gains(*sub(g, 9, 0)) == ARG


def test_batched_gains_are_the_per_row_gains(emu_net):
    """lh_embed_proj_ln_rows over nine items — a second batch group of the projection — one of them out of range: rows of the
    first group, its last row and the second group's row hold the bits of `_row_gain`; the row nobody names is not written."""
    ss = emu_net.make_session_streamer(9, "cpu", use_graph=False)
    st = ss._st
    torch.manual_seed(5)
    st.embed.copy_(torch.randn_like(st.embed))
    st.gain.fill_(7.0), st.gain_raw.fill_(7.0)
    pairs = [(4, 8), (8, 0), (0, 7), (9, 1), (7, 2), (2, 6), (6, 1), (1, 3), (3, 5)]        # (row, slot); row 9 is out of range
    emu_net._speaker_gain_rows(st.embed, st.gain_raw, st.gain, torch.tensor([(r, s, 0, 0) for r, s in pairs], dtype=torch.int32))
    got, got_raw = st.gain.clone(), st.gain_raw.clone()
    assert (got[5] == 7.0).all() and (got_raw[5] == 7.0).all()
    assert all(not (got[r] == 7.0).any() for r, _ in pairs if r < 9)
    for row, slot in (pairs[0], pairs[7], pairs[8]):
        st.gain[row].fill_(7.0), st.gain_raw[row].fill_(7.0)
        ss._row_gain(slot, row)
    assert torch.equal(got.view(torch.int32), st.gain.view(torch.int32)) and torch.equal(got_raw, st.gain_raw)


# ---- the host over the emulated device ------------------------------------------------------------------------------------
S = 4


def feed(ss, plays, mix, j):
    """One step: slot s gets chunk j of clip plays[s]; every other row is NaN."""
    x = torch.full((S, 2, NFFT), float("nan"))
    for s, clip in plays.items():
        x[s] = chunk_of(mix[clip], j)
    return ss.step(x).clone()


class Recorder:
    """The names passed to `lib.call` while it is active."""

    def __init__(self, lib):
        self.lib, self.names = lib, []

    def __enter__(self):
        call = self.lib.call
        self._patch = mock.patch.object(self.lib, "call", lambda name, *a: (self.names.append(name), call(name, *a))[1])
        self._patch.start()
        return self.names

    def __exit__(self, *exc):
        self._patch.stop()


@pytest.fixture(scope="module")
def world(emu_net):
    """Listeners A (clip 0) and B (clip 1) run 3 chunks in slots 0 and 2 of twin paced, compacting streamers; one twin parks
    them with `suspend_many((2, 0))`, the other with `suspend(2); suspend(0)`.  Then the batch goes into slots (1, 3) of
    two kinds of target through `resume_many`, and into their twins through `resume` twice, for 3 more chunks."""
    lib = emu_net.emu_lib
    d = synth.batch([20, 21, 22], HOP * 6 + NFFT - HOP)
    mix, emb = d["mixture"], d["embedding_gt"][:, 0]
    make = lambda **kw: emu_net.make_session_streamer(S, "cpu", use_graph=False, **kw)
    r = dict(mix=mix, emb=emb, names={})
    with no_host_wait():
        X = [make(pace=True, compact=True) for _ in (0, 1)]
        for x in X:
            x.open(0, emb[0]), x.open(2, emb[1])
            for j in range(3):
                feed(x, {0: 0, 2: 1}, mix, j)
        with Recorder(lib) as r["names"]["suspend_many", 2]:
            r["batch"] = batch = X[0].suspend_many((2, 0))
            r["x_after"] = [feed(X[0], {}, mix, 3)]
        with Recorder(lib) as r["names"]["suspend"]:
            r["singles"] = singles = [X[1].suspend(2), X[1].suspend(0)]
            r["x_after"].append(feed(X[1], {}, mix, 3))
        r["X"] = X
        # three listeners, for the launch count only: one chunk, parked together, back together
        X3 = make(pace=True, compact=True)
        for s in (0, 1, 3):
            X3.open(s, emb[s % 3])
        feed(X3, {0: 0, 1: 1, 3: 2}, mix, 0)
        with Recorder(lib) as r["names"]["suspend_many", 3]:
            batch3 = X3.suspend_many((3, 0, 1))
            feed(X3, {}, mix, 1)
        with Recorder(lib) as r["names"]["resume_many", 3]:
            X3.resume_many((0, 1, 2), batch3)                   # the listeners of slots 3, 0, 1: clips 2, 0, 1
            y3 = feed(X3, {0: 2, 1: 0, 2: 1}, mix, 1)
        r["three"] = (X3.active, X3.faults(), y3)

        def run(kind, resume, key, **kw):
            """A target of `kind`; `resume(target)` between its set-up and the 3 chunks B (slot 1) and A (slot 3) go on for."""
            t = make(**kw)
            plays = {1: 1, 3: 0}
            if kind == "holes":                                 # slots 0 and 2 hold rows 0 and 1; slot 0 leaves: a hole below
                t.open(0, emb[2]), t.open(2, emb[2])
                feed(t, {0: 2, 2: 2}, mix, 0)
                t.close(0)
                plays[2] = 2
            with Recorder(lib) as names:
                resume(t)
                ys = [feed(t, plays, mix, 3)]
            r["names"].setdefault(key, names)
            ys += [feed(t, plays, mix, j) for j in (4, 5)]
            return dict(t=t, ys=torch.stack(ys), active=t.active, faults=t.faults(), gen=list(t._gen),
                        rows=(list(t._row_of), t.rows_in_use, t.last_rows))

        many = lambda t: t.resume_many((1, 3), batch)
        one = lambda t: (t.resume(1, singles[0]), t.resume(3, singles[1]))
        r["paced"] = [run("fresh", f, key, pace=True, compact=True) for f, key in ((many, ("resume_many", 2)), (one, "resume"))]
        # lock-step: the ring is rotated, the shared position is 1 and the saved ones are 3
        r["holes"] = [run("holes", f, None, compact=True, row_buckets=(3, 4)) for f in (many, one)]
    return r


def test_suspend_many_is_suspend_in_order(world):
    batch, singles, X = world["batch"], world["singles"], world["X"]
    assert isinstance(batch, SessionSnapshotBatch) and len(batch) == 2 and batch.data.dtype == torch.uint8
    assert batch.data.shape == (2, SessionSnapshot.layout_bytes(batch.layout)) and batch.layout == singles[0].layout
    for i in range(2):
        assert torch.equal(batch[i].data, singles[i].data), i
        assert batch[i].data.data_ptr() == batch.data[i].data_ptr() and batch[i].event is batch.event
    assert not torch.equal(batch[0].data, batch[1].data)
    # the same host bookkeeping, the same device words, the same chunk afterwards
    assert X[0].active == X[1].active == [] and X[0]._gen == X[1]._gen and X[0]._pending == X[1]._pending == {}
    assert X[0]._row_of == X[1]._row_of and torch.equal(X[0]._tables, X[1]._tables)
    assert torch.equal(*world["x_after"]) and not world["x_after"][0].any()


@pytest.mark.parametrize("kind", ["paced", "holes"])
def test_resume_many_is_resume_in_order(world, kind):
    many, one = world[kind]
    assert torch.equal(many["ys"], one["ys"])
    for key in ("active", "faults", "gen", "rows"):
        assert many[key] == one[key], key
    assert many["faults"] == [] and many["active"] == ([1, 3] if kind == "paced" else [1, 2, 3])
    assert many["ys"][:, 1].abs().max() > 1e-3 and many["ys"][:, 3].abs().max() > 1e-3 and not many["ys"][:, 0].any()
    if kind == "paced":
        assert many["rows"] == ([-1, 0, -1, 1], 2, 2)
    else:                                                       # the resumes took the hole at row 0 and the new row 2
        assert many["rows"] == ([-1, 0, 1, 2], 3, 3)


def test_launches_do_not_grow_with_k(world):
    n = world["names"]
    assert n["suspend_many", 2] == n["suspend_many", 3] and n["resume_many", 2] == n["resume_many", 3]
    assert n["suspend_many", 2].count("lh_session_save_rows") == 1
    assert n["resume_many", 2].count("lh_session_restore_rows") == 1 and n["resume_many", 2].count("lh_embed_proj_ln_rows") == 1
    assert not {"lh_session_save", "lh_session_restore", "lh_embed_proj_ln"} & set(n["suspend_many", 2] + n["resume_many", 2])
    new = {"lh_session_save_rows", "lh_session_restore_rows", "lh_embed_proj_ln_rows"}
    assert not new & set(n["suspend"] + n["resume"])
    assert n["suspend"].count("lh_session_save") == 2 and n["resume"].count("lh_session_restore") == 2
    active, faults, y3 = world["three"]
    assert active == [0, 1, 2] and faults == [] and y3[:3].abs().amax(dim=(1, 2)).min() > 1e-3 and not y3[3].any()


def test_batch_interop_and_files(emu_net, world, tmp_path):
    """`resume(slot, batch[i])`, `stack` of single snapshots into `resume_many`, views of a batch in any order, a file round trip;
    a batch file is not a single snapshot."""
    batch, singles, mix = world["batch"], world["singles"], world["mix"]
    want = world["paced"][0]["ys"][0]                           # chunk 3 of B in slot 1 and A in slot 3
    path = str(tmp_path / "everyone.lhss")
    batch.save(path)
    back = SessionSnapshotBatch.load(path)
    assert len(back) == 2 and back.layout == batch.layout and torch.equal(back.data, batch.data) and back.event is None
    with pytest.raises(ValueError):
        SessionSnapshot.load(path)
    stacked = SessionSnapshotBatch.stack(singles)
    assert torch.equal(stacked.data, batch.data) and stacked.to("cpu") is stacked and stacked.cpu() is stacked
    with pytest.raises(ValueError):
        SessionSnapshotBatch.stack([])
    single_path = str(tmp_path / "one.lhss")
    batch[1].save(single_path)
    assert torch.equal(SessionSnapshot.load(single_path).data, singles[1].data)
    assert len(SessionSnapshotBatch.load(single_path)) == 1
    resumes = (lambda t: (t.resume(1, batch[0]), t.resume_many((3,), (batch[1],))),     # a view alone; a view of a batch: in place
               lambda t: (t.resume_many((1,), (singles[0],)), t.resume_many([3], (back[1],))))     # stacked first; from the file
    for i, resume in enumerate(resumes):
        t = emu_net.make_session_streamer(S, "cpu", use_graph=False, pace=True, compact=True)
        resume(t)
        if i == 0:
            assert len(t._resume_batches) == 1 and t._resume_batches[0][0] is batch
        assert torch.equal(feed(t, {1: 1, 3: 0}, mix, 3), want), i
        assert t.active == [1, 3] and not t._resumes and not t._resume_batches


def test_all_or_nothing(emu_net, world):
    """A slot that is idle, named twice or not yet served refuses the whole `suspend_many`; an open slot, a slot named twice or a
    snapshot of another layout the whole `resume_many`: device words and host state are what they were."""
    t = world["paced"][0]["t"]                                  # slots 1 and 3 open, 0 and 2 idle
    state = lambda: (list(t._gen), dict(t._pending), dict(t._resumes), list(t._resume_batches), t._next_gen, t.active,
                     list(t._row_of), t._tables.clone(), t._ring.clone(), t._st.embed.clone())
    eq = lambda a, b: all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(a, b))
    was = state()
    calls = Recorder(emu_net.emu_lib)
    with calls as names:
        for slots in ((1, 0), (1, 3, 1), (3, 4)):
            with pytest.raises((ValueError, IndexError)):
                t.suspend_many(slots)
        batch = world["batch"]
        other = SessionSnapshot(batch[0].data[:-16], batch.layout[:-1] + (batch.layout[-1] - 16,))
        for slots, snaps in (((0, 1), batch), ((0, 0), batch), ((0,), batch), ((0, 2), (batch[0], other)), ((0, 4), batch)):
            with pytest.raises((ValueError, IndexError)):
                t.resume_many(slots, snaps)
        assert t.suspend_many(()).data.shape[0] == 0 and t.resume_many((), ()) is None
    assert names == [] and eq(state(), was)
    t.resume_many((0, 2), batch)
    with pytest.raises(ValueError):
        t.suspend_many((1, 0))                                  # slot 0: resumed, no step has served it yet
    t.set_embedding(2, world["emb"][2])
    t.close(0)                                                  # resumed and closed before a step: not restored
    with calls as names:
        y = feed(t, {1: 1, 2: 0, 3: 0}, world["mix"], 5)
    assert names.count("lh_session_restore_rows") == 1 and names.count("lh_embed_proj_ln_rows") == 1
    assert t.active == [1, 2, 3] and not y[0].any() and y[2].abs().max() > 1e-3
    assert torch.equal(t._st.embed[2], world["emb"][2])         # `set_embedding` after `resume_many` wins over the snapshot's
    slots, everyone = t.drain()
    assert slots == [1, 2, 3] and len(everyone) == 3 and t.active == []
