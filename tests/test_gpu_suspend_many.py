"""GPU: `SessionStreamer.suspend_many` / `drain` / `resume_many` under graph replay — every listener of a streamer leaves in one
launch as a `SessionSnapshotBatch` and enters another streamer in one launch.  The batched calls claim to be the loop of
`suspend` / `resume`: snapshot bytes and the following chunks are `torch.equal` to a twin that moved its listeners one by one,
and into a paced streamer to the run nobody interrupted.  S = 6; the listeners have consumed 57 chunks when they are parked, so
every ring has wrapped past its 50 rows (position 7).  Idle input rows are NaN.  The host never waits inside the loops."""
import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.net import Net, SessionSnapshotBatch
from oracle import tfgridnet_oracle as O
from tests.test_gpu_suspend import no_host_wait

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP, NFFT = 128, 192
S, BEFORE, AFTER = 6, 57, 8


def make_net(oracle_cfg_sd, dev):
    _cabi.load()
    cfg, sd = oracle_cfg_sd
    n = Net(**O.TSH_PARAMS).eval()
    n.load_state_dict(sd, strict=True)
    return n.to(dev)


@pytest.fixture(scope="module")
def net(oracle_cfg_sd):
    assert torch.cuda.is_available()
    return make_net(oracle_cfg_sd, DEV)


@pytest.fixture(scope="module")
def clips():
    d = synth.batch([90, 91, 92, 93, 94, 95], HOP * (BEFORE + AFTER) + NFFT - HOP)
    return dict(mixd=d["mixture"].to(DEV), embd=d["embedding_gt"][:, 0].to(DEV))


def chunks(clips, plays, k, n=S, dev=DEV):
    """[n, 2, 192]: slot s gets chunk k of clip plays[s], every other row is NaN."""
    x = torch.full((n, 2, NFFT), float("nan"), device=DEV)
    for s, c in plays.items():
        x[s] = clips["mixd"][c, :, k * HOP:k * HOP + NFFT]
    return x.to(dev)


def run(ss, clips, plays, ks, dev=DEV):
    return torch.stack([ss.step(chunks(clips, plays, k, ss.S, dev)).clone() for k in ks])


@pytest.fixture(scope="module")
def plain(net, clips):
    """The run nobody interrupts: listener c plays clip c in slot c of a paced streamer.  [65, 6, 2, 128] on the host"""
    ss = net.make_session_streamer(S, DEV, pace=True)
    for s in range(S):
        ss.open(s, clips["embd"][s])
    out = run(ss, clips, {s: s for s in range(S)}, range(BEFORE + AFTER))
    torch.cuda.synchronize()
    assert ss.faults() == []
    return out.cpu()


@pytest.fixture(scope="module")
def parked(net, clips):
    """Twin paced streamers after 57 chunks of the six listeners: one drained, one suspended slot by slot."""
    twins = [net.make_session_streamer(S, DEV, pace=True) for _ in (0, 1)]
    assert all(t.graphs is not None for t in twins)
    with no_host_wait():
        for t in twins:
            for s in range(S):
                t.open(s, clips["embd"][s])
            run(t, clips, {s: s for s in range(S)}, range(BEFORE))
        slots, batch = twins[0].drain()
        singles = [twins[1].suspend(s) for s in range(S)]
        after = [t.step(chunks(clips, {}, 0)).clone() for t in twins]
    torch.cuda.synchronize()
    assert slots == list(range(S)) and all(t.active == [] and t.faults() == [] for t in twins)
    assert not after[0].any() and not after[1].any()
    return dict(batch=batch, singles=singles)


def test_snapshot_bytes(parked):
    batch, singles = parked["batch"], parked["singles"]
    assert isinstance(batch, SessionSnapshotBatch) and len(batch) == S and batch.data.is_cuda and batch.event is not None
    for i in range(S):
        assert torch.equal(batch[i].data, singles[i].data), i
    assert batch.data[0, 256:272].view(torch.int32).tolist()[2] == BEFORE % 50
    assert batch.data.shape == (S, batch.nbytes) and not torch.equal(batch.data[0], batch.data[1])


PERM = (4, 0, 5, 2, 1, 3)           # listener c resumes in slot PERM[c]


def test_paced_to_paced_continues_bit_for_bit(net, clips, plain, parked):
    t = net.make_session_streamer(S, DEV, pace=True)
    with no_host_wait():
        t.resume_many(PERM, parked["batch"])
        out = run(t, clips, {PERM[c]: c for c in range(S)}, range(BEFORE, BEFORE + AFTER))
    torch.cuda.synchronize()
    assert t.faults() == [] and t.active == list(range(S)) and t._ring[0].tolist() == [(BEFORE + AFTER) % 50] * S
    out = out.cpu()
    for c in range(S):
        assert torch.equal(out[:, PERM[c]], plain[BEFORE:, c]), c
    assert out.abs().amax(dim=(0, 2, 3)).min() > 1e-3


def test_lock_step_target_equals_the_loop_of_resumes(net, clips, parked):
    """Twin lock-step streamers at shared position 3 (saved: 7): every listener's ring is rotated by 46 either way."""
    twins = [net.make_session_streamer(S, DEV) for _ in (0, 1)]
    outs = []
    with no_host_wait():
        for t in twins:
            run(t, clips, {}, range(3))
        twins[0].resume_many(PERM, parked["batch"])
        for c in range(S):
            twins[1].resume(PERM[c], parked["singles"][c])
        for t in twins:
            outs.append(run(t, clips, {PERM[c]: c for c in range(S)}, range(BEFORE, BEFORE + AFTER)))
    torch.cuda.synchronize()
    assert all(t.faults() == [] and t.active == list(range(S)) for t in twins) and twins[0]._gen == twins[1]._gen
    assert torch.equal(outs[0], outs[1]) and outs[0].abs().amax(dim=(0, 2, 3)).min() > 1e-3


def test_compacting_target_takes_three_more(net, clips, parked):
    """row_buckets = (2, 4, 6), two listeners open in rows 0 and 1 (slots 4 and 1); listeners 2, 4 and 5 of the batch — views,
    used in place — take rows 2..4 in slots 0, 5 and 2."""
    batch, singles = parked["batch"], parked["singles"]
    twins = [net.make_session_streamer(S, DEV, pace=True, compact=True, row_buckets=(2, 4, 6)) for _ in (0, 1)]
    plays, outs = {4: 0, 1: 1}, []
    with no_host_wait():
        for t in twins:
            t.open(4, clips["embd"][0]), t.open(1, clips["embd"][1])
            run(t, clips, plays, range(2))
            assert t.rows_in_use == 2 and t.last_rows == 2
        twins[0].resume_many((0, 5, 2), (batch[2], batch[4], batch[5]))
        assert twins[0]._resume_batches[0][0] is batch
        for slot, c in ((0, 2), (5, 4), (2, 5)):
            twins[1].resume(slot, singles[c])
        plays = {**plays, 0: 2, 5: 4, 2: 5}
        for t in twins:
            outs.append(run(t, clips, plays, range(BEFORE, BEFORE + AFTER)))
    torch.cuda.synchronize()
    for t in twins:
        assert t.rows_in_use == 5 and t.last_rows == 6 and t.faults() == [] and t.active == [0, 1, 2, 4, 5]
    assert twins[0]._row_of == twins[1]._row_of == [2, 1, 4, -1, 0, 3]
    assert torch.equal(outs[0], outs[1]) and not outs[0][:, 3].any() and outs[0][:, [0, 2, 5]].abs().amax(dim=(0, 2, 3)).min() > 1e-3


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs 2 GPUs")
def test_batch_moves_to_another_gpu(oracle_cfg_sd, clips, plain, parked):
    """`batch.to(other)`: one copy behind the batch's event; `resume_many` there continues bit for bit."""
    other = "cuda:1"
    net2 = make_net(oracle_cfg_sd, other)
    t = net2.make_session_streamer(S, other, pace=True)
    with no_host_wait():
        there = parked["batch"].to(other)
        assert there.data.device == torch.device(other) and len(there) == S and there.event is not None
        t.resume_many(PERM, there)
        out = run(t, clips, {PERM[c]: c for c in range(S)}, range(BEFORE, BEFORE + AFTER), other)
    torch.cuda.synchronize(other)
    assert t.faults() == [] and t.active == list(range(S))
    out = out.cpu()
    for c in range(S):
        assert torch.equal(out[:, PERM[c]], plain[BEFORE:, c]), c
