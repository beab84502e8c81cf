"""GPU: the monitor mix under graph replay — `lh_session_mix` as a node of the captured chunk, `enroll(..., passthrough=True)`
and `relook` beside the running loop — while the host never waits: during the step loops `torch.cuda.synchronize`,
`Stream.synchronize` and `Event.synchronize` raise.  Every claim is `torch.equal` or a bit comparison: the entry point against
the numpy-fp32 restatement of tests/monitor_cases.py, a graph streamer against an EAGER twin on the same device that is told
by hand, at the same steps, what enrollment did on its own (the step an embedding arrives at is the side stream's business,
so the loop records it and the twin repeats it).  The loops end when the slot has opened or re-targeted; their cap is a
condition, not a measurement.  Nothing here times anything."""
import contextlib
from unittest import mock

import pytest
import torch

from lookoncetohear_amd import _cabi
from lookoncetohear_amd.net import Net
from tests import monitor_cases as C
from oracle import tfgridnet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP, NFFT = C.HOP, C.NFFT
S, N_ENROLL, CAP, TAIL, RAMP = 3, 3, 2000, 4, 256


@pytest.fixture(scope="module")
def net(oracle_cfg_sd):
    assert torch.cuda.is_available()
    _cabi.load()
    cfg, sd = oracle_cfg_sd
    n = Net(**O.TSH_PARAMS).eval()
    n.load_state_dict(sd, strict=True)
    return n.to(DEV)


@pytest.fixture(scope="module")
def feed():
    """streams [S, 2, 128 (CAP + TAIL + 1) + 64] and one embedding per slot."""
    g = torch.Generator(device=DEV).manual_seed(12)
    streams = 0.1 * torch.randn(S, 2, HOP * (CAP + TAIL + 1) + NFFT - HOP, device=DEV, generator=g)
    return streams, torch.randn(S, 256, device=DEV, generator=g)


@contextlib.contextmanager
def no_host_wait():
    def refuse(*a, **k):
        raise AssertionError("the host waited for the device inside the chunk loop")
    with mock.patch.object(torch.cuda, "synchronize", refuse), mock.patch.object(torch.cuda.Stream, "synchronize", refuse), \
            mock.patch.object(torch.cuda.Event, "synchronize", refuse):
        yield


def chunk(streams, i):
    return streams[:, :, i * HOP:i * HOP + NFFT].contiguous()


class FakeEmbed:
    """The first 256 samples of the clip's left channel: device work on the side stream, like the embedder's."""

    def __init__(self):
        self.calls = 0

    def __call__(self, x):
        self.calls += 1
        return x[:, 0, :256].contiguous()


@pytest.mark.parametrize("ramp", [100, 256])
def test_mix_entry_point_equals_the_restatement_on_the_device(ramp):
    """The compiled kernel, contraction and all: every sample and gain word of three slots on three trajectories."""
    lib = _cabi.load()
    C.run_trajectory(lib, 3, ramp, ["reversed", "up", "down"], device=DEV, seed=ramp)
    m = C.Mix(lib, 3, ramp, DEV, paced=True, seed=1)
    for s in range(3):
        m.post(s, 0.0, 1.0)
    got, want = m.call(held=(1,))
    assert C.same_bits(got, want) and m.gains_match()


def test_passthrough_enroll_under_graph_replay_equals_the_eager_twin(net, feed):
    """Slot 0 is open, slot 2 is idle at (0, 0.5), slot 1 enrolls with pass-through at step 1: the room, then the cross-fade
    into the target from the step that opens it."""
    streams, emb = feed
    ss = net.make_session_streamer(S, DEV, enroll_chunks=N_ENROLL, monitor=True, monitor_ramp=RAMP)
    assert ss.graphs is not None
    ss.open(0, emb[0])
    ss.set_mix(2, 0.0, 0.5)
    e, outs, opened = FakeEmbed(), [], None
    with no_host_wait():
        for i in range(CAP + TAIL):
            if i == 1:
                ss.enroll(1, e, passthrough=True)
            outs.append(ss.step(chunk(streams, i)).clone())
            if opened is None and 1 in ss.active:
                opened = i                       # the step whose poll opened it, and posted (1, 0) with the OPEN
            assert ss.faults() == []
            if opened is not None and i == opened + TAIL:
                break
    torch.cuda.synchronize()
    n = len(outs)
    print("slot 1 opened at step", opened, "of", n)
    assert opened is not None and opened < CAP and opened >= 1 + N_ENROLL and e.calls == 1
    assert ss.mix_of(1) == (1.0, 0.0) and ss.active == [0, 1]
    y = torch.stack(outs)
    assert torch.isfinite(y).all() and torch.equal(ss._clips[1], streams[1, :, HOP:HOP * (1 + N_ENROLL)])
    # once the ramp of two chunks has arrived and until the opening: the listener's own input, sample for sample
    for i in range(3, opened):
        assert torch.equal(y[i, 1], chunk(streams, i)[1, :, :HOP] + 0.0), i
    assert not torch.equal(y[n - 1, 1], chunk(streams, n - 1)[1, :, :HOP] + 0.0) and y[n - 1, 1].any()
    assert torch.equal(y[3, 2], (chunk(streams, 3)[2, :, :HOP] * 0.5) + 0.0)
    twin = net.make_session_streamer(S, DEV, use_graph=False, monitor=True, monitor_ramp=RAMP)
    twin.open(0, emb[0])
    twin.set_mix(2, 0.0, 0.5)
    for i in range(n):
        if i == 1:
            twin.set_mix(1, 0.0, 1.0)
        if i == opened:
            twin.open(1, ss.embedding_of(1))
            twin.set_mix(1, 1.0, 0.0)
        assert torch.equal(twin.step(chunk(streams, i)), y[i]), i
    torch.cuda.synchronize()
    assert torch.equal(twin._mix, ss._mix)


def test_relook_under_graph_replay_equals_the_eager_twin(net, feed):
    """Slots 0 and 2 are open; slot 0 looks again at step 2 and is re-targeted when its embedding arrives."""
    streams, emb = feed
    ss = net.make_session_streamer(S, DEV, enroll_chunks=N_ENROLL)
    ss.open(0, emb[0]), ss.open(2, emb[2])
    e, outs, done = FakeEmbed(), [], None
    with no_host_wait():
        for i in range(CAP + TAIL):
            if i == 2:
                ss.relook(0, e)
            assert ss.active == [0, 2] and ss.enrolling == ([0] if i >= 2 and done is None else [])
            outs.append(ss.step(chunk(streams, i)).clone())
            if i >= 2 and done is None and ss.enrolling == []:
                done = i                         # the step whose poll re-targeted the slot
            if done is not None and i == done + TAIL:
                break
    torch.cuda.synchronize()
    n = len(outs)
    print("slot 0 re-targeted at step", done, "of", n)
    assert done is not None and done < CAP and done >= 2 + N_ENROLL and e.calls == 1 and ss.faults() == []
    new = streams[0, 0, 2 * HOP:2 * HOP + 256]
    assert torch.equal(ss.embedding_of(0), new)
    y = torch.stack(outs)
    twin = net.make_session_streamer(S, DEV, use_graph=False)
    twin.open(0, emb[0]), twin.open(2, emb[2])
    never = net.make_session_streamer(S, DEV, use_graph=False)
    never.open(0, emb[0]), never.open(2, emb[2])
    for i in range(n):
        if i == done:
            twin.set_embedding(0, new)
        x = chunk(streams, i)
        assert torch.equal(twin.step(x), y[i]), i
        yn = never.step(x)
        assert torch.equal(yn[2], y[i, 2]) and torch.equal(yn[0], y[i, 0]) == (i < done), i
    torch.cuda.synchronize()


def test_replays_are_deterministic_and_the_defaults_change_nothing(net, feed):
    streams, emb = feed
    ss = net.make_session_streamer(S, DEV, monitor=True, monitor_ramp=1000)
    off = net.make_session_streamer(S, DEV)

    def play(st, mixes):
        st.open(0, emb[0]), st.open(1, emb[1])
        outs = []
        with no_host_wait():
            for i in range(10):
                for slot, wet, dry in mixes.get(i, ()):
                    st.set_mix(slot, wet, dry)
                outs.append(st.step(chunk(streams, i)).clone())
        torch.cuda.synchronize()
        return torch.stack(outs)
    mixes = {0: [(0, 0.5, 0.5), (2, 0.0, 1.0)], 3: [(0, 1.0, 0.0), (1, 0.25, 1.0)], 4: [(2, 1.0, 0.0)]}
    a = play(ss, mixes)
    ss.reset()
    b = play(ss, mixes)
    assert torch.equal(a, b) and torch.isfinite(a).all() and a[:, 2].any()
    ss.reset()
    assert torch.equal(play(ss, {}), play(off, {}))
