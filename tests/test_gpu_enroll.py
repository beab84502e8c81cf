"""GPU: `SessionStreamer` enrollment under graph replay — slots record their own stream on the device, the embedder runs on the
side stream beside the chunk loop and the slots open themselves, while the host never waits: during the step loops
`torch.cuda.synchronize`, `Stream.synchronize` and `Event.synchronize` raise.  Every claim is `torch.equal`: the clips against
the samples fed, the embeddings against the embedder called afterwards on the same batches, the outputs against a control
`SessionStreamer` whose slots are `open()`ed by hand with those embeddings at the same step.  The loops end when the slots
are open; their cap of 5000 steps is a condition (the embedder takes about a dozen chunk times), not a measurement.
The inf of the fault case is ordinary input data for the capture kernel, as NaN is for lh_session_begin; it runs once."""
import contextlib
from unittest import mock

import pytest
import torch

from lookoncetohear_amd import _cabi
from lookoncetohear_amd.embed_net import EmbedTFGridNet
from lookoncetohear_amd.net import Net
from oracle import embedder_oracle as E
from oracle import tfgridnet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP, NFFT = 128, 192
S, N_ENROLL, CAP, TAIL = 8, 5, 5000, 6          # TAIL: steps after the last opening
OPEN = [0, 1, 2, 3]


@pytest.fixture(scope="module")
def net(oracle_cfg_sd):
    assert torch.cuda.is_available()
    _cabi.load()
    cfg, sd = oracle_cfg_sd
    n = Net(**O.TSH_PARAMS).eval()
    n.load_state_dict(sd, strict=True)
    return n.to(DEV)


class Recorded:
    """The embedder, keeping every call's input (a copy) and output."""

    def __init__(self, embedder):
        self.embedder, self.calls = embedder, []

    def __call__(self, x):
        out = self.embedder(x)
        self.calls.append((x.clone(), out))
        return out


@pytest.fixture(scope="module")
def embedder():
    e = EmbedTFGridNet(**E.EMBED_PARAMS).eval()
    e.load_state_dict(E.synthetic_state_dict(E.ECfg(**E.EMBED_PARAMS), 0), strict=True)
    e = e.to(DEV)
    with torch.no_grad():
        e(torch.zeros(1, 2, HOP * N_ENROLL, device=DEV))        # packs its weights: not inside a chunk loop
    torch.cuda.synchronize()
    return e


@pytest.fixture(scope="module")
def feed():
    """streams [S, 2, 128 CAP + 64]: every slot's own samples, and the embeddings slots 0..3 listen for."""
    g = torch.Generator(device=DEV).manual_seed(11)
    streams = 0.1 * torch.randn(S, 2, HOP * (CAP + TAIL + 1) + NFFT - HOP, device=DEV, generator=g)
    emb = torch.randn(S, 256, device=DEV, generator=g)
    return streams, emb


@contextlib.contextmanager
def no_host_wait():
    def refuse(*a, **k):
        raise AssertionError("the host waited for the device inside the chunk loop")
    with mock.patch.object(torch.cuda, "synchronize", refuse), mock.patch.object(torch.cuda.Stream, "synchronize", refuse), \
            mock.patch.object(torch.cuda.Event, "synchronize", refuse):
        yield


def row(streams, slot, j):
    return streams[slot, :, j * HOP:j * HOP + NFFT]


def chunk(streams, i, start):
    """Step i's input: slots 0..3 and every slot of `start` (slot -> first step of its own stream) get their samples, the
    rest NaN."""
    x = torch.full((S, 2, NFFT), float("nan"), device=DEV)
    for s in OPEN:
        x[s] = row(streams, s, i)
    for s, t0 in start.items():
        if i >= t0:
            x[s] = row(streams, s, i - t0)
    return x


def control(net, streams, emb, start, opened, embeds, n):
    """The same feed through a SessionStreamer without enrollment: slot s is open()ed with embeds[s] before step opened[s]."""
    ss = net.make_session_streamer(S, DEV)
    for s in OPEN:
        ss.open(s, emb[s])
    outs = []
    for i in range(n):
        for s, t in opened.items():
            if t == i:
                ss.open(s, embeds[s])
        outs.append(ss.step(chunk(streams, i, start)).clone())
    torch.cuda.synchronize()
    assert ss.faults() == []
    return torch.stack(outs)


def test_overlapping_enrollments_open_their_slots(net, embedder, feed):
    streams, emb = feed
    start = {5: 3, 6: 4, 7: 4}                   # slot 5 enrolls at chunk 3, slots 6 and 7 at chunk 4: they finish together
    ss = net.make_session_streamer(S, DEV, enroll_chunks=N_ENROLL)
    assert ss.graphs is not None
    for s in OPEN:
        ss.open(s, emb[s])
    rec = Recorded(embedder)
    outs, opened, last = [], {}, None
    with no_host_wait():
        for i in range(CAP + TAIL):
            for s, t0 in start.items():
                if t0 == i:
                    ss.enroll(s, rec)
            outs.append(ss.step(chunk(streams, i, start)).clone())
            for s in ss.active:
                opened.setdefault(s, i)          # the step whose poll opened it: a fresh stream from this step on
            assert ss.faults() == []
            if last is None and len(opened) == S - 1:
                last = i
            if last is not None and i == last + TAIL:
                break
    torch.cuda.synchronize()
    n = len(outs)
    print("opened at step:", {s: opened.get(s) for s in start}, "of", n, "; embedder batches:", [len(x) for x, _ in rec.calls])
    assert last is not None and last < CAP, "the enrolling slots did not open within the cap"
    assert ss.active == [0, 1, 2, 3, 5, 6, 7] and ss.enrolling == [] and ss.faults() == []
    y = torch.stack(outs)
    # the clips are the samples fed (a capture of 5 chunks crosses the two alternating graphs 3 + 2 times)
    for s in start:
        assert torch.equal(ss._clips[s], streams[s, :, :HOP * N_ENROLL]), s
    # the embeddings: the embedder called again on the same batches — ascending slots, completions of one poll together
    order = [s for x, _ in rec.calls for s in sorted(start) if any(torch.equal(r, ss._clips[s]) for r in x)]
    assert sorted(order) == [5, 6, 7] and sum(len(x) for x, _ in rec.calls) == 3
    at = 0
    with torch.no_grad():
        for x, out in rec.calls:
            slots = order[at:at + len(x)]
            at += len(x)
            assert slots == sorted(slots) and torch.equal(x, torch.stack([ss._clips[s] for s in slots]))
            again = embedder(x)
            for k, s in enumerate(slots):
                assert torch.equal(ss.embedding_of(s), again[k]) and torch.equal(out[k], again[k]), s
    embeds = {s: ss.embedding_of(s).clone() for s in start}
    for s in start:
        assert opened[s] >= start[s] + N_ENROLL
        assert not y[:opened[s], s].any()                       # idle to the separator during the look
    yc = control(net, streams, emb, start, {s: opened[s] for s in start}, embeds, n)
    for s in OPEN:
        assert torch.equal(y[:, s], yc[:, s]), s                # the listeners next door never noticed
    for s in start:
        assert torch.equal(y[opened[s]:, s], yc[opened[s]:, s]), s
        assert y[opened[s]:, s].any()
    assert not y[:, 4].any() and torch.isfinite(y).all()


def test_aborted_capture_faults_the_slot_alone(net, embedder, feed):
    """Slot 5 enrolls at chunk 2; recorded sample 17 of its third chunk is inf."""
    streams, emb = feed
    streams = streams.clone()
    streams[5, 1, 2 * HOP + 17] = float("inf")
    ss = net.make_session_streamer(S, DEV, enroll_chunks=N_ENROLL)
    for s in OPEN:
        ss.open(s, emb[s])
    start, outs, faulted, opened = {5: 2}, [], None, None
    with no_host_wait():
        for i in range(CAP + TAIL):
            if i == 2:
                ss.enroll(5, embedder)
            if faulted is None and ss.faults() == [5]:
                faulted = i
                assert 5 not in ss.active and ss.enrolling == []
                start = {5: i}                   # at once, from clean samples: its own stream starts again, past the inf
                streams[5] = streams[4]
                ss.enroll(5, embedder)
                assert ss.faults() == [] and ss.enrolling == [5]
            outs.append(ss.step(chunk(streams, i, start)).clone())
            if opened is None and 5 in ss.active:
                opened = i
            if opened is not None and i == opened + TAIL:
                break
    torch.cuda.synchronize()
    n = len(outs)
    print("fault seen before step", faulted, ", opened at step", opened, "of", n)
    assert faulted is not None and opened is not None and opened < CAP
    assert ss.faults() == [] and ss.active == [0, 1, 2, 3, 5]
    y = torch.stack(outs)
    assert not y[:opened, 5].any() and y[opened:, 5].any() and torch.isfinite(y).all()
    # the control is fed what the loop fed: the inf sits in an idle slot's row there, where it is ignored
    # (feed before `faulted`: the stream with the inf, from chunk 2; afterwards: the clean stream, from `faulted`)
    ctl = net.make_session_streamer(S, DEV)
    for s in OPEN:
        ctl.open(s, emb[s])
    clean = streams
    dirty = streams.clone()
    dirty[5] = feed[0][5]
    dirty[5, 1, 2 * HOP + 17] = float("inf")
    for i in range(n):
        if i == opened:
            ctl.open(5, ss.embedding_of(5))
        x = chunk(dirty, i, {5: 2}) if i < faulted else chunk(clean, i, {5: faulted})
        assert torch.equal(ctl.step(x), y[i]), i
    torch.cuda.synchronize()


def test_default_is_unchanged_by_the_capture_node(net, feed):
    streams, emb = feed
    a = net.make_session_streamer(S, DEV)
    b = net.make_session_streamer(S, DEV, enroll_chunks=N_ENROLL)
    for s in OPEN:
        a.open(s, emb[s]), b.open(s, emb[s])
    for i in range(12):
        x = chunk(streams, i, {})
        assert torch.equal(a.step(x), b.step(x)), i
    torch.cuda.synchronize()
    assert a.faults() == [] and b.faults() == [] and b.enrolling == [] and not b._ewords.any() and not b._edone.any()
    with pytest.raises(ValueError):
        a.enroll(5, None)
