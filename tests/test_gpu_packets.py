"""GPU: `SessionStreamer(pace=True, packets=True)` under graph replay — clients' packets of any size go in through `push`,
the device keeps a FIFO per slot, cuts its own 192-sample windows and decides which slots are present (`lh_session_feed`,
`lh_session_frame`, `lh_session_emit_s16`).  The feature moves bytes and derives presence, so every claim is `torch.equal`: a
listener's concatenated present rows against the all-present output of a plain paced streamer stepped with explicit windows
(the `plain` construction of tests/test_gpu_pace.py, which has its own float64 oracle tests).  The NaN of the fault case is
ordinary input data for lh_session_begin_paced and runs once."""
import contextlib
from unittest import mock

import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.net import Net
from oracle import tfgridnet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP, NFFT = 128, 192
S, N_CLIP = 4, 120
N_TOTAL = HOP * N_CLIP + NFFT - HOP


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
    """Four listeners: mix [4, 2, 128 * 120 + 64] on the host (packets are host tensors) and on the device, emb [4, 256]."""
    d = synth.batch([80, 81, 82, 83], N_TOTAL)
    mix, emb = d["mixture"], d["embedding_gt"][:, 0]
    return mix, mix.to(DEV), emb.to(DEV)


@pytest.fixture(scope="module")
def plain(net, clips):
    """Every listener's clip, all present, explicit windows: all four opened before the first chunk of one paced streamer.
    [4, 2, 128 * 120] on the host; computed once and never written."""
    _, mixd, embd = clips
    ss = net.make_session_streamer(S, DEV, pace=True)
    for s in range(S):
        ss.open(s, embd[s])
    outs = [ss.step(mixd[:, :, i * HOP:i * HOP + NFFT]).clone() for i in range(N_CLIP)]
    torch.cuda.synchronize()
    assert ss.faults() == []
    return torch.cat(outs, -1).cpu()


@contextlib.contextmanager
def no_host_wait():
    def refuse(*a, **k):
        raise AssertionError("the host waited for the device inside the chunk loop")
    with mock.patch.object(torch.cuda, "synchronize", refuse), mock.patch.object(torch.cuda.Stream, "synchronize", refuse), \
            mock.patch.object(torch.cuda.Event, "synchronize", refuse):
        yield


def drive(ss, mix, sizes, n_ticks=None, catch_up=lambda t: t % 2 == 1, before_tick=None, total=N_TOTAL):
    """The tick loop: push one packet per slot (`sizes(slot, tick)` samples of the slot's clip, None = no packet), then one
    `step` — or, on a catch-up tick, `step` for as long as someone is ready.  `avail` is this test's own arithmetic of what
    every slot holds; `ready()` and `last_present` must agree with it at every step.
    -> outputs [steps, S, 2, 128] and the device's hold words [steps, S] (both on the device: nothing here waits), and the
    predicted presence per step."""
    n_slots = ss.S
    pos, avail = [0] * n_slots, [0] * n_slots
    outs, holds, presents = [], [], []
    t = 0
    while t < n_ticks if n_ticks is not None else (any(p < total for p in pos) or ss.ready()):
        if before_tick is not None:
            before_tick(t, avail)
        packets = {}
        for s in range(n_slots):
            n = sizes(s, t)
            if n is None:
                continue
            n = min(n, total - pos[s])
            packets[s] = mix[s][:, pos[s]:pos[s] + n]
            pos[s] += n
            avail[s] += n
        ss.push(packets)
        first = True
        while first or (catch_up(t) and ss.ready()):
            first = False
            want = tuple(a >= NFFT for a in avail)
            assert ss.ready() == [s for s in range(n_slots) if want[s]] and [ss.buffered(s) for s in range(n_slots)] == avail
            y = ss.step()
            assert ss.last_present == want, (t, want)
            avail = [a - HOP if w else a for a, w in zip(avail, want)]
            outs.append(y.clone())
            holds.append(ss._hold.clone())
            presents.append(want)
        t += 1
    return torch.stack(outs), torch.stack(holds), presents


def listener(y, presents, s, steps=None):
    """The concatenated rows of slot `s` over the steps it was present for: y [steps, S, 2, 128] on the host."""
    rows = [y[i, s] for i in (range(len(presents)) if steps is None else steps) if presents[i][s]]
    return torch.cat(rows, -1)


def device_agrees(holds, presents):
    return torch.equal(holds.cpu() != 0, ~torch.tensor(presents))


CYCLE = (1, 127, 128, 129, 191, 192, 193, 64, 0)


def any_sizes(s, t):
    """Slot 0: a 10 ms client; slot 1: a 20 ms client; slot 2: odd sizes around the chunk and the window; slot 3: silent for
    ten ticks, then everything it missed at once."""
    if s == 3:
        return None if t < 10 else 1408 if t == 10 else 160
    return (160, 320, CYCLE[t % len(CYCLE)])[s]


def test_any_packetisation_gives_the_same_listener(net, clips, plain):
    mix, _, embd = clips
    ss = net.make_session_streamer(S, DEV, pace=True, packets=True)
    assert ss.packets and ss.graphs is not None and ss.fifo_samples == 2048
    for s in range(S):
        ss.open(s, embd[s])
    with no_host_wait():                                         # `push` and `step` never synchronise
        y, holds, presents = drive(ss, mix, any_sizes)
    torch.cuda.synchronize()
    assert ss.faults() == [] and ss.active == [0, 1, 2, 3]
    assert device_agrees(holds, presents)                        # the device decided what the mirror predicted
    y = y.cpu()
    for i, want in enumerate(presents):
        for s in range(S):
            assert want[s] or not y[i, s].any(), (i, s)          # a held row: exact zeros
    assert not any(p[3] for p in presents[:10]) and any(all(p) for p in presents) and not all(all(p) for p in presents[20:])
    for s in range(S):
        mine = listener(y, presents, s)
        assert mine.shape == plain[s].shape and torch.equal(mine, plain[s]), s
    assert [ss.buffered(s) for s in range(S)] == [NFFT - HOP] * S
    # the counters on the device are the mirror's
    assert ss._fifo_words.tolist() == [[N_TOTAL] * S, [HOP * N_CLIP] * S]


def test_small_ring_wraps_every_second_window(net, clips, plain):
    """fifo_samples = 256 and 128-sample packets: the ring is full before every step and every second window crosses its end."""
    n = 60
    mix, _, embd = clips
    ss = net.make_session_streamer(S, DEV, pace=True, packets=True, fifo_samples=256)
    for s in range(S):
        ss.open(s, embd[s])
    y, holds, presents = drive(ss, mix, lambda s, t: 128, n_ticks=n + 1, catch_up=lambda t: False)
    torch.cuda.synchronize()
    assert ss.faults() == [] and device_agrees(holds, presents)
    assert presents == [(False,) * S] + [(True,) * S] * n
    y = y.cpu()
    for s in range(S):
        assert torch.equal(listener(y, presents, s), plain[s, :, :n * HOP]), s
    with pytest.raises(BufferError):
        ss.push({0: mix[0][:, :129]})                            # 128 buffered + 129 > 256
    assert ss.buffered(0) == 128


def test_packets_with_compaction(net, clips, plain):
    """compact=True, row_buckets=(1, 2, 4): slot 3 opens at tick 10 (its client's packets start then, behind a flush), slot 1
    closes at tick 40 and slot 3's listener moves from row 3 to row 1.  Every output row of every step equals the packet
    streamer that does not compact."""
    n_ticks = 60
    mix, _, embd = clips

    def run(**kw):
        ss = net.make_session_streamer(S, DEV, pace=True, packets=True, **kw)
        for s in range(3):
            ss.open(s, embd[s])

        def events(t, avail):
            if t == 10:
                ss.open(3, embd[3])
                ss.flush(3)
                avail[3] = 0
            if t == 40:
                ss.close(1)
        y, holds, presents = drive(ss, mix, lambda s, t: None if s == 3 and t < 10 else 160, n_ticks=n_ticks,
                                   catch_up=lambda t: t % 4 == 3, before_tick=events)
        torch.cuda.synchronize()
        assert ss.faults() == [] and ss.active == [0, 2, 3] and device_agrees(holds, presents)
        return ss, y.cpu(), presents

    ss, y, presents = run(compact=True, row_buckets=(1, 2, 4))
    assert ss._row_of == [0, -1, 2, 1] and ss.last_rows == 4 and ss.rows_in_use == 3
    _, y_lock, presents_lock = run()
    assert presents == presents_lock and torch.equal(y, y_lock)
    # ... and the survivors are the listeners of the plain streamer
    for s in (0, 2):
        mine = listener(y, presents, s)
        assert mine.shape[-1] > 50 * HOP and torch.equal(mine, plain[s, :, :mine.shape[-1]]), s
    opened = next(i for i, p in enumerate(presents) if p[3])     # slot 3: nothing buffered until its packets start
    mine = listener(y, presents, 3)
    assert not y[:opened, 3].any() and mine.shape[-1] > 40 * HOP and torch.equal(mine, plain[3, :, :mine.shape[-1]])
    closed = listener(y, presents, 1)
    k = closed.abs().sum(0).nonzero().max().item() // HOP + 1       # chunks slot 1 played before it closed
    assert 30 < k < 60 and torch.equal(closed[:, :k * HOP], plain[1, :, :k * HOP]) and not closed[:, k * HOP:].any()


def test_enrollment_from_the_packet_stream(net, clips):
    """enroll_chunks = 4: slot 1's client sends 100-sample packets from tick 0, the slot is armed before tick 5.  The clip is
    the first 512 stream samples framed from the arming step on; then the slot opens.  The loop's cap is a condition (the host
    runs ahead of the device), not a measurement."""
    n_enroll, arm_at, cap = 4, 5, 2000
    mix, _, embd = clips
    got = []

    def stand_in(x):
        got.append(x.clone())
        return embd[1][None].expand(x.shape[0], -1).clone()
    ss = net.make_session_streamer(S, DEV, enroll_chunks=n_enroll, pace=True, packets=True)
    ss.open(0, embd[0])
    pos = consumed = armed_from = 0
    opened = None
    with no_host_wait():
        for t in range(cap):
            if t == arm_at:
                ss.enroll(1, stand_in)
                armed_from = consumed                            # chunks framed before the arming step are not the clip's
            at = pos % (N_TOTAL - 100)
            ss.push({1: mix[1][:, at:at + 100]})
            pos += 100
            ss.step()
            consumed += ss.last_present[1]
            if 1 in ss.active:
                opened = t
                break
        else:
            raise AssertionError("the enrolling slot did not open within the cap")
    torch.cuda.synchronize()
    assert armed_from == 3 and opened >= arm_at + n_enroll and ss.faults() == [] and ss.enrolling == [] and ss.active == [0, 1]
    assert len(got) == 1 and torch.equal(got[0].cpu(), mix[1][None, :, HOP * armed_from:HOP * (armed_from + n_enroll)])


def test_pcm16_in_and_out(net, clips):
    """16-bit packets in, 16-bit rows out: the bits of the fp32 packet streamer fed pcm / 32768, through the emit formula."""
    n_ticks = 40
    mix, _, embd = clips
    pcm = (mix * 32767).round().to(torch.int16)
    assert mix.abs().max() <= 1.0
    a = net.make_session_streamer(S, DEV, pace=True, packets=True, pcm16=True)
    b = net.make_session_streamer(S, DEV, pace=True, packets=True)
    for ss in (a, b):
        for s in range(S):
            ss.open(s, embd[s])
    sizes = lambda s, t: (160, 320, 100, 128)[s]
    ya, ha, pa = drive(a, pcm, sizes, n_ticks=n_ticks)
    yb, hb, pb = drive(b, pcm.float() / 32768, sizes, n_ticks=n_ticks)
    torch.cuda.synchronize()
    assert a.faults() == b.faults() == [] and pa == pb and device_agrees(ha, pa)
    assert ya.dtype == torch.int16 and yb.dtype == torch.float32
    want = torch.clamp(torch.round(yb * 32768), -32768, 32767).to(torch.int16)
    assert torch.equal(ya, want) and ya.any() and any(all(p) for p in pa)
    with pytest.raises(ValueError):
        a.push({0: mix[0][:, :10]})                              # a 16-bit streamer takes int16


def test_nan_in_a_packet_closes_that_listener_only(net, clips, plain):
    """One NaN sample inside slot 2's 13th packet: the chunk that frames it closes slot 2, the other three keep their bits."""
    n_ticks, bad_tick = 30, 12
    mix, _, embd = clips
    bad = mix.clone()
    bad[2, 0, 160 * bad_tick + 7] = float("nan")
    ss = net.make_session_streamer(S, DEV, pace=True, packets=True)
    for s in range(S):
        ss.open(s, embd[s])
    y, holds, presents = drive(ss, bad, lambda s, t: 160, n_ticks=n_ticks)           # never raises
    torch.cuda.synchronize()
    assert ss.faults() == [2] and ss.active == [0, 1, 3] and device_agrees(holds, presents)
    y = y.cpu()
    assert torch.isfinite(y).all()
    for s in (0, 1, 3):
        mine = listener(y, presents, s)
        assert mine.shape[-1] >= 30 * HOP and torch.equal(mine, plain[s, :, :mine.shape[-1]]), s
    mine = listener(y, presents, 2)
    k = (160 * bad_tick + 7 - NFFT) // HOP + 1                   # chunks whose window [128 j, 128 j + 192) ends before the sample
    assert torch.equal(mine[:, :k * HOP], plain[2, :, :k * HOP]) and not mine[:, k * HOP:].any() and mine[:, :k * HOP].any()
