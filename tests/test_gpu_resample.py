"""GPU: `Resampler` against the float64 restatement, and `SessionStreamer(pace=True, packets=True, client_rate=...)` under graph
replay — packets at the client's rate in, rows at the client's rate out, resampled on the device on both sides
(`lh_session_resample_in`, `lh_session_resample_out`).  The session nodes share `lh_resample`'s inner product, so the claim is
`torch.equal`: a listener's concatenated present rows against their whole stream resampled offline, served by a 16 kHz packet
streamer, and resampled offline again behind the zero prefix of the output delay."""
import contextlib
from unittest import mock

import numpy as np
import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.net import Net
from lookoncetohear_amd.resample import Resampler
from oracle import tfgridnet_oracle as O
from tests import resample_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP, NFFT = 128, 192
S, N_CLIP = 4, 24
N16 = HOP * N_CLIP + NFFT - HOP


# ---- Resampler against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new,shape", [(48000, 16000, (3, 4801)), (48000, 16000, (1, 240000)), (16000, 48000, (3, 4801)),
                                            (44100, 16000, (3, 4801))])
def test_resampler_matches_float64_within_the_dot_product_bound(orig, new, shape):
    assert torch.cuda.is_available()
    bank, width, o, n = C.bank64(orig, new)
    torch.manual_seed(shape[1])
    x = torch.randn(*shape) * 0.5
    rs = Resampler(orig, new)
    y = rs(x.to(DEV))
    assert y.is_cuda and tuple(y.shape) == (shape[0], C.out_len(shape[1], o, n))
    want, mag = C.resample64(x.numpy(), bank, width, o, n)
    err, lim = np.abs(y.cpu().numpy().astype(np.float64) - want), C.bound(mag, bank.shape[1])
    print(f"{orig}->{new} {shape}: max err {err.max():.3e}, largest err / bound {(err / np.maximum(lim, 1e-300)).max():.4f}")
    assert (err <= lim).all() and err.max() > 0
    assert Resampler(orig, orig)(y) is y
    with pytest.raises(RuntimeError):
        rs(x)                                                    # no CPU path


# ---- the client-rate streamer -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(oracle_cfg_sd):
    assert torch.cuda.is_available()
    _cabi.load()
    cfg, sd = oracle_cfg_sd
    n = Net(**O.TSH_PARAMS).eval()
    n.load_state_dict(sd, strict=True)
    return n.to(DEV)


def client_len(rate, n16=N16):
    """Client samples that make exactly n16 samples at 16 kHz: the last block's taps end with the stream."""
    _, width, o, n = C.bank64(rate, 16000)
    return (n16 // n - 1) * o + width + o


@pytest.fixture(scope="module")
def clips():
    """Four listeners' streams, long enough for 24 chunks at any client rate up to 48 kHz; |x| <= 1.  Host tensors, never
    written."""
    d = synth.batch([80, 81, 82, 83], client_len(48000))
    assert d["mixture"].abs().max() <= 1.0
    return d["mixture"], d["embedding_gt"][:, 0].to(DEV)


def served_offline(net, emb, x, rate, n_chunks=N_CLIP):
    """x [S, 2, n] at `rate` on the host -> [S, 2, n_chunks * hop_client]: resampled in one piece, through a 16 kHz packet
    streamer with everyone present, resampled in one piece behind the zero prefix."""
    n16 = HOP * n_chunks + NFFT - HOP
    x16 = Resampler(rate, 16000)(x.to(DEV))[..., :n16].cpu()
    assert x16.shape[-1] == n16
    ss = net.make_session_streamer(S, DEV, pace=True, packets=True, fifo_samples=4096)
    for s in range(S):
        ss.open(s, emb[s])
    ss.push({s: x16[s] for s in range(S)})
    rows = []
    while ss.ready():
        rows.append(ss.step().clone())
        assert all(ss.last_present)
    assert len(rows) == n_chunks and ss.faults() == []
    rows16 = torch.cat(rows, -1)
    up = Resampler(16000, rate)
    _, width, o, n = C.bank64(16000, rate)
    delay = -(-(width + o) // o) * o
    y = up(torch.cat([torch.zeros(S, 2, delay, device=DEV), rows16], -1))
    return y[..., :n_chunks * HOP * rate // 16000].cpu()


@pytest.fixture(scope="module")
def want48(net, clips):
    mix, emb = clips
    return served_offline(net, emb, mix, 48000)


@contextlib.contextmanager
def no_host_wait():
    def refuse(*a, **k):
        raise AssertionError("the host waited for the device inside the chunk loop")
    with mock.patch.object(torch.cuda, "synchronize", refuse), mock.patch.object(torch.cuda.Stream, "synchronize", refuse), \
            mock.patch.object(torch.cuda.Event, "synchronize", refuse):
        yield


def drive(ss, x, sizes, total, catch_up=lambda t: t % 2 == 1, n_ticks=None):
    """The tick loop: one packet per slot (`sizes(slot, tick)` client samples), then one `step` — on a catch-up tick, `step` for
    as long as someone is ready.  -> rows [steps, S, 2, hop_client] on the device, the presence per step."""
    pos, outs, presents, t = [0] * ss.S, [], [], 0
    while (t < n_ticks) if n_ticks is not None else (any(p < total for p in pos) or ss.ready()):
        packets = {}
        for s in range(ss.S):
            n = min(sizes(s, t), total - pos[s])
            packets[s] = x[s][:, pos[s]:pos[s] + n]
            pos[s] += n
        ss.push(packets)
        first = True
        while first or (catch_up(t) and ss.ready()):
            first = False
            ready = ss.ready()
            y = ss.step()
            assert [s for s in range(ss.S) if ss.last_present[s]] == ready
            outs.append(y.clone())
            presents.append(ss.last_present)
        t += 1
    return torch.stack(outs), presents


def listener(y, presents, s):
    return torch.cat([y[i, s] for i in range(len(presents)) if presents[i][s]], -1)


def sizes48(s, t):
    """A 10 ms client, a 20 ms client, one that sends 441 samples a tick, one that alternates 1 and 1919."""
    return (480, 960, 441, 1 if t % 2 == 0 else 1919)[s]


def test_any_packetisation_at_48k_gives_the_offline_listener(net, clips, want48):
    mix, emb = clips
    ss = net.make_session_streamer(S, DEV, pace=True, packets=True, client_rate=48000)
    assert ss.graphs is not None and ss.hop_client == 384 and ss.client_rate == 48000 and ss.raw_samples == 8192
    for s in range(S):
        ss.open(s, emb[s])
    with no_host_wait():                                         # `push` and `step` never synchronise
        y, presents = drive(ss, mix, sizes48, client_len(48000))
    torch.cuda.synchronize()
    assert ss.faults() == [] and tuple(y.shape[1:]) == (S, 2, 384)
    y = y.cpu()
    for i, p in enumerate(presents):
        for s in range(S):
            assert p[s] or not y[i, s].any(), (i, s)             # a held row: exact zeros
    assert any(all(p) for p in presents) and not all(all(p) for p in presents)
    for s in range(S):
        mine = listener(y, presents, s)
        assert mine.shape == want48[s].shape and torch.equal(mine, want48[s]), s
    assert want48.abs().max() > 1e-3
    # the counters on the device are the mirror's
    assert [[v & 0xffffffff for v in r] for r in ss._fifo_words.tolist()] == [ss._wr, ss._rd] == [[N16] * S, [HOP * N_CLIP] * S]
    assert [v & 0xffffffff for v in ss._raw_words[0].tolist()] == ss._raw_wr == [client_len(48000)] * S


def test_24k_blocks_of_two_samples(net, clips):
    n_chunks = 8
    mix, emb = clips
    total = client_len(24000, HOP * n_chunks + NFFT - HOP)
    x = mix[..., :total]
    want = served_offline(net, emb, x, 24000, n_chunks)
    ss = net.make_session_streamer(S, DEV, pace=True, packets=True, client_rate=24000)
    assert ss.hop_client == 192 and (ss._o_in, ss._n_in) == (3, 2)
    for s in range(S):
        ss.open(s, emb[s])
    y, presents = drive(ss, x, lambda s, t: (240, 480, 441, 1 if t % 2 == 0 else 959)[s], total)
    torch.cuda.synchronize()
    y = y.cpu()
    assert ss.faults() == []
    for s in range(S):
        mine = listener(y, presents, s)
        assert mine.shape == want[s].shape and torch.equal(mine, want[s]), s


def test_pcm16_at_48k_carries_the_bits_of_the_fp32_path(net, clips):
    n_ticks = 12
    mix, emb = clips
    pcm = (mix * 32767).round().to(torch.int16)
    a = net.make_session_streamer(S, DEV, pace=True, packets=True, pcm16=True, client_rate=48000)
    b = net.make_session_streamer(S, DEV, pace=True, packets=True, client_rate=48000)
    for ss in (a, b):
        for s in range(S):
            ss.open(s, emb[s])
    ya, pa = drive(a, pcm, sizes48, client_len(48000), n_ticks=n_ticks)
    yb, pb = drive(b, pcm.float() / 32768, sizes48, client_len(48000), n_ticks=n_ticks)
    torch.cuda.synchronize()
    assert a.faults() == b.faults() == [] and pa == pb and ya.dtype == torch.int16 and yb.dtype == torch.float32
    want = torch.clamp(torch.round(yb * 32768), -32768, 32767).to(torch.int16)
    assert torch.equal(ya, want) and ya.any() and any(all(p) for p in pa)
    assert torch.equal(a._tail, b._tail) and torch.equal(a._fifo, b._fifo)


def test_flush_in_mid_stream_restarts_from_silence(net, clips, want48):
    """Slot 0 plays another client's stream for a while; then the host gives the slot away: close, flush, open.  The rows that
    follow are a fresh streamer's, the ones `want48` holds."""
    mix, emb = clips
    ss = net.make_session_streamer(S, DEV, pace=True, packets=True, client_rate=48000)
    ss.open(0, emb[1])
    for t in range(5):
        ss.push({0: mix[1][:, 1000 * t + 7:1000 * (t + 1) + 7]})
        while ss.ready():
            ss.step()
    assert ss.buffered(0) > 0 and ss._raw_wr[0] == 5000
    ss.close(0)
    ss.flush(0)
    ss.open(0, emb[0])
    assert ss.buffered(0) == 0
    total = client_len(48000)
    rows, pos = [], 0
    while pos < total or ss.ready():
        ss.push({0: mix[0][:, pos:pos + 1919]})
        pos += 1919
        while ss.ready():
            rows.append(ss.step()[0].clone())
    torch.cuda.synchronize()
    assert ss.faults() == [] and len(rows) == N_CLIP
    assert torch.equal(torch.cat(rows, -1).cpu(), want48[0])


def test_client_rate_16000_is_the_packet_streamer(net, clips):
    mix, emb = clips
    a = net.make_session_streamer(S, DEV, pace=True, packets=True, client_rate=16000)
    b = net.make_session_streamer(S, DEV, pace=True, packets=True)
    assert not hasattr(a, "_raw") and not hasattr(a, "_tail") and not hasattr(a, "out_client") and a.hop_client == HOP
    assert a._stage.numel() == b._stage.numel() and a._item_words == b._item_words
    for ss in (a, b):
        for s in range(S):
            ss.open(s, emb[s])
    ya, pa = drive(a, mix, lambda s, t: 160, N16, n_ticks=12)
    yb, pb = drive(b, mix, lambda s, t: 160, N16, n_ticks=12)
    torch.cuda.synchronize()
    assert pa == pb and torch.equal(ya, yb) and ya.any() and tuple(ya.shape[1:]) == (S, 2, HOP)
