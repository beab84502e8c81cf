"""GPU: `SessionStreamer` under graph replay — listener slots open, close, are re-used and fail one at a time while the
batch advances in lock-step.  A session's reference is the float64 oracle over the session's OWN samples from the zero state
(streaming == offline), tolerance as in tests/test_gpu_parity.py; isolation and equality claims are `torch.equal`.
The non-finite and 3e38 inputs of the fault test are ordinary data for the range guard (lh_session_begin / lh_session_end
close the slot); each case runs once."""
import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.net import Net
from oracle import tfgridnet_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_gpu_parity.py
DEV = "cuda:0"
HOP, NFFT = 128, 192


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


def test_all_open_equals_streamer(net):
    """S = 4, every slot opened before the first chunk, 60 chunks (the ring wraps): bit-identical to `Streamer(4)`."""
    S, n = 4, 60
    mix, emb = clips([31, 32, 33, 34], n)
    mix, emb = mix.to(DEV), emb.to(DEV)
    st = net.make_streamer(S, DEV)
    st.set_embedding(emb)
    ss = net.make_session_streamer(S, DEV)
    assert ss.graphs is not None
    for s in range(S):
        ss.open(s, emb[s])
    for i in range(n):
        x = mix[:, :, i * HOP:i * HOP + NFFT]
        a, b = ss.step(x).clone(), st.step(x).clone()
        assert torch.equal(a, b), i
    torch.cuda.synchronize()
    assert ss.active == [0, 1, 2, 3] and ss.faults() == []


# (slot, first chunk, end chunk (exclusive), clip): openings at chunks 0, 7, 49, 50, 51 and 63 — before, at and after the
# 50-slot ring wraps — closings at 40, 49, 90 and 100, slot 1 re-used by another listener, slot 6 never opened
SESSIONS = [(0, 0, 120, 0), (1, 0, 40, 1), (7, 0, 49, 2), (2, 7, 100, 3), (3, 49, 120, 4), (4, 50, 90, 5), (5, 51, 120, 6),
            (1, 63, 120, 7)]
N_CHUNKS, N_SLOTS = 120, 8


def run_schedule(ss, mix, emb):
    """mix [8 clips, 2, N] and emb [8, 256] on the device.  Rows of idle slots are NaN: they must be ignored."""
    outs = []
    for i in range(N_CHUNKS):
        for slot, t0, t1, c in SESSIONS:
            if t1 == i:
                ss.close(slot)
        for slot, t0, t1, c in SESSIONS:
            if t0 == i:
                ss.open(slot, emb[c])
        x = torch.full((N_SLOTS, 2, NFFT), float("nan"), device=DEV)
        for slot, t0, t1, c in SESSIONS:
            if t0 <= i < t1:
                x[slot] = mix[c, :, (i - t0) * HOP:(i - t0) * HOP + NFFT]
        outs.append(ss.step(x).clone())
    torch.cuda.synchronize()
    return torch.cat(outs, -1).cpu()


def test_schedule_across_the_ring_wrap(net, oracle_cfg_sd):
    mix, emb = clips(list(range(40, 48)), N_CHUNKS)
    mixd, embd = mix.to(DEV), emb.to(DEV)
    ss = net.make_session_streamer(N_SLOTS, DEV)
    y = run_schedule(ss, mixd, embd)
    assert ss.faults() == [] and ss.active == [0, 1, 3, 5]
    assert torch.isfinite(y).all()
    busy = torch.zeros(N_SLOTS, N_CHUNKS, dtype=torch.bool)
    for slot, t0, t1, c in SESSIONS:
        ref = fresh_stream64(oracle_cfg_sd, mix[c], emb[c], t1 - t0)
        e = float((y[slot, :, t0 * HOP:t1 * HOP].double() - ref).abs().max())
        print(f"slot {slot} chunks {t0}..{t1}: max|hip - fp64 fresh stream| = {e:.2e}")
        assert e <= TOL, (slot, t0, e)
        busy[slot, t0:t1] = True
    idle = ~busy.repeat_interleave(HOP, 1)[:, None, :].expand(-1, 2, -1)
    assert idle.any() and not y[idle].any()                  # idle rows are exact zeros
    # the same bits from a second run of the same streamer, and from the eager launches
    ss.reset()
    assert torch.equal(run_schedule(ss, mixd, embd), y)
    eager = net.make_session_streamer(N_SLOTS, DEV, use_graph=False)
    assert eager.graphs is None
    assert torch.equal(run_schedule(eager, mixd, embd), y)


@pytest.mark.parametrize("kind", ["nan", "inf", "burst_3e38"])
def test_fault_isolation_under_replay(net, oracle_cfg_sd, kind):
    """S = 8, all open; slot 3's chunk 10 is bad — a NaN or an inf sample (stopped by lh_session_begin) or a finite 3e38 burst
    that overflows fp32 inside the separator (caught by lh_session_end).  `step` never raises; the other seven slots keep
    their bits; slot 3 is reported, silent from that chunk on, and opens again as a fresh stream."""
    S, n, bad_at, reopen_at, slot = 8, 32, 10, 20, 3
    mix, emb = clips(list(range(50, 59)), n)
    mixd, embd = mix.to(DEV), emb.to(DEV)

    def run(fault):
        ss = net.make_session_streamer(S, DEV)
        for s in range(S):
            ss.open(s, embd[s])
        outs, seen = [], {}
        for i in range(n):
            x = mixd[:S, :, i * HOP:i * HOP + NFFT].clone()
            if fault:
                if i == bad_at:
                    if kind == "nan":
                        x[slot, 0, 5] = float("nan")
                    elif kind == "inf":
                        x[slot, 1, 190] = float("-inf")
                    else:
                        x[slot] = 3e38
                if i in (bad_at, bad_at + 1):
                    torch.cuda.synchronize()
                    seen[i] = (ss.faults(), ss.active)
                if i == reopen_at:
                    ss.open(slot, embd[8])
                if i >= reopen_at:
                    x[slot] = mixd[8, :, (i - reopen_at) * HOP:(i - reopen_at) * HOP + NFFT]
            outs.append(ss.step(x).clone())
        torch.cuda.synchronize()
        return torch.cat(outs, -1).cpu(), seen, ss

    clean, _, _ = run(False)
    y, seen, ss = run(True)
    others = [s for s in range(S) if s != slot]
    assert seen[bad_at] == ([], list(range(S))) and seen[bad_at + 1] == ([slot], others)
    assert torch.equal(y[others], clean[others])
    assert torch.equal(y[slot, :, :bad_at * HOP], clean[slot, :, :bad_at * HOP])
    assert not y[slot, :, bad_at * HOP:reopen_at * HOP].any()
    assert torch.isfinite(y).all()
    ref = fresh_stream64(oracle_cfg_sd, mix[8], emb[8], n - reopen_at)
    e = float((y[slot, :, reopen_at * HOP:].double() - ref).abs().max())
    print(f"{kind}: re-opened slot max|hip - fp64 fresh stream| = {e:.2e}")
    assert e <= TOL
    assert ss.faults() == [] and ss.active == list(range(S))
