"""GPU: `Streamer(frames_per_chunk=m)` under graph replay and its entry points (ABI 32: `lh_qkv_proj_ln` with `ring_pos` at
T = m, `lh_local_attn_ring`, `lh_ring_advance_by`) by direct C-ABI calls on device tensors.  The cases and the ring arithmetic
they restate: tests/stream_frames_cases.py."""
import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from lookoncetohear_amd.net import Net
from oracle import tfgridnet_oracle as O
from tests import stream_frames_cases as SF
from tests.stage_cases import Rig

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_gpu_parity.py
ROW_TOL = 2e-5      # "same utterance, other launch shape": test_batch32_invariance_and_oracle
DEV = "cuda:0"
CHUNKS = {2: 60, 5: 24, 16: 9}          # each wraps its ring of 49 + m rows at least twice
LISTENERS = [11, 12, 13]


@pytest.fixture(scope="module")
def net(oracle_cfg_sd):
    assert torch.cuda.is_available()
    _cabi.load()                                   # fails loudly if the HIP extension is missing
    _, sd = oracle_cfg_sd
    n = Net(**O.TSH_PARAMS).eval()
    n.load_state_dict(sd, strict=True)
    return n.to(DEV)


@pytest.fixture(scope="module")
def rig(net):
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    return Rig(lib, net, DEV, torch.cuda.current_stream(DEV).cuda_stream, torch.cuda.synchronize)


@pytest.fixture(scope="module")
def single_frame(net):
    """The `frames_per_chunk=1` streamers the m-frame ones are compared with, built once."""
    return {B: net.make_streamer(B, DEV, use_graph=True) for B in (1, 3)}


def _err(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max())


@pytest.mark.parametrize("B", [1, 17])          # either side of the `bh8 * ntt <= 64` grid switch
@pytest.mark.parametrize("m", SF.ATTN_M)
def test_ring_attention_equals_contiguous_attention(rig, m, B):
    q, kx, vx, ref = SF.attn_contiguous(rig.call, rig.st, rig.sync, B, m, DEV)
    for pos in SF.attn_positions(m):
        out = SF.attn_on_ring(rig.call, rig.st, rig.sync, B, m, pos, q, kx, vx, DEV)
        assert torch.equal(out, ref), (m, B, pos, _err(out, ref))


@pytest.mark.parametrize("m", SF.QKV_M)
def test_qkv_ring_write(rig, m):
    SF.qkv_ring_write(rig, 2, m, SF.qkv_positions(m))


def test_ring_advance_by_and_refusals(rig):
    SF.advance_by_cases(rig.lib.raw, rig.call, rig.st, rig.sync, DEV)
    SF.refuse_17_frames(rig.lib.raw, rig.st)


@pytest.mark.parametrize("m", sorted(CHUNKS))
def test_frames_per_chunk_end_to_end(net, single_frame, m):
    n_chunks = CHUNKS[m]
    frames = m * n_chunks
    assert frames >= 2 * SF.ring_rows(m)
    d = synth.batch(LISTENERS, SF.HOP * frames + SF.LOOK)
    mix3, emb3 = d["mixture"].to(DEV), d["embedding_gt"][:, 0].to(DEV)
    ys = {}
    for B in (1, 3):
        mix, emb = mix3[:B], emb3[:B]
        chunks = SF.chunks_of(mix, m, n_chunks)
        st = net.make_streamer(B, DEV, use_graph=True, frames_per_chunk=m)
        assert st.graphs is not None and st.rings[0][0].shape[1] == m + 49 + 48
        y = ys[B] = SF.run_streamer(st, emb, chunks)
        assert tuple(y.shape) == (B, 2, SF.HOP * frames) and bool(torch.isfinite(y).all())
        # (a) the whole clip from the zero state
        whole, _ = net.predict(mix, emb, None, pad=False, want_state=False)
        ea = _err(y, whole)
        # (b) the one-frame streamer on the same samples
        s1 = single_frame[B]
        s1.reset()
        eb = _err(y, SF.run_streamer(s1, emb, SF.chunks_of(mix, 1, frames)))
        print(f"m={m} B={B}: vs whole clip {ea:.3g}, vs frames_per_chunk=1 {eb:.3g}")
        assert ea < TOL and eb < TOL, (m, B, ea, eb)
        # (c) graph replay equals the eager launches
        eager = net.make_streamer(B, DEV, use_graph=False, frames_per_chunk=m)
        assert torch.equal(SF.run_streamer(eager, emb, chunks), y), (m, B, "graph replay differs from eager")
        # (d) a second pass after reset()
        st.reset()
        assert torch.equal(SF.run_streamer(st, emb, chunks), y), (m, B, "second pass after reset() differs")
        if B == 1:
            alone = st
    # (e) every row of the batch of three against the same listener alone (row 0 alone is the B = 1 run above)
    for r in range(3):
        if r == 0:
            y1 = ys[1]
        else:
            alone.reset()
            y1 = SF.run_streamer(alone, emb3[r:r + 1], SF.chunks_of(mix3[r:r + 1], m, n_chunks))
        e = _err(ys[3][r], y1[0])
        print(f"m={m}: row {r} of B=3 vs alone {e:.3g}")
        assert e < ROW_TOL, (m, r, e)


def test_refusals(net):
    SF.refusals(net, DEV)
