"""CPU: `Streamer(frames_per_chunk=m)` and its entry points (ABI 32: `lh_qkv_proj_ln` with `ring_pos` at T = m,
`lh_local_attn_ring`, `lh_ring_advance_by`) over the emulated library, eager; the argument checks also against the hipcc-built
gfx950 library (no launch: there is no GPU here).  The cases and the ring arithmetic they restate: tests/stream_frames_cases.py."""
import pytest
import torch

from lookoncetohear_amd import _cabi, synth
from oracle import tfgridnet_oracle as O
from tests import stream_frames_cases as SF
from tests.hipemu.hosts import EmuNet
from tests.stage_cases import Rig

TOL = 1e-4          # the project's working tolerance against the oracle (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def emu_net(oracle_cfg_sd):
    from tests.hipemu.build_emu import build_emu
    _, sd = oracle_cfg_sd
    net = EmuNet(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net.emu_lib = _cabi.Lib(build_emu())
    return net


@pytest.fixture(scope="module")
def rig(emu_net):
    return Rig(emu_net.emu_lib, emu_net, "cpu", 0)


@pytest.mark.parametrize("m", SF.ATTN_M)
def test_ring_attention_equals_contiguous_attention(rig, m):
    q, kx, vx, ref = SF.attn_contiguous(rig.call, rig.st, rig.sync, 1, m, "cpu")
    for pos in SF.attn_positions(m):
        out = SF.attn_on_ring(rig.call, rig.st, rig.sync, 1, m, pos, q, kx, vx, "cpu")
        assert torch.equal(out, ref), (m, pos, float((out - ref).abs().max()))


@pytest.mark.parametrize("m", SF.QKV_M)
def test_qkv_ring_write(rig, m):
    SF.qkv_ring_write(rig, 2, m, SF.qkv_positions(m))


def test_ring_advance_by_and_refusals(rig):
    SF.advance_by_cases(rig.lib.raw, rig.call, rig.st, rig.sync, "cpu")
    SF.refuse_17_frames(rig.lib.raw, rig.st)


def test_gfx950_library_validates_arguments():
    """The product library, built by hipcc, refuses the same arguments before it touches the device."""
    from lookoncetohear_amd.build import build_hip
    lib = _cabi.Lib(build_hip())
    SF.refuse_17_frames(lib.raw, None)
    assert lib.raw("lh_ring_advance_by")(None, 1, 50, None) == 1
    word = torch.zeros(1, dtype=torch.int32)
    assert lib.raw("lh_ring_advance_by")(word.data_ptr(), 0, 50, None) == 1
    assert lib.raw("lh_ring_advance_by")(word.data_ptr(), 51, 50, None) == 1


def _recorded(net, fn):
    """Runs fn() with the names of the C-ABI entries the host calls recorded."""
    lib, names = net.emu_lib, []
    orig = lib.call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)

    lib.call = call
    try:
        return fn(), names
    finally:
        del lib.call


def test_three_frames_per_chunk_end_to_end(emu_net, oracle_cfg_sd):
    """m = 3 (R = 52), 20 chunks = 60 frames: the ring wraps.  Against the oracle's `predict` over the same 3-frame chunks; a
    second pass after `reset()` reproduces the first chunks bit for bit; the launches are the ring forms, and m = 1 issues none
    of them."""
    cfg, sd = oracle_cfg_sd
    m, n_chunks = 3, 20
    d = synth.batch([8], SF.HOP * m * n_chunks + SF.LOOK)
    mix, emb = d["mixture"], d["embedding_gt"][:, 0]
    chunks = SF.chunks_of(mix, m, n_chunks)
    st = emu_net.make_streamer(1, "cpu", use_graph=False, frames_per_chunk=m)
    ys, names = _recorded(emu_net, lambda: SF.run_streamer(st, emb, chunks))
    assert tuple(ys.shape) == (1, 2, SF.HOP * m * n_chunks)
    assert int(st.pos[0]) == (m * n_chunks) % SF.ring_rows(m)
    assert names.count("lh_local_attn_ring") == emu_net.n_blocks * n_chunks and names.count("lh_ring_advance_by") == n_chunks
    assert "lh_local_attn" not in names and "lh_ring_advance" not in names
    ost, oouts = None, []
    for c in chunks:
        yo, ost = O.predict(cfg, sd, c, emb, ost, pad=False)
        oouts.append(yo)
    e = float((ys - torch.cat(oouts, -1)).abs().max())
    print("m = 3 streamer vs oracle predict:", e)
    assert e < TOL
    st.reset()
    again = SF.run_streamer(st, emb, chunks[:3])
    assert torch.equal(again, ys[..., :SF.HOP * m * 3])

    st1 = emu_net.make_streamer(1, "cpu", use_graph=False)
    assert st1.m == 1 and st1.rings[0][0].shape[1] == 1 + 49 + 48
    _, names1 = _recorded(emu_net, lambda: SF.run_streamer(st1, emb, SF.chunks_of(mix, 1, 2)))
    assert names1.count("lh_local_attn") == emu_net.n_blocks * 2 and names1.count("lh_ring_advance") == 2
    assert "lh_local_attn_ring" not in names1 and "lh_ring_advance_by" not in names1


def test_refusals(emu_net):
    SF.refusals(emu_net, "cpu")
