"""Cases of `Streamer(frames_per_chunk=m)` (ABI 32: `lh_qkv_proj_ln` with `ring_pos` at T = m, `lh_local_attn_ring`,
`lh_ring_advance_by`) shared by tests/test_emu_stream_frames.py (hipemu, CPU) and tests/test_gpu_stream_frames.py (MI355X).

The ring arithmetic is restated here from include/lookonce_hip.h ("frames per chunk"), not taken from the library: a ring of
R = 49 + m rows in the first R rows of buffers of m + 49 + 48 rows; frame j of a chunk is written to slot (pos + j) mod R;
logical history-extended row n is read from slot (pos + m + n) mod R.  `call(name, *args)` is a `Rig.call`: tensors go in as
pointers."""
from __future__ import annotations

import torch

from lookoncetohear_amd.weights import KV_PAD_ROWS, QK_PAD
from tests.stage_cases import C, F, HIST, NH, PAT16, QKF, VF, Guarded, split_qk, split_v

HOP = 128
LOOK = 64
ATTN_M = (2, 5, 16)
QKV_M = (2, 16)


def ring_rows(m: int) -> int:
    return HIST + m


def attn_positions(m: int) -> list:
    """No wrap, one step, the new rows ending on the ring's last slot, the new rows wrapping, the history wrapping."""
    R = ring_rows(m)
    return [0, 1, R - m, R - m + 1, R - 1]


def qkv_positions(m: int) -> list:
    """... and R + 3: a position outside [0, R) is taken modulo R as an unsigned number."""
    R = ring_rows(m)
    return [0, R - m + 1, R - 1, R + 3]


def read_slot(pos: int, m: int, n: int) -> int:
    return (pos + m + n) % ring_rows(m)


def write_slot(pos: int, m: int, j: int) -> int:
    return (pos + j) % ring_rows(m)


def attn_inputs(B: int, m: int, dev, seed: int = 0):
    """(q, kx, vx) for T = m in the contiguous layout: random split-precision rows 0 .. R - 1, the pad rows zero."""
    gen = torch.Generator().manual_seed(7100 + 37 * m + B + seed)
    R, rows = ring_rows(m), m + HIST + KV_PAD_ROWS
    q = split_qk(torch.randn(B * NH, m, QKF, generator=gen))
    kx = torch.zeros(B * NH, rows, 2 * QK_PAD, dtype=torch.float16)
    vx = torch.zeros(B * NH, rows, 2 * VF, dtype=torch.float16)
    kx[:, :R] = split_qk(torch.randn(B * NH, R, QKF, generator=gen))
    vx[:, :R] = split_v(torch.randn(B * NH, R, VF, generator=gen))
    return q.to(dev), kx.to(dev), vx.to(dev)


def to_ring(x: torch.Tensor, m: int, pos: int) -> torch.Tensor:
    """Rows 0 .. R - 1 of a contiguous buffer scattered into a ring by the read rule; the pad rows stay zero."""
    R = ring_rows(m)
    ring = torch.zeros_like(x)
    slots = torch.tensor([read_slot(pos, m, n) for n in range(R)], device=x.device)
    assert sorted(slots.tolist()) == list(range(R))
    ring[:, slots] = x[:, :R]
    return ring


def attn_contiguous(call, st, sync, B: int, m: int, dev):
    """The inputs and `lh_local_attn`'s output on them: the reference of every position of (B, m), computed once."""
    q, kx, vx = attn_inputs(B, m, dev)
    ref = Guarded((B, m, NH, F, 16), torch.float32, dev).fill_pattern()
    call("lh_local_attn", q, kx, vx, ref.t, B, m, st)
    sync()
    ref.check("lh_local_attn")
    assert bool(torch.isfinite(ref.t).all())
    return q, kx, vx, ref.t


def attn_on_ring(call, st, sync, B: int, m: int, pos: int, q, kx, vx, dev):
    out = Guarded((B, m, NH, F, 16), torch.float32, dev).fill_pattern()
    p = torch.tensor([pos], dtype=torch.int32, device=dev)
    kr, vr = to_ring(kx, m, pos), to_ring(vx, m, pos)
    kr0, vr0 = kr.clone(), vr.clone()
    call("lh_local_attn_ring", q, kr, vr, out.t, p, B, m, st)
    sync()
    out.check(f"lh_local_attn_ring m={m} pos={pos}")
    assert int(p[0]) == pos and torch.equal(kr, kr0) and torch.equal(vr, vr0), "the attention launch reads only"
    return out.t


def qkv_ring_write(rig, B: int, m: int, positions) -> None:
    """Test 2 of the feature: the ring form writes the chunk's K / V rows where the write rule says, with the bits of the
    `ring_pos = NULL` call, and nothing else."""
    dev = rig.dev
    R, rows = ring_rows(m), m + HIST + KV_PAD_ROWS
    bp = rig.bp
    y = rig.randn(B, m, F, C, scales=[1.0, 30.0][:B] if B <= 2 else None)

    def run(pos):
        q = Guarded((B * NH, m, 2 * QK_PAD), torch.float16, dev).fill_pattern()
        kx = Guarded((B * NH, rows, 2 * QK_PAD), torch.float16, dev).fill_pattern()
        vx = Guarded((B * NH, rows, 2 * VF), torch.float16, dev).fill_pattern()
        p = None if pos is None else torch.tensor([pos], dtype=torch.int32, device=dev)
        rig.call("lh_qkv_proj_ln", y, bp["qkv_w"], bp["qkv_b"], bp["qkv_slopes"], bp["lnq_w"], bp["lnq_b"], bp["lnk_w"],
                 bp["lnk_b"], bp["lnv_w"], bp["lnv_b"], q.t, kx.t, vx.t, p, B, m, rig.st)
        rig.sync()
        for n, t in (("q", q), ("kx", kx), ("vx", vx)):
            t.check(f"m={m} pos={pos}: {n}")
        if p is not None:
            assert int(p[0]) == pos, "the Q/K/V launch does not move the ring position"
        return tuple(t.t.view(torch.int16).clone() for t in (q, kx, vx))

    q0, k0, v0 = run(None)
    assert not bool((k0[:, HIST:HIST + m] == PAT16).all(-1).any()) and not bool((v0[:, HIST:HIST + m] == PAT16).all(-1).any())
    for pos in positions:
        q1, k1, v1 = run(pos)
        assert torch.equal(q1, q0), f"m={m} pos={pos}: Q rows"
        slots = [write_slot(pos, m, j) for j in range(m)]
        for name, ring, plain in (("kx", k1, k0), ("vx", v1, v0)):
            for j, s in enumerate(slots):
                assert torch.equal(ring[:, s], plain[:, HIST + j]), f"m={m} pos={pos}: {name} frame {j} in slot {s}"
            rest = [r for r in range(rows) if r not in slots]
            assert bool((ring[:, rest] == PAT16).all()), f"m={m} pos={pos}: {name} rows outside the chunk's slots written"


def advance_by_cases(call_raw, call, st, sync, dev) -> None:
    """Test 3: `lh_ring_advance_by` from the ring's last slot and from 0, and its refusals (raw return codes)."""
    for m in (2, 5, 16):
        R = ring_rows(m)
        for pos in (R - 1, 0, R - m):
            p = torch.tensor([pos, 0x5A5A], dtype=torch.int32, device=dev)
            call("lh_ring_advance_by", p, m, R, st)
            sync()
            assert p.tolist() == [(pos + m) % R, 0x5A5A], (m, pos, p.tolist())
    p = torch.zeros(1, dtype=torch.int32, device=dev)
    assert call_raw("lh_ring_advance_by")(p.data_ptr(), 0, 50, st) == 1
    assert call_raw("lh_ring_advance_by")(p.data_ptr(), 51, 50, st) == 1
    assert call_raw("lh_ring_advance_by")(None, 1, 50, st) == 1
    assert call_raw("lh_ring_advance_by")(p.data_ptr(), 1, (1 << 30) + 1, st) == 1
    sync()
    assert int(p[0]) == 0


def refuse_17_frames(call_raw, st) -> None:
    """Both ring entries refuse T = 17 (and T = 0, and null) before anything is launched: the pointers are never followed."""
    one = torch.zeros(16, dtype=torch.int32)          # a host word: only its address is passed
    a = one.data_ptr()
    args = [a] * 13
    assert call_raw("lh_qkv_proj_ln")(*args, a, 1, 17, st) == 1
    assert call_raw("lh_qkv_proj_ln_win")(*args, a, 1, 17, 0, 17, st) == 1
    assert call_raw("lh_qkv_proj_ln_win")(*args, a, 1, 16, 1, 15, st) == 1          # whole clip only
    assert call_raw("lh_local_attn_ring")(a, a, a, a, a, 1, 17, st) == 1
    assert call_raw("lh_local_attn_ring")(a, a, a, a, a, 1, 0, st) == 1
    assert call_raw("lh_local_attn_ring")(a, a, a, a, None, 1, 2, st) == 1
    assert call_raw("lh_local_attn_ring")(None, a, a, a, a, 1, 2, st) == 1


def chunks_of(mix: torch.Tensor, m: int, n_chunks: int) -> list:
    """`n_chunks` chunks of m frames: 128 m new samples plus the 64 of look-ahead each."""
    return [mix[:, :, i * HOP * m:(i + 1) * HOP * m + LOOK] for i in range(n_chunks)]


def run_streamer(st, emb: torch.Tensor, chunks: list) -> torch.Tensor:
    st.set_embedding(emb)
    return torch.cat([st.step(c).clone() for c in chunks], -1)


def refusals(net, dev) -> None:
    """Test 6: `frames_per_chunk` outside the integers 1..16 and a chunk of the wrong length raise ValueError."""
    import pytest
    for bad in (0, 17, 2.5, -1, True):
        with pytest.raises(ValueError, match="frames_per_chunk"):
            net.make_streamer(1, dev, use_graph=False, frames_per_chunk=bad)
    st = net.make_streamer(1, dev, use_graph=False, frames_per_chunk=2)
    assert tuple(st.chunk.shape) == (1, 2, 2 * HOP + LOOK) and tuple(st.out.shape) == (1, 2, 2 * HOP)
    assert all(tuple(kx.shape[:2]) == (NH, 2 + HIST + KV_PAD_ROWS) for kx, _ in st.rings)
    for n in (HOP + LOOK, 2 * HOP, 3 * HOP + LOOK):
        with pytest.raises(ValueError, match="chunk"):
            st.step(torch.zeros(1, 2, n, device=dev))
