"""GPU: the Q/K/V frame kernel (`lh_qkv_proj_ln`, `lh_qkv_proj_ln_win`, the `ring_pos` one-frame form) is bit-identical to
the build that wrote tests/golden/qkv_bits.json (the commit named in that file).

The kernel's instruction schedule may change; its arithmetic may not: per output element the same products in the same order,
the same LayerNorm sums in the same order.  So the Q, K and V rows of seeded inputs are compared as SHA-256 of the whole
buffers — rows outside a window and behind the clip included (pre-filled with a bit pattern: they must stay untouched) —
at 1, 41 and 20 000 frames, for one window that is not tile-aligned, for the ring form, and for PReLU slopes above 1 (the
compare + select epilogue).  The pad features 582..607 of every written Q / K row must be exactly 0.  The inputs are hashed
too, so a golden that does not fit the generator fails as such and not as a kernel difference.

The golden is written by scripts/make_qkv_bits_golden.py on the GPU, from the build to compare against."""
import hashlib
import json
import os

import pytest
import torch

from lookoncetohear_amd import _cabi
from lookoncetohear_amd.net import Net
from lookoncetohear_amd.weights import KV_PAD_ROWS, QK_PAD
from oracle import tfgridnet_oracle as O
from tests.stage_cases import C, F, HIST, NH, PAT16, QKF, VF, Guarded, Rig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qkv_bits.json")

# name -> (B, T, window (t0, Tc) or None, ring position or None, PReLU slopes or None = the checkpoint's)
CASES = {
    "plain_1": (1, 1, None, None, None),
    "plain_41": (1, 41, None, None, None),
    "plain_20000": (32, 625, None, None, None),
    "plain_41_slopes_gt1": (1, 41, None, None, (1.5, 0.25, 2.0)),
    "win_41_t17_c23": (1, 41, (17, 23), None, None),
    "win_20000_t17_c23": (32, 625, (17, 23), None, None),
    "ring_1_pos7": (1, 1, None, 7, None),
    "ring_3_pos57": (3, 1, None, 57, None),
}


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def make_rig(sd):
    net = Net(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    return Rig(lib, net, DEV, torch.cuda.current_stream(DEV).cuda_stream, torch.cuda.synchronize)


def run_case(rig, name):
    """-> {"y", "q", "kx", "vx"}: SHA-256 of the input and of the three whole output buffers."""
    B, T, win, pos, slopes = CASES[name]
    gen = torch.Generator().manual_seed(20240 + sorted(CASES).index(name))
    y = torch.randn(B, T, F, C, generator=gen, dtype=torch.float32)
    y = (y * torch.logspace(-2, 2, B).reshape(B, 1, 1, 1)).to(DEV)           # utterances of different scale (row scaling path)
    rows = T + HIST + KV_PAD_ROWS
    q = Guarded((B * NH, T, 2 * QK_PAD), torch.float16, DEV).fill_pattern()
    kx = Guarded((B * NH, rows, 2 * QK_PAD), torch.float16, DEV).fill_pattern()
    vx = Guarded((B * NH, rows, 2 * VF), torch.float16, DEV).fill_pattern()
    bp = dict(rig.bp)
    if slopes is not None:
        bp["qkv_slopes"] = torch.tensor(slopes, dtype=torch.float32, device=DEV)
    ring = None if pos is None else torch.tensor([pos], dtype=torch.int32, device=DEV)
    args = [y, bp["qkv_w"], bp["qkv_b"], bp["qkv_slopes"], bp["lnq_w"], bp["lnq_b"], bp["lnk_w"], bp["lnk_b"], bp["lnv_w"],
            bp["lnv_b"], q.t, kx.t, vx.t, ring if ring is not None else None, B, T]
    if win is None:
        rig.call("lh_qkv_proj_ln", *args, rig.st)
    else:
        rig.call("lh_qkv_proj_ln_win", *args, *win, rig.st)
    rig.sync()
    for n, t in (("q", q), ("kx", kx), ("vx", vx)):
        t.check(f"{name}: {n}")
    # which rows were to be written
    t0, Tc = win if win is not None else (0, T)
    k0 = (pos % 50) if pos is not None else HIST + t0
    qi, ki, vi = (t.t.view(torch.int16) for t in (q, kx, vx))
    for n, a, lo in (("q", qi, t0), ("kx", ki, k0)):
        w = a[:, lo:lo + Tc].reshape(B * NH, Tc, QK_PAD // 8, 2, 8)          # [block][hi | lo][8 features]
        assert not bool(w[:, :, QKF // 8, :, QKF % 8:].any()) and not bool(w[:, :, QKF // 8 + 1:].any()), \
            f"{name}: pad features of {n} are not exactly 0"
        assert bool((a[:, :lo] == PAT16).all()) and bool((a[:, lo + Tc:] == PAT16).all()), f"{name}: {n} rows outside the window written"
    assert bool((vi[:, :k0] == PAT16).all()) and bool((vi[:, k0 + Tc:] == PAT16).all()), f"{name}: vx rows outside the window written"
    assert not bool((vi[:, k0:k0 + Tc] == PAT16).all(-1).any()), f"{name}: a vx row of the window was not written"
    return {"y": sha(y), "q": sha(q.t), "kx": sha(kx.t), "vx": sha(vx.t)}


@pytest.fixture(scope="module")
def rig(oracle_cfg_sd):
    return make_rig(oracle_cfg_sd[1])


@pytest.fixture(scope="module")
def golden_bits():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["producing_commit"], "the golden names the commit whose build wrote it"
    return g["cases"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_qkv_rows_bit_identical_to_golden_build(rig, golden_bits, name):
    got, want = run_case(rig, name), golden_bits[name]
    print(name, got)
    assert got["y"] == want["y"], f"{name}: the seeded input differs from the one the golden was written for"
    for n in ("q", "kx", "vx"):
        assert got[n] == want[n], f"{name}: {n} rows differ bitwise from the golden build"
