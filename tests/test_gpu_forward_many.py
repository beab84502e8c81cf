"""GPU: `Net.forward_many` (several enrolled speakers per mixture, block 0 shared) and the fan-out form of block 0's closing
stage (`lh_proj_ln_res_fan` / `_win`, ABI 25).  The stage at the edges of its persistent grid against the single-gain kernel (bits)
and float64; the forward on 2 s clips pair by pair against `forward` and the float64 oracle, over the shapes where the shared
and the per-target part take different kernels and windows.  Run: pytest -m gpu tests/test_gpu_forward_many.py -s"""
import importlib.util
import os

import pytest
import torch

from lookoncetohear_amd import _cabi
from lookoncetohear_amd.net import Net
from oracle import tfgridnet_oracle as O
from tests.forward_many_cases import proj_ln_res_fan, scene
from tests.stage_cases import Rig, check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE = [1e-6, 1e4, 1.0, 3e-3, 250.0, 0.5, 1e-2, 7.0]          # per-utterance input scales, as in tests/test_gpu_stages.py
TOL = 1e-4                                                     # tests/test_gpu_parity.py: the HIP forward against the oracle
SAME_UTTERANCE = 2e-5                                          # ... and the same utterance in another batch shape
N = 32000                                                      # 2 s: T = 250 frames
SHAPES = [(1, 1), (1, 3), (2, 2), (4, 3)]


def _net(sd):
    net = Net(**O.TSH_PARAMS).eval()
    net.load_state_dict(sd, strict=True)
    # the fused / unfused crossing between 4 and 12 rows of 250 frames, as at 5 s (6000 frames: between 9 and 10 rows of 625)
    net.fuse_intra_min_frames = 2400
    return net.to(DEV)


@pytest.fixture(scope="module")
def net(oracle_cfg_sd):
    assert torch.cuda.is_available()
    return _net(oracle_cfg_sd[1])


@pytest.fixture(scope="module")
def rig(net):
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    return Rig(lib, net, DEV, torch.cuda.current_stream(DEV).cuda_stream, torch.cuda.synchronize)


# ---- the stage: 1, 511, 512, 513 and 1025 frames on the grid of min(B T, 512) persistent workgroups
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("B,T", [(1, 1), (7, 73), (8, 64), (3, 171), (5, 205)])
def test_fan_stage_at_the_grid_edges(rig, B, T, K):
    check(proj_ln_res_fan(rig, B, T, K, RANGE[:B]), f"B={B} T={T} K={K}")


@pytest.mark.parametrize("B,T,t0,Tc", [(3, 97, 33, 41), (1, 64, 17, 23)])
def test_fan_stage_windows(rig, B, T, t0, Tc):
    check(proj_ln_res_fan(rig, B, T, 3, RANGE[:B], win=(t0, Tc)), f"B={B} T={T} t0={t0} Tc={Tc} K=3")


# ---- the forward
@pytest.fixture(scope="module")
def clips():
    x, E = scene(4, 3, N)
    return x.to(DEV), E.to(DEV)


def _oracle_pairs(B, K):
    return [(0, 0), (B - 1, K - 1)]


@pytest.fixture(scope="module")
def oracle(oracle_cfg_sd, clips):
    """float64 oracle outputs of the pairs the shapes check, one batched CPU forward: {(b, k): y [2, N]}."""
    cfg, sd = oracle_cfg_sd
    x, E = clips[0].cpu(), clips[1].cpu()
    pairs = sorted({p for B, K in SHAPES for p in _oracle_pairs(B, K)})
    yo = O.forward(cfg, sd, torch.stack([x[b] for b, _ in pairs]), torch.stack([E[b, k] for b, k in pairs])[:, None],
                   dtype=torch.float64, fast_lstm=True)
    return {p: yo[i] for i, p in enumerate(pairs)}


@pytest.fixture(scope="module")
def alone(net, clips):
    """`forward` on one (mixture, speaker) pair alone, computed once per pair: alone(b, k) -> y [2, N]."""
    x, E = clips
    done = {}

    def get(b, k):
        if (b, k) not in done:
            done[(b, k)] = net(x[b:b + 1], E[b:b + 1, k:k + 1])[0].clone()
        return done[(b, k)]
    return get


@pytest.mark.parametrize("B,K", SHAPES)
def test_forward_many_pairs_oracle_and_windows(net, clips, oracle, alone, B, K):
    """(1, 3): block 0 on the per-sequence inter kernel in 2 windows, the rest on the tiled one in 3; (2, 2): block 0 whole-clip;
    (4, 3): block 0 on the unfused intra pair in 3 windows, the rest on the fused kernels in 2."""
    x, E = clips[0][:B], clips[1][:B, :K]
    y = net.forward_many(x, E)
    assert tuple(y.shape) == (B, K, 2, N) and bool(torch.isfinite(y).all())
    assert torch.equal(net.forward_many(x, E), y)                                   # no race between the parts and their windows
    for b in range(B):
        for k in range(K):
            e = float((y[b, k] - alone(b, k)).abs().max())
            print(f"B={B} K={K} [{b}, {k}] max|forward_many - forward alone| = {e:.3e}")
            assert e <= SAME_UTTERANCE, (b, k)
    for b, k in _oracle_pairs(B, K):
        e = float((y[b, k].cpu().double() - oracle[(b, k)]).abs().max())
        print(f"B={B} K={K} [{b}, {k}] max|forward_many - oracle64| = {e:.3e}")
        assert e < TOL, (b, k)
    assert torch.equal(net.forward_many(x, E[:, :1])[:, 0], net(x, E[:, :1]))       # K = 1 is `forward`
    auto = (net._n_time_chunks(B, 250, 1), net._n_time_chunks(B * K, 250, 1))
    saved = net.time_chunks, net.time_chunks_small
    net.time_chunks = net.time_chunks_small = 1
    try:
        assert net._n_time_chunks(B, 250, 1) == 1 and net._n_time_chunks(B * K, 250, 1) == 1
        y1 = net.forward_many(x, E)
    finally:
        net.time_chunks, net.time_chunks_small = saved
    print(f"B={B} K={K}: automatic windows {auto}")
    assert auto == {(1, 1): (2, 2), (1, 3): (2, 3), (2, 2): (1, 3), (4, 3): (3, 2)}[(B, K)]
    assert torch.equal(y1, y)


def test_nan_stays_in_its_mixture(oracle_cfg_sd, clips):
    net = _net(oracle_cfg_sd[1])                                # its own range flag
    x, E = clips[0][:2].clone(), clips[1][:2, :2]
    clean = net.forward_many(x, E)
    assert not net.range_status(DEV)
    x[1, 0, 5000] = float("nan")
    y = net.forward_many(x, E)
    torch.cuda.synchronize()
    assert all(not bool(torch.isfinite(y[1, k]).all()) for k in range(2))
    assert torch.equal(y[0], clean[0])
    with pytest.raises(RuntimeError, match="LH_ERR_RANGE"):    # deferred: raised when the next forward starts
        net.forward_many(clips[0][:2], E)


def test_bench_script_writes_its_file(tmp_path):
    """scripts/bench_forward_many.py on one small shape, in this process: it runs both arms and writes the table."""
    spec = importlib.util.spec_from_file_location("bench_forward_many", os.path.join(ROOT, "scripts", "bench_forward_many.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "forward_many_cost.txt"
    mod.main(["--out", str(out), "--shapes", "2x2", "--seconds", "1", "--steps", "2", "--blocks", "2", "--warmup", "1"])
    text = out.read_text()
    assert "B = 2, K = 2: forward on 4 rows p50" in text and "forward_many: p50" in text and "three times the scatter" in text
