"""GPU: every embedder entry point of include/lookonce_hip.h (lh_emb_frontend, lh_emb_axis_fused, lh_emb_axis_mv,
lh_emb_attn_block, lh_emb_head) against its float64 stage function (tests/embed_stage_cases.py) at the smallest shapes that reach
each edge of its launch code: tile and chunk boundaries, persistent loops, both recurrence forms of the inter axis, all eight
register softmax instantiations and the three-pass fallback, with NaN-filled scratch, guard regions and exact-zero pads.
Run: pytest -m gpu tests/test_gpu_embed_stages.py -s (prints each error next to its bound)."""
import pytest
import torch

from lookoncetohear_amd import _cabi
from lookoncetohear_amd.embed_net import EmbedTFGridNet
from oracle import embedder_oracle as E
from tests.embed_stage_cases import FRONT_SCALES, EmbedRig, check, cl
from tests.stage_cases import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BS = [1, 2, 3, 5]


@pytest.fixture(scope="module")
def net():
    cfg = E.ECfg(**E.EMBED_PARAMS)
    net = EmbedTFGridNet(**E.EMBED_PARAMS).eval()
    net.load_state_dict(E.synthetic_state_dict(cfg, 0), strict=True)
    return net.to(DEV)


@pytest.fixture(scope="module")
def rig(net):
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    return EmbedRig(lib, net, DEV, torch.cuda.current_stream(DEV).cuda_stream, torch.cuda.synchronize)


# ---- front end: k_emb_std, k_emb_stft_conv (14-frame tiles, reflect padding at an unaligned right edge), k_emb_gn_apply
@pytest.mark.parametrize("B", BS)
def test_front_end_tiles_and_right_edge(rig, B):
    for T in (4, 13, 14, 15, 28, 29, 43):
        for r in (0, 1, 31, 63):
            for emit in (0, 1):
                check(rig.frontend(B, 64 * (T - 1) + r, FRONT_SCALES[:B], emit), f"B={B} T={T} r={r} emit={emit}")


def test_front_end_persistent_loop(rig):
    """B = 3, N = 80000: 3 x 90 = 270 tiles on the 256 workgroups of k_emb_stft_conv."""
    for emit in (0, 1):
        check(rig.frontend(3, 80000, FRONT_SCALES[:3], emit), f"B=3 N=80000 emit={emit}")


# ---- intra axis: k_emb_lnsplit, k_emb_rec<false> (16-sequence tiles), k_emb_convt2<false> (80-row tiles)
INTRA = [(1, 4), (3, 5), (1, 15), (2, 8), (1, 16), (1, 17), (3, 11), (1, 33)]        # B T = 4, 15, 16, 17, 33


@pytest.mark.parametrize("prio", [0, 1])
def test_intra_axis_sequence_tiles(rig, prio):
    for have, emit in ((0, 0), (0, 1), (1, 0), (1, 1)):
        check(rig.axis_fused(1, 17, 0, have, emit, prio), f"B=1 T=17 have={have} emit={emit}")
    for B, T in INTRA:
        check(rig.axis_fused(B, T, 0, 1, 1, prio), f"B={B} T={T} have=1 emit=1")


def test_intra_axis_persistent_transposed_conv(rig):
    """B = 3, T = 171: 513 sequences = 513 tiles of k_emb_convt2 on its 512 workgroups."""
    check(rig.axis_fused(3, 171, 0, 1, 1), "B=3 T=171")
    check(rig.axis_fused(3, 171, 0, 0, 0), "B=3 T=171")


# ---- inter axis on k_emb_rec<true> (8-slot position ring: P = T - 3 = 7 / 8 / 9; 65 B sequences: ragged below B = 16) and
# k_emb_convt2<true> (64-row tiles: T = 63 / 64 / 65 / 129)
@pytest.mark.parametrize("B", BS)
def test_inter_axis_fused(rig, B):
    for T in (4, 5, 10, 11, 12, 19, 63, 64, 65, 67, 129):
        check(rig.axis_fused(B, T, 1, 1, 0), f"B={B} T={T} have=1 emit=0")
        check(rig.axis_fused(B, T, 1, 0, 1, prio=1), f"B={B} T={T} have=0 emit=1 prio")


def test_inter_axis_fused_large_grids(rig):
    check(rig.axis_fused(1, 449, 1, 1, 0), "B=1 T=449")               # 65 x 8 = 520 transposed-conv tiles
    check(rig.axis_fused(16, 12, 1, 1, 0), "B=16 T=12")               # 1040 sequences: every 16-sequence tile full
    check(rig.axis_fused(8, 20, 1, 1, 0), "B=8 T=20")                 # the first batch the product sends to k_emb_rec


# ---- inter axis on k_emb_inter_mv: 32-step chunks (P = 31 / 32 / 33 / 64 / 65 / 97), IS_NT for B = 1 and IS_NR above
@pytest.mark.parametrize("B", [1, 2, 3, 7])
def test_inter_axis_matvec(rig, B):
    for T in (4, 34, 35, 36, 67, 68, 100):
        check(rig.axis_mv(B, T, 1, 0), f"B={B} T={T} have=1 emit=0")
        check(rig.axis_mv(B, T, 0, 1), f"B={B} T={T} have=0 emit=1")


# ---- attention block: k_emb_qkv, k_emb_vt, k_gemm_nt3_occ3<0> / <1>, k_gemm_nt3_wide<1>, softmax, k_emb_proj
@pytest.mark.parametrize("B", BS)
def test_attention_block_gemm_tile_edges(rig, B):
    for T in (4, 63, 64, 65, 127, 128, 129, 193, 257):
        check(rig.attn_block(B, T, T % 2), f"B={B} T={T} emit={T % 2}")


@pytest.mark.parametrize("T", [513, 769, 1025, 1281, 1537, 1793])
def test_attention_block_softmax_instantiations(rig, T):
    """Tp = 576 .. 1856: k_emb_softmax_reg<3> .. <8> (<1>, <2> and <5> run in the tile-edge test and the realistic size)."""
    check(rig.attn_block(1, T, 0), f"B=1 T={T}")


def test_attention_block_three_pass_softmax(rig):
    """T = 2049, Tp = 2112 > 2048: k_emb_softmax."""
    check(rig.attn_block(1, 2049, 1), "B=1 T=2049")


@pytest.mark.parametrize("T", [65, 257, 2049])
def test_attention_block_peaked_softmax(rig, T):
    check(rig.attn_block(1, T, 0, peaked=True), f"B=1 T={T} peaked")


# ---- head: k_emb_head (64-frame tiles), k_emb_head_mean
@pytest.mark.parametrize("B", [1, 3])
def test_head_frame_tiles(rig, B):
    for T in (1, 2, 63, 64, 65, 129):
        check(rig.head(B, T), f"B={B} T={T}")


def test_realistic_size(rig):
    """B = 4 clips of 5 s (T = 1251): one call per entry point; k_emb_lnsplit beyond its 4096-workgroup grid."""
    B, N, T = 4, 80000, 1251
    check(rig.frontend(B, N, FRONT_SCALES[:B], 1), "B=4 N=80000")
    check(rig.axis_fused(B, T, 0, 0, 1), "B=4 T=1251 intra")
    check(rig.axis_fused(B, T, 1, 1, 0), "B=4 T=1251 inter")
    check(rig.axis_mv(B, T, 1, 0), "B=4 T=1251")
    check(rig.attn_block(B, T, 1), "B=4 T=1251")
    check(rig.head(B, T), "B=4 T=1251")


@pytest.mark.parametrize("B, N", [(2, 1280), (1, 64 * 79), (8, 4160)])
def test_debug_taps_on_the_device(rig, net, B, N):
    """`EmbedTFGridNet._debug_taps` (z0 and x1, x2, O, out of every block) against the composed float64 stages; B = 8: 2 x 8 x 65
    workgroups > 1024 sends the inter axis to k_emb_rec."""
    rig.seed("taps", B, N)
    x = rig.randn(B, 2, N)
    taps, otaps = {}, {}
    net._debug_taps = taps
    try:
        emb = net(x)
    finally:
        net._debug_taps = None
    torch.cuda.synchronize()
    z, _ = E.front_end(rig.cfg, rig.p, x.double())
    otaps["z0"] = cl(z)
    for i in range(rig.cfg.nblk):
        z = E.block(rig.cfg, rig.p, f"blocks.{i}.", z, otaps)
        otaps[f"blocks.{i}.out"] = cl(z)
    assert set(taps) == {"z0"} | {f"blocks.{i}.{n}" for i in range(rig.cfg.nblk) for n in ("x1", "x2", "O", "out")}
    res = {"tap." + k: rel_err(v, otaps[k], B) for k, v in taps.items()}
    res["tap.emb"] = rel_err(emb, E.head(rig.cfg, rig.p, z), B)
    assert all(bool(torch.isfinite(v).all()) for v in taps.values())
    check(res, f"B={B} N={N}")
