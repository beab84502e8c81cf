"""CPU: the embedder stage cases of tests/test_gpu_embed_stages.py (tests/embed_stage_cases.py) on the hipemu emulator at tiny
shapes — one ragged and one exact shape per entry point, NaN-filled scratch, guard regions and the pad-is-zero assertions against
float64, with the same bounds.  The emulator's -DLH_LEGACY build also has the three-launch lh_emb_axis: it goes through the same
`axis` reference as an independent cross-check."""
import pytest

from lookoncetohear_amd import _cabi
from oracle import embedder_oracle as E
from tests.embed_stage_cases import FRONT_SCALES, EmbedRig, check
from tests.hipemu.hosts import EmuEmbed


@pytest.fixture(scope="module")
def rig():
    from tests.hipemu.build_emu import build_emu
    cfg = E.ECfg(**E.EMBED_PARAMS)
    net = EmuEmbed(**E.EMBED_PARAMS).eval()
    net.load_state_dict(E.synthetic_state_dict(cfg, 0), strict=True)
    return EmbedRig(_cabi.Lib(build_emu()), net, "cpu", 0)


def test_front_end(rig):
    """T = 4 (one ragged 14-frame tile) and T = 15 (a full tile + 1 frame), N = 64 (T - 1) + 31: reflect padding at an unaligned
    right edge; five utterances of far-apart scale; with and without the split side output."""
    check(rig.frontend(3, 64 * 3 + 31, FRONT_SCALES[:3], 1), "B=3 T=4 r=31")
    check(rig.frontend(5, 64 * 14 + 31, FRONT_SCALES, 0), "B=5 T=15 r=31")
    check(rig.frontend(1, 64 * 13, [1.0], 1), "B=1 T=14 r=0")


def test_intra_axis_fused(rig):
    """17 sequences: one full 16-sequence tile of k_emb_rec and a ragged one; both issue-priority settings."""
    check(rig.axis_fused(1, 17, 0, 0, 1, 0), "B=1 T=17")
    check(rig.axis_fused(1, 17, 0, 1, 0, 1), "B=1 T=17 prio")


def test_inter_axis_fused(rig):
    """P = T - 3 = 2 and 9: below and past the 8-slot position ring; 65 sequences = four tiles + 1."""
    check(rig.axis_fused(1, 5, 1, 0, 1), "B=1 T=5")
    check(rig.axis_fused(1, 12, 1, 1, 1), "B=1 T=12")


def test_inter_axis_matvec(rig):
    """B = 1: the eight-wave form, P = 33 (a 32-step chunk + 1); B = 2: the four-wave form."""
    check(rig.axis_mv(1, 36, 0, 1), "B=1 T=36")
    check(rig.axis_mv(2, 5, 1, 0), "B=2 T=5")


def test_legacy_axis_through_the_same_reference(rig):
    check(rig.axis_legacy(1, 5, 0), "B=1 T=5 intra")
    check(rig.axis_legacy(1, 5, 1), "B=1 T=5 inter")


def test_attention_block(rig):
    """B = 1: four of the eight batches the GEMM grids are rounded to; T = 5 and 65 (Tp = 64 and 128: one and two key tiles)."""
    check(rig.attn_block(1, 5, 1), "B=1 T=5")
    check(rig.attn_block(1, 65, 0), "B=1 T=65")
    check(rig.attn_block(1, 5, 0, peaked=True), "B=1 T=5 peaked")


def test_head(rig):
    check(rig.head(3, 1), "B=3 T=1")
    check(rig.head(3, 65), "B=3 T=65")
