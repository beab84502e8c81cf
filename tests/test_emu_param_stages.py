"""CPU: the parameter cases of tests/test_gpu_param_stages.py (tests/param_cases.py) on the hipemu emulator — PReLU slopes on
both sides of 1, at 1, at 0 and below, weight scales of 2^-3 .. 2^-9 against the fp32 yardstick, and the recurrences under small
norm weights and wide gate biases, at the same shapes and with the same bounds."""
import pytest

from lookoncetohear_amd import _cabi
from tests import param_cases as PC
from tests.hipemu.hosts import EmuEmbed, EmuNet


@pytest.fixture(scope="module")
def mk(oracle_cfg_sd):
    from tests.hipemu.build_emu import build_emu
    return PC.Maker(_cabi.Lib(build_emu()), "cpu", 0, lambda: None, EmuNet, EmuEmbed, oracle_cfg_sd[1])


@pytest.mark.parametrize("qkv,proj", PC.SLOPES)
def test_slopes(mk, qkv, proj):
    PC.slope_case(mk, qkv, proj)


@pytest.mark.parametrize("k", PC.LOG2S)
@pytest.mark.parametrize("layer", sorted(PC.LAYERS))
def test_weight_scale(mk, layer, k):
    PC.weight_scale_case(mk, layer, k)


@pytest.mark.parametrize("which", sorted(PC.RECURRENCE))
def test_recurrence_parameters(mk, which):
    PC.recurrence_case(mk, which)
