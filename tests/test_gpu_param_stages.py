"""GPU: the stage kernels under parameters the synthetic state dict never takes (tests/param_cases.py): PReLU slopes on both
sides of 1, at 1, at 0 and below through every entry point of the two frame-kernel bodies; a layer's weight and bias times
2^-3, 2^-6, 2^-9 against max(existing bound, 4 x the fp32 yardstick computed in the test); the recurrences under small norm
weights and gate biases of U(+-6) and +-80.  Run: pytest -m gpu tests/test_gpu_param_stages.py -s (prints the hip error, the
yardstick and the bound of every case); with LOOKONCE_CURVE_DIR set, the weight-scale curve of the run is written to
weight_scale.json in that directory (profiles/weight_scale.json is a copy of one such run)."""
import json
import os

import pytest
import torch

from lookoncetohear_amd import _cabi
from lookoncetohear_amd.embed_net import EmbedTFGridNet
from lookoncetohear_amd.net import Net
from tests import param_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def mk(oracle_cfg_sd):
    lib = _cabi.load()
    _cabi.selftest_device(lib, 0)
    yield PC.Maker(lib, DEV, torch.cuda.current_stream(DEV).cuda_stream, torch.cuda.synchronize, Net, EmbedTFGridNet, oracle_cfg_sd[1])
    out = os.environ.get("LOOKONCE_CURVE_DIR")
    if PC.CURVE and out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "weight_scale.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "metric": "max|hip - ref| / max|ref| per utterance, worst utterance",
                       "bound": "max(existing bound, 4 x fp32)", "curve": PC.CURVE}, f, indent=1)


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
