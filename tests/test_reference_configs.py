"""CPU: the drop-in classes are resolved the way the reference resolves its models — `utils.import_attr(model)(**model_params)`
(reference src/utils.py:7-9, src/ts_hear_embed_pl_module.py:25) — from the reference's OWN config files, with only the
dotted string changed as INTEGRATION.md prescribes; `config.TSH_PARAMS / EMBED_PARAMS` must equal those files.

The reference's configs/tsh.json and configs/embed.json are stored verbatim under tests/golden/reference_configs/, next to
class_methods.json: the methods each reference class defines, as listed from its source."""
import importlib
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_configs")

DROP_IN = {"src.models.tfgridnet_realtime.net.Net": "lookoncetohear_amd.net.Net",
           "src.models.tfgridnet_orig.tfgridnet.EmbedTFGridNet": "lookoncetohear_amd.embed_net.EmbedTFGridNet"}


def import_attr(import_path):                      # reference src/utils.py:7-9, restated (its module imports wandb)
    module, attr = import_path.rsplit(".", 1)
    return getattr(importlib.import_module(module), attr)


@pytest.mark.parametrize("cfg_name, const", [("tsh.json", "TSH_PARAMS"), ("embed.json", "EMBED_PARAMS")])
def test_reference_config_instantiates_the_drop_in(cfg_name, const):
    from lookoncetohear_amd import config
    args = json.load(open(os.path.join(GOLDEN, cfg_name)))["pl_module_args"]
    assert args["model"] in DROP_IN, args["model"]
    assert getattr(config, const) == args["model_params"]            # the restated constants track the reference files
    model = import_attr(DROP_IN[args["model"]])(**args["model_params"])
    ref_methods = json.load(open(os.path.join(GOLDEN, "class_methods.json")))[args["model"]]
    # same public surface as the reference class the string used to name
    for method in ("forward",) + (("predict", "init_buffers") if cfg_name == "tsh.json" else ()):
        assert method in ref_methods and callable(getattr(model, method))
    assert sum(p.numel() for p in model.parameters()) > 0
