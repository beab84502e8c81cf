"""Writes tests/golden/binaural_golden.npz: the reference's binaural cue metrics (src/eval/binaural.py: itd_diff, ild_diff
and the per-frame quantities behind them) on FLOAT64 copies of the inputs of tests/binaural_cases.py.

CPU only, and only where the reference checkout is importable (oracle/ref_stubs.REFERENCE_ROOT, or the path given as the
first argument).  The fixture holds the expected outputs and each case's parameters (JSON), no waveform:
    <name>/params                      JSON of the case (tests/binaural_cases.py regenerates the inputs from it)
    <name>/delta_itd, <name>/delta_ild [B]      itd_diff / ild_diff
    <name>/itd_est, itd_gt, ild_est, ild_gt, counted   [B, C] per segment (C = 1 in static mode; counted = chunk mask)

    python scripts/make_binaural_golden.py [REFERENCE_ROOT]
"""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_reference(root):
    path = os.path.join(root, "src", "eval", "binaural.py")
    spec = importlib.util.spec_from_file_location("reference_binaural", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_case(ref, case):
    from tests.binaural_cases import inputs
    est, gt = (a.astype(np.float64) for a in inputs(case))
    sr, moving = case["sr"], case["moving"]
    tmax = int(round(1e-3 * sr))
    out = dict(delta_itd=ref.itd_diff(est, gt, sr, moving=moving), delta_ild=ref.ild_diff(est, gt, sr, moving=moving))
    if moving:
        e, g, mask = ref.chunk_and_mask(est, gt, sr)            # (C, B, 2, FW), (C, B)
        e, g, mask = e.transpose(1, 0, 2, 3), g.transpose(1, 0, 2, 3), mask.T
    else:
        e, g, mask = est[:, None], gt[:, None], np.ones((len(est), 1), dtype=bool)
    out["itd_est"] = ref.compute_itd(e[..., 0, :], e[..., 1, :], sr, tmax)
    out["itd_gt"] = ref.compute_itd(g[..., 0, :], g[..., 1, :], sr, tmax)
    out["ild_est"] = ref.compute_ild(e[..., 0, :], e[..., 1, :])
    out["ild_gt"] = ref.compute_ild(g[..., 0, :], g[..., 1, :])
    out["counted"] = mask
    return out


def main():
    from oracle.ref_stubs import REFERENCE_ROOT
    from tests.binaural_cases import CASES
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else REFERENCE_ROOT)
    arrays = {}
    with np.errstate(divide="ignore", invalid="ignore"):       # silent channels: inf / NaN ILDs, empty means
        for case in CASES:
            arrays[case["name"] + "/params"] = np.array(json.dumps(case))
            for k, v in reference_case(ref, case).items():
                arrays[case["name"] + "/" + k] = np.asarray(v)
    out = os.path.join(ROOT, "tests", "golden", "binaural_golden.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
