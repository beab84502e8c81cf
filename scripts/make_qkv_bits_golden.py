"""Writes the golden of tests/test_gpu_qkv_bits.py: SHA-256 of the Q / K / V buffers the CURRENT build of the library (or the
one LOOKONCE_HIP_LIB names) produces for that test's seeded cases.  Run on the GPU with the build to compare against:

    python scripts/make_qkv_bits_golden.py <commit of that build> [out.json]      (default: tests/golden/qkv_bits.json)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import tfgridnet_oracle as O  # noqa: E402
from tests import test_gpu_qkv_bits as T  # noqa: E402

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
rig = T.make_rig(O.synthetic_state_dict(O.Cfg(**O.TSH_PARAMS), seed=0))
doc = {"producing_commit": commit,
       "what": "SHA-256 of the seeded input y and of the whole q / kx / vx buffers (bit pattern pre-fill, guards excluded) per case of "
               "tests/test_gpu_qkv_bits.py",
       "cases": {name: T.run_case(rig, name) for name in sorted(T.CASES)}}
with open(out, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(doc["cases"], indent=1))
