"""CPU: the cache policy of the activation streams (csrc/lh_cachepol.h) in the product code object.  Every frame kernel that
carries a policy exists twice: POL 0 must be free of non-temporal accesses (it is what small batches and streaming run), POL 1
must have some; the attention kernel keeps plain loads for the K / V rows its neighbouring tile re-reads; no other kernel of
the library has a non-temporal access; and lh_set_tuning(19, v) takes exactly 0, 1, 2.  Only the `nt` modifier is looked at —
instruction counts move with unrolling."""
import os
import re

import pytest

from lookoncetohear_amd import _cabi
from lookoncetohear_amd import build

POLICY_KERNELS = ("k_qkv_proj_ln", "k_local_attn", "k_proj_ln_res")
ATT_K_LD, ATT_V_LD = 3, 4            # bits of lh::cp::Stream


@pytest.fixture(scope="module")
def kernels():
    """mangled kernel name -> its global loads / stores, as llvm-objdump prints them"""
    text = build.disassemble_lib(build.build_hip(verbose=False))
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and re.search(r"\bglobal_(load|store)", line):
            cur.append(line.strip())
    assert any("k_local_attn" in k for k in out), "could not disassemble the gfx950 code object"
    return out


def _is_nt(ins: str) -> bool:
    return re.search(r"\bnt\b", ins.split("//")[0]) is not None


def _policy(name: str):
    """(kernel, POL) of an instantiation of a policy kernel: POL is its last template argument"""
    for k in POLICY_KERNELS:
        m = re.search(k + r"I.*Li(\d)EEEv", name)
        if m:
            return k, int(m.group(1))
    return None


def _mask() -> int:
    src = open(os.path.join(build.CSRC, "lh_cachepol.h")).read()
    return int(re.search(r"#define LH_NT_MASK (0x[0-9a-fA-F]+)u", src).group(1), 16)


def test_pol0_is_plain_and_pol1_is_not(kernels):
    seen = {}
    for name, acc in kernels.items():
        p = _policy(name)
        if p is None:
            continue
        seen.setdefault(p[0], set()).add(p[1])
        n_nt = sum(_is_nt(a) for a in acc)
        if p[1] == 0:
            assert n_nt == 0, (name, [a for a in acc if _is_nt(a)][:3])
        else:
            assert n_nt > 0, name
    assert set(seen) == set(POLICY_KERNELS) and all(0 in v and 1 in v for v in seen.values()), seen


def test_attention_keeps_plain_loads_for_shared_rows(kernels):
    if _mask() >> ATT_K_LD & 1 and _mask() >> ATT_V_LD & 1:
        return                        # the committed table sends K and V non-temporal: nothing to keep
    for name, acc in kernels.items():
        if _policy(name) == ("k_local_attn", 1):
            plain = [a for a in acc if "global_load" in a and not _is_nt(a)]
            assert plain, name


def test_no_other_kernel_is_non_temporal(kernels):
    for name, acc in kernels.items():
        if _policy(name) is None:
            assert not any(_is_nt(a) for a in acc), name


def test_tuning_key_19():
    lib = _cabi.Lib(build.build_hip(verbose=False))
    try:
        for v in (0, 1, 2):
            assert lib.raw("lh_set_tuning")(19, v) == 0
        assert lib.raw("lh_set_tuning")(19, 3) == 1          # LH_ERR_ARG
        assert lib.raw("lh_set_tuning")(19, -1) == 1
    finally:
        lib.raw("lh_set_tuning")(19, 1)
