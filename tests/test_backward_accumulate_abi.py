"""CPU: the backward's accumulate-kernel query at the C ABI -- ``boxattn_bwd_accumulate_kind`` is declared in
include/boxattn.h, exported by the built library and bound by the ctypes loader; option key 23 (``"inst_acc16"``)
exists; the route table: box attention (both storage widths, the float32 switch 19), instance attention in float32
and -- the new route -- in 16-bit storage under key 23.  The query is pure host code: there is no GPU here."""
import ctypes
import re

import numpy as np
import pytest
from capi_cases import C2, C2P, HEADER


VALU, TR, F32, SPLIT = range(4)
# What the measurement decided for 16-bit instance attention under key 23 = 0 (profiles/instance_accumulate16_step.log,
# DESIGN.md 4.2.2): C3' (235 200 points a slice) passed the step rule for both types and batch sizes, the 77 k and 19 k
# cells did not -- the matrix cores from 235 200 points up
DEFAULT_INST16 = {"C3": VALU, "C3p": TR}
OPT_INST_ACC16, OPT_ACC_F32 = 23, 19
INST16_VALU, INST16_TR = 1, 2

# instance workloads: levels, Lq, P
INST = {"C3": (C2, 300, 16), "C3p": (C2P, 300, 196)}


@pytest.fixture(scope="module")
def lib():
    from boxer_amd import _lib
    _lib.build()
    return _lib.load()


def kind(elem, instance, levels, Lq, P, B=2, H=8, C=32):
    from boxer_amd import _lib
    S = int(np.asarray(levels, dtype=np.int64).prod(1).sum())
    return _lib.bwd_accumulate_kind(elem, instance, (B, S, H, C, len(levels), S if Lq is None else Lq, P))


def test_query_declared_exported_bound_and_key_23(lib):
    from boxer_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+boxattn_bwd_accumulate_kind\s*\(([^;{]*?)\)\s*;", text, re.S)
    assert m, "boxattn_bwd_accumulate_kind is not declared"
    assert " ".join(m.group(1).split()) == (
        "int elem_bytes, int instance, int B, int S, int H, int C, int L, int Lq, int P")
    values = {name: int(v) for name, v in re.findall(r"#define\s+BOXATTN_ACC_(\w+)\s+(\d+)", text)}
    assert values == {"VALU": VALU, "TR": TR, "F32": F32, "SPLIT": SPLIT}
    assert (_lib.ACC_VALU, _lib.ACC_TR, _lib.ACC_F32, _lib.ACC_SPLIT) == (VALU, TR, F32, SPLIT)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "boxattn_bwd_accumulate_kind")
    assert "boxattn_bwd_accumulate_kind" in _lib.EXPORTS
    fn = lib.boxattn_bwd_accumulate_kind
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert _lib.OPTIONS["inst_acc16"] == OPT_INST_ACC16
    assert lib.boxattn_set_option(OPT_INST_ACC16, 1) != -1
    assert lib.boxattn_set_option(OPT_INST_ACC16, 0) == 1         # (the old value comes back)
    assert lib.boxattn_abi_version() == 8
    from boxer_amd import ops
    assert callable(ops.backward_accumulate_kind)


def test_box_attention_rows(lib):
    for key23 in (0, INST16_VALU, INST16_TR):                      # key 23 never changes a box-attention answer
        lib.boxattn_set_option(OPT_INST_ACC16, key23)
        for C in (16, 32, 64):
            assert kind(2, 0, C2, None, 4, C=C) == TR
        for key19, want in ((0, SPLIT), (1, VALU), (2, F32)):
            lib.boxattn_set_option(OPT_ACC_F32, key19)
            assert kind(4, 0, C2, None, 4) == want
        lib.boxattn_set_option(OPT_ACC_F32, 0)
        assert kind(4, 0, C2, None, 4, C=16) == VALU
    lib.boxattn_set_option(OPT_INST_ACC16, 0)


def test_float32_instance_rows(lib):
    for key23 in (0, INST16_VALU, INST16_TR):                      # ... nor a float32 answer
        lib.boxattn_set_option(OPT_INST_ACC16, key23)
        assert kind(4, 1, *INST["C3p"]) == SPLIT
        assert kind(4, 1, *INST["C3"]) == VALU
    lib.boxattn_set_option(OPT_INST_ACC16, 0)


@pytest.mark.parametrize("name", ["C3", "C3p"])
def test_16bit_instance_rows(lib, name):
    levels, Lq, P = INST[name]
    lib.boxattn_set_option(OPT_INST_ACC16, INST16_TR)
    for C in (16, 32, 64):
        assert kind(2, 1, levels, Lq, P, C=C) == TR
    assert kind(2, 1, levels, Lq, P, C=30) == VALU
    lib.boxattn_set_option(OPT_INST_ACC16, INST16_VALU)
    for C in (16, 32, 64):
        assert kind(2, 1, levels, Lq, P, C=C) == VALU
    lib.boxattn_set_option(OPT_INST_ACC16, 0)
    assert kind(2, 1, levels, Lq, P) == DEFAULT_INST16[name]
    assert kind(2, 1, levels, Lq, P, C=30) == VALU


def test_grad_mask_of_2_gib_takes_the_valu_walk(lib):
    """grad_mask (B, Lq, P, H, C) is fetched by 32-bit offsets: below 2 GiB only."""
    lib.boxattn_set_option(OPT_INST_ACC16, INST16_TR)
    levels, Lq, P = INST["C3p"]
    assert kind(2, 1, levels, Lq, P, B=35, C=64) == TR            # 35 x 300 x 196 x 8 x 64 x 2 bytes = 2^31 - 40 M
    assert kind(2, 1, levels, Lq, P, B=36, C=64) == VALU          # 36 x ...                     = 2^31 + 20 M
    lib.boxattn_set_option(OPT_INST_ACC16, 0)


def test_invalid_arguments(lib):
    for inst in (0, 1):
        assert kind(8, inst, C2P, 300, 196) < 0
        assert kind(3, inst, C2P, 300, 196) < 0
        assert kind(2, inst, C2P, 300, 0) < 0
        assert kind(2, inst, C2P, 300, 196, H=0) < 0
