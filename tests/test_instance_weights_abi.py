"""CPU: the instance-attention weight passes at the C ABI -- instattn_weights_{fwd,bwd}_{f32,bf16,f16} are
declared in include/boxattn.h, exported by the built library and bound by the ctypes loader; the three types
share one parameter list up to the element type; the kernels exist for every type and use no scratch.  No
compute calls: there is no GPU here."""
import ctypes
import os
import re
import sys

import pytest
from capi_cases import HEADER, ROOT, header_declarations as declarations

NAMES = ["instattn_weights_%s_%s" % (way, suf) for way in ("fwd", "bwd") for suf in ("f32", "bf16", "f16")]


@pytest.fixture(scope="module")
def lib():
    from boxer_amd import _lib
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_six_entry_points_declared_exported_and_bound(lib):
    from boxer_amd import _lib
    decl = declarations()
    for name in NAMES:
        assert name in decl, "missing declaration: " + name
        assert hasattr(lib, name), "missing export: " + name
        assert name in _lib.EXPORTS, "not bound: " + name
    handle = _lib.load()
    for way, n_args in (("fwd", 7), ("bwd", 8)):
        types = [getattr(handle, "instattn_weights_%s_%s" % (way, suf)).argtypes for suf in ("f32", "bf16", "f16")]
        assert types[0] == types[1] == types[2] and len(types[0]) == n_args
        assert getattr(handle, "instattn_weights_%s_f32" % way).restype is ctypes.c_int


def test_the_three_types_share_one_parameter_list():
    decl = declarations()
    assert decl["instattn_weights_fwd_f32"] == (
        "const float *logits, long long rows, int L, int k, float *spatial_w, float *level_w, void *stream")
    assert decl["instattn_weights_bwd_f32"] == (
        "const float *logits, const float *grad_spatial_w, const float *grad_level_w, long long rows, int L, "
        "int k, float *grad_logits, void *stream")
    for way in ("fwd", "bwd"):
        f32 = decl["instattn_weights_%s_f32" % way]
        # the element type appears on the logits and, backward, on grad_logits; everything else is float32
        want = re.sub(r"float \*(logits|grad_logits)\b", r"uint16_t *\1", f32)
        assert want != f32
        assert decl["instattn_weights_%s_bf16" % way] == want
        assert decl["instattn_weights_%s_f16" % way] == want


def test_abi_version_is_still_8():
    from boxer_amd import _lib
    assert re.search(r"#define BOXATTN_ABI_VERSION 8\b", open(HEADER).read())
    assert _lib.ABI_VERSION == 8


def test_kernels_exist_for_every_type_without_scratch(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    from boxer_amd import _lib
    rows = kernel_resources.kernels(_lib.LIB_PATH)
    # (an older c++filt leaves names with _Float16 parameters mangled: DF16_ is the type's code there)
    types = {"float": lambda n: "<float," in n, "bf16": lambda n: "<unsigned short," in n,
             "f16": lambda n: "<_Float16," in n or "IDF16_" in n}
    for kernel in ("inst_weights_fwd_kernel", "inst_weights_bwd_kernel"):
        mine = [r for r in rows if kernel in r[0]]
        for label, is_type in types.items():
            assert any(is_type(r[0]) for r in mine), (kernel, label, [r[0] for r in mine])
        assert all(int(r[4]) == 0 for r in mine), [(r[0], r[4]) for r in mine]
