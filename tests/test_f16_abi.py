"""CPU: the float16 storage mode at the C ABI -- every _bf16 entry point has an _f16 twin in
include/boxattn.h, the library and the ctypes bindings export them, and the library's code holds the
f16 instructions of the hot path (the f16 instantiations of the matrix-core and dot-product
kernels).  No compute calls: there is no GPU here."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import pytest
from capi_cases import HEADER, ROOT, header_declarations as declarations


F16_ENTRY_POINTS = [
    "%s_%s_f16" % (kind, op)
    for kind in ("boxattn", "instattn") for op in ("fwd", "bwd", "bwd_ws", "fwd_train")
] + ["boxattn_fwd_hl_f16", "boxattn_softmax_fwd_f16", "boxattn_softmax_bwd_f16",
     "boxattn_value_prep_f32_f16", "boxattn_value_prep_f16"]


@pytest.fixture(scope="module")
def lib():
    from boxer_amd import _lib
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_declares_every_f16_entry_point():
    decl = declarations()
    for name in F16_ENTRY_POINTS:
        assert name in decl, "missing declaration: " + name


def test_f16_twins_share_the_bf16_signatures():
    """The storage pointers are uint16_t * as for bf16: each twin's parameter list is its bf16 one."""
    decl = declarations()
    for name in F16_ENTRY_POINTS:
        if name.startswith("boxattn_value_prep"):
            continue
        assert decl[name] == decl[name[:-len("_f16")] + "_bf16"], name
    assert decl["boxattn_value_prep_f16"] == decl["boxattn_value_prep_bf16"]
    assert decl["boxattn_value_prep_f32_f16"] == decl["boxattn_value_prep_f32"]


def test_abi_version_stays_8_and_size_queries_keep_their_signature():
    text = open(HEADER).read()
    assert re.search(r"#define BOXATTN_ABI_VERSION 8\b", text)
    decl = declarations()
    for name in ("boxattn_plan_bytes", "boxattn_bwd_workspace_bytes"):
        assert decl[name].startswith("int is_16bit, int B, int S, int H, int C, int L, int Lq, int P,"), name


def test_library_and_bindings_export_the_f16_entry_points(lib):
    from boxer_amd import _lib
    for name in F16_ENTRY_POINTS:
        assert hasattr(lib, name), "missing export: " + name
        assert name in _lib.EXPORTS, "not bound: " + name
    handle = _lib.load()
    assert getattr(handle, "boxattn_bwd_f16").argtypes == getattr(handle, "boxattn_bwd_bf16").argtypes
    assert "f16" in _lib.build_info()


def _disassembly(path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_guard
    finally:
        sys.path.pop(0)
    text = []
    with tempfile.TemporaryDirectory() as tmp:
        for co in isa_guard.code_objects(path, tmp):
            text.append(subprocess.run([isa_guard.LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co],
                                       capture_output=True, text=True, check=True).stdout)
    return "\n".join(text)


def test_library_holds_the_f16_hot_path_instructions(lib):
    """The window-staged forward on v_mfma_f32_4x4x4_16b_f16, the binned accumulate on
    v_mfma_f32_32x32x16_f16, the point gradients on v_dot2c_f32_f16."""
    from boxer_amd import _lib
    asm = _disassembly(_lib.LIB_PATH)
    for insn in ("v_mfma_f32_4x4x4_16b_f16", "v_mfma_f32_32x32x16_f16", "v_dot2c_f32_f16"):
        assert re.search(r"\b%s(?:_e32|_e64)?\b" % insn, asm), insn


def test_f16_kernels_are_instantiated_without_scratch():
    """Both 16-bit instantiations of the window-staged and matrix-core kernels exist, and none of the f16
    kernels spills (the library-wide guards of test_capi_symbols cover the rest)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    from boxer_amd import _lib
    _lib.build()
    rows = kernel_resources.kernels(_lib.LIB_PATH)
    # (an older c++filt leaves names with _Float16 parameters mangled: DF16_ is the type's code there)
    is_f16 = lambda name: "_Float16" in name or "DF16_" in name
    for family in ("fwd_dense_kernel", "pointgrad_dense_kernel", "binned_accumulate_tr_kernel"):
        names = [r[0] for r in rows if family in r[0]]
        assert any(is_f16(n) for n in names) and any("unsigned short" in n for n in names), (family, names)
    f16 = [(r[0], r[4]) for r in rows if is_f16(r[0])]
    assert len(f16) > 50 and all(int(s) == 0 for _n, s in f16), f16


def test_f16_mfma_kernels_issue_no_packed_f32():
    """no kernel that issues an MFMA may contain a packed float32 instruction -- the f16
    instantiations live in the -fno-slp-vectorize translation unit like the bf16 ones."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_guard
    finally:
        sys.path.pop(0)
    from boxer_amd import _lib
    _lib.build()
    _n, n_mfma, offenders = isa_guard.scan(_lib.LIB_PATH)
    assert not offenders, offenders
