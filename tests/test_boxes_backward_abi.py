"""CPU: instance attention's box and logit gradients from boxes and 2x2 logits at the C ABI -- instattn_bwd_boxes_{f32,
bf16, f16} and the eligibility query instattn_bwd_boxes_ok are declared in include/boxattn.h, exported and bound, the
query equals instattn_fwd_boxes_ok, and the entry points refuse what the query refuses, ref_dim < 4 and NULL required
pointers, with hipErrorInvalidValue before any device call.  No compute calls: there is no GPU here."""
import ctypes
import inspect
import itertools
import re

import pytest

from capi_cases import HEADER, INST_GEOMETRIES as GEOMETRIES, INVALID_VALUE, declarations

ENTRY_POINTS = ["instattn_bwd_boxes_" + suf for suf in ("f32", "bf16", "f16")]
OK = "instattn_bwd_boxes_ok"


@pytest.fixture(scope="module")
def lib():
    from boxer_amd import _lib
    _lib.build()
    _lib.set_variant(0)
    yield _lib
    _lib.set_variant(0)


def test_header_declares_the_four_names_and_the_bindings_know_them(lib):
    decl = declarations()
    for name in ENTRY_POINTS + [OK]:
        assert name in decl, "missing declaration: " + name
        assert name in lib.EXPORTS, "not bound: " + name
        assert hasattr(ctypes.CDLL(lib.LIB_PATH), name), "missing export: " + name
    assert decl[OK] == "int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int k"
    for name in ENTRY_POINTS:
        st = "float" if name.endswith("f32") else "uint16_t"
        assert decl[name] == (
            "const %s *value, const int64_t *shapes, const int64_t *lsi, const float *ref, int ref_dim, "
            "int ref_per_head, const float *offsets, const float *kernel_idx, const float *valid_ratios, "
            "const float *logits, const %s *grad_out, const %s *grad_mask, int B, int S, int H, int C, int L, int Lq, "
            "int k, float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream" % (st, st, st)), name
        fn = getattr(lib.load(), name)
        assert len(fn.argtypes) == 23 and fn.restype is ctypes.c_int
    assert lib.load().instattn_bwd_boxes_ok.argtypes == [ctypes.c_int] * 9
    assert re.search(r"#define BOXATTN_ABI_VERSION 8\b", open(HEADER).read())        # nothing existing changed
    assert lib.ABI_VERSION == 8 and lib.load().boxattn_abi_version() == 8


def test_query_equals_the_forward_query(lib):
    seen = {True: 0, False: 0}
    for (levels, B, Lq, H), C, k, elem, aligned in itertools.product(
            GEOMETRIES, (8, 16, 32, 64), (2, 3, 4, 6, 14, 32, 34), (2, 4), (16, 8, 0)):
        S, L = sum(h * w for h, w in levels), len(levels)
        dims = (B, S, H, C, L, Lq)
        want = lib.fwd_boxes_ok(elem, aligned, dims, k)
        assert lib.bwd_boxes_ok(elem, aligned, dims, k) == want, (dims, k, elem, aligned)
        seen[want] += 1
    assert seen[True] >= 20 and seen[False] >= 20, seen          # the grid holds both answers
    ok = (2, 9 * 11 + 4 * 5, 8, 32, 2, 4)
    lib.set_variant(1)
    try:
        assert not lib.bwd_boxes_ok(4, 16, ok, 14)                # generic kernels only
    finally:
        lib.set_variant(0)
    assert lib.bwd_boxes_ok(4, 16, ok, 14) and not lib.bwd_boxes_ok(8, 16, ok, 14)


# value, shapes, lsi, ref, offsets, kernel_idx, valid_ratios, logits, grad_out, grad_mask, grad_offsets, grad_ref_rows,
# grad_logits
OPTIONAL = (6, 9, 11)


def call(lib, name, ptrs, dims, k, ref_dim=4):
    """An entry call with fake (never dereferenced) pointers."""
    v, sh, ls, ref, off, kid, vr, lg, go, gm, goff, grows, glog = ptrs
    return getattr(lib.load(), name)(v, sh, ls, ref, ref_dim, 0, off, kid, vr, lg, go, gm, *dims, k, goff, grows, glog,
                                     None)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_refuse_before_any_device_call(lib, name):
    """hipErrorInvalidValue for dimensions the query refuses, ref_dim 3 and NULL required pointers; a call without
    queries returns 0 having done nothing.  (An accepted call would launch: there is none here.)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    p -= p % 16
    p += 16
    all_ptrs = [p] * 13
    S = 9 * 11 + 4 * 5
    good = (2, S, 8, 32, 2, 4)
    elem = 4 if name.endswith("f32") else 2
    assert lib.bwd_boxes_ok(elem, 16, good, 14)
    for dims, k in [(good, 13), (good, 34), ((2, 17, 8, 32, 17, 4), 14), ((2, S, 8, 8, 2, 4), 14),
                    (good, 0), ((2, S, 0, 32, 2, 4), 14), ((-1, S, 8, 32, 2, 4), 14)]:
        assert not lib.bwd_boxes_ok(elem, 16, dims[:6], k), (dims, k)
        assert call(lib, name, all_ptrs, dims, k) == INVALID_VALUE, (dims, k)
    assert call(lib, name, all_ptrs, good, 14, ref_dim=3) == INVALID_VALUE
    for missing in range(13):
        ptrs = list(all_ptrs)
        ptrs[missing] = None
        if missing in OPTIONAL:
            continue                                                         # (accepted: it would launch)
        assert call(lib, name, ptrs, good, 14) == INVALID_VALUE, missing
    lib.set_variant(1)
    try:
        assert call(lib, name, all_ptrs, good, 14) == INVALID_VALUE         # no generic fallback behind this entry
    finally:
        lib.set_variant(0)
    assert call(lib, name, [None] * 13, (2, S, 8, 32, 2, 0), 14) == 0       # no queries: nothing to do


def test_python_surface():
    import boxer_amd
    from boxer_amd import ops
    from boxer_amd.modules import InstanceAttention
    assert list(inspect.signature(ops.backward_boxes_ok).parameters) == ["value", "num_level", "num_query",
                                                                         "kernel_size"]
    p = inspect.signature(ops.instance_attn_backward_boxes).parameters
    assert list(p) == ["value", "spatial_shapes", "level_start_index", "ref_windows", "offsets", "kernel_indices",
                       "valid_ratios", "logits", "kernel_size", "grad_output", "grad_mask_output", "need_ref_grad"]
    assert p["need_ref_grad"].default is False
    assert "InstanceAttnBoxesFunction" in boxer_amd.__all__
    assert boxer_amd.InstanceAttnBoxesFunction is boxer_amd.functions.InstanceAttnBoxesFunction
    m = InstanceAttention(32, 1, 2, 4)
    assert m.fused_boxes_train is False and m.fused_boxes is False
