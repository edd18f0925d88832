"""CPU: box attention's inference forward from boxes and L*P logits at the C ABI -- boxattn_fwd_boxes_{f32, bf16, f16}
and the eligibility query boxattn_fwd_boxes_ok are declared in include/boxattn.h, exported and bound, the query equals
"the box flavour's forward route without host tables is the row gather, L <= 16, L*P <= 64" (expectations from
``boxattn_fwd_route``, nothing hard-coded), and the entry points refuse what the query refuses, a reference window or
offsets that do not fit the angle mode, and NULL required pointers, with hipErrorInvalidValue before any device call.
No compute calls: there is no GPU here."""
import ctypes
import itertools
import re

import pytest
from capi_cases import BOX_GEOMETRIES as GEOMETRIES, HEADER, INVALID_VALUE, declarations

ENTRY_POINTS = ["boxattn_fwd_boxes_" + suf for suf in ("f32", "bf16", "f16")]
GATHER = 2


@pytest.fixture(scope="module")
def lib():
    from boxer_amd import _lib
    _lib.build()
    _lib.set_variant(0)
    yield _lib
    _lib.set_variant(0)


def test_header_declares_the_four_names_and_the_bindings_know_them(lib):
    decl = declarations()
    for name in ENTRY_POINTS + ["boxattn_fwd_boxes_ok"]:
        assert name in decl, "missing declaration: " + name
        assert name in lib.EXPORTS, "not bound: " + name
        assert hasattr(ctypes.CDLL(lib.LIB_PATH), name), "missing export: " + name
    assert decl["boxattn_fwd_boxes_ok"] == "int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P"
    for name in ENTRY_POINTS:
        st = "float" if name.endswith("f32") else "uint16_t"
        assert decl[name] == (
            "const %s *value, const int64_t *shapes, const int64_t *lsi, const float *ref, int ref_dim, "
            "int ref_per_head, const float *offsets, int V, int angle_mode, const float *kernel_idx, "
            "const float *valid_ratios, const float *logits, int B, int S, int H, int C, int L, int Lq, int P, "
            "%s *out, void *stream" % (st, st)), name
        fn = getattr(lib.load(), name)
        assert len(fn.argtypes) == 21 and fn.restype is ctypes.c_int
    ok = lib.load().boxattn_fwd_boxes_ok
    assert len(ok.argtypes) == 9 and ok.restype is ctypes.c_int
    assert re.search(r"#define BOXATTN_ABI_VERSION 8\b", open(HEADER).read())        # nothing existing changed
    assert lib.load().boxattn_abi_version() == 8


def expected(lib, elem, aligned, dims):
    B, S, H, C, L, Lq, P = dims
    return lib.fwd_route(elem, 0, aligned, dims) == GATHER and L <= 16 and L * P <= 64


def test_query_equals_the_box_route_and_the_limits_on_L_and_LP(lib):
    seen = {True: 0, False: 0}
    for (levels, B, Lq, H), C, P, L, elem, aligned in itertools.product(
            GEOMETRIES, (8, 16, 32, 64), (1, 4, 9, 16, 64, 65), (1, 4, 16, 17), (2, 4, 8), (16, 8, 0)):
        S = sum(h * w for h, w in levels)
        dims = (B, S, H, C, L, Lq, P)
        want = expected(lib, elem, aligned, dims)
        assert lib.box_fwd_boxes_ok(elem, aligned, dims) == want, (dims, elem, aligned)
        seen[want] += 1
    assert seen[True] >= 20 and seen[False] >= 20, seen          # the grid holds both answers


def call(lib, name, ptrs, dims, ref_dim=4, V=4, angle_mode=0):
    """An entry call with fake (never dereferenced) pointers; ptrs: value, shapes, lsi, ref, offsets, kernel_idx,
    valid_ratios, logits, out."""
    v, sh, ls, ref, off, kid, vr, lg, out = ptrs
    return getattr(lib.load(), name)(v, sh, ls, ref, ref_dim, 0, off, V, angle_mode, kid, vr, lg, *dims, out, None)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_refuse_before_any_device_call(lib, name):
    """hipErrorInvalidValue for dimensions the query refuses, for a reference window or offsets that do not fit the
    angle mode and for NULL required pointers; a call without queries returns 0 having done nothing.  (An accepted
    call would launch: there is none here.)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    p -= p % 16
    p += 16
    all_ptrs = [p] * 9
    S = 9 * 11 + 4 * 5
    good = (2, S, 8, 32, 2, 4, 4)
    elem = 4 if name.endswith("f32") else 2
    assert lib.box_fwd_boxes_ok(elem, 16, good)
    refused = [(2, S, 8, 8, 2, 4, 4), (2, S, 8, 32, 1, 4, 65), (2, S, 8, 32, 17, 4, 1), (2, S, 8, 32, 4, 4, 17),
               (2, S, 8, 32, 2, 4, 0), (2, S, 0, 32, 2, 4, 4), (-1, S, 8, 32, 2, 4, 4)]
    for dims in refused:
        assert not lib.box_fwd_boxes_ok(elem, 16, dims), dims
        assert call(lib, name, all_ptrs, dims) == INVALID_VALUE, dims
    assert call(lib, name, all_ptrs, good, ref_dim=3) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, ref_dim=4, angle_mode=2) == INVALID_VALUE      # an angle needs ref_dim 5
    assert call(lib, name, all_ptrs, good, ref_dim=5, V=4, angle_mode=1) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, ref_dim=5, V=5, angle_mode=0) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, ref_dim=5, V=5, angle_mode=3) == INVALID_VALUE
    for missing in (0, 1, 2, 3, 4, 5, 7, 8):                               # every required pointer (6: optional)
        ptrs = list(all_ptrs)
        ptrs[missing] = None
        assert call(lib, name, ptrs, good) == INVALID_VALUE, missing
    lib.set_variant(1)
    try:
        assert not lib.box_fwd_boxes_ok(elem, 16, good)
        assert call(lib, name, all_ptrs, good) == INVALID_VALUE             # no generic fallback behind this entry
    finally:
        lib.set_variant(0)
    assert call(lib, name, [None] * 9, (2, S, 8, 32, 2, 0, 4)) == 0         # no queries: nothing to do


def test_python_surface():
    import inspect
    from boxer_amd import ops
    from boxer_amd.modules import Box3dAttention, BoxAttention
    p = inspect.signature(ops.box_attn_forward_boxes).parameters
    assert list(p) == ["value", "spatial_shapes", "level_start_index", "ref_windows", "offsets", "kernel_indices",
                       "valid_ratios", "logits", "angle_mode"]
    assert p["angle_mode"].default == 0
    assert callable(ops.box_forward_boxes_ok)
    assert list(inspect.signature(ops.box_forward_boxes_ok).parameters) == ["value", "num_level", "num_query",
                                                                            "num_point"]
    assert BoxAttention(32, 1, 2).fused_boxes is False and Box3dAttention(32, 1, 2).fused_boxes is False
