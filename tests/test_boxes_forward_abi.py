"""CPU: instance attention's inference forward from boxes and 2x2 logits at the C ABI -- instattn_fwd_boxes_{f32, bf16,
f16} and the eligibility query instattn_fwd_boxes_ok are declared in include/boxattn.h, exported and bound, the query
equals "the instance flavour's forward route is the wave-per-pair family, k even, 2 <= k <= 32, L <= 16" (expectations
from ``boxattn_fwd_route``, nothing hard-coded), and the entry points refuse what the query refuses, and NULL required
pointers, with hipErrorInvalidValue before any device call.  No compute calls: there is no GPU here."""
import ctypes
import itertools
import re

import pytest
from capi_cases import HEADER, INST_GEOMETRIES as GEOMETRIES, INVALID_VALUE, declarations

ENTRY_POINTS = ["instattn_fwd_boxes_" + suf for suf in ("f32", "bf16", "f16")]
WIDE = 3


@pytest.fixture(scope="module")
def lib():
    from boxer_amd import _lib
    _lib.build()
    _lib.set_variant(0)
    yield _lib
    _lib.set_variant(0)


def test_header_declares_the_four_names_and_the_bindings_know_them(lib):
    decl = declarations()
    for name in ENTRY_POINTS + ["instattn_fwd_boxes_ok"]:
        assert name in decl, "missing declaration: " + name
        assert name in lib.EXPORTS, "not bound: " + name
        assert hasattr(ctypes.CDLL(lib.LIB_PATH), name), "missing export: " + name
    assert decl["instattn_fwd_boxes_ok"] == "int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int k"
    for name in ENTRY_POINTS:
        st = "float" if name.endswith("f32") else "uint16_t"
        assert decl[name].startswith("const %s *value, const int64_t *shapes, const int64_t *lsi, const float *ref, "
                                     "int ref_dim, int ref_per_head, const float *offsets" % st), name
        assert decl[name].endswith("int k, %s *out, %s *mask_out, void *stream" % (st, st)), name
        fn = getattr(lib.load(), name)
        assert len(fn.argtypes) == 20 and fn.restype is ctypes.c_int
    assert re.search(r"#define BOXATTN_ABI_VERSION 8\b", open(HEADER).read())        # nothing existing changed


def expected(lib, elem, aligned, dims, k):
    B, S, H, C, L, Lq = dims
    return (lib.fwd_route(elem, 1, aligned, (B, S, H, C, L, Lq, k * k)) == WIDE
            and k % 2 == 0 and 2 <= k <= 32 and L <= 16)


def test_query_equals_the_instance_route_and_the_limits_on_k_and_L(lib):
    seen = {True: 0, False: 0}
    for (levels, B, Lq, H), C, k, elem, aligned in itertools.product(
            GEOMETRIES, (8, 16, 32, 64), (2, 3, 4, 6, 14, 32, 34), (2, 4), (16, 8, 0)):
        S, L = sum(h * w for h, w in levels), len(levels)
        dims = (B, S, H, C, L, Lq)
        want = expected(lib, elem, aligned, dims, k)
        assert lib.fwd_boxes_ok(elem, aligned, dims, k) == want, (dims, k, elem, aligned)
        seen[want] += 1
    assert seen[True] >= 20 and seen[False] >= 20, seen          # the grid holds both answers


def test_query_is_zero_outside_the_family(lib):
    S, ok = 9 * 11 + 4 * 5, (2, 9 * 11 + 4 * 5, 8, 32, 2, 4)
    assert lib.fwd_boxes_ok(4, 16, ok, 14) and lib.fwd_boxes_ok(2, 16, ok, 14)
    for k in (1, 3, 5, 13, 33, 34, 0, -2):                                  # odd, too large, nonsense
        assert not lib.fwd_boxes_ok(4, 16, ok, k), k
    assert not lib.fwd_boxes_ok(4, 16, (2, 17, 8, 32, 17, 4), 14)           # L = 17
    assert lib.fwd_route(4, 1, 16, (2, 16, 8, 32, 16, 4, 196)) == WIDE
    assert lib.fwd_boxes_ok(4, 16, (2, 16, 8, 32, 16, 4), 14)               # L = 16 is in
    assert not lib.fwd_boxes_ok(4, 16, (2, S, 8, 8, 2, 4), 14)              # C = 8: no fast kernels
    assert not lib.fwd_boxes_ok(4, 0, ok, 14) and not lib.fwd_boxes_ok(2, 0, ok, 14)      # aligned = 0
    assert not lib.fwd_boxes_ok(8, 16, ok, 14)                              # float64 has no such kernel
    lib.set_variant(1)
    try:
        assert not lib.fwd_boxes_ok(4, 16, ok, 14)                          # generic kernels only
    finally:
        lib.set_variant(0)
    assert lib.fwd_boxes_ok(4, 16, ok, 14)


def call(lib, name, ptrs, dims, k, ref_dim=4):
    """An entry call with fake (never dereferenced) pointers; ptrs: value, shapes, lsi, ref, offsets, kernel_idx,
    valid_ratios, logits, out, mask_out."""
    v, sh, ls, ref, off, kid, vr, lg, out, mk = ptrs
    return getattr(lib.load(), name)(v, sh, ls, ref, ref_dim, 0, off, kid, vr, lg, *dims, k, out, mk, None)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_refuse_before_any_device_call(lib, name):
    """hipErrorInvalidValue for dimensions the query refuses and for NULL required pointers; a call without queries
    returns 0 having done nothing.  (An accepted call would launch: there is none here.)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    p -= p % 16
    p += 16
    all_ptrs = [p] * 10
    S = 9 * 11 + 4 * 5
    good = (2, S, 8, 32, 2, 4)
    elem = 4 if name.endswith("f32") else 2
    assert lib.fwd_boxes_ok(elem, 16, good, 14)
    for dims, k in [((2, S, 8, 8, 2, 4), 14), (good, 13), (good, 34), ((2, 17, 8, 32, 17, 4), 14),
                    ((2, S, 8, 32, 2, 4), 0), ((2, S, 0, 32, 2, 4), 14), ((-1, S, 8, 32, 2, 4), 14)]:
        assert call(lib, name, all_ptrs, dims, k) == INVALID_VALUE, (dims, k)
    small = (2, 6 * 5, 8, 32, 1, 4)
    if not lib.fwd_boxes_ok(elem, 16, small, 2):                            # k = 2: the row gather's shape
        assert call(lib, name, all_ptrs, small, 2) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, 14, ref_dim=3) == INVALID_VALUE
    for missing in (0, 1, 2, 3, 4, 5, 7, 8):                               # every required pointer (6, 9: optional)
        ptrs = list(all_ptrs)
        ptrs[missing] = None
        assert call(lib, name, ptrs, good, 14) == INVALID_VALUE, missing
    lib.set_variant(1)
    try:
        assert call(lib, name, all_ptrs, good, 14) == INVALID_VALUE         # no generic fallback behind this entry
    finally:
        lib.set_variant(0)
    assert call(lib, name, [None] * 10, (2, S, 8, 32, 2, 0), 14) == 0       # no queries: nothing to do


def test_python_surface():
    import inspect
    from boxer_amd import ops
    from boxer_amd.modules import InstanceAttention
    p = inspect.signature(ops.instance_attn_forward_boxes).parameters
    assert list(p) == ["value", "spatial_shapes", "level_start_index", "ref_windows", "offsets", "kernel_indices",
                       "valid_ratios", "logits", "kernel_size", "need_mask"]
    assert callable(ops.forward_boxes_ok)
    assert InstanceAttention(32, 1, 2, 4).fused_boxes is False
