"""CPU: the window-staged forward from boxes and L*P logits at the C ABI -- boxattn_fwd_boxes_hl_{f32, bf16, f16} and
the eligibility query boxattn_fwd_boxes_hl_ok are declared in include/boxattn.h, exported and bound, the query equals
"the box flavour's forward route WITH these host tables is the window-staged family" (expectations from
``boxattn_fwd_route``, nothing hard-coded), and the entry points refuse what the query refuses, a reference window or
offsets that do not fit the angle mode, NULL required pointers and NULL host tables, with hipErrorInvalidValue before
any device call.  No compute calls: there is no GPU here."""
import ctypes
import itertools
import re

import pytest

from capi_cases import HEADER, INVALID_VALUE, STAGED_GEOMETRIES as GEOMETRIES, declarations, host_tables

ENTRY_POINTS = ["boxattn_fwd_boxes_hl_" + suf for suf in ("f32", "bf16", "f16")]
QUERY = "boxattn_fwd_boxes_hl_ok"
STAGED = 4


@pytest.fixture(scope="module")
def lib():
    from boxer_amd import _lib
    _lib.build()
    _lib.set_variant(0)
    yield _lib
    _lib.set_variant(0)


def test_header_declares_the_four_names_and_the_bindings_know_them(lib):
    decl = declarations()
    for name in ENTRY_POINTS + [QUERY]:
        assert name in decl, "missing declaration: " + name
        assert name in lib.EXPORTS, "not bound: " + name
        assert hasattr(ctypes.CDLL(lib.LIB_PATH), name), "missing export: " + name
    assert decl[QUERY] == ("int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P, "
                           "const int64_t *shapes_host, const int64_t *lsi_host")
    for name in ENTRY_POINTS:
        st = "float" if name.endswith("f32") else "uint16_t"
        assert decl[name] == (
            "const %s *value, const int64_t *shapes, const int64_t *lsi, const float *ref, int ref_dim, "
            "int ref_per_head, const float *offsets, int V, int angle_mode, const float *kernel_idx, "
            "const float *valid_ratios, const float *logits, int B, int S, int H, int C, int L, int Lq, int P, "
            "%s *out, const int64_t *shapes_host, const int64_t *lsi_host, void *stream" % (st, st)), name
        # ... the parameters of boxattn_fwd_boxes_* plus the two host tables before stream
        assert decl[name].replace(" const int64_t *shapes_host, const int64_t *lsi_host,", "") == \
            decl[name.replace("_hl_", "_")]
        fn = getattr(lib.load(), name)
        assert len(fn.argtypes) == 23 and fn.restype is ctypes.c_int
    ok = getattr(lib.load(), QUERY)
    assert len(ok.argtypes) == 11 and ok.restype is ctypes.c_int
    assert re.search(r"#define BOXATTN_ABI_VERSION 8\b", open(HEADER).read())        # nothing existing changed
    assert lib.load().boxattn_abi_version() == 8 and lib.ABI_VERSION == 8


def test_query_equals_the_staged_route_with_the_host_tables(lib):
    seen = {True: 0, False: 0}
    kinds = set()
    try:
        for variant in (0, 1):
            lib.set_variant(variant)
            for (levels, B, H), C, P, L, lq_off, elem, aligned, broken in itertools.product(
                    GEOMETRIES, (16, 32, 64), (4, 9), (None, 5), (0, 1), (2, 4), (16, 8, 0), (False, True)):
                shapes, lsi, S = host_tables(levels, L, broken)
                dims = (B, S, H, C, len(shapes), S + lq_off, P)
                want = lib.fwd_route(elem, 0, aligned, dims, shapes, lsi) == STAGED
                assert lib.box_fwd_boxes_hl_ok(elem, aligned, dims, shapes, lsi) == want, (dims, elem, aligned, broken)
                assert not lib.box_fwd_boxes_hl_ok(elem, aligned, dims), "no host tables: %r" % (dims,)
                assert not lib.box_fwd_boxes_hl_ok(elem, aligned, dims, shapes, None)
                assert not lib.box_fwd_boxes_hl_ok(elem, aligned, dims, None, lsi)
                seen[want] += 1
                if want:
                    kinds.add((elem, len(shapes)))
                    assert C == 32 and P == 4 and len(shapes) <= 4 and lq_off == 0 and aligned == 16 and not broken
                    assert variant == 0
    finally:
        lib.set_variant(0)
    assert seen[True] >= 20 and seen[False] >= 20, seen          # the grid holds both answers
    assert kinds == {(e, n) for e in (2, 4) for n in (1, 2, 4)}, kinds
    # variant 1 (generic kernels only) and option `dense` off: make_dense_plan honours them, and so does the query
    levels, B, H = GEOMETRIES[-1]
    shapes, lsi, S = host_tables(levels)
    dims = (B, S, H, 32, len(levels), S, 4)
    assert lib.box_fwd_boxes_hl_ok(2, 16, dims, shapes, lsi)
    try:
        lib.set_variant(1)
        assert lib.fwd_route(2, 0, 16, dims, shapes, lsi) != STAGED
        assert not lib.box_fwd_boxes_hl_ok(2, 16, dims, shapes, lsi)
        lib.set_variant(0)
        old = lib.set_option("dense", 1)
        try:
            assert lib.fwd_route(2, 0, 16, dims, shapes, lsi) != STAGED
            assert not lib.box_fwd_boxes_hl_ok(2, 16, dims, shapes, lsi)
        finally:
            lib.set_option("dense", old)
    finally:
        lib.set_variant(0)
    assert lib.box_fwd_boxes_hl_ok(2, 16, dims, shapes, lsi)
    assert not lib.box_fwd_boxes_hl_ok(8, 16, dims, shapes, lsi)       # float64: no such kernel


def call(lib, name, ptrs, dims, tables, ref_dim=4, V=4, angle_mode=0):
    """An entry call with fake (never dereferenced) device pointers; ptrs: value, shapes, lsi, ref, offsets, kernel_idx,
    valid_ratios, logits, out; tables: (shapes_host, lsi_host) numpy arrays or None each (those ARE read)."""
    v, sh, ls, ref, off, kid, vr, lg, out = ptrs
    host = [None if t is None else t.ctypes.data for t in tables]
    return getattr(lib.load(), name)(v, sh, ls, ref, ref_dim, 0, off, V, angle_mode, kid, vr, lg, *dims, out, *host,
                                     None)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_refuse_before_any_device_call(lib, name):
    """hipErrorInvalidValue for dimensions the query refuses, for a reference window or offsets that do not fit the
    angle mode, for NULL required pointers and for NULL host tables; a call without queries returns 0 having done
    nothing.  (An accepted call would launch: there is none here.)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    p -= p % 16
    p += 16
    all_ptrs = [p] * 9
    levels = [(9, 11), (4, 5)]
    shapes, lsi, S = host_tables(levels)
    tables = (shapes, lsi)
    good = (2, S, 8, 32, 2, S, 4)
    elem = 4 if name.endswith("f32") else 2
    assert lib.box_fwd_boxes_hl_ok(elem, 16, good, shapes, lsi)
    refused = [(2, S, 8, 16, 2, S, 4), (2, S, 8, 64, 2, S, 4), (2, S, 8, 32, 2, S, 9), (2, S, 8, 32, 2, S - 1, 4),
               (2, S, 8, 32, 2, 4, 4), (2, S + 1, 8, 32, 2, S + 1, 4), (2, S, 8, 32, 2, S, 0), (2, S, 0, 32, 2, S, 4),
               (-1, S, 8, 32, 2, S, 4), (2, S, 8, 32, 17, S, 4)]
    for dims in refused:
        assert not lib.box_fwd_boxes_hl_ok(elem, 16, dims, shapes, lsi), dims
        assert call(lib, name, all_ptrs, dims, tables) == INVALID_VALUE, dims
    five = host_tables(levels, 5)
    dims5 = (2, five[2], 8, 32, 5, five[2], 4)
    assert not lib.box_fwd_boxes_hl_ok(elem, 16, dims5, five[0], five[1])
    assert call(lib, name, all_ptrs, dims5, five[:2]) == INVALID_VALUE                # L = 5
    short = host_tables(levels[:1] + [(4, 4)])
    assert call(lib, name, all_ptrs, good, short[:2]) == INVALID_VALUE                # sizes that do not sum to S
    off8 = list(all_ptrs)
    off8[0] = p + 8                                                                    # value 8 bytes off
    assert call(lib, name, off8, good, tables) == INVALID_VALUE
    off8 = list(all_ptrs)
    off8[8] = p + 8                                                                    # ... and out
    assert call(lib, name, off8, good, tables) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, tables, ref_dim=3) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, tables, ref_dim=4, angle_mode=2) == INVALID_VALUE     # an angle needs ref_dim 5
    assert call(lib, name, all_ptrs, good, tables, ref_dim=5, V=4, angle_mode=1) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, tables, ref_dim=5, V=5, angle_mode=0) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, tables, ref_dim=5, V=5, angle_mode=3) == INVALID_VALUE
    for missing in (0, 1, 2, 3, 4, 5, 7, 8):                               # every required pointer (6: optional)
        ptrs = list(all_ptrs)
        ptrs[missing] = None
        assert call(lib, name, ptrs, good, tables) == INVALID_VALUE, missing
    for host in ((None, None), (shapes, None), (None, lsi)):                # there is no other kernel behind these entries
        assert call(lib, name, all_ptrs, good, host) == INVALID_VALUE
    lib.set_variant(1)
    try:
        assert not lib.box_fwd_boxes_hl_ok(elem, 16, good, shapes, lsi)
        assert call(lib, name, all_ptrs, good, tables) == INVALID_VALUE     # no generic fallback behind this entry
    finally:
        lib.set_variant(0)
    assert call(lib, name, [None] * 9, (2, S, 8, 32, 2, 0, 4), (None, None)) == 0      # no queries: nothing to do


def test_python_surface():
    import inspect
    from boxer_amd import ops
    from boxer_amd.modules import Box3dAttention, BoxAttention, InstanceAttention
    p = inspect.signature(ops.box_attn_forward_boxes_staged).parameters
    assert list(p) == ["value", "spatial_shapes", "level_start_index", "ref_windows", "offsets", "kernel_indices",
                       "valid_ratios", "logits", "angle_mode"]
    assert p["angle_mode"].default == 0
    assert list(inspect.signature(ops.box_forward_boxes_staged_ok).parameters) == [
        "value", "spatial_shapes", "level_start_index", "num_query", "num_point"]
    # ... and the row-gather call keeps its own
    assert list(inspect.signature(ops.box_attn_forward_boxes).parameters) == list(p)
    assert list(inspect.signature(ops.box_forward_boxes_ok).parameters) == ["value", "num_level", "num_query",
                                                                            "num_point"]
    for m in (BoxAttention(32, 1, 2), Box3dAttention(32, 1, 2), InstanceAttention(32, 1, 2, 4)):
        assert m.fused_boxes_staged is False and m.fused_boxes is False
