"""CPU: the window-staged backward from boxes and L*P logits at the C ABI -- boxattn_bwd_boxes_hl_{f32, bf16, f16} and
the eligibility query boxattn_bwd_boxes_hl_ok are declared in include/boxattn.h, exported and bound with the header's
parameter counts, the query equals boxattn_fwd_boxes_hl_ok over the dimension table capi_cases.STAGED_GEOMETRIES, and
the entry points refuse, with hipErrorInvalidValue before any device call, NULL host tables, Lq != S, C = 64, P = 9,
L = 5, an unaligned grad_out, a NULL among the required pointers and V / ref_dim that do not fit the angle mode.  No
compute calls: there is no GPU here."""
import ctypes
import inspect
import itertools
import re

import pytest

from capi_cases import HEADER, INVALID_VALUE, STAGED_GEOMETRIES as GEOMETRIES, declarations, host_tables

ENTRY_POINTS = ["boxattn_bwd_boxes_hl_" + suf for suf in ("f32", "bf16", "f16")]
QUERY = "boxattn_bwd_boxes_hl_ok"


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
        fn = getattr(lib.load(), name)
        assert len(fn.argtypes) == decl[name].count(",") + 1 and fn.restype is ctypes.c_int, name
    assert decl[QUERY] == decl["boxattn_fwd_boxes_hl_ok"]
    assert len(getattr(lib.load(), QUERY).argtypes) == 11
    for name in ENTRY_POINTS:
        # the parameters of boxattn_bwd_boxes_* plus the two host tables before stream
        assert decl[name].endswith("float *grad_logits, const int64_t *shapes_host, const int64_t *lsi_host, void *stream")
        assert decl[name].replace(" const int64_t *shapes_host, const int64_t *lsi_host,", "") == \
            decl[name.replace("_hl_", "_")]
        assert len(getattr(lib.load(), name).argtypes) == 26
    assert re.search(r"#define BOXATTN_ABI_VERSION 8\b", open(HEADER).read())        # additions only
    assert lib.load().boxattn_abi_version() == 8 and lib.ABI_VERSION == 8


def test_query_equals_the_forward_query(lib):
    seen = {True: 0, False: 0}
    try:
        for variant in (0, 1):
            lib.set_variant(variant)
            for (levels, B, H), C, P, L, lq_off, elem, aligned, broken in itertools.product(
                    GEOMETRIES, (16, 32, 64), (4, 9), (None, 5), (0, 1), (2, 4), (16, 8, 0), (False, True)):
                shapes, lsi, S = host_tables(levels, L, broken)
                dims = (B, S, H, C, len(shapes), S + lq_off, P)
                want = lib.box_fwd_boxes_hl_ok(elem, aligned, dims, shapes, lsi)
                assert lib.box_bwd_boxes_hl_ok(elem, aligned, dims, shapes, lsi) == want, (dims, elem, aligned, broken)
                assert not lib.box_bwd_boxes_hl_ok(elem, aligned, dims), "no host tables: %r" % (dims,)
                assert not lib.box_bwd_boxes_hl_ok(elem, aligned, dims, shapes, None)
                assert not lib.box_bwd_boxes_hl_ok(elem, aligned, dims, None, lsi)
                seen[want] += 1
    finally:
        lib.set_variant(0)
    assert seen[True] >= 20 and seen[False] >= 20, seen          # the grid holds both answers
    levels, B, H = GEOMETRIES[-1]
    shapes, lsi, S = host_tables(levels)
    assert not lib.box_bwd_boxes_hl_ok(8, 16, (B, S, H, 32, len(levels), S, 4), shapes, lsi)     # float64: no such kernel


def call(lib, name, ptrs, dims, tables, ref_dim=4, V=4, angle_mode=0):
    """An entry call with fake (never dereferenced) device pointers; ptrs: value, shapes, lsi, ref, offsets, kernel_idx,
    valid_ratios, logits, grad_out, grad_offsets, grad_ref_rows, grad_logits; tables: (shapes_host, lsi_host) numpy
    arrays or None each (those ARE read)."""
    v, sh, ls, ref, off, kid, vr, lg, gout, goff, grow, glog = ptrs
    host = [None if t is None else t.ctypes.data for t in tables]
    return getattr(lib.load(), name)(v, sh, ls, ref, ref_dim, 0, off, V, angle_mode, kid, vr, lg, gout, *dims, goff, grow,
                                     glog, *host, None)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_refuse_before_any_device_call(lib, name):
    """(An accepted call would launch: there is none here.)  A call without queries returns 0 having done nothing."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    p -= p % 16
    p += 16
    all_ptrs = [p] * 12
    levels = [(9, 11), (4, 5)]
    shapes, lsi, S = host_tables(levels)
    tables = (shapes, lsi)
    good = (2, S, 8, 32, 2, S, 4)
    elem = 4 if name.endswith("f32") else 2
    assert lib.box_bwd_boxes_hl_ok(elem, 16, good, shapes, lsi)
    for host in ((None, None), (shapes, None), (None, lsi)):                # NULL host tables
        assert call(lib, name, all_ptrs, good, host) == INVALID_VALUE
    refused = [(2, S, 8, 32, 2, S - 1, 4), (2, S, 8, 32, 2, 4, 4),         # Lq != S
               (2, S, 8, 64, 2, S, 4), (2, S, 8, 16, 2, S, 4),             # C = 64 (and 16)
               (2, S, 8, 32, 2, S, 9),                                      # P = 9
               (2, S + 1, 8, 32, 2, S + 1, 4), (2, S, 8, 32, 2, S, 0), (2, S, 0, 32, 2, S, 4), (-1, S, 8, 32, 2, S, 4),
               (2, S, 8, 32, 17, S, 4)]
    for dims in refused:
        assert not lib.box_bwd_boxes_hl_ok(elem, 16, dims, shapes, lsi), dims
        assert call(lib, name, all_ptrs, dims, tables) == INVALID_VALUE, dims
    five = host_tables(levels, 5)
    dims5 = (2, five[2], 8, 32, 5, five[2], 4)
    assert not lib.box_bwd_boxes_hl_ok(elem, 16, dims5, five[0], five[1])
    assert call(lib, name, all_ptrs, dims5, five[:2]) == INVALID_VALUE                # L = 5
    short = host_tables(levels[:1] + [(4, 4)])
    assert call(lib, name, all_ptrs, good, short[:2]) == INVALID_VALUE                # sizes that do not sum to S
    for at in (0, 8):                                                                  # value / grad_out 8 bytes off
        off8 = list(all_ptrs)
        off8[at] = p + 8
        assert not lib.box_bwd_boxes_hl_ok(elem, 8, good, shapes, lsi)
        assert call(lib, name, off8, good, tables) == INVALID_VALUE, at
    off8 = list(all_ptrs)
    off8[11] = p + 8                                                                   # grad_logits: 16-byte stores
    assert call(lib, name, off8, good, tables) == INVALID_VALUE
    for missing in (0, 1, 2, 3, 4, 5, 7, 8, 9, 11):          # every required pointer (6, 10: optional)
        ptrs = list(all_ptrs)
        ptrs[missing] = None
        assert call(lib, name, ptrs, good, tables) == INVALID_VALUE, missing
    assert call(lib, name, all_ptrs, good, tables, ref_dim=3) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, tables, ref_dim=4, angle_mode=2) == INVALID_VALUE     # an angle needs ref_dim 5
    assert call(lib, name, all_ptrs, good, tables, ref_dim=4, V=5, angle_mode=1) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, tables, ref_dim=5, V=4, angle_mode=1) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, tables, ref_dim=5, V=5, angle_mode=0) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, tables, ref_dim=5, V=5, angle_mode=3) == INVALID_VALUE
    lib.set_variant(1)
    try:
        assert not lib.box_bwd_boxes_hl_ok(elem, 16, good, shapes, lsi)
        assert call(lib, name, all_ptrs, good, tables) == INVALID_VALUE     # no generic fallback behind this entry
    finally:
        lib.set_variant(0)
    assert call(lib, name, [None] * 12, (2, S, 8, 32, 2, 0, 4), (None, None)) == 0     # no queries: nothing to do


def test_python_surface():
    import boxer_amd
    from boxer_amd import ops
    from boxer_amd.modules import Box3dAttention, BoxAttention, InstanceAttention
    p = inspect.signature(ops.box_attn_backward_boxes_staged).parameters
    assert list(p) == list(inspect.signature(ops.box_attn_backward_boxes).parameters)
    assert list(p)[-3:] == ["angle_mode", "grad_output", "need_ref_grad"] and p["need_ref_grad"].default is False
    assert list(inspect.signature(ops.box_backward_boxes_staged_ok).parameters)[:5] == [
        "value", "spatial_shapes", "level_start_index", "num_query", "num_point"]
    fn = boxer_amd.BoxAttnBoxesStagedFunction
    assert "BoxAttnBoxesStagedFunction" in boxer_amd.__all__
    assert list(inspect.signature(fn.forward).parameters) == \
        list(inspect.signature(boxer_amd.BoxAttnBoxesFunction.forward).parameters)
    for m in (BoxAttention(32, 1, 2), Box3dAttention(32, 1, 2), InstanceAttention(32, 1, 2, 4)):
        assert m.fused_boxes_train_staged is False and m.fused_boxes_train is False and m.fused_boxes_staged is False
