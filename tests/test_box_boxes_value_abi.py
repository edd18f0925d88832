"""CPU: box attention's training step from boxes with grad_value in the backward's own launch, at the C ABI --
boxattn_bwd_boxes_value_{f32, bf16, f16}, the eligibility query boxattn_bwd_boxes_value_ok and the size query
boxattn_bwd_boxes_value_workspace_bytes are declared in include/boxattn.h, exported and bound; the ABI version is still
8; the eligibility query answers exactly what boxattn_bwd_boxes_ok answers over the sweep of
tests/test_box_boxes_backward_abi.py; the size query answers 0 for 4-byte storage and 4 B S H C for 2-byte storage; the
entry points refuse, with hipErrorInvalidValue before any device call, what their siblings refuse and a bad ``want``, a
missing grad_value and a workspace that is missing, too small or misaligned (16-bit); and the Python surface is part of
the package.  No compute calls: there is no GPU here."""
import ctypes
import itertools
import re

import pytest

from capi_cases import BOX_GEOMETRIES as GEOMETRIES, HEADER, INVALID_VALUE, call_value as call, declarations

SUFFIXES = ("f32", "bf16", "f16")
ENTRY_POINTS = ["boxattn_bwd_boxes_value_" + suf for suf in SUFFIXES]
OK, WS = "boxattn_bwd_boxes_value_ok", "boxattn_bwd_boxes_value_workspace_bytes"


@pytest.fixture(scope="module")
def lib():
    from boxer_amd import _lib
    _lib.build()
    _lib.set_variant(0)
    yield _lib
    _lib.set_variant(0)


def test_header_declares_the_five_names_and_the_bindings_know_them(lib):
    decl = declarations()
    for name in ENTRY_POINTS + [OK, WS]:
        assert name in decl, "missing declaration: " + name
        assert name in lib.EXPORTS, "not bound: " + name
        assert hasattr(ctypes.CDLL(lib.LIB_PATH), name), "missing export: " + name
    assert decl[OK] == "int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P"
    assert decl[WS] == "int elem_bytes, int B, int S, int H, int C"
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    for name in ENTRY_POINTS:
        st = "float" if name.endswith("f32") else "uint16_t"
        assert decl[name] == (
            "const %s *value, const int64_t *shapes, const int64_t *lsi, const float *ref, int ref_dim, "
            "int ref_per_head, const float *offsets, int V, int angle_mode, const float *kernel_idx, "
            "const float *valid_ratios, const float *logits, const %s *grad_out, int B, int S, int H, int C, int L, "
            "int Lq, int P, int want, %s *grad_value, void *workspace, size_t workspace_bytes, float *grad_offsets, "
            "float *grad_ref_rows, float *grad_logits, void *stream" % (st, st, st)), name
        fn = getattr(lib.load(), name)
        assert list(fn.argtypes) == [vp] * 4 + [i, i] + [vp] + [i, i] + [vp] * 4 + [i] * 7 + [i, vp, vp, sz] + [vp] * 4
        assert fn.restype is ctypes.c_int
    ok, ws = getattr(lib.load(), OK), getattr(lib.load(), WS)
    assert list(ok.argtypes) == [i] * 9 and ok.restype is ctypes.c_int
    assert list(ws.argtypes) == [i] * 5 and ws.restype is sz
    assert re.search(r"#define BOXATTN_ABI_VERSION 8\b", open(HEADER).read())        # additions only
    assert lib.load().boxattn_abi_version() == 8 and lib.ABI_VERSION == 8
    text = open(HEADER).read()
    assert re.search(r"#define BOXATTN_WANT_VALUE\s+1\b", text) and re.search(r"#define BOXATTN_WANT_POINTS\s+2\b", text)
    assert (lib.WANT_VALUE, lib.WANT_POINTS, lib.WANT_ALL) == (1, 2, 3)


@pytest.mark.parametrize("variant", [0, 1])
def test_query_answers_what_the_points_query_answers(lib, variant):
    """The sweep of tests/test_box_boxes_backward_abi.py: element sizes 2 / 4 / 8, alignments 16 / 8 / 4 (and 0: none),
    L = 17 and L P = 65 among the dimensions, under the default switches and boxattn_set_variant(1)."""
    lib.set_variant(variant)
    try:
        seen = {True: 0, False: 0}
        for (levels, B, Lq, H), C, P, L, elem, aligned in itertools.product(
                GEOMETRIES, (8, 16, 32, 64), (1, 4, 9, 16, 64, 65), (1, 4, 16, 17), (2, 4, 8), (16, 8, 4, 0)):
            S = sum(h * w for h, w in levels)
            dims = (B, S, H, C, L, Lq, P)
            want = lib.box_bwd_boxes_ok(elem, aligned, dims)
            assert lib.box_bwd_boxes_value_ok(elem, aligned, dims) == want, (dims, elem, aligned)
            seen[want] += 1
        if variant == 0:
            assert seen[True] >= 20 and seen[False] >= 20, seen      # the grid holds both answers
        else:
            assert seen[True] == 0, seen
    finally:
        lib.set_variant(0)


def test_workspace_query(lib):
    for B, S, H, C in [(2, 138, 8, 32), (1, 30, 2, 16), (3, 1, 1, 64), (2, 0, 8, 32), (0, 138, 8, 32),
                       (2, 100000, 8, 64)]:
        dims = (B, S, H, C, 4, 5, 4)
        assert lib.box_bwd_boxes_value_workspace_bytes(4, dims) == 0
        assert lib.box_bwd_boxes_value_workspace_bytes(2, dims) == 4 * B * S * H * C
        assert getattr(lib.load(), WS)(2, B, S, H, C) == 4 * B * S * H * C
    assert getattr(lib.load(), WS)(2, 16, 1 << 20, 8, 64) == 4 * 16 * (1 << 20) * 8 * 64      # beyond 32 bits


@pytest.mark.parametrize("want", [1, 2, 3])
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_refuse_before_any_device_call(lib, name, want):
    """(An accepted call would launch: there is none here.)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    p -= p % 16
    p += 16
    all_ptrs = [p] * 12
    S = 9 * 11 + 4 * 5
    good = (2, S, 8, 32, 2, 4, 4)
    elem = 4 if name.endswith("f32") else 2
    ws_bytes = lib.box_bwd_boxes_value_workspace_bytes(elem, good)
    full = dict(gv=p, ws=p, ws_bytes=ws_bytes)
    assert lib.box_bwd_boxes_value_ok(elem, 16, good)
    refused = [(2, S, 8, 8, 2, 4, 4), (2, S, 8, 32, 1, 4, 65), (2, S, 8, 32, 17, 4, 1), (2, S, 8, 32, 4, 4, 17),
               (2, S, 8, 32, 2, 4, 0), (2, S, 0, 32, 2, 4, 4), (-1, S, 8, 32, 2, 4, 4)]
    for dims in refused:
        assert not lib.box_bwd_boxes_value_ok(elem, 16, dims), dims
        assert call(lib, name, all_ptrs, dims, want, **full) == INVALID_VALUE, dims
    assert call(lib, name, all_ptrs, good, want, ref_dim=3, **full) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, want, ref_dim=4, angle_mode=2, **full) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, want, ref_dim=5, V=4, angle_mode=1, **full) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, want, ref_dim=5, V=5, angle_mode=0, **full) == INVALID_VALUE
    assert call(lib, name, all_ptrs, good, want, ref_dim=5, V=5, angle_mode=3, **full) == INVALID_VALUE
    # every required pointer (6, 10: optional); with VALUE alone the two gradient outputs are not looked at
    required = (0, 1, 2, 3, 4, 5, 7, 8) + ((9, 11) if want & 2 else ())
    for missing in required:
        ptrs = list(all_ptrs)
        ptrs[missing] = None
        assert call(lib, name, ptrs, good, want, **full) == INVALID_VALUE, missing
    for bad in (0, 4, -1, 7):
        assert call(lib, name, all_ptrs, good, bad, **full) == INVALID_VALUE, bad
    if want & 1:
        assert call(lib, name, all_ptrs, good, want, gv=None, ws=p, ws_bytes=ws_bytes) == INVALID_VALUE
        if elem == 2:
            assert call(lib, name, all_ptrs, good, want, gv=p, ws=None, ws_bytes=ws_bytes) == INVALID_VALUE
            assert call(lib, name, all_ptrs, good, want, gv=p, ws=p, ws_bytes=ws_bytes - 1) == INVALID_VALUE
            assert call(lib, name, all_ptrs, good, want, gv=p, ws=p, ws_bytes=0) == INVALID_VALUE
            for off in (4, 8):
                assert call(lib, name, all_ptrs, good, want, gv=p, ws=p + off, ws_bytes=ws_bytes) == INVALID_VALUE, off
    lib.set_variant(1)
    try:
        assert not lib.box_bwd_boxes_value_ok(elem, 16, good)
        assert call(lib, name, all_ptrs, good, want, **full) == INVALID_VALUE   # no generic fallback behind this entry
    finally:
        lib.set_variant(0)
    # neither queries nor pixels: nothing to do
    assert call(lib, name, [None] * 12, (2, 0, 8, 32, 2, 0, 4), want, gv=None, ws=None, ws_bytes=0) == 0


def test_python_surface():
    import inspect
    import boxer_amd
    from boxer_amd import BoxAttnBoxesFunction, BoxAttnBoxesValueFunction, ops
    from boxer_amd.modules import Box3dAttention, BoxAttention, InstanceAttention
    assert "BoxAttnBoxesValueFunction" in boxer_amd.__all__
    assert issubclass(BoxAttnBoxesValueFunction, boxer_amd.functions.Function)
    p = inspect.signature(ops.box_attn_backward_boxes_value).parameters
    assert list(p) == ["value", "spatial_shapes", "level_start_index", "ref_windows", "offsets", "kernel_indices",
                       "valid_ratios", "logits", "angle_mode", "grad_output", "want", "need_ref_grad"]
    assert p["want"].default == 3 and p["need_ref_grad"].default is False
    assert list(inspect.signature(ops.box_backward_boxes_value_ok).parameters) == ["value", "num_level", "num_query",
                                                                                   "num_point"]
    assert list(inspect.signature(BoxAttnBoxesValueFunction.forward).parameters) == \
        list(inspect.signature(BoxAttnBoxesFunction.forward).parameters)
    for m in (BoxAttention(32, 1, 2), Box3dAttention(32, 1, 2), InstanceAttention(32, 1, 2, 2)):
        assert m.fused_boxes_value is False and m.fused_boxes_train is False
