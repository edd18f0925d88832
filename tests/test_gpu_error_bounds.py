"""GPU: every forward and backward route held to the per-element error bound of tests/error_bounds.py on
small shapes.  Every case selects its route with the library's option keys and kernel variants, asserts through the
library's own queries that it is the route that runs (ops.forward_route, ops.backward_accumulate_kind,
ops.backward_record_kind, the one-pass counters), runs the forward and the full backward and holds every output.  The
weight-split term of the bound follows the asserted route: SPLIT_OF_ACC for grad_value, the window-staged forward's hi / lo
weight rows for ``out`` of 16-bit storage.

The inputs are generated on the CPU, so tests/test_error_bounds.py checks the same numbers without a GPU (the cell-edge
condition of grad_loc, the route every case expects).  Each case prints ``error-bound | route | type | output | worst
err / bound``; profiles/error_bounds.log is that table from one run."""

import numpy as np
import pytest
import torch

import error_bounds as eb
from point_cases import (DECODER_FORWARD, DECODER_ROUTES, ENCODER_ROUTES, ENCODER_SEEDS, box_tensors, boxes_input,
                         decoder_input, encoder_expectation, encoder_input, inst_tensors, k14_input, run_box,
                         run_instance, seeded6_input, shape_a_input, wide_input)
from route_vocab import (ACC_SPLIT, ACC_TR, ACC_VALU, DTYPES, F32, GATHER, REC_POINT, STAGED, WIDE, routes,
                         set_encoder_keys, split_of, to_device as dev)

pytestmark = pytest.mark.gpu


def report(route, dtype, res):
    for name, worst in res.items():
        print("error-bound | %s | %s | %s | %.3f" % (route, eb.store_name(dtype), name, worst))


# ------------------------------------------------------------------ inputs (CPU; moved to the device by the cases)


reference = eb.reference_of          # the bound's reference of an input dictionary, once per input


# ------------------------------------------------------------------ running


@pytest.fixture(autouse=True)
def _fresh_state():
    from boxer_amd import ops
    ops.release_workspaces()
    yield
    ops.release_workspaces()


# ------------------------------------------------------------------ box attention: the encoder on odd maps


@pytest.mark.parametrize("riders", [0, 1], ids=["riders", "own_launches"])
@pytest.mark.parametrize("dense", [2, 1], ids=["staged", "row_gather"])
@pytest.mark.parametrize("dtype,acc_key,rec_key", ENCODER_ROUTES,
                         ids=["f32_split", "f32_valu", "f32_mfma", "bf16_point", "bf16_group", "f16_point", "f16_group"])
@pytest.mark.parametrize("family", ["model", "test", "border"])
def test_encoder_odd_maps(family, dtype, acc_key, rec_key, dense, riders):
    """(13, 13), (7, 5), one query per pixel: partial blocks on every edge.  Cold, then twice more on new inputs on the
    same state (the one-pass fill where the route has it)."""
    from point_cases import counters
    dt = DTYPES[dtype]
    set_encoder_keys(dense, riders, acc_key, rec_key)
    fwd, acc, rec, one_pass = encoder_expectation(dtype, dense, riders, acc_key, rec_key)
    route = "encoder %s: %s forward, %s accumulate, %s records, riders %s" % (
        family, "staged" if dense == 2 else "row-gather", ("valu", "tr", "f32", "split")[acc], ("point", "group")[rec],
        "on" if riders == 0 else "off")
    worst, seen = {}, []
    for i, seed in enumerate(ENCODER_SEEDS):
        inp = encoder_input(family, dtype, seed)
        t = box_tensors(inp, dt)
        assert routes(t) == (fwd, acc, rec), "%s: the library answers %r" % (route, routes(t))
        got = run_box(t)
        seen.append(counters())
        res = eb.hold_all(got, reference(inp), dt, split_of(acc, dt), "%s, call %d" % (route, i),
                          splits={"out": eb.store_name(dt) if fwd == STAGED and dt != F32 else "none"})
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in res.items()}
    ns = t["value"].size(0) * t["value"].size(2)            # (image, head) slices
    assert seen[0] == (0, 0), "a cold state runs the two-pass passes: %r" % (seen,)
    if one_pass:
        assert seen[1][0] == ns and seen[2][0] == 2 * ns, "the one-pass fill ran from the second call on: %r" % (seen,)
    else:
        assert seen[2][0] == 0, "no one-pass fill on this route: %r" % (seen,)
    report(route, dt, worst)


# ------------------------------------------------------------------ box attention: SEEDED[6], decoder shapes, wave per pair
@pytest.mark.parametrize("variant", [0, 3], ids=["auto", "binned"])
@pytest.mark.parametrize("dtype,C", [("f32", 32), ("bf16", 32), ("f16", 32), ("bf16", 16), ("bf16", 64)],
                         ids=["f32", "bf16", "f16", "bf16_c16", "bf16_c64"])
def test_seeded_6_one_pixel_levels_and_chunked_items(dtype, C, variant):
    """(25, 25), (13, 13), (7, 5), (1, 3), (2, 1), 700 queries: odd blocks, levels one pixel wide / high, up to ~2 500
    terms in a grad_value element."""
    from boxer_amd import _lib
    dt = DTYPES[dtype]
    inp = seeded6_input(C)
    t = box_tensors(inp, dt)
    _lib.set_variant(variant)
    fwd, acc, rec = routes(t)
    assert fwd == GATHER and rec == REC_POINT
    assert acc == (ACC_SPLIT if dt == F32 else ACC_TR), acc
    route = "SEEDED[6] C=%d, variant %d: row-gather forward, %s accumulate" % (C, variant, ("valu", "tr", "f32", "split")[acc])
    report(route, dt, eb.hold_all(run_box(t), reference(inp), dt, split_of(acc, dt), route))


@pytest.mark.parametrize("dtype,variant", DECODER_ROUTES,
                         ids=["%s_%s" % (dt, ("auto", "generic", "atomic", "binned")[v]) for dt, v in DECODER_ROUTES])
@pytest.mark.parametrize("family", ["model", "test"])
def test_decoder_shape_every_variant(family, dtype, variant):
    """Four levels, 50 queries: the generic kernels (float32), the atomic backward, the binned backward."""
    from boxer_amd import _lib
    dt = DTYPES[dtype]
    inp = decoder_input(family, dtype)
    t = box_tensors(inp, dt)
    _lib.set_variant(variant)
    fwd, acc, rec = routes(t)
    assert fwd == DECODER_FORWARD[variant] and rec == REC_POINT, (fwd, rec)
    assert acc == (ACC_SPLIT if dt == F32 else ACC_TR), acc
    # variants 1 and 2 sum grad_value with float32 multiply-adds / atomics; 0 and 3 may take the binned accumulate
    split = "none" if variant in (1, 2) else split_of(acc, dt)
    route = "decoder %s, variant %s: %s forward, grad_value split %s" % (
        family, ("auto", "generic", "atomic", "binned")[variant], _lib.FWD_FAMILIES[fwd], split)
    report(route, dt, eb.hold_all(run_box(t), reference(inp), dt, split, route))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("P", [196, 36])
def test_wave_per_pair_forward(P, dtype):
    from boxer_amd import ops
    from route_vocab import take_family
    dt = DTYPES[dtype]
    inp = wide_input(P)
    t = box_tensors(inp, dt)
    take_family(t["value"], t["loc"], t["shapes"], t["lsi"], WIDE)
    out = ops.box_attn_forward(t["value"], t["shapes"], t["lsi"], t["loc"], t["attn"], 64)
    torch.cuda.synchronize()
    route = "wave-per-pair forward, P = %d" % P
    report(route, dt, eb.hold_all(dict(out=out), reference(inp), dt, what=route))


# ------------------------------------------------------------------ instance attention
@pytest.mark.parametrize("dtype,key", [("bf16", 1), ("bf16", 2), ("f16", 1), ("f16", 2), ("f32", 0)],
                         ids=["bf16_valu", "bf16_tr", "f16_valu", "f16_tr", "f32"])
def test_instance_shape_a(dtype, key):
    """(16, 24), (7, 5), (1, 3), B 2, H 3, 300 queries, 4 x 4 points: the 16-bit accumulate on the VALU (key 23 = 1) and on
    the matrix cores (2), float32 on its default route; the binned backward required, as the neighbouring file does."""
    from boxer_amd import _lib
    dt = DTYPES[dtype]
    inp = shape_a_input("bf16" if dtype == "f32" else dtype)
    t = inst_tensors(inp, dt)
    _lib.set_option("inst_acc16", key)
    _lib.set_variant(3)
    fwd, acc, rec = routes(t, instance=True)
    assert acc == {0: ACC_VALU, 1: ACC_VALU, 2: ACC_TR}[key] and rec == REC_POINT, (acc, rec)
    route = "instance shape A: %s forward, %s accumulate" % (_lib.FWD_FAMILIES[fwd], ("valu", "tr", "f32", "split")[acc])
    report(route, dt, eb.hold_all(run_instance(t), reference(inp), dt, split_of(acc, dt), route))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_instance_14_by_14_points(dtype):
    """k = 14, six queries, four levels: the wave-per-pair instance forward and the backward on its default route."""
    from boxer_amd import _lib
    dt = DTYPES[dtype]
    inp = k14_input(dtype)
    t = inst_tensors(inp, dt)
    fwd, acc, rec = routes(t, instance=True)
    assert fwd == WIDE and rec == REC_POINT, (fwd, rec)
    route = "instance k = 14: wide forward, %s accumulate" % ("valu", "tr", "f32", "split")[acc]
    report(route, dt, eb.hold_all(run_instance(t), reference(inp), dt, split_of(acc, dt), route))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_instance_14_by_14_forward_from_boxes(dtype):
    """ops.instance_attn_forward_boxes (with ops.instance_attn_backward_boxes on the same operands: its reduced box and
    logit gradients keep their own test, here it must run and be finite): out and mask_out held against the reference
    on the float32 grid and weights this build's chain produces (test_gpu_boxes_backward.expectations)."""
    from boxer_amd import ops
    from boxes_cases import inst_kernel_indices as kernel_indices
    dt = DTYPES[dtype]
    g, k = boxes_input(), 14
    B, S, H, C, L, Lq = g["dims"]
    value, shapes, lsi = dev(g["value"], dt), dev(g["shapes"]), dev(g["lsi"])
    ref, off, logits, kidx = dev(g["ref"]), dev(g["off"]), dev(g["logits"]), kernel_indices(k)
    assert ops.forward_boxes_ok(value, L, Lq, k) and ops.backward_boxes_ok(value, L, Lq, k)
    out, mask = ops.instance_attn_forward_boxes(value, shapes, lsi, ref, off, kidx, None, logits, k, True)
    grid = ops.box_grid_forward(ref, off, kidx, None, 0)
    sw, lw = ops.instance_weights_forward(logits, k, need_level=True)
    rng = np.random.default_rng(5)
    gout = dev(rng.standard_normal((B, Lq, H * C)), dt)
    gmask = dev(rng.standard_normal((B, Lq, k * k, H * C)), dt)
    grads = ops.instance_attn_backward_boxes(value, shapes, lsi, ref, off, kidx, None, logits, k, gout, gmask)
    torch.cuda.synchronize()
    assert all(torch.isfinite(x).all() for x in grads if x is not None)
    refs = eb.instance_reference(value, g["shapes"], g["lsi"], grid, sw.view(B, Lq, H, L, k * k),
                                 lw.view(B, Lq, H, L, k * k), gout, gmask)
    route = "instance k = 14: forward from boxes"
    report(route, dt, eb.hold_all(dict(out=out, mask_out=mask), refs, dt, what=route))
