"""GPU tests (``-m gpu``) of instance attention's inference forward from boxes and 2x2 logits in one launch
(``ops.instance_attn_forward_boxes``, include/boxattn.h instattn_fwd_boxes_*) and of the module flag
``fused_boxes`` that takes it.

Every seeded case holds the one call against two expectations, at the project's own tolerances (DESIGN.md 5:
``|got - want| <= tol * (max(1, rms(want)) + |want|)``, tol 1e-4 for float32 and 1e-2 for 16-bit storage -- the harness
of test_gpu_wide_box_forward.py):
  (a) the three launches of this same build -- ``ops.box_grid_forward`` -> ``ops.instance_weights_forward`` ->
      ``ops.instance_attn_forward`` (``ops.box_attn_forward`` for the flavour without mask), route asserted;
  (b) the float64 C oracle fed with the locations and weights those two GPU kernels produced and with ``value``
      rounded to the storage type.
How many elements differ BITWISE from (a) is printed per case (locations and weights come from shared device
functions, so none is expected); it is reported, not asserted."""
import itertools

import pytest
import torch

from oracle import boxattn_oracle as oc
from boxes_cases import (INST_BOXES_FLAVOURS as FLAVOURS, INST_GEOMETRY as GEOMETRY, KERNEL_SIZES, golden_err,
                         inst_boxes_problem as problem, inst_golden_module as golden_module,
                         inst_kernel_indices as kernel_indices, module_problem)
from compare_rules import check_scaled as check, rounded, tol_of
from route_vocab import DTYPES, WIDE, dev, take_family

pytestmark = pytest.mark.gpu


def run_case(g, k, dt, need_mask, value=None):
    """-> (got, three_launch, oracle): lists [out] or [out, mask_out]; got and three_launch tensors, oracle numpy."""
    from boxer_amd import ops
    B, S, H, C, L, Lq = g["dims"]
    P = k * k
    value = dev(g["value"], dt) if value is None else value
    shapes, lsi = dev(g["shapes"]), dev(g["lsi"])
    ref, off, logits, kidx = dev(g["ref"]), dev(g["off"]), dev(g["logits"]), kernel_indices(k)
    vr = None if g["vr"] is None else dev(g["vr"])
    assert ops.forward_boxes_ok(value, L, Lq, k), "not eligible: %s k=%d %s" % (g["dims"], k, dt)
    got = ops.instance_attn_forward_boxes(value, shapes, lsi, ref, off, kidx, vr, logits, k, need_mask)
    # (a) the three launches of this build
    grid = ops.box_grid_forward(ref, off, kidx, vr, 0)
    spatial, level = ops.instance_weights_forward(logits, k, need_level=need_mask)
    assert (1 + off[..., 2:4] / 8 <= 0).any() and (grid < 0).any() and (grid > 1).any()
    if need_mask:
        assert ops.forward_route(value, grid, instance=True) == WIDE
        three = ops.instance_attn_forward(value, shapes, lsi, grid, spatial, level, 64)
    else:
        attn = spatial.view(B, Lq, H, L, P)
        take_family(value, grid, shapes, lsi, WIDE)
        three = [ops.box_attn_forward(value, shapes, lsi, grid, attn, 64)]
        assert got[1] is None
    torch.cuda.synchronize()
    got = [t for t in got if t is not None]
    # (b) the float64 oracle on what the two GPU kernels produced
    v64 = rounded(g["value"], dt)
    loc64 = grid.double().cpu().numpy()
    sw64 = spatial.double().cpu().numpy().reshape(B, Lq, H, L, P)
    if need_mask:
        want = list(oc.instance_attn_forward(v64, g["shapes"], g["lsi"], loc64, sw64,
                                             level.double().cpu().numpy().reshape(B, Lq, H, L, P)))
    else:
        want = [oc.box_attn_forward(v64, g["shapes"], g["lsi"], loc64, sw64)]
    return got, three, want


def hold(got, three, want, dt, what):
    tol = tol_of(dt)
    for name, a, b, w in zip(("out", "mask_out"), got, three, want):
        assert a.dtype == dt and a.shape == b.shape
        differ = int((a.view(torch.int16 if dt != torch.float32 else torch.int32)
                      != b.view(torch.int16 if dt != torch.float32 else torch.int32)).sum().item())
        print("%s %s: %d of %d elements differ bitwise from the three launches" % (what, name, differ, a.numel()))
        check(a, b.double().cpu().numpy(), tol, "%s %s against the three launches" % (what, name))
        check(a, w, tol, "%s %s against the oracle" % (what, name))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("k", KERNEL_SIZES)
@pytest.mark.parametrize("C", [16, 32, 64])
@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
def test_seeded_matrix(geometry, C, k, dtype):
    """Reference windows shared and per head x valid_ratios None and given x mask_out given and NULL."""
    dt = DTYPES[dtype]
    for per_head, with_vr, need_mask in FLAVOURS:
        g = problem(geometry, C, k, per_head, with_vr)
        what = "%s C=%d k=%d %s per_head=%d vr=%d mask=%d" % (geometry, C, k, dtype, per_head, with_vr, need_mask)
        hold(*run_case(g, k, dt, need_mask), dt, what)


@pytest.mark.parametrize("need_mask", [True, False], ids=["mask", "no_mask"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("k", [4, 14])
def test_value_rows_offset_by_eight_bytes(k, dtype, need_mask):
    """A 16-bit `value` 8 bytes off a 16-byte boundary: 4 channels a lane instead of 8, the same family."""
    dt = DTYPES[dtype]
    g = problem("five_levels", 32, k, True, True)
    flat = torch.zeros(g["value"].size + 4, dtype=dt, device="cuda")
    value = flat[4:].view(g["value"].shape)
    value.copy_(dev(g["value"], dt))
    assert value.data_ptr() % 16 == 8 and value.is_contiguous()
    hold(*run_case(g, k, dt, need_mask, value=value), dt, "offset value k=%d %s mask=%d" % (k, dtype, need_mask))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("k", KERNEL_SIZES)
def test_two_runs_are_equal(k, dtype):
    from boxer_amd import ops
    dt = DTYPES[dtype]
    g = problem("head_xcd", 32, k, False, True)
    B, S, H, C, L, Lq = g["dims"]
    args = (dev(g["value"], dt), dev(g["shapes"]), dev(g["lsi"]), dev(g["ref"]), dev(g["off"]), kernel_indices(k),
            dev(g["vr"]), dev(g["logits"]), k)
    first = ops.instance_attn_forward_boxes(*args, True)
    again = ops.instance_attn_forward_boxes(*args, True)
    torch.cuda.synchronize()
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), "the kernel has no atomics"


def test_ops_refuse_what_has_no_kernel():
    from boxer_amd import ops
    g = problem("one_level", 32, 4, False, False)
    args = [dev(g["value"], torch.float32), dev(g["shapes"]), dev(g["lsi"]), dev(g["ref"]), dev(g["off"]),
            kernel_indices(4), None, dev(g["logits"]), 4]
    with pytest.raises(RuntimeError):
        ops.instance_attn_forward_boxes(*args[:7], args[7].double(), 4)          # float32 logits required
    with pytest.raises(RuntimeError):
        ops.instance_attn_forward_boxes(args[0].double(), *args[1:])             # no float64 kernel
    with pytest.raises(RuntimeError):
        ops.instance_attn_forward_boxes(*args[:5], kernel_indices(6), *args[6:])  # kernel_indices of another k


# ------------------------------------------------------------------ the module


@pytest.mark.parametrize("native_bf16", [False, True], ids=["fp32", "bf16"])
def test_module_reference_golden(native_bf16):
    """G9_module_inst_k4 under no_grad: with the flag the outputs agree with the reference's (the tolerances
    test_g9_modules_fast_paths holds outputs to), with the flag-off module, and `inferencing` gives the same `out`."""
    from boxer_amd import ops
    m, g, args = golden_module(native_bf16)
    dt = torch.bfloat16 if native_bf16 else torch.float32
    B, S = g["value"].shape[:2]
    assert ops.forward_boxes_ok(torch.empty(B, S, 8, 32, dtype=dt, device="cuda"), 4, g["query"].shape[1], 4), \
        "G9_module_inst_k4 is not eligible"
    calls = []
    orig = ops.instance_attn_forward_boxes
    ops.instance_attn_forward_boxes = lambda *a, **k: calls.append(1) or orig(*a, **k)
    outs = {}
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=native_bf16):
            for flag, inferencing in itertools.product((True, False), (False, True)):
                m.fused_boxes, m.inferencing = flag, inferencing
                outs[flag, inferencing] = m(*args)
    finally:
        ops.instance_attn_forward_boxes = orig
    torch.cuda.synchronize()
    assert len(calls) == 2, "the flag did not take the one-launch path (or the flag-off module did)"
    tol_g, tol = (4e-2, 1e-2) if native_bf16 else (2e-4, 1e-4)
    on, off = outs[True, False], outs[False, False]
    assert on[2] == () and len(off[2]) == 2
    assert on[1].shape == off[1].shape == (B, g["query"].shape[1], 4, 4, 256)
    for i in range(2):
        e = golden_err(on[i], g["out%d" % i])
        print("G9_module_inst_k4 out%d bf16=%d: %.3e (tol %.0e)" % (i, native_bf16, e, tol_g))
        assert e <= tol_g
        check(on[i], off[i].double().cpu().numpy(), tol, "flag on against flag off, out%d" % i)
    inf_on, inf_off = outs[True, True], outs[False, True]
    assert inf_on[1] is None and inf_on[2] == () and inf_off[1] is None
    check(inf_on[0], inf_off[0].double().cpu().numpy(), tol, "inferencing: flag on against flag off")
    check(inf_on[0], on[0].double().cpu().numpy(), tol, "inferencing against training output, flag on")


@pytest.mark.parametrize("mode", ["f32", "f16_autocast"])
def test_module_at_the_mask_models_point_count(mode):
    """InstanceAttention(256, 4, 8, 14) on the G6_inst_ms14 levels: flag on against flag off, both `inferencing`."""
    from boxer_amd import ops
    m, args, dims, g6 = module_problem()
    f16 = mode == "f16_autocast"
    m.native_f16 = f16
    B, S, H, C, L, Lq, P = dims
    assert ops.forward_boxes_ok(torch.empty(B, S, H, C, dtype=torch.float16 if f16 else torch.float32, device="cuda"),
                                L, Lq, 14)
    tol = 1e-2 if f16 else 1e-4
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=f16):
        for inferencing in (False, True):
            m.inferencing = inferencing
            m.fused_boxes = True
            on = m(*args)
            m.fused_boxes = False
            off = m(*args)
            torch.cuda.synchronize()
            assert on[2] == () and len(off[2]) == (1 if inferencing else 2)
            check(on[0], off[0].double().cpu().numpy(), tol, "%s inferencing=%d out" % (mode, inferencing))
            if inferencing:
                assert on[1] is None and off[1] is None
            else:
                assert on[1].shape == off[1].shape
                check(on[1], off[1].double().cpu().numpy(), tol, "%s mask" % mode)


def test_module_with_grad_runs_todays_code():
    """Flag on, grad enabled, inputs requiring grad: the per-point path -- the usual weight tuple, a backward, and the
    gradients of the flag-off module."""
    m, args, dims, g6 = module_problem()
    assert m.fused_boxes is False                    # the default: nothing changes unless it is set
    m.inferencing = False
    grads = {}
    for flag in (True, False):
        m.fused_boxes = flag
        m.zero_grad()
        query, value, ref = (args[0].clone().requires_grad_(), args[1].clone().requires_grad_(),
                             args[6].clone().requires_grad_())
        out, mask, weights = m(query, value, args[2], None, args[4], None, ref)
        assert isinstance(weights, tuple) and len(weights) == 2 and weights[0].shape[-2:] == (14, 14)
        (out.sum() + 0.01 * mask.square().sum()).backward()
        grads[flag] = [query.grad, value.grad, ref.grad] + [p.grad.clone() for p in m.parameters()]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(grads[True], grads[False])):
        assert a is not None and b is not None
        check(a, b.double().cpu().numpy(), 1e-4, "gradient %d, flag on against flag off" % i)
