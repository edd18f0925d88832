"""GPU tests (``-m gpu``) of box attention's inference forward from boxes and L*P logits on the WINDOW-STAGED kernels
(``ops.box_attn_forward_boxes_staged``, include/boxattn.h boxattn_fwd_boxes_hl_*) and of the module flag
``fused_boxes_staged`` that takes it in BoxAttention / Box3dAttention.  Every case has one query a pixel, 32 channels
a head and 2 x 2 points a level: the only shapes the entry accepts.

Two families of inputs per geometry, both with the poisoned rows of boxes_cases.box_boxes_problem (windows wholly and
partly outside the map, negative and exactly-zero sizes, angles of several turns):
  local      query i is pixel i, its window the pixel's centre and four pixels of its level, offsets x 0.5: the points
             are served from the staged windows;
  scattered  random windows as in the decoder geometries: the points leave the windows and take the in-kernel global path.
The finest level of "four_levels" (37 x 23) is staged as a 16 x 16 sub-window (make_dense_plan: 8 + 2 * 3.5 + 1 columns),
so its tiles' windows are placed, clamped at the map's edges and missed by the scattered points.

Every (geometry, family, type) holds the one call, over the 16 flavours (angle mode, reference values) x windows shared /
per head x valid ratios None / given,
  * per element within error_bounds.bound of the float64 model from boxes and logits (error_bounds.boxes_reference), with
    the weight split of the kernel: "bf16" / "f16" two-term weights on the matrix cores, "none" for float32;
  * at the project's tolerance (tol_of) against the three launches of this build -- ``ops.box_grid_forward`` ->
    ``ops.softmax_forward`` -> ``ops.box_attn_forward``, window-staged route asserted -- and against
    ``ops.box_attn_forward_boxes``, the row gather from the same operands.
How many elements differ BITWISE from the three launches is printed, not asserted (the locations are the grid kernel's;
the softmax sums in another order)."""
import functools

import pytest
import torch

import error_bounds as eb
from boxes_cases import (FAMILIES, STAGED_C as C, STAGED_P as P, STAGED_SPLIT as SPLIT, encoder_module, flavours_of,
                         hold, kernel_offsets, operands, run_staged_forward as run_staged, staged_problem as problem)
from compare_rules import check_scaled as check, report_bound as report, tol_of
from route_vocab import DTYPES, STAGED, dev

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=16)
def reference(geometry, family, flavour):
    """The float64 model's ``out`` planes, computed once for the three storage types."""
    (angle_mode, ref_dim), per_head, with_vr = flavour
    g = problem(geometry, family, angle_mode, ref_dim, per_head, with_vr)
    return eb.boxes_reference("box", g["value"], g["shapes"], g["lsi"], g["ref"], g["off"], kernel_offsets(2), g["vr"],
                              g["logits"], g["angle_mode"])["out"]


def three_launches(g, args):
    """The three launches of this build on the same operands, the window-staged route asserted -> out."""
    from boxer_amd import ops
    B, S, H, _, L, Lq, _ = g["dims"]
    value, shapes, lsi, ref, off, kidx, vr, logits, mode = args
    grid = ops.box_grid_forward(ref, off, kidx, vr, mode)
    attn = ops.softmax_forward(logits).view(B, Lq, H, L, P)
    taken = ops.forward_route(value, grid, shapes, lsi)
    assert taken == STAGED, "the three launches take route %d, wanted the window-staged one" % taken
    return ops.box_attn_forward(value, shapes, lsi, grid, attn, 64), grid


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("geometry", ["two_levels", "four_levels", "three_levels", "one_level", "tiny_levels"])
def test_seeded_matrix(geometry, family, dtype):
    """Angle modes 0, 1 (reference windows of 5 and 7 values) and 2 x reference windows shared and per head x
    valid_ratios None and given; "four_levels" with the four (angle mode, reference values) pairs, per head / valid
    ratios alternating (flavours_of)."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    worst, served = 0.0, []
    for flavour in flavours_of(geometry):
        (angle_mode, ref_dim), per_head, with_vr = flavour
        g = problem(geometry, family, angle_mode, ref_dim, per_head, with_vr)
        what = "staged from boxes: %s %s %s angle=%d D=%d per_head=%d vr=%d" % (geometry, family, dtype, angle_mode,
                                                                                ref_dim, per_head, with_vr)
        args = operands(g, dt)
        got = run_staged(g, args)
        three, grid = three_launches(g, args)
        assert (1 + args[4][..., 2:4] / 8 <= 0).any() and (grid < 0).any() and (grid > 1).any()   # relu hit, outside both ways
        boxes = ops.box_attn_forward_boxes(*args)
        torch.cuda.synchronize()
        w = eb.hold(got, reference(geometry, family, flavour), dt, SPLIT[dtype], what)
        print("%s: worst err / bound %.3f" % (what, w))
        worst = max(worst, w)
        # (hold: the bitwise count against the three launches, then both legs at tol_of)
        hold(got, three, boxes.double().cpu().numpy(), dt, what + " [second leg: ops.box_attn_forward_boxes]")
        served.append(float(((grid >= 0) & (grid <= 1)).all(-1).float().mean()))
    report("window-staged from boxes: %s %s (split %s)" % (geometry, family, SPLIT[dtype]), dt, "out", worst)
    print("%s %s: share of points inside the map per flavour: %s" % (geometry, family,
                                                                      " ".join("%.2f" % s for s in served)))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_two_runs_are_equal(dtype):
    from boxer_amd import ops
    dt = DTYPES[dtype]
    for family in FAMILIES:
        g = problem("four_levels", family, 1, 5, False, True)
        args = operands(g, dt)
        first = ops.box_attn_forward_boxes_staged(*args)
        again = ops.box_attn_forward_boxes_staged(*args)
        torch.cuda.synchronize()
        assert torch.equal(first, again), "the kernel has no atomics (%s)" % family


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_value_off_a_16_byte_boundary_is_refused(dtype):
    """A ``value`` 8 bytes off a 16-byte boundary: the query answers no and the op raises ValueError before any device
    call (the launch spy sees nothing); the same operands with ``value`` aligned are accepted."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    g = problem("two_levels", "local", 0, 4, False, False)
    B, S, H, _, L, Lq, _ = g["dims"]
    n = 8 // torch.empty(0, dtype=dt).element_size()
    flat = torch.zeros(g["value"].size + n, dtype=dt, device="cuda")
    value = flat[n:].view(g["value"].shape)
    value.copy_(dev(g["value"], dt))
    assert value.data_ptr() % 16 == 8 and value.is_contiguous()
    args = operands(g, dt, value=value)
    assert not ops.box_forward_boxes_staged_ok(value, args[1], args[2], Lq, P)
    launches = []
    orig = ops._grid_call
    ops._grid_call = lambda *a, **k: launches.append(a[0]) or orig(*a, **k)
    try:
        with pytest.raises(ValueError):
            ops.box_attn_forward_boxes_staged(*args)
        assert not launches
        out = ops.box_attn_forward_boxes_staged(*operands(g, dt))
        torch.cuda.synchronize()
        assert launches == ["boxattn_fwd_boxes_hl_" + dtype] and out.shape == (B, Lq, H * C)
    finally:
        ops._grid_call = orig


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_mid_size(dtype):
    """C2 levels, B 2, H 8, angle mode 0, local windows: 5 400 workgroups.  Against the three launches only."""
    dt = DTYPES[dtype]
    g = problem("mid", "local", 0, 4, False, True)
    args = operands(g, dt)
    got = run_staged(g, args)
    three, _ = three_launches(g, args)
    torch.cuda.synchronize()
    bits = torch.int32 if dt == torch.float32 else torch.int16
    differ = int((got.view(bits) != three.view(bits)).sum().item())
    print("mid %s: %d of %d elements differ bitwise from the three launches" % (dtype, differ, got.numel()))
    check(got, three.double().cpu().numpy(), tol_of(dt), "mid %s against the three launches" % dtype)


# ------------------------------------------------------------------ the modules


class StagedCalls:
    """Counts the calls of ops.box_attn_forward_boxes_staged and ops.box_attn_forward_boxes while it is active."""
    def __init__(self, monkeypatch):
        from boxer_amd import ops
        self.staged, self.gather = [], []
        for name, calls in (("box_attn_forward_boxes_staged", self.staged), ("box_attn_forward_boxes", self.gather)):
            orig = getattr(ops, name)
            monkeypatch.setattr(ops, name, lambda *a, _o=orig, _c=calls, **k: _c.append(1) or _o(*a, **k))


@pytest.mark.parametrize("native_bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["box", "box3d_rot"])
def test_module_flag_takes_the_staged_call_on_encoder_input(kind, native_bf16, monkeypatch):
    """Under no_grad, ``fused_boxes`` + ``fused_boxes_staged`` equals ``fused_boxes`` alone at tol_of, through ONE call
    of ops.box_attn_forward_boxes_staged and none of ops.box_attn_forward_boxes; the staged flag alone does nothing."""
    m, args = encoder_module(kind, native_bf16)
    assert m.fused_boxes_staged is False
    calls = StagedCalls(monkeypatch)
    outs = {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=native_bf16):
        for boxes, staged in ((True, True), (True, False), (False, True)):
            m.fused_boxes, m.fused_boxes_staged = boxes, staged
            del calls.staged[:], calls.gather[:]
            outs[boxes, staged] = m(*args)
            assert (len(calls.staged), len(calls.gather)) == ((1, 0) if boxes and staged else (0, 1) if boxes else (0, 0))
    torch.cuda.synchronize()
    assert outs[True, True][1] == () and outs[True, False][1] == ()
    assert isinstance(outs[False, True][1], torch.Tensor)
    tol = tol_of(torch.bfloat16 if native_bf16 else torch.float32)
    check(outs[True, True][0], outs[True, False][0].double().cpu().numpy(), tol, "%s: staged flag on against off" % kind)


def test_module_with_decoder_queries_keeps_the_row_gather(monkeypatch):
    """Fewer queries than pixels: the staged function is not called, ``fused_boxes`` runs as without the flag."""
    m, args = encoder_module("box", False)
    query = torch.randn(2, 5, 64, device="cuda")
    ref = torch.rand(2, 5, 4, device="cuda") * 0.5 + 0.25
    args = (query,) + args[1:6] + (ref,)
    calls = StagedCalls(monkeypatch)
    m.fused_boxes = m.fused_boxes_staged = True
    with torch.no_grad():
        on = m(*args)[0]
        m.fused_boxes_staged = False
        off = m(*args)[0]
    torch.cuda.synchronize()
    assert (len(calls.staged), len(calls.gather)) == (0, 2)
    assert torch.equal(on, off)


def test_module_with_grad_ignores_the_flag(monkeypatch):
    """Grad enabled: neither one-launch function is called, the output and the weights are bitwise those of the module
    without the flag, and every parameter gradient agrees at tol_of (the encoder backward sums grad_value in an order
    that changes from run to run, so two backward passes of the SAME module are not bitwise equal either)."""
    m, args = encoder_module("box", False)
    calls = StagedCalls(monkeypatch)
    results = {}
    for flag in (True, False):
        m.fused_boxes, m.fused_boxes_staged = True, flag
        m.zero_grad()
        out, weights = m(*args)
        out.square().sum().backward()
        assert isinstance(weights, torch.Tensor)
        results[flag] = [out.detach().clone(), weights.detach().clone()] + [p.grad.clone() for p in m.parameters()]
    torch.cuda.synchronize()
    assert not calls.staged and not calls.gather, "grad mode took a one-launch path"
    names = ["out", "weights"] + [k for k, _ in m.named_parameters()]
    for what, a, b in zip(names, results[True], results[False]):
        if what in ("out", "weights"):
            assert torch.equal(a, b), "%s differs between flag on and flag off" % what
        else:
            check(a, b.double().cpu().numpy(), tol_of(torch.float32), "grad of %s, flag on against off" % what)
