"""GPU tests (``-m gpu``) of box attention's training step from boxes and L*P logits: the one-launch box and logit
gradients (``ops.box_attn_backward_boxes``, include/boxattn.h boxattn_bwd_boxes_*), the autograd
Function on top of it (``BoxAttnBoxesFunction``) and the module flag ``fused_boxes_train`` in BoxAttention /
Box3dAttention.  The problems are those of test_gpu_box_boxes_forward.py (boxes_cases.box_boxes_problem).

Every seeded case holds the three outputs of the one call -- grad_offsets, grad_ref_rows, grad_logits, all float32 --
against two expectations with ``|got - want| <= tol * (max(1, rms(want)) + |want|)``, tol 1e-4 (the point gradients
are float32 in every storage mode):
  (a) this build's chain, none of whose kernels is the one under test: ``ops.box_grid_forward`` ->
      ``ops.softmax_forward`` -> ``ops.box_attn_backward(want=2)`` -> ``ops.box_grid_backward`` +
      ``ops.softmax_backward``;
  (b) the float64 C oracle's per-point gradients -- from the float32 locations and weights the GPU made and the
      rounded ``value`` and upstream gradient -- reduced in float64 numpy by the formulas of boxattn_grid.h
      (grid_grad_add / grid_grad_store, all three angle modes) and the plain softmax Jacobian, written out below
      (tests/test_box_boxes_backward_cases.py holds them against float64 autograd without a GPU).
A sample point within 1e-4 px of a bilinear cell edge has an ambiguous grad_loc and cannot be left out of a sum: for
those points only, (b) takes the chain's per-point grad_loc.  Their share is printed and must stay <= 0.2 % of a case's
points (a condition on the inputs, not a tolerance; the CPU file checks it too).

The rule above has an absolute floor of 1e-4 and both expectations rest on this build's kernels; the per-element check
of the same call -- every element of the three outputs within a derived bound of a float64 model that starts from the
boxes and logits, the rotated terms and the must-be-zero rows included -- lives in
tests/test_gpu_boxes_error_bounds.py (test_box_backward_from_boxes; model: tests/error_bounds.py boxes_reference,
CPU twin: tests/test_boxes_error_bounds.py).  The assertions here stay as they are."""

import numpy as np
import pytest
import torch

from oracle import boxattn_oracle as oc
from boxes_cases import (BOX_BWD_CHANNELS as CHANNELS, EDGE_CAP, FLAVOURS, G9_NAMES, GOLDENS, GRAD_NAMES as NAMES,
                         LEAVES, SMALL, _g9_check, box_boxes_problem as problem, box_bwd_case as case,
                         box_golden_module as golden_module, box_reduce_grid as reduce_grid,
                         box_reduce_logits as reduce_logits, box_upstream as upstream, device_args, eligible,
                         function_inputs, golden_loss, module_grads, offset_by_eight, run_boxes_function,
                         run_point_functions)
from compare_rules import POINT_TOL, check_scaled as check, exact_zeros, rounded, tol_of
from point_cases import on_cell_edge
from route_vocab import DTYPES, dev

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the float64 reductions of expectation (b)


# ------------------------------------------------------------------ one case: the call and its two expectations


def boxes_call(a, gout):
    from boxer_amd import ops
    return ops.box_attn_backward_boxes(a["value"], a["shapes"], a["lsi"], a["ref"], a["off"], a["kidx"], a["vr"],
                                       a["logits"], a["mode"], gout, need_ref_grad=True)


def expectations(g, dt, a, gout64, what):
    """-> ((grad_offsets, grad_ref_rows, grad_logits) of the chain, tensors; the same of the oracle, numpy; the float32
    grid the chain made, numpy)."""
    from boxer_amd import ops
    B, S, H, C, L, Lq, P = g["dims"]
    gout = dev(gout64, dt)
    grid = ops.box_grid_forward(a["ref"], a["off"], a["kidx"], a["vr"], a["mode"])
    attn = ops.softmax_forward(a["logits"])
    _, gloc, gattn = ops.box_attn_backward(a["value"], a["shapes"], a["lsi"], grid, attn.view(B, Lq, H, L, P), gout,
                                           64, want=2)
    assert gloc.dtype == gattn.dtype == torch.float32
    goff, rows = ops.box_grid_backward(a["ref"], a["off"], a["kidx"], a["vr"], a["mode"], gloc, need_ref_grad=True)
    glog = ops.softmax_backward(attn, gattn.view(attn.shape), torch.float32)
    torch.cuda.synchronize()
    # (b)
    loc64 = grid.double().cpu().numpy()
    _, ol, oa = oc.box_attn_backward(rounded(g["value"], dt), g["shapes"], g["lsi"], loc64,
                                     attn.double().cpu().numpy().reshape(B, Lq, H, L, P), gout64)
    edge = on_cell_edge(loc64, g["shapes"])
    share = float(edge.mean())
    print("%s: %.4f %% of the points lie on a bilinear cell edge (cap %.1f %%)" % (what, 100 * share, 100 * EDGE_CAP))
    assert share <= EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (what, 100 * share)
    ol = np.where(edge, gloc.double().cpu().numpy(), np.asarray(ol).reshape(loc64.shape))
    want_off, want_rows = reduce_grid(g["ref"], g["off"], a["kidx"].double().cpu().numpy(), g["vr"], a["mode"], ol)
    want_log = reduce_logits(g["logits"], oa)
    return (goff, rows, glog), (want_off, want_rows, want_log), loc64


def hold(got, chain, oracle, what):
    for name, t, c, o in zip(NAMES, got, chain, oracle):
        assert t.dtype == torch.float32 and t.shape == c.shape, name
        check(t, c.double().cpu().numpy(), POINT_TOL, "%s %s against the chain" % (what, name))
        check(t, o, POINT_TOL, "%s %s against the oracle" % (what, name))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("geometry", SMALL)
def test_seeded_matrix(geometry, C, dtype):
    """Angle modes 0, 1 (reference windows of 5 and 7 values) and 2 x reference windows shared and per head x
    valid_ratios None and given."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    if geometry == "k4" and not eligible(geometry, C, dt):
        pytest.skip("k4: no row gather for %s at C = %d (boxattn_bwd_boxes_ok answers 0)" % (dtype, C))
    for (angle_mode, ref_dim), per_head, with_vr in FLAVOURS:
        g = case(geometry, C, angle_mode, ref_dim, per_head, with_vr)
        B, S, H, _, L, Lq, P = g["dims"]
        what = "%s C=%d %s angle=%d D=%d per_head=%d vr=%d" % (geometry, C, dtype, angle_mode, ref_dim, per_head,
                                                                 with_vr)
        a = device_args(g, dt)
        assert ops.box_backward_boxes_ok(a["value"], L, Lq, P), "not eligible: " + what
        gout64 = upstream(g, dt)
        got = boxes_call(a, dev(gout64, dt))
        V = 5 if angle_mode == 1 else 4
        assert got[0].shape == (B, Lq, H, L, V) and got[1].shape == (B, Lq, H, L, 5) and \
            got[2].shape == (B, Lq, H, L * P)
        chain, oracle, loc64 = expectations(g, dt, a, gout64, what)
        hold(got, chain, oracle, what)
        exact_zeros(g, got, loc64, what)


@pytest.mark.parametrize("angle_mode", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("geometry", ["mid", "mid_h3"])
def test_mid_size(geometry, dtype, angle_mode):
    """C2 levels, 300 queries, B 2, C 32: 75 and more workgroups, the XCD re-map and the magic divisions."""
    dt = DTYPES[dtype]
    g = problem(geometry, 32, angle_mode, 5 if angle_mode else 4, False, True)
    what = "%s %s angle=%d" % (geometry, dtype, angle_mode)
    a = device_args(g, dt)
    gout64 = upstream(g, dt)
    got = boxes_call(a, dev(gout64, dt))
    chain, oracle, _ = expectations(g, dt, a, gout64, what)
    hold(got, chain, oracle, what)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_two_runs_are_bitwise_equal(dtype):
    dt = DTYPES[dtype]
    g = case("model", 32, 1, 5, False, True)
    a = device_args(g, dt)
    gout = dev(upstream(g, dt), dt)
    first = boxes_call(a, gout)
    again = boxes_call(a, gout)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, first, again):
        assert torch.equal(x, y), "%s: two runs differ (the kernel has no atomics)" % name


def raw_entry(dtype, a, g, gout, outs):
    from boxer_amd import _lib
    B, S, H, C, L, Lq, P = g["dims"]
    entry = getattr(_lib.load(), "boxattn_bwd_boxes_" + dtype)
    ptr = lambda t: None if t is None else t.data_ptr()
    return entry(ptr(a["value"]), ptr(a["shapes"]), ptr(a["lsi"]), ptr(a["ref"]), a["ref"].size(-1),
                 int(a["ref"].dim() == 4), ptr(a["off"]), a["off"].size(-1), a["mode"], ptr(a["kidx"]), ptr(a["vr"]),
                 ptr(a["logits"]), ptr(gout), B, S, H, C, L, Lq, P, *[ptr(t) for t in outs],
                 torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("geometry", ["model", "ragged"])
def test_rows_offset_by_eight_bytes(geometry, dtype):
    """16-bit ``value`` and ``grad_out`` 8 bytes off a 16-byte boundary: the same result (4 channels a lane instead of
    8) or a clean refusal, whichever boxattn_bwd_boxes_ok says -- and the entry says the same."""
    from boxer_amd import _lib
    dt = DTYPES[dtype]
    g = case(geometry, 32, 1, 5, True, True)
    B, S, H, C, L, Lq, P = g["dims"]
    a = device_args(g, dt)
    gout64 = upstream(g, dt)
    what = "offset rows %s %s" % (geometry, dtype)
    chain, oracle, _ = expectations(g, dt, a, gout64, what)
    a["value"] = offset_by_eight(a["value"])
    gout = offset_by_eight(dev(gout64, dt))
    ok = _lib.box_bwd_boxes_ok(2, 8, g["dims"])
    outs = [torch.empty((B, Lq, H, L, n), dtype=torch.float32, device="cuda") for n in (5, 5, P)]
    rc = raw_entry(dtype, a, g, gout, outs)
    torch.cuda.synchronize()
    assert (rc == 0) == ok, "the entry answered %d, the query %d" % (rc, ok)
    if not ok:
        assert rc == 1
        with pytest.raises(ValueError):
            boxes_call(a, gout)
        return
    got = boxes_call(a, gout)
    torch.cuda.synchronize()
    for x, y in zip(got, outs):
        assert torch.equal(x.reshape(-1), y.reshape(-1)), "ops and the entry differ"
    hold(got, chain, oracle, what)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_no_queries_and_no_pixels(dtype):
    """The raw entry: without queries nothing is launched or written; without pixels the three outputs are zeros."""
    dt = DTYPES[dtype]
    g = case("model", 32, 1, 5, False, True)
    B, S, H, C, L, Lq, P = g["dims"]
    a = device_args(g, dt)
    gout = dev(upstream(g, dt), dt)
    outs = [torch.full((B, Lq, H, L, n), 7.0, dtype=torch.float32, device="cuda") for n in (5, 5, P)]
    empty = dict(g, dims=(B, S, H, C, L, 0, P))
    assert raw_entry(dtype, dict(a, value=None, ref=a["ref"][:, :0], off=a["off"][:, :0]), empty, None, outs) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs), "a call without queries wrote"
    nopix = dict(g, dims=(B, 0, H, C, L, Lq, P))
    assert raw_entry(dtype, dict(a, value=None), nopix, gout, outs) == 0
    torch.cuda.synchronize()
    assert all(not t.any() for t in outs), "no pixels: the outputs are zeros"


# ------------------------------------------------------------------ the autograd Function


@pytest.mark.parametrize("per_head", [False, True], ids=["shared_windows", "windows_per_head"])
@pytest.mark.parametrize("angle_mode", [0, 1])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_function_equals_the_per_point_functions(dtype, angle_mode, per_head):
    dt = DTYPES[dtype]
    g = case("model", 32, angle_mode, 5 if angle_mode else 4, per_head, True)
    gout = dev(upstream(g, dt)).float()
    res = {}
    for name, run in (("boxes", run_boxes_function), ("points", run_point_functions)):
        x = function_inputs(g)
        out = run(x, dt)
        (out.float() * gout).sum().backward()
        res[name] = (out, [x[n].grad for n in LEAVES])
    torch.cuda.synchronize()
    (o_b, g_b), (o_p, g_p) = res["boxes"], res["points"]
    what = "%s angle=%d per_head=%d" % (dtype, angle_mode, per_head)
    assert o_b.dtype == dt and o_b.shape == o_p.shape
    check(o_b, o_p.detach().double().cpu().numpy(), tol_of(dt), "out " + what)
    for name, a, b in zip(LEAVES, g_b, g_p):
        assert a is not None and a.dtype == torch.float32 and a.shape == b.shape, name
        check(a, b.double().cpu().numpy(), tol_of(dt) if name == "value" else POINT_TOL,
              "grad of %s %s" % (name, what))


class Counters:
    """Counts the calls of the two ops functions the Function's backward chooses between."""

    def __enter__(self):
        from boxer_amd import ops
        self.ops, self.n = ops, {"boxes": 0, "value": 0}
        self.orig = (ops.box_attn_backward_boxes, ops.box_attn_backward)

        def spy(key, fn):
            def inner(*a, **k):
                self.n[key] += 1
                return fn(*a, **k)
            return inner
        ops.box_attn_backward_boxes = spy("boxes", self.orig[0])
        ops.box_attn_backward = spy("value", self.orig[1])
        return self

    def __exit__(self, *exc):
        self.ops.box_attn_backward_boxes, self.ops.box_attn_backward = self.orig


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_function_computes_only_what_is_asked_for(dtype):
    """Only ``value`` / only ``logits`` requiring a gradient: the others stay None and the call that is not needed is
    not made."""
    dt = DTYPES[dtype]
    g = case("model", 32, 1, 5, False, True)
    gout = dev(upstream(g, dt)).float()
    ref = function_inputs(g)
    (run_point_functions(ref, dt).float() * gout).sum().backward()
    want = {n: ref[n].grad for n in LEAVES}
    for only, calls in (("value", {"boxes": 0, "value": 1}), ("logits", {"boxes": 1, "value": 0}),
                        (None, {"boxes": 1, "value": 1})):
        x = function_inputs(g)
        for n in LEAVES:
            x[n].requires_grad_(only is None or n == only)
        with Counters() as c:
            (run_boxes_function(x, dt).float() * gout).sum().backward()
        torch.cuda.synchronize()
        assert c.n == calls, (only, c.n)
        for n in LEAVES:
            if only is not None and n != only:
                assert x[n].grad is None, n
                continue
            check(x[n].grad, want[n].double().cpu().numpy(), tol_of(dt) if n == "value" else POINT_TOL,
                  "only=%s: grad of %s %s" % (only, n, dtype))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_function_saves_no_per_point_tensor(dtype):
    dt = DTYPES[dtype]
    g = case("k4", 32, 1, 5, True, True)
    B, S, H, C, L, Lq, P = g["dims"]
    if not eligible("k4", 32, dt):
        g = case("odd_k", 32, 1, 5, True, True)
        B, S, H, C, L, Lq, P = g["dims"]
    x = function_inputs(g)
    out = run_boxes_function(x, dt)
    saved = [t for t in out.grad_fn.saved_tensors if t is not None]
    value_bytes = B * S * H * C * (4 if dt == torch.float32 else 2)
    total = sum(t.numel() * t.element_size() for t in saved)
    print("saved for the backward: %d bytes in %d tensors (value: %d)" % (total, len(saved), value_bytes))
    assert total < value_bytes + 64 * B * Lq * H * L * 4
    for t in saved:
        assert t.dim() < 5 or t.shape[-1] != P, tuple(t.shape)       # (no (.., L, P[, 2]) tensor)
        assert t.dim() != 6, tuple(t.shape)


# ------------------------------------------------------------------ the modules
G7_NAMES = sorted(n for n in GOLDENS if n.startswith("G7"))


@pytest.mark.parametrize("native_bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", G9_NAMES)
def test_module_reference_golden(name, native_bf16):
    """The G9 goldens with grad enabled: with ``fused_boxes_train`` the output and the gradients of query, value,
    reference windows and every parameter meet the reference's at the tolerances test_g9_modules_fast_paths holds
    these fixtures to, through exactly one ``ops.box_attn_backward_boxes`` call, and the second return is (); with the
    flag off nothing changes: no call, the weights tensor as second return."""
    m, g, args = golden_module(name, native_bf16)
    assert m.fused_boxes_train is False
    tol = 4e-2 if native_bf16 else 2e-4
    rms_only = ("ref_windows", "linear_box", "query") if native_bf16 else ()
    for flag in (True, False):
        m.fused_boxes_train = flag
        with Counters() as c:
            outs, grads = module_grads(m, args, golden_loss(g), torch.bfloat16 if native_bf16 else None)
        torch.cuda.synchronize()
        assert c.n["boxes"] == (1 if flag else 0), "flag %s: %s" % (flag, c.n)
        if flag:
            assert outs[1] == ()
        else:
            assert isinstance(outs[1], torch.Tensor) and outs[1].shape[-2:] == (2, 2)
        _g9_check(name, outs[:1], grads, g, tol, "fused_boxes_train=%s bf16=%s" % (flag, native_bf16),
                  rms_only=rms_only)


@pytest.mark.parametrize("name", G7_NAMES)
def test_module_without_a_kernel_falls_through(name):
    """8 channels a head: the library has generic kernels only, the flag runs today's code without a call."""
    m, g, args = golden_module(name)
    res = {}
    for flag in (True, False):
        m.fused_boxes_train = flag
        with Counters() as c:
            res[flag] = module_grads(m, args, lambda outs: outs[0].square().sum())
        assert c.n["boxes"] == 0, name
    torch.cuda.synchronize()
    (o_on, g_on), (o_off, g_off) = res[True], res[False]
    assert isinstance(o_on[1], torch.Tensor)
    check(o_on[0], o_off[0].detach().double().cpu().numpy(), 1e-4, "%s out" % name)
    for k in g_on:                                   # (the generic backward sums with atomics: not bitwise)
        check(g_on[k], g_off[k].double().cpu().numpy(), 1e-4, "%s gradient of %s" % (name, k))


@pytest.mark.parametrize("what", ["float64", "valid_ratios_shape", "no_grad"])
def test_module_falls_back_to_the_per_point_path(what):
    """Flag on where the path from boxes does not run: today's code, with the weights as second return."""
    m, g, args = golden_module("G9_module_box_dec")
    B, Lq = args[0].shape[:2]
    args = list(args)
    if what == "float64":
        m = m.double()
        args = [a.double() if a is not None and a.is_floating_point() else a for a in args]
    if what == "valid_ratios_shape":
        torch.manual_seed(11)
        args[5] = (0.5 + 0.5 * torch.rand(B, 1, 1, 4, 1, 2, device="cuda")).expand(B, Lq, 1, 4, 1, 2).contiguous()
    m.fused_boxes_train = True
    with Counters() as c:
        if what == "no_grad":
            with torch.no_grad():
                out, weights = m(*args)
        else:
            (out, weights), grads = module_grads(m, args, lambda outs: outs[0].square().sum())
            assert all(v is not None for v in grads.values())
    torch.cuda.synchronize()
    assert c.n["boxes"] == 0, what
    assert isinstance(weights, torch.Tensor) and weights.shape[-2:] == (2, 2)
