"""GPU tests (``-m gpu``) of instance attention's training step from boxes and 2x2 logits: the one-launch box and logit
gradients (``ops.instance_attn_backward_boxes``, include/boxattn.h instattn_bwd_boxes_*), the autograd
Function on top of it (``InstanceAttnBoxesFunction``) and the module flag ``fused_boxes_train`` that takes it.

Every seeded case holds the three outputs of the one call -- grad_offsets, grad_ref_rows, grad_logits, all float32 --
against two expectations with ``|got - want| <= tol * (max(1, rms(want)) + |want|)``, tol 1e-4 (the point gradients
are float32 in every storage mode):
  (a) this build's chain, none of whose kernels is the one under test: ``ops.box_grid_forward`` ->
      ``ops.instance_weights_forward`` -> ``ops.instance_attn_backward(want=2)`` (``ops.box_attn_backward(want=2)`` on
      the spatial weights where the mask output took no part) -> ``ops.box_grid_backward`` +
      ``ops.instance_weights_backward``;
  (b) the float64 C oracle's per-point gradients -- from the float32 locations and weights the GPU made and the
      rounded ``value`` and upstream gradients -- reduced in float64 numpy by the formulas of boxattn_grid.h
      (grid_grad_add / grid_grad_store) and boxattn_pointwise.h (grad_z), written out below.
A sample point within 1e-4 px of a bilinear cell edge has an ambiguous grad_loc and cannot be left out of a sum: for
those points only, (b) takes the chain's per-point grad_loc.  Their share is printed and must stay <= 0.2 % of a case's
points (a condition on the inputs, not a tolerance; tests/test_boxes_backward_cases.py checks it without a GPU)."""

import numpy as np
import pytest
import torch

from oracle import boxattn_oracle as oc
from boxes_cases import (EDGE_CAP, GRAD_NAMES as NAMES, INST_BOXES_FLAVOURS as FLAVOURS, INST_GEOMETRY as GEOMETRY,
                         KERNEL_SIZES, LEAVES, _g9_check, inst_bwd_case as case, inst_golden_module as golden_module,
                         inst_kernel_indices as kernel_indices, inst_reduce_grid as reduce_grid,
                         inst_reduce_logits as reduce_logits, module_grads, module_problem, offset_by_eight)
from compare_rules import POINT_TOL, check_scaled as check, rounded, tol_of
from point_cases import on_cell_edge
from route_vocab import DTYPES, dev

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the float64 reductions of expectation (b)


# ------------------------------------------------------------------ one case: the call and its two expectations


def upstream(g, k, dt, seed=0):
    B, S, H, C, L, Lq = g["dims"]
    rng = np.random.default_rng(100 + seed)
    return (rounded(rng.standard_normal((B, Lq, H * C)), dt), rounded(rng.standard_normal((B, Lq, k * k, H * C)), dt))


def device_args(g, k, dt):
    return dict(value=dev(g["value"], dt), shapes=dev(g["shapes"]), lsi=dev(g["lsi"]), ref=dev(g["ref"]),
                off=dev(g["off"]), kidx=kernel_indices(k), vr=None if g["vr"] is None else dev(g["vr"]),
                logits=dev(g["logits"]))


def boxes_call(a, k, gout, gmask):
    from boxer_amd import ops
    return ops.instance_attn_backward_boxes(a["value"], a["shapes"], a["lsi"], a["ref"], a["off"], a["kidx"], a["vr"],
                                            a["logits"], k, gout, gmask, need_ref_grad=True)


def expectations(g, k, dt, a, gout64, gmask64, what):
    """-> ((grad_offsets, grad_ref_rows, grad_logits) of the chain, tensors; the same of the oracle, numpy)."""
    from boxer_amd import ops
    B, S, H, C, L, Lq = g["dims"]
    P = k * k
    gout = dev(gout64, dt)
    gmask = None if gmask64 is None else dev(gmask64, dt)
    grid = ops.box_grid_forward(a["ref"], a["off"], a["kidx"], a["vr"], 0)
    sw, lw = ops.instance_weights_forward(a["logits"], k, need_level=gmask is not None)
    if gmask is not None:
        _, gloc, gsw, glw = ops.instance_attn_backward(a["value"], a["shapes"], a["lsi"], grid, sw, lw, gout, gmask,
                                                       64, want=2)
        glw = glw.view(B, Lq, H, L, k, k)
    else:
        _, gloc, gsw = ops.box_attn_backward(a["value"], a["shapes"], a["lsi"], grid, sw.view(B, Lq, H, L, P), gout,
                                             64, want=2)
        glw = None
    assert gloc.dtype == gsw.dtype == torch.float32
    goff, rows = ops.box_grid_backward(a["ref"], a["off"], a["kidx"], a["vr"], 0, gloc, need_ref_grad=True)
    glog = ops.instance_weights_backward(a["logits"], gsw.view(B, Lq, H, L, k, k), glw)
    torch.cuda.synchronize()
    # (b)
    v64 = rounded(g["value"], dt)
    loc64 = grid.double().cpu().numpy()
    sw64 = sw.double().cpu().numpy().reshape(B, Lq, H, L, P)
    if gmask is not None:
        _, ol, os_, ot = oc.instance_attn_backward(v64, g["shapes"], g["lsi"], loc64, sw64,
                                                   lw.double().cpu().numpy().reshape(B, Lq, H, L, P), gout64, gmask64)
        ot = np.asarray(ot).reshape(B, Lq, H, L, P)
    else:
        _, ol, os_ = oc.box_attn_backward(v64, g["shapes"], g["lsi"], loc64, sw64, gout64)
        ot = None
    edge = on_cell_edge(loc64, g["shapes"])
    share = float(edge.mean())
    print("%s: %.4f %% of the points lie on a bilinear cell edge (cap %.1f %%)" % (what, 100 * share, 100 * EDGE_CAP))
    assert share <= EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (what, 100 * share)
    ol = np.where(edge, gloc.double().cpu().numpy(), np.asarray(ol).reshape(loc64.shape))
    kidx64 = a["kidx"].double().cpu().numpy()
    want_off, want_rows = reduce_grid(g["ref"], g["off"], kidx64, g["vr"], ol)
    want_log = reduce_logits(g["logits"], k, np.asarray(os_).reshape(B, Lq, H, L, P), ot)
    return (goff, rows, glog), (want_off, want_rows, want_log)


def hold(got, chain, oracle, what):
    for name, t, c, o in zip(NAMES, got, chain, oracle):
        assert t.dtype == torch.float32 and t.shape == c.shape, name
        check(t, c.double().cpu().numpy(), POINT_TOL, "%s %s against the chain" % (what, name))
        check(t, o, POINT_TOL, "%s %s against the oracle" % (what, name))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("k", KERNEL_SIZES)
@pytest.mark.parametrize("C", [16, 32, 64])
@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
def test_seeded_matrix(geometry, C, k, dtype):
    """Reference windows shared and per head x valid_ratios None and given x grad_mask given and NULL."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    for per_head, with_vr, with_mask in FLAVOURS:
        g = case(geometry, C, k, per_head, with_vr)
        B, S, H, _, L, Lq = g["dims"]
        what = "%s C=%d k=%d %s per_head=%d vr=%d mask=%d" % (geometry, C, k, dtype, per_head, with_vr, with_mask)
        a = device_args(g, k, dt)
        assert ops.backward_boxes_ok(a["value"], L, Lq, k), "not eligible: " + what
        gout64, gmask64 = upstream(g, k, dt)
        gmask64 = gmask64 if with_mask else None
        got = boxes_call(a, k, dev(gout64, dt), None if gmask64 is None else dev(gmask64, dt))
        assert got[0].shape == (B, Lq, H, L, 4) and got[1].shape == (B, Lq, H, L, 5) and \
            got[2].shape == (B, Lq, H, L, 2, 2)
        hold(got, *expectations(g, k, dt, a, gout64, gmask64, what), what)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("k", KERNEL_SIZES)
def test_two_runs_are_bitwise_equal(k, dtype):
    dt = DTYPES[dtype]
    g = case("head_xcd", 32, k, False, True)
    a = device_args(g, k, dt)
    gout64, gmask64 = upstream(g, k, dt)
    gout, gmask = dev(gout64, dt), dev(gmask64, dt)
    first = boxes_call(a, k, gout, gmask)
    again = boxes_call(a, k, gout, gmask)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, first, again):
        assert torch.equal(x, y), "%s: two runs differ (the kernel has no atomics)" % name


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "no_mask"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("k", [4, 14])
def test_rows_offset_by_eight_bytes(k, dtype, with_mask):
    """16-bit ``value``, ``grad_out`` and ``grad_mask`` 8 bytes off a 16-byte boundary: the same result (4 channels a
    lane instead of 8) or a clean refusal, whichever instattn_bwd_boxes_ok says -- and the entry says the same."""
    from boxer_amd import _lib, ops
    dt = DTYPES[dtype]
    g = case("five_levels", 32, k, True, True)
    B, S, H, C, L, Lq = g["dims"]
    a = device_args(g, k, dt)
    gout64, gmask64 = upstream(g, k, dt)
    gmask64 = gmask64 if with_mask else None
    what = "offset rows k=%d %s mask=%d" % (k, dtype, with_mask)
    chain, oracle = expectations(g, k, dt, a, gout64, gmask64, what)
    a["value"] = offset_by_eight(a["value"])
    gout = offset_by_eight(dev(gout64, dt))
    gmask = offset_by_eight(dev(gmask64, dt)) if with_mask else None
    ok = _lib.bwd_boxes_ok(2, 8, g["dims"], k)
    outs = [torch.empty((B, Lq, H, L, n), dtype=torch.float32, device="cuda") for n in (4, 5, 4)]
    entry = getattr(_lib.load(), "instattn_bwd_boxes_" + dtype)
    rc = entry(a["value"].data_ptr(), a["shapes"].data_ptr(), a["lsi"].data_ptr(), a["ref"].data_ptr(), 4, 1,
               a["off"].data_ptr(), a["kidx"].data_ptr(), a["vr"].data_ptr(), a["logits"].data_ptr(), gout.data_ptr(),
               gmask.data_ptr() if with_mask else None, B, S, H, C, L, Lq, k, *[t.data_ptr() for t in outs],
               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (rc == 0) == ok, "the entry answered %d, the query %d" % (rc, ok)
    if not ok:
        assert rc == 1
        with pytest.raises(RuntimeError):
            boxes_call(a, k, gout, gmask)
        return
    got = boxes_call(a, k, gout, gmask)
    torch.cuda.synchronize()
    for x, y in zip(got, outs):
        assert torch.equal(x.reshape(-1), y.reshape(-1)), "ops and the entry differ"
    hold(got, chain, oracle, what)


# ------------------------------------------------------------------ the autograd Function
def function_inputs(g, k):
    leaf = lambda x: dev(x).float().requires_grad_()
    return dict(value=leaf(g["value"]), ref=leaf(g["ref"]), off=leaf(g["off"]), logits=leaf(g["logits"]),
                shapes=dev(g["shapes"]), lsi=dev(g["lsi"]), kidx=kernel_indices(k),
                vr=None if g["vr"] is None else dev(g["vr"]))


def run_boxes_function(x, k, dt):
    from boxer_amd import InstanceAttnBoxesFunction
    value = x["value"] if dt == torch.float32 else x["value"].to(dt)
    vr = None if x["vr"] is None else x["vr"].view(-1, x["off"].size(3), 2)
    return InstanceAttnBoxesFunction.apply(value, x["shapes"], x["lsi"], x["ref"], x["off"], x["kidx"], vr,
                                           x["logits"], k)


def run_point_functions(x, k, dt):
    import boxer_amd as ba
    grid = ba.BoxGridFunction.apply(x["ref"], x["off"], x["kidx"], x["vr"], 0)
    sw, lw = ba.InstanceWeightsFunction.apply(x["logits"], k, True)
    fn = {torch.float32: ba.InstanceAttnFunction, torch.bfloat16: ba.InstanceAttnBF16Function,
          torch.float16: ba.InstanceAttnF16Function}[dt]
    return fn.apply(x["value"], x["shapes"], x["lsi"], grid, sw, lw, k, 64)


def loss_of(outs, gout, gmask):
    loss = (outs[0].float() * gout).sum()
    return loss if gmask is None else loss + (outs[1].float() * gmask.view(outs[1].shape)).sum()


@pytest.mark.parametrize("per_head", [False, True], ids=["shared_windows", "windows_per_head"])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("k", [4, 14])
def test_function_equals_the_per_point_functions(k, dtype, per_head):
    dt = DTYPES[dtype]
    g = case("five_levels", 32, k, per_head, True)
    gout64, gmask64 = upstream(g, k, dt)
    gout, gmask = dev(gout64).float(), dev(gmask64).float()
    res = {}
    for name, run in (("boxes", run_boxes_function), ("points", run_point_functions)):
        x = function_inputs(g, k)
        outs = run(x, k, dt)
        loss_of(outs, gout, gmask).backward()
        res[name] = (outs, [x[n].grad for n in LEAVES])
    torch.cuda.synchronize()
    (o_b, g_b), (o_p, g_p) = res["boxes"], res["points"]
    for i, name in enumerate(("out", "mask_out")):
        assert o_b[i].dtype == dt and o_b[i].shape == o_p[i].shape
        check(o_b[i], o_p[i].detach().double().cpu().numpy(), tol_of(dt), "%s k=%d %s" % (name, k, dtype))
    for name, a, b in zip(LEAVES, g_b, g_p):
        assert a is not None and a.dtype == torch.float32 and a.shape == b.shape, name
        tol = tol_of(dt) if name == "value" else POINT_TOL
        check(a, b.double().cpu().numpy(), tol, "grad of %s k=%d %s" % (name, k, dtype))


class Counters:
    """Counts the calls of the two ops functions the Function's backward chooses between."""

    def __enter__(self):
        from boxer_amd import ops
        self.ops, self.n = ops, {"boxes": 0, "value": 0}
        self.orig = (ops.instance_attn_backward_boxes, ops.instance_attn_backward, ops.box_attn_backward)

        def spy(key, fn):
            def inner(*a, **k):
                self.n[key] += 1
                return fn(*a, **k)
            return inner
        ops.instance_attn_backward_boxes = spy("boxes", self.orig[0])
        ops.instance_attn_backward = spy("value", self.orig[1])
        ops.box_attn_backward = spy("value", self.orig[2])
        return self

    def __exit__(self, *exc):
        (self.ops.instance_attn_backward_boxes, self.ops.instance_attn_backward, self.ops.box_attn_backward) = self.orig


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_function_computes_only_what_is_asked_for(dtype):
    """Only ``value`` / only ``logits`` requiring a gradient: the others stay None and the entry that is not needed is
    not called; a mask output the loss did not use: the gradients of the per-point Functions under that loss."""
    dt = DTYPES[dtype]
    k = 4
    g = case("five_levels", 32, k, False, True)
    gout64, _ = upstream(g, k, dt)
    gout = dev(gout64).float()
    ref = function_inputs(g, k)
    loss_of(run_point_functions(ref, k, dt), gout, None).backward()
    want = {n: ref[n].grad for n in LEAVES}
    for only, calls in (("value", {"boxes": 0, "value": 1}), ("logits", {"boxes": 1, "value": 0}),
                        (None, {"boxes": 1, "value": 1})):
        x = function_inputs(g, k)
        for n in LEAVES:
            x[n].requires_grad_(only is None or n == only)
        with Counters() as c:
            loss_of(run_boxes_function(x, k, dt), gout, None).backward()          # (the mask output is not used)
        torch.cuda.synchronize()
        assert c.n == calls, (only, c.n)
        for n in LEAVES:
            if only is not None and n != only:
                assert x[n].grad is None, n
                continue
            check(x[n].grad, want[n].double().cpu().numpy(), tol_of(dt) if n == "value" else POINT_TOL,
                  "only=%s mask unused: grad of %s %s" % (only, n, dtype))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_function_saves_no_per_point_tensor(dtype):
    dt = DTYPES[dtype]
    k = 14
    g = case("five_levels", 32, k, True, True)
    B, S, H, C, L, Lq = g["dims"]
    x = function_inputs(g, k)
    out, mask = run_boxes_function(x, k, dt)
    saved = [t for t in out.grad_fn.saved_tensors if t is not None]
    value_bytes = B * S * H * C * (4 if dt == torch.float32 else 2)
    total = sum(t.numel() * t.element_size() for t in saved)
    print("saved for the backward: %d bytes in %d tensors (value: %d)" % (total, len(saved), value_bytes))
    assert total < value_bytes + 64 * B * Lq * H * L * 4
    for t in saved:
        assert k * k not in t.shape, tuple(t.shape)


# ------------------------------------------------------------------ the module


@pytest.mark.parametrize("native_bf16", [False, True], ids=["fp32", "bf16"])
def test_module_reference_golden(native_bf16):
    """G9_module_inst_k4 with grad enabled: with ``fused_boxes_train`` the outputs and the gradients of query, value,
    reference windows and every parameter meet the reference's at the tolerances test_g9_modules_fast_paths holds this
    fixture to, the third return is (); with the flag off nothing changes."""
    m, g, args = golden_module(native_bf16)
    m.inferencing = False
    assert m.fused_boxes_train is False
    loss_fn = lambda outs: sum((o.double() * dev(g["gout%d" % i]).double()).sum() for i, o in enumerate(outs[:2]))
    tol = 4e-2 if native_bf16 else 2e-4
    rms_only = ("ref_windows", "linear_box", "query") if native_bf16 else ()
    for flag in (True, False):
        m.fused_boxes_train = flag
        with Counters() as c:
            outs, grads = module_grads(m, args, loss_fn, torch.bfloat16 if native_bf16 else None)
        torch.cuda.synchronize()
        assert c.n["boxes"] == (1 if flag else 0), "flag %s: %s" % (flag, c.n)
        assert outs[2] == () if flag else len(outs[2]) == 2
        _g9_check("G9_module_inst_k4", outs[:2], grads, g, tol, "fused_boxes_train=%s bf16=%s" % (flag, native_bf16),
                  rms_only=rms_only)


MASK_LOSS = lambda outs: outs[0].float().sum() + 0.01 * outs[1].float().square().sum()


@pytest.mark.parametrize("mode", ["f32", "f16_autocast"])
def test_module_at_the_mask_models_point_count(mode):
    """InstanceAttention(256, 4, 8, 14) on the G6_inst_ms14 levels: flag on against flag off, outputs and every
    gradient.  float16: both paths round the same quantities to float16, at different places -- the storage
    tolerance 1e-2."""
    m, args, dims, g6 = module_problem()
    f16 = mode == "f16_autocast"
    m.native_f16, m.inferencing = f16, False
    tol = 1e-2 if f16 else 1e-4
    res = {}
    for flag in (True, False):
        m.fused_boxes_train = flag
        with Counters() as c:
            res[flag] = module_grads(m, args, MASK_LOSS, torch.float16 if f16 else None)
        assert c.n["boxes"] == (1 if flag else 0)
    torch.cuda.synchronize()
    (o_on, g_on), (o_off, g_off) = res[True], res[False]
    assert o_on[2] == () and len(o_off[2]) == 2
    for i in range(2):
        check(o_on[i], o_off[i].detach().double().cpu().numpy(), tol, "%s out%d" % (mode, i))
    for name in g_on:
        assert g_on[name] is not None and g_off[name] is not None, name
        check(g_on[name], g_off[name].double().cpu().numpy(), tol, "%s gradient of %s" % (mode, name))


@pytest.mark.parametrize("case", ["inferencing", "float64", "valid_ratios_shape"])
def test_module_falls_back_to_the_per_point_path(case):
    """Flag on where the path from boxes does not run: today's tuple-returning code, with the flag-off gradients."""
    m, args, dims, g6 = module_problem()
    B, Lq = args[0].shape[:2]
    m.inferencing = case == "inferencing"
    args = list(args)
    if case == "float64":
        m = m.double()
        args = [a.double() if a is not None and a.is_floating_point() else a for a in args]
    if case == "valid_ratios_shape":
        torch.manual_seed(11)
        args[5] = (0.5 + 0.5 * torch.rand(B, 1, 1, 4, 1, 2, device="cuda")).expand(B, Lq, 1, 4, 1, 2).contiguous()
    loss_fn = (lambda outs: outs[0].sum()) if m.inferencing else MASK_LOSS
    res = {}
    for flag in (True, False):
        m.fused_boxes_train = flag
        with Counters() as c:
            res[flag] = module_grads(m, args, loss_fn)
        assert c.n["boxes"] == 0, case
    torch.cuda.synchronize()
    (o_on, g_on), (o_off, g_off) = res[True], res[False]
    assert isinstance(o_on[2], tuple) and len(o_on[2]) == (1 if m.inferencing else 2)
    for name in g_on:
        assert g_on[name] is not None, name
        check(g_on[name], g_off[name].double().cpu().numpy(), 1e-4, "%s: gradient of %s" % (case, name))
