"""GPU: BoxAttention's / Box3dAttention's training step from boxes with grad_value in the backward's own launch
(``ops.box_attn_backward_boxes_value``, include/boxattn.h boxattn_bwd_boxes_value_*), the autograd
Function ``BoxAttnBoxesValueFunction`` and the modules' ``fused_boxes_value`` flag.

grad_value is held per element to ``boxes_cases.value_reference``: the float64 model from boxes and
logits (tests/test_box_boxes_value_cases.py checks that yardstick without a GPU), stored in the storage type, split
"none" -- the kernel adds a w_k g[c] in float32, whatever the storage type.  The order of the atomic adds is not fixed,
so nothing here compares two grad_values bit for bit; the three parameter gradients of the same call are
``torch.equal`` to ``ops.box_attn_backward_boxes``'s, which has no atomics.

The shapes are those of tests/test_gpu_boxes_error_bounds.py (tests/boxes_cases.py): ragged has 42 pairs (dead waves in the last
workgroup; L no power of two), sixteen_levels has more levels than lanes in a group (several passes, lanes without a
level) and every query adding into the same 1 x 1 / 2 x 1 maps, one_level and odd_k the tile edges; the problems hold
windows wholly outside the map and boxes of size <= 0.  Each case prints ``error-bound | route | type | output | worst
err / bound``; profiles/box_boxes_value_error_bounds.log is that table from one run."""
import pytest
import torch

import error_bounds as eb
import boxes_cases
import compare_rules
from boxes_cases import (BOX_GEOMETRIES, CHANNELS, box_args, bwd_problem, bwd_upstream, model_of, offset_by_eight,
                         same_parameter_gradients, value_call, value_reference)
from compare_rules import must_be_zero_share, report_bound as report
from route_vocab import DTYPES, dev

pytestmark = pytest.mark.gpu

FLAVOURS = boxes_cases.FLAVOURS


def flavour_text(geometry, C, flavour):
    return "%s C=%d angle=%d D=%d per_head=%d vr=%d" % ((geometry, C) + flavour[0] + flavour[1:])


def points_call(args, gout):
    from boxer_amd import ops
    res = ops.box_attn_backward_boxes(*args, gout, need_ref_grad=True)
    torch.cuda.synchronize()
    return res


def hold_value(got, ref, dt, value, what):
    assert got.dtype == dt and got.shape == value.shape and got.is_contiguous(), what
    return eb.hold(got, ref, dt, "none", what + ": grad_value")


# (the topmost parametrisation varies fastest: the three types of a (geometry, C) run one after the other on the cached
# references)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("geometry", BOX_GEOMETRIES)
def test_all_gradients_over_every_flavour(dtype, C, geometry):
    """want = 3: grad_value within the bound in the storage type; the three parameter gradients bit for bit those of
    ``ops.box_attn_backward_boxes`` on the same inputs."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    worst, zeros = 0.0, []
    for flavour in FLAVOURS:
        g = bwd_problem(geometry, C, flavour)
        B, S, H, _, L, Lq, P = g["dims"]
        args = box_args(g, dt)
        gout = dev(bwd_upstream(g), dt)
        if geometry == "k4" and not ops.box_backward_boxes_value_ok(args[0], L, Lq, P):
            assert not ops.box_backward_boxes_ok(args[0], L, Lq, P)
            with pytest.raises(ValueError):          # no row gather for this type at this C: an error, not a fall-back
                ops.box_attn_backward_boxes_value(*args, gout)
            pytest.skip("k4: no row gather for %s at C = %d (boxattn_bwd_boxes_value_ok answers 0)" % (dtype, C))
        assert ops.box_backward_boxes_value_ok(args[0], L, Lq, P), "not eligible: %s %s" % (g["dims"], dt)
        what = "box backward with grad_value: " + flavour_text(geometry, C, flavour)
        ref = value_reference(geometry, C, flavour)
        got = value_call(args, gout)
        worst = max(worst, hold_value(got[0], ref, dt, args[0], what))
        zeros.append(must_be_zero_share(ref))
        assert got[1].shape == (B, Lq, H, L, 5 if flavour[0][0] == 1 else 4) and got[2].shape == (B, Lq, H, L, 5)
        same_parameter_gradients(got[1:], points_call(args, gout), what)
    report("box backward with grad_value: %s C=%d [%s storage], must-be-zero share %.2f ... %.2f"
           % (geometry, C, dtype, min(zeros), max(zeros)), dt, "grad_value", worst)


@pytest.mark.parametrize("geometry", ["model", "ragged", "sixteen_levels"])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_want(dtype, geometry):
    """want = 1: grad_value within the same bound and None for the rest; want = 2: ``ops.box_attn_backward_boxes``'s
    results and no grad_value; need_ref_grad off: no reference rows."""
    dt = DTYPES[dtype]
    flavour = ((1, 5), False, True)
    g = bwd_problem(geometry, 32, flavour)
    args = box_args(g, dt)
    gout = dev(bwd_upstream(g), dt)
    what = "want: %s %s" % (geometry, dtype)
    base = points_call(args, gout)
    only_value = value_call(args, gout, want=1)
    assert only_value[1:] == (None, None, None)
    report("box backward, grad_value alone: %s C=32 [%s storage]" % (geometry, dtype), dt, "grad_value",
           hold_value(only_value[0], value_reference(geometry, 32, flavour), dt, args[0], what))
    only_points = value_call(args, gout, want=2)
    assert only_points[0] is None
    same_parameter_gradients(only_points[1:], base, what)
    no_rows = value_call(args, gout, want=3, need_ref_grad=False)
    assert no_rows[2] is None and torch.equal(no_rows[1], base[0]) and torch.equal(no_rows[3], base[2])
    hold_value(no_rows[0], value_reference(geometry, 32, flavour), dt, args[0], what + " without reference rows")


@pytest.mark.parametrize("geometry", ["model", "ragged"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_rows_offset_by_eight_bytes(dtype, geometry):
    """16-bit ``value`` and ``grad_out`` 8 bytes off a 16-byte boundary: 4 channels a lane instead of 8."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    flavour = ((1, 5), True, True)
    g = bwd_problem(geometry, 32, flavour)
    B, S, H, C, L, Lq, P = g["dims"]
    args = box_args(g, dt, value=offset_by_eight(dev(boxes_cases.every_type(g["value"]), dt)))
    gout = offset_by_eight(dev(bwd_upstream(g), dt))
    assert ops.box_backward_boxes_value_ok(args[0], L, Lq, P), "not eligible at this alignment: %s %s" % (g["dims"], dt)
    what = "box backward with grad_value, rows 8 bytes off: %s C=32 [%s storage]" % (geometry, dtype)
    got = value_call(args, gout)
    report(what, dt, "grad_value", hold_value(got[0], value_reference(geometry, 32, flavour), dt, args[0], what))
    same_parameter_gradients(got[1:], points_call(args, gout), what)


MID = "mid"          # (its float64 model takes about two seconds an angle mode on the CPU, shared by the storage types)
_mid_references = {}


def mid_reference(angle_mode):
    if angle_mode not in _mid_references:
        g = boxes_cases.box_boxes_problem(MID, 32, angle_mode, 5 if angle_mode else 4, False, True)
        _mid_references[angle_mode] = (g, model_of(g, bwd_upstream(g)))
    return _mid_references[angle_mode]


@pytest.mark.parametrize("angle_mode", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_mid_size(dtype, angle_mode):
    """C2 levels, 300 queries, B 2, H 8, C 32: 75 and more workgroups, the XCD re-map, real contention of the adds."""
    dt = DTYPES[dtype]
    g, ref = mid_reference(angle_mode)
    args = box_args(g, dt)
    gout = dev(bwd_upstream(g), dt)
    what = "box backward with grad_value: %s C=32 angle=%d [%s storage]" % (MID, angle_mode, dtype)
    got = value_call(args, gout)
    report(what, dt, "grad_value", hold_value(got[0], ref, dt, args[0], what))
    same_parameter_gradients(got[1:], points_call(args, gout), what)


def raw_entry(dtype, a, dims, gout, want, grad_value, ws, ws_bytes, outs):
    """boxattn_bwd_boxes_value_* with the device arguments ``a`` (boxes_cases.device_args)."""
    from boxer_amd import _lib
    entry = getattr(_lib.load(), "boxattn_bwd_boxes_value_" + dtype)
    ptr = lambda t: None if t is None else t.data_ptr()
    return entry(ptr(a["value"]), ptr(a["shapes"]), ptr(a["lsi"]), ptr(a["ref"]), a["ref"].size(-1),
                 int(a["ref"].dim() == 4), ptr(a["off"]), a["off"].size(-1), a["mode"], ptr(a["kidx"]), ptr(a["vr"]),
                 ptr(a["logits"]), ptr(gout), *dims, want, ptr(grad_value), ptr(ws), ws_bytes,
                 *[ptr(t) for t in outs], torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_no_queries_and_no_pixels(dtype):
    """The raw entry: without queries grad_value is zero-filled and nothing else is written; without pixels the three
    parameter gradients are zeros."""
    from boxer_amd import _lib
    dt = DTYPES[dtype]
    g = boxes_cases.box_bwd_case("model", 32, 1, 5, False, True)
    B, S, H, C, L, Lq, P = g["dims"]
    a = boxes_cases.device_args(g, dt)
    gout = dev(boxes_cases.box_upstream(g, dt), dt)
    outs = [torch.full((B, Lq, H, L, n), 7.0, dtype=torch.float32, device="cuda") for n in (5, 5, P)]
    ws_bytes = _lib.box_bwd_boxes_value_workspace_bytes(a["value"].element_size(), g["dims"])
    ws = torch.full((max(ws_bytes // 4, 4),), 3.0, dtype=torch.float32, device="cuda")
    for want in (1, 3):
        gv = torch.full((B, S, H, C), 7.0, device="cuda").to(dt)
        for t in outs:
            t.fill_(7.0)
        none = dict(a, ref=a["ref"][:, :0], off=a["off"][:, :0])
        assert raw_entry(dtype, none, (B, S, H, C, L, 0, P), None, want, gv, ws, ws_bytes, outs) == 0
        torch.cuda.synchronize()
        assert not gv.any(), "no queries: grad_value is zeros (want %d)" % want
        assert all(bool((t == 7.0).all()) for t in outs), "a call without queries wrote a parameter gradient"
        empty = torch.empty((B, 0, H, C), dtype=dt, device="cuda")
        assert raw_entry(dtype, dict(a, value=None), (B, 0, H, C, L, Lq, P), gout, want, empty, None, 0, outs) == 0
        torch.cuda.synchronize()
        if want == 3:
            assert all(not t.any() for t in outs), "no pixels: the parameter gradients are zeros"
        else:
            assert all(bool((t == 7.0).all()) for t in outs), "grad_value alone: the parameter gradients are not written"


def test_argument_errors_come_before_any_device_call():
    from boxer_amd import ops
    g = boxes_cases.box_bwd_case("model", 32, 1, 5, False, True)
    B, S, H, C, L, Lq, P = g["dims"]
    args = box_args(g, torch.float32)
    gout = dev(bwd_upstream(g), torch.float32)
    orig, calls = ops._grid_call, []
    ops._grid_call = lambda *a, **k: calls.append(a[0])
    try:
        for want in (0, 4, -1, None, True, "3", 1.5):
            with pytest.raises(ValueError, match="box_attn_backward_boxes_value"):
                ops.box_attn_backward_boxes_value(*args, gout, want=want)
        for bad in (gout.to(torch.bfloat16), gout.double(), gout[:, :-1].contiguous(), gout.view(-1)[:-1],
                    gout.cpu()):
            with pytest.raises(ValueError, match="box_attn_backward_boxes_value"):
                ops.box_attn_backward_boxes_value(*args, bad)
        with pytest.raises(TypeError):
            ops.box_attn_backward_boxes_value(*args, None)
        with pytest.raises(ValueError, match="box_attn_backward_boxes_value"):
            ops.box_attn_backward_boxes_value(args[0].double(), *args[1:], gout.double())
        assert calls == []
        ops.box_attn_backward_boxes_value(*args, gout)                  # (the arguments as they should be: one call)
        assert calls == ["boxattn_bwd_boxes_value_f32"]
    finally:
        ops._grid_call = orig


# ------------------------------------------------------------------ the autograd Function
class Spies:
    """Counts the calls of the ops functions a training step from boxes may reach."""
    WATCHED = ("box_attn_backward_boxes_value", "box_attn_backward_boxes", "box_attn_backward", "box_grid_forward",
               "softmax_forward")

    def __enter__(self):
        from boxer_amd import ops
        self.ops, self.n = ops, {name: 0 for name in self.WATCHED}
        self.orig = {name: getattr(ops, name) for name in self.WATCHED}

        def spy(name, fn):
            def inner(*a, **k):
                self.n[name] += 1
                return fn(*a, **k)
            return inner
        for name, fn in self.orig.items():
            setattr(ops, name, spy(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(self.ops, name, fn)


def only(name):
    return dict({n: 0 for n in Spies.WATCHED}, **{name: 1})


def exact_problem(g):
    """``g`` with a value every storage type holds exactly: one float64 model serves the three types."""
    return dict(g, value=boxes_cases.every_type(g["value"]))


def run_function(fn, x, dt):
    value = x["value"] if dt == torch.float32 else x["value"].to(dt)
    vr = None if x["vr"] is None else x["vr"].view(-1, x["off"].size(3), 2)
    return fn.apply(value, x["shapes"], x["lsi"], x["ref"], x["off"], x["kidx"], vr, x["logits"], x["mode"])


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_function_against_the_function_it_completes(dtype):
    """A decoder-like case (5 queries against 138 pixels): the same output, parameter gradients bit for bit those of
    ``BoxAttnBoxesFunction``, both grad_values within the bound (the binned backward's with the split term of its
    accumulate route, this one's with none), and the backward is one ops call that builds neither a grid nor
    weights."""
    from boxer_amd import BoxAttnBoxesFunction, BoxAttnBoxesValueFunction, _lib
    dt = DTYPES[dtype]
    g = exact_problem(boxes_cases.box_bwd_case("model", 32, 1, 5, False, True))
    gout64 = bwd_upstream(g)
    gout = dev(gout64).float()
    ref = model_of(g, gout64)
    res = {}
    for name, fn in (("value", BoxAttnBoxesValueFunction), ("boxes", BoxAttnBoxesFunction)):
        x = boxes_cases.function_inputs(g)
        out = run_function(fn, x, dt)
        with Spies() as spies:
            (out.float() * gout).sum().backward()
        torch.cuda.synchronize()
        res[name] = (out, [x[n].grad for n in boxes_cases.LEAVES], spies.n)
    (o_v, g_v, n_v), (o_b, g_b, n_b) = res["value"], res["boxes"]
    assert o_v.dtype == dt and torch.equal(o_v, o_b)
    assert n_v == only("box_attn_backward_boxes_value"), n_v
    assert n_b["box_attn_backward_boxes_value"] == 0 and n_b["box_attn_backward_boxes"] == 1, n_b
    for name, a, b in zip(boxes_cases.LEAVES, g_v, g_b):
        assert a is not None and a.dtype == torch.float32 and a.shape == b.shape, name
        if name != "value":
            assert torch.equal(a, b), "gradient of %s differs from BoxAttnBoxesFunction's" % name
    acc = _lib.bwd_accumulate_kind(2 if dt != torch.float32 else 4, 0, g["dims"])
    from route_vocab import split_of
    what = "Function, model C=32 [%s storage]" % dtype
    report("BoxAttnBoxesValueFunction: " + what, dt, "grad_value", eb.hold(g_v[0], ref, dt, "none", what))
    report("BoxAttnBoxesFunction: " + what, dt, "grad_value",
           eb.hold(g_b[0], ref, dt, split_of(acc, dt) if acc >= 0 else "none", what))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_function_computes_only_what_is_asked_for(dtype):
    """A frozen ``value``: want = 2 and no grad_value; frozen heads: want = 1; each time one call."""
    from boxer_amd import BoxAttnBoxesValueFunction, ops
    dt = DTYPES[dtype]
    g = exact_problem(boxes_cases.box_bwd_case("model", 32, 1, 5, False, True))
    gout = dev(bwd_upstream(g)).float()
    full = boxes_cases.function_inputs(g)
    (run_function(BoxAttnBoxesValueFunction, full, dt).float() * gout).sum().backward()
    ref = model_of(g, bwd_upstream(g))
    wants = []
    orig = ops.box_attn_backward_boxes_value
    spy = lambda *a, **k: wants.append(k["want"]) or orig(*a, **k)
    for only, want in (("value", 1), ("logits", 2), ("off", 2), (None, 3)):
        x = boxes_cases.function_inputs(g)
        for n in boxes_cases.LEAVES:
            x[n].requires_grad_(only is None or n == only)
        out = run_function(BoxAttnBoxesValueFunction, x, dt)
        del wants[:]
        ops.box_attn_backward_boxes_value = spy
        try:
            with Spies() as spies:
                (out.float() * gout).sum().backward()
        finally:
            ops.box_attn_backward_boxes_value = orig
        torch.cuda.synchronize()
        assert wants == [want], (only, wants)
        assert spies.n["box_attn_backward"] == 0 and spies.n["box_grid_forward"] == 0 and spies.n["softmax_forward"] == 0
        for n in boxes_cases.LEAVES:
            if only is not None and n != only:
                assert x[n].grad is None, (only, n)
            elif n == "value":
                eb.hold(x[n].grad, ref, dt, "none", "only=%s: grad_value %s" % (only, dtype))
            else:
                assert torch.equal(x[n].grad, full[n].grad), (only, n)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_function_saves_no_per_point_tensor_and_builds_none_in_the_backward(dtype):
    from boxer_amd import BoxAttnBoxesValueFunction, ops
    dt = DTYPES[dtype]
    g = boxes_cases.box_bwd_case("k4", 32, 1, 5, True, True)
    if not boxes_cases.eligible("k4", 32, dt):
        g = boxes_cases.box_bwd_case("odd_k", 32, 1, 5, True, True)
    B, S, H, C, L, Lq, P = g["dims"]
    x = boxes_cases.function_inputs(g)
    out = run_function(BoxAttnBoxesValueFunction, x, dt)
    saved = [t for t in out.grad_fn.saved_tensors if t is not None]
    value_bytes = B * S * H * C * (4 if dt == torch.float32 else 2)
    total = sum(t.numel() * t.element_size() for t in saved)
    assert total < value_bytes + 64 * B * Lq * H * L * 4
    for t in saved:
        assert t.dim() < 5 or t.shape[-1] != P, tuple(t.shape)       # (no (.., L, P[, 2]) tensor)
        assert t.dim() != 6, tuple(t.shape)

    def refuse(*a, **k):
        raise AssertionError("the backward built a per-point tensor")
    orig = ops.box_grid_forward, ops.softmax_forward
    ops.box_grid_forward = ops.softmax_forward = refuse
    try:
        out.float().square().sum().backward()
    finally:
        ops.box_grid_forward, ops.softmax_forward = orig
    torch.cuda.synchronize()
    assert all(x[n].grad is not None for n in boxes_cases.LEAVES)


# ------------------------------------------------------------------ the modules
def both_flags(m, value):
    m.fused_boxes_train, m.fused_boxes_value = True, value


@pytest.mark.parametrize("native_bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", boxes_cases.G9_NAMES)
def test_module_reference_golden(name, native_bf16):
    """The G9 goldens with ``fused_boxes_train`` and ``fused_boxes_value``: fewer queries than pixels -> exactly one
    ``ops.box_attn_backward_boxes_value`` call and no other backward; as many queries as pixels (the encoder
    goldens) -> ``BoxAttnBoxesFunction`` as without the flag.  Either way the output and every gradient meet the
    reference's at the tolerances tests/test_gpu_box_boxes_backward.py holds these fixtures to.  ``fused_boxes_value``
    alone changes nothing."""
    m, g, args = boxes_cases.box_golden_module(name, native_bf16)
    assert m.fused_boxes_value is False
    Lq, S = args[0].size(1), args[1].size(1)
    cross = Lq < S
    assert cross == name.endswith("_dec"), (name, Lq, S)
    tol = 4e-2 if native_bf16 else 2e-4
    rms_only = ("ref_windows", "linear_box", "query") if native_bf16 else ()
    both_flags(m, True)
    with Spies() as spies:
        outs, grads = boxes_cases.module_grads(m, args, boxes_cases.golden_loss(g), torch.bfloat16 if native_bf16 else None)
    torch.cuda.synchronize()
    assert outs[1] == ()
    if cross:
        assert spies.n == only("box_attn_backward_boxes_value"), spies.n
    else:
        assert spies.n["box_attn_backward_boxes_value"] == 0 and spies.n["box_attn_backward_boxes"] == 1, spies.n
    boxes_cases._g9_check(name, outs[:1], grads, g, tol, "fused_boxes_value bf16=%s" % native_bf16, rms_only=rms_only)
    m.fused_boxes_train, m.fused_boxes_value = False, True
    with Spies() as spies:
        outs, _ = boxes_cases.module_grads(m, args, boxes_cases.golden_loss(g), torch.bfloat16 if native_bf16 else None)
    assert spies.n["box_attn_backward_boxes_value"] == 0 and isinstance(outs[1], torch.Tensor)


@pytest.mark.parametrize("name", [n for n in boxes_cases.G9_NAMES if not n.endswith("_dec")])
def test_module_with_as_many_queries_as_pixels_is_unchanged(name):
    """Lq = S: the flag changes nothing -- the output and the parameter gradients are bit for bit those without it
    (the same Function, whose grad_value sums in a fixed order at these shapes or within 1e-4 where it does not)."""
    m, g, args = boxes_cases.box_golden_module(name)
    res = {}
    for flag in (False, True):
        both_flags(m, flag)
        res[flag] = boxes_cases.module_grads(m, args, boxes_cases.golden_loss(g))
    torch.cuda.synchronize()
    (o_off, g_off), (o_on, g_on) = res[False], res[True]
    assert torch.equal(o_on[0], o_off[0])
    for k in g_on:
        compare_rules.check_scaled(g_on[k], g_off[k].double().cpu().numpy(), 1e-4, "%s gradient of %s" % (name, k))


@pytest.mark.parametrize("what", ["float64", "cpu", "no_grad", "instance"])
def test_module_falls_through(what):
    """Flags on where the step from boxes does not run: no call of the new backward."""
    import boxer_amd
    m, g, args = boxes_cases.box_golden_module("G9_module_box_dec")
    args = list(args)
    both_flags(m, True)
    if what == "cpu":
        B, S = args[1].shape[:2]
        assert m._boxes_train(args[0].cpu(), torch.zeros(B, S, 8, 32), None) is None
        assert m._boxes_train(args[0], torch.zeros(B, S, 8, 32, device="cuda"), None) is not None      # (the control)
        return
    if what == "instance":
        inst = boxer_amd.InstanceAttention(256, 4, 8, 4)
        assert inst.fused_boxes_value is False
        assert not hasattr(boxer_amd.InstanceAttention, "_boxes_train_function")
        return
    if what == "float64":
        m = m.double()
        args = [a.double() if a is not None and a.is_floating_point() else a for a in args]
    with Spies() as spies:
        if what == "no_grad":
            with torch.no_grad():
                out, weights = m(*args)
        else:
            (out, weights), grads = boxes_cases.module_grads(m, args, lambda outs: outs[0].square().sum())
            assert all(v is not None for v in grads.values())
    torch.cuda.synchronize()
    assert spies.n["box_attn_backward_boxes_value"] == 0 and spies.n["box_attn_backward_boxes"] == 0, spies.n
    assert isinstance(weights, torch.Tensor) and weights.shape[-2:] == (2, 2)
