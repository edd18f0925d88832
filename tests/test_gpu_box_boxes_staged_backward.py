"""GPU tests (``-m gpu``) of box attention's training step from boxes and L*P logits on the WINDOW-STAGED kernels: the
one-launch box and logit gradients of the encoder case (``ops.box_attn_backward_boxes_staged``, include/boxattn.h
boxattn_bwd_boxes_hl_*), the autograd Function on top of it and of the staged forward
(``BoxAttnBoxesStagedFunction``) and the module flag ``fused_boxes_train_staged`` in BoxAttention / Box3dAttention.
Every case has one query a pixel, 32 channels a head and 2 x 2 points a level: the only shapes the entry accepts.

The inputs are boxes_cases.staged_problem's -- the geometries (whole tiles, ragged tiles, H = 3, a level
smaller than a tile, a 1 x 1 level, a staged sub-window) and the two families: ``local``, served from the staged
windows, and ``scattered``, the in-kernel global path -- four of them from another seed
(tests/test_box_boxes_staged_backward_cases.py: the cell-edge condition of every case, proven on the CPU).

Every (geometry, family, type) of the seeded matrix holds the three float32 outputs of the one call, over the flavours
of ``flavours_of``,
  * per element within error_bounds.bound of the float64 model from boxes and logits (error_bounds.boxes_reference with
    grad_out), weight split "none" in every storage type: the split test_gpu_error_bounds.py applies to grad_loc /
    grad_attn of the window-staged point-gradient route (the per-point gradients are float32 products of float32
    weights whatever the storage).  Where the model says zero the bound is zero: the size gradients of a box of size
    <= 0, the rows of a window wholly outside the map, the angle entries of mode 0;
  * at POINT_TOL against this build's chain -- ``ops.box_grid_forward`` -> ``ops.softmax_forward`` ->
    ``ops.box_attn_backward(want=2)``, window-staged route asserted -> ``ops.box_grid_backward`` +
    ``ops.softmax_backward`` -- and against ``ops.box_attn_backward_boxes``, the row gather from the same operands."""
import functools

import numpy as np
import pytest
import torch

import error_bounds as eb
import isolation as iso
from boxes_cases import (FAMILIES, GRAD_NAMES, LEAVES, MATRIX, STAGED_C as C, STAGED_P as P, encoder_module,
                         flavours_of, function_inputs, kernel_offsets, operands, run_boxes_function,
                         run_point_functions, run_staged_backward as run_staged, staged_bwd_case as case,
                         staged_upstream as upstream)
from compare_rules import POINT_TOL, check_scaled as check, exact_zeros, must_be_zero, report_bound as report, tol_of
from route_vocab import DTYPES, STAGED, dev

pytestmark = pytest.mark.gpu

SPLIT = "none"            # grad_loc / grad_attn of the window-staged point-gradient route, every storage type


@functools.lru_cache(maxsize=16)
def reference(geometry, family, flavour):
    """The float64 model's planes of the three gradients, computed once for the three storage types."""
    g = case(geometry, family, *flavour[0], *flavour[1:])
    return eb.boxes_reference("box", g["value"], g["shapes"], g["lsi"], g["ref"], g["off"], kernel_offsets(2), g["vr"],
                              g["logits"], g["angle_mode"], grad_out=upstream(g))


def chain(g, args, gout):
    """This build's chain on the same operands, the window-staged route asserted -> (the three gradients, the grid)."""
    from boxer_amd import ops
    B, S, H, _, L, Lq, _ = g["dims"]
    value, shapes, lsi, ref, off, kidx, vr, logits, mode = args
    grid = ops.box_grid_forward(ref, off, kidx, vr, mode)
    attn = ops.softmax_forward(logits)
    taken = ops.forward_route(value, grid, shapes, lsi)
    assert taken == STAGED, "the chain takes route %d, wanted the window-staged one" % taken
    _, gloc, gattn = ops.box_attn_backward(value, shapes, lsi, grid, attn.view(B, Lq, H, L, P), gout, 64, want=2)
    goff, rows = ops.box_grid_backward(ref, off, kidx, vr, mode, gloc, need_ref_grad=True)
    glog = ops.softmax_backward(attn, gattn.view(attn.shape), torch.float32)
    return (goff, rows, glog), grid


def hold_legs(got, legs, what):
    """``got`` against (name of the leg, its three tensors) at POINT_TOL."""
    for leg, want in legs:
        for name, t, w in zip(GRAD_NAMES, got, want):
            assert t.shape == w.shape, name
            check(t, w.double().cpu().numpy(), POINT_TOL, "%s %s against %s" % (what, name, leg))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("geometry", MATRIX)
def test_seeded_matrix(geometry, family, dtype):
    """Angle modes 0, 1 (reference windows of 5 and 7 values) and 2 x reference windows shared and per head x
    valid_ratios None and given; "four_levels" with the four (angle mode, reference values) pairs (flavours_of)."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    worst, zeros = {}, {n: 0 for n in GRAD_NAMES}
    for flavour in flavours_of(geometry):
        (angle_mode, ref_dim), per_head, with_vr = flavour
        g = case(geometry, family, angle_mode, ref_dim, per_head, with_vr)
        what = "staged backward from boxes: %s %s %s angle=%d D=%d per_head=%d vr=%d" % (
            geometry, family, dtype, angle_mode, ref_dim, per_head, with_vr)
        args = operands(g, dt)
        gout = dev(upstream(g), dt)
        got = run_staged(g, args, gout)
        legs, grid = chain(g, args, gout)
        gather = ops.box_attn_backward_boxes(*args, gout, need_ref_grad=True)
        torch.cuda.synchronize()
        ref = reference(geometry, family, flavour)
        assert ref["edge_share"] <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (what, 100 * ref["edge_share"])
        for name, t in zip(GRAD_NAMES, got):
            w = eb.hold(t, ref[name], torch.float32, SPLIT, "%s: %s" % (what, name))
            print("%s %s: worst err / bound %.3f" % (what, name, w))
            worst[name] = max(worst.get(name, 0.0), w)
            zeros[name] += must_be_zero(ref[name])
        exact_zeros(g, got, grid.double().cpu().numpy(), what)
        hold_legs(got, (("the chain", legs), ("ops.box_attn_backward_boxes", gather)), what)
    route = "window-staged backward from boxes: %s %s [%s storage]" % (geometry, family, dtype)
    for name, w in worst.items():
        assert zeros[name] > 0, "%s: no must-be-zero element of %s in the case" % (route, name)
        report("%s (%d must-be-zero elements)" % (route, zeros[name]), torch.float32, name, w)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_two_runs_are_bitwise_equal(dtype):
    dt = DTYPES[dtype]
    for family in FAMILIES:
        g = case("four_levels", family, 1, 5, True, False)
        args = operands(g, dt)
        gout = dev(upstream(g), dt)
        first = run_staged(g, args, gout)
        again = run_staged(g, args, gout)
        torch.cuda.synchronize()
        for name, x, y in zip(GRAD_NAMES, first, again):
            assert torch.equal(x, y), "%s: two runs differ (the kernel has no atomics; %s)" % (name, family)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_mid_size(dtype):
    """C2 levels, B 2, H 8, angle mode 0, local windows: 5 400 workgroups.  Against the chain and the row gather only
    (the float64 model is too slow here)."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    g = case("mid", "local", 0, 4, False, True)
    args = operands(g, dt)
    gout = dev(upstream(g), dt)
    got = run_staged(g, args, gout)
    legs, _ = chain(g, args, gout)
    gather = ops.box_attn_backward_boxes(*args, gout, need_ref_grad=True)
    torch.cuda.synchronize()
    hold_legs(got, (("the chain", legs), ("ops.box_attn_backward_boxes", gather)), "mid %s" % dtype)


def offset_copy(t):
    """The same tensor 8 bytes off a 16-byte boundary."""
    n = 8 // t.element_size()
    flat = torch.zeros(t.numel() + n, dtype=t.dtype, device=t.device)
    view = flat[n:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


class Launches:
    """The entry points ops._grid_call reaches while it is active."""

    def __enter__(self):
        from boxer_amd import ops
        self.ops, self.orig, self.names = ops, ops._grid_call, []
        ops._grid_call = lambda *a, **k: self.names.append(a[0]) or self.orig(*a, **k)
        return self

    def __exit__(self, *exc):
        self.ops._grid_call = self.orig


@pytest.mark.parametrize("which", ["value", "grad_out"])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_rows_off_a_16_byte_boundary_are_refused(dtype, which):
    """``value`` or ``grad_out`` 8 bytes off a 16-byte boundary: ValueError before any device call (the launch spy sees
    nothing); the same operands aligned are accepted."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    g = case("two_levels", "local", 0, 4, False, False)
    Lq = g["dims"][5]
    args = operands(g, dt)
    gout = dev(upstream(g), dt)
    bad_args, bad_gout = args, gout
    if which == "value":
        bad_args = operands(g, dt, value=offset_copy(args[0]))
        assert not ops.box_backward_boxes_staged_ok(bad_args[0], args[1], args[2], Lq, P)
    else:
        bad_gout = offset_copy(gout)
        assert not ops.box_backward_boxes_staged_ok(args[0], args[1], args[2], Lq, P, also=[bad_gout])
    with Launches() as seen:
        with pytest.raises(ValueError):
            ops.box_attn_backward_boxes_staged(*bad_args, bad_gout, need_ref_grad=True)
        assert not seen.names
        run_staged(g, args, gout)
        torch.cuda.synchronize()
        assert seen.names == ["boxattn_bwd_boxes_hl_" + dtype]


def test_decoder_queries_are_refused():
    """Fewer queries than pixels: there is no other kernel behind the call."""
    from boxer_amd import ops
    g = case("two_levels", "scattered", 0, 4, False, False)
    value, shapes, lsi, ref, off, kidx, vr, logits, mode = operands(g, torch.float32)
    gout = dev(upstream(g), torch.float32)
    few = (value, shapes, lsi, ref[:, :5].contiguous(), off[:, :5].contiguous(), kidx, vr, logits[:, :5].contiguous(), mode)
    assert not ops.box_backward_boxes_staged_ok(value, shapes, lsi, 5, P)
    with Launches() as seen:
        with pytest.raises(ValueError):
            ops.box_attn_backward_boxes_staged(*few, gout[:, :5].contiguous(), need_ref_grad=True)
        assert not seen.names
    assert ops.box_backward_boxes_ok(value, len(g["shapes"]), 5, P)           # (the row gather takes them)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_without_ref_grad_no_rows_are_written(dtype):
    dt = DTYPES[dtype]
    g = case("three_levels", "local", 1, 7, True, True)
    args = operands(g, dt)
    gout = dev(upstream(g), dt)
    with_rows = run_staged(g, args, gout)
    without = run_staged(g, args, gout, need_ref_grad=False)
    torch.cuda.synchronize()
    assert without[1] is None
    assert torch.equal(with_rows[0], without[0]) and torch.equal(with_rows[2], without[2])


# ------------------------------------------------------------------ the autograd Function
def run_staged_function(x, dt):
    from boxer_amd import BoxAttnBoxesStagedFunction
    value = x["value"] if dt == torch.float32 else x["value"].to(dt)
    vr = None if x["vr"] is None else x["vr"].view(-1, x["off"].size(3), 2)
    return BoxAttnBoxesStagedFunction.apply(value, x["shapes"], x["lsi"], x["ref"], x["off"], x["kidx"], vr, x["logits"],
                                            x["mode"])


class Counters:
    """Counts the calls of the ops functions the two Functions' backward passes choose between."""
    NAMES = {"staged": "box_attn_backward_boxes_staged", "gather": "box_attn_backward_boxes", "value": "box_attn_backward",
             "staged_forward": "box_attn_forward_boxes_staged", "gather_forward": "box_attn_forward_boxes"}

    def __enter__(self):
        from boxer_amd import ops
        self.ops, self.n = ops, {k: 0 for k in self.NAMES}
        self.orig = {k: getattr(ops, name) for k, name in self.NAMES.items()}

        def spy(key, fn):
            def inner(*a, **k):
                self.n[key] += 1
                return fn(*a, **k)
            return inner
        for key, name in self.NAMES.items():
            setattr(ops, name, spy(key, self.orig[key]))
        return self

    def __exit__(self, *exc):
        for key, name in self.NAMES.items():
            setattr(self.ops, name, self.orig[key])


@pytest.mark.parametrize("angle_mode,per_head", [(0, False), (1, True)], ids=["plain_shared", "turns_per_head"])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_function_equals_the_row_gather_function(dtype, angle_mode, per_head):
    dt = DTYPES[dtype]
    g = case("three_levels", "local", angle_mode, 5 if angle_mode else 4, per_head, True)
    gout = dev(upstream(g)).float()
    res = {}
    for name, run in (("staged", run_staged_function), ("gather", run_boxes_function)):
        x = function_inputs(g)
        with Counters() as c:
            out = run(x, dt)
            (out.float() * gout).sum().backward()
        assert (c.n["staged"], c.n["staged_forward"]) == ((1, 1) if name == "staged" else (0, 0)), c.n
        res[name] = (out, [x[n].grad for n in LEAVES])
    torch.cuda.synchronize()
    (o_s, g_s), (o_g, g_g) = res["staged"], res["gather"]
    what = "%s angle=%d per_head=%d" % (dtype, angle_mode, per_head)
    assert o_s.dtype == dt and o_s.shape == o_g.shape
    check(o_s, o_g.detach().double().cpu().numpy(), tol_of(dt), "out " + what)
    for name, a, b in zip(LEAVES, g_s, g_g):
        assert a is not None and a.dtype == torch.float32 and a.shape == b.shape, name
        check(a, b.double().cpu().numpy(), tol_of(dt), "grad of %s %s" % (name, what))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_function_computes_only_what_is_asked_for(dtype):
    """Only ``value`` / only ``logits`` requiring a gradient: the others stay None and the call that is not needed is
    not made; the row gather's backward is never made."""
    dt = DTYPES[dtype]
    g = case("two_levels", "local", 1, 5, False, True)
    gout = dev(upstream(g)).float()
    ref = function_inputs(g)
    (run_point_functions(ref, dt).float() * gout).sum().backward()
    want = {n: ref[n].grad for n in LEAVES}
    for only, calls in (("value", (0, 1)), ("logits", (1, 0)), (None, (1, 1))):
        x = function_inputs(g)
        for n in LEAVES:
            x[n].requires_grad_(only is None or n == only)
        with Counters() as c:
            (run_staged_function(x, dt).float() * gout).sum().backward()
        torch.cuda.synchronize()
        assert (c.n["staged"], c.n["value"], c.n["gather"]) == calls + (0,), (only, c.n)
        for n in LEAVES:
            if only is not None and n != only:
                assert x[n].grad is None, n
                continue
            check(x[n].grad, want[n].double().cpu().numpy(), tol_of(dt) if n == "value" else POINT_TOL,
                  "only=%s: grad of %s %s" % (only, n, dtype))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_function_saves_no_per_point_tensor(dtype):
    dt = DTYPES[dtype]
    g = case("three_levels", "scattered", 1, 5, True, True)
    B, S, H, _, L, Lq, _ = g["dims"]
    out = run_staged_function(function_inputs(g), dt)
    saved = [t for t in out.grad_fn.saved_tensors if t is not None]
    value_bytes = B * S * H * C * (4 if dt == torch.float32 else 2)
    total = sum(t.numel() * t.element_size() for t in saved)
    print("saved for the backward: %d bytes in %d tensors (value: %d)" % (total, len(saved), value_bytes))
    assert total < value_bytes + 64 * B * Lq * H * L * 4
    for t in saved:
        assert t.dim() < 5 or t.shape[-1] != P, tuple(t.shape)       # (no (.., L, P[, 2]) tensor)
        assert t.dim() != 6, tuple(t.shape)


# ------------------------------------------------------------------ the modules
def module_step(m, args, native_bf16):
    m.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=native_bf16):
        out, second = m(*args)
    out.float().square().sum().backward()
    return out.detach().clone(), second, {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("native_bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["box", "box3d_rot"])
def test_module_flag_takes_both_staged_calls_on_encoder_input(kind, native_bf16):
    """Grad mode, ``fused_boxes_train`` + ``fused_boxes_train_staged``: one call each of the staged forward and the
    staged backward and none of the row gather's; output and every parameter gradient equal the flag-off module's at
    tol_of."""
    m, args = encoder_module(kind, native_bf16)
    assert m.fused_boxes_train_staged is False
    m.fused_boxes_train = True
    res = {}
    for flag in (True, False):
        m.fused_boxes_train_staged = flag
        with Counters() as c:
            res[flag] = module_step(m, args, native_bf16)
        taken = (c.n["staged_forward"], c.n["staged"], c.n["gather_forward"], c.n["gather"])
        assert taken == ((1, 1, 0, 0) if flag else (0, 0, 1, 1)), "flag %s: %s" % (flag, c.n)
        assert res[flag][1] == ()
    torch.cuda.synchronize()
    tol = tol_of(torch.bfloat16 if native_bf16 else torch.float32)
    check(res[True][0], res[False][0].double().cpu().numpy(), tol, "%s: out, staged flag on against off" % kind)
    for k, grad in res[True][2].items():
        check(grad, res[False][2][k].double().cpu().numpy(), tol, "%s: grad of %s, staged flag on against off" % (kind, k))


@pytest.mark.parametrize("what", ["decoder_queries", "train_flag_off"])
def test_module_elsewhere_never_makes_the_staged_calls(what):
    """With decoder queries, and with ``fused_boxes_train`` off, the staged calls are never made and the results are
    those of the module without the flag."""
    m, args = encoder_module("box", False)
    if what == "decoder_queries":
        torch.manual_seed(5)
        query = torch.randn(2, 5, 64, device="cuda")
        ref = torch.rand(2, 5, 4, device="cuda") * 0.5 + 0.25
        args = (query,) + args[1:6] + (ref,)
    m.fused_boxes_train = what == "decoder_queries"
    res = {}
    for flag in (True, False):
        m.fused_boxes_train_staged = flag
        with Counters() as c:
            res[flag] = module_step(m, args, False)
        assert c.n["staged"] == 0 and c.n["staged_forward"] == 0, "flag %s: %s" % (flag, c.n)
        assert c.n["gather"] == (1 if what == "decoder_queries" else 0), c.n
    torch.cuda.synchronize()
    assert torch.equal(res[True][0], res[False][0]), "out differs between flag on and flag off"
    for k, grad in res[True][2].items():          # (grad_value sums in an order that changes from run to run)
        check(grad, res[False][2][k].double().cpu().numpy(), tol_of(torch.float32), "%s: grad of %s" % (what, k))


def test_instance_attention_ignores_the_flag():
    import boxer_amd
    torch.manual_seed(3)
    m = boxer_amd.InstanceAttention(64, 2, 2, 4).cuda()
    m.fused_boxes_train = m.fused_boxes_train_staged = True
    assert not hasattr(m, "_boxes_train_function")


# ------------------------------------------------------------------ isolation
ISOLATION = {"local": (1, 5, True, False), "scattered": (1, 7, False, True)}     # flavours of flavours_of("four_levels")
INPUTS = ("value", "shapes", "lsi", "ref", "off", "kidx", "vr", "logits")


def hold_isolated(what, g, args, gout, unreferenced):
    """NaN in the ``unreferenced`` value rows (B, S, H), in the other batch entry, in the other head and around every
    input: the three outputs are bitwise the clean run's outside what was poisoned on purpose (isolation.check_outputs).
    -> the number of elements held."""
    B, S, H, _, L, Lq, _ = g["dims"]

    def run(value=None, tensors=None):
        a = list(args)
        if value is not None:
            a[0] = value
        if tensors is not None:
            a[:8] = [tensors.get(n, x) for n, x in zip(INPUTS, a[:8])]
        got = run_staged(g, tuple(a), gout if tensors is None else tensors["grad_out"])
        torch.cuda.synchronize()
        return dict(zip(GRAD_NAMES, got))
    clean = run()
    n = iso.check_outputs(clean, run(iso.poison_rows(args[0], unreferenced)), what=what + ": unreferenced rows")
    if B > 1:
        other = args[0].clone()
        other[1:] = float("nan")
        b1 = np.zeros((B, Lq, H), dtype=bool)
        b1[1:] = True
        n += iso.check_outputs(clean, run(other), bqh=b1, what=what + ": batch 1")
    if H > 1:
        other = args[0].clone()
        other[:, :, 1] = float("nan")
        h1 = np.zeros((B, Lq, H), dtype=bool)
        h1[:, :, 1] = True
        n += iso.check_outputs(clean, run(other), bqh=h1, what=what + ": head 1")
    arenas = {k: iso.input_arena(x) for k, x in zip(INPUTS + ("grad_out",), tuple(args[:8]) + (gout,)) if x is not None}
    n += iso.check_outputs(clean, run(tensors={k: a.view for k, a in arenas.items()}), what=what + ": guards")
    for k, a in arenas.items():
        assert iso.guards_intact(a), "the guards of input %s were written" % k
    print("isolation | %s | %d elements held bitwise, %.1f %% of the value rows unreferenced"
          % (what, n, 100 * iso.share(unreferenced)))
    return n


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("family", FAMILIES)
def test_outputs_depend_on_nothing_their_definition_does_not_name(family, dtype):
    """"four_levels" (B 2, H 3), one case of each family.  (Every query looks at every level here, so few rows -- none
    in the local family -- are unreferenced: the edge family below is the case where most are.)"""
    dt = DTYPES[dtype]
    g = case("four_levels", family, *ISOLATION[family])
    S = g["dims"][1]
    loc = eb.grid_reference(g["ref"], g["off"], kernel_offsets(2), g["vr"], g["angle_mode"])[0]
    un = ~iso.touched(g["shapes"], loc, 1, S, g["lsi"])
    hold_isolated("staged backward from boxes, four_levels %s %s" % (family, dtype), g, operands(g, dt),
                  dev(upstream(g), dt), un)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("edge", ["right", "top"])
def test_outputs_are_isolated_on_the_edge_family(edge, dtype):
    """isolation.boxes_problem on the levels of "four_levels", one query a pixel: every level's boxes crowd into one
    patch astride ``edge``, most of every level is unreferenced, and the rows a careless kernel would fetch instead are."""
    from boxes_cases import STAGED_GEOMETRY as GEOMETRY
    dt = DTYPES[dtype]
    geo = GEOMETRY["four_levels"]
    g = iso.boxes_problem(geo["levels"], "S", 2, edge, kind="box", B=geo["B"], H=geo["H"], angle_mode=1, ref_dim=5,
                          per_head=edge == "top", with_vr=edge == "right")
    assert iso.share(g["unreferenced"]) > 0.5, iso.share(g["unreferenced"])
    args = (dev(g["value"], dt), dev(g["shapes"]), dev(g["lsi"]), dev(g["ref"]), dev(g["off"]), dev(g["kidx"]),
            None if g["vr"] is None else dev(g["vr"]), dev(g["logits"]), g["angle_mode"])
    hold_isolated("staged backward from boxes, edge family %s %s" % (edge, dtype), g, args, dev(g["grad_out"], dt),
                  g["unreferenced"])
