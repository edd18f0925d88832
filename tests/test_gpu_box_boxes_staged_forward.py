"""GPU tests (``-m gpu``) of box attention's inference forward from boxes and L*P logits on the WINDOW-STAGED kernels
(``ops.box_attn_forward_boxes_staged``, include/boxattn.h boxattn_fwd_boxes_hl_*) and of the module flag
``fused_boxes_staged`` that takes it in BoxAttention / Box3dAttention.  Every case has one query a pixel, 32 channels
a head and 2 x 2 points a level: the only shapes the entry accepts.

Two families of inputs per geometry, both with the poisoned rows of test_gpu_box_boxes_forward.problem (windows wholly and
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

import numpy as np
import pytest
import torch

import error_bounds as eb
from test_gpu_box_boxes_forward import C2_LEVELS, FLAVOURS, hold, kernel_indices, tables
from test_gpu_boxes_error_bounds import every_type, kernel_offsets, report
from test_gpu_wide_box_forward import DTYPES, STAGED, check, dev, tol_of

pytestmark = pytest.mark.gpu

C, P = 32, 4
GEOMETRY = {
    "two_levels": dict(levels=[(8, 8), (4, 4)], B=1, H=2),                               # whole tiles
    # ragged tiles on every level, a head count that is neither 8 nor a power of two
    "four_levels": dict(levels=[(37, 23), (19, 12), (10, 6), (5, 3)], B=2, H=3),
    "three_levels": dict(levels=[(16, 16), (8, 8), (4, 4)], B=1, H=8),
    "one_level": dict(levels=[(9, 13)], B=2, H=1),
    "tiny_levels": dict(levels=[(4, 5), (2, 3), (1, 1)], B=1, H=2),                      # smaller than a tile, a 1 x 1 level
    # tile numbering and XCD order beyond a handful of workgroups (test_mid_size only)
    "mid": dict(levels=C2_LEVELS, B=2, H=8),
}
FAMILIES = ["local", "scattered"]
SPLIT = {"f32": "none", "bf16": "bf16", "f16": "f16"}


@functools.lru_cache(maxsize=None)
def problem(geometry, family, angle_mode, ref_dim, per_head, with_vr):
    """numpy / float32 inputs of one case (the same for every storage type): test_gpu_box_boxes_forward.problem with one
    query a pixel and the two families."""
    geo = GEOMETRY[geometry]
    shapes, lsi, S = tables(geo["levels"])
    B, H, L, Lq = geo["B"], geo["H"], len(geo["levels"]), S
    V = 5 if angle_mode == 1 else 4
    rng = np.random.default_rng(104729 + 1000 * sorted(GEOMETRY).index(geometry) + 500 * FAMILIES.index(family)
                                + 8 * angle_mode + 2 * ref_dim + per_head)
    rshape = (B, Lq, H) if per_head else (B, Lq)
    ref = np.concatenate([rng.uniform(0.05, 0.95, rshape + (2,)), rng.uniform(0.05, 0.7, rshape + (2,)),
                          rng.uniform(-3.0, 3.0, rshape + (ref_dim - 4,))], -1)
    if family == "local":                          # query i = pixel i: a window of four pixels of its own level
        rows = []
        for hl, wl in geo["levels"]:
            ys, xs = np.meshgrid(np.arange(hl), np.arange(wl), indexing="ij")
            rows.append(np.stack([(xs.ravel() + 0.5) / wl, (ys.ravel() + 0.5) / hl,
                                  np.full(hl * wl, 4.0 / wl), np.full(hl * wl, 4.0 / hl)], -1))
        win = np.concatenate(rows, 0)[None]        # (1, S, 4)
        ref[..., :4] = win[:, :, None, :] if per_head else win
    flat = ref.reshape(-1, ref_dim)
    flat[0, :4] = (2.6, 2.4, 0.2, 0.3)                       # a window wholly outside the map (valid ratios >= 0.5)
    flat[1, :4] = (0.97, 0.02, 0.5, 0.4)                     # ... and one partly outside
    flat[-1, :4] = (-0.7, 0.5, 0.3, 0.3)                     # wholly outside on the other side
    if ref_dim > 4:
        flat[2 % len(flat), 4] = 23.0                        # angles of several turns (mode 2: radians; 1: turns)
        flat[3 % len(flat), 4] = -7.25
    off = 3.0 * rng.standard_normal((B, Lq, H, L, V))
    if family == "local":
        off[..., :4] *= 0.5
    rows = off.reshape(-1, V)
    rows[rng.random(len(rows)) < 0.15, 2] = -12.0            # negative predicted sizes: relu puts every point on the
    rows[rng.random(len(rows)) < 0.15, 3] = -9.5             # centre line / centre
    rows[0, 2:4] = -8.0                                      # size exactly zero: w + (-8 / 8) w
    if V == 5:
        rows[1, 4] = 77.0                                    # 4.8 turns
    logits = 3.0 * rng.standard_normal((B, Lq, H, L * P))
    logits += 30.0 * np.where(rng.random((B, Lq, H, 1)) < 0.5, -1.0, 1.0)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(shapes=shapes, lsi=lsi, S=S, dims=(B, S, H, C, L, Lq, P),
                value=every_type(rng.standard_normal((B, S, H, C))),     # (numbers every storage type holds exactly)
                ref=f32(ref), off=f32(off), logits=f32(logits), angle_mode=angle_mode,
                vr=f32(rng.uniform(0.5, 1.0, (B, 1, 1, L, 1, 2))) if with_vr else None)


def flavours_of(geometry):
    """The 16 flavours; for the largest geometry of the matrix the four (angle mode, reference values) pairs with
    windows per head / valid ratios alternating (its float64 model is the slowest)."""
    if geometry != "four_levels":
        return FLAVOURS
    return [(pair, i % 2 == 1, i % 2 == 0) for i, pair in enumerate(sorted({f[0] for f in FLAVOURS}))]


@functools.lru_cache(maxsize=16)
def reference(geometry, family, flavour):
    """The float64 model's ``out`` planes, computed once for the three storage types."""
    (angle_mode, ref_dim), per_head, with_vr = flavour
    g = problem(geometry, family, angle_mode, ref_dim, per_head, with_vr)
    return eb.boxes_reference("box", g["value"], g["shapes"], g["lsi"], g["ref"], g["off"], kernel_offsets(2), g["vr"],
                              g["logits"], g["angle_mode"])["out"]


def operands(g, dt, value=None):
    return (dev(g["value"], dt) if value is None else value, dev(g["shapes"]), dev(g["lsi"]), dev(g["ref"]),
            dev(g["off"]), kernel_indices(P), None if g["vr"] is None else dev(g["vr"]), dev(g["logits"]),
            g["angle_mode"])


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


def run_staged(g, args):
    from boxer_amd import ops
    B, S, H, _, L, Lq, _ = g["dims"]
    assert ops.box_forward_boxes_staged_ok(args[0], args[1], args[2], Lq, P), "not eligible: %s" % (g["dims"],)
    out = ops.box_attn_forward_boxes_staged(*args)
    assert out.dtype == args[0].dtype and tuple(out.shape) == (B, Lq, H * C)
    return out


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
LEVELS = [(8, 8), (4, 4)]


def encoder_module(kind, native_bf16):
    """BoxAttention / rotated Box3dAttention with 2 heads of 32 channels and random parameters, and a small encoder input
    built as boxer_amd.layers builds it: -> (module, forward arguments)."""
    import boxer_amd
    from boxer_amd import layers
    torch.manual_seed(11)
    if kind == "box":
        m = boxer_amd.BoxAttention(64, len(LEVELS), 2)
    else:
        m = boxer_amd.Box3dAttention(64, len(LEVELS), 2, with_rotation=True)
    for p in m.parameters():
        torch.nn.init.normal_(p, std=0.1)
    m = m.cuda()
    m.native_bf16 = native_bf16
    m.fused_grid = m.fused_pointwise = True
    shapes, lsi, S = tables(LEVELS)
    B = 2
    if kind == "box":
        ref = layers.encoder_ref_windows_2d(LEVELS, B, device="cuda")
    else:
        ref = layers.encoder_ref_windows_3d(LEVELS, B, device="cuda")[:, :, :2].contiguous()
    src = torch.randn(B, S, 64, device="cuda")
    ratios = 0.5 + 0.5 * torch.rand(B, 1, 1, len(LEVELS), 1, 2, device="cuda")
    return m, (src + 0.1 * torch.randn_like(src), src, dev(shapes), None, dev(lsi), ratios, ref)


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
