"""GPU: the four kernels that take boxes and logits -- ``ops.box_attn_forward_boxes``,
``ops.box_attn_backward_boxes``, ``ops.instance_attn_forward_boxes``, ``ops.instance_attn_backward_boxes`` -- and their
building blocks each way (``ops.box_grid_forward`` / ``box_grid_backward``, ``ops.softmax_forward`` /
``softmax_backward``, ``ops.instance_weights_forward`` / ``instance_weights_backward``) held per element against
``error_bounds.boxes_reference``: a float64 model that starts from what the kernel receives (reference windows,
offsets, kernel_indices, valid ratios, logits), with nothing taken from a GPU chain.

The problems are those of tests/test_gpu_box_boxes_forward.py, tests/test_gpu_box_boxes_backward.py,
tests/test_gpu_boxes_forward.py and tests/test_gpu_boxes_backward.py (all of them built in tests/boxes_cases.py).
``value`` and the upstream gradients are rounded to bf16 and then to f16: numbers every storage type holds exactly, so
one reference serves the three types.  A case whose share of points within EDGE_PX + slack of a cell edge is above
EDGE_CAP takes another seed
(RESEED for the instance matrix, BWD_RESEED for the box training step; tests/test_boxes_error_bounds.py checks every
input here without a GPU).  The building blocks' backward kernels get exact float32 upstream gradients, so their bound
is the reduction's own roundings, the rotation allowance and the weights' dw.  Each case prints ``error-bound | route |
type | output | worst err / bound``; profiles/boxes_error_bounds.log and profiles/box_boxes_backward_error_bounds.log
are that table from one run each."""

import numpy as np
import pytest
import torch

import error_bounds as eb
import boxes_cases
import boxes_cases as box_cases
from boxes_cases import (BOX_GEOMETRIES, CHANNELS, GRAD_NAMES, GRID_FLAVOURS, GRID_POINTS, INST_FLAVOURS,
                         SOFTMAX_BWD_LENGTHS, SOFTMAX_BWD_ROWS, box_args, box_problem, box_reference, bwd_problem,
                         bwd_reference, bwd_upstream, cell_rows, cell_upstream, every_type, grid_problem, grid_upstream,
                         inst_problem, inst_reference, inst_upstream, kernel_offsets, offset_by_eight,
                         softmax_bwd_problem, softmax_rows)
from compare_rules import must_be_zero, report_bound as report, within
from route_vocab import DTYPES, dev

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ inputs and references (CPU)


# ------------------------------------------------------------------ running


def run_box(g, dt, value=None):
    from boxer_amd import ops
    B, S, H, C, L, Lq, P = g["dims"]
    args = box_args(g, dt, value)
    assert ops.box_forward_boxes_ok(args[0], L, Lq, P), "not eligible: %s %s" % (g["dims"], dt)
    out = ops.box_attn_forward_boxes(*args)
    torch.cuda.synchronize()
    assert out.dtype == dt
    return out


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("geometry", BOX_GEOMETRIES)
def test_box_forward_from_boxes(geometry, C, dtype):
    """fwd2_boxes_kernel over every flavour (angle modes 0, 1 with 5 and 7 reference values, 2 x windows shared and per
    head x valid ratios None and given).  The split is "none": float32 weights on the VALU."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    worst, zeros = 0.0, 0
    for flavour in box_cases.FLAVOURS:
        g = box_problem(geometry, C, flavour)
        B, S, H, _, L, Lq, P = g["dims"]
        if geometry == "k4" and not ops.box_forward_boxes_ok(torch.empty(B, S, H, C, dtype=dt, device="cuda"), L, Lq, P):
            with pytest.raises(ValueError):          # no row gather for this type at this C: an error, not a fall-back
                ops.box_attn_forward_boxes(*box_args(g, dt))
            continue
        ref = box_reference(geometry, C, flavour)["out"]
        what = "box from boxes: %s C=%d angle=%d D=%d per_head=%d vr=%d" % ((geometry, C) + flavour[0] + flavour[1:])
        worst = max(worst, eb.hold(run_box(g, dt), ref, dt, "none", what))
        zeros += int(((ref["A"] + ref["E"]) == 0).sum())
    report("box from boxes: %s C=%d (%d must-be-zero elements)" % (geometry, C, zeros), dt, "out", worst)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("geometry", ["model", "ragged"])
def test_box_forward_value_offset_by_eight_bytes(geometry, dtype):
    """A 16-bit ``value`` 8 bytes off a 16-byte boundary: 4 channels a lane instead of 8."""
    dt = DTYPES[dtype]
    flavour = ((1, 5), True, True)
    g = box_problem(geometry, 32, flavour)
    value = offset_by_eight(dev(every_type(g["value"]), dt))
    worst = eb.hold(run_box(g, dt, value=value), box_reference(geometry, 32, flavour)["out"], dt, "none",
                    "box from boxes, value offset: %s" % geometry)
    report("box from boxes: %s C=32, value 8 bytes off" % geometry, dt, "out", worst)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("k", boxes_cases.KERNEL_SIZES)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("geometry", sorted(boxes_cases.INST_GEOMETRY))
def test_instance_forward_and_backward_from_boxes(geometry, C, k, dtype):
    """ops.instance_attn_forward_boxes with and without mask_out and ops.instance_attn_backward_boxes with and without
    grad_mask (need_ref_grad), windows shared and per head x valid ratios None and given; the gradients are float32 in
    every storage type.  (One test for both: they share the reference.)"""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    worst, edge = {}, {}
    for per_head, with_vr in INST_FLAVOURS:
        g = inst_problem(geometry, C, k, per_head, with_vr)
        B, S, H, _, L, Lq = g["dims"]
        gout64, gmask64 = inst_upstream(g, k)
        value, gout, gmask = dev(every_type(g["value"]), dt), dev(gout64, dt), dev(gmask64, dt)
        a = (value, dev(g["shapes"]), dev(g["lsi"]), dev(g["ref"]), dev(g["off"]), dev(kernel_offsets(k)),
             None if g["vr"] is None else dev(g["vr"]), dev(g["logits"]), k)
        assert ops.forward_boxes_ok(value, L, Lq, k) and ops.backward_boxes_ok(value, L, Lq, k), \
            "not eligible: %s k=%d %s" % (g["dims"], k, dt)
        for with_mask in (True, False):
            ref = inst_reference(geometry, C, k, per_head, with_vr, with_mask)
            what = "instance from boxes: %s C=%d k=%d per_head=%d vr=%d mask=%d" % (geometry, C, k, per_head, with_vr,
                                                                                     with_mask)
            assert ref["edge_share"] <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (
                what, 100 * ref["edge_share"])
            out, mask = ops.instance_attn_forward_boxes(*a, with_mask)
            grads = ops.instance_attn_backward_boxes(*a, gout, gmask if with_mask else None, need_ref_grad=True)
            torch.cuda.synchronize()
            assert (mask is None) == (not with_mask) and out.dtype == dt
            got = dict(zip(GRAD_NAMES, grads), out=out, **({"mask_out": mask} if with_mask else {}))
            for name, t in got.items():
                store = dt if name in ("out", "mask_out") else torch.float32
                assert t.dtype == store, name
                key = "%s%s" % (name, "" if with_mask or name == "out" else " (no grad_mask)")
                worst[key] = max(worst.get(key, 0.0), eb.hold(t, ref[name], store, "none", "%s: %s" % (what, name)))
                if name in GRAD_NAMES:
                    edge[key] = max(edge.get(key, 0.0), eb.edge_dominated(ref[name]))
    route = "instance from boxes: %s C=%d k=%d" % (geometry, C, k)
    for name, w in worst.items():
        report(route, dt if name.split()[0] in ("out", "mask_out") else torch.float32, name, w)
    print("%s: share of elements whose bound is more than half edge allowance: %s"
          % (route, ", ".join("%s %.4f" % kv for kv in edge.items())))


# ------------------------------------------------------------------ the building blocks on their own
@pytest.mark.parametrize("P", GRID_POINTS)
def test_box_grid_forward_is_within_dloc(P):
    """ops.box_grid_forward against grid_reference within dloc: the three angle modes x windows shared and per head x
    valid ratios None and given, angles of several turns."""
    from boxer_amd import ops
    worst = {}
    for angle_mode, per_head, with_vr in GRID_FLAVOURS:
        g = grid_problem(P, angle_mode, per_head, with_vr)
        loc, dloc = eb.grid_reference(g["ref"], g["off"], g["kidx"], g["vr"], angle_mode)
        got = ops.box_grid_forward(dev(g["ref"]), dev(g["off"]), dev(g["kidx"]),
                                   None if g["vr"] is None else dev(g["vr"]), angle_mode)
        torch.cuda.synchronize()
        w = within(got, loc, dloc, "grid P=%d angle=%d per_head=%d vr=%d" % (P, angle_mode, per_head, with_vr))
        worst[angle_mode] = max(worst.get(angle_mode, 0.0), w)
    for angle_mode, w in sorted(worst.items()):
        report("box_grid_forward P=%d angle mode %d" % (P, angle_mode), torch.float32, "grid / dloc", w)


SOFTMAX_FWD_LENGTHS = [1, 4, 8, 12, 18, 32, 63, 64]


def softmax_forward_within_dw(n, dtype):
    from boxer_amd import ops
    dt = DTYPES[dtype]
    z = eb.round_to(softmax_rows(n), dt).astype(np.float32)          # (16-bit logits: exact inputs, the same dw applies)
    want, dw = eb.softmax_reference(z)
    got = ops.softmax_forward(dev(z, dt))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32
    report("softmax_forward n=%d%s" % (n, "" if dtype == "f32" else ", %s logits" % dtype), torch.float32, "weights / dw",
           within(got, want, dw * want, "softmax n=%d %s" % (n, dtype)))


@pytest.mark.parametrize("n", SOFTMAX_FWD_LENGTHS)
def test_softmax_forward_is_within_dw(n):
    softmax_forward_within_dw(n, "f32")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n", SOFTMAX_FWD_LENGTHS)
def test_softmax_forward_of_16_bit_logits_is_within_dw(n, dtype):
    softmax_forward_within_dw(n, dtype)


@pytest.mark.parametrize("k", boxes_cases.KERNEL_SIZES)
@pytest.mark.parametrize("L", [1, 5, 16])
def test_instance_weights_forward_is_within_dw(L, k):
    from boxer_amd import ops
    z = cell_rows(L)
    sw, lw, dsw, dlw = eb.instance_weights_reference(z, k, True)
    got_s, got_l = ops.instance_weights_forward(dev(z), k, need_level=True)
    torch.cuda.synchronize()
    route = "instance_weights_forward L=%d k=%d" % (L, k)
    report(route, torch.float32, "spatial / dw", within(got_s, sw, dsw * sw, route + " spatial"))
    report(route, torch.float32, "level / dw", within(got_l, lw, dlw * lw, route + " level"))


# ------------------------------------------------------------------ the box training step from boxes


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("geometry", BOX_GEOMETRIES)
def test_box_backward_from_boxes(geometry, C, dtype):
    """bwd2_boxes_kernel (ops.box_attn_backward_boxes, need_ref_grad) over every flavour: grad_offsets, grad_ref_rows
    and grad_logits, float32 in every storage type, each element within the bound of the float64 model from boxes and
    logits.  Where A + E = 0 the bound is 0: the size gradients of a box of size <= 0, the rows of a window wholly
    outside the map and the angle entries of mode 0 must be exactly zero because the model says so."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    worst, edge, zeros = {}, {}, {n: 0 for n in GRAD_NAMES}
    for flavour in box_cases.FLAVOURS:
        g = bwd_problem(geometry, C, flavour)
        B, S, H, _, L, Lq, P = g["dims"]
        args = box_args(g, dt)
        gout = dev(bwd_upstream(g), dt)
        if geometry == "k4" and not ops.box_backward_boxes_ok(args[0], L, Lq, P):
            with pytest.raises(ValueError):          # no row gather for this type at this C: an error, not a fall-back
                ops.box_attn_backward_boxes(*args, gout, need_ref_grad=True)
            continue
        assert ops.box_backward_boxes_ok(args[0], L, Lq, P), "not eligible: %s %s" % (g["dims"], dt)
        ref = bwd_reference(geometry, C, flavour)
        what = "box backward from boxes: %s C=%d angle=%d D=%d per_head=%d vr=%d" % ((geometry, C) + flavour[0]
                                                                                     + flavour[1:])
        assert ref["edge_share"] <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (what,
                                                                                              100 * ref["edge_share"])
        grads = ops.box_attn_backward_boxes(*args, gout, need_ref_grad=True)
        torch.cuda.synchronize()
        for name, t in zip(GRAD_NAMES, grads):
            assert t.dtype == torch.float32 and tuple(t.shape) == ref[name]["want"].shape, name
            worst[name] = max(worst.get(name, 0.0), eb.hold(t, ref[name], torch.float32, "none", "%s: %s" % (what, name)))
            edge[name] = max(edge.get(name, 0.0), eb.edge_dominated(ref[name]))
            zeros[name] += must_be_zero(ref[name])
    route = "box backward from boxes: %s C=%d [%s storage]" % (geometry, C, dtype)
    for name, w in worst.items():
        report("%s (%d must-be-zero elements)" % (route, zeros[name]), torch.float32, name, w)
    if worst:
        print("%s: share of elements whose bound is more than half edge allowance: %s"
              % (route, ", ".join("%s %.4f" % kv for kv in edge.items())))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("geometry", ["model", "ragged"])
def test_box_backward_rows_offset_by_eight_bytes(geometry, dtype):
    """16-bit ``value`` and ``grad_out`` 8 bytes off a 16-byte boundary: 4 channels a lane instead of 8."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    flavour = ((1, 5), True, True)
    g = bwd_problem(geometry, 32, flavour)
    B, S, H, C, L, Lq, P = g["dims"]
    args = box_args(g, dt, value=offset_by_eight(dev(every_type(g["value"]), dt)))
    gout = offset_by_eight(dev(bwd_upstream(g), dt))
    assert ops.box_backward_boxes_ok(args[0], L, Lq, P), "not eligible at this alignment: %s %s" % (g["dims"], dt)
    ref = bwd_reference(geometry, 32, flavour)
    assert ref["edge_share"] <= eb.EDGE_CAP
    grads = ops.box_attn_backward_boxes(*args, gout, need_ref_grad=True)
    torch.cuda.synchronize()
    for name, t in zip(GRAD_NAMES, grads):
        worst = eb.hold(t, ref[name], torch.float32, "none", "box backward from boxes, rows offset: %s %s" % (geometry,
                                                                                                              name))
        report("box backward from boxes: %s C=32 [%s storage], rows 8 bytes off" % (geometry, dtype), torch.float32,
               name, worst)


# ------------------------------------------------------------------ the backward building blocks on their own
@pytest.mark.parametrize("need_ref_grad", [False, True], ids=["offsets_only", "with_ref_rows"])
@pytest.mark.parametrize("P", GRID_POINTS)
def test_box_grid_backward_is_within_the_bound(P, need_ref_grad):
    """ops.box_grid_backward with float32 random grad_grid as an exact input: the reduction's roundings and the
    rotation allowance are all the bound has.  The share of SINCOS_ABS the device sine and cosine use is printed: the
    largest |sin - float64 sin| is not observable here, so what is printed is the worst err / bound of the rotated
    modes, whose bound is mostly that allowance."""
    from boxer_amd import ops
    worst = {}
    for angle_mode, per_head, with_vr in GRID_FLAVOURS:
        g = grid_problem(P, angle_mode, per_head, with_vr)
        gg = grid_upstream(P, angle_mode, per_head, with_vr)
        ref = eb.grid_backward_reference(g["ref"], g["off"], g["kidx"], g["vr"], angle_mode, gg)
        goff, rows = ops.box_grid_backward(dev(g["ref"]), dev(g["off"]), dev(g["kidx"]),
                                           None if g["vr"] is None else dev(g["vr"]), angle_mode, dev(gg),
                                           need_ref_grad=need_ref_grad)
        torch.cuda.synchronize()
        assert (rows is None) == (not need_ref_grad)
        for name, t in (("grad_offsets", goff), ("grad_ref_rows", rows)):
            if t is None:
                continue
            what = "box_grid_backward P=%d angle=%d per_head=%d vr=%d: %s" % (P, angle_mode, per_head, with_vr, name)
            key = (angle_mode, name)
            worst[key] = max(worst.get(key, 0.0), eb.hold(t, ref[name], torch.float32, "none", what))
    for (angle_mode, name), w in sorted(worst.items()):
        report("box_grid_backward P=%d angle mode %d" % (P, angle_mode), torch.float32, name, w)


def offset_by_four(t):
    flat = torch.zeros(t.numel() + 4, dtype=t.dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0 and t.dtype == torch.float32
    out = flat[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("n", SOFTMAX_BWD_LENGTHS)
@pytest.mark.parametrize("rows", SOFTMAX_BWD_ROWS)
def test_softmax_backward_is_within_the_bound(rows, n, dtype):
    """ops.softmax_backward: ``attn`` is the float64 softmax rounded to float32, an exact input like ``grad_attn``, so
    the bound holds the kernel's own n + 3 roundings and the one rounding to the output's type.  Every dispatch branch:
    the vector kernels (n = 4, 8, 32, 64: 1, 2, 8 and 16 lanes a row), the one-thread-per-row kernels with 16 (n = 1, 3,
    12) and 64 registers (n = 18, 63) -- 12 being a multiple of 4 that is no power of two."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    a, g = softmax_bwd_problem(rows, n)
    got = ops.softmax_backward(dev(a), dev(g), dt)
    torch.cuda.synchronize()
    assert got.dtype == dt
    worst = eb.hold(got, eb.softmax_backward_reference(a, g), dt, "none", "softmax_backward rows=%d n=%d" % (rows, n))
    report("softmax_backward rows=%d n=%d" % (rows, n), dt, "grad_logits", worst)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_softmax_backward_grad_attn_off_a_16_byte_boundary(dtype):
    """n = 16 would take the vector kernel; with ``grad_attn`` 4 bytes off a 16-byte boundary it must take the row
    kernel (a float4 load there would be misaligned) and still hold."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    a, g = softmax_bwd_problem(257, 16)
    got = ops.softmax_backward(dev(a), offset_by_four(dev(g)), dt)
    torch.cuda.synchronize()
    worst = eb.hold(got, eb.softmax_backward_reference(a, g), dt, "none", "softmax_backward, grad_attn 4 bytes off")
    report("softmax_backward rows=257 n=16, grad_attn 4 bytes off", dt, "grad_logits", worst)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("k", boxes_cases.KERNEL_SIZES)
@pytest.mark.parametrize("L", [1, 5, 16])
def test_instance_weights_backward_is_within_the_bound(L, k, dtype):
    """ops.instance_weights_backward against the 2 x 2-logit reduction of the model, exact float32 upstream gradients,
    either of them None; logits (and so their gradient) in the three types -- 16-bit logits are exact inputs."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    z = eb.round_to(cell_rows(L), dt).astype(np.float32)
    gs, gl = cell_upstream(L, k)
    for which, (s, l) in (("both", (gs, gl)), ("spatial only", (gs, None)), ("level only", (None, gl))):
        got = ops.instance_weights_backward(dev(z, dt), None if s is None else dev(s), None if l is None else dev(l))
        torch.cuda.synchronize()
        assert got.dtype == dt
        ref = eb.cell_logits_backward_reference(z, k, s, l)
        worst = eb.hold(got, ref, dt, "none", "instance_weights_backward L=%d k=%d %s" % (L, k, which))
        report("instance_weights_backward L=%d k=%d %s" % (L, k, which), dt, "grad_logits", worst)


def test_device_sine_and_cosine_are_within_the_allowance():
    """How much of SINCOS_ABS the device uses, read off ops.box_grid_backward exactly: angle mode 2 (theta is an input),
    a reference window of size 8 with offsets 0, one point with kidx (1/2, 1/2) and grad_grid (1, 0), no valid ratios:
    grad_offsets[2] = kx (1 cos + 0 sin) 8 / 8 = cos / 2 and grad_offsets[3] = ky (0 cos - 1 sin) = -sin / 2 without a
    rounding (products with 0, 1 and powers of two).  Angles: the range the cases reach, 23 + 77 / 16 turns = 175 rad."""
    from boxer_amd import ops
    rng = np.random.default_rng(4)
    N = 4096
    theta = np.concatenate([rng.uniform(-180.0, 180.0, N - 8), [0.0, 23.0, -7.25, 174.75, 0.5 * np.pi, np.pi, 1e-3, -3.0]])
    ref = np.zeros((1, N, 5), np.float32)
    ref[..., :4], ref[..., 4] = (0.5, 0.5, 8.0, 8.0), theta
    kidx = np.zeros((4, 2), np.float32)
    kidx[0] = 0.5
    gg = np.zeros((1, N, 1, 1, 4, 2), np.float32)
    gg[..., 0, 0] = 1.0
    goff, _ = ops.box_grid_backward(dev(ref), dev(np.zeros((1, N, 1, 1, 4), np.float32)), dev(kidx), None, 2, dev(gg))
    torch.cuda.synchronize()
    goff = eb.f64(goff).reshape(N, 4)
    t = ref[0, :, 4].astype(np.float64)
    err = np.maximum(np.abs(2 * goff[:, 2] - np.cos(t)), np.abs(-2 * goff[:, 3] - np.sin(t)))
    at = int(np.argmax(err))
    print("error-bound | device sincosf, %d angles in [-180, 180] rad | float32 | |sin|, |cos| error / SINCOS_ABS | %.3f "
          "(%.3g = %.2f ulp at 1.0, at theta = %.9g)" % (N, err[at] / eb.SINCOS_ABS, err[at], err[at] * 2.0 ** 23, t[at]))
    assert err[at] <= eb.SINCOS_ABS, "the device sine or cosine is off by %.3g at theta = %.9g" % (err[at], t[at])
