"""GPU tests (``-m gpu``) of the wave-per-pair forward kernel's BOX flavour (the mask model at inference: box
attention with few queries on a 14 x 14 grid): reference goldens, seeded problems against the fp64
C oracle on the rounded inputs, the parity of the two kernel families (option key 22), the training forward with
the backward's count riders, and the module that runs it.

Tolerances are the project's own: ``|got - want| <= tol * (max(1, rms(want)) + |want|)`` with
tol = 1e-4 for float32 and 1e-2 for 16-bit storage.  Every case first asserts through ``ops.forward_route`` that
the family it means to test is the one the library launches (key 22 is forced on where the default is off)."""
import functools

import numpy as np
import pytest
import torch

import golden_io
from oracle import boxattn_oracle as oc
from boxes_cases import module_problem, tables
from compare_rules import check_scaled as check, rounded, tol_of
from route_vocab import DTYPES, GATHER, WIDE, WIDE_OFF, WIDE_ON, dev, take_family

pytestmark = pytest.mark.gpu


def box_forward(g, dtype, family=WIDE, value=None):
    """ops.box_attn_forward on the problem `g` (numpy, float64) in storage `dtype`, on `family`."""
    from boxer_amd import ops
    value = dev(g["value"], dtype) if value is None else value
    loc, attn = dev(g["loc"], torch.float32), dev(g["attn"], torch.float32)
    shapes, lsi = dev(g["shapes"]), dev(g["lsi"])
    take_family(value, loc, shapes, lsi, family)
    out = ops.box_attn_forward(value, shapes, lsi, loc, attn, 64)
    torch.cuda.synchronize()
    assert out.dtype == dtype
    return out


def oracle_out(g, dtype):
    return oc.box_attn_forward(rounded(g["value"], dtype), g["shapes"], g["lsi"], g["loc"], g["attn"])


# ------------------------------------------------------------------ 1. reference goldens
def golden_as_box(name):
    """An instance-attention fixture read as box attention: `out` is the sum over the spatial weights alone."""
    g = golden_io.load(name)
    B, Lq, H, L, P = g["loc"].shape[:5]
    # (locations and weights are float32 on the device for every storage type: the oracle gets what the GPU gets)
    g["loc"] = rounded(g["loc"], torch.float32)
    g["attn"] = rounded(g["spatial_w"].reshape(B, Lq, H, L, P), torch.float32)
    return g


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", ["G6_inst_ms14", "G6_inst_ms4"])
def test_reference_goldens(name, dtype):
    """G6_inst_ms14: 6 pairs of 196 points, four waves share a pair; G6_inst_ms4: head = XCD placement, one step.
    float32 against the reference's own output, 16-bit storage against the C oracle on the rounded inputs."""
    g = golden_as_box(name)
    dt = DTYPES[dtype]
    out = box_forward(g, dt)
    want = g["out"] if dt == torch.float32 else oracle_out(g, dt)
    check(out, want, tol_of(dt), "%s %s out" % (name, dtype))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_control_with_four_points_takes_the_row_gather(dtype):
    g = golden_as_box("G3_inst_C32")
    dt = DTYPES[dtype]
    out = box_forward(g, dt, family=GATHER)
    check(out, g["out"] if dt == torch.float32 else oracle_out(g, dt), tol_of(dt), "G3_inst_C32 %s out" % dtype)


# ------------------------------------------------------------------ 2. seeded, against the C oracle
# five levels: more than a 4-lane group has lanes (the l0 > 0 reload); 30 pairs: a last workgroup with dead waves
GEOMETRY = {"five_levels": dict(levels=[(5, 7), (3, 4), (2, 2), (1, 3), (1, 1)], B=2, Lq=5, H=3),
            "head_xcd": dict(levels=[(9, 11), (4, 5)], B=2, Lq=4, H=8)}
# one, two and four waves a pair for both lane-group widths; 17 and 100 leave a ragged last step
POINTS = [16, 17, 36, 64, 100, 196]


@functools.lru_cache(maxsize=None)
def seeded(geometry, C, P):
    geo = GEOMETRY[geometry]
    shapes, lsi, S = tables(geo["levels"])
    B, Lq, H, L = geo["B"], geo["Lq"], geo["H"], len(geo["levels"])
    rng = np.random.default_rng(1000 * C + P + (7 if geometry == "head_xcd" else 0))
    a = rng.random((B, Lq, H, L, P))
    a[rng.random(a.shape) < 0.1] = 0.0                                   # some exact zeros, not normalised
    return dict(shapes=shapes, lsi=lsi, value=rng.standard_normal((B, S, H, C)),
                loc=rounded(rng.uniform(-0.2, 1.2, (B, Lq, H, L, P, 2)), torch.float32),   # points outside included
                attn=rounded(a, torch.float32))


@functools.lru_cache(maxsize=None)
def seeded_want(geometry, C, P, dtype):
    return oracle_out(seeded(geometry, C, P), DTYPES[dtype])


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("P", POINTS)
@pytest.mark.parametrize("C", [16, 32, 64])
@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
def test_seeded_against_oracle(geometry, C, P, dtype):
    dt = DTYPES[dtype]
    out = box_forward(seeded(geometry, C, P), dt)
    check(out, seeded_want(geometry, C, P, dtype), tol_of(dt), "%s C=%d P=%d %s" % (geometry, C, P, dtype))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("P", [17, 196])
def test_value_rows_offset_by_eight_bytes(P, dtype):
    """A 16-bit `value` 8 bytes off a 16-byte boundary: 4 channels a lane instead of 8, the same family."""
    dt = DTYPES[dtype]
    g = seeded("five_levels", 32, P)
    flat = torch.zeros(g["value"].size + 4, dtype=dt, device="cuda")
    value = flat[4:].view(g["value"].shape)
    value.copy_(dev(g["value"], dt))
    assert value.data_ptr() % 16 == 8 and value.is_contiguous()
    out = box_forward(g, dt, value=value)
    check(out, seeded_want("five_levels", 32, P, dtype), tol_of(dt), "offset value P=%d %s" % (P, dtype))


# ------------------------------------------------------------------ 3. the two families against each other
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("P", [36, 196])
def test_two_families_agree_and_the_wide_one_is_reproducible(P, dtype):
    from boxer_amd import _lib
    dt = DTYPES[dtype]
    g = seeded("head_xcd", 32, P)
    wide = box_forward(g, dt)
    again = box_forward(g, dt)
    assert torch.equal(wide, again), "two runs of the wave-per-pair kernel differ (it has no atomics)"
    _lib.set_option("wide_box", WIDE_OFF)
    rows = box_forward(g, dt, family=GATHER)
    check(wide, rows.double().cpu().numpy(), tol_of(dt), "wide against row gather P=%d %s" % (P, dtype))


# ------------------------------------------------------------------ 4. training forward: the count riders ride along
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_training_forward_hands_over_a_plan(dtype):
    """B=2, Lq=10, H=8, C=32, P=196 on the G6 levels with the two-pass binning (key 15 = 4: the backward's count pass
    and scans ride in the forward's launch -- here the wide box kernel's): the plan has a buffer, `out` matches, and
    the backward that takes the plan gives the gradients of the plan-less backward and of the oracle."""
    from boxer_amd import _lib, ops
    dt = DTYPES[dtype]
    tol = tol_of(dt)
    g6 = golden_io.load("G6_inst_ms4")
    shapes, lsi, S = tables(g6["shapes"])
    rng = np.random.default_rng(5)
    B, Lq, H, C, L, P = 2, 10, 8, 32, 4, 196
    a = rng.random((B, Lq, H, L, P))
    g = dict(shapes=shapes, lsi=lsi, value=rounded(rng.standard_normal((B, S, H, C)), dt),
             loc=rounded(rng.uniform(-0.2, 1.2, (B, Lq, H, L, P, 2)), torch.float32),
             attn=rounded(a / a.sum((-1, -2), keepdims=True), torch.float32),
             grad_out=rounded(rng.standard_normal((B, Lq, H * C)), dt))
    _lib.set_option("riders", 4)
    value = dev(g["value"], dt).requires_grad_()
    loc, attn = dev(g["loc"], torch.float32), dev(g["attn"], torch.float32)
    tsh, tls, gout = dev(shapes), dev(lsi), dev(g["grad_out"], dt)
    take_family(value, loc, tsh, tls, WIDE)
    out, plan = ops.box_attn_forward_train(value, tsh, tls, loc, attn, 64)
    assert plan is not None and plan.buf is not None
    with_plan = ops.box_attn_backward(value.detach(), tsh, tls, loc, attn, gout, 64, plan=plan)
    without = ops.box_attn_backward(value.detach(), tsh, tls, loc, attn, gout, 64)
    torch.cuda.synchronize()
    args = (g["value"], shapes, lsi, g["loc"], g["attn"])
    check(out, oc.box_attn_forward(*args), tol, "train forward %s out" % dtype)
    pix = g["loc"] * shapes.astype(np.float64)[None, None, None, :, None, ::-1] - 0.5
    off_edge = ~(np.abs(pix - np.round(pix)) < 1e-4).any(-1, keepdims=True)
    for name, a_, b_, w in zip(("grad_value", "grad_loc", "grad_attn"), with_plan, without,
                               oc.box_attn_backward(*args, g["grad_out"])):
        t = tol if name == "grad_value" else 1e-4                        # (point gradients are float32)
        keep = off_edge if name == "grad_loc" else 1.0
        w = np.asarray(w).reshape(a_.shape)
        check(a_ * dev(np.broadcast_to(keep, w.shape) * 1.0, a_.dtype), w * keep, t, "%s %s with plan" % (name, dtype))
        check(b_ * dev(np.broadcast_to(keep, w.shape) * 1.0, b_.dtype), w * keep, t, "%s %s plan-less" % (name, dtype))


# ------------------------------------------------------------------ 5. the module and the compiled operator


@pytest.mark.parametrize("fused_pointwise", [False, True], ids=["torch_pointwise", "fused_pointwise"])
@pytest.mark.parametrize("mode", ["f32", "f16_autocast"])
def test_module_inference_equals_the_training_output(mode, fused_pointwise):
    """InstanceAttention(256, 4, 8, 14): `out` with inferencing set is the `output` of the training branch -- the
    same sum, once by the wide box kernel and once by the wide instance kernel."""
    from boxer_amd import _lib
    m, args, dims, g6 = module_problem()
    f16 = mode == "f16_autocast"
    m.native_f16, m.fused_pointwise = f16, fused_pointwise
    elem = 2 if f16 else 4
    if _lib.fwd_route(elem, 0, 16, dims, g6["shapes"], g6["lsi"]) != WIDE:
        _lib.set_option("wide_box", WIDE_ON)
    assert _lib.fwd_route(elem, 0, 16, dims, g6["shapes"], g6["lsi"]) == WIDE
    assert _lib.fwd_route(elem, 1, 16, dims) == WIDE
    outs = {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=f16):
        for inferencing in (True, False):
            m.inferencing = inferencing
            outs[inferencing] = m(*args)[0]
    torch.cuda.synchronize()
    assert outs[True].shape == outs[False].shape
    check(outs[True], outs[False].double().cpu().numpy(), 1e-2 if f16 else 1e-4, "module out %s" % mode)


def test_compiled_module_takes_the_route():
    """boxer_amd._ext (the compiled operator module) reaches the same entry point: box_attn_forward at the
    G6_inst_ms14 shape, against ops and the reference's output."""
    from boxer_amd import _ext, ops
    g = golden_as_box("G6_inst_ms14")
    value, loc, attn = dev(g["value"], torch.float32), dev(g["loc"], torch.float32), dev(g["attn"], torch.float32)
    shapes, lsi = dev(g["shapes"]), dev(g["lsi"])
    take_family(value, loc, shapes, lsi, WIDE)
    a = _ext.load().box_attn_forward(value, shapes, lsi, loc, attn, 64)
    b = ops.box_attn_forward(value, shapes, lsi, loc, attn, 64)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    check(a, g["out"], 1e-4, "compiled module out")
