"""GPU tests (``-m gpu``) of box attention's inference forward from boxes and L*P logits in one launch
(``ops.box_attn_forward_boxes``, include/boxattn.h boxattn_fwd_boxes_*) and of the module flag
``fused_boxes`` that takes it in BoxAttention / Box3dAttention.

Every seeded case holds the one call against two expectations, at the project's own tolerances (DESIGN.md 5:
``|got - want| <= tol * (max(1, rms(want)) + |want|)``, tol 1e-4 for float32 and 1e-2 for 16-bit storage -- the harness
of test_gpu_wide_box_forward.py):
  (a) the three launches of this same build -- ``ops.box_grid_forward`` -> ``ops.softmax_forward`` ->
      ``ops.box_attn_forward``, route asserted;
  (b) the float64 C oracle fed with the locations and weights those two GPU kernels produced and with ``value``
      rounded to the storage type.
How many elements differ BITWISE from (a) is printed per case (the locations come from shared device functions; the
softmax sums in another order, and the window-staged forward in yet another); it is reported, not asserted."""

import pytest
import torch

from oracle import boxattn_oracle as oc
from boxes_cases import (BOX_GEOMETRY as GEOMETRY, FLAVOURS, GOLDENS, box_boxes_problem as problem,
                         box_golden_module as golden_module, box_kernel_indices as kernel_indices, golden_err, hold,
                         tables)
from compare_rules import check_scaled as check, rounded
from route_vocab import DTYPES, GATHER, STAGED, dev

pytestmark = pytest.mark.gpu


def three_route(geometry, C):
    """The family the three launches' sampling call must take."""
    return STAGED if geometry == "encoder" and C == 32 else GATHER


def run_case(g, dt, route, value=None):
    """-> (got, three_launch, oracle): got and three_launch tensors, oracle numpy."""
    from boxer_amd import ops
    B, S, H, C, L, Lq, P = g["dims"]
    value = dev(g["value"], dt) if value is None else value
    shapes, lsi = dev(g["shapes"]), dev(g["lsi"])
    ref, off, logits, kidx = dev(g["ref"]), dev(g["off"]), dev(g["logits"]), kernel_indices(P)
    vr = None if g["vr"] is None else dev(g["vr"])
    assert ops.box_forward_boxes_ok(value, L, Lq, P), "not eligible: %s %s" % (g["dims"], dt)
    got = ops.box_attn_forward_boxes(value, shapes, lsi, ref, off, kidx, vr, logits, g["angle_mode"])
    # (a) the three launches of this build
    grid = ops.box_grid_forward(ref, off, kidx, vr, g["angle_mode"])
    attn = ops.softmax_forward(logits).view(B, Lq, H, L, P)
    assert (1 + off[..., 2:4] / 8 <= 0).any() and (grid < 0).any() and (grid > 1).any()   # relu hit, outside both ways
    taken = ops.forward_route(value, grid, shapes, lsi)
    assert taken == route, "the three launches take route %d, wanted %d" % (taken, route)
    three = ops.box_attn_forward(value, shapes, lsi, grid, attn, 64)
    torch.cuda.synchronize()
    # (b) the float64 oracle on what the two GPU kernels produced
    want = oc.box_attn_forward(rounded(g["value"], dt), g["shapes"], g["lsi"], grid.double().cpu().numpy(),
                               attn.double().cpu().numpy())
    return got, three, want


def all_flavours(geometry, C, dtype):
    from boxer_amd import ops
    dt = DTYPES[dtype]
    geo = GEOMETRY[geometry]
    B, L, Lq, H, P = geo["B"], len(geo["levels"]), geo["Lq"], geo["H"], geo["P"]
    S = tables(geo["levels"])[2]
    if geometry == "k4" and not ops.box_forward_boxes_ok(torch.empty(B, S, H, C, dtype=dt, device="cuda"), L, Lq, P):
        pytest.skip("k4: no row gather for %s at C = %d (boxattn_fwd_boxes_ok answers 0)" % (dtype, C))
    for (angle_mode, ref_dim), per_head, with_vr in FLAVOURS:
        g = problem(geometry, C, angle_mode, ref_dim, per_head, with_vr)
        what = "%s C=%d %s angle=%d D=%d per_head=%d vr=%d" % (geometry, C, dtype, angle_mode, ref_dim, per_head,
                                                                 with_vr)
        hold(*run_case(g, dt, three_route(geometry, C)), dt, what)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("C", [16, 32, 64])
@pytest.mark.parametrize("geometry", ["model", "ragged", "one_level", "odd_k", "sixteen_levels", "k4", "encoder"])
def test_seeded_matrix(geometry, C, dtype):
    """Angle modes 0, 1 (reference windows of 5 and 7 values) and 2 x reference windows shared and per head x
    valid_ratios None and given."""
    all_flavours(geometry, C, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("geometry", ["mid", "mid_h3"])
def test_mid_size(geometry, dtype):
    """C2 levels, 300 queries, B 2, C 32, angle mode 0: 75 and more workgroups."""
    dt = DTYPES[dtype]
    g = problem(geometry, 32, 0, 4, False, True)
    hold(*run_case(g, dt, GATHER), dt, "%s %s" % (geometry, dtype))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("geometry", ["model", "ragged"])
def test_value_rows_offset_by_eight_bytes(geometry, dtype):
    """A 16-bit `value` 8 bytes off a 16-byte boundary: 4 channels a lane instead of 8, the same family."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    g = problem(geometry, 32, 1, 5, True, True)
    flat = torch.zeros(g["value"].size + 4, dtype=dt, device="cuda")
    value = flat[4:].view(g["value"].shape)
    value.copy_(dev(g["value"], dt))
    assert value.data_ptr() % 16 == 8 and value.is_contiguous()
    B, S, H, C, L, Lq, P = g["dims"]
    assert ops.box_forward_boxes_ok(value, L, Lq, P)
    hold(*run_case(g, dt, GATHER, value=value), dt, "offset value %s %s" % (geometry, dtype))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_two_runs_are_equal(dtype):
    from boxer_amd import ops
    dt = DTYPES[dtype]
    g = problem("model", 32, 1, 5, False, True)
    B, S, H, C, L, Lq, P = g["dims"]
    args = (dev(g["value"], dt), dev(g["shapes"]), dev(g["lsi"]), dev(g["ref"]), dev(g["off"]), kernel_indices(P),
            dev(g["vr"]), dev(g["logits"]), 1)
    first = ops.box_attn_forward_boxes(*args)
    again = ops.box_attn_forward_boxes(*args)
    torch.cuda.synchronize()
    assert torch.equal(first, again), "the kernel has no atomics"


def test_ops_refuse_what_has_no_kernel():
    """ValueError before any launch: the launch spy sees nothing."""
    from boxer_amd import ops

    def inputs(levels, B, Lq, H, C, P, V=4, D=4, dt=torch.float32):
        shapes, lsi, S = tables(levels)
        L = len(levels)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
        return [torch.zeros(B, S, H, C, dtype=dt, device="cuda"), dev(shapes), dev(lsi), z(B, Lq, D),
                z(B, Lq, H, L, V), z(P, 2), None, z(B, Lq, H, L * P)]

    launches = []
    orig = ops._grid_call
    ops._grid_call = lambda *a, **k: launches.append(a[0]) or orig(*a, **k)
    try:
        cases = {"L P = 65": (inputs([(6, 5)], 1, 3, 2, 32, 65), 0),
                 "L = 17": (inputs([(1, 1)] * 17, 1, 3, 2, 32, 1), 0),
                 "float64": (inputs([(6, 5)], 1, 3, 2, 32, 4, dt=torch.float64), 0),
                 "C = 8": (inputs([(6, 5)], 1, 3, 2, 8, 4), 0),
                 "V = 4 with angle_mode 1": (inputs([(6, 5)], 1, 3, 2, 32, 4, V=4, D=5), 1),
                 "V = 5 with angle_mode 0": (inputs([(6, 5)], 1, 3, 2, 32, 4, V=5, D=5), 0),
                 "ref_dim 4 with angle_mode 2": (inputs([(6, 5)], 1, 3, 2, 32, 4), 2)}
        strided = inputs([(6, 5)], 1, 3, 2, 32, 4)
        strided[0] = torch.zeros(1, 30, 2, 64, device="cuda")[..., ::2]
        assert not strided[0].is_contiguous()
        cases["value not contiguous"] = (strided, 0)
        for what, (args, mode) in cases.items():
            with pytest.raises(ValueError):
                ops.box_attn_forward_boxes(*args, mode)
            assert not launches, what
        ok = inputs([(6, 5)], 1, 3, 2, 32, 4)                   # (the control: the same arguments, accepted)
        out = ops.box_attn_forward_boxes(*ok, 0)
        torch.cuda.synchronize()
        assert launches == ["boxattn_fwd_boxes_f32"] and out.shape == (1, 3, 64) and not out.any()
    finally:
        ops._grid_call = orig


# ------------------------------------------------------------------ the modules


def golden_out(g):
    return g["out0"] if "out0" in g else g["out"]


class CallCounter:
    """Counts the calls of ops.box_attn_forward_boxes while it is active."""
    def __enter__(self):
        from boxer_amd import ops
        self.calls, self.orig = [], ops.box_attn_forward_boxes
        ops.box_attn_forward_boxes = lambda *a, **k: self.calls.append(1) or self.orig(*a, **k)
        return self

    def __exit__(self, *exc):
        from boxer_amd import ops
        ops.box_attn_forward_boxes = self.orig


@pytest.mark.parametrize("native_bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_module_reference_golden(name, native_bf16):
    """Under no_grad with the flag: the output agrees with the reference's at the golden's tolerance and with the
    flag-off module, through ONE call of ops.box_attn_forward_boxes -- where that has its kernel: the G9 goldens (32
    channels a head; asserted eligible).  The G7 goldens have 8 channels a head, for which the library has generic
    kernels only: there the flag must fall through to today's code without a call.  The flag-off module never calls."""
    from boxer_amd import ops
    m, g, args = golden_module(name, native_bf16)
    dt = torch.bfloat16 if native_bf16 else torch.float32
    B, S = args[1].shape[:2]
    eligible = ops.box_forward_boxes_ok(torch.empty(B, S, m.num_head, m.head_dim, dtype=dt, device="cuda"),
                                        m.num_level, args[0].shape[1], m.num_point)
    assert eligible == name.startswith("G9"), "%s: eligible = %s" % (name, eligible)
    outs, counts = {}, {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=native_bf16):
        for flag in (True, False):
            m.fused_boxes = flag
            with CallCounter() as counter:
                outs[flag] = m(*args)
            counts[flag] = len(counter.calls)
    torch.cuda.synchronize()
    assert counts[False] == 0, "the flag-off module called ops.box_attn_forward_boxes"
    assert counts[True] == (1 if eligible else 0), "the flag took %d calls of the one-launch path" % counts[True]
    if eligible:
        assert outs[True][1] == ()
    assert outs[True][0].shape == outs[False][0].shape and outs[True][0].dtype == outs[False][0].dtype
    tol_g = GOLDENS[name][4][1 if native_bf16 else 0]
    e = golden_err(outs[True][0], golden_out(g))
    print("%s bf16=%d: %.3e against the golden (tol %.0e)" % (name, native_bf16, e, tol_g))
    assert e <= tol_g
    check(outs[True][0], outs[False][0].double().cpu().numpy(), 1e-2 if native_bf16 else 1e-4,
          "%s bf16=%d flag on against flag off" % (name, native_bf16))


def test_module_with_grad_runs_todays_code():
    """Flag on, grad enabled: no call of the one-launch path, the usual weights as second element, and the output and
    every parameter gradient bitwise those of the flag-off module."""
    m, g, args = golden_module("G9_module_box_dec")
    results = {}
    for flag in (True, False):
        m.fused_boxes = flag
        m.zero_grad()
        with CallCounter() as counter:
            out, weights = m(*args)
            out.square().sum().backward()
        assert not counter.calls, "grad mode took the one-launch path"
        assert isinstance(weights, torch.Tensor) and weights.shape[-2:] == (2, 2)
        results[flag] = [out.detach().clone()] + [p.grad.clone() for p in m.parameters()]
    torch.cuda.synchronize()
    names = ["out"] + [k for k, _ in m.named_parameters()]
    for what, a, b in zip(names, results[True], results[False]):
        assert torch.equal(a, b), "%s differs between flag on and flag off" % what
