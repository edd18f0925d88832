"""GPU: grad_value of 16-bit instance attention summed on the matrix cores (boxattn_set_option(23, 2): the INST
flavour of binned_accumulate_tr_kernel) against the float64 oracle and against the VALU list walk (23 = 1, the route
the library took before the flavour existed) on the same inputs.

Per shape and storage type: both routes pass the suite's 16-bit comparison against the oracle; the new route's
largest error is at most TWICE the VALU route's (both are dominated by the one rounding to the storage type; the factor
leaves room for the 2^-17 weight split and the summation order, nothing more); the point gradients of the two routes
are bit-identical (the same kernel produced them).  Inputs: locations uniform in [-0.2, 1.2], positive row-normalised
weights, N(0, 1) gradients rounded to the storage type before the oracle sees them."""
import numpy as np
import pytest
import torch

import error_bounds as eb
from oracle import boxattn_oracle as oc
from compare_rules import check_f16, close_parity
from point_cases import LEVELS_A, SHAPE_A, instance_problem as problem
from route_vocab import BF16, F16, dev

pytestmark = pytest.mark.gpu

DTYPES = [BF16, F16]
IDS = ["bf16", "f16"]
OPT_INST_ACC16, OPT_BIN_CHUNK = 23, 10
ROUTE_VALU, ROUTE_TR = 1, 2


@pytest.fixture(autouse=True)
def _reset_switches():
    from boxer_amd import _lib
    yield
    _lib.set_variant(0)
    lib = _lib.load()
    lib.boxattn_set_option(OPT_INST_ACC16, 0)
    lib.boxattn_set_option(OPT_BIN_CHUNK, 0)


def close16(got, want, dtype, what):
    """The suite's 16-bit comparison: bf16 by compare_rules.close_parity at the bf16 tolerance, f16 by compare_rules.check_f16
    (parity.close has no f16 entry; that check is the f16 suite's own, at 1e-3)."""
    if dtype == BF16:
        close_parity(got, want, BF16, what)
    else:
        assert got.dtype == F16
        check_f16(got, want, what)


def oracle_backward(g):
    return oc.instance_attn_backward(g["value"], g["shapes"], g["lsi"], g["loc"], g["spatial_w"], g["level_w"],
                                     g["grad_out"], g["grad_mask"])


def tensors(g, dtype, mask_offset_bytes=0):
    t = dict(value=dev(g["value"], dtype), shapes=dev(g["shapes"]), lsi=dev(g["lsi"]),
             loc=dev(g["loc"], torch.float32), sw=dev(g["spatial_w"], torch.float32),
             lw=dev(g["level_w"], torch.float32), gout=dev(g["grad_out"], dtype))
    gm = dev(g["grad_mask"], dtype)
    if mask_offset_bytes:          # the same numbers as a view that starts inside its allocation
        n = mask_offset_bytes // 2
        buf = torch.empty(gm.numel() + n, dtype=dtype, device="cuda")
        buf[n:].copy_(gm.reshape(-1))
        gm = buf[n:].view(gm.shape)
        assert gm.data_ptr() % 16 == mask_offset_bytes % 16
    t["gmask"] = gm
    return t


def set_route(route):
    from boxer_amd import _lib
    return _lib.load().boxattn_set_option(OPT_INST_ACC16, route)


def query(g, elem=2, instance=1):
    from boxer_amd import _lib
    return _lib.bwd_accumulate_kind(elem, instance, g["dims"])


def backward(t, route, want=3, expect=None, g=None):
    """ops.instance_attn_backward under key 23 = ``route`` (restored), the binned backward required."""
    from boxer_amd import _lib, ops
    old = set_route(route)
    try:
        if expect is not None:
            assert query(g) == expect
        _lib.set_variant(3)
        grads = ops.instance_attn_backward(t["value"], t["shapes"], t["lsi"], t["loc"], t["sw"], t["lw"], t["gout"],
                                           t["gmask"], 64, want=want)
        torch.cuda.synchronize()
    finally:
        _lib.set_variant(0)
        set_route(old)
    return grads


def planned_backward(t, g, dtype):
    """Training forward, then the backward with its plan, under the CURRENT switches (a switch set in between would
    age the plan: its key carries the option epoch).  The plan is checked to be the one the backward will accept."""
    from boxer_amd import ops
    _, plan = ops.instance_attn_forward_train(t["value"], t["shapes"], t["lsi"], t["loc"], t["sw"], t["lw"], 64)
    assert plan is not None and plan.buf is not None
    assert plan.key == ops._plan_key(g["dims"], t["loc"], (t["sw"], t["lw"]), dtype)
    grads = ops.instance_attn_backward(t["value"], t["shapes"], t["lsi"], t["loc"], t["sw"], t["lw"], t["gout"],
                                       t["gmask"], 64, plan=plan)
    torch.cuda.synchronize()
    return grads


def max_err(got, want):
    return float(np.abs(got.detach().double().cpu().numpy() - np.asarray(want)).max())


def compare_routes(g, dtype, what, t=None, want=None):
    """Checks 1-3 of a shape: -> (grads of the new route, grads of the VALU route, the oracle's gradients)."""
    from boxer_amd import _lib
    t = tensors(g, dtype) if t is None else t
    want = oracle_backward(g) if want is None else want
    new = backward(t, ROUTE_TR, expect=_lib.ACC_TR, g=g)
    old = backward(t, ROUTE_VALU, expect=_lib.ACC_VALU, g=g)
    for name, grads in (("matrix cores", new), ("VALU", old)):
        assert grads[0].dtype == dtype
        close16(grads[0], want[0], dtype, "%s: grad_value (%s)" % (what, name))
    e_new, e_old = max_err(new[0], want[0]), max_err(old[0], want[0])
    print("%s %s: max |err| matrix cores %.4e, VALU %.4e, ratio %.3f" % (
        what, str(dtype)[6:], e_new, e_old, e_new / e_old if e_old else float("nan")))
    assert e_new <= 2.0 * e_old, (what, e_new, e_old)
    for a, b, name in zip(new[1:], old[1:], ("grad_loc", "grad_spatial", "grad_level")):
        assert torch.equal(a, b), (what, name)
    # every element inside the bound of tests/error_bounds.py on both routes: the matrix cores with the
    # weights in two 16-bit terms, the VALU walk with float32 weights (the uniform locations of ``problem`` keep the
    # cell-edge share of grad_loc under its cap: asserted)
    if "_ref" not in g:
        g["_ref"] = eb.instance_reference(g["value"], g["shapes"], g["lsi"], g["loc"], g["spatial_w"], g["level_w"],
                                          g["grad_out"], g["grad_mask"])
    names = ("grad_value", "grad_loc", "grad_spatial", "grad_level")
    for route, grads, split in (("matrix cores", new, eb.store_name(dtype)), ("VALU", old, "none")):
        eb.hold_all(dict(zip(names, grads)), g["_ref"], dtype, split, "%s (%s)" % (what, route))
    return new, old, want


# ------------------------------------------------------------------ the shapes
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_prefetch_pipeline_partial_blocks_one_row_level(dtype):
    """A: ~400 records in each of level 0's twelve 8 x 4 blocks (four or more rounds of 64: the whole prefetch
    pipeline), partial blocks on the 7 x 5 map, a one-row level."""
    compare_routes(problem(dtype=dtype, **SHAPE_A), dtype, "A")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_b_packed_point_ids_at_14_by_14(dtype):
    """B: L P = 588 -- point ids packed with 10 bits, a_l looked up by a stride that is no power of two."""
    compare_routes(problem(LEVELS_A, 2, 3, 32, 12, 14, dtype, seed=6), dtype, "B")


@pytest.mark.parametrize("C", [16, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_c_other_channel_counts(dtype, C):
    compare_routes(problem(LEVELS_A, 2, 3, C, 64, 4, dtype, seed=7), dtype, "C (C=%d)" % C)


@pytest.mark.parametrize("chunk", [64, 192])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_d_chunked_blocks(dtype, chunk):
    """D: key 10 cuts the heavy blocks into chunks -- float32 partial tiles and chunk_finish."""
    from boxer_amd import _lib
    _lib.load().boxattn_set_option(OPT_BIN_CHUNK, chunk)
    compare_routes(problem(dtype=dtype, **SHAPE_A), dtype, "D (chunk %d)" % chunk)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_e_every_location_outside(dtype):
    g = problem(dtype=dtype, loc_range=(1.5, 2.5), **SHAPE_A)
    from boxer_amd import _lib
    t = tensors(g, dtype)
    for route, kind in ((ROUTE_TR, _lib.ACC_TR), (ROUTE_VALU, _lib.ACC_VALU)):
        gv = backward(t, route, expect=kind, g=g)[0]
        assert gv.dtype == dtype and not gv.any().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_e2_every_location_inside_one_block(dtype):
    """E': one heavy item (all 4 800 level-0 points of a slice in that level's first block), every other block empty."""
    g = problem(dtype=dtype, loc_range=(0.03, 0.12), **SHAPE_A)
    g["loc"][:, :, :, 1:] += 2.0          # the other levels: outside
    compare_routes(g, dtype, "E'")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f_sparse_map(dtype):
    """F: 1 056 blocks with under two expected records each: the zero workers run in front of the new kernel."""
    compare_routes(problem([(128, 264)], 1, 2, 32, 8, 4, dtype, seed=8), dtype, "F")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_g_nine_points(dtype):
    """G: P = 9 -- the wide fill without its four-points-per-thread flavour."""
    compare_routes(problem(LEVELS_A, 2, 3, 32, 100, 3, dtype, seed=9), dtype, "G")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_h_grad_mask_view_8_bytes_into_its_allocation(dtype):
    """H: the matrix-core route reads grad_mask rows 16 bytes at a time; a view that is only 8-byte aligned is no error,
    the call takes the VALU walk -- with the plan of a training forward (made for the other record order) too."""
    from boxer_amd import _lib
    g = problem(dtype=dtype, **SHAPE_A)
    want = oracle_backward(g)
    t = tensors(g, dtype, mask_offset_bytes=8)
    assert t["gmask"].data_ptr() % 16 == 8
    new = backward(t, ROUTE_TR, expect=_lib.ACC_TR, g=g)            # (the query sees dimensions, not addresses)
    old = backward(t, ROUTE_VALU, expect=_lib.ACC_VALU, g=g)
    set_route(ROUTE_TR)
    _lib.set_variant(3)
    planned = planned_backward(t, g, dtype)
    for grads, name in ((new, "self-planned"), (old, "key 23 = 1"), (planned, "forward's plan")):
        close16(grads[0], want[0], dtype, "H: grad_value (%s)" % name)
        for a, b in zip(grads[1:], old[1:]):
            assert torch.equal(a, b), name
    e_new, e_old = max_err(new[0], want[0]), max_err(old[0], want[0])
    assert e_new <= 2.0 * e_old and max_err(planned[0], want[0]) <= 2.0 * e_old


# ------------------------------------------------------------------ shape A through every entry
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_through_every_entry(dtype):
    from boxer_amd import _ext, _lib
    from boxer_amd import InstanceAttnBF16Function, InstanceAttnF16Function
    g = problem(dtype=dtype, **SHAPE_A)
    t = tensors(g, dtype)
    new, old, want = compare_routes(g, dtype, "A (self-planned)", t=t)
    e_old = max_err(old[0], want[0])

    def value_ok(gv, what):
        close16(gv, want[0], dtype, "A: grad_value (%s)" % what)
        assert max_err(gv, want[0]) <= 2.0 * e_old, what

    old_key = set_route(ROUTE_TR)
    try:
        assert query(g) == _lib.ACC_TR
        # the training forward's plan: count and scans ride in the forward, the fill in the point gradients
        _lib.set_variant(3)
        grads = planned_backward(t, g, dtype)
        _lib.set_variant(0)
        value_ok(grads[0], "forward's plan")
        for a, b in zip(grads[1:], old[1:]):
            assert torch.equal(a, b)
        # grad_value alone: the fill is a launch of its own
        only = backward(t, ROUTE_TR, want=1)
        assert only[1] is None and only[2] is None and only[3] is None
        value_ok(only[0], "want = 1")
        # the autograd Function
        fn = InstanceAttnBF16Function if dtype == BF16 else InstanceAttnF16Function
        B, S, H, C, L, Lq, P = g["dims"]
        v = t["value"].float().requires_grad_()
        loc = t["loc"].clone().requires_grad_()
        sw = t["sw"].view(B, Lq, H, L, g["k"], g["k"]).clone().requires_grad_()
        lw = t["lw"].view(B, Lq, H, L, g["k"], g["k"]).clone().requires_grad_()
        out, mask = fn.apply(v, t["shapes"], t["lsi"], loc, sw, lw, g["k"], 64)
        torch.autograd.backward([out, mask], [t["gout"], t["gmask"].view_as(mask)])
        torch.cuda.synchronize()
        value_ok(v.grad.to(dtype), "Function")
        assert torch.equal(loc.grad, old[1]) and torch.equal(sw.grad.view_as(old[2]), old[2])
        assert torch.equal(lw.grad.view_as(old[3]), old[3])
        # the compiled module, once
        mod = _ext.load()
        got = mod.instance_attn_backward(t["value"], t["shapes"], t["lsi"], t["loc"], t["sw"], t["lw"], t["gout"],
                                         t["gmask"], 64)
        torch.cuda.synchronize()
        value_ok(got[0], "compiled module")
        for a, b in zip(got[1:], old[1:]):
            assert torch.equal(a, b)
    finally:
        set_route(old_key)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_same_launches_per_profile_slot(dtype):
    from boxer_amd import _lib
    g = problem(dtype=dtype, **SHAPE_A)
    t = tensors(g, dtype)
    launches = {}
    for route in (ROUTE_VALU, ROUTE_TR):
        backward(t, route)                # (warm: workspace, state)
        _lib.profile_begin()
        try:
            backward(t, route)
        finally:
            prof = _lib.profile_end()
        launches[route] = {slot: v["launches"] for slot, v in prof.items()}
    assert launches[ROUTE_TR] == launches[ROUTE_VALU]
    assert launches[ROUTE_TR]["bwd_accumulate"] == 1


def test_key_23_touches_nothing_else():
    """Box attention (bf16, float32) and float32 instance attention at shape A: the same routes and results under key
    23 = 2 as under 23 = 0.  Forward outputs and point gradients are compared bit for bit.  grad_value is compared bit
    for bit wherever two runs under key 23 = 0 agree bit for bit (the fill claims record slots with integer atomics:
    the order of a pixel's float32 sum, hence its last bit, may differ from call to call); where they do not, to the
    bound test_binned_backward_run_to_run sets for that."""
    from boxer_amd import _lib, ops
    g = problem(dtype=BF16, **SHAPE_A)
    B, S, H, C, L, Lq, P = g["dims"]

    def run_all():
        res = []
        _lib.set_variant(3)
        for dtype in (BF16, torch.float32):
            t = tensors(g, dtype)
            res.append(ops.box_attn_forward(t["value"], t["shapes"], t["lsi"], t["loc"], t["sw"], 64))
            res.extend(ops.box_attn_backward(t["value"], t["shapes"], t["lsi"], t["loc"], t["sw"], t["gout"], 64))
        res.extend(ops.instance_attn_forward(t["value"], t["shapes"], t["lsi"], t["loc"], t["sw"], t["lw"], 64))
        res.extend(ops.instance_attn_backward(t["value"], t["shapes"], t["lsi"], t["loc"], t["sw"], t["lw"], t["gout"],
                                              t["gmask"], 64))
        torch.cuda.synchronize()
        _lib.set_variant(0)
        return res

    grad_value_at = (1, 5, 10)            # out, gv, gl, ga | out, gv, gl, ga | out, mask, gv, gl, gs, glw
    kinds = lambda: [query(g, 2, 0), query(g, 4, 0), query(g, 4, 1)]
    base, again, kinds0 = run_all(), run_all(), kinds()
    old = set_route(ROUTE_TR)
    try:
        forced, kinds2 = run_all(), kinds()
    finally:
        set_route(old)
    assert kinds2 == kinds0
    for i, (a, b, c) in enumerate(zip(base, again, forced)):
        if i not in grad_value_at or torch.equal(a, b):
            assert torch.equal(a, c), i
        else:
            tol = 8e-3 if a.dtype == BF16 else 1e-6
            assert (a.float() - c.float()).abs().max().item() <= tol * max(1.0, a.float().abs().max().item()), i
