"""GPU: every route held to its bound away from magnitude 1 ("Range").  The problems, route setters and
route assertions are those of tests/test_gpu_error_bounds.py and the from-boxes files (tests/point_cases.py,
tests/boxes_cases.py, tests/route_vocab.py); tests/dynamic_range.py holds this file's own cases and scales them:
``value`` by 2^a, the upstream gradients by 2^b.

  exact      float32 and bf16 storage, (20, 0), (0, 20), (20, 20), (-12, -12): the case runs at (0, 0) and again on the
             device tensors times the power of two (exact in both types); ``out``, ``mask_out`` and every location,
             weight, box, window and logit gradient are ``torch.equal`` to the base run times the output's factor;
             grad_value, whose summation order no route fixes, is held to the scaled reference with the route's split;
  far        the same types, (48, -48) and (-48, 48): every output within the scaled bound;
  f16 high   the largest (a, b) at which every input is finite and every f16 output stays below 65504 / 2
             (dynamic_range.high_exponents): every output within the bound, the float32 ones finite;
  f16 low    (a, 0), (0, b), (a, b) with nearly every stored number an f16 subnormal (dynamic_range.low_exponents):
             the reference recomputed from the rounded inputs, every output within the bound with its t term;
  f16 overflow   grad_value of very many one-signed terms on one pixel a level: inf of the right sign where the exact
             sum less R is beyond 65520, finite and within the bound where the sum plus R is below, never a NaN;
             ``out``, grad_loc and grad_attn finite and within their bounds.

Every exponent is a property of the inputs (tests/test_dynamic_range.py computes and checks them without a GPU).  Each
case prints ``dynamic-range | route | type | family (a, b) | output | worst err / bound`` (``exact`` for the bitwise
claims); profiles/dynamic_range.log is that table from one run."""

import pytest
import torch

import dynamic_range as dr
import error_bounds as eb
import point_cases
import route_vocab
from dynamic_range import (BOXES_GROUPS, EXACT, FAR, INST_CASE, VALUE_OVERFLOW, base_input, boxes_problem,
                           f16_exponents, f16_reference, overflow_problem, reference_of, value_overflow_problem)
from point_cases import box_tensors, encoder_expectation, inst_tensors, run_box, run_instance
from route_vocab import ACC_TR, ACC_VALU, DTYPES, F16, F32, REC_POINT, STAGED, WIDE, routes, set_encoder_keys, split_of

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ inputs (CPU; the twin reads the same)


def f16_pairs(group):
    (ah, bh), (al, bl) = f16_exponents(group)
    pairs = [("f16 high", ah, bh), ("f16 low", al, 0), ("f16 low", 0, bl), ("f16 low", al, bl)]
    if group == "wide":                       # (a forward alone: no upstream gradient)
        pairs = [p for p in pairs if p[2] == 0 or p[0] == "f16 high"]
    return pairs


# ------------------------------------------------------------------ running
@pytest.fixture(autouse=True)
def _fresh_state():
    from boxer_amd import ops
    ops.release_workspaces()
    yield
    ops.release_workspaces()


def tensors_of(inp, dt):
    if inp["kind"] == "boxes":
        return dict({k: route_vocab.to_device(inp[k], dt) for k in ("value",) + dr.UPSTREAM if k in inp},
                    group=inp["group"])
    return inst_tensors(inp, dt) if inp["kind"] == "instance" else box_tensors(inp, dt)


def times(t, a, b):
    """The device tensors with value 2^a and the upstream gradients 2^b times as large: exact in float32 and bf16."""
    s = dict(t, value=t["value"] * 2.0 ** a)
    for k in dr.UPSTREAM:
        if k in t:
            s[k] = t[k] * 2.0 ** b
    assert s["value"].dtype == t["value"].dtype and torch.equal(s["value"].double(), t["value"].double() * 2.0 ** a)
    return s


def run_forward(t):
    from boxer_amd import ops
    out = ops.box_attn_forward(t["value"], t["shapes"], t["lsi"], t["loc"], t["attn"], 64)
    torch.cuda.synchronize()
    return dict(out=out)


def line(route, dtype, family, a, b, name, worst):
    print("dynamic-range | %s | %s | %s (%d, %d) | %s | %s" % (
        route, eb.store_name(dtype), family, a, b, name, worst if isinstance(worst, str) else "%.3f" % worst))


def hold_scaled(route, dt, family, a, b, got, ref, split, splits):
    assert ref.get("edge_share", 0.0) <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (route, 100 * ref["edge_share"])
    res = eb.hold_all(got, ref, dt, split, "%s, %s (%d, %d)" % (route, family, a, b), splits=splits)
    for name, worst in res.items():
        line(route, dt, family, a, b, name, worst)
    return res


def exact_and_far(route, inp, dt, prepare, run, split, splits=None):
    """float32 / bf16 storage: the base run, the four exact scalings against it, the two far ones against the bound."""
    t = tensors_of(inp, dt)
    prepare(t)
    base = run(t)
    ref = reference_of(inp)
    hold_scaled(route, dt, "base", 0, 0, base, ref, split, splits)
    for a, b in EXACT:
        s = times(t, a, b)
        prepare(s)
        got = run(s)
        for name, x in got.items():
            if name == "grad_value":
                worst = eb.hold(x, dr.scaled_reference(ref, a, b)[name], dt, split, "%s (%d, %d): grad_value" % (route, a, b))
                line(route, dt, "exact", a, b, name, worst)
                continue
            want = base[name] * 2.0 ** dr.factor(name, a, b)
            assert x.dtype == want.dtype and torch.isfinite(want).all()
            differ = int((x != want).sum())
            assert torch.equal(x, want), "%s (%d, %d): %s is not the base run times 2^%d in %d of %d elements" % (
                route, a, b, name, dr.factor(name, a, b), differ, x.numel())
            line(route, dt, "exact", a, b, name, "exact")
    for a, b in FAR:
        s = times(t, a, b)
        prepare(s)
        hold_scaled(route, dt, "far", a, b, run(s), dr.scaled_reference(ref, a, b), split, splits)


def f16_ends(route, group, prepare, run, split, splits=None):
    """f16 storage: the high end and the three low pairs, each against the reference of the rounded inputs."""
    for family, a, b in f16_pairs(group):
        s, ref = f16_reference(group, a, b)
        t = tensors_of(s, F16)
        assert all(bool(torch.isfinite(t[k]).all()) for k in ("value",) + dr.UPSTREAM if k in t)
        prepare(t)
        got = run(t)
        for name, x in got.items():
            assert torch.isfinite(x).all(), "%s, %s (%d, %d): %s is not finite" % (route, family, a, b, name)
        hold_scaled(route, F16, family, a, b, got, ref, split, splits)


# ------------------------------------------------------------------ the encoder on odd maps
ENCODER_IDS = ["f32_split", "f32_valu", "f32_mfma", "bf16_point", "bf16_group", "f16_point", "f16_group"]


def encoder_route(dtype, acc_key, rec_key, dense):
    """-> (route text, prepare, split of grad_value, splits)."""
    dt = DTYPES[dtype]
    fwd, acc, rec, _ = encoder_expectation(dtype, dense, 0, acc_key, rec_key)

    def prepare(t):
        set_encoder_keys(dense, 0, acc_key, rec_key)
        assert routes(t) == (fwd, acc, rec), "the library answers %r" % (routes(t),)
    route = "encoder: %s forward, %s accumulate, %s records" % (
        "staged" if dense == 2 else "row-gather", ("valu", "tr", "f32", "split")[acc], ("point", "group")[rec])
    return route, prepare, split_of(acc, dt), {"out": eb.store_name(dt) if fwd == STAGED and dt != F32 else "none"}


@pytest.mark.parametrize("dense", [2, 1], ids=["staged", "row_gather"])
@pytest.mark.parametrize("dtype,acc_key,rec_key", point_cases.ENCODER_ROUTES, ids=ENCODER_IDS)
def test_encoder(dtype, acc_key, rec_key, dense):
    """(13, 13), (7, 5), one query per pixel, riders as by default."""
    route, prepare, split, splits = encoder_route(dtype, acc_key, rec_key, dense)
    if dtype == "f16":
        f16_ends(route, "encoder", prepare, run_box, split, splits)
    else:
        exact_and_far(route, base_input("encoder", dtype), DTYPES[dtype], prepare, run_box, split, splits)


# ------------------------------------------------------------------ decoder shapes, every variant
@pytest.mark.parametrize("dtype,variant", point_cases.DECODER_ROUTES,
                         ids=["%s_%s" % (dt, ("auto", "generic", "atomic", "binned")[v]) for dt, v in point_cases.DECODER_ROUTES])
def test_decoder(dtype, variant):
    """Four levels, 50 queries: the generic kernels (float32), the atomic backward with the first-generation forward, the
    binned backward."""
    from boxer_amd import _lib
    dt = DTYPES[dtype]
    seen = {}

    def prepare(t):
        _lib.set_variant(variant)
        fwd, acc, rec = routes(t)
        assert fwd == point_cases.DECODER_FORWARD[variant] and rec == REC_POINT, (fwd, rec)
        assert acc == (route_vocab.ACC_SPLIT if dt == F32 else ACC_TR), acc
        seen["acc"] = acc
    prepare(box_tensors(base_input("decoder", dtype), dt, "cpu"))            # (the route queries are host code)
    split = "none" if variant in (1, 2) else split_of(seen["acc"], dt)
    route = "decoder, variant %s: %s forward, grad_value split %s" % (
        ("auto", "generic", "atomic", "binned")[variant], _lib.FWD_FAMILIES[point_cases.DECODER_FORWARD[variant]], split)
    if dtype == "f16":
        f16_ends(route, "decoder", prepare, run_box, split)
    else:
        exact_and_far(route, base_input("decoder", dtype), dt, prepare, run_box, split)


# ------------------------------------------------------------------ wave per pair
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_wave_per_pair_forward(dtype):
    from route_vocab import take_family
    route = "wave-per-pair forward, P = 36"

    def prepare(t):
        take_family(t["value"], t["loc"], t["shapes"], t["lsi"], WIDE)
    if dtype == "f16":
        f16_ends(route, "wide", prepare, run_forward, "none")
    else:
        exact_and_far(route, base_input("wide", dtype), DTYPES[dtype], prepare, run_forward, "none")


# ------------------------------------------------------------------ instance attention
@pytest.mark.parametrize("dtype,key", [("bf16", 2), ("f16", 2), ("f32", 0)], ids=["bf16_tr", "f16_tr", "f32"])
def test_instance_shape_a(dtype, key):
    """(16, 24), (7, 5), (1, 3), 300 queries, 4 x 4 points: the 16-bit accumulate on the matrix cores, float32 on its
    default route; the binned backward required."""
    from boxer_amd import _lib
    dt = DTYPES[dtype]
    acc = ACC_TR if key == 2 else ACC_VALU

    def prepare(t):
        _lib.set_option("inst_acc16", key)
        _lib.set_variant(3)
        assert routes(t, instance=True)[1:] == (acc, REC_POINT), routes(t, instance=True)
    route = "instance shape A: %s accumulate" % ("valu", "tr", "f32", "split")[acc]
    if dtype == "f16":
        f16_ends(route, "shape_a", prepare, run_instance, split_of(acc, dt))
    else:
        exact_and_far(route, base_input("shape_a", dtype), dt, prepare, run_instance, split_of(acc, dt))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_instance_14_by_14_points(dtype):
    """k = 14, six queries, four levels: the wave-per-pair instance forward and the backward on its default route."""
    dt = DTYPES[dtype]
    seen = {}

    def prepare(t):
        fwd, acc, rec = routes(t, instance=True)
        assert fwd == WIDE and rec == REC_POINT, (fwd, rec)
        assert seen.setdefault("acc", acc) == acc
    prepare(inst_tensors(base_input("k14", dtype), dt, "cpu"))
    split = split_of(seen["acc"], dt)
    route = "instance k = 14: wide forward, %s accumulate" % ("valu", "tr", "f32", "split")[seen["acc"]]
    if dtype == "f16":
        f16_ends(route, "k14", prepare, run_instance, split)
    else:
        exact_and_far(route, base_input("k14", dtype), dt, prepare, run_instance, split)


# ------------------------------------------------------------------ f16 overflow
OVERFLOW_ROUTES = [("point", 0, 1), ("group", 0, 2), ("atomic", 2, 0)]          # name, kernel variant, group_records key


@pytest.mark.parametrize("name,variant,rec_key", OVERFLOW_ROUTES, ids=[r[0] for r in OVERFLOW_ROUTES])
def test_f16_grad_value_overflows_to_inf(name, variant, rec_key):
    """Every point of a level on about one pixel, |grad_out| 2^b: some elements of grad_value are beyond 65520 whatever
    the bound allows, most are below.  The former are inf of the sum's sign, the latter finite and within the bound,
    nothing is NaN; ``out`` cannot overflow; grad_loc and grad_attn are float32 and within their bounds."""
    from boxer_amd import _lib
    b, s, ref = overflow_problem()
    t = box_tensors(s, F16)
    assert all(bool(torch.isfinite(t[k]).all()) for k in ("value", "grad_out"))
    if variant == 2:
        _lib.set_variant(2)
        fwd, acc, rec = routes(t)
        assert fwd == route_vocab.FAST, fwd
        split = "none"
    else:
        set_encoder_keys(2, 0, 0, rec_key)
        fwd, acc, rec = routes(t)
        assert (fwd, acc, rec) == encoder_expectation("f16", 2, 0, 0, rec_key)[:3], (fwd, acc, rec)
        split = "f16"
    route = "encoder, one pixel a level: %s" % name
    got = run_box(t)
    for k, x in got.items():
        assert not torch.isnan(x).any(), "%s: NaN in %s" % (route, k)
    gv = got.pop("grad_value")
    n_inf, n_fin, n_either, live = dr.overflow_counts(ref["grad_value"], split)
    assert n_inf >= dr.OVERFLOW_MIN and n_fin >= dr.OVERFLOW_MIN and n_either <= dr.OVERFLOW_EITHER * live
    worst = dr.hold_saturating(gv, ref["grad_value"], split, route + ": grad_value")
    line(route, F16, "f16 overflow", 0, b, "grad_value (%d inf / %d finite / %d either)" % (n_inf, n_fin, n_either), worst)
    assert int(torch.isinf(gv).sum()) >= n_inf
    for k, x in got.items():
        assert torch.isfinite(x).all(), "%s: %s is not finite" % (route, k)
    hold_scaled(route, F16, "f16 overflow", 0, b, got, ref, split,
                {"out": "f16" if fwd == STAGED else "none"})


# ------------------------------------------------------------------ from boxes
def run_boxes(t):
    """Every from-boxes entry point of the group on the device tensors ``t`` -> its outputs by name; each asserts that
    the route it is about is the one that runs (the library's eligibility queries, as the files it comes from do)."""
    import boxes_cases
    import boxes_cases
    import boxes_cases as value_route
    import boxes_cases
    import route_vocab
    from boxer_amd import ops
    group = t["group"]
    p, _ = boxes_problem(group)
    value, gout = t["value"], t["grad_out"]
    if group.startswith("instance"):
        k = INST_CASE[2]
        B, S, H, C, L, Lq = p["dims"]
        a = (value, route_vocab.dev(p["shapes"]), route_vocab.dev(p["lsi"]), route_vocab.dev(p["ref"]),
             route_vocab.dev(p["off"]), route_vocab.dev(boxes_cases.kernel_offsets(k)),
             None if p["vr"] is None else route_vocab.dev(p["vr"]), route_vocab.dev(p["logits"]), k)
        assert ops.forward_boxes_ok(value, L, Lq, k) and ops.backward_boxes_ok(value, L, Lq, k)
        out, mask = ops.instance_attn_forward_boxes(*a, True)
        grads = ops.instance_attn_backward_boxes(*a, gout, t["grad_mask"], need_ref_grad=True)
        got = dict(zip(boxes_cases.GRAD_NAMES, grads), out=out, mask_out=mask)
    elif group.startswith("box"):
        B, S, H, C, L, Lq, P = p["dims"]
        args = boxes_cases.box_args(p, value.dtype, value=value)
        assert ops.box_forward_boxes_ok(value, L, Lq, P) and ops.box_backward_boxes_ok(value, L, Lq, P)
        assert ops.box_backward_boxes_value_ok(value, L, Lq, P)
        out = ops.box_attn_forward_boxes(*args)
        grads = ops.box_attn_backward_boxes(*args, gout, need_ref_grad=True)
        with_value = value_route.value_call(args, gout)
        value_route.same_parameter_gradients(with_value[1:], grads, group)
        got = dict(zip(boxes_cases.GRAD_NAMES, grads), out=out, grad_value=with_value[0])
    else:
        args = boxes_cases.operands(p, value.dtype, value=value)
        out = boxes_cases.run_staged_forward(p, args)
        got = dict(zip(boxes_cases.GRAD_NAMES, boxes_cases.run_staged_backward(p, args, gout)), out=out)
    torch.cuda.synchronize()
    for name, x in got.items():
        assert x.dtype == (value.dtype if name in dr.STORED else F32), name
    return got


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("group", BOXES_GROUPS)
def test_from_boxes(group, dtype):
    """Instance attention forward and backward from boxes; box attention forward, backward and the backward with
    grad_value in its own launch; the window-staged forward and backward -- the grid and the weights are made inside the
    kernels, from operands that are not scaled."""
    import boxes_cases
    splits = {"out": boxes_cases.STAGED_SPLIT[dtype] if group.startswith("staged") else "none"}
    nothing = lambda t: None
    if dtype == "f16":
        f16_ends(group, group, nothing, run_boxes, "none", splits)
    else:
        exact_and_far(group, base_input(group, dtype), DTYPES[dtype], nothing, run_boxes, "none", splits)


def test_f16_grad_value_from_boxes_overflows_to_inf():
    """ops.box_attn_backward_boxes_value: float32 scratch, then a cast pass to f16."""
    import boxes_cases as value_route
    import boxes_cases
    import route_vocab
    from boxer_amd import ops
    b, p, gout64, ref = value_overflow_problem()
    B, S, H, C, L, Lq, P = p["dims"]
    args = boxes_cases.box_args(p, F16)
    gout = route_vocab.dev(gout64, F16)
    assert torch.isfinite(gout).all() and torch.equal(gout.double().cpu(), torch.from_numpy(gout64))
    assert ops.box_backward_boxes_value_ok(args[0], L, Lq, P)
    got = value_route.value_call(args, gout)
    route = "box backward with grad_value from boxes: %s" % VALUE_OVERFLOW[0]
    n_inf, n_fin, n_either, live = dr.overflow_counts(ref, "none")
    assert n_inf >= dr.OVERFLOW_MIN and n_fin >= dr.OVERFLOW_MIN and n_either <= dr.OVERFLOW_EITHER * live
    worst = dr.hold_saturating(got[0], ref, "none", route + ": grad_value")
    line(route, F16, "f16 overflow", 0, b, "grad_value (%d inf / %d finite / %d either)" % (n_inf, n_fin, n_either), worst)
    for name, x in zip(boxes_cases.GRAD_NAMES, got[1:]):
        assert x.dtype == F32 and torch.isfinite(x).all(), "%s: %s is not finite" % (route, name)
