"""The same problems at other magnitudes (test helper; not a conftest, never imported by boxer_amd): ``value`` times
2^a, the upstream gradients times 2^b, against the float64 model and bound of tests/error_bounds.py (DESIGN.md 5,
"Range").  The operator is linear in ``value`` and in the upstream gradients:

  out, mask_out                                       scale by 2^a
  grad_value                                          scales by 2^b
  every location, weight, box, window, logit gradient scales by 2^(a + b)

and so do the planes want / A / E / G / W / J of the reference, bit for bit, as long as the scaled inputs are the stored
numbers times the power of two (float32 and bf16 anywhere near the middle of their range; f16 upwards, until a value
rounds to inf).  Downwards f16 rounds -- most of the scaled numbers are subnormals -- and the reference is recomputed from
the rounded inputs (``reference``).

The rules that choose the exponents of the f16 families are here too: they read the inputs and the float64 model, never
a kernel's output.  ``wrong_box`` is box attention in numpy with three deliberate faults, the tests of these tests.
"""
import functools

import numpy as np

import error_bounds as eb
from boxes_cases import (bwd_problem, bwd_upstream, every_type, inst_problem, inst_upstream, kernel_offsets, model_of,
                         staged_bwd_case, staged_upstream)
from point_cases import decoder_input, encoder_input, k14_input, shape_a_input, wide_input

F16_MAX = 65504.0
F16_TIE = 65520.0            # round-to-nearest: the tie between 65504 and 2^16, the first magnitude that becomes inf
F16_MIN_NORMAL = 2.0 ** -14
STORED = ("out", "mask_out", "grad_value")
UPSTREAM = ("grad_out", "grad_mask")
_PLANES = ("want", "A", "E", "G", "W", "J", "unmasked")

EXACT = [(20, 0), (0, 20), (20, 20), (-12, -12)]          # float32 and bf16 storage: bit for bit
FAR = [(48, -48), (-48, 48)]                              # ... within the scaled bound


def factor(name, a, b):
    """The exponent an output scales by."""
    return a if name in ("out", "mask_out") else b if name == "grad_value" else a + b


def scaled(inp, a, b, store):
    """``inp`` (error_bounds' keys; tensors or numpy) with value 2^a and the upstream gradients 2^b times as large, each
    rounded to the stored type; float64 numpy.  Everything else is the same object."""
    out = {k: v for k, v in inp.items() if k != "_ref"}
    with np.errstate(over="ignore"):
        out["value"] = eb.round_to(np.ldexp(eb.f64(inp["value"]), a), store)
        for k in UPSTREAM:
            if k in inp:
                out[k] = eb.round_to(np.ldexp(eb.f64(inp[k]), b), store)
    return out


def is_exact(inp, a, b, store):
    """Does ``scaled`` round nothing?"""
    s = scaled(inp, a, b, store)
    return all(np.array_equal(s[k], np.ldexp(eb.f64(inp[k]), e))
               for k, e in (("value", a), ("grad_out", b), ("grad_mask", b)) if k in inp)


def scaled_reference(ref, a, b):
    """The reference of an exactly scaled problem: every magnitude plane times the output's factor; n, skip and the
    edge shares as they are."""
    res = {}
    for name, planes in ref.items():
        if not (isinstance(planes, dict) and "want" in planes):
            if name not in ("points", "grid", "weights"):       # (boxes_reference's working planes: not scaled, not kept)
                res[name] = planes
            continue
        f = factor(name, a, b)
        res[name] = {k: np.ldexp(v, f) if k in _PLANES else v for k, v in planes.items()}
    return res


def reference(inp, a, b, store, model=eb.reference_of):
    """The reference of ``inp`` at (a, b) in ``store`` -- scaled where that is exact, recomputed from the rounded inputs
    where it is not -- and the scaled inputs.  ``model``: inputs -> reference (error_bounds.reference_of; the from-boxes
    cases bring their own)."""
    s = scaled(inp, a, b, store)
    if is_exact(inp, a, b, store):
        return s, scaled_reference(model(inp), a, b)
    return s, model(s)


def slack(ref, split="none"):
    """R of the bound (error_bounds.bound): how far the value before the one rounding may be from want."""
    R = ((ref["n"] + 8.0) * 2.0 ** -24 + eb.SPLIT[split]) * ref["A"] + ref["E"]
    if split == "f16":
        R = R + 2.0 ** -25 * ref["G"]
    if "W" in ref:
        R = R + ref["W"]
    return R


def saturation(ref, store="f16", split="none"):
    """Per element of an f16 output -> dict of boolean planes:
      inf     must be +-inf with want's sign: |want| - R >= 65520, every value the bound allows rounds to inf;
      finite  must be finite and within the bound: |want| + R < 65520;
      either  the rest (the bound straddles the tie);
      live    somebody contributes (A + E > 0)."""
    assert eb.store_name(store) == "f16"
    R, w = slack(ref, split), np.abs(ref["want"])
    inf = w - R >= F16_TIE
    finite = w + R < F16_TIE
    return dict(inf=inf, finite=finite, either=~inf & ~finite, live=(ref["A"] + ref["E"]) > 0)


def hold_saturating(got, ref, split, what):
    """An f16 output that may overflow: inf of want's sign where it must be, finite and within the bound where it must
    be, either of the two in between, and never a NaN.  -> worst err / bound over the finite class."""
    g = eb.f64(got).reshape(ref["want"].shape)
    assert not np.isnan(g).any(), "%s: %d NaN" % (what, int(np.isnan(g).sum()))
    cls = saturation(ref, "f16", split)
    sign_inf = np.isinf(g) & (np.sign(g) == np.sign(ref["want"]))
    bad = cls["inf"] & ~sign_inf
    assert not bad.any(), "%s: %d of %d elements beyond 65520 are not inf of the exact sum's sign (the first: %r)" % (
        what, int(bad.sum()), int(cls["inf"].sum()), g[bad][:4])
    # held to the bound: what must be finite, and what may be either and is not inf of the right sign
    judged = cls["finite"] | (cls["either"] & ~sign_inf)
    r, _, _ = eb.ratio(np.where(judged, g, ref["want"]), ref, "f16", split)
    worst = float(r.max()) if r.size else 0.0
    assert worst <= 1.0, "%s: %d elements that must be finite (or may be) are outside the bound, worst err / bound %.3g" % (
        what, int((r > 1).sum()), worst)
    return worst


# ------------------------------------------------------------------ the rules that choose the exponents
def _outputs_of(ref, names):
    return [ref[n] for n in names if n in ref]


def high_exponents(inp, model=eb.reference_of):
    """f16 high -> (a, b): the largest exponents at which every rounded input is finite and max(|want| + R) of every
    f16 output -- out and mask_out for a, grad_value for b; R with the f16 split, the widest -- is at most 65504 / 2.
    Upwards the scaling is exact, so the base reference decides."""
    ref = model(inp)
    res = []
    for names, keys in ((("out", "mask_out"), ("value",)), (("grad_value",), UPSTREAM)):
        top_in = max(float(np.abs(eb.f64(inp[k])).max()) for k in keys if k in inp)
        top_out = max([float((np.abs(r["want"]) + slack(r, "f16")).max()) for r in _outputs_of(ref, names)] + [0.0])
        e = 40 if top_in > 0 else 0                 # (a forward alone has no upstream gradient to scale)
        while e > 0 and not (np.ldexp(top_in, e) <= F16_MAX and np.ldexp(top_out, e) <= F16_MAX / 2):
            e -= 1
        res.append(e)
    return tuple(res)


def low_shares(x, e):
    """x 2^e rounded to f16 -> (share of the nonzero rounded elements that are subnormal, share of the nonzero elements
    that round to zero)."""
    x = eb.f64(x).ravel()
    x = x[x != 0]
    r = np.abs(eb.round_to(np.ldexp(x, e), "f16"))
    return float(((r > 0) & (r < F16_MIN_NORMAL)).sum() / max(int((r > 0).sum()), 1)), float((r == 0).mean())


LOW_SUBNORMAL, LOW_ZERO = 0.90, 0.05          # the two shares every f16 low case keeps (asserted by the CPU twin)
LOW_PICK = 0.99                               # ... and the share the rule picks the exponent at


def low_exponent(x):
    """f16 low: the largest exponent at which at least LOW_PICK of the nonzero rounded elements of x 2^e are f16
    subnormals (-16 for randn; -8 for 0.01 rand)."""
    for e in range(0, -40, -1):
        if low_shares(x, e)[0] >= LOW_PICK:
            return e
    raise AssertionError("no exponent found")


def low_exponents(inp):
    ups = np.concatenate([eb.f64(inp[k]).ravel() for k in UPSTREAM if k in inp])
    return low_exponent(inp["value"]), (low_exponent(ups) if ups.any() else 0)


def overflow_input(inp):
    """The f16 overflow construction: every point of a level on about one pixel (loc 0.02 + 0.4, the one-block input of
    tests/test_gpu_onepass.py) and an upstream gradient of one sign -- grad_value is a sum of terms of one sign over
    very many points."""
    out = {k: v for k, v in inp.items() if k != "_ref"}
    out["loc"] = (eb.f64(inp["loc"]) * 0.02 + 0.4).astype(np.float32).astype(np.float64)
    out["grad_out"] = np.abs(eb.f64(inp["grad_out"]))
    return out


OVERFLOW_MIN = 64           # elements that must be inf, and elements that must be finite
OVERFLOW_EITHER = 0.01      # the largest share of the live elements the bound may leave undecided


def overflow_counts(ref_gv, split):
    c = saturation(ref_gv, "f16", split)
    live = c["live"]
    return int((c["inf"] & live).sum()), int((c["finite"] & live).sum()), int((c["either"] & live).sum()), int(live.sum())


def overflow_exponent(inp, upstream="grad_out", ref=None, split="f16"):
    """f16 overflow -> b: the smallest exponent that leaves at least OVERFLOW_MIN elements of grad_value in *must be
    inf* while every upstream element stays finite in f16.  ``inp`` has an upstream gradient f16 holds exactly, so the
    base reference scales."""
    ref = eb.reference_of(inp) if ref is None else ref
    top = float(np.abs(eb.f64(inp[upstream])).max())
    for b in range(0, 40):
        assert np.ldexp(top, b) <= F16_MAX, "the upstream gradient itself overflows at 2^%d" % b
        if overflow_counts(scaled_reference(dict(grad_value=ref["grad_value"]), 0, b)["grad_value"], split)[0] >= OVERFLOW_MIN:
            return b
    raise AssertionError("no exponent found")


# ------------------------------------------------------------------ three deliberately wrong implementations
FAULTS = ("flush", "saturate", "epsilon")


def wrong_box(inp, store, fault=None):
    """Box attention's forward and its grad_value in numpy: exact float64 sums of the stored inputs' products, rounded
    once to ``store`` -> dict(out, grad_value).  ``fault``: None (the definition), or one of three careless kernels
      "flush"     f16 subnormal operands (value, grad_out) read as zero -- a denormal mode left off;
      "saturate"  the f16 store clamps at +-65504 instead of rounding to inf;
      "epsilon"   2^-40 added to every product of a weight and an operand -- an absolute constant in a linear
                  operator."""
    value, loc, gout = (eb.f64(inp[k]) for k in ("value", "loc", "grad_out"))
    shapes, lsi = eb.f64(inp["shapes"]).astype(np.int64), eb.f64(inp["lsi"]).astype(np.int64)
    B, S, H, C = value.shape
    Lq, L = loc.shape[1], loc.shape[3]
    attn = eb.f64(inp["attn"]).reshape(loc.shape[:5])
    gout = gout.reshape(B, Lq, H, C)
    f16 = eb.store_name(store) == "f16"                       # (the first two faults are faults of f16 kernels)
    if fault == "flush" and f16:
        value = np.where(np.abs(value) < F16_MIN_NORMAL, 0.0, value)
        gout = np.where(np.abs(gout) < F16_MIN_NORMAL, 0.0, gout)
    more = 2.0 ** -40 if fault == "epsilon" else 0.0
    out, gv = np.zeros((B * Lq * H, C)), np.zeros((B * S * H, C))
    for l in range(L):
        t = eb.level_terms(value, shapes, lsi, loc, l)
        b, q, h, p, ok = t["b"], t["q"], t["h"], t["p"], t["ok"]
        aw = attn[b, q, h, l, p][:, None] * t["w"]                                    # (m, 4)
        np.add.at(out, (b * Lq + q) * H + h, ((aw[:, :, None] * t["v"] + more) * ok[:, :, None]).sum(1))
        g = gout[b, q, h]
        for k in range(4):
            rows = ((b * S + int(lsi[l]) + t["rows"][:, k]) * H + h)[ok[:, k]]
            np.add.at(gv, rows, aw[ok[:, k], k][:, None] * g[ok[:, k]] + more)
    res = dict(out=out.reshape(B, Lq, H * C), grad_value=gv.reshape(B, S, H, C))
    if fault == "saturate" and f16:
        res = {k: np.clip(v, -F16_MAX, F16_MAX) for k, v in res.items()}
    with np.errstate(over="ignore"):
        return {k: eb.round_to(v, store) for k, v in res.items()}


def base_input(group, dtype):
    if group == "encoder":
        return encoder_input("model", dtype, 1)
    if group == "decoder":
        return decoder_input("model", dtype)
    if group == "wide":
        return wide_input(36)
    if group == "shape_a":
        return shape_a_input("bf16" if dtype == "f32" else dtype)
    if group == "k14":
        return k14_input(dtype)
    return boxes_input(group)                  # (numbers every storage type holds: one input for the three)


GROUPS = ("encoder", "decoder", "wide", "shape_a", "k14")


# from boxes: the smallest geometry of each file; angle mode 0 and one rotated flavour (turns, valid ratios given)
PLAIN, TURNS = ((0, 4), False, True), ((1, 5), False, True)
BOXES_GROUPS = ("instance from boxes", "box from boxes, plain", "box from boxes, turns", "staged from boxes, plain",
                "staged from boxes, turns")
INST_CASE = ("one_level", 32, 4, False, True)               # geometry, C, k, per_head, with_vr
BOX_GEOMETRY, STAGED_GEOMETRY = "one_level", "tiny_levels"


def boxes_problem(group):
    """-> (the problem of the file the group comes from, its float64 upstream gradients)."""
    flavour = TURNS if group.endswith("turns") else PLAIN
    if group.startswith("instance"):
        p = inst_problem(*INST_CASE)
        return p, inst_upstream(p, INST_CASE[2])
    if group.startswith("box"):
        p = bwd_problem(BOX_GEOMETRY, 32, flavour)
        return p, (bwd_upstream(p),)
    p = staged_bwd_case(STAGED_GEOMETRY, "local", *flavour[0], *flavour[1:])
    return p, (staged_upstream(p),)


@functools.lru_cache(maxsize=None)
def boxes_input(group):
    p, ups = boxes_problem(group)
    return dict(zip(UPSTREAM, ups), kind="boxes", group=group, value=every_type(p["value"]))


def boxes_model(inp):
    """The float64 model of a from-boxes input (the files' own: error_bounds.boxes_reference; grad_value of the box
    step by boxes_cases.model_of), once per input."""
    if "_ref" not in inp:
        p, _ = boxes_problem(inp["group"])
        P = p["dims"][6] if len(p["dims"]) > 6 else INST_CASE[2] ** 2
        common = (inp["value"], p["shapes"], p["lsi"], p["ref"], p["off"], kernel_offsets(int(round(P ** 0.5))),
                  p["vr"], p["logits"])
        if inp["group"].startswith("instance"):
            ref = eb.boxes_reference("instance", *common, 0, INST_CASE[2], inp["grad_out"], inp["grad_mask"])
        else:
            ref = eb.boxes_reference("box", *common, p["angle_mode"], grad_out=inp["grad_out"])
            if inp["group"].startswith("box"):
                ref["grad_value"] = model_of(p, inp["grad_out"])         # (grad_value does not read ``value``)
        inp["_ref"] = {k: v for k, v in ref.items() if k not in ("points", "grid", "weights")}
    return inp["_ref"]


def reference_of(inp):
    return boxes_model(inp) if inp["kind"] == "boxes" else eb.reference_of(inp)


@functools.lru_cache(maxsize=None)
def f16_exponents(group):
    """-> ((a, b) of f16 high, (a, b) of f16 low)."""
    inp = base_input(group, "f16")
    return high_exponents(inp, reference_of), low_exponents(inp)


@functools.lru_cache(maxsize=None)
def f16_reference(group, a, b):
    """-> (the inputs at (a, b) rounded to f16, their reference)."""
    return reference(base_input(group, "f16"), a, b, "f16", reference_of)


@functools.lru_cache(maxsize=None)
def overflow_problem():
    """-> (b, the one-pixel encoder input with |grad_out| 2^b, its reference)."""
    inp = overflow_input(scaled(encoder_input("model", "f16", 1), 0, 0, "f16"))
    b = overflow_exponent(inp)
    s, ref = reference(inp, 0, b, "f16")
    return b, s, ref


VALUE_OVERFLOW = ("encoder", 32, PLAIN)          # geometry, C, flavour of boxes_cases.bwd_problem


@functools.lru_cache(maxsize=None)
def value_overflow_problem():
    """-> (b, the problem, |upstream| 2^b, grad_value's reference): the box step from boxes with every reference window
    shrunk onto one spot (centre 0.02 + 0.4, size 0.02: the construction of dynamic_range.overflow_input, on the windows)
    and an upstream gradient of one sign -- the weights are a softmax, so every term of grad_value is positive and the 80
    queries add into the same four pixels a level.  (The files' own problems never get there: their largest sums stay
    finite at every exponent the upstream gradient itself survives.)"""
    p = dict(bwd_problem(*VALUE_OVERFLOW))
    ref = p["ref"].copy()
    ref[..., :4] = ref[..., :4] * np.float32(0.02) + np.asarray([0.4, 0.4, 0.0, 0.0], dtype=np.float32)
    p["ref"] = ref
    gout = np.abs(bwd_upstream(p))
    base = model_of(p, gout)
    b = overflow_exponent(dict(grad_out=gout), ref=dict(grad_value=base), split="none")
    return b, p, np.ldexp(gout, b), scaled_reference(dict(grad_value=base), 0, b)["grad_value"]
