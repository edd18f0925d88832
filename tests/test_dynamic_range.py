"""CPU: the twin of tests/test_gpu_dynamic_range.py -- what that file's cases assume about their inputs, checked on the
inputs and the float64 model alone.

  * the cell-edge share of every input is under the cap (the locations are those of tests/test_gpu_error_bounds.py);
  * the range conditions of every family hold: exact and far scalings round nothing and leave every stored number and
    every output normal and finite; the f16 high exponents are the largest the rule allows; at the f16 low exponents
    at least 90 % of the nonzero stored numbers are subnormals and at most 5 % round to zero; the overflow case has at
    least 64 elements that must be inf, 64 that must be finite and at most 1 % undecided, at the smallest such exponent;
  * error_bounds' references are exactly homogeneous: every plane of every output of the scaled problem is the base
    plane times the output's power of two, bit for bit;
  * the C oracle's float32 build, the arithmetic yardstick, is bitwise homogeneous at every exact exponent and inside
    the scaled bound at every far one;
  * three deliberately wrong implementations each fail the check aimed at them and nothing else.
"""
import numpy as np
import pytest

import dynamic_range as dr
import error_bounds as eb
import dynamic_range
import point_cases
from point_cases import oracle
from oracle import boxattn_oracle as oc

GROUP_TYPES = [(group, dtype) for group in dynamic_range.GROUPS for dtype in ("f32", "bf16")]
# (the from-boxes inputs are numbers every storage type holds: float32 and bf16 take the same)
ALL_GROUP_TYPES = GROUP_TYPES + [(group, "bf16") for group in dynamic_range.BOXES_GROUPS]
STORE = {"f32": "float32", "bf16": "bf16", "f16": "f16"}
TINY = {"float32": 2.0 ** -126, "bf16": 2.0 ** -126, "f16": 2.0 ** -14}
HUGE = {"float32": 3.4028234663852886e38, "bf16": 3.3895313892515355e38, "f16": 65504.0}


def numpy_of(inp):
    """An input dictionary (tensors or numpy) as the float64 / int64 arrays the C oracle takes."""
    d = {k: eb.f64(inp[k]) for k in ("value", "loc", "attn", "grad_out")}
    d["shapes"], d["lsi"] = (eb.f64(inp[k]).astype(np.int64) for k in ("shapes", "lsi"))
    d["kind"] = inp["kind"]
    if inp["kind"] == "instance":
        d["spatial_w"], d["level_w"], d["grad_mask"] = d["attn"], eb.f64(inp["level_w"]), eb.f64(inp["grad_mask"])
    return d


def outputs(ref):
    return {k: v for k, v in ref.items() if isinstance(v, dict)}


@pytest.fixture
def one_thread():
    """(grad_value compared bit for bit: one summation order)"""
    n = oc.num_threads()
    oc.set_num_threads(1)
    yield
    oc.set_num_threads(n)


# ------------------------------------------------------------------ 1. the cell-edge share
def test_edge_share_of_every_input_is_under_the_cap():
    inputs = [("%s %s" % (group, dtype), dynamic_range.base_input(group, dtype))
              for group in dynamic_range.GROUPS for dtype in STORE]
    inputs.append(("overflow", dynamic_range.overflow_problem()[1]))
    for name, inp in inputs:
        share = float(eb.on_edge(eb.f64(inp["loc"]), eb.f64(inp["shapes"])).mean())
        assert share <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (name, 100 * share)
        assert eb.reference_of(inp)["grad_loc"]["edge_share"] <= eb.EDGE_CAP
    for group in dynamic_range.BOXES_GROUPS:              # (with the locations' own slack: boxes_reference's count)
        share = dynamic_range.reference_of(dynamic_range.base_input(group, "f32"))["edge_share"]
        assert share <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (group, 100 * share)


# ------------------------------------------------------------------ 2. the range conditions, family by family
@pytest.mark.parametrize("group,dtype", ALL_GROUP_TYPES)
def test_exact_and_far_scalings_round_nothing_and_stay_normal(group, dtype):
    inp, store = dynamic_range.base_input(group, dtype), STORE[dtype]
    ref = dynamic_range.reference_of(inp)
    for a, b in dynamic_range.EXACT + dynamic_range.FAR:
        assert dr.is_exact(inp, a, b, store), (group, dtype, a, b)
        s = dr.scaled(inp, a, b, store)
        for k in ("value",) + dr.UPSTREAM:
            x = np.abs(s[k][s[k] != 0]) if k in s else np.ones(1)
            assert not x.size or (x.min() >= TINY[store] * 2.0 ** 32 and x.max() <= HUGE[store] * 2.0 ** -32), (k, a, b)
        for name, r in outputs(dr.scaled_reference(ref, a, b)).items():
            st = store if name in dr.STORED else "float32"
            top = float((np.abs(r["want"]) + eb.bound(r, st, "bf16")).max())
            assert top <= HUGE[st] * 2.0 ** -32, (name, a, b, top)
            # no stored result leaves the normal range either: an element is zero (nobody contributes, or an upstream
            # of zeros) or far above the smallest normal number, but for the few that cancel
            w = np.abs(r["want"][r["want"] != 0])
            assert not w.size or float((w < TINY[st] * 2.0 ** 24).mean()) <= 1e-3, (name, a, b)


@pytest.mark.parametrize("group", dynamic_range.GROUPS + dynamic_range.BOXES_GROUPS)
def test_f16_exponents_follow_their_rules(group):
    inp = dynamic_range.base_input(group, "f16")
    (ah, bh), (al, bl) = dynamic_range.f16_exponents(group)
    print("dynamic-range exponents | %s | f16 high (%d, %d) | f16 low (%d, %d)" % (group, ah, bh, al, bl))
    # high: every input finite, every f16 output at most 65504 / 2 -- and not so one exponent further
    assert dr.is_exact(inp, ah, bh, "f16")
    s, ref = dynamic_range.f16_reference(group, ah, bh)
    assert all(np.isfinite(s[k]).all() for k in ("value",) + dr.UPSTREAM if k in s)
    for name in dr.STORED:
        if name in ref:
            top = float((np.abs(ref[name]["want"]) + dr.slack(ref[name], "f16")).max())
            assert top <= dr.F16_MAX / 2, (name, top)
    for a, b, names in ((ah + 1, bh, ("out", "mask_out")), (ah, bh + 1, ("grad_value",))):
        s1 = dr.scaled(inp, a, b, "f16")
        r1 = dr.scaled_reference(dynamic_range.reference_of(inp), a, b)
        over = not all(np.isfinite(s1[k]).all() for k in ("value",) + dr.UPSTREAM if k in s1)
        over = over or any(float((np.abs(r1[n]["want"]) + dr.slack(r1[n], "f16")).max()) > dr.F16_MAX / 2
                           for n in names if n in r1)
        has_upstream = any(eb.f64(inp[k]).any() for k in dr.UPSTREAM if k in inp)
        assert over or (names == ("grad_value",) and not has_upstream), "(%d, %d) would do as well" % (a, b)
    # low: nearly everything a subnormal, hardly anything zero
    sub, zero = dr.low_shares(inp["value"], al)
    assert sub >= dr.LOW_SUBNORMAL and zero <= dr.LOW_ZERO, ("value", al, sub, zero)
    print("dynamic-range exponents | %s | value 2^%d: %.1f %% subnormal, %.1f %% zero" % (group, al, 100 * sub, 100 * zero))
    ups = [eb.f64(inp[k]).ravel() for k in dr.UPSTREAM if k in inp]
    if np.concatenate(ups).any():
        sub, zero = dr.low_shares(np.concatenate(ups), bl)
        assert sub >= dr.LOW_SUBNORMAL and zero <= dr.LOW_ZERO, ("upstream", bl, sub, zero)
        print("dynamic-range exponents | %s | upstream 2^%d: %.1f %% subnormal, %.1f %% zero" % (group, bl, 100 * sub, 100 * zero))
    # ... and the bound still tells: the median bound of out is a small part of the median |want|
    s, ref = dynamic_range.f16_reference(group, al, 0)
    live = ref["out"]["want"] != 0
    share = float(np.median(eb.bound(ref["out"], "f16", "f16")[live]) / np.median(np.abs(ref["out"]["want"][live])))
    print("dynamic-range exponents | %s | out at (%d, 0): median bound / median |want| = %.4f" % (group, al, share))
    assert share <= 0.05


def test_the_overflow_case_decides_nearly_every_element():
    b, s, ref = dynamic_range.overflow_problem()
    assert all(np.isfinite(s[k]).all() for k in ("value", "grad_out")) and (s["grad_out"] >= 0).all()
    for split in ("f16", "none"):
        n_inf, n_fin, n_either, live = dr.overflow_counts(ref["grad_value"], split)
        print("dynamic-range exponents | f16 overflow | b = %d, split %s: %d inf / %d finite / %d either of %d live"
              % (b, split, n_inf, n_fin, n_either, live))
        assert n_inf >= dr.OVERFLOW_MIN and n_fin >= dr.OVERFLOW_MIN and n_either <= dr.OVERFLOW_EITHER * live
    base = dr.overflow_input(dr.scaled(point_cases.encoder_input("model", "f16", 1), 0, 0, "f16"))
    less = dr.scaled_reference(eb.reference_of(base), 0, b - 1)["grad_value"]
    assert dr.overflow_counts(less, "f16")[0] < dr.OVERFLOW_MIN, "b - 1 would do as well"
    # out is a convex combination of finite values
    assert float(np.abs(ref["out"]["want"]).max()) <= float(np.abs(s["value"]).max())


def test_slack_is_the_bounds_r():
    ref = eb.reference_of(dynamic_range.base_input("encoder", "f16"))["grad_value"]
    for split in ("none", "f16", "bf16", "split3"):
        R = dr.slack(ref, split)
        want = np.where(ref["A"] + ref["E"] > 0, eb.half_ulp(np.abs(ref["want"]) + R, "f16") + R, 0.0)
        assert np.array_equal(want, eb.bound(ref, "f16", split))


# ------------------------------------------------------------------ 3. the float64 model is exactly homogeneous
@pytest.mark.parametrize("group,dtype", ALL_GROUP_TYPES)
def test_the_reference_is_exactly_homogeneous(group, dtype):
    """error_bounds.box_reference, instance_reference and boxes_reference (both kinds, rotated and not)."""
    inp, store = dynamic_range.base_input(group, dtype), STORE[dtype]
    ref = dynamic_range.reference_of(inp)
    for a, b in [(12, -7)] + dynamic_range.EXACT + dynamic_range.FAR:
        s = dr.scaled(inp, a, b, store)
        got, want = dynamic_range.reference_of(s), dr.scaled_reference(ref, a, b)
        for name, planes in outputs(want).items():
            for k, v in planes.items():
                assert np.array_equal(got[name][k], v), "%s %s (%d, %d): %s.%s" % (group, dtype, a, b, name, k)


# ------------------------------------------------------------------ 4. the float32 oracle, the arithmetic yardstick
@pytest.mark.parametrize("group,dtype", GROUP_TYPES)
def test_the_float32_oracle_is_homogeneous_and_inside_the_scaled_bound(group, dtype, one_thread):
    inp, store = dynamic_range.base_input(group, dtype), STORE[dtype]
    ref = eb.reference_of(inp)
    base = oracle(numpy_of(inp), np.float32)
    for a, b in dynamic_range.EXACT:
        got = oracle(numpy_of(dr.scaled(inp, a, b, store)), np.float32)
        for name, x in got.items():
            want = np.asarray(base[name], dtype=np.float32) * np.float32(2.0) ** dr.factor(name, a, b)
            assert np.array_equal(np.asarray(x), want), "%s %s (%d, %d): %s" % (group, dtype, a, b, name)
    for a, b in dynamic_range.FAR:
        got = oracle(numpy_of(dr.scaled(inp, a, b, store)), np.float32)
        sref = dr.scaled_reference(ref, a, b)
        worst = {name: eb.hold(x, sref[name], "float32", "none", "%s float32 oracle (%d, %d): %s" % (group, a, b, name))
                 for name, x in got.items()}
        print("%s %s (%d, %d): float32 oracle, worst err / bound %s" % (group, dtype, a, b,
                                                                       ", ".join("%s %.3f" % kv for kv in worst.items())))


# ------------------------------------------------------------------ 5. the tests can fail
def fault_checks():
    """name -> (inputs, store, check(got)): the f16 low, f16 overflow and far checks on the encoder input, and scale 1."""
    (_, _), (al, bl) = dynamic_range.f16_exponents("encoder")
    low, low_ref = dynamic_range.f16_reference("encoder", al, bl)
    b, over, over_ref = dynamic_range.overflow_problem()
    far32 = dynamic_range.base_input("encoder", "f32")

    def bounded(ref, store, split="none"):
        def check(got):
            for name, x in got.items():
                eb.hold(x, ref[name], store, split, name)
        return check

    def saturating(got):
        eb.hold(got["out"], over_ref["out"], "f16", "none", "out")
        dr.hold_saturating(got["grad_value"], over_ref["grad_value"], "none", "grad_value")
    # scale 1: randn leaves a handful of f16 subnormals among the 26 000 stored numbers, and the bound is sharp enough
    # to see one of them flushed; the input without them is what "magnitude about 1" means
    one = dr.scaled(dynamic_range.base_input("encoder", "f16"), 0, 0, "f16")
    for k in ("value", "grad_out"):
        few = (np.abs(one[k]) < dr.F16_MIN_NORMAL) & (one[k] != 0)
        assert few.sum() <= 8
        one[k] = np.where(few, 0.0, one[k])
    res = {"scale 1": (one, "f16", bounded(eb.reference_of(one), "f16")),
           "f16 low": (low, "f16", bounded(low_ref, "f16")),
           "f16 overflow": (over, "f16", saturating)}
    for a, b in dynamic_range.FAR:
        res["far (%d, %d)" % (a, b)] = (dr.scaled(far32, a, b, "float32"), "float32",
                                        bounded(dr.scaled_reference(eb.reference_of(far32), a, b), "float32"))
    return res


TARGET = {"flush": ("f16 low",), "saturate": ("f16 overflow",), "epsilon": ("far (48, -48)", "far (-48, 48)")}


def test_each_wrong_implementation_fails_the_check_aimed_at_it_and_no_other():
    checks = fault_checks()
    for name, (inp, store, check) in checks.items():
        check(dr.wrong_box(inp, store))                                  # the definition passes everything
    for fault in dr.FAULTS:
        for name, (inp, store, check) in checks.items():
            got = dr.wrong_box(inp, store, fault)
            if name in TARGET[fault]:
                with pytest.raises(AssertionError):
                    check(got)
                print("%s: reported by %s" % (fault, name))
            else:
                check(got)


def test_the_overflow_case_from_boxes_decides_nearly_every_element():
    b, p, gout, ref = dynamic_range.value_overflow_problem()
    assert np.isfinite(eb.round_to(gout, "f16")).all() and np.array_equal(eb.round_to(gout, "f16"), gout) and (gout >= 0).all()
    n_inf, n_fin, n_either, live = dr.overflow_counts(ref, "none")
    print("dynamic-range exponents | f16 overflow, grad_value from boxes (%s) | b = %d: %d inf / %d finite / %d either "
          "of %d live" % (dynamic_range.VALUE_OVERFLOW[0], b, n_inf, n_fin, n_either, live))
    assert n_inf >= dr.OVERFLOW_MIN and n_fin >= dr.OVERFLOW_MIN and n_either <= dr.OVERFLOW_EITHER * live
    less = dr.scaled_reference(dict(grad_value=ref), 0, -1)["grad_value"]
    assert dr.overflow_counts(less, "none")[0] < dr.OVERFLOW_MIN, "b - 1 would do as well"
