"""CPU: the per-element error bound of tests/error_bounds.py itself.

  * its exact values agree with the float64 C oracle (oracle/boxattn_oracle.c) on every output;
  * the oracle's own float32 arithmetic -- the yardstick, never a HIP kernel -- is inside the float32 bound on every
    output, and exact sums rounded once to bf16 / f16 are inside the 16-bit bounds;
  * the bound notices what the suite's global-scale comparisons do not: a dropped bilinear corner, weights kept as ONE
    16-bit term, a sample point with f_x and 1 - f_x swapped;
  * the inputs of tests/test_gpu_error_bounds.py keep the cell-edge condition of grad_loc, and the library's route
    queries (host code) answer what every case of that file expects.
"""
import numpy as np
import pytest
import torch

import error_bounds as eb
import point_cases
import route_vocab
from compare_rules import check_f16, close_parity
from point_cases import SEEDED, _seeded, oracle

STORED = ("out", "mask_out", "grad_value")
TABLE = [([(16, 16), (8, 8)], "S", "model"), ([(13, 13), (7, 7)], "S", "model"), ([(8, 8)], 192, "model"),
         ([(16, 16), (8, 8)], "S", "test"), ([(20, 30), (10, 15), (5, 8), (3, 4)], 50, "model")]
CASES = {"table%d" % i: (lambda r=r: eb.numpy_inputs(eb.make(r[0], r[1], r[2], torch.bfloat16, seed=1)))
         for i, r in enumerate(TABLE)}
CASES["seeded6"] = lambda: dict(_seeded(*SEEDED[6], seed=11), kind="box")
CASES["inst_k14"] = lambda: eb.numpy_inputs(eb.make([(20, 30), (10, 15), (5, 8), (3, 4)], 6, "model", torch.bfloat16,
                                                    kind="instance", P=196, seed=1))
CASES["inst_k4"] = lambda: eb.numpy_inputs(eb.make([(11, 9), (6, 5), (3, 2)], 40, "test", torch.bfloat16, kind="instance",
                                                   P=16, seed=1))
_CACHE = {}


def case(name):
    """-> (inputs as float64 numpy, the helper's reference), once per case."""
    if name not in _CACHE:
        d = CASES[name]()
        d.setdefault("kind", "instance" if "grad_mask" in d else "box")
        if d["kind"] == "instance":
            ref = eb.instance_reference(d["value"], d["shapes"], d["lsi"], d["loc"], d["spatial_w"], d["level_w"],
                                        d["grad_out"], d["grad_mask"])
        else:
            ref = eb.box_reference(d["value"], d["shapes"], d["lsi"], d["loc"], d["attn"], d["grad_out"])
        _CACHE[name] = (d, ref)
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_values_agree_with_the_float64_oracle(name):
    d, ref = case(name)
    for out, want in oracle(d, np.float64).items():
        mine = ref[out]["want"]
        err = float(np.abs(np.asarray(want).reshape(mine.shape) - mine).max())
        assert err <= 1e-11 * float(np.abs(mine).max()), "%s %s: %.3e" % (name, out, err)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_oracles_float32_arithmetic_is_inside_the_bound(name):
    d, ref = case(name)
    assert ref["grad_loc"]["edge_share"] <= eb.EDGE_CAP
    worst = {out: eb.hold(got, ref[out], "float32", "none", "%s float32 oracle: %s" % (name, out))
             for out, got in oracle(d, np.float32).items()}
    print("%s: float32 oracle, worst err / bound %s" % (name, ", ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_sums_rounded_once_are_inside_the_bound(name, store):
    d, ref = case(name)
    for out in ref:
        st = store if out in STORED else "float32"
        eb.hold(eb.round_to(ref[out]["want"], st), ref[out], st, "none", "%s rounded once: %s" % (name, out))


def test_an_element_nobody_contributes_to_must_be_zero():
    d, ref = case("table4")
    r = ref["grad_value"]
    empty = (r["A"] + r["E"]) == 0
    assert empty.any(), "the decoder case leaves pixels untouched"
    got = r["want"].copy()
    got[tuple(np.argwhere(empty)[0])] = 1e-30
    with pytest.raises(AssertionError, match="outside the bound"):
        eb.hold(got, r, "float32", "none", "stray write")


# ------------------------------------------------------------------ mutations: what the bound is for
MUTATED = ["table0", "table2", "table3"]


def dropped_corner_share(d, ref, store, split):
    """Share of the (point, corner) terms whose loss the bound notices in grad_value and in out: the exact sum without
    the term, rounded once, is outside the bound in at least one channel."""
    B, S, Hh, C = d["value"].shape
    Lq = d["loc"].shape[1]
    g = d["grad_out"].reshape(B, Lq, Hh, C)
    bnd = {k: eb.bound(ref[k], store, split).reshape(-1, C) for k in ("grad_value", "out")}
    want = {k: ref[k]["want"].reshape(-1, C) for k in ("grad_value", "out")}
    seen = {"grad_value": [], "out": []}
    for l in range(len(d["shapes"])):
        t = eb.level_terms(d["value"], d["shapes"], d["lsi"], d["loc"], l)
        b, q, h, p = t["b"], t["q"], t["h"], t["p"]
        a = d["attn"].reshape(d["loc"].shape[:5])[b, q, h, l, p]
        for k in range(4):
            ok = t["ok"][:, k]
            aw = (a * t["w"][:, k])[ok]
            rows = {"grad_value": ((b * S + int(d["lsi"][l]) + t["rows"][:, k]) * Hh + h)[ok],
                    "out": ((b * Lq + q) * Hh + h)[ok]}
            term = {"grad_value": aw[:, None] * g[b, q, h][ok], "out": aw[:, None] * t["v"][:, k][ok]}
            for name in seen:
                w = want[name][rows[name]]
                got = eb.round_to(w - term[name], store)
                seen[name].append((np.abs(got - w) > bnd[name][rows[name]]).any(-1))
    return {k: float(np.concatenate(v).mean()) for k, v in seen.items()}


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("name", MUTATED)
def test_a_dropped_corner_is_noticed(name, store):
    """At least 95 % of the (point, corner) terms must be noticed when they go missing, in grad_value and in out.
    Measured (exact sum without the term, rounded once to the storage type; bf16 / f16):
      (16, 16), (8, 8) model   grad_value 99.4 / 99.8 %   out 99.5 / 99.8 %
      (8, 8), 192 queries      grad_value 99.3 / 99.7 %   out 99.6 / 99.9 %
      (16, 16), (8, 8) test    grad_value 99.2 / 99.7 %   out 98.0 / 99.4 %
    The hardest case is ``out`` of the "test" family in bf16: its values are all positive (rand * 0.01), an element is a
    sum of up to 32 terms of one sign, and a small corner moves the stored number by one step at most.  With the store
    term as u |want| -- a whole step at the top of a binade -- only 94.5 % were noticed there; error_bounds.half_ulp is
    what brings it to 98.0 %.  What is left changes no stored digit in any of the 32 channels."""
    d, ref = case(name)
    share = dropped_corner_share(d, ref, store, store)
    print("%s %s: a dropped corner is noticed in grad_value for %.1f %% of the corners, in out for %.1f %%"
          % (name, store, 100 * share["grad_value"], 100 * share["out"]))
    assert share["grad_value"] >= 0.95 and share["out"] >= 0.95, share


def as_tensor(a, store):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16 if store == "bf16" else torch.float16)


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("name", MUTATED)
def test_one_term_weights_fail_the_bound_and_pass_the_global_scale_checks(name, store):
    """Every weight a w_k kept as ONE 16-bit number (the lo term of the matrix-core kernels lost), the sums exact and
    rounded once: outside the bound, inside compare_rules.close_parity (bf16) and compare_rules.check_f16 (f16) -- the
    gap the
    bound closes."""
    d, ref = case(name)
    mut = eb.box_reference(d["value"], d["shapes"], d["lsi"], d["loc"], d["attn"], d["grad_out"],
                           weight_hook=lambda aw: eb.round_to(aw, store))
    for out in ("grad_value", "out"):
        got = eb.round_to(mut[out]["want"], store)
        r, _, _ = eb.ratio(got, ref[out], store, store)
        print("%s %s %s: one-term weights, %.1f %% of the elements outside the bound, worst err / bound %.1f"
              % (name, store, out, 100 * float((r > 1).mean()), float(r.max())))
        with pytest.raises(AssertionError, match="outside the bound"):
            eb.hold(got, ref[out], store, store, "one-term weights")
        if store == "bf16":
            close_parity(as_tensor(got, store), ref[out]["want"], torch.bfloat16, out)
        else:
            check_f16(as_tensor(got, store), ref[out]["want"], out)


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("name", MUTATED)
def test_a_point_with_swapped_fractions_is_noticed(name, store):
    """One sample point of level 0 -- the first whose four corners lie inside the map and whose f_x is at least 0.1 from
    1/2 -- with f_x and 1 - f_x swapped."""
    d, ref = case(name)
    t = eb.level_terms(d["value"], d["shapes"], d["lsi"], d["loc"], 0)
    pick = int(np.nonzero(t["ok"].all(1) & (np.abs(t["fx"] - 0.5) > 0.1))[0][0])

    def swap(l, sel, fy, fx):
        if l == 0:
            fx = fx.copy()
            fx[pick] = 1 - fx[pick]
        return fy, fx
    mut = eb.box_reference(d["value"], d["shapes"], d["lsi"], d["loc"], d["attn"], d["grad_out"], frac_hook=swap)
    for out in ("grad_value", "out"):
        with pytest.raises(AssertionError, match="outside the bound"):
            eb.hold(eb.round_to(mut[out]["want"], store), ref[out], store, store, "swapped fractions")


# ------------------------------------------------------------------ the CPU twin of tests/test_gpu_error_bounds.py
def test_edge_share_of_every_gpu_input_is_under_the_cap():
    worst = 0.0
    for name, build in point_cases.all_inputs():
        inp = build()
        share = float(eb.on_edge(eb.f64(inp["loc"]), eb.f64(inp["shapes"])).mean())
        worst = max(worst, share)
        assert share <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (name, 100 * share)
    from boxes_cases import inst_edge_share as edge_share
    share = edge_share(point_cases.boxes_input(), 14)
    assert share <= eb.EDGE_CAP, "forward from boxes: %.4f %%" % (100 * share)
    print("worst share %.4f %%" % (100 * max(worst, share)))


def test_every_gpu_case_expects_the_route_the_library_answers():
    """boxattn_fwd_route / boxattn_bwd_accumulate_kind / boxattn_bwd_record_kind are host code: what the GPU cases
    assert before they run can be checked here."""
    from boxer_amd import _lib
    try:
        for family in ("model",):
            for (dtype, acc_key, rec_key) in point_cases.ENCODER_ROUTES:
                for dense in (2, 1):
                    for riders in (0, 1):
                        route_vocab.set_encoder_keys(dense, riders, acc_key, rec_key)
                        t = point_cases.box_tensors(point_cases.encoder_input(family, dtype, 1),
                                                    route_vocab.DTYPES[dtype], "cpu")
                        want = point_cases.encoder_expectation(dtype, dense, riders, acc_key, rec_key)[:3]
                        assert route_vocab.routes(t) == want, (dtype, acc_key, rec_key, dense, riders,
                                                               route_vocab.routes(t), want)
        route_vocab.set_encoder_keys(0, 0, 0, 0)
        for dtype, dt in route_vocab.DTYPES.items():
            acc = route_vocab.ACC_SPLIT if dtype == "f32" else route_vocab.ACC_TR
            for variant in (0, 3):
                _lib.set_variant(variant)
                for C in ((16, 32, 64) if dtype == "bf16" else (32,)):
                    if C == 32 or dtype == "bf16":
                        t = point_cases.box_tensors(point_cases.seeded6_input(C), dt, "cpu")
                        assert route_vocab.routes(t) == (route_vocab.GATHER, acc, route_vocab.REC_POINT), \
                            (dtype, C, variant, route_vocab.routes(t))
            for _, variant in [r for r in point_cases.DECODER_ROUTES if r[0] == dtype]:
                _lib.set_variant(variant)
                t = point_cases.box_tensors(point_cases.decoder_input("model", dtype), dt, "cpu")
                want = (point_cases.DECODER_FORWARD[variant], acc, route_vocab.REC_POINT)
                assert route_vocab.routes(t) == want, (dtype, variant, route_vocab.routes(t), want)
            _lib.set_variant(3)
            t = point_cases.inst_tensors(point_cases.shape_a_input("bf16" if dtype == "f32" else dtype), dt, "cpu")
            for key in ((0,) if dtype == "f32" else (1, 2)):
                _lib.set_option("inst_acc16", key)
                assert route_vocab.routes(t, instance=True)[1:] == (
                    route_vocab.ACC_TR if key == 2 else route_vocab.ACC_VALU, route_vocab.REC_POINT)
            _lib.set_option("inst_acc16", 0)
            _lib.set_variant(0)
            t = point_cases.inst_tensors(point_cases.k14_input(dtype), dt, "cpu")
            assert route_vocab.routes(t, instance=True)[0] == route_vocab.WIDE
            for P in (196, 36):
                t = point_cases.box_tensors(point_cases.wide_input(P), dt, "cpu")
                _lib.set_option("wide_box", 2)
                assert route_vocab.routes(t)[0] == route_vocab.WIDE, (dtype, P)
                _lib.set_option("wide_box", 0)
            b = point_cases.boxes_input()
            B, S, H, C, L, Lq = b["dims"]
            assert _lib.fwd_boxes_ok(dt.itemsize, 16, b["dims"], 14) and _lib.bwd_boxes_ok(dt.itemsize, 16, b["dims"], 14)
    finally:
        route_vocab.set_encoder_keys(0, 0, 0, 0)
        _lib.set_option("inst_acc16", 0)
        _lib.set_option("wide_box", 0)
        _lib.set_variant(0)
