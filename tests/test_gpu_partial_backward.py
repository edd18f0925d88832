"""GPU tests of the partial backward (``-m gpu``): *_bwd_part_* compute only the gradient groups the caller asks
for -- VALUE (grad_value) or POINTS (grad_loc + the weight gradients) -- and the autograd Functions derive that from
``ctx.needs_input_grad``.

Reference gradients come from the fp64 CPU oracle (oracle/boxattn_oracle.c), compared the way the existing GPU
tests compare the same quantity and storage type: tests/compare_rules.py ``close_parity`` (fp64 1e-10, fp32 1e-4, bf16
1e-2, scaled by the magnitude of the expected tensor; grad_loc without the points on a bilinear cell edge),
``check_f16`` for float16 storage (1e-3 for f16 tensors, 1e-4 for float32 ones), and
bench.parity_report (``check_onepass``) for the encoder shapes of tests/test_gpu_dense.py (point_cases.make_dense_case).

grad_value sums are not ordered (float atomics; the record order inside a bin follows atomics): the bitwise claim of
want = 3 against the existing call is made where repeated runs of the existing call agree -- two runs first, and
REPEATS more of the existing call before a mismatch is held against the new entry (seen on an MI355X: the two-level generic float32 instance
case gave the same bits twice and other bits the third time).

Every case runs the full call twice, then the new entry with want = 3, 2, 1; all findings of a case are printed and
collected before the test asserts, so one run shows everything a kernel family gets wrong.
"""

import numpy as np
import pytest
import torch

import bench
import compare_rules
import point_cases
from point_cases import (ALL, Case, PARTIAL_DECODER as DECODER, POINTS, P_OF, REPEATS, SUFFIX, VALUE, _blib, call,
                         profiled, seeded_case, untouched)
from route_vocab import OPT_DENSE

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ cases


# ---- seeded problems (tests/test_gpu_parity.py's generator: storage values exact in every 16-bit type)


GRAD_NAMES = {"box": ("grad_value", "grad_loc", "grad_attn"),
              "instance": ("grad_value", "grad_loc", "grad_spatial_w", "grad_level_w")}


def oracle_errors(case, outs, want, on_edge, which):
    """The project's comparison for this storage type, for the outputs `which`: -> list of failure texts."""
    bad = []
    for i in which:
        name = GRAD_NAMES[case.kind][i]
        ignore = on_edge if name == "grad_loc" else None
        try:
            if case.dtype == torch.float16:
                compare_rules.check_f16(outs[i], want[i], name, ignore=ignore)
            else:
                compare_rules.close_parity(outs[i], np.asarray(want[i]).reshape(outs[i].shape), outs[i].dtype, name,
                                           ignore=ignore)
        except AssertionError as e:
            bad.append(str(e))
    return bad


def bench_errors(inp, out, outs, which):
    """bench.parity_report (tests/test_gpu_dense.py's check) for the gradients `which` of a box-attention step."""
    grads = [t if i in which else torch.zeros_like(z) for i, (t, z) in enumerate(zip(outs, outs))]
    return ["%s: worst %.3e > %.0e" % r for i, r in enumerate(bench.parity_report(inp, out, grads)[1:])
            if i in which and not r[1] <= r[2]]


def run_family(case, errors, states=True, inexact_points=""):
    """Assertions 1-5 of one case.  errors(outs, which) -> failures against the oracle.  inexact_points: why this
    family's POINTS-only gradients are not the full call's bit for bit (then checked at the oracle tolerance only)."""
    bad = []
    note = lambda ok, text: (print(("ok   " if ok else "FAIL ") + text), ok or bad.append(text))
    points = tuple(range(1, case.n_out))
    state = case.new_state() if states and case.dtype != torch.float64 else None
    rc1, full1 = call(case, state=state, fresh=True)
    rc2, full2 = call(case, state=state)
    note(rc1 == 0 and rc2 == 0, "full call returns 0 (%d, %d)" % (rc1, rc2))
    for e in errors(full2, (0,) + points):
        note(False, "full call vs oracle: " + e)
    value_repeats = torch.equal(full1[0], full2[0])
    print("     grad_value of two full calls bitwise equal: %s" % value_repeats)
    note(all(torch.equal(full1[i], full2[i]) for i in points), "point gradients of two full calls bitwise equal")

    # 2. want = 3 through the new entry is the full call
    rc, p3 = call(case, want=ALL, state=state)
    note(rc == 0, "want=3 returns 0 (%d)" % rc)
    note(all(torch.equal(p3[i], full2[i]) for i in points), "want=3: point gradients bitwise equal to the full call")
    if value_repeats and not torch.equal(p3[0], full2[0]):
        # Two equal runs do not prove an ordered sum: float atomics (and the order of the records inside a bin, which
        # follows atomics) may differ from any run to the next, rarely on a small problem.  Before the mismatch is held
        # against want=3, the probe of the EXISTING call is repeated: one run of it that differs from the first two puts
        # the family among those whose runs differ (oracle tolerance then); if the existing call never wavers, the
        # claim stands and has failed.
        more = [call(case, state=state)[1][0] for _ in range(REPEATS)]
        value_repeats = all(torch.equal(m, full2[0]) for m in more)
        print("     grad_value: want=3 differed; %d more full calls all bitwise equal: %s" % (REPEATS, value_repeats))
        if value_repeats:
            note(False, "want=3: grad_value bitwise equal to the full call (%d full calls agree with each other)"
                 % (REPEATS + 2))
    elif value_repeats:
        note(True, "want=3: grad_value bitwise equal to the full call")
    if not value_repeats:
        for e in errors(p3, (0,)):
            note(False, "want=3 grad_value vs oracle: " + e)

    # POINTS only: real buffers with a bit pattern for the unwanted group, then NULL (and no workspace, no state)
    pat = case.outputs(pattern=True)
    (rc, p2), slots = profiled(lambda: call(case, want=POINTS, outs=pat, state=state))
    print("     want=2 launches: %s" % slots)
    note(rc == 0, "want=2 returns 0 (%d)" % rc)
    note(slots["bwd_points"] == 1 and slots["bwd_accumulate"] == slots["bwd_binning"] == slots["bwd_combine"] == 0,
         "want=2: exactly one point-gradient launch, nothing else (%s)" % slots)
    note(untouched(p2[0]), "want=2: grad_value buffer untouched")
    for e in errors(p2, points):                                                    # 1.
        note(False, "want=2 vs oracle: " + e)
    if inexact_points:                                                              # 3.
        # (a family that cannot meet the bitwise claim: the oracle tolerance above is its check; the figure is printed)
        worst = max((p2[i].double() - full2[i].double()).abs().max().item() for i in points)
        print("     want=2 vs full call, not claimed bitwise equal (%s): max |diff| = %.3e" % (inexact_points, worst))
    else:
        note(all(torch.equal(p2[i], full2[i]) for i in points),
             "want=2: bitwise equal to the point gradients of the full call")
    (rc, p2n), slots = profiled(lambda: call(case, want=POINTS, ws=None, state=None, null=(0,)))
    note(rc == 0, "want=2 with NULL grad_value / workspace / state returns 0 (%d)" % rc)
    note(slots["bwd_points"] == 1 and slots["bwd_accumulate"] == slots["bwd_binning"] == slots["bwd_combine"] == 0,
         "want=2 with NULLs: still exactly one point-gradient launch (%s)" % slots)
    note(all(torch.equal(p2n[i], p2[i]) for i in points), "want=2 with NULLs: same point gradients")

    # VALUE only
    pat = case.outputs(pattern=True)
    snap = state.clone() if state is not None else None
    (rc, p1), slots = profiled(lambda: call(case, want=VALUE, outs=pat, state=state))
    print("     want=1 launches: %s" % slots)
    note(rc == 0, "want=1 returns 0 (%d)" % rc)
    note(slots["bwd_points"] == 0 and slots["bwd_accumulate"] >= 1,
         "want=1: no point-gradient launch, an accumulate launch (%s)" % slots)
    note(all(untouched(p1[i]) for i in points), "want=1: location / weight gradient buffers untouched")
    if snap is not None:
        note(torch.equal(snap, state), "want=1: the state buffer is not written")
    for e in errors(p1, (0,)):                                                      # 1.
        note(False, "want=1 vs oracle: " + e)
    rc, p1n = call(case, want=VALUE, state=None, null=points)
    note(rc == 0, "want=1 with NULL point gradients returns 0 (%d)" % rc)
    for e in errors(p1n, (0,)):
        note(False, "want=1 with NULLs vs oracle: " + e)
    # ... and the full call still behaves
    rc, full3 = call(case, state=state)
    note(rc == 0 and all(torch.equal(full3[i], full2[i]) for i in points), "a full call afterwards: same point gradients")
    for e in errors(full3, (0,)):
        note(False, "full call afterwards, grad_value vs oracle: " + e)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------- 1-5: generic, fast atomic, gather / binned decoder
GENERIC = ((((6, 4), (3, 2)), 1, 2, 2, 2), (((6, 4), (3, 2)), 1, 2, 5, 2))          # shapes, B, H, C, Lq  (+ P per kind)

FAMILY_CASES = (
    [("generic", cfg, dt, v) for cfg in GENERIC for dt in (torch.float32, torch.float64) for v in (0, 1)] +
    [("decoder", DECODER, dt, v) for dt in (torch.float32, torch.bfloat16, torch.float16) for v in (0, 2)] +
    [("decoder", DECODER, torch.float32, 1)])            # the generic kernels forced on a shape the fast ones take


@pytest.mark.parametrize("kind", ["box", "instance"])
@pytest.mark.parametrize("family,cfg,dtype,variant", FAMILY_CASES,
                         ids=["%s-C%d-%s-variant%d" % (f, c[3], SUFFIX[d], v) for f, c, d, v in FAMILY_CASES])
def test_partial_backward_atomic_gather_binned(kind, family, cfg, dtype, variant):
    case, want, on_edge = seeded_case(kind, dtype, cfg + (P_OF[family][kind],))
    _blib().set_variant(variant)
    # The one family that cannot meet the bitwise claim of assertion 3: the fast atomic kernels (variant 2), instance
    # flavour.  There the full call and the POINTS-only call are two instantiations of bwd_fast_kernel (with and
    # without the grad_value atomics), both older than the partial backward and both left instruction for instruction
    # as they were.  The compiler contracts a * b + c into a fused multiply-add where the product has no other use; the
    # instance flavour's upstream term t = g * a_s + g_mask * a_l and the corner weights feed the atomics in one
    # instantiation and only the sums in the other, so the two round a few sums differently (last-bit differences,
    # measured below).  In the disassembly (float32, C = 32): 11 v_pk_fma_f32 + 11 v_pk_add_f32 with the atomics, 7 + 15
    # without; the box flavour has 7 + 11 either way.  The box flavour of the same kernels, the generic kernels and the gather / window-staged
    # kernels (one kernel, with or without riders) meet the claim.
    why = "two instantiations of bwd_fast_kernel<INST>, contracted differently" \
        if variant == 2 and kind == "instance" else ""
    run_family(case, lambda outs, which: oracle_errors(case, outs, want, on_edge, which), inexact_points=why)


# ------------------------------------------------------------- 1-5: the window-staged encoder kernels
@pytest.mark.parametrize("staged", [True, False], ids=["option11_on", "option11_off"])
@pytest.mark.parametrize("family", ["model", "border"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("lv", ["3lv", "4lv_odd"])
def test_partial_backward_encoder(lv, dtype, family, staged):
    from boxer_amd import ops
    inp = point_cases.make_dense_case(point_cases.LEVELS[lv], family, dtype=dtype)
    _blib().load().boxattn_set_option(OPT_DENSE, 2 if staged else 1)
    case = Case("box", dtype, inp["value"], inp["shapes"], inp["lsi"], inp["loc"], [inp["attn"]], inp["grad_out"])
    out = ops.box_attn_forward(inp["value"], inp["shapes"], inp["lsi"], inp["loc"], inp["attn"], 64)
    run_family(case, lambda outs, which: bench_errors(inp, out, outs, which))


# ------------------------------------------------------------- 6: the state of the one-pass fill
def test_partial_calls_leave_the_one_pass_state_alone():
    """Smallest shape of tests/test_gpu_onepass.py that fills its bins in one pass (900 queries on LEVELS4, bf16,
    16 channels a head).  full, full, VALUE-only, POINTS-only, full: the partial calls neither read nor write the
    state -- its bytes are the same before and after them -- and the last full call is one more one-pass call, no
    block redone, the oracle's tensors."""
    from boxer_amd import ops
    ops.release_workspaces()
    inp = point_cases.make_onepass_case(point_cases.LEVELS4, 900, dtype=torch.bfloat16, C=16, seed=3)
    ns = inp["dims"]["B"] * inp["dims"]["H"]
    v, sh, ls, loc, attn, go = (inp[k] for k in ("value", "shapes", "lsi", "loc", "attn", "grad_out"))
    point_cases.step(inp)
    out, grads = point_cases.step(inp)
    compare_rules.check_onepass(inp, out, grads, "second full call")
    before = point_cases.counters()
    assert before == (ns, 0), "the second full call on this shape is a one-pass call"
    snap = {k: st.clone() for k, st in ops._STATE.items()}
    for want in (VALUE, POINTS):
        out, plan = ops.box_attn_forward_train(v, sh, ls, loc, attn, 64)
        part = ops.box_attn_backward(v, sh, ls, loc, attn, go, 64, plan=plan, want=want)
        torch.cuda.synchronize()
        assert [g is None for g in part] == ([False, True, True] if want == VALUE else [True, False, False])
        for name, worst, tol in bench.parity_report(inp, out, [g if g is not None else torch.zeros_like(f)
                                                                for g, f in zip(part, grads)]):
            if name == "out" or part[("grad_value", "grad_loc", "grad_attn").index(name)] is not None:
                assert worst <= tol, "want=%d %s: worst %.3e > %.0e" % (want, name, worst, tol)
    # (the training forwards above add to the locality counters in the state's first 1 KiB; everything behind them --
    # one-pass counters, tickets, ranges -- is what the backward owns)
    assert set(snap) == set(ops._STATE)
    for k, st in ops._STATE.items():
        assert torch.equal(st[1024:], snap[k][1024:]), "a partial call wrote the state"
    assert point_cases.counters() == before
    out, grads, launches = point_cases.binning_launches(inp)
    compare_rules.check_onepass(inp, out, grads, "full call after the partial calls")
    assert launches == 0, "still the one-pass steady state: no count / scan / fill launch"
    assert point_cases.counters() == (before[0] + ns, before[1]), "exactly one more one-pass call, nothing redone"


# ------------------------------------------------------------- 7: errors
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64], ids=["f32", "bf16", "f64"])
@pytest.mark.parametrize("kind", ["box", "instance"])
def test_errors_return_invalid_value_and_launch_nothing(kind, dtype):
    case, _want, _edge = seeded_case(kind, dtype, DECODER + (P_OF["decoder"][kind],))
    points = tuple(range(1, case.n_out))

    def refused(what, **kw):
        pat = case.outputs(pattern=True)
        (rc, outs), slots = profiled(lambda: call(case, outs=pat, **kw))
        assert rc == 1, "%s: returned %d, not hipErrorInvalidValue" % (what, rc)
        assert not any(slots.values()), "%s: launched %s" % (what, slots)
        assert all(untouched(t) for i, t in enumerate(outs) if i not in kw.get("null", ())), what + ": wrote an output"

    for want in (0, 4, -1):
        refused("want=%d" % want, want=want)
    refused("want=1, grad_value NULL", want=VALUE, null=(0,))
    for i in points:
        refused("want=2, %s NULL" % GRAD_NAMES[kind][i], want=POINTS, null=(i,))
    if dtype == torch.bfloat16:
        # 16-bit VALUE-only on the atomic path: the workspace is the float32 accumulation buffer, B*S*H*C floats
        _blib().set_variant(2)
        B, S, H, C = case.dims[:4]
        small = torch.empty(B * S * H * C * 4 - 256, dtype=torch.uint8, device="cuda")
        refused("16-bit want=1, atomic path, workspace too small", want=VALUE, ws=small)
        rc, outs = call(case, want=VALUE, ws=torch.empty(B * S * H * C * 4, dtype=torch.uint8, device="cuda"))
        assert rc == 0


# ------------------------------------------------------------- 8: the autograd Functions
def _functions(kind, dtype):
    import boxer_amd
    table = {("box", torch.float32): boxer_amd.BoxAttnFunction, ("box", torch.bfloat16): boxer_amd.BoxAttnBF16Function,
             ("box", torch.float16): boxer_amd.BoxAttnF16Function,
             ("instance", torch.float32): boxer_amd.InstanceAttnFunction,
             ("instance", torch.bfloat16): boxer_amd.InstanceAttnBF16Function,
             ("instance", torch.float16): boxer_amd.InstanceAttnF16Function}
    return table[(kind, dtype)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", ["box", "instance"])
def test_functions_compute_what_autograd_asks_for(kind, dtype, monkeypatch):
    from boxer_amd import ops
    ops.release_workspaces()
    case, _want, _edge = seeded_case(kind, dtype, DECODER + (P_OF["decoder"][kind],))
    fn = _functions(kind, dtype)
    k = int(round(case.dims[6] ** 0.5))
    seen = {"want": [], "train": 0}
    bwd_name = "box_attn_backward" if kind == "box" else "instance_attn_backward"
    train_name = "box_attn_forward_train" if kind == "box" else "instance_attn_forward_train"
    real_bwd, real_train = getattr(ops, bwd_name), getattr(ops, train_name)

    def spy_bwd(*a, **kw):
        seen["want"].append(kw.get("want", 3))
        return real_bwd(*a, **kw)

    def spy_train(*a, **kw):
        seen["train"] += 1
        return real_train(*a, **kw)
    monkeypatch.setattr(ops, bwd_name, spy_bwd)
    monkeypatch.setattr(ops, train_name, spy_train)

    def run(mask):
        leaves = [t.detach().clone().requires_grad_(m) for t, m in zip([case.value, case.loc] + case.weights, mask)]
        value, loc, *weights = leaves
        if kind == "box":
            fn.apply(value, case.shapes, case.lsi, loc, weights[0], 64).backward(case.grad_out)
        else:
            shape6 = loc.shape[:4] + (k, k)
            w6 = [w.view(shape6) for w in weights]
            out, mask_out = fn.apply(value, case.shapes, case.lsi, loc, w6[0], w6[1], k, 64)
            torch.autograd.backward([out, mask_out], [case.grad_out, case.grad_mask.view_as(mask_out)])
        torch.cuda.synchronize()
        return [t.grad for t in leaves]

    n = len(case.weights) + 2
    ref = run((True,) * n)
    assert seen["want"] == [3] and all(g is not None for g in ref)
    tol_of = lambda t: {torch.float32: 1e-4, torch.bfloat16: 1e-2, torch.float16: 1e-3}[t.dtype]
    for bits in range(1, 2 ** n - 1):
        mask = tuple(bool(bits >> i & 1) for i in range(n))
        seen["want"], seen["train"] = [], 0
        grads = run(mask)
        assert seen["want"] == [(VALUE if mask[0] else 0) | (POINTS if any(mask[1:]) else 0)], (mask, seen)
        if not mask[0]:
            assert seen["train"] == 0, "value needs no gradient: the training forward must not run"
            assert len(ops._PARKED) == 0
        for i, (g, r, m) in enumerate(zip(grads, ref, mask)):
            assert (g is not None) == m, (mask, i)
            if m:
                assert g.dtype == r.dtype and g.shape == r.shape
                err = (g.double() - r.double()).abs().max().item()
                scale = max(1.0, r.double().abs().max().item())
                print("mask %s grad %d: max |diff| / scale = %.3e" % (mask, i, err / scale))
                assert err <= tol_of(r) * scale, (mask, i, err, scale)
    assert len(ops._PARKED) == 0


# ------------------------------------------------------------- 9: a module with a frozen memory
@pytest.mark.parametrize("kind", ["box", "instance"])
def test_module_with_frozen_value_path_runs_the_short_backward(kind):
    """BoxAttention / InstanceAttention at the decoder shape with value_proj frozen and a value that needs no
    gradient: nothing of the grad_value half is launched, and the parameters that do train get the gradients of
    the unfrozen run (the point gradients are the same kernel on the same inputs: bit for bit)."""
    import boxer_amd
    from boxer_amd import ops
    ops.release_workspaces()
    shapes, B, H, C, Lq = DECODER
    torch.manual_seed(5)
    if kind == "box":
        mod = boxer_amd.BoxAttention(H * C, len(shapes), H, 2)
    else:
        mod = boxer_amd.InstanceAttention(H * C, len(shapes), H, 4)
        mod.inferencing = False
    mod = mod.cuda()
    with torch.no_grad():
        for p in (mod.linear_box_weight, mod.linear_attn_weight, mod.linear_attn_bias):
            p.normal_(0, 0.1)
    v_shape = torch.tensor(shapes, dtype=torch.long, device="cuda")
    v_start = torch.cat((v_shape.new_zeros(1), v_shape.prod(1).cumsum(0)[:-1]))
    S = int(v_shape.prod(1).sum())
    query, value = torch.randn(B, Lq, H * C, device="cuda"), torch.randn(B, S, H * C, device="cuda")
    ref = torch.cat([0.1 + 0.8 * torch.rand(B, Lq, 2, device="cuda"), 0.1 + 0.4 * torch.rand(B, Lq, 2, device="cuda")], -1)
    seeds = {}

    def step(value):
        mod.zero_grad(set_to_none=True)
        res = mod(query, value, v_shape, None, v_start, None, ref)
        outs = [res[0]] if kind == "box" else [res[0], res[1]]
        for i, o in enumerate(outs):
            seeds.setdefault(i, torch.randn_like(o))
        torch.autograd.backward(outs, [seeds[i] for i in range(len(outs))])
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}

    full = step(value.clone().requires_grad_())
    assert "value_proj.weight" in full
    mod.value_proj.requires_grad_(False)
    frozen, slots = profiled(lambda: step(value.clone()))
    print("launches with the value path frozen: %s" % slots)
    assert slots["bwd_points"] == 1
    assert slots["bwd_accumulate"] == 0 and slots["bwd_binning"] == 0 and slots["bwd_combine"] == 0, slots
    assert not any(n.startswith("value_proj") for n in frozen)
    names = [n for n in full if n.startswith(("linear_box_", "linear_attn_", "out_proj"))]
    assert len(names) == 6
    for n in names:
        assert torch.equal(frozen[n], full[n]), n
    assert len(ops._PARKED) == 0
