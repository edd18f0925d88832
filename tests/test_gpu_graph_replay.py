"""GPU: every training route captured in a HIP graph and replayed on NEW inputs -- the way ``bench_train.py --graph`` runs
the operator, and the mode in which the host layer behaves differently: boxer_amd/ops.py keeps no state buffer or
workspace it created while the stream captured, never touches the locality event, never queues a read of the counters;
the library decides from its host-side note of the state ("cold" / "ranges planned") which launches a call makes, once,
at capture time, while the device-side state moves on under every replay.

Every test follows one pattern (graph_cases.replay_on): two or three input sets of one geometry, the capture on the
first, a replay on each in turn with a return to the first, a synchronisation after each, and what the graph produced
for a set held to the rule the eager test of the same route uses on the same kind of case -- the float64 models of
tests/error_bounds.py (``eb.hold`` / ``eb.hold_all``) or, for the per-point encoder step, ``compare_rules.check_onepass``
against the CPU oracle.  The expectation is the model or the oracle on the inputs of THAT replay, never another run of
the library.  On top of it the outputs documented as bitwise reproducible equal an eager call on the same inputs, made
after the replay on the default stream; ``grad_value`` of the binned and of the atomic route is held to its bound only.

Both ways a step can meet its capture (graph_cases.capture):
  "same_stream"  warmed up on the stream it is captured on: state buffer, workspace and locality entry are the warmed
                 ones, the library's note of the state says "ranges planned", and what is captured for the encoder step
                 is the ONE-PASS fill -- the counters in the state buffer say so: one chain per (image, head) slice and
                 replay, blocks redone on the first replay whose locations outgrow the planned ranges, none on the next;
  "new_stream"   captured on a stream that has run nothing (bench.graph_step, bench_train.graphed_step): the state
                 buffer is a ``torch.zeros`` node of the graph, handed over as fresh, so every replay runs the COLD
                 two-pass step on a buffer its own memset has just cleared.  These tests also hold the lifetime rules:
                 the capture leaves no entry in a table of boxer_amd.ops, and after the graph is gone and the cached
                 buffers are dropped an eager step on the default stream is still right.
The route of every case is asserted with the library's queries, so that no test passes on a fall-back."""
import pytest
import torch

import boxes_cases
import error_bounds as eb
import graph_cases as gc
import point_cases
from boxes_cases import LEAVES, STAGED_SPLIT
from compare_rules import check_f16, check_onepass
from oracle import boxattn_oracle as oc
from point_cases import INST_NAMES, LEVELS_A, SHAPE_A, box_tensors, counters, inst_tensors
from route_vocab import (ACC_SPLIT, ACC_TR, ACC_VALU, BF16, DTYPES, F16, F32, GATHER, REC_POINT, STAGED, WIDE, dev, routes,
                         split_of, take_family)

pytestmark = pytest.mark.gpu

EACH_MODE = pytest.mark.parametrize("mode", gc.MODES)
EACH_TYPE = pytest.mark.parametrize("dtype", sorted(DTYPES))


@pytest.fixture(autouse=True)
def _fresh_tables(monkeypatch):
    """No buffer of an earlier test, and one kernel family per shape for the whole test (outputs are compared bit for
    bit with an eager call: ops._Locality may otherwise move a shape from the window-staged to the gather kernels
    between the two; its host code -- the event, the queued reads -- still runs)."""
    from boxer_amd import ops
    ops.release_workspaces()
    monkeypatch.setattr(ops._Locality, "enabled", False)
    yield
    ops.release_workspaces()


# ------------------------------------------------------------------ a, b: the per-point box step of the encoder
ORDER_ABBCA, onepass_sets = gc.ORDER_ABBCA, gc.onepass_sets


def oracle_out(inp):
    f64 = point_cases.f64
    return oc.box_attn_forward(f64(inp["value"]), inp["shapes"].cpu().numpy(), inp["lsi"].cpu().numpy(), f64(inp["loc"]),
                               f64(inp["attn"]))


def check_point_step(inp, out, grads, what):
    """float32 / bf16: compare_rules.check_onepass; f16 (bench.parity_report has no f16 tolerance): the f16 suite's
    check_f16 for ``out``, point_cases.check_oracle (check_f16 and the per-element bound) for the gradients."""
    if inp["value"].dtype == F16:
        check_f16(out, oracle_out(inp), what + ": out")
        point_cases.check_oracle(inp, grads, what)
    else:
        check_onepass(inp, out, grads, what)


def same_bits(got, eager, names, what):
    for name, a, b in zip(names, got, eager):
        assert a.dtype == b.dtype and torch.equal(a, b), "%s: %s differs from the eager call on the same inputs" % (what, name)


def assert_encoder_route(t):
    from boxer_amd import ops
    fwd, acc, rec = routes(t)
    assert fwd in (STAGED, GATHER), "forward route %d: not an encoder family" % fwd
    assert acc == (ACC_SPLIT if t["value"].dtype == F32 else ACC_TR), "accumulate kind %d: no matrix-core accumulate" % acc
    return fwd, acc, rec


@EACH_MODE
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("lq", ["S", 900], ids=["encoder", "dense_decoder"])
def test_box_step_train_entry(lq, dtype, mode, monkeypatch):
    """ops.box_attn_forward_train -> ops.box_attn_backward with the plan handed over, replayed on A, B, B, C, A.

    Expectation, from boxattn_host_plan.h (state_check, spec_ok) and boxattn_capi.hip (launch_bwd_routed) before any
    run: "same_stream": the three warm-up calls leave the stream's state buffer in ops._STATE with its ranges planned by
    A and the library's note "learned", so the captured backward is the one-pass fill (spec_warm) -- every replay adds
    B * H to the chain count of that buffer; replay 0 (A on A's ranges) redoes nothing, replay 1 (B on A's ranges) redoes
    blocks, replay 2 (B on the ranges replay 1 planned) redoes none.  "new_stream": the forward's and the backward's
    call each create a state buffer inside the capture (ops._state_buffer keeps neither) and hand it over as fresh, so
    the library's note says "cold": the two-pass step is captured, on buffers the graph zeroes in every replay -- their
    one-pass counters stay (0, 0)."""
    from boxer_amd import ops
    sets = onepass_sets(lq, dtype)
    static = gc.clone(sets[0])
    assert_encoder_route(static)
    ns = static["dims"]["B"] * static["dims"]["H"]

    def step():
        v, sh, ls, loc, attn, go = (static[k] for k in ("value", "shapes", "lsi", "loc", "attn", "grad_out"))
        out, plan = ops.box_attn_forward_train(v, sh, ls, loc, attn, 64)
        return out, ops.box_attn_backward(v, sh, ls, loc, attn, go, 64, plan=plan)

    def check(i, kept, what):
        out, grads = kept
        check_point_step(sets[i], out, grads, what)
        e_out, e_grads = point_cases.step(sets[i])
        same_bits([out, grads[1], grads[2]], [e_out, e_grads[1], e_grads[2]], ("out", "grad_loc", "grad_attn"), what)

    seen, in_capture, cold = [], [], []
    make_state = ops._state_buffer

    def spy(key, device, nbytes):
        buf = make_state(key, device, nbytes)
        if torch.cuda.is_current_stream_capturing() and getattr(buf, "_boxattn_fresh", False):
            in_capture.append(buf)                # (created by this call: a node of the graph, alive with it)
        return buf
    monkeypatch.setattr(ops, "_state_buffer", spy)

    def around(pos, replay):
        before = counters()
        replay()
        seen.append((before, counters()))
        for buf in in_capture:
            cold.append(tuple(buf[point_cases.STAT_OFF:point_cases.STAT_OFF + 16].view(torch.int64).tolist()))
        if pos == len(ORDER_ABBCA) - 1:
            del in_capture[:]                     # (nothing of the graph's pool outlives the graph here)

    gc.replay_on(mode, step, static, sets, ORDER_ABBCA, check, around_replay=around)
    if mode == "new_stream":
        # the forward's and the backward's call each made a state buffer of their own inside the capture, both handed
        # over as fresh: every replay zeroes them and runs the two-pass step; the one-pass chain never runs
        assert len(cold) == 2 * len(ORDER_ABBCA), "state buffers created inside the capture: %d" % (len(cold) // len(ORDER_ABBCA))
        assert all(c == (0, 0) for c in cold), "one-pass counters of the captured state buffers: %s" % cold
    else:
        assert not cold, "a state buffer was created inside the capture although the stream was warmed up"
    if mode == "same_stream":
        chains = [after[0] - before[0] for before, after in seen]
        redone = [after[1] - before[1] for before, after in seen]
        print("chain counts per replay %s, blocks redone per replay %s" % (chains, redone))
        assert chains == [ns] * len(seen), "the one-pass fill was not what was captured: chains per replay %s" % chains
        assert redone[0] == 0, "A on the ranges A's warm-up planned: %s" % redone
        assert redone[1] > 0, "B on A's ranges: no block outgrew its range? %s" % redone
        assert redone[2] == 0, "B on the ranges the replay before planned from B: %s" % redone


def function_of(dtype):
    import boxer_amd as ba
    return {F32: ba.BoxAttnFunction, BF16: ba.BoxAttnBF16Function, F16: ba.BoxAttnF16Function}[dtype]


def function_step(fn, static, leaves):
    def step():
        out = fn.apply(static["value"], static["shapes"], static["lsi"], static["loc"], static["attn"], 64)
        grads = dict(zip(leaves, torch.autograd.grad(out, [static[n] for n in leaves], static["grad_out"])))
        return out.detach(), [grads.get(n) for n in ("value", "loc", "attn")]
    return step


def assert_nothing_parked():
    from boxer_amd import ops
    assert len(ops._PARKED) == 0, "a plan stayed parked: %r" % (list(ops._PARKED),)


@EACH_MODE
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_box_step_reference_functions(dtype, mode):
    """The reference's pair of Functions on the encoder geometry, every input requiring a gradient, forward and
    ``torch.autograd.grad`` inside the capture; nothing is parked after the captured step or after any replay."""
    sets = onepass_sets("S", dtype)
    static = gc.clone(sets[0], leaves=("value", "loc", "attn"))
    assert_encoder_route(static)
    fn = function_of(dtype)
    step = function_step(fn, static, ("value", "loc", "attn"))

    def check(i, kept, what):
        out, grads = kept
        check_point_step(sets[i], out, grads, what)
        eager = gc.clone(sets[i], leaves=("value", "loc", "attn"))
        e_out, e_grads = function_step(fn, eager, ("value", "loc", "attn"))()
        torch.cuda.synchronize()
        same_bits([out, grads[1], grads[2]], [e_out, e_grads[1], e_grads[2]], ("out", "grad_loc", "grad_attn"), what)
        assert_nothing_parked()

    gc.replay_on(mode, step, static, sets, ORDER_ABBCA, check, after_capture=assert_nothing_parked)


@EACH_MODE
def test_box_step_with_a_plan_parked_inside_the_capture(mode):
    """The reference's two calls with nothing but the tensors between them (plan hand-over off, two-pass riders): the
    captured forward parks the plan its launch prepared, the captured backward takes it -- the table is empty after the
    capture and after every replay, and the plan the graph replays is rebuilt from each replay's locations."""
    from boxer_amd import _lib, functions, ops
    _lib.set_option("riders", 4)
    sets = onepass_sets("S", F32)[:2]            # (float32: point records in every configuration, so a plan is built)
    static = gc.clone(sets[0], leaves=("value", "loc", "attn"))
    fn = function_of(F32)
    step = function_step(fn, static, ("value", "loc", "attn"))
    old = functions.set_plan_in_forward(False)
    try:
        static_out = fn.apply(static["value"], static["shapes"], static["lsi"], static["loc"], static["attn"], 64)
        assert len(ops._PARKED) == 1, "this shape parks no plan under the two-pass riders: the test needs another one"
        ops._PARKED.clear()
        del static_out

        def check(i, kept, what):
            check_point_step(sets[i], kept[0], kept[1], what)
            assert_nothing_parked()

        gc.replay_on(mode, step, static, sets, (0, 1, 0), check, after_capture=assert_nothing_parked)
    finally:
        functions.set_plan_in_forward(old)


# ------------------------------------------------------------------ c: the instance attention step
SHAPE_C16 = dict(levels=LEVELS_A, B=2, H=3, C=16, Lq=64, k=4)       # test_gpu_instance_accumulate16's smallest case


@EACH_MODE
@pytest.mark.parametrize("shape,dtype,key", [("A", "f32", 0), ("A", "bf16", 2), ("A", "f16", 2), ("C16", "bf16", 2)],
                         ids=["A_f32", "A_bf16_tr", "A_f16_tr", "C16_bf16_tr"])
def test_instance_step(shape, dtype, key, mode):
    """ops.instance_attn_forward_train -> ops.instance_attn_backward (its plan handed over) on point_cases.SHAPE_A and on
    the smallest case of test_gpu_instance_accumulate16 that takes the matrix-core accumulate; the second set is the
    same builder from another seed: locations, both weight tensors, value and both upstream gradients.  The binned
    backward is required and the 16-bit accumulate put on the matrix cores as test_gpu_error_bounds does."""
    from boxer_amd import _lib, ops
    dt = DTYPES[dtype]
    inputs = gc.instance_sets(SHAPE_A if shape == "A" else SHAPE_C16, dtype, (5, 6) if shape == "A" else (7, 8))
    sets = [inst_tensors(inp, dt) for inp in inputs]
    static = gc.clone(sets[0])
    _lib.set_option("inst_acc16", key)
    _lib.set_variant(3)
    fwd, acc, rec = routes(static, instance=True)
    assert acc == (ACC_TR if key == 2 else ACC_VALU) and rec == REC_POINT, (acc, rec)

    def step():
        a = [static[k] for k in ("value", "shapes", "lsi", "loc", "attn", "level_w")]
        (out, mask), plan = ops.instance_attn_forward_train(*a, 64)
        return [out, mask] + ops.instance_attn_backward(*a, static["grad_out"], static["grad_mask"], 64, plan=plan)

    def check(i, kept, what):
        eb.hold_all(dict(zip(INST_NAMES, kept)), eb.reference_of(inputs[i]), dt, split_of(acc, dt),
                    "instance step %s %s, %s" % (shape, dtype, what))

    gc.replay_on(mode, step, static, sets, (0, 1, 0), check)


# ------------------------------------------------------------------ d: the four Functions from boxes
def boxes_function_inputs(s):
    """The leaves and operands of one input set (boxes_cases.function_inputs) with its upstream gradients."""
    x = boxes_cases.function_inputs(s["g"])
    x["gout"] = dev(s["gout"]).float()
    if s.get("gmask") is not None:
        x["gmask"] = dev(s["gmask"]).float()
    return x


def run_box_function(fn, x, dt):
    value = x["value"] if dt == torch.float32 else x["value"].to(dt)
    vr = None if x["vr"] is None else x["vr"].view(-1, x["off"].size(3), 2)
    return fn.apply(value, x["shapes"], x["lsi"], x["ref"], x["off"], x["kidx"], vr, x["logits"], x["mode"])


def box_function_step(fn, x, dt, leaves=LEAVES):
    def step():
        out = run_box_function(fn, x, dt)
        grads = torch.autograd.grad(out, [x[n] for n in leaves], x["gout"].to(out.dtype))
        return out.detach(), dict(zip(leaves, grads))
    return step


def accumulate_split(dims, dt):
    """The weight-split term of grad_value from the binned backward, as test_gpu_box_boxes_value holds
    BoxAttnBoxesFunction's: that of the accumulate kind the library names for the shape."""
    from boxer_amd import _lib
    acc = _lib.bwd_accumulate_kind(4 if dt == torch.float32 else 2, 0, dims)
    return split_of(acc, dt) if acc >= 0 else "none"


def hold_box_function(s, kept, dt, out_split, value_split, what, leaves=LEAVES):
    out, grads = kept
    ref = s["ref"]
    assert ref["edge_share"] <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (what, 100 * ref["edge_share"])
    assert out.dtype == dt
    worst = {"out": eb.hold(out, ref["out"], dt, out_split, what + ": out")}
    if "value" in leaves:
        worst["grad_value"] = eb.hold(grads["value"], s["grad_value"], dt, value_split, what + ": grad_value")
    for leaf, name in (("off", "grad_offsets"), ("logits", "grad_logits")):
        if leaf in leaves:
            assert grads[leaf].dtype == torch.float32
            worst[name] = eb.hold(grads[leaf], ref[name], torch.float32, "none", "%s: %s" % (what, name))
    print("%s: worst err / bound %s" % (what, ", ".join("%s %.3f" % kv for kv in worst.items())))


def box_function_test(fn, sets, dt, mode, out_split, value_split, what, leaves=LEAVES, bitwise=("ref", "off", "logits")):
    static = boxes_function_inputs(sets[0])
    for n in LEAVES:
        static[n].requires_grad_(n in leaves)
    step = box_function_step(fn, static, dt, leaves)
    loaded = [boxes_function_inputs(s) for s in sets]

    def check(i, kept, where):
        hold_box_function(sets[i], kept, dt, out_split, value_split, "%s, %s" % (what, where), leaves)
        for n in LEAVES:
            loaded[i][n].requires_grad_(n in leaves)
        e_out, e_grads = box_function_step(fn, loaded[i], dt, leaves)()
        torch.cuda.synchronize()
        names = ["out"] + [n for n in bitwise if n in leaves]
        same_bits([kept[0]] + [kept[1][n] for n in names[1:]], [e_out] + [e_grads[n] for n in names[1:]], names,
                  "%s, %s" % (what, where))

    gc.replay_on(mode, step, static, loaded, (0, 1, 0), check)


GATHER_FLAVOUR = {0: ((0, 4), False, True), 1: ((1, 5), False, True)}


@EACH_MODE
@EACH_TYPE
@pytest.mark.parametrize("angle_mode", [0, 1])
@pytest.mark.parametrize("geometry", ["model", "encoder"])
def test_box_boxes_function(geometry, angle_mode, dtype, mode):
    """BoxAttnBoxesFunction: ops.box_attn_forward_boxes, ops.box_attn_backward_boxes and grad_value from the binned
    backward on the grid and weights rebuilt inside the captured backward."""
    from boxer_amd import BoxAttnBoxesFunction, ops
    dt = DTYPES[dtype]
    assert boxes_cases.eligible(geometry, 32, dt), "not eligible: %s %s" % (geometry, dtype)
    sets = gc.box_sets("gather", geometry, GATHER_FLAVOUR[angle_mode])
    B, S, H, C, L, Lq, P = sets[0]["g"]["dims"]
    assert ops.box_forward_boxes_ok(torch.empty(B, S, H, C, dtype=dt, device="cuda"), L, Lq, P)
    box_function_test(BoxAttnBoxesFunction, sets, dt, mode, "none", accumulate_split(sets[0]["g"]["dims"], dt),
                      "BoxAttnBoxesFunction %s angle=%d %s" % (geometry, angle_mode, dtype))


STAGED_CASES = {"four_levels": ("local", ((1, 5), True, False)), "tiny_levels": ("scattered", ((0, 4), False, True))}


def assert_staged(g, dt):
    from boxer_amd import ops
    B, S, H, C, L, Lq, P = g["dims"]
    value = torch.empty(B, S, H, C, dtype=dt, device="cuda")
    shapes, lsi = dev(g["shapes"]), dev(g["lsi"])
    assert ops.box_forward_boxes_staged_ok(value, shapes, lsi, Lq, P) and \
        ops.box_backward_boxes_staged_ok(value, shapes, lsi, Lq, P), "not eligible for the staged calls: %s" % (g["dims"],)


@EACH_MODE
@EACH_TYPE
@pytest.mark.parametrize("geometry", sorted(STAGED_CASES))
def test_box_boxes_staged_function(geometry, dtype, mode):
    """BoxAttnBoxesStagedFunction: the window-staged forward and point-gradient kernels from boxes; its offset, window
    and logit gradients are bitwise reproducible."""
    from boxer_amd import BoxAttnBoxesStagedFunction
    dt = DTYPES[dtype]
    family, flavour = STAGED_CASES[geometry]
    sets = gc.box_sets("staged", geometry, flavour, family)
    assert_staged(sets[0]["g"], dt)
    box_function_test(BoxAttnBoxesStagedFunction, sets, dt, mode, STAGED_SPLIT[dtype],
                      accumulate_split(sets[0]["g"]["dims"], dt),
                      "BoxAttnBoxesStagedFunction %s %s %s" % (geometry, family, dtype))


def assert_value_route(g, dt):
    from boxer_amd import ops
    B, S, H, C, L, Lq, P = g["dims"]
    assert ops.box_backward_boxes_value_ok(torch.empty(B, S, H, C, dtype=dt, device="cuda"), L, Lq, P), \
        "not eligible for the value route: %s" % (g["dims"],)


@EACH_MODE
@EACH_TYPE
def test_box_boxes_value_function(dtype, mode):
    """BoxAttnBoxesValueFunction: the whole backward one ops.box_attn_backward_boxes_value call, grad_value scattered with
    float32 atomics (held to its bound only, split "none"), the other three bitwise reproducible."""
    from boxer_amd import BoxAttnBoxesValueFunction
    dt = DTYPES[dtype]
    sets = gc.box_sets("gather", "model", GATHER_FLAVOUR[1])
    assert_value_route(sets[0]["g"], dt)
    box_function_test(BoxAttnBoxesValueFunction, sets, dt, mode, "none", "none",
                      "BoxAttnBoxesValueFunction model %s" % dtype)


def run_inst_function(x, k, dt):
    from boxer_amd import InstanceAttnBoxesFunction
    value = x["value"] if dt == torch.float32 else x["value"].to(dt)
    vr = None if x["vr"] is None else x["vr"].view(-1, x["off"].size(3), 2)
    return InstanceAttnBoxesFunction.apply(value, x["shapes"], x["lsi"], x["ref"], x["off"], x["kidx"], vr, x["logits"], k)


def inst_function_inputs(s, k):
    g = s["g"]
    leaf = lambda a: dev(a).float().requires_grad_()
    x = dict(value=leaf(g["value"]), ref=leaf(g["ref"]), off=leaf(g["off"]), logits=leaf(g["logits"]),
             shapes=dev(g["shapes"]), lsi=dev(g["lsi"]), kidx=boxes_cases.inst_kernel_indices(k),
             vr=None if g["vr"] is None else dev(g["vr"]), gout=dev(s["gout"]).float())
    if s["gmask"] is not None:
        x["gmask"] = dev(s["gmask"]).float()
    return x


def inst_function_step(x, k, dt):
    def step():
        out, mask = run_inst_function(x, k, dt)
        leaves = [x[n] for n in LEAVES]
        if "gmask" in x:
            grads = torch.autograd.grad([out, mask], leaves, [x["gout"].to(dt), x["gmask"].to(dt).view(mask.shape)])
        else:
            grads = torch.autograd.grad(out, leaves, x["gout"].to(dt))
        return out.detach(), mask.detach(), dict(zip(LEAVES, grads))
    return step


@EACH_MODE
@EACH_TYPE
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask_used", "mask_unused"])
@pytest.mark.parametrize("k", [4, 14])
def test_instance_boxes_function(k, with_mask, dtype, mode):
    """InstanceAttnBoxesFunction on "five_levels": ops.instance_attn_forward_boxes, ops.instance_attn_backward_boxes (a mask
    output the loss did not use reaches it as NULL) and grad_value from the binned backward on rebuilt per-point
    tensors."""
    from boxer_amd import _lib, ops
    dt = DTYPES[dtype]
    sets = gc.inst_sets("five_levels", k, False, True, with_mask)
    B, S, H, C, L, Lq = sets[0]["g"]["dims"]
    probe = torch.empty(B, S, H, C, dtype=dt, device="cuda")
    assert ops.forward_boxes_ok(probe, L, Lq, k) and ops.backward_boxes_ok(probe, L, Lq, k), "not eligible"
    acc = _lib.bwd_accumulate_kind(4 if dt == torch.float32 else 2, int(with_mask), (B, S, H, C, L, Lq, k * k))
    value_split = split_of(acc, dt) if acc >= 0 else "none"
    static = inst_function_inputs(sets[0], k)
    loaded = [inst_function_inputs(s, k) for s in sets]
    step = inst_function_step(static, k, dt)
    title = "InstanceAttnBoxesFunction five_levels k=%d mask=%d %s" % (k, with_mask, dtype)

    def check(i, kept, where):
        out, mask, grads = kept
        ref, what = sets[i]["ref"], "%s, %s" % (title, where)
        assert ref["edge_share"] <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (what, 100 * ref["edge_share"])
        worst = {"out": eb.hold(out, ref["out"], dt, "none", what + ": out")}
        if with_mask:
            worst["mask_out"] = eb.hold(mask, ref["mask_out"], dt, "none", what + ": mask_out")
        worst["grad_value"] = eb.hold(grads["value"], sets[i]["grad_value"], dt, value_split, what + ": grad_value")
        for leaf, name in (("off", "grad_offsets"), ("logits", "grad_logits")):
            worst[name] = eb.hold(grads[leaf], ref[name], torch.float32, "none", "%s: %s" % (what, name))
        print("%s: worst err / bound %s" % (what, ", ".join("%s %.3f" % kv for kv in worst.items())))
        e_out, e_mask, e_grads = inst_function_step(loaded[i], k, dt)()
        torch.cuda.synchronize()
        same_bits([out, mask] + [grads[n] for n in ("ref", "off", "logits")],
                  [e_out, e_mask] + [e_grads[n] for n in ("ref", "off", "logits")],
                  ("out", "mask_out", "grad_ref", "grad_offsets", "grad_logits"), what)

    gc.replay_on(mode, step, static, loaded, (0, 1, 0), check)


# ------------------------------------------------------------------ e: a partial backward inside a graph
def encoder_point_sets(dtype):
    """Two seeds of the odd-map encoder case of test_gpu_error_bounds (references computed once, shared)."""
    return [point_cases.encoder_input("model", dtype, seed) for seed in point_cases.ENCODER_SEEDS[:2]]


@EACH_MODE
@EACH_TYPE
@pytest.mark.parametrize("frozen", ["value", "points"])
def test_partial_backward_of_the_per_point_functions(frozen, dtype, mode):
    """A frozen ``value``: the location and weight gradients alone -- one launch, no workspace, no state; frozen locations
    and weights: grad_value alone (two-pass binning, the state neither read nor written)."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    inputs = encoder_point_sets(dtype)
    sets = [box_tensors(inp, dt) for inp in inputs]
    leaves = ("loc", "attn") if frozen == "value" else ("value",)
    static = gc.clone(sets[0], leaves=leaves)
    fwd, acc, rec = routes(static)
    assert fwd in (STAGED, GATHER) and acc != ACC_VALU, (fwd, acc)
    fn = function_of(dt)
    step = function_step(fn, static, leaves)
    names = ("grad_value", "grad_loc", "grad_attn")
    out_split = eb.store_name(dt) if fwd == STAGED and dt != F32 else "none"

    def check(i, kept, what):
        out, grads = kept
        got = dict(out=out, **{n: t for n, t in zip(names, grads) if t is not None})
        assert sorted(got) == sorted(("out",) + (names[1:] if frozen == "value" else names[:1])), sorted(got)
        eb.hold_all(got, eb.reference_of(inputs[i]), dt, split_of(acc, dt), "frozen %s %s, %s" % (frozen, dtype, what),
                    splits={"out": out_split})
        eager = gc.clone(sets[i], leaves=leaves)
        e_out, e_grads = function_step(fn, eager, leaves)()
        torch.cuda.synchronize()
        same = [(n, a, b) for n, a, b in zip(names[1:], grads[1:], e_grads[1:]) if a is not None]
        same_bits([out] + [a for _, a, _ in same], [e_out] + [b for _, _, b in same], ["out"] + [n for n, _, _ in same], what)

    gc.replay_on(mode, step, static, sets, (0, 1, 0), check)
    if frozen == "value":
        assert not ops._WORKSPACE, "the point gradients alone took a workspace: %r" % (list(ops._WORKSPACE),)


@EACH_MODE
@EACH_TYPE
@pytest.mark.parametrize("want", [1, 2])
def test_partial_backward_of_the_value_function(want, dtype, mode):
    """BoxAttnBoxesValueFunction with ``want`` 1 (frozen heads: grad_value alone) and 2 (a frozen ``value``)."""
    from boxer_amd import BoxAttnBoxesValueFunction
    dt = DTYPES[dtype]
    sets = gc.box_sets("gather", "model", GATHER_FLAVOUR[1])
    assert_value_route(sets[0]["g"], dt)
    box_function_test(BoxAttnBoxesValueFunction, sets, dt, mode, "none", "none",
                      "BoxAttnBoxesValueFunction want=%d model %s" % (want, dtype),
                      leaves=("value",) if want == 1 else ("ref", "off", "logits"))


# ------------------------------------------------------------------ f: the one-launch inference forwards
def forward_test(mode, static, loaded, call, check):
    def step():
        with torch.no_grad():
            return call(static)
    gc.replay_on(mode, step, static, loaded, (0, 1, 0), check)


def boxes_operands(x, dt):
    return dict(value=x["value"].detach().to(dt), shapes=x["shapes"], lsi=x["lsi"], ref=x["ref"].detach(),
                off=x["off"].detach(), kidx=x["kidx"], vr=x["vr"], logits=x["logits"].detach(), mode=x.get("mode", 0))


@EACH_MODE
@EACH_TYPE
@pytest.mark.parametrize("route", ["gather", "staged"])
def test_box_forward_from_boxes(route, dtype, mode):
    """ops.box_attn_forward_boxes ("model") and ops.box_attn_forward_boxes_staged ("tiny_levels") under no_grad."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    if route == "gather":
        sets, fn, split = gc.box_sets("gather", "model", GATHER_FLAVOUR[1]), ops.box_attn_forward_boxes, "none"
        B, S, H, C, L, Lq, P = sets[0]["g"]["dims"]
        assert ops.box_forward_boxes_ok(torch.empty(B, S, H, C, dtype=dt, device="cuda"), L, Lq, P)
    else:
        family, flavour = STAGED_CASES["tiny_levels"]
        sets, fn, split = gc.box_sets("staged", "tiny_levels", flavour, family), ops.box_attn_forward_boxes_staged, \
            STAGED_SPLIT[dtype]
        assert_staged(sets[0]["g"], dt)
    loaded = [boxes_operands(boxes_function_inputs(s), dt) for s in sets]
    static = gc.clone(loaded[0])
    call = lambda a: fn(a["value"], a["shapes"], a["lsi"], a["ref"], a["off"], a["kidx"], a["vr"], a["logits"], a["mode"])

    def check(i, out, what):
        assert out.dtype == dt
        eb.hold(out, sets[i]["ref"]["out"], dt, split, "%s forward from boxes %s, %s" % (route, dtype, what))
        with torch.no_grad():
            eager = call(loaded[i])
        torch.cuda.synchronize()
        same_bits([out], [eager], ["out"], what)

    forward_test(mode, static, loaded, call, check)


@EACH_MODE
@EACH_TYPE
@pytest.mark.parametrize("need_mask", [True, False], ids=["mask", "no_mask"])
def test_instance_forward_from_boxes(need_mask, dtype, mode):
    """ops.instance_attn_forward_boxes with and without the mask output ("five_levels", k = 4)."""
    from boxer_amd import ops
    dt, k = DTYPES[dtype], 4
    sets = gc.inst_sets("five_levels", k, False, True, True)
    B, S, H, C, L, Lq = sets[0]["g"]["dims"]
    assert ops.forward_boxes_ok(torch.empty(B, S, H, C, dtype=dt, device="cuda"), L, Lq, k)
    loaded = [boxes_operands(inst_function_inputs(s, k), dt) for s in sets]
    static = gc.clone(loaded[0])
    call = lambda a: ops.instance_attn_forward_boxes(a["value"], a["shapes"], a["lsi"], a["ref"], a["off"], a["kidx"],
                                                     a["vr"], a["logits"], k, need_mask)

    def check(i, kept, what):
        out, mask = kept
        assert (mask is None) == (not need_mask)
        what = "instance forward from boxes %s, %s" % (dtype, what)
        eb.hold(out, sets[i]["ref"]["out"], dt, "none", what + ": out")
        if need_mask:
            eb.hold(mask, sets[i]["ref"]["mask_out"], dt, "none", what + ": mask_out")
        with torch.no_grad():
            e_out, e_mask = call(loaded[i])
        torch.cuda.synchronize()
        same_bits([out] + ([mask] if need_mask else []), [e_out] + ([e_mask] if need_mask else []), ["out", "mask_out"], what)

    forward_test(mode, static, loaded, call, check)


@EACH_MODE
@EACH_TYPE
def test_wave_per_pair_forward(dtype, mode):
    """ops.box_attn_forward on the wave-per-pair kernels: test_gpu_wide_box_forward's smallest case (P = 36)."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    inputs = [point_cases.wide_input(36), gc.reseeded(point_cases.wide_input, 1, 36)]
    loaded = [box_tensors(inp, dt) for inp in inputs]
    static = gc.clone(loaded[0])
    take_family(static["value"], static["loc"], static["shapes"], static["lsi"], WIDE)
    call = lambda a: ops.box_attn_forward(a["value"], a["shapes"], a["lsi"], a["loc"], a["attn"], 64)

    def check(i, out, what):
        eb.hold_all(dict(out=out), eb.reference_of(inputs[i]), dt, what="wave-per-pair forward %s, %s" % (dtype, what))
        with torch.no_grad():
            eager = call(loaded[i])
        torch.cuda.synchronize()
        same_bits([out], [eager], ["out"], what)

    forward_test(mode, static, loaded, call, check)


# ------------------------------------------------------------------ g: the modules, forward and backward in one graph
class CallCounts:
    """Counts the calls of the ops functions a module's step from boxes may reach."""
    WATCHED = ("box_attn_forward_boxes", "box_attn_forward_boxes_staged", "box_attn_backward_boxes",
               "box_attn_backward_boxes_staged", "box_attn_backward_boxes_value", "box_attn_backward")

    def __init__(self, monkeypatch):
        from boxer_amd import ops
        self.n = {name: 0 for name in self.WATCHED}
        for name in self.WATCHED:
            monkeypatch.setattr(ops, name, self._spy(name, getattr(ops, name)))

    def _spy(self, name, fn):
        def inner(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return inner


def module_step(m, static, fixed, loss_of, native_bf16):
    """Forward, loss and every gradient -- query, value, reference windows, parameters -- as one step (what
    bench_train.graphed_step captures, without the optimizer)."""
    names = ["query", "value", "ref_windows"] + ["param." + n for n, _ in m.named_parameters()]

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=native_bf16):
            outs = m(static["query"], static["value"], fixed[2], fixed[3], fixed[4], fixed[5], static["ref"])
        leaves = [static["query"], static["value"], static["ref"]] + list(m.parameters())
        return outs, dict(zip(names, torch.autograd.grad(loss_of(outs), leaves)))
    return step


def two_batches(args):
    """The module's batch and another one of the same shapes: queries, values and windows moved along the sequence and
    rescaled (windows stay windows)."""
    first = dict(query=args[0], value=args[1], ref=args[6])
    other = dict(query=(args[0].roll(1, 1) * 0.75).contiguous(), value=(args[1].roll(3, 1) * 1.25).contiguous(),
                 ref=args[6].roll(1, 1).contiguous())
    return other, first


@EACH_MODE
@pytest.mark.parametrize("native_bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("value_flag", [False, True], ids=["boxes_train", "boxes_value"])
@pytest.mark.parametrize("name", ["G9_module_box_dec", "G9_module_box3d_rot_dec"])
def test_golden_decoder_module_step(name, value_flag, native_bf16, mode, monkeypatch):
    """The golden decoder modules with ``fused_boxes_train`` (and ``fused_boxes_value``): captured on another batch,
    replayed on it, on the golden batch and on it again; the replay on the golden batch meets the reference's float64
    output and gradients at the tolerances the eager module tests hold these fixtures to (boxes_cases._g9_check)."""
    m, g, args = boxes_cases.box_golden_module(name, native_bf16)
    m.fused_boxes_train, m.fused_boxes_value = True, value_flag
    calls = CallCounts(monkeypatch)
    batches = list(two_batches(args))
    static = gc.clone(batches[0], leaves=("query", "value", "ref"))
    gout = dev(g["gout0"]).double()
    step = module_step(m, static, args, lambda outs: (outs[0].double() * gout).sum(), native_bf16)
    tol = 4e-2 if native_bf16 else 2e-4
    rms_only = ("ref_windows", "linear_box", "query") if native_bf16 else ()

    def check(i, kept, what):
        outs, grads = kept
        assert outs[1] == ()
        assert all(torch.isfinite(t).all() for t in grads.values()), what
        if i == 1:
            boxes_cases._g9_check(name, outs[:1], grads, g, tol, what, rms_only=rms_only)

    gc.replay_on(mode, step, static, batches, (0, 1, 0), check)
    taken = "box_attn_backward_boxes_value" if value_flag else "box_attn_backward_boxes"
    assert calls.n[taken] > 0 and calls.n["box_attn_forward_boxes"] > 0, calls.n
    assert calls.n["box_attn_backward_boxes" if value_flag else "box_attn_backward_boxes_value"] == 0, calls.n
