"""GPU characterisation of the backward's host routing (``-m gpu``): which route a ``*_bwd_ws_*`` / ``*_bwd_part_*``
call takes -- refused, the atomic kernels, the binned backward -- as a function of ``want``, the workspace, the plan
of a training forward and the variant switch.  No gradient values are compared with an oracle here
(tests/test_gpu_partial_backward.py does that); a route shows in the return code, in the launches per profile slot
and in which output buffers the call wrote.

The table is DESIGN.md 4.2 (route table) and 4.10 written out, for the DECODER shape of
tests/test_gpu_partial_backward.py -- the smallest there that the binned route accepts; it does not qualify for the
one-pass fill, so no state buffer takes part.  At this shape the binned layout is larger than the B*S*H*C floats of
the 16-bit atomic fallback, so a workspace that is 256 bytes too small for the binned layout still serves the atomic
kernels.

What the rows can tell apart: with want = POINTS the binned route (launch_pointgrad without a ride) and the atomic
route (the points-only atomic kernel) look alike from outside -- return code 0, one launch in "bwd_points", the same
buffers written.  That a POINTS-only call stays on the binned route without a workspace is carried by the variant-3
rows alone: there a call that is not binned is refused.  The variant-0 POINTS rows only hold that the call succeeds
with one launch whatever the workspace is.
"""
import ctypes

import pytest
import torch

from point_cases import (ALL, PARTIAL_DECODER as DECODER, POINTS, P_OF, REPEATS, SUFFIX, VALUE, _blib,
                         backward_with_plan as backward, call, profiled, seeded_case, untouched)

pytestmark = pytest.mark.gpu

REFUSED, ATOMIC, BINNED = "refused", "atomic", "binned"
# ROUTE[variant][want][workspace] -> route, or (route with float32 storage, route with bfloat16 storage).
# Workspace: "ok" the size the library asks for, 256-aligned | "null" | "small" 256 bytes less than the binned layout
# needs (with a plan: than the scratch alone) | "misaligned" the full size, 16 bytes off a 256-byte boundary.
_VALUE_AUTO = {"ok": BINNED, "null": (ATOMIC, REFUSED), "small": ATOMIC, "misaligned": ATOMIC}
_VALUE_ATOMIC = {"ok": ATOMIC, "null": (ATOMIC, REFUSED), "small": ATOMIC, "misaligned": ATOMIC}
_VALUE_BINNED = {"ok": BINNED, "null": REFUSED, "small": REFUSED, "misaligned": REFUSED}
_POINTS = lambda route: {"ok": route, "null": route, "small": route, "misaligned": route}     # no workspace needed
ROUTE = {
    0: {ALL: _VALUE_AUTO, VALUE: _VALUE_AUTO, POINTS: _POINTS(BINNED)},
    2: {ALL: _VALUE_ATOMIC, VALUE: _VALUE_ATOMIC, POINTS: _POINTS(ATOMIC)},
    3: {ALL: _VALUE_BINNED, VALUE: _VALUE_BINNED, POINTS: _POINTS(BINNED)},
}
# LAUNCHES[route][want] -> launches per profile slot (slots not named: 0); binned, "bwd_binning": (no plan, plan) --
# count + scans are one timed group of launches, which a plan saves; the fill is another unless it rides in the
# point-gradient launch (want = 3)
LAUNCHES = {
    REFUSED: {ALL: {}, VALUE: {}, POINTS: {}},
    ATOMIC: {ALL: {"bwd_points": 1}, VALUE: {"bwd_accumulate": 1}, POINTS: {"bwd_points": 1}},
    BINNED: {ALL: {"bwd_points": 1, "bwd_accumulate": 1, "bwd_binning": (1, 0)},
             VALUE: {"bwd_accumulate": 1, "bwd_binning": (2, 1)},
             POINTS: {"bwd_points": 1}},
}
RC = {REFUSED: 1, ATOMIC: 0, BINNED: 0}       # 1: hipErrorInvalidValue


def expected(dtype, want, ws, plan, variant):
    """-> (rc, {slot: launches}, (grad_value written, point gradients written))"""
    route = ROUTE[variant][want][ws]
    if isinstance(route, tuple):
        route = route[dtype == torch.bfloat16]
    slots = {k: (v[plan] if isinstance(v, tuple) else v) for k, v in LAUNCHES[route][want].items()}
    wrote = route != REFUSED
    return RC[route], {k: v for k, v in slots.items() if v}, (wrote and bool(want & VALUE), wrote and bool(want & POINTS))


def train_plan(case):
    """The plan of a training forward (*_fwd_train_*, variant 0, no state), as a fresh device buffer."""
    lib = _blib().load()
    host = (case.sh.ctypes.data, case.ls.ctypes.data)
    nbytes = int(lib.boxattn_plan_bytes(int(case.dtype != torch.float32), *case.dims, *host))
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    B, S, H, C, L, Lq, P = case.dims
    outs = [torch.empty((B, Lq, H * C), dtype=case.dtype, device="cuda")]
    if case.kind == "instance":
        outs.append(torch.empty((B, Lq, P, H * C), dtype=case.dtype, device="cuda"))
    built = ctypes.c_int(0)
    stem = "boxattn" if case.kind == "box" else "instattn"
    args = [t.data_ptr() for t in [case.value, case.shapes, case.lsi, case.loc, *case.weights]] + list(case.dims)
    args += [t.data_ptr() for t in outs] + [*host, buf.data_ptr(), nbytes, 0, 0, 0, ctypes.addressof(built),
                                            torch.cuda.current_stream().cuda_stream]
    rc = getattr(lib, "%s_fwd_train_%s" % (stem, SUFFIX[case.dtype]))(*args)
    torch.cuda.synchronize()
    assert rc == 0 and built.value == 1, "the training forward builds a plan at this shape (%d, %d)" % (rc, built.value)
    return buf


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["box", "instance"])
def test_backward_routes(kind, dtype):
    case, _want, _edge = seeded_case(kind, dtype, DECODER + (P_OF["decoder"][kind],))
    blib = _blib()
    B, S, H, C = case.dims[:4]
    plan_bytes = train_plan(case).numel()
    # the premise of the "small" rows: the query's answer is the binned layout, and the atomic fallback fits below it
    assert case.ws_bytes - plan_bytes - 256 >= B * S * H * C * 4 and case.ws_bytes % 256 == 0
    arena = torch.empty(case.ws_bytes + 512, dtype=torch.uint8, device="cuda")
    base = (-arena.data_ptr()) % 256
    bad = []
    for variant in (0, 2, 3):
        for with_plan in (False, True):
            need = case.ws_bytes - (plan_bytes if with_plan else 0)        # what the binned route needs of the workspace
            spaces = {"ok": arena[base:base + case.ws_bytes], "null": None, "small": arena[base:base + need - 256],
                      "misaligned": arena[base + 16:base + 16 + case.ws_bytes]}
            for entry, want in (("ws", ALL), ("part", ALL), ("part", POINTS), ("part", VALUE)):
                for ws_name, ws in spaces.items():
                    blib.set_variant(0)
                    plan = train_plan(case) if with_plan else None
                    blib.set_variant(variant)
                    outs = case.outputs(pattern=True)
                    rc, slots = profiled(lambda: backward(case, entry, want, outs, ws, plan))
                    got = (rc, {k: v for k, v in slots.items() if v},
                           (not untouched(outs[0]), tuple(not untouched(t) for t in outs[1:])))
                    exp = expected(dtype, want, ws_name, with_plan, variant)
                    exp = exp[:2] + ((exp[2][0], (exp[2][1],) * (case.n_out - 1)),)
                    what = "variant %d, %s want=%d, workspace %s, %s" % (variant, entry, want, ws_name,
                                                                         "plan" if with_plan else "no plan")
                    print("%s %s: rc, launches, (grad_value, point gradients) written = %s" %
                          ("ok  " if got == exp else "FAIL", what, got))
                    if got != exp:
                        bad.append("%s: got %s, expected %s" % (what, got, exp))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("variant", [0, 2], ids=["binned", "atomic"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["box", "instance"])
def test_want_all_is_one_call_through_both_entries(kind, dtype, variant):
    """want = 3 through *_bwd_part_* against *_bwd_ws_*: the point gradients bit for bit (their sums are ordered);
    grad_value bit for bit where the *_bwd_ws_* call agrees with itself (test_gpu_partial_backward.run_family's
    repeat-probe rule: a mismatch counts only if REPEATS more *_bwd_ws_* calls all give the first one's bits)."""
    case, _want, _edge = seeded_case(kind, dtype, DECODER + (P_OF["decoder"][kind],))
    _blib().set_variant(variant)
    (rc1, ws1), (rc2, ws2), (rc3, part) = call(case), call(case), call(case, want=ALL)
    assert (rc1, rc2, rc3) == (0, 0, 0)
    for i in range(1, case.n_out):
        assert torch.equal(ws1[i], ws2[i]) and torch.equal(part[i], ws2[i]), "point gradient %d" % i
    if torch.equal(ws1[0], ws2[0]) and not torch.equal(part[0], ws2[0]):
        more = [call(case)[1][0] for _ in range(REPEATS)]
        assert not all(torch.equal(m, ws2[0]) for m in more), \
            "grad_value of want=3 differs from %d *_bwd_ws_* calls that agree with each other" % (REPEATS + 2)
