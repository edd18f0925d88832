"""GPU: no output depends on input data its definition does not name ("Isolation"; tests/isolation.py).

Every case builds an edge family on the shapes, option keys and route assertions of tests/test_gpu_error_bounds.py (and,
from boxes, of tests/test_gpu_boxes_error_bounds.py and tests/test_gpu_box_boxes_staged_forward.py; all of them in
tests/point_cases.py, tests/boxes_cases.py and tests/route_vocab.py), asserts its route
through the library's queries, runs the call clean twice (the second on the warm state: the one-pass fill where the route
has it) and then poisoned, and compares bit for bit:

  value     NaN in every unreferenced value row and the padded tail; then in all of batch 1; then in all of head 1;
  upstream  NaN in grad_out (and grad_mask) of the victim queries of batch 0; then in head 0's channels of them only;
  weights   NaN in the weights (logits) of (0, one victim, head 0);
  guards    every input tensor a view inside a buffer with 64 KiB of NaN on either side; outputs, workspace, plan and
            state of the raw C entry points views of exactly the reported bytes inside 0xA5 guards.

grad_value is compared bit for bit where the route's sum is ordered (two clean runs agree; a mismatch is held against
the route only after REPEATS more clean runs agreed, the rule of test_gpu_partial_backward.run_family, and no further
poisoned run reproduced the clean bits: GradValue), otherwise at compare_rules.tol_of against the oracle on the
clean inputs.  On the matrix-core accumulates a victim's non-finite upstream row may reach all pixels of the 8 x 4 blocks
the victim touches (spread_for); the contract itself is kept for them as xfail(strict=True) cases.  Only
data is poisoned, never a location, a box or a shape.  Each case prints ``isolation | route | type | family | edge |
poisoned share | result``; profiles/isolation.log is that table from one run, its rows folded to one line a route."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import isolation as iso
import point_cases
import route_vocab
from compare_rules import check_scaled as check, tol_of
from isolation import BOX_FLAVOURS, DECODER, ENCODER, STAGED_GEOMETRY, STAGED_LEVELS, WIDE_LEVELS
from point_cases import (ALL, Case, DECODER_FORWARD, DECODER_ROUTES, ENCODER_ROUTES, REPEATS, SEEDED, SHAPE_A, SUFFIX,
                         backward_with_plan, call)
from route_vocab import (ACC_SPLIT, ACC_TR, ACC_VALU, DTYPES, F32, GATHER, REC_GROUP, REC_POINT, STAGED, WIDE, routes,
                         take_family, to_device as dev)
from oracle import boxattn_oracle as oc

pytestmark = pytest.mark.gpu

NAN = float("nan")
EDGES = iso.EDGES


@pytest.fixture(autouse=True)
def _same_kernels_in_every_run(monkeypatch):
    from boxer_amd import ops
    monkeypatch.setattr(ops._Locality, "enabled", False)        # both runs of a pair take the same kernels
    ops.release_workspaces()
    yield
    ops.release_workspaces()


@functools.lru_cache(maxsize=64)
def problem(levels, Lq, P, edge, kind="box", B=2, H=2, C=32, pad=0):
    return iso.problem([tuple(lv) for lv in levels], Lq, P, edge, kind=kind, B=B, H=H, C=C, pad=pad)


def key(levels):
    return tuple(tuple(lv) for lv in levels)


# ------------------------------------------------------------------ the families of one case
class Table:
    """The rows of one case; a leak is a row and, at the end, the case's failure."""

    def __init__(self, route, dtype, edge):
        self.head, self.edge, self.bad = "isolation | %s | %s" % (route, dtype), edge, []

    def hold(self, family, share, fn):
        try:
            n = fn()
            res = "ok (%d elements held)" % n
        except AssertionError as e:
            res = "LEAK: " + " ".join(str(e).split())[:300]
            self.bad.append("%s: %s" % (family, e))
        print("%s | %s | %s | %.2f | %s" % (self.head, family, self.edge, share, res))

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def poisoned(t, name, index):
    c = t[name].clone()
    c[index] = NAN
    return dict(t, **{name: c})


def oracle_grad_value(g):
    if "_gv" not in g:
        a = [g[k] for k in ("value", "shapes", "lsi", "loc")]
        if g["kind"] == "instance":
            g["_gv"] = oc.instance_attn_backward(*a, g["spatial_w"], g["level_w"], g["grad_out"], g["grad_mask"])[0]
        else:
            g["_gv"] = oc.box_attn_backward(*a, g["attn"], g["grad_out"])[0]
    return g["_gv"]


class GradValue:
    """How a case's grad_value is held: bit for bit while the route's sum looks ordered, else at the project's tolerance
    against the oracle on the clean inputs.  No route sums grad_value in a fixed order by construction (float atomics, or
    records whose order inside a bin follows integer atomics: tests/test_gpu_parity.test_binned_backward_run_to_run), and
    on these small problems most runs agree all the same; so a mismatch is held against the route only after REPEATS more
    clean runs agreed with the first (the rule of test_gpu_partial_backward.run_family) AND none of REPEATS more
    poisoned runs reproduced the clean result -- one that does shows that the poison is not what changed the bits.
    The poison is NaN: what leaks of it is not finite, and that is asserted on either path."""

    def __init__(self, g, dt, clean, again, run_clean):
        self.g, self.dt, self.clean, self.run_clean = g, dt, clean, run_clean
        self.ordered = torch.equal(clean, again)

    def hold(self, got, bsh, what, rerun=None):
        ex = None if bsh is None else np.asarray(bsh, dtype=bool)[..., None]
        if self.ordered:
            try:
                return iso.isolated("grad_value", self.clean, got, ex, what)
            except AssertionError as e:
                if "differ from the clean run" not in str(e):
                    raise
                more = [self.run_clean() for _ in range(REPEATS)]
                self.ordered = all(torch.equal(m, self.clean) for m in more)
                print("     grad_value differed; %d more clean runs all bitwise equal: %s" % (REPEATS, self.ordered))
                if self.ordered and rerun is not None:
                    for i in range(REPEATS):
                        try:
                            iso.isolated("grad_value", self.clean, rerun(), ex, what)
                        except AssertionError:
                            continue
                        print("     ... and poisoned run %d more reproduced the clean result: the sum is not ordered" % (i + 1))
                        self.ordered = False
                        break
                if self.ordered:
                    raise
        n = iso.finite_outside("grad_value", got, ex, what)
        want = oracle_grad_value(self.g)
        held = got.detach().double().cpu().numpy()
        if ex is not None:
            held = np.where(np.broadcast_to(ex, held.shape), want, held)
        check(torch.from_numpy(held), want, tol_of(self.dt), what + " grad_value (unordered sum)")
        return n


def spread_of(g, groups):
    """(B, S, H): where a matrix-core accumulate may put a non-finite upstream row of the victims (iso.block_spread),
    with the widened footprint of the contract."""
    name = "_spread_groups" if groups else "_spread"
    if name not in g:
        B = g["loc"].shape[0]
        s = iso.block_spread(g["shapes"], g["loc"][:1], g["victims"], g["value"].shape[1], g["lsi"], groups)
        g[name] = np.concatenate([s, np.zeros((B - 1,) + s.shape[1:], dtype=bool)], 0) | g["opposite"]
    return g[name]


def spread_for(acc, rec):
    """The upstream family's allowance for grad_value on a binned route: None (the contract: the victims' footprint) on
    the VALU accumulate, their 8 x 4 blocks on the matrix cores, their groups' block ranges with group records."""
    return None if acc == ACC_VALU else "groups" if rec == REC_GROUP else "blocks"


def hold_families(route, dtype, g, run, instance=False, tensors=None, upstream=None, weights=None, tab=None, spread=None,
                  only=None):
    """run(tensors) -> {output name: tensor}; every family of the module docstring that the outputs allow.  upstream /
    weights: the keys of the upstream gradients (grad_out first, then grad_mask) and of the weights or logits among the
    tensors (default: those of box or instance attention on a sampling grid; () for a forward alone).  spread: None --
    the contract: a non-finite upstream row of a victim reaches grad_value only inside the victim's footprint -- or
    "blocks" / "groups": the documented deviation of the matrix-core accumulates (spread_of).  only: the families to run
    (default all)."""
    dt = DTYPES[dtype]
    t = (point_cases.inst_tensors if instance else point_cases.box_tensors)(g, dt) if tensors is None else tensors
    tab = Table(route, dtype, g["edge"]) if tab is None else tab
    clean, again = run(t), run(t)
    backward = "grad_value" in clean
    if upstream is None:
        upstream = () if len(clean) == 1 else ("grad_out", "grad_mask") if instance else ("grad_out",)
    if weights is None:
        weights = ("attn", "level_w") if instance else ("attn",)
    B, Lq, H = g["loc"].shape[:3]
    C = g["value"].shape[-1]
    assert all(bool(torch.isfinite(v).all()) for v in clean.values()), "the clean run is finite"
    for name in clean:
        if name != "grad_value":
            assert torch.equal(clean[name], again[name]), "%s of two clean runs" % name
    gv = GradValue(g, dt, clean["grad_value"], again["grad_value"], lambda: run(t)["grad_value"]) if backward else None
    heads = np.arange(H)

    def family(name, share, tp, bqh=None, bsh=None, value_only_finite=False):
        if only is not None and name.split(":")[0] not in only:
            return

        def fn():
            got = run(tp)
            n = iso.check_outputs(clean, got, bqh=bqh, bsh=bsh, grad_value="finite" if value_only_finite else "skip",
                                  what=name)
            if backward and not value_only_finite:
                n += gv.hold(got["grad_value"], bsh, name, lambda: run(tp)["grad_value"])
            return n
        tab.hold(name, share, fn)

    # 1. value
    un = g["unreferenced"]
    family("value: unreferenced rows", iso.share(un), dict(t, value=iso.poison_rows(t["value"], un)))
    if B > 1:
        b1 = np.zeros((B, Lq, H), dtype=bool)
        b1[1:] = True
        family("value: batch 1", (B - 1) / B, poisoned(t, "value", np.s_[1:]), bqh=b1, value_only_finite=True)
    if H > 1:
        h1 = np.zeros((B, Lq, H), dtype=bool)
        h1[:, :, 1] = True
        family("value: head 1", 1 / H, poisoned(t, "value", np.s_[:, :, 1]), bqh=h1, value_only_finite=True)
    # 2. upstream
    v = g["victims"]
    if upstream:
        for what, hs, ch in (("upstream: victims", None, np.s_[:]), ("upstream: victims, head 0", (0,), np.s_[:C])):
            tp = poisoned(t, upstream[0], (0, v, ch))
            if len(upstream) > 1:
                tp = poisoned(tp, upstream[1], (0, v, slice(None), ch))
            hm = np.ones(H, dtype=bool) if hs is None else heads == 0
            reach = g["opposite"] if spread is None else spread_of(g, spread == "groups")
            family(what, len(v) / (B * Lq) * hm.mean(), tp, bqh=iso.victim_triples(g, hs), bsh=reach & hm)
    # 3. weights
    q = v[len(v) // 2]
    one = np.zeros((B, Lq, H), dtype=bool)
    one[0, q, 0] = True
    tp = t
    for w in weights:
        tp = poisoned(tp, w, (0, q, 0))
    family("weights: (0, %d, 0)" % q, 1 / (B * Lq * H), tp, bqh=one, bsh=g["opposite"] & (heads == 0))

    # 4. guards, inputs
    def guarded():
        arenas = {k: iso.input_arena(x) for k, x in t.items() if isinstance(x, torch.Tensor)}
        got = run(dict(t, **{k: a.view for k, a in arenas.items()}))
        n = iso.check_outputs(clean, got, grad_value="skip", what="guards")
        if backward:
            n += gv.hold(got["grad_value"], None, "guards", lambda: run(dict(t, **{k: a.view for k, a in arenas.items()}))["grad_value"])
        for k, a in arenas.items():
            assert iso.guards_intact(a), "the guards of input %s were written" % k
        return n
    if only is None or "guards" in only:
        tab.hold("guards: inputs", 0.0, guarded)
    return tab


# ------------------------------------------------------------------ box attention: the encoder routes, the staged levels
@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("riders", [0, 1], ids=["riders", "own_launches"])
@pytest.mark.parametrize("dense", [2, 1], ids=["staged", "row_gather"])
@pytest.mark.parametrize("dtype,acc_key,rec_key", ENCODER_ROUTES,
                         ids=["f32_split", "f32_valu", "f32_mfma", "bf16_point", "bf16_group", "f16_point", "f16_group"])
def test_encoder(dtype, acc_key, rec_key, dense, riders, edge):
    """(13, 13), (7, 5), one query a pixel: every forward / accumulate / record route of the encoder, the full backward,
    the second clean call on the warm state (the one-pass fill where the route has it)."""
    from point_cases import counters
    route_vocab.set_encoder_keys(dense, riders, acc_key, rec_key)
    fwd, acc, rec, one_pass = point_cases.encoder_expectation(dtype, dense, riders, acc_key, rec_key)
    g = problem(key(ENCODER), "S", 4, edge)
    t = point_cases.box_tensors(g, DTYPES[dtype])
    assert routes(t) == (fwd, acc, rec), "the library answers %r" % (routes(t),)
    route = "encoder: %s forward, %s accumulate, %s records, riders %s" % (
        "staged" if dense == 2 else "row-gather", ("valu", "tr", "f32", "split")[acc], ("point", "group")[rec],
        "on" if riders == 0 else "off")
    seen = []

    def run(tt):
        got = point_cases.run_box(tt)
        seen.append(counters())
        return got
    tab = hold_families(route, dtype, g, run, tensors=t, spread=spread_for(acc, rec))
    ns = t["value"].size(0) * t["value"].size(2)
    assert seen[0] == (0, 0), "a cold state runs the two-pass passes: %r" % (seen[:3],)
    if one_pass:
        assert seen[1][0] == ns and seen[2][0] == 2 * ns, "the one-pass fill ran from the second call on: %r" % (seen[:3],)
    else:
        assert seen[-1][0] == 0, "no one-pass fill on this route: %r" % (seen[-1],)
    tab.done()


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_staged_levels(levels, dtype, edge):
    """(37, 23), (19, 12), (10, 6), (5, 3) and its first 1 - 3 levels, one query a pixel: the 1- to 4-level instantiations
    of the window-staged kernels, the finest level staged as clamped sub-windows."""
    from boxer_amd import _lib
    _lib.set_option("dense", 2)
    g = problem(key(STAGED_LEVELS[:levels]), "S", 4, edge)
    t = point_cases.box_tensors(g, DTYPES[dtype])
    fwd, acc, rec = routes(t)
    assert fwd == STAGED, fwd
    route = "staged levels, %d: staged forward, %s accumulate, %s records" % (
        levels, ("valu", "tr", "f32", "split")[acc], ("point", "group")[rec])
    hold_families(route, dtype, g, point_cases.run_box, tensors=t, spread=spread_for(acc, rec)).done()


# ------------------------------------------------------------------ box attention: decoder shapes, SEEDED[6], wave per pair
@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype,variant", DECODER_ROUTES,
                         ids=["%s_%s" % (dt, ("auto", "generic", "atomic", "binned")[v]) for dt, v in DECODER_ROUTES])
def test_decoder(dtype, variant, edge):
    """Four levels, 50 queries: the generic kernels (float32) and the atomic backward with three rows of padded tail, the
    binned backward without (a padded tail rules the binned route out: boxattn_host_plan.h, make_plan_blocks)."""
    from boxer_amd import _lib
    g = problem(key(DECODER), 50, 4, edge, pad=3 if variant in (1, 2) else 0)
    t = point_cases.box_tensors(g, DTYPES[dtype])
    _lib.set_variant(variant)
    fwd, acc, rec = routes(t)
    assert fwd == DECODER_FORWARD[variant] and rec == REC_POINT, (fwd, rec)
    assert acc == (ACC_SPLIT if dtype == "f32" else ACC_TR), acc
    route = "decoder, variant %s: %s forward" % (("auto", "generic", "atomic", "binned")[variant], _lib.FWD_FAMILIES[fwd])
    hold_families(route, dtype, g, point_cases.run_box, tensors=t,
                  spread=None if variant in (1, 2) else spread_for(acc, rec)).done()


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("variant", [0, 3], ids=["auto", "binned"])
@pytest.mark.parametrize("dtype,C", [("f32", 32), ("bf16", 32), ("f16", 32), ("bf16", 16), ("bf16", 64)],
                         ids=["f32", "bf16", "f16", "bf16_c16", "bf16_c64"])
def test_seeded_6(dtype, C, variant, edge):
    """(25, 25), (13, 13), (7, 5), (1, 3), (2, 1), 700 queries: the one-pixel-wide levels are wholly outside and wholly
    poisoned."""
    from boxer_amd import _lib
    shapes, B, H, _, Lq, P = SEEDED[6]
    g = problem(key(shapes), Lq, P, edge, B=B, H=H, C=C)
    assert g["unreferenced"][:, iso.level_rows(shapes, 3)].all() and g["unreferenced"][:, iso.level_rows(shapes, 4)].all()
    t = point_cases.box_tensors(g, DTYPES[dtype])
    _lib.set_variant(variant)
    fwd, acc, rec = routes(t)
    assert fwd == GATHER and rec == REC_POINT and acc == (ACC_SPLIT if dtype == "f32" else ACC_TR), (fwd, acc, rec)
    route = "SEEDED[6] C=%d, variant %d: row-gather forward, %s accumulate" % (C, variant, ("valu", "tr", "f32", "split")[acc])
    hold_families(route, dtype, g, point_cases.run_box, tensors=t, spread=spread_for(acc, rec)).done()


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("P", [196, 36])
def test_wave_per_pair_forward(P, dtype, edge):
    from boxer_amd import ops
    g = problem(key(WIDE_LEVELS), 6, P, edge, pad=3)
    t = point_cases.box_tensors(g, DTYPES[dtype])
    take_family(t["value"], t["loc"], t["shapes"], t["lsi"], WIDE)

    def run(tt):
        assert ops.forward_route(tt["value"], tt["loc"], tt["shapes"], tt["lsi"]) == WIDE
        out = ops.box_attn_forward(tt["value"], tt["shapes"], tt["lsi"], tt["loc"], tt["attn"], 64)
        torch.cuda.synchronize()
        return dict(out=out)
    hold_families("wave-per-pair forward, P = %d" % P, dtype, g, run, tensors=t).done()


# ------------------------------------------------------------------ instance attention
@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype,opt", [("bf16", 1), ("bf16", 2), ("f16", 1), ("f16", 2), ("f32", 0)],
                         ids=["bf16_valu", "bf16_tr", "f16_valu", "f16_tr", "f32"])
def test_instance_shape_a(dtype, opt, edge):
    """(16, 24), (7, 5), (1, 3), B 2, H 3, 300 queries, 4 x 4 points: the 16-bit accumulate on the VALU (inst_acc16 = 1)
    and on the matrix cores (2), float32 on its default route; the binned backward required."""
    from boxer_amd import _lib
    a = SHAPE_A
    g = problem(key(a["levels"]), a["Lq"], a["k"] ** 2, edge, kind="instance", B=a["B"], H=a["H"], C=a["C"])
    t = point_cases.inst_tensors(g, DTYPES[dtype])
    _lib.set_option("inst_acc16", opt)
    _lib.set_variant(3)
    fwd, acc, rec = routes(t, instance=True)
    assert acc == {0: ACC_VALU, 1: ACC_VALU, 2: ACC_TR}[opt] and rec == REC_POINT, (acc, rec)
    route = "instance shape A: %s forward, %s accumulate" % (_lib.FWD_FAMILIES[fwd], ("valu", "tr", "f32", "split")[acc])
    hold_families(route, dtype, g, point_cases.run_instance, instance=True, tensors=t, spread=spread_for(acc, rec)).done()


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_instance_14_by_14_points(dtype, edge):
    """k = 14, six queries, four levels: the wave-per-pair instance forward and the backward on its default route."""
    g = problem(key(DECODER), 6, 196, edge, kind="instance")
    t = point_cases.inst_tensors(g, DTYPES[dtype])
    fwd, acc, rec = routes(t, instance=True)
    assert fwd == WIDE and rec == REC_POINT, (fwd, rec)
    route = "instance k = 14: wide forward, %s accumulate" % ("valu", "tr", "f32", "split")[acc]
    hold_families(route, dtype, g, point_cases.run_instance, instance=True, tensors=t, spread=spread_for(acc, rec)).done()


# ------------------------------------------------------------------ the contract the matrix-core accumulates miss
# DESIGN.md 5, "Isolation": the accumulates on the matrix cores multiply a record's upstream row by the zero weights of its
# block's other pixels, so a non-finite grad_out / grad_mask row of a query turns all 32 pixels of every 8 x 4 block the
# query touches to NaN (group records: of its groups' block ranges), not only its footprint.  The cases above hold
# that spread (spread_for); these hold the contract itself and are expected to fail until the accumulates stage
# such rows apart.
MATRIX_CORE_ROUTES = [r for r in ENCODER_ROUTES if r[:2] != ("f32", 1)]
LEAK = "a non-finite upstream row reaches all 32 pixels of the blocks its query touches (DESIGN.md 5, Isolation)"


@pytest.mark.xfail(strict=True, raises=AssertionError, reason=LEAK)
@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype,acc_key,rec_key", MATRIX_CORE_ROUTES,
                         ids=["f32_split", "f32_mfma", "bf16_point", "bf16_group", "f16_point", "f16_group"])
def test_upstream_contract_on_the_encoder_matrix_core_accumulates(dtype, acc_key, rec_key, edge):
    route_vocab.set_encoder_keys(2, 0, acc_key, rec_key)
    fwd, acc, rec, _ = point_cases.encoder_expectation(dtype, 2, 0, acc_key, rec_key)
    g = problem(key(ENCODER), "S", 4, edge)
    t = point_cases.box_tensors(g, DTYPES[dtype])
    assert routes(t) == (fwd, acc, rec) and acc != ACC_VALU
    route = "contract, encoder: %s accumulate, %s records" % (("valu", "tr", "f32", "split")[acc], ("point", "group")[rec])
    hold_families(route, dtype, g, point_cases.run_box, tensors=t, only=("upstream",)).done()


@pytest.mark.xfail(strict=True, raises=AssertionError, reason=LEAK)
@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_upstream_contract_on_the_instance_matrix_core_accumulate(dtype, edge):
    from boxer_amd import _lib
    a = SHAPE_A
    g = problem(key(a["levels"]), a["Lq"], a["k"] ** 2, edge, kind="instance", B=a["B"], H=a["H"], C=a["C"])
    t = point_cases.inst_tensors(g, DTYPES[dtype])
    _lib.set_option("inst_acc16", 2)
    _lib.set_variant(3)
    assert routes(t, instance=True)[1:] == (ACC_TR, REC_POINT)
    hold_families("contract, instance shape A: tr accumulate", dtype, g, point_cases.run_instance, instance=True, tensors=t,
                  only=("upstream",)).done()


# ------------------------------------------------------------------ guards around outputs, workspace, plan and state
def raw_case(g, dt, value=None):
    cdt = F32
    kind = g["kind"]
    weights = [dev(g["attn"], cdt)] + ([dev(g["level_w"], cdt)] if kind == "instance" else [])
    return Case(kind, dt, dev(g["value"], dt) if value is None else value, dev(g["shapes"]), dev(g["lsi"]), dev(g["loc"], cdt),
                weights, dev(g["grad_out"], dt), dev(g["grad_mask"], dt) if kind == "instance" else None)


def byte_arena(nbytes, zero=False):
    a = iso.arena((nbytes,), torch.uint8, "cuda", align=256)
    if zero:
        a.view.zero_()
    return a


def raw_forward_train(case, outs, plan, state):
    """*_fwd_train_* (test_gpu_backward_routes.train_plan) on the caller's buffers -> (rc, plan built)."""
    from boxer_amd import _lib
    lib = _lib.load()
    built = ctypes.c_int(0)
    stem = "boxattn" if case.kind == "box" else "instattn"
    args = [x.data_ptr() for x in [case.value, case.shapes, case.lsi, case.loc, *case.weights]] + list(case.dims)
    args += [x.data_ptr() for x in outs]
    args += [case.sh.ctypes.data, case.ls.ctypes.data, plan.data_ptr() if plan is not None else 0,
             plan.numel() if plan is not None else 0, state.data_ptr() if state is not None else 0,
             state.numel() if state is not None else 0, 0, ctypes.addressof(built), torch.cuda.current_stream().cuda_stream]
    rc = getattr(lib, "%s_fwd_train_%s" % (stem, SUFFIX[case.dtype]))(*args)
    torch.cuda.synchronize()
    return rc, built.value


def raw_step(case, guarded):
    """The training forward, *_bwd_ws_* twice (cold, then warm state) and *_bwd_part_* (want = 3) through the raw entry
    points.  guarded: outputs, workspace, plan and state are arena views of exactly the reported bytes -> (results of the
    last calls, arenas)."""
    from boxer_amd import _lib
    lib = _lib.load()
    B, S, H, C, L, Lq, P = case.dims
    h16 = int(case.dtype != F32)
    host = (case.sh.ctypes.data, case.ls.ctypes.data)
    sizes = dict(ws=int(lib.boxattn_bwd_workspace_bytes(h16, *case.dims, *host)),
                 plan=int(lib.boxattn_plan_bytes(h16, *case.dims, *host)),
                 state=int(lib.boxattn_state_bytes(*case.dims, *host)))
    arenas = {}

    def buf(name, nbytes, zero=False):
        if not nbytes:
            return None
        if guarded:
            arenas[name] = byte_arena(nbytes, zero)
            return arenas[name].view
        return (torch.zeros if zero else torch.empty)(nbytes, dtype=torch.uint8, device="cuda")

    def out(name, shape, dtype):
        if guarded:
            arenas[name] = iso.arena(shape, dtype, "cuda")
            return arenas[name].view
        return torch.empty(shape, dtype=dtype, device="cuda")
    fouts = [out("out", (B, Lq, H * C), case.dtype)]
    if case.kind == "instance":
        fouts.append(out("mask_out", (B, Lq, P, H * C), case.dtype))
    ws, plan, state = buf("workspace", sizes["ws"]), buf("plan", sizes["plan"]), buf("state", sizes["state"], zero=True)
    rc, built = raw_forward_train(case, fouts, plan, state)
    assert rc == 0, "training forward: %d" % rc
    names = ("grad_value", "grad_loc") + (("grad_attn",) if case.kind == "box" else ("grad_spatial", "grad_level"))
    res = dict(zip(("out", "mask_out"), fouts))
    for leg, want in (("ws cold", None), ("ws warm", None), ("part", ALL)):
        gouts = [out("%s %s" % (n, leg), x.shape, x.dtype) for n, x in zip(names, case.outputs())]
        rc, _ = call(case, want=want, outs=gouts, ws=ws, state=state, fresh=False)
        assert rc == 0, "%s: %d" % (leg, rc)
        if leg != "ws cold":
            for n, x in zip(names, gouts):
                res["%s|%s" % (n, leg)] = x
    if built:                                    # ... and the backward on the forward's plan (no state then)
        gouts = [out("%s plan" % n, x.shape, x.dtype) for n, x in zip(names, case.outputs())]
        rc = backward_with_plan(case, "ws", ALL, gouts, ws, plan)
        assert rc == 0, "ws with the plan: %d" % rc
        for n, x in zip(names, gouts):
            res["%s|ws with the plan" % n] = x
    return res, arenas, sizes, built


RAW_CASES = [("encoder", key(ENCODER), "S", 4, "box", 0), ("decoder", key(DECODER), 50, 4, "box", 0),
             ("decoder, padded tail", key(DECODER), 50, 4, "box", 3),
             ("instance shape A", key(SHAPE_A["levels"]), SHAPE_A["Lq"], 16, "instance", 0)]


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name,levels,Lq,P,kind,pad", RAW_CASES, ids=[c[0].replace(", ", "_").replace(" ", "_") for c in RAW_CASES])
def test_raw_entries_stay_inside_their_buffers(name, levels, Lq, P, kind, pad, dtype, edge):
    """The training forward, *_bwd_ws_* (cold, then on the warm state) and *_bwd_part_* with every output, the
    workspace, the plan and the state as views of exactly the reported bytes between 0xA5 guards, on inputs whose
    unreferenced value rows hold NaN: the guards are intact, the results those of the plain clean call."""
    dt = DTYPES[dtype]
    H = SHAPE_A["H"] if kind == "instance" else 2
    g = problem(levels, Lq, P, edge, kind=kind, H=H, pad=pad)
    tab = Table("raw entries, %s" % name, dtype, edge)
    clean_case = raw_case(g, dt)
    clean, _, sizes, built = raw_step(clean_case, guarded=False)
    again = raw_step(clean_case, guarded=False)[0]
    poisoned_value = iso.input_arena(iso.poison_rows(clean_case.value, g["unreferenced"]))
    print("     reported bytes: %s; plan built: %d" % (sizes, built))

    def guarded_step():
        return raw_step(raw_case(g, dt, value=poisoned_value.view), guarded=True)

    def fn():
        got, arenas, _, _ = guarded_step()
        n = 0
        for k, x in got.items():
            if k.startswith("grad_value"):
                gv = GradValue(g, dt, clean[k], again[k], lambda: raw_step(clean_case, guarded=False)[0][k])
                n += gv.hold(x, None, "raw " + k, lambda: guarded_step()[0][k])
            else:
                n += iso.isolated(k, clean[k], x, None, "raw")
        written = [k for k, a in arenas.items() if not iso.guards_intact(a)]
        assert not written, "written outside its bytes: %s" % ", ".join(written)
        assert iso.guards_intact(poisoned_value)
        return n
    tab.hold("guards: outputs, workspace, plan, state", iso.share(g["unreferenced"]), fn)
    tab.done()


# ------------------------------------------------------------------ from boxes and logits
WINDOWS = [(False, True), (True, False)]                         # (reference windows per head, valid ratios given)


@functools.lru_cache(maxsize=32)
def boxes_problem(levels, Lq, k, edge, kind, B, H, angle_mode, ref_dim, per_head, with_vr, pad=0):
    return iso.boxes_problem([tuple(lv) for lv in levels], Lq, k, edge, kind=kind, B=B, H=H, pad=pad,
                             angle_mode=angle_mode, ref_dim=ref_dim, per_head=per_head, with_vr=with_vr)


def boxes_tensors(g, dt):
    t = dict(value=dev(g["value"], dt), shapes=dev(g["shapes"]), lsi=dev(g["lsi"]), ref=dev(g["ref"]), off=dev(g["off"]),
             kidx=dev(g["kidx"]), vr=None if g["vr"] is None else dev(g["vr"]), logits=dev(g["logits"]),
             grad_out=dev(g["grad_out"], dt))
    if g["kind"] == "instance":
        t["grad_mask"] = dev(g["grad_mask"], dt)
    return t


def operands(t):
    return tuple(t[k] for k in ("value", "shapes", "lsi", "ref", "off", "kidx", "vr", "logits"))


def boxes_conditions(g, levels, edge):
    """What tests/test_isolation.py asserts of these inputs without a GPU, in short: a level with a patch is read and
    more than half unreferenced where no victim is, a level without one is not read at all."""
    for l, lv in enumerate(levels):
        un = g["unreferenced"][:, iso.level_rows(levels, l)]
        if iso.has_patch(lv, edge):
            assert not un.all() and un[-1].mean() >= 0.5, (l, un.mean((1, 2)))
        else:
            assert un.all(), l


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("angle_mode,ref_dim", BOX_FLAVOURS, ids=["plain", "turns_5", "turns_7", "radians"])
def test_box_attention_from_boxes(angle_mode, ref_dim, dtype, edge):
    """ops.box_attn_forward_boxes, _backward_boxes and _backward_boxes_value at P = 4 on the decoder levels, 50 queries:
    the three angle modes, reference windows shared (with valid ratios) and per head (without)."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    tab = None
    for per_head, with_vr in WINDOWS:
        g = boxes_problem(key(DECODER), 50, 2, edge, "box", 2, 2, angle_mode, ref_dim, per_head, with_vr, 3)
        boxes_conditions(g, DECODER, edge)
        t = boxes_tensors(g, dt)
        L, Lq, P = g["dims"][4:]
        assert ops.box_forward_boxes_ok(t["value"], L, Lq, P) and ops.box_backward_boxes_ok(t["value"], L, Lq, P) and \
            ops.box_backward_boxes_value_ok(t["value"], L, Lq, P)

        def run(tt):
            a = operands(tt)
            out = ops.box_attn_forward_boxes(*a, angle_mode)
            goff, grow, glog = ops.box_attn_backward_boxes(*a, angle_mode, tt["grad_out"], need_ref_grad=True)
            gv, voff, vrow, vlog = ops.box_attn_backward_boxes_value(*a, angle_mode, tt["grad_out"], 3, True)
            torch.cuda.synchronize()
            return dict(out=out, grad_offsets=goff, grad_ref_rows=grow, grad_logits=glog, grad_value=gv,
                        grad_offsets_with_value=voff, grad_ref_rows_with_value=vrow, grad_logits_with_value=vlog)
        route = "box attention from boxes, angle mode %d, D = %d, windows %s, valid ratios %s" % (
            angle_mode, ref_dim, "per head" if per_head else "shared", "given" if with_vr else "none")
        tab = Table(route, dtype, edge) if tab is None else tab
        tab.head = "isolation | %s | %s" % (route, dtype)
        hold_families(route, dtype, g, run, tensors=t, upstream=("grad_out",), weights=("logits",), tab=tab)
    tab.done()


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("k", [4, 14])
def test_instance_attention_from_boxes(k, dtype, edge):
    """ops.instance_attn_forward_boxes / _backward_boxes at k = 4 and 14 on the decoder levels, six queries."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    tab = None
    for per_head, with_vr in WINDOWS:
        g = boxes_problem(key(DECODER), 6, k, edge, "instance", 2, 2, 0, 4, per_head, with_vr, 3)
        boxes_conditions(g, DECODER, edge)
        t = boxes_tensors(g, dt)
        L, Lq = g["dims"][4:6]
        assert ops.forward_boxes_ok(t["value"], L, Lq, k) and ops.backward_boxes_ok(t["value"], L, Lq, k)

        def run(tt):
            a = operands(tt)
            out, mask = ops.instance_attn_forward_boxes(*a, k, True)
            goff, grow, glog = ops.instance_attn_backward_boxes(*a, k, tt["grad_out"], tt["grad_mask"], need_ref_grad=True)
            torch.cuda.synchronize()
            return dict(out=out, mask_out=mask, grad_offsets=goff, grad_ref_rows=grow, grad_logits=glog)
        route = "instance attention from boxes, k = %d, windows %s, valid ratios %s" % (
            k, "per head" if per_head else "shared", "given" if with_vr else "none")
        tab = Table(route, dtype, edge) if tab is None else tab
        tab.head = "isolation | %s | %s" % (route, dtype)
        hold_families(route, dtype, g, run, tensors=t, upstream=("grad_out", "grad_mask"), weights=("logits",), tab=tab)
    tab.done()


def test_staged_geometries_are_the_staged_files():
    from boxes_cases import STAGED_GEOMETRY as GEOMETRY
    for name, (levels, B, H) in STAGED_GEOMETRY.items():
        assert GEOMETRY[name] == dict(levels=levels, B=B, H=H)


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("geometry", sorted(STAGED_GEOMETRY))
def test_box_attention_from_boxes_staged(geometry, dtype, edge):
    """ops.box_attn_forward_boxes_staged, one query a pixel: the four (angle mode, reference values) pairs, windows per
    head / valid ratios alternating."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    levels, B, H = STAGED_GEOMETRY[geometry]
    tab = None
    for i, (angle_mode, ref_dim) in enumerate(BOX_FLAVOURS):
        per_head, with_vr = i % 2 == 1, i % 2 == 0
        g = boxes_problem(key(levels), "S", 2, edge, "box", B, H, angle_mode, ref_dim, per_head, with_vr)
        boxes_conditions(g, levels, edge)
        t = boxes_tensors(g, dt)
        Lq, P = g["dims"][5:]
        assert ops.box_forward_boxes_staged_ok(t["value"], t["shapes"], t["lsi"], Lq, P), "not eligible: %r" % (g["dims"],)

        def run(tt):
            out = ops.box_attn_forward_boxes_staged(*operands(tt), angle_mode)
            torch.cuda.synchronize()
            return dict(out=out)
        route = "window-staged from boxes, %s, angle mode %d, D = %d, windows %s, valid ratios %s" % (
            geometry, angle_mode, ref_dim, "per head" if per_head else "shared", "given" if with_vr else "none")
        tab = Table(route, dtype, edge) if tab is None else tab
        tab.head = "isolation | %s | %s" % (route, dtype)
        hold_families(route, dtype, g, run, tensors=t, upstream=(), weights=("logits",), tab=tab)
    tab.done()


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("angle_mode,ref_dim", BOX_FLAVOURS, ids=["plain", "turns_5", "turns_7", "radians"])
def test_raw_backward_from_boxes_stays_inside_its_buffers(angle_mode, ref_dim, dtype, edge):
    """boxattn_bwd_boxes_value_* (want = 3) through tests/capi_cases.call_value with grad_value, the three other
    gradients and the workspace (exactly boxattn_bwd_boxes_value_workspace_bytes) between 0xA5 guards, on a value
    tensor between NaN guards whose unreferenced rows hold NaN: the guards are intact, the results the clean call's."""
    from boxer_amd import _lib
    from capi_cases import call_value
    dt = DTYPES[dtype]
    g = boxes_problem(key(DECODER), 50, 2, edge, "box", 2, 2, angle_mode, ref_dim, False, True, 3)
    t = boxes_tensors(g, dt)
    B, S, H, C, L, Lq, P = g["dims"]
    V = g["off"].shape[-1]
    ws_bytes = int(_lib.box_bwd_boxes_value_workspace_bytes(t["value"].element_size(), g["dims"]))
    assert ws_bytes == (0 if dt == F32 else 4 * B * S * H * C)
    shapes_of = dict(grad_value=((B, S, H, C), dt), grad_offsets=((B, Lq, H, L, V), F32),
                     grad_ref_rows=((B, Lq, H, L, 5), F32), grad_logits=((B, Lq, H, L * P), F32))

    def step(value, guarded):
        arenas = {}
        if guarded:
            arenas = {n: iso.arena(shape, d, "cuda") for n, (shape, d) in shapes_of.items()}
            outs = {n: a.view for n, a in arenas.items()}
            if ws_bytes:
                arenas["workspace"] = byte_arena(ws_bytes)
        else:
            outs = {n: torch.empty(shape, dtype=d, device="cuda") for n, (shape, d) in shapes_of.items()}
        ws = arenas["workspace"].view if "workspace" in arenas else \
            torch.empty(ws_bytes, dtype=torch.uint8, device="cuda") if ws_bytes else None
        ptrs = [x.data_ptr() for x in (value, t["shapes"], t["lsi"], t["ref"], t["off"], t["kidx"], t["vr"], t["logits"],
                                       t["grad_out"], outs["grad_offsets"], outs["grad_ref_rows"], outs["grad_logits"])]
        rc = call_value(_lib, "boxattn_bwd_boxes_value_" + dtype, ptrs, g["dims"], 3, outs["grad_value"].data_ptr(),
                        ws.data_ptr() if ws is not None else None, ws_bytes, ref_dim, V, angle_mode)
        torch.cuda.synchronize()
        assert rc == 0, rc
        return outs, arenas
    clean, again = step(t["value"], False)[0], step(t["value"], False)[0]
    poisoned_value = iso.input_arena(iso.poison_rows(t["value"], g["unreferenced"]))
    tab = Table("raw entry, backward from boxes with grad_value, angle mode %d, D = %d" % (angle_mode, ref_dim), dtype, edge)

    def fn():
        got, arenas = step(poisoned_value.view, True)
        gv = GradValue(g, dt, clean["grad_value"], again["grad_value"], lambda: step(t["value"], False)[0]["grad_value"])
        n = gv.hold(got["grad_value"], None, "raw", lambda: step(poisoned_value.view, True)[0]["grad_value"])
        for k in ("grad_offsets", "grad_ref_rows", "grad_logits"):
            n += iso.isolated(k, clean[k], got[k], None, "raw")
        written = [k for k, a in arenas.items() if not iso.guards_intact(a)]
        assert not written, "written outside its bytes: %s" % ", ".join(written)
        assert iso.guards_intact(poisoned_value)
        return n
    tab.hold("guards: outputs, workspace", iso.share(g["unreferenced"]), fn)
    tab.done()
