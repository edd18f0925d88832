"""GPU tests of the float16 storage mode (``-m gpu``): value / out / mask_out / grad_out / grad_mask /
grad_value IEEE float16, locations / weights and their gradients float32, float32 accumulation, on every
kernel family the bf16 mode takes.

Every operator comparison is against the fp64 CPU oracle (oracle/boxattn_oracle.c) on the f16-ROUNDED
inputs, per element as tests/test_gpu_fullsize.py checks: ``|got - want| <= tol * (max(1, rms(want)) +
|want|)`` with tol = 1e-3 for float16 tensors (half an f16 ulp is 2^-11 = 4.9e-4 relative) and 1e-4 for
float32 ones (what the bf16 mode's float32 outputs meet).
"""
import numpy as np
import pytest
import torch

import bench
import golden_io
from oracle import boxattn_oracle as oc
from compare_rules import check_f16 as check, tol_of_f16 as tol_of
from point_cases import LEVELS4, PARITY_G9 as G9, STAT_OFF
from route_vocab import F16, VARIANTS, dev

pytestmark = pytest.mark.gpu

OPT_DENSE, OPT_RIDERS = 11, 15


@pytest.fixture(autouse=True)
def _reset_switches():
    from boxer_amd import _lib
    yield
    _lib.set_variant(0)
    lib = _lib.load()
    lib.boxattn_set_option(OPT_DENSE, 0)
    lib.boxattn_set_option(OPT_RIDERS, 0)


def f16_rounded(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def seeded(shapes, B, H, C, Lq, P, seed):
    """Random problem, the storage tensors already f16 numbers (the oracle sees what the GPU sees)."""
    rng = np.random.default_rng(seed)
    shapes = np.asarray(shapes, dtype=np.int64)
    sizes = shapes.prod(1)
    lsi = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    S, L = int(sizes.sum()), len(shapes)
    loc = rng.uniform(-0.1, 1.1, (B, Lq, H, L, P, 2)).astype(np.float32).astype(np.float64)
    a = rng.uniform(1e-5, 1, (B, Lq, H, L, P))
    size = shapes.astype(np.float64)[None, None, None, :, None, ::-1]
    pix = loc * size - 0.5
    return dict(shapes=shapes, lsi=lsi, loc=loc,
                value=f16_rounded(rng.standard_normal((B, S, H, C))),
                attn=(a / a.sum((-1, -2), keepdims=True)).astype(np.float32).astype(np.float64),
                level_w=(a / a.sum(-2, keepdims=True)).astype(np.float32).astype(np.float64),
                grad_out=f16_rounded(rng.standard_normal((B, Lq, H * C))),
                grad_mask=f16_rounded(rng.standard_normal((B, Lq, P, H * C))),
                on_edge=(np.abs(pix - np.round(pix)) < 1e-4).any(-1, keepdims=True))


def run_ops(g, kind, variant):
    from boxer_amd import _lib, ops
    _lib.set_variant(VARIANTS[variant])
    value, loc, attn = dev(g["value"], F16), dev(g["loc"], torch.float32), dev(g["attn"], torch.float32)
    shapes, lsi, gout = dev(g["shapes"]), dev(g["lsi"]), dev(g["grad_out"], F16)
    if kind == "box":
        out = ops.box_attn_forward(value, shapes, lsi, loc, attn, 64)
        grads = ops.box_attn_backward(value, shapes, lsi, loc, attn, gout, 64)
        torch.cuda.synchronize()
        return [out] + list(grads)
    lw = dev(g["level_w"], torch.float32)
    gm = dev(g["grad_mask"], F16)
    out, mask = ops.instance_attn_forward(value, shapes, lsi, loc, attn, lw, 64)
    grads = ops.instance_attn_backward(value, shapes, lsi, loc, attn, lw, gout, gm, 64)
    torch.cuda.synchronize()
    return [out, mask] + list(grads)


def oracle(g, kind):
    if kind == "box":
        a = (g["value"], g["shapes"], g["lsi"], g["loc"], g["attn"])
        return [oc.box_attn_forward(*a)] + list(oc.box_attn_backward(*a, g["grad_out"]))
    a = (g["value"], g["shapes"], g["lsi"], g["loc"], g["attn"], g["level_w"])
    return list(oc.instance_attn_forward(*a)) + list(oc.instance_attn_backward(*a, g["grad_out"], g["grad_mask"]))


NAMES = {"box": ("out", "grad_value", "grad_loc", "grad_attn"),
         "instance": ("out", "mask_out", "grad_value", "grad_loc", "grad_spatial_w", "grad_level_w")}


# ------------------------------------------------------------------ 1. every kernel family and variant
# (the first-generation fast kernels, variant 2, take C in {16, 32, 64}; C = 24 runs the generic kernels)
CASES = [(C, v) for C in (16, 32, 64) for v in ("auto", "generic", "atomic")] + [(24, "auto"), (24, "generic")]


@pytest.mark.parametrize("C,variant", CASES, ids=["C%d-%s" % c for c in CASES])
@pytest.mark.parametrize("kind", ["box", "instance"])
def test_f16_matches_oracle(kind, C, variant):
    g = seeded([(23, 31), (12, 16), (6, 8), (3, 4)], 2, 8, C, 300, 4, seed=C + 7)
    got = run_ops(g, kind, variant)
    want = oracle(g, kind)
    for name, t, w in zip(NAMES[kind], got, want):
        assert t.dtype == (F16 if name in ("out", "mask_out", "grad_value") else torch.float32), name
        check(t, w, "%s C=%d %s: %s" % (kind, C, variant, name), ignore=g["on_edge"] if name == "grad_loc" else None)


@pytest.mark.parametrize("C", [16, 32, 64])
@pytest.mark.parametrize("kind", ["box", "instance"])
def test_f16_binned_backward_is_eligible(kind, C):
    """Variant 3 raises when the destination-binned backward cannot run: f16 must be sized and planned as 16-bit
    storage (a float32-sized workspace would fall back to the atomic kernels)."""
    g = seeded([(23, 31), (12, 16), (6, 8), (3, 4)], 2, 8, C, 300, 4, seed=C)
    got = run_ops(g, kind, "binned")
    want = oracle(g, kind)
    for name, t, w in zip(NAMES[kind], got, want):
        check(t, w, "%s C=%d binned: %s" % (kind, C, name), ignore=g["on_edge"] if name == "grad_loc" else None)


# ------------------------------------------------------------------ 2. the bench workloads at full size
def parity(inp, out, grads):
    report = bench.parity_report(inp, out, grads)
    for (name, worst, _tol), t in zip(report, bench.step_outputs(inp["kind"], out, grads)):
        assert worst <= tol_of(t), "%s: worst |err| / (max(1, rms) + |want|) = %.3e > %.0e" % (name, worst, tol_of(t))


@pytest.mark.parametrize("workload", sorted(bench.WORKLOADS))
def test_f16_bench_workload_matches_oracle(workload):
    from boxer_amd import ops
    inp = bench.make_inputs(workload, F16, "cuda", family="model", seed=0)
    plans = []
    orig = ops._forward_train

    def spy(*a, **k):
        plans.append(orig(*a, **k))
        return plans[-1]
    ops._forward_train = spy
    try:
        out, grads = bench.make_step(inp)()
    finally:
        ops._forward_train = orig
    torch.cuda.synchronize()
    assert plans and plans[-1] is not None, "the training forward did not build a backward plan"
    parity(inp, out, grads)


# ------------------------------------------------------------------ 3. encoder case: staged / riders / one pass


def encoder_case(seed=3):
    name = "_f16_encoder"
    bench.WORKLOADS[name] = (list(LEVELS4), "S", 4, "box")
    try:
        return bench.make_inputs(name, F16, "cuda", family="model", seed=seed)
    finally:
        del bench.WORKLOADS[name]


def train_step(inp):
    from boxer_amd import ops
    v, sh, ls, loc, attn, go = (inp[k] for k in ("value", "shapes", "lsi", "loc", "attn", "grad_out"))
    out, plan = ops.box_attn_forward_train(v, sh, ls, loc, attn, 64)
    grads = ops.box_attn_backward(v, sh, ls, loc, attn, go, 64, plan=plan)
    return out, grads


def state_counts():
    """(window counters: sum over the locality pairs, one-pass chain calls) over the state buffers ops keeps."""
    from boxer_amd import ops
    torch.cuda.synchronize()
    win = calls = 0
    for st in ops._STATE.values():
        win += int(st[:1024].view(torch.int64).sum().item())
        calls += int(st[STAT_OFF:STAT_OFF + 8].view(torch.int64).item())
    return win, calls


@pytest.mark.parametrize("dense,riders", [(0, 0), (1, 0), (0, 1)], ids=["staged", "gather", "own_launches"])
def test_f16_encoder_paths(dense, riders):
    """Window-staged kernels (option 11 on) against the row gathers (off), and the riders (option 15 default)
    against launches of their own, each against the oracle, cold and warm.  The staged forward ran when the
    state's window counters grew; the one-pass fill ran when its call counter grew on the second call."""
    from boxer_amd import _lib, ops
    ops.release_workspaces()
    lib = _lib.load()
    lib.boxattn_set_option(OPT_DENSE, dense)
    lib.boxattn_set_option(OPT_RIDERS, riders)
    inp = encoder_case()
    win0, calls0 = state_counts()
    out, grads = train_step(inp)
    torch.cuda.synchronize()
    parity(inp, out, grads)                                     # cold
    win1, calls1 = state_counts()
    out2, grads2 = train_step(inp)
    torch.cuda.synchronize()
    parity(inp, out2, grads2)                                   # warm
    win2, calls2 = state_counts()
    if dense == 0:
        assert win1 > win0, "the window-staged forward did not run (no locality counts)"
    if riders == 0:
        assert calls2 > calls1, "the second call did not fill its bins in one pass"
    assert torch.equal(out, out2)


# ------------------------------------------------------------------ 4. correctly rounded single contributions
@pytest.mark.parametrize("C", [16, 32, 64])
def test_f16_accumulate_single_terms_are_correctly_rounded(C):
    """The matrix-core accumulate splits every float32 weight w into two f16 terms, w ~ hi + lo, hi = f16(w),
    lo = f16(w - hi).  One point per (query, head) on a map with one query: every grad_value element is ONE
    product w * g (w = bilinear weight x attention weight, g an f16 number of grad_out), so the stored value must
    be that product rounded once to f16.  Bound, per element:
      |w - hi| <= 2^-11 |w| exactly representable in float32, so |w - hi - lo| <= 2^-11 |w - hi| <= 2^-22 |w|
        while w - hi is an f16 normal number, and <= 2^-25 (half the f16 subnormal spacing 2^-24) below it;
      hi * g and lo * g are exact in float32 (11 x 11 bits), their float32 sum rounds by <= 2^-24 |w g|;
      the kernel forms w in float32 (two roundings, <= 2^-23 |w|) where the oracle is exact;
    so before the final rounding the sum is within 2^-21 |w g| + 2^-25 |g| of w g, and the result within half an
    f16 ulp of w g plus that slack.  A one-term split (lo dropped) is off by up to 2^-11 |w g| = another half ulp,
    which this bound rejects (checked below on the same data)."""
    rng = np.random.default_rng(4321 + C)
    shapes = np.asarray([(8, 16)], dtype=np.int64)
    B, H, Lq, P = 2, 8, 1, 1
    S = int(shapes.prod(1).sum())
    g = dict(shapes=shapes, lsi=np.zeros(1, dtype=np.int64),
             value=f16_rounded(rng.standard_normal((B, S, H, C))),
             # dyadic locations: the pixel coordinate loc * size - 0.5 and its fractions are exact in float32
             loc=(rng.integers(16, 112, (B, Lq, H, 1, P, 2)) / 128.0 + 1.0 / 512),
             attn=rng.uniform(0.2, 1.0, (B, Lq, H, 1, P)).astype(np.float32).astype(np.float64),
             level_w=np.ones((B, Lq, H, 1, P)),
             grad_out=f16_rounded(rng.uniform(0.25, 4.0, (B, Lq, H * C)) * rng.choice([-1, 1], (B, Lq, H * C))),
             grad_mask=np.zeros((B, Lq, P, H * C)))
    want = oc.box_attn_backward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attn"], g["grad_out"])[0]
    gv = run_ops(g, "box", "binned")[1]
    got = gv.double().cpu().numpy()
    nz = want != 0
    assert nz.sum() == B * H * 4 * C                         # four corners per point, all inside
    assert (got[~nz] == 0).all()
    gsc = np.broadcast_to(np.abs(g["grad_out"]).reshape(B, 1, H, C), want.shape)[nz]
    w = want[nz]
    half_ulp = 2.0 ** (np.maximum(np.floor(np.log2(np.abs(w))), -14) - 11)
    bound = half_ulp + 2.0 ** -21 * np.abs(w) + 2.0 ** -25 * gsc
    worst = float((np.abs(got[nz] - w) / bound).max())
    assert worst <= 1.0, "worst error %.4f of the bound" % worst
    # the bound is tight enough to tell: the product of a ONE-term split, rounded, fails it
    gs = np.broadcast_to(g["grad_out"].reshape(B, 1, H, C), want.shape)[nz]
    hi_only = (w / gs).astype(np.float16).astype(np.float64) * gs
    one_term = hi_only.astype(np.float16).astype(np.float64)
    assert float((np.abs(one_term - w) / bound).max()) > 1.0


# ------------------------------------------------------------------ 5. determinism, HIP graphs
def test_f16_binned_backward_is_reproducible_and_graph_replays():
    """Warm calls (one-pass fill) give bitwise the same output and point gradients run to run; grad_value
    matches to within f16 rounding (the fill claims record slots with atomics, so the order in which the
    matrix cores sum a pixel's records -- and the last float32 bit -- may differ, as for bf16:
    tests/test_gpu_onepass.py soak).  A fwd+bwd step captured in a HIP graph replays to the eager results."""
    from boxer_amd import ops
    ops.release_workspaces()
    inp = encoder_case(seed=5)
    train_step(inp)                                            # cold call: plans the one-pass ranges
    eager = [train_step(inp) for _ in range(3)]
    torch.cuda.synchronize()

    def same(got, ref, what):
        out, grads = got
        assert torch.equal(out, ref[0]), what
        assert torch.equal(grads[1], ref[1][1]) and torch.equal(grads[2], ref[1][2]), what
        gv, rv = grads[0].float(), ref[1][0].float()
        assert float((gv - rv).abs().max()) <= 1e-3 * max(1.0, float(rv.abs().max())), what
    for k, got in enumerate(eager[1:]):
        same(got, eager[0], "eager call %d" % (k + 1))
    replay = bench.graph_step(lambda: train_step(inp))
    for _ in range(3):
        replay()
    torch.cuda.synchronize()
    out, grads = replay.__self__._keep
    same((out, grads), eager[0], "graph replay")
    parity(inp, out, grads)


# ------------------------------------------------------------------ 6. modules with native_f16 (G9 goldens)


def g9_run(name, mode, fused_grid, fused_pointwise):
    """mode "autocast": a float32 module under torch.autocast(float16); mode "half": the module after .half()."""
    import boxer_amd
    from boxer_amd import ops
    cls_name, kw, n_out = G9[name]
    g = golden_io.load(name)
    m = getattr(boxer_amd, cls_name)(d_model=256, num_level=4, num_head=8, **kw)
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    dtype = F16 if mode == "half" else torch.float32
    m = m.cuda().to(dtype)
    m.fused_grid, m.fused_pointwise, m.native_f16 = fused_grid, fused_pointwise, True
    if cls_name == "InstanceAttention":
        m.inferencing = False

    def t(key, grad=False):
        if key not in g:
            return None
        x = dev(g[key])
        x = x.to(dtype) if x.is_floating_point() else x
        return x.requires_grad_() if grad else x
    query, value, rw = t("query", True), t("value", True), t("ref_windows", True)
    calls = []
    orig = ops._forward_train

    def spy(name_, value_, *a, **k):
        calls.append(value_.dtype)
        return orig(name_, value_, *a, **k)
    ops._forward_train = spy
    try:
        with torch.autocast("cuda", dtype=F16, enabled=mode == "autocast"):
            outs = m(query, value, dev(g["shapes"]), t("v_mask"), dev(g["lsi"]), t("ratios"), rw)[:n_out]
        loss = sum((o.double() * dev(g["gout%d" % i]).double()).sum() for i, o in enumerate(outs))
        loss.backward()
    finally:
        ops._forward_train = orig
    grads = {"query": query.grad, "value": value.grad, "ref_windows": rw.grad}
    grads.update({"param." + k: p.grad for k, p in m.named_parameters()})
    return m, outs, grads, g, calls, dtype


@pytest.mark.parametrize("mode", ["autocast", "half"])
@pytest.mark.parametrize("fused_pointwise", [False, True], ids=["torch_pointwise", "fused_pointwise"])
@pytest.mark.parametrize("fused_grid", [0, 1])
@pytest.mark.parametrize("name", sorted(G9))
def test_f16_modules_match_reference_goldens(name, fused_grid, fused_pointwise, mode):
    """Outputs and every gradient against the reference module's float64 autograd, within the 2e-2 of the bf16
    module test (the dense layers run in f16 too); the f16 operator ran (float16 value into the training entry);
    gradients come back in the inputs' dtypes.  The gradients that flow through the sampling LOCATIONS are held to
    the root-mean-square criterion, as in the bf16 test: a few points land across a bilinear cell edge."""
    from boxer_amd import ops
    ops.release_workspaces()
    m, outs, grads, g, calls, dtype = g9_run(name, mode, fused_grid, fused_pointwise)
    assert calls and all(c == F16 for c in calls), calls
    for k, v in grads.items():
        assert v is not None and v.dtype == dtype, (k, None if v is None else v.dtype)
    worst = {}

    def errs(got, want):
        got = got.detach().double().cpu().numpy()
        want = np.asarray(want, dtype=np.float64).reshape(got.shape)
        return (float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max())),
                float(np.sqrt(((got - want) ** 2).mean()) / max(1e-30, np.sqrt((want ** 2).mean()))))
    for i, o in enumerate(outs):
        worst["out%d" % i] = errs(o, g["out%d" % i])[0]
    location_path = ("ref_windows", "linear_box", "query")
    for k, v in grads.items():
        key = "grad_" + k if not k.startswith("param.") else "grad." + k[6:]
        e_max, e_rms = errs(v, g[key])
        worst[k] = e_rms / 2 if any(r in k for r in location_path) else e_max
    # After .half() the box decoding runs in float16 too: reference windows, offsets and the sampling grid are
    # 11-bit numbers (a location on a 100-pixel level moves by up to 0.05 px), so the location-path gradients are
    # held to the rms criterion at the 4e-2 ... 5e-2 that such a model's own geometry allows (the bf16 G9 test
    # allows 4e-2 under autocast, where the grid stays float32); everything else to 2e-2.
    loose = 5e-2 if mode == "half" else 2e-2
    bad = {k: v for k, v in worst.items()
           if not v <= (loose if any(r in k for r in location_path) else 2e-2)}
    assert not bad, "%s (%s, fused_grid=%s pointwise=%s): errors above 2e-2: %s" % (
        name, mode, fused_grid, fused_pointwise, bad)


def test_native_bf16_and_native_f16_are_exclusive():
    from boxer_amd import BoxAttention
    m = BoxAttention(d_model=256, num_level=4, num_head=8, kernel_size=2).cuda()
    m.native_bf16 = m.native_f16 = True
    with pytest.raises(ValueError):
        m._box_function()


# ------------------------------------------------------------------ 7. the compiled module
def test_compiled_module_with_half_value_matches_ops():
    from boxer_amd import _ext, ops
    mod = _ext.load()
    for workload in ("C2", "C3"):
        inp = bench.make_inputs(workload, F16, "cuda", family="model", batch=1, seed=2)
        v, sh, ls, loc, attn, go = (inp[k] for k in ("value", "shapes", "lsi", "loc", "attn", "grad_out"))
        if inp["kind"] == "box":
            a = mod.box_attn_forward(v, sh, ls, loc, attn, 64)
            b = ops.box_attn_forward(v, sh, ls, loc, attn, 64)
            ga = mod.box_attn_backward(v, sh, ls, loc, attn, go, 64)
            gb = ops.box_attn_backward(v, sh, ls, loc, attn, go, 64)
            outs = [(a, b)]
        else:
            lw, gm = inp["level_w"], inp["grad_mask"]
            a = mod.instance_attn_forward(v, sh, ls, loc, attn, lw, 64)
            b = ops.instance_attn_forward(v, sh, ls, loc, attn, lw, 64)
            ga = mod.instance_attn_backward(v, sh, ls, loc, attn, lw, go, gm.view_as(a[1]), 64)
            gb = ops.instance_attn_backward(v, sh, ls, loc, attn, lw, go, gm.view_as(b[1]), 64)
            outs = list(zip(a, b))
        torch.cuda.synchronize()
        assert (a[0] if isinstance(a, (list, tuple)) else a).dtype == F16
        # forward outputs and point gradients bit for bit; grad_value to f16 rounding (the binned fill claims
        # record slots with atomics: the order of a pixel's sum may differ from call to call, as for bf16)
        for x, y in outs + list(zip(ga[1:], gb[1:])):
            assert x.dtype == y.dtype and torch.equal(x, y), workload
        assert ga[0].dtype == gb[0].dtype == F16
        gv_a, gv_b = ga[0].float(), gb[0].float()
        assert float((gv_a - gv_b).abs().max()) <= 1e-3 * max(1.0, float(gv_b.abs().max())), workload


# ------------------------------------------------------------------ 8. pointwise passes
@pytest.mark.parametrize("n", [16, 12, 40])
def test_f16_softmax_passes_match_torch(n):
    from boxer_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(n)
    logits = torch.randn(2, 300, 8, n, device="cuda", generator=gen).to(F16)
    attn = ops.softmax_forward(logits)
    want = torch.softmax(logits.float(), -1)
    assert attn.dtype == torch.float32
    assert float((attn - want).abs().max()) <= 1e-6
    ga = torch.randn(attn.shape, device="cuda", generator=gen)
    gl = ops.softmax_backward(attn, ga, F16)
    want_gl = (want * (ga - (want * ga).sum(-1, keepdim=True))).to(F16)
    assert gl.dtype == F16
    diff = (gl.float() - want_gl.float()).abs()
    assert float((diff / (want_gl.float().abs() * 2.0 ** -10 + 2.0 ** -24)).max()) <= 1.0 + 1e-3


@pytest.mark.parametrize("src", [torch.float32, F16])
def test_f16_value_cast_matches_torch(src):
    from boxer_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(7)
    value = (torch.randn(2, 1000, 256, device="cuda", generator=gen) * 100).to(src)
    mask = torch.rand(2, 1000, device="cuda", generator=gen) < 0.3
    for m in (mask, None):
        got = ops.value_mask_cast(value, m, F16)
        want = value if m is None else value.masked_fill(m[..., None], 0)
        assert got.dtype == F16 and torch.equal(got, want.to(F16))
    big = torch.full((4, 8), 1e6, device="cuda")
    assert torch.isinf(ops.value_mask_cast(big, None, F16)).all()         # no overflow guarding: inf, as .half()
