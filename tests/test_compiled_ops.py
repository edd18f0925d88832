"""The compiled operator module (boxer_amd/csrc/e2edet_ops.cpp): the reference's pybind11 module
``e2edet.ops`` (vision.cpp:7-12) on the C ABI.

CPU: it builds with the host compiler, loads, exports the reference's four functions and refuses
CPU tensors the way the reference does (box_attn.h:53 "Not implemented on the CPU").
GPU: the four functions against the reference's golden vectors (fp64 / fp32 / bf16 storage), and
autograd Functions written the way the reference writes them (``_C.box_attn_forward(...)`` in
forward, ``_C.box_attn_backward(...)`` in backward, box_attention_func.py:9-64) running on it.
"""
import numpy as np
import pytest
import torch

import golden_io
from compare_rules import PARITY_TOL as TOL
from route_vocab import _cdt


@pytest.fixture(scope="module")
def compiled():
    from boxer_amd import _ext
    _ext.build()
    return _ext.load()


def test_module_exports_the_reference_functions(compiled):
    from boxer_amd import _ext, _lib
    for name in _ext.FUNCTIONS:
        assert callable(getattr(compiled, name)), name
    assert compiled.abi_version() == _lib.ABI_VERSION


def test_cpu_tensors_are_refused(compiled):
    value = torch.zeros(1, 4, 1, 4)
    shapes = torch.tensor([[2, 2]])
    lsi = torch.zeros(1, dtype=torch.long)
    loc = torch.zeros(1, 1, 1, 1, 1, 2)
    attn = torch.ones(1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        compiled.box_attn_forward(value, shapes, lsi, loc, attn, 64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        compiled.instance_attn_forward(value, shapes, lsi, loc, attn, attn, 64)


# ------------------------------------------------------------------ GPU


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(dtype) if dtype is not None else t


def _close(got, want, tol, what):
    got = got.detach().double().cpu().numpy()
    want = np.asarray(want, dtype=np.float64).reshape(got.shape)
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    assert err <= tol, "%s: max scaled err %.3e > %.1e" % (what, err, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["G1_box_reftest", "G3_box_C32", "G5_box_C1", "G6_box_ml"])
def test_box_functions_match_goldens(compiled, name, dtype):
    if dtype == torch.bfloat16 and name not in ("G5_box_C1", "G6_box_ml"):
        pytest.skip("bf16 storage is pinned on the fixtures whose inputs are exact in bf16")
    g = golden_io.load(name)
    cdt = _cdt(dtype)
    value, loc, attn = _dev(g["value"], dtype), _dev(g["loc"], cdt), _dev(g["attn"], cdt)
    shapes, lsi = _dev(g["shapes"]), _dev(g["lsi"])
    out = compiled.box_attn_forward(value, shapes, lsi, loc, attn, 64)
    gv, gl, ga = compiled.box_attn_backward(value, shapes, lsi, loc, attn,
                                            _dev(g["grad_out"], dtype), 64)
    torch.cuda.synchronize()
    assert out.dtype == dtype and gv.dtype == dtype and gl.dtype == cdt and ga.dtype == cdt
    _close(out, g["out"], TOL[dtype], "out")
    _close(gv, g["grad_value"], TOL[dtype], "grad_value")
    _close(gl, g["grad_loc"], TOL[cdt], "grad_loc")
    _close(ga, g["grad_attn"], TOL[cdt], "grad_attn")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["G2_inst_reftest", "G6_inst_ms4", "G6_inst_ms14"])
def test_instance_functions_match_goldens(compiled, name, dtype):
    if dtype == torch.bfloat16 and name == "G2_inst_reftest":
        pytest.skip("bf16 storage is pinned on the fixtures whose inputs are exact in bf16")
    g = golden_io.load(name)
    cdt = _cdt(dtype)
    value, loc = _dev(g["value"], dtype), _dev(g["loc"], cdt)
    sw, lw = _dev(g["spatial_w"], cdt), _dev(g["level_w"], cdt)
    shapes, lsi = _dev(g["shapes"]), _dev(g["lsi"])
    gm = g["grad_mask"]
    gmask = _dev(gm.reshape(gm.shape[0], gm.shape[1], -1, gm.shape[-1]), dtype)
    out, mask = compiled.instance_attn_forward(value, shapes, lsi, loc, sw, lw, 64)
    gv, gl, gs, glw = compiled.instance_attn_backward(value, shapes, lsi, loc, sw, lw,
                                                      _dev(g["grad_out"], dtype), gmask, 64)
    torch.cuda.synchronize()
    _close(out, g["out"], TOL[dtype], "out")
    _close(mask, g["mask_out"], TOL[dtype], "mask_out")
    _close(gv, g["grad_value"], TOL[dtype], "grad_value")
    _close(gl, g["grad_loc"], TOL[cdt], "grad_loc")
    _close(gs, g["grad_spatial"], TOL[cdt], "grad_spatial")
    _close(glw, g["grad_level"], TOL[cdt], "grad_level")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["box", "instance"])
def test_same_results_as_the_ctypes_binding(compiled, kind, dtype):
    """Both bindings marshal into the same library, from the same device tensors.  float32 and the 16-bit types:
    identical forward, location- and weight-gradient bits; grad_value to the order of its sums (float32: rtol 1e-5,
    atol 1e-6; 16-bit: 1e-3 of the largest element, the bound of test_gpu_f16's compiled-module test).  float64:
    every tensor to the parity tolerance -- its backward adds with atomics, no bits are claimed.
    The forward runs twice: with nothing requiring a gradient (the plain / host-table entries) and with the inputs
    requiring one (the training entries; the backward then meets whatever plan they parked), so that every entry
    point the module calls is compared in every storage type that has it."""
    from boxer_amd import ops
    from compare_rules import close_parity
    g = golden_io.load("G6_box_ml" if kind == "box" else "G6_inst_ms4")
    cdt = torch.float64 if dtype == torch.float64 else torch.float32       # locations, weights and their gradients
    weights = ("attn",) if kind == "box" else ("spatial_w", "level_w")
    value, loc = _dev(g["value"], dtype), _dev(g["loc"], cdt)
    ws = [_dev(g[k], cdt) for k in weights]
    shapes, lsi = _dev(g["shapes"]), _dev(g["lsi"])
    grads = [_dev(g["grad_out"], dtype)]
    if kind == "instance":
        gm = g["grad_mask"]
        grads.append(_dev(gm.reshape(gm.shape[0], gm.shape[1], -1, gm.shape[-1]), dtype))
    fwd, bwd = "%s_attn_forward" % kind, "%s_attn_backward" % kind

    def same(a, b, what):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        if dtype == torch.float64:
            close_parity(a, b.detach().cpu().numpy(), torch.float64, what)
        else:
            assert torch.equal(a, b), what

    def forwards(what):
        a = getattr(compiled, fwd)(value, shapes, lsi, loc, *ws, 64)
        b = getattr(ops, fwd)(value, shapes, lsi, loc, *ws, 64)
        a, b = ([a], [b]) if kind == "box" else (a, b)
        assert len(a) == len(b) == len(grads)
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s output %d" % (what, i))

    forwards("inference forward")
    for t in [value, loc] + ws:
        t.requires_grad_()
    forwards("training forward")
    ga = getattr(compiled, bwd)(value, shapes, lsi, loc, *ws, *grads, 64)
    gb = getattr(ops, bwd)(value, shapes, lsi, loc, *ws, *grads, 64)
    assert len(ga) == len(gb) == 2 + len(ws)
    for i in range(1, len(ga)):
        same(ga[i], gb[i], "gradient %d" % i)
    if dtype == torch.float64:
        same(ga[0], gb[0], "grad_value")
    elif dtype == torch.float32:
        assert ga[0].dtype == gb[0].dtype == dtype
        assert torch.allclose(ga[0], gb[0], rtol=1e-5, atol=1e-6)
    else:
        assert ga[0].dtype == gb[0].dtype == dtype
        gv_a, gv_b = ga[0].float(), gb[0].float()
        assert float((gv_a - gv_b).abs().max()) <= 1e-3 * max(1.0, float(gv_b.abs().max()))


@pytest.mark.gpu
def test_error_behaviour(compiled):
    g = golden_io.load("G6_box_ml")
    value, loc, attn = (_dev(g[k], torch.float32) for k in ("value", "loc", "attn"))
    shapes, lsi = _dev(g["shapes"]), _dev(g["lsi"])
    with pytest.raises(RuntimeError, match="must be contiguous"):
        compiled.box_attn_forward(value.transpose(2, 3), shapes, lsi, loc, attn, 64)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        compiled.box_attn_forward(value.cpu(), shapes, lsi, loc, attn, 64)
    # the backward's own refusals, all before any launch
    gout = _dev(g["grad_out"], torch.float32)
    with pytest.raises(RuntimeError, match="must have the dtype of value"):
        compiled.box_attn_backward(value, shapes, lsi, loc, attn, gout.double(), 64)
    with pytest.raises(RuntimeError, match=r"B\*Lq\*H\*C elements"):
        compiled.box_attn_backward(value, shapes, lsi, loc, attn, gout.flatten()[:-1].contiguous(), 64)
    gi = golden_io.load("G6_inst_ms4")
    ivalue, iloc, sw, lw = (_dev(gi[k], torch.float32) for k in ("value", "loc", "spatial_w", "level_w"))
    ishapes, ilsi, igout = _dev(gi["shapes"]), _dev(gi["lsi"]), _dev(gi["grad_out"], torch.float32)
    gm = gi["grad_mask"]
    gmask = _dev(gm.reshape(gm.shape[0], gm.shape[1], -1, gm.shape[-1]), torch.float32)
    with pytest.raises(RuntimeError, match="wrong number of elements"):
        compiled.instance_attn_backward(ivalue, ishapes, ilsi, iloc, sw, lw, igout, gmask[:, :, :-1].contiguous(), 64)
    assert not gmask.transpose(1, 2).is_contiguous()
    with pytest.raises(RuntimeError, match="grad_mask_output must be contiguous"):
        compiled.instance_attn_backward(ivalue, ishapes, ilsi, iloc, sw, lw, igout, gmask.transpose(1, 2), 64)
    b = value.size(0)
    if b % 2 == 1:
        value, loc, attn = (torch.cat([t, t]) for t in (value, loc, attn))
    with pytest.raises(RuntimeError, match="must divide"):
        compiled.box_attn_forward(torch.cat([value, value[:1]]), shapes, lsi,
                                  torch.cat([loc, loc[:1]]), torch.cat([attn, attn[:1]]), 2)


@pytest.mark.gpu
def test_reference_style_function_on_the_compiled_module(compiled):
    """An autograd Function in the reference's shape (forward saves the five tensors and calls
    ``_C.box_attn_forward``; backward calls ``_C.box_attn_backward`` and returns
    (grad_value, None, None, grad_loc, grad_attn, None)) passes gradcheck in float64 on it."""
    from torch.autograd import Function, gradcheck
    from torch.autograd.function import once_differentiable
    _C = compiled

    class RefStyleBoxAttn(Function):
        @staticmethod
        def forward(ctx, value, shapes, lsi, loc, attn, im2col_step):
            ctx.im2col_step = im2col_step
            ctx.save_for_backward(value, shapes, lsi, loc, attn)
            return _C.box_attn_forward(value, shapes, lsi, loc, attn, im2col_step)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_output):
            value, shapes, lsi, loc, attn = ctx.saved_tensors
            gv, gl, ga = _C.box_attn_backward(value, shapes, lsi, loc, attn,
                                              grad_output.contiguous(), ctx.im2col_step)
            return gv, None, None, gl, ga, None

    shapes = torch.tensor([(6, 4), (3, 2)], dtype=torch.long, device="cuda")
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    S = int(shapes.prod(1).sum())
    torch.manual_seed(5)
    value = (torch.rand(1, S, 2, 32, device="cuda", dtype=torch.double) * 0.01).requires_grad_()
    loc = torch.rand(1, 2, 2, 2, 2, 2, device="cuda", dtype=torch.double).requires_grad_()
    attn = torch.rand(1, 2, 2, 2, 2, device="cuda", dtype=torch.double) + 1e-5
    attn = (attn / attn.sum((-1, -2), keepdim=True)).requires_grad_()
    assert gradcheck(RefStyleBoxAttn.apply, (value, shapes, lsi, loc, attn, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["box", "instance"])
def test_reference_style_functions_get_the_parked_plan(compiled, dtype, kind):
    """Functions in the reference's own shape (bench.reference_style_functions: forward calls ``_C.*_forward``,
    backward calls ``_C.*_backward`` with the saved tensors only -- box_attention_func.py:10-150) on the compiled
    module: the forward parks the plan its launch prepared, the backward takes it -- no count / scan launches in the
    backward (the library's "bwd_binning" timing slot stays empty) -- and the gradients are the golden ones.
    Without gradient requirements nothing is parked; the module caches the host level tables per tensor object and
    one scratch tensor per stream (no device -> host copy and no allocation per call)."""
    import bench
    from boxer_amd import _lib
    _lib.set_option("riders", 4)     # (two-pass riders: box attention parks a plan too; its default backward -- the
                                     # one-pass fill -- takes none: test_one_pass_backward_through_the_compiled_module)
    g = golden_io.load("G6_box_ml" if kind == "box" else "G6_inst_ms4")    # (inputs exact in bf16)
    compiled.release_buffers()
    ref_box, ref_inst = bench.reference_style_functions(compiled)
    cdt = torch.float32
    shapes, lsi = _dev(g["shapes"]), _dev(g["lsi"])
    v = _dev(g["value"], dtype).requires_grad_()
    l = _dev(g["loc"], cdt).requires_grad_()
    tol = TOL[dtype]
    _lib.profile_begin()
    try:
        if kind == "box":
            a = _dev(g["attn"], cdt).requires_grad_()
            out = ref_box.apply(v, shapes, lsi, l, a, 64)
            assert compiled.parked_plans() == 1
            out.backward(_dev(g["grad_out"], dtype))
        else:
            sw, lw = _dev(g["spatial_w"], cdt).requires_grad_(), _dev(g["level_w"], cdt).requires_grad_()
            out, mask = ref_inst.apply(v, shapes, lsi, l, sw, lw, 64)
            assert compiled.parked_plans() == 1
            torch.autograd.backward([out, mask], [_dev(g["grad_out"], dtype),
                                                  _dev(g["grad_mask"], dtype).reshape(mask.shape)])
        torch.cuda.synchronize()
    finally:
        slots = _lib.profile_end()
    assert compiled.parked_plans() == 0
    assert slots["bwd_binning"]["launches"] == 0, slots
    _close(out, g["out"], tol, "out")
    _close(v.grad, g["grad_value"], tol, "grad_value")
    if kind == "box":
        _close(a.grad, g["grad_attn"], max(tol, 1e-4), "grad_attn")
        with torch.no_grad():          # nothing requires a gradient: an inference forward, nothing parked
            compiled.box_attn_forward(v.detach(), shapes, lsi, l.detach(), a.detach(), 64)
        assert compiled.parked_plans() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_pass_backward_through_the_compiled_module(compiled, dtype):
    """The reference's four functions, default switches, an encoder shape (one query per pixel): box attention's
    backward fills its bins in one pass from the ranges in the module's per-geometry state buffer -- the forward parks
    nothing, and from the second step on the backward launches no count / scan / fill pass of its own; every step's
    tensors are the oracle's."""
    import bench
    from boxer_amd import _lib
    bench.WORKLOADS["_compiled_enc"] = ([(37, 53), (19, 27), (10, 14), (5, 7)], "S", 4, "box")
    try:
        inp = bench.make_inputs("_compiled_enc", dtype, "cuda", family="model", batch=2, seed=2)
    finally:
        del bench.WORKLOADS["_compiled_enc"]
    compiled.release_buffers()
    ref_box, _ = bench.reference_style_functions(compiled)
    for it in range(3):
        v, l, a = (inp[k].detach().clone().requires_grad_() for k in ("value", "loc", "attn"))
        _lib.profile_begin()
        try:
            out = ref_box.apply(v, inp["shapes"], inp["lsi"], l, a, 64)
            assert compiled.parked_plans() == 0
            out.backward(inp["grad_out"])
            torch.cuda.synchronize()
        finally:
            slots = _lib.profile_end()
        assert (slots["bwd_binning"]["launches"] > 0) == (it == 0), (it, slots)
        for name, worst, tol in bench.parity_report(inp, out, [v.grad, l.grad, a.grad]):
            assert worst <= tol, (it, name, worst)


@pytest.mark.gpu
def test_runs_on_the_current_stream(compiled):
    """The module launches on torch's CURRENT stream of the tensors' device (c10's stream guard):
    work queued on a side stream behind a long-running kernel must see that kernel's result."""
    g = golden_io.load("G6_box_ml")
    value, loc, attn = (_dev(g[k], torch.float32) for k in ("value", "loc", "attn"))
    shapes, lsi = _dev(g["shapes"]), _dev(g["lsi"])
    want = compiled.box_attn_forward(value, shapes, lsi, loc, attn, 64)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    scratch = torch.zeros_like(value)
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(20):                       # keeps the side stream busy for a while
            big = big @ big * 1e-4
        scratch.copy_(value)                      # queued behind the matmuls, on the side stream
        out = compiled.box_attn_forward(scratch, shapes, lsi, loc, attn, 64)
    side.synchronize()
    assert torch.equal(out, want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["same_stream", "new_stream"])
@pytest.mark.parametrize("kind,dtype", [("box", torch.bfloat16), ("box", torch.float32), ("instance", torch.bfloat16)],
                         ids=["box_bf16", "box_f32", "instance_bf16"])
def test_step_replayed_from_a_hip_graph_on_new_inputs(compiled, kind, dtype, mode, monkeypatch):
    """Forward + backward through the module's four functions (the reference's own Functions,
    bench.reference_style_functions) captured in a HIP graph -- warmed up on the capture stream, and captured on a stream
    that has run nothing, where the module's ``capturing()`` keeps state, workspace and plan out of its tables -- and
    replayed on a second input set and on the first again.  Each replay is held to the rule of the eager tests of the
    route (tests/test_gpu_graph_replay.py: compare_rules.check_onepass for the encoder box step, error_bounds.hold_all
    for instance attention with the binned backward required and its accumulate on the matrix cores); the bitwise
    reproducible outputs equal the ctypes binding's, called eagerly on the same inputs after the replay."""
    import bench
    import error_bounds as eb
    import graph_cases as gc
    import point_cases
    from boxer_amd import _lib, ops
    from compare_rules import check_onepass
    from route_vocab import ACC_TR, REC_POINT, routes, split_of
    monkeypatch.setattr(ops._Locality, "enabled", False)       # (the module gives no locality hint: the same kernels)
    ops.release_workspaces()
    compiled.release_buffers()
    ref_box, ref_inst = bench.reference_style_functions(compiled)
    if kind == "box":
        inputs = gc.onepass_sets("S", dtype)[:2]
        sets, leaves = inputs, ("value", "loc", "attn")
    else:
        _lib.set_option("inst_acc16", 2)
        _lib.set_variant(3)
        inputs = gc.instance_sets(point_cases.SHAPE_A, "bf16", (5, 6))
        sets, leaves = [point_cases.inst_tensors(inp, dtype) for inp in inputs], ("value", "loc", "attn", "level_w")
        fwd, acc, rec = routes(sets[0], instance=True)
        assert acc == ACC_TR and rec == REC_POINT, (acc, rec)
    static = gc.clone(sets[0], leaves=leaves)

    def step():
        a = [static[k] for k in ("value", "shapes", "lsi", "loc", "attn")]
        if kind == "box":
            outs, ups = [ref_box.apply(*a, 64)], [static["grad_out"]]
        else:
            outs, ups = list(ref_inst.apply(*a, static["level_w"], 64)), [static["grad_out"], static["grad_mask"]]
        grads = torch.autograd.grad(outs, [static[n] for n in leaves], ups)
        return [o.detach() for o in outs], list(grads)

    def check(i, kept, what):
        outs, grads = kept
        if kind == "box":
            check_onepass(sets[i], outs[0], grads, what)
            e_out, e_grads = point_cases.step(sets[i], entry="reference")
            pairs = [("out", outs[0], e_out), ("grad_loc", grads[1], e_grads[1]), ("grad_attn", grads[2], e_grads[2])]
        else:
            eb.hold_all(dict(zip(point_cases.INST_NAMES, outs + grads)), eb.reference_of(inputs[i]), dtype,
                        split_of(ACC_TR, dtype), what)
            e = point_cases.run_instance(sets[i])
            pairs = [(n, t, e[n]) for n, t in zip(point_cases.INST_NAMES, outs + grads) if n != "grad_value"]
        for name, a, b in pairs:
            assert a.dtype == b.dtype and torch.equal(a, b), "%s: %s differs from the ctypes binding's" % (what, name)
        assert compiled.parked_plans() == 0, what

    try:
        gc.replay_on(mode, step, static, sets, (0, 1, 0), check)
    finally:
        compiled.release_buffers()
        ops.release_workspaces()
