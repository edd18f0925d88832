"""GPU tests (``-m gpu``) of InstanceAttention's single-pass weights: ``ops.instance_weights_forward`` /
``_backward``, ``InstanceWeightsFunction`` and the module's ``fused_pointwise`` path.

The yardstick is the module's own torch chain -- two ``repeat_interleave`` and the two softmaxes, with autograd
for the gradients -- evaluated in float64 on the same logits (16-bit logits: on their upcast values).  The
tolerance is measured, not fixed: in the same test the chain is also run in float32, and the kernels are held to
4 x that float32 chain's error against float64 plus 2^-23 max|want| (``__expf`` is a few ulp coarser than
``expf``; the floor is one float32 ulp of the largest value, so a lucky float32 result cannot make the bound
zero).  ``grad_logits`` in a 16-bit type is compared against the float64 result rounded to the type, with one
further ulp of the type allowed.
"""
import pytest
import torch
from route_vocab import DTYPES

pytestmark = pytest.mark.gpu

MANTISSA = {torch.bfloat16: 7, torch.float16: 10}


def chain(logits, k):
    """The module's torch chain on (rows, L, 2, 2) logits -> spatial_w, level_w (rows, L, k, k)."""
    rows, L = logits.shape[:2]
    e = logits.repeat_interleave(k // 2, dim=-1).repeat_interleave(k // 2, dim=-2)
    spatial = torch.softmax(e.reshape(rows, -1), dim=-1).view(rows, L, k, k)
    return spatial, torch.softmax(e, dim=1)


def chain_with_grads(logits, k, grad_spatial, grad_level):
    z = logits.detach().clone().requires_grad_()
    spatial, level = chain(z, k)
    outs, grads = [spatial], [grad_spatial]
    if grad_level is not None:
        outs.append(level)
        grads.append(grad_level)
    torch.autograd.backward(outs, grads)
    return spatial.detach(), level.detach(), z.grad


def problem(rows, L, k, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed * 1000 + rows + 17 * L + k)
    logits = 3 * torch.randn(rows, L, 2, 2, device="cuda", generator=g)
    sign = (torch.rand(rows, 1, 1, 1, device="cuda", generator=g) < 0.5).float() * 2 - 1
    logits = (logits + 30 * sign).to(dtype)
    gs = torch.randn(rows, L, k, k, device="cuda", generator=g)
    gl = torch.randn(rows, L, k, k, device="cuda", generator=g)
    return logits, gs, gl


def err(got, want):
    return (got.double() - want).abs().max().item() if want.numel() else 0.0


def bound(err32, want):
    return 4 * err32 + 2.0 ** -23 * (want.abs().max().item() if want.numel() else 0.0)


def ulp_of(want_rounded, dtype):
    """One unit in the last place of `dtype` at each (already rounded) value, as float64."""
    w = want_rounded.double().abs()
    tiny = torch.finfo(dtype).tiny                       # (below the normal range the spacing stays that of tiny)
    return torch.exp2(torch.floor(torch.log2(w.clamp_min(tiny))) - MANTISSA[dtype])


def check_parity(rows, L, k, name):
    from boxer_amd import ops
    dtype = DTYPES[name]
    logits, gs, gl = problem(rows, L, k, dtype)
    want_s, want_l, want_g = chain_with_grads(logits.double(), k, gs.double(), gl.double())
    t32_s, t32_l, t32_g = chain_with_grads(logits.float(), k, gs, gl)

    got_s, got_l = ops.instance_weights_forward(logits, k)
    got_g = ops.instance_weights_backward(logits, gs, gl)
    assert got_s.dtype == got_l.dtype == torch.float32 and got_g.dtype == dtype
    assert got_s.shape == got_l.shape == (rows, L, k, k) and got_g.shape == logits.shape

    report = []
    for what, got, t32, want in (("spatial_w", got_s, t32_s, want_s), ("level_w", got_l, t32_l, want_l)):
        e_k, e_t = err(got, want), err(t32, want)
        report.append((what, e_k, e_t, bound(e_t, want)))
    e_t = err(t32_g, want_g)
    if dtype == torch.float32:
        report.append(("grad_logits", err(got_g, want_g), e_t, bound(e_t, want_g)))
        over = (got_g.double() - want_g).abs() - bound(e_t, want_g)
    else:
        rounded = want_g.to(dtype)
        report.append(("grad_logits (vs rounded)", err(got_g, rounded.double()), e_t, bound(e_t, want_g)))
        over = (got_g.double() - rounded.double()).abs() - bound(e_t, want_g) - ulp_of(rounded, dtype)
    for what, e_k, e_t, b in report:
        print("rows %d L %d k %d %s %s: kernel err %.3e, torch float32 chain err %.3e, bound %.3e"
              % (rows, L, k, name, what, e_k, e_t, b))
    for what, e_k, e_t, b in report[:2]:
        assert e_k <= b, (what, e_k, e_t, b)
    assert torch.isfinite(got_g.float()).all()
    assert over.max().item() <= 0, (report[2], over.max().item())


@pytest.mark.parametrize("name", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("rows", [1, 77, 4800])
@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("k", [2, 4, 14])
def test_forward_and_backward_parity(k, L, rows, name):
    check_parity(rows, L, k, name)


@pytest.mark.parametrize("name", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("k,L,rows", [(6, 3, 101), (8, 5, 33), (2, 16, 50), (32, 16, 9), (14, 7, 3), (32, 1, 130)])
def test_parity_at_padded_levels_and_the_largest_shapes(k, L, rows, name):
    """Level counts that are not powers of two leave dead lanes in a row's group; L = 16 and k = 32 are the
    limits."""
    check_parity(rows, L, k, name)


@pytest.mark.parametrize("name", ["f32", "bf16", "f16"])
def test_null_legs(name):
    from boxer_amd import InstanceWeightsFunction, ops
    logits, gs, gl = problem(77, 4, 14, DTYPES[name], seed=1)
    spatial, level = ops.instance_weights_forward(logits, 14)
    only, none = ops.instance_weights_forward(logits, 14, need_level=False)
    assert none is None and torch.equal(only, spatial)

    zeros = torch.zeros_like(gl)
    assert torch.equal(ops.instance_weights_backward(logits, gs, None),
                       ops.instance_weights_backward(logits, gs, zeros))
    assert torch.equal(ops.instance_weights_backward(logits, None, gl),
                       ops.instance_weights_backward(logits, zeros, gl))

    # through the Function: a loss that uses one output only hands None for the other
    for use in (0, 1):
        z = logits.clone().requires_grad_()
        outs = InstanceWeightsFunction.apply(z, 14, True)
        (outs[use] * (gs, gl)[use]).sum().backward()
        explicit = ops.instance_weights_backward(logits, gs if use == 0 else zeros, gl if use == 1 else zeros)
        assert z.grad.dtype == logits.dtype and torch.equal(z.grad, explicit)
    z = logits.clone().requires_grad_()
    s, lv = InstanceWeightsFunction.apply(z, 14, False)
    assert lv is None
    (s * gs).sum().backward()
    assert torch.equal(z.grad, ops.instance_weights_backward(logits, gs, zeros))


@pytest.mark.parametrize("k,L", [(2, 1), (4, 2), (14, 4), (6, 3)])
def test_exact_structure(k, L):
    from boxer_amd import ops
    logits, _, _ = problem(77, L, k, torch.float32, seed=2)
    m = k // 2
    for w in ops.instance_weights_forward(logits, k):
        cells = w.view(77, L, 2, m, 2, m)
        first = cells[:, :, :, :1, :, :1].expand_as(cells)
        assert torch.equal(cells, first)                      # all m^2 values of a cell are the same bits
    spatial, level = ops.instance_weights_forward(logits, k)
    assert (spatial.double().sum(dim=(1, 2, 3)) - 1).abs().max().item() <= 1e-6
    assert (level.double().sum(dim=1) - 1).abs().max().item() <= 1e-6


def test_backward_is_reproducible_run_to_run():
    from boxer_amd import ops
    for name, dtype in DTYPES.items():
        logits, gs, gl = problem(4800, 4, 14, dtype, seed=3)
        first = ops.instance_weights_backward(logits, gs, gl)
        assert torch.equal(first, ops.instance_weights_backward(logits, gs, gl)), name


def test_gradients_that_are_views_into_a_storage():
    """The kernels read the gradients 16 bytes at a time; a contiguous view that starts off that alignment is
    taken all the same."""
    from boxer_amd import ops
    logits, gs, gl = problem(33, 4, 14, torch.float32, seed=4)
    pool = torch.zeros(gs.numel() + 1, device="cuda")
    shifted = pool[1:].view_as(gs)
    shifted.copy_(gs)
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    assert torch.equal(ops.instance_weights_backward(logits, shifted, gl),
                       ops.instance_weights_backward(logits, gs, gl))


def test_rejected_shapes_and_empty_input():
    from boxer_amd import ops
    z = torch.randn(5, 4, 2, 2, device="cuda")
    for k in (3, 0, 34, 1):
        with pytest.raises(RuntimeError):
            ops.instance_weights_forward(z, k)
    with pytest.raises(RuntimeError):
        ops.instance_weights_forward(torch.randn(5, 17, 2, 2, device="cuda"), 4)
    with pytest.raises(RuntimeError):
        ops.instance_weights_backward(torch.randn(5, 17, 2, 2, device="cuda"),
                                      torch.randn(5, 17, 4, 4, device="cuda"), None)
    with pytest.raises(RuntimeError):
        ops.instance_weights_backward(z, torch.randn(5, 4, 3, 3, device="cuda"), None)
    with pytest.raises(RuntimeError):
        ops.instance_weights_forward(torch.randn(5, 4, 2, 3, device="cuda"), 4)
    with pytest.raises(RuntimeError):
        ops.instance_weights_forward(z.cpu(), 4)
    with pytest.raises(RuntimeError):
        ops.instance_weights_forward(z.double(), 4)

    empty = torch.empty(0, 4, 2, 2, device="cuda")
    spatial, level = ops.instance_weights_forward(empty, 14)
    assert spatial.shape == level.shape == (0, 4, 14, 14) and spatial.dtype == torch.float32
    assert ops.instance_weights_backward(empty, spatial, level).shape == (0, 4, 2, 2)


# ------------------------------------------------------------------------------------------ the module
class Spy:
    """Records the library calls of the weight passes (ops._grid_call: name, anchor, arguments)."""

    def __init__(self, monkeypatch):
        from boxer_amd import ops
        self.calls = []
        inner = ops._grid_call

        def wrapper(name, anchor, *args):
            if name.startswith("instattn_weights_"):
                self.calls.append((name, args))
            return inner(name, anchor, *args)
        monkeypatch.setattr(ops, "_grid_call", wrapper)

    def forwards(self):
        return [c for c in self.calls if "_fwd_" in c[0]]

    def level_pointers(self):
        """The forward calls' level_w argument: the output tensor, or None for a NULL pointer."""
        return [None if not isinstance(args[-1], torch.Tensor) and args[-1] == 0 else args[-1]
                for _name, args in self.forwards()]


def module_problem(k, seed=0):
    from boxer_amd import InstanceAttention
    torch.manual_seed(seed)
    shapes = torch.tensor([(20, 16), (10, 8), (5, 4), (3, 2)], device="cuda")
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    S = int(shapes.prod(1).sum())
    B, Lq, d = 2, 19, 256
    m = InstanceAttention(d, 4, 8, k).cuda()
    with torch.no_grad():
        m.linear_box_weight.normal_(0, 0.05)
        m.linear_attn_weight.normal_(0, 0.1)
    query = torch.randn(B, Lq, d, device="cuda")
    value = torch.randn(B, S, d, device="cuda")
    v_mask = torch.rand(B, S, device="cuda") < 0.15
    ref = torch.rand(B, Lq, 4, device="cuda") * 0.5 + 0.2
    return m, (query, value, shapes, v_mask, lsi, None, ref)


def run_module(m, args, autocast):
    query, value = args[0].clone().requires_grad_(), args[1].clone().requires_grad_()
    m.zero_grad()
    with torch.autocast("cuda", dtype=autocast or torch.bfloat16, enabled=autocast is not None):
        out, mask_out, weights = m(query, value, *args[2:])
    loss = out.float().square().sum()
    if mask_out is not None:
        loss = loss + mask_out.float().square().sum()
    loss.backward()
    grads = [p.grad.detach().clone() for p in m.parameters()] + [query.grad, value.grad]
    return out.detach().float(), None if mask_out is None else mask_out.detach().float(), weights, grads


def assert_close(a, b, tol, what):
    assert (a.double() - b.double()).abs().max().item() <= tol * max(1.0, a.abs().max().item()), what


@pytest.mark.parametrize("autocast", [None, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("k", [14, 4])
def test_module_fused_against_unfused(k, autocast, monkeypatch):
    m, args = module_problem(k)
    m.inferencing = False
    m.native_bf16 = autocast == torch.bfloat16           # the 16-bit storage modes, as the trainer runs them
    m.native_f16 = autocast == torch.float16
    spy = Spy(monkeypatch)
    m.fused_pointwise = False
    off = run_module(m, args, autocast)
    assert not spy.calls                                  # flag off: the torch chain
    m.fused_pointwise = True
    on = run_module(m, args, autocast)
    assert len(spy.forwards()) == 1 and len(spy.calls) == 2, [c[0] for c in spy.calls]
    assert isinstance(spy.level_pointers()[0], torch.Tensor)   # training: the level weights are asked for

    tol = 1e-5 if autocast is None else 2e-2
    assert_close(off[0], on[0], tol, "output")
    assert_close(off[1], on[1], tol, "mask output")
    assert len(on[2]) == 2
    for w_off, w_on in zip(off[2], on[2]):
        assert w_on.shape == w_off.shape == (2, 19, 8, 4, k, k) and w_on.dtype == torch.float32
        assert_close(w_off, w_on, tol, "attention weights")
    for i, (ga, gb) in enumerate(zip(off[3], on[3])):
        assert ga.dtype == gb.dtype
        assert_close(ga, gb, tol, "gradient %d" % i)


@pytest.mark.parametrize("k", [14, 4])
def test_module_inference_asks_for_spatial_weights_only(k, monkeypatch):
    m, args = module_problem(k, seed=1)
    m.inferencing = True
    spy = Spy(monkeypatch)
    m.fused_pointwise = False
    off = run_module(m, args, None)
    assert not spy.calls
    m.fused_pointwise = True
    on = run_module(m, args, None)
    assert len(spy.forwards()) == 1
    assert spy.level_pointers() == [None]                 # level_w: a NULL pointer
    assert on[1] is None and len(on[2]) == 1
    assert_close(off[0], on[0], 1e-5, "output")
    assert_close(off[2][0], on[2][0], 1e-5, "spatial weights")
    for i, (ga, gb) in enumerate(zip(off[3], on[3])):
        assert_close(ga, gb, 1e-5, "gradient %d" % i)


def test_fused_path_saves_the_logits_only():
    from boxer_amd import InstanceWeightsFunction
    saved = []
    hooks = torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t)

    z = torch.randn(2, 19, 8, 4, 2, 2, device="cuda", requires_grad=True)
    with hooks:
        InstanceWeightsFunction.apply(z, 14, True)
    assert saved == [(2, 19, 8, 4, 2, 2)]

    # the module: expanded tensors are saved by the operator alone (its own spatial_w and level_w)
    m, args = module_problem(14, seed=2)
    m.inferencing = False
    expanded = 2 * 19 * 8 * 4 * 14 * 14
    assert args[1].numel() != expanded
    counts = {}
    for fused in (False, True):
        m.fused_pointwise = fused
        del saved[:]
        with hooks:
            out, mask_out, _ = m(*args)
        counts[fused] = sum(1 for s in saved if torch.Size(s).numel() == expanded)
    assert counts[True] == 2 and counts[False] > 2, counts
