"""GPU tests (``-m gpu``) of box attention's inference forward from boxes and L*P logits in one launch
(``ops.box_attn_forward_boxes``, include/boxattn.h boxattn_fwd_boxes_*) and of the module flag
``fused_boxes`` that takes it in BoxAttention / Box3dAttention.

Every seeded case holds the one call against two expectations, at the project's own tolerances (DESIGN.md 5:
``|got - want| <= tol * (max(1, rms(want)) + |want|)``, tol 1e-4 for float32 and 1e-2 for 16-bit storage -- the harness
of test_gpu_wide_box_forward.py):
  (a) the three launches of this same build -- ``ops.box_grid_forward`` -> ``ops.softmax_forward`` ->
      ``ops.box_attn_forward``, route asserted;
  (b) the float64 C oracle fed with the locations and weights those two GPU kernels produced and with ``value``
      rounded to the storage type.
How many elements differ BITWISE from (a) is printed per case (the locations come from shared device functions; the
softmax sums in another order, and the window-staged forward in yet another); it is reported, not asserted."""
import functools
import itertools

import numpy as np
import pytest
import torch

import golden_io
from oracle import boxattn_oracle as oc
from test_gpu_wide_box_forward import DTYPES, GATHER, STAGED, check, dev, rounded, tables, tol_of

pytestmark = pytest.mark.gpu

C2_LEVELS = [(100, 100), (50, 50), (25, 25), (13, 13)]
GEOMETRY = {
    # L P = 4 G at C 32 (16-bit storage): the model's shape; head = XCD placement
    "model": dict(levels=[(9, 11), (4, 5), (3, 3), (2, 2)], B=2, Lq=5, H=8, P=4),
    # L P = 12: a ragged last tile at G = 8; 42 pairs: dead waves in the last workgroup; L no power of two
    "ragged": dict(levels=[(5, 7), (3, 4), (1, 3)], B=2, Lq=7, H=3, P=4),
    "one_level": dict(levels=[(6, 5)], B=1, Lq=3, H=2, P=4),
    # an odd kernel size: tiles that straddle levels
    "odd_k": dict(levels=[(6, 5), (3, 2)], B=1, Lq=3, H=2, P=9),
    # L P = 64 both ways
    "sixteen_levels": dict(levels=[(1, 1), (2, 1)] * 8, B=1, Lq=3, H=2, P=4),
    "k4": dict(levels=[(9, 11), (4, 5), (3, 3), (2, 2)], B=1, Lq=3, H=2, P=16),
    # one query a pixel, windows of four pixels of the query's level: the three launches take the window-staged forward
    "encoder": dict(levels=[(8, 8), (4, 4)], B=1, Lq=80, H=2, P=4),
    # more than 8 workgroups: the XCD re-map and the magic divisions
    "mid": dict(levels=C2_LEVELS, B=2, Lq=300, H=8, P=4),
    "mid_h3": dict(levels=C2_LEVELS, B=2, Lq=300, H=3, P=4),
}
# (angle_mode, ref_dim) x per_head x with_vr
FLAVOURS = list(itertools.product(((0, 4), (1, 5), (1, 7), (2, 5)), (False, True), (False, True)))


def kernel_indices(P):
    """The modules' buffer for a k x k kernel (P = k * k), divisor k."""
    from boxer_amd.modules import _kernel_offsets
    k = int(round(P ** 0.5))
    assert k * k == P
    return _kernel_offsets(k, k).float().cuda().contiguous()


@functools.lru_cache(maxsize=None)
def problem(geometry, C, angle_mode, ref_dim, per_head, with_vr):
    """numpy / float32 inputs of one case (the same for every storage type)."""
    geo = GEOMETRY[geometry]
    shapes, lsi, S = tables(geo["levels"])
    B, Lq, H, L, P = geo["B"], geo["Lq"], geo["H"], len(geo["levels"]), geo["P"]
    V = 5 if angle_mode == 1 else 4
    rng = np.random.default_rng(7919 * C + 31 * P + 1000 * sorted(GEOMETRY).index(geometry) + 8 * angle_mode
                                + 2 * ref_dim + per_head)
    rshape = (B, Lq, H) if per_head else (B, Lq)
    ref = np.concatenate([rng.uniform(0.05, 0.95, rshape + (2,)), rng.uniform(0.05, 0.7, rshape + (2,)),
                          rng.uniform(-3.0, 3.0, rshape + (ref_dim - 4,))], -1)
    if geometry == "encoder":                      # query i = pixel i: a window of four pixels of its own level
        rows = []
        for hl, wl in geo["levels"]:
            ys, xs = np.meshgrid(np.arange(hl), np.arange(wl), indexing="ij")
            rows.append(np.stack([(xs.ravel() + 0.5) / wl, (ys.ravel() + 0.5) / hl,
                                  np.full(hl * wl, 4.0 / wl), np.full(hl * wl, 4.0 / hl)], -1))
        win = np.concatenate(rows, 0)[None]        # (1, S, 4)
        ref[..., :4] = win[:, :, None, :] if per_head else win
    flat = ref.reshape(-1, ref_dim)
    flat[0, :4] = (2.6, 2.4, 0.2, 0.3)                       # a window wholly outside the map (valid ratios >= 0.5)
    flat[1, :4] = (0.97, 0.02, 0.5, 0.4)                     # ... and one partly outside
    flat[-1, :4] = (-0.7, 0.5, 0.3, 0.3)                     # wholly outside on the other side
    if ref_dim > 4:
        flat[2 % len(flat), 4] = 23.0                        # angles of several turns (mode 2: radians; 1: turns)
        flat[3 % len(flat), 4] = -7.25
    off = 3.0 * rng.standard_normal((B, Lq, H, L, V))
    if geometry == "encoder":
        off[..., :4] *= 0.5
    rows = off.reshape(-1, V)
    rows[rng.random(len(rows)) < 0.15, 2] = -12.0            # negative predicted sizes: relu puts every point on the
    rows[rng.random(len(rows)) < 0.15, 3] = -9.5             # centre line / centre
    rows[0, 2:4] = -8.0                                      # size exactly zero: w + (-8 / 8) w
    if V == 5:
        rows[1, 4] = 77.0                                    # 4.8 turns
    logits = 3.0 * rng.standard_normal((B, Lq, H, L * P))
    logits += 30.0 * np.where(rng.random((B, Lq, H, 1)) < 0.5, -1.0, 1.0)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(shapes=shapes, lsi=lsi, S=S, dims=(B, S, H, C, L, Lq, P), value=rng.standard_normal((B, S, H, C)),
                ref=f32(ref), off=f32(off), logits=f32(logits), angle_mode=angle_mode,
                vr=f32(rng.uniform(0.5, 1.0, (B, 1, 1, L, 1, 2))) if with_vr else None)


def three_route(geometry, C):
    """The family the three launches' sampling call must take."""
    return STAGED if geometry == "encoder" and C == 32 else GATHER


def run_case(g, dt, route, value=None):
    """-> (got, three_launch, oracle): got and three_launch tensors, oracle numpy."""
    from boxer_amd import ops
    B, S, H, C, L, Lq, P = g["dims"]
    value = dev(g["value"], dt) if value is None else value
    shapes, lsi = dev(g["shapes"]), dev(g["lsi"])
    ref, off, logits, kidx = dev(g["ref"]), dev(g["off"]), dev(g["logits"]), kernel_indices(P)
    vr = None if g["vr"] is None else dev(g["vr"])
    assert ops.box_forward_boxes_ok(value, L, Lq, P), "not eligible: %s %s" % (g["dims"], dt)
    got = ops.box_attn_forward_boxes(value, shapes, lsi, ref, off, kidx, vr, logits, g["angle_mode"])
    # (a) the three launches of this build
    grid = ops.box_grid_forward(ref, off, kidx, vr, g["angle_mode"])
    attn = ops.softmax_forward(logits).view(B, Lq, H, L, P)
    assert (1 + off[..., 2:4] / 8 <= 0).any() and (grid < 0).any() and (grid > 1).any()   # relu hit, outside both ways
    taken = ops.forward_route(value, grid, shapes, lsi)
    assert taken == route, "the three launches take route %d, wanted %d" % (taken, route)
    three = ops.box_attn_forward(value, shapes, lsi, grid, attn, 64)
    torch.cuda.synchronize()
    # (b) the float64 oracle on what the two GPU kernels produced
    want = oc.box_attn_forward(rounded(g["value"], dt), g["shapes"], g["lsi"], grid.double().cpu().numpy(),
                               attn.double().cpu().numpy())
    return got, three, want


def hold(got, three, want, dt, what):
    tol = tol_of(dt)
    assert got.dtype == dt and got.shape == three.shape
    bits = torch.int32 if dt == torch.float32 else torch.int16
    differ = int((got.view(bits) != three.view(bits)).sum().item())
    print("%s: %d of %d elements differ bitwise from the three launches" % (what, differ, got.numel()))
    check(got, three.double().cpu().numpy(), tol, "%s against the three launches" % what)
    check(got, want, tol, "%s against the oracle" % what)


def all_flavours(geometry, C, dtype):
    from boxer_amd import ops
    dt = DTYPES[dtype]
    geo = GEOMETRY[geometry]
    B, L, Lq, H, P = geo["B"], len(geo["levels"]), geo["Lq"], geo["H"], geo["P"]
    S = tables(geo["levels"])[2]
    if geometry == "k4" and not ops.box_forward_boxes_ok(torch.empty(B, S, H, C, dtype=dt, device="cuda"), L, Lq, P):
        pytest.skip("k4: no row gather for %s at C = %d (boxattn_fwd_boxes_ok answers 0)" % (dtype, C))
    for (angle_mode, ref_dim), per_head, with_vr in FLAVOURS:
        g = problem(geometry, C, angle_mode, ref_dim, per_head, with_vr)
        what = "%s C=%d %s angle=%d D=%d per_head=%d vr=%d" % (geometry, C, dtype, angle_mode, ref_dim, per_head,
                                                                 with_vr)
        hold(*run_case(g, dt, three_route(geometry, C)), dt, what)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("C", [16, 32, 64])
@pytest.mark.parametrize("geometry", ["model", "ragged", "one_level", "odd_k", "sixteen_levels", "k4", "encoder"])
def test_seeded_matrix(geometry, C, dtype):
    """Angle modes 0, 1 (reference windows of 5 and 7 values) and 2 x reference windows shared and per head x
    valid_ratios None and given."""
    all_flavours(geometry, C, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("geometry", ["mid", "mid_h3"])
def test_mid_size(geometry, dtype):
    """C2 levels, 300 queries, B 2, C 32, angle mode 0: 75 and more workgroups."""
    dt = DTYPES[dtype]
    g = problem(geometry, 32, 0, 4, False, True)
    hold(*run_case(g, dt, GATHER), dt, "%s %s" % (geometry, dtype))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("geometry", ["model", "ragged"])
def test_value_rows_offset_by_eight_bytes(geometry, dtype):
    """A 16-bit `value` 8 bytes off a 16-byte boundary: 4 channels a lane instead of 8, the same family."""
    from boxer_amd import ops
    dt = DTYPES[dtype]
    g = problem(geometry, 32, 1, 5, True, True)
    flat = torch.zeros(g["value"].size + 4, dtype=dt, device="cuda")
    value = flat[4:].view(g["value"].shape)
    value.copy_(dev(g["value"], dt))
    assert value.data_ptr() % 16 == 8 and value.is_contiguous()
    B, S, H, C, L, Lq, P = g["dims"]
    assert ops.box_forward_boxes_ok(value, L, Lq, P)
    hold(*run_case(g, dt, GATHER, value=value), dt, "offset value %s %s" % (geometry, dtype))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_two_runs_are_equal(dtype):
    from boxer_amd import ops
    dt = DTYPES[dtype]
    g = problem("model", 32, 1, 5, False, True)
    B, S, H, C, L, Lq, P = g["dims"]
    args = (dev(g["value"], dt), dev(g["shapes"]), dev(g["lsi"]), dev(g["ref"]), dev(g["off"]), kernel_indices(P),
            dev(g["vr"]), dev(g["logits"]), 1)
    first = ops.box_attn_forward_boxes(*args)
    again = ops.box_attn_forward_boxes(*args)
    torch.cuda.synchronize()
    assert torch.equal(first, again), "the kernel has no atomics"


def test_ops_refuse_what_has_no_kernel():
    """ValueError before any launch: the launch spy sees nothing."""
    from boxer_amd import ops

    def inputs(levels, B, Lq, H, C, P, V=4, D=4, dt=torch.float32):
        shapes, lsi, S = tables(levels)
        L = len(levels)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
        return [torch.zeros(B, S, H, C, dtype=dt, device="cuda"), dev(shapes), dev(lsi), z(B, Lq, D),
                z(B, Lq, H, L, V), z(P, 2), None, z(B, Lq, H, L * P)]

    launches = []
    orig = ops._grid_call
    ops._grid_call = lambda *a, **k: launches.append(a[0]) or orig(*a, **k)
    try:
        cases = {"L P = 65": (inputs([(6, 5)], 1, 3, 2, 32, 65), 0),
                 "L = 17": (inputs([(1, 1)] * 17, 1, 3, 2, 32, 1), 0),
                 "float64": (inputs([(6, 5)], 1, 3, 2, 32, 4, dt=torch.float64), 0),
                 "C = 8": (inputs([(6, 5)], 1, 3, 2, 8, 4), 0),
                 "V = 4 with angle_mode 1": (inputs([(6, 5)], 1, 3, 2, 32, 4, V=4, D=5), 1),
                 "V = 5 with angle_mode 0": (inputs([(6, 5)], 1, 3, 2, 32, 4, V=5, D=5), 0),
                 "ref_dim 4 with angle_mode 2": (inputs([(6, 5)], 1, 3, 2, 32, 4), 2)}
        strided = inputs([(6, 5)], 1, 3, 2, 32, 4)
        strided[0] = torch.zeros(1, 30, 2, 64, device="cuda")[..., ::2]
        assert not strided[0].is_contiguous()
        cases["value not contiguous"] = (strided, 0)
        for what, (args, mode) in cases.items():
            with pytest.raises(ValueError):
                ops.box_attn_forward_boxes(*args, mode)
            assert not launches, what
        ok = inputs([(6, 5)], 1, 3, 2, 32, 4)                   # (the control: the same arguments, accepted)
        out = ops.box_attn_forward_boxes(*ok, 0)
        torch.cuda.synchronize()
        assert launches == ["boxattn_fwd_boxes_f32"] and out.shape == (1, 3, 64) and not out.any()
    finally:
        ops._grid_call = orig


# ------------------------------------------------------------------ the modules
# name -> (class, constructor arguments, v_mask given, valid ratios given, (float32, bf16) tolerance on the output as
# test_gpu_parity.py holds the golden to: max |got - want| / max(1, max |want|))
G7 = dict(d_model=32, num_level=2, num_head=4)
G9 = dict(d_model=256, num_level=4, num_head=8)
GOLDENS = {
    "G7_module_box": ("BoxAttention", dict(G7, kernel_size=2), True, True, (1e-4, 2e-2)),
    "G7_module_box_perhead": ("BoxAttention", dict(G7, kernel_size=2), False, False, (1e-4, 2e-2)),
    "G7_module_box3d_rot": ("Box3dAttention", dict(G7, with_rotation=True, kernel_size=2), True, True, (1e-4, 2e-2)),
    "G7_module_box3d_fixed": ("Box3dAttention", dict(G7, with_rotation=False, kernel_size=3), False, False,
                              (1e-4, 2e-2)),
    "G9_module_box_dec": ("BoxAttention", dict(G9, kernel_size=2), True, True, (2e-4, 4e-2)),
    "G9_module_box_enc": ("BoxAttention", dict(G9, kernel_size=2), True, True, (2e-4, 4e-2)),
    "G9_module_box_enc_masked": ("BoxAttention", dict(G9, kernel_size=2), True, True, (2e-4, 4e-2)),
    "G9_module_box3d_rot_dec": ("Box3dAttention", dict(G9, with_rotation=True, kernel_size=2), True, True,
                                (2e-4, 4e-2)),
    "G9_module_box3d_fixed_enc": ("Box3dAttention", dict(G9, with_rotation=False, kernel_size=2), True, True,
                                  (2e-4, 4e-2)),
}


def golden_module(name, native_bf16=False):
    import boxer_amd
    cls, kw, with_mask, with_ratio, _ = GOLDENS[name]
    g = golden_io.load(name)
    m = getattr(boxer_amd, cls)(**kw).double()
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    m = m.float().cuda()
    assert m.fused_boxes is False                    # the default: nothing changes unless it is set
    m.native_bf16 = native_bf16

    def t(key, given=True):
        if not given or key not in g:
            return None
        x = dev(g[key])
        return x.float() if x.is_floating_point() else x
    args = (t("query"), t("value"), dev(g["shapes"]), t("v_mask", with_mask), dev(g["lsi"]), t("ratios", with_ratio),
            t("ref_windows"))
    return m, g, args


def golden_out(g):
    return g["out0"] if "out0" in g else g["out"]


def golden_err(got, want):
    got = got.detach().double().cpu().numpy()
    want = np.asarray(want, dtype=np.float64).reshape(got.shape)
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


class CallCounter:
    """Counts the calls of ops.box_attn_forward_boxes while it is active."""
    def __enter__(self):
        from boxer_amd import ops
        self.calls, self.orig = [], ops.box_attn_forward_boxes
        ops.box_attn_forward_boxes = lambda *a, **k: self.calls.append(1) or self.orig(*a, **k)
        return self

    def __exit__(self, *exc):
        from boxer_amd import ops
        ops.box_attn_forward_boxes = self.orig


@pytest.mark.parametrize("native_bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_module_reference_golden(name, native_bf16):
    """Under no_grad with the flag: the output agrees with the reference's at the golden's tolerance and with the
    flag-off module, through ONE call of ops.box_attn_forward_boxes -- where that has its kernel: the G9 goldens (32
    channels a head; asserted eligible).  The G7 goldens have 8 channels a head, for which the library has generic
    kernels only: there the flag must fall through to today's code without a call.  The flag-off module never calls."""
    from boxer_amd import ops
    m, g, args = golden_module(name, native_bf16)
    dt = torch.bfloat16 if native_bf16 else torch.float32
    B, S = args[1].shape[:2]
    eligible = ops.box_forward_boxes_ok(torch.empty(B, S, m.num_head, m.head_dim, dtype=dt, device="cuda"),
                                        m.num_level, args[0].shape[1], m.num_point)
    assert eligible == name.startswith("G9"), "%s: eligible = %s" % (name, eligible)
    outs, counts = {}, {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=native_bf16):
        for flag in (True, False):
            m.fused_boxes = flag
            with CallCounter() as counter:
                outs[flag] = m(*args)
            counts[flag] = len(counter.calls)
    torch.cuda.synchronize()
    assert counts[False] == 0, "the flag-off module called ops.box_attn_forward_boxes"
    assert counts[True] == (1 if eligible else 0), "the flag took %d calls of the one-launch path" % counts[True]
    if eligible:
        assert outs[True][1] == ()
    assert outs[True][0].shape == outs[False][0].shape and outs[True][0].dtype == outs[False][0].dtype
    tol_g = GOLDENS[name][4][1 if native_bf16 else 0]
    e = golden_err(outs[True][0], golden_out(g))
    print("%s bf16=%d: %.3e against the golden (tol %.0e)" % (name, native_bf16, e, tol_g))
    assert e <= tol_g
    check(outs[True][0], outs[False][0].double().cpu().numpy(), 1e-2 if native_bf16 else 1e-4,
          "%s bf16=%d flag on against flag off" % (name, native_bf16))


def test_module_with_grad_runs_todays_code():
    """Flag on, grad enabled: no call of the one-launch path, the usual weights as second element, and the output and
    every parameter gradient bitwise those of the flag-off module."""
    m, g, args = golden_module("G9_module_box_dec")
    results = {}
    for flag in (True, False):
        m.fused_boxes = flag
        m.zero_grad()
        with CallCounter() as counter:
            out, weights = m(*args)
            out.square().sum().backward()
        assert not counter.calls, "grad mode took the one-launch path"
        assert isinstance(weights, torch.Tensor) and weights.shape[-2:] == (2, 2)
        results[flag] = [out.detach().clone()] + [p.grad.clone() for p in m.parameters()]
    torch.cuda.synchronize()
    names = ["out"] + [k for k, _ in m.named_parameters()]
    for what, a, b in zip(names, results[True], results[False]):
        assert torch.equal(a, b), "%s differs between flag on and flag off" % what
