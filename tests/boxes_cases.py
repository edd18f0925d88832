"""From-boxes problems, for the kernels that take reference boxes, offsets and logits: geometries, kernel
index tables, the problem, reference and upstream builders of each route (box and instance, forward, backward, value,
window-staged), the goldens read as modules, and the runners that call the library's functions on them."""
import functools
import itertools
import math

import numpy as np
import torch

import error_bounds as eb
import golden_io
from compare_rules import check_scaled, rounded, tol_of
from point_cases import on_cell_edge
from route_vocab import dev


def tables(levels):
    shapes = np.asarray(levels, dtype=np.int64)
    sizes = shapes.prod(1)
    return shapes, np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64), int(sizes.sum())


def module_problem():
    from boxer_amd import InstanceAttention
    torch.manual_seed(3)
    g6 = golden_io.load("G6_inst_ms14")
    shapes = dev(g6["shapes"])
    lsi = dev(g6["lsi"])
    S = int(g6["shapes"].prod(1).sum())
    B, Lq, d = 2, 6, 256
    m = InstanceAttention(d, 4, 8, 14).cuda()
    with torch.no_grad():
        m.linear_box_weight.normal_(0, 0.05)
        m.linear_attn_weight.normal_(0, 0.1)
    query = torch.randn(B, Lq, d, device="cuda")
    value = torch.randn(B, S, d, device="cuda")
    ref = torch.rand(B, Lq, 4, device="cuda") * 0.5 + 0.2
    return m, (query, value, shapes, None, lsi, None, ref), (B, S, 8, 32, 4, Lq, 196), g6


# five_levels: more levels than a 4-lane group (the box is decoded again for l0 > 0), 30 pairs with a last workgroup of
# dead waves, L no power of two; head_xcd: head = XCD placement; one_level; sixteen_levels: the widest cell group
INST_GEOMETRY = {"five_levels": dict(levels=[(5, 7), (3, 4), (2, 2), (1, 3), (1, 1)], B=2, Lq=5, H=3),
                 "head_xcd": dict(levels=[(9, 11), (4, 5)], B=2, Lq=4, H=8),
                 "one_level": dict(levels=[(6, 5)], B=1, Lq=3, H=2),
                 "sixteen_levels": dict(levels=[(1, 1), (2, 1)] * 8, B=1, Lq=3, H=2)}
KERNEL_SIZES = [4, 6, 14]           # one, two and four waves a pair; m odd at k = 6; a ragged last step
INST_BOXES_FLAVOURS = list(itertools.product((False, True), (False, True), (True, False)))     # per_head, with_vr, need_mask


def inst_kernel_indices(k):
    from boxer_amd.modules import _kernel_offsets
    return _kernel_offsets(k, k).float().cuda().contiguous()


@functools.lru_cache(maxsize=None)
def inst_boxes_problem(geometry, C, k, per_head, with_vr):
    """numpy / float32 inputs of one case (the same for every storage type and both mask flavours)."""
    geo = INST_GEOMETRY[geometry]
    shapes, lsi, S = tables(geo["levels"])
    B, Lq, H, L = geo["B"], geo["Lq"], geo["H"], len(geo["levels"])
    rng = np.random.default_rng(7919 * C + 31 * k + 2 * sorted(INST_GEOMETRY).index(geometry) + per_head)
    rshape = (B, Lq, H) if per_head else (B, Lq)
    ref = np.concatenate([rng.uniform(0.05, 0.95, rshape + (2,)), rng.uniform(0.05, 0.7, rshape + (2,))], -1)
    ref.reshape(-1, 4)[0] = (2.6, 2.4, 0.2, 0.3)             # a window wholly outside the map (valid ratios >= 0.5)
    ref.reshape(-1, 4)[1] = (0.97, 0.02, 0.5, 0.4)           # ... and one partly outside
    ref.reshape(-1, 4)[-1] = (-0.7, 0.5, 0.3, 0.3)           # wholly outside on the other side
    off = 3.0 * rng.standard_normal((B, Lq, H, L, 4))
    flat = off.reshape(-1, 4)
    flat[rng.random(len(flat)) < 0.15, 2] = -12.0            # negative predicted sizes: relu puts every point on the
    flat[rng.random(len(flat)) < 0.15, 3] = -9.5             # centre line / centre
    flat[0, 2:] = -8.0                                       # size exactly zero: w + (-8 / 8) w
    logits = 3.0 * rng.standard_normal((B, Lq, H, L, 2, 2))
    logits += 30.0 * np.where(rng.random((B, Lq, H, 1, 1, 1)) < 0.5, -1.0, 1.0)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(shapes=shapes, lsi=lsi, S=S, dims=(B, S, H, C, L, Lq), value=rng.standard_normal((B, S, H, C)),
                ref=f32(ref), off=f32(off), logits=f32(logits),
                vr=f32(rng.uniform(0.5, 1.0, (B, 1, 1, L, 1, 2))) if with_vr else None)


def inst_golden_module(native_bf16):
    from boxer_amd import InstanceAttention
    g = golden_io.load("G9_module_inst_k4")
    m = InstanceAttention(256, 4, 8, 4).double()
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    m = m.float().cuda()
    assert m.fused_boxes is False, m.fused_boxes
    m.native_bf16 = native_bf16
    f = lambda key: dev(g[key]).float()
    return m, g, (f("query"), f("value"), dev(g["shapes"]), dev(g["v_mask"]), dev(g["lsi"]), f("ratios"),
                  f("ref_windows"))


def golden_err(got, want):
    got = got.detach().double().cpu().numpy()
    want = np.asarray(want, dtype=np.float64).reshape(got.shape)
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def _g9_check(name, outs, grads, g, tol, what, rms_only=()):
    """Every output and gradient: max |got - want| / max(1, max |want|) <= tol; for the tensors named in `rms_only`
    the relative root-mean-square error instead (bf16 autocast: the box offsets are bf16 numbers, a few sample
    points per image land on the other side of a bilinear cell edge than in the float64 run, and the gradients
    that flow through the LOCATIONS -- reference windows, box projection, query -- jump there; the reference under
    autocast has the same sensitivity)."""
    def errs(got, want):
        got = got.detach().double().cpu().numpy()
        want = np.asarray(want, dtype=np.float64).reshape(got.shape)
        return (float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max())),
                float(np.sqrt(((got - want) ** 2).mean()) / max(1e-30, np.sqrt((want ** 2).mean()))))
    worst = {}
    for i, o in enumerate(outs):
        worst["out%d" % i] = errs(o, g["out%d" % i])[0]
    for k, v in grads.items():
        key = "grad_" + k if not k.startswith("param.") else "grad." + k[6:]
        assert v is not None, "%s: no gradient reached %s" % (name, k)
        e_max, e_rms = errs(v, g[key])
        worst[k] = e_rms / 2 if any(r in k for r in rms_only) else e_max       # (rms criterion: 2 tol)
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, "%s %s: errors above %.0e: %s" % (name, what, tol, bad)


EDGE_CAP = 2e-3


def inst_grid_f32(ref, off, kidx, vr):
    """The sampling grid (B,Lq,H,L,P,2) in float32 numpy: grid_box / grid_point of boxattn_grid.h, operation by
    operation (angle_mode 0)."""
    f = np.float32
    r = ref[:, :, None, None] if ref.ndim == 3 else ref[:, :, :, None]             # (B,Lq,1|H,1,4)
    rw, rh = r[..., 2], r[..., 3]
    cx = r[..., 0] + off[..., 0] / f(8) * rw
    cy = r[..., 1] + off[..., 1] / f(8) * rh
    w = rw + off[..., 2] / f(8) * rw
    h = rh + off[..., 3] / f(8) * rh
    gx = cx[..., None] + kidx[:, 0] * np.maximum(w, f(0))[..., None]
    gy = cy[..., None] + kidx[:, 1] * np.maximum(h, f(0))[..., None]
    grid = np.stack([gx, gy], -1).astype(f)
    return grid * vr if vr is not None else grid                                    # vr: (B,1,1,L,1,2)


def inst_edge_share(g, k):
    """Share of the sample points of the problem ``g`` within 1e-4 px of a bilinear cell edge (float32 grid on the CPU)."""
    from boxer_amd.modules import _kernel_offsets
    kidx = _kernel_offsets(k, k).float().numpy()
    return float(on_cell_edge(inst_grid_f32(g["ref"], g["off"], kidx, g["vr"]).astype(np.float64), g["shapes"]).mean())


def inst_reduce_grid(ref, off, kidx, vr, gloc):
    """Per-point grad_loc (B,Lq,H,L,P,2) -> grad_offsets (B,Lq,H,L,4), grad_ref_rows (B,Lq,H,L,5), float64."""
    ref, off, kidx, gloc = (np.asarray(a, dtype=np.float64) for a in (ref, off, kidx, gloc))
    r = ref[:, :, None, None] if ref.ndim == 3 else ref[:, :, :, None]
    rw, rh = np.broadcast_to(r[..., 2], off.shape[:4]), np.broadcast_to(r[..., 3], off.shape[:4])
    w = rw + off[..., 2] / 8 * rw
    h = rh + off[..., 3] / 8 * rh
    if vr is not None:
        gloc = gloc * np.asarray(vr, dtype=np.float64)                  # d / d (unscaled grid)
    gx, gy = gloc[..., 0], gloc[..., 1]
    a_cx, a_cy = gx.sum(-1), gy.sum(-1)
    a_w = np.where(w > 0, (kidx[:, 0] * gx).sum(-1), 0.0)               # d / d relu(w), relu'
    a_h = np.where(h > 0, (kidx[:, 1] * gy).sum(-1), 0.0)
    go = np.stack([a_cx * rw / 8, a_cy * rh / 8, a_w * rw / 8, a_h * rh / 8], -1)
    rows = np.stack([a_cx, a_cy, a_cx * off[..., 0] / 8 + a_w * (1 + off[..., 2] / 8),
                     a_cy * off[..., 1] / 8 + a_h * (1 + off[..., 3] / 8), np.zeros_like(a_cx)], -1)
    return go, rows


def inst_reduce_logits(logits, k, gsw, glw):
    """Per-point weight gradients (B,Lq,H,L,k*k) -> grad_logits (B,Lq,H,L,2,2), float64:
    grad_z[c] = a[c] / m^2 (Gs[c] - sum_c' a[c'] Gs[c']) + t[c] (Gt[c] - sum_l' t[l'] Gt[l'])."""
    z = np.asarray(logits, dtype=np.float64)
    m = k // 2
    lead = z.shape[:4]
    cells = lambda g: np.asarray(g, dtype=np.float64).reshape(lead + (2, m, 2, m)).sum((-1, -3))
    e = np.exp(z - z.max((-1, -2, -3), keepdims=True))
    a = e / e.sum((-1, -2, -3), keepdims=True)
    Gs = cells(gsw)
    gz = a / (m * m) * (Gs - (a * Gs).sum((-1, -2, -3), keepdims=True))
    if glw is not None:
        e = np.exp(z - z.max(-3, keepdims=True))
        t = e / e.sum(-3, keepdims=True)
        Gt = cells(glw)
        gz = gz + t * (Gt - (t * Gt).sum(-3, keepdims=True))
    return gz


# The cases of the matrix whose inputs from ``problem`` break the cell-edge condition (a box of size <= 0 puts a whole
# row of points on one line, and that line fell on an edge): the same construction from another seed.
INST_BWD_RESEED = {("five_levels", 16, 6, False, False): 1000003, ("five_levels", 64, 14, True, True): 1000003,
                   ("head_xcd", 16, 14, False, True): 2000006, ("head_xcd", 32, 4, True, True): 2000006,
                   ("sixteen_levels", 16, 4, False, True): 1000003, ("sixteen_levels", 32, 4, False, False): 1000003,
                   ("sixteen_levels", 64, 4, True, True): 1000003}


@functools.lru_cache(maxsize=None)
def inst_bwd_case(geometry, C, k, per_head, with_vr):
    bump = INST_BWD_RESEED.get((geometry, C, k, per_head, with_vr))
    if bump is None:
        return inst_boxes_problem(geometry, C, k, per_head, with_vr)
    make = np.random.default_rng
    np.random.default_rng = lambda seed: make(seed + bump)           # (problem() seeds its generator from its arguments)
    try:
        return inst_boxes_problem.__wrapped__(geometry, C, k, per_head, with_vr)
    finally:
        np.random.default_rng = make


def offset_by_eight(t):
    flat = torch.zeros(t.numel() + 4, dtype=t.dtype, device="cuda")
    out = flat[4:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 8 and out.is_contiguous(), (out.data_ptr() % 16, out.is_contiguous())
    return out


LEAVES = ("value", "ref", "off", "logits")


def module_grads(m, args, loss_fn, autocast=None):
    m.zero_grad()
    query, value, ref = (args[0].clone().requires_grad_(), args[1].clone().requires_grad_(),
                         args[6].clone().requires_grad_())
    with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        outs = m(query, value, args[2], args[3], args[4], args[5], ref)
    loss_fn(outs).backward()
    grads = {"query": query.grad, "value": value.grad, "ref_windows": ref.grad}
    grads.update({"param." + n: p.grad.clone() for n, p in m.named_parameters()})
    return outs, grads


C2_LEVELS = [(100, 100), (50, 50), (25, 25), (13, 13)]
BOX_GEOMETRY = {
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


def box_kernel_indices(P):
    """The modules' buffer for a k x k kernel (P = k * k), divisor k."""
    from boxer_amd.modules import _kernel_offsets
    k = int(round(P ** 0.5))
    assert k * k == P, (k, P)
    return _kernel_offsets(k, k).float().cuda().contiguous()


@functools.lru_cache(maxsize=None)
def box_boxes_problem(geometry, C, angle_mode, ref_dim, per_head, with_vr):
    """numpy / float32 inputs of one case (the same for every storage type)."""
    geo = BOX_GEOMETRY[geometry]
    shapes, lsi, S = tables(geo["levels"])
    B, Lq, H, L, P = geo["B"], geo["Lq"], geo["H"], len(geo["levels"]), geo["P"]
    V = 5 if angle_mode == 1 else 4
    rng = np.random.default_rng(7919 * C + 31 * P + 1000 * sorted(BOX_GEOMETRY).index(geometry) + 8 * angle_mode
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


def hold(got, three, want, dt, what):
    tol = tol_of(dt)
    assert got.dtype == dt and got.shape == three.shape, (got.dtype, dt, got.shape, three.shape)
    bits = torch.int32 if dt == torch.float32 else torch.int16
    differ = int((got.view(bits) != three.view(bits)).sum().item())
    print("%s: %d of %d elements differ bitwise from the three launches" % (what, differ, got.numel()))
    check_scaled(got, three.double().cpu().numpy(), tol, "%s against the three launches" % what)
    check_scaled(got, want, tol, "%s against the oracle" % what)


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


def box_golden_module(name, native_bf16=False):
    import boxer_amd
    cls, kw, with_mask, with_ratio, _ = GOLDENS[name]
    g = golden_io.load(name)
    m = getattr(boxer_amd, cls)(**kw).double()
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    m = m.float().cuda()
    assert m.fused_boxes is False, m.fused_boxes     # the default: nothing changes unless it is set
    m.native_bf16 = native_bf16

    def t(key, given=True):
        if not given or key not in g:
            return None
        x = dev(g[key])
        return x.float() if x.is_floating_point() else x
    args = (t("query"), t("value"), dev(g["shapes"]), t("v_mask", with_mask), dev(g["lsi"]), t("ratios", with_ratio),
            t("ref_windows"))
    return m, g, args


BOX_GEOMETRIES = ["model", "ragged", "one_level", "odd_k", "sixteen_levels", "k4", "encoder"]
CHANNELS = [16, 32, 64]
INST_FLAVOURS = list(itertools.product((False, True), (False, True)))          # per_head, with_vr
# (geometry, C, k, per_head, with_vr) -> what is added to the seed of inst_boxes_problem
RESEED = {}


def kernel_offsets(k):
    """The modules' kernel_indices buffer of a k x k kernel, float32 numpy."""
    from boxer_amd.modules import _kernel_offsets
    return _kernel_offsets(k, k).float().numpy()


def every_type(a):
    """float64 numbers that float32, bf16 and f16 all hold exactly: rounded to bf16, then to f16 (which changes a bf16
    number only below 2^-17, to a multiple of 2^-24 of at most 7 bits)."""
    return eb.round_to(eb.round_to(a, "bf16"), "f16")


def box_problem(geometry, C, flavour):
    (angle_mode, ref_dim), per_head, with_vr = flavour
    return box_boxes_problem(geometry, C, angle_mode, ref_dim, per_head, with_vr)


@functools.lru_cache(maxsize=16)
def box_reference(geometry, C, flavour):
    g = box_problem(geometry, C, flavour)
    P = g["dims"][6]
    return eb.boxes_reference("box", every_type(g["value"]), g["shapes"], g["lsi"], g["ref"], g["off"],
                              kernel_offsets(int(round(P ** 0.5))), g["vr"], g["logits"], g["angle_mode"])


@functools.lru_cache(maxsize=None)
def inst_problem(geometry, C, k, per_head, with_vr):
    """inst_bwd_case (inst_boxes_problem, re-seeded where that file had to), re-seeded again
    where the condition with the locations' own slack asks for it."""
    bump = RESEED.get((geometry, C, k, per_head, with_vr))
    if bump is None:
        return inst_bwd_case(geometry, C, k, per_head, with_vr)
    make = np.random.default_rng
    np.random.default_rng = lambda seed: make(seed + bump)
    try:
        return inst_boxes_problem.__wrapped__(geometry, C, k, per_head, with_vr)
    finally:
        np.random.default_rng = make


def inst_upstream(g, k):
    B, S, H, C, L, Lq = g["dims"]
    rng = np.random.default_rng(100)
    return every_type(rng.standard_normal((B, Lq, H * C))), every_type(rng.standard_normal((B, Lq, k * k, H * C)))


@functools.lru_cache(maxsize=8)
def inst_reference(geometry, C, k, per_head, with_vr, with_mask):
    """with_mask: {out, mask_out, the three gradients with grad_mask}; without: {out, the gradients without}."""
    g = inst_problem(geometry, C, k, per_head, with_vr)
    gout, gmask = inst_upstream(g, k)
    return eb.boxes_reference("instance", every_type(g["value"]), g["shapes"], g["lsi"], g["ref"], g["off"],
                              kernel_offsets(k), g["vr"], g["logits"], 0, k, gout, gmask if with_mask else None)


GRAD_NAMES = ("grad_offsets", "grad_ref_rows", "grad_logits")
# (geometry, C, angle_mode, ref_dim, per_head, with_vr) -> what is added to the seed box_bwd_case
# uses, where the condition with the locations' own slack asks for it
BWD_RESEED = {("k4", 32, 2, 5, False, True): 1000003}           # 2 points of 768 (0.26 %) with the slack, 1 without


@functools.lru_cache(maxsize=None)
def bwd_problem(geometry, C, flavour):
    """box_bwd_case (the forward's problem, re-seeded where that file had to), re-seeded again
    where the share of points within EDGE_PX + slack of a cell edge is above EDGE_CAP."""
    (angle_mode, ref_dim), per_head, with_vr = flavour
    key = (geometry, C, angle_mode, ref_dim, per_head, with_vr)
    bump = BWD_RESEED.get(key)
    if bump is None:
        return box_bwd_case(*key)
    make = np.random.default_rng
    np.random.default_rng = lambda seed: make(seed + BOX_BWD_RESEED.get(key, 0) + bump)
    try:
        return box_boxes_problem.__wrapped__(*key)
    finally:
        np.random.default_rng = make


def bwd_upstream(g):
    B, S, H, C, L, Lq, P = g["dims"]
    return every_type(np.random.default_rng(100).standard_normal((B, Lq, H * C)))


def bwd_model_args(g):
    P = g["dims"][6]
    return ("box", every_type(g["value"]), g["shapes"], g["lsi"], g["ref"], g["off"],
            kernel_offsets(int(round(P ** 0.5))), g["vr"], g["logits"], g["angle_mode"])


@functools.lru_cache(maxsize=16)
def bwd_reference(geometry, C, flavour):
    """{out, grad_offsets, grad_ref_rows, grad_logits, edge_share, points} of the training step from boxes."""
    g = bwd_problem(geometry, C, flavour)
    return eb.boxes_reference(*bwd_model_args(g), grad_out=bwd_upstream(g))


@functools.lru_cache(maxsize=None)
def grid_upstream(P, angle_mode, per_head, with_vr):
    """float32 grad_grid (B, Lq, H, L, P, 2) for ops.box_grid_backward on its own: randn, a few rows of zeros."""
    g = grid_problem(P, angle_mode, per_head, with_vr)
    rng = np.random.default_rng(900 + P)
    gg = rng.standard_normal(g["off"].shape[:4] + (P, 2))
    gg[0, 1] = 0.0
    return np.ascontiguousarray(gg, dtype=np.float32)


SOFTMAX_BWD_LENGTHS = [1, 3, 4, 8, 12, 18, 32, 63, 64]
SOFTMAX_BWD_ROWS = [1, 257]


@functools.lru_cache(maxsize=None)
def softmax_bwd_problem(rows, n):
    """-> (attn: the float64 softmax of softmax_rows(n)'s kinds rounded to float32, grad_attn float32), (rows, n)."""
    z = np.resize(softmax_rows(n), (rows, n)).astype(np.float64)
    rng = np.random.default_rng(1000 * rows + n)
    z = z + 0.5 * (np.arange(rows) >= 8)[:, None] * rng.standard_normal((rows, n))      # (the first 8 rows: as they are)
    a, _ = eb.softmax_reference(z)
    g = rng.standard_normal((rows, n)) * np.exp2(rng.integers(-6, 7, (rows, 1)))
    return np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(g, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def cell_upstream(L, k):
    """float32 grad_spatial, grad_level (1, 8, 1, L, k, k) for ops.instance_weights_backward on its own."""
    rng = np.random.default_rng(70 * L + k)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f32(rng.standard_normal((1, 8, 1, L, k, k))), f32(rng.standard_normal((1, 8, 1, L, k, k)))


GRID_POINTS = [1, 4, 9, 196]
GRID_FLAVOURS = list(itertools.product((0, 1, 2), (False, True), (False, True)))   # angle_mode, per_head, with_vr


@functools.lru_cache(maxsize=None)
def grid_problem(P, angle_mode, per_head, with_vr):
    """A few boxes for ops.box_grid_forward on its own: windows inside, partly and wholly outside the map, sizes below
    and exactly zero, angles of 23 and -7.25 (turns in mode 1, radians in mode 2) and an offset angle of 77 / 16 turns."""
    B, Lq, H, L = 2, 5, 3, 2
    D, V = (7 if angle_mode else 4), (5 if angle_mode == 1 else 4)
    rng = np.random.default_rng(500 + 10 * P + 3 * angle_mode + per_head)
    rshape = (B, Lq, H) if per_head else (B, Lq)
    ref = np.concatenate([rng.uniform(0.05, 0.95, rshape + (2,)), rng.uniform(0.05, 0.7, rshape + (2,)),
                          rng.uniform(-3.0, 3.0, rshape + (D - 4,))], -1)
    flat = ref.reshape(-1, D)
    flat[0, :4] = (2.6, 2.4, 0.2, 0.3)
    flat[1, :4] = (0.97, 0.02, 0.5, 0.4)
    flat[-1, :4] = (-0.7, 0.5, 0.3, 0.3)
    if D > 4:
        flat[2, 4], flat[3, 4] = 23.0, -7.25
    off = 3.0 * rng.standard_normal((B, Lq, H, L, V))
    rows = off.reshape(-1, V)
    rows[rng.random(len(rows)) < 0.15, 2] = -12.0
    rows[0, 2:4] = -8.0
    if V == 5:
        rows[1, 4] = 77.0
    k = int(round(P ** 0.5))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(ref=f32(ref), off=f32(off), kidx=kernel_offsets(k), angle_mode=angle_mode,
                vr=f32(rng.uniform(0.5, 1.0, (B, 1, 1, L, 1, 2))) if with_vr else None)


@functools.lru_cache(maxsize=None)
def softmax_rows(n):
    """Rows of n logits: 3 randn; the same with a shared shift of +- 30; a spread of 60 (one logit on top, the others
    60 and 30 below); all equal; float32."""
    rng = np.random.default_rng(n)
    z = 3.0 * rng.standard_normal((8, n))
    z[2:4] += np.asarray([[30.0], [-30.0]])
    z[4] = np.where(np.arange(n) % 2 == 0, -60.0, -30.0)
    z[4, n // 2] = 0.0
    z[5] = 1.25
    z[6] = np.linspace(-60.0, 0.0, n)
    return np.ascontiguousarray(z, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def cell_rows(L):
    """(1, 8, 1, L, 2, 2) logits of the same kinds for ops.instance_weights_forward."""
    return softmax_rows(4 * L).reshape(1, 8, 1, L, 2, 2)


def box_args(g, dt, value=None):
    B, S, H, C, L, Lq, P = g["dims"]
    value = dev(every_type(g["value"]), dt) if value is None else value
    return (value, dev(g["shapes"]), dev(g["lsi"]), dev(g["ref"]), dev(g["off"]),
            dev(kernel_offsets(int(round(P ** 0.5)))), None if g["vr"] is None else dev(g["vr"]), dev(g["logits"]),
            g["angle_mode"])


F = np.float32


def grid_f32(ref, off, kidx, vr, angle_mode):
    """_where_to_attend in float32 numpy in the documented order: every operation rounds once, no
    fused multiply-add."""
    r = ref[:, :, None, None] if ref.ndim == 3 else ref[:, :, :, None]
    lead = off.shape[:4]
    col = lambda j: np.broadcast_to(r[..., j], lead)
    cx = col(0) + off[..., 0] / F(8) * col(2)
    cy = col(1) + off[..., 1] / F(8) * col(3)
    w = col(2) + off[..., 2] / F(8) * col(2)
    h = col(3) + off[..., 3] / F(8) * col(3)
    lx = kidx[:, 0] * np.maximum(w, F(0))[..., None]
    ly = kidx[:, 1] * np.maximum(h, F(0))[..., None]
    if angle_mode:
        theta = (col(4) + off[..., 4] / F(16)) * F(2) * F(math.pi) if angle_mode == 1 else col(4)
        sn, cs = np.sin(theta.astype(F))[..., None], np.cos(theta.astype(F))[..., None]
        gx = cx[..., None] + (lx * cs - ly * sn)
        gy = cy[..., None] + (lx * sn + ly * cs)
    else:
        gx, gy = cx[..., None] + lx, cy[..., None] + ly
    grid = np.stack([gx, gy], -1)
    assert grid.dtype == F, grid.dtype
    return grid * vr if vr is not None else grid


c32 = lambda a: np.ascontiguousarray(a, dtype=F)

SMALL = ["model", "ragged", "one_level", "odd_k", "sixteen_levels", "k4", "encoder"]
BOX_BWD_CHANNELS = (16, 32, 64)


def box_reduce_grid(ref, off, kidx, vr, angle_mode, gloc):
    """Per-point grad_loc (B,Lq,H,L,P,2) -> grad_offsets (B,Lq,H,L,V), grad_ref_rows (B,Lq,H,L,5), float64:
    grid_grad_add summed over the points of a row, then grid_grad_store."""
    ref, off, kidx, gloc = (np.asarray(a, dtype=np.float64) for a in (ref, off, kidx, gloc))
    lead = off.shape[:4]
    r = ref[:, :, None, None] if ref.ndim == 3 else ref[:, :, :, None]
    col = lambda j: np.broadcast_to(r[..., j], lead)
    rw, rh = col(2), col(3)
    w = rw + off[..., 2] / 8 * rw
    h = rh + off[..., 3] / 8 * rh
    sn, cs = np.zeros(lead), np.ones(lead)
    if angle_mode:
        theta = (col(4) + off[..., 4] / 16) * 2 * math.pi if angle_mode == 1 else col(4)
        sn, cs = np.sin(theta), np.cos(theta)
    sn, cs = sn[..., None], cs[..., None]
    if vr is not None:
        gloc = gloc * np.asarray(vr, dtype=np.float64)                  # d / d (unscaled grid)
    gx, gy = gloc[..., 0], gloc[..., 1]
    kx, ky = kidx[:, 0], kidx[:, 1]
    lx, ly = kx * np.maximum(w, 0.0)[..., None], ky * np.maximum(h, 0.0)[..., None]
    a_cx, a_cy = gx.sum(-1), gy.sum(-1)
    a_w = np.where(w > 0, (kx * (gx * cs + gy * sn)).sum(-1), 0.0)      # d / d relu(w), relu'
    a_h = np.where(h > 0, (ky * (gy * cs - gx * sn)).sum(-1), 0.0)
    a_t = (gx * (-lx * sn - ly * cs) + gy * (lx * cs - ly * sn)).sum(-1)
    go = [a_cx * rw / 8, a_cy * rh / 8, a_w * rw / 8, a_h * rh / 8]
    if off.shape[-1] == 5:
        go.append(a_t * 2 * math.pi / 16 if angle_mode == 1 else np.zeros(lead))
    row_t = a_t * 2 * math.pi if angle_mode == 1 else a_t if angle_mode == 2 else np.zeros(lead)
    rows = np.stack([a_cx, a_cy, a_cx * off[..., 0] / 8 + a_w * (1 + off[..., 2] / 8),
                     a_cy * off[..., 1] / 8 + a_h * (1 + off[..., 3] / 8), row_t], -1)
    return np.stack(go, -1), rows


def box_reduce_logits(logits, gattn):
    """Per-point weight gradients -> grad_logits (B,Lq,H,L*P), float64: a (g - sum a g), a the softmax of the row."""
    z = np.asarray(logits, dtype=np.float64)
    g = np.asarray(gattn, dtype=np.float64).reshape(z.shape)
    e = np.exp(z - z.max(-1, keepdims=True))
    a = e / e.sum(-1, keepdims=True)
    return a * (g - (a * g).sum(-1, keepdims=True))


# The cases of the matrix whose inputs from ``problem`` break the cell-edge condition (a box of size <= 0 puts a whole
# row of points on one line, and that line fell on an edge; 1-4 points of 384-1 280): the same construction from
# another seed.  Keys: (geometry, C, angle_mode, ref_dim, per_head, with_vr).
BOX_BWD_RESEED = {("model", 64, 0, 4, False, True): 1000003, ("model", 64, 1, 5, False, False): 1000003,
                  ("ragged", 16, 1, 5, False, False): 1000003, ("ragged", 64, 0, 4, True, False): 1000003,
                  ("sixteen_levels", 16, 2, 5, True, False): 1000003, ("sixteen_levels", 32, 1, 7, True, False): 1000003,
                  ("sixteen_levels", 32, 1, 7, True, True): 1000003, ("sixteen_levels", 32, 2, 5, True, True): 1000003,
                  ("sixteen_levels", 64, 2, 5, True, True): 2000006, ("k4", 32, 1, 5, True, True): 1000003,
                  ("k4", 32, 1, 7, False, False): 2000006, ("k4", 64, 0, 4, True, False): 1000003,
                  ("k4", 64, 1, 5, True, False): 1000003, ("k4", 64, 1, 7, True, True): 1000003,
                  ("encoder", 32, 0, 4, False, False): 1000003, ("encoder", 32, 1, 5, False, False): 1000003,
                  ("encoder", 32, 1, 7, True, True): 1000003, ("encoder", 64, 1, 7, True, False): 1000003}


@functools.lru_cache(maxsize=None)
def box_bwd_case(geometry, C, angle_mode, ref_dim, per_head, with_vr):
    bump = BOX_BWD_RESEED.get((geometry, C, angle_mode, ref_dim, per_head, with_vr))
    if bump is None:
        return box_boxes_problem(geometry, C, angle_mode, ref_dim, per_head, with_vr)
    make = np.random.default_rng
    np.random.default_rng = lambda seed: make(seed + bump)           # (problem() seeds its generator from its arguments)
    try:
        return box_boxes_problem.__wrapped__(geometry, C, angle_mode, ref_dim, per_head, with_vr)
    finally:
        np.random.default_rng = make


def box_edge_share(g):
    """Share of the sample points of the problem ``g`` within 1e-4 px of a bilinear cell edge (float32 grid on the CPU)."""
    from boxer_amd.modules import _kernel_offsets
    P = g["dims"][6]
    k = int(round(P ** 0.5))
    kidx = _kernel_offsets(k, k).float().numpy()
    grid = grid_f32(g["ref"], g["off"], kidx, g["vr"], g["angle_mode"])
    return float(on_cell_edge(grid.astype(np.float64), g["shapes"]).mean())


def box_upstream(g, dt, seed=0):
    B, S, H, C, L, Lq, P = g["dims"]
    return rounded(np.random.default_rng(100 + seed).standard_normal((B, Lq, H * C)), dt)


def device_args(g, dt):
    return dict(value=dev(g["value"], dt), shapes=dev(g["shapes"]), lsi=dev(g["lsi"]), ref=dev(g["ref"]),
                off=dev(g["off"]), kidx=box_kernel_indices(g["dims"][6]), vr=None if g["vr"] is None else dev(g["vr"]),
                logits=dev(g["logits"]), mode=g["angle_mode"])


def eligible(geometry, C, dt):
    from boxer_amd import ops
    geo = BOX_GEOMETRY[geometry]
    S = tables(geo["levels"])[2]
    return ops.box_backward_boxes_ok(torch.empty(geo["B"], S, geo["H"], C, dtype=dt, device="cuda"),
                                     len(geo["levels"]), geo["Lq"], geo["P"])


def function_inputs(g):
    leaf = lambda x: dev(x).float().requires_grad_()
    return dict(value=leaf(g["value"]), ref=leaf(g["ref"]), off=leaf(g["off"]), logits=leaf(g["logits"]),
                shapes=dev(g["shapes"]), lsi=dev(g["lsi"]), kidx=box_kernel_indices(g["dims"][6]),
                vr=None if g["vr"] is None else dev(g["vr"]), mode=g["angle_mode"])


def run_boxes_function(x, dt):
    from boxer_amd import BoxAttnBoxesFunction
    value = x["value"] if dt == torch.float32 else x["value"].to(dt)
    vr = None if x["vr"] is None else x["vr"].view(-1, x["off"].size(3), 2)
    return BoxAttnBoxesFunction.apply(value, x["shapes"], x["lsi"], x["ref"], x["off"], x["kidx"], vr, x["logits"],
                                      x["mode"])


def run_point_functions(x, dt):
    import boxer_amd as ba
    B, Lq, H, L = x["off"].shape[:4]
    grid = ba.BoxGridFunction.apply(x["ref"], x["off"], x["kidx"], x["vr"], x["mode"])
    attn = ba.LogitSoftmaxFunction.apply(x["logits"]).view(B, Lq, H, L, -1)
    fn = {torch.float32: ba.BoxAttnFunction, torch.bfloat16: ba.BoxAttnBF16Function,
          torch.float16: ba.BoxAttnF16Function}[dt]
    return fn.apply(x["value"], x["shapes"], x["lsi"], grid, attn, 64)


G9_NAMES = sorted(n for n in GOLDENS if n.startswith("G9"))


def golden_loss(g):
    return lambda outs: (outs[0].double() * dev(g["gout0"]).double()).sum()


STAGED_C, STAGED_P = 32, 4
STAGED_GEOMETRY = {
    "two_levels": dict(levels=[(8, 8), (4, 4)], B=1, H=2),                               # whole tiles
    # ragged tiles on every level, a head count that is neither 8 nor a power of two
    "four_levels": dict(levels=[(37, 23), (19, 12), (10, 6), (5, 3)], B=2, H=3),
    "three_levels": dict(levels=[(16, 16), (8, 8), (4, 4)], B=1, H=8),
    "one_level": dict(levels=[(9, 13)], B=2, H=1),
    "tiny_levels": dict(levels=[(4, 5), (2, 3), (1, 1)], B=1, H=2),                      # smaller than a tile, a 1 x 1 level
    # tile numbering and XCD order beyond a handful of workgroups (test_mid_size only)
    "mid": dict(levels=C2_LEVELS, B=2, H=8),
}
FAMILIES = ["local", "scattered"]
STAGED_SPLIT = {"f32": "none", "bf16": "bf16", "f16": "f16"}


@functools.lru_cache(maxsize=None)
def staged_problem(geometry, family, angle_mode, ref_dim, per_head, with_vr):
    """numpy / float32 inputs of one case (the same for every storage type): box_boxes_problem with one
    query a pixel and the two families."""
    geo = STAGED_GEOMETRY[geometry]
    shapes, lsi, S = tables(geo["levels"])
    B, H, L, Lq = geo["B"], geo["H"], len(geo["levels"]), S
    V = 5 if angle_mode == 1 else 4
    rng = np.random.default_rng(104729 + 1000 * sorted(STAGED_GEOMETRY).index(geometry) + 500 * FAMILIES.index(family)
                                + 8 * angle_mode + 2 * ref_dim + per_head)
    rshape = (B, Lq, H) if per_head else (B, Lq)
    ref = np.concatenate([rng.uniform(0.05, 0.95, rshape + (2,)), rng.uniform(0.05, 0.7, rshape + (2,)),
                          rng.uniform(-3.0, 3.0, rshape + (ref_dim - 4,))], -1)
    if family == "local":                          # query i = pixel i: a window of four pixels of its own level
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
    if family == "local":
        off[..., :4] *= 0.5
    rows = off.reshape(-1, V)
    rows[rng.random(len(rows)) < 0.15, 2] = -12.0            # negative predicted sizes: relu puts every point on the
    rows[rng.random(len(rows)) < 0.15, 3] = -9.5             # centre line / centre
    rows[0, 2:4] = -8.0                                      # size exactly zero: w + (-8 / 8) w
    if V == 5:
        rows[1, 4] = 77.0                                    # 4.8 turns
    logits = 3.0 * rng.standard_normal((B, Lq, H, L * STAGED_P))
    logits += 30.0 * np.where(rng.random((B, Lq, H, 1)) < 0.5, -1.0, 1.0)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(shapes=shapes, lsi=lsi, S=S, dims=(B, S, H, STAGED_C, L, Lq, STAGED_P),
                value=every_type(rng.standard_normal((B, S, H, STAGED_C))),     # (numbers every storage type holds exactly)
                ref=f32(ref), off=f32(off), logits=f32(logits), angle_mode=angle_mode,
                vr=f32(rng.uniform(0.5, 1.0, (B, 1, 1, L, 1, 2))) if with_vr else None)


def flavours_of(geometry):
    """The 16 flavours; for the largest geometry of the matrix the four (angle mode, reference values) pairs with
    windows per head / valid ratios alternating (its float64 model is the slowest)."""
    if geometry != "four_levels":
        return FLAVOURS
    return [(pair, i % 2 == 1, i % 2 == 0) for i, pair in enumerate(sorted({f[0] for f in FLAVOURS}))]


def operands(g, dt, value=None):
    return (dev(g["value"], dt) if value is None else value, dev(g["shapes"]), dev(g["lsi"]), dev(g["ref"]),
            dev(g["off"]), box_kernel_indices(STAGED_P), None if g["vr"] is None else dev(g["vr"]), dev(g["logits"]),
            g["angle_mode"])


def run_staged_forward(g, args):
    from boxer_amd import ops
    B, S, H, _, L, Lq, _ = g["dims"]
    assert ops.box_forward_boxes_staged_ok(args[0], args[1], args[2], Lq, STAGED_P), "not eligible: %s" % (g["dims"],)
    out = ops.box_attn_forward_boxes_staged(*args)
    assert out.dtype == args[0].dtype and tuple(out.shape) == (B, Lq, H * STAGED_C), (out.dtype, tuple(out.shape))
    return out


ENCODER_MODULE_LEVELS = [(8, 8), (4, 4)]


def encoder_module(kind, native_bf16):
    """BoxAttention / rotated Box3dAttention with 2 heads of 32 channels and random parameters, and a small encoder input
    built as boxer_amd.layers builds it: -> (module, forward arguments)."""
    import boxer_amd
    from boxer_amd import layers
    torch.manual_seed(11)
    if kind == "box":
        m = boxer_amd.BoxAttention(64, len(ENCODER_MODULE_LEVELS), 2)
    else:
        m = boxer_amd.Box3dAttention(64, len(ENCODER_MODULE_LEVELS), 2, with_rotation=True)
    for p in m.parameters():
        torch.nn.init.normal_(p, std=0.1)
    m = m.cuda()
    m.native_bf16 = native_bf16
    m.fused_grid = m.fused_pointwise = True
    shapes, lsi, S = tables(ENCODER_MODULE_LEVELS)
    B = 2
    if kind == "box":
        ref = layers.encoder_ref_windows_2d(ENCODER_MODULE_LEVELS, B, device="cuda")
    else:
        ref = layers.encoder_ref_windows_3d(ENCODER_MODULE_LEVELS, B, device="cuda")[:, :, :2].contiguous()
    src = torch.randn(B, S, 64, device="cuda")
    ratios = 0.5 + 0.5 * torch.rand(B, 1, 1, len(ENCODER_MODULE_LEVELS), 1, 2, device="cuda")
    return m, (src + 0.1 * torch.randn_like(src), src, dev(shapes), None, dev(lsi), ratios, ref)


MATRIX = ["two_levels", "four_levels", "three_levels", "one_level", "tiny_levels"]
# (geometry, family, angle_mode, ref_dim, per_head, with_vr) -> what is added to problem's seed
STAGED_BWD_RESEED = {("one_level", "local", 1, 5, True, False): 1000003,        # 0.214 % from problem's own seed
                     ("one_level", "scattered", 1, 7, False, False): 1000003,   # 0.214 %
                     ("tiny_levels", "local", 0, 4, True, True): 1000003,       # 0.309 %
                     ("tiny_levels", "scattered", 1, 5, True, True): 1000003}   # 0.309 %


@functools.lru_cache(maxsize=None)
def staged_bwd_case(geometry, family, angle_mode, ref_dim, per_head, with_vr):
    """staged_problem, from another seed for the keys of RESEED."""
    key = (geometry, family, angle_mode, ref_dim, per_head, with_vr)
    bump = STAGED_BWD_RESEED.get(key)
    if bump is None:
        return staged_problem(*key)
    make = np.random.default_rng
    np.random.default_rng = lambda seed: make(seed + bump)           # (problem() seeds its generator from its arguments)
    try:
        return staged_problem.__wrapped__(*key)
    finally:
        np.random.default_rng = make


def model_of(g, gout):
    """grad_value's planes (want / A / E / n / G / W, (B, S, H, C)) for the problem ``g`` (keys of
    box_boxes_problem) and the upstream gradient ``gout`` (B, Lq, H * C)."""
    value = eb.f64(every_type(g["value"]))
    B, S, H, C = value.shape
    P = g["dims"][6]
    loc, dloc = eb.grid_reference(g["ref"], g["off"], kernel_offsets(int(round(P ** 0.5))), g["vr"],
                                  g["angle_mode"])
    Lq, L = loc.shape[1], loc.shape[3]
    w, dw = eb.softmax_reference(g["logits"])
    r = eb._reference(value, eb.f64(g["shapes"]).astype(np.int64), eb.f64(g["lsi"]).astype(np.int64), loc,
                      [w.reshape(B, Lq, H, L, P)], [eb.f64(gout).reshape(B, Lq, H, C)], False, slack=dloc,
                      dws=[dw.reshape(B, Lq, H, L, P)])
    return r["grad_value"]


@functools.lru_cache(maxsize=16)
def value_reference(geometry, C, flavour):
    g = bwd_problem(geometry, C, flavour)
    return model_of(g, bwd_upstream(g))


def value_call(args, gout, want=3, need_ref_grad=True):
    from boxer_amd import ops
    res = ops.box_attn_backward_boxes_value(*args, gout, want=want, need_ref_grad=need_ref_grad)
    torch.cuda.synchronize()
    return res


def same_parameter_gradients(got, base, what):
    for name, x, y in zip(GRAD_NAMES, got, base):
        assert x.dtype == torch.float32 and torch.equal(x, y), "%s: %s differs from box_attn_backward_boxes" % (what, name)


def staged_upstream(g):
    B, S, H, _, L, Lq, _ = g["dims"]
    return every_type(np.random.default_rng(100).standard_normal((B, Lq, H * STAGED_C)))     # (every storage type holds it)


def run_staged_backward(g, args, gout, need_ref_grad=True):
    from boxer_amd import ops
    B, S, H, _, L, Lq, _ = g["dims"]
    assert ops.box_backward_boxes_staged_ok(args[0], args[1], args[2], Lq, STAGED_P), "not eligible: %s" % (g["dims"],)
    got = ops.box_attn_backward_boxes_staged(*args, gout, need_ref_grad=need_ref_grad)
    V = 5 if g["angle_mode"] == 1 else 4
    assert tuple(got[0].shape) == (B, Lq, H, L, V) and tuple(got[2].shape) == (B, Lq, H, L * STAGED_P), \
        (tuple(got[0].shape), tuple(got[2].shape))
    assert (got[1] is None) != need_ref_grad and (got[1] is None or tuple(got[1].shape) == (B, Lq, H, L, 5)), \
        (need_ref_grad, None if got[1] is None else tuple(got[1].shape))
    assert all(t is None or t.dtype == torch.float32 for t in got), [None if t is None else t.dtype for t in got]
    return got
