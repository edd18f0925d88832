"""A second reference for box and instance attention that also says how wrong a result may be (test helper; not a
conftest, never imported by boxer_amd).  Vectorised numpy in float64, restated from the operator's definition
(DESIGN.md 1), not from any kernel.

For every output the reference is a dict of arrays of that output's shape:

  want   the exact value (float64 sums of exact products of the stored, already rounded inputs);
  A      the sum of the absolute values of the same terms (every factor by its absolute value, every difference by the
         sum of the absolute values);
  E      the allowance for the float32 pixel coordinate: pix = loc * size - 0.5 is formed in float32 by every kernel (and
         by the reference); for loc in [-0.5, 1.5] a coordinate is off by at most 3 size 2^-24 (one rounding of the
         product, <= 1.5 size 2^-24, one of the difference, likewise), a corner weight -- a product of two fractions in
         [0, 1] -- by at most eps_l = 3 (W_l + H_l) 2^-24 = 1.5 (W_l + H_l) 2^-23.  E is the sum over the element's terms
         with the corner weight replaced by eps_l.  A point whose coordinate is within 3 size 2^-24 of an integer, of -1
         or of the map's far side may land in the neighbouring cell, or on the other side of the window test, in float32:
         it adds E-only entries to every pixel (and reads E-only entries from every value row) it would touch if its
         coordinates moved by that much -- there its weight is at most the distance moved, which eps_l covers;
  n      the number of terms of the element;
  G      (out, mask_out, grad_value) the sum of the absolute values of the terms' 16-bit operand (value, grad_out,
         grad_mask element): what the absolute part of an f16 weight split multiplies.

grad_loc jumps at cell edges: its reference also has ``skip`` (points within 1e-4 px of an edge, left out of the check)
and ``edge_share`` (their share; callers assert it is <= EDGE_CAP -- a condition on the inputs, not a tolerance).

``hold`` asserts, for every element,

    |got - want| <= u (|want| + R) + R + t,      R = ((n + 8) 2^-24 + s) A + E  [+ 2^-25 G for f16 splits]

u, t: the one RNE rounding to the stored type (STORE); s: the accumulate route's weight split (SPLIT).  Where
A + E = 0 the bound is 0: an element nobody contributes to must be exactly zero.  The store term u (|want| + R) + t is
evaluated exactly, as half the type's spacing at |want| + R (half_ulp): u x is that only at the bottom of a binade and
twice it at the top, where a result one whole step off the correctly rounded one would still pass -- with u x a dropped
corner went unnoticed in 5.5 % of the cases on all-positive bf16 data, with half_ulp in 2.0 %
(tests/test_error_bounds.py).  Whatever passes this passes the formula above.

From boxes (``boxes_reference``): the kernels that take reference windows, offsets, kernel_indices, valid ratios and
logits instead of a sampling grid and weights are held against a model that starts from those inputs -- the modules'
_where_to_attend and softmaxes restated from DESIGN.md 1 / 4.4 / 4.6 and the reference's module code, in float64.
float32 locations and weights are not the float64 ones, so two allowances join the bound; u = 2^-24 below.

  dloc   (grid_reference) per point and axis, normalised units: what a float32 evaluation in the documented order
         (every operation rounded once, no fused multiply-add) may differ by.  Without rotation the chain to a
         coordinate is  off / 8 * size (/ 8 is exact; 1 rounding), + centre (1), off / 8 * size, + size (2),
         kidx * relu(size) (1), the sum (1): n = 6 roundings, each of a partial result that is at most
         T = |centre| + |off / 8 size_ref| + |kidx| (|size_ref| + |off / 8 size_ref|) in magnitude (the last term only
         where the float64 size is positive), so dloc = 6 u T to first order; the cancellation in a size near zero is
         covered because T sums absolute values.  With rotation both local coordinates enter either axis: T takes both
         |kidx| terms (|cos|, |sin| <= 1) and n = 9 (two more products, the difference).  The sine and cosine are each off
         by at most dtheta + 2^-22: dtheta = 3 u (|ref angle| + |off / 16|) 2 pi in mode 1 (the sum, the product with
         float32's 2 pi, that constant's own representation error; / 16 and * 2 are exact), 0 in mode 2 (theta is an input);
         2^-22 = 4 ulp at 1.0 is an ALLOWANCE for the device sincosf at any argument, not a measurement -- no
         accuracy statement for it was found in the ROCm documentation installed beside this project, so none is cited;
         profiles/boxes_error_bounds.log records how much of dloc the kernel uses.  They multiply the local coordinates:
         (dtheta + 2^-22) (|lx| + |ly|) on either axis.  Valid ratios: one more rounding, everything times |vr|.
  dw     (softmax_reference, instance_weights_reference) per weight, relative.  exp(d), d = z - max, is formed as
         exp2(d log2 e): the subtraction (1 rounding of |d|), the constant log2 e (relative u) and the product (1) move
         the exponent by at most 3 u |d| log2 e, the result by the factor 2^that = 1 +- 3 u |d|; the exp2 instruction adds
         an ulp (2 u, relative): de = (3 |d| + 2) u.  The float32 sum of N positive terms, in any order, is off by at
         most (N - 1) u relatively plus the weighted mean of its terms' de, sum_j a_j de_j; the reciprocal (a division:
         1 rounding) and the product (1).  dw_i = de_i + sum_j a_j de_j + (N + 1) u; the spatial weights of instance
         attention -- a softmax over the row's 4 L cells, times 1 / m^2 -- take 2 u more (that constant, the product).
         A logit more than 87 below its row's maximum would leave float32's normal range, where a relative allowance
         means nothing: the reference refuses such a row (no case has one; the widest spread tested is 60).

How they enter.  level_terms / _reference take the locations' ``slack`` = dloc: a point's coordinate allowance becomes
3 size u + size dloc (it was 3 size u), its eps the sum of the two axes', and the alternative cells are searched with it.
A weight a_i off by dw_i |a_i| moves a term by dw_i |term|: the plane W sums that per element and is added to R beside the
split term (``bound``); the constants of R are untouched, and without slack / dws nothing changes, bit for bit.

The three gradients of the backward from boxes are linear in the per-point grad_loc, grad_spatial, grad_level:
  grad_offsets[0:2] = size_ref / 8 sum_p g_p,   [2:4] = relu'(size) size_ref / 8 sum_p kidx_p g_p    (g = grad_loc vr)
  grad_ref_rows[0:2] = sum_p g_p,   [2:4] = off[0:2] / 8 sum_p g_p + relu'(size) (1 + off[2:4] / 8) sum_p kidx_p g_p,  [4] = 0
  grad_logits[c] = a_c / m^2 (Gs_c - sum_c' a_c' Gs_c') + t_c (Gt_c - sum_l' t_l' Gt_l')        (Gs, Gt: the cells' sums)
(d grid / d box and the Jacobians of the two softmaxes, from the definitions).  want reduces in float64; A and E (with
W) with the absolute values of the same coefficients, every difference as a sum; n is the largest n of the points plus
the reduction's own roundings (P + 6 for the box rows: the vr and kidx products, a P-term sum, the row's last few;
m^2 + 4 L + 8 for the logits); a weight a_c off by da_c adds (da_c + max da) times the A of its bracket to E.  A size whose
float32 sign is not certain (|size| <= 2 u (|size_ref| + |off / 8 size_ref|), not exactly 0) allows either relu'.
grad_loc jumps at cell edges and a sum cannot leave a point out: a point within EDGE_PX + its coordinate allowance of
an integer coordinate has two legitimate own-axis gradients; want takes the float64 side, J = |the neighbouring
cell's - that| goes into E of every element the point feeds (times the coefficient).  ``edge_share`` is the share of
such points (callers assert <= EDGE_CAP), ``edge_dominated`` the share of elements whose bound is more than half J.

The box kind's training step (``boxes_reference(kind="box", grad_out=...)``: grad_offsets (.., L, V), grad_ref_rows
(.., L, 5), grad_logits (.., L P)) in the three angle modes, V = 4 or 5; g = grad_loc vr, l = kidx relu(size), the sums
over the P points of a (b, q, h, l) row, sin and cos of the row's theta (1 and 0 in mode 0):
  a_cx = sum gx,   a_cy = sum gy,   a_w = relu'(w) sum kx (gx cos + gy sin),   a_h = relu'(h) sum ky (gy cos - gx sin),
  a_t = sum gx (-lx sin - ly cos) + gy (lx cos - ly sin)
  grad_offsets = [a_cx rw / 8, a_cy rh / 8, a_w rw / 8, a_h rh / 8, a_t 2 pi / 16 (mode 1 only; else 0)]
  grad_ref_rows = [a_cx, a_cy, a_cx off0 / 8 + a_w (1 + off2 / 8), a_cy off1 / 8 + a_h (1 + off3 / 8),
                   a_t 2 pi (mode 1) | a_t (mode 2) | 0 (mode 0)]
  grad_logits = a (Gw - sum_row a Gw)                         (a: the softmax over the row's L P logits, Gw: grad_attn)
(d grid / d box through the rotation, and the softmax Jacobian, from the definitions of DESIGN.md 1 / 4.4).  A takes every
factor by its absolute value -- |cos| and |sin| with their own values, every difference as a sum, and in a_t the size
inside l as |size_ref| + |off / 8 size_ref| where the float32 size may be positive: the size is a difference, and its two
roundings are then relative to something A holds.  E carries the points' E + W and the edge jumps J times the same
coefficients, and three more terms: the float32 sine and cosine, each within dtheta + SINCOS_ABS of the float64 one (the
ALLOWANCE of grid_reference again, not a measurement; test_gpu_boxes_error_bounds measures 0.49 ulp on one device), add
(dtheta + SINCOS_ABS) sum |kx| (A_gx + A_gy) to a_w, the like to a_h and (dtheta + SINCOS_ABS) sum (|lx| + |ly|)
(A_gx + A_gy) to a_t; a size whose float32 sign is not certain allows either relu' (the whole A of a_w / a_h into E) and
either relu(size) in a_t (A covers it).  The weights' allowance enters grad_logits as (da + max da) a (A_Gw + sum a A_Gw).
n is the points' largest n plus the reduction's roundings, counted from boxattn_grid.h (grid_grad_add, grid_grad_store) and
the softmax backward of boxattn_pointwise.h:
  mode 0, the box rows: P + 6 as above (g vr; kx g; the P-term sum; 1 + off / 8, the product, the sum of the row's two);
  rotated, the box rows: P + 8 (two more: a product with cos or sin, the sum of the two);
  the angle entries: P + 10 (g vr; the size's two; kx relu(w); the product with sin; the difference; the product with gx;
    the sum of the two halves; the P-term sum; float32's 2 pi and the product with it; / 16 is exact);
  grad_logits: L P + 3 (a Gw; the L P-term sum in any order; Gw - sum; the product with a).
A fused multiply-add only removes roundings from these counts.  ``box_gradients`` redoes the reductions from the kept
per-point planes with a wrong formula written into ``want`` (``mutation``: the tests of the bound).  The building blocks
on their own -- ``grid_backward_reference``, ``softmax_backward_reference``, ``cell_logits_backward_reference`` -- are the
same reductions on exact float32 upstream gradients (want = g, A = |g|, E = 0, n = 0).
"""

import numpy as np
import torch

EDGE_PX = 1e-4          # grad_loc: points this close to a bilinear cell edge are left out (tests/point_cases.on_cell_edge)
EDGE_CAP = 2e-3         # ... and may be at most this share of a case's points (tests/boxes_cases.EDGE_CAP)

# stored type -> (u, t): one round-to-nearest-even; f16's t is half the subnormal spacing 2^-24
STORE = {"float32": (2.0 ** -24, 0.0), "bf16": (2.0 ** -8, 0.0), "f16": (2.0 ** -11, 2.0 ** -25)}
# stored type -> (significand bits p, smallest normal exponent): what half_ulp evaluates u x + t from
FORMAT = {"float32": (24, -126), "bf16": (8, -126), "f16": (11, -14)}
# accumulate route -> s
#   none    VALU, atomic, generic and float32-MFMA kernels: float32 products of float32 weights
#   split3  BOXATTN_ACC_SPLIT: rows and weights in three exact bf16 terms, the six partial products above 2^-24 of the
#           product kept (boxattn_binned_tr.h: binned_accumulate_split_kernel); the dropped ones, w2 g3 and w3 g2, are
#           at most 2^-24 |w g| each (w3 g3: 2^-32, inside the slack of the (n + 8) 2^-24 term)
#   bf16    two bf16 terms, |w - hi - lo| <= 2^-17 |w| (boxattn_dense_fwd.h, boxattn_binned_tr.h); twice that: the group
#           records sum coinciding corners in float32 before the split
#   f16     two f16 terms, |w - hi - lo| <= 2^-22 |w| + 2^-25; twice the relative part, the absolute part
#           times the operand it multiplies (G)
SPLIT = {"none": 0.0, "split3": 2.0 ** -23, "bf16": 2.0 ** -16, "f16": 2.0 ** -21}
_NAMES = {torch.float32: "float32", torch.bfloat16: "bf16", torch.float16: "f16"}


def store_name(dtype):
    return dtype if isinstance(dtype, str) else _NAMES[dtype]


def f64(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def round_to(x, store):
    """float64 -> the nearest number of the stored type (ties to even), as float64.  bf16: 8 significant bits."""
    x = np.asarray(x, dtype=np.float64)
    store = store_name(store)
    if store == "float32":
        return x.astype(np.float32).astype(np.float64)
    if store == "f16":
        return x.astype(np.float16).astype(np.float64)
    m, e = np.frexp(x)
    return np.ldexp(np.rint(m * 256.0), e - 8)


# ------------------------------------------------------------------ the terms of one level
class _Acc:
    """want / A / E / n / G of one output, as (rows, C) float64 planes summed into by row index."""

    def __init__(self, shape, with_g, more=()):
        self.shape = shape
        self.C = shape[-1]
        self.rows = int(np.prod(shape[:-1]))
        names = ("want", "A", "E", "n") + (("G",) if with_g else ()) + more
        self.planes = {k: np.zeros(self.rows * self.C) for k in names}

    def add(self, idx, **vals):
        """idx (m,): row of every entry; vals: name -> (m, C) or (m, 1) array."""
        flat = (idx[:, None] * self.C + np.arange(self.C)[None, :]).ravel()
        for name, v in vals.items():
            v = np.broadcast_to(v, (idx.shape[0], self.C)).ravel()
            self.planes[name] += np.bincount(flat, v, minlength=self.rows * self.C)

    def result(self):
        return {k: v.reshape(self.shape) for k, v in self.planes.items()}


def _corners(y0, x0, Hl, Wl):
    """-> rows (m, 4) of the four corners inside the level (clipped where outside), ok (m, 4).  Corner k = 2 dy + dx."""
    ys = np.stack([y0, y0, y0 + 1, y0 + 1], 1)
    xs = np.stack([x0, x0 + 1, x0, x0 + 1], 1)
    ok = (ys >= 0) & (ys <= Hl - 1) & (xs >= 0) & (xs <= Wl - 1)
    return np.clip(ys, 0, Hl - 1) * Wl + np.clip(xs, 0, Wl - 1), ok


def level_terms(value, shapes, lsi, loc, l, frac_hook=None, slack=None):
    """The sample points of level ``l`` that pass the window test (-1, H) x (-1, W) (a coordinate of exactly -1 is
    outside, as in the reference kernels): dict of b, q, h, p (m,), rows / ok (m, 4), w (m, 4) bilinear weights,
    v (m, 4, C) corner rows (zeros outside the map), fy, fx, eps.  Also ``alts``: the (point, cell) pairs float32 could
    take instead (see the module docstring), each b, q, h, p, rows, ok, v.  ``slack`` (B, Lq, H, L, P, 2), normalised
    units: what the location itself may be off by (grid_reference's dloc); a point's coordinate allowance is then
    3 size 2^-24 + size slack, its eps (an (m, 1) column in every returned entry) the sum of the two axes'."""
    B, S, Hh, C = value.shape
    Lq, P = loc.shape[1], loc.shape[4]
    Hl, Wl = int(shapes[l][0]), int(shapes[l][1])
    x = (loc[:, :, :, l, :, 0] * Wl - 0.5).ravel()
    y = (loc[:, :, :, l, :, 1] * Hl - 0.5).ravel()
    b, q, h, p = (a.ravel() for a in np.indices((B, Lq, Hh, P)))
    vlev = value[:, int(lsi[l]):int(lsi[l]) + Hl * Wl]

    def gather(sel, y0, x0):
        rows, ok = _corners(y0, x0, Hl, Wl)
        v = vlev[b[sel][:, None], rows, h[sel][:, None]] * ok[:, :, None]
        d = dict(b=b[sel], q=q[sel], h=h[sel], p=p[sel], rows=rows, ok=ok, v=v)
        if slack is not None:
            d["eps"] = (dx + dy)[sel][:, None]
        return d

    # what float32 may do instead: both coordinates moved by +- 3 size 2^-24 (plus the location's own slack)
    dx, dy = 3.0 * Wl * 2.0 ** -24, 3.0 * Hl * 2.0 ** -24
    if slack is not None:
        dx = dx + Wl * slack[:, :, :, l, :, 0].ravel()
        dy = dy + Hl * slack[:, :, :, l, :, 1].ravel()
    inside = (y > -1) & (x > -1) & (y < Hl) & (x < Wl)
    sel = np.nonzero(inside)[0]
    y0, x0 = np.floor(y[sel]).astype(np.int64), np.floor(x[sel]).astype(np.int64)
    fy, fx = y[sel] - y0, x[sel] - x0
    if frac_hook is not None:
        fy, fx = frac_hook(l, sel, fy, fx)
    t = gather(sel, y0, x0)
    t.update(fy=fy, fx=fx, w=np.stack([(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx], 1),
             Hl=Hl, Wl=Wl, sel=sel)
    if slack is None:
        t["eps"] = 3.0 * (Wl + Hl) * 2.0 ** -24
    cand = {}
    for name, c, d, size in (("x", x, dx, Wl), ("y", y, dy, Hl)):
        for s in (-1, 1):
            m = c + s * d
            cand[name, s] = ((m > -1) & (m < size), np.floor(m).astype(np.int64))
    xdiff = (cand["x", 1][0] != cand["x", -1][0]) | (cand["x", 1][1] != cand["x", -1][1])
    ydiff = (cand["y", 1][0] != cand["y", -1][0]) | (cand["y", 1][1] != cand["y", -1][1])
    y0_all, x0_all = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
    alts = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            (okx, cx), (oky, cy) = cand["x", sx], cand["y", sy]
            take = okx & oky & ~(inside & (cy == y0_all) & (cx == x0_all))
            if sx == 1:
                take &= xdiff
            if sy == 1:
                take &= ydiff
            s2 = np.nonzero(take)[0]
            if s2.size:
                alts.append(gather(s2, cy[s2], cx[s2]))
    t["alts"] = alts
    return t


def on_edge(loc, shapes):
    """(B, Lq, H, L, P, 1): points within EDGE_PX of a bilinear cell edge."""
    size = np.asarray(shapes, dtype=np.float64)[None, None, None, :, None, ::-1]
    pix = loc * size - 0.5
    return (np.abs(pix - np.round(pix)) < EDGE_PX).any(-1, keepdims=True)


def _edge_jumps(gloc, value, shapes, lsi, loc, l, weights, ups, instance, slack):
    """grad_loc of level ``l``: for every point and axis whose pixel coordinate is within EDGE_PX + its slack of an
    integer (a cell edge, -1 or the far side of the window test) the own-axis gradient has two legitimate values;
    J gets |the value in the neighbouring cell - the float64 side's| (the gradient along an axis does not depend on that
    axis' fraction, so any coordinate inside the neighbouring cell gives it)."""
    B, S, Hh, C = value.shape
    Lq, P = loc.shape[1], loc.shape[4]
    Hl, Wl = int(shapes[l][0]), int(shapes[l][1])
    vlev = value[:, int(lsi[l]):int(lsi[l]) + Hl * Wl]
    pix = [loc[:, :, :, l, :, 0] * Wl - 0.5, loc[:, :, :, l, :, 1] * Hl - 0.5]
    sl = np.zeros(loc.shape[:3] + (P, 2)) if slack is None else slack[:, :, :, l]
    near_all = gloc.setdefault("near", np.zeros(gloc["want"].shape, dtype=bool))

    def grad(b, q, h, p, x, y, axis):
        inside = (y > -1) & (x > -1) & (y < Hl) & (x < Wl)
        y0, x0 = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
        fy, fx = (y - y0)[:, None], (x - x0)[:, None]
        rows, ok = _corners(y0, x0, Hl, Wl)
        v = vlev[b[:, None], rows, h[:, None]] * ok[:, :, None]
        tt = weights[0][b, q, h, l, p][:, None] * ups[0][b, q, h]
        if instance:
            tt = tt + weights[1][b, q, h, l, p][:, None] * ups[1][b, q, p, h]
        dv = (1 - fy) * (v[:, 1] - v[:, 0]) + fy * (v[:, 3] - v[:, 2]) if axis == 0 else \
            (1 - fx) * (v[:, 2] - v[:, 0]) + fx * (v[:, 3] - v[:, 1])
        return np.where(inside, (Wl, Hl)[axis] * (tt * dv).sum(1), 0.0)

    for axis, size in ((0, Wl), (1, Hl)):
        c = pix[axis]
        r = np.round(c)
        near = np.abs(c - r) < EDGE_PX + (3.0 * size * 2.0 ** -24 + size * sl[..., axis])
        near_all[:, :, :, l, :, axis] = near
        b, q, h, p = np.nonzero(near)
        if not b.size:
            continue
        xy = [pix[0][b, q, h, p], pix[1][b, q, h, p]]
        here = grad(b, q, h, p, xy[0], xy[1], axis)
        xy[axis] = np.where(c[b, q, h, p] >= r[b, q, h, p], r[b, q, h, p] - 0.5, r[b, q, h, p] + 0.5)
        gloc["J"][b, q, h, l, p, axis] = np.abs(grad(b, q, h, p, xy[0], xy[1], axis) - here)


def _reference(value, shapes, lsi, loc, weights, ups, instance, frac_hook=None, weight_hook=None, slack=None, dws=None):
    """weights: [attn] or [spatial_w, level_w], (B, Lq, H, L, P); ups: [grad_out (B, Lq, H, C)] or that and grad_mask
    (B, Lq, P, H, C).  The hooks mutate what goes into ``want`` only (tests of the bound itself): frac_hook(l, sel, fy,
    fx) -> fy, fx; weight_hook(a w_k) -> the weight products the sums of out / mask_out / grad_value use.
    slack: level_terms' (the locations' own allowance); dws: one relative allowance (B, Lq, H, L, P) per weight set.
    With either, every output that multiplies a weight gets a plane W = sum of dw |term| (beside the split term in
    R), and grad_loc no ``skip``: its points within EDGE_PX + slack of a cell edge get ``J``, the size of the jump of
    the own-axis gradient to the other side of the edge (also added to E; want stays on the float64 side)."""
    B, S, Hh, C = value.shape
    ext = slack is not None or dws is not None
    if ext and dws is None:
        dws = [np.zeros(loc.shape[:5]) for _ in weights]
    _AccW = (lambda shape, g: _Acc(shape, g, ("W",))) if ext else _Acc
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    out = _AccW((B, Lq, Hh, C), True)
    mask = _AccW((B, Lq, P, Hh, C), True) if instance else None
    gval = _AccW((B, S, Hh, C), True)
    point = {k: {m: np.zeros((B, Lq, Hh, L, P)) for m in ("want", "A", "E", "n")}
             for k in (("grad_spatial", "grad_level") if instance else ("grad_attn",))}
    gloc = {m: np.zeros((B, Lq, Hh, L, P, 2)) for m in ("want", "A", "E", "n") + (("W", "J") if ext else ())}
    wh = weight_hook if weight_hook is not None else (lambda aw: aw)
    for l in range(L):
        t = level_terms(value, shapes, lsi, loc, l, frac_hook, slack)
        for alt, u in enumerate([t] + t["alts"]):
            b, q, h, p, ok, v = u["b"], u["q"], u["h"], u["p"], u["ok"], u["v"]
            eps = u["eps"] if slack is not None else t["eps"]          # a scalar, or an (m, 1) column
            eps1 = eps[:, 0] if slack is not None else eps
            sub = (lambda e, m: e[m]) if slack is not None else (lambda e, m: e)
            dw = [d[b, q, h, l, p] for d in dws] if ext else None
            av = np.abs(v)
            qh = (b * Lq + q) * Hh + h
            a = [w[b, q, h, l, p] for w in weights]
            g = [ups[0][b, q, h]] + ([ups[1][b, q, p, h]] if instance else [])        # (m, C)
            outs = [(out, qh)] + ([(mask, ((b * Lq + q) * P + p) * Hh + h)] if instance else [])
            sum_av = av.sum(1)                                                          # (m, C)
            # |t_c| = sum over the upstream rows of |a g_c|: what a corner weight multiplies in grad_value / grad_loc
            abs_t = sum(np.abs(ai)[:, None] * np.abs(gi) for ai, gi in zip(a, g))
            for k in range(4):
                idx = ((b * S + int(lsi[l]) + u["rows"][:, k]) * Hh + h)[ok[:, k]]
                if alt:
                    gval.add(idx, E=sub(eps, ok[:, k]) * abs_t[ok[:, k]])
                    continue
                for j, (ai, gi) in enumerate(zip(a, g)):
                    aw = (ai * t["w"][:, k])[ok[:, k]]
                    gk = gi[ok[:, k]]
                    gval.add(idx, want=wh(aw)[:, None] * gk, A=np.abs(aw)[:, None] * np.abs(gk),
                             n=np.ones((idx.size, 1)), G=np.abs(gk))
                    if ext:
                        gval.add(idx, W=(dw[j][ok[:, k]] * np.abs(aw))[:, None] * np.abs(gk))
                gval.add(idx, E=sub(eps, ok[:, k]) * abs_t[ok[:, k]])
            for j, ((acc, idx), ai) in enumerate(zip(outs, a)):
                if alt:
                    acc.add(idx, E=eps * np.abs(ai)[:, None] * sum_av)
                    continue
                aw = ai[:, None] * t["w"]                                                # (m, 4)
                acc.add(idx, want=(wh(aw)[:, :, None] * v).sum(1), A=(np.abs(aw)[:, :, None] * av).sum(1),
                        E=eps * np.abs(ai)[:, None] * sum_av, n=ok.sum(1)[:, None].astype(np.float64), G=sum_av)
                if ext:
                    acc.add(idx, W=dw[j][:, None] * (np.abs(aw)[:, :, None] * av).sum(1))
            at = (b, q, h, l, p)
            for name, gi in zip(sorted(point, reverse=True) if instance else ["grad_attn"], g):   # spatial, then level
                d = point[name]
                d["E"][at] += eps1 * (np.abs(gi) * sum_av).sum(1)
                if alt:
                    continue
                d["want"][at] = (gi * (t["w"][:, :, None] * v).sum(1)).sum(1)
                d["A"][at] = (np.abs(gi) * (t["w"][:, :, None] * av).sum(1)).sum(1)
                d["n"][at] = C * ok.sum(1)
            if alt:
                continue                       # (such a point is within EDGE_PX of an edge: skipped in grad_loc, or given J)
            tt = sum(ai[:, None] * gi for ai, gi in zip(a, g))                           # (m, C)
            fy, fx = t["fy"][:, None], t["fx"][:, None]
            dxv = (1 - fy) * (v[:, 1] - v[:, 0]) + fy * (v[:, 3] - v[:, 2])
            dyv = (1 - fx) * (v[:, 2] - v[:, 0]) + fx * (v[:, 3] - v[:, 1])
            dxa = (1 - fy) * (av[:, 1] + av[:, 0]) + fy * (av[:, 3] + av[:, 2])
            dya = (1 - fx) * (av[:, 2] + av[:, 0]) + fx * (av[:, 3] + av[:, 1])
            for j, (size, dv, da) in enumerate(((t["Wl"], dxv, dxa), (t["Hl"], dyv, dya))):
                gloc["want"][at + (j,)] = size * (tt * dv).sum(1)
                gloc["A"][at + (j,)] = size * (abs_t * da).sum(1)
                gloc["E"][at + (j,)] = size * eps1 * (abs_t * sum_av).sum(1)
                gloc["n"][at + (j,)] = C * ok.sum(1) * len(a)
                if ext:
                    dw_t = sum((di * np.abs(ai))[:, None] * np.abs(gi) for di, ai, gi in zip(dw, a, g))
                    gloc["W"][at + (j,)] = size * (dw_t * da).sum(1)
        if ext:
            _edge_jumps(gloc, value, shapes, lsi, loc, l, weights, ups, instance, slack)
    if ext:
        gloc["E"] += gloc["J"]
        gloc["edge_share"] = float(gloc.pop("near").any(-1).mean())
    else:
        edge = on_edge(loc, shapes)
        gloc["skip"] = np.broadcast_to(edge, gloc["want"].shape)
        gloc["edge_share"] = float(edge.mean())
    ref = {"out": out.result(), "grad_value": gval.result(), "grad_loc": gloc}
    ref["out"] = {k: a.reshape(B, Lq, Hh * C) for k, a in ref["out"].items()}
    if instance:
        ref["mask_out"] = {k: a.reshape(B, Lq, P, Hh * C) for k, a in mask.result().items()}
    ref.update(point)
    return ref


def box_reference(value, shapes, lsi, loc, attn, grad_out, **hooks):
    """Stored inputs (float64 numpy or tensors): value (B, S, H, C), loc (B, Lq, H, L, P, 2), attn (B, Lq, H, L, P),
    grad_out (B, Lq, H * C) -> {out, grad_value, grad_loc, grad_attn}."""
    value, loc, attn, grad_out = (f64(a) for a in (value, loc, attn, grad_out))
    B, S, Hh, C = value.shape
    Lq = loc.shape[1]
    return _reference(value, f64(shapes).astype(np.int64), f64(lsi).astype(np.int64), loc,
                      [attn.reshape(loc.shape[:5])], [grad_out.reshape(B, Lq, Hh, C)], False, **hooks)


def instance_reference(value, shapes, lsi, loc, spatial_w, level_w, grad_out, grad_mask, **hooks):
    """As box_reference with the two weight sets (B, Lq, H, L, P) and grad_mask (B, Lq, P, H * C) -> {out, mask_out,
    grad_value, grad_loc, grad_spatial, grad_level}: out sums a_s val, mask_out[p] sums a_l val over the levels, the
    upstream row of a point is a_s grad_out + a_l grad_mask[p] (two terms a corner in grad_value)."""
    value, loc, spatial_w, level_w, grad_out, grad_mask = (f64(a) for a in (value, loc, spatial_w, level_w, grad_out,
                                                                            grad_mask))
    B, S, Hh, C = value.shape
    Lq, P = loc.shape[1], loc.shape[4]
    return _reference(value, f64(shapes).astype(np.int64), f64(lsi).astype(np.int64), loc,
                      [spatial_w.reshape(loc.shape[:5]), level_w.reshape(loc.shape[:5])],
                      [grad_out.reshape(B, Lq, Hh, C), grad_mask.reshape(B, Lq, P, Hh, C)], True, **hooks)


# ------------------------------------------------------------------ the bound
def half_ulp(x, store):
    """The largest error of one RNE rounding of a number of magnitude <= x to the stored type: half the spacing of the
    type at x, 2^(max(floor(log2 x), emin) - p).  Never above u x + t of STORE (equal to u x at a power of two, half of it
    just below the next one; equal to t in f16's subnormal range)."""
    p, emin = FORMAT[store_name(store)]
    with np.errstate(divide="ignore"):
        e = np.maximum(np.floor(np.log2(x)), emin)
    return np.exp2(e - p)


def bound(ref, store, split="none"):
    """The bound of the module docstring with its store term u (|want| + R) + t taken exactly: the value before the one
    rounding is within R of want, so at most |want| + R in magnitude, and RNE moves it by at most half_ulp of that."""
    R = ((ref["n"] + 8.0) * 2.0 ** -24 + SPLIT[split]) * ref["A"] + ref["E"]
    if split == "f16":
        R = R + 2.0 ** -25 * ref["G"]
    if "W" in ref:                                     # the weights' own allowance (boxes_reference): sum of dw |term|
        R = R + ref["W"]
    return np.where(ref["A"] + ref["E"] > 0, half_ulp(np.abs(ref["want"]) + R, store) + R, 0.0)


def ratio(got, ref, store, split="none"):
    """-> (err / bound per element -- 0 where both are 0, inf where only the bound is --, err, bound)."""
    got = f64(got).reshape(ref["want"].shape)
    bnd = bound(ref, store, split)
    err = np.abs(got - ref["want"])
    err = np.where(np.isfinite(got), err, np.inf)
    if "skip" in ref:
        err = np.where(ref["skip"], 0.0, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    return r, err, bnd


def hold(got, ref, store, split, what):
    """Assert the bound for every element; -> the worst err / bound."""
    r, err, bnd = ratio(got, ref, store, split)
    if not r.size:
        return 0.0
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    worst = float(r[at])
    if not worst <= 1.0:
        g = f64(got).reshape(r.shape)
        bad = int((r > 1.0).sum())
        raise AssertionError("%s (%s, split %s): %d of %d elements outside the bound; worst at %s: got %.9g, want %.9g, "
                             "bound %.3e, err / bound %.3g (n = %d)" % (what, store_name(store), split, bad, r.size,
                                                                        tuple(int(i) for i in at), g[at],
                                                                        ref["want"][at], bnd[at], worst, ref["n"][at]))
    return worst


def hold_all(got, refs, dtype, split="none", what="", splits=None, table=None):
    """got: {output name: tensor}; outputs of the stored type are out / mask_out / grad_value, the rest float32.
    ``split`` applies to grad_value, ``splits`` overrides per output.  -> {name: worst err / bound}; appended to the
    list ``table`` as (what, stored type, name, worst)."""
    res = {}
    for name, t in got.items():
        ref = refs[name]
        if name == "grad_loc":
            assert ref["edge_share"] <= EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (what, 100 * ref["edge_share"])
        store = store_name(dtype) if name in ("out", "mask_out", "grad_value") else "float32"
        s = (splits or {}).get(name, split if name == "grad_value" else "none")
        res[name] = hold(t, ref, store, s, "%s: %s" % (what, name))
        if table is not None:
            table.append((what, store_name(dtype), name, res[name]))
    print("%s [%s]: worst err / bound %s" % (what, store_name(dtype),
                                             ", ".join("%s %.3f" % kv for kv in res.items())))
    return res


# ------------------------------------------------------------------ inputs, generated on the CPU (the same on every machine)
def make(levels, lq, family="model", dtype=torch.bfloat16, B=2, H=2, C=32, seed=0, kind="box", P=4):
    """bench.make_inputs for an ad-hoc shape on the CPU (tests/point_cases.make); family "border": uniform
    locations in [-0.2, 1.2] (tests/point_cases.make_dense_case)."""
    import bench
    name = "_error_bounds_test"
    bench.WORKLOADS[name] = (list(levels), lq, P, kind)
    old = bench.H_HEADS, bench.C_HEAD
    bench.H_HEADS, bench.C_HEAD = H, C
    try:
        inp = bench.make_inputs(name, dtype, "cpu", family="test" if family == "border" else family, batch=B, seed=seed)
    finally:
        bench.H_HEADS, bench.C_HEAD = old
        del bench.WORKLOADS[name]
    if family == "border":
        g = torch.Generator().manual_seed(seed + 100)
        inp["loc"] = (torch.rand(inp["loc"].shape, generator=g) * 1.4 - 0.2).contiguous()
    return inp


def reference_of(inp):
    """The reference of an input dictionary (bench.make_inputs' keys; tensors or numpy; box or instance), computed once."""
    if "_ref" not in inp:
        if inp["kind"] == "instance":
            inp["_ref"] = instance_reference(inp["value"], inp["shapes"], inp["lsi"], inp["loc"], inp["attn"],
                                             inp["level_w"], inp["grad_out"], inp["grad_mask"])
        else:
            inp["_ref"] = box_reference(inp["value"], inp["shapes"], inp["lsi"], inp["loc"], inp["attn"],
                                        inp["grad_out"])
    return inp["_ref"]


def numpy_inputs(inp):
    """A bench.make_inputs dictionary as the float64 / int64 numpy arrays the C oracle takes."""
    d = {k: f64(inp[k]) for k in ("value", "loc", "attn", "grad_out")}
    d["shapes"], d["lsi"] = inp["shapes"].cpu().numpy(), inp["lsi"].cpu().numpy()
    if inp["kind"] == "instance":
        d["spatial_w"], d["level_w"], d["grad_mask"] = d["attn"], f64(inp["level_w"]), f64(inp["grad_mask"])
    return d


# ------------------------------------------------------------------ from boxes and logits (see "From boxes" in the module docstring)
U32 = 2.0 ** -24                 # one float32 rounding, relative
SINCOS_ABS = 2.0 ** -22          # the device sincosf: an allowance of 4 ulp at 1.0, absolute (not a measurement)
LOG2E = 1.4426950408889634
EXP_MIN = -87.0                  # z - max below this: exp leaves float32's normal range, a relative dw means nothing


def grid_reference(ref, off, kidx, vr, angle_mode):
    """The modules' _where_to_attend after the offset projection, float64.  ref (B, Lq, D) or (B, Lq, H, D), off
    (B, Lq, H, L, V), kidx (P, 2), vr (B, 1, 1, L, 1, 2) or None; angle_mode 0: no rotation, 1: theta = (ref[4] +
    off[4] / 16) 2 pi, 2: theta = ref[4].  -> loc (B, Lq, H, L, P, 2), dloc (the same shape, normalised units)."""
    ref, off, kidx = f64(ref), f64(off), f64(kidx)
    lead = off.shape[:4]
    r = ref[:, :, None, None] if ref.ndim == 3 else ref[:, :, :, None]                 # (B, Lq, 1 | H, 1, D)
    col = lambda j: np.broadcast_to(r[..., j], lead)
    centre = [col(j) + off[..., j] / 8 * col(2 + j) for j in (0, 1)]
    size = [col(2 + j) + off[..., 2 + j] / 8 * col(2 + j) for j in (0, 1)]
    local = [kidx[:, j] * np.maximum(size[j], 0.0)[..., None] for j in (0, 1)]           # (B, Lq, H, L, P)
    # the absolute values of the terms the roundings act on, per axis
    t_centre = [np.abs(col(j)) + np.abs(off[..., j] / 8 * col(2 + j)) for j in (0, 1)]
    t_local = [np.abs(kidx[:, j]) * ((np.abs(col(2 + j)) + np.abs(off[..., 2 + j] / 8 * col(2 + j)))
                                     * (size[j] > 0))[..., None] for j in (0, 1)]
    if angle_mode:
        if angle_mode == 1:
            theta = (col(4) + off[..., 4] / 16) * 2 * np.pi
            # the sum ref[4] + off[4] / 16, the product with float32's 2 pi, that constant itself: 3 roundings
            dtheta = 3 * U32 * (np.abs(col(4)) + np.abs(off[..., 4] / 16)) * 2 * np.pi
        else:
            theta, dtheta = col(4), np.zeros(lead)
        cs, sn = np.cos(theta)[..., None], np.sin(theta)[..., None]
        rot = [local[0] * cs - local[1] * sn, local[0] * sn + local[1] * cs]
        dsc = (dtheta + SINCOS_ABS)[..., None] * (np.abs(local[0]) + np.abs(local[1]))
        # product, sum (centre); product, sum, product (size, local) on either axis; two products, the difference, the sum
        terms = [t_centre[j][..., None] + t_local[0] + t_local[1] for j in (0, 1)]
        n, local = 9, rot
    else:
        dsc = 0.0
        terms = [t_centre[j][..., None] + t_local[j] for j in (0, 1)]
        n = 6                     # product, sum (centre); product, sum (size); kidx relu(size); the sum
    loc = np.stack([centre[j][..., None] + local[j] for j in (0, 1)], -1)
    dloc = np.stack([n * U32 * terms[j] + dsc for j in (0, 1)], -1)
    if vr is not None:
        v = np.abs(f64(vr))
        loc, dloc = loc * f64(vr), (dloc + U32 * np.stack(terms, -1)) * v                # one more rounding
    return loc, dloc


def _softmax(z, axes, count, more=0):
    """float64 softmax of ``z`` over ``axes`` and its relative allowance (``count`` terms in the sum, ``more`` further
    roundings of the result)."""
    d = z - z.max(axes, keepdims=True)
    assert d.min() >= EXP_MIN, "a logit %.1f below its row's maximum" % -d.min()
    e = np.exp(d)
    a = e / e.sum(axes, keepdims=True)
    de = (3.0 * np.abs(d) + 2.0) * U32                      # the exponent's three roundings, the instruction's ulp
    dw = de + (a * de).sum(axes, keepdims=True) + (count - 1 + 1 + 1 + more) * U32      # sum, reciprocal, product
    return a, np.broadcast_to(dw, a.shape)


def softmax_reference(logits):
    """logits (..., N) -> (softmax over the last axis in float64, dw)."""
    z = f64(logits)
    return _softmax(z, (-1,), z.shape[-1])


def cell_weights_reference(logits):
    """logits (B, Lq, H, L, 2, 2) -> a (softmax over the row's 4 L cells), da, t (softmax over the levels), dt."""
    z = f64(logits)
    L = z.shape[3]
    a, da = _softmax(z, (-1, -2, -3), 4 * L, more=2)       # ... / m^2: the constant and the product
    t, dt = _softmax(z, (-3,), L)
    return a, da, t, dt


def _expand(cells, k):
    """(B, Lq, H, L, 2, 2) -> (B, Lq, H, L, k * k): repeat_interleave by k / 2 along both axes, row-major (y, x)."""
    m = k // 2
    return np.repeat(np.repeat(cells, m, -2), m, -1).reshape(cells.shape[:4] + (k * k,))


def instance_weights_reference(logits, k, need_level=True):
    """The spatial weights -- softmax over all L k k repeated logits = a[cell] / m^2 -- and, with need_level, the level
    weights t[cell], (B, Lq, H, L, k * k) each, float64 -> (spatial, level | None, dw_spatial, dw_level | None)."""
    a, da, t, dt = cell_weights_reference(logits)
    m = k // 2
    sw, dsw = _expand(a / (m * m), k), _expand(da, k)
    return (sw, _expand(t, k), dsw, _expand(dt, k)) if need_level else (sw, None, dsw, None)


def _reduce_boxes(r, names, ref, off, kidx, vr, logits, k):
    """The per-point planes of ``_reference`` -> grad_offsets (B, Lq, H, L, 4), grad_ref_rows (B, Lq, H, L, 5),
    grad_logits (B, Lq, H, L, 2, 2), angle mode 0.  want reduces in float64; A, E (with W and the edge jumps) and J with
    the absolute values of the same coefficients; n is the largest n of the points plus the reduction's own roundings.
    grad_offsets also gets ``unmasked``: its exact value with relu' left out (a mutation, for the tests of the bound)."""
    ref, off, kidx = f64(ref), f64(off), f64(kidx)
    lead = off.shape[:4]
    P = kidx.shape[0]
    rr = ref[:, :, None, None] if ref.ndim == 3 else ref[:, :, :, None]
    col = lambda j: np.broadcast_to(rr[..., j], lead)
    g = r["grad_loc"]
    scale = f64(vr) if vr is not None else 1.0                       # d / d (unscaled grid)
    pl = {"want": g["want"] * scale, "A": g["A"] * np.abs(scale), "E": (g["E"] + g["W"]) * np.abs(scale),
          "J": g["J"] * np.abs(scale)}
    n_out = g["n"].max((-1, -2)) + P + 6             # the vr product, kidx product, P-term sum, and the row's few
    goff = {m: np.zeros(lead + (4,)) for m in ("want", "A", "E", "J", "n", "unmasked")}
    rows = {m: np.zeros(lead + (5,)) for m in ("want", "A", "E", "J", "n")}
    for j in (0, 1):
        sz = col(2 + j) + off[..., 2 + j] / 8 * col(2 + j)
        dsz = 2 * U32 * (np.abs(col(2 + j)) + np.abs(off[..., 2 + j] / 8 * col(2 + j)))
        pos = sz > 0
        unsure = (np.abs(sz) <= dsz) & (sz != 0)     # the sign of a float32 size may differ: either relu' is legitimate
        for m, p in pl.items():
            kj = kidx[:, j] if m == "want" else np.abs(kidx[:, j])
            ab = (lambda x: x) if m == "want" else np.abs
            s_c, s_k = p[..., j].sum(-1), (kj * p[..., j]).sum(-1)
            goff[m][..., j] = s_c * ab(col(2 + j)) / 8
            goff[m][..., 2 + j] = pos * s_k * ab(col(2 + j)) / 8
            if m == "want":
                goff["unmasked"][..., j], goff["unmasked"][..., 2 + j] = goff[m][..., j], s_k * col(2 + j) / 8
            rows[m][..., j] = s_c
            rows[m][..., 2 + j] = s_c * ab(off[..., j] / 8) + pos * s_k * ab(1 + off[..., 2 + j] / 8)
            if m == "A":
                goff["E"][..., 2 + j] += unsure * s_k * np.abs(col(2 + j)) / 8
                rows["E"][..., 2 + j] += unsure * s_k * np.abs(1 + off[..., 2 + j] / 8)
    for d in (goff, rows):
        d["n"][...] = n_out[..., None]
    rows["n"][..., 4] = 0
    glog = _reduce_cells(r[names[0]], r[names[1]] if len(names) > 1 else None, logits, k)
    return {"grad_offsets": goff, "grad_ref_rows": rows, "grad_logits": glog}


def _reduce_cells(sp, lvp, logits, k):
    """The per-point planes want / A / E / n (B, Lq, H, L, k k) of grad_spatial (``sp``) and grad_level (``lvp``, or
    None) -> grad_logits (B, Lq, H, L, 2, 2): the Jacobians of the two softmaxes over the 2 x 2 logits (module
    docstring); a weight off by da adds (da + max da) times the A of its bracket to E; n: the points' largest plus
    m^2 + 4 L + 8."""
    lead = f64(logits).shape[:4]
    a, da, t, dt = cell_weights_reference(logits)
    m2 = (k // 2) ** 2
    L = a.shape[3]
    cells = lambda x: x.reshape(lead + (2, k // 2, 2, k // 2)).sum((-1, -3))
    row, lev = (-1, -2, -3), (-3,)
    glog = {}
    for m in ("want", "A", "E"):
        Gs = cells(sp[m])
        if m == "want":
            x = a / m2 * (Gs - (a * Gs).sum(row, keepdims=True))
        else:
            x = a / m2 * (Gs + (a * Gs).sum(row, keepdims=True))
        if m == "E":       # the weights' own allowance: a is within da of its value, every a of the row within the largest
            As = cells(sp["A"])
            x = x + (da + da.max(row, keepdims=True)) * a / m2 * (As + (a * As).sum(row, keepdims=True))
        if lvp is not None:
            Gt = cells(lvp[m])
            if m == "want":
                x = x + t * (Gt - (t * Gt).sum(lev, keepdims=True))
            else:
                x = x + t * (Gt + (t * Gt).sum(lev, keepdims=True))
            if m == "E":
                At = cells(lvp["A"])
                x = x + (dt + dt.max(lev, keepdims=True)) * t * (At + (t * At).sum(lev, keepdims=True))
        glog[m] = x
    n_pt = sp["n"].max(-1) if lvp is None else np.maximum(sp["n"].max(-1), lvp["n"].max(-1))
    glog["n"] = np.broadcast_to((n_pt + m2 + 4 * L + 8)[..., None, None], glog["want"].shape).copy()
    glog["J"] = np.zeros_like(glog["want"])
    return glog


def _reduce_grid(pl, n_pt, ref, off, kidx, vr, angle_mode, mutation=()):
    """Per-point planes of grad_loc -- ``pl`` = {want, A, E, J}, each (B, Lq, H, L, P, 2), E with the weights' W and
    the edge jumps J already in it -- and the points' term counts ``n_pt`` (the same shape, or 0) -> grad_offsets
    (B, Lq, H, L, V) and grad_ref_rows (B, Lq, H, L, 5) in the three angle modes, V = 4 or 5 (the box terms of the
    module docstring, "box kind").  ``mutation``: names of wrong formulas written into ``want`` only (the tests of the
    bound): "no_relu_grad", ("flip_sin_h", level), "no_relu_t", "no_sixteenth"."""
    ref, off, kidx = f64(ref), f64(off), f64(kidx)
    lead = off.shape[:4]
    P, V = kidx.shape[0], off.shape[-1]
    rr = ref[:, :, None, None] if ref.ndim == 3 else ref[:, :, :, None]
    col = lambda j: np.broadcast_to(rr[..., j], lead)
    mut = {m if isinstance(m, str) else m[0]: m for m in mutation}
    size = [col(2 + j) + off[..., 2 + j] / 8 * col(2 + j) for j in (0, 1)]
    asz = [np.abs(col(2 + j)) + np.abs(off[..., 2 + j] / 8 * col(2 + j)) for j in (0, 1)]   # the difference as a sum
    pos = [s > 0 for s in size]
    # the sign of a float32 size may differ (two roundings of |asz|): either relu' is legitimate
    unsure = [(np.abs(s) <= 2 * U32 * a) & (s != 0) for s, a in zip(size, asz)]
    if angle_mode == 1:
        theta = (col(4) + off[..., 4] / 16) * 2 * np.pi
        dsc = 3 * U32 * (np.abs(col(4)) + np.abs(off[..., 4] / 16)) * 2 * np.pi + SINCOS_ABS     # dtheta + the allowance
    elif angle_mode == 2:
        theta, dsc = col(4), np.full(lead, SINCOS_ABS)
    else:
        theta, dsc = np.zeros(lead), np.zeros(lead)          # cos = 1 and sin = 0 are exact: no allowance
    cs, sn = np.cos(theta)[..., None], np.sin(theta)[..., None]
    acs, asn, dsc = np.abs(cs), np.abs(sn), dsc[..., None]
    kx, ky = kidx[:, 0], kidx[:, 1]
    akx, aky = np.abs(kx), np.abs(ky)
    scale = f64(vr) if vr is not None else np.ones(2)                 # d / d (unscaled grid)
    g = {m: [p[..., j] * (scale if m == "want" else np.abs(scale))[..., j] for j in (0, 1)] for m, p in pl.items()}
    # local coordinates: l = kidx relu(size); by absolute values with the size's difference as a sum, and where the
    # float32 size may be positive
    lx, ly = kx * np.maximum(size[0], 0.0)[..., None], ky * np.maximum(size[1], 0.0)[..., None]
    alx, aly = akx * (asz[0] * (pos[0] | unsure[0]))[..., None], aky * (asz[1] * (pos[1] | unsure[1]))[..., None]
    term = {}                                                         # name -> (a_cx, a_cy, a_w, a_h, a_t), (B, Lq, H, L)
    for m, (gx, gy) in g.items():
        if m == "want":
            sh = sn
            if "flip_sin_h" in mut:
                sh = np.broadcast_to(sn, lead + (1,)).copy()
                sh[:, :, :, mut["flip_sin_h"][1]] *= -1.0
            tx, ty = (kx * size[0][..., None], ky * size[1][..., None]) if "no_relu_t" in mut else (lx, ly)
            a_w = (kx * (gx * cs + gy * sn)).sum(-1)
            a_h = (ky * (gy * cs - gx * sh)).sum(-1)
            if "no_relu_grad" not in mut:
                a_w, a_h = pos[0] * a_w, pos[1] * a_h
            a_t = (gx * (-tx * sn - ty * cs) + gy * (tx * cs - ty * sn)).sum(-1)
        else:
            a_w = pos[0] * (akx * (gx * acs + gy * asn)).sum(-1)
            a_h = pos[1] * (aky * (gy * acs + gx * asn)).sum(-1)
            a_t = (gx * (alx * asn + aly * acs) + gy * (alx * acs + aly * asn)).sum(-1)
        term[m] = [gx.sum(-1), gy.sum(-1), a_w, a_h, a_t]
    # E: the float32 sine and cosine (each within dsc), and a relu' that may go either way
    gxa, gya = g["A"]
    mag = gxa + gya
    term["E"][2] = term["E"][2] + pos[0] * (dsc * akx * mag).sum(-1) + unsure[0] * (akx * (gxa * acs + gya * asn)).sum(-1)
    term["E"][3] = term["E"][3] + pos[1] * (dsc * aky * mag).sum(-1) + unsure[1] * (aky * (gya * acs + gxa * asn)).sum(-1)
    term["E"][4] = term["E"][4] + (dsc * (alx + aly) * mag).sum(-1)
    goff = {m: np.zeros(lead + (V,)) for m in ("want", "A", "E", "J", "n")}
    rows = {m: np.zeros(lead + (5,)) for m in ("want", "A", "E", "J", "n")}
    two_pi = 2 * np.pi
    for m, (a_cx, a_cy, a_w, a_h, a_t) in term.items():
        ab = (lambda x: x) if m == "want" else np.abs
        rw, rh = ab(col(2)), ab(col(3))
        goff[m][..., 0], goff[m][..., 1] = a_cx * rw / 8, a_cy * rh / 8
        goff[m][..., 2], goff[m][..., 3] = a_w * rw / 8, a_h * rh / 8
        if V == 5 and angle_mode == 1:
            goff[m][..., 4] = a_t * two_pi if (m == "want" and "no_sixteenth" in mut) else a_t * two_pi / 16
        rows[m][..., 0], rows[m][..., 1] = a_cx, a_cy
        rows[m][..., 2] = a_cx * ab(off[..., 0] / 8) + a_w * ab(1 + off[..., 2] / 8)
        rows[m][..., 3] = a_cy * ab(off[..., 1] / 8) + a_h * ab(1 + off[..., 3] / 8)
        if angle_mode:
            rows[m][..., 4] = a_t * two_pi if angle_mode == 1 else a_t
    n_max = np.max(n_pt, axis=(-1, -2)) if np.ndim(n_pt) else np.full(lead, float(n_pt))
    for d in (goff, rows):
        d["n"][...] = (n_max + P + (8 if angle_mode else 6))[..., None]
        if angle_mode:
            d["n"][..., 4:] = (n_max + P + 10)[..., None]
    if not angle_mode:
        rows["n"][..., 4] = 0
        goff["n"][..., 4:] = 0
    return {"grad_offsets": goff, "grad_ref_rows": rows}


def _reduce_logits(gp, n_pt, a, da, mutation=()):
    """Per-point planes want / A / E (..., N) of the weights' gradient Gw, their term counts ``n_pt`` (the same shape,
    or 0), the row's softmax ``a`` and its relative allowance ``da`` -> grad_logits (..., N) = a (Gw - sum a Gw).
    ``mutation`` (into ``want`` only): ("dot_first", m): the sum over the first m entries only; "drop_lowest": the
    lowest-weight point's Gw left out."""
    mut = {m if isinstance(m, str) else m[0]: m for m in mutation}
    N = a.shape[-1]
    Gw = gp["want"]
    if "drop_lowest" in mut:
        Gw = Gw.copy()
        np.put_along_axis(Gw, np.argmin(a, -1)[..., None], 0.0, -1)
    m = mut["dot_first"][1] if "dot_first" in mut else N
    res = {"want": a * (Gw - (a * Gw)[..., :m].sum(-1, keepdims=True))}
    bracket = lambda x: x + (a * x).sum(-1, keepdims=True)
    res["A"] = a * bracket(gp["A"])
    res["E"] = a * bracket(gp["E"]) + (da + da.max(-1, keepdims=True)) * a * bracket(gp["A"])
    n_max = np.max(n_pt, axis=-1, keepdims=True) if np.ndim(n_pt) else float(n_pt)
    res["n"] = np.broadcast_to(n_max + N + 3, a.shape).astype(np.float64)
    res["J"] = np.zeros_like(res["want"])
    return res


def box_gradients(points, ref, off, kidx, vr, angle_mode, mutation=()):
    """The three gradients of the box kind from the per-point planes boxes_reference keeps under "points" (so that a
    mutation costs the reductions only)."""
    res = _reduce_grid(points["loc"], points["n_loc"], ref, off, kidx, vr, angle_mode, mutation)
    res["grad_logits"] = _reduce_logits(points["attn"], points["attn"]["n"], points["a"], points["da"], mutation)
    return res


def grid_backward_reference(ref, off, kidx, vr, angle_mode, grad_grid):
    """ops.box_grid_backward on its own: ``grad_grid`` (B, Lq, H, L, P, 2) float32 is an exact input (want = g,
    A = |g|, E = 0, no terms of its own), so what remains is the reduction's roundings and the rotation allowance."""
    g = f64(grad_grid)
    zero = np.zeros_like(g)
    return _reduce_grid({"want": g, "A": np.abs(g), "E": zero, "J": zero}, 0, ref, off, kidx, vr, angle_mode)


def softmax_backward_reference(attn, grad_attn):
    """ops.softmax_backward on its own: float32 ``attn`` and ``grad_attn`` (..., N) are exact inputs."""
    a, g = f64(attn), f64(grad_attn)
    zero = np.zeros_like(g)
    return _reduce_logits({"want": g, "A": np.abs(g), "E": zero}, 0, a, np.zeros_like(a))


def cell_logits_backward_reference(logits, k, grad_spatial, grad_level):
    """ops.instance_weights_backward on its own: float32 upstream gradients (B, Lq, H, L, k k) as exact inputs
    (either may be None: zeros); the weights are recomputed from the logits, so their da / dt stay."""
    shape = f64(logits).shape[:4] + (k * k,)

    def planes(g):
        g = np.zeros(shape) if g is None else f64(g).reshape(shape)
        return {"want": g, "A": np.abs(g), "E": np.zeros(shape), "n": np.zeros(shape)}
    return _reduce_cells(planes(grad_spatial), None if grad_level is None else planes(grad_level), logits, k)


def boxes_reference(kind, value, shapes, lsi, ref, off, kidx, vr, logits, angle_mode=0, k=None, grad_out=None,
                    grad_mask=None, loc=None, weights=None, mutation=()):
    """What the kernels that take boxes and logits must give, from their own inputs (float32 ref, off, kidx, vr,
    logits; ``value`` and the upstream gradients as stored).  kind "box": logits (B, Lq, H, L P) -> {out} and, with
    grad_out, {grad_offsets (.., L, V), grad_ref_rows (.., L, 5), grad_logits (.., L P)} in any angle mode (planes want / A
    / E / n / J), ``edge_share`` and ``points`` (what ``box_gradients`` reduces; ``mutation`` goes to it); kind
    "instance": logits (B, Lq, H, L, 2, 2), k -> {out, mask_out} and, with grad_out (grad_mask None: the mask output took
    no part), {grad_offsets, grad_ref_rows, grad_logits}.  ``loc`` / ``weights`` (a list) replace the model's own in
    ``want``: mutations, for the tests of the bound itself.  Also "grid" and
    "weights": (loc, dloc) and [(w, dw), ...] of the model."""
    value = f64(value)
    B, S, Hh, C = value.shape
    shapes, lsi = f64(shapes).astype(np.int64), f64(lsi).astype(np.int64)
    loc0, dloc = grid_reference(ref, off, kidx, vr, angle_mode)
    Lq, L, P = loc0.shape[1], loc0.shape[3], loc0.shape[4]
    if kind == "box":
        w, dw = softmax_reference(logits)
        ws, dws = [w.reshape(B, Lq, Hh, L, P)], [dw.reshape(B, Lq, Hh, L, P)]
    else:
        sw, lw, dsw, dlw = instance_weights_reference(logits, k, True)
        ws, dws = [sw, lw], [dsw, dlw]
    res = {"grid": (loc0, dloc), "weights": list(zip(ws, dws))}
    ws = ws if weights is None else [f64(w).reshape(B, Lq, Hh, L, P) for w in weights]
    loc = loc0 if loc is None else f64(loc)
    gout = np.zeros((B, Lq, Hh, C)) if grad_out is None else f64(grad_out).reshape(B, Lq, Hh, C)
    if kind == "box":
        r = _reference(value, shapes, lsi, loc, ws, [gout], False, slack=dloc, dws=dws)
        res["out"] = r["out"]
        if grad_out is not None:
            g = r["grad_loc"]
            res["points"] = dict(
                loc={"want": g["want"], "A": g["A"], "E": g["E"] + g["W"], "J": g["J"]}, n_loc=g["n"],
                attn={m: r["grad_attn"][m].reshape(B, Lq, Hh, L * P) for m in ("want", "A", "E", "n")},
                a=ws[0].reshape(B, Lq, Hh, L * P), da=dws[0].reshape(B, Lq, Hh, L * P))
            res.update(box_gradients(res["points"], ref, off, kidx, vr, angle_mode, mutation))
            res["edge_share"] = g["edge_share"]
        return res
    if grad_out is None or grad_mask is not None:
        gmask = np.zeros((B, Lq, P, Hh, C)) if grad_mask is None else f64(grad_mask).reshape(B, Lq, P, Hh, C)
        r = _reference(value, shapes, lsi, loc, ws, [gout, gmask], True, slack=dloc, dws=dws)
        res.update(out=r["out"], mask_out=r["mask_out"])
        names = ("grad_spatial", "grad_level")
    else:
        r = _reference(value, shapes, lsi, loc, ws[:1], [gout], False, slack=dloc, dws=dws[:1])
        res["out"] = r["out"]
        names = ("grad_attn",)
    if grad_out is not None:
        res.update(_reduce_boxes(r, names, ref, off, kidx, vr, logits, k))
        res["edge_share"] = r["grad_loc"]["edge_share"]
    return res


def edge_dominated(ref, store="float32"):
    """The share of an output's elements whose bound is more than half edge allowance (the J plane)."""
    bnd = bound(ref, store)
    return float((ref["J"] > 0.5 * bnd).mean()) if bnd.size else 0.0
