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
"""

import numpy as np
import torch

EDGE_PX = 1e-4          # grad_loc: points this close to a bilinear cell edge are left out (tests/test_gpu_parity.on_cell_edge)
EDGE_CAP = 2e-3         # ... and may be at most this share of a case's points (tests/test_gpu_boxes_backward.EDGE_CAP)

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

    def __init__(self, shape, with_g):
        self.shape = shape
        self.C = shape[-1]
        self.rows = int(np.prod(shape[:-1]))
        names = ("want", "A", "E", "n") + (("G",) if with_g else ())
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


def level_terms(value, shapes, lsi, loc, l, frac_hook=None):
    """The sample points of level ``l`` that pass the window test (-1, H) x (-1, W) (a coordinate of exactly -1 is
    outside, as in the reference kernels): dict of b, q, h, p (m,), rows / ok (m, 4), w (m, 4) bilinear weights,
    v (m, 4, C) corner rows (zeros outside the map), fy, fx, eps.  Also ``alts``: the (point, cell) pairs float32 could
    take instead (see the module docstring), each b, q, h, p, rows, ok, v."""
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
        return dict(b=b[sel], q=q[sel], h=h[sel], p=p[sel], rows=rows, ok=ok, v=v)

    inside = (y > -1) & (x > -1) & (y < Hl) & (x < Wl)
    sel = np.nonzero(inside)[0]
    y0, x0 = np.floor(y[sel]).astype(np.int64), np.floor(x[sel]).astype(np.int64)
    fy, fx = y[sel] - y0, x[sel] - x0
    if frac_hook is not None:
        fy, fx = frac_hook(l, sel, fy, fx)
    t = gather(sel, y0, x0)
    t.update(fy=fy, fx=fx, w=np.stack([(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx], 1),
             eps=3.0 * (Wl + Hl) * 2.0 ** -24, Hl=Hl, Wl=Wl, sel=sel)
    # what float32 may do instead: both coordinates moved by +- 3 size 2^-24
    dx, dy = 3.0 * Wl * 2.0 ** -24, 3.0 * Hl * 2.0 ** -24
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


def _reference(value, shapes, lsi, loc, weights, ups, instance, frac_hook=None, weight_hook=None):
    """weights: [attn] or [spatial_w, level_w], (B, Lq, H, L, P); ups: [grad_out (B, Lq, H, C)] or that and grad_mask
    (B, Lq, P, H, C).  The hooks mutate what goes into ``want`` only (tests of the bound itself): frac_hook(l, sel, fy,
    fx) -> fy, fx; weight_hook(a w_k) -> the weight products the sums of out / mask_out / grad_value use."""
    B, S, Hh, C = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    out = _Acc((B, Lq, Hh, C), True)
    mask = _Acc((B, Lq, P, Hh, C), True) if instance else None
    gval = _Acc((B, S, Hh, C), True)
    point = {k: {m: np.zeros((B, Lq, Hh, L, P)) for m in ("want", "A", "E", "n")}
             for k in (("grad_spatial", "grad_level") if instance else ("grad_attn",))}
    gloc = {m: np.zeros((B, Lq, Hh, L, P, 2)) for m in ("want", "A", "E", "n")}
    wh = weight_hook if weight_hook is not None else (lambda aw: aw)
    for l in range(L):
        t = level_terms(value, shapes, lsi, loc, l, frac_hook)
        for alt, u in enumerate([t] + t["alts"]):
            b, q, h, p, ok, v = u["b"], u["q"], u["h"], u["p"], u["ok"], u["v"]
            eps = t["eps"]
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
                    gval.add(idx, E=eps * abs_t[ok[:, k]])
                    continue
                for ai, gi in zip(a, g):
                    aw = (ai * t["w"][:, k])[ok[:, k]]
                    gk = gi[ok[:, k]]
                    gval.add(idx, want=wh(aw)[:, None] * gk, A=np.abs(aw)[:, None] * np.abs(gk),
                             n=np.ones((idx.size, 1)), G=np.abs(gk))
                gval.add(idx, E=eps * abs_t[ok[:, k]])
            for (acc, idx), ai in zip(outs, a):
                if alt:
                    acc.add(idx, E=eps * np.abs(ai)[:, None] * sum_av)
                    continue
                aw = ai[:, None] * t["w"]                                                # (m, 4)
                acc.add(idx, want=(wh(aw)[:, :, None] * v).sum(1), A=(np.abs(aw)[:, :, None] * av).sum(1),
                        E=eps * np.abs(ai)[:, None] * sum_av, n=ok.sum(1)[:, None].astype(np.float64), G=sum_av)
            at = (b, q, h, l, p)
            for name, gi in zip(sorted(point, reverse=True) if instance else ["grad_attn"], g):   # spatial, then level
                d = point[name]
                d["E"][at] += eps * (np.abs(gi) * sum_av).sum(1)
                if alt:
                    continue
                d["want"][at] = (gi * (t["w"][:, :, None] * v).sum(1)).sum(1)
                d["A"][at] = (np.abs(gi) * (t["w"][:, :, None] * av).sum(1)).sum(1)
                d["n"][at] = C * ok.sum(1)
            if alt:
                continue                       # (such a point is within EDGE_PX of an edge: skipped in grad_loc)
            tt = sum(ai[:, None] * gi for ai, gi in zip(a, g))                           # (m, C)
            fy, fx = t["fy"][:, None], t["fx"][:, None]
            dxv = (1 - fy) * (v[:, 1] - v[:, 0]) + fy * (v[:, 3] - v[:, 2])
            dyv = (1 - fx) * (v[:, 2] - v[:, 0]) + fx * (v[:, 3] - v[:, 1])
            dxa = (1 - fy) * (av[:, 1] + av[:, 0]) + fy * (av[:, 3] + av[:, 2])
            dya = (1 - fx) * (av[:, 2] + av[:, 0]) + fx * (av[:, 3] + av[:, 1])
            for j, (size, dv, da) in enumerate(((t["Wl"], dxv, dxa), (t["Hl"], dyv, dya))):
                gloc["want"][at + (j,)] = size * (tt * dv).sum(1)
                gloc["A"][at + (j,)] = size * (abs_t * da).sum(1)
                gloc["E"][at + (j,)] = size * eps * (abs_t * sum_av).sum(1)
                gloc["n"][at + (j,)] = C * ok.sum(1) * len(a)
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
    """bench.make_inputs for an ad-hoc shape on the CPU (tests/test_gpu_group_records.make); family "border": uniform
    locations in [-0.2, 1.2] (tests/test_gpu_dense.make_case)."""
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
