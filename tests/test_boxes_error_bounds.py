"""CPU: the float64 model from boxes and logits of tests/error_bounds.py (grid_reference, softmax_reference,
instance_weights_reference, boxes_reference) and the inputs of tests/test_gpu_boxes_error_bounds.py.

  * the float64 grid agrees with the float64 torch restatement of the reference's _where_to_attend to 1e-12;
  * a float32 numpy evaluation in the documented operation order stays within dloc / dw at every point of every case
    -- the angles of 23 and 77 / 16 turns and the windows far outside the map included;
  * the whole chain in float32 on the CPU -- float32 grid and weights, the C oracle's float32 build, float32
    reductions -- stays within the bound for every case (its worst err / bound is printed per output);
  * five mutations fail the bound where today's one-scale ``check`` at today's tolerances passes; a sixth (the softmax
    maximum over the first tile only) fails ``dw`` and, a softmax being shift invariant, stays inside the bound on ``out``;
  * every input keeps the cell-edge condition, and every geometry has elements that must be exactly zero.
"""
import itertools
import math

import numpy as np
import pytest
import torch

import error_bounds as eb
import test_gpu_boxes_error_bounds as gpu_cases
from oracle import boxattn_oracle as oc
from test_gpu_parity import _torch_grid
from test_gpu_wide_box_forward import check

F = np.float32
BOX_CASES = list(itertools.product(gpu_cases.BOX_GEOMETRIES, gpu_cases.CHANNELS, gpu_cases.box_cases.FLAVOURS))
INST_GEOMETRIES = sorted(gpu_cases.inst_cases.GEOMETRY)
KERNEL_SIZES = gpu_cases.inst_cases.KERNEL_SIZES


# ------------------------------------------------------------------ float32 numpy, operation by operation
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
    assert grid.dtype == F
    return grid * vr if vr is not None else grid


def softmax_f32(z, axes=(-1,), first=None):
    """exp(z - max) as exp2((z - max) log2 e), times the reciprocal of the float32 sum.  ``first``: the maximum over the
    first ``first`` logits of the last axis only (a mutation)."""
    z = np.asarray(z, dtype=F)
    m = z.max(axes, keepdims=True) if first is None else z[..., :first].max(-1, keepdims=True)
    e = np.exp2((z - m) * F(eb.LOG2E))
    a = e * (F(1) / e.sum(axes, keepdims=True, dtype=F))
    assert a.dtype == F
    return a


def instance_weights_f32(logits, k):
    m = k // 2
    a = softmax_f32(logits, (-1, -2, -3)) * F(1.0 / (m * m))
    t = softmax_f32(logits, (-3,))
    return eb._expand(a, k), eb._expand(t, k)


def reduce_f32(g, k, gloc, gs, gl):
    """The three gradients from float32 per-point gradients, float32 numpy: d grid / d box with relu' and the softmax
    Jacobians of the 2 x 2 logits, from their definitions."""
    ref, off, kidx, vr = g["ref"], g["off"], gpu_cases.kernel_offsets(k), g["vr"]
    lead = off.shape[:4]
    r = ref[:, :, None, None] if ref.ndim == 3 else ref[:, :, :, None]
    col = lambda j: np.broadcast_to(r[..., j], lead)
    gloc = gloc.astype(F) * vr if vr is not None else gloc.astype(F)
    goff, rows = np.zeros(lead + (4,), F), np.zeros(lead + (5,), F)
    for j in (0, 1):
        size = col(2 + j) + off[..., 2 + j] / F(8) * col(2 + j)
        s_c = gloc[..., j].sum(-1, dtype=F)
        s_k = np.where(size > 0, (kidx[:, j] * gloc[..., j]).sum(-1, dtype=F), F(0))
        goff[..., j] = s_c * col(2 + j) / F(8)
        goff[..., 2 + j] = s_k * col(2 + j) / F(8)
        rows[..., j] = s_c
        rows[..., 2 + j] = s_c * off[..., j] / F(8) + s_k * (F(1) + off[..., 2 + j] / F(8))
    m = k // 2
    z = g["logits"]
    cells = lambda x: x.astype(F).reshape(lead + (2, m, 2, m)).sum((-1, -3), dtype=F)
    a = softmax_f32(z, (-1, -2, -3))
    Gs = cells(gs)
    glog = a * F(1.0 / (m * m)) * (Gs - (a * Gs).sum((-1, -2, -3), keepdims=True, dtype=F))
    if gl is not None:
        t = softmax_f32(z, (-3,))
        Gt = cells(gl)
        glog = glog + t * (Gt - (t * Gt).sum(-3, keepdims=True, dtype=F))
    assert goff.dtype == rows.dtype == glog.dtype == F
    return goff, rows, glog


c32 = lambda a: np.ascontiguousarray(a, dtype=F)


# ------------------------------------------------------------------ the grid
@pytest.mark.parametrize("P", gpu_cases.GRID_POINTS)
def test_float64_grid_agrees_with_the_reference_module_in_double(P):
    for angle_mode, per_head, with_vr in gpu_cases.GRID_FLAVOURS:
        g = gpu_cases.grid_problem(P, angle_mode, per_head, with_vr)
        t = lambda a: None if a is None else torch.from_numpy(a).double()
        want = _torch_grid(t(g["ref"]), t(g["off"]), t(g["kidx"]), t(g["vr"]), angle_mode).numpy()
        loc, dloc = eb.grid_reference(g["ref"], g["off"], g["kidx"], g["vr"], angle_mode)
        assert loc.shape == want.shape == dloc.shape
        assert float(np.abs(loc - want).max()) <= 1e-12, (P, angle_mode, per_head, with_vr)


def grid_inputs():
    """(name, ref, off, kidx, vr, angle_mode) of every input of the GPU file."""
    for P, (angle_mode, per_head, with_vr) in itertools.product(gpu_cases.GRID_POINTS, gpu_cases.GRID_FLAVOURS):
        g = gpu_cases.grid_problem(P, angle_mode, per_head, with_vr)
        yield ("grid P=%d %s" % (P, (angle_mode, per_head, with_vr)), g["ref"], g["off"], g["kidx"], g["vr"], angle_mode)
    for geometry, C, flavour in BOX_CASES:
        g = gpu_cases.box_problem(geometry, C, flavour)
        k = int(round(g["dims"][6] ** 0.5))
        yield ("box %s C=%d %s" % (geometry, C, flavour), g["ref"], g["off"], gpu_cases.kernel_offsets(k), g["vr"],
               g["angle_mode"])
    for geometry, C, k, (per_head, with_vr) in itertools.product(INST_GEOMETRIES, gpu_cases.CHANNELS, KERNEL_SIZES,
                                                                 gpu_cases.INST_FLAVOURS):
        g = gpu_cases.inst_problem(geometry, C, k, per_head, with_vr)
        yield ("instance %s C=%d k=%d %s" % (geometry, C, k, (per_head, with_vr)), g["ref"], g["off"],
               gpu_cases.kernel_offsets(k), g["vr"], 0)


def test_float32_grid_stays_within_dloc_at_every_point_of_every_case():
    worst = {0: 0.0, 1: 0.0, 2: 0.0}
    turns = 0.0
    for name, ref, off, kidx, vr, angle_mode in grid_inputs():
        loc, dloc = eb.grid_reference(ref, off, kidx, vr, angle_mode)
        got = grid_f32(ref, off, kidx, vr, angle_mode)
        worst[angle_mode] = max(worst[angle_mode], gpu_cases.within(got, loc, dloc, name))
        if angle_mode:
            turns = max(turns, float(np.abs(ref[..., 4]).max()) / (1.0 if angle_mode == 1 else 2 * math.pi))
    assert turns >= 3.0, "no angle of several turns among the cases"
    print("float32 numpy grid, worst err / dloc: %s" % ", ".join("angle mode %d %.3f" % kv for kv in worst.items()))


def test_float32_weights_stay_within_dw():
    worst = {"softmax": 0.0, "spatial": 0.0, "level": 0.0}
    rows = [gpu_cases.softmax_rows(n) for n in (1, 4, 12, 18, 64)]
    rows += [gpu_cases.box_problem(*c)["logits"] for c in BOX_CASES]
    for z in rows:
        want, dw = eb.softmax_reference(z)
        worst["softmax"] = max(worst["softmax"], gpu_cases.within(softmax_f32(z), want, dw * want, "softmax"))
    cells = [(gpu_cases.cell_rows(L), k) for L in (1, 5, 16) for k in KERNEL_SIZES]
    cells += [(gpu_cases.inst_problem(geo, C, k, ph, vr)["logits"], k) for geo, C, k, (ph, vr) in
              itertools.product(INST_GEOMETRIES, gpu_cases.CHANNELS, KERNEL_SIZES, gpu_cases.INST_FLAVOURS)]
    for z, k in cells:
        sw, lw, dsw, dlw = eb.instance_weights_reference(z, k, True)
        got_s, got_l = instance_weights_f32(z, k)
        worst["spatial"] = max(worst["spatial"], gpu_cases.within(got_s, sw, dsw * sw, "spatial weights"))
        worst["level"] = max(worst["level"], gpu_cases.within(got_l, lw, dlw * lw, "level weights"))
    print("float32 numpy weights, worst err / dw: %s" % ", ".join("%s %.3f" % kv for kv in worst.items()))


def test_weights_of_a_row_sum_to_one_and_expand_row_major():
    z = gpu_cases.cell_rows(5)
    sw, lw, _, _ = eb.instance_weights_reference(z, 6, True)
    assert np.abs(sw.sum((-1, -2)) - 1).max() < 1e-14 and np.abs(lw.sum(-2) - 1).max() < 1e-14
    # point (y, x) of a 6 x 6 kernel lies in cell (y >= 3, x >= 3); the reference module repeats along both axes
    t = torch.from_numpy(z).double()
    rep = t.repeat_interleave(3, -1).repeat_interleave(3, -2)
    want = torch.softmax(rep.reshape(1, 8, 1, -1), -1).reshape(1, 8, 1, 5, 36).numpy()
    assert np.abs(sw - want).max() < 1e-15
    assert np.abs(lw - torch.softmax(rep, -3).reshape(1, 8, 1, 5, 36).numpy()).max() < 1e-15


# ------------------------------------------------------------------ the whole chain in float32 on the CPU
@pytest.mark.parametrize("geometry", gpu_cases.BOX_GEOMETRIES)
def test_box_chain_in_float32_is_within_the_bound(geometry):
    worst, zeros = 0.0, 0
    for C, flavour in itertools.product(gpu_cases.CHANNELS, gpu_cases.box_cases.FLAVOURS):
        g = gpu_cases.box_problem(geometry, C, flavour)
        B, S, H, _, L, Lq, P = g["dims"]
        ref = gpu_cases.box_reference(geometry, C, flavour)["out"]
        kidx = gpu_cases.kernel_offsets(int(round(P ** 0.5)))
        loc = grid_f32(g["ref"], g["off"], kidx, g["vr"], g["angle_mode"])
        attn = softmax_f32(g["logits"]).reshape(B, Lq, H, L, P)
        out = oc.box_attn_forward(c32(gpu_cases.every_type(g["value"])), g["shapes"], g["lsi"], c32(loc), c32(attn))
        worst = max(worst, eb.hold(out, ref, "float32", "none", "float32 chain: %s C=%d %s" % (geometry, C, flavour)))
        must = ((ref["A"] + ref["E"]) == 0).reshape(-1, C)          # a row: the C channels of a (query, head) pair
        zeros += int(must.all(-1).sum())
    assert zeros, "%s: no row of out that must be all zero" % geometry
    print("error-bound | float32 chain on the CPU, box from boxes: %s (%d must-be-zero rows) | float32 | out | %.3f"
          % (geometry, zeros, worst))


def inst_chain_f32(g, k, with_mask):
    B, S, H, C, L, Lq = g["dims"]
    P = k * k
    gout, gmask = gpu_cases.inst_upstream(g, k)
    loc = c32(grid_f32(g["ref"], g["off"], gpu_cases.kernel_offsets(k), g["vr"], 0))
    sw, lw = (c32(a) for a in instance_weights_f32(g["logits"], k))
    value = c32(gpu_cases.every_type(g["value"]))
    if with_mask:
        a = (value, g["shapes"], g["lsi"], loc, sw, lw)
        out, mask = oc.instance_attn_forward(*a)
        _, gloc, gs, gl = oc.instance_attn_backward(*a, c32(gout), c32(gmask))
        gl = np.asarray(gl).reshape(B, Lq, H, L, P)
    else:
        a = (value, g["shapes"], g["lsi"], loc, sw)
        out, mask, gl = oc.box_attn_forward(*a), None, None
        _, gloc, gs = oc.box_attn_backward(*a, c32(gout))
    grads = reduce_f32(g, k, np.asarray(gloc).reshape(loc.shape), np.asarray(gs).reshape(B, Lq, H, L, P), gl)
    res = dict(zip(gpu_cases.GRAD_NAMES, grads), out=out)
    if with_mask:
        res["mask_out"] = mask
    return res


@pytest.mark.parametrize("k", KERNEL_SIZES)
@pytest.mark.parametrize("geometry", INST_GEOMETRIES)
def test_instance_chain_in_float32_is_within_the_bound(geometry, k):
    """Also: every input keeps the cell-edge condition, and every case has an all-zero row of ``out`` and a
    ``grad_offsets`` size component that must be exactly zero."""
    worst, edge, zero_rows, zero_sizes = {}, {}, 0, 0
    for C, (per_head, with_vr), with_mask in itertools.product(gpu_cases.CHANNELS, gpu_cases.INST_FLAVOURS,
                                                              (True, False)):
        g = gpu_cases.inst_problem(geometry, C, k, per_head, with_vr)
        ref = gpu_cases.inst_reference(geometry, C, k, per_head, with_vr, with_mask)
        what = "float32 chain: %s C=%d k=%d per_head=%d vr=%d mask=%d" % (geometry, C, k, per_head, with_vr, with_mask)
        assert ref["edge_share"] <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (what,
                                                                                              100 * ref["edge_share"])
        for name, got in inst_chain_f32(g, k, with_mask).items():
            key = "%s%s" % (name, "" if with_mask or name == "out" else " (no grad_mask)")
            worst[key] = max(worst.get(key, 0.0), eb.hold(got, ref[name], "float32", "none", "%s: %s" % (what, name)))
            if name in gpu_cases.GRAD_NAMES:
                edge[key] = max(edge.get(key, 0.0), eb.edge_dominated(ref[name]))
        go = ref["grad_offsets"]
        zero_rows += int(((ref["out"]["A"] + ref["out"]["E"]) == 0).reshape(-1, C).all(-1).sum())
        zero_sizes += int((((go["A"] + go["E"]) == 0)[..., 2:4] & (go["unmasked"][..., 2:4] != 0)).sum())
    assert zero_rows, "%s k=%d: no row of out that must be all zero" % (geometry, k)
    assert zero_sizes, "%s k=%d: no collapsed box whose size gradient must be zero and is not without relu'" % (geometry, k)
    for name, w in worst.items():
        print("error-bound | float32 chain on the CPU, instance from boxes: %s k=%d | float32 | %s | %.3f"
              % (geometry, k, name, w))
    print("%s k=%d: share of elements whose bound is more than half edge allowance: %s"
          % (geometry, k, ", ".join("%s %.4f" % kv for kv in edge.items())))


def test_reductions_agree_with_those_of_the_gpu_tests_expectation():
    """reduce_grid / reduce_logits of tests/test_gpu_boxes_backward.py (restated from the kernels) on the reference's own
    per-point float64 gradients give the reference's three gradients."""
    import test_gpu_boxes_backward as bw
    k = 6
    g = gpu_cases.inst_problem("five_levels", 32, k, True, True)
    gout, gmask = gpu_cases.inst_upstream(g, k)
    kidx = gpu_cases.kernel_offsets(k)
    loc, dloc = eb.grid_reference(g["ref"], g["off"], kidx, g["vr"], 0)
    sw, lw, _, _ = eb.instance_weights_reference(g["logits"], k, True)
    pts = eb.instance_reference(gpu_cases.every_type(g["value"]), g["shapes"], g["lsi"], loc, sw, lw, gout, gmask)
    ref = gpu_cases.inst_reference("five_levels", 32, k, True, True, True)
    goff, rows = bw.reduce_grid(g["ref"], g["off"], kidx, g["vr"], pts["grad_loc"]["want"])
    glog = bw.reduce_logits(g["logits"], k, pts["grad_spatial"]["want"], pts["grad_level"]["want"])
    for name, got in zip(gpu_cases.GRAD_NAMES, (goff, rows, glog)):
        want = ref[name]["want"]
        assert float(np.abs(got - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max())), name


# ------------------------------------------------------------------ mutations: what the bound buys
STORES = {"float32": 1e-4, "bf16": 1e-2, "f16": 1e-2}        # today's tolerances (test_gpu_wide_box_forward.tol_of)


def passes_todays_check(got, want, tol):
    try:
        check(torch.from_numpy(np.ascontiguousarray(got)), want, tol, "mutation")
    except AssertionError:
        return False
    return True


def gap(mutant, ref, stores=STORES):
    """The storage types in which the mutant (its exact value rounded once to the type) is outside the bound while
    today's check against the unmutated exact value passes."""
    found = []
    for store, tol in stores.items():
        got = eb.round_to(mutant["want"], store)
        r, _, _ = eb.ratio(got, ref, store, "none")
        outside, passes = bool((r > 1).any()), passes_todays_check(got, ref["want"], tol)
        print("  %s: outside the bound %s (worst err / bound %.3g), today's check passes %s"
              % (store, outside, float(r.max()), passes))
        if outside and passes:
            found.append(store)
    return found


def box_mutation_case(geometry, flavour=((0, 4), False, True), C=32):
    g = gpu_cases.box_problem(geometry, C, flavour)
    ref = gpu_cases.box_reference(geometry, C, flavour)
    B, S, H, _, L, Lq, P = g["dims"]
    args = ("box", gpu_cases.every_type(g["value"]), g["shapes"], g["lsi"], g["ref"], g["off"],
            gpu_cases.kernel_offsets(int(round(P ** 0.5))), g["vr"], g["logits"], g["angle_mode"])
    return g, ref, args


def live_pairs(ref, C):
    """(b, q, h) of the pairs whose row of ``out`` has contributions, in order."""
    A = ref["out"]["A"]
    B, Lq = A.shape[:2]
    return [tuple(int(i) for i in at) for at in np.argwhere(A.reshape(B, Lq, -1, C).sum(-1) > 0)]


def first_with_a_gap(candidates, ref_out, stores=STORES):
    """candidates: an iterator of (name, mutated reference of ``out``).  -> (name, stores) of the first mutant that is
    outside the bound where today's check passes."""
    for name, mutant in candidates:
        print("%s:" % name)
        found = gap(mutant, ref_out, stores)
        if found:
            return name, found
    return None, []


def test_mutation_the_lowest_weight_point_of_a_pair_dropped():
    g, ref, args = box_mutation_case("model")
    w = ref["weights"][0][0]

    def candidates():
        for b, q, h in live_pairs(ref, 32):
            m = w.copy()
            l, p = np.unravel_index(int(np.argmin(m[b, q, h])), m.shape[3:])
            m[b, q, h, l, p] = 0.0
            yield "pair %s, weight %.2e" % ((b, q, h), w[b, q, h, l, p]), eb.boxes_reference(*args, weights=[m])["out"]
    name, found = first_with_a_gap(candidates(), ref["out"])
    assert found, "no pair whose lowest-weight point is missed by today's check and noticed by the bound"


def test_mutation_the_last_tiles_out_of_range_slot_given_a_points_weight():
    """ragged: L P = 12, tiles of G = 8: slot 12 of the second tile does not exist; it reads the last point's location
    (the index is clamped) and must weigh nothing -- here it weighs what point 11 weighs."""
    g, ref, args = box_mutation_case("ragged")
    w = ref["weights"][0][0]
    L, P = w.shape[3:]

    def candidates():
        for b, q, h in live_pairs(ref, 32):
            m = w.copy()
            m[b, q, h, L - 1, P - 1] *= 2.0
            yield ("pair %s, weight %.2e" % ((b, q, h), w[b, q, h, L - 1, P - 1]),
                   eb.boxes_reference(*args, weights=[m])["out"])
    name, found = first_with_a_gap(candidates(), ref["out"])
    assert found


def test_mutation_the_next_levels_box_for_the_first_point_of_a_straddling_tile():
    """odd_k: P = 9, tiles of 8: the second tile starts with point 8 of level 0 and goes on with level 1."""
    def candidates():
        for C, flavour in itertools.product(gpu_cases.CHANNELS, gpu_cases.box_cases.FLAVOURS):
            g, ref, args = box_mutation_case("odd_k", flavour, C)
            loc = ref["grid"][0]
            nxt, _ = eb.grid_reference(g["ref"], np.roll(g["off"], -1, 3), args[6], g["vr"], g["angle_mode"])
            for b, q, h in live_pairs(ref, C):
                m = loc.copy()
                m[b, q, h, 0, 8] = nxt[b, q, h, 0, 8]
                yield ("C=%d %s pair %s, weight %.2e" % (C, flavour, (b, q, h), ref["weights"][0][0][b, q, h, 0, 8]),
                       ref["out"], eb.boxes_reference(*args, loc=m)["out"])
    for name, ref_out, mutant in candidates():
        print("%s:" % name)
        if gap(mutant, ref_out):
            return
    raise AssertionError("the next level's box is nowhere missed by today's check")


def test_mutation_valid_ratios_swapped_on_one_level():
    g, ref, args = box_mutation_case("sixteen_levels")
    L = g["dims"][4]

    def candidates():
        for l in range(L):
            vr = g["vr"].copy()
            vr[:, :, :, l] = vr[:, :, :, l, :, ::-1]
            m, _ = eb.grid_reference(g["ref"], g["off"], args[6], vr, g["angle_mode"])
            yield "level %d" % l, eb.boxes_reference(*args, loc=m)["out"]
    name, found = first_with_a_gap(candidates(), ref["out"])
    assert found


def test_mutation_the_softmax_maximum_over_the_first_tile_only():
    """ragged (L P = 12, tiles of G = 8): the weights in float32 with the maximum of the first 8 logits, which lie 60
    below the other four, so that exp is taken of arguments near +60 instead of near 0 and the rounding of
    (z - m) log2 e is that of a number near 87, not near 0.  A softmax does not depend on what is subtracted, so the
    mutant differs from the float32 weights by roundings alone: it is outside ``dw`` (what the weights are held to),
    about four times, but in ``out`` it stays inside the bound -- the (n + 8) 2^-24 A of 48 corner terms is as large as the
    damage -- and only an exponent past float32's range (non-finite weights, which today's check refuses too) would
    show there.  The figure is printed, not asserted to be above 1."""
    geometry, C, flavour = "ragged", 32, ((0, 4), False, True)
    g = gpu_cases.box_problem(geometry, C, flavour)
    z = g["logits"].copy()
    z[..., :8] -= F(60)
    args = ("box", gpu_cases.every_type(g["value"]), g["shapes"], g["lsi"], g["ref"], g["off"],
            gpu_cases.kernel_offsets(2), g["vr"], z, g["angle_mode"])
    ref = eb.boxes_reference(*args)
    want, dw = eb.softmax_reference(z)
    fair, mutant = softmax_f32(z), softmax_f32(z, first=8)
    print("float32 weights with the row's maximum: worst err / dw %.3f" % gpu_cases.within(fair, want, dw * want, "fair"))
    with pytest.raises(AssertionError, match="outside the allowance"):
        gpu_cases.within(mutant, want, dw * want, "the maximum of the first 8 logits")
    print("... with the maximum of the first 8 logits: worst err / dw %.3f"
          % float((np.abs(mutant - want) / (dw * want)).max()))
    out = eb.boxes_reference(*args, weights=[mutant])["out"]
    for store, tol in STORES.items():
        got = eb.round_to(out["want"], store)
        r, _, _ = eb.ratio(got, ref["out"], store, "none")
        print("  out, %s: worst err / bound %.3f" % (store, float(r.max())))
        assert passes_todays_check(got, ref["out"]["want"], tol)


def test_mutation_relu_gradient_omitted_in_grad_offsets():
    """Without relu' a collapsed box gets the size gradient of an open one: everywhere (today's check notices that in
    every case here), and in one row of a case only -- the smallest such value of every k = 4 case in turn."""
    k = 4

    def candidates():
        for geometry, C, (per_head, with_vr) in itertools.product(INST_GEOMETRIES, gpu_cases.CHANNELS,
                                                                  gpu_cases.INST_FLAVOURS):
            ref = gpu_cases.inst_reference(geometry, C, k, per_head, with_vr, True)["grad_offsets"]
            whole = ref["unmasked"]
            changed = np.argwhere(whole != ref["want"])
            assert len(changed), "no collapsed box with a gradient"
            assert (ref["A"] + ref["E"])[tuple(changed.T)].max() == 0
            if (geometry, C, per_head, with_vr) == (INST_GEOMETRIES[0], gpu_cases.CHANNELS[0], False, False):
                yield "every row", ref, dict(want=whole)
            at = tuple(min(changed.tolist(), key=lambda a: abs(whole[tuple(a)])))
            m = ref["want"].copy()
            m[at] = whole[at]
            yield "%s C=%d per_head=%d vr=%d row %s, %.2e instead of 0" % (geometry, C, per_head, with_vr, at,
                                                                          whole[at]), ref, dict(want=m)
    for name, ref, mutant in candidates():
        print("%s:" % name)
        if gap(mutant, ref, {"float32": 1e-4}):          # (the gradients are float32 in every storage mode)
            return
    raise AssertionError("relu' omitted is nowhere missed by today's check")
