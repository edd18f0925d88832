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

The box kind's training step (grad_offsets, grad_ref_rows, grad_logits in the three angle modes):
  * the model's ``want`` agrees with float64 torch autograd through grid -> softmax -> bilinear sampling for the 16
    flavours on two geometries, within a tolerance made of float64's unit roundoff and the model's own planes;
  * the float32 chain on the CPU -- ``reduce_box_f32``: the reduction in the kernels' operation order -- stays within
    the bound for every case of the GPU matrix, every case keeps the cell-edge condition with the locations' own slack
    (one case re-seeded: boxes_cases.BWD_RESEED), and every geometry has must-be-zero elements in all
    three outputs; the backward building blocks restated in float32 numpy stay within theirs;
  * six wrong formulas (relu' omitted, a sine term's sign, a_t without the relu, the / 16, a partial softmax-Jacobian
    sum, a dropped gw) are all rejected by the bound; wrong everywhere, today's rule of
    tests/test_gpu_box_boxes_backward.py rejects them too; wrong in one row, each has rows it accepts.
"""
import itertools
import math

import numpy as np
import pytest
import torch

import error_bounds as eb
import boxes_cases
import compare_rules
from boxes_cases import F, c32, grid_f32
from compare_rules import POINT_TOL, check_scaled as check
from point_cases import _torch_grid
from oracle import boxattn_oracle as oc

BOX_CASES = list(itertools.product(boxes_cases.BOX_GEOMETRIES, boxes_cases.CHANNELS, boxes_cases.FLAVOURS))
INST_GEOMETRIES = sorted(boxes_cases.INST_GEOMETRY)
KERNEL_SIZES = boxes_cases.KERNEL_SIZES


# ------------------------------------------------------------------ float32 numpy, operation by operation


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
    ref, off, kidx, vr = g["ref"], g["off"], boxes_cases.kernel_offsets(k), g["vr"]
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


# ------------------------------------------------------------------ the grid
@pytest.mark.parametrize("P", boxes_cases.GRID_POINTS)
def test_float64_grid_agrees_with_the_reference_module_in_double(P):
    for angle_mode, per_head, with_vr in boxes_cases.GRID_FLAVOURS:
        g = boxes_cases.grid_problem(P, angle_mode, per_head, with_vr)
        t = lambda a: None if a is None else torch.from_numpy(a).double()
        want = _torch_grid(t(g["ref"]), t(g["off"]), t(g["kidx"]), t(g["vr"]), angle_mode).numpy()
        loc, dloc = eb.grid_reference(g["ref"], g["off"], g["kidx"], g["vr"], angle_mode)
        assert loc.shape == want.shape == dloc.shape
        assert float(np.abs(loc - want).max()) <= 1e-12, (P, angle_mode, per_head, with_vr)


def grid_inputs():
    """(name, ref, off, kidx, vr, angle_mode) of every input of the GPU file."""
    for P, (angle_mode, per_head, with_vr) in itertools.product(boxes_cases.GRID_POINTS, boxes_cases.GRID_FLAVOURS):
        g = boxes_cases.grid_problem(P, angle_mode, per_head, with_vr)
        yield ("grid P=%d %s" % (P, (angle_mode, per_head, with_vr)), g["ref"], g["off"], g["kidx"], g["vr"], angle_mode)
    for geometry, C, flavour in BOX_CASES:
        g = boxes_cases.box_problem(geometry, C, flavour)
        k = int(round(g["dims"][6] ** 0.5))
        yield ("box %s C=%d %s" % (geometry, C, flavour), g["ref"], g["off"], boxes_cases.kernel_offsets(k), g["vr"],
               g["angle_mode"])
    for geometry, C, k, (per_head, with_vr) in itertools.product(INST_GEOMETRIES, boxes_cases.CHANNELS, KERNEL_SIZES,
                                                                 boxes_cases.INST_FLAVOURS):
        g = boxes_cases.inst_problem(geometry, C, k, per_head, with_vr)
        yield ("instance %s C=%d k=%d %s" % (geometry, C, k, (per_head, with_vr)), g["ref"], g["off"],
               boxes_cases.kernel_offsets(k), g["vr"], 0)


def test_float32_grid_stays_within_dloc_at_every_point_of_every_case():
    worst = {0: 0.0, 1: 0.0, 2: 0.0}
    turns = 0.0
    for name, ref, off, kidx, vr, angle_mode in grid_inputs():
        loc, dloc = eb.grid_reference(ref, off, kidx, vr, angle_mode)
        got = grid_f32(ref, off, kidx, vr, angle_mode)
        worst[angle_mode] = max(worst[angle_mode], compare_rules.within(got, loc, dloc, name))
        if angle_mode:
            turns = max(turns, float(np.abs(ref[..., 4]).max()) / (1.0 if angle_mode == 1 else 2 * math.pi))
    assert turns >= 3.0, "no angle of several turns among the cases"
    print("float32 numpy grid, worst err / dloc: %s" % ", ".join("angle mode %d %.3f" % kv for kv in worst.items()))


def test_float32_weights_stay_within_dw():
    worst = {"softmax": 0.0, "spatial": 0.0, "level": 0.0}
    rows = [boxes_cases.softmax_rows(n) for n in (1, 4, 12, 18, 64)]
    rows += [boxes_cases.box_problem(*c)["logits"] for c in BOX_CASES]
    for z in rows:
        want, dw = eb.softmax_reference(z)
        worst["softmax"] = max(worst["softmax"], compare_rules.within(softmax_f32(z), want, dw * want, "softmax"))
    cells = [(boxes_cases.cell_rows(L), k) for L in (1, 5, 16) for k in KERNEL_SIZES]
    cells += [(boxes_cases.inst_problem(geo, C, k, ph, vr)["logits"], k) for geo, C, k, (ph, vr) in
              itertools.product(INST_GEOMETRIES, boxes_cases.CHANNELS, KERNEL_SIZES, boxes_cases.INST_FLAVOURS)]
    for z, k in cells:
        sw, lw, dsw, dlw = eb.instance_weights_reference(z, k, True)
        got_s, got_l = instance_weights_f32(z, k)
        worst["spatial"] = max(worst["spatial"], compare_rules.within(got_s, sw, dsw * sw, "spatial weights"))
        worst["level"] = max(worst["level"], compare_rules.within(got_l, lw, dlw * lw, "level weights"))
    print("float32 numpy weights, worst err / dw: %s" % ", ".join("%s %.3f" % kv for kv in worst.items()))


def test_weights_of_a_row_sum_to_one_and_expand_row_major():
    z = boxes_cases.cell_rows(5)
    sw, lw, _, _ = eb.instance_weights_reference(z, 6, True)
    assert np.abs(sw.sum((-1, -2)) - 1).max() < 1e-14 and np.abs(lw.sum(-2) - 1).max() < 1e-14
    # point (y, x) of a 6 x 6 kernel lies in cell (y >= 3, x >= 3); the reference module repeats along both axes
    t = torch.from_numpy(z).double()
    rep = t.repeat_interleave(3, -1).repeat_interleave(3, -2)
    want = torch.softmax(rep.reshape(1, 8, 1, -1), -1).reshape(1, 8, 1, 5, 36).numpy()
    assert np.abs(sw - want).max() < 1e-15
    assert np.abs(lw - torch.softmax(rep, -3).reshape(1, 8, 1, 5, 36).numpy()).max() < 1e-15


# ------------------------------------------------------------------ the whole chain in float32 on the CPU
@pytest.mark.parametrize("geometry", boxes_cases.BOX_GEOMETRIES)
def test_box_chain_in_float32_is_within_the_bound(geometry):
    worst, zeros = 0.0, 0
    for C, flavour in itertools.product(boxes_cases.CHANNELS, boxes_cases.FLAVOURS):
        g = boxes_cases.box_problem(geometry, C, flavour)
        B, S, H, _, L, Lq, P = g["dims"]
        ref = boxes_cases.box_reference(geometry, C, flavour)["out"]
        kidx = boxes_cases.kernel_offsets(int(round(P ** 0.5)))
        loc = grid_f32(g["ref"], g["off"], kidx, g["vr"], g["angle_mode"])
        attn = softmax_f32(g["logits"]).reshape(B, Lq, H, L, P)
        out = oc.box_attn_forward(c32(boxes_cases.every_type(g["value"])), g["shapes"], g["lsi"], c32(loc), c32(attn))
        worst = max(worst, eb.hold(out, ref, "float32", "none", "float32 chain: %s C=%d %s" % (geometry, C, flavour)))
        must = ((ref["A"] + ref["E"]) == 0).reshape(-1, C)          # a row: the C channels of a (query, head) pair
        zeros += int(must.all(-1).sum())
    assert zeros, "%s: no row of out that must be all zero" % geometry
    print("error-bound | float32 chain on the CPU, box from boxes: %s (%d must-be-zero rows) | float32 | out | %.3f"
          % (geometry, zeros, worst))


def inst_chain_f32(g, k, with_mask):
    B, S, H, C, L, Lq = g["dims"]
    P = k * k
    gout, gmask = boxes_cases.inst_upstream(g, k)
    loc = c32(grid_f32(g["ref"], g["off"], boxes_cases.kernel_offsets(k), g["vr"], 0))
    sw, lw = (c32(a) for a in instance_weights_f32(g["logits"], k))
    value = c32(boxes_cases.every_type(g["value"]))
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
    res = dict(zip(boxes_cases.GRAD_NAMES, grads), out=out)
    if with_mask:
        res["mask_out"] = mask
    return res


@pytest.mark.parametrize("k", KERNEL_SIZES)
@pytest.mark.parametrize("geometry", INST_GEOMETRIES)
def test_instance_chain_in_float32_is_within_the_bound(geometry, k):
    """Also: every input keeps the cell-edge condition, and every case has an all-zero row of ``out`` and a
    ``grad_offsets`` size component that must be exactly zero."""
    worst, edge, zero_rows, zero_sizes = {}, {}, 0, 0
    for C, (per_head, with_vr), with_mask in itertools.product(boxes_cases.CHANNELS, boxes_cases.INST_FLAVOURS,
                                                              (True, False)):
        g = boxes_cases.inst_problem(geometry, C, k, per_head, with_vr)
        ref = boxes_cases.inst_reference(geometry, C, k, per_head, with_vr, with_mask)
        what = "float32 chain: %s C=%d k=%d per_head=%d vr=%d mask=%d" % (geometry, C, k, per_head, with_vr, with_mask)
        assert ref["edge_share"] <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (what,
                                                                                              100 * ref["edge_share"])
        for name, got in inst_chain_f32(g, k, with_mask).items():
            key = "%s%s" % (name, "" if with_mask or name == "out" else " (no grad_mask)")
            worst[key] = max(worst.get(key, 0.0), eb.hold(got, ref[name], "float32", "none", "%s: %s" % (what, name)))
            if name in boxes_cases.GRAD_NAMES:
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
    """inst_reduce_grid / inst_reduce_logits of tests/boxes_cases.py (restated from the kernels) on the reference's own
    per-point float64 gradients give the reference's three gradients."""
    import boxes_cases
    k = 6
    g = boxes_cases.inst_problem("five_levels", 32, k, True, True)
    gout, gmask = boxes_cases.inst_upstream(g, k)
    kidx = boxes_cases.kernel_offsets(k)
    loc, dloc = eb.grid_reference(g["ref"], g["off"], kidx, g["vr"], 0)
    sw, lw, _, _ = eb.instance_weights_reference(g["logits"], k, True)
    pts = eb.instance_reference(boxes_cases.every_type(g["value"]), g["shapes"], g["lsi"], loc, sw, lw, gout, gmask)
    ref = boxes_cases.inst_reference("five_levels", 32, k, True, True, True)
    goff, rows = boxes_cases.inst_reduce_grid(g["ref"], g["off"], kidx, g["vr"], pts["grad_loc"]["want"])
    glog = boxes_cases.inst_reduce_logits(g["logits"], k, pts["grad_spatial"]["want"], pts["grad_level"]["want"])
    for name, got in zip(boxes_cases.GRAD_NAMES, (goff, rows, glog)):
        want = ref[name]["want"]
        assert float(np.abs(got - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max())), name


# ------------------------------------------------------------------ mutations: what the bound buys
STORES = {"float32": 1e-4, "bf16": 1e-2, "f16": 1e-2}        # today's tolerances (compare_rules.tol_of)


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
    g = boxes_cases.box_problem(geometry, C, flavour)
    ref = boxes_cases.box_reference(geometry, C, flavour)
    B, S, H, _, L, Lq, P = g["dims"]
    args = ("box", boxes_cases.every_type(g["value"]), g["shapes"], g["lsi"], g["ref"], g["off"],
            boxes_cases.kernel_offsets(int(round(P ** 0.5))), g["vr"], g["logits"], g["angle_mode"])
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
        for C, flavour in itertools.product(boxes_cases.CHANNELS, boxes_cases.FLAVOURS):
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
    g = boxes_cases.box_problem(geometry, C, flavour)
    z = g["logits"].copy()
    z[..., :8] -= F(60)
    args = ("box", boxes_cases.every_type(g["value"]), g["shapes"], g["lsi"], g["ref"], g["off"],
            boxes_cases.kernel_offsets(2), g["vr"], z, g["angle_mode"])
    ref = eb.boxes_reference(*args)
    want, dw = eb.softmax_reference(z)
    fair, mutant = softmax_f32(z), softmax_f32(z, first=8)
    print("float32 weights with the row's maximum: worst err / dw %.3f" % compare_rules.within(fair, want, dw * want, "fair"))
    with pytest.raises(AssertionError, match="outside the allowance"):
        compare_rules.within(mutant, want, dw * want, "the maximum of the first 8 logits")
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
        for geometry, C, (per_head, with_vr) in itertools.product(INST_GEOMETRIES, boxes_cases.CHANNELS,
                                                                  boxes_cases.INST_FLAVOURS):
            ref = boxes_cases.inst_reference(geometry, C, k, per_head, with_vr, True)["grad_offsets"]
            whole = ref["unmasked"]
            changed = np.argwhere(whole != ref["want"])
            assert len(changed), "no collapsed box with a gradient"
            assert (ref["A"] + ref["E"])[tuple(changed.T)].max() == 0
            if (geometry, C, per_head, with_vr) == (INST_GEOMETRIES[0], boxes_cases.CHANNELS[0], False, False):
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


# ------------------------------------------------------------------ the box training step from boxes (box kind, gradients)
BWD_NAMES = boxes_cases.GRAD_NAMES


def reduce_box_f32(g, kidx, gloc, gattn, attn):
    """The box kind's three gradients from float32 per-point gradients, float32 numpy in the kernels' operation order
    (boxattn_grid.h grid_grad_add point by point, grid_grad_store; the softmax Jacobian of boxattn_pointwise.h): every
    operation rounds once, no fused multiply-add."""
    ref, off, vr, mode = g["ref"], g["off"], g["vr"], g["angle_mode"]
    lead = off.shape[:4]
    V = off.shape[-1]
    r = ref[:, :, None, None] if ref.ndim == 3 else ref[:, :, :, None]
    col = lambda j: np.broadcast_to(r[..., j], lead)
    rw, rh = col(2), col(3)
    w = rw + off[..., 2] / F(8) * rw
    h = rh + off[..., 3] / F(8) * rh
    sn, cs = np.zeros(lead, F), np.ones(lead, F)
    two_pi = F(2) * F(math.pi)
    if mode:
        theta = ((col(4) + off[..., 4] / F(16)) * F(2) * F(math.pi) if mode == 1 else col(4)).astype(F)
        sn, cs = np.sin(theta), np.cos(theta)
    vx, vy = (vr[..., 0, 0], vr[..., 0, 1]) if vr is not None else (F(1), F(1))
    wr, hr = np.maximum(w, F(0)), np.maximum(h, F(0))
    gloc = gloc.astype(F)
    a_cx, a_cy, a_w, a_h, a_t = (np.zeros(lead, F) for _ in range(5))
    for p in range(kidx.shape[0]):
        gx, gy = gloc[..., p, 0] * vx, gloc[..., p, 1] * vy
        kx, ky = kidx[p]
        a_cx = a_cx + gx
        a_cy = a_cy + gy
        a_w = a_w + kx * (gx * cs + gy * sn)
        a_h = a_h + ky * (gy * cs - gx * sn)
        lx, ly = kx * wr, ky * hr
        a_t = a_t + (gx * (-lx * sn - ly * cs) + gy * (lx * cs - ly * sn))
    a_w, a_h = np.where(w > 0, a_w, F(0)), np.where(h > 0, a_h, F(0))
    go = [a_cx * rw / F(8), a_cy * rh / F(8), a_w * rw / F(8), a_h * rh / F(8)]
    if V == 5:
        go.append(a_t * two_pi / F(16) if mode == 1 else np.zeros(lead, F))
    row_t = a_t * two_pi if mode == 1 else a_t if mode == 2 else np.zeros(lead, F)
    rows = np.stack([a_cx, a_cy, a_cx * off[..., 0] / F(8) + a_w * (F(1) + off[..., 2] / F(8)),
                     a_cy * off[..., 1] / F(8) + a_h * (F(1) + off[..., 3] / F(8)), row_t], -1)
    goff = np.stack(go, -1)
    attn, gattn = attn.astype(F).reshape(lead[:3] + (-1,)), gattn.astype(F).reshape(lead[:3] + (-1,))
    glog = attn * (gattn - (attn * gattn).sum(-1, keepdims=True, dtype=F))
    assert goff.dtype == rows.dtype == glog.dtype == F
    return goff, rows, glog


def box_chain_f32(g):
    """The training step from boxes in float32 on the CPU: float32 grid and weights, the C oracle's float32 build for
    the per-point gradients, float32 reductions."""
    B, S, H, C, L, Lq, P = g["dims"]
    kidx = boxes_cases.kernel_offsets(int(round(P ** 0.5)))
    loc = c32(grid_f32(g["ref"], g["off"], kidx, g["vr"], g["angle_mode"]))
    attn = c32(softmax_f32(g["logits"]).reshape(B, Lq, H, L, P))
    _, gloc, gattn = oc.box_attn_backward(c32(boxes_cases.every_type(g["value"])), g["shapes"], g["lsi"], loc, attn,
                                          c32(boxes_cases.bwd_upstream(g)))
    return reduce_box_f32(g, kidx, np.asarray(gloc).reshape(loc.shape), np.asarray(gattn).reshape(attn.shape), attn)


@pytest.mark.parametrize("geometry", boxes_cases.BOX_GEOMETRIES)
def test_box_backward_chain_in_float32_is_within_the_bound(geometry):
    """Every case of the GPU matrix: the reference's own arithmetic in float32 meets the bound, the inputs keep the
    cell-edge condition (with the locations' own slack), and the model has elements that must be exactly zero."""
    worst, edge, zeros, share = {}, {}, {n: 0 for n in BWD_NAMES}, 0.0
    for C, flavour in itertools.product(boxes_cases.CHANNELS, boxes_cases.FLAVOURS):
        g = boxes_cases.bwd_problem(geometry, C, flavour)
        ref = boxes_cases.bwd_reference(geometry, C, flavour)
        what = "float32 chain, box backward from boxes: %s C=%d angle=%d D=%d per_head=%d vr=%d" % (
            (geometry, C) + flavour[0] + flavour[1:])
        share = max(share, ref["edge_share"])
        assert ref["edge_share"] <= eb.EDGE_CAP, "%s: %.4f %% of the points on a cell edge" % (what,
                                                                                              100 * ref["edge_share"])
        for name, got in zip(BWD_NAMES, box_chain_f32(g)):
            assert got.shape == ref[name]["want"].shape, name
            worst[name] = max(worst.get(name, 0.0), eb.hold(got, ref[name], "float32", "none", "%s: %s" % (what, name)))
            edge[name] = max(edge.get(name, 0.0), eb.edge_dominated(ref[name]))
            zeros[name] += int(((ref[name]["A"] + ref[name]["E"]) == 0).sum())
    assert all(zeros.values()), "%s: an output without elements that must be exactly zero: %s" % (geometry, zeros)
    for name, w in worst.items():
        print("error-bound | float32 chain on the CPU, box backward from boxes: %s (%d must-be-zero elements) | float32 "
              "| %s | %.3f" % (geometry, zeros[name], name, w))
    print("%s: worst share of points on a cell edge %.4f %% (cap %.1f %%); share of elements whose bound is more than "
          "half edge allowance: %s" % (geometry, 100 * share, 100 * eb.EDGE_CAP,
                                       ", ".join("%s %.4f" % kv for kv in edge.items())))


@pytest.mark.parametrize("geometry", ["ragged", "odd_k"])
def test_box_gradient_model_agrees_with_float64_autograd(geometry):
    """grid -> softmax -> bilinear sampling in torch float64, differentiated, against the model's ``want``: all 16
    flavours.  Both sides evaluate the same sums in float64; either is within (n + 8) 2^-53 A of the exact value (the
    bound's own rounding term with float64's unit), and every float32 allowance in E that is not an edge jump -- the
    sine and cosine, the weights, the pixel coordinates -- has a float64 counterpart 2^-29 = 2^-53 / 2^-24 times its size
    or smaller (SINCOS_ABS 2^-22 against one ulp of a double-precision sine, 2^-52).  So
    |model - autograd| <= 2 (n + 8) 2^-53 A + 2^-29 (E - J) per element; reference-window gradients are compared summed
    over the levels (and heads) as autograd returns them, with the sums of the planes and that many more terms."""
    from oracle import torch_fallback
    worst = 0.0
    for flavour in boxes_cases.FLAVOURS:
        g = boxes_cases.bwd_problem(geometry, 16, flavour)
        model = boxes_cases.bwd_reference(geometry, 16, flavour)
        B, S, H, C, L, Lq, P = g["dims"]
        leaf = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_()
        ref, off, logits = leaf(g["ref"]), leaf(g["off"]), leaf(g["logits"])
        vr = None if g["vr"] is None else torch.from_numpy(g["vr"]).double()
        kidx = torch.from_numpy(boxes_cases.kernel_offsets(int(round(P ** 0.5)))).double()
        loc = _torch_grid(ref, off, kidx, vr, g["angle_mode"])
        attn = torch.softmax(logits, -1).view(B, Lq, H, L, P)
        out = torch_fallback.box_attn(torch.from_numpy(boxes_cases.every_type(g["value"])), g["shapes"], loc, attn)
        (out * torch.from_numpy(boxes_cases.bwd_upstream(g))).sum().backward()
        n5 = min(5, g["ref"].shape[-1])
        axes = (3,) if g["ref"].ndim == 4 else (2, 3)
        rows = model["grad_ref_rows"]
        summed = {m: rows[m].sum(axes)[..., :n5] for m in ("want", "A", "E", "J")}
        summed["n"] = rows["n"].max(axes)[..., :n5] + np.prod([rows["n"].shape[a] for a in axes])
        assert not ref.grad.numpy()[..., n5:].any()              # (the values past the angle take no part)
        for name, planes, want in (("offsets", model["grad_offsets"], off.grad.numpy()),
                                   ("ref_windows", summed, ref.grad.numpy()[..., :n5]),
                                   ("logits", model["grad_logits"], logits.grad.numpy())):
            assert planes["want"].shape == want.shape, name
            tol = 2 * (planes["n"] + 8) * 2.0 ** -53 * planes["A"] + 2.0 ** -29 * (planes["E"] - planes["J"])
            err = np.abs(planes["want"] - want)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(err == 0, 0.0, err / tol)
            at = np.unravel_index(int(np.argmax(r)), r.shape)
            worst = max(worst, float(r[at]))
            assert r[at] <= 1.0, "%s %s: %s at %s: model %.17g, autograd %.17g, allowed %.3e" % (
                geometry, flavour, name, at, planes["want"][at], want[at], tol[at])
    print("%s: worst |model - autograd| / float64 tolerance %.3f" % (geometry, worst))


def test_backward_building_blocks_in_float32_are_within_the_bound():
    """ops.box_grid_backward, ops.softmax_backward and ops.instance_weights_backward on their own, restated in float32
    numpy on the inputs of the GPU tests: exact float32 upstream gradients, so the bound is the reduction's roundings,
    the rotation allowance and the weights' dw alone."""
    worst = {}
    for P, (angle_mode, per_head, with_vr) in itertools.product(boxes_cases.GRID_POINTS, boxes_cases.GRID_FLAVOURS):
        g = boxes_cases.grid_problem(P, angle_mode, per_head, with_vr)
        gg = boxes_cases.grid_upstream(P, angle_mode, per_head, with_vr)
        ref = eb.grid_backward_reference(g["ref"], g["off"], g["kidx"], g["vr"], angle_mode, gg)
        one = np.ones(g["off"].shape[:3] + (1,), F)
        goff, rows, _ = reduce_box_f32(g, g["kidx"], gg, one, one)
        for name, got in (("grad_offsets", goff), ("grad_ref_rows", rows)):
            what = "box_grid_backward P=%d angle=%d per_head=%d vr=%d: %s" % (P, angle_mode, per_head, with_vr, name)
            worst[name] = max(worst.get(name, 0.0), eb.hold(got, ref[name], "float32", "none", what))
    for rows_, n in itertools.product(boxes_cases.SOFTMAX_BWD_ROWS, boxes_cases.SOFTMAX_BWD_LENGTHS):
        a, gw = boxes_cases.softmax_bwd_problem(rows_, n)
        got = a * (gw - (a * gw).sum(-1, keepdims=True, dtype=F))
        ref = eb.softmax_backward_reference(a, gw)
        for store in eb.STORE:
            worst["softmax " + store] = max(worst.get("softmax " + store, 0.0),
                                            eb.hold(eb.round_to(got, store), ref, store, "none",
                                                    "softmax_backward rows=%d n=%d" % (rows_, n)))
    for L, k in itertools.product((1, 5, 16), KERNEL_SIZES):
        z = boxes_cases.cell_rows(L)
        gs, gl = boxes_cases.cell_upstream(L, k)
        for which, (s, l) in (("both", (gs, gl)), ("spatial", (gs, None)), ("level", (None, gl))):
            ref = eb.cell_logits_backward_reference(z, k, s, l)
            _, _, got = reduce_f32(dict(ref=np.zeros((1, 8, 4), F), off=np.zeros((1, 8, 1, L, 4), F), vr=None, logits=z), k,
                                   np.zeros((1, 8, 1, L, k * k, 2), F), np.zeros_like(gs) if s is None else s, l)
            worst["cells " + which] = max(worst.get("cells " + which, 0.0),
                                          eb.hold(got, ref, "float32", "none", "cells L=%d k=%d %s" % (L, k, which)))
    print("float32 numpy building blocks, worst err / bound: %s" % ", ".join("%s %.3f" % kv for kv in worst.items()))


# ---- mutations of the box kind's gradients: written into ``want``, held against the unmutated reference
def todays_rule(got, want):
    """tests/test_gpu_box_boxes_backward.py: |got - want| <= 1e-4 (max(1, rms(want)) + |want|)."""
    return passes_todays_check(got, want, POINT_TOL)


def judge(name, mutant, ref):
    """The float32 rounding of the mutant's exact value against the unmutated reference -> (the bound rejects the
    mutant, today's rule accepts it, rows with a gap, rows changed).  Both checks are per element, so a kernel that is
    wrong in one row only -- one (b, q, h, l) box, one (b, q, h) row of logits: a lane, a level slot -- is judged from
    the same figures: such a row has a gap if the bound rejects an element of it and today's rule accepts them all."""
    got = eb.round_to(mutant["want"], "float32")
    want = ref["want"]
    r, err, _ = eb.ratio(got, ref, "float32", "none")
    outside, passes = bool((r > 1).any()), todays_rule(got, want)
    fine_today = err / (max(1.0, float(np.sqrt(np.mean(want * want)))) + np.abs(want)) <= POINT_TOL      # ``check``
    assert bool(fine_today.all()) == passes
    changed = (mutant["want"] != want).any(-1)
    gaps = (r > 1).any(-1) & fine_today.all(-1)
    print("mutation | %s | worst err / bound %.3g | everywhere: the bound %s, today's rule %s | in one row: a gap in %d "
          "of the %d rows it changes" % (name, float(r.max()), "rejects" if outside else "ACCEPTS",
                                         "accepts" if passes else "rejects", int(gaps.sum()), int(changed.sum())))
    return outside, passes, int(gaps.sum()), int(changed.sum())


def bwd_mutants(geometry, flavour, mutation, C=32):
    g = boxes_cases.bwd_problem(geometry, C, flavour)
    ref = boxes_cases.bwd_reference(geometry, C, flavour)
    a = boxes_cases.bwd_model_args(g)
    return g, ref, eb.box_gradients(ref["points"], a[4], a[5], a[6], a[7], a[9], mutation)


ROTATED = ((1, 5), False, True)
# name -> (geometry, flavour, the mutation, the outputs it changes): (i) relu' omitted in a rotated case, (ii) the sine
# term of a_h with its sign flipped on one level, (iii) a_t from kidx size without the relu, (iv) grad_offsets[4] without
# the / 16, (v) the Jacobian's sum a gw over the first 8 of 16 levels, (vi) the lowest-weight point's gw dropped from its row
MUTATIONS = {
    "i_relu_grad_omitted": ("model", ROTATED, ("no_relu_grad",), ("grad_offsets", "grad_ref_rows")),
    "ii_sine_of_a_h_flipped_on_level_1": ("model", ROTATED, (("flip_sin_h", 1),), ("grad_offsets", "grad_ref_rows")),
    "iii_a_t_without_the_relu": ("model", ROTATED, ("no_relu_t",), ("grad_offsets", "grad_ref_rows")),
    "iv_angle_offset_without_the_sixteenth": ("model", ROTATED, ("no_sixteenth",), ("grad_offsets",)),
    "v_jacobian_sum_over_8_of_16_levels": ("sixteen_levels", ROTATED, (("dot_first", 32),), ("grad_logits",)),
    "vi_lowest_weight_gw_dropped": ("model", ROTATED, ("drop_lowest",), ("grad_logits",)),
}
# The table of DESIGN.md 5.  Wrong everywhere, every one of the six is rejected by the bound AND by today's rule on
# these inputs (the gradients are of order 0.1 ... 10, far above the rule's floor of 1e-4).  Wrong in one row only, every
# one has rows that today's rule accepts and the bound rejects (10, 3, 11, 1, 1 and 47 in the first output each changes).


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_of_the_box_gradients(name):
    """Each wrong formula, in every output it changes: the bound rejects it.  What today's rule says is printed and must
    be what DESIGN.md 5 records: it rejects the formula that is wrong everywhere, and accepts it in some single row
    that the bound rejects."""
    geometry, flavour, mutation, outputs = MUTATIONS[name]
    g, ref, mutant = bwd_mutants(geometry, flavour, mutation)
    if mutation == ("no_relu_t",):
        assert (np.concatenate([1 + g["off"][..., 2] / 8, 1 + g["off"][..., 3] / 8]) < 0).any(), "no size below zero"
    everywhere, one_row = [], 0
    for out in outputs:
        assert (mutant[out]["want"] != ref[out]["want"]).any(), "%s changes nothing in %s" % (name, out)
        outside, passes, gaps, changed = judge("%s | %s" % (name, out), mutant[out], ref[out])
        assert outside, "%s in %s is inside the bound" % (name, out)
        everywhere.append(passes)
        one_row += gaps
    assert not any(everywhere), "%s: today's rule accepts it everywhere in %s of %s" % (name, everywhere, outputs)
    assert one_row, "%s: no single row that today's rule accepts and the bound rejects" % name
