"""No GPU: the inputs of tests/test_gpu_isolation.py meet their conditions, the operator's definition (the C oracle) has
the property the kernels are held to, and the checking function reports three deliberately leaky forwards (DESIGN.md 5,
"Isolation")."""
import functools

import numpy as np
import pytest

import isolation as iso
from oracle import boxattn_oracle as oc
from isolation import BOX_FLAVOURS, DECODER, ENCODER, STAGED_GEOMETRY, STAGED_LEVELS, WIDE_LEVELS
from point_cases import LEVELS_A

SEEDED_6 = [(25, 25), (13, 13), (7, 5), (1, 3), (2, 1)]
# name -> levels, queries, points: every geometry of the GPU cases
GEOMETRIES = {
    "encoder": (ENCODER, "S", 4), "staged": (STAGED_LEVELS, "S", 4), "decoder": (DECODER, 50, 4),
    "seeded_6": (SEEDED_6, 700, 4), "wide_36": (WIDE_LEVELS, 6, 36), "wide_196": (WIDE_LEVELS, 6, 196),
    "shape_a": (LEVELS_A, 300, 16), "k14": (DECODER, 6, 196),
}


def test_geometries_are_the_gpu_files():
    import isolation as geb
    from point_cases import LEVELS_A as A
    from point_cases import SEEDED
    assert (geb.ENCODER, geb.DECODER, geb.WIDE_LEVELS, A) == (ENCODER, DECODER, WIDE_LEVELS, LEVELS_A)
    assert SEEDED[6][0] == SEEDED_6 and SEEDED[6][4] == 700


@functools.lru_cache(maxsize=None)
def case(name, edge, kind="box", pad=0):
    levels, Lq, P = GEOMETRIES[name]
    return iso.problem(levels, Lq, P, edge, kind=kind, C=4, pad=pad)


# ------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("edge", iso.EDGES)
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_conditions_on_the_inputs(name, edge):
    levels, _, P = GEOMETRIES[name]
    hold_conditions(name, levels, edge, case(name, edge, pad=3))


def hold_conditions(name, levels, edge, g):
    un, x, y, inside = g["unreferenced"], *iso.pixels(g["shapes"], g["loc"])
    for l, lv in enumerate(levels):
        rows = iso.level_rows(levels, l)
        if not iso.has_patch(lv, edge):
            assert un[:, rows].all(), "level %d is wholly outside: nothing of it is read" % l
            assert not inside[:, :, :, l].any()
            continue
        # the main patch alone (every batch entry but the victims'): at least half of the level is unreferenced; the
        # victims add the opposite patch in batch 0, where the share is printed and must stay above a quarter
        shares = un[:, rows].mean((1, 2))
        print("isolation inputs | %s | %s | level %d %r | unreferenced share per batch entry %s" % (
            name, edge, l, lv, " ".join("%.2f" % s for s in shares)))
        assert shares[1:].min() >= 0.5, shares
        assert shares[0] >= 0.25, shares
        # the patch holds all three kinds of point: wholly inside, with corners outside the map, outside the window
        size = (lv[1], lv[0])
        c = (x, y)[edge in ("bottom", "top")][:, :, :, l]
        n = size[edge in ("bottom", "top")]
        inner = ((c > 0) & (c < n - 1)).any()
        corner = (((c > -1) & (c < 0)) | ((c > n - 1) & (c < n))).any()
        outer = ((c <= -1) | (c >= n)).any()
        assert inner and corner and outer, (inner, corner, outer)
    for what, rows in iso.sentinels(levels, edge, g["value"].shape[1]).items():
        free = un | g["opposite"] if what.startswith("flat:") else un
        assert free[:, rows].all(), "%s %s: %s is referenced" % (name, edge, what)
    # the victims' own footprint (not widened) is disjoint from the widened footprint of everyone else
    B, Lq = g["loc"].shape[:2]
    others = [q for q in range(Lq) if q not in g["victims"]]
    own = iso.touched(g["shapes"], g["loc"][:1], 0, g["value"].shape[1], g["lsi"], queries=g["victims"])
    main = iso.touched(g["shapes"], g["loc"][:1], 1, g["value"].shape[1], g["lsi"], queries=others)
    assert own.any() == any(iso.has_patch(lv, edge) for lv in levels) and not (own & main).any()
    assert not (g["opposite"] & ~g["touched"]).any()


@pytest.mark.parametrize("edge", iso.EDGES)
@pytest.mark.parametrize("per_head,with_vr", [(False, True), (True, False)], ids=["shared_vr", "per_head"])
@pytest.mark.parametrize("angle_mode,ref_dim", BOX_FLAVOURS, ids=["plain", "turns_5", "turns_7", "radians"])
def test_conditions_on_the_inputs_from_boxes(angle_mode, ref_dim, per_head, with_vr, edge):
    """The same conditions on the points the float64 model makes of the reference windows and offsets."""
    for kind, Lq, k in (("box", 50, 2), ("instance", 6, 4), ("instance", 6, 14)):
        if kind == "instance" and angle_mode:
            continue
        g = iso.boxes_problem(DECODER, Lq, k, edge, kind=kind, C=4, pad=3, angle_mode=angle_mode, ref_dim=ref_dim,
                              per_head=per_head, with_vr=with_vr)
        hold_conditions("from boxes %s k=%d" % (kind, k), DECODER, edge, g)
        assert np.abs(g["off"][:, :, 0, 0, :4]).max() == 0 and np.abs(g["off"]).max() > 0      # level 0, head 0: no offset


@pytest.mark.parametrize("edge", iso.EDGES)
@pytest.mark.parametrize("geometry", sorted(STAGED_GEOMETRY))
def test_conditions_on_the_inputs_from_boxes_staged(geometry, edge):
    levels, B, H = STAGED_GEOMETRY[geometry]
    for i, (angle_mode, ref_dim) in enumerate(BOX_FLAVOURS):
        g = iso.boxes_problem(levels, "S", 2, edge, B=B, H=H, C=4, angle_mode=angle_mode, ref_dim=ref_dim,
                              per_head=i % 2 == 1, with_vr=i % 2 == 0)
        hold_conditions("staged from boxes " + geometry, levels, edge, g)


def test_touched_ignores_the_weights_and_widens_by_the_margin():
    shapes = np.array([[5, 6]])
    loc = np.full((1, 1, 1, 1, 1, 2), np.nan)
    loc[..., 0], loc[..., 1] = (2.25 + 0.5) / 6, (1.5 + 0.5) / 5            # pixel (2.25, 1.5): cell x 2..3, y 1..2
    want = np.zeros((5, 6), dtype=bool)
    want[1:3, 2:4] = True
    assert (iso.touched(shapes, loc, 0)[0, :, 0].reshape(5, 6) == want).all()
    want[0:4, 1:5] = True
    assert (iso.touched(shapes, loc, 1)[0, :, 0].reshape(5, 6) == want).all()
    loc[..., 0] = (6.0 + 0.5) / 6                                          # x = 6 = W: outside the window test
    assert not iso.touched(shapes, loc, 1).any()
    loc[..., 0] = (5.5 + 0.5) / 6                                          # x in (W - 1, W): column 5 only, widened 4..5
    assert (np.nonzero(iso.touched(shapes, loc, 1)[0, :, 0].reshape(5, 6).any(0))[0] == [4, 5]).all()


# ------------------------------------------------------------------ the definition itself has the property
def run_oracle(g, **over):
    d = dict(g, **over)
    a = [d[k] for k in ("value", "shapes", "lsi", "loc")]
    if g["kind"] == "instance":
        w = [d["spatial_w"], d["level_w"]]
        out, mask = oc.instance_attn_forward(*a, *w)
        gv, gl, gs, glw = oc.instance_attn_backward(*a, *w, d["grad_out"], d["grad_mask"])
        return dict(out=out, mask_out=mask, grad_value=gv, grad_loc=gl, grad_spatial=gs, grad_level=glw)
    out = oc.box_attn_forward(*a, d["attn"])
    gv, gl, ga = oc.box_attn_backward(*a, d["attn"], d["grad_out"])
    return dict(out=out, grad_value=gv, grad_loc=gl, grad_attn=ga)


@pytest.fixture
def one_thread():
    """(grad_value compared bit for bit: one summation order)"""
    n = oc.num_threads()
    oc.set_num_threads(1)
    yield
    oc.set_num_threads(n)


def nan_at(a, index):
    a = a.copy()
    a[index] = np.nan
    return a


@pytest.mark.parametrize("edge", iso.EDGES)
@pytest.mark.parametrize("kind,name", [("box", "encoder"), ("box", "decoder"), ("box", "seeded_6"), ("box", "wide_36"),
                                       ("instance", "shape_a"), ("instance", "k14")])
def test_the_definition_is_isolated(kind, name, edge, one_thread):
    g = case(name, edge, kind, pad=3)
    B, Lq, H = g["loc"].shape[:3]
    C = g["value"].shape[-1]
    what = "oracle %s %s %s" % (kind, name, edge)
    clean = run_oracle(g)
    assert all(np.isfinite(v).all() for v in clean.values())
    # 1. value: the unreferenced rows and the tail; all of batch 1; all of head 1
    n = iso.check_outputs(clean, run_oracle(g, value=iso.poison_rows(g["value"], g["unreferenced"])), what=what + " value")
    b1 = np.zeros((B, Lq, H), dtype=bool)
    b1[1:] = True
    iso.check_outputs(clean, run_oracle(g, value=nan_at(g["value"], np.s_[1:])), bqh=b1, grad_value="finite",
                      what=what + " value of batch 1")
    h1 = np.zeros((B, Lq, H), dtype=bool)
    h1[:, :, 1] = True
    iso.check_outputs(clean, run_oracle(g, value=nan_at(g["value"], np.s_[:, :, 1])), bqh=h1, grad_value="finite",
                      what=what + " value of head 1")
    # 2. upstream: the victims' rows; then head 0's channels of them only
    v = g["victims"]
    for heads, ch in ((None, np.s_[:]), ((0,), np.s_[:C])):
        over = dict(grad_out=nan_at(g["grad_out"], (0, v, ch)))
        if kind == "instance":
            over["grad_mask"] = nan_at(g["grad_mask"], (0, v, slice(None), ch))
        hm = np.ones(H, dtype=bool) if heads is None else np.arange(H) == 0
        got = run_oracle(g, **over)
        del got["out"]
        got.pop("mask_out", None)
        iso.check_outputs(clean, got, bqh=iso.victim_triples(g, heads), bsh=g["opposite"] & hm, what=what + " upstream")
    # 3. weights: (0, victim, head 0)
    q = v[len(v) // 2]
    one = np.zeros((B, Lq, H), dtype=bool)
    one[0, q, 0] = True
    over = {k: nan_at(g[k], (0, q, 0)) for k in (("spatial_w", "level_w") if kind == "instance" else ("attn",))}
    iso.check_outputs(clean, run_oracle(g, **over), bqh=one, bsh=g["opposite"] & (np.arange(H) == 0),
                      what=what + " weights")
    assert n > 0


# ------------------------------------------------------------------ the checker detects a leak
def forward_model(g, value, leak=None, beyond=0.0):
    """Box attention's forward in numpy, float64.  ``leak``: None (the definition), or one of three careless kernels
      "clamp"  every corner clamped into the map, the corners and points that do not count multiplied by 0;
      "row0"   a point outside the window test fetches its level's row 0, times 0;
      "flat"   a corner outside the map is read at its flat index -- (y, W) is the next line's first pixel, (-1, x) the
               preceding level's last line -- times 0."""
    shapes, lsi, loc, attn = g["shapes"], g["lsi"], g["loc"], g["attn"]
    B, S, H, C = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    guard = 64                                           # rows of ``beyond`` in front of and behind the tensor
    vp = np.full((B, S + 2 * guard, H, C), beyond)
    vp[:, guard:guard + S] = value
    x, y, inside = iso.pixels(shapes, loc)
    out = np.zeros((B, Lq, H, C))
    b, q, h = (a[..., None] for a in np.indices((B, Lq, H)))            # (B, Lq, H, 1) against the points' (.., P)
    for l in range(L):
        Hl, Wl = int(shapes[l, 0]), int(shapes[l, 1])
        xl, yl, ins = x[:, :, :, l], y[:, :, :, l], inside[:, :, :, l]
        x0, y0 = np.floor(xl).astype(np.int64), np.floor(yl).astype(np.int64)
        fx, fy = xl - x0, yl - y0
        for dy, dx, w in ((0, 0, (1 - fy) * (1 - fx)), (0, 1, (1 - fy) * fx), (1, 0, fy * (1 - fx)), (1, 1, fy * fx)):
            ys, xs = y0 + dy, x0 + dx
            ok = ins & (ys >= 0) & (ys < Hl) & (xs >= 0) & (xs < Wl)
            row = np.where(ok, ys * Wl + xs, 0)
            fetch = ok
            if leak == "clamp":
                row, fetch = np.clip(ys, 0, Hl - 1) * Wl + np.clip(xs, 0, Wl - 1), np.ones_like(ok)
            elif leak == "row0":
                fetch = ok | ~ins
            elif leak == "flat":
                row, fetch = np.where(ins, np.clip(ys * Wl + xs, -guard, S), 0), ins
            v = vp[b, guard + int(lsi[l]) + row, h]                   # (B, Lq, H, P, C)
            term = (attn[:, :, :, l] * w * ok)[..., None] * v
            out += np.where(fetch[..., None], term, 0.0).sum(3)
    return out.reshape(B, Lq, H * C)


@pytest.mark.parametrize("edge", iso.EDGES)
@pytest.mark.parametrize("name", ["decoder", "seeded_6"])
def test_the_checker_reports_three_leaky_forwards(name, edge):
    g = case(name, edge, pad=3)
    poisoned = iso.poison_rows(g["value"], g["unreferenced"])
    clean = forward_model(g, g["value"])
    np.testing.assert_allclose(clean, oc.box_attn_forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attn"]),
                               rtol=1e-12, atol=1e-12)
    assert iso.isolated("out", clean, forward_model(g, poisoned, None, np.nan)) == clean.size
    for leak in ("clamp", "row0", "flat"):
        # (on clean data the leaky kernel is right: only the poison tells)
        assert (forward_model(g, g["value"], leak) == clean).all(), leak
        with pytest.raises(AssertionError, match="not finite although nothing they depend on is"):
            iso.isolated("out", clean, forward_model(g, poisoned, leak, np.nan), what=leak)


def test_the_checker_reports_a_changed_bit_and_honours_the_exemption():
    clean = np.linspace(1.0, 2.0, 12).reshape(3, 4).astype(np.float32)
    got = clean.copy()
    got[1, 2] = np.nextafter(got[1, 2], np.float32(3.0))
    with pytest.raises(AssertionError, match=r"differ from the clean run; first at \(1, 2\)"):
        iso.isolated("x", clean, got)
    exempt = np.zeros((3, 4), dtype=bool)
    exempt[1, 2] = True
    assert iso.isolated("x", clean, got, exempt) == 11
    got[1, 2] = np.nan
    assert iso.isolated("x", clean, got, exempt) == 11
    got[0, 0] = -0.0 * clean[0, 0]
    with pytest.raises(AssertionError):
        iso.isolated("x", clean, got, exempt)


def test_block_spread_follows_the_balanced_partition():
    """(9, 13): two block columns, pixels 0..6 and 7..12; three block rows, 0..2, 3..5, 6..8."""
    shapes = np.array([[9, 13]])
    loc = np.empty((1, 1, 1, 1, 1, 2))
    loc[..., 0], loc[..., 1] = (6.5 + 0.5) / 13, (1.25 + 0.5) / 9          # corners x 6, 7; y 1, 2: both block columns
    got = iso.block_spread(shapes, loc, [0])[0, :, 0].reshape(9, 13)
    want = np.zeros((9, 13), dtype=bool)
    want[0:3, :] = True
    assert (got == want).all()
    loc[..., 0] = (12.5 + 0.5) / 13                                       # x 12, 13: the corner outside the map has no block
    got = iso.block_spread(shapes, loc, [0])[0, :, 0].reshape(9, 13)
    want[:] = False
    want[0:3, 7:] = True
    assert (got == want).all()
    four = np.repeat(loc, 4, 4)
    four[0, 0, 0, 0, 0, 0], four[0, 0, 0, 0, 1, 1] = (0.5 + 0.5) / 13, (7.5 + 0.5) / 9
    got = iso.block_spread(shapes, four, [0], groups=True)[0, :, 0].reshape(9, 13)
    assert got.all()                                                       # the group's block range: the whole map
