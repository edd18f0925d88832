"""No output may depend on input data its definition does not name (test helper; not a conftest, never imported by
boxer_amd).  DESIGN.md 5, "Isolation".

The method is metamorphic: everything the definition of an output does not name is overwritten with NaN, and the
output must not change.  Only data is poisoned -- value, grad_out, grad_mask, weights, logits -- never a location, a box,
a shape or anything an address is computed from.

  touched       the value rows a set of float64 locations may read: every in-window point's 2 x 2 footprint, widened by
                a margin (a corner whose weight is exactly 0 may be read, and the float32 pixel coordinate may land in
                the neighbouring cell); its complement is the unreferenced set, which is poisoned;
  edge_family   locations that crowd every level's points into one patch astride one edge of the map, so that most of
                every level is unreferenced and the rows a careless kernel would fetch instead (the neighbouring line's
                end, the neighbouring level, row 0) are;
  isolated      the check itself: a poisoned run against a clean run of the same call, bit for bit outside what was
                poisoned on purpose;
  arena         a tensor as a view inside a larger buffer with 64 KiB of guard on either side (NaN in front of and
                behind inputs, the byte 0xA5 around outputs, scratch, plan and state); guards_intact compares them
                bitwise after the call.
"""
import numpy as np

EDGES = ("right", "left", "bottom", "top")
OPPOSITE = {"right": "left", "left": "right", "bottom": "top", "top": "bottom"}
ACROSS_PX = 1.4          # the patch reaches this far across the edge, both ways: more than a pixel inside and outside
ALONG_PX = 0.4           # ... and this far along it, about the edge's midpoint
MIN_ALONG, MIN_ACROSS = 7, 5        # a level smaller than this gets no patch: its points lie far outside
FAR = 2.5                # (normalised) where the points of a level without a patch go: more than a whole map outside
GUARD = 64 * 1024        # bytes of guard on either side of an arena view: a condition (more than any row pitch and window
#                          row of the shapes tested), not a measurement
GUARD_BYTE = 0xA5        # around outputs, scratch, plan, state
NAN_BYTE = 0xFF          # 0xFF.. is a NaN in float32, bfloat16 and float16: around float inputs


def tables(levels, pad=0):
    """-> shapes (L, 2) int64, level_start_index (L,), S (with ``pad`` rows after the last level)."""
    shapes = np.asarray(levels, dtype=np.int64).reshape(-1, 2)
    sizes = shapes.prod(1)
    return shapes, np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64), int(sizes.sum()) + pad


def pixels(shapes, loc):
    """float64 pixel coordinates (x, y), each (B, Lq, H, L, P), and the window test (-1, size) of the definition."""
    loc = np.asarray(loc, dtype=np.float64)
    size = np.asarray(shapes, dtype=np.float64)
    x = loc[..., 0] * size[None, None, None, :, None, 1] - 0.5
    y = loc[..., 1] * size[None, None, None, :, None, 0] - 0.5
    inside = (x > -1) & (y > -1) & (x < size[None, None, None, :, None, 1]) & (y < size[None, None, None, :, None, 0])
    return x, y, inside


def touched(shapes, loc, margin=1, S=None, lsi=None, queries=None):
    """(B, S, H) bool: the pixels of every in-window point's 2 x 2 footprint, widened by ``margin`` pixels each way and
    clipped to the map.  The weights are not looked at.  ``S`` / ``lsi``: the value tensor's (default: the levels packed,
    no padded tail); ``queries``: only these queries' points (default all)."""
    shapes = np.asarray(shapes, dtype=np.int64)
    lsi0, S0 = tables(shapes)[1:]
    lsi = lsi0 if lsi is None else np.asarray(lsi, dtype=np.int64)
    S = S0 if S is None else int(S)
    x, y, inside = pixels(shapes, loc)
    B, Lq, H, L, P = x.shape
    if queries is not None:
        keep = np.zeros(Lq, dtype=bool)
        keep[np.asarray(queries, dtype=np.int64)] = True
        inside = inside & keep[None, :, None, None, None]
    t = np.zeros((B, S, H), dtype=bool)
    for l in range(L):
        Hl, Wl = int(shapes[l, 0]), int(shapes[l, 1])
        b, q, h, p = np.nonzero(inside[:, :, :, l])
        x0 = np.floor(x[b, q, h, l, p]).astype(np.int64)
        y0 = np.floor(y[b, q, h, l, p]).astype(np.int64)
        for dy in range(-margin, 2 + margin):
            for dx in range(-margin, 2 + margin):
                ys, xs = y0 + dy, x0 + dx
                ok = (ys >= 0) & (ys < Hl) & (xs >= 0) & (xs < Wl)
                t[b[ok], int(lsi[l]) + ys[ok] * Wl + xs[ok], h[ok]] = True
    return t


BLOCK_W, BLOCK_H = 8, 4         # the binned backward's blocks of pixels: a balanced partition of the map into
#                                 ceil(W / 8) x ceil(H / 4) blocks, pixel x in block column floor(x nbx / W)
#                                 (boxattn_binplan.h, blk_of)


def block_spread(shapes, loc, queries, S=None, lsi=None, groups=False):
    """(B, S, H) bool: every pixel of every 8 x 4 block that holds a corner (inside the map) of an in-window point of
    ``queries`` -- where the matrix-core accumulates put a non-finite upstream row of such a query (the
    documented deviation).  ``groups``: group records -- every block of the block range that the points of one
    (query, head, level) span."""
    shapes = np.asarray(shapes, dtype=np.int64)
    lsi0, S0 = tables(shapes)[1:]
    lsi = lsi0 if lsi is None else np.asarray(lsi, dtype=np.int64)
    S = S0 if S is None else int(S)
    x, y, inside = pixels(shapes, loc)
    B, Lq, H, L, P = x.shape
    t = np.zeros((B, S, H), dtype=bool)
    for l in range(L):
        Hl, Wl = int(shapes[l, 0]), int(shapes[l, 1])
        nbx, nby = -(-Wl // BLOCK_W), -(-Hl // BLOCK_H)
        for b in range(B):
            for q in queries:
                for h in range(H):
                    p = np.nonzero(inside[b, q, h, l])[0]
                    if not p.size:
                        continue
                    x0 = np.floor(x[b, q, h, l, p]).astype(np.int64)
                    y0 = np.floor(y[b, q, h, l, p]).astype(np.int64)
                    bx = np.concatenate([np.clip(x0, 0, Wl - 1), np.clip(x0 + 1, 0, Wl - 1)]) * nbx // Wl
                    by = np.concatenate([np.clip(y0, 0, Hl - 1), np.clip(y0 + 1, 0, Hl - 1)]) * nby // Hl
                    if groups:
                        cells = [(i, j) for j in range(by.min(), by.max() + 1) for i in range(bx.min(), bx.max() + 1)]
                    else:       # a point's blocks: the 2 x 2 (or fewer) its own corners fall into
                        n = p.size
                        cells = {(i, j) for k in range(n) for i in (bx[k], bx[n + k]) for j in (by[k], by[n + k])}
                    for i, j in cells:
                        ys = np.nonzero(np.arange(Hl) * nby // Hl == j)[0]
                        xs = np.nonzero(np.arange(Wl) * nbx // Wl == i)[0]
                        t[b, int(lsi[l]) + (ys[:, None] * Wl + xs[None, :]).ravel(), h] = True
    return t


def has_patch(level, edge):
    Hl, Wl = int(level[0]), int(level[1])
    along, across = (Hl, Wl) if edge in ("right", "left") else (Wl, Hl)
    return along >= MIN_ALONG and across >= MIN_ACROSS


def _patch(level, edge, rng, n):
    """n points (normalised x, y) of the patch of ``level`` astride ``edge``, at the edge's midpoint."""
    Hl, Wl = int(level[0]), int(level[1])
    across = rng.uniform(-ACROSS_PX, ACROSS_PX, n)
    along = rng.uniform(-ALONG_PX, ALONG_PX, n)
    if edge in ("right", "left"):
        # pixel coordinates: the border is at -0.5 (left) / W - 0.5 (right); the midpoint is the pixel row H // 2
        px = (Wl - 0.5 if edge == "right" else -0.5) + across
        py = Hl // 2 + along
    else:
        px = Wl // 2 + along
        py = (Hl - 0.5 if edge == "bottom" else -0.5) + across
    return np.stack([(px + 0.5) / Wl, (py + 0.5) / Hl], -1)


def victims_of(Lq):
    """Query 0, one in the middle and the last one (of batch 0)."""
    return sorted({0, Lq // 2, Lq - 1})


def edge_family(levels, Lq, P, edge, rng, B=2, H=2):
    """Locations (B, Lq, H, L, P, 2), float32 numbers held in float64.  On a level with a patch (has_patch) all points
    lie in one patch at the midpoint of ``edge``: +-1.4 px across the border, +-0.4 px along it -- points wholly inside,
    points with corners outside the map, points outside the window test.  The points of a smaller level lie more than a
    whole map outside: the level is never read.  The victim queries (victims_of; batch 0 only) sample the patch at the
    opposite edge instead.  -> dict(loc, victims, patch (L,) bool, edge, levels)."""
    assert edge in EDGES
    levels = [tuple(int(v) for v in lv) for lv in levels]
    L = len(levels)
    loc = np.empty((B, Lq, H, L, P, 2))
    victims = victims_of(Lq)
    for l, lv in enumerate(levels):
        if has_patch(lv, edge):
            loc[:, :, :, l] = _patch(lv, edge, rng, B * Lq * H * P).reshape(B, Lq, H, P, 2)
            loc[0, victims, :, l] = _patch(lv, OPPOSITE[edge], rng, len(victims) * H * P).reshape(len(victims), H, P, 2)
        else:
            loc[:, :, :, l] = FAR + rng.uniform(0.0, 1.0, (B, Lq, H, P, 2))
    loc = loc.astype(np.float32).astype(np.float64)
    return dict(loc=loc, victims=victims, patch=np.array([has_patch(lv, edge) for lv in levels]), edge=edge,
                levels=levels)


def level_rows(levels, l):
    lsi = tables(levels)[1]
    return slice(int(lsi[l]), int(lsi[l]) + int(levels[l][0]) * int(levels[l][1]))


def sentinels(levels, edge, S=None):
    """The rows (indices into S) a careless kernel would fetch and that an edge_family must leave unreferenced:
    -> {name: int64 array}."""
    shapes, lsi, S0 = tables(levels)
    S = S0 if S is None else S
    out = {}
    for l, lv in enumerate(levels):
        Hl, Wl = int(lv[0]), int(lv[1])
        base = int(lsi[l])
        if not has_patch(lv, edge):
            out["level %d: wholly unread" % l] = base + np.arange(Hl * Wl)
            continue
        out["level %d: first pixel" % l] = np.array([base])
        out["level %d: last pixel" % l] = np.array([base + Hl * Wl - 1])
        # the patch's image rows / columns: y0, y0 + 1 of +-0.4 px about the midpoint, widened by the margin
        rows = np.arange(Hl // 2 - 2, Hl // 2 + 3)
        cols = np.arange(Wl // 2 - 2, Wl // 2 + 3)
        # "flat: ..." is what a corner outside the map is when read at its flat index; in batch 0 the victims' patch at
        # the opposite edge (of this level, or of the neighbouring level) may hold some of those rows: there they are
        # sentinels of everyone but the victims
        if edge == "right":
            out["level %d: first pixel of the image row after the patch's" % l] = np.array([base + (rows[-1] + 1) * Wl])
            out["flat: level %d: (y, W), the next image row's first pixel" % l] = base + (rows[1:-1] + 1) * Wl
        elif edge == "left":
            out["level %d: last pixel of the image row before the patch's" % l] = np.array([base + rows[0] * Wl - 1])
            out["flat: level %d: (y, -1), the image row before's last pixel" % l] = base + rows[1:-1] * Wl - 1
        elif edge == "top" and l > 0:
            out["flat: level %d: the preceding level's last image row, at the patch's columns" % l] = \
                base - int(levels[l - 1][1]) + cols
            out["flat: level %d: (-1, x)" % l] = base - Wl + cols
        elif edge == "bottom" and l + 1 < len(levels):
            out["flat: level %d: (H, x), the following level's first image row at the patch's columns" % l] = \
                base + Hl * Wl + cols
    if S > S0:
        out["padded tail"] = np.arange(S0, S)
    return out


def problem(levels, Lq, P, edge, kind="box", B=2, H=2, C=32, pad=0, seed=0):
    """One edge_family case as float64 / int64 numpy arrays with the keys of error_bounds' input dictionaries.  value,
    grad_out and grad_mask are multiples of 1 / 64 below 2 (the same numbers in every storage type), the weights
    float32 numbers in (0, 1], none of them zero.  Lq "S": one query a pixel.  Also: fam (edge_family's dictionary),
    S0 (the levels' rows; ``pad`` more follow), touched / unreferenced (B, S, H) at margin 1, opposite (B, S, H): the
    widened footprint of the victims alone."""
    shapes, lsi, S = tables(levels, pad)
    S0 = S - pad
    Lq = S0 if Lq == "S" else int(Lq)
    L = len(levels)
    rng = np.random.default_rng([seed, EDGES.index(edge), Lq, P, S0])
    fam = edge_family(levels, Lq, P, edge, rng, B, H)
    grid = lambda *shape: rng.integers(-127, 128, shape).astype(np.float64) / 64.0
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    a = rng.uniform(0.05, 1.0, (B, Lq, H, L, P))
    g = dict(kind=kind, shapes=shapes, lsi=lsi, value=grid(B, S, H, C), loc=fam["loc"],
             attn=f32(a / a.sum((-1, -2), keepdims=True)), grad_out=grid(B, Lq, H * C), fam=fam, S0=S0, edge=edge,
             victims=fam["victims"])
    if kind == "instance":
        t = rng.uniform(0.05, 1.0, (B, Lq, H, L, P))
        g["level_w"] = f32(t / t.sum(-2, keepdims=True))
        g["spatial_w"] = g["attn"]
        g["grad_mask"] = grid(B, Lq, P, H * C)
    g["touched"] = touched(shapes, g["loc"], 1, S, lsi)
    g["unreferenced"] = ~g["touched"]
    opp = touched(shapes, g["loc"][:1], 1, S, lsi, queries=fam["victims"])
    g["opposite"] = np.concatenate([opp, np.zeros((B - 1,) + opp.shape[1:], dtype=bool)], 0)
    return g


BOX_ACROSS_PX, BOX_ALONG_PX = 1.0, 0.4       # a box's size in pixels: its points stay within +-0.5 / +-0.2 px of its centre
QUARTER_TURN, HALF_TURN = 0.25, float(np.float32(np.pi))


def boxes_problem(levels, Lq, k, edge, kind="box", B=2, H=2, C=32, pad=0, angle_mode=0, ref_dim=4, per_head=False,
                  with_vr=False, seed=0):
    """The edge family through reference windows: every (b, q, h, l) gets one box whose k x k points lie inside the
    patch of edge_family (its centre within +-0.9 px across the border and +-0.2 px along it, 1.0 x 0.4 px in size), the
    boxes of a level without a patch more than a whole map outside, the victims' boxes at the opposite edge.  The
    reference window of a query (or of a (query, head)) is its box on level 0, so that level's offsets are 0 for head 0;
    the other levels' offsets move and resize it.  angle_mode 1: a quarter turn (ref[4] = 0.25, offset 0), 2: half a turn
    (ref[4] = pi); the box's sides are chosen so that the rotated points fill the same patch.  with_vr: valid ratios in
    [0.5, 1], divided out of the boxes.  ``touched`` is computed from the model's locations (error_bounds.grid_reference
    on the float32 operands), never assumed.  -> problem()'s dictionary plus ref, off, kidx, vr, logits, angle_mode;
    loc / attn (and level_w): the model's, float64."""
    import error_bounds as eb
    from boxer_amd.modules import _kernel_offsets
    shapes, lsi, S = tables(levels, pad)
    S0 = S - pad
    Lq = S0 if Lq == "S" else int(Lq)
    L, P = len(levels), k * k
    V = 5 if angle_mode == 1 else 4
    rng = np.random.default_rng([seed, EDGES.index(edge), Lq, P, S0, angle_mode, ref_dim, per_head, with_vr])
    victims = victims_of(Lq)
    vr = rng.uniform(0.5, 1.0, (B, 1, 1, L, 1, 2)).astype(np.float32) if with_vr else None
    box = np.empty((B, Lq, H, L, 4))                    # cx, cy, extent along x, extent along y of the points: normalised
    for l, lv in enumerate(levels):
        Hl, Wl = int(lv[0]), int(lv[1])

        def boxes(e, n):
            across, along = rng.uniform(-0.9, 0.9, n), rng.uniform(-0.2, 0.2, n)
            if e in ("right", "left"):
                px, py = (Wl - 0.5 if e == "right" else -0.5) + across, Hl // 2 + along
                ex, ey = BOX_ACROSS_PX, BOX_ALONG_PX
            else:
                px, py = Wl // 2 + along, (Hl - 0.5 if e == "bottom" else -0.5) + across
                ex, ey = BOX_ALONG_PX, BOX_ACROSS_PX
            return np.stack([(px + 0.5) / Wl, (py + 0.5) / Hl, np.full(n, ex / Wl), np.full(n, ey / Hl)], -1)
        if has_patch(lv, edge):
            box[:, :, :, l] = boxes(edge, B * Lq * H).reshape(B, Lq, H, 4)
            box[0, victims, :, l] = boxes(OPPOSITE[edge], len(victims) * H).reshape(len(victims), H, 4)
        else:
            box[:, :, :, l, :2] = FAR + rng.uniform(0.0, 1.0, (B, Lq, H, 2))
            box[:, :, :, l, 2:] = 1.0 / Wl, 1.0 / Hl
    if vr is not None:                                  # the grid is multiplied by the valid ratios last
        r = vr.astype(np.float64)[:, :, :, :, 0]        # (B, 1, 1, L, 2)
        box = np.concatenate([box[..., :2] / r, box[..., 2:] / r], -1)
    if angle_mode == 1:                                 # a quarter turn: x = cx - ly, y = cy + lx
        box = box[..., [0, 1, 3, 2]]
    ref = np.empty((B, Lq, H, ref_dim))
    ref[..., :4] = box[:, :, :, 0]
    if ref_dim > 4:
        ref[..., 4:] = rng.uniform(-3.0, 3.0, (B, Lq, H, ref_dim - 4))
        ref[..., 4] = {0: ref[..., 4], 1: QUARTER_TURN, 2: HALF_TURN}[angle_mode]
    if not per_head:
        ref = ref[:, :, 0]
    ref = ref.astype(np.float32)
    r64 = ref.astype(np.float64)
    r64 = r64[:, :, None, None] if not per_head else r64[:, :, :, None]         # (B, Lq, 1 | H, 1, D)
    off = np.zeros((B, Lq, H, L, V))
    off[..., :2] = 8.0 * (box[..., :2] - r64[..., :2]) / r64[..., 2:4]
    off[..., 2:4] = 8.0 * (box[..., 2:] / r64[..., 2:4] - 1.0)
    off[:, :, slice(None) if per_head else 0, 0, :4] = 0.0        # (the window IS that box, up to its rounding to float32)
    off = off.astype(np.float32)
    kidx = _kernel_offsets(k, k).float().numpy()
    grid = lambda *shape: rng.integers(-127, 128, shape).astype(np.float64) / 64.0
    loc = eb.grid_reference(ref, off, kidx, vr, angle_mode)[0]
    g = dict(kind=kind, shapes=shapes, lsi=lsi, value=grid(B, S, H, C), loc=loc, grad_out=grid(B, Lq, H * C), S0=S0,
             edge=edge, victims=victims, ref=ref, off=off, kidx=kidx, vr=vr, angle_mode=angle_mode, k=k,
             dims=(B, S, H, C, L, Lq, P))
    if kind == "instance":
        g["logits"] = rng.standard_normal((B, Lq, H, L, 2, 2)).astype(np.float32)
        g["attn"], g["level_w"] = eb.instance_weights_reference(g["logits"], k)[:2]
        g["spatial_w"] = g["attn"]
        g["grad_mask"] = grid(B, Lq, P, H * C)
    else:
        g["logits"] = rng.standard_normal((B, Lq, H, L * P)).astype(np.float32)
        g["attn"] = eb.softmax_reference(g["logits"])[0].reshape(B, Lq, H, L, P)
    g["touched"] = touched(shapes, loc, 1, S, lsi)
    g["unreferenced"] = ~g["touched"]
    opp = touched(shapes, loc[:1], 1, S, lsi, queries=victims)
    g["opposite"] = np.concatenate([opp, np.zeros((B - 1,) + opp.shape[1:], dtype=bool)], 0)
    return g


def victim_triples(g, heads=None):
    """(B, Lq, H) bool: (0, victims, heads) (default: every head)."""
    B, Lq, H = g["loc"].shape[:3]
    m = np.zeros((B, Lq, H), dtype=bool)
    m[0, g["victims"]] = True
    if heads is not None:
        keep = np.zeros(H, dtype=bool)
        keep[list(heads)] = True
        m &= keep
    return m


# ------------------------------------------------------------------ the check
def _bits(a):
    """Any float array / tensor -> (unsigned integer numpy array of its bits, bool numpy array: finite)."""
    if not isinstance(a, np.ndarray):                  # a torch tensor
        import torch
        a = a.detach().contiguous()
        finite = torch.isfinite(a).cpu().numpy()
        ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return a.view(ints).cpu().numpy(), finite
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize]), np.isfinite(a)


def isolated(name, clean, poisoned, exempt=None, what=""):
    """The poisoned run's ``name`` against the clean run's: outside ``exempt`` (bool, broadcastable; what was poisoned on
    purpose or depends on it by the definition) the clean result is finite and the poisoned one is the same, bit for
    bit.  -> the number of elements compared; AssertionError names the first leak."""
    cb, cf = _bits(clean)
    pb, pf = _bits(poisoned)
    assert cb.shape == pb.shape, "%s %s: shapes %r / %r" % (what, name, cb.shape, pb.shape)
    held = np.ones(cb.shape, dtype=bool) if exempt is None else ~np.broadcast_to(np.asarray(exempt, dtype=bool), cb.shape)
    bad = held & ~cf
    assert not bad.any(), "%s %s: the clean run itself is not finite at %s" % (
        what, name, tuple(int(i) for i in np.argwhere(bad)[0]))
    leak = held & ~pf
    assert not leak.any(), "%s %s: %d of %d elements are not finite although nothing they depend on is; first at %s" % (
        what, name, int(leak.sum()), int(held.sum()), tuple(int(i) for i in np.argwhere(leak)[0]))
    diff = held & (cb != pb)
    assert not diff.any(), "%s %s: %d of %d elements differ from the clean run; first at %s" % (
        what, name, int(diff.sum()), int(held.sum()), tuple(int(i) for i in np.argwhere(diff)[0]))
    return int(held.sum())


def finite_outside(name, got, may=None, what=""):
    """Every element of ``got`` outside ``may`` (bool, broadcastable) is finite."""
    f = _bits(got)[1]
    held = np.ones(f.shape, dtype=bool) if may is None else ~np.broadcast_to(np.asarray(may, dtype=bool), f.shape)
    bad = held & ~f
    assert not bad.any(), "%s %s: %d of %d elements are not finite although nothing they depend on is; first at %s" % (
        what, name, int(bad.sum()), int(held.sum()), tuple(int(i) for i in np.argwhere(bad)[0]))
    return int(held.sum())


def spread(name, shape, bqh):
    """A (B, Lq, H) bool mask over the (b, q, h) triples -> the elements of output ``name`` that belong to them.
    out (B, Lq, H C), mask_out (B, Lq, P, H C); every other output (B, Lq, H, ...), or (B, Lq, ...) where the heads
    share it (then: any head)."""
    bqh = np.asarray(bqh, dtype=bool)
    B, Lq, H = bqh.shape
    shape = tuple(shape)
    if name == "out":
        return np.broadcast_to(bqh[..., None], (B, Lq, H, shape[-1] // H)).reshape(shape)
    if name == "mask_out":
        return np.broadcast_to(bqh[:, :, None, :, None], (B, Lq, shape[2], H, shape[-1] // H)).reshape(shape)
    if len(shape) >= 3 and shape[:3] == (B, Lq, H):
        return np.broadcast_to(bqh.reshape((B, Lq, H) + (1,) * (len(shape) - 3)), shape)
    assert shape[:2] == (B, Lq), (name, shape)
    return np.broadcast_to(bqh.any(-1).reshape((B, Lq) + (1,) * (len(shape) - 2)), shape)


def check_outputs(clean, got, bqh=None, bsh=None, grad_value="equal", what=""):
    """Every output of the poisoned run ``got`` against the clean run: bitwise equal outside the (b, q, h) triples
    ``bqh`` (B, Lq, H) -- and, for grad_value (B, S, H, C), outside the rows ``bsh`` (B, S, H).  grad_value: "equal"
    (an ordered sum), "finite" (only that: an unordered sum; the caller holds it to a tolerance), or "skip".
    -> the number of elements held."""
    n = 0
    for name, t in got.items():
        if t is None:
            continue
        if name == "grad_value":
            ex = None if bsh is None else np.asarray(bsh, dtype=bool)[..., None]
            if grad_value == "equal":
                n += isolated(name, clean[name], t, ex, what)
            elif grad_value == "finite":
                n += finite_outside(name, t, ex, what)
            continue
        n += isolated(name, clean[name], t, None if bqh is None else spread(name, t.shape, bqh), what)
    return n


# ------------------------------------------------------------------ poison
def poison_rows(value, unreferenced):
    """A copy of value (B, S, H, C) (numpy or tensor) with NaN in every row (b, s, h) of ``unreferenced`` (B, S, H)."""
    if isinstance(value, np.ndarray):
        v = value.copy()
        v[unreferenced] = np.nan
        return v
    import torch
    v = value.clone()
    v[torch.from_numpy(np.ascontiguousarray(unreferenced)).to(v.device)] = float("nan")
    return v


def share(unreferenced):
    return float(np.mean(unreferenced))


# ------------------------------------------------------------------ arenas
class Arena:
    """``view``: a contiguous tensor inside ``buf`` (uint8) with GUARD bytes on either side."""

    def __init__(self, buf, start, nbytes, view, byte):
        self.buf, self.start, self.nbytes, self.view, self.byte = buf, start, nbytes, view, byte

    def guards(self):
        return self.buf[:self.start], self.buf[self.start + self.nbytes:]


def arena(shape, dtype, device, byte=GUARD_BYTE, align=16, like=None):
    """A tensor of ``shape`` / ``dtype`` as a view ``align`` bytes aligned inside a buffer whose every other byte is
    ``byte``.  ``like``: the view's contents (a tensor of the same shape); else the view holds ``byte`` too."""
    import torch
    shape = tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = int(np.prod(shape, dtype=np.int64)) * item
    buf = torch.full((GUARD + nbytes + GUARD + align,), byte, dtype=torch.uint8, device=device)
    start = GUARD + (-(buf.data_ptr() + GUARD)) % align
    view = buf[start:start + nbytes].view(dtype).view(shape)
    assert view.data_ptr() % align == 0 and view.is_contiguous()
    if like is not None:
        view.copy_(like)
    return Arena(buf, start, nbytes, view, byte)


def input_arena(t, align=16):
    """A float input surrounded by NaN; an integer one by GUARD_BYTE."""
    return arena(t.shape, t.dtype, t.device, NAN_BYTE if t.is_floating_point() else GUARD_BYTE, align, like=t)


def guards_intact(a):
    """Every guard byte of the arena still holds what it was filled with."""
    return all(bool((g == a.byte).all().item()) for g in a.guards())


ENCODER = [(13, 13), (7, 5)]
DECODER = [(20, 30), (10, 15), (5, 8), (3, 4)]
WIDE_LEVELS = [(11, 9), (6, 5), (3, 2)]

STAGED_LEVELS = [(37, 23), (19, 12), (10, 6), (5, 3)]


BOX_FLAVOURS = [(0, 4), (1, 5), (1, 7), (2, 5)]                  # angle mode, values a reference window
STAGED_GEOMETRY = {"four_levels": (STAGED_LEVELS, 2, 3), "one_level": ([(9, 13)], 2, 1),
                   "tiny_levels": ([(4, 5), (2, 3), (1, 1)], 1, 2)}
