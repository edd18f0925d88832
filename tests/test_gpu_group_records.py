"""GPU tests of the binned backward's group records (option key 24, boxer_amd/csrc/boxattn_binplan.h: group_blocks): 16-bit
box attention with P = 4 writes one 4-byte record per (query, level, block) and the matrix-core accumulate gathers the
group's locations and weights by id.  Every case checks grad_value, grad_loc and grad_attn of key 24 = 2

  * against the C oracle with the suite's helpers for the storage type (compare_rules.close_parity for bf16,
    compare_rules.check_f16 for f16);
  * against the same call under key 24 = 1 (point records): grad_loc / grad_attn come from the same launch and are
    bitwise equal, grad_value is held to the suite's run-to-run bound (test_gpu_onepass.test_soak_over_changing_inputs:
    tol x max(1, max |ref|) with the storage type's oracle tolerance).

The ratio of the two routes' worst grad_value errors is printed, not asserted: both multiply the same two-term weights in
float32, only the order of summation differs (sums of coinciding corners are formed before the hi / lo split).
"""
import numpy as np
import pytest
import torch

from point_cases import (EACH_16BIT_DTYPE as DTYPES, RUN_TO_RUN, backward, both_routes, check_oracle, check_routes,
                         counters, f64, make)
from route_vocab import BF16, KEY_GROUP, KEY_POINT

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _reset():
    from boxer_amd import _lib, ops
    ops.release_workspaces()
    yield
    _lib.set_option("group_records", 0)
    ops.release_workspaces()


# ------------------------------------------------------------------ encoder, odd maps: cold, then the one-pass riders
@DTYPES
def test_encoder_odd_maps_cold_then_one_pass(dtype):
    """(13, 13), (7, 7): every edge block is partial.  First call on a fresh state: two-pass.  Second and third call, on
    new inputs: the one-pass riders -- their chain ran once per (image, head) slice and call."""
    sets = [make([(13, 13), (7, 7)], "S", dtype=dtype, seed=s) for s in (1, 2, 3)]
    ns = sets[0]["dims"]["B"] * sets[0]["dims"]["H"]
    seen = both_routes(sets, "encoder")
    assert seen[0] == (0, 0), "a cold state runs the two-pass passes"
    assert seen[1][0] == ns and seen[2][0] == 2 * ns, "the one-pass riders ran: %r" % (seen,)


# ------------------------------------------------------------------ boundary groups
def boundary_case(dtype):
    """Hand-placed boxes on (16, 16), (8, 8) -- blocks of 8 x 4 pixels: block edges at x = 8 and y = 4, 8, 12 of level 0."""
    base = make([(16, 16), (8, 8)], 12, dtype=dtype, B=1, H=2, seed=5)
    # (centre x, centre y, size) in pixels of level 0; the points are the corners centre +- size / 2
    boxes = [(8.0, 2.3, 2.0),        # straddles a block edge in x
             (3.3, 4.1, 1.5),        # ... in y
             (8.1, 3.9, 1.5),        # a block corner: four blocks
             (5.3, 6.7, 0.0),        # size 0: all 16 corners on one pixel quad
             (5.0, 6.0, 0.0),        # size 0, exactly on a pixel centre
             (9.0, 5.0, 2.0),        # centred exactly on a pixel centre
             (0.2, 0.3, 3.0),        # partly outside: negative coordinates
             (-5.0, -5.0, 2.0),      # wholly outside, negative
             (15.6, 15.7, 2.0),      # partly outside at the far corner
             (20.0, 20.0, 2.0),      # wholly outside, beyond the map
             (8.0, 8.0, 14.0),       # wide: more than 2 x 2 blocks -- the slow path
             (7.9, 11.9, 0.5)]       # a small box on a block corner
    loc = torch.empty_like(base["loc"])                      # (1, 12, 2, 2, 4, 2)
    sign = torch.tensor([[-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0], [1.0, 1.0]], device=loc.device)
    for q, (cx, cy, sz) in enumerate(boxes):
        for l, (scale, n) in enumerate(((1.0, 16.0), (0.5, 8.0))):
            ctr = torch.tensor([cx, cy], device=loc.device) * scale
            pix = ctr + sign * (sz * scale / 2)
            loc[0, q, :, l] = (pix + 0.5) / n                # pixel coordinate = loc * size - 0.5
    base["loc"] = loc.contiguous()
    return base


@DTYPES
def test_boundary_groups(dtype):
    both_routes([boundary_case(dtype)], "boundary groups")


@DTYPES
def test_boundary_groups_through_the_one_pass_fill(dtype):
    """The same hand-placed boxes as the first twelve queries of an encoder-shaped call (one query per pixel of (16, 16),
    (8, 8)): cold, then twice through the one-pass riders' rank / claim / store."""
    enc = make([(16, 16), (8, 8)], "S", dtype=dtype, B=1, H=2, seed=6)
    hand = boundary_case(dtype)
    enc["loc"][:, :hand["loc"].size(1)] = hand["loc"]
    ns = enc["dims"]["B"] * enc["dims"]["H"]
    seen = both_routes([enc, enc, enc], "boundary groups, one-pass")
    assert seen[0] == (0, 0) and seen[1][0] == ns and seen[2][0] == 2 * ns, "the one-pass riders ran: %r" % (seen,)


# ------------------------------------------------------------------ slow path and mixture
def decision(inp):
    """group_blocks in numpy: per (b, q, h, level) group -> 0 no record, 1 fast, 2 slow."""
    shapes = inp["shapes"].cpu().numpy()
    loc = f64(inp["loc"].float())
    out = np.zeros(loc.shape[:4], dtype=np.int64)
    for l, (H, W) in enumerate(shapes):
        nby, nbx = (H + 3) // 4, (W + 7) // 8
        x = (loc[:, :, :, l, :, 0].astype(np.float32) * np.float32(W) - np.float32(0.5)).astype(np.float64)
        y = (loc[:, :, :, l, :, 1].astype(np.float32) * np.float32(H) - np.float32(0.5)).astype(np.float64)
        ok = (y > -1) & (x > -1) & (y < H) & (x < W)
        y0, x0 = np.floor(np.where(ok, y, 0)).astype(np.int64), np.floor(np.where(ok, x, 0)).astype(np.int64)
        big = 1 << 30
        ylo = np.where(ok, np.maximum(y0, 0), big).min(-1); yhi = np.where(ok, np.minimum(y0 + 1, H - 1), 0).max(-1)
        xlo = np.where(ok, np.maximum(x0, 0), big).min(-1); xhi = np.where(ok, np.minimum(x0 + 1, W - 1), 0).max(-1)
        some = ok.any(-1)
        ylo, xlo = np.where(some, ylo, 0), np.where(some, xlo, 0)
        wide = ((yhi * nby) // H - (ylo * nby) // H > 1) | ((xhi * nbx) // W - (xlo * nbx) // W > 1)
        out[:, :, :, l] = np.where(some, np.where(wide, 2, 1), 0)
    return out


@DTYPES
def test_model_and_uniform_mixture(dtype):
    """Half the queries model-like, half i.i.d. uniform, on (16, 16), (8, 8): fast and slow groups side by side."""
    levels = [(16, 16), (8, 8)]
    model = make(levels, "S", "model", dtype, seed=7)
    test = make(levels, "S", "test", dtype, seed=8)
    odd = (torch.arange(model["loc"].size(1), device="cuda") % 2 == 1)
    mix = dict(model)
    mix["loc"] = torch.where(odd[None, :, None, None, None, None], test["loc"], model["loc"]).contiguous()
    mix["attn"] = torch.where(odd[None, :, None, None, None], test["attn"], model["attn"]).contiguous()
    d = decision(mix)
    fast, slow = float((d == 1).mean()), float((d == 2).mean())
    print("mixture: %.1f %% of the groups fast, %.1f %% slow" % (100 * fast, 100 * slow))
    assert fast >= 0.1 and slow >= 0.1
    both_routes([mix, mix], "mixture")


@DTYPES
def test_rotated_windows(dtype):
    """Rotated windows (a learned angle per box, as the 3D encoder builds them): groups that are no axis-parallel 2 x 2."""
    inp = make([(16, 16), (8, 8)], "S", "model", dtype, seed=9, kind="box3d")
    both_routes([inp, inp], "rotated")


# ------------------------------------------------------------------ one live state under both record kinds
def test_key_24_flipped_on_one_live_state():
    """Ranges a state learned under one record kind count other records: they must read as cold under the other.  One
    state buffer, never released: group, group (one-pass), point (cold again: no chain), point (one-pass), group (cold),
    group (one-pass) -- every call the oracle's tensors, and the routes agree on the same inputs."""
    from boxer_amd import ops
    sets = [make([(13, 13), (7, 7)], "S", dtype=BF16, seed=s) for s in (31, 32)]
    ns = sets[0]["dims"]["B"] * sets[0]["dims"]["H"]
    ops.release_workspaces()
    got, chain = {}, []
    for i, key in enumerate((KEY_GROUP, KEY_GROUP, KEY_POINT, KEY_POINT, KEY_GROUP, KEY_GROUP)):
        inp = sets[i % 2]
        before = counters()[0]
        grads = backward(inp, key)
        chain.append(counters()[0] - before)
        check_oracle(inp, grads, "live state, call %d (key 24 = %d)" % (i, key))
        got[(i % 2, key)] = grads
    assert chain == [0, ns, 0, ns, 0, ns], "a flip of the record kind is a cold call, the call after it one pass: %r" % (chain,)
    for k in (0, 1):
        check_routes(sets[k], got[(k, KEY_GROUP)], got[(k, KEY_POINT)], "live state, set %d" % k)


# ------------------------------------------------------------------ decoder shape: two-pass riders
@DTYPES
def test_decoder_shape(dtype):
    """Lq = 37 != S, L = 2: too few records a block for the one-pass fill -- the two-pass riders, every call."""
    sets = [make([(20, 30), (10, 15)], 37, dtype=dtype, seed=s) for s in (11, 12)]
    seen = both_routes(sets, "decoder")
    assert seen[-1] == (0, 0), "no one-pass chain at decoder shapes"


# ------------------------------------------------------------------ degenerate distributions
def test_degenerate_record_distributions():
    """As test_gpu_onepass.test_degenerate_record_distributions: no record at all, every point in ONE block (its range was
    planned for none: redone, then planned: chunked items and their combine), ordinary data again."""
    base = make([(20, 30), (10, 15)], "S", dtype=BF16, seed=13)
    outside = dict(base, loc=(base["loc"] * 0 + 7.5).contiguous())
    one_block = dict(base, loc=(base["loc"] * 0.02 + 0.4).contiguous())
    for d in (outside, one_block):
        d.pop("_want", None)
    seq = [base, base, outside, outside, one_block, one_block, one_block, base, base]
    seen = both_routes(seq, "degenerate")
    redone = [s[1] for s in seen]
    assert redone[4] > redone[3], "every point in one block: its range was planned for none -- the redo workers"
    assert redone[6] == redone[5], "planned by the same data: nothing to redo"
    assert redone[8] == redone[7], redone


# ------------------------------------------------------------------ key 24 touches nothing else
def _same(a, b, dtype, what):
    if torch.equal(a, b):
        return
    err = (a.float() - b.float()).abs().max().item()
    assert err <= RUN_TO_RUN[dtype] * max(1.0, b.float().abs().max().item()), (what, err)


def test_float32_and_instance_do_not_read_the_key():
    from boxer_amd import _lib, ops
    f32 = make([(13, 13), (7, 7)], "S", dtype=torch.float32, seed=21)
    inst = make([(13, 13), (7, 7)], 37, dtype=BF16, seed=22, kind="instance")
    got = {}
    for key in (KEY_POINT, KEY_GROUP, KEY_POINT):           # (the third run: do two runs of ONE key agree bitwise?)
        ops.release_workspaces()
        _lib.set_option("group_records", key)
        assert ops.backward_record_kind(f32["value"], f32["loc"]) == _lib.REC_POINT
        assert ops.backward_record_kind(inst["value"], inst["loc"], instance=True) == _lib.REC_POINT
        v, sh, ls, loc, attn, go = (f32[k] for k in ("value", "shapes", "lsi", "loc", "attn", "grad_out"))
        a = ops.box_attn_backward(v, sh, ls, loc, attn, go, 64)
        v, sh, ls, loc, sw, lw, go, gm = (inst[k] for k in ("value", "shapes", "lsi", "loc", "attn", "level_w", "grad_out",
                                                            "grad_mask"))
        b = ops.instance_attn_backward(v, sh, ls, loc, sw, lw, go, gm, 64)
        torch.cuda.synchronize()
        got.setdefault(key, []).append((list(a), list(b)))
    (p0a, p0b), (p1a, p1b) = got[KEY_POINT]
    ga, gb = got[KEY_GROUP][0]
    for what, p0, p1, g, dtype in (("float32 box", p0a, p1a, ga, torch.float32), ("bf16 instance", p0b, p1b, gb, BF16)):
        for i, (x0, x1, y) in enumerate(zip(p0, p1, g)):
            if torch.equal(x0, x1):                      # two runs of one key agree bitwise: so must the other key
                assert torch.equal(x0, y), "%s: output %d changes with key 24" % (what, i)
            else:
                _same(y, x0, dtype if i == 0 else torch.float32, "%s output %d" % (what, i))
