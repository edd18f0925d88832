"""GPU tests of the group-record accumulate's round (boxer_amd/csrc/boxattn_binned_tr.h, the GRP branch): the aligned 2 x 2
path -- a wave whose groups are all axis-parallel grids locates two rows and two columns instead of eight coordinates --, its
fall-back when one lane is not aligned, and the shortened last round of an item (ceil(remaining / 16) K-steps).

Every case runs key 24 = 2 (group records) and checks grad_value, grad_loc and grad_attn against the C oracle and against the
point-record route (key 24 = 1) with the helpers and tolerances of test_gpu_group_records; H = 2, C = 32, B = 2 unless said.
"""
import numpy as np
import pytest
import torch

from point_cases import EACH_16BIT_DTYPE as DTYPES, RUN_TO_RUN, backward, both_routes, make
from route_vocab import BF16, KEY_GROUP

pytestmark = pytest.mark.gpu

LEVELS = [(16, 16), (8, 8)]
SIGN = [[-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0], [1.0, 1.0]]       # points 0, 1 share y; 0, 2 share x


@pytest.fixture(autouse=True)
def _reset():
    from boxer_amd import _lib, ops
    ops.release_workspaces()
    yield
    _lib.set_option("group_records", 0)
    ops.release_workspaces()


def aligned(loc):
    """Which (b, q, h, level) groups are axis-parallel 2 x 2 grids bit for bit -- what the kernel tests per lane."""
    w = loc.contiguous().view(torch.int32)
    return ((w[..., 0, 0] == w[..., 2, 0]) & (w[..., 1, 0] == w[..., 3, 0]) &
            (w[..., 0, 1] == w[..., 1, 1]) & (w[..., 2, 1] == w[..., 3, 1]))


def place(inp, per_level, first=0):
    """Hand-placed boxes for the queries first, first + 1, ...: per_level[l] lists (centre x, centre y, size) in pixels of
    level l; the four points are the corners centre +- size / 2 (the same float32 sum for the points that share it)."""
    shapes = inp["shapes"].cpu().numpy()
    loc = inp["loc"].clone()
    sign = torch.tensor(SIGN, device=loc.device)
    for l, boxes in enumerate(per_level):
        H, W = (float(v) for v in shapes[l])
        wh = torch.tensor([W, H], device=loc.device)
        for q, (cx, cy, sz) in enumerate(boxes):
            pix = torch.tensor([cx, cy], device=loc.device) + sign * (sz / 2)
            loc[:, first + q, :, l] = (pix + 0.5) / wh                # pixel coordinate = loc * size - 0.5
    out = dict(inp, loc=loc.contiguous())
    out.pop("_want", None)
    return out


# ------------------------------------------------------------------ the aligned path
@DTYPES
def test_aligned_model_boxes(dtype):
    inp = make(LEVELS, "S", "model", dtype, seed=41)
    assert bool(aligned(inp["loc"]).all()), "model-like grids share their x and y bit for bit"
    both_routes([inp, inp], "aligned")


def test_aligned_model_boxes_16_channels():
    inp = make(LEVELS, "S", "model", BF16, C=16, seed=42)
    assert bool(aligned(inp["loc"]).all())
    both_routes([inp, inp], "aligned, C = 16")


# ------------------------------------------------------------------ one lane of a wave not aligned: the whole wave falls back
@DTYPES
def test_mixed_wave_falls_back(dtype):
    """Every 16th query's point 1 is moved by 1 ulp in x -- about four such groups in every round of 64 --: the oracle and
    the point route on the moved inputs.  Then the same move on a point whose weight is zero: it adds nothing anywhere, so
    the per-point code the wave falls back to must give what the aligned path gives on the inputs without the move --
    bitwise where two runs of one input agree bitwise, else within the suite's run-to-run bound."""
    base = make(LEVELS, "S", "model", dtype, seed=43)
    q = torch.arange(0, base["loc"].size(1), 16, device="cuda")

    def nudged(inp):
        loc = inp["loc"].clone()
        x = loc[:, q, :, :, 1, 0]
        loc[:, q, :, :, 1, 0] = torch.nextafter(x, torch.full_like(x, 2.0))
        out = dict(inp, loc=loc.contiguous())
        out.pop("_want", None)
        return out

    mixed = nudged(base)
    ok = aligned(mixed["loc"])
    assert not bool(ok[:, q].any()) and float(ok.float().mean()) > 0.9
    both_routes([mixed, mixed], "mixed wave")

    from boxer_amd import ops
    attn = base["attn"].clone()
    attn[:, q, :, :, 1] = 0.0
    zero = dict(base, attn=attn.contiguous())
    zero.pop("_want", None)
    got = []
    for inp in (zero, zero, nudged(zero)):
        ops.release_workspaces()
        got.append(backward(inp, KEY_GROUP)[0])
    if torch.equal(got[0], got[1]):
        assert torch.equal(got[0], got[2]), "the fall-back differs from the aligned path"
    else:
        err = (got[0].float() - got[2].float()).abs().max().item()
        assert err <= RUN_TO_RUN[dtype] * max(1.0, got[0].float().abs().max().item()), err


# ------------------------------------------------------------------ never aligned
@DTYPES
def test_iid_locations(dtype):
    inp = make(LEVELS, "S", "test", dtype, seed=44)
    assert not bool(aligned(inp["loc"]).any())
    both_routes([inp, inp], "i.i.d.")


# ------------------------------------------------------------------ collisions on a block corner
@DTYPES
def test_collisions_on_a_block_corner(dtype):
    """Boxes of size 0, 0.3 px and 1 px whose footprint covers the pixels on both sides of a block corner (blocks of 8 x 4
    pixels: x = 7 | 8, y = 3 | 4 and 7 | 8 of level 0): each of the four blocks of the 2 x 2 range gets a record, and up to
    sixteen corners fall on one pixel quad."""
    base = make(LEVELS, 12, "model", dtype, seed=45)
    lv0 = [(7.5, 3.5, 0.0), (7.5, 3.5, 0.3), (7.5, 3.5, 1.0), (7.7, 3.8, 0.0), (7.3, 7.6, 0.3), (7.5, 7.5, 1.0),
           (7.0, 3.0, 0.0), (7.99, 3.99, 0.0), (7.5, 11.5, 0.3), (7.2, 11.3, 1.0), (7.9, 3.1, 0.3), (7.5, 3.5, 0.999)]
    lv1 = [(7.5, 3.5, 0.0), (7.5, 3.5, 0.3), (7.5, 3.5, 1.0), (7.7, 3.8, 0.0), (6.9, 3.6, 0.3), (7.2, 3.2, 1.0),
           (7.0, 3.0, 0.0), (7.99, 3.99, 0.0), (7.1, 3.9, 0.3), (7.4, 3.3, 1.0), (7.9, 3.1, 0.3), (7.5, 3.5, 0.999)]
    inp = place(base, [lv0, lv1])
    assert bool(aligned(inp["loc"]).all())
    both_routes([inp], "collisions")
    enc = make(LEVELS, "S", "model", dtype, seed=46)          # ... and as the first queries of an encoder-shaped call
    enc = place(enc, [lv0, lv1])
    both_routes([enc, enc], "collisions, encoder")


# ------------------------------------------------------------------ round and K-step boundaries
ROUND_LQ = 192


def round_case(n, dtype):
    """One level (8, 8): two blocks of 8 x 4 pixels.  n queries' boxes lie wholly inside block 0 (rows 0-3), the other
    192 - n wholly inside block 1: items of n and of 192 - n records in every slice."""
    base = make([(8, 8)], ROUND_LQ, "model", dtype, seed=50 + n)
    g = torch.Generator().manual_seed(n)
    cx = 1.5 + 4.0 * torch.rand(ROUND_LQ, generator=g)
    cy = 1.0 + 0.9 * torch.rand(ROUND_LQ, generator=g)        # rows floor(cy - 0.5) .. floor(cy + 0.5) + 1 <= 3
    sz = torch.rand(ROUND_LQ, generator=g)
    cy[n:] += 4.0
    return place(base, [[(float(cx[i]), float(cy[i]), float(sz[i])) for i in range(ROUND_LQ)]])


@DTYPES
@pytest.mark.parametrize("n", [1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 129])
def test_round_and_k_step_boundaries(n, dtype):
    """The cold two-pass call, then the one-pass fill twice (the ranges the first call planned)."""
    inp = round_case(n, dtype)
    ns = inp["dims"]["B"] * inp["dims"]["H"]
    seen = both_routes([inp, inp, inp], "n = %d" % n)
    assert seen[0] == (0, 0), "a cold state runs the two-pass passes"
    assert seen[1][0] == ns and seen[2][0] == 2 * ns, "the one-pass riders ran: %r" % (seen,)


# ------------------------------------------------------------------ edge blocks
@DTYPES
def test_edge_blocks(dtype):
    """Maps (13, 13) and (7, 5): the last block row and column are partial blocks (bh < 4, bw < 8).  Points on the last row
    and column, half outside (some points of a group fail the window test: a mask that is not all four), and wholly
    outside."""
    enc = make([(13, 13), (7, 5)], "S", "model", dtype, seed=47)
    lv0 = [(12.0, 12.0, 1.0), (12.6, 3.0, 0.0), (13.2, 6.0, 1.0), (-0.7, -0.7, 1.0), (6.0, 12.9, 0.5), (-3.0, -3.0, 1.0),
           (20.0, 20.0, 2.0), (12.0, 12.0, 0.0), (12.5, 12.5, 1.2), (7.5, 12.0, 0.3)]
    lv1 = [(4.0, 6.0, 1.0), (4.6, 2.0, 0.0), (5.2, 3.0, 1.0), (-0.7, -0.7, 1.0), (2.0, 6.9, 0.5), (-3.0, -3.0, 1.0),
           (20.0, 20.0, 2.0), (4.0, 6.0, 0.0), (4.5, 6.5, 1.2), (3.5, 6.0, 0.3)]
    inp = place(enc, [lv0, lv1])
    assert bool(aligned(inp["loc"]).all())
    both_routes([inp, inp], "edge blocks")
