"""CPU: what the float64 expectation of tests/test_gpu_box_boxes_backward.py rests on.

(a) Its numpy reductions -- ``reduce_grid`` (grid_grad_add / grid_grad_store of boxattn_grid.h with the rotation terms)
    and ``reduce_logits`` (the softmax Jacobian) -- fed with the float64 C oracle's per-point gradients agree with
    float64 torch autograd through the reference modules' grid construction, a softmax and the grid_sample statement of
    the operator, for offsets, reference windows and logits, in all three angle modes, to 1e-9 of max(1, max |want|):
    float64 against float64.
(b) The inputs of the GPU matrix keep the cell-edge condition: at most 0.2 % of a case's sample points lie within
    1e-4 px of a bilinear cell edge, where grad_loc is ambiguous and the expectation has to take the chain's value.
    18 of the 336 cases from the seeds of boxes_cases.box_boxes_problem break it (by 1-4 points of 384-1 280: a box
    of size <= 0 puts a whole row of points on one line; the worst, k4 C = 64 mode 0 per head without valid ratios, has
    1.04 %); they take another seed (RESEED).  The grid is evaluated in float32 numpy, operation by operation as the
    kernels do."""
import numpy as np
import pytest
import torch

from oracle import boxattn_oracle as oc
from oracle import torch_fallback
from boxes_cases import (BOX_BWD_CHANNELS as CHANNELS, BOX_BWD_RESEED as RESEED, EDGE_CAP, FLAVOURS, SMALL,
                         box_boxes_problem as problem, box_bwd_case as case, box_edge_share as edge_share,
                         box_reduce_grid as reduce_grid, box_reduce_logits as reduce_logits)
from point_cases import _torch_grid


def autograd_and_reductions(g):
    """-> [(name, reduced oracle gradient, autograd gradient)] for offsets, reference windows and logits."""
    from boxer_amd.modules import _kernel_offsets
    B, S, H, C, L, Lq, P = g["dims"]
    k = int(round(P ** 0.5))
    kidx = _kernel_offsets(k, k).double()
    leaf = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_()
    ref, off, logits = leaf(g["ref"]), leaf(g["off"]), leaf(g["logits"])
    vr = None if g["vr"] is None else torch.from_numpy(g["vr"]).double()
    value = torch.from_numpy(g["value"])
    gout = torch.from_numpy(np.random.default_rng(5).standard_normal((B, Lq, H * C)))
    loc = _torch_grid(ref, off, kidx, vr, g["angle_mode"])
    attn = torch.softmax(logits, -1).view(B, Lq, H, L, P)
    out = torch_fallback.box_attn(value, g["shapes"], loc, attn)
    (out * gout).sum().backward()
    _, gloc, gattn = oc.box_attn_backward(g["value"], g["shapes"], g["lsi"], loc.detach().numpy(),
                                          attn.detach().numpy(), gout.numpy())
    goff, rows = reduce_grid(g["ref"], g["off"], kidx.numpy(), g["vr"], g["angle_mode"],
                             np.asarray(gloc).reshape(tuple(loc.shape)))
    glog = reduce_logits(g["logits"], gattn)
    n = min(5, g["ref"].shape[-1])
    gref = rows.sum(3) if g["ref"].ndim == 4 else rows.sum((2, 3))
    want_ref = ref.grad.numpy()
    assert not want_ref[..., n:].any()                       # (the values past the angle take no part)
    return [("offsets", goff, off.grad.numpy()), ("ref_windows", gref[..., :n], want_ref[..., :n]),
            ("logits", glog, logits.grad.numpy())]


@pytest.mark.parametrize("geometry", SMALL)
def test_reductions_agree_with_float64_autograd(geometry):
    worst = 0.0
    for (angle_mode, ref_dim), per_head, with_vr in FLAVOURS:
        g = problem(geometry, 16, angle_mode, ref_dim, per_head, with_vr)
        for name, got, want in autograd_and_reductions(g):
            assert got.shape == want.shape, name
            err = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
            worst = max(worst, err)
            assert err <= 1e-9, "%s angle=%d D=%d per_head=%d vr=%d: %s off by %.3e" % (
                geometry, angle_mode, ref_dim, per_head, with_vr, name, err)
    print("%s: worst error %.3e" % (geometry, worst))


@pytest.mark.parametrize("geometry", SMALL)
def test_edge_share_of_every_case_is_under_the_cap(geometry):
    worst = 0.0
    for C in CHANNELS:
        for (angle_mode, ref_dim), per_head, with_vr in FLAVOURS:
            share = edge_share(case(geometry, C, angle_mode, ref_dim, per_head, with_vr))
            worst = max(worst, share)
            assert share <= EDGE_CAP, "%s C=%d angle=%d D=%d per_head=%d vr=%d: %.4f %%" % (
                geometry, C, angle_mode, ref_dim, per_head, with_vr, 100 * share)
    print("%s: worst share %.4f %%" % (geometry, 100 * worst))


def test_the_reseeded_cases_are_the_ones_over_the_cap():
    """Every entry of RESEED is a case whose inputs from ``problem`` break the condition, and there is no other."""
    over = set()
    for geometry in SMALL:
        for C in CHANNELS:
            for (angle_mode, ref_dim), per_head, with_vr in FLAVOURS:
                if edge_share(problem(geometry, C, angle_mode, ref_dim, per_head, with_vr)) > EDGE_CAP:
                    over.add((geometry, C, angle_mode, ref_dim, per_head, with_vr))
    assert over == set(RESEED) and len(over) == 18
