"""CPU: the yardstick of ``ops.box_attn_backward_boxes_value``'s grad_value, without a GPU.

``value_reference`` is grad_value's float64 model from boxes and logits: ``error_bounds.grid_reference``,
``softmax_reference`` and ``_reference(..., slack=dloc, dws=[dw])["grad_value"]`` -- exactly the arguments
``boxes_reference(kind="box")`` passes; it computes this plane too and discards it.  The problems are those of
``boxes_cases.bwd_problem`` with upstream ``bwd_upstream`` and value ``every_type(value)`` (the GPU file's
own).  tests/test_gpu_box_boxes_value.py holds the kernel to the same planes.

Here: a float32 evaluation on the CPU -- ``boxes_cases.grid_f32``, a float32 torch softmax, the C oracle's
float32 ``box_attn_backward`` -- holds the bound (``error_bounds.hold``, split "none") in float32 and rounded to bf16 and
f16, over all 16 flavours of seven cases; the same result scaled by 1 + 2^-12 does not hold it in float32.  grad_value
has no cell-edge ambiguity: no exclusion and no cap.  Elements whose bound is 0 (pixels no point touches) must be
exactly zero; their share is printed per case."""

import numpy as np
import pytest
import torch

import error_bounds as eb
import boxes_cases
from boxes_cases import c32, grid_f32, value_reference
from compare_rules import must_be_zero_share
from oracle import boxattn_oracle as oc

CASES = [("model", 32), ("ragged", 16), ("k4", 32), ("sixteen_levels", 64), ("encoder", 32), ("odd_k", 32),
         ("one_level", 16)]


def value_f32(g, gout):
    """grad_value in float32 on the CPU: float32 grid, float32 torch softmax, the C oracle's float32 build."""
    B, S, H, C, L, Lq, P = g["dims"]
    kidx = boxes_cases.kernel_offsets(int(round(P ** 0.5)))
    loc = c32(grid_f32(g["ref"], g["off"], kidx, g["vr"], g["angle_mode"]))
    logits = torch.from_numpy(c32(g["logits"])).reshape(B, Lq, H, L * P)
    attn = c32(torch.softmax(logits, -1).numpy().reshape(B, Lq, H, L, P))
    gval, _, _ = oc.box_attn_backward(c32(boxes_cases.every_type(g["value"])), g["shapes"], g["lsi"], loc, attn, c32(gout))
    gval = np.asarray(gval).reshape(B, S, H, C)
    assert gval.dtype == np.float32
    return gval


@pytest.mark.parametrize("geometry,C", CASES)
def test_float32_evaluation_holds_the_bound_and_a_scaled_one_does_not(geometry, C):
    worst = {"float32": 0.0, "bf16": 0.0, "f16": 0.0}
    shares, outside = [], []
    for flavour in boxes_cases.FLAVOURS:
        g = boxes_cases.bwd_problem(geometry, C, flavour)
        ref = value_reference(geometry, C, flavour)
        got = value_f32(g, boxes_cases.bwd_upstream(g))
        what = "float32 grad_value on the CPU: %s C=%d angle=%d D=%d per_head=%d vr=%d" % ((geometry, C) + flavour[0]
                                                                                         + flavour[1:])
        assert got.shape == ref["want"].shape
        worst["float32"] = max(worst["float32"], eb.hold(got, ref, "float32", "none", what))
        for store in ("bf16", "f16"):
            worst[store] = max(worst[store], eb.hold(eb.round_to(got.astype(np.float64), store), ref, store, "none", what))
        shares.append(must_be_zero_share(ref))
        r, _, _ = eb.ratio(got.astype(np.float64) * (1 + 2.0 ** -12), ref, "float32", "none")
        outside.append(int((r > 1.0).sum()))
        with pytest.raises(AssertionError):
            eb.hold(got.astype(np.float64) * (1 + 2.0 ** -12), ref, "float32", "none", what + ", scaled")
    for store, w in worst.items():
        print("error-bound | float32 grad_value on the CPU: %s C=%d | %s | grad_value | %.3f" % (geometry, C, store, w))
    print("%s C=%d: must-be-zero share %.3f ... %.3f; scaled by 1 + 2^-12: %d ... %d elements outside"
          % (geometry, C, min(shares), max(shares), min(outside), max(outside)))
