"""CPU: the input condition of tests/test_gpu_box_boxes_staged_backward.py.  grad_loc is discontinuous where a sample
point crosses a bilinear cell edge, so a box gradient that sums such a point cannot be held to a bound; the GPU matrix
therefore asks of its INPUTS that the share of sample points within 1e-4 px of a cell edge is at most
error_bounds.EDGE_CAP (0.2 %) -- a condition on inputs, not a tolerance.  The inputs are
boxes_cases.staged_problem's; four of them are over the cap (two points each) and are built from another
seed (RESEED, as tests/test_gpu_box_boxes_backward.py does).  This file proves the cap for every case the GPU file
uses, with the float32 grid of boxes_cases.grid_f32 and point_cases.on_cell_edge, and that the four
are the only ones that needed it."""

import numpy as np
import pytest

import error_bounds as eb
from boxes_cases import (FAMILIES, MATRIX, STAGED_BWD_RESEED as RESEED, flavours_of, grid_f32, kernel_offsets,
                         staged_bwd_case as case, staged_problem as problem)
from point_cases import on_cell_edge


def edge_share(g):
    """Share of the sample points of the problem ``g`` within 1e-4 px of a bilinear cell edge (float32 grid on the CPU)."""
    grid = grid_f32(g["ref"], g["off"], kernel_offsets(2), g["vr"], g["angle_mode"])
    return float(on_cell_edge(grid.astype(np.float64), g["shapes"]).mean())


def keys_of(geometry):
    return [(geometry, family) + flavour[0] + flavour[1:] for family in FAMILIES for flavour in flavours_of(geometry)]


@pytest.mark.parametrize("geometry", MATRIX + ["mid"])
def test_edge_share_of_every_case_is_under_the_cap(geometry):
    keys = keys_of(geometry) if geometry != "mid" else [("mid", "local", 0, 4, False, True)]
    worst = 0.0
    for key in keys:
        share = edge_share(case(*key))
        worst = max(worst, share)
        assert share <= eb.EDGE_CAP, "%s %s angle=%d D=%d per_head=%d vr=%d: %.4f %%" % (key + (100 * share,))
    print("%s: worst share of points on a cell edge %.3f %% (cap %.1f %%)" % (geometry, 100 * worst, 100 * eb.EDGE_CAP))


def test_the_reseeded_cases_are_the_ones_over_the_cap():
    over = {key for geometry in MATRIX for key in keys_of(geometry) if edge_share(problem(*key)) > eb.EDGE_CAP}
    assert over == set(RESEED), sorted(over ^ set(RESEED))
