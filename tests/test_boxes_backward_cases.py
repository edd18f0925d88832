"""CPU: the inputs of tests/test_gpu_boxes_backward.py's seeded matrix keep the condition its float64 expectation
rests on -- at most 0.2 % of a case's sample points lie within 1e-4 px of a bilinear cell edge, where grad_loc is
ambiguous and the expectation has to take the chain's value (about 0.04 % is expected for these uniform inputs; a case
that broke the condition got another seed there, RESEED).  The grid is evaluated in float32 numpy, operation by
operation as the kernels do."""
import itertools

import pytest

from boxes_cases import (EDGE_CAP, INST_GEOMETRY as GEOMETRY, KERNEL_SIZES, inst_bwd_case as case,
                         inst_edge_share as edge_share)


@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
def test_edge_share_of_every_case_is_under_the_cap(geometry):
    worst = 0.0
    for C, k, per_head, with_vr in itertools.product((16, 32, 64), KERNEL_SIZES, (False, True), (False, True)):
        share = edge_share(case(geometry, C, k, per_head, with_vr), k)
        worst = max(worst, share)
        assert share <= EDGE_CAP, "%s C=%d k=%d per_head=%d vr=%d: %.4f %%" % (geometry, C, k, per_head, with_vr,
                                                                              100 * share)
    print("%s: worst share %.4f %%" % (geometry, 100 * worst))
