// The window-staged encoder BACKWARD from boxes: the box and logit gradients of BoxAttention / Box3dAttention per
// (query, head) pair -- V offsets and 5 reference-window terms a level, 4 L logits -- in the launch of the staged
// point-gradient kernels (boxattn_dense.h, boxattn_dense_f32.h: an 8x8 query tile's value windows in LDS once, lane =
// one sample point, a quad = one pair), the sibling of the staged forwards from boxes (boxattn_dense_fwd.h):
//   prologue   dense_boxes_points (boxattn_dense_boxes.h) instead of the loads of loc / attn, behind the window
//              requests: the locations are grid_fwd_kernel's and the weights the staged forward's, bit for bit;
//   main loop  the per-point kernels' text (boxattn_dense_pg_body.h, boxattn_dense_f32_pg_body.h);
//   epilogue   boxattn_dense_boxes_epilogue.h: grad_loc / grad_attn never leave the chip -- the softmax Jacobian from
//              one sum over the quad, the results transposed through the per-point kernels' wave-private LDS tiles,
//              lane (q, j < L) runs grid_grad_add over level j's four points in point order and grid_grad_store.
// No riders, no state, no atomics; every sum in a fixed order: the three outputs are bitwise reproducible.  Queries
// beyond the map's edge write nothing.  What bwd2_boxes_kernel (boxattn_gather2_boxes_bwd.h) computes by gathering each
// pair's corner rows from the L2, for the encoder case.
#pragma once
#include "boxattn_dense.h"
#include "boxattn_dense_boxes.h"
#include "boxattn_dense_f32.h"

namespace boxattn {

#define BOXATTN_DENSE_FROM_BOXES 1
template <typename ST, int L>
__global__ __launch_bounds__(256, kDenseWpe) void pointgrad_dense_boxes_kernel(
    const ST *__restrict__ value, const float *__restrict__ ref, const float *__restrict__ offsets,
    const float *__restrict__ kidx, const float *__restrict__ vr, const float *__restrict__ logits,
    const ST *__restrict__ grad_out, float *__restrict__ grad_offsets, float *__restrict__ grad_ref_rows,
    float *__restrict__ grad_logits, DensePlan pl, unsigned value_bytes, GridDims gd)
{
#include "boxattn_dense_pg_body.h"
}

template <int L>
__global__ __launch_bounds__(256, 3) void pointgrad_dense_f32_boxes_kernel(
    const float *__restrict__ value, const float *__restrict__ ref, const float *__restrict__ offsets,
    const float *__restrict__ kidx, const float *__restrict__ vr, const float *__restrict__ logits,
    const float *__restrict__ grad_out, float *__restrict__ grad_offsets, float *__restrict__ grad_ref_rows,
    float *__restrict__ grad_logits, DensePlan pl, unsigned value_bytes, GridDims gd)
{
#include "boxattn_dense_f32_pg_body.h"
}
#undef BOXATTN_DENSE_FROM_BOXES

}  // namespace boxattn
