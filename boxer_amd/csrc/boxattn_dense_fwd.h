// Window-staged FORWARD for the encoder case of 16-bit (bf16 or f16) box attention (one query per pixel, C = 32,
// 2x2 points, <= 4 levels): the staging of boxattn_dense.h (the value windows of an 8x8 query tile and head in LDS) with the
// arithmetic on the matrix cores.
//
// out[q][c] = sum over the query's 16 points and their 4 corners of w * v[corner][c], w a float32 weight.  On the
// VALU that is an unpack + a multiply-add per bf16 element: 2/3 of fwd2_kernel's instructions.  Here one
// v_mfma_f32_4x4x4_16B_bf16 (16 independent 4x4x4 products, one per lane QUAD) does 4 channels x 4 corners of one
// point for 16 queries at once:
//
//     D[i][j] += sum_k A[i][k] B[k][j]      k = corner, j = channel (4 per instruction), i = term of the weight
//
//   A (lane i of the quad holds row i): the point's four corner weights split into two bf16 terms, w = hi + lo
//     (|w - hi - lo| <= 2^-17 |w|; f16 terms on v_mfma_f32_4x4x4_16b_f16: <= 2^-22 |w| + 2^-25):
//     row 0 = hi, row 1 = lo (rows 2, 3 repeat them; their results are not used);
//     broadcast inside the quad from the lane that located the point (DPP quad_perm), hi or lo by the lane's parity;
//   B (lane j holds column j = 4 corners of one channel): exactly what ds_read_b64_tr_b16 delivers -- in a 16-lane
//     group lane 4 k + q supplies the address of corner k's row for the query of quad q, and lane 4 q + r receives
//     element r (channel c0 + r) of the four rows.  Eight reads (c0 = 0, 4, .. 28) and eight MFMAs per point;
//   D: lane r of a quad ends with channels r, 4 + r, .. 28 + r of its query (term rows 0 and 1 are added at the end).
//
// A quad = one query; its four lanes locate the four points of a level (lane r: point r), then the quad walks the
// four points together.  The supplier lane of (corner k, quad q) gets the point's packed {slot of its top-left
// corner, which corners count} from the locating lane with one ds_bpermute and derives its own corner's slot.
// Corners that do not count (outside the map) and points that are not served from the window read a zero row.
//
// Points whose footprint is not inside the staged window (and every point of a level that is not staged) take the
// global path of the gather kernels inside the same kernel: the quad fetches the four corner rows together, 16
// bytes per lane (out-of-map corners and the other quads of the wave: an offset outside the buffer, for which the
// hardware returns zeros), unpack + multiply-add on the VALU into a second, channel-contiguous accumulator.
// Entered per (level, point step) only if some quad of the wave needs it.  Same results either way.
//
// Epilogue: the matrix-core sums (channel 4 m + r in lane r) are brought into the channel-contiguous order through
// LDS (the window buffer, after a barrier), added to the VALU sums and stored as one 16-byte piece per lane.
#pragma once
#include "boxattn_dense.h"
#include "boxattn_dense_boxes.h"

namespace boxattn {

// lanes (0, 1, 2, 3) of every quad <- lanes (2 u, 2 u, 2 u + 1, 2 u + 1)
__device__ __forceinline__ unsigned quad_pairs_u32(unsigned v, int u)       // u is a constant after unrolling
{
    return u == 0 ? (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x50, 0xF, 0xF, true)      // quad_perm [0,0,1,1]
                  : (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xFA, 0xF, 0xF, true);     // quad_perm [2,2,3,3]
}
// lanes (0, 1, 2, 3) <- lanes (2 u, 2 u + 1, 2 u, 2 u + 1)
__device__ __forceinline__ unsigned quad_evenodd_u32(unsigned v, int u)
{
    return u == 0 ? (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x44, 0xF, 0xF, true)      // quad_perm [0,1,0,1]
                  : (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xEE, 0xF, 0xF, true);     // quad_perm [2,3,2,3]
}

typedef short fwd_i16x4 __attribute__((ext_vector_type(4)));
typedef float fwd_f32x4 __attribute__((ext_vector_type(4)));

// (the body: boxattn_dense_fwd_body.h, shared by text inclusion with the from-boxes flavour below)
#define BOXATTN_DENSE_FROM_BOXES 0
template <typename ST, int L>
__global__ __launch_bounds__(256, kDenseWpe) void fwd_dense_kernel(
    const ST *__restrict__ value, const float *__restrict__ loc, const float *__restrict__ attn,
    ST *__restrict__ out, DensePlan pl, unsigned value_bytes, BinRide ride,
    unsigned long long *__restrict__ stats)
{
#include "boxattn_dense_fwd_body.h"
}
#undef BOXATTN_DENSE_FROM_BOXES

// The same forward at inference straight from what the module predicts per (query, head) -- L boxes (reference window
// + V offsets a level) and 4 L logits, the operands of fwd2_boxes_kernel -- instead of loc and attn: the quad makes
// its query's 4 L locations and weights in registers while the window requests are in flight (dense_boxes_points,
// boxattn_dense_boxes.h).  No riders, no statistics, no atomics.
#define BOXATTN_DENSE_FROM_BOXES 1
template <typename ST, int L>
__global__ __launch_bounds__(256, kDenseWpe) void fwd_dense_boxes_kernel(
    const ST *__restrict__ value, const float *__restrict__ ref, const float *__restrict__ offsets,
    const float *__restrict__ kidx, const float *__restrict__ vr, const float *__restrict__ logits,
    ST *__restrict__ out, DensePlan pl, unsigned value_bytes, GridDims gd)
{
#include "boxattn_dense_fwd_body.h"
}
#undef BOXATTN_DENSE_FROM_BOXES

}  // namespace boxattn
