// The prologue of the window-staged forwards from boxes (fwd_dense_boxes_kernel, fwd_dense_f32_boxes_kernel): what
// those kernels' per-point flavours load as loc and attn, made in registers from what the module predicts.
//
// A quad = one (query, head) pair, lane r = point r of every level (P = 4, L <= 4):
//   weights    lane r takes the logits 4 l + r, l = 0 .. L - 1.  Softmax in float32 in the order of fwd2_boxes_kernel
//              (boxattn_gather2_boxes.h): maximum of the lane's own L values, then over the quad (group_fmax<4>);
//              __expf(z - max); the sum of the lane's own L values in level order, then over the quad (group_sum<4>);
//              each exponential * (1 / sum).  With a lane group of 4 (16-bit storage) those are fwd2_boxes_kernel's
//              weights bit for bit; softmax_rows_fwd_kernel, one thread a row, sums in another order.
//   boxes      lane r decodes the box of level min(r, L - 1) (grid_box_rows, boxattn_grid.h: one sincosf a lane in the
//              rotated modes, not L) and the quad shares the L boxes by DPP broadcasts, 4 to 8 registers a level.
//              Every lane decoding every level compiled to the same register counts (the main loop sets them), with
//              L times the loads and sincosf.
//   locations  grid_point on the box of level l and kernel_indices row r.
// grid_box_rows / grid_point keep their fp contract(off): the locations are grid_fwd_kernel's bit for bit.
// All lanes of the wave are active here (the DPP steps read their neighbours): a query beyond the map's edge comes
// in clamped to a valid one, so every load is in range and every value finite where the inputs are.
#pragma once
#include "boxattn_dense.h"
#include "boxattn_grid.h"

namespace boxattn {

__device__ __forceinline__ float quad_bcast_f32(float v, int t)        // t is a constant after unrolling
{
    return __uint_as_float(quad_bcast_u32(__float_as_uint(v), t));
}

// b: image, bq = b Lq + q, qh = bq H + h: the pair's rows of ref (bq or qh), offsets and logits (qh)
template <int L>
__device__ __forceinline__ void dense_boxes_points(const float *__restrict__ ref, const float *__restrict__ offsets,
                                                   const float *__restrict__ kidx, const float *__restrict__ vr,
                                                   const float *__restrict__ logits, const GridDims &gd, unsigned b,
                                                   unsigned bq, unsigned qh, int r, float2 (&xy)[L], float (&a)[L])
{
    static_assert(L >= 1 && L <= 4, "a lane of the quad per level");
    constexpr int P = 4;
    const bool has_vr = vr != nullptr;
    const int angle_mode = gd.angle_mode;
    // ---- every load first
    const float *zrow = logits + (size_t)qh * (L * P) + r;
    float z[L];
#pragma unroll
    for (int l = 0; l < L; ++l) z[l] = zrow[P * l];
    const float kxy[2] = {kidx[2 * r], kidx[2 * r + 1]};
    const int lr = min(r, L - 1);                                  // the level this lane decodes
    const GridBox g = grid_box_rows(ref + (size_t)(gd.ref_per_head ? qh : bq) * (unsigned)gd.ref_dim,
                                    offsets + ((size_t)qh * L + lr) * (unsigned)gd.V,
                                    has_vr ? vr + ((size_t)b * L + lr) * 2 : nullptr, angle_mode);
    // ---- softmax over the quad's 4 L logits
    float m = z[0];
#pragma unroll
    for (int l = 1; l < L; ++l) m = fmaxf(m, z[l]);
    m = group_fmax<4>(m);
    float sum = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        z[l] = __expf(z[l] - m);
        sum += z[l];
    }
    const float inv = 1.f / group_sum<4>(sum);
    // ---- the L boxes from their lanes, this lane's point of each
#pragma unroll
    for (int l = 0; l < L; ++l) {
        a[l] = z[l] * inv;
        GridBox gl;
        gl.cx = quad_bcast_f32(g.cx, l); gl.cy = quad_bcast_f32(g.cy, l);
        gl.w = quad_bcast_f32(g.w, l); gl.h = quad_bcast_f32(g.h, l);
        gl.sn = 0.f; gl.cs = 1.f; gl.vx = gl.vy = 1.f;
        if (angle_mode) {                                          // (wave-uniform, as has_vr)
            gl.sn = quad_bcast_f32(g.sn, l);
            gl.cs = quad_bcast_f32(g.cs, l);
        }
        if (has_vr) {
            gl.vx = quad_bcast_f32(g.vx, l);
            gl.vy = quad_bcast_f32(g.vy, l);
        }
        gl.rw = gl.rh = 0.f;
        xy[l] = grid_point(gl, kxy, 0, has_vr, angle_mode);
        // (opaque from here on: the compiler otherwise sinks a level's arithmetic to its use behind the barrier and
        // keeps the decoded box, the exponentials and 1 / sum alive through the levels -- spills at 96 registers)
        asm volatile("" : "+v"(xy[l].x), "+v"(xy[l].y), "+v"(a[l]));
    }
}

}  // namespace boxattn
