// The body of the window-staged float32 point-gradient kernel (boxattn_dense_f32.h), included once into each of its
// two kernels: BOXATTN_DENSE_FROM_BOXES 0 -- pointgrad_dense_f32_kernel, the per-point inputs loc / attn are read,
// grad_loc / grad_attn written, the backward's fill riders in the launch; 1 -- pointgrad_dense_f32_boxes_kernel, loc /
// attn are made from the boxes and logits (dense_boxes_points) and the per-point gradients are reduced on the chip to
// the gradients of the pair's L boxes and 4 L logits (boxattn_dense_boxes_epilogue.h), no riders.  Text inclusion, as
// boxattn_dense_pg_body.h.  No include guard.
    constexpr int C = 32, P = 4, LP = L * P;
    __shared__ __attribute__((aligned(16))) unsigned char win_lds[kDenseF32LdsBytes];
    static_assert(4 * kDenseResFloats * sizeof(float) <= sizeof(win_lds), "the result tiles reuse the window buffer");
#if !BOXATTN_DENSE_FROM_BOXES
    static_assert(kRideLdsInts * sizeof(int) <= sizeof(win_lds), "so do the riders");
#endif
    const int lane = threadIdx.x & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
#if BOXATTN_DENSE_FROM_BOXES
    const unsigned tile_block = blockIdx.x;                        // no riders
#else
    const RideRole role = ride_role(blockIdx.x, ride.grid);
    if (role.rider) {
        bin_fill_ride<256>(ride, role.id, reinterpret_cast<int *>(win_lds));
        return;
    }
    const unsigned tile_block = role.id;
#endif
    DenseHot<L> hot;
    DenseMap Q;
    DenseWin wrow[L];
    const DenseTileId t = dense_tile_of_block<L>(pl, tile_block, hot, Q, wrow);
    if (t.lq < 0) return;                                          // workgroup-uniform
    const int H = hot.H, h = t.h;
    const int qi = lane >> 2, p = lane & 3;
    const int qy = t.ty * kDenseTile + (wv >> 1) * kDenseSub + (qi >> 2);
    const int qx = t.tx * kDenseTile + (wv & 1) * kDenseSub + (qi & 3);
    const bool vq = qy < Q.H && qx < Q.W;
    const unsigned q = (unsigned)(Q.start + min(qy, Q.H - 1) * Q.W + min(qx, Q.W - 1));
    const unsigned qh = (t.b * (unsigned)hot.Lq + q) * (unsigned)H + (unsigned)h;
#if !BOXATTN_DENSE_FROM_BOXES
    const unsigned pt0 = qh * (unsigned)LP;
    const float2 *loc2 = reinterpret_cast<const float2 *>(loc);
#endif
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(value), 0, value_bytes, 0x00020000);
    DenseWinPosF32 win[L];
    dense_f32_stage_issue<L>(hot, wrow, t, lane, wv, rs, win_lds, win);
    float2 xy[L];
    float a[L];
#if BOXATTN_DENSE_FROM_BOXES
    // lane p of the quad: point p of every level, from the query's boxes and logits (behind the window requests)
    dense_boxes_points<L>(ref, offsets, kidx, vr, logits, gd, t.b, t.b * (unsigned)hot.Lq + q, qh, p, xy, a);
#else
#pragma unroll
    for (int l = 0; l < L; ++l) {
        xy[l] = loc2[pt0 + l * P + p];
        a[l] = attn[pt0 + l * P + p];
    }
#endif
    float gw[32];                                                  // the query's grad_out row
    dense_f32_load_row(grad_out + (size_t)qh * C, gw);
    dense_stage_wait();                                            // windows complete

    float ga[L], gx[L], gy[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const DenseMap T = hot.lv[l];
        const DenseWinPosF32 &o = win[l];
        const DensePoint s = dense_locate(xy[l].x, xy[l].y, T.H, T.W);
        const DenseFoot f = dense_f32_foot(s, T, o);
        const bool act = vq && s.inside;
        const bool slow = act && f.d < 0, fast = act && f.d >= 0;
        float sk[4];
        if (__builtin_amdgcn_ballot_w64(fast) != 0ull) {           // wave-uniform: somebody reads the window
            int slot[4];
            dense_f32_slots(s, o, slot);
#pragma unroll
            for (int k = 0; k < 4; ++k) {                          // a corner at a time: 8 LDS reads, then the 32 products
                float va[32];
                dense_f32_load_row(win_lds + slot[k], va);
                sk[k] = __uint_as_float(__float_as_uint(dense_f32_dot_row(gw, va)) & f.m[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) sk[k] = 0.f;
        }
        if (__builtin_amdgcn_ballot_w64(slow) != 0ull) {           // wave-uniform: the global path
            // one point of every quad at a time: the quad's lanes fetch the four corner rows of point tp together,
            // 32 bytes each, and sum their partial dot products with DPP adds (as the bf16 kernel)
            float gch[8];                                          // this lane's 8 channels of the grad_out row
#pragma unroll
            for (int i = 0; i < 8; ++i) gch[i] = p == 0 ? gw[i] : p == 1 ? gw[8 + i] : p == 2 ? gw[16 + i] : gw[24 + i];
            const unsigned row0 = t.b * (unsigned)hot.S + (unsigned)T.start;
            const int pra = __mul24(f.ra, T.W), prb = __mul24(f.rb, T.W);
            const int pix[4] = {pra + f.ca, pra + f.cb, prb + f.ca, prb + f.cb};
            unsigned off[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) off[k] = (unsigned)(((row0 + (unsigned)pix[k]) * H + h) * (C * 4));
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) {
                float4 v[4][2];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 *src = reinterpret_cast<const float4 *>(
                        reinterpret_cast<const char *>(value) + quad_bcast_u32(off[k], tp) + (unsigned)p * 32u);
                    v[k][0] = src[0];
                    v[k][1] = src[1];
                }
                float part[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float dd = gch[0] * v[k][0].x;
                    dd = fmaf(gch[1], v[k][0].y, dd); dd = fmaf(gch[2], v[k][0].z, dd); dd = fmaf(gch[3], v[k][0].w, dd);
                    dd = fmaf(gch[4], v[k][1].x, dd); dd = fmaf(gch[5], v[k][1].y, dd);
                    dd = fmaf(gch[6], v[k][1].z, dd); dd = fmaf(gch[7], v[k][1].w, dd);
                    part[k] = group_sum<4>(dd);
                }
                if (p == tp && slow) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) sk[k] = __uint_as_float(__float_as_uint(part[k]) & f.m[k]);
                }
            }
        }
        const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
        const float gs_ = w1 * sk[0] + w2 * sk[1] + w3 * sk[2] + w4 * sk[3];
        const float gx_ = (float)T.W * a[l] * (s.hh * (sk[1] - sk[0]) + s.lh * (sk[3] - sk[2]));
        const float gy_ = (float)T.H * a[l] * (s.hw * (sk[2] - sk[0]) + s.lw * (sk[3] - sk[1]));
        ga[l] = s.inside ? gs_ : 0.f;
        gx[l] = s.inside ? gx_ : 0.f;
        gy[l] = s.inside ? gy_ : 0.f;
        asm volatile("" : "+v"(ga[l]), "+v"(gx[l]), "+v"(gy[l]));
    }
#if BOXATTN_DENSE_FROM_BOXES
#include "boxattn_dense_boxes_epilogue.h"
#else
    // ---- results through (wave-private) LDS: lane (q, j) writes level j's 4 points as 16 + 32 contiguous bytes
    __syncthreads();                                               // every wave is done with the windows
    float *res = reinterpret_cast<float *>(win_lds) + wv * kDenseResFloats;
    float *res_a = res + qi * LP, *res_xy = res + 16 * LP + qi * LP * 2;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        res_a[l * P + p] = ga[l];
        *reinterpret_cast<float2 *>(res_xy + (l * P + p) * 2) = make_float2(gx[l], gy[l]);
    }
    wave_lds_sync();
    if (vq && p < L) {
        const float4 o_a = *reinterpret_cast<const float4 *>(res_a + p * P);
        const float4 o_0 = *reinterpret_cast<const float4 *>(res_xy + p * P * 2);
        const float4 o_1 = *reinterpret_cast<const float4 *>(res_xy + p * P * 2 + 4);
        float4 *ga4 = reinterpret_cast<float4 *>(grad_attn + pt0 + p * P);
        float4 *gl = reinterpret_cast<float4 *>(grad_loc + 2 * (size_t)(pt0 + p * P));
        typedef float pg_f32x4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(pg_f32x4{o_a.x, o_a.y, o_a.z, o_a.w}, reinterpret_cast<pg_f32x4 *>(ga4));
        __builtin_nontemporal_store(pg_f32x4{o_0.x, o_0.y, o_0.z, o_0.w}, reinterpret_cast<pg_f32x4 *>(gl));
        __builtin_nontemporal_store(pg_f32x4{o_1.x, o_1.y, o_1.z, o_1.w}, reinterpret_cast<pg_f32x4 *>(gl + 1));
    }
#endif
