// The body of the window-staged 16-bit point-gradient kernel (boxattn_dense.h), included once into each of its two
// kernels: BOXATTN_DENSE_FROM_BOXES 0 -- pointgrad_dense_kernel, the per-point inputs loc / attn are read, grad_loc /
// grad_attn written, the backward's fill riders in the launch; 1 -- pointgrad_dense_boxes_kernel
// (boxattn_dense_boxes_bwd.h), loc / attn are made from the boxes and logits (dense_boxes_points) and the per-point
// gradients are reduced on the chip to the gradients of the L boxes and the 4 L logits of the (query, head) pair
// (BOXATTN_DENSE_BOXES_EPILOGUE), no riders.  Text inclusion, not a shared __device__ function: behind two __global__
// wrappers the existing kernel came out with other instructions.  No include guard.
    constexpr int C = 32, P = 4, LP = L * P;
    // (+ 256 * 16: a lane parks its L attention weights in LDS until it needs them (4 registers))
    __shared__ __attribute__((aligned(16))) unsigned char win_lds[kDenseLdsBytes + 256 * 16];
    static_assert(4 * kDenseResFloats * sizeof(float) <= sizeof(win_lds), "the result tiles reuse the window buffer");
#if !BOXATTN_DENSE_FROM_BOXES
    static_assert(kRideLdsInts * sizeof(int) <= sizeof(win_lds), "so do the riders");
#endif
    // (the wave index as a scalar: everything per window row -- row index, clamps, byte offsets, the
    // "row exists" branches -- is then scalar code; derived from threadIdx in a vector register it was
    // ~25 vector instructions, a v_readfirstlane and an exec-mask branch per row)
    const int lane = threadIdx.x & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
#if BOXATTN_DENSE_FROM_BOXES
    const unsigned tile_block = blockIdx.x;                        // no riders
#else
    // the backward's fill pass rides in this launch (boxattn_ride.h): rider workgroups write the bin
    // records while the tiles' workgroups compute -- the one waits on memory, the other on issue slots
    const RideRole role = ride_role(blockIdx.x, ride.grid);
    if (role.rider) {
        bin_fill_ride<256, true>(ride, role.id, reinterpret_cast<int *>(win_lds));
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

    // ---- lane -> (query of the wave's 4x4 sub-tile, point)
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
        __builtin_amdgcn_make_buffer_rsrc(const_cast<ST *>(value), 0, value_bytes, 0x00020000);
    // the window rows first: they are what the workgroup's barrier waits for; the lane's own inputs
    // (locations, weights, grad_out row) are requested behind them and land while the rows are staged
    DenseWinPos win[L];
    dense_stage_issue<L>(hot, wrow, t, lane, wv, rs, win_lds, win);
    float2 xy[L];
    float a[L];
#if BOXATTN_DENSE_FROM_BOXES
    // lane p of the quad: point p of every level, from the query's boxes and logits (behind the window requests)
    dense_boxes_points<L>(ref, offsets, kidx, vr, logits, gd, t.b, t.b * (unsigned)hot.Lq + q, qh, p, xy, a);
#else
#pragma unroll
    for (int l = 0; l < L; ++l) {
        // (plain loads: the training forward read these lines a launch ago and most are still in the Infinity
        // Cache -- with non-temporal loads here and in the fill riders the launch took 81 us instead of 51)
        xy[l] = loc2[pt0 + l * P + p];
        a[l] = attn[pt0 + l * P + p];
    }
#endif
    unsigned gw[16];                                               // the query's grad_out row
    dense_load_row(grad_out + (size_t)qh * C, gw);
    // (the attention weights are needed last, for the location gradients: parked in a lane-private piece of LDS
    // meanwhile -- held in registers the kernel does not fit five waves per SIMD, and the compiler's own spill
    // goes to scratch with a full memory wait per value)
    // (an LDS pointer BY TYPE: address spaces are not inferred for volatile accesses -- through a generic pointer these
    // were flat stores / loads with system scope, each followed by s_waitcnt vmcnt(0): four serialised round trips in
    // front of the barrier, with every window row and operand load of the wave still in flight)
    typedef __attribute__((address_space(3))) float dense_lds_float;
    volatile dense_lds_float *a_stash = (volatile dense_lds_float *)(win_lds + kDenseLdsBytes) + 4 * threadIdx.x;
#pragma unroll
    for (int l = 0; l < L; ++l) a_stash[l] = a[l];
    dense_stage_wait();                    // windows complete

    float ga[L], gx[L], gy[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const DenseMap T = hot.lv[l];
        const DensePoint s = dense_locate(xy[l].x, xy[l].y, T.H, T.W);
        float sk[4];
        dense_corner_sums<ST>(s, T, win[l], win_lds, gw, value, t.b * (unsigned)hot.S + (unsigned)T.start, H, h, vq, p, sk);
        const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
        const float gs_ = w1 * sk[0] + w2 * sk[1] + w3 * sk[2] + w4 * sk[3];
        const float al = a_stash[l];
        const float gx_ = (float)T.W * al * (s.hh * (sk[1] - sk[0]) + s.lh * (sk[3] - sk[2]));
        const float gy_ = (float)T.H * al * (s.hw * (sk[2] - sk[0]) + s.lw * (sk[3] - sk[1]));
        ga[l] = s.inside ? gs_ : 0.f;
        gx[l] = s.inside ? gx_ : 0.f;
        gy[l] = s.inside ? gy_ : 0.f;
        // (finished HERE: left alone the compiler postpones this arithmetic to the epilogue and carries nine
        // values per level -- corner sums and weights -- instead of three)
        asm volatile("" : "+v"(ga[l]), "+v"(gx[l]), "+v"(gy[l]));
    }
#if BOXATTN_DENSE_FROM_BOXES
#pragma unroll
    for (int l = 0; l < L; ++l) a[l] = a_stash[l];
#include "boxattn_dense_boxes_epilogue.h"
#else
    // ---- results: lane (q, p) holds its point on every level; memory wants, per (query, head),
    //      [level][point] runs -- transposed through (wave-private) LDS so that lane (q, j) writes
    //      level j's 4 points as 16 + 32 contiguous bytes (whole 64- / 128-byte runs per query)
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
        // the point gradients leave with non-temporal stores: nobody on the GPU reads them soon, and
        // the bin records the fill riders of this launch write should stay in the Infinity Cache
        typedef float pg_f32x4 __attribute__((ext_vector_type(4)));
        pg_f32x4 *ga4 = reinterpret_cast<pg_f32x4 *>(grad_attn + pt0 + p * P);
        pg_f32x4 *gl = reinterpret_cast<pg_f32x4 *>(grad_loc + 2 * (size_t)(pt0 + p * P));
        __builtin_nontemporal_store(pg_f32x4{o_a.x, o_a.y, o_a.z, o_a.w}, ga4);
        __builtin_nontemporal_store(pg_f32x4{o_0.x, o_0.y, o_0.z, o_0.w}, gl);
        __builtin_nontemporal_store(pg_f32x4{o_1.x, o_1.y, o_1.z, o_1.w}, gl + 1);
    }
#endif
