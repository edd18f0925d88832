// The body of the window-staged float32 forward (boxattn_dense_f32.h), included once into each of its two kernels:
// BOXATTN_DENSE_FROM_BOXES 0 -- fwd_dense_f32_kernel; 1 -- fwd_dense_f32_boxes_kernel (as boxattn_dense_fwd_body.h for
// the 16-bit pair).  No include guard.
    constexpr int C = 32;
    __shared__ __attribute__((aligned(16))) unsigned char win_lds[kDenseF32LdsBytes];
    static_assert(256 * 33 * sizeof(float) <= sizeof(win_lds), "the result tiles reuse the window buffer");
    const int lane = threadIdx.x & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
#if BOXATTN_DENSE_FROM_BOXES
    const unsigned tile_block = blockIdx.x;                        // no riders
#else
    const RideRole role = ride_role(blockIdx.x, ride.grid);
    if (role.rider) {
        bin_count_ride<256>(ride, role.id, reinterpret_cast<int *>(win_lds));
        return;
    }
    const unsigned tile_block = role.id;
#endif
    DenseHot<L> hot;
    DenseMap Q;
    DenseWin wrow[L];
    const DenseTileId t = dense_tile_of_block<L>(pl, tile_block, hot, Q, wrow);
    if (t.lq < 0) return;
    const int H = hot.H, h = t.h;
    const int qi = lane >> 2, p = lane & 3;
    const int qy = t.ty * kDenseTile + (wv >> 1) * kDenseSub + (qi >> 2);
    const int qx = t.tx * kDenseTile + (wv & 1) * kDenseSub + (qi & 3);
    const bool vq = qy < Q.H && qx < Q.W;
    const unsigned q = (unsigned)(Q.start + min(qy, Q.H - 1) * Q.W + min(qx, Q.W - 1));
    const unsigned qh = (t.b * (unsigned)hot.Lq + q) * (unsigned)H + (unsigned)h;
#if !BOXATTN_DENSE_FROM_BOXES
    constexpr int P = 4, LP = L * P;
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
    if (threadIdx.x < 8)
        *reinterpret_cast<float4 *>(win_lds + kDenseF32ZeroOff + 16 * threadIdx.x) = make_float4(0.f, 0.f, 0.f, 0.f);
    dense_stage_wait();

#if !BOXATTN_DENSE_FROM_BOXES
    unsigned n_slow = 0, n_act = 0;                                // locality statistics of this wave (stats != nullptr)
#endif
    float acc[32];                                                 // this lane's point(s): all 32 channels
    float accs[8];                                                 // global path: channels 8 p .. 8 p + 7 of the QUERY
#pragma unroll
    for (int c = 0; c < 32; ++c) acc[c] = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) accs[c] = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const DenseMap T = hot.lv[l];
        const DenseWinPosF32 &o = win[l];
        const DensePoint s = dense_locate(xy[l].x, xy[l].y, T.H, T.W);
        const DenseFoot f = dense_f32_foot(s, T, o);
        const bool act = vq && s.inside;
        const bool slow = act && f.d < 0, fast = act && f.d >= 0;
        // the reference's products: (hh hw) v a, summed per point, then over the points
        const float wk[4] = {s.hh * s.hw, s.hh * s.lw, s.lh * s.hw, s.lh * s.lw};
        if (__builtin_amdgcn_ballot_w64(fast) != 0ull) {
            int slot[4];
            dense_f32_slots(s, o, slot);
            const float af = fast ? a[l] : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // (a corner outside the map -- or a lane that is not served from the window -- reads the row of ZEROS:
                // whatever pixel its clamped slot names, finite or not, never meets its (zero) weight: 0 * Inf is NaN)
                const bool counts = fast && f.m[k] != 0u;
                float va[32];
                dense_f32_load_row(win_lds + (counts ? slot[k] : kDenseF32ZeroOff), va);
                const float wa = counts ? wk[k] * af : 0.f;
#pragma unroll
                for (int c = 0; c < 32; ++c) acc[c] = fmaf(wa, va[c], acc[c]);
            }
        }
        const unsigned long long slow_lanes = __builtin_amdgcn_ballot_w64(slow);
#if !BOXATTN_DENSE_FROM_BOXES
        n_slow += (unsigned)__builtin_popcountll(slow_lanes);
        n_act += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(act));
#endif
        if (slow_lanes != 0ull) {                                  // wave-uniform: the global path, quad-cooperative
            constexpr unsigned kNoRow = 0x80000000u;               // outside the buffer: the load returns zeros
            const unsigned row0 = t.b * (unsigned)hot.S + (unsigned)T.start;
            const int pra = __mul24(f.ra, T.W), prb = __mul24(f.rb, T.W);
            const int pix[4] = {pra + f.ca, pra + f.cb, prb + f.ca, prb + f.cb};
            unsigned goff[4];
            float wsl[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                goff[k] = slow && f.m[k] ? (unsigned)(((row0 + (unsigned)pix[k]) * H + h) * (C * 4)) : kNoRow;
                wsl[k] = slow ? wk[k] * a[l] : 0.f;
            }
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) {
                if ((slow_lanes & (0x1111111111111111ull << tp)) == 0ull) continue;     // nobody's point tp
                dense_u32x4 rw[4][2];
                float wv_[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned oo = quad_bcast_u32(goff[k], tp) + (unsigned)p * 32u;
                    rw[k][0] = __builtin_amdgcn_raw_buffer_load_b128(rs, oo, 0, 0);
                    rw[k][1] = __builtin_amdgcn_raw_buffer_load_b128(rs, oo + 16u, 0, 0);
                    wv_[k] = __uint_as_float(quad_bcast_u32(__float_as_uint(wsl[k]), tp));
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned w8[8] = {rw[k][0].x, rw[k][0].y, rw[k][0].z, rw[k][0].w,
                                            rw[k][1].x, rw[k][1].y, rw[k][1].z, rw[k][1].w};
#pragma unroll
                    for (int i = 0; i < 8; ++i) accs[i] = fmaf(wv_[k], __uint_as_float(w8[i]), accs[i]);
                }
            }
        }
    }
#if !BOXATTN_DENSE_FROM_BOXES
    // how local were this wave's points (one tile in 61 reports, as the bf16 forward: boxattn_dense_fwd_body.h)
    if (stats && lane == 0 && role.id % 61u == 0u) {
        unsigned long long *slot = stats + 2 * (((role.id / 61u) * 4u + (unsigned)wv) & (kDenseStatSlots - 1));
        __hip_atomic_fetch_add(slot, (unsigned long long)n_slow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(slot + 1, (unsigned long long)n_act, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#endif
    // ---- the quad's four points -> the query's row: through LDS (the window buffer, after a barrier); lane p of the
    //      quad sums channels 8 p .. 8 p + 7 over the four points and adds the global path's sums
    __syncthreads();
    float *res = reinterpret_cast<float *>(win_lds) + (wv * kWave + lane) * 33;        // (33: conflict-free columns)
#pragma unroll
    for (int c = 0; c < 32; ++c) res[c] = acc[c];
    wave_lds_sync();
    const float *quad = reinterpret_cast<float *>(win_lds) + (wv * kWave + (lane & ~3)) * 33 + 8 * p;
    float o8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o8[i] = ((quad[i] + quad[33 + i]) + (quad[66 + i] + quad[99 + i])) + accs[i];
    if (vq) {
        float4 *dst = reinterpret_cast<float4 *>(out + (size_t)qh * C + 8 * p);
        dst[0] = make_float4(o8[0], o8[1], o8[2], o8[3]);
        dst[1] = make_float4(o8[4], o8[5], o8[6], o8[7]);
    }
