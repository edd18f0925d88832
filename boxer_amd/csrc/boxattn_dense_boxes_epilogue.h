// The epilogue of the window-staged point-gradient kernels from boxes (pointgrad_dense_boxes_kernel,
// pointgrad_dense_f32_boxes_kernel): included by their bodies (boxattn_dense_pg_body.h, boxattn_dense_f32_pg_body.h)
// where the per-point flavours store grad_loc / grad_attn.  In scope: lane (qi, p) of wave wv holds point p of every
// level of its (query, head) pair qh -- the weight a[l], its gradient ga[l] and the location gradient (gx[l], gy[l]).
// All 64 lanes are active (a query beyond the map's edge came in clamped: the DPP sum reads every lane of the quad);
// such a query (vq false) writes nothing.  No atomics, a fixed order of every sum: bitwise reproducible.  No include
// guard.
    // ---- the softmax Jacobian needs one sum over the pair's 4 L points: the lane's L levels in level order, then the quad
    float jac = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) jac += a[l] * ga[l];
    jac = group_sum<4>(jac);
    // ---- the box of level p again, with rw / rh (the lane that decoded it in the prologue; kept through the levels it
    //      would cost the main loop ten registers): requested here, in front of the barrier and the transposition
    // (the pair's index opaque from here on: the row offsets below are the prologue's, and knowing it the compiler keeps
    // those 64-bit products through the main loop -- 24 bytes of scratch in the 16-bit kernel of four levels)
    unsigned qe = qh;
    asm volatile("" : "+v"(qe));
    const int lr = min(p, L - 1);
    const float *orow = offsets + ((size_t)qe * L + lr) * (unsigned)gd.V;
    const GridBox box =
        grid_box_rows(ref + (size_t)(gd.ref_per_head ? qe : t.b * (unsigned)hot.Lq + q) * (unsigned)gd.ref_dim, orow,
                      vr != nullptr ? vr + ((size_t)t.b * L + lr) * 2 : nullptr, gd.angle_mode);
    // ---- lane (q, p) holds its point on every level, a box wants the four points of ITS level: transposed through
    //      (wave-private) LDS, the tiles of the per-point flavour, so that lane (q, j) reads level j's 4 points
    __syncthreads();                                               // every wave is done with the windows
    float *res = reinterpret_cast<float *>(win_lds) + wv * kDenseResFloats;
    float *res_a = res + qi * LP, *res_xy = res + 16 * LP + qi * LP * 2;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        res_a[l * P + p] = a[l] * (ga[l] - jac);                   // d / d logit (l, p)
        *reinterpret_cast<float2 *>(res_xy + (l * P + p) * 2) = make_float2(gx[l], gy[l]);
    }
    wave_lds_sync();
    if (vq && p < L) {
        const float4 o_a = *reinterpret_cast<const float4 *>(res_a + p * P);
        const float4 o_0 = *reinterpret_cast<const float4 *>(res_xy + p * P * 2);
        const float4 o_1 = *reinterpret_cast<const float4 *>(res_xy + p * P * 2 + 4);
        *reinterpret_cast<float4 *>(grad_logits + (size_t)qe * LP + p * P) = o_a;
        // the level's four points in point order (grid_bwd_kernel's shares, valid ratios included), then its row
        GridGrad bg{0.f, 0.f, 0.f, 0.f, 0.f};
        grid_grad_add(bg, box, kidx, 0, make_float2(o_0.x, o_0.y));
        grid_grad_add(bg, box, kidx, 1, make_float2(o_0.z, o_0.w));
        grid_grad_add(bg, box, kidx, 2, make_float2(o_1.x, o_1.y));
        grid_grad_add(bg, box, kidx, 3, make_float2(o_1.z, o_1.w));
        const size_t n = (size_t)qe * L + (unsigned)p;
        grid_grad_store(bg, box, orow, gd, grad_offsets + n * (unsigned)gd.V,
                        grad_ref_rows ? grad_ref_rows + n * 5 : nullptr);
    }
