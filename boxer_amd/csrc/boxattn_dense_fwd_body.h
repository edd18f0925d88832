// The body of the window-staged 16-bit forward (boxattn_dense_fwd.h), included once into each of its two kernels:
// BOXATTN_DENSE_FROM_BOXES 0 -- fwd_dense_kernel, the per-point inputs loc / attn are read, riders and locality
// statistics; 1 -- fwd_dense_boxes_kernel, they are made from the boxes and logits (boxattn_dense_boxes.h), inference
// only.  Text inclusion, not a shared __device__ function: behind two __global__ wrappers the existing kernel came
// out with other instructions.  No include guard.
    constexpr int C = 32;
    constexpr int kBias = 4096;                         // keeps the packed slot offset non-negative
    constexpr int kZeroOff = kDenseZeroOff;
    __shared__ __attribute__((aligned(16))) unsigned char win_lds[kDenseLdsBytes];
    const int lane = threadIdx.x & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
#if BOXATTN_DENSE_FROM_BOXES
    const unsigned tile_block = blockIdx.x;                        // no riders
#else
    // training forward: the backward's count pass and the scans chained behind it ride in this launch
    // (boxattn_ride.h, bin_count_ride)
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
    if (t.lq < 0) return;                                          // workgroup-uniform
    const int H = hot.H, h = t.h;
    // ---- lane -> (query of the wave's 4x4 sub-tile, lane of its quad)
    const int qi = lane >> 2, r = lane & 3;
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
        __builtin_amdgcn_make_buffer_rsrc(const_cast<ST *>(value), 0, value_bytes, 0x00020000);
    DenseWinPos win[L];
    dense_stage_issue<L>(hot, wrow, t, lane, wv, rs, win_lds, win);
    float2 xy[L];
    float a[L];
#if BOXATTN_DENSE_FROM_BOXES
    // lane r of the quad: point r of every level, from the query's boxes and logits (behind the window requests)
    dense_boxes_points<L>(ref, offsets, kidx, vr, logits, gd, t.b, t.b * (unsigned)hot.Lq + q, qh, r, xy, a);
#else
#pragma unroll
    for (int l = 0; l < L; ++l) {                                  // lane r of the quad: point r of every level
        xy[l] = loc2[pt0 + l * P + r];
        a[l] = attn[pt0 + l * P + r];
    }
#endif
    if (threadIdx.x < 4)
        *reinterpret_cast<dense_u32x4 *>(win_lds + kZeroOff + 16 * threadIdx.x) = dense_u32x4{0u, 0u, 0u, 0u};
    dense_stage_wait();                                            // windows complete

    // supplier role inside the 16-lane group: the row of corner jc for the query of quad qs
    const int jc = (lane >> 2) & 3, qs = lane & 3;
    const unsigned odd_mask = 0u - (unsigned)(lane & 1);
    const int src_lane4 = ((lane & 48) + 4 * qs) * 4;              // ds_bpermute address of lane 0 of that quad
#if !BOXATTN_DENSE_FROM_BOXES
    unsigned n_slow = 0, n_act = 0;                                // locality statistics of this wave (stats != nullptr)
#endif
    fwd_f32x4 acc[8];                                              // matrix cores: channel 4 m + r, rows = weight terms
    float accv[8];                                                 // VALU (global path): channels 8 r .. 8 r + 7
#pragma unroll
    for (int m = 0; m < 8; ++m) { acc[m] = fwd_f32x4{0.f, 0.f, 0.f, 0.f}; accv[m] = 0.f; }
#if BOXATTN_DENSE_FROM_BOXES
    // (opaque zeros: knowing the sums to be zero the compiler specialises the first level for it, and with the copies
    // between the two versions the bf16 kernel of 3 levels spilled 7 registers around its global path; 78-93 this way)
#pragma unroll
    for (int m = 0; m < 8; ++m) asm volatile("" : "+v"(acc[m]), "+v"(accv[m]));
#endif
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const DenseMap T = hot.lv[l];
        const DenseWinPos &o = win[l];
        const DensePoint s = dense_locate(xy[l].x, xy[l].y, T.H, T.W);
        const int rows = o.rows(), cols = o.cols();
        const int Hm1 = T.H - 1, Wm1 = T.W - 1;
        // which corners count (bit k), and is the footprint inside the staged window
        const unsigned mr0 = ~(unsigned)(s.y0 >> 31), mr1 = (unsigned)((s.y0 - Hm1) >> 31);
        const unsigned mc0 = ~(unsigned)(s.x0 >> 31), mc1 = (unsigned)((s.x0 - Wm1) >> 31);
        const unsigned bits = ((mr0 & mc0) & 1u) | ((mr0 & mc1) & 2u) | ((mr1 & mc0) & 4u) | ((mr1 & mc1) & 8u);
        const int ra = max(s.y0, 0), rb = min(s.y0 + 1, Hm1), ca = max(s.x0, 0), cb = min(s.x0 + 1, Wm1);
        const int d = min(min(ra - o.y0, o.y0 + rows - 1 - rb), min(ca - o.x0, o.x0 + cols - 1 - cb));
        const bool act = vq && s.inside;
        const bool fast = act && d >= 0, slow = act && d < 0;
        const int pitchb = o.pitchb(), offb = o.offb();
        const int slot0 = offb + __mul24(s.y0 - o.y0, pitchb) + __mul24(s.x0 - o.x0, kDenseSlotBytes) + kBias;
        const unsigned pack = fast ? ((unsigned)slot0 | (bits << 20)) : 0u;
        // the four corner weights x attention weight; for the matrix cores as hi + lo bf16 terms
        const float aa = s.inside ? a[l] : 0.f;
        const float ha = s.hh * aa, la = s.lh * aa;
        const float wk[4] = {ha * s.hw, ha * s.lw, la * s.hw, la * s.lw};
        typedef Half16<ST> H16;
        const unsigned hi01 = H16::pack(wk[0], wk[1]), hi23 = H16::pack(wk[2], wk[3]);
        const unsigned lo01 = H16::pack(wk[0] - H16::lo(hi01), wk[1] - H16::hi(hi01));
        const unsigned lo23 = H16::pack(wk[2] - H16::lo(hi23), wk[3] - H16::hi(hi23));
        const int dj = (jc & 1) * kDenseSlotBytes + (jc >> 1) * pitchb - kBias;       // my corner relative to the packed slot
        // A operand: lane i of a quad holds row i -- rows 0, 2: the hi terms, rows 1, 3: the lo terms of the point
        // the quad is working on.  Arranged once per level so that ONE quad permute per register and point
        // delivers it: z_[0] = {hi(0), lo(0), hi(1), lo(1)} by lane, z_[1] = {hi(2), lo(2), hi(3), lo(3)}
        // (bitwise merges, not ?: -- the compiler turns a select of two DPP moves into a branch and runs each move
        // with half of the lanes switched off, where a DPP read of a disabled lane returns 0)
        unsigned z01[2], z23[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            z01[u] = (quad_pairs_u32(lo01, u) & odd_mask) | (quad_pairs_u32(hi01, u) & ~odd_mask);
            z23[u] = (quad_pairs_u32(lo23, u) & odd_mask) | (quad_pairs_u32(hi23, u) & ~odd_mask);
        }
        if (rows > 0 && __builtin_amdgcn_ballot_w64(fast) != 0ull) {   // (wave-uniform: staged, and somebody reads it)
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) {
                const unsigned pk = (unsigned)__builtin_amdgcn_ds_bpermute(src_lane4 + 4 * tp, (int)pack);
                const bool counts = ((pk >> (20 + jc)) & 1u) != 0u;
                const int addr = counts ? (int)(pk & 0xfffffu) + dj : kZeroOff;
                const unsigned a0 = quad_evenodd_u32(z01[tp >> 1], tp & 1), a1 = quad_evenodd_u32(z23[tp >> 1], tp & 1);
                const uint2 av = uint2{a0, a1};
                typedef __attribute__((address_space(3))) fwd_i16x4 lds_vec;
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    const fwd_i16x4 bv = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_vec *)(win_lds + addr + 8 * m));
                    acc[m] = H16::mfma4x4x4(av, __builtin_bit_cast(uint2, bv), acc[m]);
                }
            }
        }
        const unsigned long long slow_lanes = __builtin_amdgcn_ballot_w64(slow);
#if !BOXATTN_DENSE_FROM_BOXES
        n_slow += (unsigned)__builtin_popcountll(slow_lanes);
        n_act += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(act));
#endif
        if (slow_lanes != 0ull) {                                  // wave-uniform: the global path
            constexpr unsigned kNoRow = 0x80000000u;               // outside the buffer: the load returns zeros
            const unsigned row0 = t.b * (unsigned)hot.S + (unsigned)T.start;
            const int pra = __mul24(ra, T.W), prb = __mul24(rb, T.W);
            const int pix[4] = {pra + ca, pra + cb, prb + ca, prb + cb};
            unsigned goff[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                goff[k] = slow && ((bits >> k) & 1u) ? (unsigned)(((row0 + (unsigned)pix[k]) * H + h) * (C * 2)) : kNoRow;
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) {
                if ((slow_lanes & (0x1111111111111111ull << tp)) == 0ull) continue;     // nobody's point tp
                dense_u32x4 rw[4];
                float wv_[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    rw[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, quad_bcast_u32(goff[k], tp) + (unsigned)r * 16u, 0, 0);
                    wv_[k] = __uint_as_float(quad_bcast_u32(__float_as_uint(wk[k]), tp));
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned w4[4] = {rw[k].x, rw[k].y, rw[k].z, rw[k].w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        accv[2 * i] = fmaf(wv_[k], H16::lo(w4[i]), accv[2 * i]);
                        accv[2 * i + 1] = fmaf(wv_[k], H16::hi(w4[i]), accv[2 * i + 1]);
                    }
                }
            }
        }
    }
#if !BOXATTN_DENSE_FROM_BOXES
    // How local were this wave's points?  {points served from global memory, points inside the window test}
    // into one of kDenseStatSlots pairs of monotonic 64-bit counters of the caller's state buffer -- from one tile
    // in 61 only (a prime: the sample walks through the XCDs' bands of the map; every wave of every tile doing it
    // was 15 k same-line atomics, +20 us).  Fire and forget: nobody waits for these atomics.  The caller reads the
    // counters now and then and, when most points miss their windows, asks for the row-gather kernels instead
    // (hints, include/boxattn.h).
    if (stats && lane == 0 && role.id % 61u == 0u) {
        unsigned long long *slot = stats + 2 * (((role.id / 61u) * 4u + (unsigned)wv) & (kDenseStatSlots - 1));
        __hip_atomic_fetch_add(slot, (unsigned long long)n_slow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(slot + 1, (unsigned long long)n_act, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#endif
    // ---- lane r of the quad holds channels r, 4 + r, .. 28 + r from the matrix cores: through LDS into the
    //      channel-contiguous order of the VALU sums, then one 16-byte piece of the query's row per lane
    constexpr int kResPitch = 36;                                  // floats per query (16-byte aligned rows, 2-way banks)
    __syncthreads();                                               // every wave is done with the windows
    float *res = reinterpret_cast<float *>(win_lds) + (wv * 16 + qi) * kResPitch;
#pragma unroll
    for (int m = 0; m < 8; ++m) res[4 * m + r] = acc[m][0] + acc[m][1];
    wave_lds_sync();
    const float4 x0 = *reinterpret_cast<const float4 *>(res + 8 * r), x1 = *reinterpret_cast<const float4 *>(res + 8 * r + 4);
    if (vq) {
        dense_u32x4 o4;
        o4.x = Half16<ST>::pack(x0.x + accv[0], x0.y + accv[1]);
        o4.y = Half16<ST>::pack(x0.z + accv[2], x0.w + accv[3]);
        o4.z = Half16<ST>::pack(x1.x + accv[4], x1.y + accv[5]);
        o4.w = Half16<ST>::pack(x1.z + accv[6], x1.w + accv[7]);
        *reinterpret_cast<dense_u32x4 *>(out + (size_t)qh * C + 8 * r) = o4;
    }
