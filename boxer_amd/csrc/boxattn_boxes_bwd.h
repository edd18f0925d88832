// Instance attention's backward straight to what the module needs per (query, head, level): the gradients of ONE box
// (4 offsets, 5 reference-window terms) and of the 2 x 2 logits -- the walk of fwd_wide_boxes_kernel (boxattn_boxes.h)
// with the corner sums and the finish of pointgrad2_kernel<.., WP> (boxattn_gather2.h).  The per-point tensors are
// neither read nor written: locations and weights are recomputed from the boxes and logits as in the forward (same
// device functions: bit for bit what it sampled), and a point's (gx, gy), gs and gl go into running sums in registers
// instead of grad_loc / grad_sw / grad_lw for grid_bwd_kernel and inst_weights_bwd_kernel to reduce:
//   lane (group, t) stays on level l0 + t for a whole pass over the pair's points, so its sums are one GridGrad
//   (grid_grad_add) and two InstCellSums (inst_cell_add, by the point's (y >= m, x >= m)); more levels than lanes in
//   a group: one pass per level group, the sums are handed over at the end of each;
//   the grad_mask row of a point is shared by the levels of its group: one load per point and pass;
//   epilogue: sum over the lane groups (__shfl_xor, strides G .. 32) into sums[wave][level][13] in LDS, over the
//   pair's `ws` waves in wave order, then lane l: grid_grad_store of level l, lane c: the logit gradient of cell c
//   (boxattn_pointwise.h: a[c] / m^2 (Gs[c] - sum a Gs) + t[c] (Gt[c] - sum_l t Gt)).
// No atomics, no split over blockIdx.y, fixed summation order: bitwise reproducible.
// INST = false: grad_mask NULL (the mask output took no part in the loss) -- no m* corner sums, no level term.
#pragma once
#include "boxattn_boxes.h"

namespace boxattn {

constexpr int kBoxGradTerms = 13;          // GridGrad (5) + InstCellSums of the spatial (4) and the level weights (4)

template <typename ST, int G, int VEC, bool INST>
__global__ __launch_bounds__(256) void pointgrad_boxes_kernel(
    const ST *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ lsi,
    const float *__restrict__ ref, const float *__restrict__ offsets, const float *__restrict__ kidx,
    const float *__restrict__ vr, const float *__restrict__ logits, const ST *__restrict__ grad_out,
    typename ArgIf<INST, const ST *__restrict__>::type grad_mask, int S, int H, int L, int Lq, int P,
    float *__restrict__ grad_offsets, float *__restrict__ grad_ref_rows, float *__restrict__ grad_logits,
    GridDims gd, BoxesDims bd, GatherIdx ix, unsigned value_bytes, unsigned ws)
{
    constexpr int C = VEC * G, NG = kWave / G;
    typedef Row<ST, VEC> RowT;
    constexpr int PSB = RowGeom<ST, VEC, G>::kPieceStride;
    constexpr int LCH = RowT::kLaneBytes / (int)sizeof(ST);
    constexpr int UL = sizeof(ST) == 2 ? 4 : 2;                         // levels of a point in flight
    __shared__ float sums[kGatherWaves][16][kBoxGradTerms];             // (odd stride: the levels on different banks)
    __shared__ LevelTable lv;
    const LevelRegs lv_regs = levels_request(shapes, lsi, L);           // published below, behind the first loads

    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const unsigned blk = blockIdx.x;
    // `ws` (1, 2, 4) waves share a pair: wave `sub` of them takes the point steps sub, sub + ws, ...
    const unsigned ppw = kGatherWaves / ws, sub = wv % ws;
    unsigned qh = blk * ppw + wv / ws;
    if (ix.head_xcd)                                                    // head = XCD (pair_of_lane)
        qh = ((blk / 8) * ppw + wv / ws) * (unsigned)H + blk % 8;
    const bool live = qh < ix.n_qh;                                     // wave-uniform
    qh = min(qh, ix.n_qh - 1u);
    const int slot = lane % G, grp = lane / G;
    unsigned bq, hu, b, qu;
    divmod_magic(qh, (unsigned)H, ix.magic_h, bq, hu);
    divmod_magic(bq, (unsigned)Lq, ix.magic_lq, b, qu);
    const int h = (int)hu;
    const size_t HC = (size_t)H * C;
    const size_t n0 = (size_t)qh * L;                                   // the pair's first (b, q, h, l) row
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<ST *>(value), 0, value_bytes, 0x00020000);
    const unsigned lane_off = (unsigned)(slot * RowT::kLaneBytes);
    const bool has_vr = vr != nullptr;
    const ST *gmk = nullptr;
    if constexpr (INST) gmk = grad_mask + (size_t)bq * P * HC + (size_t)h * C + slot * LCH;

    // first round trip, as in the forward: the logits, the boxes of the first level group, the first step's
    // kernel_indices rows, the level table -- and the pair's grad_out row
    struct Ahead { float kx, ky; };
    auto request = [&](int p0) -> Ahead {
        const int p = min(p0 + grp, P - 1);
        return Ahead{kidx[2 * p], kidx[2 * p + 1]};
    };
    const int pstep = (int)ws * NG;
    Ahead nxt = request((int)sub * NG);
    RowT g;
    row_load<ST, VEC, PSB>(grad_out + (size_t)qh * C + slot * LCH, g);
    const GridBox box0 = grid_box(ref, offsets, vr, gd, n0 + (unsigned)min(slot, L - 1));
    float cell_a, cell_t;                                               // lane c: a[c] and t[c] of the pair
    inst_cell_softmax<float, kWave>(logits, (size_t)qh, lane, L, cell_a, cell_t);
    const float cell_am = cell_a * bd.inv_m2;                           // a[c] / m^2: the spatial weight of a point
    levels_commit(lv, lv_regs, L);

    for (int l0 = 0; l0 < L; l0 += G) {                                 // (one pass unless L > G)
        // ---- this lane's level of the pass
        const int l = l0 + slot;
        const int lc = min(l, L - 1);
        GridBox box = box0;
        if (l0 > 0) {
            box = grid_box(ref, offsets, vr, gd, n0 + (unsigned)lc);
            nxt = request((int)sub * NG);
        }
        const int Hl = lv.h[lc], Wl = lv.w[lc];
        const unsigned row0 = b * (unsigned)S + (unsigned)lv.start[lc];
        GridGrad ga{0.f, 0.f, 0.f, 0.f, 0.f};
        InstCellSums gs{0.f, 0.f, 0.f, 0.f}, gl{0.f, 0.f, 0.f, 0.f};

        for (int p0 = (int)sub * NG; live && p0 < P; p0 += pstep) {   // wave-uniform trip count
            const int p = p0 + grp;
            const bool have = p < P && l < L;
            const Ahead cur = nxt;
            if (p0 + pstep < P) nxt = request(p0 + pstep);
            const float kxy[2] = {cur.kx, cur.ky};
            const unsigned pc = (unsigned)min(p, P - 1);
            const int py = (int)small_div(pc, bd.rcp_k), px = (int)pc - py * bd.k;
            const bool hi_y = py >= bd.m, hi_x = px >= bd.m;
            const int cell = (hi_y ? 2 : 0) + (hi_x ? 1 : 0);
            // ---- step A: lane t of the group -> level l0 + t of point p
            const float2 xy = grid_point(box, kxy, 0, has_vr, 0);
            const float as = __shfl(cell_am, 4 * lc + cell, kWave);
            float al = 0.f;
            if constexpr (INST) al = __shfl(cell_t, 4 * lc + cell, kWave);
            const Sample<float> s = locate<float>(xy.x, xy.y, Hl, Wl);
            const u32x4_t my_off = corner_offsets<ST>(s, row0, H, h, C, have);
            RowT gm;
            if constexpr (INST) row_load<ST, VEC, PSB>(gmk + (size_t)pc * HC, gm);
            // ---- step B: corner sums of the group's levels (pointgrad2_kernel)
            float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;             // S_k of "my" level (slot)
            float m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;             // instance: sums with grad_mask
#pragma unroll
            for (int t0 = 0; t0 < G; t0 += UL) {
                if (l0 + t0 >= L) break;                              // wave-uniform
                RowT v[UL][4];
#pragma unroll
                for (int u = 0; u < UL; ++u) {
                    const int t = t0 + u;
                    const u32x4_t off = u32x4_t{group_bcast<G>(my_off.x, t, lane), group_bcast<G>(my_off.y, t, lane),
                                                group_bcast<G>(my_off.z, t, lane), group_bcast<G>(my_off.w, t, lane)};
                    row_load<ST, VEC, PSB>(rs, off.x + lane_off, v[u][0]);
                    row_load<ST, VEC, PSB>(rs, off.y + lane_off, v[u][1]);
                    row_load<ST, VEC, PSB>(rs, off.z + lane_off, v[u][2]);
                    row_load<ST, VEC, PSB>(rs, off.w + lane_off, v[u][3]);
                }
                loads_issued();
#pragma unroll
                for (int u = 0; u < UL; ++u) {
                    const float a1 = group_sum<G>(row_dot<ST, VEC>(g, v[u][0]));
                    const float a2 = group_sum<G>(row_dot<ST, VEC>(g, v[u][1]));
                    const float a3 = group_sum<G>(row_dot<ST, VEC>(g, v[u][2]));
                    const float a4 = group_sum<G>(row_dot<ST, VEC>(g, v[u][3]));
                    const bool mine = slot == t0 + u;
                    s1 = mine ? a1 : s1; s2 = mine ? a2 : s2; s3 = mine ? a3 : s3; s4 = mine ? a4 : s4;
                    if constexpr (INST) {
                        const float b1 = group_sum<G>(row_dot<ST, VEC>(gm, v[u][0]));
                        const float b2 = group_sum<G>(row_dot<ST, VEC>(gm, v[u][1]));
                        const float b3 = group_sum<G>(row_dot<ST, VEC>(gm, v[u][2]));
                        const float b4 = group_sum<G>(row_dot<ST, VEC>(gm, v[u][3]));
                        m1 = mine ? b1 : m1; m2 = mine ? b2 : m2; m3 = mine ? b3 : m3; m4 = mine ? b4 : m4;
                    }
                }
            }
            // ---- finish: lane (group, slot) owns level l0 + slot of point p (pointgrad2_kernel's formulas)
            const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
            const bool keep = have && s.inside;                         // a point outside the map: zeros
            float gx, gy, gw = w1 * s1 + w2 * s2 + w3 * s3 + w4 * s4;
            if constexpr (!INST) {
                gx = (float)Wl * as * (s.hh * (s2 - s1) + s.lh * (s4 - s3));
                gy = (float)Hl * as * (s.hw * (s3 - s1) + s.lw * (s4 - s2));
            } else {
                const float t1 = as * s1 + al * m1, t2 = as * s2 + al * m2;
                const float t3 = as * s3 + al * m3, t4 = as * s4 + al * m4;
                gx = (float)Wl * (s.hh * (t2 - t1) + s.lh * (t4 - t3));
                gy = (float)Hl * (s.hw * (t3 - t1) + s.lw * (t4 - t2));
                const float gt = w1 * m1 + w2 * m2 + w3 * m3 + w4 * m4;
                inst_cell_add(gl, hi_y, hi_x, keep ? gt : 0.f);
            }
            gx = keep ? gx : 0.f;
            gy = keep ? gy : 0.f;
            gw = keep ? gw : 0.f;
            grid_grad_add(ga, box, kxy, 0, make_float2(gx, gy));
            inst_cell_add(gs, hi_y, hi_x, gw);
        }

        // ---- the pass's sums over the lane groups (lanes on the same level: stride G), handed over in LDS
        float acc[kBoxGradTerms] = {ga.cx, ga.cy, ga.w, ga.h, ga.t, gs.c0, gs.c1, gs.c2, gs.c3,
                                    gl.c0, gl.c1, gl.c2, gl.c3};
#pragma unroll
        for (int o = G; o < kWave; o <<= 1)
#pragma unroll
            for (int i = 0; i < kBoxGradTerms; ++i) acc[i] += __shfl_xor(acc[i], o, kWave);
        if (grp == 0 && l < L) {
#pragma unroll
            for (int i = 0; i < kBoxGradTerms; ++i) sums[wv][l][i] = acc[i];
        }
    }
    __syncthreads();
    if (sub != 0 || !live) return;

    // ---- epilogue, the pair's first wave: lane l -> the box of level l, lane c -> cell c
    if (lane < L) {
        GridGrad a{0.f, 0.f, 0.f, 0.f, 0.f};
        for (unsigned s = 0; s < ws; ++s) {
            const float *r = sums[wv + s][lane];
            a.cx += r[0]; a.cy += r[1]; a.w += r[2]; a.h += r[3]; a.t += r[4];
        }
        const size_t n = n0 + (unsigned)lane;
        const GridBox box = grid_box(ref, offsets, vr, gd, n);
        grid_grad_store(a, box, offsets + n * 4, gd, grad_offsets + n * 4,
                        grad_ref_rows ? grad_ref_rows + n * 5 : nullptr);
    }
    const bool cell_live = lane < 4 * L;
    float Gs = 0.f, Gt = 0.f;
    if (cell_live) {
        for (unsigned s = 0; s < ws; ++s) {
            const float *r = sums[wv + s][lane / 4];
            Gs += r[5 + lane % 4];
            if constexpr (INST) Gt += r[9 + lane % 4];
        }
    }
    const float dot_s = lanes_add<1, kWave>(cell_a * Gs);
    float gz = cell_a * bd.inv_m2 * (Gs - dot_s);
    if constexpr (INST) {
        const float dot_t = lanes_add<4, kWave>(cell_t * Gt);
        gz += cell_t * (Gt - dot_t);
    }
    if (cell_live) grad_logits[(size_t)qh * (size_t)(4 * L) + lane] = gz;
}

}  // namespace boxattn
