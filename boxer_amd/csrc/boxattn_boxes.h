// Instance attention at inference straight from what the module predicts per (query, head, level): ONE box (reference
// window + 4 offsets) and 2 x 2 logits -- the walk of fwd_wide_kernel (boxattn_gather2.h: one wave per (query, head)
// pair, 64 / G lane groups over the pair's k x k points, `ws` waves sharing a pair through red[][], head = XCD
// placement, the l0 > 0 pass, register-kept mask rows; no atomics, no zero-fill) without its three per-point inputs.
// The (B,Lq,H,L,P,2) sampling grid and the (B,Lq,H,L,k,k) weight tensors -- written by grid_fwd_kernel and
// inst_weights_fwd_kernel to be read here once -- are never made:
//   prologue, once per wave   lane c takes logit c of the pair's 4 L and runs inst_cell_softmax (boxattn_cells.h) over
//                             the whole wave: it then holds a[c] / m^2 and t[c], what inst_weights_fwd_kernel
//                             replicates over the cell's m^2 points; lane (group, t) decodes the box of level t
//                             (grid_box, boxattn_grid.h) -- the box is the same for every point of the level;
//   step A                    the lane that does level l of point p = (y, x): grid_point on its box and the
//                             caller's kernel_indices row p (read through the cache, a step ahead), and its two
//                             weights by a cross-lane read from the lane of cell 4 l + 2 (y >= m) + (x >= m).
// Same device functions, same operation order (grid_box / grid_point keep their fp contract(off)) as the two kernels
// whose outputs it replaces, so locations and weights are theirs bit for bit.  Inference only: no riders.
// INST = false: mask_out NULL -- box attention with the spatial weights only, no level softmax kept, no mask rows.
#pragma once
#include "boxattn_cells.h"
#include "boxattn_gather2.h"
#include "boxattn_grid.h"

namespace boxattn {

struct BoxesDims {
    int k, m;                 // points a side, k / 2
    float rcp_k, inv_m2;      // 1 / k (small_div), 1 / m^2
};

template <typename ST, int G, int VEC, bool INST>
__global__ __launch_bounds__(256) void fwd_wide_boxes_kernel(
    const ST *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ lsi,
    const float *__restrict__ ref, const float *__restrict__ offsets, const float *__restrict__ kidx,
    const float *__restrict__ vr, const float *__restrict__ logits, int S, int H, int L, int Lq, int P,
    ST *__restrict__ out, typename ArgIf<INST, ST *__restrict__>::type mask, GridDims gd, BoxesDims bd,
    GatherIdx ix, unsigned value_bytes, unsigned ws)
{
    constexpr int C = VEC * G, NG = kWave / G;
    typedef Row<ST, VEC> RowT;
    constexpr int PSB = RowGeom<ST, VEC, G>::kPieceStride;
    constexpr int LCH = RowT::kLaneBytes / (int)sizeof(ST);
    __shared__ float red[kGatherWaves][VEC * G];
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
    ST *mk = nullptr;
    if constexpr (INST) mk = mask + (size_t)bq * P * HC + (size_t)h * C + slot * LCH;

    f32x2 acc[VEC / 2];
#pragma unroll
    for (int i = 0; i < VEC / 2; ++i) acc[i] = f32x2{0.f, 0.f};

    // The wave's first round trip carries everything it needs from memory besides value rows: its logits, the boxes
    // of its first level group, the first step's kernel_indices rows and the level table; every later step's
    // kernel_indices rows are requested a step ahead (1.5 KB at 14 x 14: they stay in the cache).
    struct Ahead { float kx, ky; };
    auto request = [&](int p0) -> Ahead {
        const int p = min(p0 + grp, P - 1);
        return Ahead{kidx[2 * p], kidx[2 * p + 1]};
    };
    const int pstep = (int)ws * NG;
    Ahead nxt = request((int)sub * NG);
    const GridBox box0 = grid_box(ref, offsets, vr, gd, n0 + (unsigned)min(slot, L - 1));
    float cell_a, cell_t;                                               // lane c: a[c] / m^2 and t[c] of the pair
    inst_cell_softmax<float, kWave>(logits, (size_t)qh, lane, L, cell_a, cell_t);
    cell_a *= bd.inv_m2;
    levels_commit(lv, lv_regs, L);
    if (ws == 1 && !live) return;

    for (int p0 = (int)sub * NG; live && p0 < P; p0 += pstep) {       // wave-uniform trip count
        const int p = p0 + grp;
        const bool have_p = p < P;
        const Ahead cur = nxt;
        if (p0 + pstep < P) nxt = request(p0 + pstep);
        const float kxy[2] = {cur.kx, cur.ky};
        // the point's 2 x 2 cell inside a level: 2 (y >= m) + (x >= m), p = y k + x
        const unsigned pc = (unsigned)min(p, P - 1);
        const int py = (int)small_div(pc, bd.rcp_k), px = (int)pc - py * bd.k;
        const int cell = (py >= bd.m ? 2 : 0) + (px >= bd.m ? 1 : 0);
        f32x2 macc[INST ? VEC / 2 : 1];
        if constexpr (INST) {
#pragma unroll
            for (int i = 0; i < VEC / 2; ++i) macc[i] = f32x2{0.f, 0.f};
        }
        for (int l0 = 0; l0 < L; l0 += G) {
            // ---- step A: lane t of the group -> level l0 + t of point p
            const int l = l0 + slot;
            const bool have = have_p && l < L;
            const int lc = min(l, L - 1);
            GridBox box = box0;
            if (l0 > 0) box = grid_box(ref, offsets, vr, gd, n0 + (unsigned)lc);   // (more levels than lanes in a group)
            const float2 xy = grid_point(box, kxy, 0, has_vr, 0);
            float as = __shfl(cell_a, 4 * lc + cell, kWave), al = 0.f;
            if constexpr (INST) al = __shfl(cell_t, 4 * lc + cell, kWave);
            as = have ? as : 0.f;
            al = have ? al : 0.f;
            const Sample<float> s = locate<float>(xy.x, xy.y, lv.h[lc], lv.w[lc]);
            const u32x4_t my_off =
                corner_offsets<ST>(s, b * (unsigned)S + (unsigned)lv.start[lc], H, h, C, have);
            const u32x4_t my_wt = as_u32x4(s.hh * s.hw, s.hh * s.lw, s.lh * s.hw, s.lh * s.lw);
            // ---- step B: the G lanes walk the group's levels together, four at a time (fwd_wide_kernel)
            constexpr int UL = 4;
#pragma unroll
            for (int t0 = 0; t0 < G; t0 += UL) {
                if (l0 + t0 >= L) break;                         // wave-uniform
                u32x4_t off[UL], wt[UL];
                unsigned aas[UL], aal[UL];
                RowT v[UL][4];
#pragma unroll
                for (int u = 0; u < UL; ++u) {
                    const int t = t0 + u;
                    off[u] = u32x4_t{group_bcast<G>(my_off.x, t, lane), group_bcast<G>(my_off.y, t, lane),
                                     group_bcast<G>(my_off.z, t, lane), group_bcast<G>(my_off.w, t, lane)};
                    wt[u] = u32x4_t{group_bcast<G>(my_wt.x, t, lane), group_bcast<G>(my_wt.y, t, lane),
                                    group_bcast<G>(my_wt.z, t, lane), group_bcast<G>(my_wt.w, t, lane)};
                    aas[u] = group_bcast<G>(__float_as_uint(as), t, lane);
                    if constexpr (INST) aal[u] = group_bcast<G>(__float_as_uint(al), t, lane);
                    else aal[u] = 0u;
                    row_load<ST, VEC, PSB>(rs, off[u].x + lane_off, v[u][0]);
                    row_load<ST, VEC, PSB>(rs, off[u].y + lane_off, v[u][1]);
                    row_load<ST, VEC, PSB>(rs, off[u].z + lane_off, v[u][2]);
                    row_load<ST, VEC, PSB>(rs, off[u].w + lane_off, v[u][3]);
                }
                loads_issued();
#pragma unroll
                for (int u = 0; u < UL; ++u) {
                    f32x2 val[VEC / 2];
#pragma unroll
                    for (int i = 0; i < VEC / 2; ++i) val[i] = f32x2{0.f, 0.f};
                    row_axpy<ST, VEC>(val, __uint_as_float(wt[u].x), v[u][0]);
                    row_axpy<ST, VEC>(val, __uint_as_float(wt[u].y), v[u][1]);
                    row_axpy<ST, VEC>(val, __uint_as_float(wt[u].z), v[u][2]);
                    row_axpy<ST, VEC>(val, __uint_as_float(wt[u].w), v[u][3]);
                    const float a_s = __uint_as_float(aas[u]), a_l = __uint_as_float(aal[u]);
                    const f32x2 as2 = {a_s, a_s}, al2 = {a_l, a_l};
#pragma unroll
                    for (int i = 0; i < VEC / 2; ++i) {
                        acc[i] = __builtin_elementwise_fma(val[i], as2, acc[i]);
                        if constexpr (INST) macc[i] = __builtin_elementwise_fma(val[i], al2, macc[i]);
                    }
                }
            }
        }
        if constexpr (INST) {
            if (have_p) row_store<ST, VEC, PSB>(mk + (size_t)p * HC, macc);
        }
    }
    // out = sum over the lane groups (lanes with the same channel chunk: stride G)
#pragma unroll
    for (int o = G; o < kWave; o <<= 1)
#pragma unroll
        for (int i = 0; i < VEC / 2; ++i) {
            acc[i].x += __shfl_xor(acc[i].x, o, kWave);
            acc[i].y += __shfl_xor(acc[i].y, o, kWave);
        }
    if (ws > 1) {                                                       // ... and over the pair's waves
        if (grp == 0) {
#pragma unroll
            for (int i = 0; i < VEC / 2; ++i)
                *reinterpret_cast<f32x2 *>(&red[wv][slot * VEC + 2 * i]) = acc[i];
        }
        __syncthreads();
        if (sub != 0 || !live) return;
        if (grp == 0) {
            for (unsigned s = 1; s < ws; ++s)
#pragma unroll
                for (int i = 0; i < VEC / 2; ++i) {
                    const f32x2 o = *reinterpret_cast<const f32x2 *>(&red[wv + s][slot * VEC + 2 * i]);
                    acc[i].x += o.x;
                    acc[i].y += o.y;
                }
        }
    }
    if (grp == 0) row_store<ST, VEC, PSB>(out + (size_t)qh * C + slot * LCH, acc);
}

}  // namespace boxattn
