// Box attention's backward straight to what BoxAttention / Box3dAttention need per (query, head): the gradients of L
// boxes (4 or 5 offsets, 5 reference-window terms a level) and of the L P logits -- the geometry of fwd2_boxes_kernel
// (boxattn_gather2_boxes.h: a lane group of G = C / VEC lanes per (query, head) pair, pair_of_lane placement with
// head = XCD, buffer loads) with the corner sums and the finish of pointgrad2_kernel (boxattn_gather2.h).  The
// per-point tensors are neither read nor written: locations and weights are recomputed from the boxes and logits by the
// forward's device functions in its operation order (bit for bit what it sampled), and a point's (gx, gy) and gw go into
// sums instead of grad_loc / grad_attn for grid_bwd_kernel and the softmax backward to reduce:
//   prologue   the forward's softmax over the pair's L P logits (lane `slot` takes logits slot, slot + G, ...; DPP
//              maximum and sum; a = exp(z - max) * (1 / sum)); the weights go to a wave-private piece of LDS;
//   passes     lane (pair, t) stays on level l0 + t for a whole pass over the P points of a level (the hand-out of
//              pointgrad_boxes_kernel), so the level's box -- decoded once by grid_box_rows, with rw / rh -- and its
//              five box terms (GridGrad, grid_grad_add in point order) stay in that lane's registers.  Step A: the
//              lane's point (l0 + t, p); step B: the G lanes walk the levels of the pass together (row_dot, group_sum);
//              finish: gw to the pair's piece of LDS, (gx, gy) into the running sums.  After the pass the lane runs
//              grid_grad_store for its level.  More levels than lanes: one pass per G levels;
//   epilogue   lane `slot` takes logits slot, slot + G, ... again: grad_logits = a (gw - sum a gw), the sum over the
//              lane's rounds in order, then over the group with DPP.
// No atomics, no split over workgroups, fixed summation order: bitwise reproducible.  LDS: 2 L P floats a pair, read
// and written 4 bytes at a time (nothing here depends on where the dynamic region starts).
//
// Two compile-time flags in the manner of bwd_fast_kernel (boxattn_fast.h): POINTS, the three parameter gradients above,
// and SCATTER, grad_value in the same launch.  SCATTER: in step B the owner lane of level l0 + t broadcasts a w_k of its
// point (a: the softmax weight) next to the corner offsets, and every lane of the group adds a w_k g[c] for its channels
// into the float32 accumulator at the row the offset names -- one hardware atomic an element (atomic_add), issued only
// where the corner is inside the map, the level exists and the pair is real (a predicate, not a product with zero: a
// clamped address never receives an add and a non-finite grad_out row reaches only the rows its points touch).  The
// order of these adds is the hardware's: grad_value of this kernel is NOT bitwise reproducible; the parameter gradients
// of the SCATTER + POINTS flavour are the POINTS flavour's instructions in its order and still are.  Without POINTS:
// no corner loads, no dots, no gw, no box terms and no epilogue -- softmax, geometry and the adds.
#pragma once
#include "boxattn_gather2_boxes.h"

namespace boxattn {

// floats of wave-private LDS a pair takes: its L P weights, then its L P gw
inline __host__ __device__ unsigned bwd2_boxes_pair_stride(int LP) { return 2u * (unsigned)LP; }

extern __shared__ float bwd2_boxes_dyn[];        // 4 waves x 64 / G pairs x bwd2_boxes_pair_stride

// the lane's channels of one corner row: acc[row + c] += aw * g[c]; `byte`: the row's byte offset in `value` plus the
// lane's (the pieces of a lane as row_load fetches them)
template <typename ST, int VEC, int PSB>
__device__ __forceinline__ void row_scatter(float *__restrict__ acc, unsigned byte, float aw, const Row<ST, VEC> &g)
{
    constexpr int NW = Row<ST, VEC>::NW, WPP = NW / Row<ST, VEC>::NP;   // words of a piece
    float *row = acc + byte / (unsigned)sizeof(ST);                      // byte offset in value -> element index
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        float *d = row + ((j / WPP) * PSB + (j % WPP) * 4) / (int)sizeof(ST);
        if constexpr (sizeof(ST) == 4) {
            atomic_add(d, aw * __uint_as_float(g.w[j]));
        } else {
            atomic_add(d, aw * Half16<ST>::lo(g.w[j]));
            atomic_add(d + 1, aw * Half16<ST>::hi(g.w[j]));
        }
    }
}

template <typename ST, int G, int U, int VEC, bool SCATTER = false, bool POINTS = true>
__global__ __launch_bounds__(256) void bwd2_boxes_kernel(
    const ST *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ lsi,
    const float *__restrict__ ref, const float *__restrict__ offsets, const float *__restrict__ kidx,
    const float *__restrict__ vr, const float *__restrict__ logits, const ST *__restrict__ grad_out, int S, int H,
    int L, int Lq, int P, float *__restrict__ grad_offsets, float *__restrict__ grad_ref_rows,
    float *__restrict__ grad_logits, GridDims gd, GatherIdx ix, unsigned value_bytes, unsigned pair_stride,
    float *__restrict__ grad_value_acc)
{
    static_assert(SCATTER || POINTS, "nothing to compute");
    constexpr int C = VEC * G, PAIRS = kWave / G, NZ = kBoxesMaxLP / G;
    typedef Row<ST, VEC> RowT;
    constexpr int PSB = RowGeom<ST, VEC, G>::kPieceStride;    // bytes between a lane's pieces
    constexpr int LCH = RowT::kLaneBytes / (int)sizeof(ST);   // channels of one piece
    __shared__ LevelTable lv;
    __shared__ float2 kidx_lds[kBoxesMaxLP];
    const LevelRegs lv_regs = levels_request(shapes, lsi, L);   // published below, behind the first loads

    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    bool active;
    const unsigned qh = pair_of_lane<PAIRS>(ix, blockIdx.x, H, lane / G, wv, active);
    const int slot = lane % G;                      // step A: level slot; step B: channel chunk
    unsigned bq, hu, b, qu;
    divmod_magic(qh, (unsigned)H, ix.magic_h, bq, hu);
    divmod_magic(bq, (unsigned)Lq, ix.magic_lq, b, qu);
    const int h = (int)hu;
    const int LP = L * P;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<ST *>(value), 0, value_bytes, 0x00020000);
    const unsigned lane_off = (unsigned)(slot * RowT::kLaneBytes);
    const bool has_vr = vr != nullptr;
    const int angle_mode = gd.angle_mode;
    float *wts = bwd2_boxes_dyn + (size_t)(wv * PAIRS + lane / G) * pair_stride;   // this pair's weights ...
    [[maybe_unused]] float *gws = wts + LP;                                        // ... and gw

    // ---- prologue: everything besides value rows, requested before the first wait
    const int kp = min((int)threadIdx.x, P - 1);               // thread t of the workgroup: kernel_indices row t
    const float kx = kidx[2 * kp], ky = kidx[2 * kp + 1];
    const float *zrow = logits + (size_t)qh * LP;
    float z[NZ];
#pragma unroll
    for (int k = 0; k < NZ; ++k) {
        z[k] = -INFINITY;
        if (k * G < LP) z[k] = zrow[min(k * G + slot, LP - 1)];   // wave-uniform: no loads past the pair's rounds
    }
    RowT g;
    row_load<ST, VEC, PSB>(grad_out + (size_t)qh * C + slot * LCH, g);
    const float *rrow = ref + (size_t)(gd.ref_per_head ? qh : bq) * (unsigned)gd.ref_dim;
    const float *orow = offsets + (size_t)qh * L * (unsigned)gd.V;
    const float *vrow = has_vr ? vr + (size_t)b * L * 2 : nullptr;
    {   // softmax over the pair's L P logits, as fwd2_boxes_kernel: lane `slot` holds z[slot], z[slot + G], ...
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < NZ; ++k) {
            z[k] = k * G + slot < LP ? z[k] : -INFINITY;
            m = fmaxf(m, z[k]);
        }
        m = group_fmax<G>(m);
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < NZ; ++k) {
            z[k] = k * G + slot < LP ? __expf(z[k] - m) : 0.f;
            sum += z[k];
        }
        const float inv = 1.f / group_sum<G>(sum);
#pragma unroll
        for (int k = 0; k < NZ; ++k)
            if (k * G + slot < LP) wts[k * G + slot] = z[k] * inv;
    }
    if ((int)threadIdx.x < P) kidx_lds[threadIdx.x] = make_float2(kx, ky);
    levels_commit(lv, lv_regs, L);                             // (its barrier publishes kidx_lds and this wave's LDS too)

#pragma unroll 1
    for (int l0 = 0; l0 < L; l0 += G) {                        // (one pass unless there are more levels than lanes)
        // ---- this lane's level of the pass
        const int l = l0 + slot;
        const bool have = l < L;
        const int lc = min(l, L - 1);
        const GridBox box = grid_box_rows(rrow, orow + lc * gd.V, has_vr ? vrow + 2 * lc : nullptr, angle_mode);
        const int Hl = lv.h[lc], Wl = lv.w[lc];
        const unsigned row0 = b * (unsigned)S + (unsigned)lv.start[lc];
        [[maybe_unused]] GridGrad ga{0.f, 0.f, 0.f, 0.f, 0.f};

        // a rolled loop over the points: unrolled, the scheduler pulls the row loads of every step to the front
#pragma unroll 1
        for (int p = 0; p < P; ++p) {
            // ---- step A: lane t of the group -> point p of level l0 + t
            const float2 kk = kidx_lds[p];
            const float kxy[2] = {kk.x, kk.y};
            const float2 xy = grid_point(box, kxy, 0, has_vr, angle_mode);
            const float a = wts[lc * P + p];
            const Sample<float> s = locate<float>(xy.x, xy.y, Hl, Wl);
            const u32x4_t my_off = corner_offsets<ST>(s, row0, H, h, C, have);
            // SCATTER: a w_k of this lane's point; the offset of a corner that gets no add is the marker (a level
            // past L, a corner or the whole point outside the map: corner_offsets; a lane group without a pair)
            [[maybe_unused]] u32x4_t my_aw, my_soff;
            if constexpr (SCATTER) {
                my_aw = as_u32x4(a * (s.hh * s.hw), a * (s.hh * s.lw), a * (s.lh * s.hw), a * (s.lh * s.lw));
                const bool live = active && have && s.inside;
                my_soff = u32x4_t{live && s.ok[0] ? my_off.x : kOobOffset, live && s.ok[1] ? my_off.y : kOobOffset,
                                  live && s.ok[2] ? my_off.z : kOobOffset, live && s.ok[3] ? my_off.w : kOobOffset};
            }
            // ---- step B: corner sums of the pass's levels (pointgrad2_kernel), U of them in flight
            [[maybe_unused]] float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;     // S_k of "my" level (slot)
#pragma unroll
            for (int t0 = 0; t0 < G; t0 += U) {
                if (l0 + t0 >= L) break;                      // wave-uniform
                [[maybe_unused]] RowT v[U][4];
                if constexpr (POINTS) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int t = t0 + u;
                        const u32x4_t off =
                            u32x4_t{group_bcast<G>(my_off.x, t, lane), group_bcast<G>(my_off.y, t, lane),
                                    group_bcast<G>(my_off.z, t, lane), group_bcast<G>(my_off.w, t, lane)};
                        row_load<ST, VEC, PSB>(rs, off.x + lane_off, v[u][0]);
                        row_load<ST, VEC, PSB>(rs, off.y + lane_off, v[u][1]);
                        row_load<ST, VEC, PSB>(rs, off.z + lane_off, v[u][2]);
                        row_load<ST, VEC, PSB>(rs, off.w + lane_off, v[u][3]);
                    }
                    loads_issued();
                }
                if constexpr (SCATTER) {                      // (behind the loads: the adds go out while the rows come)
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int t = t0 + u;
                        const unsigned so[4] = {group_bcast<G>(my_soff.x, t, lane), group_bcast<G>(my_soff.y, t, lane),
                                                group_bcast<G>(my_soff.z, t, lane), group_bcast<G>(my_soff.w, t, lane)};
                        const unsigned aw[4] = {group_bcast<G>(my_aw.x, t, lane), group_bcast<G>(my_aw.y, t, lane),
                                                group_bcast<G>(my_aw.z, t, lane), group_bcast<G>(my_aw.w, t, lane)};
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (so[k] != kOobOffset)
                                row_scatter<ST, VEC, PSB>(grad_value_acc, so[k] + lane_off, __uint_as_float(aw[k]), g);
                    }
                    if constexpr (POINTS) loads_issued();
                }
                if constexpr (POINTS) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float a1 = group_sum<G>(row_dot<ST, VEC>(g, v[u][0]));
                        const float a2 = group_sum<G>(row_dot<ST, VEC>(g, v[u][1]));
                        const float a3 = group_sum<G>(row_dot<ST, VEC>(g, v[u][2]));
                        const float a4 = group_sum<G>(row_dot<ST, VEC>(g, v[u][3]));
                        const bool mine = slot == t0 + u;
                        s1 = mine ? a1 : s1; s2 = mine ? a2 : s2; s3 = mine ? a3 : s3; s4 = mine ? a4 : s4;
                    }
                }
            }
            if constexpr (POINTS) {
                // ---- finish: lane (pair, slot) owns point p of level l0 + slot (pointgrad2_kernel's formulas)
                const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
                const bool keep = have && s.inside;               // a point outside the map: zeros
                float gw = w1 * s1 + w2 * s2 + w3 * s3 + w4 * s4;
                float gx = (float)Wl * a * (s.hh * (s2 - s1) + s.lh * (s4 - s3));
                float gy = (float)Hl * a * (s.hw * (s3 - s1) + s.lw * (s4 - s2));
                gx = keep ? gx : 0.f;
                gy = keep ? gy : 0.f;
                gw = keep ? gw : 0.f;
                if (have) gws[l * P + p] = gw;
                grid_grad_add(ga, box, kxy, 0, make_float2(gx, gy));
            }
        }
        // ---- the level's results from its summed shares
        if constexpr (POINTS) {
            if (active && have) {
                const size_t n = (size_t)qh * L + (unsigned)l;
                grid_grad_store(ga, box, orow + l * gd.V, gd, grad_offsets + n * (unsigned)gd.V,
                                grad_ref_rows ? grad_ref_rows + n * 5 : nullptr);
            }
        }
    }

    if constexpr (POINTS) {
        // ---- epilogue: the softmax Jacobian over the pair's L P points, lane `slot` on slot, slot + G, ...
        wave_lds_sync();                                      // the pair's lanes wrote `gws`
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < NZ; ++k) {
            const int lp = k * G + slot;
            z[k] = 0.f;
            if (lp < LP) {
                z[k] = gws[lp];
                dot += wts[lp] * z[k];
            }
        }
        dot = group_sum<G>(dot);
        if (active) {
            float *gz = grad_logits + (size_t)qh * LP;
#pragma unroll
            for (int k = 0; k < NZ; ++k) {
                const int lp = k * G + slot;
                if (lp < LP) gz[lp] = wts[lp] * (z[k] - dot);
            }
        }
    }
}

}  // namespace boxattn
