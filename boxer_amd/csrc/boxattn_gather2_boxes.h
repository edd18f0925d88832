// Box attention at inference straight from what the module predicts per (query, head): L boxes (reference window +
// 4 or 5 offsets a level) and L P logits -- the box-attention walk of fwd2_kernel (boxattn_gather2.h: a lane group of
// G = C / VEC lanes per (query, head) pair, pair_of_lane placement with head = XCD, step B with buffer loads, row_axpy
// and U points in flight) without its two per-point inputs.  The (B,Lq,H,L,P,2) sampling grid and the (B,Lq,H,L P)
// weights -- written by grid_fwd_kernel and the softmax kernels to be read here once -- are never made:
//   prologue, one round trip per wave   lane (pair, slot) takes the pair's logits slot, slot + G, ... and the G lanes
//                             reduce the row maximum and the sum of exponentials with DPP (float32, exp(z - max) *
//                             (1 / sum) as softmax_rows_fwd_kernel); the same lane decodes the boxes of the levels
//                             slot, slot + G, ... (grid_box_rows, boxattn_grid.h).  Weights and boxes go to a
//                             wave-private piece of LDS, the kernel_indices rows and the level table to the workgroup's;
//   step A, per tile          lane (pair, slot) owns point lp = t0 + slot, l = lp / P, p = lp - l P: grid_point on the
//                             box of level l and kernel_indices row p, the weight of point lp -- three LDS reads, no
//                             memory round trip between tiles -- then locate / corner_offsets as in fwd2_kernel.
// Same device functions and operation order (grid_box_rows / grid_point keep their fp contract(off)) as grid_fwd_kernel,
// so the locations are its locations bit for bit; the softmax sums in another order than the one-thread-per-row kernel.
// Inference only: no riders, no atomics.
#pragma once
#include "boxattn_gather2.h"
#include "boxattn_grid.h"

namespace boxattn {

constexpr int kBoxesMaxLP = 64;          // L P logits a pair: the limit of the softmax kernels

// 16-byte pieces of wave-private LDS a pair takes: two a level {cx, cy, w, h}{sin, cos, vx, vy}, then its L P weights
inline __host__ __device__ unsigned fwd2_boxes_pair_stride(int L, int LP) { return 2u * L + ((unsigned)LP + 3u) / 4u; }

extern __shared__ u32x4_t fwd2_boxes_dyn[];      // 4 waves x 64 / G pairs x fwd2_boxes_pair_stride

template <typename ST, int G, int U, int VEC>
__global__ __launch_bounds__(256) void fwd2_boxes_kernel(
    const ST *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ lsi,
    const float *__restrict__ ref, const float *__restrict__ offsets, const float *__restrict__ kidx,
    const float *__restrict__ vr, const float *__restrict__ logits, int S, int H, int L, int Lq, int P,
    ST *__restrict__ out, GridDims gd, GatherIdx ix, unsigned value_bytes, unsigned pair_stride)
{
    constexpr int C = VEC * G, PAIRS = kWave / G, NH = 2, NZ = kBoxesMaxLP / G;
    typedef GeoTile<G, NH> Tile;
    typedef Row<ST, VEC> RowT;
    constexpr int PSB = RowGeom<ST, VEC, G>::kPieceStride;    // bytes between a lane's pieces
    constexpr int LCH = RowT::kLaneBytes / (int)sizeof(ST);   // channels of one piece
    __shared__ LevelTable lv;
    __shared__ u32x4_t geo_all[4][Tile::kSize];
    __shared__ float2 kidx_lds[kBoxesMaxLP];
    const LevelRegs lv_regs = levels_request(shapes, lsi, L);   // published below, behind the first loads

    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    u32x4_t *geo = geo_all[wv] + Tile::base(lane);   // this group's part of the tile
    bool active;
    const unsigned qh = pair_of_lane<PAIRS>(ix, blockIdx.x, H, lane / G, wv, active);
    const int slot = lane % G;                      // step A: point slot; step B: channel chunk
    unsigned bq, hu, b, qu;
    divmod_magic(qh, (unsigned)H, ix.magic_h, bq, hu);
    divmod_magic(bq, (unsigned)Lq, ix.magic_lq, b, qu);
    const int h = (int)hu;
    const int LP = L * P;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<ST *>(value), 0, value_bytes, 0x00020000);
    const unsigned lane_off = (unsigned)(slot * RowT::kLaneBytes);
    const float rcp_p = ix.rcp_p;                   // (n + 0.5) * rcp_p truncates to n / P (fwd2_kernel)
    const bool has_vr = vr != nullptr;
    const int angle_mode = gd.angle_mode;
    u32x4_t *mine = fwd2_boxes_dyn + (size_t)(wv * PAIRS + lane / G) * pair_stride;   // this pair's boxes and weights
    float *wts = reinterpret_cast<float *>(mine + 2 * L);

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
    {
        const float *r = ref + (size_t)(gd.ref_per_head ? qh : bq) * (unsigned)gd.ref_dim;
        const float *o = offsets + (size_t)qh * L * (unsigned)gd.V;
        const float *v = has_vr ? vr + (size_t)b * L * 2 : nullptr;
        for (int l = slot; l < L; l += G) {                    // (one pass unless there are more levels than lanes)
            const GridBox g = grid_box_rows(r, o + l * gd.V, has_vr ? v + 2 * l : nullptr, angle_mode);
            mine[2 * l] = as_u32x4(g.cx, g.cy, g.w, g.h);
            mine[2 * l + 1] = as_u32x4(g.sn, g.cs, g.vx, g.vy);
        }
    }
    {   // softmax over the pair's L P logits: lane `slot` holds z[slot], z[slot + G], ...
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

    f32x2 acc[VEC / 2];
#pragma unroll
    for (int i = 0; i < VEC / 2; ++i) acc[i] = f32x2{0.f, 0.f};

    // a rolled loop over the tiles: unrolled, the scheduler pulls the row loads of every tile to the front (fwd2_kernel)
#pragma unroll 1
    for (int t0 = 0; t0 < LP; t0 += G) {
        u32x4_t my_off = {0u, 0u, 0u, 0u}, my_wt = {0u, 0u, 0u, 0u};
        {   // ---- step A
            const int lp = t0 + slot;
            const bool have = lp < LP;
            const int lq = have ? lp : LP - 1;
            const int l = (int)(((float)lq + 0.5f) * rcp_p);   // lq / P (exact, see rcp_p)
            const int p = lq - l * P;
            const u32x4_t b0 = mine[2 * l], b1 = mine[2 * l + 1];
            GridBox g;
            g.cx = __uint_as_float(b0.x); g.cy = __uint_as_float(b0.y);
            g.w = __uint_as_float(b0.z); g.h = __uint_as_float(b0.w);
            g.sn = __uint_as_float(b1.x); g.cs = __uint_as_float(b1.y);
            g.vx = __uint_as_float(b1.z); g.vy = __uint_as_float(b1.w);
            g.rw = g.rh = 0.f;
            const float2 kk = kidx_lds[p];
            const float kxy[2] = {kk.x, kk.y};
            const float2 xy = grid_point(g, kxy, 0, has_vr, angle_mode);
            const float a = have ? wts[lq] : 0.f;
            const Sample<float> s = locate<float>(xy.x, xy.y, lv.h[l], lv.w[l]);
            const u32x4_t off =
                corner_offsets<ST>(s, b * (unsigned)S + (unsigned)lv.start[l], H, h, C, have);
            const u32x4_t wt = as_u32x4(s.hh * s.hw * a, s.hh * s.lw * a, s.lh * s.hw * a,
                                        s.lh * s.lw * a);
            if constexpr (G == 4) {
                my_off = off;
                my_wt = wt;
            } else {
                wave_lds_sync();               // previous tile fully consumed
                geo[slot * NH] = off;
                geo[slot * NH + 1] = wt;
                wave_lds_sync();
            }
        }
        // ---- step B (U points' loads in flight at a time)
#pragma unroll
        for (int tb = 0; tb < G; tb += U) {
            u32x4_t off[U], wt[U];
            RowT v[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if constexpr (G == 4) {
                    off[u] = quad_bcast(my_off, tb + u);
                    wt[u] = quad_bcast(my_wt, tb + u);
                } else {
                    off[u] = geo[(tb + u) * NH];
                    wt[u] = geo[(tb + u) * NH + 1];
                }
                row_load<ST, VEC, PSB>(rs, off[u].x + lane_off, v[u][0]);
                row_load<ST, VEC, PSB>(rs, off[u].y + lane_off, v[u][1]);
                row_load<ST, VEC, PSB>(rs, off[u].z + lane_off, v[u][2]);
                row_load<ST, VEC, PSB>(rs, off[u].w + lane_off, v[u][3]);
            }
            loads_issued();
#pragma unroll
            for (int u = 0; u < U; ++u) {
                row_axpy<ST, VEC>(acc, __uint_as_float(wt[u].x), v[u][0]);
                row_axpy<ST, VEC>(acc, __uint_as_float(wt[u].y), v[u][1]);
                row_axpy<ST, VEC>(acc, __uint_as_float(wt[u].z), v[u][2]);
                row_axpy<ST, VEC>(acc, __uint_as_float(wt[u].w), v[u][3]);
            }
        }
    }
    if (active) row_store<ST, VEC, PSB>(out + (size_t)qh * C + slot * LCH, acc);
}

}  // namespace boxattn
