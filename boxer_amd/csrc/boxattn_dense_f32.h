// Window-staged kernels for the encoder case of FLOAT32 box attention -- the reference's own arithmetic
// (box_attention_func.py:11: the CUDA op computes in float32 whatever autocast says).
//
// Rounds 1-4 ran float32 on the row-gather kernels (boxattn_gather2.h: forward 64 us, point gradients 82 us at C2)
// and kept the window-staged formulation of boxattn_dense.h for bf16 storage only: the staged bf16 FORWARD is a
// matrix-core kernel (transposing 16-bit LDS reads, v_mfma_f32_4x4x4_16B_bf16) that has no float32 counterpart
// worth having.  The staged POINT-GRADIENT kernel, however, is plain VALU work on rows read from
// LDS -- lane = one sample point, four corner rows, dot products with the query's upstream row -- and so is a
// forward written the same way (lane = one sample point, four corner rows, weighted sum into 32 accumulators,
// the quad's four points summed at the end).  Both carry over to float32 with 128-byte pixels: a tile's windows are
// 2 x 25.4 KB at BoxeR-R50 shapes, three workgroups per CU instead of five, and the kernels trade the gather
// kernels' 64 L1 row requests per (query, head) for LDS reads.
//
// Same tiles, same window placement (geometry only, results never depend on it), same riders, same global path for
// points whose footprint is not inside a staged window as the bf16 kernels (boxattn_dense.h); the plan's window
// geometry is in units of a quarter pixel (32 bytes here, 16 there).  float32 throughout: products and sums in the
// order of the reference's kernel up to the association of the per-point sums (within 1e-4 of the float64 goldens,
// as the gather kernels).
#pragma once
#include "boxattn_dense.h"
#include "boxattn_dense_boxes.h"

namespace boxattn {

constexpr int kDenseF32Slot = 128;                 // one staged pixel: 32 float32 channels
constexpr int kDenseF32Unit = 32;                  // bytes per unit of DenseWin::geo's pitch / offset fields
// (kDenseF32LdsBytes is defined in boxattn_dense_plan.h, next to the host's window budget that must agree with it)
constexpr int kDenseF32Skew = 32;                  // bytes between the end of a window row and the start of the next
constexpr int kDenseF32ZeroOff = kDenseF32LdsBytes - kDenseF32Slot;    // the forward's row of zeros (make_dense_plan leaves it free)

struct DenseWinPosF32 {
    unsigned geo;
    int x0, y0;
    __device__ __forceinline__ int rows() const { return (int)(geo & 31u); }
    __device__ __forceinline__ int cols() const { return (int)((geo >> 5) & 31u); }
    // Bytes between window rows: the row's pixels + a skew of 32 bytes (one unit of the host's pitch field).  A lane reads
    // a corner row as eight 16-byte pieces, every lane of an instruction piece i of ITS row, and rows and pixels start at
    // multiples of 32 bytes: only 8 of the 16 bank groups ever hold a piece i (half of the kernels' LDS-busy time is bank
    // conflicts, profiles/r05_pmc_sq_fp32.txt).  A skew of 16 bytes -- consecutive rows then step through all 16 groups --
    // was measured in round 6 (with a build switch, since removed; same box, C2 / C2' float32): 210.0 / 342.9 us a step against
    // 210.7 / 342.5: nothing (profiles/r06_f32_skew.log) -- the lanes of a wave read few distinct ROWS (a 4 x 4 query
    // sub-tile), what collides are pixels of one row, 128 bytes apart, and a direct-to-LDS load cannot pad between the
    // pixels it writes (lane-linear destination).
    __device__ __forceinline__ int pitchb() const { return cols() * kDenseF32Slot + kDenseF32Skew; }
    __device__ __forceinline__ int offb() const { return (int)(geo >> 17) * kDenseF32Unit; }
};

// Placement + cooperative fetch (dense_stage_issue for 128-byte pixels): a wave-load of 64 x 16 bytes is 8 pixels, a
// window row of up to 16 pixels two of them; wave w takes the rows w, w + 4, ...
template <int L>
__device__ __forceinline__ void dense_f32_stage_issue(const DenseHot<L> &hot, const DenseWin (&wrow)[L], const DenseTileId &t,
                                                      int lane, int wv, __amdgpu_buffer_rsrc_t rs, unsigned char *lds,
                                                      DenseWinPosF32 (&win)[L])
{
    constexpr int C = 32, RPW = kDenseWinMax / 4;
    const int j = lane >> 3, chunk = lane & 7;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const DenseMap T = hot.lv[l];
        const DenseWin w = wrow[l];
        DenseWinPosF32 &o = win[l];
        o.geo = w.geo;
        const int x0 = (t.tx * w.ax + w.bx) >> 16, y0 = (t.ty * w.ay + w.by) >> 16;
        o.x0 = max(0, min(x0, T.W - o.cols()));
        o.y0 = max(0, min(y0, T.H - o.rows()));
        const unsigned row_bytes = (unsigned)T.W * (unsigned)hot.H * (C * 4u);
        const int rows = min(o.rows(), T.H - o.y0);
#pragma unroll
        for (int half = 0; half < 2; ++half) {                     // pixels 0-7 / 8-15 of the window row
            const int jj = j + 8 * half;
            const int jx = min(o.x0 + jj, T.W - 1);
            const unsigned voff =
                ((((t.b * (unsigned)hot.S + (unsigned)(T.start + jx)) * (unsigned)hot.H + (unsigned)t.h) * C) +
                 (unsigned)chunk * 4u) * 4u;
            unsigned soff = (unsigned)(o.y0 + wv) * row_bytes;
            int dst = o.offb() + wv * o.pitchb() + half * 1024;
            const int step = 4 * o.pitchb();
            if (8 * half < o.cols() && jj < o.cols()) {            // (first condition wave-uniform)
#pragma unroll
                for (int k = 0; k < RPW; ++k) {
                    if (wv + 4 * k < rows)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (dense_lds_void *)(lds + dst), 16, voff, soff, 0, 0);
                    soff += 4u * row_bytes;
                    dst += step;
                }
            }
        }
    }
}

// one 128-byte row (32 float32 channels)
template <typename PTR> __device__ __forceinline__ void dense_f32_load_row(PTR p, float (&w)[32])
{
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float4 t = reinterpret_cast<const float4 *>(p)[i];
        w[4 * i] = t.x; w[4 * i + 1] = t.y; w[4 * i + 2] = t.z; w[4 * i + 3] = t.w;
    }
}
__device__ __forceinline__ float dense_f32_dot_row(const float (&g)[32], const float (&v)[32])
{
    float d0 = 0.f, d1 = 0.f;                      // two chains
#pragma unroll
    for (int i = 0; i < 32; i += 2) {
        d0 = fmaf(g[i], v[i], d0);
        d1 = fmaf(g[i + 1], v[i + 1], d1);
    }
    return d0 + d1;
}

// which corners of a located point count, and how far its footprint is inside the staged window (d < 0: not)
struct DenseFoot {
    unsigned m[4];           // all-ones where the corner lies inside the map (and the point inside the window test)
    int ra, rb, ca, cb;      // rows / columns of the map the footprint needs (clamped into the map)
    int d;
};
__device__ __forceinline__ DenseFoot dense_f32_foot(const DensePoint &s, const DenseMap &T, const DenseWinPosF32 &o)
{
    DenseFoot f;
    const int Hm1 = T.H - 1, Wm1 = T.W - 1;
    const unsigned mi = s.inside ? 0xffffffffu : 0u;
    const unsigned mr0 = ~(unsigned)(s.y0 >> 31) & mi, mr1 = (unsigned)((s.y0 - Hm1) >> 31) & mi;
    const unsigned mc0 = ~(unsigned)(s.x0 >> 31), mc1 = (unsigned)((s.x0 - Wm1) >> 31);
    f.m[0] = mr0 & mc0; f.m[1] = mr0 & mc1; f.m[2] = mr1 & mc0; f.m[3] = mr1 & mc1;
    f.ra = max(s.y0, 0); f.rb = min(s.y0 + 1, Hm1); f.ca = max(s.x0, 0); f.cb = min(s.x0 + 1, Wm1);
    const int rows = o.rows(), cols = o.cols();
    f.d = min(min(f.ra - o.y0, o.y0 + rows - 1 - f.rb), min(f.ca - o.x0, o.x0 + cols - 1 - f.cb));
    return f;
}
// LDS byte offsets of the four corner rows of a footprint that lies inside the window (clamped for lanes whose does not)
__device__ __forceinline__ void dense_f32_slots(const DensePoint &s, const DenseWinPosF32 &o, int (&slot)[4])
{
    const int rows = o.rows(), cols = o.cols(), pitchb = o.pitchb(), offb = o.offb();
    const int rr0 = min(max(s.y0 - o.y0, 0), rows - 1), rr1 = min(max(s.y0 + 1 - o.y0, 0), rows - 1);
    const int cc0 = min(max(s.x0 - o.x0, 0), cols - 1), cc1 = min(max(s.x0 + 1 - o.x0, 0), cols - 1);
    const int rowb0 = offb + __mul24(rr0, pitchb), rowb1 = offb + __mul24(rr1, pitchb);
    const int colb0 = cc0 * kDenseF32Slot, colb1 = cc1 * kDenseF32Slot;
    slot[0] = rowb0 + colb0; slot[1] = rowb0 + colb1; slot[2] = rowb1 + colb0; slot[3] = rowb1 + colb1;
}

// ---------------------------------------------------------------------------------------------------------
// point gradients
// ---------------------------------------------------------------------------------------------------------
// (the body: boxattn_dense_f32_pg_body.h, shared by text inclusion with the from-boxes flavour,
// pointgrad_dense_f32_boxes_kernel of boxattn_dense_boxes_bwd.h)
#define BOXATTN_DENSE_FROM_BOXES 0
template <int L>
__global__ __launch_bounds__(256, 3) void pointgrad_dense_f32_kernel(
    const float *__restrict__ value, const float *__restrict__ loc, const float *__restrict__ attn,
    const float *__restrict__ grad_out, float *__restrict__ grad_loc, float *__restrict__ grad_attn,
    DensePlan pl, unsigned value_bytes, BinRide ride)
{
#include "boxattn_dense_f32_pg_body.h"
}
#undef BOXATTN_DENSE_FROM_BOXES

// ---------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------
// (the body: boxattn_dense_f32_fwd_body.h, shared by text inclusion with the from-boxes flavour below)
#define BOXATTN_DENSE_FROM_BOXES 0
template <int L>
__global__ __launch_bounds__(256, 3) void fwd_dense_f32_kernel(
    const float *__restrict__ value, const float *__restrict__ loc, const float *__restrict__ attn,
    float *__restrict__ out, DensePlan pl, unsigned value_bytes, BinRide ride,
    unsigned long long *__restrict__ stats)
{
#include "boxattn_dense_f32_fwd_body.h"
}
#undef BOXATTN_DENSE_FROM_BOXES

// ... at inference from boxes and logits (fwd_dense_boxes_kernel's operands; dense_boxes_points, boxattn_dense_boxes.h)
#define BOXATTN_DENSE_FROM_BOXES 1
template <int L>
__global__ __launch_bounds__(256, 3) void fwd_dense_f32_boxes_kernel(
    const float *__restrict__ value, const float *__restrict__ ref, const float *__restrict__ offsets,
    const float *__restrict__ kidx, const float *__restrict__ vr, const float *__restrict__ logits,
    float *__restrict__ out, DensePlan pl, unsigned value_bytes, GridDims gd)
{
#include "boxattn_dense_f32_fwd_body.h"
}
#undef BOXATTN_DENSE_FROM_BOXES

}  // namespace boxattn
