// Window-staged kernels for the ENCODER case of box attention: one query per pixel (Lq == S, packed
// levels), bf16 storage, C = 32 channels per head, 2x2 points per level.
//
// The gather kernels (boxattn_gather2.h) pull 4 corner rows per sample point through the vector L1
// -- 64 rows per (query, head) -- and sit at the rate at which the L1 gets rows out of the L2
// (DESIGN.md 4.1).  In the encoder the queries are the pixels and a query's boxes lie around its own
// position on every level, so the rows an 8x8 TILE of queries touches on one level form a small
// window: 16x16 pixels on the tile's own level, 9x9 / 6x6 / 4x4 on the coarser ones -- 389 rows for
// 64 queries x 64 corner rows.  One workgroup = one (tile, head): its four waves fetch the windows of
// all levels once, as whole coalesced rows, straight into LDS (26 KB), and after ONE barrier every lane works
// alone:
//
//   lane = one sample point of one query (wave = 4x4 sub-tile of queries x the 2x2 points), the
//   levels one after the other.  A lane reads the four corner rows of its point from LDS (64 bytes
//   each, 4 x ds_read_b128) and multiplies them with its query's grad_out row, which it keeps in 16
//   registers: 16 v_dot2c_f32_bf16 per corner, no cross-lane step at all (the gather kernels spread
//   a row over 4 lanes because a lane per row is poison for the vector L1; from LDS it is free).
//
// The window of (tile, level) is placed by geometry alone (wave-uniform): the tile's position
// projected onto the level plus a margin for the box size and its predicted offset.  Placement and
// staging are a performance matter only: a point whose footprint is not inside its staged window --
// and every point of a level whose window is not staged (a coarse tile looking at a fine level: too
// large) -- takes the global path, the same dot products on rows fetched by the lane itself.  The
// results are the same either way, for any input.
//
// (Round 3 first built this on the matrix cores -- S = G V^T per 4x4 tile and window row on
// v_mfma_f32_16x16x32_bf16, look-ups from an S tile in LDS: tools/experiments/boxattn_dense_mfma_v1.h.
// Parity-green, 61 us against the gather kernel's 48: with a wave-private 12x12 window per 4x4 tile
// the L2 -> L1 traffic is the gather kernel's, and that traffic is what bounds both.)
#pragma once
#include "boxattn_device.h"
#include "boxattn_binpass.h"      // the backward's fill riders sit in the point-gradient kernel's launch
#include "boxattn_dense_plan.h"

namespace boxattn {

constexpr int kDenseWpe = 5;      // waves per SIMD the register allocation aims at (96 registers; 26 / 30 KB of LDS: 5 workgroups per CU)
typedef unsigned int dense_u32x4 __attribute__((ext_vector_type(4)));

// one 64-byte row (32 bf16 / f16 channels) as 16 words.  (The words go through a plain array: a bit_cast
// of element i of an ext_vector selects element 0 for every i with this compiler)
template <typename PTR> __device__ __forceinline__ void dense_load_row(PTR p, unsigned (&w)[16])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const dense_u32x4 t = reinterpret_cast<const dense_u32x4 *>(p)[i];
        w[4 * i] = t.x; w[4 * i + 1] = t.y; w[4 * i + 2] = t.z; w[4 * i + 3] = t.w;
    }
}
template <typename ST>
__device__ __forceinline__ float dense_dot_row(const unsigned (&g)[16], const unsigned (&v)[16])
{
    // 16-bit x 16-bit products are exact in fp32; two chains: a v_dot2c waits for its own accumulator
    float d0 = 0.f, d1 = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        d0 = Half16<ST>::dot2(g[i], v[i], d0);
        d1 = Half16<ST>::dot2(g[i + 1], v[i + 1], d1);
    }
    return d0 + d1;
}

// Which (tile, head) a workgroup works on.  Workgroup w runs on XCD w % 8 (observed placement; only
// speed depends on it): every XCD gets one contiguous eighth of every level's tiles, all heads of a
// tile (the two 64-byte halves of a value line belong to neighbouring heads) -- its L2 then holds one
// spatial band of the maps -- and walks the levels coarsest first, because the tiles of the coarse
// levels are the slow ones (their fine-level points take the global path).
//
// All of it is scalar work at the top of every wave -- and scalar instructions are not free: the CU's
// one scalar unit serves its four SIMDs, an s_ instruction costs a wave as much issue time as a vector
// one (PMC: all kernels of the step retire ~1 instruction per 4 cycles and SIMD whatever the mix).  The
// decode is therefore integer-only (multiply-high divisions with host magic numbers, 16.16 fixed-point
// window origins: ~100 scalar instructions; with float estimates and v_readfirstlane it was ~450), and
// it reads the plan in two batches: what is addressed statically up front, the query level's entry and
// its L windows -- the only reads at a computed offset -- right after the level is known (read one by
// one behind branches they were a third of a wave's life: 6 600 of 17 700 cycles before the first row
// request left, s_memtime stamps).
struct DenseTileId {
    int lq;                  // query level, -1: no tile
    unsigned b;
    int ty, tx, h;
};
struct DenseMap { int H, W, start; };                   // what the kernel keeps of a level
template <int L> struct DenseHot {
    DenseMap lv[L];
    int H, Lq, S;
};
template <int L>
__device__ __forceinline__ DenseTileId dense_tile_of_block(const DensePlan &pl, unsigned block,
                                                           DenseHot<L> &hot, DenseMap &Q, DenseWin (&wrow)[L])
{
    unsigned n_all[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        hot.lv[l] = DenseMap{pl.lv[l].H, pl.lv[l].W, pl.lv[l].start};
        n_all[l] = pl.lv[l].n_all;
        // (opaque to the compiler from here on: it otherwise sinks these scalar loads to their first use,
        // one round trip per level in the middle of the row requests)
        asm volatile("" : "+s"(hot.lv[l].H), "+s"(hot.lv[l].W), "+s"(hot.lv[l].start));
    }
    hot.H = pl.H; hot.Lq = pl.Lq; hot.S = pl.S;
    asm volatile("" : "+s"(hot.H), "+s"(hot.Lq), "+s"(hot.S));
    DenseTileId t;
    const unsigned x = block & 7u;
    unsigned j, h;
    divmod_magic(block >> 3, (unsigned)hot.H, pl.mag_h, j, h);
    t.h = (int)h;
    int lq = -1;
    unsigned ti = 0, first = 0;
#pragma unroll
    for (int l = L - 1; l >= 0; --l) {
        const unsigned lo = (x * n_all[l]) >> 3, cnt = (((x + 1) * n_all[l]) >> 3) - lo;
        const bool here = j - first < cnt;                 // first <= j < first + cnt
        lq = here ? l : lq;
        ti = here ? lo + (j - first) : ti;
        first += cnt;
    }
    t.lq = lq;
    const int lqc = max(lq, 0);
    const DenseLevel q = pl.lv[lqc];                       // the reads at a computed offset: one batch
#pragma unroll
    for (int l = 0; l < L; ++l) wrow[l] = pl.win[lqc][l];
    Q = DenseMap{q.H, q.W, q.start};
    asm volatile("" : "+s"(Q.H), "+s"(Q.W), "+s"(Q.start));      // (loaded with the batch, not at first use)
    unsigned tr, ty, tx;
    divmod_magic(ti, (unsigned)q.ntiles, q.mag_ntiles, t.b, tr);
    divmod_magic(tr, (unsigned)q.ntx, q.mag_ntx, ty, tx);
    t.ty = (int)ty;
    t.tx = (int)tx;
    return t;
}

// Placement of a tile's windows (wave-uniform) and the cooperative fetch: wave w takes the window rows
// w, w + 4, ... of every level; a row of up to 16 pixels x 64 bytes is ONE direct-to-LDS load (4 lanes per
// pixel; the lanes of pixels past the window's last column are switched off and write nothing).  The data
// never passes through registers: round 3 staged through 64 VGPRs and a second pass of ds_write_b128,
// which held the kernels at 4 waves per SIMD.  The rows have landed after s_waitcnt vmcnt(0) in every
// wave + the workgroup's barrier (dense_stage_wait).
struct DenseWinPos {
    unsigned geo;            // DenseWin::geo
    int x0, y0;
    __device__ __forceinline__ int rows() const { return (int)(geo & 31u); }
    __device__ __forceinline__ int cols() const { return (int)((geo >> 5) & 31u); }
    __device__ __forceinline__ int pitchb() const { return (int)((geo >> 10) & 127u) * 16; }     // bytes per window row
    __device__ __forceinline__ int offb() const { return (int)(geo >> 17) * 16; }               // first byte
};

typedef __attribute__((address_space(3))) void dense_lds_void;

template <int L>
__device__ __forceinline__ void dense_stage_issue(const DenseHot<L> &hot, const DenseWin (&wrow)[L],
                                                  const DenseTileId &t, int lane, int wv,
                                                  __amdgpu_buffer_rsrc_t rs, unsigned char *lds, DenseWinPos (&win)[L])
{
    constexpr int C = 32, RPW = kDenseWinMax / 4;              // rows per wave and level at most
    const int j = lane >> 2, chunk = lane & 3;
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const DenseMap T = hot.lv[l];
        const DenseWin w = wrow[l];
        DenseWinPos &o = win[l];
        o.geo = w.geo;
        const int x0 = (t.tx * w.ax + w.bx) >> 16, y0 = (t.ty * w.ay + w.by) >> 16;
        o.x0 = max(0, min(x0, T.W - o.cols()));
        o.y0 = max(0, min(y0, T.H - o.rows()));
        const int jx = min(o.x0 + j, T.W - 1);
        const unsigned voff =
            ((((t.b * (unsigned)hot.S + (unsigned)(T.start + jx)) * (unsigned)hot.H + (unsigned)t.h) * C) +
             (unsigned)chunk * 8u) * 2u;
        const unsigned row_bytes = (unsigned)T.W * (unsigned)hot.H * (C * 2u);
        // (rows past the bottom of the map -- a window taller than the map -- are never looked up: a
        // corner row that counts lies inside the map; they are simply not fetched)
        const int rows = min(o.rows(), T.H - o.y0);
        unsigned soff = (unsigned)(o.y0 + wv) * row_bytes;
        int dst = o.offb() + wv * o.pitchb();                       // wave-uniform: it becomes M0
        const int step = 4 * o.pitchb();
        if (j < o.cols()) {
#pragma unroll
            for (int k = 0; k < RPW; ++k) {
                if (wv + 4 * k < rows)                                  // wave-uniform
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (dense_lds_void *)(lds + dst), 16, voff, soff, 0, 0);
                soff += 4u * row_bytes;
                dst += step;
            }
        }
    }
}
// every wave's rows have landed, and everybody knows
__device__ __forceinline__ void dense_stage_wait()
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

__device__ __forceinline__ unsigned quad_bcast_u32(unsigned v, int t)      // t is a constant after unrolling
{
    switch (t & 3) {
    case 0: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x00, 0xF, 0xF, true);
    case 1: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x55, 0xF, 0xF, true);
    case 2: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xAA, 0xF, 0xF, true);
    default: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xFF, 0xF, 0xF, true);
    }
}

// A sample point as the kernels need it (locate() of boxattn_device.h without the per-corner flags:
// the flag algebra is done on integers below -- lane masks combined in scalar registers were a third
// of this kernel's instructions, and scalar instructions are not free).
struct DensePoint {
    int y0, x0;              // top-left corner of the footprint, in [-1, H - 1] x [-1, W - 1] (0, 0 if !inside)
    float lh, lw, hh, hw;
    bool inside;             // the reference's window test (the levels of a dense plan are never empty)
};
__device__ __forceinline__ DensePoint dense_locate(float x, float y, int H, int W)
{
    DensePoint s;
    float h_im, w_im;
    {
#pragma clang fp contract(off)                   // two roundings, as in locate()
        h_im = y * (float)H - 0.5f;
        w_im = x * (float)W - 0.5f;
    }
    s.inside = (h_im > -1.f) && (w_im > -1.f) && (h_im < (float)H) && (w_im < (float)W);
    const float hs = s.inside ? h_im : 0.f, ws = s.inside ? w_im : 0.f;   // NaN / outside: finite index arithmetic
    const float hf = floorf(hs), wf = floorf(ws);
    s.y0 = (int)hf;
    s.x0 = (int)wf;
    s.lh = hs - hf;
    s.lw = ws - wf;
    s.hh = 1.f - s.lh;
    s.hw = 1.f - s.lw;
    return s;
}

// The four corner sums S_k = sum_c g_c v_k,c of one sample point: from the staged window if the part of
// its footprint that lies inside the map lies inside the window, else from global memory (`slow`,
// decided per lane, entered per wave).  Corners outside the map give exactly 0.
template <typename ST>
__device__ __forceinline__ void dense_corner_sums(const DensePoint &s, const DenseMap &T, const DenseWinPos &o,
                                                  const unsigned char *lds, const unsigned (&gw)[16],
                                                  const ST *value, unsigned row0, int H, int h, bool vq,
                                                  int lane_p, float (&sk)[4])
{
    constexpr int C = 32;
    const int rows = o.rows(), cols = o.cols();
    const int Hm1 = T.H - 1, Wm1 = T.W - 1;
    // all-ones where the corner counts: inside the map (row y0 unless y0 == -1, row y0 + 1 unless y0 == H - 1,
    // columns alike) and the point inside the window test
    const unsigned mi = s.inside ? 0xffffffffu : 0u;
    const unsigned mr0 = ~(unsigned)(s.y0 >> 31) & mi, mr1 = (unsigned)((s.y0 - Hm1) >> 31) & mi;
    const unsigned mc0 = ~(unsigned)(s.x0 >> 31), mc1 = (unsigned)((s.x0 - Wm1) >> 31);
    const unsigned m[4] = {mr0 & mc0, mr0 & mc1, mr1 & mc0, mr1 & mc1};
    // rows / columns of the map the footprint needs, and how far they are inside the staged window
    // (negative: something is missing; an unstaged level has rows == 0, so d < 0 for every point)
    const int ra = max(s.y0, 0), rb = min(s.y0 + 1, Hm1), ca = max(s.x0, 0), cb = min(s.x0 + 1, Wm1);
    const int d = min(min(ra - o.y0, o.y0 + rows - 1 - rb), min(ca - o.x0, o.x0 + cols - 1 - cb));
    const bool act = vq && s.inside;
    const bool slow = act && d < 0, fast = act && d >= 0;
    if (__builtin_amdgcn_ballot_w64(fast) != 0ull) {               // wave-uniform: somebody reads the window
        // (lanes that do not: clamped slots, results masked or overwritten below)
        const int pitchb = o.pitchb(), offb = o.offb();
        const int rr0 = min(max(s.y0 - o.y0, 0), rows - 1), rr1 = min(max(s.y0 + 1 - o.y0, 0), rows - 1);
        const int cc0 = min(max(s.x0 - o.x0, 0), cols - 1), cc1 = min(max(s.x0 + 1 - o.x0, 0), cols - 1);
        const int rowb0 = offb + __mul24(rr0, pitchb), rowb1 = offb + __mul24(rr1, pitchb);
        const int colb0 = cc0 * kDenseSlotBytes, colb1 = cc1 * kDenseSlotBytes;
        const int slot[4] = {rowb0 + colb0, rowb0 + colb1, rowb1 + colb0, rowb1 + colb1};
        // two corners at a time: 8 LDS reads in flight, then the 32 dot products; the rows of corners
        // that do not count are read from a clamped slot and masked out bitwise -- a select on the
        // finished sum lets the compiler put every corner under its own branch (reads, wait, dots, four
        // times in a row), a multiplication by 0 would let a non-finite value of an unrelated pixel through
        // (2 corner rows a lane has in flight from LDS: 8 reads, 32 registers)
#pragma unroll
        for (int k0 = 0; k0 < 4; k0 += 2) {
            unsigned va[16], vb[16];
            dense_load_row(lds + slot[k0], va);
            dense_load_row(lds + slot[k0 + 1], vb);
            const float da = dense_dot_row<ST>(gw, va), db = dense_dot_row<ST>(gw, vb);
            sk[k0] = __uint_as_float(__float_as_uint(da) & m[k0]);
            sk[k0 + 1] = __uint_as_float(__float_as_uint(db) & m[k0 + 1]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) sk[k] = 0.f;
    }
    if (__builtin_amdgcn_ballot_w64(slow) != 0ull) {               // wave-uniform
        // The global path, one point of every quad at a time (a quad = the 4 points of one query): the
        // quad's lanes fetch the four corner rows of point t together, 16 bytes each -- one 64-byte
        // request per row, as the gather kernels do it; a lane fetching whole rows alone costs the
        // vector L1 four requests per row -- and sum their partial dot products with DPP adds.
        const int p = lane_p;
        unsigned gch[4];                                           // this lane's 8 channels of the grad_out row
#pragma unroll
        for (int i = 0; i < 4; ++i)
            gch[i] = p == 0 ? gw[i] : p == 1 ? gw[4 + i] : p == 2 ? gw[8 + i] : gw[12 + i];
        const int pra = __mul24(ra, T.W), prb = __mul24(rb, T.W);
        const int pix[4] = {pra + ca, pra + cb, prb + ca, prb + cb};          // (clamped into the map: always a valid row)
        unsigned off[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            off[k] = (unsigned)(((row0 + (unsigned)pix[k]) * H + h) * (C * 2));
        // two points of the quad at a time: their 8 row pieces are requested together and unconditionally
        // (the offsets are always inside the map) -- one point at a time, each under its own "anyone
        // slow?" branch, a level was four memory round trips in a row (s_memtime: 9 000 cycles a level)
#pragma unroll
        for (int t0 = 0; t0 < 4; t0 += 2) {
            dense_u32x4 v[2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // lane t's row, my 16-byte piece of it
                    const unsigned oo = quad_bcast_u32(off[k], t0 + u) + (unsigned)p * 16u;
                    v[u][k] = *reinterpret_cast<const dense_u32x4 *>(reinterpret_cast<const char *>(value) + oo);
                }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float part[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned vw[4] = {v[u][k].x, v[u][k].y, v[u][k].z, v[u][k].w};
                    float dd = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        dd = Half16<ST>::dot2(gch[i], vw[i], dd);
                    part[k] = group_sum<4>(dd);
                }
                if (p == t0 + u && slow) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) sk[k] = __uint_as_float(__float_as_uint(part[k]) & m[k]);
                }
            }
        }
    }
}

constexpr int kDenseResFloats = 16 * 16 * 3;       // per wave: the results of 16 queries x 16 points

// (the body: boxattn_dense_pg_body.h, shared by text inclusion with the from-boxes flavour, pointgrad_dense_boxes_kernel
// of boxattn_dense_boxes_bwd.h)
#define BOXATTN_DENSE_FROM_BOXES 0
template <typename ST, int L>
__global__ __launch_bounds__(256, kDenseWpe) void pointgrad_dense_kernel(
    const ST *__restrict__ value, const float *__restrict__ loc, const float *__restrict__ attn,
    const ST *__restrict__ grad_out, float *__restrict__ grad_loc, float *__restrict__ grad_attn,
    DensePlan pl, unsigned value_bytes, BinRide ride)
{
#include "boxattn_dense_pg_body.h"
}
#undef BOXATTN_DENSE_FROM_BOXES

}  // namespace boxattn
