// The elementwise kernels around the operator (one translation unit: boxattn_extras.hip): reference windows +
// box offsets -> sampling grid and back (first step), softmax over the L*P logits of a
// (query, head) each way, instance attention's spatial / level weights from its 2x2 logits each way, value
// mask-fill + bf16 cast (N3).  The device helpers they share with the sampling kernels (grid_box, grid_point,
// grid_grad_*) live in boxattn_grid.h.
#pragma once
#include "boxattn_cells.h"
#include "boxattn_grid.h"

namespace boxattn {

__global__ __launch_bounds__(256) void grid_fwd_kernel(const float *__restrict__ ref,
                                                       const float *__restrict__ offsets,
                                                       const float *__restrict__ kidx,
                                                       const float *__restrict__ vr, GridDims d,
                                                       size_t n_pts, float *__restrict__ grid)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // (row n, point p)
    if (i >= n_pts) return;
    const size_t n = i / (unsigned)d.P;
    const int p = (int)(i - n * (unsigned)d.P);
    const GridBox g = grid_box(ref, offsets, vr, d, n);
    reinterpret_cast<float2 *>(grid)[i] = grid_point(g, kidx, p, vr != nullptr, d.angle_mode);
}

// grad_offsets (N, V) and, if asked for, the per-row gradient of the reference window
// grad_ref_rows (N, 5) = d/d(cx, cy, w, h, angle)_ref (summed over levels / heads by the
// caller): four lanes per row (a DPP quad), points strided over them, quad sum at the end.
__global__ __launch_bounds__(256) void grid_bwd_kernel(const float *__restrict__ ref,
                                                       const float *__restrict__ offsets,
                                                       const float *__restrict__ kidx,
                                                       const float *__restrict__ vr,
                                                       const float *__restrict__ grad_grid,
                                                       GridDims d, size_t n_rows,
                                                       float *__restrict__ grad_offsets,
                                                       float *__restrict__ grad_ref_rows)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t n = t / 4;
    const int j = (int)(t % 4);
    const bool live = n < n_rows;
    if (!live) n = n_rows - 1;                                  // keep the quad together
    const GridBox g = grid_box(ref, offsets, vr, d, n);
    const float2 *gg = reinterpret_cast<const float2 *>(grad_grid) + n * (unsigned)d.P;
    GridGrad a{0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p = j; p < d.P; p += 4) grid_grad_add(a, g, kidx, p, gg[p]);
    a.cx = group_sum<4>(a.cx); a.cy = group_sum<4>(a.cy);
    a.w = group_sum<4>(a.w); a.h = group_sum<4>(a.h); a.t = group_sum<4>(a.t);
    if (!(live && j == 0)) return;
    grid_grad_store(a, g, offsets + n * (unsigned)d.V, d, grad_offsets + n * (unsigned)d.V,
                    grad_ref_rows ? grad_ref_rows + n * 5 : nullptr);
}


// ---------------------------------------------------------------------------------------
// Pointwise work around the operator (reference e2edet/module/box_attention.py:222-231),
// SURVEY.md 8(f) N3:
//   * attention weights = softmax over the L*P logits of a (query, head), computed in float32
//     whatever the logits' type (float32, or the bfloat16 / float16 of an autocast projection) -- one pass
//     instead of cast + softmax (+ cast); its backward grad_logits = a (g - sum_j a_j g_j),
//     written in the logits' type;
//   * value rows of padded pixels (v_mask) zeroed and cast to bfloat16 / float16 in the same pass
//     (`value.masked_fill(v_mask[..., None], 0)` followed by the op's 16-bit conversion).
// Rows whose length is 4 * 2^k (k <= 4; BoxeR: 16 = 4 levels x 2x2 points): 2^k lanes per row,
// four consecutive values per lane, so a wave reads and writes whole contiguous runs
// (element index = 4 * thread) and the row max / sum are cross-lane butterflies.  Any other
// length <= 64: one thread per row (strided accesses; the rare shapes).
// ---------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void pw_st(T *p, float v);
template <> __device__ __forceinline__ void pw_st<float>(float *p, float v) { *p = v; }
template <> __device__ __forceinline__ void pw_st<bf16_t>(bf16_t *p, float v) { *p = f32_to_bf16(v); }
template <> __device__ __forceinline__ void pw_st<f16_t>(f16_t *p, float v) { *p = (f16_t)v; }

template <typename T, int NMAX>      // n <= NMAX: the row stays in registers
__global__ __launch_bounds__(256) void softmax_rows_fwd_kernel(const T *__restrict__ logits,
                                                               size_t rows, int n,
                                                               float *__restrict__ attn)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const T *src = logits + r * (size_t)n;
    float *dst = attn + r * (size_t)n;
    float v[NMAX];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NMAX; ++i) {
        v[i] = i < n ? pw_ld<T>(src + i) : -INFINITY;
        m = fmaxf(m, v[i]);
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NMAX; ++i) {
        v[i] = i < n ? __expf(v[i] - m) : 0.f;
        sum += v[i];
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) dst[i] = v[i] * inv;
}

template <typename T, int NMAX>
__global__ __launch_bounds__(256) void softmax_rows_bwd_kernel(const float *__restrict__ attn,
                                                               const float *__restrict__ grad_attn,
                                                               size_t rows, int n,
                                                               T *__restrict__ grad_logits)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float *a = attn + r * (size_t)n, *g = grad_attn + r * (size_t)n;
    T *dst = grad_logits + r * (size_t)n;
    float av[NMAX], gv[NMAX];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < NMAX; ++i) {
        av[i] = i < n ? a[i] : 0.f;
        gv[i] = i < n ? g[i] : 0.f;
        dot += av[i] * gv[i];
    }
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) pw_st<T>(dst + i, av[i] * (gv[i] - dot));
}

template <int G> __device__ __forceinline__ float group_max(float v)
{
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
template <int G> __device__ __forceinline__ float group_add(float v)
{
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename T, int G>         // n = 4 G values per row, G lanes per row
__global__ __launch_bounds__(256) void softmax_vec_fwd_kernel(const T *__restrict__ logits,
                                                              size_t total, float *__restrict__ attn)
{
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const bool live = i < total;             // rows are whole multiples of the group: uniform per row
    float v[4];
    VecIO<T, 4>::ld(logits + (live ? i : 0), v);
    const float m = group_max<G>(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = __expf(v[k] - m);
    const float inv = 1.f / group_add<G>((v[0] + v[1]) + (v[2] + v[3]));
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] *= inv;
    if (live) VecIO<float, 4>::st(attn + i, v);
}

template <typename T, int G>
__global__ __launch_bounds__(256) void softmax_vec_bwd_kernel(const float *__restrict__ attn,
                                                              const float *__restrict__ grad_attn,
                                                              size_t total, T *__restrict__ grad_logits)
{
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const bool live = i < total;
    float a[4], g[4];
    VecIO<float, 4>::ld(attn + (live ? i : 0), a);
    VecIO<float, 4>::ld(grad_attn + (live ? i : 0), g);
    const float dot = group_add<G>((a[0] * g[0] + a[1] * g[1]) + (a[2] * g[2] + a[3] * g[3]));
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] *= g[k] - dot;
    if (live) VecIO<T, 4>::st(grad_logits + i, a);
}

// ---------------------------------------------------------------------------------------
// Instance attention: both weight tensors from the 2x2 logits of every level, and the gradients back
// (modules.py InstanceAttention; reference box_attention.py:100-121 expands the logits with two
// repeat_interleave and runs two softmaxes over the expanded tensor).  Per row r = (b, q, h): logits
// z[l][i][j] (l < L; i, j in {0, 1}), m = k / 2, point (l, y, x) lies in cell c = (l, y >= m, x >= m):
//   a = softmax of z over the 4 L cells of the row,   t[l][i][j] = softmax of z[.][i][j] over l
//   spatial_w[l][y][x] = a[c] / m^2      (every exponential appears m^2 times in the expanded denominator)
//   level_w[l][y][x]   = t[c]
//   grad_z[c] = a[c] / m^2 (Gs[c] - sum_c' a[c'] Gs[c']) + t[c] (Gt[c] - sum_l' t[l'][i][j] Gt[l'][i][j])
// with Gs / Gt the sums of the upstream gradients over the m^2 points of a cell.  The backward reads the logits
// and the upstream gradients only: a and t are recomputed.
// Lane layout of both kernels: a row takes G = 4 * (L rounded up to a power of two) adjacent lanes, lane c of the
// group holds cell c (l = c / 4, i = c / 2 % 2, j = c % 2), a wave holds 64 / G consecutive rows.  The softmax over
// the row is a butterfly over the group, the one over the levels a butterfly over the lanes 4 apart: fixed order,
// no atomics, so both kernels are bitwise reproducible.
// The (rows, L, k, k) tensors are accessed as float4 (k even: k^2 is a multiple of 4, a float4 never crosses a
// level) and must be 16-byte aligned -- the entry points reject other pointers; the logits and their gradient are
// accessed element by element (consecutive lanes, consecutive elements) and need no alignment.
// ---------------------------------------------------------------------------------------
struct InstDims {
    int L, k;
    unsigned n4_level, n4_row;             // float4s per level (k^2 / 4) and per row
    float rcp_k, rcp_n4_level, rcp_n4_row;
    float inv_m2;                          // 1 / m^2
};

__device__ __forceinline__ float inst_pick(bool hi_y, bool hi_x, float c0, float c1, float c2, float c3)
{
    return hi_y ? (hi_x ? c3 : c2) : (hi_x ? c1 : c0);
}

// Store-bound: the 64 / G rows of a wave are one contiguous run of float4s in each output, written 64 float4s
// (1 KB) at a time; a float4's four cell values come from the lanes of its (row, level) by ds_bpermute and each
// element picks its cell with two compares.
template <typename T, int G>
__global__ __launch_bounds__(256) void inst_weights_fwd_kernel(const T *__restrict__ logits, size_t rows,
                                                               InstDims d, float *__restrict__ spatial_w,
                                                               float *__restrict__ level_w)
{
    constexpr int R = 64 / G;
    const int lane = threadIdx.x & 63;
    const size_t row0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
    if (row0 >= rows) return;                                  // (wave-uniform)
    const size_t my_row = row0 + lane / G;
    float a, t;
    inst_cell_softmax<T, G>(logits, my_row < rows ? my_row : rows - 1, lane % G, d.L, a, t);
    a *= d.inv_m2;

    const unsigned live_rows = rows - row0 < (size_t)R ? (unsigned)(rows - row0) : (unsigned)R;
    const unsigned n4 = live_rows * d.n4_row;
    const int m = d.k / 2;
    float4 *sw = reinterpret_cast<float4 *>(spatial_w) + row0 * d.n4_row;
    float4 *lw = level_w ? reinterpret_cast<float4 *>(level_w) + row0 * d.n4_row : nullptr;
    for (unsigned base = 0; base < n4; base += 64) {          // uniform trip count: every lane takes part in the permutes
        const bool live = base + lane < n4;
        const unsigned q = live ? base + lane : 0;
        const unsigned rw = small_div(q, d.rcp_n4_row), q_row = q - rw * d.n4_row;
        const unsigned l = small_div(q_row, d.rcp_n4_level), e0 = 4 * (q_row - l * d.n4_level);
        const int y0 = (int)small_div(e0, d.rcp_k), x0 = (int)e0 - y0 * d.k;
        bool hi_y[4], hi_x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                          // x0 + 3 < 2 k: at most one wrap
            const bool wrap = x0 + j >= d.k;
            hi_x[j] = (wrap ? x0 + j - d.k : x0 + j) >= m;
            hi_y[j] = y0 + (wrap ? 1 : 0) >= m;
        }
        const int src = (int)(rw * G + l * 4);
        {
            const float c0 = __shfl(a, src, 64), c1 = __shfl(a, src + 1, 64), c2 = __shfl(a, src + 2, 64),
                        c3 = __shfl(a, src + 3, 64);
            if (live)
                sw[q] = make_float4(inst_pick(hi_y[0], hi_x[0], c0, c1, c2, c3), inst_pick(hi_y[1], hi_x[1], c0, c1, c2, c3),
                                    inst_pick(hi_y[2], hi_x[2], c0, c1, c2, c3), inst_pick(hi_y[3], hi_x[3], c0, c1, c2, c3));
        }
        if (lw) {                                              // (uniform)
            const float c0 = __shfl(t, src, 64), c1 = __shfl(t, src + 1, 64), c2 = __shfl(t, src + 2, 64),
                        c3 = __shfl(t, src + 3, 64);
            if (live)
                lw[q] = make_float4(inst_pick(hi_y[0], hi_x[0], c0, c1, c2, c3), inst_pick(hi_y[1], hi_x[1], c0, c1, c2, c3),
                                    inst_pick(hi_y[2], hi_x[2], c0, c1, c2, c3), inst_pick(hi_y[3], hi_x[3], c0, c1, c2, c3));
        }
    }
}

// Load-bound: the four lanes of a (row, level) walk that level's k^2 / 4 float4s of each upstream gradient (a
// quad reads 64 consecutive bytes), every lane keeps four per-cell sums per gradient, chosen by predicate; quad
// sums, then lane c holds Gs[c] and Gt[c] next to its a[c] and t[c].  Either gradient may be NULL (= zeros).
template <typename T, int G>
__global__ __launch_bounds__(256) void inst_weights_bwd_kernel(const T *__restrict__ logits,
                                                               const float *__restrict__ grad_spatial,
                                                               const float *__restrict__ grad_level,
                                                               size_t rows, InstDims d,
                                                               T *__restrict__ grad_logits)
{
    constexpr int R = 64 / G;
    const int lane = threadIdx.x & 63;
    const size_t row0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
    if (row0 >= rows) return;                                  // (wave-uniform)
    const size_t my_row = row0 + lane / G;
    const int c = lane % G, l = c / 4, sub = c % 4;
    const bool live = my_row < rows && l < d.L;
    const size_t row = my_row < rows ? my_row : rows - 1;
    float a, t;
    inst_cell_softmax<T, G>(logits, row, c, d.L, a, t);

    const int m = d.k / 2;
    InstCellSums gs{0.f, 0.f, 0.f, 0.f}, gt{0.f, 0.f, 0.f, 0.f};
    if (live) {
        const size_t at = (row * (unsigned)d.L + (unsigned)l) * d.n4_level;
        const float4 *ps = grad_spatial ? reinterpret_cast<const float4 *>(grad_spatial) + at : nullptr;
        const float4 *pt = grad_level ? reinterpret_cast<const float4 *>(grad_level) + at : nullptr;
#pragma unroll 4
        for (unsigned q = sub; q < d.n4_level; q += 4) {
            const float4 s = ps ? ps[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 u = pt ? pt[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            const int y0 = (int)small_div(4 * q, d.rcp_k), x0 = (int)(4 * q) - y0 * d.k;
            const float sv[4] = {s.x, s.y, s.z, s.w}, uv[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool wrap = x0 + j >= d.k;
                const bool hi_x = (wrap ? x0 + j - d.k : x0 + j) >= m, hi_y = y0 + (wrap ? 1 : 0) >= m;
                inst_cell_add(gs, hi_y, hi_x, sv[j]);
                inst_cell_add(gt, hi_y, hi_x, uv[j]);
            }
        }
    }
    const float Gs = inst_cell_total(gs, sub), Gt = inst_cell_total(gt, sub);
    const float dot_s = lanes_add<1, G>(a * Gs), dot_t = lanes_add<4, G>(t * Gt);
    if (live) pw_st<T>(grad_logits + row * (size_t)(4 * d.L) + c, a * d.inv_m2 * (Gs - dot_s) + t * (Gt - dot_t));
}

// value (rows, d) of type T -> 16-bit OT (bfloat16 or float16), rows with mask != 0 zeroed; 8 channels
// per thread
template <typename T, typename OT>
__global__ __launch_bounds__(256) void value_mask_cast_kernel(const T *__restrict__ value,
                                                              const unsigned char *__restrict__ mask,
                                                              size_t rows, int d,
                                                              OT *__restrict__ out)
{
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= rows * (size_t)d) return;
    const size_t r = i / (unsigned)d;
    const bool dead = mask && mask[r];
    float v[8];
    if constexpr (IsHalf16<T>::value) {
        VecIO<T, 8>::ld(value + i, v);
    } else {
        float lo[4], hi[4];
        VecIO<float, 4>::ld(value + i, lo);
        VecIO<float, 4>::ld(value + i + 4, hi);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = lo[k]; v[4 + k] = hi[k]; }
    }
    if (dead) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = 0.f;
    }
    VecIO<OT, 8>::st(out + i, v);
}

}  // namespace boxattn
