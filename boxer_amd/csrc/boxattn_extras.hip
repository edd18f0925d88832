// C ABI, part two (declared in include/boxattn.h): the opt-in extras around the operator that are
// plain elementwise kernels -- reference windows + box offsets -> sampling grid (first step;
// the modules' `_where_to_attend`, e2edet/module/box_attention.py:63-81, 196-214, 304-338) and the softmax /
// mask-fill + cast passes (N3; box_attention.py:222-231), instance attention's weights from its 2x2 logits
// (box_attention.py:100-121).  The operator itself is boxattn_capi.hip.
#include "../../include/boxattn.h"

#include <hip/hip_runtime.h>

#include "boxattn_pointwise.h"

using namespace boxattn;

namespace {
inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
inline int finish() { return (int)hipGetLastError(); }
// the C ABI passes 16-bit storage as uint16_t; f16 storage is f16_t inside
inline const f16_t *as_f16(const uint16_t *p) { return reinterpret_cast<const f16_t *>(p); }
inline f16_t *as_f16(uint16_t *p) { return reinterpret_cast<f16_t *>(p); }

int grid_dims(int ref_dim, int ref_per_head, int V, int angle_mode, int B, int Lq, int H,
              int L, int P, GridDims &d)
{
    if (B < 0 || Lq < 0 || H <= 0 || L <= 0 || P <= 0 || angle_mode < 0 || angle_mode > 2)
        return 0;
    if (V != (angle_mode == 1 ? 5 : 4) || ref_dim < (angle_mode ? 5 : 4)) return 0;
    d = GridDims{Lq, H, L, P, V, ref_dim, ref_per_head ? 1 : 0, angle_mode};
    return ((size_t)B * Lq == 0) ? 2 : 1;                       // 2: nothing to do
}
}  // namespace

extern "C" {

int boxattn_grid_fwd_f32(const float *ref, int ref_dim, int ref_per_head, const float *offsets,
                         int V, int angle_mode, const float *kernel_idx,
                         const float *valid_ratios, int B, int Lq, int H, int L, int P,
                         float *grid, void *stream)
{
    GridDims d{};
    const int ok = grid_dims(ref_dim, ref_per_head, V, angle_mode, B, Lq, H, L, P, d);
    if (ok == 2) return 0;
    if (ok != 1 || !ref || !offsets || !kernel_idx || !grid) return (int)hipErrorInvalidValue;
    const size_t n_pts = (size_t)B * Lq * H * L * P;
    const size_t blocks = (n_pts + 255) / 256;
    if (blocks > 0x7fffffffu) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(grid_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       ref, offsets, kernel_idx, valid_ratios, d, n_pts, grid);
    return finish();
}

int boxattn_grid_bwd_f32(const float *ref, int ref_dim, int ref_per_head, const float *offsets,
                         int V, int angle_mode, const float *kernel_idx,
                         const float *valid_ratios, const float *grad_grid, int B, int Lq, int H,
                         int L, int P, float *grad_offsets, float *grad_ref_rows, void *stream)
{
    GridDims d{};
    const int ok = grid_dims(ref_dim, ref_per_head, V, angle_mode, B, Lq, H, L, P, d);
    if (ok == 2) return 0;
    if (ok != 1 || !ref || !offsets || !kernel_idx || !grad_grid || !grad_offsets)
        return (int)hipErrorInvalidValue;
    const size_t n_rows = (size_t)B * Lq * H * L;
    const size_t blocks = (n_rows * 4 + 255) / 256;
    if (blocks > 0x7fffffffu) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(grid_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       ref, offsets, kernel_idx, valid_ratios, grad_grid, d, n_rows, grad_offsets,
                       grad_ref_rows);
    return finish();
}

}  // extern "C"

// ---- pointwise work around the operator ---------------------------------
// lanes per row of the vector kernels (rows of 4, 8, 16, 32 or 64 values, 16-byte aligned
// tensors), 0: the one-thread-per-row kernels
template <typename T>
static int softmax_group(int n, const T *typed, const float *f32)
{
    if (n % 4 != 0 || (n / 4 & (n / 4 - 1)) != 0 || n > 64) return 0;
    return aligned(typed, 16) && aligned(f32, 16) ? n / 4 : 0;
}

template <typename T>
static int softmax_fwd(const T *logits, long long rows, int n, float *attn, hipStream_t st)
{
    if (rows < 0 || n <= 0 || n > 64) return (int)hipErrorInvalidValue;
    if (rows == 0) return 0;
    if (!logits || !attn) return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((rows + 255) / 256);
    const int g = softmax_group(n, logits, attn);
    const size_t total = (size_t)rows * n;
    const unsigned vblocks = (unsigned)((total / 4 + 255) / 256);
#define BOXATTN_SOFTMAX_VEC(G) \
    hipLaunchKernelGGL((softmax_vec_fwd_kernel<T, G>), dim3(vblocks), dim3(256), 0, st, logits, total, attn)
    if (g == 1) BOXATTN_SOFTMAX_VEC(1);
    else if (g == 2) BOXATTN_SOFTMAX_VEC(2);
    else if (g == 4) BOXATTN_SOFTMAX_VEC(4);
    else if (g == 8) BOXATTN_SOFTMAX_VEC(8);
    else if (g == 16) BOXATTN_SOFTMAX_VEC(16);
#undef BOXATTN_SOFTMAX_VEC
    else if (n <= 16)
        hipLaunchKernelGGL((softmax_rows_fwd_kernel<T, 16>), dim3(blocks), dim3(256), 0, st, logits,
                           (size_t)rows, n, attn);
    else
        hipLaunchKernelGGL((softmax_rows_fwd_kernel<T, 64>), dim3(blocks), dim3(256), 0, st, logits,
                           (size_t)rows, n, attn);
    return finish();
}
template <typename T>
static int softmax_bwd(const float *attn, const float *grad_attn, long long rows, int n,
                       T *grad_logits, hipStream_t st)
{
    if (rows < 0 || n <= 0 || n > 64) return (int)hipErrorInvalidValue;
    if (rows == 0) return 0;
    if (!attn || !grad_attn || !grad_logits) return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((rows + 255) / 256);
    const int g = aligned(grad_attn, 16) ? softmax_group(n, grad_logits, attn) : 0;
    const size_t total = (size_t)rows * n;
    const unsigned vblocks = (unsigned)((total / 4 + 255) / 256);
#define BOXATTN_SOFTMAX_VEC(G) \
    hipLaunchKernelGGL((softmax_vec_bwd_kernel<T, G>), dim3(vblocks), dim3(256), 0, st, attn, \
                       grad_attn, total, grad_logits)
    if (g == 1) BOXATTN_SOFTMAX_VEC(1);
    else if (g == 2) BOXATTN_SOFTMAX_VEC(2);
    else if (g == 4) BOXATTN_SOFTMAX_VEC(4);
    else if (g == 8) BOXATTN_SOFTMAX_VEC(8);
    else if (g == 16) BOXATTN_SOFTMAX_VEC(16);
#undef BOXATTN_SOFTMAX_VEC
    else if (n <= 16)
        hipLaunchKernelGGL((softmax_rows_bwd_kernel<T, 16>), dim3(blocks), dim3(256), 0, st, attn,
                           grad_attn, (size_t)rows, n, grad_logits);
    else
        hipLaunchKernelGGL((softmax_rows_bwd_kernel<T, 64>), dim3(blocks), dim3(256), 0, st, attn,
                           grad_attn, (size_t)rows, n, grad_logits);
    return finish();
}

template <typename T, typename OT = bf16_t>
static int value_prep(const T *value, const unsigned char *mask, long long rows, int d,
                      OT *out, hipStream_t st)
{
    if (rows < 0 || d <= 0 || d % 8 != 0) return (int)hipErrorInvalidValue;
    if (rows == 0) return 0;
    if (!value || !out || !aligned(value, 16) || !aligned(out, 16)) return (int)hipErrorInvalidValue;
    const size_t n8 = (size_t)rows * d / 8;
    hipLaunchKernelGGL((value_mask_cast_kernel<T, OT>), dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0,
                       st, value, mask, (size_t)rows, d, out);
    return finish();
}

// ---- instance attention: spatial / level weights from the 2x2 logits and back --------------------------
// k even, 2 <= k <= 32; 1 <= L <= 16 (4 L <= 64 cells: a row fits the lanes of a wave)
static bool inst_dims(int L, int k, InstDims &d)
{
    if (L < 1 || L > 16 || k < 2 || k > 32 || k % 2 != 0) return false;
    const unsigned n4_level = (unsigned)(k * k / 4);
    const float m = (float)(k / 2);
    d = InstDims{L, k, n4_level, n4_level * (unsigned)L, 1.f / (float)k, 1.f / (float)n4_level,
                 1.f / (float)(n4_level * (unsigned)L), 1.f / (m * m)};
    return true;
}
// lanes per row: 4 * (L rounded up to a power of two); blocks of 4 waves with 64 / G rows each, 0: too many
static int inst_group(int L, long long rows, unsigned &blocks)
{
    int g = 4;
    while (g < 4 * L) g *= 2;
    const long long per_block = 4 * (64 / g);
    const long long n = (rows + per_block - 1) / per_block;
    blocks = (unsigned)n;
    return n > 0x7fffffffLL ? 0 : g;
}
#define BOXATTN_INST_GROUPS(LAUNCH) \
    if (g == 4) LAUNCH(4); \
    else if (g == 8) LAUNCH(8); \
    else if (g == 16) LAUNCH(16); \
    else if (g == 32) LAUNCH(32); \
    else LAUNCH(64)

template <typename T>
static int inst_weights_fwd(const T *logits, long long rows, int L, int k, float *spatial_w, float *level_w,
                            hipStream_t st)
{
    InstDims d{};
    unsigned blocks = 0;
    if (rows < 0 || !inst_dims(L, k, d)) return (int)hipErrorInvalidValue;
    if (rows == 0) return 0;
    const int g = inst_group(L, rows, blocks);
    if (!g || !logits || !spatial_w || !aligned(spatial_w, 16) || !aligned(level_w, 16))
        return (int)hipErrorInvalidValue;
#define BOXATTN_INST_FWD(G) \
    hipLaunchKernelGGL((inst_weights_fwd_kernel<T, G>), dim3(blocks), dim3(256), 0, st, logits, (size_t)rows, d, \
                       spatial_w, level_w)
    BOXATTN_INST_GROUPS(BOXATTN_INST_FWD);
#undef BOXATTN_INST_FWD
    return finish();
}

template <typename T>
static int inst_weights_bwd(const T *logits, const float *grad_spatial_w, const float *grad_level_w, long long rows,
                            int L, int k, T *grad_logits, hipStream_t st)
{
    InstDims d{};
    unsigned blocks = 0;
    if (rows < 0 || !inst_dims(L, k, d)) return (int)hipErrorInvalidValue;
    if (rows == 0) return 0;
    const int g = inst_group(L, rows, blocks);
    if (!g || !logits || !grad_logits || !aligned(grad_spatial_w, 16) || !aligned(grad_level_w, 16))
        return (int)hipErrorInvalidValue;
#define BOXATTN_INST_BWD(G) \
    hipLaunchKernelGGL((inst_weights_bwd_kernel<T, G>), dim3(blocks), dim3(256), 0, st, logits, grad_spatial_w, \
                       grad_level_w, (size_t)rows, d, grad_logits)
    BOXATTN_INST_GROUPS(BOXATTN_INST_BWD);
#undef BOXATTN_INST_BWD
    return finish();
}
#undef BOXATTN_INST_GROUPS

extern "C" {

// The storage types of the entry points below: X(suffix, element type of the C ABI, type inside, cast)
#define STORAGE_TYPES(X) X(f32, float, float, ) X(bf16, uint16_t, bf16_t, ) X(f16, uint16_t, f16_t, as_f16)
#define ST_ (hipStream_t) stream

#define SOFTMAX_FWD(SUF, CT, T, CAST)                                                                          \
    int boxattn_softmax_fwd_##SUF(const CT *logits, long long rows, int n, float *attn, void *stream)          \
    {                                                                                                          \
        return softmax_fwd<T>(CAST(logits), rows, n, attn, ST_);                                               \
    }
STORAGE_TYPES(SOFTMAX_FWD)
#undef SOFTMAX_FWD

#define SOFTMAX_BWD(SUF, CT, T, CAST)                                                                          \
    int boxattn_softmax_bwd_##SUF(const float *attn, const float *grad_attn, long long rows, int n,            \
                                  CT *grad_logits, void *stream)                                               \
    {                                                                                                          \
        return softmax_bwd<T>(attn, grad_attn, rows, n, CAST(grad_logits), ST_);                               \
    }
STORAGE_TYPES(SOFTMAX_BWD)
#undef SOFTMAX_BWD

// value_prep: its own table, (suffix, input element type, type inside, cast) and (output type inside, cast)
#define VALUE_PREP(SUF, CT, T, CAST, OT, OCAST)                                                                \
    int boxattn_value_prep_##SUF(const CT *value, const unsigned char *mask, long long rows, int d,            \
                                 uint16_t *out, void *stream)                                                  \
    {                                                                                                          \
        return value_prep<T, OT>(CAST(value), mask, rows, d, OCAST(out), ST_);                                 \
    }
VALUE_PREP(f32, float, float, , bf16_t, )
VALUE_PREP(bf16, uint16_t, bf16_t, , bf16_t, )
VALUE_PREP(f32_f16, float, float, , f16_t, as_f16)
VALUE_PREP(f16, uint16_t, f16_t, as_f16, f16_t, as_f16)
#undef VALUE_PREP

#define INSTATTN_WEIGHTS_FWD(SUF, CT, T, CAST)                                                                 \
    int instattn_weights_fwd_##SUF(const CT *logits, long long rows, int L, int k, float *spatial_w,           \
                                   float *level_w, void *stream)                                               \
    {                                                                                                          \
        return inst_weights_fwd<T>(CAST(logits), rows, L, k, spatial_w, level_w, ST_);                         \
    }
STORAGE_TYPES(INSTATTN_WEIGHTS_FWD)
#undef INSTATTN_WEIGHTS_FWD

#define INSTATTN_WEIGHTS_BWD(SUF, CT, T, CAST)                                                                 \
    int instattn_weights_bwd_##SUF(const CT *logits, const float *grad_spatial_w, const float *grad_level_w,   \
                                   long long rows, int L, int k, CT *grad_logits, void *stream)                \
    {                                                                                                          \
        return inst_weights_bwd<T>(CAST(logits), grad_spatial_w, grad_level_w, rows, L, k, CAST(grad_logits),  \
                                   ST_);                                                                       \
    }
STORAGE_TYPES(INSTATTN_WEIGHTS_BWD)
#undef INSTATTN_WEIGHTS_BWD
#undef ST_
#undef STORAGE_TYPES

}  // extern "C"
