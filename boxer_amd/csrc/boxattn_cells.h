// Instance attention's 2x2 cells: the softmaxes over a row's 4 L logits and the per-cell gradient sums that the weight
// kernels (boxattn_pointwise.h, translation unit boxattn_extras.hip) and the kernels that take boxes and logits
// (boxattn_boxes.h, boxattn_boxes_bwd.h, translation unit boxattn_capi.hip) share -- one text, so both make the same numbers.  Device helpers only: no kernel is defined here.
#pragma once
#include "boxattn_device.h"

namespace boxattn {

template <typename T> __device__ __forceinline__ float pw_ld(const T *p);
template <> __device__ __forceinline__ float pw_ld<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float pw_ld<bf16_t>(const bf16_t *p) { return bf16_bits_to_f32(*p); }
template <> __device__ __forceinline__ float pw_ld<f16_t>(const f16_t *p) { return (float)*p; }

template <int FROM, int G> __device__ __forceinline__ float lanes_max(float v)   // over lanes FROM, 2 FROM, .. G/2 apart
{
#pragma unroll
    for (int o = FROM; o < G; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
template <int FROM, int G> __device__ __forceinline__ float lanes_add(float v)
{
#pragma unroll
    for (int o = FROM; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// q / d for q < 2^20 from rcp = 1.f / d: (q + 0.5) / d is at least 0.5 / d away from an integer, the two
// roundings (rcp, the product) move it by less than (q + 0.5) / d * 2^-22
__device__ __forceinline__ unsigned small_div(unsigned q, float rcp)
{
    return (unsigned)(((float)q + 0.5f) * rcp);
}

// this lane's cell: a (softmax over the row, not yet divided by m^2) and t (softmax over the levels).  A row takes G
// adjacent lanes (a power of two >= 4 L), lane c of them cell c (l = c / 4, i = c / 2 % 2, j = c % 2); a wider G than
// the row needs adds lanes that hold -inf / 0 and leaves every result bit for bit as it is
template <typename T, int G>
__device__ __forceinline__ void inst_cell_softmax(const T *__restrict__ logits, size_t row, int c, int L,
                                                  float &a, float &t)
{
    const float z = c < 4 * L ? pw_ld<T>(logits + row * (size_t)(4 * L) + c) : -INFINITY;
    const float ea = __expf(z - lanes_max<1, G>(z));
    a = ea * (1.f / lanes_add<1, G>(ea));
    const float et = __expf(z - lanes_max<4, G>(z));          // (level 0 is always there: the maxima are finite)
    t = et * (1.f / lanes_add<4, G>(et));
}

// per-cell sums of a level's upstream weight gradients (the weight backward, and the backward that takes boxes)
struct InstCellSums { float c0, c1, c2, c3; };
__device__ __forceinline__ void inst_cell_add(InstCellSums &s, bool hi_y, bool hi_x, float g)
{
    s.c0 += !hi_y && !hi_x ? g : 0.f;
    s.c1 += !hi_y && hi_x ? g : 0.f;
    s.c2 += hi_y && !hi_x ? g : 0.f;
    s.c3 += hi_y && hi_x ? g : 0.f;
}
// the four lanes of a level: sum the partial cell sums over them (DPP quad), lane s keeps cell s
__device__ __forceinline__ float inst_cell_total(const InstCellSums &s, int sub)
{
    const float c0 = lanes_add<1, 4>(s.c0), c1 = lanes_add<1, 4>(s.c1), c2 = lanes_add<1, 4>(s.c2),
                c3 = lanes_add<1, 4>(s.c3);
    return sub == 0 ? c0 : sub == 1 ? c1 : sub == 2 ? c2 : c3;
}

}  // namespace boxattn
