// Translation unit of the kernels that run float32 VALU arithmetic next to MFMAs: the window-staged
// encoder kernels (boxattn_dense.h) and the matrix-core accumulate (boxattn_binned_tr.h), bf16 and f16.  Built with
// -fno-slp-vectorize (boxer_amd/_lib.py SOURCES): a packed float32 instruction
// (v_pk_mul_f32 / v_pk_fma_f32, which the SLP vectoriser makes of neighbouring scalar operations) issued
// while an MFMA of the same wave is completing was seen to return wrong values on MI355X.
#include "boxattn_dense.h"
#include "boxattn_binned_tr.h"
#include "boxattn_dense_fwd.h"
#include "boxattn_dense_f32.h"
#include "boxattn_dense_boxes_bwd.h"

namespace boxattn {

// rider workgroups of a launch: the caller sets ride.grid.n_riders / .shift, the rest follows from the grid
static BinRide place_riders(BinRide ride, unsigned own_blocks, unsigned *total)
{
    ride.grid = ride_grid(ride.grid.n_riders, own_blocks, ride.grid.shift, total);
    return ride;
}

template <typename ST>
void launch_pointgrad_dense(const ST *value, const float *loc, const float *attn,
                            const ST *grad_out, const DensePlan &dp, float *grad_loc,
                            float *grad_attn, unsigned value_bytes, hipStream_t st, const BinRide &ride_in)
{
    unsigned total = 0;
    const BinRide ride = place_riders(ride_in, dense_blocks(dp), &total);
#define BOXATTN_DENSE_PG(LV_)                                                                           \
    case LV_:                                                                                           \
        hipLaunchKernelGGL((pointgrad_dense_kernel<ST, LV_>), dim3(total), dim3(256), 0, st, value, loc, attn, \
                           grad_out, grad_loc, grad_attn, dp, value_bytes, ride);                      \
        break;
    switch (dp.L) {
        BOXATTN_DENSE_PG(1) BOXATTN_DENSE_PG(2) BOXATTN_DENSE_PG(3) BOXATTN_DENSE_PG(4)
    }
#undef BOXATTN_DENSE_PG
}

template <typename ST>
void launch_fwd_dense(const ST *value, const float *loc, const float *attn, ST *out,
                      const DensePlan &dp, unsigned value_bytes, const BinRide &ride_in,
                      unsigned long long *stats, hipStream_t st)
{
    unsigned total = 0;
    const BinRide ride = place_riders(ride_in, dense_blocks(dp), &total);
#define BOXATTN_DENSE_FWD(LV_)                                                                       \
    case LV_:                                                                                        \
        hipLaunchKernelGGL((fwd_dense_kernel<ST, LV_>), dim3(total), dim3(256), 0, st, value, loc, attn, out, \
                           dp, value_bytes, ride, stats);                                            \
        break;
    switch (dp.L) {
        BOXATTN_DENSE_FWD(1) BOXATTN_DENSE_FWD(2) BOXATTN_DENSE_FWD(3) BOXATTN_DENSE_FWD(4)
    }
#undef BOXATTN_DENSE_FWD
}

void launch_pointgrad_dense_f32(const float *value, const float *loc, const float *attn, const float *grad_out,
                                const DensePlan &dp, float *grad_loc, float *grad_attn, unsigned value_bytes,
                                hipStream_t st, const BinRide &ride_in)
{
    unsigned total = 0;
    const BinRide ride = place_riders(ride_in, dense_blocks(dp), &total);
#define BOXATTN_DENSE_PG32(LV_)                                                                         \
    case LV_:                                                                                           \
        hipLaunchKernelGGL((pointgrad_dense_f32_kernel<LV_>), dim3(total), dim3(256), 0, st, value, loc, attn, \
                           grad_out, grad_loc, grad_attn, dp, value_bytes, ride);                      \
        break;
    switch (dp.L) {
        BOXATTN_DENSE_PG32(1) BOXATTN_DENSE_PG32(2) BOXATTN_DENSE_PG32(3) BOXATTN_DENSE_PG32(4)
    }
#undef BOXATTN_DENSE_PG32
}

void launch_fwd_dense_f32(const float *value, const float *loc, const float *attn, float *out, const DensePlan &dp,
                          unsigned value_bytes, const BinRide &ride_in, unsigned long long *stats, hipStream_t st)
{
    unsigned total = 0;
    const BinRide ride = place_riders(ride_in, dense_blocks(dp), &total);
#define BOXATTN_DENSE_FWD32(LV_)                                                                     \
    case LV_:                                                                                        \
        hipLaunchKernelGGL((fwd_dense_f32_kernel<LV_>), dim3(total), dim3(256), 0, st, value, loc, attn, out, \
                           dp, value_bytes, ride, stats);                                            \
        break;
    switch (dp.L) {
        BOXATTN_DENSE_FWD32(1) BOXATTN_DENSE_FWD32(2) BOXATTN_DENSE_FWD32(3) BOXATTN_DENSE_FWD32(4)
    }
#undef BOXATTN_DENSE_FWD32
}

// the forwards from boxes and logits: no riders, one workgroup a (tile, head)
template <typename ST>
void launch_fwd_dense_boxes(const ST *value, const DenseBoxes &bx, ST *out, const DensePlan &dp, unsigned value_bytes,
                            hipStream_t st)
{
    const GridDims gd{dp.Lq, dp.H, dp.L, 4, bx.V, bx.ref_dim, bx.ref_per_head, bx.angle_mode};
#define BOXATTN_DENSE_FWD_BOXES(LV_)                                                                       \
    case LV_:                                                                                              \
        if constexpr (sizeof(ST) == 2)                                                                     \
            hipLaunchKernelGGL((fwd_dense_boxes_kernel<ST, LV_>), dim3(dense_blocks(dp)), dim3(256), 0, st, value, \
                               bx.ref, bx.offsets, bx.kernel_idx, bx.valid_ratios, bx.logits, out, dp, value_bytes, gd); \
        else                                                                                               \
            hipLaunchKernelGGL((fwd_dense_f32_boxes_kernel<LV_>), dim3(dense_blocks(dp)), dim3(256), 0, st, value, \
                               bx.ref, bx.offsets, bx.kernel_idx, bx.valid_ratios, bx.logits, out, dp, value_bytes, gd); \
        break;
    switch (dp.L) {
        BOXATTN_DENSE_FWD_BOXES(1) BOXATTN_DENSE_FWD_BOXES(2) BOXATTN_DENSE_FWD_BOXES(3) BOXATTN_DENSE_FWD_BOXES(4)
    }
#undef BOXATTN_DENSE_FWD_BOXES
}
template void launch_fwd_dense_boxes<float>(const float *, const DenseBoxes &, float *, const DensePlan &, unsigned,
                                            hipStream_t);

// the box and logit gradients from boxes and logits (boxattn_dense_boxes_bwd.h): no riders, one workgroup a (tile, head)
template <typename ST>
void launch_pointgrad_dense_boxes(const ST *value, const DenseBoxes &bx, const ST *grad_out, const DenseBoxesGrads &g,
                                  const DensePlan &dp, unsigned value_bytes, hipStream_t st)
{
    const GridDims gd{dp.Lq, dp.H, dp.L, 4, bx.V, bx.ref_dim, bx.ref_per_head, bx.angle_mode};
#define BOXATTN_DENSE_PG_BOXES(LV_)                                                                        \
    case LV_:                                                                                              \
        if constexpr (sizeof(ST) == 2)                                                                     \
            hipLaunchKernelGGL((pointgrad_dense_boxes_kernel<ST, LV_>), dim3(dense_blocks(dp)), dim3(256), 0, st, value, \
                               bx.ref, bx.offsets, bx.kernel_idx, bx.valid_ratios, bx.logits, grad_out, g.offsets, \
                               g.ref_rows, g.logits, dp, value_bytes, gd);                                 \
        else                                                                                               \
            hipLaunchKernelGGL((pointgrad_dense_f32_boxes_kernel<LV_>), dim3(dense_blocks(dp)), dim3(256), 0, st, value, \
                               bx.ref, bx.offsets, bx.kernel_idx, bx.valid_ratios, bx.logits, grad_out, g.offsets, \
                               g.ref_rows, g.logits, dp, value_bytes, gd);                                 \
        break;
    switch (dp.L) {
        BOXATTN_DENSE_PG_BOXES(1) BOXATTN_DENSE_PG_BOXES(2) BOXATTN_DENSE_PG_BOXES(3) BOXATTN_DENSE_PG_BOXES(4)
    }
#undef BOXATTN_DENSE_PG_BOXES
}
template void launch_pointgrad_dense_boxes<float>(const float *, const DenseBoxes &, const float *,
                                                  const DenseBoxesGrads &, const DensePlan &, unsigned, hipStream_t);

template <typename ST>
void launch_accumulate_tr(int C, const ST *grad_out, size_t grad_out_bytes, const BinPlan &plan, int S,
                          int H, int Lq, const int4 *items, const int *n_items, const int *records,
                          ST *grad_value, float *partials, int wg_per_slice, int ns8, const ChunkCombine &cc,
                          const ZeroRole &zr, hipStream_t st)
{
#define BOXATTN_ACC_TR(C_)                                                                              \
    hipLaunchKernelGGL((binned_accumulate_tr_kernel<ST, C_>), dim3(wg_per_slice + plan.zero_workers, ns8), dim3(64), 0, st, \
                       grad_out, (unsigned)grad_out_bytes, plan, S, H, Lq, items, n_items, records,     \
                       grad_value, partials, cc, zr, InstRowsT<ST>{}, GroupPts{})
    switch (C) {
    case 16: BOXATTN_ACC_TR(16); break;
    case 32: BOXATTN_ACC_TR(32); break;
    case 64: BOXATTN_ACC_TR(64); break;
    }
#undef BOXATTN_ACC_TR
}

// group records (the kernel's GRP flavour): the group's locations and weights are gathered by the record's id
template <typename ST>
void launch_accumulate_tr_group(int C, const ST *grad_out, size_t grad_out_bytes, const BinPlan &plan, int S,
                                int H, int Lq, const int4 *items, const int *n_items, const int *records,
                                ST *grad_value, float *partials, int wg_per_slice, int ns8, const ChunkCombine &cc,
                                const ZeroRole &zr, hipStream_t st, const float *loc, const float *attn, size_t loc_bytes)
{
    const GroupPts gp{loc, attn, (unsigned)loc_bytes};
#define BOXATTN_ACC_TR_GRP(C_)                                                                          \
    hipLaunchKernelGGL((binned_accumulate_tr_kernel<ST, C_, false, true>), dim3(wg_per_slice + plan.zero_workers, ns8), dim3(64), 0, st, \
                       grad_out, (unsigned)grad_out_bytes, plan, S, H, Lq, items, n_items, records,     \
                       grad_value, partials, cc, zr, InstRowsT<ST>{}, gp)
    switch (C) {
    case 16: BOXATTN_ACC_TR_GRP(16); break;
    case 32: BOXATTN_ACC_TR_GRP(32); break;
    case 64: BOXATTN_ACC_TR_GRP(64); break;
    }
#undef BOXATTN_ACC_TR_GRP
}

// instance attention: two upstream rows per record (the kernel's INST flavour)
template <typename ST>
void launch_accumulate_tr_inst(int C, const ST *grad_out, size_t grad_out_bytes, const BinPlan &plan, int S,
                               int H, int Lq, const int4 *items, const int *n_items, const int *records,
                               ST *grad_value, float *partials, int wg_per_slice, int ns8, const ChunkCombine &cc,
                               const ZeroRole &zr, hipStream_t st, const ST *grad_mask, size_t grad_mask_bytes,
                               const float *w_lv, int P)
{
    const InstRowsT<ST> inst{grad_mask, (unsigned)grad_mask_bytes, w_lv, P};
#define BOXATTN_ACC_TR_INST(C_)                                                                         \
    hipLaunchKernelGGL((binned_accumulate_tr_kernel<ST, C_, true>), dim3(wg_per_slice + plan.zero_workers, ns8), dim3(64), 0, st, \
                       grad_out, (unsigned)grad_out_bytes, plan, S, H, Lq, items, n_items, records,     \
                       grad_value, partials, cc, zr, inst, GroupPts{})
    switch (C) {
    case 16: BOXATTN_ACC_TR_INST(16); break;
    case 32: BOXATTN_ACC_TR_INST(32); break;
    case 64: BOXATTN_ACC_TR_INST(64); break;
    }
#undef BOXATTN_ACC_TR_INST
}

// one source per kernel family, instantiated for both 16-bit storage types
#define BOXATTN_DENSE_H16(ST_)                                                                              \
    template void launch_pointgrad_dense<ST_>(const ST_ *, const float *, const float *, const ST_ *,       \
                                              const DensePlan &, float *, float *, unsigned, hipStream_t,   \
                                              const BinRide &);                                             \
    template void launch_fwd_dense<ST_>(const ST_ *, const float *, const float *, ST_ *, const DensePlan &, \
                                        unsigned, const BinRide &, unsigned long long *, hipStream_t);      \
    template void launch_fwd_dense_boxes<ST_>(const ST_ *, const DenseBoxes &, ST_ *, const DensePlan &,   \
                                              unsigned, hipStream_t);                                       \
    template void launch_pointgrad_dense_boxes<ST_>(const ST_ *, const DenseBoxes &, const ST_ *,           \
                                                    const DenseBoxesGrads &, const DensePlan &, unsigned,   \
                                                    hipStream_t);                                           \
    template void launch_accumulate_tr<ST_>(int, const ST_ *, size_t, const BinPlan &, int, int, int,       \
                                            const int4 *, const int *, const int *, ST_ *, float *, int, int, \
                                            const ChunkCombine &, const ZeroRole &, hipStream_t);              \
    template void launch_accumulate_tr_group<ST_>(int, const ST_ *, size_t, const BinPlan &, int, int, int, \
                                                  const int4 *, const int *, const int *, ST_ *, float *, int, int, \
                                                  const ChunkCombine &, const ZeroRole &, hipStream_t, const float *, \
                                                  const float *, size_t);                                   \
    template void launch_accumulate_tr_inst<ST_>(int, const ST_ *, size_t, const BinPlan &, int, int, int,  \
                                                 const int4 *, const int *, const int *, ST_ *, float *, int, int, \
                                                 const ChunkCombine &, const ZeroRole &, hipStream_t, const ST_ *, \
                                                 size_t, const float *, int);
BOXATTN_DENSE_H16(bf16_t)
BOXATTN_DENSE_H16(f16_t)
#undef BOXATTN_DENSE_H16

void launch_accumulate_split(const float *grad_out, size_t grad_out_bytes, const BinPlan &plan, int S, int H, int Lq,
                             const int4 *items, const int *n_items, const int *records, float *grad_value,
                             float *partials, int wg_per_slice, int ns8, const ChunkCombine &cc, const ZeroRole &zr,
                             hipStream_t st, const float *grad_mask, size_t grad_mask_bytes, const float *w_lv, int P)
{
    const InstRows inst{grad_mask, (unsigned)grad_mask_bytes, w_lv, P};
    if (grad_mask)      // instance attention: two upstream rows per record
        hipLaunchKernelGGL((binned_accumulate_split_kernel<32, true>), dim3(wg_per_slice + plan.zero_workers, ns8), dim3(64), 0, st,
                           grad_out, (unsigned)grad_out_bytes, plan, S, H, Lq, items, n_items, records, grad_value, partials, cc,
                           zr, inst);
    else
        hipLaunchKernelGGL((binned_accumulate_split_kernel<32, false>), dim3(wg_per_slice + plan.zero_workers, ns8), dim3(64), 0, st,
                           grad_out, (unsigned)grad_out_bytes, plan, S, H, Lq, items, n_items, records, grad_value, partials, cc,
                           zr, inst);
}

void launch_accumulate_f32(const float *grad_out, size_t grad_out_bytes, const BinPlan &plan, int S, int H, int Lq,
                           const int4 *items, const int *n_items, const int *records, float *grad_value,
                           float *partials, int wg_per_slice, int ns8, const ChunkCombine &cc, const ZeroRole &zr,
                           hipStream_t st)
{
    hipLaunchKernelGGL((binned_accumulate_f32_kernel<32>), dim3(wg_per_slice + plan.zero_workers, ns8), dim3(64), 0, st, grad_out,
                       (unsigned)grad_out_bytes, plan, S, H, Lq, items, n_items, records, grad_value, partials, cc, zr);
}

}  // namespace boxattn
