/*
 * boxattn.h -- C ABI of the MI355X (gfx950) box-attention / instance-attention operator.
 *
 * This is the drop-in boundary for the one native component of kienduynguyen/BoxeR: the
 * `e2edet.ops` extension with its four entry points (reference:
 * e2edet/module/ops/src/vision.cpp:7-12).  Each group of functions below replaces one of
 * them; the reference-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions (all functions):
 *   - Every pointer is a DEVICE pointer on the current HIP device, including the int64
 *     shape tables (the reference passes them as CUDA tensors, box_attn.cu:25-26).
 *   - Tensors are dense, row-major, contiguous (reference CHECK_CONTIGUOUS, box_attn.cu:9-11):
 *       value        (B, S, H, C)          S = sum_l H_l*W_l
 *       shapes       (L, 2) int64          (H_l, W_l)
 *       lsi          (L,)   int64          first row of level l inside S
 *       loc          (B, Lq, H, L, P, 2)   normalised [0,1]; [..,0]=x (width), [..,1]=y
 *       attn / spatial_w / level_w         (B, Lq, H, L, P)
 *       out, grad_out                      (B, Lq, H, C)
 *       mask_out, grad_mask                (B, Lq, P, H, C)
 *   - Inputs are borrowed and never written.  Outputs are FULLY DEFINED by the call: the
 *     functions zero-fill whatever they accumulate into (the reference relies on
 *     at::zeros / zeros_like in its host code, box_attn.cu:44,105-107), so callers may pass
 *     uninitialised memory.  Nothing is allocated or freed behind the ABI.
 *   - `stream` is a hipStream_t (NULL = the default stream).  Calls are asynchronous.
 *   - Return value: 0 on success, otherwise a hipError_t value (1 = hipErrorInvalidValue
 *     for bad arguments).  Launch failures are returned, never just printed (the reference
 *     only printf's them, box_attn_kernel.cuh:1118-1122).
 *   - There is no `im2col_step`: in the reference it is pure batch chunking of the launch
 *     (box_attn.cu:40-66) with no numerical effect.  One call covers the whole batch.
 *
 * Numeric types (suffix):
 *   _f32   everything float32                      (the reference's training path)
 *   _f64   everything float64                      (the reference's gradcheck path)
 *   _bf16  value / out / mask_out / grad_out / grad_mask / grad_value are bfloat16;
 *          loc, weights and their gradients stay float32; accumulation is float32.
 *          (New: the reference raises on BFloat16, box_attn.cu:54.)  The backward needs a
 *          float32 scratch of B*S*H*C elements for the grad_value accumulation.
 *   _f16   the same with IEEE binary16 storage (uint16_t bit patterns): every _bf16 entry point
 *          has an _f16 twin of the same signature and contract, running the same kernels.
 *          Results are rounded to nearest even; magnitudes beyond 65504 become +-inf (no
 *          overflow guarding: under loss scaling that is the scaler's business).
 *   "16-bit storage" below means _bf16 or _f16.
 */
#ifndef BOXATTN_H_
#define BOXATTN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header; bumped on any signature change. */
#define BOXATTN_ABI_VERSION 8
int boxattn_abi_version(void);

/* Static description of the build ("gfx950", compiler, kernel variants); never NULL. */
const char *boxattn_build_info(void);

/* ---- replaces box_attn_forward (box_attn.h:29-54, box_attn.cu:15-71) ------------------ */
int boxattn_fwd_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                    const float *loc, const float *attn, int B, int S, int H, int C, int L,
                    int Lq, int P, float *out, void *stream);
int boxattn_fwd_f64(const double *value, const int64_t *shapes, const int64_t *lsi,
                    const double *loc, const double *attn, int B, int S, int H, int C, int L,
                    int Lq, int P, double *out, void *stream);
int boxattn_fwd_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                     const float *loc, const float *attn, int B, int S, int H, int C, int L,
                     int Lq, int P, uint16_t *out, void *stream);
int boxattn_fwd_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                    const float *loc, const float *attn, int B, int S, int H, int C, int L,
                    int Lq, int P, uint16_t *out, void *stream);

/* Forward with HOST copies of the two level tables next to the device ones (either may be
 * NULL): lets the library recognise the encoder case -- one query per pixel of the packed
 * multi-level map (Lq == S; box_transformer.py:346-354) -- and run the window-staged kernels
 * (a query tile's value windows in LDS, arithmetic on the matrix cores) instead of the row
 * gathers.  Same results as boxattn_fwd_*. */
int boxattn_fwd_hl_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                       const float *loc, const float *attn, int B, int S, int H, int C, int L,
                       int Lq, int P, float *out, const int64_t *shapes_host,
                       const int64_t *lsi_host, void *stream);
int boxattn_fwd_hl_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                        const float *loc, const float *attn, int B, int S, int H, int C, int L,
                        int Lq, int P, uint16_t *out, const int64_t *shapes_host,
                        const int64_t *lsi_host, void *stream);
int boxattn_fwd_hl_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                       const float *loc, const float *attn, int B, int S, int H, int C, int L,
                       int Lq, int P, uint16_t *out, const int64_t *shapes_host,
                       const int64_t *lsi_host, void *stream);

/* ---- replaces box_attn_backward (box_attn.h:56-83, box_attn.cu:74-135) ---------------- */
int boxattn_bwd_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                    const float *loc, const float *attn, const float *grad_out, int B, int S,
                    int H, int C, int L, int Lq, int P, float *grad_value, float *grad_loc,
                    float *grad_attn, void *stream);
int boxattn_bwd_f64(const double *value, const int64_t *shapes, const int64_t *lsi,
                    const double *loc, const double *attn, const double *grad_out, int B,
                    int S, int H, int C, int L, int Lq, int P, double *grad_value,
                    double *grad_loc, double *grad_attn, void *stream);
/* grad_value_ws: float32 scratch, B*S*H*C elements, contents ignored and clobbered. */
int boxattn_bwd_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                     const float *loc, const float *attn, const uint16_t *grad_out, int B,
                     int S, int H, int C, int L, int Lq, int P, uint16_t *grad_value,
                     float *grad_loc, float *grad_attn, float *grad_value_ws, void *stream);
int boxattn_bwd_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                    const float *loc, const float *attn, const uint16_t *grad_out, int B,
                    int S, int H, int C, int L, int Lq, int P, uint16_t *grad_value,
                    float *grad_loc, float *grad_attn, float *grad_value_ws, void *stream);

/* ---- replaces instance_attn_forward (instance_attn.h:32-59, instance_attn.cu:15-82) --- */
int instattn_fwd_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                     const float *loc, const float *spatial_w, const float *level_w, int B,
                     int S, int H, int C, int L, int Lq, int P, float *out, float *mask_out,
                     void *stream);
int instattn_fwd_f64(const double *value, const int64_t *shapes, const int64_t *lsi,
                     const double *loc, const double *spatial_w, const double *level_w, int B,
                     int S, int H, int C, int L, int Lq, int P, double *out, double *mask_out,
                     void *stream);
int instattn_fwd_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                      const float *loc, const float *spatial_w, const float *level_w, int B,
                      int S, int H, int C, int L, int Lq, int P, uint16_t *out,
                      uint16_t *mask_out, void *stream);
int instattn_fwd_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                     const float *loc, const float *spatial_w, const float *level_w, int B,
                     int S, int H, int C, int L, int Lq, int P, uint16_t *out,
                     uint16_t *mask_out, void *stream);

/* ---- replaces instance_attn_backward (instance_attn.h:61-92, instance_attn.cu:85-157) - */
int instattn_bwd_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                     const float *loc, const float *spatial_w, const float *level_w,
                     const float *grad_out, const float *grad_mask, int B, int S, int H, int C,
                     int L, int Lq, int P, float *grad_value, float *grad_loc,
                     float *grad_spatial_w, float *grad_level_w, void *stream);
int instattn_bwd_f64(const double *value, const int64_t *shapes, const int64_t *lsi,
                     const double *loc, const double *spatial_w, const double *level_w,
                     const double *grad_out, const double *grad_mask, int B, int S, int H,
                     int C, int L, int Lq, int P, double *grad_value, double *grad_loc,
                     double *grad_spatial_w, double *grad_level_w, void *stream);
int instattn_bwd_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                      const float *loc, const float *spatial_w, const float *level_w,
                      const uint16_t *grad_out, const uint16_t *grad_mask, int B, int S, int H,
                      int C, int L, int Lq, int P, uint16_t *grad_value, float *grad_loc,
                      float *grad_spatial_w, float *grad_level_w, float *grad_value_ws,
                      void *stream);
int instattn_bwd_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                     const float *loc, const float *spatial_w, const float *level_w,
                     const uint16_t *grad_out, const uint16_t *grad_mask, int B, int S, int H,
                     int C, int L, int Lq, int P, uint16_t *grad_value, float *grad_loc,
                     float *grad_spatial_w, float *grad_level_w, float *grad_value_ws,
                     void *stream);

/*
 * ---- backward with a caller-provided workspace (the fast path) ---------------------------
 * Same contract as the plain backward entry points above, plus:
 *   shapes_host / lsi_host : HOST copies of the two int64 level tables (the reference keeps
 *       them only on the device; the binding caches a host copy per tensor).  They let the
 *       library plan the destination-binned algorithm without a
 *       device->host sync.  May be NULL: the call then behaves like the plain backward.
 *   workspace / workspace_bytes : device scratch, 256-byte aligned, contents ignored and
 *       clobbered; size from boxattn_bwd_workspace_bytes() (covers the 16-bit fp32 scratch too).
 *       It only lives inside the call (bin records, partial tiles).
 *   plan / plan_bytes : NULL / 0 -- the call plans for itself (count + scan passes first) -- or the
 *       buffer a *_fwd_train_* call filled (*plan_built == 1) for the SAME sampling locations,
 *       dimensions and option settings; it is only read.
 *   hints : 0, or BOXATTN_HINT_* bits (see *_fwd_train_*); speed only, never results.
 *   state / state_bytes : NULL / 0, or the caller's state buffer of this (stream, dimensions, level shapes) -- see
 *       *_fwd_train_* below.  With it, box attention whose accumulate runs on the matrix cores (16-bit storage at 16 /
 *       32 / 64 channels per head, float32 at 32) on maps of up to 1 279 blocks of 8x4 pixels per (image, head) fills
 *       its bins in ONE pass: the state keeps, per block, the record range the previous call planned
 *       from its own counts; the fill riders claim slots in those ranges with one returned atomic per block and step;
 *       a block that outgrows its range is recomputed from the sampling locations by a redo worker of the accumulate
 *       launch; every call re-plans the ranges for the next one.  Results never depend on what the state holds; the
 *       first call on a zeroed (or foreign-shaped) state runs the two-pass passes.  Such a call takes no plan.
 * If the shape is not eligible or the workspace is too small, the call falls back to the
 * atomic kernels of the plain entry points (for _bf16 / _f16 the workspace must then still hold
 * B*S*H*C floats); a plan the backward cannot use (operands the fast paths reject) is ignored.
 * Only float32, bfloat16 and float16 exist here; float64 uses the plain backward.
 * is_16bit (here and in boxattn_plan_bytes): non-zero for 16-bit storage, bf16 or f16 alike -- both
 * types plan the same way and ask for the same sizes.
 * The binned path uses no float atomics and no zero-fill.  Everything runs on `stream`:
 *   [count + scans, unless a plan is given] -> point-gradient kernel with the fill pass riding in its
 *   launch -> accumulate kernel (the partial tiles of chunked blocks summed by their last chunk).
 */
size_t boxattn_bwd_workspace_bytes(int is_16bit, int B, int S, int H, int C, int L, int Lq, int P,
                                   const int64_t *shapes_host, const int64_t *lsi_host);
int boxattn_bwd_ws_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                       const float *loc, const float *attn, const float *grad_out, int B, int S,
                       int H, int C, int L, int Lq, int P, float *grad_value, float *grad_loc,
                       float *grad_attn, const int64_t *shapes_host, const int64_t *lsi_host,
                       void *workspace, size_t workspace_bytes, const void *plan, size_t plan_bytes,
                       void *state, size_t state_bytes, int hints, void *stream);
int boxattn_bwd_ws_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                        const float *loc, const float *attn, const uint16_t *grad_out, int B,
                        int S, int H, int C, int L, int Lq, int P, uint16_t *grad_value,
                        float *grad_loc, float *grad_attn, const int64_t *shapes_host,
                        const int64_t *lsi_host, void *workspace, size_t workspace_bytes,
                        const void *plan, size_t plan_bytes, void *state, size_t state_bytes, int hints,
                        void *stream);
int boxattn_bwd_ws_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                       const float *loc, const float *attn, const uint16_t *grad_out, int B,
                       int S, int H, int C, int L, int Lq, int P, uint16_t *grad_value,
                       float *grad_loc, float *grad_attn, const int64_t *shapes_host,
                       const int64_t *lsi_host, void *workspace, size_t workspace_bytes,
                       const void *plan, size_t plan_bytes, void *state, size_t state_bytes, int hints,
                       void *stream);
int instattn_bwd_ws_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                        const float *loc, const float *spatial_w, const float *level_w,
                        const float *grad_out, const float *grad_mask, int B, int S, int H, int C,
                        int L, int Lq, int P, float *grad_value, float *grad_loc,
                        float *grad_spatial_w, float *grad_level_w, const int64_t *shapes_host,
                        const int64_t *lsi_host, void *workspace, size_t workspace_bytes,
                        const void *plan, size_t plan_bytes, void *state, size_t state_bytes, int hints,
                        void *stream);
int instattn_bwd_ws_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                         const float *loc, const float *spatial_w, const float *level_w,
                         const uint16_t *grad_out, const uint16_t *grad_mask, int B, int S, int H,
                         int C, int L, int Lq, int P, uint16_t *grad_value, float *grad_loc,
                         float *grad_spatial_w, float *grad_level_w, const int64_t *shapes_host,
                         const int64_t *lsi_host, void *workspace, size_t workspace_bytes,
                         const void *plan, size_t plan_bytes, void *state, size_t state_bytes, int hints,
                        void *stream);
int instattn_bwd_ws_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                        const float *loc, const float *spatial_w, const float *level_w,
                        const uint16_t *grad_out, const uint16_t *grad_mask, int B, int S, int H,
                        int C, int L, int Lq, int P, uint16_t *grad_value, float *grad_loc,
                        float *grad_spatial_w, float *grad_level_w, const int64_t *shapes_host,
                        const int64_t *lsi_host, void *workspace, size_t workspace_bytes,
                        const void *plan, size_t plan_bytes, void *state, size_t state_bytes, int hints,
                       void *stream);

/*
 * ---- partial backward: only the gradients the caller asks for -----------------------------------
 * A backward has two gradient groups, computed by independent launches wherever the fast paths run:
 *     VALUE  : grad_value
 *     POINTS : grad_loc + grad_attn (instance attention: grad_loc + grad_spatial_w + grad_level_w)
 * *_bwd_part_* take the arguments of *_bwd_ws_* (float64: of *_bwd_f64) and `want`, the groups to compute:
 *   - want is BOXATTN_WANT_VALUE (1), BOXATTN_WANT_POINTS (2) or both (3); anything else is hipErrorInvalidValue.
 *   - want == 3 IS the *_bwd_ws_* call (float64: the plain call): both entry points are wrappers of one routine that
 *     takes `want` -- same checks, same launches, same results.
 *   - The output pointers of a group that is not wanted are ignored and may be NULL; nothing is written through
 *     them.  A wanted group with a NULL member is hipErrorInvalidValue (nothing is launched).
 *   - The wanted outputs are fully defined by the call, as everywhere in this ABI.
 *   - The degenerate cases keep their meaning for the wanted group: no pixels (B*S == 0) -> the wanted POINTS
 *     gradients are zero-filled; no queries -> a wanted grad_value is zero-filled.
 * want == POINTS:
 *   `workspace`, `plan` and `state` are ignored (NULL / 0 are fine).  ONE launch: the point-gradient kernel the full
 *   call would pick -- window-staged in the encoder case (16-bit and float32; BOXATTN_HINT_NOT_LOCAL and option 11
 *   are honoured), else the row-gather kernel, else the atomic kernels' points-only form (float64, channel counts
 *   the fast kernels do not take, variants 1 / 2) -- with no fill pass riding in it.  No zero-fill of grad_value, no
 *   binning, no accumulate, no 16-bit conversion pass.  shapes_host / lsi_host may be NULL: the call then takes the
 *   non-staged (atomic-family) kernels, as a full call without them would.
 * want == VALUE:
 *   Where the binned path is eligible (the test of *_bwd_ws_*, less the alignment of grad_loc):
 *   [count + scans, unless a valid plan is passed] -> the fill pass as a launch of its own -> accumulate -> the
 *   combine wherever the full call would run it.  The one-pass fill is NOT used (its riders live in the
 *   point-gradient launch): `state` is neither read nor written and the library notes nothing about it -- a later
 *   full call on that state behaves as if the partial call had not happened.
 *   Otherwise: zero-fill, the atomic kernels' value-only form (no loads of `value`, no reductions), and for 16-bit
 *   storage the conversion pass; the workspace must then hold B*S*H*C floats, as for *_bwd_ws_*.
 */
#define BOXATTN_WANT_VALUE  1
#define BOXATTN_WANT_POINTS 2
int boxattn_bwd_part_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                         const float *loc, const float *attn, const float *grad_out, int B, int S,
                         int H, int C, int L, int Lq, int P, float *grad_value, float *grad_loc,
                         float *grad_attn, const int64_t *shapes_host, const int64_t *lsi_host,
                         void *workspace, size_t workspace_bytes, const void *plan, size_t plan_bytes,
                         void *state, size_t state_bytes, int hints, void *stream, int want);
int boxattn_bwd_part_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                          const float *loc, const float *attn, const uint16_t *grad_out, int B,
                          int S, int H, int C, int L, int Lq, int P, uint16_t *grad_value,
                          float *grad_loc, float *grad_attn, const int64_t *shapes_host,
                          const int64_t *lsi_host, void *workspace, size_t workspace_bytes,
                          const void *plan, size_t plan_bytes, void *state, size_t state_bytes, int hints,
                          void *stream, int want);
int boxattn_bwd_part_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                         const float *loc, const float *attn, const uint16_t *grad_out, int B,
                         int S, int H, int C, int L, int Lq, int P, uint16_t *grad_value,
                         float *grad_loc, float *grad_attn, const int64_t *shapes_host,
                         const int64_t *lsi_host, void *workspace, size_t workspace_bytes,
                         const void *plan, size_t plan_bytes, void *state, size_t state_bytes, int hints,
                         void *stream, int want);
int boxattn_bwd_part_f64(const double *value, const int64_t *shapes, const int64_t *lsi,
                         const double *loc, const double *attn, const double *grad_out, int B,
                         int S, int H, int C, int L, int Lq, int P, double *grad_value,
                         double *grad_loc, double *grad_attn, void *stream, int want);
int instattn_bwd_part_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                          const float *loc, const float *spatial_w, const float *level_w,
                          const float *grad_out, const float *grad_mask, int B, int S, int H, int C,
                          int L, int Lq, int P, float *grad_value, float *grad_loc,
                          float *grad_spatial_w, float *grad_level_w, const int64_t *shapes_host,
                          const int64_t *lsi_host, void *workspace, size_t workspace_bytes,
                          const void *plan, size_t plan_bytes, void *state, size_t state_bytes, int hints,
                          void *stream, int want);
int instattn_bwd_part_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                           const float *loc, const float *spatial_w, const float *level_w,
                           const uint16_t *grad_out, const uint16_t *grad_mask, int B, int S, int H,
                           int C, int L, int Lq, int P, uint16_t *grad_value, float *grad_loc,
                           float *grad_spatial_w, float *grad_level_w, const int64_t *shapes_host,
                           const int64_t *lsi_host, void *workspace, size_t workspace_bytes,
                           const void *plan, size_t plan_bytes, void *state, size_t state_bytes, int hints,
                           void *stream, int want);
int instattn_bwd_part_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                          const float *loc, const float *spatial_w, const float *level_w,
                          const uint16_t *grad_out, const uint16_t *grad_mask, int B, int S, int H,
                          int C, int L, int Lq, int P, uint16_t *grad_value, float *grad_loc,
                          float *grad_spatial_w, float *grad_level_w, const int64_t *shapes_host,
                          const int64_t *lsi_host, void *workspace, size_t workspace_bytes,
                          const void *plan, size_t plan_bytes, void *state, size_t state_bytes, int hints,
                          void *stream, int want);
int instattn_bwd_part_f64(const double *value, const int64_t *shapes, const int64_t *lsi,
                          const double *loc, const double *spatial_w, const double *level_w,
                          const double *grad_out, const double *grad_mask, int B, int S, int H,
                          int C, int L, int Lq, int P, double *grad_value, double *grad_loc,
                          double *grad_spatial_w, double *grad_level_w, void *stream, int want);

/*
 * ---- reference windows + box offsets -> sampling grid (opt-in) ---------------
 * Everything of the modules' `_where_to_attend` after the box-offset projection
 * (e2edet/module/box_attention.py:63-81 BoxAttention / InstanceAttention, :304-338
 * Box3dAttention) as one kernel each way:
 *     box   = ref[:4] + offsets[:4] / 8 * (w, h, w, h)_ref
 *     theta = none (angle_mode 0) | (ref[4] + offsets[4] / 16) * 2 pi (1) | ref[4] (2)
 *     grid[b,q,h,l,p,:] = (c + R(theta) (kernel_idx[p] * relu(size))) * valid_ratios[b,l,:]
 *   ref          (B, Lq, ref_dim) or, ref_per_head != 0, (B, Lq, H, ref_dim); float32,
 *                ref_dim >= 4 (>= 5 with an angle); columns beyond the angle are ignored
 *   offsets      (B, Lq, H, L, V) float32, V = 4, or 5 for angle_mode 1
 *   kernel_idx   (P, 2) float32, the module's `kernel_indices` buffer
 *   valid_ratios (B, L, 2) float32 or NULL (`v_valid_ratios`, (B,1,1,L,1,2) in the reference)
 *   grid / grad_grid (B, Lq, H, L, P, 2) float32 -- the `sampling_locations` of the operator
 *   grad_offsets (B, Lq, H, L, V) float32, fully written
 *   grad_ref_rows (B, Lq, H, L, 5) float32 or NULL: per-(head, level) gradient of
 *                (cx, cy, w, h, angle)_ref; the caller sums it over L (and H) if it needs
 *                the gradient of the reference windows
 */
int boxattn_grid_fwd_f32(const float *ref, int ref_dim, int ref_per_head, const float *offsets,
                         int V, int angle_mode, const float *kernel_idx,
                         const float *valid_ratios, int B, int Lq, int H, int L, int P,
                         float *grid, void *stream);
int boxattn_grid_bwd_f32(const float *ref, int ref_dim, int ref_per_head, const float *offsets,
                         int V, int angle_mode, const float *kernel_idx,
                         const float *valid_ratios, const float *grad_grid, int B, int Lq, int H,
                         int L, int P, float *grad_offsets, float *grad_ref_rows, void *stream);

/*
 * ---- training forward: forward + backward plan ----------------------------------------------
 * Same as the plain forward, and additionally (when the binned backward applies) the count pass and
 * the scans of the backward -- they only depend on the sampling locations -- ride in the forward
 * kernel's launch as extra workgroups and leave the backward's PLAN in `plan` (boxattn_plan_bytes()
 * bytes, 256-byte aligned, contents ignored on entry: per bin workgroup and block the first record
 * slot, the work-item list; 1.4 MB at BoxeR-R50 encoder shapes).  It must stay untouched until the
 * matching *_bwd_ws_* call.  *plan_built is 1 if a plan was built, 0 if the call was just a plain
 * forward (shape not eligible / buffer too small / NULL).
 * state / state_bytes: NULL / 0, or a device buffer of at least boxattn_state_bytes(dimensions, level tables) bytes,
 * 8-byte aligned, that the caller ZEROED ONCE and keeps for the calls it issues on ONE stream with ONE set of dimensions
 * and level shapes (ABI 8; until ABI 7 one buffer served every shape of its stream): counters, the riders' hand-off
 * tickets (every call leaves them zero), and the record ranges of the backward's one-pass fill (*_bwd_ws_*: for the
 * shapes that fill takes, the training forward carries nothing of the backward and builds no plan -- *plan_built = 0).
 * A non-NULL state that is misaligned or too small is an error (hipErrorInvalidValue), not "no state".  The library
 * remembers (host side) which shape a buffer served last and zeroes a buffer that turns up with another one.
 * Without a state the tickets live in `plan` and a zero-fill launch (~5 us) precedes the forward kernel.
 * The FIRST 1 KiB of the state buffer holds 64 pairs of uint64 counters (then 64 bytes of counters of the one-pass
 * fill: {calls, blocks recomputed because they outgrew their range}; the tickets follow)
 * that the window-staged forward of the encoder case only ever ADDS to: {sample points it had to fetch from
 * global memory because their footprint missed the staged window, sample points inside the window test}.  A
 * caller may read them whenever it likes (e.g. an asynchronous copy after a call; deltas between two reads; a
 * caller that wants them per shape keeps one state buffer per shape and stream, as boxer_amd.ops does)
 * and, when most points miss -- sampling locations that are not local to their query, e.g. uniformly random
 * ones -- pass BOXATTN_HINT_NOT_LOCAL in `hints` of its next calls: forward and point gradients then run on
 * the row-gather kernels (same results; measured 14.5 against 12.8 Gpts/s on uniformly random locations,
 * 17 against 25 on BoxeR's).  boxer_amd.ops does exactly that.
 */
#define BOXATTN_HINT_NOT_LOCAL 1
/* The state buffer passed with this call was zeroed by the caller since its last call (typically: a newly allocated
 * one, possibly at an address a released buffer had): the library drops what it remembers (host side) of that address,
 * so that the backward's first call on it runs the two-pass passes (and plans the ranges) instead of recomputing every
 * block of a state it believes planned.  Speed only: a zeroed state gives the same results either way. */
#define BOXATTN_HINT_FRESH_STATE 2
size_t boxattn_state_bytes(int B, int S, int H, int C, int L, int Lq, int P, const int64_t *shapes_host,
                           const int64_t *lsi_host);
size_t boxattn_plan_bytes(int is_16bit, int B, int S, int H, int C, int L, int Lq, int P,
                          const int64_t *shapes_host, const int64_t *lsi_host);
int boxattn_fwd_train_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                          const float *loc, const float *attn, int B, int S, int H, int C, int L,
                          int Lq, int P, float *out, const int64_t *shapes_host,
                          const int64_t *lsi_host, void *plan, size_t plan_bytes, void *state,
                          size_t state_bytes, int hints, int *plan_built, void *stream);
int boxattn_fwd_train_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                           const float *loc, const float *attn, int B, int S, int H, int C, int L,
                           int Lq, int P, uint16_t *out, const int64_t *shapes_host,
                           const int64_t *lsi_host, void *plan, size_t plan_bytes, void *state,
                           size_t state_bytes, int hints, int *plan_built, void *stream);
int boxattn_fwd_train_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                          const float *loc, const float *attn, int B, int S, int H, int C, int L,
                          int Lq, int P, uint16_t *out, const int64_t *shapes_host,
                          const int64_t *lsi_host, void *plan, size_t plan_bytes, void *state,
                          size_t state_bytes, int hints, int *plan_built, void *stream);
int instattn_fwd_train_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                           const float *loc, const float *spatial_w, const float *level_w, int B,
                           int S, int H, int C, int L, int Lq, int P, float *out, float *mask_out,
                           const int64_t *shapes_host, const int64_t *lsi_host, void *plan,
                           size_t plan_bytes, void *state, size_t state_bytes, int hints, int *plan_built,
                           void *stream);
int instattn_fwd_train_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                            const float *loc, const float *spatial_w, const float *level_w, int B,
                            int S, int H, int C, int L, int Lq, int P, uint16_t *out,
                            uint16_t *mask_out, const int64_t *shapes_host,
                            const int64_t *lsi_host, void *plan, size_t plan_bytes, void *state,
                            size_t state_bytes, int hints, int *plan_built, void *stream);
int instattn_fwd_train_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                           const float *loc, const float *spatial_w, const float *level_w, int B,
                           int S, int H, int C, int L, int Lq, int P, uint16_t *out,
                           uint16_t *mask_out, const int64_t *shapes_host,
                           const int64_t *lsi_host, void *plan, size_t plan_bytes, void *state,
                           size_t state_bytes, int hints, int *plan_built, void *stream);

/*
 * Kernel-variant override for tests and A/B benchmarks (process-global, not thread-safe):
 *   0 = automatic choice (default), 1 = force the generic kernels (any C),
 *   2 = first-generation fast kernels with fp atomics (error if the shape does not qualify;
 *       never the binned backward),
 *   3 = like 0, but an error if the binned backward is not eligible.
 * Returns the previous value.
 */
int boxattn_set_variant(int variant);

/*
 * ---- pointwise work around the operator (opt-in, beyond the reference's native module) ------
 * The modules' softmax over the L*P attention logits of every (query, head) and the zeroing of
 * padded value rows (reference e2edet/module/box_attention.py:222-231), as single passes:
 *   boxattn_softmax_fwd_*: logits (rows, n) float32 / bfloat16 / float16 -> attn (rows, n) float32, n <= 64
 *   boxattn_softmax_bwd_*: grad_logits = attn * (grad_attn - sum_j attn_j grad_attn_j), written
 *                          in the logits' type
 *   boxattn_value_prep_*:  value (rows, d) float32 / bfloat16 -> bfloat16 with the rows whose mask
 *                          byte is non-zero set to 0 (mask may be NULL); d % 8 == 0;
 *                          _f32_f16 / _f16: float32 / float16 -> float16 likewise
 */
int boxattn_softmax_fwd_f32(const float *logits, long long rows, int n, float *attn, void *stream);
int boxattn_softmax_fwd_bf16(const uint16_t *logits, long long rows, int n, float *attn,
                             void *stream);
int boxattn_softmax_fwd_f16(const uint16_t *logits, long long rows, int n, float *attn,
                            void *stream);
int boxattn_softmax_bwd_f32(const float *attn, const float *grad_attn, long long rows, int n,
                            float *grad_logits, void *stream);
int boxattn_softmax_bwd_bf16(const float *attn, const float *grad_attn, long long rows, int n,
                             uint16_t *grad_logits, void *stream);
int boxattn_softmax_bwd_f16(const float *attn, const float *grad_attn, long long rows, int n,
                            uint16_t *grad_logits, void *stream);
int boxattn_value_prep_f32(const float *value, const unsigned char *mask, long long rows, int d,
                           uint16_t *out, void *stream);
int boxattn_value_prep_bf16(const uint16_t *value, const unsigned char *mask, long long rows, int d,
                            uint16_t *out, void *stream);
int boxattn_value_prep_f32_f16(const float *value, const unsigned char *mask, long long rows, int d,
                               uint16_t *out, void *stream);
int boxattn_value_prep_f16(const uint16_t *value, const unsigned char *mask, long long rows, int d,
                           uint16_t *out, void *stream);

/*
 * Instance attention: the two weight tensors the instattn_* entry points take, from the 2x2 logits per level the
 * module predicts (reference e2edet/module/box_attention.py:100-121: two repeat_interleave and two softmaxes
 * over the expanded tensor), one pass each way.  Per row (batch, query, head): logits z[l][i][j], l < L, i, j in
 * {0, 1}; m = k / 2; point (l, y, x) lies in cell c = (l, y >= m, x >= m).  With a = softmax of z over the 4 L
 * cells of the row and t[l][i][j] = softmax of z[.][i][j] over the levels:
 *   instattn_weights_fwd_*: logits (rows, L, 2, 2) float32 / bfloat16 / float16 ->
 *                           spatial_w[l][y][x] = a[c] / m^2 and, unless level_w is NULL, level_w[l][y][x] = t[c],
 *                           each (rows, L, k, k) float32; arithmetic in float32.
 *   instattn_weights_bwd_*: grad_logits[c] = a[c] / m^2 (Gs[c] - sum_c' a[c'] Gs[c'])
 *                                          + t[c] (Gt[c] - sum_l' t[l'][i][j] Gt[l'][i][j]),
 *                           Gs / Gt = the sums of grad_spatial_w / grad_level_w over the m^2 points of a cell;
 *                           written in the logits' type.  Reads the logits and the two gradients only (a and t are
 *                           recomputed); a NULL gradient counts as zeros.  No atomics: bitwise reproducible.
 * k even, 2 <= k <= 32; 1 <= L <= 16; rows >= 0 (0: nothing is launched); anything else is hipErrorInvalidValue,
 * and so is a (rows, L, k, k) pointer that is not 16-byte aligned.  The logits need no alignment.
 */
int instattn_weights_fwd_f32(const float *logits, long long rows, int L, int k, float *spatial_w,
                             float *level_w, void *stream);
int instattn_weights_fwd_bf16(const uint16_t *logits, long long rows, int L, int k, float *spatial_w,
                              float *level_w, void *stream);
int instattn_weights_fwd_f16(const uint16_t *logits, long long rows, int L, int k, float *spatial_w,
                             float *level_w, void *stream);
int instattn_weights_bwd_f32(const float *logits, const float *grad_spatial_w, const float *grad_level_w,
                             long long rows, int L, int k, float *grad_logits, void *stream);
int instattn_weights_bwd_bf16(const uint16_t *logits, const float *grad_spatial_w,
                              const float *grad_level_w, long long rows, int L, int k,
                              uint16_t *grad_logits, void *stream);
int instattn_weights_bwd_f16(const uint16_t *logits, const float *grad_spatial_w,
                             const float *grad_level_w, long long rows, int L, int k,
                             uint16_t *grad_logits, void *stream);

/*
 * Instance attention at INFERENCE straight from what the module predicts per (batch, query, head, level) -- one box and
 * 2x2 logits -- in one launch: what boxattn_grid_fwd_f32 (angle_mode 0, V = 4), instattn_weights_fwd_f32 and
 * instattn_fwd_* compute in three, without the (B,Lq,H,L,k*k,2) sampling grid and the (B,Lq,H,L,k,k) weight tensors
 * in between.  Locations and weights are made by the device functions those kernels use, in their
 * operation order, in float32.  ref / ref_dim / ref_per_head / offsets / kernel_idx / valid_ratios as
 * boxattn_grid_fwd_f32, logits as instattn_weights_fwd_f32; P = k * k points a level, row-major over (y, x).
 *   mask_out given: out and mask_out of instattn_fwd_*;
 *   mask_out NULL:  out of boxattn_fwd_* with the spatial weights (the module with `inferencing` set).
 * Forward only (the box and logit gradients: instattn_bwd_boxes_* below).  One wave-per-pair kernel and no other
 * behind these entries: dimensions for which instattn_fwd_boxes_ok answers 0 -- with `aligned` what value, out and
 * mask_out are aligned to -- are hipErrorInvalidValue, and so is a NULL among value, shapes, lsi, ref, offsets,
 * kernel_idx, logits, out; nothing is launched then.  No queries: nothing is written; no pixels: the outputs are
 * zero-filled.  No atomics (bitwise reproducible), no host reads, no allocation: capturable.  Profile slot 0.
 */
int instattn_fwd_boxes_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                           const float *ref, int ref_dim, int ref_per_head, const float *offsets,
                           const float *kernel_idx, const float *valid_ratios, const float *logits,
                           int B, int S, int H, int C, int L, int Lq, int k, float *out, float *mask_out,
                           void *stream);
int instattn_fwd_boxes_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                            const float *ref, int ref_dim, int ref_per_head, const float *offsets,
                            const float *kernel_idx, const float *valid_ratios, const float *logits,
                            int B, int S, int H, int C, int L, int Lq, int k, uint16_t *out,
                            uint16_t *mask_out, void *stream);
int instattn_fwd_boxes_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                           const float *ref, int ref_dim, int ref_per_head, const float *offsets,
                           const float *kernel_idx, const float *valid_ratios, const float *logits,
                           int B, int S, int H, int C, int L, int Lq, int k, uint16_t *out,
                           uint16_t *mask_out, void *stream);
/* 1 where the entry points above have their kernel: boxattn_fwd_route answers BOXATTN_FWD_WIDE for the instance flavour
 * of these dimensions with P = k * k (that covers boxattn_set_variant, the alignment and value < 2 GiB), k is even,
 * 2 <= k <= 32, and L <= 16; else 0.  elem_bytes 2 / 4; aligned as boxattn_fwd_route.  The same answer with and
 * without mask_out; option key 22 is not read.  Pure host code: no device call; the entry points call the same
 * function. */
int instattn_fwd_boxes_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int k);

/*
 * BOX attention at INFERENCE straight from what BoxAttention / Box3dAttention predict per (batch, query, head) -- L
 * boxes and L*P logits -- in one launch: what boxattn_grid_fwd_f32, boxattn_softmax_fwd_f32 and boxattn_fwd_* compute
 * in three, without the (B,Lq,H,L,P,2) sampling grid and the (B,Lq,H,L*P) weights in between.  ref /
 * ref_dim / ref_per_head / offsets / V / angle_mode / kernel_idx / valid_ratios as boxattn_grid_fwd_f32 (all three
 * angle modes); logits (B,Lq,H,L*P) float32; out as boxattn_fwd_*.  The locations are made by the grid kernel's device
 * functions in its operation order; the weights are exp(z - max) * (1 / sum) in float32, summed over a lane group.
 * Forward only.  One row-gather kernel and no other behind these entries: dimensions for which boxattn_fwd_boxes_ok
 * answers 0 -- with `aligned` what value and out are aligned to --, ref_dim < 4 (< 5 with an angle), V other than 4
 * (5 for angle_mode 1), and a NULL among value, shapes, lsi, ref, offsets, kernel_idx, logits, out are
 * hipErrorInvalidValue; nothing is launched then.  No queries: nothing is written; no pixels: out is zero-filled.
 * No atomics (bitwise reproducible), no host reads, no allocation: capturable, on the one stream.  Profile slot 0.
 */
int boxattn_fwd_boxes_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                          const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                          int angle_mode, const float *kernel_idx, const float *valid_ratios,
                          const float *logits, int B, int S, int H, int C, int L, int Lq, int P, float *out,
                          void *stream);
int boxattn_fwd_boxes_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                           const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                           int angle_mode, const float *kernel_idx, const float *valid_ratios,
                           const float *logits, int B, int S, int H, int C, int L, int Lq, int P, uint16_t *out,
                           void *stream);
int boxattn_fwd_boxes_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                          const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                          int angle_mode, const float *kernel_idx, const float *valid_ratios,
                          const float *logits, int B, int S, int H, int C, int L, int Lq, int P, uint16_t *out,
                          void *stream);
/* 1 where the entry points above have their kernel: boxattn_fwd_route answers BOXATTN_FWD_GATHER for the box flavour of
 * these dimensions without host tables (that covers boxattn_set_variant, option key 22, the alignment and value <
 * 2 GiB), L <= 16 and L*P <= 64 (the limit of the softmax kernels; P itself is free); else 0.  elem_bytes 2 / 4;
 * aligned as boxattn_fwd_route.  Pure host code: no device call; the entry points call the same function. */
int boxattn_fwd_boxes_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P);

/*
 * The same call for the ENCODER case (one query per pixel, C = 32, P = 4, L <= 4) on the WINDOW-STAGED forward
 * (boxattn_fwd_hl_*'s kernels: an 8x8 query tile's value windows in LDS; 16-bit storage on the matrix cores), with the
 * host copies of the level tables (shapes_host / lsi_host as boxattn_fwd_hl_*; read during the call, never the device
 * copies).  Each quad of lanes makes its query's 4 L locations and weights in registers while the windows are fetched:
 * locations as above (the grid kernel's, bit for bit); weights exp(z - max) * (1 / sum) in float32 -- maximum and sum
 * over the lane's own L values in level order, then over the quad.  One window-staged kernel per storage type and
 * no other behind these entries: dimensions for which boxattn_fwd_boxes_hl_ok answers 0 (NULL host tables among
 * them), and everything boxattn_fwd_boxes_* refuses, are hipErrorInvalidValue; nothing is launched then.  The checks
 * run in that entry's order.  No riders, no state, no atomics (bitwise reproducible), no host reads beyond the two
 * tables, no allocation: capturable, on the one stream.  Profile slot 0.
 */
int boxattn_fwd_boxes_hl_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                             const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                             int angle_mode, const float *kernel_idx, const float *valid_ratios,
                             const float *logits, int B, int S, int H, int C, int L, int Lq, int P, float *out,
                             const int64_t *shapes_host, const int64_t *lsi_host, void *stream);
int boxattn_fwd_boxes_hl_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                              const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                              int angle_mode, const float *kernel_idx, const float *valid_ratios,
                              const float *logits, int B, int S, int H, int C, int L, int Lq, int P, uint16_t *out,
                              const int64_t *shapes_host, const int64_t *lsi_host, void *stream);
int boxattn_fwd_boxes_hl_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                             const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                             int angle_mode, const float *kernel_idx, const float *valid_ratios,
                             const float *logits, int B, int S, int H, int C, int L, int Lq, int P, uint16_t *out,
                             const int64_t *shapes_host, const int64_t *lsi_host, void *stream);
/* 1 where the entry points above have their kernel: exactly where boxattn_fwd_route answers BOXATTN_FWD_STAGED for the
 * box flavour of these dimensions WITH these host tables (Lq = S, C = 32, P = 4, L <= 4, the tables consistent with S,
 * value and out aligned to 16 bytes, value < 2 GiB, boxattn_set_variant 0 / 3 and option key 11 not 1); else 0, also
 * without host tables.  elem_bytes 2 / 4; aligned as boxattn_fwd_route.  Pure host code: no device call; the entry
 * points call the same function. */
int boxattn_fwd_boxes_hl_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P,
                            const int64_t *shapes_host, const int64_t *lsi_host);

/*
 * Instance attention's TRAINING step from the same operands: the gradients the module needs per (batch, query, head,
 * level) -- of the box offsets, of the reference window (rows, summed by the caller as after boxattn_grid_bwd_f32) and
 * of the 2x2 logits -- in one launch: what instattn_bwd_part_* (want = BOXATTN_WANT_POINTS), boxattn_grid_bwd_f32
 * (angle_mode 0, V = 4) and instattn_weights_bwd_f32 compute in three, without reading the sampling grid and the two
 * weight tensors and without writing grad_loc / grad_spatial_w / grad_level_w in between.  Locations
 * and weights are recomputed by the device functions of the forward above; everything is float32 except value and the
 * upstream gradients, which are in the storage type.  grad_value is NOT computed here.
 *   grad_out  (B,Lq,H,C), grad_mask (B,Lq,k*k,H,C) or NULL
 *   grad_mask given: the gradients of instattn_fwd_* (both outputs took part in the loss);
 *   grad_mask NULL:  those of boxattn_fwd_* with the spatial weights: grad_logits has the spatial term only.
 *   grad_offsets (B,Lq,H,L,4), grad_ref_rows (B,Lq,H,L,5) or NULL, grad_logits (B,Lq,H,L,2,2): float32, every element
 *   written.
 * One wave-per-pair kernel and no other behind these entries: dimensions for which instattn_bwd_boxes_ok answers 0 --
 * with `aligned` what value, grad_out and grad_mask are aligned to -- are hipErrorInvalidValue, and so are ref_dim < 4
 * and a NULL among value, shapes, lsi, ref, offsets, kernel_idx, logits, grad_out, grad_offsets, grad_logits; nothing
 * is launched then.  No queries: nothing is written; no pixels: the outputs are zero-filled.  No atomics and a fixed
 * summation order (bitwise reproducible), no host reads, no allocation: capturable.  Profile slot 1.
 */
int instattn_bwd_boxes_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                           const float *ref, int ref_dim, int ref_per_head, const float *offsets,
                           const float *kernel_idx, const float *valid_ratios, const float *logits,
                           const float *grad_out, const float *grad_mask,
                           int B, int S, int H, int C, int L, int Lq, int k,
                           float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream);
int instattn_bwd_boxes_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                            const float *ref, int ref_dim, int ref_per_head, const float *offsets,
                            const float *kernel_idx, const float *valid_ratios, const float *logits,
                            const uint16_t *grad_out, const uint16_t *grad_mask,
                            int B, int S, int H, int C, int L, int Lq, int k,
                            float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream);
int instattn_bwd_boxes_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                           const float *ref, int ref_dim, int ref_per_head, const float *offsets,
                           const float *kernel_idx, const float *valid_ratios, const float *logits,
                           const uint16_t *grad_out, const uint16_t *grad_mask,
                           int B, int S, int H, int C, int L, int Lq, int k,
                           float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream);
/* 1 where the entry points above have their kernel: exactly where instattn_fwd_boxes_ok answers 1 (the same host
 * function), `aligned` now speaking of value, grad_out and grad_mask.  Pure host code: no device call. */
int instattn_bwd_boxes_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int k);

/*
 * Box attention's TRAINING step from the operands of boxattn_fwd_boxes_*: the gradients BoxAttention / Box3dAttention
 * need per (batch, query, head) -- of the box offsets, of the reference window (rows, summed by the caller as after
 * boxattn_grid_bwd_f32) and of the L*P logits -- in one launch: what boxattn_bwd_part_* (want = BOXATTN_WANT_POINTS),
 * boxattn_grid_bwd_f32 (all three angle modes) and boxattn_softmax_bwd_f32 compute in three, without reading a sampling
 * grid or a weights tensor and without writing grad_loc / grad_attn in between.  Locations and weights
 * are recomputed by the device functions of the forward above, in its operation order; everything is float32 except
 * value and the upstream gradient, which are in the storage type.  grad_value is NOT computed here.
 *   grad_out  (B,Lq,H,C)
 *   grad_offsets (B,Lq,H,L,V), grad_ref_rows (B,Lq,H,L,5) or NULL, grad_logits (B,Lq,H,L*P): float32, every element
 *   written; element 4 of a grad_ref_rows row as boxattn_grid_bwd_f32 writes it in each angle mode.
 * One row-gather kernel and no other behind these entries: dimensions for which boxattn_bwd_boxes_ok answers 0 -- with
 * `aligned` what value and grad_out are aligned to --, ref_dim < 4 (< 5 with an angle), V other than 4 (5 for
 * angle_mode 1), and a NULL among value, shapes, lsi, ref, offsets, kernel_idx, logits, grad_out, grad_offsets,
 * grad_logits are hipErrorInvalidValue; nothing is launched then.  No queries: nothing is written; no pixels: the
 * outputs are zero-filled.  No atomics and a fixed summation order (bitwise reproducible), no host reads, no
 * allocation: capturable, on the one stream.  Profile slot 1.
 */
int boxattn_bwd_boxes_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                          const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                          int angle_mode, const float *kernel_idx, const float *valid_ratios,
                          const float *logits, const float *grad_out,
                          int B, int S, int H, int C, int L, int Lq, int P,
                          float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream);
int boxattn_bwd_boxes_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                           const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                           int angle_mode, const float *kernel_idx, const float *valid_ratios,
                           const float *logits, const uint16_t *grad_out,
                           int B, int S, int H, int C, int L, int Lq, int P,
                           float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream);
int boxattn_bwd_boxes_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                          const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                          int angle_mode, const float *kernel_idx, const float *valid_ratios,
                          const float *logits, const uint16_t *grad_out,
                          int B, int S, int H, int C, int L, int Lq, int P,
                          float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream);
/* 1 where the entry points above have their kernel: exactly where boxattn_fwd_boxes_ok answers 1 (the same host
 * function), `aligned` now speaking of value and grad_out.  Pure host code: no device call. */
int boxattn_bwd_boxes_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P);

/*
 * The same step for the ENCODER case (one query per pixel, C = 32, P = 4, L <= 4) on the WINDOW-STAGED point-gradient
 * kernels (boxattn_bwd_part_*'s encoder route: an 8x8 query tile's value windows in LDS once, a quad of lanes per
 * (query, head) pair), with the host copies of the level tables (shapes_host / lsi_host as boxattn_fwd_boxes_hl_*; read
 * during the call, never the device copies): the operands and outputs of boxattn_bwd_boxes_*, then the two tables.
 * Locations are the grid kernel's and weights boxattn_fwd_boxes_hl_*'s, bit for bit; grad_loc and grad_attn stay on
 * the chip: grad_logits = a (g - sum a g), the sum over the lane's L levels in level order, then over the quad; a
 * level's box gradient from its four points in point order, as boxattn_grid_bwd_f32 (all three angle modes, valid
 * ratios).  The results agree with boxattn_bwd_boxes_* up to the order of the float32 sums.
 *   grad_logits additionally aligned to 16 bytes (a level's four values leave as one store).
 * One window-staged kernel per storage type and no other behind these entries: dimensions for which
 * boxattn_bwd_boxes_hl_ok answers 0 (NULL host tables among them) -- with `aligned` what value and grad_out are aligned
 * to --, and everything boxattn_bwd_boxes_* refuses, are hipErrorInvalidValue; nothing is launched then.  The checks
 * run in that entry's order.  No queries: nothing is written.  No riders, no state, no atomics and a fixed summation
 * order (bitwise reproducible), no host reads beyond the two tables, no allocation: capturable, on the one stream.
 * Profile slot 1.
 */
int boxattn_bwd_boxes_hl_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                             const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                             int angle_mode, const float *kernel_idx, const float *valid_ratios,
                             const float *logits, const float *grad_out,
                             int B, int S, int H, int C, int L, int Lq, int P,
                             float *grad_offsets, float *grad_ref_rows, float *grad_logits,
                             const int64_t *shapes_host, const int64_t *lsi_host, void *stream);
int boxattn_bwd_boxes_hl_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                              const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                              int angle_mode, const float *kernel_idx, const float *valid_ratios,
                              const float *logits, const uint16_t *grad_out,
                              int B, int S, int H, int C, int L, int Lq, int P,
                              float *grad_offsets, float *grad_ref_rows, float *grad_logits,
                              const int64_t *shapes_host, const int64_t *lsi_host, void *stream);
int boxattn_bwd_boxes_hl_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                             const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                             int angle_mode, const float *kernel_idx, const float *valid_ratios,
                             const float *logits, const uint16_t *grad_out,
                             int B, int S, int H, int C, int L, int Lq, int P,
                             float *grad_offsets, float *grad_ref_rows, float *grad_logits,
                             const int64_t *shapes_host, const int64_t *lsi_host, void *stream);
/* 1 where the entry points above have their kernel: exactly where boxattn_fwd_boxes_hl_ok answers 1 (the same host
 * function), `aligned` now speaking of value and grad_out.  Pure host code: no device call. */
int boxattn_bwd_boxes_hl_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P,
                            const int64_t *shapes_host, const int64_t *lsi_host);

/*
 * The same step with grad_value in the SAME launch: the operands of boxattn_bwd_boxes_*, then
 *   want         BOXATTN_WANT_VALUE (1), BOXATTN_WANT_POINTS (2) or both (3); anything else is hipErrorInvalidValue.
 *                POINTS alone is boxattn_bwd_boxes_* exactly: grad_value, workspace and workspace_bytes are not read.
 *                VALUE alone: grad_offsets, grad_ref_rows and grad_logits are neither checked nor written.
 *   grad_value   (B,S,H,C) in the storage type, every element written (needed with VALUE)
 *   workspace    16-bit storage: boxattn_bwd_boxes_value_workspace_bytes() bytes, 16-byte aligned -- the float32
 *                accumulator, cast into grad_value by one pass behind the kernel (grad_value 8-byte aligned then);
 *                float32 storage accumulates into grad_value itself and reads neither workspace argument
 * The kernel of boxattn_bwd_boxes_* in a flavour that, where it walks a level's four corner rows, also adds
 * weight * corner weight * grad_out row into the accumulator with one hardware float32 atomic an element -- only at
 * corners inside the map, so a non-finite grad_out row reaches no row its points do not touch.  The entry zero-fills
 * the accumulator itself.  The order of the adds is not fixed: grad_value from this entry is NOT bitwise reproducible;
 * grad_offsets, grad_ref_rows and grad_logits are bit for bit those of boxattn_bwd_boxes_* and still are.  Meant for
 * few queries against the map (decoder cross-attention); DESIGN.md 4.1 has the measurements.
 * Refusals as boxattn_bwd_boxes_* (hipErrorInvalidValue, nothing launched), and with VALUE: a NULL grad_value, and for
 * 16-bit storage a workspace that is NULL, smaller than the query says or not 16-byte aligned.  No queries: grad_value
 * is zero-filled; no pixels: the three other gradients are.  No host reads, no allocation: capturable, on the one
 * stream.  Profile slot 1 (the zero-fill and the cast included).
 */
int boxattn_bwd_boxes_value_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                                const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                                int angle_mode, const float *kernel_idx, const float *valid_ratios,
                                const float *logits, const float *grad_out,
                                int B, int S, int H, int C, int L, int Lq, int P,
                                int want, float *grad_value, void *workspace, size_t workspace_bytes,
                                float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream);
int boxattn_bwd_boxes_value_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                                 const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                                 int angle_mode, const float *kernel_idx, const float *valid_ratios,
                                 const float *logits, const uint16_t *grad_out,
                                 int B, int S, int H, int C, int L, int Lq, int P,
                                 int want, uint16_t *grad_value, void *workspace, size_t workspace_bytes,
                                 float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream);
int boxattn_bwd_boxes_value_f16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                                const float *ref, int ref_dim, int ref_per_head, const float *offsets, int V,
                                int angle_mode, const float *kernel_idx, const float *valid_ratios,
                                const float *logits, const uint16_t *grad_out,
                                int B, int S, int H, int C, int L, int Lq, int P,
                                int want, uint16_t *grad_value, void *workspace, size_t workspace_bytes,
                                float *grad_offsets, float *grad_ref_rows, float *grad_logits, void *stream);
/* 1 where the entry points above have their kernel: boxattn_bwd_boxes_ok's function. */
int boxattn_bwd_boxes_value_ok(int elem_bytes, int aligned, int B, int S, int H, int C, int L, int Lq, int P);
/* Bytes of `workspace`: 0 for 4-byte storage, 4 * B * S * H * C for 2-byte storage.  Pure host code. */
size_t boxattn_bwd_boxes_value_workspace_bytes(int elem_bytes, int B, int S, int H, int C);

/*
 * Tuning options for A/B runs (process-wide, relaxed atomics; 0 = default).  Returns the
 * previous value, -1 for an unknown key.  (The key numbers of earlier ABI versions are kept; the keys
 * of kernels that were removed are gone.)
 *  10  binned backward: records per work item (multiple of 64; default: from the number of sample
 *      points, 128 ... 1024).  Set it before boxattn_plan_bytes / boxattn_bwd_workspace_bytes: the
 *      layouts depend on it.
 *  11  window-staged kernels of the encoder case (box attention, 16-bit or float32 storage, Lq == S, C = 32,
 *      2x2 points, <= 4 levels; forward and point gradients): 0 library default (on), 1 off
 *      (row-gather kernels -- the parity cross-check of the two kernel families; faster for uniformly random
 *      sampling locations, which the BOXATTN_HINT_NOT_LOCAL hint selects per call), 2 on
 *  15  binning passes of the backward as riders: 0 default -- the fill pass inside the point-gradient
 *      launch, chunked blocks summed inside the accumulate launch (wherever the riders run -- maps of up to 3 072
 *      blocks per (image, head) -- or the problem has < 65 536 sample points per (image, head); by a combine launch
 *      behind it otherwise); box attention on the matrix-core accumulates fills its bins in ONE pass from the ranges in
 *      the caller's state buffer (*_bwd_ws_*), everything else counts and scans inside the training forward's launch --,
 *      1 off (launches of their own), 2 on with the combine always a launch of its own, 3 on with the combine always
 *      inside, 4 on with the two-pass binning of ABI 7 for everything (count riders in the training forward, plan
 *      hand-over) instead of the one-pass fill
 *  19  float32, 32 channels per head: the grad_value accumulate -- 0 default: the bf16 matrix cores on exact
 *      three-term splits of rows and weights (float32-accurate, 16-byte records; instance attention from
 *      65 536 points per (image, head) slice up), 1: VALU list walk (4-byte records; the parity cross-check),
 *      2: v_mfma_f32_32x32x2_f32 (16-byte records; box attention only, instance attention takes the VALU walk).
 *      Set before boxattn_bwd_workspace_bytes / *_fwd_train_*.
 *  20  where the riders sit in their host kernel's grid: (s_count + 1) | (s_fill + 1) << 4 -- a group of 8
 *      rider workgroups every 2^s groups of 8 workgroups (s = 0: all in front) -- | v << 8: 64 v bin workgroups
 *      (= riders) in all; 0 = defaults (all in front; 256, or one per ~600 (query, slice) pairs -- 256 ... 768 -- for the
 *      one-pass fill at encoder sizes).  Set before boxattn_plan_bytes.
 *  22  box attention with few (query, head) pairs and many points a pair (the mask model at inference: 300 queries,
 *      14 x 14 points on 4 levels) on the wave-per-pair forward kernel: 0 library default (the
 *      kernel where it measured faster than the row-gather kernel), 1 off (row-gather kernel -- the parity
 *      cross-check of the two kernel families), 2 on wherever instance attention takes that family.  Instance
 *      attention does not read it.
 *  23  "inst_acc16": instance attention in 16-bit storage, C = 16 / 32 / 64 -- the grad_value accumulate: 0 library
 *      default (decided by measurement, DESIGN.md 4.2.2: the matrix cores from 235 200 points per (image, head) slice up
 *      -- 300 queries, 14 x 14 points on four levels --, the VALU list walk below), 1 VALU list walk (4-byte
 *      records; the parity cross-check), 2 the matrix cores wherever the shape is eligible (grad_out and grad_mask
 *      below 2 GiB; a grad_mask that is not 16-byte aligned takes the VALU walk).  Box attention and float32 do not
 *      read it.  Set before *_fwd_train_*: a plan made under another setting is not used.
 *  24  "group_records": box attention in 16-bit storage with P = 4 on the matrix-core accumulate -- the records of the
 *      binned backward: 0 library default (decided by measurement per shape class), 1 point records
 *      (16 bytes per sample point and touched block), 2 group records -- one int per (query, level, block), locations and
 *      weights gathered by id in the accumulate kernel -- wherever the shape is eligible (C = 16 / 32 / 64, grad_out and
 *      loc below 2 GiB; a call whose loc or attn is not 16-byte aligned keeps point records).  Instance attention and
 *      float32 do not read it.  Set before boxattn_bwd_workspace_bytes / boxattn_plan_bytes / *_fwd_train_*: the
 *      workspace of an eligible shape is smaller, and its training forward builds no plan.
 *  (ABI 8 removed 12 / 13 -- window margins --, 17 and 21 -- staged forward / staged float32 kernels off: 11 = 1
 *  switches every window-staged kernel off.)
 */
int boxattn_set_option(int key, int value);

/* The kernel families of the forward. */
#define BOXATTN_FWD_GENERIC 0   /* any dimensions, any alignment, float64 */
#define BOXATTN_FWD_FAST    1   /* first-generation fast kernels (boxattn_set_variant(2), or >= 2 GiB of value) */
#define BOXATTN_FWD_GATHER  2   /* row gather: a lane group walks the points of its (query, head) pair */
#define BOXATTN_FWD_WIDE    3   /* wave per pair: the lane groups of one to four waves share a pair's points */
#define BOXATTN_FWD_STAGED  4   /* window-staged (the encoder case; needs the host tables) */
/* Which forward kernel family the library would launch for these dimensions under the current
 * switches (boxattn_set_variant / boxattn_set_option); the very function the forward entry points call.
 * elem_bytes 2 / 4 / 8; instance 0 / 1; aligned != 0: every tensor 16-byte aligned (8: to 8 bytes only, 0: to
 * nothing beyond its elements); shapes_host / lsi_host may be NULL (then never window-staged).  Pure host code:
 * no device call.  < 0: invalid dimensions, or dimensions boxattn_set_variant(2) has no kernel for.
 * (BOXATTN_HINT_NOT_LOCAL of a training forward is a per-call matter: the query answers for a call without it.) */
int boxattn_fwd_route(int elem_bytes, int instance, int aligned, int B, int S, int H, int C, int L, int Lq, int P,
                      const int64_t *shapes_host, const int64_t *lsi_host);
/* The grad_value accumulate kernels of the binned backward. */
#define BOXATTN_ACC_VALU  0     /* VALU list walk over 4-byte records */
#define BOXATTN_ACC_TR    1     /* 16-bit storage on v_mfma_f32_32x32x16_bf16 / _f16 (instance attention: option 23) */
#define BOXATTN_ACC_F32   2     /* float32 on v_mfma_f32_32x32x2_f32 (option 19 = 2) */
#define BOXATTN_ACC_SPLIT 3     /* float32 on the bf16 matrix cores over exact three-term splits */
/* Which accumulate kernel a binned backward of these dimensions runs under the current switches: the very function
 * the launch calls.  elem_bytes 2 / 4; instance 0 / 1.  Pure host code.  < 0: invalid dimensions or elem_bytes (8:
 * float64 has no binned backward).  (Whether a call IS binned -- level tables, alignment, workspace -- and the
 * alignment of grad_mask, which can send a 16-bit instance call to BOXATTN_ACC_VALU, are per-call matters.) */
int boxattn_bwd_accumulate_kind(int elem_bytes, int instance, int B, int S, int H, int C, int L, int Lq, int P);
/* The records of the binned backward. */
#define BOXATTN_REC_POINT 0     /* one record per sample point and touched block */
#define BOXATTN_REC_GROUP 1     /* one 4-byte record per (query, level, block): 16-bit box attention, P = 4 (option 24) */
/* Which records a binned backward of these dimensions writes under the current switches: the very function the launch
 * calls.  Arguments and errors as boxattn_bwd_accumulate_kind.  (The alignment of loc / attn, which can send a call back
 * to BOXATTN_REC_POINT, is a per-call matter.) */
int boxattn_bwd_record_kind(int elem_bytes, int instance, int B, int S, int H, int C, int L, int Lq, int P);
/* Number of boxattn_set_variant / boxattn_set_option calls so far: lets a binding cache the size queries
 * (boxattn_plan_bytes, boxattn_bwd_workspace_bytes: pure functions of their arguments and the switches). */
int boxattn_options_epoch(void);

/*
 * Has no effect; kept for ABI 8.  (It named the device buffer of time-stamp builds of the kernels, which no
 * longer exist.)
 */
void boxattn_set_debug_buffer(float *device_buffer);

/*
 * Kernel timing for benchmarks (process-global, not thread-safe).  Between _begin and _end the
 * library brackets the launches of its main kernels with hipEvents recorded on the launch
 * stream, in BOXATTN_PROFILE_SLOTS slots:
 *   0  forward sampling kernel (training forward: + the count / scan riders of its launch)
 *   1  backward, point gradients (grad_loc / grad_weight; + the fill riders of its launch) -- or the
 *      whole atomic backward kernel when the binned algorithm is not used
 *   2  backward, grad_value accumulate kernel (+ the in-launch combine of chunked blocks)
 *   3  backward, binning passes run as launches of their own (count / scan / fill)
 *   4  backward, combine pass over the partial tiles of split blocks as a launch of its own
 *   5  unused
 * Zero-fills and the bf16 conversion pass are not included.  _end synchronises the events and
 * writes, per slot, the summed duration in milliseconds and the number of launches into the two
 * BOXATTN_PROFILE_SLOTS-element arrays.  At most 4096 launches per slot are kept.
 */
#define BOXATTN_PROFILE_SLOTS 6
int boxattn_profile_begin(void);
int boxattn_profile_end(double *ms_sum, int *launches);

#ifdef __cplusplus
}
#endif
#endif /* BOXATTN_H_ */
