"""autograd Functions with the reference's signatures.

``BoxAttnFunction`` / ``InstanceAttnFunction`` mirror
e2edet/module/ops/box_attention_func.py:9-64 and :67-150 argument for argument:
same positional inputs, same outputs, gradients only for value / sampling locations /
attention weights (``None`` for the rest), ``once_differentiable``, and the same AMP
contract (``custom_fwd(cast_inputs=torch.float32)``: under autocast every floating input
is cast to float32 and the op runs with autocast disabled).

``BoxAttnBF16Function`` / ``InstanceAttnBF16Function`` are the new native-bf16 mode
(BASELINE.json configs[1]): ``value`` and the upstream gradients are bfloat16, locations and
weights stay float32, accumulation is float32.  Same signatures otherwise.
``BoxAttnF16Function`` / ``InstanceAttnF16Function`` are the same mode with IEEE float16 storage
(the ``use_fp16: float16`` trainer setting, ``model.half()`` inference).
"""
import torch
from torch.amp import custom_bwd, custom_fwd
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops
from .ops import _H16


# Whether the Functions' forward already prepares the backward's plan: the count pass and the scans of
# the destination-binned backward ride in the forward kernel's launch (ops.*_forward_train) and leave a
# small plan buffer (boxattn_plan_bytes: 1.4 MB at BoxeR-R50 encoder shapes) that lives until the matching
# backward; the backward then starts with the point-gradient kernel (fill pass riding along) instead of
# with three launches of binning.  On by default: this is the path bench.py times.  Off: the backward
# plans for itself (same results).
PLAN_IN_FORWARD = True


def set_plan_in_forward(flag):
    """-> previous setting."""
    global PLAN_IN_FORWARD
    old, PLAN_IN_FORWARD = PLAN_IN_FORWARD, bool(flag)
    return old


def _box_forward(ctx, value, shapes, lsi, loc, attn, im2col_step):
    """Training forward (also prepares the backward's plan) when asked to (PLAN_IN_FORWARD) and the backward will
    compute grad_value -- the plan only serves that half.  Otherwise the plain forward; it parks a plan (as ever, with
    PLAN_IN_FORWARD off) unless value needs no gradient: then no riders, no plan, nothing parked."""
    need_value = ctx.needs_input_grad[0]
    if PLAN_IN_FORWARD and need_value:
        return ops.box_attn_forward_train(value, shapes, lsi, loc, attn, im2col_step)
    return ops.box_attn_forward(value, shapes, lsi, loc, attn, im2col_step, park=need_value), None


def _inst_forward(ctx, value, shapes, lsi, loc, sw, lw, im2col_step):
    need_value = ctx.needs_input_grad[0]
    if PLAN_IN_FORWARD and need_value:
        return ops.instance_attn_forward_train(value, shapes, lsi, loc, sw, lw, im2col_step)
    return ops.instance_attn_forward(value, shapes, lsi, loc, sw, lw, im2col_step, park=need_value), None


# The backward computes the gradient groups autograd asks for (ops.*_backward `want`: 1 grad_value | 2 the location and
# weight gradients, which share every load and nearly all arithmetic and stay together) and returns None for every
# input that needs no gradient.  (Written out, without helpers: the decoder shapes' steps are host-bound.)
def _box_backward(ctx, grad_output):
    if not grad_output.is_contiguous():
        grad_output = grad_output.contiguous()
    value, shapes, lsi, loc, attn = ctx.saved_tensors
    need_v, _, _, need_l, need_a, _ = ctx.needs_input_grad
    grad_value, grad_loc, grad_attn = ops.box_attn_backward(
        value, shapes, lsi, loc, attn, grad_output, ctx.im2col_step, plan=ctx.plan,
        want=(1 if need_v else 0) | (2 if need_l or need_a else 0))
    ctx.plan = None
    return (grad_value if need_v else None, None, None, grad_loc.to(ctx.loc_dtype) if need_l else None,
            grad_attn.to(ctx.attn_dtype) if need_a else None, None)


def _inst_backward(ctx, grad_output, grad_mask_output):
    if not grad_output.is_contiguous():
        grad_output = grad_output.contiguous()
    if not grad_mask_output.is_contiguous():
        grad_mask_output = grad_mask_output.contiguous()
    value, shapes, lsi, loc, sw, lw = ctx.saved_tensors
    need_v, _, _, need_l, need_s, need_w = ctx.needs_input_grad[:6]
    grad_value, grad_loc, grad_sw, grad_lw = ops.instance_attn_backward(
        value, shapes, lsi, loc, sw, lw, grad_output, grad_mask_output, ctx.im2col_step,
        plan=ctx.plan, want=(1 if need_v else 0) | (2 if need_l or need_s or need_w else 0))
    ctx.plan = None
    return (grad_value if need_v else None, None, None, grad_loc.to(ctx.loc_dtype) if need_l else None,
            grad_sw.to(ctx.w_dtype) if need_s else None, grad_lw.to(ctx.w_dtype) if need_w else None, None, None)


class BoxAttnFunction(Function):
    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations,
                attention_weights, im2col_step):
        ctx.im2col_step = im2col_step
        ctx.loc_dtype, ctx.attn_dtype = sampling_locations.dtype, attention_weights.dtype
        output, ctx.plan = _box_forward(ctx, value, value_spatial_shapes,
                                        value_level_start_index, sampling_locations,
                                        attention_weights, im2col_step)
        ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index,
                              sampling_locations, attention_weights)
        return output

    @staticmethod
    @custom_bwd(device_type="cuda")
    @once_differentiable
    def backward(ctx, grad_output):
        return _box_backward(ctx, grad_output)


class InstanceAttnFunction(Function):
    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations,
                spatial_attention_weights, level_attention_weights, mask_size, im2col_step):
        ctx.im2col_step = im2col_step
        ctx.loc_dtype, ctx.w_dtype = sampling_locations.dtype, spatial_attention_weights.dtype
        (output, mask_output), ctx.plan = _inst_forward(
            ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations,
            spatial_attention_weights, level_attention_weights, im2col_step)
        ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index,
                              sampling_locations, spatial_attention_weights,
                              level_attention_weights)
        b, l, _, c = mask_output.shape
        return output, mask_output.view(b, l, mask_size, mask_size, c)

    @staticmethod
    @custom_bwd(device_type="cuda")
    @once_differentiable
    def backward(ctx, grad_output, grad_mask_output):
        return _inst_backward(ctx, grad_output, grad_mask_output)


def _to_storage_args(storage, value, loc, *weights):
    return (value.to(storage).contiguous(), loc.float().contiguous(),
            *[w.float().contiguous() for w in weights])


# The 16-bit storage modes share one implementation; the concrete Functions below only name their
# storage dtype (bfloat16 or float16), which forward keeps on ctx for the backward.
def _box16_forward(ctx, storage, value, value_spatial_shapes, value_level_start_index,
                   sampling_locations, attention_weights, im2col_step):
    ctx.im2col_step = im2col_step
    ctx.storage = storage
    ctx.loc_dtype, ctx.attn_dtype = sampling_locations.dtype, attention_weights.dtype
    ctx.value_dtype = value.dtype
    value, loc, attn = _to_storage_args(storage, value, sampling_locations, attention_weights)
    output, ctx.plan = _box_forward(ctx, value, value_spatial_shapes,
                                    value_level_start_index, loc, attn, im2col_step)
    ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index, loc, attn)
    return output


def _inst16_forward(ctx, storage, value, value_spatial_shapes, value_level_start_index,
                    sampling_locations, spatial_attention_weights, level_attention_weights,
                    mask_size, im2col_step):
    ctx.im2col_step = im2col_step
    ctx.storage = storage
    ctx.loc_dtype, ctx.w_dtype = sampling_locations.dtype, spatial_attention_weights.dtype
    ctx.value_dtype = value.dtype
    value, loc, sw, lw = _to_storage_args(storage, value, sampling_locations,
                                          spatial_attention_weights, level_attention_weights)
    (output, mask_output), ctx.plan = _inst_forward(
        ctx, value, value_spatial_shapes, value_level_start_index, loc, sw, lw, im2col_step)
    ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index, loc, sw, lw)
    b, l, _, c = mask_output.shape
    return output, mask_output.view(b, l, mask_size, mask_size, c)


class _BoxAttn16Function(Function):
    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        grads = _box_backward(ctx, grad_output.to(ctx.storage))
        return (None if grads[0] is None else grads[0].to(ctx.value_dtype),) + grads[1:]


class _InstanceAttn16Function(Function):
    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output, grad_mask_output):
        grads = _inst_backward(ctx, grad_output.to(ctx.storage), grad_mask_output.to(ctx.storage))
        return (None if grads[0] is None else grads[0].to(ctx.value_dtype),) + grads[1:]


class BoxAttnBF16Function(_BoxAttn16Function):
    """Native-bf16 flavour: output and grad_value are bfloat16, accumulation is float32."""

    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations,
                attention_weights, im2col_step):
        return _box16_forward(ctx, torch.bfloat16, value, value_spatial_shapes, value_level_start_index,
                              sampling_locations, attention_weights, im2col_step)


class InstanceAttnBF16Function(_InstanceAttn16Function):
    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations,
                spatial_attention_weights, level_attention_weights, mask_size, im2col_step):
        return _inst16_forward(ctx, torch.bfloat16, value, value_spatial_shapes, value_level_start_index,
                               sampling_locations, spatial_attention_weights, level_attention_weights,
                               mask_size, im2col_step)


class BoxAttnF16Function(_BoxAttn16Function):
    """Native-fp16 flavour: output and grad_value are IEEE float16, accumulation is float32."""

    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations,
                attention_weights, im2col_step):
        return _box16_forward(ctx, torch.float16, value, value_spatial_shapes, value_level_start_index,
                              sampling_locations, attention_weights, im2col_step)


class InstanceAttnF16Function(_InstanceAttn16Function):
    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations,
                spatial_attention_weights, level_attention_weights, mask_size, im2col_step):
        return _inst16_forward(ctx, torch.float16, value, value_spatial_shapes, value_level_start_index,
                               sampling_locations, spatial_attention_weights, level_attention_weights,
                               mask_size, im2col_step)


class BoxGridFunction(Function):
    """(ref_windows, offsets, kernel_indices, valid_ratios, angle_mode) -> sampling grid
    (B,Lq,H,L,P,2): everything of the modules' ``_where_to_attend`` after the offset projection
    in one kernel each way (``module.fused_grid = True``; see ``ops.box_grid_forward``).
    Gradients for ``offsets`` and, if it requires one, ``ref_windows``."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, ref_windows, offsets, kernel_indices, valid_ratios, angle_mode):
        # (float32 whatever the module's type: a .half() module hands float16 here without autocast)
        ref_windows = ref_windows.float().contiguous()
        offsets = offsets.float().contiguous()
        kernel_indices = kernel_indices.float().contiguous()
        if valid_ratios is not None:
            valid_ratios = valid_ratios.float().contiguous()
        ctx.save_for_backward(ref_windows, offsets, kernel_indices, valid_ratios)
        ctx.angle_mode = angle_mode
        return ops.box_grid_forward(ref_windows, offsets, kernel_indices, valid_ratios, angle_mode)

    @staticmethod
    @once_differentiable
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_grid):
        ref_windows, offsets, kernel_indices, valid_ratios = ctx.saved_tensors
        need_ref = ctx.needs_input_grad[0]
        grad_offsets, rows = ops.box_grid_backward(
            ref_windows, offsets, kernel_indices, valid_ratios, ctx.angle_mode,
            grad_grid.contiguous().float(), need_ref_grad=need_ref)
        grad_ref = None
        if need_ref:
            # rows: d/d(cx, cy, w, h, angle)_ref per (head, level); the windows are shared by
            # the levels and, unless given per head, by the heads
            rows = rows.sum(dim=3) if ref_windows.dim() == 4 else rows.sum(dim=(2, 3))
            grad_ref = torch.zeros_like(ref_windows)
            n = min(5, ref_windows.size(-1))
            grad_ref[..., :n] = rows[..., :n]
        return grad_ref, grad_offsets, None, None, None


class LogitSoftmaxFunction(Function):
    """softmax over the last axis in float32 (``module.fused_pointwise``): one HIP pass each way
    instead of autocast's cast + softmax (+ cast back); see ``ops.softmax_forward``."""

    @staticmethod
    def forward(ctx, logits):
        logits = logits.contiguous()
        attn = ops.softmax_forward(logits)
        ctx.save_for_backward(attn)
        ctx.logits_dtype = logits.dtype
        return attn

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_attn):
        (attn,) = ctx.saved_tensors
        return ops.softmax_backward(attn, grad_attn.contiguous().float(), ctx.logits_dtype)


class InstanceWeightsFunction(Function):
    """(logits (B,Lq,H,L,2,2), kernel_size, need_level) -> (spatial_w, level_w or None), each (B,Lq,H,L,k,k)
    float32: ``InstanceAttention``'s repeat_interleave + two softmaxes as one HIP pass each way
    (``module.fused_pointwise``; see ``ops.instance_weights_forward``).  Only the logits are kept for the
    backward, which recomputes both softmaxes from them; the gradient of an output nothing used arrives as None
    and reaches the kernel as a NULL pointer."""

    @staticmethod
    def forward(ctx, logits, kernel_size, need_level=True):
        ctx.set_materialize_grads(False)
        logits = logits.contiguous()
        ctx.save_for_backward(logits)
        return ops.instance_weights_forward(logits, kernel_size, need_level)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_spatial, grad_level):
        if grad_spatial is None and grad_level is None:
            return None, None, None
        (logits,) = ctx.saved_tensors
        grads = [g if g is None else g.contiguous().float() for g in (grad_spatial, grad_level)]
        return ops.instance_weights_backward(logits, *grads), None, None


class ValueMaskCastFunction(Function):
    """value -> bfloat16 (or ``dtype``: float16) with padded rows zeroed (``ops.value_mask_cast``);
    the gradient is the upstream one with the same rows zeroed, in the input's type."""

    @staticmethod
    def forward(ctx, value, v_mask, dtype=torch.bfloat16):
        ctx.save_for_backward(v_mask)
        ctx.value_dtype = value.dtype
        return ops.value_mask_cast(value.contiguous(), v_mask, dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        (v_mask,) = ctx.saved_tensors
        grad = grad.to(ctx.value_dtype)
        if v_mask is not None:
            grad = grad.masked_fill(v_mask[..., None], 0)
        return grad, None, None


def _ref_grad(ref_windows, rows):
    """(B,Lq,H,L,5) row gradients -> gradient of the reference windows (shared by the levels
    and, unless given per head, by the heads)."""
    rows = rows.sum(dim=3) if ref_windows.dim() == 4 else rows.sum(dim=(2, 3))
    grad_ref = torch.zeros_like(ref_windows)
    n = min(5, ref_windows.size(-1))
    grad_ref[..., :n] = rows[..., :n]
    return grad_ref


# ---- the two training steps from boxes and logits (``module.fused_boxes_train``): what they share -----------------
def _boxes_operands(ctx, value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios,
                    logits):
    """-> the operands of ``ops.*_forward_boxes`` (value in its storage type, the rest detached float32), saved for
    the backward; the caller's types are kept in ``ctx.value_dtype`` / ``ctx.in_dtypes``."""
    storage = value.dtype if value.dtype in _H16 else torch.float32
    ctx.value_dtype = value.dtype
    ctx.in_dtypes = (ref_windows.dtype, offsets.dtype, logits.dtype)
    f32 = lambda t: t.detach().float().contiguous()
    value = value.detach().to(storage).contiguous()
    ref_windows, offsets, kernel_indices, logits = f32(ref_windows), f32(offsets), f32(kernel_indices), f32(logits)
    if valid_ratios is not None:
        valid_ratios = f32(valid_ratios)
    # (the (P, 2) buffer is kept flat: nothing saved here has a point axis)
    ctx.save_for_backward(value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices.view(-1),
                          valid_ratios, logits)
    return value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios, logits


def _boxes_saved(ctx):
    """-> the operands again, and whether value / any of ref_windows, offsets and logits needs a gradient."""
    value, shapes, lsi, ref_windows, offsets, kernel_indices, valid_ratios, logits = ctx.saved_tensors
    need_v, _, _, need_r, need_o, _, _, need_l = ctx.needs_input_grad[:8]
    return ((value, shapes, lsi, ref_windows, offsets, kernel_indices.view(-1, 2), valid_ratios, logits),
            need_v, need_r or need_o or need_l)


def _boxes_param_grads(ctx, ref_windows, grads):
    """(grad_offsets, grad_ref_rows, grad_logits) of ``ops.*_backward_boxes`` -> (grad_ref, grad_offsets, grad_logits)
    in the inputs' types, None for an input that needs no gradient."""
    grad_offsets, rows, grad_logits = grads
    need_r, need_o, need_l = ctx.needs_input_grad[3], ctx.needs_input_grad[4], ctx.needs_input_grad[7]
    rdt, odt, ldt = ctx.in_dtypes
    return (_ref_grad(ref_windows, rows).to(rdt) if need_r else None, grad_offsets.to(odt) if need_o else None,
            grad_logits.to(ldt) if need_l else None)


def _boxes_grad_value(ctx, operands, angle_mode, weights, grad_output, grad_mask_output=None):
    """grad_value from the destination-binned backward, whose records need the per-point tensors: the sampling grid
    and ``weights()`` -> (weights, level weights or None) are built for this call only.  ``grad_mask_output`` None:
    the box flavour of the backward."""
    value, shapes, lsi, ref_windows, offsets, kernel_indices, valid_ratios, _ = operands
    B = offsets.size(0)
    loc = ops.box_grid_forward(ref_windows, offsets, kernel_indices, valid_ratios, angle_mode)
    w, level_w = weights()
    if grad_mask_output is not None:
        grad_value = ops.instance_attn_backward(value, shapes, lsi, loc, w, level_w, grad_output, grad_mask_output, B,
                                                plan=None, want=1)[0]
    else:
        grad_value = ops.box_attn_backward(value, shapes, lsi, loc, w, grad_output, B, plan=None, want=1)[0]
    del loc, w, level_w
    return grad_value.to(ctx.value_dtype)


class InstanceAttnBoxesFunction(Function):
    """(value (B,S,H,C), spatial_shapes, level_start_index, ref_windows (B,Lq,D) / (B,Lq,H,D), offsets (B,Lq,H,L,4),
    kernel_indices (k*k,2), valid_ratios None / B*L*2 values, logits (B,Lq,H,L,2,2), kernel_size) ->
    (output (B,Lq,H*C), mask_output (B,Lq,k,k,H*C)): InstanceAttention's training step from what the module predicts
    (``module.fused_boxes_train``).  The forward is ``ops.instance_attn_forward_boxes``; nothing per point is saved.
    The gradients of ``offsets``, ``ref_windows`` and ``logits`` come from one ``ops.instance_attn_backward_boxes``
    call; ``grad_value`` comes from the destination-binned backward, whose records need the per-point tensors: they
    are rebuilt for that call (same device functions: bit for bit what the forward sampled) and dropped after it.
    ``value`` is float32, or bfloat16 / float16: that is then the storage type -- outputs in it, upstream gradients
    cast to it, ``grad_value`` in the caller's type (the conventions of the 16-bit Functions above).  A mask output
    the loss did not use arrives as None and reaches the kernels as NULL."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios,
                logits, kernel_size):
        ctx.set_materialize_grads(False)
        ctx.k = int(kernel_size)
        operands = _boxes_operands(ctx, value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices,
                                   valid_ratios, logits)
        output, mask_output = ops.instance_attn_forward_boxes(*operands, ctx.k, need_mask=True)
        b, l, _, c = mask_output.shape
        return output, mask_output.view(b, l, ctx.k, ctx.k, c)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output, grad_mask_output):
        if grad_output is None and grad_mask_output is None:
            return (None,) * 9
        operands, need_v, need_params = _boxes_saved(ctx)
        value, ref_windows, offsets, logits = operands[0], operands[3], operands[4], operands[7]
        if grad_output is None:
            B, Lq, H = offsets.shape[:3]
            grad_output = value.new_zeros((B, Lq, H * value.size(3)))
        grad_output = grad_output.to(value.dtype).contiguous()
        if grad_mask_output is not None:
            grad_mask_output = grad_mask_output.to(value.dtype).contiguous()
        grad_value = grad_ref = grad_offsets = grad_logits = None
        if need_params:
            grad_ref, grad_offsets, grad_logits = _boxes_param_grads(ctx, ref_windows, ops.instance_attn_backward_boxes(
                *operands, ctx.k, grad_output, grad_mask_output, need_ref_grad=ctx.needs_input_grad[3]))
        if need_v:
            weights = lambda: ops.instance_weights_forward(logits, ctx.k, grad_mask_output is not None)
            grad_value = _boxes_grad_value(ctx, operands, 0, weights, grad_output, grad_mask_output)
        return (grad_value, None, None, grad_ref, grad_offsets, None, None, grad_logits, None)


class BoxAttnBoxesFunction(Function):
    """(value (B,S,H,C), spatial_shapes, level_start_index, ref_windows (B,Lq,D) / (B,Lq,H,D), offsets (B,Lq,H,L,V),
    kernel_indices (P,2), valid_ratios None / B*L*2 values, logits B*Lq*H*L*P values, angle_mode) -> output
    (B,Lq,H*C): BoxAttention's / Box3dAttention's training step from what the module predicts
    (``module.fused_boxes_train``).  The forward is ``ops.box_attn_forward_boxes``; nothing per point is saved.  The
    gradients of ``offsets``, ``ref_windows`` and ``logits`` come from one ``ops.box_attn_backward_boxes`` call;
    ``grad_value`` comes from the destination-binned backward, whose records need the per-point tensors: they are
    rebuilt for that call (same device functions: bit for bit the locations the forward sampled) and dropped after it.
    ``value`` is float32, or bfloat16 / float16: that is then the storage type -- output in it, the upstream gradient
    cast to it, ``grad_value`` in the caller's type (the conventions of ``InstanceAttnBoxesFunction``)."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios,
                logits, angle_mode):
        ctx.angle_mode = int(angle_mode)
        ctx.logits_shape = tuple(logits.shape)
        b, lq, h = offsets.shape[:3]
        operands = _boxes_operands(ctx, value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices,
                                   valid_ratios, logits.reshape(b, lq, h, -1))
        return ops.box_attn_forward_boxes(*operands, ctx.angle_mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        operands, need_v, need_params = _boxes_saved(ctx)
        value, ref_windows, offsets, logits = operands[0], operands[3], operands[4], operands[7]
        grad_output = grad_output.to(value.dtype).contiguous()
        grad_value = grad_ref = grad_offsets = grad_logits = None
        if need_params:
            grad_ref, grad_offsets, grad_logits = _boxes_param_grads(ctx, ref_windows, ops.box_attn_backward_boxes(
                *operands, ctx.angle_mode, grad_output, need_ref_grad=ctx.needs_input_grad[3]))
            if grad_logits is not None:
                grad_logits = grad_logits.view(ctx.logits_shape)
        if need_v:
            weights = lambda: (ops.softmax_forward(logits).view(*offsets.shape[:4], -1), None)
            grad_value = _boxes_grad_value(ctx, operands, ctx.angle_mode, weights, grad_output)
        return (grad_value, None, None, grad_ref, grad_offsets, None, None, grad_logits, None)


class BoxAttnBoxesStagedFunction(Function):
    """``BoxAttnBoxesFunction`` -- its signature, what it saves -- for the encoder's self-attention (one query per
    pixel, 32 channels a head, 2x2 points, at most 4 levels; ``module.fused_boxes_train_staged``) on the window-staged
    kernels: the forward is ``ops.box_attn_forward_boxes_staged``, the gradients of ``offsets``, ``ref_windows`` and
    ``logits`` come from one ``ops.box_attn_backward_boxes_staged`` call (bitwise reproducible).  ``grad_value`` comes
    from the destination-binned backward on rebuilt per-point tensors, as in ``BoxAttnBoxesFunction``.  Both calls raise
    where their ``ops.*_staged_ok`` says no: the caller asks first."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios,
                logits, angle_mode):
        ctx.angle_mode = int(angle_mode)
        ctx.logits_shape = tuple(logits.shape)
        b, lq, h = offsets.shape[:3]
        operands = _boxes_operands(ctx, value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices,
                                   valid_ratios, logits.reshape(b, lq, h, -1))
        return ops.box_attn_forward_boxes_staged(*operands, ctx.angle_mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        operands, need_v, need_params = _boxes_saved(ctx)
        value, ref_windows, offsets, logits = operands[0], operands[3], operands[4], operands[7]
        grad_output = grad_output.to(value.dtype).contiguous()
        grad_value = grad_ref = grad_offsets = grad_logits = None
        if need_params:
            grad_ref, grad_offsets, grad_logits = _boxes_param_grads(
                ctx, ref_windows, ops.box_attn_backward_boxes_staged(*operands, ctx.angle_mode, grad_output,
                                                                     need_ref_grad=ctx.needs_input_grad[3]))
            if grad_logits is not None:
                grad_logits = grad_logits.view(ctx.logits_shape)
        if need_v:
            weights = lambda: (ops.softmax_forward(logits).view(*offsets.shape[:4], -1), None)
            grad_value = _boxes_grad_value(ctx, operands, ctx.angle_mode, weights, grad_output)
        return (grad_value, None, None, grad_ref, grad_offsets, None, None, grad_logits, None)


class BoxAttnBoxesValueFunction(Function):
    """``BoxAttnBoxesFunction`` -- its signature, its forward, what it saves -- with the whole backward as ONE
    ``ops.box_attn_backward_boxes_value`` call (``module.fused_boxes_value``): ``grad_value`` is scattered with
    float32 atomics by the kernel that computes the gradients of ``offsets``, ``ref_windows`` and ``logits``, so no
    sampling grid, no weights and no plan exist in the backward either.  ``want`` follows ``needs_input_grad``: a
    frozen ``value`` runs the box and logit gradients alone, frozen heads ``grad_value`` alone.  ``grad_value`` is NOT
    bitwise reproducible here (the adds' order is the hardware's); the other three are, and equal
    ``BoxAttnBoxesFunction``'s bit for bit.  For few queries against the map (decoder cross-attention)."""

    forward = staticmethod(BoxAttnBoxesFunction.forward)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        operands, need_v, need_params = _boxes_saved(ctx)
        value, ref_windows = operands[0], operands[3]
        grad_ref = grad_offsets = grad_logits = None
        if not (need_v or need_params):
            return (None,) * 9
        grad_output = grad_output.to(value.dtype).contiguous()
        grad_value, *grads = ops.box_attn_backward_boxes_value(
            *operands, ctx.angle_mode, grad_output, want=(1 if need_v else 0) | (2 if need_params else 0),
            need_ref_grad=ctx.needs_input_grad[3])
        if need_params:
            grad_ref, grad_offsets, grad_logits = _boxes_param_grads(ctx, ref_windows, grads)
            if grad_logits is not None:
                grad_logits = grad_logits.view(ctx.logits_shape)
        if need_v:
            grad_value = grad_value.to(ctx.value_dtype)
        return (grad_value, None, None, grad_ref, grad_offsets, None, None, grad_logits, None)
