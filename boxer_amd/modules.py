"""nn.Modules with the surface of the reference's ``e2edet/module/box_attention.py``.

``BoxAttention`` (box_attention.py:140-239), ``InstanceAttention`` (:10-137) and
``Box3dAttention`` (:242-363): same constructor arguments, same parameter / buffer names and
shapes (so reference checkpoints load with ``load_state_dict``), same initialisation, same
``forward(query, value, v_shape, v_mask, v_start_index, v_valid_ratios, ref_windows)``
signature and return tuples.  The sampling itself runs in the HIP operator behind
``BoxAttnFunction`` / ``InstanceAttnFunction``.

The three reference classes repeat their code; here the shared parts (parameters, kernel
grid, box decoding, value projection) live in one base class.

Extra, not in the reference: ``native_bf16`` / ``native_f16`` (default False).  When one is set,
the op runs in the 16-bit storage mode (value / output bfloat16 or IEEE float16, fp32 locations,
weights and accumulation) instead of the reference's "always float32" contract.  Setting both is
an error.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dense, ops
from .functions import (BoxAttnBF16Function, BoxAttnBoxesFunction, BoxAttnBoxesStagedFunction,
                        BoxAttnBoxesValueFunction, BoxAttnF16Function,
                        BoxAttnFunction, BoxGridFunction, InstanceAttnBF16Function, InstanceAttnBoxesFunction,
                        InstanceAttnF16Function, InstanceAttnFunction, InstanceWeightsFunction, LogitSoftmaxFunction,
                        ValueMaskCastFunction)


def _f32(t):
    return t.float().contiguous()


def _kernel_offsets(kernel_size, divisor):
    """(k*k, 2) grid of (x, y) offsets in units of the box size, row-major over (y, x).
    Even k: half-pixel centred (-k/2+0.5 .. k/2-0.5); odd k: integer centred."""
    half = (kernel_size - 1) / 2.0
    ticks = torch.linspace(-half, half, kernel_size)
    ys, xs = torch.meshgrid(ticks, ticks, indexing="ij")
    return torch.stack([xs, ys], dim=-1).reshape(-1, 2) / divisor


class _BoxAttentionBase(nn.Module):
    """Parameters and geometry shared by the three attention flavours."""

    def __init__(self, d_model, num_level, num_head, kernel_size, box_vars, attn_points,
                 offset_divisor):
        super().__init__()
        assert d_model % num_head == 0, "d_model should be divided by num_head"
        self.im2col_step = 64
        self.d_model = d_model
        self.num_head = num_head
        self.num_level = num_level
        self.head_dim = d_model // num_head
        self.kernel_size = kernel_size
        self.native_bf16 = False
        self.native_f16 = False
        # opt-in: box -> grid expansion in one HIP kernel each way (BoxGridFunction).  (Until round
        # 5 the value 2 built the grid inside the sampling kernels; it never removed the grid tensor -- both bin passes
        # and the point gradients read it -- and was no faster than the one-kernel grid build: removed in round 6, any
        # true value means the grid kernels.)
        self.fused_grid = False
        # opt-in: the attention weights -- BoxAttention / Box3dAttention: the softmax over the L*P logits
        # (LogitSoftmaxFunction); InstanceAttention: spatial and level weights from the 2x2 logits per level
        # (InstanceWeightsFunction) -- and, in the 16-bit storage modes, the value mask-fill + 16-bit cast
        # (ValueMaskCastFunction) as single HIP passes
        self.fused_pointwise = False
        # opt-in, at inference only (no grad): the whole of forward between the projections as ONE HIP launch from the
        # predicted boxes and logits -- no sampling grid, no per-point weights.  InstanceAttention:
        # ops.instance_attn_forward_boxes, the third element of the return is then the empty tuple; BoxAttention /
        # Box3dAttention: ops.box_attn_forward_boxes, the second element of the return is then the empty tuple
        self.fused_boxes = False
        # opt-in, only together with `fused_boxes` and where that path is taken (BoxAttention / Box3dAttention;
        # InstanceAttention ignores it, and so does grad mode): where ops.box_forward_boxes_staged_ok says yes -- the
        # encoder's self-attention: one query per pixel, 32 channels a head, at most 4 levels --
        # ops.box_attn_forward_boxes_staged, the window-staged forward from the same operands; elsewhere
        # ops.box_attn_forward_boxes as without it
        self.fused_boxes_staged = False
        # opt-in, in training (grad mode): forward and backward from the boxes and logits -- no per-point tensor is built
        # in the forward or kept for the backward.  InstanceAttention (`inferencing` false): InstanceAttnBoxesFunction,
        # the third element of the return is then the empty tuple; BoxAttention / Box3dAttention:
        # BoxAttnBoxesFunction, the second element of the return is then the empty tuple.  `fused_boxes` does not
        # imply it.
        self.fused_boxes_train = False
        # opt-in, only together with `fused_boxes_train` (BoxAttention / Box3dAttention; InstanceAttention ignores it):
        # where that step is taken with fewer queries than pixels (cross-attention) and ops.box_backward_boxes_value_ok
        # says yes, BoxAttnBoxesValueFunction -- grad_value from float32 atomics inside the backward's one launch, NOT
        # bitwise reproducible -- instead of BoxAttnBoxesFunction
        self.fused_boxes_value = False
        # opt-in, only together with `fused_boxes_train` (BoxAttention / Box3dAttention; InstanceAttention ignores it):
        # where that step is taken and both ops.box_forward_boxes_staged_ok and ops.box_backward_boxes_staged_ok say
        # yes -- the encoder's self-attention: one query per pixel, 32 channels a head, at most 4 levels --
        # BoxAttnBoxesStagedFunction, forward and parameter gradients on the window-staged kernels from the same
        # operands, instead of BoxAttnBoxesFunction; elsewhere as without it.  (`fused_boxes_staged` stays an
        # inference switch: grad mode ignores it.)
        self.fused_boxes_train_staged = False

        self.linear_box_weight = nn.Parameter(torch.zeros(num_level * num_head * box_vars, d_model))
        self.linear_box_bias = nn.Parameter(torch.zeros(num_head * num_level * box_vars))
        self.linear_attn_weight = nn.Parameter(
            torch.zeros(num_head * num_level * attn_points, d_model))
        self.linear_attn_bias = nn.Parameter(torch.zeros(num_head * num_level * attn_points))
        self.value_proj = nn.Linear(d_model, d_model)
        self.out_proj = nn.Linear(d_model, d_model)
        self.register_buffer("kernel_indices", _kernel_offsets(kernel_size, offset_divisor))
        self._reset_parameters()

    def _reset_parameters(self):
        for proj in (self.out_proj, self.value_proj):
            nn.init.xavier_uniform_(proj.weight)
            nn.init.constant_(proj.bias, 0.0)
        nn.init.constant_(self.linear_attn_weight, 0.0)
        nn.init.constant_(self.linear_attn_bias, 0.0)
        nn.init.constant_(self.linear_box_weight, 0.0)
        nn.init.uniform_(self.linear_box_bias)

    # -- pieces of forward -------------------------------------------------------------
    def _project_value(self, value, v_mask):
        b, s = value.shape[:2]
        value = dense.linear(value, self.value_proj.weight, self.value_proj.bias)
        storage = self._storage_dtype()
        if (self.fused_pointwise and storage is not None and value.is_cuda and
                value.dtype in (torch.float32, storage) and self.d_model % 8 == 0 and
                (v_mask is not None or value.dtype != storage)):   # else: nothing to do
            value = ValueMaskCastFunction.apply(value, v_mask, storage)
        elif v_mask is not None:
            value = value.masked_fill(v_mask[..., None], float(0))
        return value.view(b, s, self.num_head, self.head_dim)

    def _fused_logits(self, logits):
        """Whether the single-pass weight kernels take these logits: float32 / bfloat16, or float16 in the
        float16 storage mode."""
        return (self.fused_pointwise and logits.is_cuda and
                (logits.dtype in (torch.float32, torch.bfloat16) or
                 (logits.dtype == torch.float16 and self._storage_dtype() == torch.float16)))

    def _softmax(self, logits):
        """softmax over the last axis (the L * P logits of a (query, head))."""
        if logits.size(-1) <= 64 and self._fused_logits(logits):
            return LogitSoftmaxFunction.apply(logits)
        return F.softmax(logits, dim=-1)

    def _box_offsets(self, query, ref_windows, n_vars):
        b, l = ref_windows.shape[:2]
        off = dense.linear(query, self.linear_box_weight, self.linear_box_bias)
        return off.view(b, l, self.num_head, self.num_level, n_vars)

    @staticmethod
    def _per_head_level(ref_windows):
        """(B,Lq,D) -> (B,Lq,1,1,D);  (B,Lq,H,D) -> (B,Lq,H,1,D)."""
        if ref_windows.dim() == 3:
            return ref_windows[:, :, None, None]
        return ref_windows[:, :, :, None]

    @staticmethod
    def _decode_boxes(ref_boxes, offset_boxes):
        """ref (cx,cy,w,h) + offset/8 scaled by the reference size -> centre, size with a
        points axis: (..., 1, 2) each."""
        wh = ref_boxes[..., 2:4]
        boxes = ref_boxes + offset_boxes / 8 * torch.cat([wh, wh], dim=-1)
        boxes = boxes.unsqueeze(-2)
        return boxes[..., :2], boxes[..., 2:]

    def _storage_dtype(self):
        """The 16-bit storage mode the op runs in: torch.bfloat16, torch.float16 or None (float32)."""
        if self.native_bf16 and self.native_f16:
            raise ValueError("native_bf16 and native_f16 are exclusive: set one of them")
        return torch.bfloat16 if self.native_bf16 else torch.float16 if self.native_f16 else None

    def _box_function(self):
        return {torch.bfloat16: BoxAttnBF16Function, torch.float16: BoxAttnF16Function}.get(
            self._storage_dtype(), BoxAttnFunction)

    def _use_fused_grid(self, query, v_valid_ratios):
        """The fused kernel covers the reference's call shapes: CUDA tensors and
        ``v_valid_ratios`` None or (B,1,1,L,1,2) (box_transformer.py:118-138)."""
        if not (self.fused_grid and query.is_cuda) or query.dtype == torch.float64:
            return False                      # (the kernel computes in float32)
        return self._reference_valid_ratios(query, v_valid_ratios)

    def _reference_valid_ratios(self, query, v_valid_ratios):
        """``v_valid_ratios`` as the reference passes them: None or (B,1,1,L,1,2)."""
        return v_valid_ratios is None or (
            v_valid_ratios.dim() == 6 and v_valid_ratios.size(0) == query.size(0)
            and tuple(v_valid_ratios.shape[1:]) == (1, 1, self.num_level, 1, 2))

    def _boxes_operand(self, query, value, v_valid_ratios):
        """``value`` in the type the kernels from boxes take it, or None where they do not run: CPU / float64 tensors,
        ``v_valid_ratios`` of another shape than the reference's."""
        if not (query.is_cuda and value.is_cuda):
            return None
        if torch.float64 in (query.dtype, value.dtype):
            return None                       # (the kernel computes in float32)
        if not self._reference_valid_ratios(query, v_valid_ratios):
            return None
        return value.to(self._storage_dtype() or torch.float32).contiguous()

    def _boxes_kernel_ok(self, value, num_query, backward):
        """Whether the forward / the backward from boxes and logits has its kernel for ``value`` and this module
        (ops.*_boxes_ok)."""
        raise NotImplementedError

    def _boxes_value(self, query, value, v_valid_ratios):
        """The projected ``value`` as the one-launch inference forward takes it (the storage mode's type, float32
        without one), or None: that path is not taken -- flag off, grad mode, what ``_boxes_operand`` refuses, or no
        kernel for the shape."""
        if not self.fused_boxes or torch.is_grad_enabled():
            return None
        value = self._boxes_operand(query, value, v_valid_ratios)
        return value if value is not None and self._boxes_kernel_ok(value, query.size(1), False) else None

    def _boxes_train(self, query, value, v_valid_ratios):
        """``value`` as the training step from boxes and logits takes it (a differentiable cast), or None: that path
        is not taken -- ``fused_boxes_train`` off, no grad mode, what ``_boxes_operand`` refuses, or no kernel for the
        shape one way or the other."""
        if not self.fused_boxes_train or not torch.is_grad_enabled():
            return None
        value = self._boxes_operand(query, value, v_valid_ratios)
        if value is None:
            return None
        n = query.size(1)
        return value if self._boxes_kernel_ok(value, n, True) and self._boxes_kernel_ok(value, n, False) else None


class BoxAttention(_BoxAttentionBase):
    def __init__(self, d_model, num_level, num_head, kernel_size=2):
        super().__init__(d_model, num_level, num_head, kernel_size, box_vars=4,
                         attn_points=kernel_size ** 2, offset_divisor=kernel_size)
        self.num_point = kernel_size ** 2

    def _where_to_attend(self, query, v_valid_ratios, ref_windows):
        offset_boxes = self._box_offsets(query, ref_windows, 4)
        if self._use_fused_grid(query, v_valid_ratios):
            return BoxGridFunction.apply(ref_windows, offset_boxes, self.kernel_indices,
                                         v_valid_ratios, 0)
        center, size = self._decode_boxes(self._per_head_level(ref_windows), offset_boxes)
        grid = center + self.kernel_indices * torch.relu(size)
        if v_valid_ratios is not None:
            grid = grid * v_valid_ratios
        return grid.contiguous()

    def _softmax_weights(self, query):
        b, l1 = query.shape[:2]
        w = dense.linear(query, self.linear_attn_weight, self.linear_attn_bias)
        w = self._softmax(w.view(b, l1, self.num_head, -1))
        return w.view(b, l1, self.num_head, self.num_level, self.kernel_size, self.kernel_size)

    def _angle_mode(self):
        return 0

    def _boxes_kernel_ok(self, value, num_query, backward):
        ok = ops.box_backward_boxes_ok if backward else ops.box_forward_boxes_ok
        return ok(value, self.num_level, num_query, self.num_point)

    def _forward_boxes(self, query, value, v_shape, v_start_index, v_valid_ratios, ref_windows):
        b, l1 = query.shape[:2]
        mode = self._angle_mode()
        logits = dense.linear(query, self.linear_attn_weight, self.linear_attn_bias)
        offsets = self._box_offsets(query, ref_windows, 5 if mode == 1 else 4)
        staged = self.fused_boxes_staged and ops.box_forward_boxes_staged_ok(value, v_shape, v_start_index, l1,
                                                                             self.num_point)
        output = (ops.box_attn_forward_boxes_staged if staged else ops.box_attn_forward_boxes)(
            value, v_shape, v_start_index, _f32(ref_windows), _f32(offsets), _f32(self.kernel_indices),
            None if v_valid_ratios is None else _f32(v_valid_ratios).view(b, self.num_level, 2),
            _f32(logits).view(b, l1, self.num_head, -1), mode)
        return dense.linear(output, self.out_proj.weight, self.out_proj.bias), ()

    def _boxes_train_function(self, value, num_query, v_shape=None, v_start_index=None):
        """The Function of the training step from boxes for ``value`` (B,S,H,C) as ``_boxes_train`` returned it:
        ``fused_boxes_train_staged`` where both staged calls have their kernel (the encoder: one query per pixel) ->
        the window-staged one; ``fused_boxes_value`` with fewer queries than pixels and a kernel for the shape -> the
        one with grad_value in the backward's own launch."""
        if (self.fused_boxes_train_staged and v_shape is not None and
                ops.box_forward_boxes_staged_ok(value, v_shape, v_start_index, num_query, self.num_point) and
                ops.box_backward_boxes_staged_ok(value, v_shape, v_start_index, num_query, self.num_point)):
            return BoxAttnBoxesStagedFunction
        if (self.fused_boxes_value and num_query < value.size(1) and
                ops.box_backward_boxes_value_ok(value, self.num_level, num_query, self.num_point)):
            return BoxAttnBoxesValueFunction
        return BoxAttnBoxesFunction

    def _forward_boxes_train(self, query, value, v_shape, v_start_index, v_valid_ratios, ref_windows):
        b, l1 = query.shape[:2]
        mode = self._angle_mode()
        logits = dense.linear(query, self.linear_attn_weight, self.linear_attn_bias)
        # (differentiable casts: the gradients flow on to the projections, the query and the reference windows)
        output = self._boxes_train_function(value, l1, v_shape, v_start_index).apply(
            value, v_shape, v_start_index, ref_windows.float(),
            self._box_offsets(query, ref_windows, 5 if mode == 1 else 4).float(), self.kernel_indices,
            None if v_valid_ratios is None else v_valid_ratios.view(b, self.num_level, 2),
            logits.float().view(b, l1, self.num_head, -1), mode)
        return dense.linear(output, self.out_proj.weight, self.out_proj.bias), ()

    def forward(self, query, value, v_shape, v_mask, v_start_index, v_valid_ratios, ref_windows):
        value = self._project_value(value, v_mask)
        boxes_value = self._boxes_value(query, value, v_valid_ratios)
        if boxes_value is not None:
            return self._forward_boxes(query, boxes_value, v_shape, v_start_index, v_valid_ratios, ref_windows)
        boxes_value = self._boxes_train(query, value, v_valid_ratios)
        if boxes_value is not None:
            return self._forward_boxes_train(query, boxes_value, v_shape, v_start_index, v_valid_ratios, ref_windows)
        attn_weights = self._softmax_weights(query)
        sampled_grid = self._where_to_attend(query, v_valid_ratios, ref_windows)
        output = self._box_function().apply(value, v_shape, v_start_index, sampled_grid,
                                            attn_weights, self.im2col_step)
        return dense.linear(output, self.out_proj.weight, self.out_proj.bias), attn_weights


class Box3dAttention(BoxAttention):
    def __init__(self, d_model, num_level, num_head, with_rotation=True, kernel_size=2):
        # note: the 3D module scales the kernel grid by 1/2 whatever the kernel size
        # (box_attention.py:291)
        _BoxAttentionBase.__init__(self, d_model, num_level, num_head, kernel_size,
                                   box_vars=5 if with_rotation else 4,
                                   attn_points=kernel_size ** 2, offset_divisor=2)
        self.with_rotation = with_rotation
        self.num_variable = 5 if with_rotation else 4
        self.num_point = kernel_size ** 2

    def _angle_mode(self):
        return 1 if self.with_rotation else 2

    def _where_to_attend(self, query, v_valid_ratios, ref_windows):
        b, l = ref_windows.shape[:2]
        offsets = self._box_offsets(query, ref_windows, self.num_variable)
        if self._use_fused_grid(query, v_valid_ratios):
            return BoxGridFunction.apply(ref_windows, offsets, self.kernel_indices,
                                         v_valid_ratios, 1 if self.with_rotation else 2)
        ref = self._per_head_level(ref_windows)       # (cx,cy,w,h,angle[,vx,vy])
        ref_boxes, ref_angles = ref[..., :4], ref[..., 4:5]
        if self.with_rotation:
            angles = (ref_angles + offsets[..., 4:5] / 16) * 2 * math.pi
            offsets = offsets[..., :4]
        else:
            angles = ref_angles.expand(b, l, self.num_head, self.num_level, 1)
        center, size = self._decode_boxes(ref_boxes, offsets)

        cos, sin = torch.cos(angles), torch.sin(angles)           # (B,Lq,H,L,1)
        local = self.kernel_indices * torch.relu(size)            # (B,Lq,H,L,P,2), box frame
        lx, ly = local[..., 0], local[..., 1]
        rotated = torch.stack([lx * cos - ly * sin, lx * sin + ly * cos], dim=-1)
        grid = center + rotated
        if v_valid_ratios is not None:
            grid = grid * v_valid_ratios
        return grid.contiguous()


class InstanceAttention(_BoxAttentionBase):
    def __init__(self, d_model, num_level, num_head, kernel_size):
        # attention logits are predicted on a 2x2 grid per level and replicated to k x k
        super().__init__(d_model, num_level, num_head, kernel_size, box_vars=4, attn_points=4,
                         offset_divisor=kernel_size)

    _where_to_attend = BoxAttention._where_to_attend

    def _boxes_kernel_ok(self, value, num_query, backward):
        ok = ops.backward_boxes_ok if backward else ops.forward_boxes_ok
        return ok(value, self.num_level, num_query, self.kernel_size)

    def _boxes_train(self, query, value, v_valid_ratios):
        """``_BoxAttentionBase._boxes_train``, and not while ``inferencing``."""
        if not self.fused_boxes_train or not torch.is_grad_enabled() or self.inferencing:
            return None
        return super()._boxes_train(query, value, v_valid_ratios)

    def _forward_boxes_train(self, query, value, v_shape, v_start_index, v_valid_ratios, ref_windows, logits):
        b, l1 = query.shape[:2]
        # (differentiable casts: the gradients flow on to the projections, the query and the reference windows)
        output, mask_output = InstanceAttnBoxesFunction.apply(
            value, v_shape, v_start_index, ref_windows.float(), self._box_offsets(query, ref_windows, 4).float(),
            self.kernel_indices, None if v_valid_ratios is None else v_valid_ratios.view(b, self.num_level, 2),
            logits.float(), self.kernel_size)
        return self.out_proj(output), self.out_proj(mask_output), ()

    def _boxes_operand(self, query, value, v_valid_ratios):
        """``_BoxAttentionBase._boxes_operand`` where the instance weights exist: k even, 2 ... 32; else None."""
        k = self.kernel_size
        if not (isinstance(k, int) and k % 2 == 0 and 2 <= k <= 32):
            return None
        return super()._boxes_operand(query, value, v_valid_ratios)

    def _forward_boxes(self, query, value, v_shape, v_start_index, v_valid_ratios, ref_windows, logits):
        b, l1 = query.shape[:2]
        k = self.kernel_size
        offsets = _f32(self._box_offsets(query, ref_windows, 4))
        output, mask_output = ops.instance_attn_forward_boxes(
            value, v_shape, v_start_index, _f32(ref_windows), offsets, _f32(self.kernel_indices),
            None if v_valid_ratios is None else _f32(v_valid_ratios).view(b, self.num_level, 2), _f32(logits), k,
            need_mask=not self.inferencing)
        if mask_output is not None:
            mask_output = self.out_proj(mask_output.view(b, l1, k, k, self.d_model))
        return self.out_proj(output), mask_output, ()

    def forward(self, query, value, v_shape, v_mask, v_start_index, v_valid_ratios, ref_windows):
        b, l1 = query.shape[:2]
        k = self.kernel_size
        value = self._project_value(value, v_mask)

        logits = dense.linear(query, self.linear_attn_weight, self.linear_attn_bias)
        logits = logits.view(b, l1, self.num_head, self.num_level, 2, 2)
        boxes_value = self._boxes_value(query, value, v_valid_ratios)
        if boxes_value is not None:
            return self._forward_boxes(query, boxes_value, v_shape, v_start_index, v_valid_ratios, ref_windows,
                                       logits)
        boxes_value = self._boxes_train(query, value, v_valid_ratios)
        if boxes_value is not None:
            return self._forward_boxes_train(query, boxes_value, v_shape, v_start_index, v_valid_ratios, ref_windows,
                                             logits)
        # (the kernels' shapes: k even, 2 ... 32, at most 16 levels)
        fused = (k % 2 == 0 and 2 <= k <= 32 and self.num_level <= 16 and self._fused_logits(logits))
        if fused:
            spatial_attn_weights, level_attn_weights = InstanceWeightsFunction.apply(
                logits, k, not self.inferencing)
        else:
            logits = logits.repeat_interleave(k // 2, dim=-1).repeat_interleave(k // 2, dim=-2)
            spatial_attn_weights = F.softmax(logits.reshape(b, l1, self.num_head, -1), dim=-1).view(
                b, l1, self.num_head, self.num_level, k, k)

        sampled_grid = self._where_to_attend(query, v_valid_ratios, ref_windows)

        # `inferencing` is injected by the model (base_model.py:49-67); like the reference,
        # a bare module without it raises AttributeError here.
        if not self.inferencing:
            if not fused:
                level_attn_weights = F.softmax(
                    logits.view(b, l1, self.num_head, self.num_level, k, k), dim=3)
            fn = {torch.bfloat16: InstanceAttnBF16Function, torch.float16: InstanceAttnF16Function}.get(
                self._storage_dtype(), InstanceAttnFunction)
            output, mask_output = fn.apply(value, v_shape, v_start_index, sampled_grid,
                                           spatial_attn_weights, level_attn_weights, k,
                                           self.im2col_step)
            attn_weights = (spatial_attn_weights, level_attn_weights)
            mask_output = self.out_proj(mask_output)
        else:
            output = self._box_function().apply(value, v_shape, v_start_index, sampled_grid,
                                                spatial_attn_weights, self.im2col_step)
            attn_weights = (spatial_attn_weights,)
            mask_output = None
        return self.out_proj(output), mask_output, attn_weights
