"""GPU (the calls take CUDA tensors; no attention kernel is launched): the four calls from boxes and logits --
``ops.instance_attn_forward_boxes``, ``ops.instance_attn_backward_boxes``, ``ops.box_attn_forward_boxes`` and
``ops.box_attn_backward_boxes`` -- refuse arguments that do not fit before any device call, each with the exception type
and the full text it has always had: RuntimeError with the bare text from the instance calls, ValueError with the
function's name in front from the box calls, TypeError for a non-Tensor from both.  One table: geometry B 1, Lq 2, H 2,
C 32, one 3x4 level, k = 2 / P = 4, one defect a row.  The expected texts are written out, not computed."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, LQ, H, C, L, K, P = 1, 2, 2, 32, 1, 2, 4
S = 3 * 4
INST_FWD, INST_BWD, BOX_FWD, BOX_BWD = ("instance_attn_forward_boxes", "instance_attn_backward_boxes",
                                        "box_attn_forward_boxes", "box_attn_backward_boxes")
INSTANCE = (INST_FWD, INST_BWD)
BACKWARD = (INST_BWD, BOX_BWD)


def good_arguments(call, dev):
    """The keyword arguments of a call that fits (it is never made)."""
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    args = dict(value=f32(B, S, H, C), spatial_shapes=torch.tensor([[3, 4]], dtype=torch.int64, device=dev),
                level_start_index=torch.zeros(1, dtype=torch.int64, device=dev), ref_windows=f32(B, LQ, 4),
                offsets=f32(B, LQ, H, L, 4), kernel_indices=f32(P, 2), valid_ratios=f32(B, L, 2),
                logits=f32(B, LQ, H, L, 2, 2) if call in INSTANCE else f32(B, LQ, H, L * P))
    if call in INSTANCE:
        args["kernel_size"] = K
    else:
        args["angle_mode"] = 0
    if call in BACKWARD:
        args["grad_output"] = f32(B, LQ, H * C)
    if call == INST_BWD:
        args["grad_mask_output"] = f32(B, LQ, P, H * C)
    return args


# a defect: a function that breaks the good arguments in place
def non_contiguous_logits(a):
    a["logits"] = torch.zeros(tuple(a["logits"].shape) + (2,), device=a["logits"].device)[..., 0]


def float64_value(a):
    a["value"] = a["value"].double()


def int32_shapes(a):
    a["spatial_shapes"] = a["spatial_shapes"].int()


def logits_wrong_shape(a):          # the instance calls: the right count in another shape
    a["logits"] = a["logits"].view(B, LQ, H, L, 4)


def logits_wrong_count(a):          # the box calls
    a["logits"] = a["logits"].flatten()[:-1].clone()


def value_other_batch(a):
    a["value"] = a["value"].new_zeros((B + 1, S, H, C))


def nine_kernel_rows(a):
    a["kernel_indices"] = a["kernel_indices"].new_zeros((9, 2))


def five_offsets(a):
    a["offsets"] = a["offsets"].new_zeros((B, LQ, H, L, 5))


def valid_ratios_wrong_count(a):
    a["valid_ratios"] = a["valid_ratios"].new_zeros((B, L, 3))


def grad_output_bf16(a):
    a["grad_output"] = a["grad_output"].bfloat16()


def grad_output_wrong_count(a):
    a["grad_output"] = a["grad_output"].new_zeros((B, LQ, H * C - 1))


def grad_output_no_tensor(a):
    a["grad_output"] = None


def value_no_tensor(a):
    a["value"] = [0.0]


def eight_channels(a):
    a["value"] = a["value"].new_zeros((B, S, H, 8))
    if "grad_output" in a:
        a["grad_output"] = a["grad_output"].new_zeros((B, LQ, H * 8))
    if "grad_mask_output" in a:
        a["grad_mask_output"] = a["grad_mask_output"].new_zeros((B, LQ, P, H * 8))


R, V, T = RuntimeError, ValueError, TypeError
TABLE = [
    # non-contiguous logits
    (INST_FWD, non_contiguous_logits, R, "logits must be contiguous"),
    (INST_BWD, non_contiguous_logits, R, "logits must be contiguous"),
    (BOX_FWD, non_contiguous_logits, V, "box_attn_forward_boxes: logits must be contiguous"),
    (BOX_BWD, non_contiguous_logits, V, "box_attn_backward_boxes: logits must be contiguous"),
    # float64 value
    (INST_FWD, float64_value, R,
     "instance_attn_forward_boxes: float32, bfloat16 or float16 value expected, got torch.float64"),
    (INST_BWD, float64_value, R,
     "instance_attn_backward_boxes: float32, bfloat16 or float16 value expected, got torch.float64"),
    (BOX_FWD, float64_value, V, "box_attn_forward_boxes: float32, bfloat16 or float16 value expected, got torch.float64"),
    (BOX_BWD, float64_value, V, "box_attn_backward_boxes: float32, bfloat16 or float16 value expected, got torch.float64"),
    # int32 spatial_shapes
    (INST_FWD, int32_shapes, R, "spatial_shapes / level_start_index must be int64"),
    (INST_BWD, int32_shapes, R, "spatial_shapes / level_start_index must be int64"),
    (BOX_FWD, int32_shapes, V, "box_attn_forward_boxes: spatial_shapes / level_start_index must be int64"),
    (BOX_BWD, int32_shapes, V, "box_attn_backward_boxes: spatial_shapes / level_start_index must be int64"),
    # logits of the wrong shape (instance) or count (box)
    (INST_FWD, logits_wrong_shape, R, "expected logits (B,Lq,H,L,2,2) float32 matching offsets"),
    (INST_BWD, logits_wrong_shape, R, "expected logits (B,Lq,H,L,2,2) float32 matching offsets"),
    (BOX_FWD, logits_wrong_count, V, "box_attn_forward_boxes: expected B*Lq*H*L*P float32 logits matching offsets"),
    (BOX_BWD, logits_wrong_count, V, "box_attn_backward_boxes: expected B*Lq*H*L*P float32 logits matching offsets"),
    # value with another B
    (INST_FWD, value_other_batch, R, "offsets / spatial_shapes do not match value (B,S,H,C)"),
    (INST_BWD, value_other_batch, R, "offsets / spatial_shapes do not match value (B,S,H,C)"),
    (BOX_FWD, value_other_batch, V, "box_attn_forward_boxes: offsets / spatial_shapes do not match value (B,S,H,C)"),
    (BOX_BWD, value_other_batch, V, "box_attn_backward_boxes: offsets / spatial_shapes do not match value (B,S,H,C)"),
    # kernel_indices with the wrong row count (instance)
    (INST_FWD, nine_kernel_rows, R, "kernel_indices must have kernel_size**2 rows"),
    (INST_BWD, nine_kernel_rows, R, "kernel_indices must have kernel_size**2 rows"),
    # offsets with V = 5 under angle_mode 0 (box)
    (BOX_FWD, five_offsets, V, "box_attn_forward_boxes: box_grid: offsets / ref_windows do not fit angle_mode 0"),
    (BOX_BWD, five_offsets, V, "box_attn_backward_boxes: box_grid: offsets / ref_windows do not fit angle_mode 0"),
    # valid_ratios of the wrong count
    (INST_FWD, valid_ratios_wrong_count, R, "expected valid_ratios with B*L*2 float32 elements"),
    (INST_BWD, valid_ratios_wrong_count, R, "expected valid_ratios with B*L*2 float32 elements"),
    (BOX_FWD, valid_ratios_wrong_count, V, "box_attn_forward_boxes: expected valid_ratios with B*L*2 float32 elements"),
    (BOX_BWD, valid_ratios_wrong_count, V, "box_attn_backward_boxes: expected valid_ratios with B*L*2 float32 elements"),
    # grad_output of the wrong type and of the wrong count (the backward calls)
    (INST_BWD, grad_output_bf16, R, "grad_output: 128 elements of type torch.float32 expected"),
    (BOX_BWD, grad_output_bf16, V, "box_attn_backward_boxes: grad_output: 128 elements of type torch.float32 expected"),
    (INST_BWD, grad_output_wrong_count, R, "grad_output: 128 elements of type torch.float32 expected"),
    (BOX_BWD, grad_output_wrong_count, V,
     "box_attn_backward_boxes: grad_output: 128 elements of type torch.float32 expected"),
    # a non-Tensor: a TypeError with the bare text from every call
    (INST_BWD, grad_output_no_tensor, T, "grad_output must be a Tensor"),
    (BOX_BWD, grad_output_no_tensor, T, "grad_output must be a Tensor"),
    (INST_FWD, value_no_tensor, T, "value must be a Tensor"),
    (INST_BWD, value_no_tensor, T, "value must be a Tensor"),
    (BOX_FWD, value_no_tensor, T, "value must be a Tensor"),
    (BOX_BWD, value_no_tensor, T, "value must be a Tensor"),
    # C = 8: no kernel
    (INST_FWD, eight_channels, R, "instance_attn_forward_boxes: no kernel for value (1, 12, 2, 8), 1 levels, 2 queries, "
                                  "kernel_size 2 (forward_boxes_ok)"),
    (INST_BWD, eight_channels, R, "instance_attn_backward_boxes: no kernel for value (1, 12, 2, 8), 1 levels, 2 queries, "
                                  "kernel_size 2 at the alignment of value and the gradients (backward_boxes_ok)"),
    (BOX_FWD, eight_channels, V, "box_attn_forward_boxes: no kernel for value (1, 12, 2, 8), 1 levels, 2 queries, "
                                 "4 points a level (box_forward_boxes_ok)"),
    (BOX_BWD, eight_channels, V, "box_attn_backward_boxes: no kernel for value (1, 12, 2, 8), 1 levels, 2 queries, "
                                 "4 points a level at the alignment of value and grad_output (box_backward_boxes_ok)"),
]


@pytest.fixture(scope="module")
def ops():
    from boxer_amd import _lib, ops
    _lib.set_variant(0)
    return ops


@pytest.fixture
def no_launch(ops):
    """Fails the test if a call gets as far as its device call."""
    launched = []
    orig = ops._grid_call
    ops._grid_call = lambda name, *a: launched.append(name)
    yield launched
    ops._grid_call = orig


@pytest.mark.parametrize("call, defect, exc, text", TABLE,
                         ids=["%s-%s" % (row[0], row[1].__name__) for row in TABLE])
def test_refused_with_the_type_and_text(ops, no_launch, call, defect, exc, text):
    args = good_arguments(call, torch.device("cuda:0"))
    defect(args)
    with pytest.raises(exc) as info:
        getattr(ops, call)(**args)
    assert type(info.value) is exc and str(info.value) == text
    assert no_launch == []


def test_the_good_arguments_pass_every_check(ops, no_launch):
    """The table's base case passes every check of every call, so each defect is the only one of its row: the box
    calls reach their device call (intercepted: nothing is launched); the instance calls get as far as the last check,
    the kernel's eligibility, which k = 2 (4 points a level: too few for the wave-per-pair kernels) does not pass."""
    dev = torch.device("cuda:0")
    for call in (BOX_FWD, BOX_BWD):
        getattr(ops, call)(**good_arguments(call, dev))
    assert no_launch == ["boxattn_fwd_boxes_f32", "boxattn_bwd_boxes_f32"]
    for call, text in (
            (INST_FWD, "instance_attn_forward_boxes: no kernel for value (1, 12, 2, 32), 1 levels, 2 queries, "
                       "kernel_size 2 (forward_boxes_ok)"),
            (INST_BWD, "instance_attn_backward_boxes: no kernel for value (1, 12, 2, 32), 1 levels, 2 queries, "
                       "kernel_size 2 at the alignment of value and the gradients (backward_boxes_ok)")):
        with pytest.raises(RuntimeError) as info:
            getattr(ops, call)(**good_arguments(call, dev))
        assert str(info.value) == text
