"""Per-point problems, for the routes of the reference's API (locations and weights per sampling point): seeded
inputs and their expectations, the inputs and runners of the per-element error bounds, raw backward calls with their
workspace and state, launch counters, and the group-record helpers.  Inputs are built on the CPU when a case asks."""
import functools
import math

import numpy as np
import pytest
import torch

import bench
import error_bounds as eb
import route_vocab
from compare_rules import check_f16, close_parity, rounded_from_f32
from isolation import DECODER, ENCODER, WIDE_LEVELS
from oracle import boxattn_oracle as oc
from route_vocab import (ACC_F32, ACC_SPLIT, ACC_TR, ACC_VALU, BF16, DTYPES, F16, F32, FAST, GATHER, GENERIC, KEY_GROUP,
                         KEY_POINT, REC_GROUP, REC_POINT, STAGED, to_device)


def _seeded(shapes, B, H, C, Lq, P, seed, lo=-0.1, hi=1.1):
    rng = np.random.default_rng(seed)
    shapes = np.asarray(shapes, dtype=np.int64)
    sizes = shapes.prod(1)
    lsi = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    S, L = int(sizes.sum()), len(shapes)
    value = rng.integers(-127, 128, (B, S, H, C)).astype(np.float64) / 64
    loc = rng.uniform(lo, hi, (B, Lq, H, L, P, 2)).astype(np.float32).astype(np.float64)
    a = rng.uniform(1e-5, 1, (B, Lq, H, L, P))
    attn = (a / a.sum((-1, -2), keepdims=True)).astype(np.float32).astype(np.float64)
    lvl = (a / a.sum(-2, keepdims=True)).astype(np.float32).astype(np.float64)
    gout = rng.integers(-64, 65, (B, Lq, H * C)).astype(np.float64) / 32
    gmask = rng.integers(-64, 65, (B, Lq, P, H * C)).astype(np.float64) / 32
    return dict(value=value, shapes=shapes, lsi=lsi, loc=loc, attn=attn, spatial_w=attn,
                level_w=lvl, grad_out=gout, grad_mask=gmask, on_edge=on_cell_edge(loc, shapes))


def on_cell_edge(loc, shapes, eps=1e-4):
    """(B,Lq,H,L,P,1) mask of points whose pixel coordinate is within eps of an integer.
    grad_loc is discontinuous there (the bilinear cell changes), so float32 arithmetic and the
    float64 oracle may legitimately pick different cells; such points are excluded from the
    grad_loc comparison (their other outputs are continuous and stay checked)."""
    size = np.asarray(shapes, dtype=np.float64)[None, None, None, :, None, ::-1]   # (W, H)
    pix = loc * size - 0.5
    return (np.abs(pix - np.round(pix)) < eps).any(-1, keepdims=True)


SEEDED = [
    # shapes, B, H, C, Lq, P
    ([(20, 30), (10, 15), (5, 8), (3, 4)], 2, 8, 32, 333, 4),     # BoxeR encoder geometry
    ([(20, 30), (10, 15)], 1, 8, 32, 7, 16),                      # ragged tail wave
    ([(9, 7)], 3, 4, 16, 50, 4),                                  # G=4 path
    ([(9, 7), (4, 3)], 2, 2, 64, 21, 9),                          # G=16 path, odd P
    ([(9, 7), (4, 3)], 2, 3, 12, 5, 4),                           # C%4==0 but no fast variant
    ([(6, 5)], 1, 1, 1, 3, 1),                                    # minimum everything
    # odd map sizes (uneven destination blocks), one-pixel-wide / -high levels, enough points
    # per block for chunked work items
    ([(25, 25), (13, 13), (7, 5), (1, 3), (2, 1)], 1, 2, 32, 700, 4),
    ([(13, 21), (5, 4)], 2, 2, 64, 300, 9),                       # 8 channels per lane, G=8 (bf16)
    # few queries x many points: one wave per (query, head) pair in the instance forward;
    # 3 and 5 levels do not fill the lane groups evenly
    ([(11, 9), (6, 5), (3, 2)], 1, 4, 32, 6, 49),
    ([(11, 9), (6, 5), (3, 2), (2, 2), (1, 1)], 2, 2, 32, 3, 36),
    # ... two waves per pair (head = workgroup mod 8), an odd number of (image, query) rows: the last workgroup's second
    # pair does not exist
    ([(11, 9), (6, 5)], 1, 8, 32, 7, 40),
]


# d = 256, 8 heads (32 channels per head), 4 levels, 2 x 2 points: the shapes the window-staged / gather / binned
# kernels run (G7 / G8: d = 32 with 4 heads = 8 channels per head, generic kernels only).  Outputs AND gradients --
# of query, value, reference windows and every parameter -- against what torch's autograd gives for the reference's
# own module code in float64 (tests/golden/make_goldens.py g9), for every opt-in path, with the path that ran asserted.
PARITY_G9 = {
    "G9_module_box_enc": ("BoxAttention", dict(kernel_size=2), 1),
    "G9_module_box_enc_masked": ("BoxAttention", dict(kernel_size=2), 1),
    "G9_module_box_dec": ("BoxAttention", dict(kernel_size=2), 1),
    "G9_module_box3d_fixed_enc": ("Box3dAttention", dict(with_rotation=False, kernel_size=2), 1),
    "G9_module_box3d_rot_dec": ("Box3dAttention", dict(with_rotation=True, kernel_size=2), 1),
    "G9_module_inst_k4": ("InstanceAttention", dict(kernel_size=4), 2),
}


def _torch_grid(ref, off, kidx, vr, angle_mode):
    """The reference modules' _where_to_attend after the offset projection
    (box_attention.py:63-81, 304-338)."""
    r = ref[:, :, None, None] if ref.dim() == 3 else ref[:, :, :, None]
    wh = r[..., 2:4]
    boxes = r[..., :4] + off[..., :4] / 8 * torch.cat([wh, wh], dim=-1)
    boxes = boxes.unsqueeze(-2)
    c, size = boxes[..., :2], boxes[..., 2:]
    local = kidx * torch.relu(size)
    if angle_mode:
        ang = (r[..., 4:5] + off[..., 4:5] / 16) * 2 * math.pi if angle_mode == 1 \
            else r[..., 4:5].expand(off.shape[:4] + (1,))
        cos, sin = torch.cos(ang), torch.sin(ang)
        lx, ly = local[..., 0], local[..., 1]
        local = torch.stack([lx * cos - ly * sin, lx * sin + ly * cos], dim=-1)
    grid = c + local
    return grid * vr if vr is not None else grid


STAT_OFF = 1024          # state buffer: the one-pass counters behind the locality counters (include/boxattn.h)


LEVELS4 = [(37, 53), (19, 27), (10, 14), (5, 7)]


def _lib():
    from boxer_amd import _lib
    return _lib.load()


def make_onepass_case(levels, lq, family="model", B=2, H=8, C=32, seed=0, dtype=torch.bfloat16):
    name = "_onepass_test"
    bench.WORKLOADS[name] = (list(levels), lq, 4, "box")
    old = bench.H_HEADS, bench.C_HEAD
    bench.H_HEADS, bench.C_HEAD = H, C
    try:
        return bench.make_inputs(name, dtype, "cuda", family=family, batch=B, seed=seed)
    finally:
        bench.H_HEADS, bench.C_HEAD = old
        del bench.WORKLOADS[name]


def step(inp, entry="train"):
    from boxer_amd import ops
    v, sh, ls, loc, attn, go = (inp[k] for k in ("value", "shapes", "lsi", "loc", "attn", "grad_out"))
    if entry == "train":
        out, plan = ops.box_attn_forward_train(v, sh, ls, loc, attn, 64)
        grads = ops.box_attn_backward(v, sh, ls, loc, attn, go, 64, plan=plan)
    else:                      # the reference's two calls: nothing but the tensors goes from one to the other
        out = ops.box_attn_forward(v, sh, ls, loc, attn, 64)
        grads = ops.box_attn_backward(v, sh, ls, loc, attn, go, 64)
    torch.cuda.synchronize()
    return out, grads


def counters():
    """{calls of the one-pass chain, blocks redone} summed over the state buffers boxer_amd.ops keeps."""
    from boxer_amd import ops
    tot = np.zeros(2, dtype=np.int64)
    for st in ops._STATE.values():
        tot += st[STAT_OFF:STAT_OFF + 16].view(torch.int64).cpu().numpy()
    return int(tot[0]), int(tot[1])


def binning_launches(inp, entry="train"):
    from boxer_amd import _lib
    _lib.profile_begin()
    try:
        out, grads = step(inp, entry)
    finally:
        slots = _lib.profile_end()
    return out, grads, slots["bwd_binning"]["launches"]


LEVELS_A = [(16, 24), (7, 5), (1, 3)]
SHAPE_A = dict(levels=LEVELS_A, B=2, H=3, C=32, Lq=300, k=4)


def instance_problem(levels, B, H, C, Lq, k, dtype, seed=5, loc_range=(-0.2, 1.2)):
    """numpy float64 inputs whose storage tensors are already numbers of ``dtype``."""
    rng = np.random.default_rng(seed)
    shapes = np.asarray(levels, dtype=np.int64)
    sizes = shapes.prod(1)
    lsi = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    S, L, P = int(sizes.sum()), len(levels), k * k
    loc = rng.uniform(*loc_range, (B, Lq, H, L, P, 2)).astype(np.float32).astype(np.float64)
    a = rng.uniform(1e-5, 1, (B, Lq, H, L, P))
    return dict(shapes=shapes, lsi=lsi, loc=loc, k=k, dims=(B, S, H, C, L, Lq, P),
                value=rounded_from_f32(rng.standard_normal((B, S, H, C)), dtype),
                spatial_w=(a / a.sum((-1, -2), keepdims=True)).astype(np.float32).astype(np.float64),
                level_w=(a / a.sum(-2, keepdims=True)).astype(np.float32).astype(np.float64),
                grad_out=rounded_from_f32(rng.standard_normal((B, Lq, H * C)), dtype),
                grad_mask=rounded_from_f32(rng.standard_normal((B, Lq, P, H * C)), dtype))


ENCODER_SEEDS = (1, 2, 3)
# (family, seed) -> the seed actually taken: a case whose share of cell-edge points is above eb.EDGE_CAP is re-seeded
# here (tests/test_error_bounds.py checks every input below)
RESEED = {}


@functools.lru_cache(maxsize=None)
def encoder_input(family, dtype, seed):
    return eb.make(ENCODER, "S", family, DTYPES[dtype], seed=RESEED.get((family, seed), seed))


@functools.lru_cache(maxsize=None)
def decoder_input(family, dtype):
    return eb.make(DECODER, 50, family, DTYPES[dtype], seed=RESEED.get((family, "decoder"), 1))


@functools.lru_cache(maxsize=None)
def seeded6_input(C):
    """SEEDED[6] of test_gpu_parity: value and grad_out on a 1/64 grid -- the same numbers in every storage type."""
    shapes, B, H, _, Lq, P = SEEDED[6]
    g = _seeded(shapes, B, H, C, Lq, P, seed=11)
    return dict(kind="box", value=g["value"], shapes=g["shapes"], lsi=g["lsi"], loc=g["loc"], attn=g["attn"],
                grad_out=g["grad_out"])


@functools.lru_cache(maxsize=None)
def wide_input(P):
    """Few queries x many points on three levels: the wave-per-pair forward (test_gpu_wide_box_forward.seeded)."""
    rng = np.random.default_rng(100 + P)
    shapes = np.asarray(WIDE_LEVELS, dtype=np.int64)
    sizes = shapes.prod(1)
    B, Lq, H, C, L = 2, 6, 2, 32, len(WIDE_LEVELS)
    a = rng.random((B, Lq, H, L, P))
    a[rng.random(a.shape) < 0.1] = 0.0
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    return dict(kind="box", shapes=shapes, lsi=np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64),
                value=eb.round_to(rng.standard_normal((B, int(sizes.sum()), H, C)), "bf16"),
                loc=f32(rng.uniform(-0.2, 1.2, (B, Lq, H, L, P, 2))), attn=f32(a),
                grad_out=np.zeros((B, Lq, H * C)))


@functools.lru_cache(maxsize=None)
def shape_a_input(dtype):
    g = instance_problem(dtype=DTYPES[dtype], **SHAPE_A)
    return dict(g, kind="instance", attn=g["spatial_w"])


@functools.lru_cache(maxsize=None)
def k14_input(dtype):
    return eb.make(DECODER, 6, "model", DTYPES[dtype], kind="instance", P=196, seed=RESEED.get(("k14", 1), 1))


@functools.lru_cache(maxsize=None)
def boxes_input():
    """Reference windows, box offsets and 2 x 2 logits for the forward from boxes: k = 14, six queries, four levels."""
    rng = np.random.default_rng(RESEED.get(("boxes", 14), 14))
    B, Lq, H, C, L = 2, 6, 2, 32, len(DECODER)
    shapes = np.asarray(DECODER, dtype=np.int64)
    sizes = shapes.prod(1)
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    ref = np.concatenate([rng.uniform(0.05, 0.95, (B, Lq, 2)), rng.uniform(0.05, 0.7, (B, Lq, 2))], -1)
    return dict(shapes=shapes, lsi=np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64), vr=None,
                dims=(B, int(sizes.sum()), H, C, L, Lq), value=rng.standard_normal((B, int(sizes.sum()), H, C)),
                ref=f32(ref), off=f32(rng.standard_normal((B, Lq, H, L, 4))),
                logits=f32(rng.standard_normal((B, Lq, H, L, 2, 2))))


# every input the cases below use, for the CPU twin: name -> a function that builds it
def all_inputs():
    for family in ("model", "test", "border"):
        for dtype in DTYPES:
            for seed in ENCODER_SEEDS:
                yield "encoder %s %s seed %d" % (family, dtype, seed), functools.partial(encoder_input, family, dtype, seed)
    for family in ("model", "test"):
        for dtype in DTYPES:
            yield "decoder %s %s" % (family, dtype), functools.partial(decoder_input, family, dtype)
    for C in (16, 32, 64):
        yield "SEEDED[6] C=%d" % C, functools.partial(seeded6_input, C)
    for dtype in ("bf16", "f16"):            # (float32 takes the bf16 numbers)
        yield "instance shape A %s" % dtype, functools.partial(shape_a_input, dtype)
    for dtype in DTYPES:
        yield "instance k=14 %s" % dtype, functools.partial(k14_input, dtype)


def box_tensors(inp, dtype, device="cuda"):
    """(device "cpu": for the route queries of the CPU twin, which are host code)"""
    d = lambda a, dt=None: to_device(a, dt, device)
    return dict(value=d(inp["value"], dtype), shapes=d(inp["shapes"]), lsi=d(inp["lsi"]), loc=d(inp["loc"], F32),
                attn=d(inp["attn"], F32), grad_out=d(inp["grad_out"], dtype))


def run_box(t):
    """The reference's two calls: forward, then the full backward."""
    from boxer_amd import ops
    a = [t[k] for k in ("value", "shapes", "lsi", "loc", "attn")]
    out = ops.box_attn_forward(*a, 64)
    gv, gl, ga = ops.box_attn_backward(*a, t["grad_out"], 64)
    torch.cuda.synchronize()
    return dict(out=out, grad_value=gv, grad_loc=gl, grad_attn=ga)


def run_instance(t):
    from boxer_amd import ops
    a = [t[k] for k in ("value", "shapes", "lsi", "loc", "attn", "level_w")]
    out, mask = ops.instance_attn_forward(*a, 64)
    gv, gl, gs, glw = ops.instance_attn_backward(*a, t["grad_out"], t["grad_mask"], 64)
    torch.cuda.synchronize()
    return dict(out=out, mask_out=mask, grad_value=gv, grad_loc=gl, grad_spatial=gs, grad_level=glw)


def inst_tensors(inp, dtype, device="cuda"):
    t = box_tensors(inp, dtype, device)
    t["level_w"], t["grad_mask"] = to_device(inp["level_w"], F32, device), to_device(inp["grad_mask"], dtype, device)
    return t


def encoder_expectation(dtype, dense, riders, acc_key, rec_key):
    """-> (forward family, accumulate kind, record kind, one pass?) of an encoder case under its keys."""
    if dtype == "f32":
        acc = {0: ACC_SPLIT, 1: ACC_VALU, 2: ACC_F32}[acc_key]
        rec = REC_POINT
    else:
        acc, rec = ACC_TR, REC_GROUP if rec_key == 2 else REC_POINT
    # the one-pass fill: riders on and a matrix-core accumulate (boxattn_host_plan.h: spec_ok)
    return STAGED if dense == 2 else GATHER, acc, rec, riders == 0 and acc != ACC_VALU


ENCODER_ROUTES = [("f32", acc, 0) for acc in (0, 1, 2)] + [(dt, 0, rec) for dt in ("bf16", "f16") for rec in (1, 2)]


DECODER_FORWARD = {0: GATHER, 1: GENERIC, 2: FAST, 3: GATHER}        # the forward family of every kernel variant
# (the generic variant is held in float32)
DECODER_ROUTES = [(dt, v) for dt in sorted(DTYPES) for v in (0, 1, 2, 3) if v != 1 or dt == "f32"]

BOX_NAMES = ("out", "grad_value", "grad_loc", "grad_attn")
INST_NAMES = ("out", "mask_out", "grad_value", "grad_loc", "grad_spatial", "grad_level")


def oracle(d, cast):
    """Every output of the C oracle in float64 (cast = np.float64) or float32 arithmetic."""
    c = lambda a: np.ascontiguousarray(a, dtype=cast)
    if d["kind"] == "instance":
        a = (c(d["value"]), d["shapes"], d["lsi"], c(d["loc"]), c(d["spatial_w"]), c(d["level_w"]))
        res = list(oc.instance_attn_forward(*a)) + list(oc.instance_attn_backward(*a, c(d["grad_out"]), c(d["grad_mask"])))
        return dict(zip(INST_NAMES, res))
    a = (c(d["value"]), d["shapes"], d["lsi"], c(d["loc"]), c(d["attn"]))
    return dict(zip(BOX_NAMES, [oc.box_attn_forward(*a)] + list(oc.box_attn_backward(*a, c(d["grad_out"])))))


def make_dense_case(levels, family, H=8, B=2, seed=0, dtype=torch.bfloat16):
    """bench.make_inputs for an ad-hoc encoder shape; extra families on top of "model" / "test":
    "mixed" = model-like with every 7th box thrown far away, "border" = locations in [-0.2, 1.2]."""
    name = "_dense_test"
    bench.WORKLOADS[name] = (list(levels), "S", 4, "box")
    old_h = bench.H_HEADS
    bench.H_HEADS = H
    try:
        base = "model" if family in ("model", "mixed") else "test"
        inp = bench.make_inputs(name, dtype, "cuda", family=base, batch=B, seed=seed)
    finally:
        bench.H_HEADS = old_h
        del bench.WORKLOADS[name]
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    loc = inp["loc"]
    if family == "mixed":
        far = torch.rand(loc.shape[:-2], device="cuda", generator=g) < 1.0 / 7
        shift = torch.rand(loc.shape[:-2] + (1, 2), device="cuda", generator=g) - 0.5
        inp["loc"] = torch.where(far[..., None, None], loc + shift, loc).contiguous()
    elif family == "border":
        inp["loc"] = (torch.rand(loc.shape, device="cuda", generator=g) * 1.4 - 0.2).contiguous()
    return inp


LEVELS = {
    "4lv": [(20, 28), (10, 14), (5, 7), (3, 4)],
    "4lv_odd": [(37, 23), (19, 12), (10, 6), (5, 3)],
    "3lv": [(16, 16), (8, 8), (4, 4)],
    "2lv": [(33, 17), (16, 9)],
    "1lv": [(9, 13)],
    "tiny": [(4, 5), (2, 3), (1, 1)],
}

VALUE, POINTS, ALL = 1, 2, 3


HINT_FRESH_STATE = 2
REPEATS = 6                          # further runs that settle whether a family's grad_value sum is ordered
PATTERN = 0x5A                       # what an output nobody asked for must still hold after the call
SUFFIX = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16", torch.float16: "f16"}


def _blib():
    from boxer_amd import _lib
    return _lib


class Case:
    """Device tensors of one problem + what the raw entry points need."""

    def __init__(self, kind, dtype, value, shapes, lsi, loc, weights, grad_out, grad_mask=None):
        self.kind, self.dtype = kind, dtype
        self.cdt = torch.float32 if dtype in (torch.bfloat16, torch.float16) else dtype
        self.value, self.shapes, self.lsi, self.loc = value, shapes, lsi, loc
        self.weights, self.grad_out, self.grad_mask = list(weights), grad_out, grad_mask
        B, S, H, C = value.shape
        self.dims = (B, S, H, C, shapes.size(0), loc.size(1), loc.size(4))
        self.sh, self.ls = shapes.cpu().numpy().copy(), lsi.cpu().numpy().copy()
        lib = _blib().load()
        h16 = int(dtype in (torch.bfloat16, torch.float16))
        host = (self.sh.ctypes.data, self.ls.ctypes.data)
        self.ws_bytes = max(256, int(lib.boxattn_bwd_workspace_bytes(h16, *self.dims, *host)))
        self.state_bytes = int(lib.boxattn_state_bytes(*self.dims, *host))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")

    @property
    def n_out(self):
        return 3 if self.kind == "box" else 4

    def new_state(self):
        return torch.zeros(self.state_bytes, dtype=torch.uint8, device="cuda")

    def outputs(self, pattern=False):
        """[grad_value, grad_loc, weight gradients ...], uninitialised or filled with PATTERN bytes."""
        outs = [torch.empty_like(self.value), torch.empty(self.loc.shape, dtype=self.cdt, device="cuda")]
        outs += [torch.empty(w.shape, dtype=self.cdt, device="cuda") for w in self.weights]
        if pattern:
            for t in outs:
                t.view(torch.uint8).fill_(PATTERN)
        return outs


def untouched(t):
    return bool((t.view(torch.uint8) == PATTERN).all().item())


def call(case, want=None, outs=None, ws="own", state=None, fresh=False, hints=0, null=()):
    """One raw backward call: want None -> *_bwd_ws_* (float64: the plain backward), else *_bwd_part_*.
    null: indices of outputs passed as NULL.  -> (rc, outs)"""
    lib = _blib().load()
    outs = case.outputs() if outs is None else outs
    stem = "boxattn" if case.kind == "box" else "instattn"
    f64 = case.dtype == torch.float64
    name = "%s_bwd%s_%s" % (stem, "_part" if want is not None else ("" if f64 else "_ws"), SUFFIX[case.dtype])
    args = [case.value, case.shapes, case.lsi, case.loc, *case.weights, case.grad_out]
    if case.kind == "instance":
        args.append(case.grad_mask)
    args = [a.data_ptr() for a in args] + list(case.dims)
    args += [0 if i in null else t.data_ptr() for i, t in enumerate(outs)]
    if not f64:
        wsbuf = case.ws if isinstance(ws, str) else ws
        args += [case.sh.ctypes.data, case.ls.ctypes.data,
                 wsbuf.data_ptr() if wsbuf is not None else 0, wsbuf.numel() if wsbuf is not None else 0, 0, 0,
                 state.data_ptr() if state is not None else 0, state.numel() if state is not None else 0,
                 hints | (HINT_FRESH_STATE if fresh else 0)]
    args.append(torch.cuda.current_stream().cuda_stream)
    if want is not None:
        args.append(want)
    rc = getattr(lib, name)(*args)
    torch.cuda.synchronize()
    return rc, outs


def profiled(fn):
    """-> (result of fn(), {slot: launches})"""
    blib = _blib()
    blib.profile_begin()
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        slots = blib.profile_end()
    return res, {k: v["launches"] for k, v in slots.items()}


@functools.lru_cache(maxsize=None)
def seeded(shapes, B, H, C, Lq, P, seed):
    g = _seeded([list(s) for s in shapes], B, H, C, Lq, P, seed=seed)
    box = oc.box_attn_backward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attn"], g["grad_out"])
    inst = oc.instance_attn_backward(g["value"], g["shapes"], g["lsi"], g["loc"], g["spatial_w"], g["level_w"],
                                     g["grad_out"], g["grad_mask"])
    return g, {"box": list(box), "instance": list(inst)}        # computed once, shared, never written


def seeded_case(kind, dtype, cfg, seed=31):
    g, want = seeded(*cfg, seed)
    dev = route_vocab.dev
    cdt = torch.float32 if dtype in (torch.bfloat16, torch.float16) else dtype
    weights = [dev(g["attn"], cdt)] + ([dev(g["level_w"], cdt)] if kind == "instance" else [])
    case = Case(kind, dtype, dev(g["value"], dtype), dev(g["shapes"]), dev(g["lsi"]), dev(g["loc"], cdt), weights,
                dev(g["grad_out"], dtype), dev(g["grad_mask"], dtype) if kind == "instance" else None)
    return case, want[kind], g["on_edge"]


PARTIAL_DECODER = (((12, 10), (6, 5)), 2, 8, 32, 13)
P_OF = {"generic": {"box": 2, "instance": 4}, "decoder": {"box": 4, "instance": 16}}


def backward_with_plan(case, entry, want, outs, ws, plan):
    """One raw call of *_bwd_ws_* (entry "ws") or *_bwd_part_* ("part"): ws (tensor view | None), plan (tensor | None),
    no state.  -> rc"""
    stem = "boxattn" if case.kind == "box" else "instattn"
    args = [case.value, case.shapes, case.lsi, case.loc, *case.weights, case.grad_out]
    if case.kind == "instance":
        args.append(case.grad_mask)
    args = [a.data_ptr() for a in args] + list(case.dims) + [t.data_ptr() for t in outs]
    args += [case.sh.ctypes.data, case.ls.ctypes.data,
             ws.data_ptr() if ws is not None else 0, ws.numel() if ws is not None else 0,
             plan.data_ptr() if plan is not None else 0, plan.numel() if plan is not None else 0, 0, 0, 0,
             torch.cuda.current_stream().cuda_stream]
    if entry == "part":
        args.append(want)
    rc = getattr(_blib().load(), "%s_bwd_%s_%s" % (stem, entry, SUFFIX[case.dtype]))(*args)
    torch.cuda.synchronize()
    return rc


RUN_TO_RUN = {BF16: 1e-2, F16: 1e-3, torch.float32: 1e-4}
EACH_16BIT_DTYPE = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])


def make(levels, lq, family="model", dtype=BF16, B=2, H=2, C=32, seed=0, kind="box"):
    name = "_group_records_test"
    bench.WORKLOADS[name] = (list(levels), lq, 4, kind)
    old = bench.H_HEADS, bench.C_HEAD
    bench.H_HEADS, bench.C_HEAD = H, C
    try:
        return bench.make_inputs(name, dtype, "cuda", family=family, batch=B, seed=seed)
    finally:
        bench.H_HEADS, bench.C_HEAD = old
        del bench.WORKLOADS[name]


def f64(t):
    return t.detach().double().cpu().numpy()


def on_edge(inp):
    """Sample points on a bilinear cell edge: grad_loc jumps there (on_cell_edge)."""
    size = f64(inp["shapes"])[None, None, None, :, None, ::-1]
    pix = f64(inp["loc"]) * size - 0.5
    return (np.abs(pix - np.round(pix)) < 1e-4).any(-1, keepdims=True)


def group_records_oracle(inp):
    """grad_value, grad_loc, grad_attn of the C oracle on the stored (rounded) inputs; computed once per input set."""
    if "_want" not in inp:
        inp["_want"] = oc.box_attn_backward(f64(inp["value"]), inp["shapes"].cpu().numpy(), inp["lsi"].cpu().numpy(),
                                            f64(inp["loc"]), f64(inp["attn"]), f64(inp["grad_out"]))
        inp["_edge"] = on_edge(inp)
        inp["_ref"] = eb.box_reference(inp["value"], inp["shapes"], inp["lsi"], inp["loc"], inp["attn"], inp["grad_out"])
    return inp["_want"]


def backward(inp, key):
    from boxer_amd import _lib, ops
    _lib.set_option("group_records", key)
    v, sh, ls, loc, attn, go = (inp[k] for k in ("value", "shapes", "lsi", "loc", "attn", "grad_out"))
    want_kind = _lib.REC_GROUP if key == KEY_GROUP else _lib.REC_POINT
    assert ops.backward_record_kind(v, loc) == want_kind, (ops.backward_record_kind(v, loc), want_kind)
    ops.box_attn_forward(v, sh, ls, loc, attn, 64)
    grads = ops.box_attn_backward(v, sh, ls, loc, attn, go, 64)
    torch.cuda.synchronize()
    return grads


def worst(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(f64(got).reshape(want.shape) - want).max()) / max(1.0, float(np.abs(want).max()))


def check_oracle(inp, grads, what):
    want = group_records_oracle(inp)
    dtype = inp["value"].dtype
    for name, t, w in zip(("grad_value", "grad_loc", "grad_attn"), grads, want):
        ignore = inp["_edge"] if name == "grad_loc" else None
        if dtype == F16:
            check_f16(t, w, "%s: %s" % (what, name), ignore=ignore)
        else:
            close_parity(t, w, dtype if name == "grad_value" else torch.float32, "%s: %s" % (what, name), ignore=ignore)
    hold_bound(inp, grads, what)


def hold_bound(inp, grads, what):
    """Every element inside the bound of tests/error_bounds.py: one rounding to the storage type, float32
    sums, grad_value's weights in two 16-bit terms -- for both record kinds.  (The hand-placed cases put points on cell
    edges on purpose: those are left out of grad_loc as above, their share is not capped here.)"""
    group_records_oracle(inp)
    dtype = inp["value"].dtype
    if dtype not in (BF16, F16):
        return
    worst = []
    for name, t in zip(("grad_value", "grad_loc", "grad_attn"), grads):
        store, split = (dtype, eb.store_name(dtype)) if name == "grad_value" else ("float32", "none")
        worst.append("%s %.3f" % (name, eb.hold(t, inp["_ref"][name], store, split, "%s: %s" % (what, name))))
    print("%s: worst err / bound %s" % (what, ", ".join(worst)))


def check_routes(inp, group, point, what):
    """key 24 = 2 against key 24 = 1 on the same inputs."""
    dtype = inp["value"].dtype
    assert torch.equal(group[1], point[1]), "%s: grad_loc differs between the record kinds" % what
    assert torch.equal(group[2], point[2]), "%s: grad_attn differs between the record kinds" % what
    ref = point[0].float()
    err = (group[0].float() - ref).abs().max().item()
    bound = RUN_TO_RUN[dtype] * max(1.0, ref.abs().max().item())
    want = group_records_oracle(inp)[0]
    eg, ep = worst(group[0], want), worst(point[0], want)
    print("%s: grad_value worst scaled error group %.3e / point %.3e = %.2f; group - point %.3e (bound %.1e)"
          % (what, eg, ep, eg / max(ep, 1e-30), err, bound))
    assert err <= bound, "%s: grad_value of the two record kinds differs by %.3e > %.1e" % (what, err, bound)


def both_routes(sets, what):
    """Every input set under key 24 = 2, in order, on one state; then under key 24 = 1 on a fresh one.  -> the group
    route's (calls, redone) counters after every set."""
    from boxer_amd import ops
    ops.release_workspaces()
    group, seen = [], []
    for inp in sets:
        group.append(backward(inp, KEY_GROUP))
        seen.append(counters())
    ops.release_workspaces()
    point = [backward(inp, KEY_POINT) for inp in sets]
    for i, inp in enumerate(sets):
        check_oracle(inp, group[i], "%s, call %d, group records" % (what, i))
        hold_bound(inp, point[i], "%s, call %d, point records" % (what, i))
        check_routes(inp, group[i], point[i], "%s, call %d" % (what, i))
    return seen
