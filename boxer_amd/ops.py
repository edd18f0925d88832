"""``boxer_amd.ops`` -- drop-in for the reference's native module ``e2edet.ops``.

Same four functions, same argument order and return values as the pybind module of the
reference (e2edet/module/ops/src/vision.cpp:7-12; host code box_attn.cu:15-135,
instance_attn.cu:15-157), implemented as thin calls into the C-ABI HIP library
(include/boxattn.h).  Same error behaviour: CPU tensors raise "Not implemented on the CPU"
(box_attn.h:53), non-contiguous tensors raise "... must be contiguous" (box_attn.cu:9-11),
``batch % min(batch, im2col_step)`` is asserted (box_attn.cu:40-42).  Kernel launch errors
raise instead of being printed (box_attn_kernel.cuh:1118-1122).

Beyond the reference: ``value`` (and the upstream gradients) may be bfloat16 or float16; sampling
locations and attention weights are then taken in float32 (16-bit ones are upcast), their gradients
come back in float32, and all accumulation is float32.  float32 / float64 calls behave exactly like the reference.
"""
import os

import torch

from . import _lib

_SUFFIX = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16", torch.float16: "f16"}
_H16 = (torch.bfloat16, torch.float16)      # 16-bit storage: float32 geometry, same kernels and workspace sizes
_BOXES_DTYPES = (torch.float32,) + _H16     # the storage types of the calls from boxes


def _check(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor: Not implemented on the CPU" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


def _prepare(value, shapes, lsi, loc, weights, extra=()):
    """Validate like the reference's CHECK_INPUT block and derive the dimensions."""
    _check(value, "value")
    _check(shapes, "spatial_shapes")
    _check(lsi, "level_start_index")
    _check(loc, "sampling_loc")
    for i, w in enumerate(weights):
        _check(w, "attn_weight" if len(weights) == 1 else ("spatial_attn_weight", "level_attn_weight")[i])
    for name, t in extra:
        _check(t, name)
    if value.dtype not in _SUFFIX:
        raise RuntimeError("box_attn: unsupported dtype %s (float32, float64, bfloat16, float16)" % value.dtype)
    if shapes.dtype != torch.int64 or lsi.dtype != torch.int64:
        raise RuntimeError("spatial_shapes / level_start_index must be int64")
    if value.dim() != 4 or loc.dim() != 6 or loc.size(-1) != 2:
        raise RuntimeError("expected value (B,S,H,C) and sampling_loc (B,Lq,H,L,P,2)")
    B, S, H, C = value.shape
    L = shapes.size(0)
    Lq, P = loc.size(1), loc.size(4)
    if loc.size(0) != B or loc.size(2) != H or loc.size(3) != L or lsi.numel() != L:
        raise RuntimeError("sampling_loc / spatial_shapes do not match value")
    n_w = B * Lq * H * L * P
    for w in weights:
        if w.numel() != n_w:
            raise RuntimeError("attention weights must have B*Lq*H*L*P elements")
    cdt = torch.float32 if value.dtype in _H16 else value.dtype
    if value.dtype in _H16:
        loc = loc.float() if loc.dtype != torch.float32 else loc
        weights = [w.float() if w.dtype != torch.float32 else w for w in weights]
    elif loc.dtype != cdt or any(w.dtype != cdt for w in weights):
        raise RuntimeError("value, sampling_loc and attention weights must share one dtype")
    for name, t in extra:
        if t.dtype != value.dtype:
            raise RuntimeError("%s must have the dtype of value" % name)
    return (B, S, H, C, L, Lq, P), loc, weights, cdt


def _chunk_assert(batch, im2col_step):
    step = min(batch, int(im2col_step))
    if batch > 0:
        assert step > 0 and batch % step == 0, \
            "batch(%d) must divide im2col_step(%d)" % (batch, step)


def _host_table(t):
    """Host copy of a small int64 device table (level shapes / start indices).  The copy is
    cached ON the tensor object together with its version counter, so only the first call with
    a given tensor synchronises (BoxeR hands the same two tensors to every layer of a step).
    Keying a global cache by data_ptr would be wrong: a freed tensor's address gets reused."""
    cached = getattr(t, "_boxattn_host", None)
    if cached is None or cached[0] != t._version:
        cached = (t._version, t.detach().cpu().contiguous().numpy().copy())
        try:
            t._boxattn_host = cached
        except Exception:          # objects that refuse attributes: just do not cache
            pass
    return cached[1]


class BackwardPlan:
    """Opaque hand-over from a training forward to the matching backward: the (small) device buffer in
    which the forward's launch already counted and scanned the sample points' destination bins (the
    binning only depends on the sampling locations), plus what it is valid for."""

    __slots__ = ("buf", "key", "hints", "keep")

    def __init__(self, buf, key, hints=0):
        self.buf, self.key, self.hints = buf, key, hints       # hints: as the forward ran (BOXATTN_HINT_*)
        self.keep = None                                       # parked plans: the tensors the key names (see _park)


def _plan_key(dims, loc, weights, dtype=None):
    # (the library's option switches -- records per item, riders, accumulate flavour, variant -- change the plan's
    # layout: a plan built under other settings is not this call's plan; so does the storage type: at 16 / 64 channels
    # per head bfloat16 bins contiguous query ranges and float32 interleaved ones)
    return (tuple(dims), loc.device.index, _lib.options_epoch(), dtype) + tuple((t.data_ptr(), t._version)
                                                                                for t in (loc,) + tuple(weights))


class _NoGuard:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _device_guard(device):
    """torch.cuda.device(device) -- unless it is the current device already (the usual case: the context manager
    costs several microseconds of a 55 us step)."""
    return _NO_GUARD if device.index == torch.cuda.current_device() else torch.cuda.device(device)


_SIZES = {}          # (query name, is_h16, dims, level tables, options epoch) | ("state", dims, dtype, level tables)
                     # -> bytes: the size queries are pure functions (_query_bytes)
_CACHE_CAP = 1024    # entries per shape-keyed cache: a detector trained on variably padded batches sees thousands of
                     # shapes; everything cached per shape is cheap to rebuild


def _bounded(cache):
    """Shape-keyed caches start over instead of growing without bound (entries still referenced elsewhere -- a
    state buffer a running kernel uses -- live on until the caching allocator gets them back, in stream order)."""
    if len(cache) >= _CACHE_CAP:
        cache.clear()
    return cache


def _query_bytes(query, is_h16, dims, sh, ls, key=None):
    """What a size query of the library answers (boxattn_plan_bytes, boxattn_bwd_workspace_bytes; boxattn_state_bytes,
    which takes no storage flag: is_h16 None), asked once per shape and options epoch.  key: the cache key, from a
    caller that has the tables' bytes at hand already (the state's size depends on no option: no epoch in its key)."""
    if key is None:
        key = (query.__name__, is_h16, dims, sh.tobytes(), ls.tobytes(), _lib.options_epoch())
    nbytes = _SIZES.get(key)
    if nbytes is None:
        flag = () if is_h16 is None else (is_h16,)
        nbytes = _bounded(_SIZES)[key] = int(query(*flag, *dims, sh.ctypes.data, ls.ctypes.data))
    return nbytes


def _sized_buffer(query, value, shapes, lsi, dims):
    """A scratch tensor of the size the library asks for (None for 0 bytes) + the host level tables."""
    sh, ls = _host_table(shapes), _host_table(lsi)
    nbytes = _query_bytes(query, int(value.dtype in _H16), dims, sh, ls)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=value.device) if nbytes else None
    return buf, sh, ls


_STATE = {}          # (device index, stream handle, dims, dtype) -> the library's persistent state buffer


def _state_buffer(key, device, nbytes):
    """The library's state buffer (include/boxattn.h, *_fwd_train_*: `state`): zeroed once and kept -- calls on
    one stream never overlap and every call leaves the tickets in it zero -- instead of a zero-fill launch in
    front of every training forward.  One per (stream, shape): its first 1 KiB are the locality counters, and a
    _Locality must only ever see the misses of ITS shape's calls (one buffer per stream, which the library would
    be content with, let the counts of one test's uniformly random locations decide the kernels of the next
    shape's first calls)."""
    buf = _STATE.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.zeros(int(nbytes), dtype=torch.uint8, device=device)
        buf._boxattn_fresh = True        # (its first call says so: BOXATTN_HINT_FRESH_STATE)
        # (a tensor first created while the stream captures a graph lives in the graph's private pool: it serves
        # this call -- the graph keeps it alive -- but must not outlive the graph in this table)
        if not torch.cuda.is_current_stream_capturing():
            _bounded(_STATE)[key] = buf
    return buf


class _Locality:
    """Data-driven choice between the window-staged and the row-gather kernels of the encoder case (VERDICT
    round 3, item 7).  The staged forward adds {points that missed their window, points sampled} to counters
    in the state buffer; after a training forward the counters are copied to pinned host memory WITHOUT a
    synchronisation, and whichever copy has arrived by the next call decides its `hints`: above
    MISS_THRESHOLD the calls run the gather kernels (BOXATTN_HINT_NOT_LOCAL); every PROBE_EVERY-th call runs
    the staged kernels again to see whether the sampling locations have become local.  One instance per
    (device, stream, dimensions); results never depend on the choice."""

    MISS_THRESHOLD = 0.5
    PROBE_EVERY = 64
    enabled = True

    def __init__(self):
        self.not_local = False
        self.calls_since_probe = 0
        self.pending = None          # a read of the counters is in flight
        self.host = self.event = None    # pinned buffer / event of the reads
        self.last = None             # counters at the previous read
        self.ratio = None            # the miss ratio the current choice is based on
        self.since_read = 0
        self.reads = 0
        self.last_hints = 0          # of the last training forward (a backward that gets no plan follows them)

    READ_EVERY = 16                  # staged calls between two reads of the counters

    def hints(self):
        # (nothing here touches an event while the stream is capturing a graph: querying one from the capturing
        # thread is not a capture-safe call; the last decision stands)
        if self.pending is not None and not torch.cuda.is_current_stream_capturing() and self.event.query():
            now = self.host.view(-1, 2).sum(0)
            self.pending = None
            # the FIRST read is the baseline (a state buffer that served an earlier _Locality of this shape carries
            # that one's counts); decisions from the second read on
            if self.last is not None:
                d_miss, d_all = int(now[0] - self.last[0]), int(now[1] - self.last[1])
                if d_all > 0:
                    self.ratio = d_miss / d_all
                    self.not_local = self.ratio > self.MISS_THRESHOLD
            self.last = now
        if not self.enabled:
            return 0
        if self.not_local:
            self.calls_since_probe += 1
            if self.calls_since_probe >= self.PROBE_EVERY:
                self.calls_since_probe = 0
                self.since_read = self.READ_EVERY       # (a probe is always read)
                return 0                                   # probe: a staged call refreshes the counters
            return _lib.HINT_NOT_LOCAL
        return 0

    def after_call(self, state, hints):
        """Queue an asynchronous read of the counters: after the first staged calls, then every READ_EVERY-th
        one (one read in flight at a time; nothing here ever waits for the GPU)."""
        if hints or self.pending is not None:
            return
        self.since_read += 1
        if self.since_read < self.READ_EVERY and self.reads >= 2:
            return
        if torch.cuda.is_current_stream_capturing():
            return
        if self.host is None:
            self.host = torch.empty(128, dtype=torch.int64, pin_memory=True)
            self.event = torch.cuda.Event()
        self.host.copy_(state[:1024].view(torch.int64), non_blocking=True)   # the counters: the buffer's first 1 KiB
        self.event.record()
        self.pending = True
        self.since_read = 0
        self.reads += 1


_LOCALITY = {}       # (device index, stream handle, dims) -> _Locality


def _shape_key(value, stream, dims, sh, ls):
    # one state buffer per (device, stream, dimensions, storage type, level shapes): ABI 8 keeps the record ranges of the
    # backward's one-pass fill in it, which belong to ONE geometry
    return (value.device.index, stream, tuple(dims), value.dtype, sh.tobytes(), ls.tobytes())


def _fresh_hint(state):
    return _lib.HINT_FRESH_STATE if getattr(state, "_boxattn_fresh", False) else 0


def _state_for(lib, value, dims, sh, ls, stream):
    key = _shape_key(value, stream, dims, sh, ls)
    nbytes = _query_bytes(lib.boxattn_state_bytes, None, dims, sh, ls, ("state",) + key[2:])
    return key, _state_buffer(key, value.device, nbytes)


def _locality(key):
    # (only the window-staged kernels of box attention with one query per pixel collect the counters;
    # everything else simply never sees a non-zero miss count)
    loc = _LOCALITY.get(key)
    if loc is None:
        loc = _Locality()
        # (a shape first met while the stream captures a graph: its entry would describe the capture alone -- a replay
        # runs no host code -- under a stream handle that is another stream's once this one is gone; like the state
        # buffer created with it, it serves this call and is not kept)
        if not torch.cuda.is_current_stream_capturing():
            _bounded(_LOCALITY)[key] = loc
    return loc


def _forward_train(name, value, shapes, lsi, loc, weights, dims, args):
    """*_fwd_train_*: forward + (when the binned backward applies) the backward's plan."""
    import ctypes
    lib = _lib.load()
    buf, sh, ls = _sized_buffer(lib.boxattn_plan_bytes, value, shapes, lsi, dims)
    built = ctypes.c_int(0)
    fn = getattr(lib, "%s_%s" % (name, _SUFFIX[value.dtype]))
    with _device_guard(value.device):
        stream = torch.cuda.current_stream(value.device).cuda_stream
        key, state = _state_for(lib, value, dims, sh, ls, stream)
        adapt = _locality(key)
        hints = adapt.hints()
        rc = fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args],
                sh.ctypes.data, ls.ctypes.data, buf.data_ptr() if buf is not None else 0,
                buf.numel() if buf is not None else 0, state.data_ptr(), state.numel(), hints | _fresh_hint(state),
                ctypes.addressof(built), stream)
        if rc == 0:
            state._boxattn_fresh = False
            adapt.after_call(state, hints)
            adapt.last_hints = hints
    if rc != 0:
        _STATE.pop(key, None)                                # (its tickets may not be zero any more)
        _LOCALITY.pop(key, None)
        raise RuntimeError("%s_%s failed with hipError %d" % (name, _SUFFIX[value.dtype], rc))
    if built.value:
        return BackwardPlan(buf, _plan_key(dims, loc, weights, value.dtype), hints)
    # no plan to hand over: the backward of this shape fills its bins in one pass from the ranges in the state buffer
    # (ABI 8), or plans for itself.  The object still carries the hints the forward ran with.
    return BackwardPlan(None, _plan_key(dims, loc, weights, value.dtype), hints)


def workspace_bytes(value, shapes, lsi, dims):
    """(plan bytes, backward workspace bytes) the library asks for at these dimensions."""
    lib = _lib.load()
    sh, ls = _host_table(shapes), _host_table(lsi)
    is_h16 = int(value.dtype in _H16)
    return (_query_bytes(lib.boxattn_plan_bytes, is_h16, tuple(dims), sh, ls),
            _query_bytes(lib.boxattn_bwd_workspace_bytes, is_h16, tuple(dims), sh, ls))


_WORKSPACE = {}      # (device index, stream handle) -> the backward's scratch tensor (grown as needed)


def _workspace(lib, value, dims, sh, ls, stream):
    """The backward's scratch (bin records, partial tiles: contents only live inside one call).  One tensor per
    (device, stream), reused: calls on a stream never overlap, and a 0.3 GB torch.empty per backward was a tenth
    of the host time of a training step."""
    nbytes = max(_query_bytes(lib.boxattn_bwd_workspace_bytes, int(value.dtype in _H16), dims, sh, ls), 256)
    wkey = (value.device.index, stream)
    ws = _WORKSPACE.get(wkey)
    # (a switch that changes the layouts -- group records: 285 -> 153 MB at C2 -- lets a cached buffer shrink too: a buffer
    # that is too large after the options epoch moved is dropped; within one epoch the largest shape's buffer stays)
    epoch = _lib.options_epoch()
    if ws is not None and _WORKSPACE_EPOCH.get(wkey) != epoch and ws.numel() > nbytes and \
            not torch.cuda.is_current_stream_capturing():
        ws = None
    _WORKSPACE_EPOCH[wkey] = epoch
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=value.device)
        # cached per (device, stream) unless the caller opted out (set_workspace_caching(False): the scratch is then
        # transient inside each backward, as in rounds 1-3) or the stream is capturing a graph (private pool)
        if _CACHE_WORKSPACE and not torch.cuda.is_current_stream_capturing():
            if len(_WORKSPACE) >= _WORKSPACE_CAP:          # streams come and go: start over rather than grow
                _WORKSPACE.clear()
                _WORKSPACE_EPOCH.clear()
            _WORKSPACE[wkey] = ws
    return ws


_CACHE_WORKSPACE = os.environ.get("BOXATTN_CACHE_WORKSPACE", "1") != "0"
_WORKSPACE_CAP = 64
_WORKSPACE_EPOCH = {}          # (device, stream) -> options epoch its cached workspace was last sized under


def set_workspace_caching(on):
    """Keep the backward's scratch (0.1-0.3 GB at BoxeR-R50 shapes) per (device, stream) for the life of the process
    (default: saves a torch.empty per backward, ~10 % of a step's host time) or allocate it inside every backward
    (off: it is then not resident during the forward, i.e. not part of the step's peak activation memory).
    Environment: BOXATTN_CACHE_WORKSPACE=0."""
    global _CACHE_WORKSPACE
    _CACHE_WORKSPACE = bool(on)
    if not on:
        _WORKSPACE.clear()


def release_workspaces():
    """Drop the cached scratch / state tensors and parked plans (they are re-created on demand)."""
    _WORKSPACE.clear()
    _STATE.clear()
    _LOCALITY.clear()
    _PARKED.clear()


# ---------------------------------------------------------------------------------------
# The reference's own four-function API with the training step's fast path.
#
# BoxeR's Functions call box_attn_forward, then -- in another call, with nothing but the saved tensors --
# box_attn_backward (box_attention_func.py:10-64).  When an input of the forward requires a gradient (the
# tensors keep that flag inside a Function's forward) the forward runs the *_fwd_train_* entry and PARKS the
# plan under (stream, dimensions, location / weight tensors' addresses and versions); the matching backward
# finds it there.  A backward without a parked plan plans for itself, as ever.  Bounded: a forward whose
# backward never comes (evaluation under enable_grad, a crashed step) is evicted, oldest first.
# ---------------------------------------------------------------------------------------
_PARKED = {}         # (device, stream handle, plan key) -> BackwardPlan, insertion-ordered
_PARK_CAP = 32       # plans alive between forward and backward: layers of a model x micro-batches
_PARK_PLANS = os.environ.get("BOXATTN_PARK_PLANS", "1") != "0"


def set_plan_parking(on):
    """box_attn_forward / instance_attn_forward called with inputs that require a gradient build the backward's plan
    and park it for the matching *_backward call (default) -- or do not (off: every forward is an inference forward,
    every backward plans for itself).  Environment: BOXATTN_PARK_PLANS=0."""
    global _PARK_PLANS
    _PARK_PLANS = bool(on)
    if not on:
        _PARKED.clear()


def _wants_plan(*tensors):
    return _PARK_PLANS and any(t.requires_grad for t in tensors)


def _park(value, plan, keep):
    if plan is None or plan.buf is None:
        return
    # The key names the location / weight tensors by address and version.  A parked plan HOLDS them: as long as it is
    # parked their memory cannot be freed and handed to another tensor, so a backward that presents the same
    # addresses and versions presents the same data.  (A plan handed over explicitly needs no such hold: the
    # Function's context keeps the tensors.)
    plan.keep = keep
    stream = torch.cuda.current_stream(value.device).cuda_stream
    while len(_PARKED) >= _PARK_CAP:
        _PARKED.pop(next(iter(_PARKED)))
    _PARKED[(value.device.index, stream) + plan.key] = plan


def _parked(value, dims, loc, weights):
    if not _PARKED:
        return None
    stream = torch.cuda.current_stream(value.device).cuda_stream
    plan = _PARKED.pop((value.device.index, stream) + _plan_key(dims, loc, weights, value.dtype), None)
    if plan is not None:
        plan.keep = None
    return plan


def _want_groups(want):
    """-> (grad_value wanted, location / weight gradients wanted) of a backward's ``want`` (BOXATTN_WANT_* bits)."""
    if want not in (_lib.WANT_VALUE, _lib.WANT_POINTS, _lib.WANT_ALL):
        raise ValueError("want must be 1 (grad_value), 2 (location and weight gradients) or 3 (all), not %r" % (want,))
    return bool(want & _lib.WANT_VALUE), bool(want & _lib.WANT_POINTS)


def _ptr(a):
    """What goes over the C ABI: tensors as device pointers, a gradient nobody wants (None) as NULL."""
    return a.data_ptr() if isinstance(a, torch.Tensor) else 0 if a is None else a


def _backward(name, value, shapes, lsi, loc, weights, dims, args, plan, want):
    """Run the *_bwd_part_* entry point (float32 / bfloat16 / float16) for the gradient groups ``want``; with all
    groups wanted it is the *_bwd_ws_* call.  The host work follows the route (include/boxattn.h):
    POINTS alone: one launch, no scratch, no state.  VALUE: scratch (+ the plan of a training forward).  Only the
    full call looks the state buffer up -- the record ranges of the one-pass fill live in it from call to call -- and
    answers for it: the fresh-state hint, and no reuse of a buffer whose call failed."""
    lib = _lib.load()
    full = want == _lib.WANT_ALL
    fn = getattr(lib, "%s_%s" % (name, _SUFFIX[value.dtype]))
    with _device_guard(value.device):
        stream = torch.cuda.current_stream(value.device).cuda_stream
        sh, ls = _host_table(shapes), _host_table(lsi)
        ws_ptr = ws_len = plan_ptr = plan_len = state_ptr = state_len = fresh = 0
        if want & _lib.WANT_VALUE:
            ws = _workspace(lib, value, dims, sh, ls, stream)
            ws_ptr, ws_len = ws.data_ptr(), ws.numel()
            if plan is not None and plan.buf is not None and plan.key == _plan_key(dims, loc, weights, value.dtype):
                plan_ptr, plan_len = plan.buf.data_ptr(), plan.buf.numel()
        if full:
            key, state = _state_for(lib, value, dims, sh, ls, stream)
            state_ptr, state_len, fresh = state.data_ptr(), state.numel(), _fresh_hint(state)
        if plan is not None:
            hints = plan.hints
        elif _LOCALITY:      # no plan: as the shape's last training forward ran
            adapt = _LOCALITY.get(key if full else _shape_key(value, stream, dims, sh, ls))
            hints = adapt.last_hints if adapt is not None else 0
        else:
            hints = 0
        # (the pointers inline, not through _ptr: sixteen calls are a microsecond of a host-bound decoder step)
        rc = fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else 0 if a is None else a for a in args],
                sh.ctypes.data, ls.ctypes.data, ws_ptr, ws_len, plan_ptr, plan_len,
                state_ptr, state_len, hints | fresh, stream, want)
    if rc != 0:
        if full:
            _STATE.pop(key, None)                                # (its ranges may be half written)
        raise RuntimeError("%s_%s (want=%d) failed with hipError %d" % (name, _SUFFIX[value.dtype], want, rc))
    if full:
        state._boxattn_fresh = False


def _call(name, value, *args, want=None):
    fn = getattr(_lib.load(), "%s_%s" % (name, _SUFFIX[value.dtype]))
    with torch.cuda.device(value.device):
        stream = torch.cuda.current_stream(value.device).cuda_stream
        rc = fn(*[_ptr(a) for a in args], stream, *(() if want is None else (want,)))
    if rc != 0:
        raise RuntimeError("%s_%s failed with hipError %d" % (name, _SUFFIX[value.dtype], rc))


def box_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                     im2col_step, park=True):
    """-> output (B, Lq, H*C).  Reference: box_attn_cuda_forward (box_attn.cu:15-71).
    ``park=False``: never the training forward, whatever requires a gradient (a caller that knows the backward
    will not need grad_value: the plan only serves that half)."""
    dims, loc, (attn,), _ = _prepare(value, spatial_shapes, level_start_index, sampling_loc,
                                     [attn_weight])
    B, S, H, C, L, Lq, P = dims
    _chunk_assert(B, im2col_step)
    out = torch.empty((B, Lq, H * C), dtype=value.dtype, device=value.device)
    if value.dtype == torch.float64:
        _call("boxattn_fwd", value, value, spatial_shapes, level_start_index, loc, attn, *dims, out)
    elif park and _wants_plan(value, sampling_loc, attn_weight):      # a backward will follow: build and park its plan
        _park(value, _forward_train("boxattn_fwd_train", value, spatial_shapes, level_start_index, loc,
                                    (attn,), dims,
                                    [value, spatial_shapes, level_start_index, loc, attn, *dims, out]), (loc, attn))
    else:       # host copies of the level tables let the library recognise the encoder case
        sh, ls = _host_table(spatial_shapes), _host_table(level_start_index)
        _call("boxattn_fwd_hl", value, value, spatial_shapes, level_start_index, loc, attn, *dims,
              out, sh.ctypes.data, ls.ctypes.data)
    return out


def forward_route(value, loc, shapes_host=None, lsi_host=None, instance=False):
    """Which forward kernel family (``_lib.FWD_*``) the library launches for these tensors under the current switches:
    ``boxattn_fwd_route`` with the dimensions, element size and alignment of ``value`` (B, S, H, C) and ``loc``
    (B, Lq, H, L, P, 2).  ``shapes_host`` / ``lsi_host``: the level tables as int64 numpy arrays (or tensors, copied
    to the host), as ``box_attn_forward`` hands them over; without them the answer is never window-staged.  The outputs
    are taken as freshly allocated (aligned)."""
    B, S, H, C = value.shape
    Lq, L, P = loc.size(1), loc.size(3), loc.size(4)
    host = lambda t: _host_table(t) if isinstance(t, torch.Tensor) else t
    ptrs = (value.data_ptr(), loc.data_ptr())
    aligned = 16 if all(p % 16 == 0 for p in ptrs) else 8 if all(p % 8 == 0 for p in ptrs) else 0
    return _lib.fwd_route(value.element_size(), instance, aligned, (B, S, H, C, L, Lq, P), host(shapes_host),
                          host(lsi_host))


def backward_accumulate_kind(value, loc, instance=False):
    """Which kernel (``_lib.ACC_*``) sums grad_value in a binned backward of these tensors under the current switches:
    ``boxattn_bwd_accumulate_kind`` with the dimensions and element size of ``value`` (B, S, H, C) and ``loc``
    (B, Lq, H, L, P, 2).  Negative for float64.  (A 16-bit instance-attention call whose ``grad_mask_output`` is not
    16-byte aligned takes the VALU walk whatever this answers: the query sees no gradients.)"""
    B, S, H, C = value.shape
    Lq, L, P = loc.size(1), loc.size(3), loc.size(4)
    return _lib.bwd_accumulate_kind(value.element_size(), instance, (B, S, H, C, L, Lq, P))


def backward_record_kind(value, loc, instance=False):
    """Which records (``_lib.REC_*``) a binned backward of these tensors writes under the current switches:
    ``boxattn_bwd_record_kind`` with the dimensions and element size of ``value`` (B, S, H, C) and ``loc``
    (B, Lq, H, L, P, 2).  Negative for float64.  (A call whose ``loc`` or attention weights are not 16-byte aligned
    keeps point records whatever this answers.)"""
    B, S, H, C = value.shape
    Lq, L, P = loc.size(1), loc.size(3), loc.size(4)
    return _lib.bwd_record_kind(value.element_size(), instance, (B, S, H, C, L, Lq, P))


def box_attn_forward_train(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                           im2col_step):
    """Forward for training: -> (output, plan).  ``plan`` (or None) goes to
    ``box_attn_backward(..., plan=plan)``: the forward's launch already counted and scanned the
    destination bins of the sample points for the backward.  Not part of the reference API."""
    dims, loc, (attn,), _ = _prepare(value, spatial_shapes, level_start_index, sampling_loc,
                                     [attn_weight])
    B, S, H, C, L, Lq, P = dims
    _chunk_assert(B, im2col_step)
    out = torch.empty((B, Lq, H * C), dtype=value.dtype, device=value.device)
    if value.dtype == torch.float64:
        _call("boxattn_fwd", value, value, spatial_shapes, level_start_index, loc, attn, *dims, out)
        return out, None
    plan = _forward_train("boxattn_fwd_train", value, spatial_shapes, level_start_index, loc,
                          (attn,), dims,
                          [value, spatial_shapes, level_start_index, loc, attn, *dims, out])
    return out, plan


def box_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                      grad_output, im2col_step, plan=None, want=3):
    """-> [grad_value, grad_sampling_loc, grad_attn_weight] (box_attn.cu:74-135).
    For bfloat16 / float16 ``value`` the location / weight gradients are float32.
    ``want``: the gradient groups to compute -- 1 grad_value, 2 the location and weight gradients, 3 (default) all.
    The entries of a group that is not wanted are None: never allocated, never computed (include/boxattn.h,
    *_bwd_part_*)."""
    want_value, want_points = (True, True) if want == 3 else _want_groups(want)
    dims, loc, (attn,), cdt = _prepare(value, spatial_shapes, level_start_index, sampling_loc,
                                       [attn_weight], [("grad_output", grad_output)])
    B, S, H, C, L, Lq, P = dims
    _chunk_assert(B, im2col_step)
    if grad_output.numel() != B * Lq * H * C:
        raise RuntimeError("grad_output must have B*Lq*H*C elements")
    grad_value = torch.empty_like(value) if want_value else None
    grad_loc = torch.empty(sampling_loc.shape, dtype=cdt, device=value.device) if want_points else None
    grad_attn = torch.empty(attn_weight.shape, dtype=cdt, device=value.device) if want_points else None
    args = [value, spatial_shapes, level_start_index, loc, attn, grad_output, *dims, grad_value,
            grad_loc, grad_attn]
    if value.dtype == torch.float64:
        _call("boxattn_bwd_part", value, *args, want=want)
    else:
        # (a plan parked for this call leaves the table whether or not the call has a use for it -- only the
        # grad_value half has: the table must not keep its tensors alive)
        if plan is None:
            plan = _parked(value, dims, loc, (attn,))
        _backward("boxattn_bwd_part", value, spatial_shapes, level_start_index, loc, (attn,), dims, args, plan, want)
    return [grad_value, grad_loc, grad_attn]


def instance_attn_forward(value, spatial_shapes, level_start_index, sampling_loc,
                          spatial_attn_weight, level_attn_weight, im2col_step, park=True):
    """-> [output (B,Lq,H*C), mask_output (B,Lq,P,H*C)] (instance_attn.cu:15-82).  ``park``: see box_attn_forward."""
    dims, loc, (sw, lw), _ = _prepare(value, spatial_shapes, level_start_index, sampling_loc,
                                      [spatial_attn_weight, level_attn_weight])
    B, S, H, C, L, Lq, P = dims
    _chunk_assert(B, im2col_step)
    out = torch.empty((B, Lq, H * C), dtype=value.dtype, device=value.device)
    mask = torch.empty((B, Lq, P, H * C), dtype=value.dtype, device=value.device)
    if value.dtype != torch.float64 and park and _wants_plan(value, sampling_loc, spatial_attn_weight,
                                                             level_attn_weight):
        _park(value, _forward_train("instattn_fwd_train", value, spatial_shapes, level_start_index, loc,
                                    (sw, lw), dims,
                                    [value, spatial_shapes, level_start_index, loc, sw, lw, *dims, out, mask]),
              (loc, sw, lw))
    else:
        _call("instattn_fwd", value, value, spatial_shapes, level_start_index, loc, sw, lw, *dims,
              out, mask)
    return [out, mask]


def instance_attn_forward_train(value, spatial_shapes, level_start_index, sampling_loc,
                                spatial_attn_weight, level_attn_weight, im2col_step):
    """-> ([output, mask_output], plan); see box_attn_forward_train."""
    dims, loc, (sw, lw), _ = _prepare(value, spatial_shapes, level_start_index, sampling_loc,
                                      [spatial_attn_weight, level_attn_weight])
    B, S, H, C, L, Lq, P = dims
    _chunk_assert(B, im2col_step)
    out = torch.empty((B, Lq, H * C), dtype=value.dtype, device=value.device)
    mask = torch.empty((B, Lq, P, H * C), dtype=value.dtype, device=value.device)
    args = [value, spatial_shapes, level_start_index, loc, sw, lw, *dims, out, mask]
    if value.dtype == torch.float64:
        _call("instattn_fwd", value, *args)
        return [out, mask], None
    plan = _forward_train("instattn_fwd_train", value, spatial_shapes, level_start_index, loc,
                          (sw, lw), dims, args)
    return [out, mask], plan


def instance_attn_backward(value, spatial_shapes, level_start_index, sampling_loc,
                           spatial_attn_weight, level_attn_weight, grad_output,
                           grad_mask_output, im2col_step, plan=None, want=3):
    """-> [grad_value, grad_sampling_loc, grad_spatial_attn_weight, grad_level_attn_weight]
    (instance_attn.cu:85-157).  ``want``: see box_attn_backward."""
    want_value, want_points = (True, True) if want == 3 else _want_groups(want)
    dims, loc, (sw, lw), cdt = _prepare(
        value, spatial_shapes, level_start_index, sampling_loc,
        [spatial_attn_weight, level_attn_weight],
        [("grad_output", grad_output), ("grad_mask_output", grad_mask_output)])
    B, S, H, C, L, Lq, P = dims
    _chunk_assert(B, im2col_step)
    if grad_output.numel() != B * Lq * H * C or grad_mask_output.numel() != B * Lq * P * H * C:
        raise RuntimeError("grad_output / grad_mask_output have the wrong number of elements")
    new = lambda like: torch.empty(like.shape, dtype=cdt, device=value.device) if want_points else None
    grad_value = torch.empty_like(value) if want_value else None
    grad_loc, grad_sw, grad_lw = new(sampling_loc), new(spatial_attn_weight), new(level_attn_weight)
    args = [value, spatial_shapes, level_start_index, loc, sw, lw, grad_output, grad_mask_output,
            *dims, grad_value, grad_loc, grad_sw, grad_lw]
    if value.dtype == torch.float64:
        _call("instattn_bwd_part", value, *args, want=want)
    else:
        if plan is None:
            plan = _parked(value, dims, loc, (sw, lw))
        _backward("instattn_bwd_part", value, spatial_shapes, level_start_index, loc, (sw, lw), dims, args, plan, want)
    return [grad_value, grad_loc, grad_sw, grad_lw]


# ---------------------------------------------------------------------------------------
# reference windows + box offsets -> sampling grid (opt-in, beyond the reference's native
# module)
# ---------------------------------------------------------------------------------------
def _grid_args(ref_windows, offsets, kernel_indices, valid_ratios, angle_mode):
    _check(ref_windows, "ref_windows")
    _check(offsets, "offsets")
    _check(kernel_indices, "kernel_indices")
    for t in (ref_windows, offsets, kernel_indices):
        if t.dtype != torch.float32:
            raise RuntimeError("box_grid: float32 tensors expected")
    if offsets.dim() != 5 or ref_windows.dim() not in (3, 4):
        raise RuntimeError("expected offsets (B,Lq,H,L,V) and ref_windows (B,Lq,D) or (B,Lq,H,D)")
    if kernel_indices.dim() != 2 or kernel_indices.size(1) != 2:
        raise RuntimeError("expected kernel_indices (P,2)")
    B, Lq, H, L, V = offsets.shape
    per_head = ref_windows.dim() == 4
    D = ref_windows.size(-1)
    if tuple(ref_windows.shape[:2]) != (B, Lq) or (per_head and ref_windows.size(2) != H):
        raise RuntimeError("ref_windows do not match offsets")
    if angle_mode not in (0, 1, 2) or V != (5 if angle_mode == 1 else 4) or \
            D < (5 if angle_mode else 4):
        raise RuntimeError("box_grid: offsets / ref_windows do not fit angle_mode %r" % angle_mode)
    if valid_ratios is not None:
        _check(valid_ratios, "valid_ratios")
        if valid_ratios.dtype != torch.float32 or valid_ratios.numel() != B * L * 2:
            raise RuntimeError("expected valid_ratios with B*L*2 float32 elements")
    return (B, Lq, H, L, kernel_indices.size(0)), (D, int(per_head), V, angle_mode)


def _grid_call(name, anchor, *args):
    fn = getattr(_lib.load(), name)
    with torch.cuda.device(anchor.device):
        stream = torch.cuda.current_stream(anchor.device).cuda_stream
        rc = fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], stream)
    if rc != 0:
        raise RuntimeError("%s failed with hipError %d" % (name, rc))


def box_grid_forward(ref_windows, offsets, kernel_indices, valid_ratios=None, angle_mode=0):
    """Everything of the modules' ``_where_to_attend`` after the offset projection
    (box_attention.py:63-81, 304-338) in one kernel:
    ``box = ref[:4] + offsets[:4]/8 * (w,h,w,h)_ref``; rotation ``theta`` none (angle_mode 0),
    ``(ref[4] + offsets[4]/16) * 2 pi`` (1) or ``ref[4]`` (2);
    ``grid = (c + R(theta)(kernel_indices * relu(size))) * valid_ratios`` -> (B,Lq,H,L,P,2)."""
    dims, (D, per_head, V, mode) = _grid_args(ref_windows, offsets, kernel_indices, valid_ratios,
                                              angle_mode)
    B, Lq, H, L, P = dims
    grid = torch.empty((B, Lq, H, L, P, 2), dtype=torch.float32, device=offsets.device)
    _grid_call("boxattn_grid_fwd_f32", offsets, ref_windows, D, per_head, offsets, V, mode,
               kernel_indices, valid_ratios if valid_ratios is not None else 0, *dims, grid)
    return grid


def box_grid_backward(ref_windows, offsets, kernel_indices, valid_ratios, angle_mode, grad_grid,
                      need_ref_grad=False):
    """-> (grad_offsets (B,Lq,H,L,V), grad_ref_rows (B,Lq,H,L,5) or None)."""
    dims, (D, per_head, V, mode) = _grid_args(ref_windows, offsets, kernel_indices, valid_ratios,
                                              angle_mode)
    B, Lq, H, L, P = dims
    _check(grad_grid, "grad_grid")
    if grad_grid.dtype != torch.float32 or grad_grid.numel() != B * Lq * H * L * P * 2:
        raise RuntimeError("expected grad_grid (B,Lq,H,L,P,2) float32")
    grad_offsets = torch.empty_like(offsets)
    grad_rows = torch.empty((B, Lq, H, L, 5), dtype=torch.float32, device=offsets.device) \
        if need_ref_grad else None
    _grid_call("boxattn_grid_bwd_f32", offsets, ref_windows, D, per_head, offsets, V, mode,
               kernel_indices, valid_ratios if valid_ratios is not None else 0, grad_grid, *dims,
               grad_offsets, grad_rows if grad_rows is not None else 0)
    return grad_offsets, grad_rows


# ---------------------------------------------------------------------------------------
# pointwise work around the operator (opt-in)
# ---------------------------------------------------------------------------------------
def _pw_suffix(t, what):
    if t.dtype == torch.float32:
        return "f32"
    if t.dtype == torch.bfloat16:
        return "bf16"
    if t.dtype == torch.float16:
        return "f16"
    raise RuntimeError("%s: float32, bfloat16 or float16 expected, got %s" % (what, t.dtype))


def softmax_forward(logits):
    """softmax over the last axis (the L*P logits of a (query, head); at most 64) of float32 /
    bfloat16 / float16 ``logits`` -> float32 weights, one pass (box_attention.py:227-229)."""
    _check(logits, "logits")
    n = logits.size(-1)
    rows = logits.numel() // max(n, 1)
    attn = torch.empty(logits.shape, dtype=torch.float32, device=logits.device)
    _grid_call("boxattn_softmax_fwd_" + _pw_suffix(logits, "logits"), logits, logits, rows, n, attn)
    return attn


def softmax_backward(attn, grad_attn, dtype):
    """-> grad_logits = attn * (grad_attn - sum(attn * grad_attn)) in ``dtype``."""
    _check(attn, "attn")
    _check(grad_attn, "grad_attn")
    if attn.dtype != torch.float32 or grad_attn.dtype != torch.float32 or attn.shape != grad_attn.shape:
        raise RuntimeError("softmax_backward: float32 attn / grad_attn of one shape expected")
    out = torch.empty(attn.shape, dtype=dtype, device=attn.device)
    n = attn.size(-1)
    _grid_call("boxattn_softmax_bwd_" + _pw_suffix(out, "grad_logits"), attn, attn, grad_attn,
               attn.numel() // max(n, 1), n, out)
    return out


def value_mask_cast(value, v_mask, dtype=torch.bfloat16):
    """(B, S, d) float32 / ``dtype`` -> ``dtype`` (bfloat16 or float16) with the rows of padded pixels
    (``v_mask`` (B, S) bool, or None) zeroed, one pass (box_attention.py:223-225 + the op's 16-bit
    conversion)."""
    _check(value, "value")
    d = value.size(-1)
    rows = value.numel() // max(d, 1)
    mask = 0
    if v_mask is not None:
        _check(v_mask, "v_mask")
        if v_mask.dtype != torch.bool or v_mask.numel() != rows:
            raise RuntimeError("v_mask must be a bool tensor with one entry per value row")
        mask = v_mask
    if dtype not in _H16:
        raise RuntimeError("value_mask_cast: bfloat16 or float16 output expected, got %s" % dtype)
    if value.dtype != torch.float32 and value.dtype != dtype:
        raise RuntimeError("value_mask_cast: float32 or %s value expected, got %s" % (dtype, value.dtype))
    out = torch.empty(value.shape, dtype=dtype, device=value.device)
    # entry points: value_prep_{f32, bf16} write bf16; value_prep_{f32_f16, f16} write f16
    suffix = _pw_suffix(value, "value") + ("_f16" if dtype == torch.float16 and value.dtype == torch.float32 else "")
    _grid_call("boxattn_value_prep_" + suffix, value, value, mask, rows, d, out)
    return out


def _inst_logits(logits):
    """-> (rows, L) of (..., L, 2, 2) logits."""
    _check(logits, "logits")
    if logits.dim() < 3 or tuple(logits.shape[-2:]) != (2, 2):
        raise RuntimeError("expected logits (..., L, 2, 2), got %s" % (tuple(logits.shape),))
    L = logits.size(-3)
    return logits.numel() // max(4 * L, 1), L


def _aligned16(t):
    """The (..., L, k, k) tensors are accessed 16 bytes at a time: a view into the middle of a storage is copied."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def instance_weights_forward(logits, kernel_size, need_level=True):
    """InstanceAttention's weights from its 2x2 logits per level, one pass (box_attention.py:100-121):
    ``logits`` (..., L, 2, 2) float32 / bfloat16 / float16 -> ``spatial_w`` = softmax over the L*k*k logits
    replicated to k x k, and ``level_w`` = their softmax over L (None unless ``need_level``), each
    (..., L, k, k) float32.  ``kernel_size`` even, 2 ... 32; L <= 16."""
    rows, L = _inst_logits(logits)
    k = int(kernel_size)
    shape = tuple(logits.shape[:-2]) + (max(k, 0), max(k, 0))
    spatial = torch.empty(shape, dtype=torch.float32, device=logits.device)
    level = torch.empty(shape, dtype=torch.float32, device=logits.device) if need_level else None
    _grid_call("instattn_weights_fwd_" + _pw_suffix(logits, "logits"), logits, logits, rows, L, k, spatial,
               level if need_level else 0)
    return spatial, level


def instance_weights_backward(logits, grad_spatial, grad_level=None):
    """-> grad_logits in the logits' type from the logits and the float32 gradients of the two outputs of
    ``instance_weights_forward`` (either may be None: zeros): the closed form of include/boxattn.h, nothing of the
    forward is needed."""
    rows, L = _inst_logits(logits)
    given = [g for g in (grad_spatial, grad_level) if g is not None]
    if not given:
        raise RuntimeError("instance_weights_backward: at least one gradient expected")
    k = given[0].size(-1)
    for g in given:
        _check(g, "grad")
        if g.dtype != torch.float32 or tuple(g.shape) != tuple(logits.shape[:-2]) + (k, k):
            raise RuntimeError("instance_weights_backward: float32 gradients (..., L, k, k) matching the logits "
                               "expected")
    out = torch.empty_like(logits)
    _grid_call("instattn_weights_bwd_" + _pw_suffix(logits, "logits"), logits, logits,
               _aligned16(grad_spatial) if grad_spatial is not None else 0,
               _aligned16(grad_level) if grad_level is not None else 0, rows, L, k, out)
    return out


# ---------------------------------------------------------------------------------------
# instance attention at inference straight from boxes and 2x2 logits (opt-in; SURVEY.md 8(f) N1 + N3 inside the
# operator: include/boxattn.h, instattn_fwd_boxes_*)
# ---------------------------------------------------------------------------------------
def _align_of(*tensors):
    low = 0
    for t in tensors:
        low |= t.data_ptr()             # (the low bits of every address at once)
    return 16 if low % 16 == 0 else 8 if low % 8 == 0 else 0


def _boxes_operands(what, exc, kernel_size, operands, angle_mode=0, also=()):
    """The argument checks the four calls from boxes share.  ``operands``: value, spatial_shapes, level_start_index,
    ref_windows, offsets, kernel_indices, valid_ratios, logits; ``also``: (tensor, name) pairs checked with them;
    ``kernel_size``: the instance calls, logits (B,Lq,H,L,2,2) and kernel_size**2 points a level; None: the box calls,
    B*Lq*H*L*P logits -> (B, S, H, C, L, Lq, P), (D, per_head, V, mode), k (None: the box calls).  Raises ``exc``:
    RuntimeError with the bare texts (the instance calls), or ValueError with ``what`` in front (the box calls); a
    non-Tensor is a TypeError for both."""
    value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios, logits = operands
    try:
        (B, Lq, H, L, P), grid = _grid_args(ref_windows, offsets, kernel_indices, valid_ratios, angle_mode)
        _check(value, "value")
        _check(spatial_shapes, "spatial_shapes")
        _check(level_start_index, "level_start_index")
        _check(logits, "logits")
        for t, name in also:
            _check(t, name)
    except RuntimeError as e:
        raise _boxes_refusal(what, exc, str(e)) from None
    k = None if kernel_size is None else int(kernel_size)
    if value.dtype not in _BOXES_DTYPES:
        raise exc("%s: float32, bfloat16 or float16 value expected, got %s" % (what, value.dtype))
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise _boxes_refusal(what, exc, "spatial_shapes / level_start_index must be int64")
    if k is not None:
        if logits.dtype != torch.float32 or tuple(logits.shape) != (B, Lq, H, L, 2, 2):
            raise _boxes_refusal(what, exc, "expected logits (B,Lq,H,L,2,2) float32 matching offsets")
    elif logits.dtype != torch.float32 or logits.numel() != B * Lq * H * L * P:
        raise _boxes_refusal(what, exc, "expected B*Lq*H*L*P float32 logits matching offsets")
    if value.dim() != 4 or value.size(0) != B or value.size(2) != H or spatial_shapes.size(0) != L or \
            level_start_index.numel() != L:
        raise _boxes_refusal(what, exc, "offsets / spatial_shapes do not match value (B,S,H,C)")
    if k is not None and P != k * k:
        raise _boxes_refusal(what, exc, "kernel_indices must have kernel_size**2 rows")
    return (B, value.size(1), H, value.size(3), L, Lq, P), grid, k


def _boxes_refusal(what, exc, text):
    """The exception of a call from boxes: the box calls' ValueError carries the function's name in front."""
    return exc("%s: %s" % (what, text) if exc is ValueError else text)


def _boxes_upstream(what, exc, value, grads):
    """The upstream gradients of a backward from boxes, (name, tensor, elements) each: in the type of ``value``."""
    for name, g, n in grads:
        try:
            _check(g, name)
        except RuntimeError as e:
            raise _boxes_refusal(what, exc, str(e)) from None
        if g.dtype != value.dtype or g.numel() != n:
            raise _boxes_refusal(what, exc, "%s: %d elements of type %s expected" % (name, n, value.dtype))


def _boxes_ok(query, value, dims, *points, also=()):
    """The one body of the four ``*_boxes_ok``: ``query`` of _lib at the element size of ``value`` (B, S, H, C), the
    alignment of ``value`` and ``also``, and (B, S, H, C) + ``dims`` (+ ``points``)."""
    if not isinstance(value, torch.Tensor) or value.dim() != 4 or value.dtype not in _BOXES_DTYPES:
        return False
    return query(value.element_size(), _align_of(value, *also), (*value.shape, *dims), *points)


def _boxes_call(stem, operands, window, angle, upstream, dims, outputs):
    """``stem`` + the suffix of value's type: the operands with ``window`` = (D, per_head) and ``angle`` = (V, mode) (the
    box calls) or () in their places, the upstream gradients, the dimensions and the outputs; None: an optional tensor
    that is absent (ctypes passes it as a NULL pointer)."""
    value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios, logits = operands
    _grid_call(stem + _SUFFIX[value.dtype], value, value, spatial_shapes, level_start_index, ref_windows, *window,
               offsets, *angle, kernel_indices, valid_ratios, logits, *upstream, *dims, *outputs)


def _boxes_grads(value, rows, V, logits_shape, need_ref_grad):
    """The outputs of a backward from boxes for ``rows`` = (B, Lq, H, L) -> (grad_offsets, grad_ref_rows or None,
    grad_logits), float32."""
    f32 = {"dtype": torch.float32, "device": value.device}
    return (torch.empty((*rows, V), **f32), torch.empty((*rows, 5), **f32) if need_ref_grad else None,
            torch.empty(logits_shape, **f32))


def forward_boxes_ok(value, num_level, num_query, kernel_size):
    """Whether ``instance_attn_forward_boxes`` has its kernel under the current switches: ``instattn_fwd_boxes_ok``
    with the dimensions, element size and alignment of ``value`` (B, S, H, C), ``num_level`` levels, ``num_query``
    queries an image and ``kernel_size`` x ``kernel_size`` points a level.  The outputs are taken as freshly
    allocated (aligned).  Pure host code."""
    return _boxes_ok(_lib.fwd_boxes_ok, value, (num_level, num_query), kernel_size)


def instance_attn_forward_boxes(value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices,
                                valid_ratios, logits, kernel_size, need_mask=True):
    """InstanceAttention's inference forward in one launch, from what the module predicts:
    ``value`` (B,S,H,C) float32 / bfloat16 / float16, ``ref_windows`` (B,Lq,D) or (B,Lq,H,D), ``offsets``
    (B,Lq,H,L,4), ``kernel_indices`` (k*k,2), ``valid_ratios`` None or B*L*2 values, ``logits`` (B,Lq,H,L,2,2) -- all
    float32 but ``value`` -> ``(output (B,Lq,H*C), mask_output (B,Lq,k*k,H*C) or None)`` in the type of ``value``:
    what ``box_grid_forward`` -> ``instance_weights_forward`` -> ``instance_attn_forward`` (``need_mask``) or
    ``box_attn_forward`` on the spatial weights (not ``need_mask``) return, without the per-point tensors in
    between.  No backward here (``instance_attn_backward_boxes``).  Raises where ``forward_boxes_ok`` says no: there
    is no other kernel behind it."""
    operands = (value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios, logits)
    (B, S, H, C, L, Lq, P), (D, per_head, _, _), k = _boxes_operands("instance_attn_forward_boxes", RuntimeError,
                                                                     kernel_size, operands)
    if not _boxes_ok(_lib.fwd_boxes_ok, value, (L, Lq), k):
        raise RuntimeError("instance_attn_forward_boxes: no kernel for value %s, %d levels, %d queries, kernel_size %d "
                           "(forward_boxes_ok)" % (tuple(value.shape), L, Lq, k))
    out = torch.empty((B, Lq, H * C), dtype=value.dtype, device=value.device)
    mask = torch.empty((B, Lq, P, H * C), dtype=value.dtype, device=value.device) if need_mask else None
    _boxes_call("instattn_fwd_boxes_", operands, (D, per_head), (), (), (B, S, H, C, L, Lq, k), (out, mask))
    return out, mask


def backward_boxes_ok(value, num_level, num_query, kernel_size):
    """Whether ``instance_attn_backward_boxes`` has its kernel under the current switches: ``instattn_bwd_boxes_ok``
    (the eligibility of ``forward_boxes_ok``) with the dimensions, element size and alignment of ``value`` (B, S, H,
    C).  The upstream gradients are taken as aligned like ``value``; ``instance_attn_backward_boxes`` asks again with
    their addresses.  Pure host code."""
    return _boxes_ok(_lib.bwd_boxes_ok, value, (num_level, num_query), kernel_size)


def instance_attn_backward_boxes(value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices,
                                 valid_ratios, logits, kernel_size, grad_output, grad_mask_output, need_ref_grad=False):
    """The box and logit gradients of InstanceAttention's training step in one launch, from the operands of
    ``instance_attn_forward_boxes`` and the upstream gradients ``grad_output`` (B,Lq,H*C) and ``grad_mask_output``
    (B,Lq,k*k,H*C), or None where the mask output took no part in the loss, both in the type of ``value`` ->
    ``(grad_offsets (B,Lq,H,L,4), grad_ref_rows (B,Lq,H,L,5) or None, grad_logits (B,Lq,H,L,2,2))``, float32: what
    ``instance_attn_backward(want=2)`` -> ``box_grid_backward`` + ``instance_weights_backward`` return, without the
    per-point tensors in between.  ``grad_value`` is not computed.  Raises where ``backward_boxes_ok`` says no:
    there is no other kernel behind it."""
    operands = (value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios, logits)
    (B, S, H, C, L, Lq, P), (D, per_head, _, _), k = _boxes_operands("instance_attn_backward_boxes", RuntimeError,
                                                                     kernel_size, operands)
    upstream = [("grad_output", grad_output, B * Lq * H * C)]
    if grad_mask_output is not None:
        upstream.append(("grad_mask_output", grad_mask_output, B * Lq * P * H * C))
    _boxes_upstream("instance_attn_backward_boxes", RuntimeError, value, upstream)
    if not _boxes_ok(_lib.bwd_boxes_ok, value, (L, Lq), k, also=[g for _, g, _ in upstream]):
        raise RuntimeError("instance_attn_backward_boxes: no kernel for value %s, %d levels, %d queries, kernel_size "
                           "%d at the alignment of value and the gradients (backward_boxes_ok)"
                           % (tuple(value.shape), L, Lq, k))
    grads = _boxes_grads(value, (B, Lq, H, L), 4, (B, Lq, H, L, 2, 2), need_ref_grad)
    _boxes_call("instattn_bwd_boxes_", operands, (D, per_head), (), (grad_output, grad_mask_output),
                (B, S, H, C, L, Lq, k), grads)
    return grads


# ---------------------------------------------------------------------------------------
# box attention at inference straight from boxes and L*P logits (opt-in; SURVEY.md 8(f) N1 + N3 inside the operator:
# include/boxattn.h, boxattn_fwd_boxes_*)
# ---------------------------------------------------------------------------------------
def box_forward_boxes_ok(value, num_level, num_query, num_point):
    """Whether ``box_attn_forward_boxes`` has its kernel under the current switches: ``boxattn_fwd_boxes_ok`` with the
    dimensions, element size and alignment of ``value`` (B, S, H, C), ``num_level`` levels, ``num_query`` queries an
    image and ``num_point`` points a level.  The output is taken as freshly allocated (aligned).  Pure host code."""
    return _boxes_ok(_lib.box_fwd_boxes_ok, value, (num_level, num_query, num_point))


def box_attn_forward_boxes(value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices,
                           valid_ratios, logits, angle_mode=0):
    """BoxAttention's / Box3dAttention's inference forward in one launch, from what the module predicts: ``value``
    (B,S,H,C) float32 / bfloat16 / float16, ``ref_windows`` (B,Lq,D) or (B,Lq,H,D), ``offsets`` (B,Lq,H,L,V) with V = 5
    for ``angle_mode`` 1 and 4 otherwise, ``kernel_indices`` (P,2), ``valid_ratios`` None or B*L*2 values, ``logits``
    B*Lq*H*L*P values -- all float32 but ``value`` -> ``output`` (B,Lq,H*C) in the type of ``value``: what
    ``box_grid_forward`` -> ``softmax_forward`` -> ``box_attn_forward`` return, without the sampling grid and the
    weights in between.  No backward.  Raises ValueError, before any device call, for arguments that do not fit and
    where ``box_forward_boxes_ok`` says no: there is no other kernel behind it."""
    operands = (value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios, logits)
    dims, (D, per_head, V, mode), _ = _boxes_operands("box_attn_forward_boxes", ValueError, None, operands, angle_mode)
    B, _, H, C, L, Lq, P = dims
    if not _boxes_ok(_lib.box_fwd_boxes_ok, value, (L, Lq, P)):
        raise ValueError("box_attn_forward_boxes: no kernel for value %s, %d levels, %d queries, %d points a level "
                         "(box_forward_boxes_ok)" % (tuple(value.shape), L, Lq, P))
    out = torch.empty((B, Lq, H * C), dtype=value.dtype, device=value.device)
    _boxes_call("boxattn_fwd_boxes_", operands, (D, per_head), (V, mode), (), dims, (out,))
    return out


# ---------------------------------------------------------------------------------------
# ... for the encoder case on the window-staged forward (opt-in; include/boxattn.h, boxattn_fwd_boxes_hl_*)
# ---------------------------------------------------------------------------------------
def _host_tables_ok(spatial_shapes, level_start_index):
    """Whether the two level tables are what ``_host_table`` copies for the staged calls from boxes."""
    return (isinstance(spatial_shapes, torch.Tensor) and isinstance(level_start_index, torch.Tensor) and
            spatial_shapes.dtype == torch.int64 and level_start_index.dtype == torch.int64 and
            spatial_shapes.dim() == 2 and spatial_shapes.size(1) == 2 and
            level_start_index.numel() == spatial_shapes.size(0))


def box_forward_boxes_staged_ok(value, spatial_shapes, level_start_index, num_query, num_point):
    """Whether ``box_attn_forward_boxes_staged`` has its kernel under the current switches: ``boxattn_fwd_boxes_hl_ok``
    with the dimensions, element size and alignment of ``value`` (B, S, H, C), the host copies of the level tables
    ``spatial_shapes`` (L, 2) / ``level_start_index`` (L) (``_host_table``: the first call with a tensor synchronises),
    ``num_query`` queries an image and ``num_point`` points a level -- the encoder case: one query per pixel, C = 32,
    2x2 points, at most 4 levels.  The output is taken as freshly allocated (aligned).  Otherwise pure host code."""
    if not _host_tables_ok(spatial_shapes, level_start_index):
        return False
    sh, ls = _host_table(spatial_shapes), _host_table(level_start_index)
    return _boxes_ok(lambda elem, aligned, dims: _lib.box_fwd_boxes_hl_ok(elem, aligned, dims, sh, ls), value,
                     (spatial_shapes.size(0), num_query, num_point))


def box_attn_forward_boxes_staged(value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices,
                                  valid_ratios, logits, angle_mode=0):
    """``box_attn_forward_boxes`` -- the same operands, the same result up to the order of the float32 sums -- for the
    encoder case (one query per pixel, C = 32, 2x2 points, at most 4 levels) on the window-staged forward: the kernels
    of ``box_attn_forward``'s encoder route, the locations and weights made inside them from the boxes and logits.  The
    level tables are also read on the host (``_host_table``).  No backward.  Raises ValueError, before any device
    call, for arguments that do not fit and where ``box_forward_boxes_staged_ok`` says no: there is no other kernel
    behind it."""
    operands = (value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios, logits)
    dims, (D, per_head, V, mode), _ = _boxes_operands("box_attn_forward_boxes_staged", ValueError, None, operands,
                                                      angle_mode)
    B, _, H, C, L, Lq, P = dims
    if not box_forward_boxes_staged_ok(value, spatial_shapes, level_start_index, Lq, P):
        raise ValueError("box_attn_forward_boxes_staged: no kernel for value %s, %d levels, %d queries, %d points a "
                         "level (box_forward_boxes_staged_ok)" % (tuple(value.shape), L, Lq, P))
    sh, ls = _host_table(spatial_shapes), _host_table(level_start_index)
    out = torch.empty((B, Lq, H * C), dtype=value.dtype, device=value.device)
    _boxes_call("boxattn_fwd_boxes_hl_", operands, (D, per_head), (V, mode), (), dims,
                (out, sh.ctypes.data, ls.ctypes.data))
    return out


# ---------------------------------------------------------------------------------------
# box attention's training step from the same operands (opt-in; include/boxattn.h, boxattn_bwd_boxes_*)
# ---------------------------------------------------------------------------------------
def box_backward_boxes_ok(value, num_level, num_query, num_point):
    """Whether ``box_attn_backward_boxes`` has its kernel under the current switches: ``boxattn_bwd_boxes_ok`` (the
    eligibility of ``box_forward_boxes_ok``) with the dimensions, element size and alignment of ``value`` (B, S, H,
    C).  The upstream gradient is taken as aligned like ``value``; ``box_attn_backward_boxes`` asks again with its
    address.  Pure host code."""
    return _boxes_ok(_lib.box_bwd_boxes_ok, value, (num_level, num_query, num_point))


def box_attn_backward_boxes(value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices,
                            valid_ratios, logits, angle_mode, grad_output, need_ref_grad=False):
    """The box and logit gradients of BoxAttention's / Box3dAttention's training step in one launch, from the operands
    of ``box_attn_forward_boxes`` and the upstream gradient ``grad_output`` (B,Lq,H*C) in the type of ``value`` ->
    ``(grad_offsets (B,Lq,H,L,V), grad_ref_rows (B,Lq,H,L,5) or None, grad_logits (B,Lq,H,L*P))``, float32: what
    ``box_attn_backward(want=2)`` -> ``box_grid_backward`` + ``softmax_backward`` return, without the sampling grid, the
    weights and their per-point gradients in between.  ``grad_value`` is not computed.  Raises ValueError, before any
    device call, for arguments that do not fit and where ``boxattn_bwd_boxes_ok`` says no at the alignment of
    ``value`` and ``grad_output``: there is no other kernel behind it."""
    what = "box_attn_backward_boxes"
    operands = (value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios, logits)
    # (grad_output: checked with the operands, before their types)
    dims, (D, per_head, V, mode), _ = _boxes_operands(what, ValueError, None, operands, angle_mode,
                                                      also=[(grad_output, "grad_output")])
    B, _, H, C, L, Lq, P = dims
    _boxes_upstream(what, ValueError, value, [("grad_output", grad_output, B * Lq * H * C)])
    if not _boxes_ok(_lib.box_bwd_boxes_ok, value, (L, Lq, P), also=[grad_output]):
        raise ValueError("%s: no kernel for value %s, %d levels, %d queries, %d points a level at the alignment of "
                         "value and grad_output (box_backward_boxes_ok)" % (what, tuple(value.shape), L, Lq, P))
    grads = _boxes_grads(value, (B, Lq, H, L), V, (B, Lq, H, L * P), need_ref_grad)
    _boxes_call("boxattn_bwd_boxes_", operands, (D, per_head), (V, mode), (grad_output,), dims, grads)
    return grads


# ---------------------------------------------------------------------------------------
# ... for the encoder case on the window-staged point-gradient kernels (opt-in; include/boxattn.h, boxattn_bwd_boxes_hl_*)
# ---------------------------------------------------------------------------------------
def box_backward_boxes_staged_ok(value, spatial_shapes, level_start_index, num_query, num_point, also=()):
    """Whether ``box_attn_backward_boxes_staged`` has its kernel under the current switches: ``boxattn_bwd_boxes_hl_ok``
    (the eligibility of ``box_forward_boxes_staged_ok``) with the dimensions, element size and alignment of ``value``
    (B, S, H, C) and the host copies of the level tables (``_host_table``: the first call with a tensor synchronises).
    The upstream gradient is taken as aligned like ``value``; ``box_attn_backward_boxes_staged`` asks again with its
    address (``also``).  Otherwise pure host code."""
    if not _host_tables_ok(spatial_shapes, level_start_index):
        return False
    sh, ls = _host_table(spatial_shapes), _host_table(level_start_index)
    return _boxes_ok(lambda elem, aligned, dims: _lib.box_bwd_boxes_hl_ok(elem, aligned, dims, sh, ls), value,
                     (spatial_shapes.size(0), num_query, num_point), also=also)


def box_attn_backward_boxes_staged(value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices,
                                   valid_ratios, logits, angle_mode, grad_output, need_ref_grad=False):
    """``box_attn_backward_boxes`` -- the same operands, the same three results up to the order of the float32 sums --
    for the encoder case (one query per pixel, C = 32, 2x2 points, at most 4 levels) on the window-staged kernels of
    ``box_attn_backward``'s encoder route: the locations and weights are made inside them from the boxes and logits
    (bit for bit ``box_attn_forward_boxes_staged``'s), the per-point gradients never leave the chip.  Bitwise
    reproducible.  The level tables are also read on the host (``_host_table``).  ``grad_value`` is not computed.
    Raises ValueError, before any device call, for arguments that do not fit and where ``boxattn_bwd_boxes_hl_ok`` says
    no at the alignment of ``value`` and ``grad_output``: there is no other kernel behind it."""
    what = "box_attn_backward_boxes_staged"
    operands = (value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios, logits)
    dims, (D, per_head, V, mode), _ = _boxes_operands(what, ValueError, None, operands, angle_mode,
                                                      also=[(grad_output, "grad_output")])
    B, _, H, C, L, Lq, P = dims
    _boxes_upstream(what, ValueError, value, [("grad_output", grad_output, B * Lq * H * C)])
    if not box_backward_boxes_staged_ok(value, spatial_shapes, level_start_index, Lq, P, also=[grad_output]):
        raise ValueError("%s: no kernel for value %s, %d levels, %d queries, %d points a level at the alignment of "
                         "value and grad_output (box_backward_boxes_staged_ok)" % (what, tuple(value.shape), L, Lq, P))
    sh, ls = _host_table(spatial_shapes), _host_table(level_start_index)
    grads = _boxes_grads(value, (B, Lq, H, L), V, (B, Lq, H, L * P), need_ref_grad)
    _boxes_call("boxattn_bwd_boxes_hl_", operands, (D, per_head), (V, mode), (grad_output,), dims,
                grads + (sh.ctypes.data, ls.ctypes.data))
    return grads


# ---------------------------------------------------------------------------------------
# the same step with grad_value in the backward's own launch (opt-in; include/boxattn.h, boxattn_bwd_boxes_value_*)
# ---------------------------------------------------------------------------------------
def box_backward_boxes_value_ok(value, num_level, num_query, num_point):
    """Whether ``box_attn_backward_boxes_value`` has its kernel under the current switches:
    ``boxattn_bwd_boxes_value_ok`` (the eligibility of ``box_backward_boxes_ok``) with the dimensions, element size
    and alignment of ``value`` (B, S, H, C).  The upstream gradient is taken as aligned like ``value``;
    ``box_attn_backward_boxes_value`` asks again with its address.  Pure host code."""
    return _boxes_ok(_lib.box_bwd_boxes_value_ok, value, (num_level, num_query, num_point))


def box_attn_backward_boxes_value(value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices,
                                  valid_ratios, logits, angle_mode, grad_output, want=3, need_ref_grad=False):
    """BoxAttention's / Box3dAttention's whole backward in one call, from the operands of ``box_attn_forward_boxes`` and
    the upstream gradient ``grad_output`` (B,Lq,H*C) in the type of ``value`` -> ``(grad_value (B,S,H,C) in the type of
    value, grad_offsets (B,Lq,H,L,V), grad_ref_rows (B,Lq,H,L,5) or None, grad_logits (B,Lq,H,L*P))``, the last three
    float32.  ``want``: 1 grad_value only, 2 the three others only (``box_attn_backward_boxes`` exactly), 3 all; a group
    not wanted comes back as None.  ``grad_value`` is scattered with float32 atomics by the kernel that computes the
    other three -- no sampling grid, no weights, no plan -- into itself (float32) or into a float32 scratch from the
    caching allocator that one pass casts (16-bit): it is NOT bitwise reproducible from call to call; the other three
    are, and are bit for bit those of ``box_attn_backward_boxes``.  Raises ValueError, before any device call, for
    arguments that do not fit and where ``boxattn_bwd_boxes_value_ok`` says no at the alignment of ``value`` and
    ``grad_output``: there is no other kernel behind it."""
    what = "box_attn_backward_boxes_value"
    operands = (value, spatial_shapes, level_start_index, ref_windows, offsets, kernel_indices, valid_ratios, logits)
    dims, (D, per_head, V, mode), _ = _boxes_operands(what, ValueError, None, operands, angle_mode,
                                                      also=[(grad_output, "grad_output")])
    B, _, H, C, L, Lq, P = dims
    _boxes_upstream(what, ValueError, value, [("grad_output", grad_output, B * Lq * H * C)])
    if isinstance(want, bool) or want not in (_lib.WANT_VALUE, _lib.WANT_POINTS, _lib.WANT_ALL):
        raise ValueError("%s: want must be 1 (grad_value), 2 (the box and logit gradients) or 3, got %r" % (what, want))
    if not _boxes_ok(_lib.box_bwd_boxes_value_ok, value, (L, Lq, P), also=[grad_output]):
        raise ValueError("%s: no kernel for value %s, %d levels, %d queries, %d points a level at the alignment of "
                         "value and grad_output (box_backward_boxes_value_ok)" % (what, tuple(value.shape), L, Lq, P))
    grad_value = scratch = None
    scratch_bytes = 0
    if want & _lib.WANT_VALUE:
        grad_value = torch.empty(value.shape, dtype=value.dtype, device=value.device)
        scratch_bytes = _lib.box_bwd_boxes_value_workspace_bytes(value.element_size(), dims)
        if scratch_bytes:
            scratch = torch.empty(scratch_bytes // 4, dtype=torch.float32, device=value.device)
    grads = (None, None, None)
    if want & _lib.WANT_POINTS:
        grads = _boxes_grads(value, (B, Lq, H, L), V, (B, Lq, H, L * P), need_ref_grad)
    _boxes_call("boxattn_bwd_boxes_value_", operands, (D, per_head), (V, mode), (grad_output,), dims,
                (int(want), grad_value, scratch, scratch_bytes) + grads)
    return (grad_value,) + grads
