"""Loader (and in-tree builder) of the C-ABI HIP library ``libboxattn_hip.so``.

The library is the product: there is no CPU or PyTorch fallback behind it.  If it cannot be
found or loaded, every op raises -- nothing here ever imports ``oracle/``.
"""
import ctypes
import os
import shutil
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_PKG, "csrc")
LIB_NAME = "libboxattn_hip.so"
LIB_PATH = os.path.join(_PKG, LIB_NAME)
# the C-ABI header: the source checkout's include/ when there is one, else the copy a non-editable
# install ships inside the package (setup.py: package_data "include/*.h")
INCLUDE_DIR = os.path.join(os.path.dirname(_PKG), "include")
if not os.path.exists(os.path.join(INCLUDE_DIR, "boxattn.h")):
    INCLUDE_DIR = os.path.join(_PKG, "include")
# translation units -> extra flags.  boxattn_dense.hip (the matrix-core encoder kernels) is built
# with -fno-slp-vectorize: packed float32 VALU instructions (v_pk_mul_f32 / v_pk_add_f32, which the
# SLP vectoriser forms from adjacent scalar operations) issued while an MFMA of the same wave is
# finishing returned wrong results in lanes 48-63 on MI355X with this compiler
SOURCES = {"boxattn_capi.hip": [], "boxattn_extras.hip": [], "boxattn_dense.hip": ["-fno-slp-vectorize"]}
HEADERS = sorted(f for f in os.listdir(_CSRC) if f.endswith(".h"))     # every kernel header
# -amdgpu-kernarg-preload-count: the first 16 dwords of a kernel's arguments (its pointers) arrive in
# SGPRs with the wave instead of through scalar loads at its top (gfx94x / gfx950); every wave of
# these kernels is short, and their prologues are a measurable part of them
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-pass-failed",
               "-mllvm", "-amdgpu-kernarg-preload-count=16"]
BUILD_DIR = os.path.join(_PKG, "_build")

_lib = None

_vp, _i, _ll, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
_S3, _S4 = ("f32", "bf16", "f16"), ("f32", "f64", "bf16", "f16")
# 16-bit storage types: the suffix of their entry points, which share signatures (uint16_t storage)
H16_SUFFIXES = ("bf16", "f16")
ABI_VERSION = 8
WANT_VALUE, WANT_POINTS, WANT_ALL = 1, 2, 3      # BOXATTN_WANT_*: the gradient groups of a partial backward
HINT_NOT_LOCAL = 1          # BOXATTN_HINT_NOT_LOCAL
HINT_FRESH_STATE = 2        # BOXATTN_HINT_FRESH_STATE

# The argument lists of include/boxattn.h, in pieces
_DIMS = [_i] * 7                      # B, S, H, C, L, Lq, P
_STREAM = [_vp]
# a flavour's forward / backward up to its last output: value, shapes, lsi, loc, weights, [grad_out, [grad_mask]],
# dims, outputs
_FWD = {"boxattn": [_vp] * 5 + _DIMS + [_vp], "instattn": [_vp] * 6 + _DIMS + [_vp] * 2}
_BWD = {"boxattn": [_vp] * 6 + _DIMS + [_vp] * 3, "instattn": [_vp] * 8 + _DIMS + [_vp] * 4}
_HOST = [_vp, _vp]                    # shapes_host, lsi_host
_TRAIN = _HOST + [_vp, _sz, _vp, _sz, _i, _vp]         # + plan, plan_bytes, state, state_bytes, hints, int *plan_built
# + workspace, workspace_bytes, plan, plan_bytes, state, state_bytes, hints
_WS = _HOST + [_vp, _sz, _vp, _sz, _vp, _sz, _i]
_QUERY = [_i] * 9                     # elem_bytes, instance | aligned, dims
_SIZES = [_i] * 8 + _HOST             # is_16bit, dims, shapes_host, lsi_host


def _boxes(box, upstream, outputs):
    """The calls from boxes and logits: value, shapes, lsi, ref, ref_dim, ref_per_head, offsets, [V, angle_mode: the
    box flavour,] kernel_idx, valid_ratios | NULL, logits, <upstream gradients>, B, S, H, C, L, Lq, k | P, <outputs>,
    stream"""
    return ([_vp] * 4 + [_i, _i, _vp] + ([_i, _i] if box else []) + [_vp] * 3 + [_vp] * upstream + _DIMS +
            [_vp] * outputs + _STREAM)


def _family(stem, suffixes, argtypes, restype=_i):
    return {"%s_%s" % (stem, suf): (restype, argtypes) for suf in suffixes}


# name -> (restype, argtypes): every function include/boxattn.h declares (tests/test_capi_symbols.py holds it to that)
_SIGNATURES = {
    "boxattn_abi_version": (_i, []),
    "boxattn_build_info": (ctypes.c_char_p, []),
    "boxattn_set_variant": (_i, [_i]),
    "boxattn_set_option": (_i, [_i, _i]),
    "boxattn_options_epoch": (_i, []),
    "boxattn_set_debug_buffer": (None, [_vp]),
    "boxattn_profile_begin": (_i, []),
    "boxattn_profile_end": (_i, [_vp, _vp]),              # double *ms_sum, int *launches
    "boxattn_fwd_route": (_i, [_i] + _QUERY + _HOST),     # elem_bytes, instance, aligned, dims, shapes_host, lsi_host
    "boxattn_bwd_accumulate_kind": (_i, _QUERY),
    "boxattn_bwd_record_kind": (_i, _QUERY),
    "boxattn_state_bytes": (_sz, _DIMS + _HOST),
    "boxattn_bwd_workspace_bytes": (_sz, _SIZES),
    "boxattn_plan_bytes": (_sz, _SIZES),
    **_family("boxattn_fwd_hl", _S3, _FWD["boxattn"] + _HOST + _STREAM),
    # ref, ref_dim, ref_per_head, offsets, V, angle_mode, kernel_idx, valid_ratios, [grad_grid,] B, Lq, H, L, P, outputs,
    # stream
    "boxattn_grid_fwd_f32": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp] + [_i] * 5 + [_vp] + _STREAM),
    "boxattn_grid_bwd_f32": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp] + [_i] * 5 + [_vp, _vp] + _STREAM),
    **_family("boxattn_softmax_fwd", _S3, [_vp, _ll, _i, _vp] + _STREAM),
    **_family("boxattn_softmax_bwd", _S3, [_vp, _vp, _ll, _i, _vp] + _STREAM),
    **_family("boxattn_value_prep", _S3 + ("f32_f16",), [_vp, _vp, _ll, _i, _vp] + _STREAM),     # f32_f16: float32 -> f16
    # logits, rows, L, k, spatial_w, level_w | NULL, stream
    **_family("instattn_weights_fwd", _S3, [_vp, _ll, _i, _i, _vp, _vp] + _STREAM),
    # logits, grad_spatial_w | NULL, grad_level_w | NULL, rows, L, k, grad_logits, stream
    **_family("instattn_weights_bwd", _S3, [_vp, _vp, _vp, _ll, _i, _i, _vp] + _STREAM),
    **_family("instattn_fwd_boxes", _S3, _boxes(False, 0, 2)),          # out, mask_out | NULL
    # grad_out, grad_mask | NULL; grad_offsets, grad_ref_rows | NULL, grad_logits
    **_family("instattn_bwd_boxes", _S3, _boxes(False, 2, 3)),
    **_family("boxattn_fwd_boxes", _S3, _boxes(True, 0, 1)),            # out
    # boxattn_fwd_boxes_* up to out, then shapes_host, lsi_host, stream: the window-staged forward from boxes
    **_family("boxattn_fwd_boxes_hl", _S3, _boxes(True, 0, 1)[:-1] + _HOST + _STREAM),
    "boxattn_fwd_boxes_hl_ok": (_i, _QUERY + _HOST),      # elem_bytes, aligned, dims, shapes_host, lsi_host
    **_family("boxattn_bwd_boxes", _S3, _boxes(True, 1, 3)),            # grad_out; the three gradients
    # boxattn_bwd_boxes_* up to grad_logits, then shapes_host, lsi_host, stream: the window-staged backward from boxes
    **_family("boxattn_bwd_boxes_hl", _S3, _boxes(True, 1, 3)[:-1] + _HOST + _STREAM),
    "boxattn_bwd_boxes_hl_ok": (_i, _QUERY + _HOST),      # elem_bytes, aligned, dims, shapes_host, lsi_host
    # boxattn_bwd_boxes_* up to P, then want, grad_value, workspace, workspace_bytes, the three gradients, stream
    **_family("boxattn_bwd_boxes_value", _S3, _boxes(True, 1, 0)[:-1] + [_i, _vp, _vp, _sz] + [_vp] * 3 + _STREAM),
    **{"%s_%s_boxes_ok" % (op, way): (_i, _QUERY) for op in _FWD for way in ("fwd", "bwd")},
    "boxattn_bwd_boxes_value_ok": (_i, _QUERY),
    "boxattn_bwd_boxes_value_workspace_bytes": (_sz, [_i] * 5),      # elem_bytes, B, S, H, C
}
for _op in _FWD:
    for _stem, _suffixes, _args in (
            ("fwd", _S4, _FWD[_op] + _STREAM),
            ("fwd_train", _S3, _FWD[_op] + _TRAIN + _STREAM),
            ("bwd", ("f32", "f64"), _BWD[_op] + _STREAM),
            ("bwd", H16_SUFFIXES, _BWD[_op] + [_vp] + _STREAM),         # + float *grad_value_ws
            ("bwd_ws", _S3, _BWD[_op] + _WS + _STREAM),
            ("bwd_part", _S3, _BWD[_op] + _WS + _STREAM + [_i]),        # *_bwd_ws_* + int want
            ("bwd_part", ("f64",), _BWD[_op] + _STREAM + [_i])):        # *_bwd_f64 + int want
        _SIGNATURES.update(_family("%s_%s" % (_op, _stem), _suffixes, _args))
EXPORTS = list(_SIGNATURES)


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build %s" % LIB_NAME)


def _deps():
    deps = [os.path.join(_CSRC, f) for f in list(SOURCES) + HEADERS]
    deps.append(os.path.join(INCLUDE_DIR, "boxattn.h"))
    return [d for d in deps if os.path.exists(d)]


def _flags_stamp(extra_flags=()):
    """The command-line flags of every translation unit: a change of flags rebuilds like a change of
    sources (the -fno-slp-vectorize rule of boxattn_dense.hip is a correctness matter)."""
    return repr((HIPCC_FLAGS, sorted(SOURCES.items()), list(extra_flags)))


def _stamp_path(tag):
    return os.path.join(BUILD_DIR, tag + ".flags")


def _flags_changed(tag, extra_flags=()):
    try:
        with open(_stamp_path(tag)) as fh:
            return fh.read() != _flags_stamp(extra_flags)
    except OSError:
        return True


def needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    built = os.path.getmtime(LIB_PATH)
    # (a shipped library without a build directory is taken as it is)
    if os.path.isdir(BUILD_DIR) and _flags_changed(os.path.basename(LIB_PATH)):
        return True
    return any(os.path.getmtime(s) > built for s in _deps())


def build(force=False, verbose=False, extra_flags=(), out_path=None):
    """Cross-compile the HIP library for gfx950 in-tree (works without a GPU): one object per
    translation unit (compiled in parallel), then one shared library.  ``extra_flags`` /
    ``out_path``: a second build next to the product (the step tools' --variant, tools/kernel_diff.py)."""
    variant = out_path is not None
    out_path = out_path or LIB_PATH
    if not (force or variant or needs_build()):
        return out_path
    tag = os.path.basename(out_path)
    os.makedirs(BUILD_DIR, exist_ok=True)
    newest = max(os.path.getmtime(d) for d in _deps())
    stale_flags = _flags_changed(tag, extra_flags)
    procs, objs = [], []
    for src, flags in SOURCES.items():
        obj = os.path.join(BUILD_DIR, "%s.%s.o" % (tag, src))
        objs.append(obj)
        if not (force or variant or stale_flags) and os.path.exists(obj) and os.path.getmtime(obj) >= newest:
            continue
        cmd = [hipcc_path()] + HIPCC_FLAGS + list(flags) + list(extra_flags) + [
            "-c", os.path.join(_CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out_path + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(out_path + ".tmp", out_path)
    with open(_stamp_path(tag), "w") as fh:
        fh.write(_flags_stamp(extra_flags))
    if not variant:
        global _lib
        _lib = None
    return out_path


def load():
    """Return the ctypes handle; raises RuntimeError if the HIP library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # BOXATTN_HIP_LIB: load another build of the same library (kernel tuning experiments, built with
    # `python -m boxer_amd._lib --out PATH`); it must export the same ABI.
    path = os.environ.get("BOXATTN_HIP_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            "%s is missing. Build it with `python setup.py build_ext --inplace` (or "
            "`python -c 'import __graft_entry__ as g; g.build()'`). boxer_amd has no CPU "
            "fallback by design." % path)
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.boxattn_abi_version() != ABI_VERSION:
        raise RuntimeError("ABI version mismatch in %s" % path)
    _lib = lib
    return lib


def build_info():
    return load().boxattn_build_info().decode()


def options_epoch():
    """boxattn_options_epoch(): bumped by every set_variant / set_option call (ops.py caches the size queries
    per epoch: the workspace layouts depend on some switches)."""
    return load().boxattn_options_epoch()


def set_variant(v):
    """0 = auto, 1 = generic kernels only, 2 = fast atomic kernels only, 3 = auto with the binned
    backward required (2 and 3 return an error when the shape is not eligible)."""
    return load().boxattn_set_variant(int(v))


OPTIONS = {"bin_chunk": 10, "dense": 11, "riders": 15, "acc_f32": 19, "ride_shift": 20, "wide_box": 22,
           "inst_acc16": 23, "group_records": 24}
# boxattn_fwd_route: the forward's kernel families (BOXATTN_FWD_*)
FWD_GENERIC, FWD_FAST, FWD_GATHER, FWD_WIDE, FWD_STAGED = range(5)
FWD_FAMILIES = ("generic", "fast", "gather", "wide", "staged")


def fwd_route(elem_bytes, instance, aligned, dims, shapes_host=None, lsi_host=None):
    """boxattn_fwd_route(): the forward kernel family (FWD_*) for ``dims`` = (B, S, H, C, L, Lq, P) under the current
    switches; ``shapes_host`` / ``lsi_host``: int64 numpy arrays or None.  Pure host code (no GPU needed)."""
    ptr = lambda a: None if a is None else a.ctypes.data
    return load().boxattn_fwd_route(int(elem_bytes), int(instance), int(aligned), *[int(v) for v in dims],
                                    ptr(shapes_host), ptr(lsi_host))


def _boxes_ok(name, elem_bytes, aligned, dims):
    """The eligibility queries of the calls from boxes: ``dims`` = (B, S, H, C, L, Lq, k or P)."""
    return bool(getattr(load(), name)(int(elem_bytes), int(aligned), *[int(v) for v in dims]))


def fwd_boxes_ok(elem_bytes, aligned, dims, k):
    """instattn_fwd_boxes_ok(): whether the instattn_fwd_boxes_* entry points have their kernel for ``dims`` = (B, S, H,
    C, L, Lq) and ``k`` x ``k`` points a level under the current switches.  Pure host code (no GPU needed)."""
    return _boxes_ok("instattn_fwd_boxes_ok", elem_bytes, aligned, tuple(dims) + (k,))


def box_fwd_boxes_ok(elem_bytes, aligned, dims):
    """boxattn_fwd_boxes_ok(): whether the boxattn_fwd_boxes_* entry points have their kernel for ``dims`` = (B, S, H,
    C, L, Lq, P) under the current switches.  Pure host code (no GPU needed)."""
    return _boxes_ok("boxattn_fwd_boxes_ok", elem_bytes, aligned, dims)


def box_fwd_boxes_hl_ok(elem_bytes, aligned, dims, shapes_host=None, lsi_host=None):
    """boxattn_fwd_boxes_hl_ok(): whether the boxattn_fwd_boxes_hl_* entry points have their kernel for ``dims`` = (B, S,
    H, C, L, Lq, P) and the level tables ``shapes_host`` / ``lsi_host`` (int64 numpy arrays; None: no) under the current
    switches -- where ``fwd_route`` with them answers FWD_STAGED.  Pure host code (no GPU needed)."""
    ptr = lambda a: None if a is None else a.ctypes.data
    return bool(load().boxattn_fwd_boxes_hl_ok(int(elem_bytes), int(aligned), *[int(v) for v in dims],
                                               ptr(shapes_host), ptr(lsi_host)))


def box_bwd_boxes_hl_ok(elem_bytes, aligned, dims, shapes_host=None, lsi_host=None):
    """boxattn_bwd_boxes_hl_ok(): whether the boxattn_bwd_boxes_hl_* entry points have their kernel for ``dims`` = (B, S,
    H, C, L, Lq, P) with the host copies of the level tables (int64 numpy arrays or None) under the current switches:
    ``box_fwd_boxes_hl_ok``'s function, ``aligned`` speaking of value and grad_out.  Pure host code."""
    ptr = lambda a: None if a is None else a.ctypes.data
    return bool(load().boxattn_bwd_boxes_hl_ok(int(elem_bytes), int(aligned), *[int(v) for v in dims],
                                               ptr(shapes_host), ptr(lsi_host)))


def box_bwd_boxes_ok(elem_bytes, aligned, dims):
    """boxattn_bwd_boxes_ok(): whether the boxattn_bwd_boxes_* entry points have their kernel for ``dims`` = (B, S, H,
    C, L, Lq, P) under the current switches.  Pure host code (no GPU needed)."""
    return _boxes_ok("boxattn_bwd_boxes_ok", elem_bytes, aligned, dims)


def box_bwd_boxes_value_ok(elem_bytes, aligned, dims):
    """boxattn_bwd_boxes_value_ok(): whether the boxattn_bwd_boxes_value_* entry points have their kernel for ``dims`` =
    (B, S, H, C, L, Lq, P) under the current switches.  Pure host code (no GPU needed)."""
    return _boxes_ok("boxattn_bwd_boxes_value_ok", elem_bytes, aligned, dims)


def box_bwd_boxes_value_workspace_bytes(elem_bytes, dims):
    """boxattn_bwd_boxes_value_workspace_bytes(): the bytes of float32 accumulator a boxattn_bwd_boxes_value_* call
    takes for ``dims`` = (B, S, H, C, ...): 0 for 4-byte storage.  Pure host code (no GPU needed)."""
    return int(load().boxattn_bwd_boxes_value_workspace_bytes(int(elem_bytes), *[int(v) for v in dims[:4]]))


def bwd_boxes_ok(elem_bytes, aligned, dims, k):
    """instattn_bwd_boxes_ok(): whether the instattn_bwd_boxes_* entry points have their kernel for ``dims`` = (B, S, H,
    C, L, Lq) and ``k`` x ``k`` points a level under the current switches.  Pure host code (no GPU needed)."""
    return _boxes_ok("instattn_bwd_boxes_ok", elem_bytes, aligned, tuple(dims) + (k,))


# boxattn_bwd_accumulate_kind: the grad_value accumulate kernels of the binned backward (BOXATTN_ACC_*)
ACC_VALU, ACC_TR, ACC_F32, ACC_SPLIT = range(4)
ACC_KINDS = ("valu", "tr", "f32", "split")


def bwd_accumulate_kind(elem_bytes, instance, dims):
    """boxattn_bwd_accumulate_kind(): the accumulate kernel (ACC_*) of a binned backward at ``dims`` = (B, S, H, C, L,
    Lq, P) under the current switches; negative for invalid arguments or float64.  Pure host code (no GPU needed)."""
    return load().boxattn_bwd_accumulate_kind(int(elem_bytes), int(instance), *[int(v) for v in dims])


# boxattn_bwd_record_kind: the records of the binned backward (BOXATTN_REC_*)
REC_POINT, REC_GROUP = range(2)
REC_KINDS = ("point", "group")


def bwd_record_kind(elem_bytes, instance, dims):
    """boxattn_bwd_record_kind(): the records (REC_*) a binned backward at ``dims`` = (B, S, H, C, L, Lq, P) writes under
    the current switches; negative for invalid arguments or float64.  Pure host code (no GPU needed)."""
    return load().boxattn_bwd_record_kind(int(elem_bytes), int(instance), *[int(v) for v in dims])


def set_option(name, value):
    """Tuning knobs for A/B runs (include/boxattn.h: boxattn_set_option); returns the old value."""
    old = load().boxattn_set_option(OPTIONS[name], int(value))
    if old < 0:
        raise KeyError(name)
    return old


def profile_begin():
    """Start bracketing the library's main kernels with hipEvents (bench.py)."""
    load().boxattn_profile_begin()


PROFILE_SLOTS = ("fwd", "bwd_points", "bwd_accumulate", "bwd_binning", "bwd_combine", "bwd_prep")


def profile_end():
    """-> {slot: {"ms": average kernel duration, "launches": n}} for the timing slots."""
    ms = (ctypes.c_double * len(PROFILE_SLOTS))()
    n = (ctypes.c_int * len(PROFILE_SLOTS))()
    load().boxattn_profile_end(ms, n)
    return {name: {"ms": (ms[i] / n[i] if n[i] else None), "launches": int(n[i])}
            for i, name in enumerate(PROFILE_SLOTS)}


if __name__ == "__main__":      # python -m boxer_amd._lib [--out PATH] [extra hipcc flags ...]
    import sys
    args = sys.argv[1:]
    out = None
    if args[:1] == ["--out"]:
        out, args = args[1], args[2:]
    print(build(force=True, verbose=True, extra_flags=args, out_path=out))
