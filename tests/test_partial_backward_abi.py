"""CPU: the partial backward at the C ABI and the Python boundary -- *_bwd_part_* (only the gradient groups the
caller asks for: BOXATTN_WANT_VALUE, BOXATTN_WANT_POINTS) are declared in include/boxattn.h with the arguments of
their *_bwd_ws_* / *_bwd_f64 twins plus ``want``, the library exports them, the ctypes bindings give them
argtypes, and ``ops.*_backward`` take ``want`` (default 3: everything, as before).  No compute calls: there is no
GPU here."""
import ctypes
import inspect
import os
import re
import sys

import pytest
from capi_cases import HEADER, ROOT, header_declarations as declarations


PART_ENTRY_POINTS = ["%s_bwd_part_%s" % (kind, suf) for kind in ("boxattn", "instattn")
                     for suf in ("f32", "bf16", "f16", "f64")]


@pytest.fixture(scope="module")
def lib():
    from boxer_amd import _lib
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_declares_the_eight_entry_points_as_their_twins_plus_want():
    decl = declarations()
    assert len(PART_ENTRY_POINTS) == 8
    for name in PART_ENTRY_POINTS:
        assert name in decl, "missing declaration: " + name
        twin = name.replace("_bwd_part_f64", "_bwd_f64").replace("_bwd_part_", "_bwd_ws_")
        assert decl[name] == decl[twin] + ", int want", name


def test_header_defines_the_want_values_and_the_abi_version_stays_8():
    text = open(HEADER).read()
    assert re.search(r"#define BOXATTN_WANT_VALUE\s+1\b", text)
    assert re.search(r"#define BOXATTN_WANT_POINTS\s+2\b", text)
    assert re.search(r"#define BOXATTN_ABI_VERSION 8\b", text)


def test_library_exports_and_bindings(lib):
    from boxer_amd import _lib
    lib.boxattn_abi_version.restype = ctypes.c_int
    assert lib.boxattn_abi_version() == 8
    handle = _lib.load()
    assert (_lib.WANT_VALUE, _lib.WANT_POINTS, _lib.WANT_ALL) == (1, 2, 3)
    for name in PART_ENTRY_POINTS:
        assert hasattr(lib, name), "missing export: " + name
        assert name in _lib.EXPORTS, "not bound: " + name
        twin = name.replace("_bwd_part_f64", "_bwd_f64").replace("_bwd_part_", "_bwd_ws_")
        argtypes = getattr(handle, name).argtypes
        assert argtypes is not None, name
        assert list(argtypes) == list(getattr(handle, twin).argtypes) + [ctypes.c_int], name
        assert getattr(handle, name).restype is ctypes.c_int


def test_ops_backward_functions_take_want_with_default_3():
    from boxer_amd import ops
    for fn in (ops.box_attn_backward, ops.instance_attn_backward):
        p = inspect.signature(fn).parameters
        assert "want" in p and p["want"].default == 3, fn.__name__
        assert p["plan"].default is None                      # (as before)
    for bad in (0, 4, -1, None):
        with pytest.raises(ValueError):
            ops._want_groups(bad)
    assert [ops._want_groups(w) for w in (1, 2, 3)] == [(True, False), (False, True), (True, True)]


def test_value_only_kernels_are_instantiated_and_do_not_spill():
    """The value-only (POINTS = false) and points-only (SCATTER = false) flavours of both atomic kernels exist for
    every storage type next to the full ones, without scratch, and the value-only ones need fewer registers than
    the full form they are derived from (no corner values, no partial sums)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    from boxer_amd import _lib
    _lib.build()
    rows = [r for r in kernel_resources.kernels(_lib.LIB_PATH)
            if "bwd_fast_kernel" in r[0] or "bwd_generic_kernel" in r[0]]
    # template flags at the end of the argument list, demangled ("..., true, false>") or not ("Lb1ELb0EEEv")
    def flags(name):
        m = re.search(r"(true|false), (true|false)>\(", name) or re.search(r"Lb([01])ELb([01])EEEv", name)
        return tuple(g in ("true", "1") for g in m.groups())
    by = {}
    for r in rows:
        key = re.sub(r"(, (true|false), (true|false)>\(.*)|(Lb[01]ELb[01]EEEv.*)", "", r[0])
        by.setdefault(key, {})[flags(r[0])] = r
        assert int(r[4]) == 0, "scratch: " + r[0]
    assert len(by) >= 2 * 3 * 3 + 2 * 4, sorted(by)          # fast: INST x G x {f32, bf16, f16}; generic: INST x 4 types
    for key, inst in by.items():
        assert set(inst) == {(True, True), (False, True), (True, False)}, (key, sorted(inst))
        assert int(inst[(True, False)][1]) < int(inst[(True, True)][1]), key
