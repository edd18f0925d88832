"""CPU: group records at the C ABI -- ``boxattn_bwd_record_kind`` is declared in include/boxattn.h, exported by the built
library and bound by the ctypes loader and ``ops.backward_record_kind``; option key 24 (``"group_records"``) exists and
bumps the options epoch; the route table: group records for 16-bit box attention with P = 4 on the matrix-core accumulate
under key 24 = 2, point records for float32, instance attention, other P and key 24 = 1; the workspace of an eligible
shape is smaller under key 24 = 2.  Pure host code: there is no GPU here."""
import ctypes
import re

import numpy as np
import pytest
from capi_cases import C2, C2P, C5P, HEADER
from route_vocab import KEY_GROUP, KEY_POINT, OPT_GROUP


POINT, GROUP = 0, 1


@pytest.fixture(scope="module")
def lib():
    from boxer_amd import _lib
    _lib.build()
    lib = _lib.load()
    yield lib
    lib.boxattn_set_option(OPT_GROUP, 0)


def dims_of(levels, Lq=None, P=4, B=2, H=8, C=32):
    S = int(np.asarray(levels, dtype=np.int64).prod(1).sum())
    return (B, S, H, C, len(levels), S if Lq is None else Lq, P)


def kind(elem, instance, levels, **kw):
    from boxer_amd import _lib
    return _lib.bwd_record_kind(elem, instance, dims_of(levels, **kw))


def test_query_declared_exported_bound_and_key_24(lib):
    from boxer_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+boxattn_bwd_record_kind\s*\(([^;{]*?)\)\s*;", text, re.S)
    assert m, "boxattn_bwd_record_kind is not declared"
    assert " ".join(m.group(1).split()) == (
        "int elem_bytes, int instance, int B, int S, int H, int C, int L, int Lq, int P")
    values = {name: int(v) for name, v in re.findall(r"#define\s+BOXATTN_REC_(\w+)\s+(\d+)", text)}
    assert values == {"POINT": POINT, "GROUP": GROUP}
    assert (_lib.REC_POINT, _lib.REC_GROUP) == (POINT, GROUP)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "boxattn_bwd_record_kind")
    assert "boxattn_bwd_record_kind" in _lib.EXPORTS
    fn = lib.boxattn_bwd_record_kind
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert _lib.OPTIONS["group_records"] == OPT_GROUP
    assert lib.boxattn_abi_version() == 8
    assert callable(ops.backward_record_kind)


def test_key_24_is_accepted_and_bumps_the_epoch(lib):
    e0 = lib.boxattn_options_epoch()
    assert lib.boxattn_set_option(OPT_GROUP, KEY_GROUP) != -1
    assert lib.boxattn_options_epoch() == e0 + 1
    assert lib.boxattn_set_option(OPT_GROUP, 0) == KEY_GROUP          # (the old value comes back)
    assert lib.boxattn_options_epoch() == e0 + 2
    assert lib.boxattn_set_option(OPT_GROUP + 1, 0) == -1


def test_route_table(lib):
    lib.boxattn_set_option(OPT_GROUP, KEY_GROUP)
    for C in (16, 32, 64):
        assert kind(2, 0, C2, C=C) == GROUP                           # 16-bit box attention, P = 4, kAccTr
    assert kind(2, 0, C2, Lq=37) == GROUP                             # (a decoder's queries too)
    assert kind(2, 0, C2, C=24) == POINT                              # no matrix-core accumulate
    assert kind(4, 0, C2) == POINT                                    # float32
    assert kind(2, 1, C2, Lq=300, P=4) == POINT                       # instance attention
    assert kind(4, 1, C2, Lq=300, P=4) == POINT
    for P in (1, 16, 8):
        assert kind(2, 0, C2, Lq=300, P=P) == POINT
    lib.boxattn_set_option(OPT_GROUP, KEY_POINT)
    for C in (16, 32, 64):
        assert kind(2, 0, C2, C=C) == POINT
    lib.boxattn_set_option(OPT_GROUP, 0)
    assert kind(4, 0, C2) == POINT and kind(2, 1, C2, Lq=300) == POINT
    # the default is what the step measurement decided (profiles/group_records_step.log): the encoders
    # on the one-pass fill from C2's size up passed, the decoder queries and the BEV encoder did not
    assert kind(2, 0, C2) == GROUP and kind(2, 0, C2P) == GROUP
    assert kind(2, 0, C2P, Lq=300) == POINT and kind(2, 0, C5P) == POINT
    assert kind(2, 0, [(37, 53), (19, 27), (10, 14), (5, 7)]) == POINT  # (small maps: not measured, point records)


def test_invalid_arguments(lib):
    assert kind(8, 0, C2) < 0
    assert kind(3, 0, C2) < 0
    assert kind(2, 0, C2, P=0) < 0
    assert kind(2, 0, C2, H=0) < 0


def test_workspace_shrinks_at_c2_bf16(lib):
    dims = dims_of(C2)
    sh = np.asarray(C2, dtype=np.int64)
    ls = np.concatenate([[0], np.cumsum(sh.prod(1))[:-1]]).astype(np.int64)
    size = {}
    for key in (KEY_POINT, KEY_GROUP):
        lib.boxattn_set_option(OPT_GROUP, key)
        size[key] = int(lib.boxattn_bwd_workspace_bytes(1, *dims, sh.ctypes.data, ls.ctypes.data))
    lib.boxattn_set_option(OPT_GROUP, 0)
    print("C2 bf16 workspace: point records %d bytes (%.1f MB), group records %d bytes (%.1f MB)"
          % (size[KEY_POINT], size[KEY_POINT] / 1e6, size[KEY_GROUP], size[KEY_GROUP] / 1e6))
    assert 0 < size[KEY_GROUP] < size[KEY_POINT]
    # float32 does not read the key
    f32 = []
    for key in (KEY_POINT, KEY_GROUP):
        lib.boxattn_set_option(OPT_GROUP, key)
        f32.append(int(lib.boxattn_bwd_workspace_bytes(0, *dims, sh.ctypes.data, ls.ctypes.data)))
    lib.boxattn_set_option(OPT_GROUP, 0)
    assert f32[0] == f32[1]
