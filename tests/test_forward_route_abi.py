"""CPU: the forward's kernel-family query at the C ABI -- ``boxattn_fwd_route`` is declared in include/boxattn.h,
exported by the built library and bound by the ctypes loader; option key 22 (``"wide_box"``) exists; the route
table of the shapes that matter: box attention with few queries and a 14 x 14 grid (the mask model at inference)
against instance attention at the same shape, the benchmark's workloads, the switches.  The query is pure host
code: no compute calls, there is no GPU here."""
import ctypes
import re

import numpy as np
import pytest
from capi_cases import C2, C2P, C5P, HEADER
from route_vocab import FAST, GATHER, GENERIC, STAGED, WIDE


# What the measurement decided for box attention at B=2, Lq=300, P=196 on the C2' levels, per element size
# (profiles/inference_forward_step.log): True = the wave-per-pair family by default
DEFAULT_WIDE_P196 = {2: True, 4: True}
OPT_WIDE_BOX, OPT_DENSE = 22, 11
WIDE_BOX_OFF, WIDE_BOX_ON = 1, 2

C5 = [(468, 468)]
# bench.py's workloads: levels, Lq (None: one query per pixel), P
BOX_WORKLOADS = {"C2": (C2, None, 4), "C2p": (C2P, None, 4), "C3pp": (C2P, 300, 4), "C5": (C5, 1000, 4),
                 "C5p": (C5P, None, 4), "C5pp": (C5P, 300, 4)}
INST_WORKLOADS = {"C3": (C2, 300, 16), "C3p": (C2P, 300, 196)}


def tables(levels):
    shapes = np.asarray(levels, dtype=np.int64)
    sizes = shapes.prod(1)
    lsi = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return shapes, lsi, int(sizes.sum())


@pytest.fixture(scope="module")
def lib():
    from boxer_amd import _lib
    _lib.build()
    return _lib.load()


def route(elem, instance, levels, Lq, P, B=2, H=8, C=32, aligned=1, host=False):
    from boxer_amd import _lib
    shapes, lsi, S = tables(levels)
    dims = (B, S, H, C, len(levels), S if Lq is None else Lq, P)
    return _lib.fwd_route(elem, instance, aligned, dims, shapes if host else None, lsi if host else None)


def test_query_declared_exported_bound_and_key_22(lib):
    from boxer_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+boxattn_fwd_route\s*\(([^;{]*?)\)\s*;", text, re.S)
    assert m, "boxattn_fwd_route is not declared"
    assert " ".join(m.group(1).split()) == (
        "int elem_bytes, int instance, int aligned, int B, int S, int H, int C, int L, int Lq, int P, "
        "const int64_t *shapes_host, const int64_t *lsi_host")
    values = {name: int(v) for name, v in re.findall(r"#define\s+BOXATTN_FWD_(\w+)\s+(\d+)", text)}
    assert values == {"GENERIC": GENERIC, "FAST": FAST, "GATHER": GATHER, "WIDE": WIDE, "STAGED": STAGED}
    assert (_lib.FWD_GENERIC, _lib.FWD_FAST, _lib.FWD_GATHER, _lib.FWD_WIDE, _lib.FWD_STAGED) == (
        GENERIC, FAST, GATHER, WIDE, STAGED)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "boxattn_fwd_route")
    assert "boxattn_fwd_route" in _lib.EXPORTS
    assert lib.boxattn_fwd_route.restype is ctypes.c_int and len(lib.boxattn_fwd_route.argtypes) == 12
    assert _lib.OPTIONS["wide_box"] == OPT_WIDE_BOX
    assert lib.boxattn_set_option(OPT_WIDE_BOX, 1) != -1
    assert lib.boxattn_set_option(OPT_WIDE_BOX, 0) == 1           # (the old value comes back)
    assert lib.boxattn_abi_version() == 8


@pytest.mark.parametrize("elem", [2, 4])
def test_mask_inference_shape(lib, elem):
    """Box attention at B=2, S=22223, H=8, C=32, L=4, Lq=300, P=196."""
    want = WIDE if DEFAULT_WIDE_P196[elem] else GATHER
    assert route(elem, 0, C2P, 300, 196) == want
    assert route(elem, 0, C2P, 300, 196, host=True) == want            # host tables do not make it an encoder case
    lib.boxattn_set_option(OPT_WIDE_BOX, WIDE_BOX_ON)
    assert route(elem, 0, C2P, 300, 196) == WIDE
    lib.boxattn_set_option(OPT_WIDE_BOX, WIDE_BOX_OFF)
    assert route(elem, 0, C2P, 300, 196) == GATHER
    assert route(elem, 1, C2P, 300, 196) == WIDE                       # the instance flavour does not read key 22
    lib.boxattn_set_option(OPT_WIDE_BOX, 0)
    lib.boxattn_set_variant(1)
    assert route(elem, 0, C2P, 300, 196) == GENERIC
    assert route(elem, 1, C2P, 300, 196) == GENERIC
    lib.boxattn_set_variant(2)                                         # first-generation fast kernels only
    assert route(elem, 0, C2P, 300, 196) == FAST
    lib.boxattn_set_variant(0)
    assert route(elem, 1, C2P, 300, 196) == WIDE                       # instance attention: unchanged


@pytest.mark.parametrize("elem", [2, 4])
def test_other_rows_of_the_table(lib, elem):
    for on in (0, WIDE_BOX_ON):
        lib.boxattn_set_option(OPT_WIDE_BOX, on)
        assert route(elem, 0, C2P, 300, 4) == GATHER                   # C3'': fewer points than lane groups
        assert route(elem, 0, C2P, 300, 196, C=30) == GENERIC
        assert route(elem, 0, C2, None, 4, host=True) == STAGED        # the encoder case
        assert route(elem, 0, C2, None, 4) == GATHER                   # ... is recognised from the host tables
        assert route(8, 0, C2P, 300, 196) == GENERIC
        assert route(8, 1, C2P, 300, 196) == GENERIC
        assert route(elem, 0, C2P, 300, 196, aligned=0) == GENERIC     # nothing aligned: no fast kernel
    lib.boxattn_set_option(OPT_WIDE_BOX, 0)
    assert route(3, 0, C2P, 300, 196) < 0
    assert route(elem, 0, C2P, 300, 0) < 0
    assert route(elem, 0, C2P, 300, 196, H=0) < 0


@pytest.mark.parametrize("elem", [2, 4])
@pytest.mark.parametrize("on", [0, WIDE_BOX_ON])
def test_no_benchmark_workload_moves(lib, elem, on):
    """bench.py's box-attention shapes never take the wave-per-pair family (not even with key 22 forced on), with
    or without host tables; the instance shapes keep it."""
    lib.boxattn_set_option(OPT_WIDE_BOX, on)
    for name, (levels, Lq, P) in BOX_WORKLOADS.items():
        for host in (False, True):
            got = route(elem, 0, levels, Lq, P, host=host)
            assert got in (GATHER, STAGED), (name, host, got)
            assert host or got == GATHER, (name, got)                  # (staged needs the host tables)
    for name, (levels, Lq, P) in INST_WORKLOADS.items():
        assert route(elem, 1, levels, Lq, P) == WIDE, name


def test_query_sees_the_switches_the_launch_sees(lib):
    """One decision function behind the query and the launch: the query answers under the library's switches."""
    assert route(2, 0, C2, None, 4, host=True) == STAGED
    lib.boxattn_set_option(OPT_DENSE, 1)
    assert route(2, 0, C2, None, 4, host=True) == GATHER
    lib.boxattn_set_option(OPT_DENSE, 0)
    assert route(2, 0, C2, None, 4, host=True) == STAGED


def test_p_threshold_is_the_lane_groups_of_a_wave(lib):
    """With key 22 forced on, box attention takes the family exactly where instance attention does: from
    P = 64 / G points up (16-bit, C = 32, 16-byte rows: G = 4; float32: G = 8; 8-byte rows, 16-bit: G = 8)."""
    lib.boxattn_set_option(OPT_WIDE_BOX, WIDE_BOX_ON)
    for elem, aligned, first in ((2, 1, 16), (4, 1, 8), (2, 8, 8)):
        for P in (first - 1, first):
            for inst in (0, 1):
                assert route(elem, inst, C2P, 300, P, aligned=aligned) == (WIDE if P >= first else GATHER), (
                    elem, aligned, P, inst)
    assert route(4, 0, C2P, 300, 196, aligned=8) == GENERIC            # float32 rows need 16 bytes
