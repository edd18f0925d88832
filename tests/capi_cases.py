"""The C ABI as the header and entry-point tests see it: where include/boxattn.h lies, what it declares, the
geometries the from-boxes entry points are queried on, and raw ctypes calls with pointers that are never dereferenced.
Nothing here builds or loads the library: every function takes the ``lib`` a test module's fixture built."""
import itertools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "boxattn.h")


C2P = [(100, 167), (50, 84), (25, 42), (13, 21)]
C2 = [(100, 100), (50, 50), (25, 25), (13, 13)]

INVALID_VALUE = 1                        # hipErrorInvalidValue
# (levels, B, Lq, H): a decoder-like and an encoder-like (one query a pixel) geometry
BOX_GEOMETRIES = [([(9, 11), (4, 5), (3, 3), (2, 2)], 2, 5, 8), ([(6, 5)], 1, 30, 2)]


def declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): " ".join(m.group(2).split())
            for m in re.finditer(r"\b((?:boxattn|instattn)_\w+)\s*\(([^;{]*?)\)\s*;", text, re.S)}


# (levels, B, H): one query a pixel in all of them (Lq is varied below)
STAGED_GEOMETRIES = list(itertools.product([[(9, 11), (4, 5), (3, 3), (2, 2)], [(6, 5)], [(37, 23), (19, 12)]], (1, 2), (1, 3, 8)))


def host_tables(levels, L=None, broken=False):
    """int64 (L, 2) shapes and (L) start indices of the first L levels (cycled if there are fewer), and S; broken: an S
    one above the sum of the tables' sizes."""
    L = len(levels) if L is None else L
    shapes = np.asarray([levels[i % len(levels)] for i in range(L)], dtype=np.int64)
    sizes = shapes.prod(1)
    return shapes, np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64), int(sizes.sum()) + (1 if broken else 0)


def call_value(lib, name, ptrs, dims, want, gv, ws, ws_bytes, ref_dim=4, V=4, angle_mode=0):
    """An entry call with fake (never dereferenced) pointers; ptrs: value, shapes, lsi, ref, offsets, kernel_idx,
    valid_ratios, logits, grad_out, grad_offsets, grad_ref_rows, grad_logits."""
    v, sh, ls, ref, off, kid, vr, lg, go, goff, grow, glog = ptrs
    return getattr(lib.load(), name)(v, sh, ls, ref, ref_dim, 0, off, V, angle_mode, kid, vr, lg, go, *dims, want, gv,
                                     ws, ws_bytes, goff, grow, glog, None)


# the two small geometries of the issue: (levels, B, Lq, H)
INST_GEOMETRIES = [([(9, 11), (4, 5)], 2, 4, 8), ([(6, 5)], 1, 3, 2)]


def header_declarations():
    """name -> parameter list (whitespace-normalised) of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): " ".join(m.group(2).split())
            for m in re.finditer(r"\b((?:boxattn|instattn)_\w+)\s*\(([^;{]*?)\)\s*;", text, re.S)}


C5P = [(234, 234), (117, 117)]
