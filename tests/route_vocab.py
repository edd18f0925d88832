"""The vocabulary of routes: the forward families, accumulate and record kinds and option values as the library
numbers them (boxer_amd._lib.FWD_*, ACC_*, REC_*), the storage types, moving arrays to the device, and the helpers that
ask the library which route a call takes or set the keys that choose one."""
import numpy as np
import torch

import error_bounds as eb

GENERIC, FAST, GATHER, WIDE, STAGED = range(5)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
WIDE_OFF, WIDE_ON = 1, 2


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(dtype) if dtype is not None else t


def take_family(value, loc, shapes, lsi, family):
    """Assert that box attention on these tensors runs on `family`; WIDE: force key 22 on where the default is off."""
    from boxer_amd import _lib, ops
    if family == WIDE and ops.forward_route(value, loc, shapes, lsi) != WIDE:
        _lib.set_option("wide_box", WIDE_ON)
    got = ops.forward_route(value, loc, shapes, lsi)
    assert got == family, "route %s, wanted %s" % (_lib.FWD_FAMILIES[got], _lib.FWD_FAMILIES[family])


VARIANTS = {"auto": 0, "generic": 1, "atomic": 2, "binned": 3}


def _cdt(dtype):
    return torch.float32 if dtype == torch.bfloat16 else dtype


OPT_ACC_F32 = 19        # boxattn_set_option: float32 accumulate -- 0 default: bf16 matrix cores on exact three-term splits,

OPT_RIDERS = 15         # 0 default (one-pass fill where eligible), 1 launches of their own, 4 two-pass riders (ABI 7)

BF16, F16 = torch.bfloat16, torch.float16

F32 = torch.float32


ACC_VALU, ACC_TR, ACC_F32, ACC_SPLIT = range(4)               # _lib.ACC_*
REC_POINT, REC_GROUP = range(2)                               # _lib.REC_*
SPLIT_OF_ACC = {ACC_VALU: "none", ACC_F32: "none", ACC_SPLIT: "split3"}        # ACC_TR: the storage type's two terms


def split_of(acc, dtype):
    return eb.store_name(dtype) if acc == ACC_TR else SPLIT_OF_ACC[acc]


def to_device(a, dtype=None, device="cuda"):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.to(device)
    return t.to(dtype) if dtype is not None and t.is_floating_point() else t


def routes(t, instance=False):
    from boxer_amd import ops
    return (ops.forward_route(t["value"], t["loc"], t["shapes"], t["lsi"], instance=instance),
            ops.backward_accumulate_kind(t["value"], t["loc"], instance=instance),
            ops.backward_record_kind(t["value"], t["loc"], instance=instance))


def set_encoder_keys(dense, riders, acc_key, rec_key):
    from boxer_amd import _lib
    _lib.set_option("dense", dense)
    _lib.set_option("riders", riders)
    _lib.set_option("acc_f32", acc_key)
    _lib.set_option("group_records", rec_key)


OPT_DENSE = 11          # boxattn_set_option key: 0 library default, 1 dense kernels off, 2 on

OPT_GROUP = 24
KEY_POINT, KEY_GROUP = 1, 2
