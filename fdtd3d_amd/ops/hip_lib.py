"""The error type, ctypes shorthands and argument helpers of the HIP backend's
modules (ops/hip_ops.py, ops/hip_monitors.py)."""

from __future__ import annotations

import ctypes
from typing import Optional

import torch

c_int = ctypes.c_int
c_ll = ctypes.c_longlong
c_double = ctypes.c_double
c_vp = ctypes.c_void_p


class HipError(RuntimeError):
    pass


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise HipError("%s failed: hipError %d" % (what, rc))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
