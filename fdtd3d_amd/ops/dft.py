"""Entries of a running-DFT monitor, shared by both backends'
``dft_accumulate(entries, twiddles)``.

One entry = one (field array, array-local box, accumulators, kind).  The
accumulators of an entry are box-local, ``[k][re|im][x][y][z']``, where the z'
extent is the box's z range widened to the field's 16-byte groups (from ``lo &
~(V - 1)`` to ``hi`` rounded up, ``V`` = 4 fp32 / 2 fp64 elements): an
accumulator vector and its field vector start at the same z (csrc/
dft_kernels.hip).  The padded cells are never written and stay zero.
"""

from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch

Box = Tuple[Tuple[int, int, int], Tuple[int, int, int]]

DFT_MAX_K = 8        # monitored frequencies per launch (fdtd_dft_max_k)
DFT_ENT_SIZE = 64    # bytes of a device table entry (fdtd_dft_ent_size)
KIND_E, KIND_H = 0, 1


def vec_width(dtype) -> int:
    """Elements of a 16-byte lane."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def box_empty(box: Box) -> bool:
    return any(box[1][d] <= box[0][d] for d in range(3))


def z_pad(box: Box, v: int) -> Tuple[int, int]:
    """(first z of the padded range, padded z extent) of a box."""
    z0 = box[0][2] & ~(v - 1)
    return z0, -(-box[1][2] // v) * v - z0


def acc_shape(box: Box, k: int, v: int) -> Tuple[int, int, int, int, int]:
    if box_empty(box):
        return (k, 2, 0, 0, 0)
    return (k, 2, box[1][0] - box[0][0], box[1][1] - box[0][1], z_pad(box, v)[1])


class DftEntry:
    """``field`` is the array sampled at the next call (a monitor re-resolves
    it before every call: the scheme's F / F_alt ping-pong), ``box`` its
    array-local box, ``acc`` the accumulators (``acc_shape``), ``kind``
    KIND_E / KIND_H (which twiddle row applies)."""
    __slots__ = ("field", "box", "acc", "kind")

    def __init__(self, field: torch.Tensor, box: Box, acc: torch.Tensor, kind: int):
        self.field, self.box, self.acc, self.kind = field, box, acc, kind

    @property
    def empty(self) -> bool:
        return box_empty(self.box)

    def owned(self) -> torch.Tensor:
        """The accumulators without the padding: (K, 2, bx, by, bz)."""
        if self.empty:
            return self.acc
        v = vec_width(self.acc.dtype)
        z0 = z_pad(self.box, v)[0]
        return self.acc[..., self.box[0][2] - z0:self.box[1][2] - z0]


class DftEntries:
    """The entries of one monitor, and (HIP backend) its device tables: one
    per set of field arrays seen, so the table is built once per monitor and
    ping-pong state, not once per call."""

    def __init__(self, k: int):
        self.k = int(k)
        self.rows: List[DftEntry] = []
        self.tables = {}

    def add(self, field: torch.Tensor, box: Box, kind: int) -> DftEntry:
        v = vec_width(field.dtype)
        acc = torch.zeros(acc_shape(box, self.k, v), dtype=field.dtype, device=field.device)
        e = DftEntry(field, box, acc, kind)
        self.rows.append(e)
        self.tables.clear()
        return e

    def __iter__(self):
        return iter(self.rows)

    def __len__(self):
        return len(self.rows)
