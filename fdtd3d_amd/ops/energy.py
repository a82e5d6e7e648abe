"""Entries of a field-energy monitor, shared by both backends'
``field_sumsq(entries)``: sums of squares over boxes of field arrays.

One entry = one (field array, array-local box, result row); several entries
may add to the same row, empty boxes contribute 0 and a row without entries is
exactly 0 (models/energy.py; csrc/energy_kernels.hip).
"""

from __future__ import annotations

from typing import List, Tuple

import torch

from .dft import _Rows, box_empty

Box = Tuple[Tuple[int, int, int], Tuple[int, int, int]]

ENERGY_ENT_SIZE = 64  # bytes of a device table entry of ``field_sumsq`` (fdtd_energy_ent_size)


class EnergyEntry:
    """``field`` is the array summed at the next call (a monitor re-resolves
    it before every call: the scheme's F / F_alt ping-pong), ``box`` its
    array-local box, ``row`` the row of the result the sum is added to."""
    __slots__ = ("field", "box", "row")

    def __init__(self, field: torch.Tensor, box: Box, row: int):
        self.field = field
        self.box = (tuple(int(v) for v in box[0]), tuple(int(v) for v in box[1]))
        self.row = int(row)

    @property
    def empty(self) -> bool:
        return box_empty(self.box)


class EnergyEntries(_Rows):
    """The entries of one monitor with ``R`` result rows and (HIP backend) its
    device tables: one per set of field arrays seen, so the table is built
    once per monitor and ping-pong state, not once per call."""

    def __init__(self, rows: int):
        self.R = int(rows)
        self.rows: List[EnergyEntry] = []
        self.tables = {}

    def add(self, field: torch.Tensor, box: Box, row: int) -> EnergyEntry:
        if not 0 <= int(row) < self.R:
            raise ValueError("EnergyEntries: row %d of %d" % (row, self.R))
        e = EnergyEntry(field, box, row)
        self.rows.append(e)
        self.tables.clear()
        return e
