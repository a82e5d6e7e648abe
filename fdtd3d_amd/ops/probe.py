"""Slots of a probe monitor, shared by both backends' ``probe_sample(entries,
row)``: single elements of field arrays recorded as a time series.

One slot = one (field array, linear element offset into it).  A sample copies
every slot's element, widened to fp64, into row ``row`` of ``series``, a
row-major fp64 buffer of ``capacity`` rows and one column per slot that stays
on the arrays' device until someone reads it (models/probe.py; csrc/
probe_kernels.hip).  Slots hold raw Yee samples: means are formed on read.

The arrays are kept once each (``fields``; a slot names one by index), so a
monitor re-resolves the scheme's F / F_alt ping-pong per array, not per slot.
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from .dft import _Rows

PROBE_ENT_SIZE = 16  # bytes of a device table entry of ``probe_sample`` (fdtd_probe_ent_size)


class ProbeEntries(_Rows):
    """The slots of one monitor -- ``rows`` = [(index into ``fields``, element
    offset)] --, its ``series`` buffer of ``capacity`` rows on ``device`` and
    (HIP backend) its device tables: one per set of field arrays seen."""

    def __init__(self, capacity: int, device="cpu"):
        if int(capacity) < 1:
            raise ValueError("ProbeEntries: at least one row, got %d" % capacity)
        self.capacity = int(capacity)
        self.device = torch.device(device)
        self.fields: List[torch.Tensor] = []
        self.rows: List[Tuple[int, int]] = []
        self.tables = {}
        self._series: Optional[torch.Tensor] = None

    def add_field(self, field: torch.Tensor) -> int:
        """Register an array; the index its slots name it by."""
        self.fields.append(field)
        return len(self.fields) - 1

    def add(self, field: int, offset: int) -> int:
        """A slot on element ``offset`` of array ``field``; its column."""
        if not 0 <= int(field) < len(self.fields):
            raise ValueError("ProbeEntries: array %d of %d" % (field, len(self.fields)))
        self.rows.append((int(field), int(offset)))
        self.tables.clear()
        self._series = None
        return len(self.rows) - 1

    @property
    def series(self) -> torch.Tensor:
        """(capacity, slots) fp64, allocated (zeroed) at the first use after
        the last :meth:`add`."""
        if self._series is None:
            self._series = torch.zeros((self.capacity, len(self.rows)), dtype=torch.float64, device=self.device)
        return self._series

    def grow(self) -> None:
        """Twice the rows, the recorded ones kept (a run beyond its budget)."""
        self._series = torch.cat([self.series, torch.zeros_like(self.series)])
        self.capacity *= 2

    def offset_error(self) -> Optional[str]:
        """Why a slot does not lie inside its array (None: all do)."""
        for s, (fi, off) in enumerate(self.rows):
            n = self.fields[fi].numel()
            if not 0 <= off < n:
                return "slot %d: element %d outside its array of %d elements" % (s, off, n)
        return None
