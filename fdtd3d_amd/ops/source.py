"""Entries of a source list, shared by both backends' ``source_inject(entries,
kind, values)``: single elements of field arrays driven by a signal.

One entry = (field array, linear element offset into it, fp64 amplitude,
signal index, hard).  A launch handles the entries of one kind (``"E"`` or
``"H"``) and takes the signals' values at that half step: every distinct cell
becomes ``round(start + sum_k amplitude_k * values[signal_k])`` in fp64, the
terms added in table order, ``start`` the cell's value widened to fp64 -- or 0
when the cell's first entry is hard (layout/source_file.py refuses a hard
entry that shares its cell).  The rows of a kind are kept sorted by cell
(array, offset), entries of one cell in the order they were added.

The arrays are kept once each (``fields``; an entry names one by index), so a
scheme re-resolves its F / F_alt ping-pong per array, not per entry.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

SOURCE_ENT_SIZE = 32      # bytes of a device table entry of ``source_inject`` (fdtd_source_ent_size)
SOURCE_MAX_SIGNALS = 64   # signal values of one launch (fdtd_source_max_signals)
FLAG_SAME, FLAG_HARD = 1, 2

Row = Tuple[int, int, float, int, bool]  # (index into fields, element offset, amplitude, signal, hard)


class SourceEntries:
    """The entries of one source list on one rank -- ``rows[kind]`` = [(index
    into ``fields``, element offset, amplitude, signal index, hard)] -- and
    (HIP backend) its device tables: one per kind and set of field arrays."""

    def __init__(self):
        self.fields: List[torch.Tensor] = []
        self.rows: Dict[str, List[Row]] = {"E": [], "H": []}
        self.tables = {}

    def add_field(self, field: torch.Tensor) -> int:
        """Register an array; the index its entries name it by."""
        self.fields.append(field)
        return len(self.fields) - 1

    def add(self, kind: str, field: int, offset: int, amplitude: float, signal: int, hard: bool = False) -> None:
        if kind not in self.rows:
            raise ValueError("SourceEntries: kind E or H, got %r" % (kind,))
        if not 0 <= int(field) < len(self.fields):
            raise ValueError("SourceEntries: array %d of %d" % (field, len(self.fields)))
        rows = self.rows[kind]
        rows.append((int(field), int(offset), float(amplitude), int(signal), bool(hard)))
        rows.sort(key=lambda r: (r[0], r[1]))  # stable: a cell's entries keep their order
        self.tables.clear()

    def cells(self, kind: str) -> int:
        """Distinct cells of a kind."""
        return len({(r[0], r[1]) for r in self.rows[kind]})

    def key(self, kind: str) -> tuple:
        """What a backend's cached table of ``kind`` depends on besides the
        rows (``add`` drops the tables): the arrays in their current roles."""
        if kind not in self.rows:
            raise ValueError("SourceEntries: kind E or H, got %r" % (kind,))
        return (kind,) + tuple((f.data_ptr(), f.numel(), f.dtype, f.device) for f in self.fields)

    def table_error(self, kind: str) -> Optional[str]:
        """Why the entries of ``kind`` cannot become a table (None: they
        can): every offset against its array, every signal index against the
        launch's limit.  Checked once per table, not per launch."""
        sizes = [f.numel() for f in self.fields]
        for n, (fi, off, _, sig, _) in enumerate(self.rows[kind]):
            if not 0 <= off < sizes[fi]:
                return "entry %d: element %d outside its array of %d elements" % (n, off, sizes[fi])
            if not 0 <= sig < SOURCE_MAX_SIGNALS:
                return "entry %d: signal %d, a launch takes %d signal values" % (n, sig, SOURCE_MAX_SIGNALS)
        return None

    def signals_needed(self, kind: str) -> int:
        """Signal values a launch of ``kind`` must bring: the largest index + 1."""
        return max((r[3] for r in self.rows[kind]), default=-1) + 1

    @staticmethod
    def values_error(nvalues: int, needed: int) -> Optional[str]:
        """The per-launch check: the value count against the limit and
        against the table's largest signal index."""
        if not 0 <= nvalues <= SOURCE_MAX_SIGNALS:
            return "%d signal values, a launch takes %d" % (nvalues, SOURCE_MAX_SIGNALS)
        if nvalues < needed:
            return "%d signal values, the entries name signal %d" % (nvalues, needed - 1)
        return None
