"""Entries of a running-DFT monitor, shared by both backends'
``dft_accumulate(entries, twiddles)``.

One entry = one (field array, array-local box, accumulators, kind).  The
accumulators of an entry are box-local, ``[k][re|im][x][y][z']``, where the z'
extent is the box's z range widened to the field's 16-byte groups (from ``lo &
~(V - 1)`` to ``hi`` rounded up, ``V`` = 4 fp32 / 2 fp64 elements): an
accumulator vector and its field vector start at the same z (csrc/
dft_kernels.hip).  The padded cells are never written and stay zero.

``FluxTerms`` describe what ``dft_flux(terms)`` evaluates from such
accumulators: products of face-centre averages summed over the faces of a box
(models/flux.py; csrc/flux_kernels.hip).  ``FarTerms`` describe what
``dft_farfield(terms, dirs, wavenumbers)`` evaluates from them: the radiation
vectors of the equivalent currents on the faces (models/farfield.py; csrc/
farfield_kernels.hip).  HIP ops and device tables: ops/hip_monitors.py.
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


class _Rows:
    """A monitor's entries or terms: iterates over, and counts, its ``rows``."""

    def __iter__(self):
        return iter(self.rows)

    def __len__(self):
        return len(self.rows)


class DftEntries(_Rows):
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


# ------------------------------------------------------------------ flux terms
FLUX_ENT_SIZE = 112  # bytes of a device table entry of ``dft_flux`` (fdtd_flux_ent_size)


class FluxOperand:
    """One factor of a flux product: ``acc`` = accumulators in the padded
    ``acc_shape`` layout ``[k][re|im][x][y][z']``, ``first`` = the accumulator
    index of the first sample of the first face cell per axis, ``avg`` = per
    axis whether the face-centre value averages the samples ``first`` and
    ``first + 1`` (models/ntff.py ``_sample_plan``)."""
    __slots__ = ("acc", "first", "avg")

    def __init__(self, acc: torch.Tensor, first, avg):
        self.acc = acc
        self.first = tuple(int(v) for v in first)
        self.avg = tuple(bool(v) for v in avg)

    def reach_error(self, extent, k: int) -> Optional[str]:
        """Why the operand's samples for a face of ``extent`` cells leave its
        accumulator block (None: they do not)."""
        if self.acc.dim() != 5 or self.acc.shape[0] != k or self.acc.shape[1] != 2:
            return "accumulators of shape (%d, 2, x, y, z'), got %s" % (k, tuple(self.acc.shape))
        for a in range(3):
            last = self.first[a] + extent[a] - 1 + (1 if self.avg[a] else 0)
            if self.first[a] < 0 or last >= self.acc.shape[2 + a]:
                return "samples %d..%d along axis %d outside the accumulator block %s" % (
                    self.first[a], last, a, tuple(self.acc.shape[2:]))
        return None

    def centre(self, extent) -> torch.Tensor:
        """(K, 2) + ``extent`` float64: the face-centre average of the 1, 2 or
        4 samples around every cell of a face (the torch backend's ops)."""
        acc, cnt = None, 0
        for ox in ((0, 1) if self.avg[0] else (0,)):
            for oy in ((0, 1) if self.avg[1] else (0,)):
                for oz in ((0, 1) if self.avg[2] else (0,)):
                    o = (ox, oy, oz)
                    sl = tuple(slice(self.first[a] + o[a], self.first[a] + o[a] + extent[a]) for a in range(3))
                    v = self.acc[(slice(None), slice(None)) + sl].to(torch.float64)
                    acc = v if acc is None else acc + v
                    cnt += 1
        return acc / cnt


class FluxTerm:
    """``sign * sum over the face cells of (Re e Re h + Im e Im h)`` added to
    row ``face`` of the result; ``extent`` = the face's cells per axis (1
    along its normal)."""
    __slots__ = ("face", "sign", "extent", "e", "h")

    def __init__(self, face: int, sign: int, extent, e: FluxOperand, h: FluxOperand):
        if sign not in (1, -1):
            raise ValueError("FluxTerm: sign +1 or -1")
        self.face, self.sign = int(face), int(sign)
        self.extent = tuple(int(v) for v in extent)
        self.e, self.h = e, h

    @property
    def empty(self) -> bool:
        return any(v <= 0 for v in self.extent)


class FluxTerms(_Rows):
    """The products of one flux monitor (``ops.dft_flux``) and, on the HIP
    backend, its cached device table."""

    def __init__(self, k: int, faces: int):
        self.k, self.faces = int(k), int(faces)
        self.rows: List[FluxTerm] = []
        self.table = None

    def add(self, term: FluxTerm) -> FluxTerm:
        if not 0 <= term.face < self.faces:
            raise ValueError("FluxTerms: face %d of %d" % (term.face, self.faces))
        self.rows.append(term)
        self.table = None
        return term


# ------------------------------------------------------------- far-field terms
FAR_ENT_SIZE = 216   # bytes of a device table entry of ``dft_farfield`` (fdtd_farfield_ent_size)
FAR_GROUP = 4        # terms of one face group: they share the cells and so the phase factors
FAR_SLOTS = 6        # N_x, N_y, N_z, L_x, L_y, L_z


class FarTerm:
    """``sign * sum over the face cells c of avg(acc[k, 0] + i acc[k, 1])(c)
    exp(-i kappa_k rhat . r'(c))`` added to component ``slot`` (0..5: ``N_x,
    N_y, N_z, L_x, L_y, L_z``) of the radiation vectors; ``r'(c) = pos0 + dx *
    (cell index)``, ``pos0`` the first face-cell centre in metres relative to
    the phase origin, ``extent`` the face's cells per axis (1 along its
    normal), ``operand`` a :class:`FluxOperand`."""
    __slots__ = ("slot", "sign", "extent", "operand", "pos0")

    def __init__(self, slot: int, sign: int, extent, operand: FluxOperand, pos0):
        if sign not in (1, -1):
            raise ValueError("FarTerm: sign +1 or -1")
        if not 0 <= int(slot) < FAR_SLOTS:
            raise ValueError("FarTerm: slot 0..%d" % (FAR_SLOTS - 1))
        self.slot, self.sign = int(slot), int(sign)
        self.extent = tuple(int(v) for v in extent)
        self.operand = operand
        self.pos0 = tuple(float(v) for v in pos0)
        if len(self.extent) != 3 or len(self.pos0) != 3:
            raise ValueError("FarTerm: extent and pos0 per axis")

    @property
    def empty(self) -> bool:
        return any(v <= 0 for v in self.extent)


class FarTerms(_Rows):
    """The currents of one far-field monitor (``ops.dft_farfield``) at ``k``
    wavelengths on a grid of step ``dx`` and, on the HIP backend, its cached
    device table."""

    def __init__(self, k: int, dx: float):
        self.k, self.dx = int(k), float(dx)
        self.rows: List[FarTerm] = []
        self.table = None

    def add(self, term: FarTerm) -> FarTerm:
        self.rows.append(term)
        self.table = None
        return term
