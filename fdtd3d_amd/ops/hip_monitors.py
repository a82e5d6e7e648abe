"""The monitor operations of the HIP backend, a mixin of
:class:`~.hip_ops.HipOps`: ``dft_accumulate``, ``dft_flux``, ``dft_farfield``,
``field_sumsq``, ``probe_sample`` and ``source_inject`` (csrc/dft_, flux_,
farfield_, energy_, probe_, source_kernels.hip).  Each
runs from a device table of fixed-size entries, built once per monitor (and
set of arrays) and cached on its entries / terms; the builders validate all
the kernels rely on, which check nothing beyond their boxes.
"""

from __future__ import annotations

import numpy as np
import torch

from .dft import (DFT_ENT_SIZE, DFT_MAX_K, FAR_ENT_SIZE, FAR_GROUP, FAR_SLOTS, FLUX_ENT_SIZE, acc_shape, vec_width,
                  z_pad)
from .energy import ENERGY_ENT_SIZE
from .hip_lib import HipError, _check, _ptr, _stream, c_double, c_int
from .probe import PROBE_ENT_SIZE


def _ent_table(n: int, size: int):
    """``n`` zeroed entries of ``size`` bytes: (int64, int32, float64) views."""
    e64 = np.zeros((n, size // 8), dtype=np.int64)
    return e64, e64.view(np.int32), e64.view(np.float64)


def _put_operand(e64, e32, r: int, op, base: int, plane: int, sx: int, sy: int, first: int, avg: int,
                 flags: int = 0) -> None:
    """A ``FluxOperand`` into row ``r``: base pointer and plane size (int64
    columns), strides, first sample and averaging bits | ``flags`` (int32)."""
    nx, ny, nz = op.acc.shape[2:]
    e64[r, base] = op.acc.data_ptr()
    e64[r, plane] = nx * ny * nz
    e32[r, sx], e32[r, sy] = ny * nz, nz
    e32[r, first:first + 3] = op.first
    e32[r, avg] = sum(1 << a for a in range(3) if op.avg[a]) | flags


class HipMonitorOps:
    """Needs ``lib``, ``fn``, ``device``, ``dtype``, ``launches`` and
    ``_check_tensor`` of :class:`~.hip_ops.HipOps`."""

    def _check_ent_size(self, name: str, fn: str, size: int) -> None:
        if int(getattr(self.lib.raw, "fdtd_%s_ent_size" % fn)()) != size:
            raise HipError("%sEnt layout mismatch" % name)

    def _check_operand(self, op_name: str, operand, extent, k: int, too_large: str = "accumulator block too large"):
        """A device tensor of the backend's precision whose samples for a face
        of ``extent`` cells stay inside its aligned block of < 2^31 elements."""
        self._check_tensor(operand.acc)
        why = operand.reach_error(extent, k)
        if why:
            raise HipError("%s: %s" % (op_name, why))
        if operand.acc.data_ptr() % 16:
            raise HipError("%s: accumulators must be 16-byte aligned" % op_name)
        if operand.acc[0, 0].numel() >= 2 ** 31:
            raise HipError("%s: %s" % (op_name, too_large))

    # ----------------------------------------------------------- DFT monitors
    def _dft_table(self, entries):
        """(device table, entries, blocks) of a monitor's non-empty entries
        with their current field arrays; every box checked against its array."""
        if not 1 <= entries.k <= DFT_MAX_K:
            raise HipError("dft_accumulate: 1..%d frequencies, got %d" % (DFT_MAX_K, entries.k))
        self._check_ent_size("Dft", "dft", DFT_ENT_SIZE)
        if int(self.lib.raw.fdtd_dft_max_k()) != DFT_MAX_K:
            raise HipError("DftEnt layout mismatch")
        v = vec_width(self.dtype)
        rows = []
        blk = 0
        for e in entries:
            if e.empty:
                continue
            self._check_tensor(e.field)
            self._check_tensor(e.acc, acc_shape(e.box, entries.k, v))
            if e.field.dim() != 3:
                raise HipError("dft_accumulate: 3D field arrays")
            for d in range(3):
                if e.box[0][d] < 0 or e.box[1][d] > e.field.shape[d]:
                    raise HipError("dft_accumulate: box %s outside array %s" % (e.box, tuple(e.field.shape)))
            if e.kind not in (0, 1):
                raise HipError("dft_accumulate: kind 0 (E) or 1 (H)")
            if e.acc.data_ptr() % 16:
                raise HipError("dft_accumulate: accumulators must be 16-byte aligned")
            groups = (e.box[1][0] - e.box[0][0]) * (e.box[1][1] - e.box[0][1]) * (z_pad(e.box, v)[1] // v)
            nb = -(-groups // 256)
            if groups >= 2 ** 31 - 256 or blk + nb >= 2 ** 31:
                raise HipError("dft_accumulate: monitor too large for one launch")
            vec = e.field.shape[2] % v == 0 and e.field.data_ptr() % 16 == 0
            rows.append((e, blk, 1 if vec else 0))
            blk += nb
        if not rows:
            return None
        e64, e32, _ = _ent_table(len(rows), DFT_ENT_SIZE)
        for r, (e, b0, vec) in enumerate(rows):
            e64[r, 0] = e.field.data_ptr()
            e64[r, 1] = e.acc.data_ptr()
            e32[r, 4], e32[r, 5] = e.field.shape[1], e.field.shape[2]
            e32[r, 6:9] = e.box[0]
            e32[r, 9:12] = e.box[1]
            e32[r, 12], e32[r, 13], e32[r, 14] = b0, e.kind, vec
        return (torch.from_numpy(e64).to(self.device), len(rows), blk)

    def dft_accumulate(self, entries, twiddles) -> None:
        """One sample of a running-DFT monitor (ops/dft.py ``DftEntries``) in
        ONE launch over all its entries (dft_kernels.hip k_dft_accum):
        ``re[k] += f cos``, ``im[k] += f sin`` with ``twiddles[kind][k] =
        (cos, sin)`` passed by value.  The device table is cached on the
        monitor per set of field arrays (F / F_alt ping-pong: the current
        arrays are looked up at every call)."""
        key = tuple((e.field.data_ptr(), tuple(e.field.shape), e.acc.data_ptr(), e.box, e.kind) for e in entries)
        tab = entries.tables.get(key, False)
        if tab is False:
            tab = entries.tables[key] = self._dft_table(entries)
        if len(twiddles) != 2 or any(len(row) != entries.k or any(len(cs) != 2 for cs in row) for row in twiddles):
            raise HipError("dft_accumulate: twiddles of shape (2, %d, 2)" % entries.k)
        if tab is None:
            return
        table, n, nblocks = tab
        flat = [float(x) for row in twiddles for cs in row for x in cs]
        rc = self.fn("dft_accum")(_ptr(table), c_int(n), c_int(nblocks), c_int(entries.k),
                                  (c_double * len(flat))(*flat), _stream())
        _check(rc, "dft_accum")
        self.launches += 1

    # ---------------------------------------------------------- flux monitors
    def _flux_table(self, terms):
        """(device table, entries, blocks, face block starts, partials) of a
        flux monitor's non-empty terms, ordered by face; every operand's
        reach checked against its accumulator block."""
        if not 1 <= terms.k <= DFT_MAX_K:
            raise HipError("dft_flux: 1..%d frequencies, got %d" % (DFT_MAX_K, terms.k))
        if terms.faces < 1:
            raise HipError("dft_flux: at least one face")
        self._check_ent_size("Flux", "flux", FLUX_ENT_SIZE)
        v = vec_width(self.dtype)
        rows = []
        fblk = [0] * (terms.faces + 1)
        blk = 0
        for face in range(terms.faces):
            fblk[face] = blk
            for t in terms:
                if t.face != face or t.empty:
                    continue
                for op in (t.e, t.h):
                    self._check_operand("dft_flux", op, t.extent, terms.k)
                cells = t.extent[0] * t.extent[1] * t.extent[2]
                nb = -(-cells // 256)
                if cells >= 2 ** 31 - 256 or blk + nb >= 2 ** 31:
                    raise HipError("dft_flux: monitor too large for one launch")
                # z-normal faces: a lane loads the aligned 16-byte group around its z samples
                zvec = t.extent[2] == 1 and all(op.acc.shape[4] % v == 0 for op in (t.e, t.h))
                rows.append((t, blk, 1 if zvec else 0))
                blk += nb
        fblk[terms.faces] = blk
        e64, e32, _ = _ent_table(max(1, len(rows)), FLUX_ENT_SIZE)
        for r, (t, b0, zvec) in enumerate(rows):
            for c, op in enumerate((t.e, t.h)):
                _put_operand(e64, e32, r, op, base=c, plane=2 + c, sx=8 + 2 * c, sy=9 + 2 * c, first=12 + 3 * c,
                             avg=21 + c)
            e32[r, 18:21] = t.extent
            e32[r, 23], e32[r, 24], e32[r, 25], e32[r, 26] = t.face, t.sign, b0, zvec
        table = torch.from_numpy(e64).to(self.device)
        fb = torch.tensor(fblk, dtype=torch.int32).to(self.device)
        partials = torch.empty((max(1, blk), terms.k), dtype=torch.float64, device=self.device)
        return (table, len(rows), blk, fb, partials)

    def dft_flux(self, terms) -> torch.Tensor:
        """(faces, K) float64 on the device: per term ``sign * sum over the
        face cells of (Re e Re h + Im e Im h)`` added to its face's row
        (ops/dft.py ``FluxTerms``), operands averaged, multiplied and summed
        in fp64 -- one launch over every term and frequency plus one that
        folds the blocks' partial sums per face in a fixed order
        (flux_kernels.hip; no atomics, so the same input gives the same
        bits).  The device table is cached on ``terms`` (its accumulators are
        fixed; ``FluxTerms.add`` drops it)."""
        key = tuple((t.e.acc.data_ptr(), t.h.acc.data_ptr()) for t in terms)
        if terms.table is None or terms.table[0] != key:
            terms.table = (key, self._flux_table(terms))
        table, n, nblocks, fblk, partials = terms.table[1]
        out = torch.empty((terms.faces, terms.k), dtype=torch.float64, device=self.device)
        rc = self.fn("flux_eval")(_ptr(table), c_int(n), c_int(nblocks), c_int(terms.k), _ptr(fblk),
                                  c_int(terms.faces), _ptr(partials), _ptr(out), _stream())
        _check(rc, "flux_eval")
        self.launches += 2 if nblocks else 1
        return out

    # ----------------------------------------------------- far-field monitors
    FAR_TARGET_BLOCKS = 1024  # few directions: a face's cells are split over blocks until the launch has this many
    FAR_MAX_SPLITS = 8        # ... at most this many per face group: the partials stay (4 / 6) groups x 8 x `out`

    def _far_table(self, terms, A: int):
        """(device table, groups, blocks, fold table, partials) of a far-field
        monitor's non-empty terms for ``A`` directions; every operand's reach
        checked against its accumulator block.  Terms that share extent and
        first cell form a group of up to 4 (one phase factor serves them), in
        the order of their first term; the fold table keeps the terms' own
        order per slot."""
        K = terms.k
        if not 1 <= K <= DFT_MAX_K:
            raise HipError("dft_farfield: 1..%d wavelengths, got %d" % (DFT_MAX_K, K))
        self._check_ent_size("Far", "farfield", FAR_ENT_SIZE)
        v = vec_width(self.dtype)
        groups, where = [], {}  # [terms of the group]; (extent, pos0) -> the open group
        member = []             # per non-empty term: (group, current)
        too_large = "accumulator block or face too large"
        for t in terms:
            if t.empty:
                continue
            self._check_operand("dft_farfield", t.operand, t.extent, K, too_large)
            if t.extent[0] * t.extent[1] * t.extent[2] >= 2 ** 31 - 256:
                raise HipError("dft_farfield: " + too_large)
            key = (t.extent, t.pos0)
            g = where.get(key)
            if g is None or len(groups[g]) == FAR_GROUP:
                g = where[key] = len(groups)
                groups.append([])
            member.append((t, g, len(groups[g])))
            groups[g].append(t)
        tiles = -(-A // 256)
        per_group = K * tiles
        want = -(-self.FAR_TARGET_BLOCKS // max(1, len(groups) * per_group))
        e64, e32, f64 = _ent_table(max(1, len(groups)), FAR_ENT_SIZE)
        blk, prow, prow0 = 0, 0, []
        for r, grp in enumerate(groups):
            ext = grp[0].extent
            chunks = -(-(ext[0] * ext[1] * ext[2]) // 256)
            splits = max(1, min(want, self.FAR_MAX_SPLITS, chunks))
            if blk + splits * per_group >= 2 ** 31:
                raise HipError("dft_farfield: too many directions for one launch")
            f64[r, 8:11] = grp[0].pos0
            for c, t in enumerate(grp):
                # z-normal faces: a lane loads the aligned 16-byte group around its z samples
                zvec = t.extent[2] == 1 and t.operand.acc.shape[4] % v == 0
                _put_operand(e64, e32, r, t.operand, base=c, plane=4 + c, sx=22 + c, sy=26 + c, first=30 + 3 * c,
                             avg=42 + c, flags=8 if zvec else 0)
            e32[r, 46:49] = ext
            e32[r, 49], e32[r, 50], e32[r, 51], e32[r, 52] = len(grp), blk, splits, prow
            prow0.append((prow, splits))
            blk += splits * per_group
            prow += splits
        fold = [0] * (FAR_SLOTS + 1)
        rows = []
        for slot in range(FAR_SLOTS):
            fold[slot] = len(rows) // 3
            for t, g, c in member:
                if t.slot == slot:
                    for s in range(prow0[g][1]):
                        rows += [prow0[g][0] + s, c, t.sign]
        fold[FAR_SLOTS] = len(rows) // 3
        if prow * K * FAR_GROUP * A * 2 >= 2 ** 40:
            raise HipError("dft_farfield: too many directions for one call")
        table = torch.from_numpy(e64).to(self.device)
        fd = torch.tensor(fold + rows, dtype=torch.int32).to(self.device)
        partials = torch.empty((max(1, prow), K, FAR_GROUP, A, 2), dtype=torch.float64, device=self.device)
        return (table, len(groups), blk, fd, partials)

    def dft_farfield(self, terms, dirs, wavenumbers) -> torch.Tensor:
        """(K, A, 6, 2) float64 on the device: the radiation vectors ``N_x,
        N_y, N_z, L_x, L_y, L_z`` (re, im) of ``terms`` (ops/dft.py
        ``FarTerms``) in the directions ``dirs`` (A, 3) fp64 at
        ``wavenumbers`` (K,) fp64, averaged and summed in fp64 from the raw
        accumulators -- one launch over every face group, direction and
        wavelength plus one that folds the partial sums per slot in a fixed
        order (farfield_kernels.hip; no atomics, so the same input gives the
        same bits).  The device table is cached on ``terms`` per direction
        count (``FarTerms.add`` drops it)."""
        dirs = torch.as_tensor(dirs)
        wn = torch.as_tensor(wavenumbers)
        if dirs.dim() != 2 or dirs.shape[1] != 3 or dirs.dtype != torch.float64:
            raise HipError("dft_farfield: dirs of shape (A, 3) in float64, got %s %s" % (tuple(dirs.shape), dirs.dtype))
        if wn.dim() != 1 or wn.shape[0] != terms.k or wn.dtype != torch.float64:
            raise HipError("dft_farfield: %d wavenumbers in float64, got %s %s" % (terms.k, tuple(wn.shape), wn.dtype))
        A = int(dirs.shape[0])
        if A >= 2 ** 24:
            raise HipError("dft_farfield: at most 2^24 directions a call")
        key = (A,) + tuple(t.operand.acc.data_ptr() for t in terms)
        if terms.table is None or terms.table[0] != key:
            terms.table = (key, self._far_table(terms, A))
        table, n, nblocks, fold, partials = terms.table[1]
        out = torch.empty((terms.k, A, 6, 2), dtype=torch.float64, device=self.device)
        if A == 0:
            return out
        d = dirs.to(self.device).contiguous()
        w = wn.to(self.device).contiguous()
        rc = self.fn("farfield_eval")(_ptr(table), c_int(n), c_int(nblocks), c_int(terms.k), c_int(A), _ptr(d), _ptr(w),
                                      c_double(terms.dx), _ptr(fold), _ptr(partials), _ptr(out), _stream())
        _check(rc, "farfield_eval")
        self.launches += 2 if nblocks else 1
        return out

    # -------------------------------------------------------- energy monitors
    ENERGY_GROUPS_PER_BLOCK = 8192  # 16-byte groups a block walks at most (32 per thread)
    ENERGY_MIN_BLOCKS = 2048        # small boxes: fewer rows per block until the launch has this many blocks
    ENERGY_MERGE_MAX = 1 << 16      # longest row (elements) made by folding y into z
    ENERGY_MAX_TABLES = 4           # cached device tables per monitor (the F / F_alt ping-pong needs 2)

    def _energy_table(self, entries):
        """(device table, entries, blocks, rows per block, partials) of a
        monitor's non-empty entries with their current field arrays, or None
        where every box is empty; every box checked against its array."""
        if entries.R < 1:
            raise HipError("field_sumsq: at least one result row")
        self._check_ent_size("Energy", "energy", ENERGY_ENT_SIZE)
        v = vec_width(self.dtype)
        item = 16 // v
        rows = []

        def index(dev):
            return torch.cuda.current_device() if dev.index is None else dev.index

        for e in entries:
            t = e.field
            if t.device.type != "cuda" or index(t.device) != index(self.device):
                raise HipError("field_sumsq: tensor on %s, backend on %s" % (t.device, self.device))
            if t.dtype != self.dtype:
                raise HipError("field_sumsq: tensor of %s, backend of %s" % (t.dtype, self.dtype))
            if t.dim() != 3:
                raise HipError("field_sumsq: 3D field arrays")
            if not 0 <= e.row < entries.R:
                raise HipError("field_sumsq: row %d of %d" % (e.row, entries.R))
            lo, hi = e.box
            for d in range(3):
                if lo[d] < 0 or hi[d] > t.shape[d]:
                    raise HipError("field_sumsq: box %s outside array %s" % (e.box, tuple(t.shape)))
            if e.empty:
                continue
            sx, sy, sz = t.stride()
            if (sz != 1 and t.shape[2] > 1) or sx < 0 or sy < 0:
                raise HipError("field_sumsq: unit z stride and non-negative strides, got %s" % (t.stride(),))
            if t.data_ptr() % item:
                raise HipError("field_sumsq: field array not aligned to its element size")
            lo, ext = list(lo), [hi[d] - lo[d] for d in range(3)]
            # a box over whole short z rows of a row-contiguous array: fold y into z (2D / 1D layouts keep z = 1)
            if lo[2] == 0 and ext[2] == t.shape[2] and sy == t.shape[2] and ext[1] * ext[2] <= self.ENERGY_MERGE_MAX:
                lo, ext, sy = [lo[0], 0, lo[1] * sy], [ext[0], 1, ext[1] * ext[2]], 0
            if max(sx, sy) >= 2 ** 31 or ext[0] * ext[1] >= 2 ** 31 or lo[2] + ext[2] >= 2 ** 31 - 16:
                raise HipError("field_sumsq: stride or extent overflows int32 (%s, %s)" % (t.stride(), e.box))
            z0, z1 = lo[2] & ~(v - 1), -(-(lo[2] + ext[2]) // v) * v
            # vector loads read the aligned groups [z0, z1) of every row: every row start 16-byte aligned, and the
            # last group of the last row inside the allocation
            last = (lo[0] + ext[0] - 1) * sx + (lo[1] + ext[1] - 1) * sy + z1
            room = t.untyped_storage().nbytes() // item - t.storage_offset()
            vec = t.data_ptr() % 16 == 0 and sx % v == 0 and sy % v == 0 and last <= room
            rows.append((e, lo, ext, sx, sy, (z1 - z0) // v, 1 if vec else 0))
        if not rows:
            return None
        zg = max(r[5] for r in rows)
        total = sum(r[2][0] * r[2][1] for r in rows)
        rows_blk = max(1, min(self.ENERGY_GROUPS_PER_BLOCK // zg, total // self.ENERGY_MIN_BLOCKS))
        e64, e32, _ = _ent_table(len(rows), ENERGY_ENT_SIZE)
        blk = 0
        for r, (e, lo, ext, sx, sy, g, vec) in enumerate(rows):
            nb = -(-(ext[0] * ext[1]) // rows_blk)
            if rows_blk * g >= 2 ** 31 - 4 * 256 or blk + nb >= 2 ** 31:
                raise HipError("field_sumsq: too many blocks for one launch")
            e64[r, 0] = e.field.data_ptr()
            e32[r, 2], e32[r, 3] = sx, sy
            e32[r, 4:7] = lo
            e32[r, 7:10] = ext
            e32[r, 10], e32[r, 11], e32[r, 12], e32[r, 13] = e.row, blk, nb, vec
            blk += nb
        table = torch.from_numpy(e64).to(self.device)
        partials = torch.empty((blk,), dtype=torch.float64, device=self.device)
        return (table, len(rows), blk, rows_blk, partials)

    def field_sumsq(self, entries) -> torch.Tensor:
        """(R,) float64 on the device: per entry the sum over its box of the
        squares of the field, every element converted to fp64 first, added to
        the entry's row (ops/energy.py ``EnergyEntries``) -- one launch over
        every entry plus one that folds the blocks' partial sums per row in a
        fixed order (energy_kernels.hip; no atomics, so the same input gives
        the same bits).  Everything is validated before the first launch.  The
        device table is cached on ``entries`` per set of field arrays (F /
        F_alt ping-pong: the current arrays are looked up at every call)."""
        key = tuple((e.field.data_ptr(), tuple(e.field.shape), tuple(e.field.stride()), e.field.dtype,
                     e.field.device, e.field.storage_offset(), e.field.untyped_storage().nbytes(), e.box, e.row)
                    for e in entries)
        tab = entries.tables.get(key, False)
        if tab is False:
            tab = self._energy_table(entries)
            if len(entries.tables) >= self.ENERGY_MAX_TABLES:
                entries.tables.clear()  # reallocated field arrays: drop the tables (and partials) of the old ones
            entries.tables[key] = tab
        out = torch.empty((entries.R,), dtype=torch.float64, device=self.device)
        if tab is None:
            table, n, nblocks, rows_blk, partials = None, 0, 0, 1, None
        else:
            table, n, nblocks, rows_blk, partials = tab
        rc = self.fn("energy_eval")(_ptr(table), c_int(n), c_int(nblocks), c_int(rows_blk), c_int(entries.R),
                                    _ptr(partials), _ptr(out), _stream())
        _check(rc, "energy_eval")
        self.launches += 2 if nblocks else 1
        return out

    # --------------------------------------------------------- probe monitors
    PROBE_MAX_TABLES = 4  # cached device tables per monitor (the F / F_alt ping-pong needs 2)

    def _probe_table(self, entries):
        """The device table of a monitor's slots with their current field
        arrays (None without slots); every array and offset checked."""
        self._check_ent_size("Probe", "probe", PROBE_ENT_SIZE)
        item = 16 // vec_width(self.dtype)
        for f in entries.fields:
            self._check_tensor(f)
            if f.device != entries.series.device:
                raise HipError("probe_sample: array on %s, series on %s" % (f.device, entries.series.device))
            if f.data_ptr() % item:
                raise HipError("probe_sample: field array not aligned to its element size")
        why = entries.offset_error()
        if why:
            raise HipError("probe_sample: " + why)
        if len(entries) >= 2 ** 31 - 256:
            raise HipError("probe_sample: too many slots for one launch")
        if not len(entries):
            return None
        e64, _, _ = _ent_table(len(entries), PROBE_ENT_SIZE)
        for s, (fi, off) in enumerate(entries.rows):
            e64[s, 0] = entries.fields[fi].data_ptr()
            e64[s, 1] = off
        return torch.from_numpy(e64).to(self.device)

    def probe_sample(self, entries, row: int) -> None:
        """One sample of a probe monitor (ops/probe.py ``ProbeEntries``) in
        ONE launch over all its slots (probe_kernels.hip k_probe_sample): row
        ``row`` of ``entries.series`` = every slot's element, widened to fp64,
        ``row`` passed by value.  Everything is validated before the launch.
        The device table is cached on ``entries`` per set of field arrays (F /
        F_alt ping-pong: the current arrays are looked up at every call)."""
        row = int(row)
        if not 0 <= row < entries.capacity:
            raise HipError("probe_sample: row %d of %d" % (row, entries.capacity))
        series = entries.series
        if (series.device.type != "cuda" or series.dtype != torch.float64 or not series.is_contiguous()
                or tuple(series.shape) != (entries.capacity, len(entries))):
            raise HipError("probe_sample: series of %d x %d float64 on the device, got %s %s on %s"
                           % (entries.capacity, len(entries), tuple(series.shape), series.dtype, series.device))
        key = tuple((f.data_ptr(), f.numel(), f.dtype, f.device, f.is_contiguous()) for f in entries.fields)
        tab = entries.tables.get(key, False)
        if tab is False:
            tab = self._probe_table(entries)
            if len(entries.tables) >= self.PROBE_MAX_TABLES:
                entries.tables.clear()  # reallocated field arrays: drop the tables of the old ones
            entries.tables[key] = tab
        if tab is None:
            return
        rc = self.fn("probe_sample")(_ptr(tab), c_int(len(entries)), _ptr(series), c_int(row),
                                     c_int(entries.capacity), _stream())
        _check(rc, "probe_sample")
        self.launches += 1

    # ------------------------------------------------------------ source lists
    def _source_table(self, entries, kind: str):
        """The device table of a source list's entries of ``kind`` with their
        current field arrays (rows sorted by cell, ops/source.py)."""
        from .source import FLAG_HARD, FLAG_SAME, SOURCE_ENT_SIZE, SOURCE_MAX_SIGNALS
        self._check_ent_size("Src", "source", SOURCE_ENT_SIZE)
        if int(self.lib.raw.fdtd_source_max_signals()) != SOURCE_MAX_SIGNALS:
            raise HipError("SrcEnt layout mismatch")
        rows = entries.rows[kind]
        item = 16 // vec_width(self.dtype)
        for fi in sorted({r[0] for r in rows}):
            f = entries.fields[fi]
            self._check_tensor(f)
            if f.data_ptr() % item:
                raise HipError("source_inject: field array not aligned to its element size")
        if len(rows) >= 2 ** 31 - 256:
            raise HipError("source_inject: too many entries for one launch")
        e64, e32, ef = _ent_table(len(rows), SOURCE_ENT_SIZE)
        prev = None
        for n, (fi, off, amp, sig, hard) in enumerate(rows):
            e64[n, 0] = entries.fields[fi].data_ptr()
            e64[n, 1] = off
            ef[n, 2] = amp
            e32[n, 6] = sig
            e32[n, 7] = (FLAG_SAME if (fi, off) == prev else 0) | (FLAG_HARD if hard else 0)
            prev = (fi, off)
        return torch.from_numpy(e64).to(self.device)

    def source_inject(self, entries, kind: str, values) -> None:
        """One half step of a source list (ops/source.py ``SourceEntries``)
        in ONE launch over all its entries of ``kind`` (source_kernels.hip
        k_source_inject), ``values`` (the signals' fp64 values at this half
        step) passed by value.  Every offset and signal index is validated
        when the device table is built; the table, its length and the signal
        count it needs are cached on ``entries`` per kind and set of field
        arrays (F / F_alt ping-pong), so a launch checks the value count only
        -- nothing per launch grows with the list."""
        try:
            key = entries.key(kind)
        except ValueError as e:
            raise HipError("source_inject: %s" % e)
        cached = entries.tables.get(key)
        if cached is None:
            why = entries.table_error(kind)
            if why:
                raise HipError("source_inject: " + why)
            rows = entries.rows[kind]
            cached = (self._source_table(entries, kind) if rows else None, len(rows), entries.signals_needed(kind))
            if len(entries.tables) >= 2 * self.PROBE_MAX_TABLES:
                entries.tables.clear()  # reallocated field arrays: drop the tables of the old ones
            entries.tables[key] = cached
        tab, nrows, needed = cached
        why = entries.values_error(len(values), needed)
        if why:
            raise HipError("source_inject: " + why)
        if not nrows:
            return
        vals = (c_double * len(values))(*values)
        rc = self.fn("source_inject")(_ptr(tab), c_int(nrows), vals, c_int(len(values)), _stream())
        _check(rc, "source_inject")
        self.launches += 1
