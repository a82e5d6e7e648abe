"""Reference backend: every solver operation as vectorised torch ops.

This is the CPU oracle of the framework: it runs on
any torch device, is used by the CPU test-suite and is the numerics reference
the HIP kernels are compared against.  It implements exactly the same operation
interface as :class:`fdtd3d_amd.ops.hip_ops.HipOps`.

Operation semantics (shared by both backends):

* ``curl_update(kind, boxes, dst, src, cb)`` -- fast path
  ``dst[c] += cb[c] * curl(src)[c]`` on each component's local box.  ``curl``
  follows :data:`fdtd3d_amd.layout.yee.CURL_TERMS` (reference ``Kernels.h``).
* ``curl_update_lossy(boxes, dst, src, coefs)`` -- the E update of a lossy box,
  ``dst[c] = ca[c] * dst[c] + cb[c] * curl(src)[c]`` with box-local per-cell
  coefficients.
* ``curl_general(kind, comp, box, out, inp, src, ca, cb)`` --
  ``out = ca*inp + cb*curl(src)`` (UPML D/B update, ``Scheme3D.cpp:266-324``).
* ``lincomb(out, box, terms)`` -- ``out = sum coef_i * x_i`` (Drude ADE and
  E-from-D, ``Kernels.h:80-107``).
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..layout.yee import UPML_AXES, YeeLayout
from ..models.regions import RegionLevel
from .coef import Coef

Box = Tuple[Tuple[int, int, int], Tuple[int, int, int]]


def box_slices(box: Box) -> Tuple[slice, slice, slice]:
    return tuple(slice(box[0][d], box[1][d]) for d in range(3))


def _shift(sl, axis, off):
    s = list(sl)
    s[axis] = slice(sl[axis].start + off, sl[axis].stop + off)
    return tuple(s)


def _empty(box: Box) -> bool:
    return any(box[1][d] <= box[0][d] for d in range(3))


def box_intersect_(a: Box, b: Box) -> Box:
    return (tuple(max(a[0][d], b[0][d]) for d in range(3)), tuple(min(a[1][d], b[1][d]) for d in range(3)))


def cb_pad(cb: Dict[str, Coef]) -> Dict[str, Coef]:
    """Coefficients re-indexed for fields padded by one zero layer per side."""
    def p1(t):
        return None if t is None else torch.nn.functional.pad(t, (1, 1))

    def p3(t):
        return None if t is None else torch.nn.functional.pad(t, (1, 1, 1, 1, 1, 1))
    return {c: Coef(k.scalar, p1(k.px), p1(k.py), p1(k.pz), p3(k.cell)) for c, k in cb.items()}


class TorchOps:
    name = "torch"
    chain_rows = True  # same launch plan as the HIP backend (row-range dispersive split)
    region_aux = True  # chain_update addresses region-local D / D1 levels (models/regions.py)

    def __init__(self, layout: YeeLayout, device, dtype):
        self.layout = layout
        self.device = torch.device(device)
        self.dtype = dtype

    # ------------------------------------------------------------------ curl
    def curl(self, kind: str, comp: str, sl, src: Dict[str, torch.Tensor]):
        acc = None
        for (s, axis, sign) in self.layout.curl_terms(comp):
            S = src[s]
            if kind == "E":
                d = S[sl] - S[_shift(sl, axis, -1)]
            else:
                d = S[_shift(sl, axis, +1)] - S[sl]
            if acc is None:
                acc = d if sign > 0 else -d
            else:
                acc = acc + d if sign > 0 else acc - d
        return acc

    def curl_update(self, kind: str, boxes: Dict[str, Box], dst: Dict[str, torch.Tensor],
                    src: Dict[str, torch.Tensor], cb: Dict[str, Coef]) -> None:
        for comp, box in boxes.items():
            if _empty(box):
                continue
            sl = box_slices(box)
            c = self.curl(kind, comp, sl, src)
            if c is None:
                continue
            dst[comp][sl] += cb[comp].materialize(sl) * c

    def curl_update_lossy(self, boxes: Dict[str, Box], dst: Dict[str, torch.Tensor],
                          src: Dict[str, torch.Tensor], coefs) -> None:
        """The conductive E update of a lossy medium, ``dst[c] = ca[c] * dst[c]
        + cb[c] * curl(src)[c]`` on each E component's local box: ``coefs``
        (models/regions.py ``LossyCoefs``) holds one (ca, cb) pair per cell
        over its storage box, which contains every box.  The same ``curl`` as
        :meth:`curl_update`."""
        for comp, box in boxes.items():
            if _empty(box):
                continue
            sl = box_slices(box)
            c = self.curl("E", comp, sl, src)
            if c is None:
                continue
            cs = coefs.slices(box)
            dst[comp][sl] = coefs.ca[comp][cs] * dst[comp][sl] + coefs.cb[comp][cs] * c

    def fused_step(self, fin: Dict[str, torch.Tensor], fout: Dict[str, torch.Tensor], boxes: Dict[str, Box],
                   cb: Dict[str, Coef], source=None) -> None:
        """Reference semantics of the fused E+H kernel: E_new from (E_old,
        H_old) on the E boxes, the point source, then H_new from (H_old, E_new)
        on the H boxes, all written to ``fout``."""
        # like the kernel, only cells inside a component's box are written
        tmp = {c: fin[c].clone() for c in fin}
        e = {c: b for c, b in boxes.items() if c[0] == "E"}
        h = {c: b for c, b in boxes.items() if c[0] == "H"}
        self.curl_update("E", e, tmp, fin, cb)
        if source is not None:
            comp, idx, val = source
            tmp[comp][tuple(idx)] = val
        self.curl_update("H", h, tmp, tmp, cb)
        for c, b in boxes.items():
            if not _empty(b):
                sl = box_slices(b)
                fout[c][sl] = tmp[c][sl]

    def resident_1d_max_cells(self) -> int:
        return 1 << 30

    def resident_1d(self, F: Dict[str, torch.Tensor], boxes: Dict[str, Box], cb: Dict[str, Coef], nsteps: int,
                    src_i=None, vals=None) -> None:
        """Reference semantics of the register-resident 1D kernel
        (yee1d_res.hip): ``nsteps`` fused steps in place, hard Ez source
        ``vals[s]`` at cell ``src_i``.  CPU tensors run the native loop of
        the host library (csrc/host_yee1d.cpp); the torch ops below are the
        oracle it is tested against."""
        if self._res1d_native(F, boxes, cb, nsteps, src_i, vals):
            return
        for s in range(nsteps):
            nxt = {c: F[c].clone() for c in F}
            src = None if vals is None else ("Ez", (int(src_i), 0, 0), float(vals[s]))
            self.fused_step(F, nxt, boxes, cb, src)
            if src is not None:
                # a hard source stays in the field wherever it sits (fused_step stores the E box
                # only: on a cell outside it, cell 0, the value would reach Hy and then be lost)
                nxt["Ez"][src[1]] = src[2]
            for c in F:
                F[c].copy_(nxt[c])

    native_1d = True  # CPU 1D runs take the host library's loop (False: the torch oracle)

    def _res1d_native(self, F, boxes, cb, nsteps, src_i, vals) -> bool:
        ez, hy = F["Ez"], F["Hy"]
        if (not self.native_1d or ez.device.type != "cpu" or ez.dtype not in (torch.float32, torch.float64)
                or not ez.is_contiguous() or not hy.is_contiguous() or hy.dtype != ez.dtype):
            return False
        try:
            from ..native import load_host_library
            lib = load_host_library(build_if_missing=False)
            fn = getattr(lib, "fdtd_res1d_cpu_%s" % ("f64" if ez.dtype == torch.float64 else "f32"))
        except (OSError, AttributeError):
            return False
        import ctypes
        n = ez.numel()
        whole = tuple(slice(0, d) for d in ez.shape)

        def cell(c):  # per-cell array of a coefficient with profiles / cells, None for a scalar
            if all(getattr(c, a) is None for a in ("cell", "px", "py", "pz")):
                return None
            v = c.materialize(whole)
            v = torch.as_tensor(v, dtype=ez.dtype).expand(ez.shape)
            return v.contiguous().reshape(-1)
        pe, ph = cell(cb["Ez"]), cell(cb["Hy"])
        lim = lambda b: (b[0][0], b[1][0]) if not _empty(b) else (0, 0)
        (elo, ehi), (hlo, hhi) = lim(boxes["Ez"]), lim(boxes["Hy"])
        v = None
        if vals is not None:
            v = vals.to("cpu", ez.dtype).contiguous()
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        fn.restype = ctypes.c_int
        fn(ptr(ez), ptr(hy), ptr(pe), ptr(ph), ctypes.c_double(cb["Ez"].scalar if pe is None else 1.0),
           ctypes.c_double(cb["Hy"].scalar if ph is None else 1.0), ctypes.c_int(n),
           (ctypes.c_int * 4)(elo, ehi, hlo, hhi), ctypes.c_int(nsteps),
           ctypes.c_int(-1 if src_i is None else int(src_i)), ptr(v))
        return True

    def tb_step(self, fin: Dict[str, torch.Tensor], fout: Dict[str, torch.Tensor], boxes: Dict[str, Box],
                obox: Box, cb: Dict[str, Coef], steps: int, sources=None, tfsf=None) -> None:
        """Reference semantics of the temporally blocked kernel: ``steps``
        fused steps on the update boxes (reads outside the arrays count as
        zero, like the kernel's unloaded rows), then ``obox`` is written to
        ``fout`` for every component (cells outside a component's update box
        with their input value: the kernels store whole output boxes).
        ``tfsf`` = (TfsfSets, g table, first level): each level adds coef * g
        to the set's target cells after the curl update (the kernel adds g to
        the curl)."""
        pad = {c: torch.nn.functional.pad(fin[c], (1, 1, 1, 1, 1, 1)) for c in fin}
        shifted = {c: ((b[0][0] + 1, b[0][1] + 1, b[0][2] + 1), (b[1][0] + 1, b[1][1] + 1, b[1][2] + 1))
                   for c, b in boxes.items()}
        cbp = cb_pad(cb)
        e = {c: b for c, b in shifted.items() if c[0] == "E"}
        h = {c: b for c, b in shifted.items() if c[0] == "H"}
        cur = pad
        for l in range(steps):
            nxt = {c: cur[c].clone() for c in cur}
            self.curl_update("E", e, nxt, cur, cbp)
            if tfsf is not None:
                self._tfsf_level(nxt, tfsf, l, "E", shifted, cbp)
            if sources is not None and sources[l] is not None:
                # after the corrections, as the stepped path (and the kernel) does
                comp, idx, val = sources[l]
                nxt[comp][tuple(i + 1 for i in idx)] = val
            self.curl_update("H", h, nxt, nxt, cbp)
            if tfsf is not None:
                self._tfsf_level(nxt, tfsf, l, "H", shifted, cbp)
            cur = nxt
        # the whole output box of every component, like the kernels: a cell
        # outside its component's update box carries its input value
        if not _empty(obox):
            sl = box_slices(obox)
            sp = tuple(slice(s.start + 1, s.stop + 1) for s in sl)
            for c in boxes:
                fout[c][sl] = cur[c][sp]

    tb_drude_max_steps = 5

    def tb_drude_step(self, fin: Dict[str, torch.Tensor], fout: Dict[str, torch.Tensor], boxes: Dict[str, Box],
                      obox: Box, cb: Dict[str, Coef], steps: int, sources, drude: dict) -> None:
        """Reference semantics of the Drude pass (csrc/tb3d_mr.h DrDev):
        :meth:`tb_step`'s fused steps, with the E components inside
        ``drude["box"]`` taking E' = (b0 cbd) curl - b2 delta + m1 E + m2 Ep
        from the state ``drude["sin"]`` (delta + ids, Ep; float4 per cell),
        whose advanced values go to ``drude["sout"]`` on the cells of
        ``obox`` inside the box."""
        B = drude["box"]
        pad = {c: torch.nn.functional.pad(fin[c], (1, 1, 1, 1, 1, 1)) for c in fin}
        shifted = {c: ((b[0][0] + 1, b[0][1] + 1, b[0][2] + 1), (b[1][0] + 1, b[1][1] + 1, b[1][2] + 1))
                   for c, b in boxes.items()}
        cbp = cb_pad(cb)
        unit = {c: Coef(1.0) for c in cb}
        e = {c: b for c, b in shifted.items() if c[0] == "E"}
        h = {c: b for c, b in shifted.items() if c[0] == "H"}
        E = ("Ex", "Ey", "Ez")
        bsl = tuple(slice(B[0][d] + 1, B[1][d] + 1) for d in range(3))
        s0, s1 = drude["sin"]
        ids = drude["ids"]  # int32 over B (the kernel reads the same bits from s0[..., 3] in fp32)
        lut = drude["lut"]
        k = [lut[q][((ids >> (8 * q)) & 0xff).long()] for q in range(3)]  # (bx, by, bz, 4) per component
        delta = [s0[..., q].clone() for q in range(3)]
        ep = [s1[..., q].clone() for q in range(3)]
        cbd = float(drude["cbd"])
        cur = pad
        for l in range(steps):
            nxt = {c: cur[c].clone() for c in cur}
            self.curl_update("E", e, nxt, cur, cbp)
            curl = {c: torch.zeros_like(cur[c]) for c in E}
            self.curl_update("E", e, curl, cur, unit)
            for q, c in enumerate(E):
                cu, ec = curl[c][bsl], cur[c][bsl]
                nxt[c][bsl] = k[q][..., 0] * cu - k[q][..., 1] * delta[q] + k[q][..., 2] * ec + k[q][..., 3] * ep[q]
                delta[q] = cbd * cu
                ep[q] = ec.clone()
            if sources is not None and sources[l] is not None:
                comp, idx, val = sources[l]
                nxt[comp][tuple(i + 1 for i in idx)] = val
            self.curl_update("H", h, nxt, nxt, cbp)
            cur = nxt
        # the whole output box of every component, like the kernels: a cell
        # outside its component's update box carries its input value
        if not _empty(obox):
            sl = box_slices(obox)
            sp = tuple(slice(s.start + 1, s.stop + 1) for s in sl)
            for c in boxes:
                fout[c][sl] = cur[c][sp]
        ob = box_intersect_(B, obox)
        if not _empty(ob):
            o0, o1 = drude["sout"]
            sl = tuple(slice(ob[0][d] - B[0][d], ob[1][d] - B[0][d]) for d in range(3))
            for q in range(3):
                o0[sl + (q,)] = delta[q][sl]
                o1[sl + (q,)] = ep[q][sl]
            o0[sl + (3,)] = s0[sl + (3,)]
            o1[sl + (3,)] = 0.0

    tb_amp_max_steps = 3

    def tb_amp_step(self, fin: Dict[str, torch.Tensor], fout: Dict[str, torch.Tensor], boxes: Dict[str, Box],
                    obox: Box, cb: Dict[str, Coef], steps: int, line, vals, amps, aboxes, accuracy: float,
                    counts: torch.Tensor) -> None:
        """Reference semantics of the amplitude pass (csrc/tb3d_mr.h AmpDev):
        the fused steps of :meth:`tb_step` with, after each, the amplitude
        update (:meth:`amplitude_update`) of the cells of ``obox`` inside
        ``aboxes`` -- ``counts[l]`` += the changed cells of step l -- and the
        hard source on the z line ``line`` = (E component, i, j, k0, k1)."""
        pad = {c: torch.nn.functional.pad(fin[c], (1, 1, 1, 1, 1, 1)) for c in fin}
        shifted = {c: ((b[0][0] + 1, b[0][1] + 1, b[0][2] + 1), (b[1][0] + 1, b[1][1] + 1, b[1][2] + 1))
                   for c, b in boxes.items()}
        cbp = cb_pad(cb)
        e = {c: b for c, b in shifted.items() if c[0] == "E"}
        h = {c: b for c, b in shifted.items() if c[0] == "H"}
        comps = ("Ex", "Ey", "Ez", "Hx", "Hy", "Hz")
        cur = pad
        for l in range(steps):
            nxt = {c: cur[c].clone() for c in cur}
            self.curl_update("E", e, nxt, cur, cbp)
            if line is not None:
                comp, i, j, k0, k1 = line
                nxt[comp][i + 1, j + 1, k0 + 1:k1 + 1] = float(vals[l])
            self.curl_update("H", h, nxt, nxt, cbp)
            cur = nxt
            for c, a, ab in zip(comps, amps, aboxes):
                b = box_intersect_(ab, obox)
                if _empty(b):
                    continue
                view = {c: cur[c][tuple(slice(b[0][d] + 1, b[1][d] + 1) for d in range(3))]}
                n = self.amplitude_update(view[c], a[box_slices(b)], ((0, 0, 0), tuple(view[c].shape)), accuracy)
                counts[l] += n
        # the whole output box of every component, like the kernel (the line
        # source may sit outside its component's update box)
        sl = box_slices(obox)
        sp = tuple(slice(s_.start + 1, s_.stop + 1) for s_ in sl)
        for c in boxes:
            fout[c][sl] = cur[c][sp]

    def _tfsf_level(self, F, tfsf, l: int, kind: str, boxes, cb) -> None:
        """TF/SF corrections of level ``l`` of a blocked pass on fields padded
        by one cell: the E-form tables of the stepped path (``sets.tables``,
        models/scheme.py ``_init_tfsf``) applied from the incident line as it
        stood at that level (recorded by :meth:`tfsf_pass`), so a blocked
        pass is bit-for-bit the stepped arithmetic."""
        sets, g, level0 = tfsf
        hin, ein = g.lines[level0 + l]
        inc = hin if kind == "E" else ein
        shape = tuple(F["Ex"].shape)
        for c in (("Ex", "Ey", "Ez") if kind == "E" else ("Hx", "Hy", "Hz")):
            for tab in sets.tables.get(c, ()):
                if tab.n == 0:
                    continue
                off = tab.__dict__.setdefault("_pad_off", {}).get(shape)
                if off is None:
                    ijk = tab.ijk.long() + 1
                    off = tab._pad_off[shape] = (ijk[:, 0] * shape[1] + ijk[:, 1]) * shape[2] + ijk[:, 2]
                v = (inc[tab.i0] * tab.w0 + inc[tab.i0 + 1] * tab.w1) * tab.coef
                F[c].view(-1).index_add_(0, off, v.to(F[c].dtype))

    tfsf_sets_ok = True  # tb_step applies TfsfSets corrections (the blocked kernel's form)

    def tfsf_pass(self, einc: torch.Tensor, hinc: torch.Tensor, ce: float, ch: float, src_vals, reach: int,
                  sets, slot: int = 0, dry: bool = False) -> torch.Tensor:
        """Reference semantics of k_tfsf_pass (yee3d_tb.hip): the incident
        line advanced ``len(src_vals)`` steps, the per-level g table of the
        pass returned (levels x sets.ld).  ``dry``: the line is left as it was
        (the g table of a hybrid pass, whose shell steps the line itself)."""
        if dry:
            einc, hinc = einc.clone(), hinc.clone()
        T = len(src_vals)
        n = einc.numel()
        m = min(n, reach)
        ld = sets.ld
        g = torch.zeros(max(8, T) * max(1, ld), dtype=einc.dtype, device=einc.device)
        i0 = sets.i0.long()
        w0, w1, cc = sets.w0.to(einc.dtype), sets.w1.to(einc.dtype), sets.c.to(einc.dtype)
        ne = sets.n_e
        g.lines = []  # (H line before, E line after) each level's E half step: _tfsf_level
        for l in range(T):
            hin = hinc.clone()
            if ne:
                g[l * ld:l * ld + ne] = cc[:ne] * (w0[:ne] * hinc[i0[:ne]] + w1[:ne] * hinc[i0[:ne] + 1])
            if m > 0:
                new = einc[:m].clone()
                if m > 1:
                    new[1:m] = einc[1:m] + ce * (hinc[0:m - 1] - hinc[1:m])
                new[0] = src_vals[l]
                einc[:m] = new
            g.lines.append((hin, einc.clone()))
            if ld > ne:
                g[l * ld + ne:(l + 1) * ld] = cc[ne:] * (w0[ne:] * einc[i0[ne:]] + w1[ne:] * einc[i0[ne:] + 1])
            mh = min(m, n - 1)
            if mh > 0:
                hinc[:mh] += ch * (einc[:mh] - einc[1:mh + 1])
        return g

    def chain_update(self, kind: str, boxes: Dict[str, Box], F: Dict[str, torch.Tensor], upml: Dict[str, dict],
                     p: int, drude: bool, plain_form: bool = False, plain: Optional[Dict[str, Box]] = None,
                     cb: Optional[Dict[str, Coef]] = None, rows=None) -> None:
        """Reference semantics of the fused UPML/Drude chain kernel
        (chain_kernels.hip): D -> [D1] -> E per cell of each box, plus the
        plain Yee update on the folded ``plain`` boxes.  ``rows`` (dispersive
        launches): ``(table, lo0, lo1)``, per local row (x, y) the z range of
        the cells that run the chain; the other cells of the boxes take the
        plain update ``F += cb curl`` (their D / D1 levels are left alone)."""
        if plain:
            pb = {c: plain.get(c, ((0, 0, 0), (0, 0, 0))) for c in boxes}
            self.curl_update(kind, pb, F, F, cb)
        new = []
        for c, box in boxes.items():
            if _empty(box):
                continue
            st = upml[c]
            sl = box_slices(box)
            curl = self.curl(kind, c, sl, F)
            mask = None if rows is None else self._row_mask(rows, box)

            def lv(t, box=box, sl=sl):
                # full-grid level or region-local one (models/regions.py)
                return t.view(box) if isinstance(t, RegionLevel) else t[sl]
            D = st["D"][p]
            Dn = st["caD"].materialize(sl) * lv(D[0]) + st["cbD"].materialize(sl) * curl
            nw, old = Dn, lv(D[0])
            upd = [(lv(D[-1]), Dn)]
            if drude:
                D1 = st["D1"][p]
                D1n = (st["b0"].materialize(sl) * Dn + st["b1"].materialize(sl) * lv(D[0])
                       + st["b2"].materialize(sl) * lv(D[1]) + st["ma1"].materialize(sl) * lv(D1[0])
                       + st["ma2"].materialize(sl) * lv(D1[1]))
                upd.append((lv(D1[2]), D1n))
                nw, old = D1n, lv(D1[0])
            cbE, ccE = (st["plain"]["cbE"], st["plain"]["ccE"]) if plain_form else (st["cbE"], st["ccE"])
            En = st["caE"].materialize(sl) * F[c][sl] + cbE.materialize(sl) * nw + ccE.materialize(sl) * old
            if mask is not None:
                En = torch.where(mask, En, F[c][sl] + cb[c].materialize(sl) * curl)
                upd = [(t, torch.where(mask, v, t)) for t, v in upd]
            new.append((c, sl, En, upd))
        # every component reads the other kind only: the stores can follow in any order
        for c, sl, En, upd in new:
            for t, v in upd:
                t.copy_(v)
            F[c][sl] = En

    @staticmethod
    def _row_mask(rows, box: Box) -> torch.Tensor:
        """Boolean mask over ``box``: z inside the row's dispersive range."""
        tab, lo0, lo1 = rows
        nx, ny = tab.shape[0], tab.shape[1]
        X = torch.arange(box[0][0], box[1][0], device=tab.device) - lo0
        Y = torch.arange(box[0][1], box[1][1], device=tab.device) - lo1
        okx = (X >= 0) & (X < nx)
        oky = (Y >= 0) & (Y < ny)
        r = tab[X.clamp(0, nx - 1)][:, Y.clamp(0, ny - 1)]  # (bx, by, 2)
        ok = (okx[:, None] & oky[None, :])[..., None]
        Z = torch.arange(box[0][2], box[1][2], device=tab.device)[None, None, :]
        return ok & (Z >= r[..., 0:1]) & (Z < r[..., 1:2])

    def curl_general(self, kind: str, comp: str, box: Box, out: torch.Tensor, inp: torch.Tensor,
                     src: Dict[str, torch.Tensor], ca: Coef, cb: Coef) -> None:
        if _empty(box):
            return
        sl = box_slices(box)
        c = self.curl(kind, comp, sl, src)
        v = ca.materialize(sl) * inp[sl]
        if c is not None:
            v = v + cb.materialize(sl) * c
        out[sl] = v

    def lincomb(self, out: torch.Tensor, box: Box, terms: Sequence[Tuple[Coef, torch.Tensor]]) -> None:
        if _empty(box):
            return
        sl = box_slices(box)
        v = None
        for coef, x in terms:
            t = coef.materialize(sl) * x[sl]
            v = t if v is None else v + t
        out[sl] = v

    def cpml_apply(self, kind: str, target: torch.Tensor, src: torch.Tensor, axis: int, sign: int,
                   psi: torch.Tensor, psi_box: Box, box: Box, b: torch.Tensor, c: torch.Tensor,
                   kinv_m1: torch.Tensor, cb: Coef) -> None:
        """CPML slab correction (models/cpml.py)."""
        if _empty(box):
            return
        sl = box_slices(box)
        if kind == "E":
            diff = src[sl] - src[_shift(sl, axis, -1)]
        else:
            diff = src[_shift(sl, axis, +1)] - src[sl]
        psl = tuple(slice(box[0][d] - psi_box[0][d], box[1][d] - psi_box[0][d]) for d in range(3))
        view = [1, 1, 1]
        view[axis] = -1
        bb = b[sl[axis]].view(view)
        cc = c[sl[axis]].view(view)
        kk = kinv_m1[sl[axis]].view(view)
        psi[psl] = bb * psi[psl] + cc * diff
        corr = kk * diff + psi[psl]
        if sign < 0:
            corr = -corr
        target[sl] += cb.materialize(sl) * corr

    # --------------------------------------------------------------- sources
    def set_value(self, t: torch.Tensor, idx: Sequence[int], value: float) -> None:
        t[tuple(idx)] = value

    def set_values(self, t: torch.Tensor, flat_idx: torch.Tensor, value: float) -> None:
        t.view(-1)[flat_idx] = value

    # ------------------------------------------------------------------ halo
    def pack(self, tensors: Sequence[torch.Tensor], box: Box, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        sl = box_slices(box)
        parts = [t[sl].reshape(-1) for t in tensors]
        buf = torch.cat(parts)
        if out is not None:
            out.copy_(buf)
            return out
        return buf

    def unpack(self, tensors: Sequence[torch.Tensor], box: Box, buf: torch.Tensor) -> None:
        sl = box_slices(box)
        n = 1
        for d in range(3):
            n *= box[1][d] - box[0][d]
        for c, t in enumerate(tensors):
            t[sl] = buf[c * n:(c + 1) * n].view(t[sl].shape)

    def copy_box(self, src: Sequence[torch.Tensor], dst: Sequence[torch.Tensor], box: Box) -> None:
        """dst[c][box] = src[c][box] for every component pair."""
        sl = box_slices(box)
        for a, b in zip(src, dst):
            b[sl] = a[sl]

    # ------------------------------------------------------------ reductions
    def maxabs(self, t: torch.Tensor, box: Box) -> float:
        if _empty(box):
            return 0.0
        v = t[box_slices(box)].abs()
        if torch.isnan(v).any():
            return float("inf")
        return float(v.max())

    def amplitude_update_many(self, fields, amps, boxes, accuracy: float, counter: torch.Tensor) -> None:
        """Several components' amplitude updates; the changed count is added
        to ``counter`` (semantics of the HIP kernel)."""
        for f, a, b in zip(fields, amps, boxes):
            counter += self.amplitude_update(f, a, b, accuracy)

    def amplitude_update(self, f: torch.Tensor, amp: torch.Tensor, box: Box, accuracy: float) -> int:
        """Running max-|f| with the reference's convergence test
        (``Scheme3D::updateAmplitude``, Scheme3D.cpp:3294-3333): the stored
        amplitude is raised only when it grows by more than ``accuracy``
        (relative); returns the number of such cells."""
        if _empty(box):
            return 0
        sl = box_slices(box)
        v = f[sl].abs()
        a = amp[sl]
        ge = v >= a
        diff = v - a
        denom = torch.where(a != 0, a, torch.where(v != 0, v, torch.ones_like(v)))
        acc = diff / denom
        upd = ge & (acc > accuracy)
        amp[sl] = torch.where(upd, v, a)
        return int(upd.sum())

    # ----------------------------------------------------------------- TF/SF
    def inc_step_e(self, einc: torch.Tensor, hinc: torch.Tensor, coef: float, source: float) -> None:
        """1D incident line, E half step (Scheme3D.cpp:25-59)."""
        einc[1:] = einc[1:] + coef * (hinc[:-1] - hinc[1:])
        einc[0] = source

    def inc_step_h(self, einc: torch.Tensor, hinc: torch.Tensor, coef: float) -> None:
        """1D incident line, H half step (Scheme3D.cpp:62-82)."""
        hinc[:-1] = hinc[:-1] + coef * (einc[:-1] - einc[1:])

    def tfsf_apply(self, target: torch.Tensor, table: "TfsfTable", inc: torch.Tensor, box: Box) -> None:
        """``target[cell] += coef * (w0 inc[i0] + w1 inc[i0+1])`` for the
        table's cells inside ``box`` (local)."""
        if table.n == 0 or _empty(box):
            return
        ijk = table.ijk
        m = torch.ones(table.n, dtype=torch.bool, device=ijk.device)
        for d in range(3):
            m &= (ijk[:, d] >= box[0][d]) & (ijk[:, d] < box[1][d])
        v = (inc[table.i0] * table.w0 + inc[table.i0 + 1] * table.w1) * table.coef
        v = torch.where(m, v, torch.zeros_like(v))
        flat = target.view(-1)
        flat.index_add_(0, table.off, v.to(target.dtype))

    def dft_accumulate(self, entries, twiddles) -> None:
        """One sample of a running-DFT monitor (ops/dft.py ``DftEntries``):
        per entry and frequency k ``re[k] += f cos``, ``im[k] += f sin`` with
        ``twiddles[kind][k] = (cos, sin)`` (fp64 on the host, rounded to the
        accumulators' precision).  The oracle of csrc/dft_kernels.hip."""
        import numpy as np
        tw = np.asarray(twiddles, dtype=np.float64)
        if tw.shape != (2, entries.k, 2):
            raise ValueError("dft_accumulate: twiddles of shape (2, %d, 2), got %s" % (entries.k, tw.shape))
        for e in entries:
            if e.empty:
                continue
            (x0, y0, z0), (x1, y1, z1) = e.box
            if min(x0, y0, z0) < 0 or any(e.box[1][d] > e.field.shape[d] for d in range(3)):
                raise ValueError("dft_accumulate: box %s outside array %s" % (e.box, tuple(e.field.shape)))
            f = e.field[x0:x1, y0:y1, z0:z1]
            acc = e.owned()
            if e.acc.dtype == torch.float32:
                tw_e = tw[e.kind].astype(np.float32)
            else:
                tw_e = tw[e.kind]
            for k in range(entries.k):
                acc[k, 0] += f * float(tw_e[k, 0])
                acc[k, 1] += f * float(tw_e[k, 1])

    def dft_flux(self, terms) -> torch.Tensor:
        """(faces, K) float64: per term ``sign * sum over the face cells of
        (Re e Re h + Im e Im h)`` added to its face's row (ops/dft.py
        ``FluxTerms``).  Each operand is the face-centre average of its 1, 2
        or 4 accumulator samples, taken, multiplied and summed in fp64
        whatever the accumulators' precision.  The oracle of
        csrc/flux_kernels.hip."""
        dev = terms.rows[0].e.acc.device if len(terms) else "cpu"
        out = torch.zeros((terms.faces, terms.k), dtype=torch.float64, device=dev)

        for t in terms:
            for op in (t.e, t.h):
                why = None if t.empty else op.reach_error(t.extent, terms.k)
                if why:
                    raise ValueError("dft_flux: " + why)
            if t.empty:
                continue
            e, h = t.e.centre(t.extent), t.h.centre(t.extent)
            out[t.face] += t.sign * (e[:, 0] * h[:, 0] + e[:, 1] * h[:, 1]).sum(dim=(1, 2, 3))
        return out

    def dft_farfield(self, terms, dirs, wavenumbers) -> torch.Tensor:
        """(K, A, 6, 2) float64 (re, im): per term ``sign * sum over the face
        cells c of avg(acc[k, 0] + i acc[k, 1])(c) exp(-i kappa_k rhat_a .
        r'(c))`` added to its slot, ``r'(c) = pos0 + dx * (cell index)``
        (ops/dft.py ``FarTerms``); ``dirs`` (A, 3) fp64 unit vectors,
        ``wavenumbers`` (K,) fp64.  The face-centre average of the 1, 2 or 4
        samples is taken in fp64 whatever the accumulators' precision, and
        every (cell, direction) gets its own ``exp``: the definition, not a
        factorisation.  The oracle of csrc/farfield_kernels.hip."""
        dirs = torch.as_tensor(dirs)
        wn = torch.as_tensor(wavenumbers)
        if dirs.dim() != 2 or dirs.shape[1] != 3 or dirs.dtype != torch.float64:
            raise ValueError("dft_farfield: dirs of shape (A, 3) in float64, got %s %s" % (tuple(dirs.shape), dirs.dtype))
        if wn.dim() != 1 or wn.shape[0] != terms.k or wn.dtype != torch.float64:
            raise ValueError("dft_farfield: %d wavenumbers in float64, got %s %s" % (terms.k, tuple(wn.shape), wn.dtype))
        dev = terms.rows[0].operand.acc.device if len(terms) else dirs.device
        dirs, wn = dirs.to(dev), wn.to(dev)
        out = torch.zeros((terms.k, dirs.shape[0], 6), dtype=torch.complex128, device=dev)
        for t in terms:
            if t.empty:
                continue
            why = t.operand.reach_error(t.extent, terms.k)
            if why:
                raise ValueError("dft_farfield: " + why)
            acc = t.operand.centre(t.extent)
            val = torch.complex(acc[:, 0], acc[:, 1]).reshape(terms.k, -1)          # (K, C)
            pos = torch.stack(torch.meshgrid(*[t.pos0[a] + terms.dx * torch.arange(t.extent[a], dtype=torch.float64,
                                                                                   device=dev) for a in range(3)],
                                             indexing="ij"), dim=-1).reshape(-1, 3)  # (C, 3)
            proj = pos @ dirs.transpose(0, 1)                                        # (C, A)
            for k in range(terms.k):
                ph = torch.exp(torch.complex(torch.zeros_like(proj), -wn[k] * proj))
                out[k, :, t.slot] += t.sign * (val[k].unsqueeze(1) * ph).sum(dim=0)
        return torch.view_as_real(out).contiguous()

    def field_sumsq(self, entries) -> torch.Tensor:
        """(R,) float64: per entry the sum over its box of the squares of the
        field, converted to fp64 first, added to the entry's row (ops/energy.py
        ``EnergyEntries``).  The oracle of csrc/energy_kernels.hip."""
        dev = entries.rows[0].field.device if len(entries) else "cpu"
        out = torch.zeros((entries.R,), dtype=torch.float64, device=dev)
        for e in entries:
            if e.empty:
                continue
            (x0, y0, z0), (x1, y1, z1) = e.box
            if e.field.dim() != 3 or min(x0, y0, z0) < 0 or any(e.box[1][d] > e.field.shape[d] for d in range(3)):
                raise ValueError("field_sumsq: box %s outside array %s" % (e.box, tuple(e.field.shape)))
            out[e.row] += e.field[x0:x1, y0:y1, z0:z1].double().square().sum()
        return out

    def probe_sample(self, entries, row: int) -> None:
        """One sample of a probe monitor (ops/probe.py ``ProbeEntries``): row
        ``row`` of ``entries.series`` = every slot's element, widened to
        fp64; the other rows stay as they are.  The oracle of csrc/
        probe_kernels.hip."""
        if not 0 <= int(row) < entries.capacity:
            raise ValueError("probe_sample: row %d of %d" % (row, entries.capacity))
        why = entries.offset_error()
        if why:
            raise ValueError("probe_sample: " + why)
        series = entries.series
        if tuple(series.shape) != (entries.capacity, len(entries)) or series.dtype != torch.float64:
            raise ValueError("probe_sample: series of shape %s %s" % (tuple(series.shape), series.dtype))
        plan = entries.tables.get("torch")  # per array: its slots' columns and offsets (``add`` drops it)
        if plan is None:
            plan = []
            for fi in range(len(entries.fields)):
                cols = [s for s, (i, _) in enumerate(entries.rows) if i == fi]
                if cols:
                    plan.append((fi, torch.tensor(cols, dtype=torch.int64, device=series.device),
                                 torch.tensor([entries.rows[s][1] for s in cols], dtype=torch.int64,
                                              device=series.device)))
            entries.tables["torch"] = plan
        for fi, cols, offs in plan:
            f = entries.fields[fi]
            if not f.is_contiguous():
                raise ValueError("probe_sample: contiguous field arrays")
            series[int(row), cols] = f.reshape(-1)[offs].double()

    def source_inject(self, entries, kind: str, values) -> None:
        """One half step of a source list (ops/source.py ``SourceEntries``):
        every distinct cell of the entries of ``kind`` becomes its value
        widened to fp64 (0 when the cell's first entry is hard) plus
        ``amplitude * values[signal]`` for each of its entries in table order
        -- product and sum rounded separately --, rounded once to the field
        type.  The oracle of csrc/source_kernels.hip, bit for bit."""
        values = [float(v) for v in values]
        key = ("torch",) + entries.key(kind)
        cached = entries.tables.get(key)  # offsets and signal indices are checked once per plan
        if cached is None:
            why = entries.table_error(kind)
            if why:
                raise ValueError("source_inject: " + why)
        why = entries.values_error(len(values), entries.signals_needed(kind) if cached is None else cached[1])
        if why:
            raise ValueError("source_inject: " + why)
        rows = entries.rows[kind]
        if not rows:
            return
        plan = None if cached is None else cached[0]  # per array: its cells and, per round, the k-th entries
        if plan is None:
            plan = []
            for fi in sorted({r[0] for r in rows}):
                dev = entries.fields[fi].device
                offs, hard, rounds = [], [], []
                for (i, off, amp, sig, hd) in rows:
                    if i != fi:
                        continue
                    if not offs or offs[-1] != off:
                        offs.append(off)
                        hard.append(hd)
                        k = 0
                    else:
                        k += 1
                    while len(rounds) <= k:
                        rounds.append(([], [], []))
                    rounds[k][0].append(len(offs) - 1)
                    rounds[k][1].append(amp)
                    rounds[k][2].append(sig)
                plan.append((fi, torch.tensor(offs, dtype=torch.int64, device=dev),
                             torch.tensor(hard, dtype=torch.bool, device=dev),
                             [(torch.tensor(c, dtype=torch.int64, device=dev),
                               torch.tensor(a, dtype=torch.float64, device=dev),
                               torch.tensor(s, dtype=torch.int64, device=dev)) for c, a, s in rounds]))
            if len(entries.tables) >= 8:
                entries.tables.clear()
            entries.tables[key] = (plan, entries.signals_needed(kind))
        for fi, offs, hard, rounds in plan:
            f = entries.fields[fi]
            if not f.is_contiguous():
                raise ValueError("source_inject: contiguous field arrays")
            flat = f.reshape(-1)
            vals = torch.tensor(values, dtype=torch.float64, device=f.device)
            acc = torch.where(hard, torch.zeros((), dtype=torch.float64, device=f.device), flat[offs].double())
            for cells, amp, sig in rounds:
                term = amp * vals[sig]
                acc[cells] = acc[cells] + term
            flat[offs] = acc.to(f.dtype)

    def scene_sample(self, table, quantity: str, points, origin, shape, stride, mod, out=None) -> torch.Tensor:
        """A file scene (layout/scene_file.py ``SceneTable``) evaluated and
        averaged onto one component: fp64 tensor of ``shape``.  Cell ``i`` takes
        the points at eps-grid index ``stride * (origin + i) + offset`` (centre
        ``+ 0.5``) for every offset of ``points``; at each the objects are
        painted first to last over vacuum, then the points reduce as
        ``approximate_material`` (eps) or ``approximate_drude`` do: a plasma
        frequency (omega, omega_m) as sqrt(sum(w * w) / n), a collision
        frequency (gamma, gamma_m) as sum(g) / count over the points whose
        plasma frequency of the same kind is not zero, 0 where there is none.
        The conductivity (cond, ``table.cond``) is painted and reduced exactly
        as eps is, over 0 instead of 1.
        Every operation is rounded on its own, in the order the kernel of
        csrc/scene_kernels.hip keeps, the square roots correctly (``_sqrt_rn``):
        this is its oracle."""
        from ..layout.approximation import approximate_material
        from ..layout.scene_file import (FLAG_IGNORE_SHIFT, FLAG_SHARP, KIND_BOX, KIND_MESH, KIND_SPHERE,
                                         SceneTable, sample_args)
        if not isinstance(table, SceneTable):
            raise ValueError("scene_sample: a SceneTable, got %r" % type(table).__name__)
        if table.has_meshes() and table.range_error():
            raise ValueError("scene_sample: " + table.range_error())
        q, pts, origin, shape, stride, mod = sample_args(quantity, points, origin, shape, stride, mod)
        dev = self.device if out is None else out.device
        if out is not None and (out.dtype != torch.float64 or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError("scene_sample: out must be contiguous float64 of shape %s" % (shape,))
        vals, damps = [], []
        for off in pts:
            ax = [(torch.arange(shape[d], dtype=torch.int64, device=dev) * stride[d]
                   + (stride[d] * origin[d] + off[d])).to(torch.float64) + 0.5 for d in range(3)]
            P = torch.meshgrid(ax[0], ax[1], ax[2], indexing="ij")
            val = torch.full(shape, 1.0 if q == 0 else 0.0, dtype=torch.float64, device=dev)
            damp = torch.zeros_like(val) if q >= 3 else None
            for n, e in enumerate(table.ents):
                # what the object paints: its pole (or eps) and, for a gamma quantity, the pole's damping
                g_e, w_m, g_m = (float(v) for v in table.drude[n])
                obj = (float(e["eps"]), float(e["omega"]), w_m, float(e["omega"]), w_m, float(table.cond[n]))[q]
                obj_damp = g_e if q == 3 else g_m
                flags = int(e["flags"])
                skip = [bool((flags >> (FLAG_IGNORE_SHIFT + a)) & 1) for a in range(3)]
                a0 = [float(v) * mod for v in e["p"]]
                b0 = [float(v) * mod for v in e["q"]]
                if e["kind"] == KIND_BOX:
                    d = None
                    for a in range(3):
                        if skip[a]:
                            continue
                        t = torch.maximum(a0[a] - P[a], P[a] - b0[a])
                        d = t if d is None else torch.maximum(d, t)
                elif e["kind"] == KIND_MESH:
                    t0, tn = (int(v) for v in table.ranges[n])
                    d = _mesh_distance(table.tris[t0:t0 + tn] * mod, ax, shape,
                                       q in (0, 5) and not flags & FLAG_SHARP)
                elif e["kind"] == KIND_SPHERE:
                    sq = [torch.zeros_like(P[a]) if skip[a] else (P[a] - a0[a]) * (P[a] - a0[a]) for a in range(3)]
                    d = _sqrt_rn((sq[0] + sq[1]) + sq[2]) - b0[0]
                else:
                    ax_c = flags & 3
                    b_, c_ = [a for a in range(3) if a != ax_c]
                    db, dc = P[b_] - a0[b_], P[c_] - a0[c_]
                    d = _sqrt_rn(db * db + dc * dc) - b0[0]
                    if not skip[ax_c]:
                        d = torch.maximum(d, torch.maximum(a0[ax_c] - P[ax_c], P[ax_c] - b0[1]))
                if 1 <= q <= 4:
                    val = torch.where(d < 0, torch.full_like(val, obj), val)
                    if q >= 3:
                        damp = torch.where(d < 0, torch.full_like(damp, obj_damp), damp)
                elif flags & FLAG_SHARP:
                    val = torch.where(d < 0, torch.full_like(val, obj), val)
                else:
                    eps_in = obj
                    prop = 0.5 - d
                    mid = prop * eps_in + (1 - prop) * val
                    o = torch.where(d < -0.5, torch.full_like(val, eps_in), mid)
                    val = torch.where(d > 0.5, val, o)
            vals.append(val)
            damps.append(damp)
        if q in (0, 5):
            res = approximate_material(vals)
        elif q <= 2:
            res = _sqrt_rn(sum(w * w for w in vals) / float(len(vals)))
        else:
            count = sum((w != 0).to(torch.float64) for w in vals)
            gsum = sum(damps)
            res = torch.where(count > 0, gsum / torch.clamp(count, min=1.0), torch.zeros_like(gsum))
        if out is None:
            return res.contiguous()
        out.copy_(res)
        return out


def _mesh_distance(tris, ax, shape, magnitude: bool) -> torch.Tensor:
    """The signed distance of a closed triangle mesh at the points ``ax[0] x
    ax[1] x ax[2]``: ``tris`` = (n, 3, 3) fp64 numpy, already scaled, every
    triangle's vertices v0 <= v1 <= v2 in (x, y, z) order (layout/scene_file.py
    ``Mesh``).  The oracle of scene_kernels.hip ``mesh_parity`` and
    ``mesh_dist2``, the same expressions in the same order.

    Sign: a point is inside when a ray along +z crosses an odd number of
    triangles.  A triangle is crossed when the point lies in its bounding box
    in x and y and not above it, on the inner side of its three projected
    edges -- edge functions ``e = (v.x - u.x) * (p.y - u.y) - (v.y - u.y) *
    (p.x - u.x)`` from the lower vertex u to the higher one v, so the two
    triangles of an edge see one value, and ``e >= 0`` counts as left of it
    in both: the ray displaced by (-e^2, +e) -- and below its plane.
    Triangles with zero projected area never count.

    Magnitude (``magnitude``; +-1 otherwise): the distance to the closest
    point of the closest triangle, by the regions of that point (vertex,
    edge, face).  Triangles that cannot come within half a cell of any point
    are left out, so beyond 0.5 the value is only a lower bound."""
    import numpy as np
    dev = ax[0].device
    par = torch.zeros(shape, dtype=torch.bool, device=dev)
    dmin = torch.full(shape, float("inf"), dtype=torch.float64, device=dev)
    if 0 in shape or len(tris) == 0:
        return dmin if magnitude else torch.ones_like(dmin)
    X, Y, Z = ax[0].reshape(1, -1, 1, 1), ax[1].reshape(1, 1, -1, 1), ax[2].reshape(1, 1, 1, -1)
    rlo, rhi = [float(a[0]) for a in ax], [float(a[-1]) for a in ax]
    lo, hi = tris.min(axis=1), tris.max(axis=1)
    hit = ((hi[:, 0] >= rlo[0]) & (lo[:, 0] <= rhi[0]) & (hi[:, 1] >= rlo[1]) & (lo[:, 1] <= rhi[1])
           & (hi[:, 2] >= rlo[2]))
    near = np.ones(len(tris), dtype=bool)
    for c in range(3):
        near &= ~((lo[:, c] - rhi[c] > 1.0) | (rlo[c] - hi[:, c] > 1.0))
    chunk = max(1, (1 << 18) // (shape[0] * shape[1] * shape[2]))

    def columns(t):
        """v[i][c], bounding box lo / hi: (chunk, 1, 1, 1) tensors"""
        def col(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev).reshape(-1, 1, 1, 1)
        return ([[col(t[:, i, c]) for c in range(3)] for i in range(3)],
                [col(t[:, :, c].min(axis=1)) for c in range(3)], [col(t[:, :, c].max(axis=1)) for c in range(3)])

    def dot(u, w):
        return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]

    def normal(ab, ac):
        return [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]

    T = tris[hit]
    for s in range(0, len(T), chunk):
        (v0, v1, v2), blo, bhi = columns(T[s:s + chunk])
        ab, ac, bc = ([b - a for a, b in zip(u, w)] for u, w in ((v0, v1), (v0, v2), (v1, v2)))
        n = normal(ab, ac)
        ap = [X - v0[0], Y - v0[1], Z - v0[2]]
        bp = [X - v1[0], Y - v1[1]]
        l01 = ab[0] * ap[1] - ab[1] * ap[0] >= 0
        l02 = ac[0] * ap[1] - ac[1] * ap[0] >= 0
        l12 = bc[0] * bp[1] - bc[1] * bp[0] >= 0
        up, down = n[2] > 0, n[2] < 0
        inside = (up & l01 & l12 & ~l02) | (down & ~l01 & ~l12 & l02)
        box = (X >= blo[0]) & (X <= bhi[0]) & (Y >= blo[1]) & (Y <= bhi[1]) & (Z <= bhi[2])
        tt = dot(n, ap)
        crossed = inside & box & ((up & (tt < 0)) | (down & (tt > 0)))
        par ^= (crossed.sum(dim=0) % 2).bool()
    if not magnitude:
        return torch.where(par, -torch.ones_like(dmin), torch.ones_like(dmin))

    T = tris[near]
    for s in range(0, len(T), chunk):
        (v0, v1, v2), _, _ = columns(T[s:s + chunk])
        ab, ac, bc = ([b - a for a, b in zip(u, w)] for u, w in ((v0, v1), (v0, v2), (v1, v2)))
        n = normal(ab, ac)
        nn = dot(n, n)
        full = (len(v0[0]),) + tuple(shape)
        ap, bp, cp = ([(X - v[0]).expand(full), (Y - v[1]).expand(full), (Z - v[2]).expand(full)]
                      for v in (v0, v1, v2))
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        d43, d56 = d4 - d3, d5 - d6
        tt = dot(n, ap)
        zero, one = torch.zeros_like(d1), torch.ones_like(d1)
        # the regions of the closest point, the last one that holds winning: face, then the edges
        # v1v2, v0v2, the vertex v2, the edge v0v1, the vertices v1, v0
        num, den, face = tt * tt, nn.expand(full), torch.ones_like(d1, dtype=torch.bool)
        r, e = ap, ab
        for cond, num_c, den_c, r_c, e_c in (
                ((va <= 0) & (d43 >= 0) & (d56 >= 0), d43, d43 + d56, bp, bc),
                ((vb <= 0) & (d2 >= 0) & (d6 <= 0), d2, d2 - d6, ap, ac),
                ((d6 >= 0) & (d5 <= d6), zero, one, cp, ac),
                ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, d1 - d3, ap, ab),
                ((d3 >= 0) & (d4 <= d3), zero, one, bp, ab),
                ((d1 <= 0) & (d2 <= 0), zero, one, ap, ab)):
            num, den, face = torch.where(cond, num_c, num), torch.where(cond, den_c, den), face & ~cond
            r = [torch.where(cond, a, b) for a, b in zip(r_c, r)]
            e = [torch.where(cond, a.expand(full), b.expand(full)) for a, b in zip(e_c, e)]
        x = num / den
        qv = [a - x * b for a, b in zip(r, e)]
        ds = torch.where(face, x, dot(qv, qv))
        ds = torch.where(ds == ds, ds, torch.full_like(ds, float("inf")))   # (a NaN never lowers the minimum)
        dmin = torch.minimum(dmin, ds.amin(dim=0))
    dist = _sqrt_rn(dmin)
    return torch.where(par, -dist, dist)


def _sqrt_rn(t: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp64 square root.  ``torch.sqrt`` on the CPU is
    not: about 0.7% of arguments come out one ulp off (for instance
    sqrt(19.637599999999992)); numpy's is the hardware instruction.  On a
    device ``torch.sqrt`` is the device library's correctly rounded one."""
    if t.device.type != "cpu":
        return torch.sqrt(t)
    import numpy as np
    return torch.from_numpy(np.sqrt(t.contiguous().numpy()))


class TfsfTable:
    """Per-component TF/SF correction list: ``target[off] += coef *
    (w0*inc[i0] + w1*inc[i0+1])`` (built by :mod:`fdtd3d_amd.models.tfsf`).
    Target cells within one table are unique."""

    def __init__(self, off, i0, w0, w1, coef, ijk):
        self.off = off
        self.i0 = i0
        self.w0 = w0
        self.w1 = w1
        self.coef = coef
        self.ijk = ijk
        # host-side bounds, so the HIP op validates without a device sync
        # (required inside HIP graph capture)
        self.max_off = int(off.max()) if off.numel() else -1
        self.max_inc = int(i0.max()) + 1 if i0.numel() else -1

    @property
    def n(self) -> int:
        return int(self.off.numel())
