"""The two low-dimensional fast paths, one launch at a time on live state,
against the fp64 torch oracle:

* the 2D blocked kernel ``ops.tb_step`` on (nx, ny, 1) arrays
  (csrc/yee2d_tb.hip k_tb2d: TMz / TEz, T <= 8 steps per pass, fp32 / fp64);
  the oracle is ``TorchOps.tb_step`` on CPU fp64 tensors;
* the register-resident 1D kernel ``ops.resident_1d`` (csrc/yee1d_res.hip
  k_res1d: a run in one launch of one workgroup); the oracle is
  ``TorchOps.resident_1d`` with ``native_1d = False`` (the torch loop).

Every test builds a HIP scheme and an fp64 torch / CPU scheme from one
``SchemeConfig``, draws seeded fp64 values once (E on the scale of the wave
impedance ``sqrt(cb_E / db_H)``, so old field and curl term weigh the same),
rounds them to the kernel's type, makes ONE op call per backend and compares
everything the op may touch:

* 2D outputs start as the sentinel pattern of test_tb_variants_gpu.sentinel;
  outside the output box they stay bit-identical to it;
* the 1D arrays are views into one device buffer with sentinel guards of
  ``GUARD`` elements (256 / 512 bytes) before, between and after them; the
  guards stay bit-identical;
* inputs, per-cell coefficient arrays and the 1D source table are bit-unchanged;
* a cell the oracle writes with its input value -- 2D: in the output box but
  outside its component's update box, 1D: outside the E / H box -- is
  bit-identical to it (a hard source's cell: to the source's last value);
* errors are taken per component against the maximum of its kind (E or H)
  over what the oracle wrote, with no ``+ 1``.

Bounds.  fp64 keeps the project's 1e-12.  The fp32 bound of a family is 8 x
the largest error of the float32 torch oracle against the fp64 oracle over
the family's cases, through the same check code (the 8 x is for the kernels'
other operation order and FMA contraction), never more than the project's
2e-5.  Measured by tests/test_lowdim_blocked_cpu.py (which asserts that every
fp32 case stays within 1 / 8 of the bound and prints the maxima):

    family   largest fp32-oracle error   bound
    2D       4.51e-7 (narrow-3x256, TEz; the seam cases at T = 8: 3.2e-7)
             8 x = 3.61e-6 -> BOUND32_2D = 3.7e-6
    1D       9.53e-7 (cells-EH-16; cells-H 9.3e-7, cells-E 9.0e-7)
             8 x = 7.62e-6 -> BOUND32_1D = 7.7e-6

On an MI355X the fp32 kernels reach at most 0.125 (2D) and 0.122 (1D) of
these bounds and the fp64 kernels 0.0012 of theirs: no bound was raised
(``RAISED`` is empty).

2D geometry (yee2d_tb.hip launch2d).  N = 4 (fp32) / 2 (fp64) cells per lane,
``HL = ceil(T / N)`` halo lanes per side, a wave run owns
``OWN = (64 - 2 HL) N`` cells of a row: fp32 248 for T <= 4, else 240; fp64
124 / 120 / 116 / 112 for T in 1-2 / 3-4 / 5-6 / 7-8.  With
``y0 = O.lo.y & ~(N - 1)`` run k owns y in ``[y0 + k OWN, y0 + (k + 1) OWN)``,
four runs make a workgroup, x chunks of ``tb_xchunk`` rows start at ``O.lo.x``:

    runs = ceil((O.hi.y - y0) / OWN)     workgroups = ceil(runs / 4)
    chunks = ceil((O.hi.x - O.lo.x) / xchunk)

``tb_xchunk = 0`` takes pick_xchunk2d (``auto_xchunk`` below, with the
device's CU count); on these grids every choice fits one round, so it is one
row per chunk.  Every case claims (least runs, least workgroups, chunks) per
type and every test asserts the claim with ``launch2d``.

1D instance rule (yee1d_res.hip res1d).  1024 threads hold CPL cells each; the
kernel takes the first CPL in {1, 2, 4, 6, 8, 12, 16} (16: fp32 only) with
``n + off <= 1024 CPL``, ``off = (CPL - src % CPL) % CPL`` (0 without a
source): the map is shifted so that the source is element 0 of its thread.
Every case claims the CPL it reaches and every test asserts it with ``cpl_of``.

Found by these tests: ``TorchOps.resident_1d`` (the oracle) dropped a hard
source on a cell outside the E box (cell 0) from the stored field, against
its own description, the stepped path, the native CPU loop and k_res1d; fixed
in ops/torch_ops.py.
"""
import dataclasses
import functools
import math

import pytest
import torch

from fdtd3d_amd.models.scheme import SchemeConfig
from fdtd3d_amd.ops.coef import Coef
from fdtd3d_amd.ops.torch_ops import box_slices
from test_tb_variants_gpu import cdiv, rand, randn, scheme, sentinel, to_dev

pytestmark = pytest.mark.gpu

CAP32 = 2e-5          # the project's fp32 bound: no family bound is wider
BOUND32_2D = 3.7e-6   # see the module docstring
BOUND32_1D = 7.7e-6
BOUND64 = 1e-12
RAISED = ()           # fp32 bounds raised above 8 x the measured maximum on GPU evidence (none)
DT = {"f32": torch.float32, "f64": torch.float64}
PRECS = ("f32", "f64")


def bound_of(family, prec):
    return BOUND64 if prec == "f64" else {"2d": BOUND32_2D, "1d": BOUND32_1D}[family]


def assert_unchanged(now, before, tag):
    for k in before:
        assert torch.equal(now[k], before[k]), (tag, "input changed", k)


# ======================================================================= 2D
NV = {"f32": 4, "f64": 2}   # cells per lane
WPB = 4                     # wave runs per workgroup
COMPS2 = {"tmz": ("Ez", "Hx", "Hy"), "tez": ("Ex", "Ey", "Hz")}
MODES = ("tmz", "tez")
# per-cell coefficient specs -> slots (component order of the mode)
CELL_SLOTS = {"tmz": {"": (), "E": (0,), "H": (1, 2), "EH": (0, 1, 2), "one": (1,)},
              "tez": {"": (), "E": (0, 1), "H": (2,), "EH": (0, 1, 2), "one": (0,)}}


def own_cells(T, prec):
    n = NV[prec]
    return (64 - 2 * cdiv(T, n)) * n


def auto_xchunk(wgs, nxo, T, cus):
    """pick_xchunk2d of yee2d_tb.hip."""
    slots = 8 * cus
    best, best_cost = nxo, -1
    for k in range(1, 513):
        xc = cdiv(nxo, k)
        rounds = cdiv(wgs * cdiv(nxo, xc), slots)
        cost = rounds * (xc + 2 * T)
        if best_cost < 0 or cost < best_cost:
            best, best_cost = xc, cost
        if xc == 1:
            break
    return best


def launch2d(T, prec, obox, xchunk, cus=256):
    """(runs, workgroups, chunks, rows per chunk, y0, OWN) of a launch: the
    module docstring's formulas."""
    n, own = NV[prec], own_cells(T, prec)
    y0 = obox[0][1] & ~(n - 1)
    runs = cdiv(obox[1][1] - y0, own)
    wgs = cdiv(runs, WPB)
    nxo = obox[1][0] - obox[0][0]
    xc = xchunk if xchunk > 0 else auto_xchunk(wgs, nxo, T, cus)
    return runs, wgs, cdiv(nxo, xc), xc, y0, own


@dataclasses.dataclass(frozen=True)
class Case2:
    name: str
    T: int
    claim: dict             # per type (least runs, least workgroups, chunks): the seams the case is for
    why: str
    size: object = (23, 1000)  # (nx, ny), or one per type
    xchunk: int = 5         # tb_xchunk (0: automatic)
    obox: object = None     # None: the grid; else ((x0, y0), (x1, y1))
    shrink: object = None   # per slot (lo x, lo y, hi x, hi y): update box = local_box shrunk by these
    src: object = None      # (slot, x, y); y: a cell (negative: from ny) or ("run", k, d) = y0 + k OWN + d
    at: tuple = ()          # where the source sits (``src_tags``)
    cells: str = ""         # per-cell coefficients: "", "E", "H", "EH", "one" (CELL_SLOTS)
    same_as: str = ""       # inputs and oracle of that case (only the chunking differs)


SEAM = {"f32": (5, 2, 5), "f64": (8, 2, 5)}     # (23, 1000) whole, 5 rows per chunk
ROWS23 = {"f32": (5, 2, 23), "f64": (8, 2, 23)}
ONE23 = {"f32": (5, 2, 1), "f64": (8, 2, 1)}
CUT = {"f32": (5, 2, 4), "f64": (8, 2, 4)}
CORNER = {"f32": (2, 1, 3), "f64": (3, 1, 3)}
SHRINK = ((2, 3, 2, 3), (3, 2, 3, 2), (2, 2, 3, 3))
CUT_BOX = ((3, 5), (20, 1000))

_SEAMS = [
    # chunks of 5 rows from x = 0: the middle chunk 2 is rows 10 .. 14
    Case2("seam-T1", 1, SEAM, "source on the last owned cell of run 0 (lane element N - 1), first row of chunk 2",
          src=(0, 10, ("run", 1, -1)), at=("lane-last", "chunk-first")),
    Case2("seam-T2", 2, SEAM, "source on the first cell of run 1 (lane element 0), last row of chunk 2",
          src=(1, 14, ("run", 1, 0)), at=("lane-first", "chunk-last")),
    Case2("seam-T3", 3, SEAM, "third component (TMz Hy / TEz Hz) on the first cell of run 4 -- the workgroup seam "
          "-- on grid row 0", src=(2, 0, ("run", 4, 0)), at=("wg-seam", "lane-first", "row0")),
    Case2("seam-T4", 4, SEAM, "third component on y = 0 of the last grid row",
          src=(2, 22, 0), at=("y0", "row-last")),
    Case2("seam-T5", 5, SEAM, "first component on y = ny - 1", src=(0, 12, -1), at=("y-last",)),
    Case2("seam-T6", 6, SEAM, "second component on the workgroup seam", src=(1, 11, ("run", 4, 0)),
          at=("wg-seam", "lane-first")),
    Case2("seam-T7", 7, SEAM, "no source"),
    Case2("seam-T8", 8, SEAM, "third component on the last owned cell of run 0, first row of chunk 2",
          src=(2, 10, ("run", 1, -1)), at=("lane-last", "chunk-first")),
]


def _rechunk(base, tag, xchunk, claim, why):
    return dataclasses.replace(base, name="%s-%s" % (base.name, tag), xchunk=xchunk, claim=claim, why=why,
                               same_as=base.name, at=tuple(t for t in base.at if not t.startswith("chunk")))


_S5, _S8 = _SEAMS[4], _SEAMS[7]
_CHUNKS = [
    _rechunk(_S5, "auto", 0, ROWS23, "automatic chunk: one row per chunk on a grid this small"),
    _rechunk(_S5, "rows", 1, ROWS23, "one row per chunk"),
    _rechunk(_S5, "all", 64, ONE23, "a chunk longer than the grid"),
    _rechunk(_S8, "auto", 0, ROWS23, "automatic chunk at T = 8: 16 lead-in / lead-out rows per stored row"),
    _rechunk(_S8, "rows", 1, ROWS23, "one row per chunk at T = 8"),
    _rechunk(_S8, "all", 23, ONE23, "a chunk of exactly nx rows"),
]

_SMALL = [
    Case2("narrow-3x256", 8, {"f32": (2, 1, 2), "f64": (3, 1, 2)}, "nx = 3 < T: every lead-in row of chunk 0 is "
          "outside the array", size=(3, 256), xchunk=2, src=(1, 1, 100)),
    Case2("tiny-5x8", 8, {"f32": (1, 1, 3), "f64": (1, 1, 3)}, "5 x 8 at T = 8: two (fp32) / four (fp64) live lanes",
          size=(5, 8), xchunk=2, src=(0, 2, 3)),
    Case2("one-lane", 3, {"f32": (1, 1, 2), "f64": (1, 1, 2)}, "ny = N: one lane holds the whole row",
          size={"f32": (6, 4), "f64": (6, 2)}, src=(2, 3, 1)),
]

_INNER = [
    Case2("in-whole-T4", 4, SEAM, "update boxes 2 - 3 cells inside the grid on every side (another amount per "
          "component), the grid stored: coefficients masked to 0 inside the array",
          shrink=SHRINK, src=(0, 9, ("run", 1, 0)), at=("lane-first", "chunk-last")),
    Case2("in-odd-T6", 6, CUT, "the same boxes, the output box from an odd y to 1 short of a multiple of N",
          shrink=SHRINK, obox=((2, 3), (21, 999))),
    Case2("corner-00-T5", 5, CORNER, "output box on the (0, 0) corner; the source outside it, 1 row and 2 cells away",
          shrink=SHRINK, obox=((0, 0), (12, 333)), src=(0, 12, 334), at=("outside",)),
    Case2("corner-01-T2", 2, CORNER, "output box on the (0, ny) corner", shrink=SHRINK, obox=((0, 667), (12, 1000))),
    Case2("corner-10-T3", 3, CORNER, "output box on the (nx, 0) corner, source on its first row",
          shrink=SHRINK, obox=((11, 0), (23, 333)), src=(1, 11, 100)),
    Case2("corner-11-T7", 7, CORNER, "output box on the (nx, ny) corner; a third-component source outside it, "
          "one cell away diagonally", shrink=SHRINK, obox=((11, 667), (23, 1000)), src=(2, 10, 666), at=("outside",)),
]

_CELLS = []
for _k, _kind in enumerate(("E", "H", "EH", "one")):
    for _t, (_T, _x, _y) in enumerate(((1, 8, 500), (5, 13, ("run", 2, 0)), (8, 7, ("run", 3, -1)))):
        _CELLS.append(Case2("cells-%s-T%d" % (_kind, _T), _T, CUT, "per-cell coefficients (%s), a source and an "
                            "output box cut on three sides" % _kind, obox=CUT_BOX, src=((_k + _t) % 3, _x, _y),
                            cells=_kind))

CASES2_LIST = _SEAMS + _CHUNKS + _SMALL + _INNER + _CELLS
CASES2 = {c.name: c for c in CASES2_LIST}
PARAMS2 = [(c.name, m, p) for c in CASES2_LIST for m in MODES for p in PRECS]


def size_of(cs, prec):
    return cs.size[prec] if isinstance(cs.size, dict) else cs.size


def obox_of(cs, prec):
    nx, ny = size_of(cs, prec)
    return cs.obox if cs.obox is not None else ((0, 0), (nx, ny))


def src_cell(cs, prec):
    """(slot, x, y) of the source with the symbolic y resolved."""
    if cs.src is None:
        return None
    slot, x, y = cs.src
    ny = size_of(cs, prec)[1]
    if isinstance(y, tuple):
        _, _, _, _, y0, own = launch2d(cs.T, prec, obox_of(cs, prec), cs.xchunk)
        y = y0 + y[1] * own + y[2]
    elif y < 0:
        y += ny
    return slot, x, y


def src_tags(cs, prec):
    """Where the source really sits, from the launch geometry."""
    slot, x, y = src_cell(cs, prec)
    nx, ny = size_of(cs, prec)
    ob = obox_of(cs, prec)
    runs, _, chunks, xc, y0, own = launch2d(cs.T, prec, ob, cs.xchunk)
    n = NV[prec]
    tags = set()
    k, r = divmod(y - y0, own)
    if r == own - 1 and k + 1 < runs:
        assert y % n == n - 1
        tags.add("lane-last")
    if r == 0 and 1 <= k < runs:
        assert y % n == 0
        tags.add("lane-first")
        if k % WPB == 0:
            tags.add("wg-seam")
    if y == 0:
        tags.add("y0")
    if y == ny - 1:
        tags.add("y-last")
    ck, cr = divmod(x - ob[0][0], xc)
    if 0 < ck < chunks - 1 and cr == 0:
        tags.add("chunk-first")
    if 0 < ck < chunks - 1 and cr == xc - 1:
        tags.add("chunk-last")
    if x == 0:
        tags.add("row0")
    if x == nx - 1:
        tags.add("row-last")
    if not (ob[0][0] <= x < ob[1][0] and ob[0][1] <= y < ob[1][1]):
        dist = max(ob[0][0] - x, x - ob[1][0] + 1, 0) + max(ob[0][1] - y, y - ob[1][1] + 1, 0)
        assert dist < cs.T, (cs.name, "the source cannot reach the output box")
        tags.add("outside")
    return tags


def assert_claim2(cs, prec, cus=256):
    got = launch2d(cs.T, prec, obox_of(cs, prec), cs.xchunk, cus)[:3]
    want = cs.claim[prec]
    assert got[0] >= want[0] and got[1] >= want[1] and got[2] == want[2], (cs.name, prec, "launch", got, "claimed", want)
    if cs.src is not None:
        assert set(cs.at) <= src_tags(cs, prec), (cs.name, prec, cs.at, src_tags(cs, prec))
    return got


def cfg2(mode, size):
    return SchemeConfig(scheme=mode, size=(size[0], size[1], 1), scene="vacuum", dtype="f64", use_fused=True)


def pair2(mode, size, prec, device, backend):
    """(scheme under test, fp64 torch oracle scheme) of one config."""
    cfg = cfg2(mode, size)
    ref = scheme(cfg, "torch", "cpu", torch.float64)
    dut = scheme(dataclasses.replace(cfg, dtype=prec), backend, device, DT[prec])
    return dut, ref


def impedance(s):
    e = next(c for c in s.comps if c[0] == "E")
    h = next(c for c in s.comps if c[0] == "H")
    return math.sqrt(s.cb[e].scalar / s.cb[h].scalar)


def box3(b):
    return ((b[0][0], b[0][1], 0), (b[1][0], b[1][1], 1))


@functools.lru_cache(None)
def inputs2(name, mode, prec):
    """Everything a 2D case reads, in fp64 on the CPU, rounded to the kernel's type."""
    cs = CASES2[name]
    if cs.same_as:
        return inputs2(cs.same_as, mode, prec)
    size = size_of(cs, prec)
    comps = COMPS2[mode]
    ref = scheme(cfg2(mode, size), "torch", "cpu", torch.float64)
    Z = impedance(ref)
    seed = 20000 + 100 * CASES2_LIST.index(cs) + 50 * MODES.index(mode)
    shape = (size[0], size[1], 1)
    rnd = lambda t: t.to(DT[prec]).double()
    fin = {c: rnd(randn(shape, seed + n) * (Z if c[0] == "E" else 1.0)) for n, c in enumerate(comps)}
    upd = {}
    for n, c in enumerate(comps):
        b = ref.local_box(c)
        if cs.shrink is not None:
            lx, ly, hx, hy = cs.shrink[n]
            b = ((b[0][0] + lx, b[0][1] + ly, 0), (b[1][0] - hx, b[1][1] - hy, 1))
        upd[c] = b
    src = None
    if cs.src is not None:
        slot, x, y = src_cell(cs, prec)
        amp = Z if comps[slot][0] == "E" else 1.0
        # (one value more than the pass takes: the level-shift probe of the CPU companion)
        src = [(comps[slot], (x, y, 0), float(rnd(torch.tensor(amp * (0.5 + 0.25 * l), dtype=torch.float64))))
               for l in range(cs.T + 1)]
    cells = {c: rnd(0.3 + 0.7 * rand(shape, seed + 10 + n)) for n, c in enumerate(comps)}
    return dict(size=size, shape=shape, fin=fin, upd=upd, obox=box3(obox_of(cs, prec)), src=src, cells=cells, Z=Z)


def _shift_y(b, ny):
    """A box moved one cell along y, towards the side with room."""
    sh = -1 if b[0][1] >= 1 else 1
    return ((b[0][0], b[0][1] + sh, b[0][2]), (b[1][0], b[1][1] + sh, b[1][2]))


def run2(name, mode, prec, dut, device, dtype, mutate=None):
    """One ``tb_step`` of a 2D case on the backend of scheme ``dut``; returns
    what it wrote (on the CPU) and the sentinels.  ``mutate`` (CPU companion):
    a deliberate error in what the op is handed, or in the order of its steps."""
    cs, inp = CASES2[name], inputs2(name, mode, prec)
    comps = COMPS2[mode]
    hip = dut.ops.name == "hip"
    if hip:
        dut.ops.tb_xchunk = cs.xchunk
    shape = inp["shape"]
    fin = {c: to_dev(inp["fin"][c], device, dtype) for c in comps}
    sent = {c: sentinel(shape, n) for n, c in enumerate(comps)}
    fout = {c: to_dev(sent[c], device, dtype) for c in comps}
    slots = list(CELL_SLOTS[mode][cs.cells])
    owner = {comps[n]: comps[n] for n in slots}
    if mutate == "swap-cells":
        a = comps[slots[0]]
        b = comps[(slots[0] + 1) % 3]
        owner[a], owner[b] = owner.get(b), owner.get(a)
    cb = dict(dut.cb)
    for c, o in owner.items():
        cb[c] = Coef(scalar=dut.cb[c].scalar, cell=None if o is None else to_dev(inp["cells"][o], device, dtype))
    upd = dict(inp["upd"])
    if mutate == "shift-box":
        c = comps[CASES2_LIST.index(CASES2[cs.same_as or name]) % 3]
        upd[c] = _shift_y(upd[c], shape[1])
    src = None if inp["src"] is None else inp["src"][:cs.T]
    if mutate == "src-level":
        src = [(s[0], s[1], nxt[2]) for s, nxt in zip(inp["src"][:-1], inp["src"][1:])]
    keep = {c: fin[c].clone() for c in comps}
    keep.update({"cell " + c: cb[c].cell.clone() for c in comps if cb[c].cell is not None})
    if mutate == "h-after":
        # the H source set AFTER the H update of its level: single steps of the op, the value forced behind each
        assert not hip and src is not None and src[0][0][0] == "H"
        whole = box3(((0, 0), (shape[0], shape[1])))
        cur = fin
        for l in range(cs.T):
            nxt = {c: cur[c].clone() for c in comps}
            dut.ops.tb_step(cur, nxt, upd, whole, cb, 1, None)
            nxt[src[l][0]][src[l][1]] = src[l][2]
            cur = nxt
        for c in comps:
            fout[c][box_slices(inp["obox"])] = cur[c][box_slices(inp["obox"])]
    else:
        dut.ops.tb_step(fin, fout, upd, inp["obox"], cb, cs.T, src)
    if hip:
        torch.cuda.synchronize()
    now = dict(fin)
    now.update({"cell " + c: cb[c].cell for c in comps if cb[c].cell is not None})
    assert_unchanged(now, keep, (name, mode, prec))
    return dict(fout={c: fout[c].cpu() for c in comps}, sent=sent)


@functools.lru_cache(None)
def oracle2(name, mode, prec, mutate=None):
    """The fp64 oracle's result (cases that differ in the chunking alone share it)."""
    cs = CASES2[name]
    if cs.same_as:
        return oracle2(cs.same_as, mode, prec, mutate)
    ref = scheme(cfg2(mode, size_of(cs, prec)), "torch", "cpu", torch.float64)
    return run2(name, mode, prec, ref, "cpu", torch.float64, mutate)


def masks2(name, mode, prec):
    """Per component: the cells the pass stores, and those of them outside the update box."""
    inp = inputs2(name, mode, prec)
    inside = torch.zeros(inp["shape"], dtype=torch.bool)
    inside[box_slices(inp["obox"])] = True
    carried = {}
    for c in COMPS2[mode]:
        u = torch.zeros(inp["shape"], dtype=torch.bool)
        u[box_slices(inp["upd"][c])] = True
        carried[c] = inside & ~u
    return inside, carried


def scales2(want, inside, comps):
    sc = {}
    for kind in "EH":
        sc[kind] = max(float(want[c][inside].abs().max()) for c in comps if c[0] == kind) + 1e-300
    return sc


def check2(name, mode, prec, out, bound):
    """``out`` of a backend (its type, on the CPU) against the oracle's;
    returns the largest error on its kind's scale."""
    want = oracle2(name, mode, prec)
    comps, dtype = COMPS2[mode], DT[prec]
    inside, carried = masks2(name, mode, prec)
    sc = scales2(want["fout"], inside, comps)
    worst = 0.0
    for c in comps:
        got, w, snt = out["fout"][c], want["fout"][c], want["sent"][c].to(dtype)
        bad = got[~inside] != snt[~inside]
        assert not bool(bad.any()), (name, mode, prec, c, "stored outside the output box", int(bad.sum()))
        m = carried[c]
        bad = got[m] != w[m].to(dtype)
        assert not bool(bad.any()), (name, mode, prec, c, "a cell outside the update box changed", int(bad.sum()))
        d = (got.double() - w).abs() * inside
        err = float(d.max())
        print("err 2d %s %s %s %s %.3g of %.3g" % (name, mode, prec, c, err / sc[c[0]], bound))
        if not err <= bound * sc[c[0]]:
            at = torch.nonzero(d == err)[0].tolist()
            raise AssertionError((name, mode, prec, c, "error", err, "scale", sc[c[0]], "bound", bound * sc[c[0]],
                                  "cell", at))
        worst = max(worst, err / sc[c[0]])
    return worst


@pytest.mark.parametrize("name,mode,prec", PARAMS2)
def test_tb2d_pass(gpu, name, mode, prec):
    """One k_tb2d launch from live fields against the fp64 oracle."""
    cs = CASES2[name]
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert_claim2(cs, prec, cus)
    dut, ref = pair2(mode, size_of(cs, prec), prec, gpu, "hip")
    assert all(dut.cb[c].scalar == ref.cb[c].scalar and dut.cb[c].is_scalar for c in COMPS2[mode])
    out = run2(name, mode, prec, dut, gpu, DT[prec])
    bound = bound_of("2d", prec)
    worst = check2(name, mode, prec, out, bound)
    print("worst 2d %s %s %s: %.3g of the bound" % (name, mode, prec, worst / bound))


# ======================================================================= 1D
NT = 1024                       # threads of the one workgroup
CPLS = {"f32": (1, 2, 4, 6, 8, 12, 16), "f64": (1, 2, 4, 6, 8, 12)}
GUARD = 64                      # guard elements around the 1D arrays: 256 B fp32, 512 B fp64


def cpl_of(n, src, prec):
    """The instance res1d takes (the module docstring's rule); None: too long."""
    for cpl in CPLS[prec]:
        off = 0 if src is None else (cpl - src % cpl) % cpl
        if n + off <= NT * cpl:
            return cpl
    return None


def max_cells(prec):
    """fdtd_res1d_max_cells: the longest grid that fits whatever the source cell."""
    c = CPLS[prec][-1]
    return NT * c - (c - 1)


@dataclasses.dataclass(frozen=True)
class Case1:
    name: str
    n: int
    src: object         # None or the source cell (negative: from n)
    cpl: int            # the instance the case reaches
    why: str
    steps: int = 37
    ebox: object = None  # None: the whole E box (1, n); (lo, hi) with hi <= 0 from n; "empty"
    hbox: object = None  # None: (0, n - 1)
    cells: str = ""     # per-cell coefficients on "E", "H" or "EH"
    precs: tuple = PRECS


F32 = ("f32",)
CASES1_LIST = [
    # every instance: a small n just past the previous one (source residue 0), the largest n that fits with
    # off = CPL - 1 (residue 1) and with off = 1 (residue CPL - 1), the largest n without a source
    Case1("cpl1-small", 7, 3, 1, "7 cells"),
    Case1("cpl1-max", 1024, 1000, 1, "the largest one-cell-per-thread grid"),
    Case1("cpl2-lo-r0", 1025, 512, 2, "just past CPL 1, src % 2 = 0"),
    Case1("cpl2-max-r1", 2047, 1001, 2, "src % 2 = 1: off 1, n + off = 2048"),
    Case1("cpl2-max-nosrc", 2048, None, 2, "no source: 2048 cells fit CPL 2"),
    Case1("cpl4-lo-r0", 2049, 1000, 4, "just past CPL 2, src % 4 = 0"),
    Case1("cpl4-max-r1", 4093, 2001, 4, "src % 4 = 1: off 3, n + off = 4096"),
    Case1("cpl4-max-rm", 4095, 3, 4, "src % 4 = 3: off 1, n + off = 4096"),
    Case1("cpl4-max-nosrc", 4096, None, 4, "no source"),
    Case1("cpl6-lo-r0", 4097, 3000, 6, "just past CPL 4, src % 6 = 0"),
    Case1("cpl6-max-r1", 6139, 3001, 6, "src % 6 = 1: off 5, n + off = 6144"),
    Case1("cpl6-max-rm", 6143, 4097, 6, "src % 6 = 5: off 1, n + off = 6144"),
    Case1("cpl6-max-nosrc", 6144, None, 6, "no source"),
    Case1("cpl8-lo-r0", 6145, 4000, 8, "just past CPL 6, src % 8 = 0"),
    Case1("cpl8-max-r1", 8185, 4001, 8, "src % 8 = 1: off 7, n + off = 8192"),
    Case1("cpl8-max-rm", 8191, 6151, 8, "src % 8 = 7: off 1, n + off = 8192"),
    Case1("cpl8-max-nosrc", 8192, None, 8, "no source"),
    Case1("cpl12-lo-r0", 8193, 6000, 12, "just past CPL 8, src % 12 = 0"),
    Case1("cpl12-max-r1", 12277, 6001, 12, "src % 12 = 1: off 11, n + off = 12288: resident_1d_max_cells() in fp64"),
    Case1("cpl12-max-rm", 12287, 6011, 12, "src % 12 = 11: off 1 (past the fp64 limit)", precs=F32),
    Case1("cpl12-rm", 9000, 6011, 12, "src % 12 = 11: off 1"),
    Case1("cpl12-max-nosrc", 12288, None, 12, "no source (past the fp64 limit)", precs=F32),
    Case1("cpl16-lo-r0", 12289, 8000, 16, "just past CPL 12, src % 16 = 0", precs=F32),
    Case1("cpl16-max-r1", 16369, 8001, 16, "src % 16 = 1: off 15: resident_1d_max_cells() in fp32", precs=F32),
    Case1("cpl16-rm", 12300, 8015, 16, "src % 16 = 15: off 1", precs=F32),
    # the shift pushes a grid into the next instance
    Case1("shift-2048-odd", 2048, 1023, 4, "2048 cells, odd source cell: CPL 2 needs 2049"),
    Case1("shift-2048-even", 2048, 1024, 2, "2048 cells, even source cell: CPL 2"),
    Case1("shift-4096", 4096, 4093, 6, "4096 cells, src % 4 = 1: CPL 4 needs 4099"),
    Case1("shift-8192", 8192, 8189, 12, "8192 cells, src % 8 = 5: CPL 8 needs 8195"),
    # source cells
    Case1("src-cell0", 3000, 0, 4, "source on cell 0, outside the E box: it still drives Hy[0] and stays in Ez"),
    Case1("src-last", 5001, -1, 6, "source on cell n - 1"),
    # steps
    Case1("steps0", 2049, 1000, 4, "no step: everything bit-identical", steps=0),
    Case1("steps1", 2049, 1000, 4, "one step", steps=1),
    Case1("steps1-r2", 3001, 1002, 4, "one step, src % 4 = 2", steps=1),
    # boxes
    Case1("boxes-in", 4100, 2050, 6, "E (5, n - 7), H (3, n - 9)", ebox=(5, -7), hbox=(3, -9)),
    Case1("boxes-in-src-out", 4100, 2, 6, "the same boxes, source outside both", ebox=(5, -7), hbox=(3, -9), steps=13),
    Case1("ebox-empty", 1500, 700, 2, "empty E box: Ez changes at the source alone", ebox="empty", steps=13),
    # per-cell coefficients
    Case1("cells-E", 6145, 4000, 8, "per-cell Cb alone (the kernel takes both arrays or neither)", cells="E"),
    Case1("cells-H", 6145, 4001, 8, "per-cell Db alone, src % 8 = 1", cells="H"),
    Case1("cells-EH", 6145, None, 8, "both, no source", cells="EH"),
    Case1("cells-EH-small", 700, 300, 1, "both at CPL 1", cells="EH"),
    Case1("cells-EH-12", 12277, 6001, 12, "both at CPL 12: the fp64 instance with the most registers", cells="EH"),
    Case1("cells-EH-16", 16369, 8001, 16, "both at CPL 16", cells="EH", precs=F32),
]
CASES1 = {c.name: c for c in CASES1_LIST}
PARAMS1 = [(c.name, p) for c in CASES1_LIST for p in c.precs]


def cfg1(n):
    return SchemeConfig(scheme="1d", size=(n, 1, 1), scene="vacuum", dtype="f64", use_fused=True)


def pair1(n, prec, device, backend):
    cfg = cfg1(n)
    ref = scheme(cfg, "torch", "cpu", torch.float64)
    dut = scheme(dataclasses.replace(cfg, dtype=prec), backend, device, DT[prec])
    return dut, ref


def src_of(cs):
    return None if cs.src is None else (cs.src + cs.n if cs.src < 0 else cs.src)


def boxes1(cs):
    """(E lo, E hi), (H lo, H hi)"""
    n = cs.n
    res = []
    for b, whole in ((cs.ebox, (1, n)), (cs.hbox, (0, n - 1))):
        if b is None:
            res.append(whole)
        elif b == "empty":
            res.append((0, 0))
        else:
            res.append((b[0], b[1] + n if b[1] <= 0 else b[1]))
    return res


def assert_claim1(cs, prec):
    got = cpl_of(cs.n, src_of(cs), prec)
    assert got == cs.cpl and cs.n <= max_cells(prec), (cs.name, prec, "CPL", got, "claimed", cs.cpl)


@functools.lru_cache(None)
def inputs1(name, prec):
    cs = CASES1[name]
    n = cs.n
    ref = scheme(cfg1(n), "torch", "cpu", torch.float64)
    Z = impedance(ref)
    seed = 60000 + 100 * CASES1_LIST.index(cs)
    rnd = lambda t: t.to(DT[prec]).double()
    # (one value more than the run takes: the level-shift probe of the CPU companion)
    vals = None if cs.src is None else rnd(Z * (0.5 + 0.05 * torch.arange(cs.steps + 1, dtype=torch.float64)))
    return dict(ez=rnd(Z * randn((n,), seed)), hy=rnd(randn((n,), seed + 1)), vals=vals, Z=Z,
                cells={"Ez": rnd(0.3 + 0.7 * rand((n, 1, 1), seed + 2)), "Hy": rnd(0.3 + 0.7 * rand((n, 1, 1), seed + 3))})


def run1(name, prec, dut, device, dtype, native=False, mutate=None):
    """One ``resident_1d`` of a 1D case on the backend of scheme ``dut``, the
    arrays inside one guarded buffer; returns Ez and Hy on the CPU."""
    cs, inp = CASES1[name], inputs1(name, prec)
    n, G = cs.n, GUARD
    hip = dut.ops.name == "hip"
    assert (G * dtype.itemsize) % 64 == 0
    guard = sentinel((3 * G + 2 * n,), 5)
    buf = to_dev(guard, device, dtype)
    ez, hy = buf[G:G + n], buf[2 * G + n:2 * G + 2 * n]
    ez.copy_(inp["ez"].to(dtype))
    hy.copy_(inp["hy"].to(dtype))
    F = {"Ez": ez.view(n, 1, 1), "Hy": hy.view(n, 1, 1)}
    (elo, ehi), (hlo, hhi) = boxes1(cs)
    if mutate == "shift-box":
        # one cell up where there is room, else the low edge alone (the H box when E is empty)
        if ehi > elo:
            elo, ehi = elo + 1, ehi + (1 if ehi < n else 0)
        else:
            hlo, hhi = hlo + 1, hhi + (1 if hhi < n - 1 else 0)
    boxes = {"Ez": ((elo, 0, 0), (ehi, 1, 1)), "Hy": ((hlo, 0, 0), (hhi, 1, 1))}
    owner = {c: c for c in ("Ez", "Hy") if c[0] in cs.cells}
    if mutate == "swap-cells":
        owner = {"Ez": owner.get("Hy"), "Hy": owner.get("Ez")}
    cb = dict(dut.cb)
    for c, o in owner.items():
        cb[c] = Coef(scalar=dut.cb[c].scalar, cell=None if o is None else to_dev(inp["cells"][o], device, dtype))
    src, vals = src_of(cs), None
    if src is not None:
        v = inp["vals"][1:] if mutate == "src-level" else inp["vals"][:max(cs.steps, 1)]
        vals = to_dev(v, device, dtype)
        if mutate == "src-cell":
            src = src + 1 if src + 1 < n else src - 1
    keep = {"cell " + c: cb[c].cell.clone() for c in cb if cb[c].cell is not None}
    if vals is not None:
        keep["vals"] = vals.clone()
    if not hip:
        dut.ops.native_1d = native
    dut.ops.resident_1d(F, boxes, cb, cs.steps, src, vals)
    if hip:
        torch.cuda.synchronize()
    else:
        dut.ops.native_1d = True
    now = {"cell " + c: cb[c].cell for c in cb if cb[c].cell is not None}
    if vals is not None:
        now["vals"] = vals
    assert_unchanged(now, keep, (name, prec))
    host, g = buf.cpu(), guard.to(dtype)
    for a, b in ((0, G), (G + n, 2 * G + n), (2 * G + 2 * n, 3 * G + 2 * n)):
        assert torch.equal(host[a:b], g[a:b]), (name, prec, "guard cells %d .. %d changed" % (a, b))
    return {"Ez": host[G:G + n].clone(), "Hy": host[2 * G + n:2 * G + 2 * n].clone()}


@functools.lru_cache(None)
def oracle1(name, prec, mutate=None):
    ref = scheme(cfg1(CASES1[name].n), "torch", "cpu", torch.float64)
    return run1(name, prec, ref, "cpu", torch.float64, False, mutate)


def check1(name, prec, out, bound):
    cs, inp, want = CASES1[name], inputs1(name, prec), oracle1(name, prec)
    dtype = DT[prec]
    worst = 0.0
    for c, (lo, hi) in zip(("Ez", "Hy"), boxes1(cs)):
        got, w = out[c], want[c]
        outside = torch.ones(cs.n, dtype=torch.bool)
        outside[lo:hi] = False
        if cs.steps == 0:
            outside[:] = True
            assert torch.equal(w, inp[c.lower()]), (name, "the oracle moved without a step")
        bad = got[outside] != w[outside].to(dtype)
        assert not bool(bad.any()), (name, prec, c, "a cell outside the box changed", int(bad.sum()))
        scale = float(w.abs().max()) + 1e-300
        d = (got.double() - w).abs()
        err = float(d.max())
        print("err 1d %s %s %s %.3g of %.3g" % (name, prec, c, err / scale, bound))
        if not err <= bound * scale:
            raise AssertionError((name, prec, c, "error", err, "scale", scale, "bound", bound * scale,
                                  "cell", int(d.argmax())))
        worst = max(worst, err / scale)
    return worst


@pytest.mark.parametrize("name,prec", PARAMS1)
def test_res1d_run(gpu, name, prec):
    """One k_res1d launch from live fields against the fp64 torch loop."""
    cs = CASES1[name]
    assert_claim1(cs, prec)
    dut, ref = pair1(cs.n, prec, gpu, "hip")
    assert dut.ops.resident_1d_max_cells() == max_cells(prec)
    assert all(dut.cb[c].scalar == ref.cb[c].scalar and dut.cb[c].is_scalar for c in ("Ez", "Hy"))
    out = run1(name, prec, dut, gpu, DT[prec])
    bound = bound_of("1d", prec)
    worst = check1(name, prec, out, bound)
    print("worst 1d %s %s: %.3g of the bound" % (name, prec, worst / bound))
