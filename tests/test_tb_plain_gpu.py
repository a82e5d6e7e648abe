"""The plain temporally blocked 3D passes -- ``ops.tb_step`` without TF/SF,
Drude or amplitude features: the fp32 multi-row kernel (csrc/tb3d_mr.h
k_tb3d_mr, the kernel the benchmark measures), the fp32 single-row kernel
(csrc/yee3d_tb.hip k_tb3d) and the fp64 kernel (csrc/yee3d_tb64.hip
k_tb3d_f64) -- one launch at a time on live state against the fp64 torch
oracle, interior tiles included.

The form is that of tests/test_tb_variants_gpu.py, whose helpers this module
imports: one ``SchemeConfig`` gives a HIP scheme and an fp64 torch / CPU
scheme; the fields are drawn once in fp64 (E ~ Z N(0, 1), H ~ N(0, 1), Z the
wave impedance, so Cb curl H is of the size of E and Db curl E of the size of
H from the first level on), source values are scaled by Z, every output is
pre-filled with the sentinel pattern, and ONE ``tb_step`` runs per backend.
Then

* outside what the oracle wrote the outputs are bit-identical to the sentinel,
* the inputs (fields and per-cell coefficient arrays) are bit-unchanged,
* errors are taken per component against the kind's maximum over what the
  oracle wrote, within ``BOUND32`` = 2e-5 (fp32) or ``BOUND64_PLAIN`` = 1e-12
  (fp64): the project's own bounds for these kernels.

Tile arithmetic (``V.tiles`` / ``V.seams`` / ``all_in`` mirror the launchers
launch_tb_mr, launch_tb and launch_tb64): tile (ty, tz) of a launch over the
output box O loads the rows ``O.lo.y - T + (ROWS - 2T) ty .. + ROWS`` and the
lanes ``O.lo.z - T + (LANES - 2T) tz .. + LANES`` (``V.GEOM``).  k_tb3d_mr runs
two copies of its x loop: the masked one, and a fast path for the tiles whose
every row and lane lies inside the arrays and inside all six update boxes in
y / z (``all_in``), where a coefficient is only the x-range-selected scalar.
(The kernel takes the decision per wave, ``__all`` over the wave's own rows:
in an all-in tile every wave runs the fast path, in a border tile the waves
off the border do and the others run the masked loop.)  On a benchmark grid
nearly every tile takes the fast path; the cases here have tiles of both kinds
and say which (asserted by tests/test_tb_plain_cpu.py for every case, together
with fp32 conditioning and liveness).

Every case table below is shared with tests/test_tb_plain_cpu.py, so the GPU
tests cannot run a case the CPU checks did not see.
"""
import copy
import dataclasses
import functools
import os
import subprocess
import sys

import pytest
import torch

import test_tb_variants_gpu as V
from fdtd3d_amd.ops.coef import Coef
from fdtd3d_amd.ops.torch_ops import box_slices

pytestmark = pytest.mark.gpu

BOUND = {"f32": V.BOUND32, "f64": V.BOUND64_PLAIN}
SIZE = (14, 72, 144)         # the main grid: nz % 4 == 0, 145k cells
MAP_SIZE = (6, 250, 118)     # the fp64 tile-map grid: 177k cells
PC1_SIZE = (12, 40, 264)     # per-cell planes on the single-row kernel: a z seam at T = 2 needs nz > 248
NOBOX = ((0, 0, 0), (0, 0, 0))

# kernel -> (precision, the knobs that force it); the name is also the family of V.GEOM / V.tiles
KERN = {
    "mr16x2": ("f32", dict(tb_mrows=2, tb_mr_shape=0)),
    "mr8x4": ("f32", dict(tb_mrows=2, tb_mr_shape=1)),
    "mr8x2": ("f32", dict(tb_mrows=2, tb_mr_shape=2)),   # T <= 5 (launch_tb_mr_sel; T = 6 runs the 16 x 2 form)
    "single": ("f32", dict(tb_mrows=1)),                 # T <= 4
    "f64half": ("f64", dict(tb64_half=1)),               # T <= 5
    "f64full": ("f64", dict(tb64_half=0)),
}
# every tuning knob at its default (``tb_thin_mr16`` follows an environment variable: off here unless a test asks)
KNOBS0 = dict(tb_xchunk=V.XCHUNK, tb_mrows=0, tb_mr_shape=0, tb_vec=0, tb_rows=0, tb_xcd=0, tb_variant=4, tb64_half=1,
              tb_thin_single_row=True, tb_thin_mr16=False, tb_sparse=True)


# ==================================================================== cases
@dataclasses.dataclass(frozen=True)
class Case:
    """What one pass computes (the oracle's side): kernels and knobs are the tests' parameters."""
    name: str
    T: int
    size: tuple
    obox: tuple
    upd: str        # update boxes: "local" (the scheme's), "whole", "six", "xcut", "empty" (``update_boxes``)
    src: object     # None or (E component, cell)
    region: object  # None or the box of per-cell coefficients
    kinds: str      # "", "E", "H", "EH": the kinds with per-cell coefficients
    seed: int


CASES = {}


def case(name, T, size=SIZE, obox=None, upd="local", src=None, region=None, kinds=""):
    if name not in CASES:
        CASES[name] = Case(name, T, tuple(size), obox or ((0, 0, 0), tuple(size)), upd, src, region, kinds,
                           20000 + 40 * len(CASES))
    return name


# (b) of the update-box cases: six different unaligned interior boxes.  Ey's cuts in y (40) and z (100) through
# tile (1, 1) of the 32-row launches (T = 3: rows 23 .. 55, lanes 55 .. 119; T = 5: 17 .. 49, 49 .. 113), Hz's cuts
# mostly in x.
SIX = {"Ex": ((1, 3, 5), (12, 69, 139)), "Ey": ((2, 1, 2), (13, 40, 100)), "Ez": ((0, 2, 3), (14, 70, 141)),
       "Hx": ((3, 0, 1), (11, 71, 143)), "Hy": ((1, 4, 0), (13, 68, 137)), "Hz": ((4, 2, 6), (9, 72, 144))}
# ... and boxes that differ from the scheme's in x only: the interior tile stays all-in and only ``xin`` selects
XCUT = {"Ex": (3, 11), "Ez": (2, 9), "Hy": (4, 13), "Hz": (0, 6)}
EMPTY = ("Ey", "Hz")  # (c): one E and one H component never update


def update_boxes(kind, ref):
    local = V.drude_upd(ref)
    size = tuple(ref.F[0]["Ex"].shape)
    if kind == "local":
        return local
    if kind == "whole":
        return {c: ((0, 0, 0), size) for c in V.COMPS}
    if kind == "six":
        assert size == SIZE
        return dict(SIX)
    if kind == "xcut":
        return {c: ((XCUT[c][0],) + tuple(b[0][1:]), (XCUT[c][1],) + tuple(b[1][1:])) if c in XCUT else b
                for c, b in local.items()}
    if kind == "empty":
        return {c: NOBOX if c in EMPTY else b for c, b in local.items()}
    raise KeyError(kind)


@functools.lru_cache(None)
def cells_of(name, shift=0):
    """Per-cell factors (fp64 values exact in fp32) of a case: 0.3 .. 1.0 inside the region (``shift``: the region
    moved by that many rows, the CPU companion's deliberate error), 1 outside.  Ex, Ez / Hy, Hz vary; one
    component per kind stays scalar (tests/test_tb_gpu.py test_tb_sparse_coefs)."""
    cs = CASES[name]
    out = {}
    for n, c in enumerate(("Ex", "Ez", "Hy", "Hz")):
        if c[0] not in cs.kinds:
            continue
        r = cs.region
        sl = box_slices(r)
        cell = torch.ones(cs.size, dtype=torch.float64)
        vals = 0.3 + 0.7 * V.rand(cell[sl].shape, cs.seed + 10 + n)
        cell[box_slices(((r[0][0], r[0][1] + shift, r[0][2]), (r[1][0], r[1][1] + shift, r[1][2])))] = vals
        out[c] = cell.float().double()
    return out


@functools.lru_cache(None)
def inputs(name):
    """Everything a case reads, in fp64 on the CPU (drawn once)."""
    cs = CASES[name]
    ref = V.scheme(V.vacuum_cfg(cs.size, "f64"), "torch", "cpu", torch.float64)
    Z = V.impedance(ref)
    src = None
    if cs.src is not None:
        src = [(cs.src[0], tuple(cs.src[1]), Z * (0.5 + 0.25 * l)) for l in range(cs.T)]
    return dict(fin=V.live_fields(cs.size, cs.seed, Z), Z=Z, upd=update_boxes(cs.upd, ref), src=src)


def device_state(name, device, dtype):
    """Device inputs, outputs, sentinels, input clones and the sentinel fill: one set serves a loop of launches."""
    fin, fout, sent, keep = V.run_pair_fields(inputs(name)["fin"], CASES[name].size, device, dtype)
    return fin, fout, sent, keep, {c: fout[c].clone() for c in V.COMPS}


def _shift_box(b, size):
    """``b`` moved by one row in y, towards the side with room."""
    sh = 1 if b[1][1] + 1 <= size[1] else -1
    return ((b[0][0], b[0][1] + sh, b[0][2]), (b[1][0], b[1][1] + sh, b[1][2]))


def _db_scaled(ops, factor):
    """A copy of the torch ops whose first H half step (the first level's) runs with Db * factor."""
    out = copy.copy(ops)
    inner, calls = ops.curl_update, [0]

    def curl_update(kind, boxes, dst, src, cb):
        if kind == "H":
            calls[0] += 1
            if calls[0] == 1:
                cb = {c: Coef(k.scalar * factor, k.px, k.py, k.pz, k.cell) if c[0] == "H" else k for c, k in cb.items()}
        return inner(kind, boxes, dst, src, cb)
    out.curl_update = curl_update
    return out


MUTATIONS = ("shift-box", "drop-last", "move-src", "no-src", "db-1e-3", "db-1e-2", "shift-region")


def run(name, dut, device, dtype, mutate=None, state=None, record=None, **knobs):
    """One ``tb_step`` of case ``name`` on the backend of scheme ``dut``; returns what it wrote (on the CPU) and
    the sentinels.  ``knobs`` override ``KNOBS0``; ``state`` (``device_state``) is reused when given; ``record``
    (a list) receives the launch (``HipOps.record``); ``mutate`` (CPU companion): a deliberate error in what
    the oracle is handed."""
    cs, inp = CASES[name], inputs(name)
    hip = dut.ops.name == "hip"
    V.set_knobs(dut.ops, **{**KNOBS0, **knobs})
    upd, src, ops, shift = inp["upd"], inp["src"], dut.ops, 0
    assert mutate is None or (mutate in MUTATIONS and not hip)
    if mutate == "shift-box":
        victim = next(c for c in ("Hz", "Ex", "Hx") if not V._empty(upd[c]))
        upd = {**upd, victim: _shift_box(upd[victim], cs.size)}
    elif mutate == "drop-last":
        src = src[:-1] + [None]
    elif mutate == "move-src":
        i = src[0][1][0]
        at = (i + 1 if i + 1 < cs.size[0] else i - 1,) + tuple(src[0][1][1:])
        src = [(s[0], at, s[2]) for s in src]
    elif mutate == "no-src":
        src = None
    elif mutate in ("db-1e-3", "db-1e-2"):
        ops = _db_scaled(ops, 1.0 + float(mutate[3:]))
    elif mutate == "shift-region":
        shift = 1
    if state is None:
        state = device_state(name, device, dtype)
    fin, fout, sent, keep, fill = state
    for c in V.COMPS:
        fout[c].copy_(fill[c])
    cb, cells = dict(dut.cb), {}
    for c, cell in cells_of(name, shift).items():
        cells[c] = cell.to(dtype).to(device).contiguous().clone()
        cb[c] = Coef(scalar=dut.cb[c].scalar, cell=cells[c])
    kept = {c: t.clone() for c, t in cells.items()}
    if record is not None:
        ops.record(record)
    try:
        ops.tb_step(fin, fout, upd, cs.obox, cb, cs.T, src)
    finally:
        if record is not None:
            ops.record(None)
        if hip:
            torch.cuda.synchronize()
            V.set_knobs(dut.ops, **KNOBS0)
    V.assert_unchanged(fin, keep, name)
    V.assert_unchanged(cells, kept, (name, "coefficient arrays"))
    return dict(fout={c: fout[c].detach().to("cpu", copy=True) for c in V.COMPS}, sent=sent)


@functools.lru_cache(None)
def oracle(name, mutate=None):
    ref = V.scheme(V.vacuum_cfg(CASES[name].size, "f64"), "torch", "cpu", torch.float64)
    return run(name, ref, "cpu", torch.float64, mutate)


def check(name, out, prec, tag=(), bound=None):
    """``out`` of a backend against the oracle's; returns the worst error as a fraction of the bound."""
    want = oracle(name)
    bound = BOUND[prec] if bound is None else bound
    worst, _ = V.check_fields(out["fout"], want["fout"], want["sent"], V.DT[prec], bound, (name,) + tuple(tag))
    return worst / bound


def hip_pair(name, prec, device):
    return V.pair(V.vacuum_cfg(CASES[name].size, "f64"), prec, device, "hip")[0]


def run_check(name, kern, device, tag=(), state=None, **knobs):
    """Case ``name`` on kernel ``kern`` (``KERN``) of the HIP backend, checked: the fraction of the bound."""
    prec, force = KERN[kern]
    dut = hip_pair(name, prec, device)
    out = run(name, dut, device, V.DT[prec], state=state, **{**force, **knobs})
    return check(name, out, prec, (kern,) + tuple(tag))


# ========================================================== tile arithmetic
def all_in(family, T, obox, upd, size, ty, tz):
    """Tile (ty, tz): every row and lane it loads lies inside the arrays and inside all six update boxes in
    y / z (tb3d_mr.h ``tile_all``; the box's x range does not count: ``xin`` selects it per plane)."""
    rows, lanes = V.GEOM[family]
    j0 = obox[0][1] - T + (rows - 2 * T) * ty
    k0 = obox[0][2] - T + (lanes - 2 * T) * tz
    if j0 < 0 or j0 + rows > size[1] or k0 < 0 or k0 + lanes > size[2]:
        return False
    return all(b[0][1] <= j0 and j0 + rows <= b[1][1] and b[0][2] <= k0 and k0 + lanes <= b[1][2]
               for b in upd.values())


def tile_kinds(family, T, name):
    """(all-in tiles, the others) of the launch of case ``name``."""
    cs, inp = CASES[name], inputs(name)
    _, gy, gz = V.tiles(family, T, cs.obox)
    inn = [(ty, tz) for ty in range(gy) for tz in range(gz) if all_in(family, T, cs.obox, inp["upd"], cs.size, ty, tz)]
    return inn, [(ty, tz) for ty in range(gy) for tz in range(gz) if (ty, tz) not in inn]


def lib_family(prec, T, mrows, mr_shape, percell=False, half=1):
    """The kernel a plain pass lands in from the options it passes: the rule of fdtd_tb3d_v4_f32 and
    launch_tb_mr_sel (fp32), tb64_run (fp64)."""
    if prec == "f64":
        return "f64half" if half else "f64full"
    mr = mrows if mrows else (2 if T >= 4 and not percell else 1)
    if not percell and (mr > 1 or T > 4):
        return "mr8x4" if mr_shape == 1 else "mr8x2" if mr_shape == 2 and T <= 5 else "mr16x2"
    assert T <= 4
    return "single"


def auto_opts(T, obox, thin_mr16, mrows=0, mr_shape=0, thin_single_row=True):
    """(mrows, mr_shape) a plain fp32 pass hands the library: ``HipOps._tb_opts``'s thin-shell rule."""
    if mrows == 0 and thin_single_row and T <= 4 and obox[1][1] - obox[0][1] <= 8:
        return (0, 2) if thin_mr16 else (1, mr_shape)
    return mrows, mr_shape


def passed_opts(rec):
    """The ``TbOpts`` of the one recorded launch."""
    assert len(rec) == 1, [f.__name__ for f, _ in rec]
    opts = [a._obj for a in rec[0][1] if type(getattr(a, "_obj", None)).__name__ == "TbOpts"]
    assert len(opts) == 1
    return rec[0][0].__name__, opts[0]


# ======================================= 1. interior tiles, every T and shape
MR_SHAPES = ("mr16x2", "mr8x4", "mr8x2")
INTERIOR = [(T, k) for T in range(1, 7) for k in MR_SHAPES if not (k == "mr8x2" and T == 6)]
for _T in range(1, 7):
    case("int-T%d" % _T, _T)


def interior_claims(T, kern):
    """The launch has at least one all-in tile and one that is not, two tiles per axis and x chunks."""
    name = "int-T%d" % T
    inn, out = tile_kinds(kern, T, name)
    assert inn and out, (T, kern, "all-in", inn, "masked", out)
    V.assert_tiles(kern, T, CASES[name].obox, (3, 3, 3))
    return inn, out


@pytest.mark.parametrize("T,kern", INTERIOR)
def test_interior_tiles(gpu, T, kern):
    """Whole grid, the scheme's update boxes: interior tiles take the fast path, border tiles the masked loop.
    All 16 ``tb_variant`` values (bit 0 deferred stores, 1 two planes prefetched, 2 XCD-contiguous order, 3 no
    fast path) from one set of device inputs: bit 3 set and clear both meet the bound."""
    name = "int-T%d" % T
    inn, out = interior_claims(T, kern)
    state = device_state(name, gpu, torch.float32)
    worst = {}
    for variant in range(16):
        try:
            worst[variant] = run_check(name, kern, gpu, ("variant %d" % variant,), state, tb_variant=variant)
        except AssertionError as e:
            raise AssertionError("tb_variant %d (T %d, %s): %s" % (variant, T, kern, e)) from e
    fast = max(v for k, v in worst.items() if not k & 8)
    masked = max(v for k, v in worst.items() if k & 8)
    print("worst interior T %d %s: fast path %.3g, masked everywhere %.3g of the bound (%d all-in tiles, %d others)"
          % (T, kern, fast, masked, len(inn), len(out)))


# ============================================================== 2. x chunks
XCHUNK_KERNELS = [("mr16x2", 5), ("mr16x2", 2), ("single", 2), ("f64half", 4)]
XCHUNKS = (1, 3, SIZE[0], 0)  # 1 and 3: shorter than T (lead-in and drain overlap); one chunk; automatic


@pytest.mark.parametrize("kern,T", XCHUNK_KERNELS)
def test_xchunks(gpu, kern, T):
    """``tb_xchunk`` 1, 3, nx and 0 (pick_xchunk / tb_mr_xchunk / pick_xchunk64 with the device's CU count)."""
    name = "int-T%d" % T
    assert min(XCHUNKS[:2]) < T or T == 2
    state = device_state(name, gpu, V.DT[KERN[kern][0]])
    worst, outs = 0.0, []
    for xc in XCHUNKS:
        prec, force = KERN[kern]
        dut = hip_pair(name, prec, gpu)
        out = run(name, dut, gpu, V.DT[prec], state=state, **{**force, "tb_xchunk": xc})
        try:
            worst = max(worst, check(name, out, prec, (kern, "xchunk %d" % xc)))
        except AssertionError as e:
            raise AssertionError("tb_xchunk %d (T %d, %s): %s" % (xc, T, kern, e)) from e
        outs.append(out["fout"])
    same = all(torch.equal(outs[0][c], o[c]) for o in outs[1:] for c in V.COMPS)
    print("worst xchunk T %d %s: %.3g of the bound; the four chunkings agree bit for bit: %s" % (T, kern, worst, same))


# =========================================================== 3. update boxes
UPD_KINDS = ("whole", "six", "xcut", "empty")
UPD_KERNELS = [("mr16x2", 3), ("mr16x2", 5), ("single", 3), ("f64half", 4)]
UPDATE = [(w, k, T) for w in UPD_KINDS for k, T in UPD_KERNELS]
for _w in UPD_KINDS:
    for _T in (3, 4, 5):
        case("upd-%s-T%d" % (_w, _T), _T, upd=_w)


def update_claims(which, kern, T):
    """Tile (1, 1) is all-in under the scheme's boxes; (a) whole-array boxes and the x-only cut keep it so, (b)
    the six boxes and (c) the empty ones do not: there the masked copy runs on an interior tile."""
    if not kern.startswith("mr"):
        return None
    assert (1, 1) in tile_kinds(kern, T, "int-T%d" % T)[0]
    inn, out = tile_kinds(kern, T, "upd-%s-T%d" % (which, T))
    assert ((1, 1) in inn) == (which in ("whole", "xcut")), (which, kern, T, inn)
    return inn, out


@pytest.mark.parametrize("which,kern,T", UPDATE)
def test_update_boxes(gpu, which, kern, T):
    """Update boxes other than the scheme's: a cell outside its component's box carries its input value at every
    level, and its neighbours read it."""
    update_claims(which, kern, T)
    worst = run_check("upd-%s-T%d" % (which, T), kern, gpu)
    print("worst update boxes %s T %d %s: %.3g of the bound" % (which, T, kern, worst))


# =========================================================== 4. output boxes
OUT_BOXES = {
    "inner-z1": ((2, 5, 5), (12, 66, 131)),     # unaligned, lo.z % 4 == 1
    "inner-z2": ((3, 7, 6), (11, 60, 139)),     # lo.z % 4 == 2
    "inner-z3": ((1, 9, 7), (13, 70, 141)),     # lo.z % 4 == 3
    "z-shell": ((0, 0, 2), (14, 72, 4)),        # 2 cells in z
    "x-shell": ((7, 0, 0), (8, 72, 144)),       # one plane
    "y-shell5": ((0, 3, 0), (14, 8, 144)),      # 5 rows
    "y-shell8": ((0, 64, 0), (14, 72, 144)),    # 8 rows: the thin-shell switch of _tb_opts
    "cell": ((6, 35, 70), (7, 36, 71)),
    "corner": ((9, 50, 101), (14, 72, 144)),    # ends on the grid's high corner
}
OUT_T = (2, 4, 5)  # defaults: T = 2 single-row, 4 multi-row or (thin y shells) 16-row tiles, 5 multi-row
OUTPUT = [(b, T, thin) for b in OUT_BOXES for T in OUT_T for thin in ((False, True) if b == "y-shell8" else (False,))]
for _b, _ob in OUT_BOXES.items():
    for _T in OUT_T:
        case("out-%s-T%d" % (_b, _T), _T, obox=_ob)


def output_family(box, T, thin_mr16):
    """The family a default-knob fp32 pass over the box lands in, spelt out: T = 2 is below the multi-row
    threshold; T = 5 is above the thin branch's; at T = 4 the y shells and the single cell (<= 8 rows) take
    16-row tiles."""
    if T == 2:
        return "single"
    if T == 4 and box in ("y-shell5", "y-shell8", "cell"):
        return "mr8x2" if thin_mr16 else "single"
    return "mr16x2"


@pytest.mark.parametrize("box,T,thin_mr16", OUTPUT)
def test_output_boxes(gpu, box, T, thin_mr16):
    """Output boxes with the tuning knobs at their defaults: ``_tb_opts`` and the library choose the kernel.
    The family comes from the options the launch really passed (recorded), by the library's rule."""
    name = "out-%s-T%d" % (box, T)
    dut = hip_pair(name, "f32", gpu)
    rec = []
    out = run(name, dut, gpu, torch.float32, record=rec, tb_thin_mr16=thin_mr16)
    fn, o = passed_opts(rec)
    assert fn == "fdtd_tb3d_v4_f32", fn
    assert (o.mrows, o.mr_shape) == auto_opts(T, OUT_BOXES[box], thin_mr16), (box, T, o.mrows, o.mr_shape)
    family = lib_family("f32", T, o.mrows, o.mr_shape)
    assert family == output_family(box, T, thin_mr16), (box, T, thin_mr16, family)
    worst = check(name, out, "f32", (family,))
    print("worst output box %s T %d thin_mr16 %s -> %s: %.3g of the bound" % (box, T, thin_mr16, family, worst))


@pytest.mark.parametrize("box", list(OUT_BOXES))
def test_output_boxes_f64(gpu, box):
    worst = run_check("out-%s-T4" % box, "f64half", gpu)
    print("worst output box %s T 4 f64half: %.3g of the bound" % (box, worst))


# =============================================================== 5. sources
SRC_OBOX = ((0, 0, 8), (14, 72, 136))  # whole in x and y (border cells are stored), room below it in z
SRC_KERNELS = [("mr16x2", 5), ("single", 3), ("f64half", 4)]
SRC_WHERE = ("inside", "first", "last", "xseam", "near", "border", "far")
SOURCES = [(k, T, c) for k, T in SRC_KERNELS for c in V.E]


def source_cell(kern, T, comp, where):
    """The source's cell: ``inside`` tile (1, 1) off its seams; on the ``first`` / ``last`` owned row and lane
    of a tile (both sides of a y seam and a z seam); on the first plane of x chunk 1 (``xseam``); two cells
    below the output box (``near``: within T of it); on a grid ``border`` cell outside the component's update
    box (inside the output box: the value is still set and stored); ``far``: T + 2 cells below the box."""
    sx, sy, sz = (s[0] for s in V.seams(kern, T, SRC_OBOX))
    mid = (7, sy + 4, sz + 5)
    return {"inside": mid, "first": (7, sy, sz), "last": (7, sy - 1, sz - 1), "xseam": (sx, mid[1], mid[2]),
            "near": (7, mid[1], SRC_OBOX[0][2] - 2), "far": (7, mid[1], SRC_OBOX[0][2] - T - 2),
            "border": (0, mid[1], mid[2]) if comp == "Ey" else (7, 0, mid[2])}[where]


def source_case(kern, T, comp, where):
    return "src-%s-%s-%s" % (kern, comp, where)


for _k, _T, _c in SOURCES:
    for _w in SRC_WHERE:
        case(source_case(_k, _T, _c, _w), _T, obox=SRC_OBOX, src=(_c, source_cell(_k, _T, _c, _w)))


@pytest.mark.parametrize("kern,T,comp", SOURCES)
def test_sources(gpu, kern, T, comp):
    """A hard source on each E component, the same point at every level with the values Z (0.5 + 0.25 l)."""
    worst = {}
    for where in SRC_WHERE:
        try:
            worst[where] = run_check(source_case(kern, T, comp, where), kern, gpu, (where,))
        except AssertionError as e:
            raise AssertionError("source %s %s (T %d, %s): %s" % (comp, where, T, kern, e)) from e
    print("worst source %s T %d %s: %.3g of the bound (%s)" % (comp, T, kern, max(worst.values()),
                                                              ", ".join("%s %.3g" % kv for kv in worst.items())))


# ================================================= 6. per-cell coefficients
PC_REGION = ((3, 20, 40), (9, 50, 126))     # on SIZE: crosses the x-chunk seam at 5 and y / z seams of every form
PC1_REGION = ((3, 6, 100), (9, 30, 256))    # on PC1_SIZE: ... the single-row kernel's, z = 248 at T = 2 included
# (kernel whose tiles the region must cross, knobs, T, grid): the sparse float4 form runs on the multi-row
# kernel through fdtd_tb3d_ext_f32 whatever tb_mrows says, full planes on the single-row kernel
PC_FORMS = {
    "sparse": ("mr16x2", dict(tb_sparse=True), (1, 3, 5), "pc"),
    "planes": ("single", dict(tb_sparse=False), (2, 4), "pc1"),
    "f64half": ("f64half", dict(tb64_half=1), (4,), "pc"),
    "f64full": ("f64full", dict(tb64_half=0), (4,), "pc"),
}
PERCELL = [(f, T, kinds) for f, (_, _, Ts, _) in PC_FORMS.items() for T in Ts for kinds in ("E", "H", "EH")]
for _f, _T, _kinds in PERCELL:
    if PC_FORMS[_f][3] == "pc":
        case("pc-%s-T%d" % (_kinds, _T), _T, region=PC_REGION, kinds=_kinds)
    else:
        case("pc1-%s-T%d" % (_kinds, _T), _T, size=PC1_SIZE, region=PC1_REGION, kinds=_kinds)


def percell_case(form, T, kinds):
    return "%s-%s-T%d" % (PC_FORMS[form][3], kinds, T)


def percell_claims(form, T, kinds):
    """The region crosses an x-chunk seam, a y seam and a z seam of the form's launch."""
    cs = CASES[percell_case(form, T, kinds)]
    sm = V.seams(PC_FORMS[form][0], T, cs.obox)
    for d in range(3):
        assert any(cs.region[0][d] < q < cs.region[1][d] for q in sm[d]), (form, T, "xyz"[d], sm[d], cs.region)


@pytest.mark.parametrize("form,T,kinds", PERCELL)
def test_percell(gpu, form, T, kinds):
    """A dielectric / magnetic region (0.3 .. 1.0 times the scalar per cell) on live state: E only, H only and
    both, in the sparse multi-row form, the single-row full-plane form and fp64 (both tile shapes)."""
    percell_claims(form, T, kinds)
    kern, knobs, _, _ = PC_FORMS[form]
    name = percell_case(form, T, kinds)
    prec = KERN[kern][0]
    dut = hip_pair(name, prec, gpu)
    rec = []
    out = run(name, dut, gpu, V.DT[prec], record=rec, **knobs)
    fn = passed_opts(rec)[0]
    assert fn == {"sparse": "fdtd_tb3d_ext_f32", "planes": "fdtd_tb3d_v4_f32"}.get(form, "fdtd_tb3d_f64"), fn
    worst = check(name, out, prec, (form,))
    print("worst per-cell %s %s T %d: %.3g of the bound" % (form, kinds, T, worst))


def test_sparse_arrays_follow_the_coefficients(gpu):
    """Two passes of ONE scheme whose H coefficient dicts share the scalar ``Hx`` object and differ in the
    per-cell ``Hy`` / ``Hz``: the wrapper's cached float4 arrays (``HipOps._sparse_kind``, kept on the kind's
    first Coef) belong to the three Coef objects they were built from, so the second pass runs with its own."""
    first, second = percell_case("sparse", 1, "H"), percell_case("sparse", 3, "H")
    assert not torch.equal(cells_of(first)["Hy"], cells_of(second)["Hy"])
    dut = hip_pair(first, "f32", gpu)
    assert hip_pair(second, "f32", gpu) is dut
    for name in (first, second, first):
        worst = check(name, run(name, dut, gpu, torch.float32, tb_sparse=True), "f32", ("shared Hx",))
        print("worst sparse arrays %s: %.3g of the bound" % (name, worst))


# ========================================================= 7. fp64 tile map
MAP = [(T, half) for T in range(1, 6) for half in (1, 0)]
for _T in range(1, 6):
    case("map-T%d" % _T, _T, size=MAP_SIZE)


def map_grid(T, half):
    """(gx, gy, gz) and the launch's place in the 2 x 8 patch walk of tb64_patch: ``narrow`` = a narrower last
    band (gy > 8, gy % 8 != 0) and a narrower last column (odd gz), ``tail`` = a tile count that is no multiple
    of 8 (the tiles past ``n8`` keep their own index)."""
    g = V.tiles("f64half" if half else "f64full", T, CASES["map-T%d" % T].obox)
    return g, dict(narrow=g[1] > 8 and g[1] % 8 != 0 and g[2] % 2 == 1, tail=(g[0] * g[1] * g[2]) % 8 != 0)


@pytest.mark.parametrize("T,half", MAP)
def test_f64_tile_map(gpu, T, half):
    """The default patch walk over grids with a narrower last band and column: with sentinel outputs every tile
    ran exactly where it should."""
    g, what = map_grid(T, half)
    worst = run_check("map-T%d" % T, "f64half" if half else "f64full", gpu)
    print("worst fp64 tile map T %d half %d tiles %s %s: %.3g of the bound" % (T, half, g, what, worst))


# ==================================== 8. tile-order environment knobs (child)
CHILD_ENV = {"FDTD3D_TB_PATCH": "2x3", "FDTD3D_TB64_PATCH": "3x2"}  # read once at first use: a fresh process
CHILD_RUNS = [("int-T5", "mr16x2", dict(tb_variant=4)), ("map-T4", "f64half", {})]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_main():
    """The child's work: the runs of ``CHILD_RUNS`` through ``run_check``, one line each; stops at the first
    mismatch (nothing is launched after a failure) with a non-zero status."""
    assert all(os.environ.get(k) == v for k, v in CHILD_ENV.items())
    from fdtd3d_amd.ops import hip_ops
    hip_ops.load_library(build_if_missing=True)
    for name, kern, knobs in CHILD_RUNS:
        try:
            worst = run_check(name, kern, "cuda:0", **knobs)
        except AssertionError as e:
            print("child FAILED %s %s: %s" % (name, kern, e), flush=True)
            return 1
        print("child worst %s %s: %.3g of the bound" % (name, kern, worst), flush=True)
    return 0


def test_tile_order_knobs_in_child(gpu):
    """FDTD3D_TB_PATCH = 2x3 (the multi-row kernel's XCD run in 2 x 3 patches: 3 x 4 tiles at T = 5, so the last
    band and the last column are narrower) and FDTD3D_TB64_PATCH = 3x2, in ONE fresh child process."""
    g32 = V.tiles("mr16x2", 5, CASES["int-T5"].obox)
    g64 = V.tiles("f64half", 4, CASES["map-T4"].obox)
    assert g32[2] % 2 and g32[1] % 3 and g64[2] % 3 and g64[1] % 2, (g32, g64)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_tb_plain_gpu as P; sys.exit(P.child_main())" % (
        os.path.join(ROOT, "tests"), ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env={**os.environ, **CHILD_ENV}, capture_output=True,
                       text=True, timeout=240)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("child worst")]
    assert len(lines) == len(CHILD_RUNS), r.stdout[-2000:]


# ================================================ 9. refusals launch nothing
def test_refusals_launch_nothing(gpu):
    """Every refused call raises ``HipError`` before anything is launched (``ops.launches`` stands still, the
    outputs stay the sentinel); an empty output box is accepted and stores nothing; a valid call afterwards
    still meets the bound."""
    from fdtd3d_amd.ops.hip_lib import HipError
    name = "int-T3"
    cs, inp = CASES[name], inputs(name)
    whole = ((0, 0, 0), SIZE)
    for prec in ("f32", "f64"):
        dut = hip_pair(name, prec, gpu)
        ops, dt = dut.ops, V.DT[prec]
        V.set_knobs(ops, **KNOBS0)
        fin, fout, sent, keep, fill = device_state(name, gpu, dt)
        upd, cb, Z = inp["upd"], dut.cb, inp["Z"]
        src = lambda comp, cells: [(comp, c, Z) for c in cells]
        cell = torch.ones(SIZE, dtype=dt, device=gpu)
        cell[3:9, 20:50, 40:100] = 0.5
        bad = {
            "steps 0": lambda: ops.tb_step(fin, fout, upd, whole, cb, 0),
            "steps max + 1": lambda: ops.tb_step(fin, fout, upd, whole, cb, ops.tb_max_steps + 1),
            "shared buffer": lambda: ops.tb_step(fin, {**fout, "Hy": fin["Hy"]}, upd, whole, cb, 3),
            "update box outside": lambda: ops.tb_step(fin, fout, {**upd, "Ex": ((0, 1, 1), (SIZE[0] + 1, 72, 144))},
                                                      whole, cb, 3),
            "output box outside": lambda: ops.tb_step(fin, fout, upd, ((0, 0, 0), (14, 72, 148)), cb, 3),
            "source outside": lambda: ops.tb_step(fin, fout, upd, whole, cb, 3, src("Ez", [(SIZE[0], 0, 0)] * 3)),
            "source on H": lambda: ops.tb_step(fin, fout, upd, whole, cb, 3, src("Hx", [(7, 30, 60)] * 3)),
            "moving source": lambda: ops.tb_step(fin, fout, upd, whole, cb, 3,
                                                 src("Ez", [(7, 30, 60), (7, 30, 61), (7, 30, 60)])),
            "scalars differ": lambda: ops.tb_step(fin, fout, upd, whole,
                                                  {**cb, "Ey": Coef(scalar=cb["Ey"].scalar * 1.5)}, 3),
        }
        if prec == "f32":
            odd = {c: torch.zeros((6, 10, 10), dtype=dt, device=gpu) for c in V.COMPS}
            odd_out = {c: torch.zeros((6, 10, 10), dtype=dt, device=gpu) for c in V.COMPS}
            box = ((0, 0, 0), (6, 10, 10))
            bad["nz % 4"] = lambda: ops.tb_step(odd, odd_out, {c: box for c in V.COMPS}, box, cb, 2)
            bad["sparse per-cell, T = 6"] = lambda: ops.tb_step(
                fin, fout, upd, whole, {**cb, "Ex": Coef(scalar=cb["Ex"].scalar, cell=cell)}, 6)
        for what, call in bad.items():
            before = ops.launches
            with pytest.raises(HipError):
                call()
            assert ops.launches == before, (prec, what, "launched")
        ops.tb_step(fin, fout, upd, ((2, 3, 4), (2, 30, 40)), cb, 3)  # empty in x: accepted, nothing stored
        torch.cuda.synchronize()
        V.assert_unchanged(fin, keep, (name, prec, "refusals"))
        V.assert_unchanged(fout, fill, (name, prec, "a refused or empty pass stored something"))
        worst = run_check(name, "mr16x2" if prec == "f32" else "f64half", gpu, ("after refusals",))
        print("worst after refusals %s: %.3g of the bound" % (prec, worst))
