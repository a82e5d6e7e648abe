"""The physics variants of the blocked kernels, one launch at a time on live
state, against the fp64 torch oracle:

* the Drude pass ``ops.tb_drude_step`` (csrc/tb3d_mr.h DrDev, feature bit 16,
  both tile shapes; fp64: csrc/yee3d_tb64.hip fdtd_tb3d_drude_f64),
* the amplitude pass ``ops.tb_amp_step`` (tb3d_mr.h AmpDev, feature bit 8,
  ``tb_mr_shape`` 0 and 1),
* the incident-line kernel ``ops.tfsf_pass`` (csrc/yee3d_tb.hip k_tfsf_pass,
  fp32 and fp64) and the in-kernel TF/SF of ``ops.tb_step(tfsf=...)``
  (feature bit 4 alone and with sparse per-cell coefficients, features 5, 6
  and 7; fp64: fdtd_tb3d_tf_f64, both tile shapes),
* a sentinel check of the plain passes (multi-row, single-row, fp64).

Every test builds a HIP scheme and an fp64 torch / CPU scheme from one
``SchemeConfig``, fills all state with seeded random values drawn once in fp64
(E on the scale of the wave impedance, so that every term of an update
matters from the first level on), pre-fills every output with a sentinel
pattern, makes ONE op call per backend and compares everything the op writes:

* outside what the oracle writes the outputs are bit-identical to the sentinel;
* the inputs (fields, state, tables, coefficient arrays) are bit-unchanged;
* errors are taken per component against the maximum of the component's kind
  (E or H) in what the oracle wrote, as tests/test_drude_blk_gpu.py does.

Bounds (none is wider than the project's own for the same kernel family):
``BOUND32`` = 2e-5 for fp32 fields and state (test_tb_gpu.py,
test_drude_blk_gpu.py, test_tfsf_tb_gpu.py), ``BOUND64`` = 1e-11 for the fp64
Drude and TF/SF kernels (test_drude_blk_gpu.py, test_tfsf_tb_gpu.py); the
plain fp64 pass keeps test_tb_gpu.py's 1e-12.

Tile arithmetic (``tiles`` below; the launchers' grid formulas of
tb3d_mr.h launch_tb_mr, yee3d_tb.hip launch_tb and yee3d_tb64.hip
launch_tb64): a tile owns ``ROWS - 2T`` rows in y and ``LANES - 2T`` cells in
z (scalar lanes), and a workgroup ``tb_xchunk`` planes in x:

    family     ROWS  LANES   kernel
    mr16x2      32     64    fp32 multi-row, 16 waves x 2 rows (tb_mr_shape 0)
    mr8x4       32     64    fp32 multi-row, 8 waves x 4 rows (tb_mr_shape 1)
    drude32     16     64    fp32 Drude variant, both tb_dr_shape values
    f64half     32     32    fp64, two 32-lane rows per wave (tb64_half 1)
    f64full     16     64    fp64, one 64-lane row per wave (tb64_half 0)
    drude64     16     32    fp64 Drude variant (always 8 waves of two
                             32-lane rows: tb64_half does not reach it, the
                             parameter is kept so a later change of that
                             shows)

    gy = ceil((O.hi.y - O.lo.y) / (ROWS - 2T))
    gz = ceil((O.hi.z - O.lo.z) / (LANES - 2T))
    gx = ceil((O.hi.x - O.lo.x) / tb_xchunk)

(the fp32 single-row kernel of the plain sentinel test has 16-row tiles of V
wide lanes, V = 4 for T <= 2 and 2 above: ``(64 - 2 ceil(T / V)) V`` cells in
z from ``O.lo.z`` rounded down to V.)  Every case carries the tile counts it
claims -- the seams it exists for -- and every test asserts them with these
formulas; ``tb_xchunk`` is 5 throughout, so every case has x-chunk seams too.

The amplitude pass's 8 x 2 tile shape is chosen by an environment variable
the library reads once at load (FDTD3D_TB_AMP_SHAPE); it is left out here.

Amplitude thresholds: the fp32 kernel and the fp64 oracle may decide
differently in a cell whose growth sits at the threshold.  With the oracle's
per-level values a cell is ambiguous at level l when ``|v - a (1 + acc)|`` or
``|v - a|`` is at most ``eps`` = BOUND32 x the kind's scale x (2 + acc).
After an ambiguous level the cell may hold either value, so at the later
levels the test is made for every maximum ``a`` the cell may hold by then
(``amp_ambiguous`` carries their range), and the cell is also ambiguous at a
level where those maxima decide differently; a cell that was never ambiguous
is judged on the oracle's own ``a`` alone.  Cells ambiguous at no level must
match within the bound, ``counts[l]`` may differ by at most the number of
cells ambiguous at level l, a cell ambiguous at some level must still hold
its old value or one of its ``|f_l|``, and the cells ambiguous at any level
are capped at 0.5 % of the cells inside the amplitude boxes (asserted on the CPU for every
case by tests/test_tb_variants_cpu.py, which also shows that every case is
well conditioned in fp32 and live).
"""
import copy
import dataclasses
import functools
import math

import pytest
import torch

from fdtd3d_amd.models.scheme import ACCURACY, SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.coef import Coef
from fdtd3d_amd.ops.torch_ops import _empty, box_intersect_, box_slices

pytestmark = pytest.mark.gpu

BOUND32 = 2e-5       # fp32 fields and state, on the kind's scale
BOUND64 = 1e-11      # fp64 Drude and TF/SF kernels
BOUND64_PLAIN = 1e-12  # the plain fp64 pass (test_tb_gpu.py)
XCHUNK = 5           # x planes per workgroup: every case has at least two chunks
E, H = ("Ex", "Ey", "Ez"), ("Hx", "Hy", "Hz")
COMPS = E + H
DT = {"f32": torch.float32, "f64": torch.float64}

# family -> (ROWS, LANES): see the module docstring
GEOM = {"mr16x2": (32, 64), "mr8x4": (32, 64), "drude32": (16, 64), "f64half": (32, 32), "f64full": (16, 64),
        "drude64": (16, 32),
        "mr8x2": (16, 64)}  # fp32 multi-row, 8 waves x 2 rows (tb_mr_shape 2, T <= 5: tests/test_tb_plain_gpu.py)


def cdiv(a, b):
    return -(-a // b)


def tiles(family, T, obox, xchunk=XCHUNK):
    """(gx, gy, gz) of a launch over ``obox``: the module docstring's formulas."""
    ext = [obox[1][d] - obox[0][d] for d in range(3)]
    if family == "single":
        V = 4 if T <= 2 else 2
        tbz = (64 - 2 * cdiv(T, V)) * V
        return cdiv(ext[0], xchunk), cdiv(ext[1], 16 - 2 * T), cdiv(obox[1][2] - (obox[0][2] & ~(V - 1)), tbz)
    rows, lanes = GEOM[family]
    return cdiv(ext[0], xchunk), cdiv(ext[1], rows - 2 * T), cdiv(ext[2], lanes - 2 * T)


def seams(family, T, obox, xchunk=XCHUNK):
    """Interior tile / chunk boundaries of the launch along x, y, z."""
    if family == "single":
        # (16-row tiles of V wide lanes from ``O.lo.z`` rounded down to V: see ``tiles``)
        V = 4 if T <= 2 else 2
        step = (xchunk, 16 - 2 * T, (64 - 2 * cdiv(T, V)) * V)
        lo = (obox[0][0], obox[0][1], obox[0][2] & ~(V - 1))
        return [list(range(lo[d] + step[d], obox[1][d], step[d])) for d in range(3)]
    rows, lanes = GEOM[family]
    step = (xchunk, rows - 2 * T, lanes - 2 * T)
    return [list(range(obox[0][d] + step[d], obox[1][d], step[d])) for d in range(3)]


def assert_tiles(family, T, obox, claim):
    got = tiles(family, T, obox)
    assert all(g >= c for g, c in zip(got, claim)), (family, T, obox, "tiles", got, "claimed", claim)
    return got


# ------------------------------------------------------------------ schemes
_SCHEMES = {}


def scheme(cfg, backend, device, dtype):
    """One scheme per (config, backend, dtype), shared by the tests (they
    read its geometry, coefficients and tables and never step it)."""
    key = (repr(cfg), backend, str(device), dtype)
    s = _SCHEMES.get(key)
    if s is None:
        s = YeeScheme(cfg, make_ops(backend, None, device, dtype))
        s.init_scheme()
        s.init_grids()
        _SCHEMES[key] = s
    return s


def vacuum_cfg(size, prec, **extra):
    return SchemeConfig(scheme="3d", size=tuple(size), scene="vacuum", dtype=prec, use_fused=True, **extra)


def pair(cfg64, prec, device, backend):
    """(scheme under test, fp64 torch oracle scheme) of one config."""
    ref = scheme(cfg64, "torch", "cpu", torch.float64)
    dut = scheme(dataclasses.replace(cfg64, dtype=prec), backend, device, DT[prec])
    return dut, ref


def set_knobs(ops, **kw):
    """The blocked kernels' tuning knobs of a HIP backend (a torch backend
    stands in for it in the CPU companion and has none)."""
    if ops.name != "hip":
        return
    ops.tb_xchunk = XCHUNK
    for k, v in kw.items():
        setattr(ops, k, v)


# --------------------------------------------------------------- live state
def randn(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float64)


def rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(tuple(shape), generator=g, dtype=torch.float64)


def impedance(s):
    return math.sqrt(s.cb["Ex"].scalar / s.cb["Hx"].scalar)


def live_fields(size, seed, Z):
    """Random fields, non-zero everywhere: E ~ Z N(0, 1), H ~ N(0, 1), so
    Cb curl H is of the size of E and Db curl E of the size of H."""
    return {c: randn(size, seed + n) * (Z if c[0] == "E" else 1.0) for n, c in enumerate(COMPS)}


def sentinel(shape, salt):
    """A pattern no update produces (negative half integers around -600,
    exact in fp32), different in every cell of a row and from array to array."""
    idx = torch.arange(int(torch.tensor(shape).prod()), dtype=torch.int64).reshape(tuple(shape))
    return -(500.0 + ((idx * 7 + salt * 37) % 211).double() * 0.5)


def to_dev(t, device, dtype):
    return t.to(dtype).to(device).contiguous().clone()  # (never the cached fp64 draw itself)


def kind_scales(want, sent):
    """Maximum per kind over what the oracle wrote."""
    sc = {}
    for kind, names in (("E", E), ("H", H)):
        m = 0.0
        for c in names:
            w = want[c][want[c] != sent[c]]
            if w.numel():
                m = max(m, float(w.abs().max()))
        sc[kind] = m + 1e-300
    return sc


def check_written(got, want, sent, dtype, scale, bound, tag):
    """``got`` (from the backend under test, its dtype, on the CPU) against
    the oracle's ``want``: bit-identical to the sentinel wherever the oracle
    left it, within ``bound * scale`` elsewhere.  Returns error / scale."""
    mask = want != sent
    keep = ~mask
    assert torch.equal(got[keep], sent.to(dtype)[keep]), (tag, "stored outside what the pass writes",
                                                          int((got[keep] != sent.to(dtype)[keep]).sum()))
    if not bool(mask.any()):
        return 0.0
    diff = (got.double() - want)[mask].abs()
    err = float(diff.max())
    print("err %s %.3g of %.3g" % (tag, err / scale, bound))
    if not err <= bound * scale:
        at = torch.nonzero(((got.double() - want).abs() * mask) == err)[0].tolist()
        raise AssertionError((tag, "error", err, "scale", scale, "bound", bound * scale, "cell", at))
    return err / scale


def check_fields(got, want, sent, dtype, bound, tag):
    sc = kind_scales(want, sent)
    worst = 0.0
    for c in COMPS:
        worst = max(worst, check_written(got[c], want[c], sent[c], dtype, sc[c[0]], bound, tag + (c,)))
    return worst, sc


def run_pair_fields(fin64, size, device, dtype):
    """Device input fields, sentinel-filled outputs, and clones of the inputs."""
    fin = {c: to_dev(fin64[c], device, dtype) for c in COMPS}
    sent = {c: sentinel(size, n) for n, c in enumerate(COMPS)}
    fout = {c: to_dev(sent[c], device, dtype) for c in COMPS}
    keep = {c: fin[c].clone() for c in COMPS}
    return fin, fout, sent, keep


def assert_unchanged(now, before, tag):
    for k in before:
        assert torch.equal(now[k], before[k]), (tag, "input changed", k)


def grow(box, T, size):
    return (tuple(max(0, box[0][d] - T) for d in range(3)), tuple(min(size[d], box[1][d] + T) for d in range(3)))


# ===================================================================== Drude
DRUDE_SIZE = (16, 44, 84)
DRUDE_B = ((5, 7, 9), (11, 36, 74))  # strictly inside; grown by T = 1 it still spans 3 x 2 Drude tiles
DRUDE_CBD = 0.375                  # the D coefficient of the hand-built dicts (exact in fp32)
DRUDE_NID = 5                      # four dispersive rows per component and the plain row


@dataclasses.dataclass(frozen=True)
class DrudeCase:
    name: str
    T: int
    B: tuple        # the Drude box, local
    obox: object    # "serial": B grown by T and clipped; else the output box
    src: object     # None or (E component, cell)
    claim: tuple    # least (gx, gy, gz) of the fp32 launch (16-row tiles): the seams the case is for
    why: str
    size: tuple = DRUDE_SIZE
    plan: bool = False
    src_at: str = ""  # where the source sits: "inside" B off its faces, on a "face" cell of B, in the "halo"


# The E update boxes of the (16, 44, 84) grid meet in (1, 1, 1) .. (15, 43, 83): the corner boxes touch it.
# Owned rows / z cells of a Drude tile: T = 1: 14 / 62, 2: 12 / 60, 3: 10 / 58, 4: 8 / 56, 5: 6 / 54 (fp32).
DRUDE_CASES = [
    DrudeCase("in-T1", 1, DRUDE_B, "serial", ("Ez", (8, 20, 40)), (2, 3, 2),
              "B inside, obox 8 x 31 x 67: 3 y tiles of 14 rows, 2 z tiles of 62; source inside B", src_at="inside"),
    DrudeCase("in-T2", 2, DRUDE_B, "serial", ("Ex", (3, 20, 40)), (2, 3, 2),
              "obox 10 x 33 x 69: 3 x 2 tiles; source in the grown halo (x = 3, B starts at 5)", src_at="halo"),
    DrudeCase("in-T3", 3, DRUDE_B, "serial", ("Ey", (5, 20, 40)), (3, 4, 2),
              "obox 12 x 35 x 71: 4 x 2 tiles; source exactly on B's low x face", src_at="face"),
    DrudeCase("in-T4", 4, DRUDE_B, "serial", None, (3, 5, 2), "obox 14 x 37 x 73: 5 x 2 tiles; no source"),
    DrudeCase("in-T5", 5, DRUDE_B, "serial", ("Ex", (10, 35, 73)), (4, 7, 2),
              "obox 16 x 39 x 75: 7 x 2 tiles, T - 1 = 4 carried state levels; source in B's high corner cell", src_at="face"),
    DrudeCase("lo-T3", 3, ((1, 1, 1), (7, 20, 66)), "serial", None, (2, 3, 2),
              "B on the low corner of the E update boxes: B grown by 3 is clipped at x = y = z = 0"),
    DrudeCase("lo-T5", 5, ((1, 1, 1), (7, 20, 66)), "serial", ("Ez", (1, 1, 1)), (3, 5, 2),
              "the same at T = 5 (halo rows and lanes below the array), source in the corner cell of B", src_at="face"),
    DrudeCase("hi-T4", 4, ((9, 24, 20), (15, 43, 83)), "serial", None, (3, 3, 2),
              "B on the high corner: clipped at the three high faces, obox 11 x 24 x 68"),
    DrudeCase("hi-T1", 1, ((9, 10, 15), (15, 43, 83)), "serial", ("Ey", (14, 42, 82)), (2, 3, 2),
              "the same at T = 1: obox 7 x 35 x 70", src_at="face"),
    DrudeCase("thin-x", 3, ((8, 7, 9), (9, 36, 74)), "serial", None, (2, 4, 2), "B one plane thick in x"),
    DrudeCase("thin-y", 5, ((5, 20, 9), (11, 21, 74)), "serial", None, (4, 2, 2),
              "B one row thick in y: every Drude row is another tile's halo row at T = 5"),
    DrudeCase("thin-z", 4, ((5, 7, 40), (11, 36, 41)), "serial", ("Ez", (8, 20, 40)), (3, 5, 1),
              "B one cell thick in z (one z tile: 9 cells)", src_at="face"),
    DrudeCase("cut-x-T5", 5, DRUDE_B, ((0, 2, 4), (8, 41, 79)), ("Ez", (6, 20, 40)), (2, 7, 2),
              "decomposed form: obox cuts B in x (state written on x = 5 .. 7 only)", src_at="inside"),
    DrudeCase("cut-x-T1", 1, DRUDE_B, ((7, 6, 8), (16, 37, 75)), None, (2, 3, 2),
              "obox cuts B in x from the other side at T = 1"),
    DrudeCase("cut-y-T5", 5, DRUDE_B, ((0, 20, 4), (16, 41, 79)), ("Ey", (8, 36, 40)), (4, 4, 2),
              "obox cuts B in y; source on the row above B's high y face (halo)", src_at="halo"),
    DrudeCase("cut-z-T3", 3, DRUDE_B, ((2, 4, 30), (14, 39, 77)), ("Ex", (8, 20, 30)), (3, 4, 1),
              "obox cuts B in z at a z that is no multiple of 4; source on the cut", src_at="inside"),
    DrudeCase("cut-z-T4", 4, DRUDE_B, ((1, 3, 5), (15, 40, 70)), None, (3, 5, 2),
              "obox cuts B's high z end: 65 cells, 2 z tiles"),
    DrudeCase("plan-T3", 3, None, "serial", None, (3, 2, 1),
              "the dict of a real drude-sphere scheme's plan (box, ids, LUT, cbd) with the state randomised",
              size=(32, 40, 64), plan=True),
]
DRUDE = {c.name: c for c in DRUDE_CASES}
PLAN_EXTRA = dict(scene="drude-sphere", use_metamaterials=True, sphere_center=(16.0, 20.0, 32.0), sphere_radius=6.0,
                  blocked_drude="on", time_block=3)


def drude_cfg(cs):
    if cs.plan:
        return SchemeConfig(scheme="3d", size=cs.size, dtype="f64", **PLAN_EXTRA)
    return vacuum_cfg(cs.size, "f64")


def drude_upd(s):
    return {c: s.local_box(c, s.domain.allocated_global()) for c in COMPS}


@functools.lru_cache(None)
def drude_inputs(name):
    """Everything a Drude case reads, in fp64 on the CPU (drawn once)."""
    cs = DRUDE[name]
    seed = 1000 + 50 * DRUDE_CASES.index(cs)
    ref = scheme(drude_cfg(cs), "torch", "cpu", torch.float64)
    cb, Z = ref.cb["Ex"].scalar, impedance(ref)
    if cs.plan:
        db = ref.drude_blk
        assert db is not None and db["T"] == cs.T
        B, cbd, ids = db["box"], float(db["cbd"]), db["ids"].clone()
        lut = db["lut"].double().clone()  # (the fp64 plan's rows; a fp32 scheme's plan rounds them itself)
    else:
        B, cbd = cs.B, DRUDE_CBD
        bshape = tuple(B[1][d] - B[0][d] for d in range(3))
        # rows near physical values: b0 cbd in (0.3, 1) Cb, |b2 cbd| <= 0.3 Cb, m1 in (0.5, 1.5), |m2| <= 0.8
        u = rand((3, DRUDE_NID, 4), seed + 20)
        lut = torch.stack([cb * (0.3 + 0.7 * u[..., 0]), (cb / cbd) * 0.3 * (2 * u[..., 1] - 1), 0.5 + u[..., 2],
                           0.8 * (2 * u[..., 3] - 1)], -1)
        lut[:, DRUDE_NID - 1] = torch.tensor([cb, 0.0, 1.0, 0.0], dtype=torch.float64)
        lut = lut.float().double()
        # a different id per component in every cell, the plain row on a scattered ~15 % per component
        g = torch.Generator().manual_seed(seed + 21)
        r = [torch.randint(0, 4, bshape, generator=g), torch.randint(1, 4, bshape, generator=g),
             torch.randint(1, 4, bshape, generator=g)]
        idq = [r[0], (r[0] + r[1]) % 4, (r[0] + r[1] + r[2]) % 4]
        idq = [torch.where(rand(bshape, seed + 22 + q) < 0.15, torch.full_like(i, DRUDE_NID - 1), i)
               for q, i in enumerate(idq)]
        ids = (idq[0] | (idq[1] << 8) | (idq[2] << 16)).to(torch.int32)
    bshape = tuple(B[1][d] - B[0][d] for d in range(3))
    s0 = torch.zeros(bshape + (4,), dtype=torch.float64)
    s1 = torch.zeros(bshape + (4,), dtype=torch.float64)
    s0[..., :3] = 2.0 * cbd * randn(bshape + (3,), seed + 30)  # delta = cbd curl H
    s1[..., :3] = Z * randn(bshape + (3,), seed + 31)          # Ep
    obox = grow(B, cs.T, cs.size) if cs.obox == "serial" else cs.obox
    src = None
    if cs.src is not None:
        src = [(cs.src[0], cs.src[1], Z * (0.5 + 0.25 * l)) for l in range(cs.T)]
    return dict(B=B, cbd=cbd, ids=ids, lut=lut, s0=s0, s1=s1, obox=obox, src=src, Z=Z,
                fin=live_fields(cs.size, seed, Z), upd=drude_upd(ref))


def drude_run(name, dut, device, dtype, mutate=None, own=None):
    """One ``tb_drude_step`` of case ``name`` on the backend of scheme
    ``dut``; returns what it wrote (on the CPU) and the sentinels.  ``mutate``
    (CPU companion): a deliberate error in what the op is handed.  ``own``:
    (ids, lut) of the backend's own plan instead of the oracle's."""
    cs, inp = DRUDE[name], drude_inputs(name)
    hip = dut.ops.name == "hip"
    B, ids, lut = inp["B"], inp["ids"], inp["lut"]
    if own is not None:
        ids, lut = own
    if mutate == "shift-B":
        # (one cell along x, towards the side with room inside the E update boxes)
        sh = 1 if B[1][0] + 1 <= cs.size[0] - 1 else -1
        B = ((B[0][0] + sh,) + tuple(B[0][1:]), (B[1][0] + sh,) + tuple(B[1][1:]))
    elif mutate == "swap-ids":
        ids = ((ids & 0xff) << 8) | ((ids >> 8) & 0xff) | (ids & 0xff0000)
    elif mutate == "no-m2":
        lut = lut.clone()
        lut[..., 3] = 0.0
    fin, fout, sent, keep = run_pair_fields(inp["fin"], cs.size, device, dtype)
    sin = [to_dev(inp["s0"], device, dtype), to_dev(inp["s1"], device, dtype)]
    ids_d = ids.to(device)
    if hip:
        # the kernels' material ids: .w of the first state array, exactly as models/blocking.py _drude_ids_in
        if dtype == torch.float32:
            sin[0][..., 3] = ids_d.view(torch.float32)
        else:
            sin[0][..., 3] = (ids_d.to(torch.int64) & 0xFFFFFFFF).view(torch.float64)
    ssent = [sentinel(tuple(inp["s0"].shape), 11), sentinel(tuple(inp["s0"].shape), 12)]
    sout = [to_dev(ssent[0], device, dtype), to_dev(ssent[1], device, dtype)]
    lut_d = to_dev(lut, device, dtype)
    keep.update(s0=sin[0].clone(), s1=sin[1].clone(), lut=lut_d.clone())
    dut.ops.tb_drude_step(fin, fout, inp["upd"], inp["obox"], dut.cb, cs.T, inp["src"],
                          {"box": B, "sin": sin, "sout": sout, "lut": lut_d, "cbd": inp["cbd"], "ids": ids_d})
    if hip:
        torch.cuda.synchronize()
    assert_unchanged(dict(fin, s0=sin[0], s1=sin[1], lut=lut_d), keep, name)
    return dict(fout={c: fout[c].cpu() for c in COMPS}, sout=[t.cpu() for t in sout], sent=sent, ssent=ssent,
                obox=inp["obox"], B=B)


@functools.lru_cache(None)
def drude_oracle(name, mutate=None):
    ref = scheme(drude_cfg(DRUDE[name]), "torch", "cpu", torch.float64)
    return drude_run(name, ref, "cpu", torch.float64, mutate)


def drude_check(name, out, dtype, bound, id_bits, ids=None):
    """``out`` of a backend against the oracle's; ``id_bits``: the backend
    keeps the ids (``ids``, default the oracle's) in .w of the state (the
    HIP kernels)."""
    cs, inp, want = DRUDE[name], drude_inputs(name), drude_oracle(name)
    worst, sc = check_fields(out["fout"], want["fout"], want["sent"], dtype, bound, (name,))
    ob = box_intersect_(inp["B"], inp["obox"])
    assert not _empty(ob)
    B = inp["B"]
    sl = tuple(slice(ob[0][d] - B[0][d], ob[1][d] - B[0][d]) for d in range(3))
    inside = torch.zeros(tuple(inp["s0"].shape[:3]), dtype=torch.bool)
    inside[sl] = True
    # delta is cbd curl H (scale: cbd / Cb of the E scale), Ep an E field
    sscale = (sc["E"] * inp["cbd"] / scheme(drude_cfg(cs), "torch", "cpu", torch.float64).cb["Ex"].scalar, sc["E"])
    for n in range(2):
        got, w, snt = out["sout"][n], want["sout"][n], want["ssent"][n]
        assert torch.equal(got[~inside], snt.to(dtype)[~inside]), (name, "state %d stored outside obox and B" % n)
        d = (got[..., :3].double() - w[..., :3])[inside].abs()
        err = float(d.max())
        print("err %s state %d %.3g of %.3g" % (name, n, err / sscale[n], bound))
        assert err <= bound * sscale[n], (name, "state", n, err, sscale[n])
        worst = max(worst, err / sscale[n])
    if id_bits:
        w0 = out["sout"][0][..., 3].contiguous()
        bits = w0.view(torch.int32) if dtype == torch.float32 else (w0.view(torch.int64) & 0xFFFFFFFF).to(torch.int32)
        hi = torch.zeros_like(bits) if dtype == torch.float32 else (w0.view(torch.int64) >> 32).to(torch.int32)
        ids = inp["ids"] if ids is None else ids
        assert torch.equal(bits[inside], ids[inside]) and not bool(hi[inside].any()), (name, "id bits")
        w1 = out["sout"][1][..., 3].contiguous()
        assert not bool((w1.view(torch.int32 if dtype == torch.float32 else torch.int64)[inside] != 0).any()), \
            (name, "Ep.w not zero")
    return worst


def drude_claims(name):
    cs, inp = DRUDE[name], drude_inputs(name)
    got32 = assert_tiles("drude32", cs.T, inp["obox"], cs.claim)
    got64 = assert_tiles("drude64", cs.T, inp["obox"], cs.claim)  # (half as many z lanes: never fewer tiles)
    return got32, got64


@pytest.mark.parametrize("prec,shape", [("f32", 0), ("f32", 1), ("f64", 1), ("f64", 0)])
@pytest.mark.parametrize("name", list(DRUDE))
def test_drude_pass(gpu, name, prec, shape):
    """One Drude launch from live fields and state: fp32 with both tile
    shapes (``tb_dr_shape``), fp64 with both ``tb64_half`` values."""
    cs = DRUDE[name]
    drude_claims(name)
    dut, ref = pair(drude_cfg(cs), prec, gpu, "hip")
    if prec == "f32":
        set_knobs(dut.ops, tb_dr_shape=shape)
    else:
        set_knobs(dut.ops, tb64_half=shape)
    own = None
    if cs.plan:
        # the HIP scheme's own plan (its ids and table: the rows may be numbered differently) gives every
        # cell the coefficient tuple of the oracle's plan: the hand-built form is what the planner produces
        inp, db = drude_inputs(name), dut.drude_blk
        assert db is not None and db["box"] == inp["B"] and db["T"] == cs.T
        assert abs(db["cbd"] - inp["cbd"]) <= 1e-6 * inp["cbd"]
        own = (db["ids"].cpu(), db["lut"].double().cpu())
        for q in range(3):
            mine = own[1][q][((own[0] >> (8 * q)) & 0xff).long()]
            ref_ = inp["lut"][q][((inp["ids"] >> (8 * q)) & 0xff).long()]
            assert float(((mine - ref_).abs() / (ref_.abs() + 1e-30)).max()) <= 1e-6, (name, q, "plans differ")
    out = drude_run(name, dut, gpu, DT[prec], own=own)
    worst = drude_check(name, out, DT[prec], BOUND32 if prec == "f32" else BOUND64, id_bits=True,
                        ids=None if own is None else own[0])
    print("worst drude %s %s shape %d: %.3g of the bound" % (name, prec, shape,
                                                            worst / (BOUND32 if prec == "f32" else BOUND64)))


# ================================================================= amplitude
AMP_SIZE = (12, 64, 68)
WHOLE = ((0, 0, 0), AMP_SIZE)
# The amplitude boxes keep off the grid's faces (the computation box minus an absorbing layer, as in a run):
# a face cell outside its component's update box never changes, so from level 1 on |f| EQUALS its maximum
# and the cell would count as ambiguous although nothing about it is.
INNER = ((1, 1, 1), (11, 63, 67))
NOBOX = ((0, 0, 0), (0, 0, 0))


@dataclasses.dataclass(frozen=True)
class AmpCase:
    name: str
    T: int
    obox: tuple
    aboxes: tuple   # Ex .. Hz
    line: object    # None or (E component, i, j, k0, k1)
    acc: float
    claim: tuple    # least (gx, gy, gz): 32-row tiles own 32 - 2T rows, 64 - 2T cells in z
    why: str
    line_is: tuple = ()  # "seam": spans a z tile seam; "cell": one cell long; "outside": ends outside its update box


# z seams of the whole-grid launches: T = 1: z = 62, T = 2: 60, T = 3: 58; y seams at 30 / 28 / 26 and twice that.
# The Ez update box ends at z = 67: a line reaching z = 68 has its last cell outside it.
AMP_SUB = ((2, 3, 4), (11, 64, 68))   # sub-box: seams at y = 3 + k (32 - 2T), z = 4 + 64 - 2T
AMP_CASES = [
    AmpCase("whole-T1", 1, WHOLE,
            (((1, 2, 3), (11, 60, 66)), INNER, ((2, 5, 1), (9, 33, 64)), NOBOX,
             ((3, 29, 60), (8, 32, 64)), ((1, 10, 1), (11, 50, 67))),
            ("Ez", 6, 30, 55, 67), ACCURACY, (3, 3, 2),
            "whole grid, 3 x 2 tiles; Hx box empty; the line spans the z seam at 62 on the y seam row 30", line_is=('seam',)),
    AmpCase("whole-T2", 2, WHOLE,
            (((1, 2, 3), (11, 60, 66)), NOBOX, ((2, 5, 1), (9, 33, 64)), INNER,
             ((3, 27, 58), (8, 30, 62)), ((1, 10, 1), (11, 50, 67))),
            ("Ex", 5, 28, 60, 61), 0.05, (3, 3, 2),
            "coarse accuracy; Ey box empty; a one-cell line on the first cell past the z seam (60), y seam row 28", line_is=('cell',)),
    AmpCase("whole-T3", 3, WHOLE,
            (((1, 2, 3), (11, 60, 66)), INNER, ((2, 5, 1), (9, 33, 64)), ((4, 25, 57), (6, 27, 59)),
             NOBOX, ((1, 10, 1), (11, 50, 67))),
            ("Ez", 4, 26, 50, 66), ACCURACY, (3, 3, 2),
            "T - 1 = 2 LDS hand-off levels; a 2 x 2 x 2 Hx box on the y / z seam corner; line across the seam at 58", line_is=('seam',)),
    AmpCase("whole-T3-coarse", 3, WHOLE,
            (INNER, ((1, 2, 3), (11, 60, 66)), INNER, INNER,
             INNER, INNER),
            None, 0.05, (3, 3, 2), "no line source, coarse accuracy, (nearly) every cell in a box"),
    AmpCase("sub-T3", 3, AMP_SUB,
            (((3, 10, 12), (9, 40, 60)), ((1, 1, 1), (8, 30, 67)), NOBOX, ((5, 20, 30), (11, 63, 67)),
             ((2, 3, 4), (11, 63, 67)), ((1, 2, 3), (11, 63, 67))),
            ("Ez", 6, 29, 60, 68), ACCURACY, (2, 3, 2),
            "sub-box output; Ex box inside it, Ey / Hz boxes sticking out, Ez box empty; the line ends on "
            "z = 67, outside the Ez update box, and spans the z seam at 62 on the y seam row 29", line_is=('seam', 'outside')),
    AmpCase("sub-T2", 2, AMP_SUB,
            (((3, 10, 12), (9, 40, 60)), ((1, 1, 1), (8, 30, 67)), ((4, 3, 60), (7, 63, 67)), NOBOX,
             ((2, 3, 4), (11, 63, 67)), ((1, 2, 3), (11, 63, 67))),
            ("Ey", 7, 31, 62, 68), 0.05, (2, 3, 2),
            "coarse accuracy on the sub-box; the line on the y seam row 31 (3 + 28) across the z seam at 64", line_is=('seam',)),
    AmpCase("sub-T1", 1, AMP_SUB,
            (((3, 10, 12), (9, 40, 60)), NOBOX, ((4, 3, 60), (7, 63, 67)), ((5, 20, 30), (11, 63, 67)),
             ((2, 3, 4), (11, 63, 67)), ((1, 2, 3), (11, 63, 67))),
            None, ACCURACY, (2, 3, 2), "T = 1: no hand-off level at all (level 0 reads and writes memory)"),
]
AMP = {c.name: c for c in AMP_CASES}
AMP_COUNTS0 = (7, 11, 13)  # the kernel adds to the counters


def amp_cfg():
    return vacuum_cfg(AMP_SIZE, "f64")


@functools.lru_cache(None)
def amp_inputs(name):
    cs = AMP[name]
    seed = 5000 + 50 * AMP_CASES.index(cs)
    ref = scheme(amp_cfg(), "torch", "cpu", torch.float64)
    Z = impedance(ref)
    # running maxima on the fields' scale: 20 % exact zeros, 15 % far above any |f|, the rest around |f|
    amp = torch.zeros((AMP_SIZE[0], 6) + AMP_SIZE[1:], dtype=torch.float64)
    for n, c in enumerate(COMPS):
        s = (Z if c[0] == "E" else 1.0) * 3.0
        a = randn(AMP_SIZE, seed + 10 + n).abs() * s
        u = rand(AMP_SIZE, seed + 20 + n)
        a = torch.where(u < 0.20, torch.zeros_like(a), a)
        a = torch.where(u > 0.85, a * 1e3 + 1e3 * s, a)
        amp[:, n] = a.float().double()  # (exact in fp32: both backends compare with the same maximum)
    vals = [Z * (0.75 + 0.5 * l) for l in range(cs.T)]
    return dict(fin=live_fields(AMP_SIZE, seed, Z), amp=amp, vals=vals, upd=drude_upd(ref), Z=Z)


def amp_run(name, dut, device, dtype, shape=0, shift_abox=False, record=None):
    cs, inp = AMP[name], amp_inputs(name)
    hip = dut.ops.name == "hip"
    set_knobs(dut.ops, tb_mr_shape=shape)
    fin, fout, sent, keep = run_pair_fields(inp["fin"], AMP_SIZE, device, dtype)
    buf = to_dev(inp["amp"], device, dtype)  # one [x][6][y][z] allocation
    amps = [buf[:, n] for n in range(6)]
    counts = torch.tensor(AMP_COUNTS0[:cs.T], dtype=torch.int32, device=device)
    aboxes = list(cs.aboxes)
    if shift_abox:
        aboxes = [b if _empty(b) else ((b[0][0], b[0][1] + 1, b[0][2]), (b[1][0], min(AMP_SIZE[1], b[1][1] + 1), b[1][2]))
                  for b in aboxes]
    ops = dut.ops
    if record is not None:
        ops = copy.copy(dut.ops)
        inner = dut.ops.amplitude_update

        def rec(f, a, box, accuracy):
            record.append((f.abs().clone(), a.clone()))
            return inner(f, a, box, accuracy)
        ops.amplitude_update = rec
    ops.tb_amp_step(fin, fout, inp["upd"], cs.obox, dut.cb, cs.T, cs.line, inp["vals"], amps, aboxes, cs.acc, counts)
    if hip:
        torch.cuda.synchronize()
        dut.ops.tb_mr_shape = 0
    assert_unchanged(fin, keep, name)
    return dict(fout={c: fout[c].cpu() for c in COMPS}, amp=buf.cpu(), counts=counts.cpu(), sent=sent)


@functools.lru_cache(None)
def amp_oracle(name, shift_abox=False):
    """The oracle's result and, per level and component, |f_l| and the
    maximum it was compared with (over obox ∩ the component's box)."""
    cs = AMP[name]
    ref = scheme(amp_cfg(), "torch", "cpu", torch.float64)
    record = []
    out = amp_run(name, ref, "cpu", torch.float64, shift_abox=shift_abox, record=record)
    calls = [(l, n) for l in range(cs.T) for n in range(6) if not _empty(box_intersect_(cs.aboxes[n], cs.obox))]
    assert shift_abox or len(calls) == len(record)
    if not shift_abox:
        out["levels"] = {ln: rc for ln, rc in zip(calls, record)}
    return out


def _amp_decides(v, a, acc):
    """The reference's test (TorchOps.amplitude_update): |f| replaces the maximum."""
    den = torch.where(a != 0, a, torch.where(v != 0, v, torch.ones_like(v)))
    return (v >= a) & ((v - a) / den > acc)


@functools.lru_cache(None)
def amp_ambiguous(name):
    """Per level: bool arrays (6, nx, ny, nz) of the cells ambiguous at that
    level (module docstring); the cells ambiguous at any level; the cells
    inside the boxes; every cell's candidate values (old, |f_0|, ...)."""
    cs, want = AMP[name], amp_oracle(name)
    sc = kind_scales(want["fout"], want["sent"])
    amb = torch.zeros((cs.T, 6) + AMP_SIZE, dtype=torch.bool)
    inbox = torch.zeros((6,) + AMP_SIZE, dtype=torch.bool)
    cand = [[amp_inputs(name)["amp"][:, n]] for n in range(6)]
    for n in range(6):
        b = box_intersect_(cs.aboxes[n], cs.obox)
        if _empty(b):
            continue
        sl = box_slices(b)
        inbox[n][sl] = True
        eps = BOUND32 * sc[COMPS[n][0]] * (2.0 + cs.acc)
        near = lambda v, a: ((v - a * (1.0 + cs.acc)).abs() <= eps) | ((v - a).abs() <= eps)
        # the range of maxima the cell may hold: one value until a level is ambiguous
        lo = hi = amp_inputs(name)["amp"][:, n][sl]
        for l in range(cs.T):
            v, a = want["levels"][(l, n)]
            assert bool(((lo <= a) & (a <= hi)).all())
            dlo, dhi = _amp_decides(v, lo, cs.acc), _amp_decides(v, hi, cs.acc)
            doubt = near(v, lo) | near(v, hi) | (dlo != dhi)
            amb[l, n][sl] = doubt
            lo, hi = (torch.where(doubt, torch.minimum(v, lo), torch.where(dlo, v, lo)),
                      torch.where(doubt, torch.maximum(v, hi), torch.where(dhi, v, hi)))
            full = torch.full(AMP_SIZE, float("inf"), dtype=torch.float64)
            full[sl] = v
            cand[n].append(full)
    return amb, amb.any(0), inbox, cand


def amp_check(name, out, dtype, bound):
    cs, want = AMP[name], amp_oracle(name)
    worst, sc = check_fields(out["fout"], want["fout"], want["sent"], dtype, bound, (name,))
    amb, ever, inbox, cand = amp_ambiguous(name)
    a0 = amp_inputs(name)["amp"]
    for n, c in enumerate(COMPS):
        got, w = out["amp"][:, n], want["amp"][:, n]
        scale = sc[c[0]]
        # outside obox ∩ abox the maxima are untouched, bit for bit
        assert torch.equal(got[~inbox[n]], a0[:, n].to(dtype)[~inbox[n]]), (name, c, "maxima stored outside the box")
        clear = inbox[n] & ~ever[n]
        if bool(clear.any()):
            err = float((got.double() - w)[clear].abs().max())
            print("err %s amp %s %.3g of %.3g" % (name, c, err / scale, bound))
            assert err <= bound * scale, (name, c, "amplitude", err, scale)
            worst = max(worst, err / scale)
        doubt = inbox[n] & ever[n]
        if bool(doubt.any()):
            g = got.double()[doubt]
            near = torch.stack([(g - k[doubt]).abs() for k in cand[n]]).min(0).values
            assert float(near.max()) <= bound * scale, (name, c, "ambiguous cell holds none of its values")
    for l in range(cs.T):
        slack = int(amb[l].sum())
        d = abs(int(out["counts"][l]) - int(want["counts"][l]))
        print("counts %s level %d: %d vs %d (ambiguous %d)" % (name, l, int(out["counts"][l]),
                                                              int(want["counts"][l]), slack))
        assert d <= slack, (name, "counts", l, int(out["counts"][l]), int(want["counts"][l]), slack)
    return worst


@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("name", list(AMP))
def test_amp_pass(gpu, name, shape):
    """One amplitude launch from live fields and maxima: 16 waves x 2 rows
    and 8 waves x 4 rows."""
    cs = AMP[name]
    assert_tiles("mr16x2" if shape == 0 else "mr8x4", cs.T, cs.obox, cs.claim)
    dut, ref = pair(amp_cfg(), "f32", gpu, "hip")
    out = amp_run(name, dut, gpu, torch.float32, shape=shape)
    worst = amp_check(name, out, torch.float32, BOUND32)
    print("worst amp %s shape %d: %.3g of the bound" % (name, shape, worst / BOUND32))


# ==================================================================== TF/SF
TF_SIZE = (24, 64, 72)
TF_BASE = dict(use_tfsf=True, tfsf_size=(5, 6, 7))
TF_INC = {"x": {}, "y": dict(phi=90.0, psi=30.0)}  # incidence along x and along y (tests/test_tfsf_tb_gpu.py)
TF_WHOLE = ((0, 0, 0), TF_SIZE)


def tf_cfg(inc):
    return vacuum_cfg(TF_SIZE, "f64", **TF_BASE, **TF_INC[inc])


@functools.lru_cache(None)
def tf_lines(inc, reach):
    """Random incident lines (E on the impedance scale); ``reach`` > 0: zero
    beyond it, so every cell a level reads lies inside what a dry pass copies."""
    ref = scheme(tf_cfg(inc), "torch", "cpu", torch.float64)
    Z = math.sqrt(ref.inc_ce / ref.inc_ch)
    e, h = Z * randn((ref.inc_len,), 9000 + len(inc)), randn((ref.inc_len,), 9001 + len(inc))
    if reach > 0:
        e[reach + 1:] = 0.0
        h[reach + 1:] = 0.0
    return e, h, Z


def tf_short_reach(inc):
    """The shortest reach whose dry copy (reach + 1 cells) holds every i0 + 1."""
    ref = scheme(tf_cfg(inc), "torch", "cpu", torch.float64)
    return int(ref.tfsf_sets.i0.max()) + 2


def tf_pass_run(inc, T, dry, short, dut, device, dtype):
    """One ``tfsf_pass``; returns (g table levels x ld, E line, H line) on
    the CPU, and the raw return value (the ``g`` of ``tb_step``)."""
    sets = dut.tfsf_sets
    assert sets is not None
    reach = tf_short_reach(inc) if short else dut.inc_len + 3
    e64, h64, Z = tf_lines(inc, reach if short else 0)
    e, h = to_dev(e64, device, dtype), to_dev(h64, device, dtype)
    keep = (e.clone(), h.clone())
    vals = [Z * (0.3 + 0.2 * l) for l in range(T)]
    sets.__dict__.pop("scratch_lines", None)  # (a dry pass's scratch lines: zero beyond the reach, as at a run's start)
    tabs = {k: getattr(sets, k).clone() for k in ("i0", "w0", "w1", "c", "dev")}
    g = dut.ops.tfsf_pass(e, h, dut.inc_ce, dut.inc_ch, vals, reach, sets, slot=0, dry=dry)
    if dut.ops.name == "hip":
        torch.cuda.synchronize()
    assert_unchanged({k: getattr(sets, k) for k in tabs}, tabs, (inc, T, dry, short))
    if dry:
        assert torch.equal(e, keep[0]) and torch.equal(h, keep[1]), "a dry pass moved the real line"
    return g[:T * sets.ld].cpu().clone().reshape(T, sets.ld), e.cpu(), h.cpu(), g


@functools.lru_cache(None)
def tf_pass_oracle(inc, T, dry, short):
    ref = scheme(tf_cfg(inc), "torch", "cpu", torch.float64)
    return tf_pass_run(inc, T, dry, short, ref, "cpu", torch.float64)[:3]


def tf_pass_check(inc, T, dry, short, got, bound):
    want = tf_pass_oracle(inc, T, dry, short)
    ref = scheme(tf_cfg(inc), "torch", "cpu", torch.float64)
    ne = ref.tfsf_sets.n_e
    worst = 0.0
    for l in range(T):
        # the E sets' values come from the H line, the H sets' from the E line: one scale each
        for part, sl in (("E", slice(0, ne)), ("H", slice(ne, None))):
            w = want[0][l, sl]
            scale = float(w.abs().max()) + 1e-300
            err = float((got[0][l, sl].double() - w).abs().max())
            assert err <= bound * scale, (inc, T, dry, short, "g level", l, part, err, scale)
            worst = max(worst, err / scale)
    for n, nm in ((1, "E line"), (2, "H line")):
        scale = float(want[n].abs().max()) + 1e-300
        err = float((got[n].double() - want[n]).abs().max())
        assert err <= bound * scale, (inc, T, dry, short, nm, err, scale)
        worst = max(worst, err / scale)
    print("worst tfsf_pass %s T %d dry %s short %s: %.3g of the bound" % (inc, T, dry, short, worst / bound))
    return worst


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("inc", list(TF_INC))
def test_tfsf_pass(gpu, inc, T, prec):
    """k_tfsf_pass from a live line: the g table level by level and both
    lines, moving the line and dry, with a reach past the line's end and one
    just long enough for the sets."""
    dut, ref = pair(tf_cfg(inc), prec, gpu, "hip")
    assert tf_short_reach(inc) < ref.inc_len
    for dry in (False, True):
        for short in (False, True):
            got = tf_pass_run(inc, T, dry, short, dut, gpu, DT[prec])
            tf_pass_check(inc, T, dry, short, got, BOUND32 if prec == "f32" else BOUND64)


@dataclasses.dataclass(frozen=True)
class TfCase:
    name: str
    inc: str
    T: int
    level0: int
    obox: tuple
    sparse: str     # "", "E", "H" or "EH": sparse per-cell coefficients (fp32: features 5, 6, 7)
    claim: tuple    # least (gx, gy, gz) of the fp32 launch (32-row tiles)
    why: str


# The TF box's faces (x = 4 / 5 and 18 / 19, y = 5 / 6 and 57 / 58, z = 6 / 7 and 64 / 65) are planes through
# the whole box: with at least two tiles per axis every y seam, z seam and x-chunk seam (x = 5, 10, 15, 20)
# cuts a face (``tf_straddles`` asserts it per case).  fp32: 32 - 2T rows, 64 - 2T cells in z per tile.
TF_SUBBOX = ((3, 10, 4), (24, 64, 40))  # cuts the low x face region's y range and both z-face planes' extent
TF_SPARSE_BOX = ((8, 20, 20), (16, 47, 62))  # inside the TF box, clear of every target cell, across y / z seams
TF_CASES = [
    TfCase("x-T1", "x", 1, 0, TF_WHOLE, "", (5, 3, 2), "3 x 2 tiles of 30 rows x 62 cells"),
    TfCase("x-T2-l3", "x", 2, 3, TF_WHOLE, "", (5, 3, 2), "table offset: levels 3, 4 of a 5-level table"),
    TfCase("x-T3-sub", "x", 3, 0, TF_SUBBOX, "", (5, 3, 1), "sub-box output that cuts through the faces"),
    TfCase("x-T4", "x", 4, 0, TF_WHOLE, "", (5, 3, 2), "3 x 2 tiles of 24 rows x 56 cells"),
    TfCase("x-T5-l3", "x", 5, 3, TF_WHOLE, "", (5, 3, 2), "the last 5 levels of an 8-level table"),
    TfCase("y-T1-l2", "y", 1, 2, TF_WHOLE, "", (5, 3, 2), "incidence along y (16 sets), level 2 of 3"),
    TfCase("y-T2", "y", 2, 0, TF_WHOLE, "", (5, 3, 2), "incidence along y"),
    TfCase("y-T3", "y", 3, 0, TF_WHOLE, "", (5, 3, 2), "incidence along y"),
    TfCase("y-T4-sub-l1", "y", 4, 1, TF_SUBBOX, "", (5, 3, 1), "sub-box and table offset together"),
    TfCase("y-T5", "y", 5, 0, TF_WHOLE, "", (5, 3, 2), "incidence along y, 3 x 2 tiles of 22 rows x 54 cells"),
    TfCase("x-T3-E", "x", 3, 0, TF_WHOLE, "E", (5, 3, 2), "feature 5: TF/SF + sparse per-cell E coefficients"),
    TfCase("y-T5-H", "y", 5, 0, TF_WHOLE, "H", (5, 3, 2), "feature 6: TF/SF + sparse per-cell H coefficients"),
    TfCase("y-T2-EH", "y", 2, 1, TF_WHOLE, "EH", (5, 3, 2), "feature 7: both kinds, with a table offset"),
    TfCase("x-T5-EH-sub", "x", 5, 0, TF_SUBBOX, "EH", (5, 3, 1), "feature 7 at T = 5 on the sub-box"),
]
TF = {c.name: c for c in TF_CASES}


def tf_straddles(cs, family):
    """Some set's box is cut by a y seam, some by a z seam, some by an
    x-chunk seam of the launch (inside the output box)."""
    ref = scheme(tf_cfg(cs.inc), "torch", "cpu", torch.float64)
    sm = seams(family, cs.T, cs.obox)
    cut = [False, False, False]
    for s in ref.tfsf_sets.sets:
        b = box_intersect_((s["lo"], s["hi"]), cs.obox)
        if _empty(b):
            continue
        for d in range(3):
            cut[d] |= any(b[0][d] < q < b[1][d] for q in sm[d])
    return cut


def tf_sparse_cb(cs, dut, device, dtype):
    """``cb`` with sparse per-cell coefficients of the asked kinds: Ex, Ez /
    Hy, Hz vary inside TF_SPARSE_BOX (one component per kind stays scalar)."""
    cb = dict(dut.cb)
    sl = box_slices(TF_SPARSE_BOX)
    for n, c in enumerate(("Ex", "Ez", "Hy", "Hz")):
        if c[0] not in cs.sparse:
            continue
        cell = torch.ones(TF_SIZE, dtype=torch.float64)
        cell[sl] = 0.3 + 0.7 * rand(cell[sl].shape, 9100 + n)
        cb[c] = Coef(scalar=dut.cb[c].scalar, cell=cell.float().to(dtype).to(device))
    return cb


def tf_step_run(name, dut, device, dtype, level_shift=0, drop_set=False, scalar_cb=False):
    cs = TF[name]
    sets = dut.tfsf_sets
    levels = cs.T + cs.level0 + (1 if cs.level0 + cs.T < 8 else 0)  # (one more level: the off-by-one probe)
    g = tf_pass_run(cs.inc, levels, True, False, dut, device, dtype)[3]
    seed = 9500 + 50 * TF_CASES.index(cs)
    fin64 = live_fields(TF_SIZE, seed, impedance(dut))
    fin, fout, sent, keep = run_pair_fields(fin64, TF_SIZE, device, dtype)
    cb = dict(dut.cb) if scalar_cb else tf_sparse_cb(cs, dut, device, dtype)
    cells = {c: cb[c].cell.clone() for c in cb if cb[c].cell is not None}
    upd = drude_upd(dut)
    if drop_set:
        sets = copy.copy(sets)
        tables = {c: list(v) for c, v in sets.tables.items()}
        victim = next(c for c in COMPS if any(t.n for t in tables[c]))
        tables[victim] = []
        sets.tables = tables
    gk = g.clone() if dut.ops.name == "hip" else None
    dut.ops.tb_step(fin, fout, upd, cs.obox, cb, cs.T, None, tfsf=(sets, g, cs.level0 + level_shift))
    if dut.ops.name == "hip":
        torch.cuda.synchronize()
        assert torch.equal(g, gk), (name, "g table changed")
    assert_unchanged(fin, keep, name)
    assert_unchanged({c: cb[c].cell for c in cells}, cells, name)
    return dict(fout={c: fout[c].cpu() for c in COMPS}, sent=sent)


@functools.lru_cache(None)
def tf_step_oracle(name, level_shift=0, drop_set=False, scalar_cb=False):
    ref = scheme(tf_cfg(TF[name].inc), "torch", "cpu", torch.float64)
    return tf_step_run(name, ref, "cpu", torch.float64, level_shift, drop_set, scalar_cb)


TF_STEP_PARAMS = ([(c.name, "f32", 0) for c in TF_CASES]
                  + [(c.name, "f64", half) for c in TF_CASES if not c.sparse for half in (1, 0)])


@pytest.mark.parametrize("name,prec,half", TF_STEP_PARAMS)
def test_tfsf_step(gpu, name, prec, half):
    """One blocked pass with in-kernel TF/SF from live fields and a live
    incident line (the g table of a dry ``tfsf_pass``), against the stepped
    table arithmetic of the oracle's ``_tfsf_level``."""
    cs = TF[name]
    family = "mr16x2" if prec == "f32" else ("f64half" if half else "f64full")
    claim = cs.claim if family != "f64full" else (cs.claim[0], cs.claim[1], 1)
    assert_tiles(family, cs.T, cs.obox, claim)
    cut = tf_straddles(cs, family)
    assert cut[0] and cut[1] and (cut[2] or claim[2] == 1), (name, family, "TF/SF faces miss a seam", cut)
    dut, ref = pair(tf_cfg(cs.inc), prec, gpu, "hip")
    set_knobs(dut.ops, tb64_half=half)
    out = tf_step_run(name, dut, gpu, DT[prec])
    bound = BOUND32 if prec == "f32" else BOUND64
    worst, _ = check_fields(out["fout"], tf_step_oracle(name)["fout"], out["sent"], DT[prec], bound, (name,))
    print("worst tfsf step %s %s half %d: %.3g of the bound" % (name, prec, half, worst / bound))


# ==================================================================== plain
PLAIN_SIZE = (12, 40, 72)
PLAIN_CASES = [
    # name, T, output box, least (gx, gy, gz) of the fp32 multi-row launch
    ("whole", 3, ((0, 0, 0), PLAIN_SIZE), (3, 2, 2)),
    ("inner", 3, ((2, 5, 6), (11, 37, 70)), (2, 2, 2)),
    ("z-shell", 2, ((0, 0, 2), (12, 40, 4)), (3, 2, 1)),  # a decomposed rank's thin z shell
]
PLAIN = {c[0]: c for c in PLAIN_CASES}
PLAIN_KERNELS = [("f32", "multi"), ("f32", "single"), ("f64", "half")]


def plain_claim(family, claim):
    """(the single-row kernel's wide lanes span the 72 cells in one z tile)"""
    return (claim[0], claim[1], 1) if family == "single" else claim


def plain_run(name, dut, device, dtype, kernel="multi", record=None, **knobs):
    """One plain pass of a case; ``knobs`` override the default tuning knobs,
    ``record`` (a list) receives the pass's launches (``HipOps.record``).
    ``dev`` = the device tensors (fin, fout, clones of fin): a record's
    arguments point into them."""
    _, T, obox, _ = PLAIN[name]
    set_knobs(dut.ops, **{**dict(tb_mrows=2 if kernel == "multi" else 1, tb_mr_shape=0, tb_vec=0, tb_rows=0, tb_xcd=0,
                                 tb_variant=4, tb64_half=1), **knobs})
    seed = 9900 + 10 * list(PLAIN).index(name)
    Z = impedance(dut)
    fin, fout, sent, keep = run_pair_fields(live_fields(PLAIN_SIZE, seed, Z), PLAIN_SIZE, device, dtype)
    src = [("Ez", (6, 20, 3), Z * (0.5 + 0.25 * l)) for l in range(T)]
    if record is not None:
        dut.ops.record(record)
    try:
        dut.ops.tb_step(fin, fout, drude_upd(dut), obox, dut.cb, T, src)
    finally:
        if record is not None:
            dut.ops.record(None)
    if dut.ops.name == "hip":
        torch.cuda.synchronize()
        set_knobs(dut.ops, tb_mrows=0, tb_mr_shape=0, tb_variant=4)
    assert_unchanged(fin, keep, name)
    return dict(fout={c: fout[c].cpu() for c in COMPS}, sent=sent, dev=(fin, fout, keep))


@functools.lru_cache(None)
def plain_oracle(name):
    return plain_run(name, scheme(vacuum_cfg(PLAIN_SIZE, "f64"), "torch", "cpu", torch.float64), "cpu", torch.float64)


@pytest.mark.parametrize("prec,kernel", PLAIN_KERNELS)
@pytest.mark.parametrize("name", list(PLAIN))
def test_plain_pass_sentinel(gpu, name, prec, kernel):
    """The plain passes store nothing outside the output box (test_tb_gpu.py
    pre-fills the output with the input and cannot see such a store)."""
    _, T, obox, claim = PLAIN[name]
    family = {"multi": "mr16x2", "single": "single", "half": "f64half"}[kernel]
    assert_tiles(family, T, obox, plain_claim(family, claim))
    dut, ref = pair(vacuum_cfg(PLAIN_SIZE, "f64"), prec, gpu, "hip")
    out = plain_run(name, dut, gpu, DT[prec], kernel)
    bound = BOUND32 if prec == "f32" else BOUND64_PLAIN
    worst, _ = check_fields(out["fout"], plain_oracle(name)["fout"], out["sent"], DT[prec], bound, (name,))
    print("worst plain %s %s %s: %.3g of the bound" % (name, prec, kernel, worst / bound))


def test_plain_pass_is_one_recorded_launch(gpu):
    """A plain pass is ONE recorded launch that carries its own tile options:
    recorded with 8 waves x 4 rows, it replays bit for bit after the object's
    knobs changed and another HipOps object ran a pass with other knobs.
    (Tile shapes do not change a cell's arithmetic: the bitwise comparison
    guards the replayed arguments, the one-entry assertion the structure.)"""
    name = "whole"
    _, T, obox, claim = PLAIN[name]
    assert_tiles("mr8x4", T, obox, claim)
    dut, _ = pair(vacuum_cfg(PLAIN_SIZE, "f64"), "f32", gpu, "hip")
    rec = []
    first = plain_run(name, dut, gpu, torch.float32, "multi", record=rec, tb_mr_shape=1)
    assert len(rec) == 1, [f.__name__ for f, _ in rec]
    check_fields(first["fout"], plain_oracle(name)["fout"], first["sent"], torch.float32, BOUND32, (name, "recorded"))
    dut.ops.tb_mr_shape, dut.ops.tb_mrows = 0, 1
    other = copy.copy(dut)
    other.ops = make_ops("hip", None, gpu, torch.float32)
    assert other.ops is not dut.ops
    plain_run("inner", other, gpu, torch.float32, "multi", tb_mr_shape=2, tb_variant=7)
    fin, fout, keep = first["dev"]
    for c in COMPS:
        fout[c].copy_(to_dev(first["sent"][c], gpu, torch.float32))
    try:
        type(dut.ops).replay(rec)
        torch.cuda.synchronize()
    finally:
        dut.ops.tb_mrows = 0
    assert_unchanged(fin, keep, (name, "replay"))
    for c in COMPS:
        assert torch.equal(fout[c].cpu(), first["fout"][c]), (name, c, "the replayed pass differs from the recorded one")


def test_passes_of_two_objects_interleave(gpu):
    """Object A (8 waves x 4 rows, deferred stores + two planes prefetched)
    runs a plain pass, object B (defaults) a TF/SF pass through
    fdtd_tb3d_ext_f32, then A again: every pass runs with its own object's
    options and meets the bound of its own test."""
    plain, tf = "whole", "x-T1"
    a, _ = pair(vacuum_cfg(PLAIN_SIZE, "f64"), "f32", gpu, "hip")
    b, _ = pair(tf_cfg(TF[tf].inc), "f32", gpu, "hip")
    assert a.ops is not b.ops
    set_knobs(b.ops, tb_mrows=0, tb_mr_shape=0, tb_vec=0, tb_rows=0, tb_xcd=0, tb_variant=4)
    for who in ("A", "B", "A"):
        if who == "A":
            out = plain_run(plain, a, gpu, torch.float32, "multi", tb_mr_shape=1, tb_variant=7)
            want = plain_oracle(plain)
        else:
            out = tf_step_run(tf, b, gpu, torch.float32)
            want = tf_step_oracle(tf)
        worst, _ = check_fields(out["fout"], want["fout"], out["sent"], torch.float32, BOUND32, (who, plain, tf))
        print("worst interleaved %s: %.3g of the bound" % (who, worst / BOUND32))
