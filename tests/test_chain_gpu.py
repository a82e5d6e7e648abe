"""UPML / Drude chain kernels against the fp64 torch oracle on live levels.

The other GPU suites reach ``chain_kernels.hip`` either from zero fields and a
source (the slabs then hold field orders below the tolerance) or from
``randomize_fields``, which leaves every D / D1 level at exactly zero.  Here
every field and every level of every component carries values of the size a
run holds them at, and the reference is ``TorchOps`` in float64 on the CPU
with the same (z-widened) chain boxes:

* half steps through ``scheme._update_chain_regions`` on the whole grid and on
  sub-windows (``test_half_step``), in every launch form of the library: one
  component per thread, three per thread, the float4 form, region-local and
  full-grid levels, the uint8 id + table and the five per-cell arrays, with
  and without the row table, and the generic D-form path of a TF/SF box;
* plain boxes folded into a chain launch (``test_folded_plain``);
* ``curl_general`` / ``lincomb`` on their own (``test_generic_ops``);
* short runs from the live state, level rotation included (``test_run``).

Inside the launch boxes the fields and the new levels are within tolerance of
the oracle; every other cell of every field and level is bit-identical to the
input.  Controls (the oracle rerun with D, Dp, D1 / D1p or the incident line
zeroed) show that each of those operands moves the result by more than
``LIVE`` tolerances on the cells of the form that reads it.

Tolerances are measured: ``e32`` is the error of the whole-grid half step
through ``TorchOps`` in float32 against the float64 oracle from the same
state, fields scaled by the oracle's largest value of the kind, each level by
the oracle's largest value of that level.  fp32 HIP gets ``4 e32`` (FMA
contraction, another order of the sums, the factored ``s cell ica (...)``
against the oracle's pre-multiplied ``Coef``), never more than the run-level
2e-5; fp64 HIP gets that times eps64 / eps32.
"""
import contextlib

import pytest
import torch

from fdtd3d_amd.layout.yee import YeeLayout
from fdtd3d_amd.models.regions import RegionLevel
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.coef import Coef
from fdtd3d_amd.ops.torch_ops import TorchOps
from fdtd3d_amd.parallel.domain import box_empty
from fdtd3d_amd.utils.constants import EPS0, MU0

pytestmark = pytest.mark.gpu

E, H = ("Ex", "Ey", "Ez"), ("Hx", "Hy", "Hz")
COMPS = E + H
TD = {"f32": torch.float32, "f64": torch.float64}
ALIGN = {"f32": 32, "f64": 16}  # cells of a 128-byte row segment: the HIP scheme's z_align
EPS_RATIO = 2.0 ** -52 / 2.0 ** -23
EMPTY = ((0, 0, 0), (0, 0, 0))

# x slabs of 5 planes (less than the 8-plane x chunk), a dispersive box of 11 planes (a chunk seam
# inside), y z footprints that are no multiples of 256; the z slabs widen to [0, 32) / [96, 128) in
# fp32 and [0, 16) / [112, 128) in fp64, clear of a sphere around z = 60
SIZE = (24, 22, 128)
PML = (5, 6, 7)
SEED = 7
BASE = dict(scheme="3d", size=SIZE, time_steps=1, use_pml=True, pml_type="upml", pml_size=PML, hybrid_block=1)
DRUDE = dict(use_metamaterials=True, scene="drude-sphere", sphere_radius=5.0, sphere_center=(12.0, 11.0, 60.0))
SCENES = {
    "upml": dict(scene="vacuum"),
    # a dielectric sphere reaching z = 2.5, inside the low z slab: per-cell 1/(eps eps0) for E
    "upml-sphere": dict(scene="sphere", sphere_radius=4.0, sphere_center=(10.5, 11.5, 6.5)),
    # (radius 4.5: at 5 the dispersive box of Ey touches the y slabs, 10 cells apart)
    "drude": dict(DRUDE, sphere_radius=4.5),
    "lorentz": dict(DRUDE, sphere_radius=4.5, dispersion="lorentz", lorentz_omega0_ratio=0.7),
    "drude-face": dict(DRUDE, sphere_center=(7.0, 11.0, 60.0)),  # reaches x = 2: inside the low x slab
    "drude-tfsf": dict(DRUDE, use_tfsf=True, tfsf_size=(9, 9, 40)),  # the x / y faces cut the dispersive box
}
DISPERSIVE = ("drude", "lorentz", "drude-face", "drude-tfsf")

# e32 (fields, new D level, new D1 level or None) per (scene, kind): see the module docstring.
# test_e32_constants re-measures them.
E32 = {
    ("upml", "E"): (1.259e-07, 1.100e-07, None),
    ("upml", "H"): (1.386e-07, 1.001e-07, None),
    ("upml-sphere", "E"): (1.264e-07, 1.100e-07, None),
    ("upml-sphere", "H"): (1.386e-07, 1.001e-07, None),
    ("drude", "E"): (1.320e-07, 9.373e-08, 8.804e-08),
    ("drude", "H"): (1.807e-07, 9.872e-08, None),
    ("lorentz", "E"): (1.320e-07, 9.373e-08, 1.022e-07),
    ("lorentz", "H"): (1.807e-07, 9.872e-08, None),
    ("drude-face", "E"): (1.283e-07, 9.373e-08, 9.669e-08),
    ("drude-face", "H"): (1.807e-07, 9.872e-08, None),
    ("drude-tfsf", "E"): (1.057e-07, 9.373e-08, 1.032e-07),
    ("drude-tfsf", "H"): (1.807e-07, 9.872e-08, None),
}
# Tolerances from these: fp32 4.2e-7 .. 7.2e-7 for fields, 3.7e-7 .. 4.4e-7 for D, 3.5e-7 .. 4.1e-7 for D1; fp64
# those times 2^-29 (7.9e-16 .. 1.3e-15, 7.0e-16 .. 8.2e-16, 6.6e-16 .. 7.7e-16).
# Observed on the MI355X, largest error / scale over all scenes and windows (fields, D, D1):
#   k_chain3d_c (default, region-local), k_chain3d dispersive with rows + LUT
#                                   fp32 E 1.6e-7, 1.1e-7, 1.0e-7   H 1.8e-7, 1.0e-7
#                                   fp64 E 3.7e-16, 1.7e-16, 1.9e-16  H 3.8e-16, 1.9e-16
#   k_chain3d non-dispersive (three components per thread)
#                                   fp32 E 1.6e-7, 9.5e-8   H 1.8e-7, 9.8e-8;  fp64 E 3.8e-16, 1.7e-16  H 3.8e-16, 2.0e-16
#   k_chain3d_v4 / full-grid levels fp32 E 1.6e-7, 1.1e-7, 1.0e-7   H 1.8e-7, 1.0e-7 (fp64 full-grid: as the default)
#   per-cell arrays, no row table   fp32 E 1.6e-7, 9.4e-8, 1.0e-7   H 1.7e-7, 9.9e-8;  fp64 E 3.7e-16, 1.7e-16, 1.9e-16
#   folded plain boxes (pbox)       fp32 E 1.3e-7, 1.2e-7   H 1.5e-7, 1.0e-7;  fp64 E 2.8e-16, 1.4e-16  H 3.2e-16, 1.8e-16
#   curl_general / lincomb          fp32 1.1e-7 / 9.3e-8;  fp64 1.6e-16 / 1.4e-16
# No case exceeds 1.4 e32: the factored s cell ica (...) of chain_finish costs no more than the oracle's Coef.
# Smallest liveness ratio: E (drude-tfsf, whole) fp32 6.2e4, fp64 3.3e13; H (xslab-edge) fp32 4.1e5, fp64 2.2e14.
# Runs of RUN_STEPS steps, error / final peak: fp32 at most 5.4e-7 (lorentz D1; TorchOps in float32: 5.6e-7), fp64
# at most 8.9e-16.
LIVE = 100.0  # every control moves the result by more than LIVE x tolerance


def _cfg(scene, dtype):
    return SchemeConfig(dtype=dtype, **dict(BASE, **SCENES[scene]))


def _kind(c):
    return c[0]


def _names(kind):
    return E if kind == "E" else H


def _sl(box):
    return tuple(slice(box[0][d], box[1][d]) for d in range(3))


def _levels(s):
    """(component, "D" | "D1", index) of every level of a scheme, in a fixed order."""
    out = []
    for c in COMPS:
        st = s.upml[c]
        out += [(c, "D", n) for n in range(st["nlev"])]
        if "D1" in st:
            out += [(c, "D1", n) for n in range(3)]
    return out


def _new(s, c, name):
    """Index of the level a launch writes."""
    return s.upml[c]["nlev"] - 1 if name == "D" else 2


class Side:
    """One scheme of the harness.  Fields, levels and the incident line are
    loaded in place from a CPU float64 state whose levels are full-grid
    tensors: region-local levels take their parts of them."""

    def __init__(self, scene, backend, device, dtype, align):
        name = {torch.float32: "f32", torch.float64: "f64"}[dtype]
        s = YeeScheme(_cfg(scene, name), make_ops(backend, None, device, dtype))
        s.init_scheme()
        s.init_grids()
        if backend != "hip":
            # the HIP scheme widens its z chain boxes to whole row segments (init_grids); the torch one does not
            s._init_chain_regions(s._chain_prof, z_align=align)
        s.randomize_fields(SEED)
        self.s = s
        self.scene = scene

    def level(self, key):
        c, name, n = key
        return self.s.upml[c][name][0][n]

    def load(self, state):
        s = self.s
        for c in COMPS:
            s.F[0][c].copy_(state["F"][c])
        for key in _levels(s):
            lv, v = self.level(key), state["L"][key]
            if isinstance(lv, RegionLevel):
                for t, b in zip(lv.data, lv.boxes):
                    t.copy_(v[_sl(b)])
            else:
                lv.copy_(v)
        if s.cfg.use_tfsf:
            s.einc[0].copy_(state["inc"][0])
            s.hinc[0].copy_(state["inc"][1])
        s.t = 0

    def grab(self, state):
        """The state after a launch, in the form of ``state`` (cells no
        region-local part holds keep the input's values)."""
        s = self.s
        out = {"F": {c: s.F[0][c].double().cpu().clone() for c in COMPS}, "L": {}}
        for key in _levels(s):
            lv = self.level(key)
            if isinstance(lv, RegionLevel):
                v = state["L"][key].clone()
                for t, b in zip(lv.data, lv.boxes):
                    v[_sl(b)] = t.double().cpu()
            else:
                v = lv.double().cpu().clone()
            out["L"][key] = v
        return out

    def plan(self, kind, w, pws=None):
        s = self.s
        s.__dict__.pop("_chain_plan_cache", None)
        return s._chain_plan(kind, w, tuple(pws) if pws is not None else None)

    def half(self, kind, w, pws=None):
        self.s._update_chain_regions(kind, 0, w, plain_windows=pws)


_HARNESS = {}


def harness(scene, dtype):
    """The CPU part of a (scene, dtype): the float64 oracle on the chain boxes
    of that dtype's HIP scheme, the float32 reference (fp32 boxes only) and the
    start state: E / H of ``randomize_fields``, every D / B level uniform in
    [-1, 1) eps0 |E|max (mu0 |H|max), every D1 / B1 level at the size of the
    fields of its kind, the incident line likewise -- one seeded float64
    generator in a fixed order, all rounded to float32."""
    hs = _HARNESS.get((scene, dtype))
    if hs is None:
        ref = Side(scene, "torch", "cpu", torch.float64, ALIGN[dtype])
        r32 = Side(scene, "torch", "cpu", torch.float32, ALIGN[dtype]) if dtype == "f32" else None
        s = ref.s
        F = {c: s.F[0][c].float().double() for c in COMPS}
        fmax = {k: max(float(F[c].abs().max()) for c in _names(k)) for k in "EH"}
        gen = torch.Generator().manual_seed(SEED)

        def rnd(shape, scale):
            return ((torch.rand(shape, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * scale).float().double()

        L = {}
        for key in _levels(s):
            k = _kind(key[0])
            scale = fmax[k] * ((EPS0 if k == "E" else MU0) if key[1] == "D" else 1.0)
            L[key] = rnd(SIZE, scale)
        state = {"F": F, "L": L}
        if s.cfg.use_tfsf:
            state["inc"] = (rnd(tuple(s.einc[0].shape), fmax["E"]), rnd(tuple(s.hinc[0].shape), fmax["H"]))
        hs = _HARNESS[(scene, dtype)] = dict(ref=ref, r32=r32, state=state, fmax=fmax, cache={})
    return hs


def zeroed(state, zero):
    """``state`` with the operand of a control zeroed: "D" the current D level,
    "Dp" the previous one, "D1" the current and previous D1 levels, "inc" the
    incident line."""
    if zero is None:
        return state
    out = dict(state, L=dict(state["L"]))
    for key, v in state["L"].items():
        if (zero, key[1], key[2]) in (("D", "D", 0), ("Dp", "D", 1), ("D1", "D1", 0), ("D1", "D1", 1)):
            out["L"][key] = torch.zeros_like(v)
    if zero == "inc":
        out["inc"] = tuple(torch.zeros_like(v) for v in state["inc"])
    return out


def oracle(scene, dtype, kind, launch, zero=None):
    """Oracle result of a launch (a callable on a Side), cached by its name."""
    hs = harness(scene, dtype)
    key = (kind, launch.name, zero, hs["ref"].s.ops.chain_rows)
    if key not in hs["cache"]:
        st = zeroed(hs["state"], zero)
        hs["ref"].load(st)
        launch(hs["ref"], kind)
        hs["cache"][key] = hs["ref"].grab(st)
    return hs["cache"][key]


class Launch:
    """A half step of one kind: ``window`` through _update_chain_regions
    (``pws``: its plain windows), or ``fn(side, kind)``."""

    def __init__(self, name, window=None, pws=None, fn=None):
        self.name, self.window, self.pws, self.fn = name, window, pws, fn

    def __call__(self, side, kind):
        if self.fn is not None:
            self.fn(side, kind)
        else:
            side.half(kind, self.window if self.window is not None else side.s._window(kind), self.pws)

    def masks(self, side, kind):
        """Per component the cells whose field the launch updates, and per new
        level the cells it writes; ``forms``: the cells of every chain launch
        (reads D), of the dispersive ones (read Dp, D1, D1p) and of the generic
        path (reads the incident line)."""
        s = side.s
        zeros = lambda: torch.zeros(SIZE, dtype=torch.bool)
        mf = {c: zeros() for c in _names(kind)}
        ml = {}
        forms = {n: {c: zeros() for c in _names(kind)} for n in ("D", "disp", "slow")}
        if self.fn is not None:
            items = self.fn.items(side, kind)
            plain = self.fn.plain(side, kind)
            slow = []
        else:
            w = self.window if self.window is not None else s._window(kind)
            plan = side.plan(kind, w, self.pws)
            items = [(sel, form, rows) for launches, _ in plan["chain"] for sel, form, _, _, rows in launches]
            slow = [x for _, sl in plan["chain"] for x in sl]
            plain = plan["plain"] + plan["folded"]
            plain += [fold for launches, _ in plan["chain"] for _, _, _, fold, _ in launches if fold is not None
                      and fold not in plan["folded"]]
        for boxes in plain:
            for c, b in boxes.items():
                if not box_empty(b):
                    assert not bool(mf[c][_sl(b)].any()), "launch boxes overlap"
                    mf[c][_sl(b)] = True
        for sel, form, rows in items:
            for c, b in sel.items():
                if box_empty(b):
                    continue
                assert not bool(mf[c][_sl(b)].any()), "launch boxes overlap"
                mf[c][_sl(b)] = True
                m = torch.ones(tuple(b[1][d] - b[0][d] for d in range(3)), dtype=torch.bool)
                if rows is not None:
                    m = TorchOps._row_mask((rows[0].cpu(), rows[1], rows[2]), b)
                forms["D"][c][_sl(b)] |= m
                ml.setdefault((c, "D", _new(s, c, "D")), zeros())[_sl(b)] |= m
                if form:
                    forms["disp"][c][_sl(b)] |= m
                    ml.setdefault((c, "D1", 2), zeros())[_sl(b)] |= m
        for c, b in slow:
            assert not bool(mf[c][_sl(b)].any()), "launch boxes overlap"
            mf[c][_sl(b)] = True
            forms["D"][c][_sl(b)] = True
            forms["slow"][c][_sl(b)] = True
            ml.setdefault((c, "D", _new(s, c, "D")), zeros())[_sl(b)] = True
            if "D1" in s.upml[c]:
                forms["disp"][c][_sl(b)] = True
                ml.setdefault((c, "D1", 2), zeros())[_sl(b)] = True
        return mf, ml, forms


def scales(scene, dtype, kind, want):
    """Scale of the fields of a kind and of its new D / D1 levels in an oracle result."""
    s = harness(scene, dtype)["ref"].s
    out = {"F": max(float(want["F"][c].abs().max()) for c in _names(kind))}
    for name in ("D", "D1"):
        v = [float(want["L"][(c, name, _new(s, c, name))].abs().max()) for c in _names(kind) if name in s.upml[c]]
        out[name] = max(v) if v else None
    return out


def errors(kind, got, want, sc, mf, ml):
    """Largest error / scale over the launch's cells: fields, D, D1."""
    out = {"F": 0.0, "D": 0.0, "D1": 0.0}
    for c, m in mf.items():
        if bool(m.any()):
            out["F"] = max(out["F"], float((got["F"][c] - want["F"][c])[m].abs().max()) / sc["F"])
    for key, m in ml.items():
        if bool(m.any()):
            out[key[1]] = max(out[key[1]], float((got["L"][key] - want["L"][key])[m].abs().max()) / sc[key[1]])
    return out


def measure_e32(scene, kind):
    hs = harness(scene, "f32")
    launch = Launch("whole")
    want = oracle(scene, "f32", kind, launch)
    hs["r32"].load(hs["state"])
    launch(hs["r32"], kind)
    got = hs["r32"].grab(hs["state"])
    mf, ml, _ = launch.masks(hs["ref"], kind)
    e = errors(kind, got, want, scales(scene, "f32", kind, want), mf, ml)
    return e["F"], e["D"], (e["D1"] if any(k[1] == "D1" for k in ml) else None)


def tolerances(scene, kind, dtype):
    f = 1.0 if dtype == "f32" else EPS_RATIO
    return {n: (None if e is None else min(4.0 * e, 2e-5) * f) for n, e in zip(("F", "D", "D1"), E32[(scene, kind)])}


def check(scene, dtype, kind, launch, got, want, what):
    """Every cell of every field and level: inside the launch's boxes within
    tolerance of the oracle, everywhere else bit-identical to the input.
    Returns the errors / scale."""
    hs = harness(scene, dtype)
    state = hs["state"]
    mf, ml, _ = launch.masks(hs["ref"], kind)
    tols = tolerances(scene, kind, dtype)
    for c in COMPS:
        m = mf.get(c)
        keep = ~m if m is not None else torch.ones(SIZE, dtype=torch.bool)
        assert torch.equal(got["F"][c][keep], state["F"][c][keep]), (what, c, "field cells outside the boxes changed")
    for key, v in state["L"].items():
        m = ml.get(key)
        keep = ~m if m is not None else torch.ones(SIZE, dtype=torch.bool)
        assert torch.equal(got["L"][key][keep], v[keep]), (what, key, "level cells outside the boxes changed")
    errs = errors(kind, got, want, scales(scene, dtype, kind, want), mf, ml)
    for n, e in errs.items():
        assert tols[n] is not None or e == 0.0, (what, n)
        assert tols[n] is None or e <= tols[n], (what, kind, n, "error / scale", e, "tolerance", tols[n])
    return errs


def controls(scene, launch, side, kind):
    """(zeroed operand, cells of the form that reads it) per control of a launch."""
    _, _, forms = launch.masks(side, kind)
    out = [("D", forms["D"])]
    if any(bool(m.any()) for m in forms["disp"].values()):
        out += [("Dp", forms["disp"]), ("D1", forms["disp"])]
    if any(bool(m.any()) for m in forms["slow"].values()):
        out.append(("inc", forms["slow"]))
    return out


def liveness(scene, dtype, kind, launch, want, results):
    """Per result the smallest (distance from a control) / (field tolerance)
    over the launch's controls, on the cells of the form concerned."""
    hs = harness(scene, dtype)
    tol = tolerances(scene, kind, dtype)["F"]
    fs = scales(scene, dtype, kind, want)["F"]
    worst = [float("inf")] * len(results)
    for zero, cells in controls(scene, launch, hs["ref"], kind):
        assert any(bool(m.any()) for m in cells.values()), (launch.name, zero)
        ctrl = oracle(scene, dtype, kind, launch, zero)
        for q, res in enumerate(results):
            d = max(float((res["F"][c] - ctrl["F"][c])[m].abs().max()) for c, m in cells.items() if bool(m.any()))
            worst[q] = min(worst[q], d / fs / tol)
    return worst


def box(x=(0, SIZE[0]), y=(0, SIZE[1]), z=(0, SIZE[2])):
    return ((x[0], y[0], z[0]), (x[1], y[1], z[1]))


# windows of test_half_step: name -> (global window, dispersive scenes only, a launch box with a
# non-zero offset on every axis of its region-local storage box)
WINDOWS = {
    "whole": (None, False, False),
    "xslab-edge": (box(x=(3, 6), y=(2, 21), z=(3, 125)), False, True),  # starts inside the low x slab, ends past it
    "xplane": (box(x=(2, 3)), False, False),                            # one plane inside the low x slab
    "yrow-high": (box(y=(19, 20)), False, False),                       # one row inside the high y slab [16, 22)
    "corner": (box(x=(0, 5), y=(0, 6), z=(0, 8)), False, False),        # the three low slabs overlap
    # cuts the dispersive box (Ex of "drude": [7, 16) x [7, 15) x [56, 64)) on every axis, in z inside the
    # material range of the middle rows
    "disp-cut": (box(x=(8, 18), y=(8, 15), z=(58, 63)), True, True),
}


def launches(scene, kind):
    """(The dispersive box holds chain cells of E only: H takes the plain update there.)"""
    return [Launch(n, w) for n, (w, disp, _) in WINDOWS.items() if not disp or (scene in DISPERSIVE and kind == "E")]


def offset_inside(side, kind, launch):
    """True when a component's chain launch box is strictly smaller than the
    region-local storage box of its levels, at a non-zero offset on every axis."""
    s = side.s
    plan = side.plan(kind, launch.window)
    for ls, _ in plan["chain"]:
        for sel, form, _, _, _ in ls:
            for c, b in sel.items():
                lv = s.upml[c]["D"][0][0]
                if box_empty(b) or not isinstance(lv, RegionLevel):
                    continue
                t, sb = lv.part(b)
                if all(b[0][d] > sb[0][d] for d in range(3)) and all(b[1][d] <= sb[1][d] for d in range(3)):
                    return True
    return False


def test_e32_constants():
    """The E32 table is what TorchOps in float32 gives against the oracle."""
    for (scene, kind), want in E32.items():
        got = measure_e32(scene, kind)
        print("e32", scene, kind, " ".join("-" if v is None else "%.4g" % v for v in got))
        for a, b in zip(want, got):
            assert (a is None) == (b is None), (scene, kind, want, got)
            assert a is None or 0.8 * b <= a <= 1.25 * b, (scene, kind, want, got)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_scene_forms(scene, dtype):
    """Conditions on the inputs, the oracle alone: each scene reaches the form
    it is there for, and every launch of test_half_step is live."""
    hs = harness(scene, dtype)
    s = hs["ref"].s
    percell = {k: s.upml[_names(k)[0]]["prof"]["cell"] is not None for k in "EH"}
    assert percell == {"E": scene == "upml-sphere", "H": False}
    assert s.upml_regional == (scene != "drude-tfsf")
    zlo = min(b[0][2] for r in s.chain_regions["E"]["plain"] for b in r.values() if not box_empty(b))
    assert zlo == ALIGN[dtype]
    if scene in DISPERSIVE:
        for c in E:
            assert "D1" in s.upml[c] and s.upml[c]["nlev"] == 3
        for c in H:
            assert "D1" not in s.upml[c] and s.upml[c]["nlev"] == 2
    for kind in "EH":
        plan = hs["ref"].plan(kind, s._window(kind))
        forms = [(form, pf, rows is not None) for ls, _ in plan["chain"] for _, form, pf, _, rows in ls]
        slow = [x for _, sl in plan["chain"] for x in sl]
        if scene in ("upml", "upml-sphere"):
            assert forms == [(False, False, False)] * 6 and not slow
        elif kind == "H":
            assert all(f == (False, True, False) for f in forms) and (not slow or scene == "drude-tfsf")
        elif scene in ("drude", "lorentz"):
            assert forms == [(False, True, False)] * 6 + [(True, False, True)] and not slow
        elif scene == "drude-face":
            # a slab region with dispersive cells: the dispersive form with sigma != 0 and no row table
            reg = [(r, dru) for r, dru in s.chain_regions["E"]["chain"][:6] if any(dru.values())]
            assert len(reg) >= 1
            for r, dru in reg:
                sel = {c: s.domain.to_local(r[c]) for c in E if dru[c]}
                assert not s._sigma0_launch(sel)
            assert (True, False, False) in forms and (True, False, True) in forms
        else:
            assert slow and all(c in E for c, _ in slow), "TF/SF targets inside the dispersive box: generic D form"
        for launch in launches(scene, kind):
            want = oracle(scene, dtype, kind, launch)
            (live,) = liveness(scene, dtype, kind, launch, want, [want])
            print("live", scene, dtype, kind, launch.name, "%.3g" % live)
            assert live > LIVE, (scene, kind, launch.name, "launch not live", live)
            if WINDOWS[launch.name][2] and s.upml_regional:
                assert offset_inside(hs["ref"], kind, launch), (scene, kind, launch.name)


# ---------------------------------------------------------------- HIP side
_HIP = {}


def hip_side(gpu, scene, dtype):
    key = (scene, dtype)
    if key not in _HIP:
        side = Side(scene, "hip", gpu, TD[dtype], ALIGN[dtype])
        ref = harness(scene, dtype)["ref"]
        assert side.s.chain_regions == ref.s.chain_regions, "chain boxes of the two sides differ"
        assert side.s.upml_regional == ref.s.upml_regional
        assert _levels(side.s) == _levels(ref.s)
        # stepped launches of chain_kernels.hip only: no blocked core, no blocked Drude box
        assert side.s.hybrid is None and side.s.drude_blk is None and side.s._drude_plan is None
        _HIP[key] = side
    return _HIP[key]


def _realloc_levels(s):
    for c in COMPS:
        s.upml[c]["D"] = None
        if "D1" in s.upml[c]:
            s.upml[c]["D1"] = None
    s._alloc_upml_levels()


def _disp_cells(s):
    return [c for c in COMPS if "D1" in s.upml[c]]


@contextlib.contextmanager
def variant(name, side, ref):
    """One launch form of the HIP library, restored on the way out."""
    from fdtd3d_amd.ops.hip_ops import load_library
    s, ops, lib = side.s, side.s.ops, load_library()
    regional = s.upml_regional
    luts = {}
    try:
        if name == "three":
            ops.set_chain_split(0)
        if name in ("v4", "fullgrid"):
            ops.region_aux = False
            _realloc_levels(s)
            assert not s.upml_regional and not isinstance(s.upml["Ex"]["D"][0][0], RegionLevel)
        if name == "v4":
            lib.fdtd_set_chain_v4(1)
        if name == "cells":
            for c in _disp_cells(s):
                s._drude_cells(c)
                luts[c] = s.upml[c].pop("_drude_lut")
                assert all(s.upml[c][n].cell is not None for n in ("b0", "b1", "b2", "ma1", "ma2"))
            ops.drude_lut = False
        if name == "norows":
            ops.chain_rows = ref.s.ops.chain_rows = False
        if name not in ("fullgrid", "v4"):
            assert s.upml_regional == regional
        if name != "cells":
            for c in _disp_cells(s):
                ids = s.upml[c].get("_drude_lut")
                assert ids is not None and ids[0] is not None and ids[0].dtype == torch.uint8
        yield
    finally:
        ops.set_chain_split(-1)
        lib.fdtd_set_chain_v4(0)
        ops.drude_lut = True
        for c, v in luts.items():
            s.upml[c]["_drude_lut"] = v
        ops.chain_rows = ref.s.ops.chain_rows = True
        if not ops.region_aux:
            ops.region_aux = True
            _realloc_levels(s)
        assert s.upml_regional == regional
        for x in (s, ref.s):
            x.__dict__.pop("_chain_plan_cache", None)


def variants(scene, dtype):
    out = ["default", "three"]
    if scene != "drude-tfsf":
        out.append("fullgrid")  # (drude-tfsf holds full-grid levels by itself)
        if dtype == "f32":
            out.append("v4")
    if scene in DISPERSIVE:
        out += ["cells", "norows"]
    return out


def reached(scene, name, side, kind, launch):
    """The plan and the ops flags say the launch takes the form ``name``."""
    s = side.s
    plan = side.plan(kind, launch.window if launch.window is not None else s._window(kind), launch.pws)
    forms = [(form, rows is not None) for ls, _ in plan["chain"] for _, form, _, _, rows in ls]
    if name in ("three", "v4") and launch.name == "whole":
        assert any(not form for form, _ in forms), "no non-dispersive launch"
    if name in ("v4", "fullgrid"):
        assert not s.upml_regional and not s.ops.region_aux
    if name == "norows":
        assert not any(rows for _, rows in forms)
    if name == "default" and scene in ("drude", "lorentz") and kind == "E" and launch.name in ("whole", "disp-cut"):
        assert (True, True) in forms
    if name == "cells":
        assert not s.ops.drude_lut and all("_drude_lut" not in s.upml[c] for c in _disp_cells(s))
    if scene == "drude-tfsf" and kind == "E" and launch.name in ("whole", "disp-cut"):
        assert any(sl for _, sl in plan["chain"]), "generic D-form path not taken"


WORST = {}


def note(tag, errs, live):
    w = WORST.setdefault(tag, dict(F=0.0, D=0.0, D1=0.0, live=float("inf")))
    for n in ("F", "D", "D1"):
        w[n] = max(w[n], errs[n])
    w["live"] = min(w["live"], live)
    return w


def run_launch(gpu, scene, dtype, name, kind, launch, side):
    hs = harness(scene, dtype)
    want = oracle(scene, dtype, kind, launch)
    side.load(hs["state"])
    n0 = side.s.ops.launches
    launch(side, kind)
    torch.cuda.synchronize()
    assert side.s.ops.launches > n0
    got = side.grab(hs["state"])
    live_cpu, live = liveness(scene, dtype, kind, launch, want, [want, got])
    assert live_cpu > LIVE, (scene, kind, launch.name, "launch not live", live_cpu)
    what = (scene, dtype, name, kind, launch.name)
    errs = check(scene, dtype, kind, launch, got, want, what)
    tols = tolerances(scene, kind, dtype)
    print("chain", *what, "err/scale F %.3g D %.3g D1 %.3g" % (errs["F"], errs["D"], errs["D1"]),
          "tol", " ".join("-" if v is None else "%.3g" % v for v in tols.values()), "live %.3g" % live)
    assert live > LIVE, (what, "an operand is missing from the HIP result", live)
    w = note((name, dtype, kind), errs, live)
    print("worst", name, dtype, kind, "F %.3g D %.3g D1 %.3g live %.3g" % (w["F"], w["D"], w["D1"], w["live"]))


CASES = [(scene, dtype, name) for scene in SCENES for dtype in ("f32", "f64") for name in variants(scene, dtype)]


@pytest.mark.parametrize("scene,dtype,name", CASES)
def test_half_step(gpu, scene, dtype, name):
    """One half step of E and of H through _update_chain_regions, on the whole
    grid and on every window, in one launch form of the library."""
    hs = harness(scene, dtype)
    side = hip_side(gpu, scene, dtype)
    with variant(name, side, hs["ref"]):
        for kind in "EH":
            for launch in launches(scene, kind):
                reached(scene, name, side, kind, launch)
                if name == "default" and WINDOWS[launch.name][2] and side.s.upml_regional:
                    assert offset_inside(side, kind, launch)
                run_launch(gpu, scene, dtype, name, kind, launch, side)


# ---------------------------------------------------------------- folded plain boxes
class Folded:
    """chain_update on the low z slab region with a hand-made plain box of 40
    z cells on top of it, inside its (x, y) footprint."""

    def __init__(self, dtype):
        self.dtype = dtype

    def _boxes(self, side, kind):
        s = side.s
        r, dru = s.chain_regions[kind]["chain"][4]  # (x-low, x-high, y-low, y-high, z-low, z-high, dispersive)
        sel = {c: s.domain.to_local(r[c]) for c in _names(kind)}
        z1 = ALIGN[self.dtype]
        assert all(b[1][2] == z1 and b[0][2] <= 1 for b in sel.values()) and not any(dru.values())
        pb = {}
        for n, (c, b) in enumerate(sel.items()):
            # inside the footprint, one cell in on some sides; one component without a plain box
            pb[c] = EMPTY if n == 2 else ((b[0][0] + n, b[0][1] + 1, z1), (b[1][0] - 1, b[1][1] - n, z1 + 40))
        return sel, pb

    def items(self, side, kind):
        return [(self._boxes(side, kind)[0], False, None)]

    def plain(self, side, kind):
        return [self._boxes(side, kind)[1]]

    def __call__(self, side, kind):
        s = side.s
        sel, pb = self._boxes(side, kind)
        s.ops.chain_update(kind, sel, s.F[0], s.upml, 0, False, False, plain={c: b for c, b in pb.items()
                                                                               if not box_empty(b)}, cb=s.cb)


@pytest.mark.parametrize("name", ["default", "three", "v4"])
@pytest.mark.parametrize("scene", ["upml", "upml-sphere"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_folded_plain(gpu, dtype, scene, name):
    """Plain Yee cells folded into a chain launch (pbox): scalar and per-cell
    plain coefficients, by hand and through the plan's folded list."""
    if name == "v4" and dtype == "f64":
        name = "fullgrid"  # (the float4 form is fp32 only)
    hs = harness(scene, dtype)
    side = hip_side(gpu, scene, dtype)
    assert (side.s.cb["Ex"].cell is not None) == (scene == "upml-sphere") and side.s.cb["Hx"].cell is None
    by_hand = Launch("folded-hand", fn=Folded(dtype))
    # the plain cells of z < 60 next to the whole low z slab: the plan folds them into its launch
    by_plan = Launch("folded-plan", window=box(), pws=[box(z=(0, 60))])
    with variant(name, side, hs["ref"]):
        for kind in "EH":
            plan = side.plan(kind, by_plan.window, by_plan.pws)
            assert plan["folded"] and not plan["plain"], "the plan folds no plain box"
            assert all(b[1][2] - b[0][2] <= 64 for f in plan["folded"] for b in f.values())
            for launch in (by_hand, by_plan):
                F0 = hs["state"]["F"]
                want = oracle(scene, dtype, kind, launch)
                mf, _, forms = launch.masks(hs["ref"], kind)
                tol = tolerances(scene, kind, dtype)["F"]
                fs = scales(scene, dtype, kind, want)["F"]
                for c in _names(kind):
                    m = mf[c] & ~forms["D"][c]  # the plain cells: their update is far above the tolerance
                    if launch is by_hand and c == _names(kind)[2]:
                        assert not bool(m.any())
                        continue
                    assert int(m.sum()) > 1000
                    assert float((want["F"][c] - F0[c])[m].abs().max()) / fs > LIVE * tol
                run_launch(gpu, scene, dtype, name + "-folded", kind, launch, side)


# ---------------------------------------------------------------- generic building blocks
GSHAPE = (13, 11, 37)
G2SHAPE = (29, 23, 1)
GBOXES = {"odd": ((2, 1, 3), (11, 10, 34)), "thin": ((1, 2, 5), (12, 3, 36))}
G2BOXES = {"odd": ((3, 1, 0), (26, 20, 1)), "thin": ((5, 2, 0), (6, 21, 1))}
COEFS = ("scalar", "one-profile", "two-profiles", "cell", "all")
# e32 of TorchOps in float32 against float64 per (op, coefficient form), the larger of the two boxes, scaled by
# the oracle's largest value in the box; test_e32_generic re-measures them
E32_GEN = {
    ("curl3d", "scalar"): 8.428e-08, ("curl3d", "one-profile"): 1.611e-07, ("curl3d", "two-profiles"): 8.642e-08,
    ("curl3d", "cell"): 1.087e-07, ("curl3d", "all"): 9.654e-08,
    ("curl2d", "scalar"): 9.187e-08, ("curl2d", "one-profile"): 1.005e-07, ("curl2d", "two-profiles"): 1.062e-07,
    ("curl2d", "cell"): 7.987e-08, ("curl2d", "all"): 9.488e-08,
    ("lincomb3", "scalar"): 6.399e-08, ("lincomb3", "one-profile"): 6.329e-08, ("lincomb3", "two-profiles"): 6.993e-08,
    ("lincomb3", "cell"): 7.993e-08, ("lincomb3", "all"): 1.351e-07,
    ("lincomb5", "scalar"): 7.953e-08, ("lincomb5", "one-profile"): 8.883e-08, ("lincomb5", "two-profiles"): 7.610e-08,
    ("lincomb5", "cell"): 7.750e-08, ("lincomb5", "all"): 9.825e-08,
}


def _coef(form, shape, gen, n):
    """The n-th coefficient of a case: values in [0.5, 1.5), float32-representable."""
    def rnd(*sh):
        return (torch.rand(sh, generator=gen, dtype=torch.float64) + 0.5).float().double()
    k = Coef(0.75 + 0.125 * n)
    if form in ("one-profile", "two-profiles", "all"):
        k.px = rnd(shape[0])
    if form in ("two-profiles", "all"):
        k.py = rnd(shape[1])
    if form == "all":
        k.pz = rnd(shape[2])
    if form in ("cell", "all"):
        k.cell = rnd(*shape)
    return k


_GEN = {}


def generic_case(op, form, bname):
    """(input tensors, coefficients, box, apply(ops, tensors, coefs) -> out
    tensor, oracle result, e32, scale) of one generic op case."""
    key = (op, form, bname)
    if key in _GEN:
        return _GEN[key]
    two_d = op == "curl2d"
    shape = G2SHAPE if two_d else GSHAPE
    bx = (G2BOXES if two_d else GBOXES)[bname]
    lay = YeeLayout(shape, "tmz") if two_d else YeeLayout(shape)
    ops_ = ("curl3d", "curl2d", "lincomb3", "lincomb5")
    gen = torch.Generator().manual_seed(SEED + 100 * ops_.index(op) + 10 * COEFS.index(form) + list(GBOXES).index(bname))
    nt = {"curl3d": 4, "curl2d": 4, "lincomb3": 3, "lincomb5": 5}[op]
    T = [torch.randn(shape, generator=gen, dtype=torch.float64).float().double() for _ in range(nt)]
    K = [_coef(form, shape, gen, n) for n in range(nt)]

    def apply(ops, T, K):
        if op == "curl3d":    # Ex: two curl terms (Hz along y, Hy along z)
            assert len(lay.curl_terms("Ex")) == 2
            ops.curl_general("E", "Ex", bx, T[0], T[1], {"Hz": T[2], "Hy": T[3]}, K[0], K[1])
        elif op == "curl2d":  # TMz Hx: one term (Ez along y)
            assert len(lay.curl_terms("Hx")) == 1
            ops.curl_general("H", "Hx", bx, T[0], T[1], {"Ez": T[2]}, K[0], K[1])
        else:                 # out aliases the first term, as _upml_region's F[c]
            ops.lincomb(T[0], bx, [(K[n], T[n]) for n in range(nt)])
        return T[0]

    res = {}
    for dt in (torch.float64, torch.float32):
        ops = TorchOps(lay, "cpu", dt)
        res[dt] = apply(ops, [t.clone().to(dt) for t in T], [k.to("cpu", dt) for k in K]).double()
    want = res[torch.float64]
    scale = float(want[_sl(bx)].abs().max())
    e32 = float((res[torch.float32] - want).abs().max()) / scale
    _GEN[key] = (T, K, bx, lay, apply, want, e32, scale)
    return _GEN[key]


def test_e32_generic():
    for (op, form), e in E32_GEN.items():
        m = max(generic_case(op, form, b)[6] for b in GBOXES)
        print("e32 generic", op, form, "%.4g" % m)
        assert 0.8 * m <= e <= 1.25 * m, (op, form, e, m)


@pytest.mark.parametrize("form", COEFS)
@pytest.mark.parametrize("op", ["curl3d", "curl2d", "lincomb3", "lincomb5"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_generic_ops(gpu, dtype, op, form):
    """curl_general / lincomb of generic_kernels.hip on an odd and a one-cell-
    thick box against TorchOps in float64; cells outside the box bit-identical."""
    from fdtd3d_amd.ops.hip_ops import HipOps
    tol = min(4.0 * E32_GEN[(op, form)], 2e-5) * (1.0 if dtype == "f32" else EPS_RATIO)
    for bname in GBOXES:
        T, K, bx, lay, apply, want, _, scale = generic_case(op, form, bname)
        ops = HipOps(lay, gpu, TD[dtype])
        got = apply(ops, [t.to(gpu, TD[dtype]) for t in T], [k.to(gpu, TD[dtype]) for k in K])
        torch.cuda.synchronize()
        got = got.double().cpu()
        m = torch.zeros(tuple(T[0].shape), dtype=torch.bool)
        m[_sl(bx)] = True
        assert torch.equal(got[~m], T[0][~m]), (op, form, bname, "cells outside the box changed")
        assert float((want - T[0])[m].abs().max()) > LIVE * tol * scale
        err = float((got - want)[m].abs().max()) / scale
        print("generic", dtype, op, form, bname, "err/scale %.3g tol %.3g" % (err, tol))
        assert err <= tol, (op, form, bname, err, tol)


# ---------------------------------------------------------------- short runs from the live state
RUN_STEPS = 6
_RUN = {}


def run_oracle(scene, dtype, side=None):
    """RUN_STEPS steps of perform_steps from the live state (level rotation
    included) on ``side``; default and cached: the oracle."""
    hs = harness(scene, dtype)
    if side is None and (scene, dtype) in _RUN:
        return _RUN[(scene, dtype)]
    x = side or hs["ref"]
    x.load(hs["state"])
    x.s.perform_steps(RUN_STEPS)
    out = x.grab(hs["state"])
    if side is None:
        _RUN[(scene, dtype)] = out
    return out


def run_errors(scene, dtype, got, want):
    """Per kind: fields / their final peak; current D and D1 levels / their own peaks (cells the chain boxes
    hold: the others are never read)."""
    s = harness(scene, dtype)["ref"].s
    out = {}
    for kind in "EH":
        names = _names(kind)
        fs = max(float(want["F"][c].abs().max()) for c in names)
        out[(kind, "F")] = max(float((got["F"][c] - want["F"][c]).abs().max()) for c in names) / fs
        for name in ("D", "D1"):
            keys = [(c, name, 0) for c in names if name in s.upml[c]]
            if keys:
                sc = max(float(want["L"][k].abs().max()) for k in keys)
                out[(kind, name)] = max(float((got["L"][k] - want["L"][k]).abs().max()) for k in keys) / sc
    return out


def test_run_f32_reference():
    """The float32 TorchOps run stays under a quarter of the fp32 run tolerance: RUN_STEPS is not too long."""
    for scene in SCENES:
        hs = harness(scene, "f32")
        errs = run_errors(scene, "f32", run_oracle(scene, "f32", hs["r32"]), run_oracle(scene, "f32"))
        print("run f32 torch", scene, " ".join("%s/%s %.3g" % (k + (v,)) for k, v in errs.items()))
        assert max(errs.values()) <= 0.25 * 2e-5, (scene, errs)


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_run(gpu, dtype, scene):
    """RUN_STEPS whole steps on HIP from the live state against the oracle,
    at the project's run tolerances."""
    side = hip_side(gpu, scene, dtype)
    want = run_oracle(scene, dtype)
    got = run_oracle(scene, dtype, side)
    torch.cuda.synchronize()
    tol = 2e-5 if dtype == "f32" else 1e-11
    errs = run_errors(scene, dtype, got, want)
    print("run", dtype, scene, " ".join("%s/%s %.3g" % (k + (v,)) for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= tol, (scene, dtype, k, v, tol)
