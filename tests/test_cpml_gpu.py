"""CPML kernels against the fp64 torch oracle while the slabs carry field.

The other GPU suites reach the absorbing slabs either with fields far below
their tolerance (runs from zero fields and a source) or compare HIP with HIP
(random fields, hybrid vs stepped).  Here every slab carries field and psi of
the size of the fields themselves, and the reference is ``TorchOps`` in
float64 on the CPU:

* half steps of the fused kernels (yee3d_cpml.hip) on single windows that land
  in every row layout, cross the padded z slab borders and start / end inside
  slabs (``test_fused_window``), with a control that the psi and the kappa
  terms are far above the tolerance on those windows;
* the multi-window launch ``curl_update_cpml_multi`` (``test_multi_windows``);
* the unfused corrections ``cpml_apply`` / ``cpml_apply_many``
  (``test_unfused_window``);
* the fp64 plain update on the double4 lanes (``test_f64_plain_windows``);
* whole runs from random fields, 3D fused / unfused and 2D, stepped and hybrid
  (``test_run_*``).

Tolerances of the half-step tests are measured, not guessed: ``e32`` is the
max error of the same half step through ``TorchOps`` in float32 on the CPU
against the float64 oracle, scaled by the oracle's largest value of the kind.
fp32 HIP gets ``4 e32`` (FMA contraction, another order of the sums), never
more than the run-level 2e-5; fp64 HIP gets ``4 e32 eps64 / eps32``.
"""
import dataclasses

import pytest
import torch

from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.parallel.domain import box_empty, box_intersect

pytestmark = pytest.mark.gpu

E, H = ("Ex", "Ey", "Ez"), ("Hx", "Hy", "Hz")
COMPS = E + H
TD = {"f32": torch.float32, "f64": torch.float64}
EPS_RATIO = 2.0 ** -52 / 2.0 ** -23
EMPTY = ((0, 0, 0), (0, 0, 0))

# nz = 240: the smallest multiple of 4 at which a whole-row window takes the
# 64-lane layout (lanes_z: a z span of at least 218); 7-cell z slabs are padded
# to float4 groups ([0, 8) and [232, 240))
SIZE = (20, 22, 240)
PML = (5, 6, 7)
SEED = 5

# e32 (fields, psi) per (scene, kind): the whole-range half step through
# TorchOps in float32 against the float64 oracle from the same (fp32-
# representable) fields and psi; fields scaled by the oracle's largest value of
# the kind, psi by the largest field of the source kind (psi is filled at that
# size).  test_e32_constants re-measures them.
E32 = {
    ("vacuum", "E"): (1.199e-7, 1.286e-7),
    ("vacuum", "H"): (1.220e-7, 1.227e-7),
    ("sphere", "E"): (1.199e-7, 1.286e-7),  # (the largest errors lie outside the sphere)
    ("sphere", "H"): (1.220e-7, 1.227e-7),
}
# Tolerances from these: fp32 4.8e-7 (E) / 4.9e-7 (H) for fields, 5.1e-7 / 4.9e-7 for psi; fp64 8.9e-16 /
# 9.1e-16 and 9.6e-16 / 9.1e-16.
# Observed on the MI355X, largest error / scale over all windows and both scenes (fields, psi):
#   fused and multi-window kernels  fp32 E 9.5e-8, 1.05e-7   H 8.9e-8, 9.2e-8
#                                   fp64 E 1.8e-16, 1.6e-16  H 2.3e-16, 2.2e-16
#   unfused (k_cpml / k_cpml_many)  fp32 E 1.2e-7, 1.1e-7    H 1.1e-7, 9.2e-8
#                                   fp64 E 2.9e-16, 1.6e-16  H 3.1e-16, 2.2e-16
# Smallest liveness ratio (window xslab-edge): fp32 E 1.1e4, H 2.1e3; fp64 E 5.9e12, H 1.1e12.
LIVE = 100.0  # the psi and the kappa term each move the result by more than LIVE x tolerance


def _cfg(scene, dtype):
    return SchemeConfig(scheme="3d", size=SIZE, dtype=dtype, time_steps=1, use_pml=True, pml_type="cpml",
                        pml_size=PML, cpml_kappa_max=3.0, cpml_alpha_max=0.05, scene=scene, sphere_radius=4.0,
                        sphere_center=(10.5, 11.5, 6.5))  # the sphere reaches z = 2.5: inside the low z slab


def _kind(c):
    return c[0]


def _names(kind):
    return E if kind == "E" else H


def _sl(box):
    return tuple(slice(box[0][d], box[1][d]) for d in range(3))


def _shift(box, lo):
    return (tuple(box[0][d] - lo[d] for d in range(3)), tuple(box[1][d] - lo[d] for d in range(3)))


def lanes_z(lo, hi):
    """Row layout of a window whose boxes span z [lo, hi) (yee3d_cpml.hip ``lanes_z``)."""
    kspan = hi - (lo & ~3)
    for lz in (64, 16):
        seg = 4 * lz
        if 20 * kspan >= 17 * (-(-kspan // seg) * seg):
            return lz
    return 8


class Side:
    """One scheme of the harness: fields and psi are loaded in place (the
    kernel table holds the psi pointers) from a CPU float64 state."""

    def __init__(self, scene, backend, device, dtype):
        name = {torch.float32: "f32", torch.float64: "f64"}[dtype]
        s = YeeScheme(_cfg(scene, name), make_ops(backend, None, device, dtype))
        s.init_scheme()
        s.init_grids()
        s.randomize_fields(SEED)
        self.s = s
        self.slabs = [sl for c in s.comps for sl in s.cpml.slabs[c]]

    def load(self, state):
        F, P = state
        for c in COMPS:
            self.s.F[0][c].copy_(F[c])
        for sl, v in zip(self.slabs, P):
            sl.psi[0].copy_(v)

    def grab(self):
        # (clones: a float64 CPU tensor converts to itself)
        return ({c: self.s.F[0][c].double().cpu().clone() for c in COMPS},
                [sl.psi[0].double().cpu().clone() for sl in self.slabs])

    def native(self):
        return [self.s.F[0][c].clone() for c in COMPS] + [sl.psi[0].clone() for sl in self.slabs]

    def boxes(self, kind, w):
        if isinstance(w, dict):
            return w
        return {c: self.s.local_box(c, w) for c in _names(kind)}

    def items(self, kind, boxes):
        """The corrections of models/cpml.py ``CPML.apply``, one per (component, slab)."""
        s = self.s
        F = s.F[0]
        out = []
        for c, box in boxes.items():
            for sl in s.cpml.slabs[c]:
                b = box_intersect(box, sl.lbox)
                if not box_empty(box) and not box_empty(b):
                    out.append((F[c], F[sl.src], sl.axis, sl.sign, sl.psi[0], sl.lbox, b, sl.b, sl.c, sl.kinv_m1,
                                s.cb[c]))
        return out

    def half(self, kind, windows, mode, ops=None):
        s = self.s
        ops = ops or s.ops
        F = s.F[0]
        wins = [self.boxes(kind, w) for w in windows]
        if mode == "multi":
            ops.curl_update_cpml_multi(kind, wins, F, F, s.cb, s.cpml.kernel_table(kind, 0))
            return
        for boxes in wins:
            if mode == "fused":
                ops.curl_update_cpml(kind, boxes, F, F, s.cb, s.cpml.kernel_table(kind, 0))
            elif mode == "oracle":  # the two independent pieces of TorchOps; cpml_apply_many where the backend has it
                ops.curl_update(kind, boxes, F, F, s.cb)
                s.cpml.apply(kind, 0, boxes)
            else:  # "single": one cpml_apply launch per correction
                ops.curl_update(kind, boxes, F, F, s.cb)
                for it in self.items(kind, boxes):
                    ops.cpml_apply(kind, *it)


_HARNESS = {}


def harness(scene):
    """The CPU part, shared by every test of a scene: the float64 oracle, the
    float32 reference and the start state (fields of ``randomize_fields``
    rounded to float32, so that every backend starts from the same values; psi
    of every slab from one float64 generator at the size of the source kind's
    fields, rounded likewise)."""
    hs = _HARNESS.get(scene)
    if hs is None:
        ref = Side(scene, "torch", "cpu", torch.float64)
        r32 = Side(scene, "torch", "cpu", torch.float32)
        F = {c: ref.s.F[0][c].float().double() for c in COMPS}
        gen = torch.Generator().manual_seed(SEED)
        P = []
        for sl in ref.slabs:
            scale = max(float(F[o].abs().max()) for o in COMPS if _kind(o) == _kind(sl.src))
            v = (torch.rand(sl.psi[0].shape, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * scale
            P.append(v.float().double())
        hs = _HARNESS[scene] = dict(ref=ref, r32=r32, state=(F, P))
    return hs


def oracle(scene, kind, windows, zero=None):
    """Oracle result of a half step; ``zero`` = ("psi" | "kappa", axis) runs it
    with that axis's psi tensors / kappa term zeroed."""
    hs = harness(scene)
    ref = hs["ref"]
    F, P = hs["state"]
    if zero is not None and zero[0] == "psi":
        P = [torch.zeros_like(v) if sl.axis == zero[1] else v for sl, v in zip(ref.slabs, P)]
    ref.load((F, P))
    saved = []
    if zero is not None and zero[0] == "kappa":
        for sl in ref.slabs:
            if sl.axis == zero[1]:
                saved.append((sl, sl.kinv_m1))
                sl.kinv_m1 = torch.zeros_like(sl.kinv_m1)
    try:
        ref.half(kind, windows, "oracle")
    finally:
        for sl, k in saved:
            sl.kinv_m1 = k
    return ref.grab()


def scales(scene, want, kind):
    """(field scale, psi scale) of a half step of ``kind``."""
    F0 = harness(scene)["state"][0]
    fs = max(float(want[0][c].abs().max()) for c in _names(kind))
    ps = max(float(F0[c].abs().max()) for c in COMPS if _kind(c) != kind)
    return fs, ps


def measure_e32(scene, kind):
    hs = harness(scene)
    whole = [((0, 0, 0), SIZE)]
    want = oracle(scene, kind, whole)
    hs["r32"].load(hs["state"])
    hs["r32"].half(kind, whole, "oracle")
    got = hs["r32"].grab()
    fs, ps = scales(scene, want, kind)
    ef = max(float((got[0][c] - want[0][c]).abs().max()) for c in COMPS) / fs
    ep = max(float((a - b).abs().max()) for a, b in zip(got[1], want[1])) / ps
    return ef, ep


def tolerances(scene, kind, dtype):
    ef, ep = E32[(scene, kind)]
    if dtype == "f32":
        return min(4.0 * ef, 2e-5), min(4.0 * ep, 2e-5)
    return 4.0 * ef * EPS_RATIO, 4.0 * ep * EPS_RATIO


def masks(side, kind, windows):
    """Per component / per slab the cells a half step of ``kind`` on
    ``windows`` updates: the boxes, and box ∩ slab in psi coordinates."""
    s = side.s
    wins = [side.boxes(kind, w) for w in windows]
    mf = {c: torch.zeros(s.domain.shape, dtype=torch.bool) for c in COMPS}
    mp = [torch.zeros(tuple(sl.psi[0].shape), dtype=torch.bool) for sl in side.slabs]
    for boxes in wins:
        for c, b in boxes.items():
            if box_empty(b):
                continue
            assert not bool(mf[c][_sl(b)].any()), "windows overlap"
            mf[c][_sl(b)] = True
            for n, sl in enumerate(side.slabs):
                x = box_intersect(b, sl.lbox)
                if sl.comp == c and not box_empty(x):
                    mp[n][_sl(_shift(x, sl.lbox[0]))] = True
    return mf, mp


def check(scene, side, kind, windows, got, want, tols, what):
    """Every cell of every field and psi tensor: inside the update boxes
    within tolerance of the oracle, outside them bit-identical to the input.
    Returns the largest (field, psi) errors / scale."""
    F0, P0 = harness(scene)["state"]
    mf, mp = masks(side, kind, windows)
    fs, ps = scales(scene, want, kind)
    worst = [0.0, 0.0]
    for c in COMPS:
        m = mf[c]
        assert torch.equal(got[0][c][~m], F0[c][~m]), (what, c, "cells outside the box changed")
        if bool(m.any()):
            err = float((got[0][c] - want[0][c])[m].abs().max()) / fs
            worst[0] = max(worst[0], err)
            assert err <= tols[0], (what, kind, c, "field error / scale", err, "tolerance", tols[0])
    for n, sl in enumerate(side.slabs):
        m = mp[n]
        assert torch.equal(got[1][n][~m], P0[n][~m]), (what, sl.comp, sl.axis, sl.side,
                                                       "psi outside box ∩ slab changed")
        if bool(m.any()):
            err = float((got[1][n] - want[1][n])[m].abs().max()) / ps
            worst[1] = max(worst[1], err)
            assert err <= tols[1], (what, kind, sl.comp, sl.axis, sl.side, "psi error / scale", err, "tolerance",
                                    tols[1])
    return worst


def liveness(scene, side, kind, windows, want, results, tol):
    """Per result in ``results`` the smallest ratio (its distance from the
    oracle run with one axis's psi / kappa term zeroed) / tolerance, over the
    slab axes the windows touch, on those slabs' cells of the windows."""
    fs, _ = scales(scene, want, kind)
    mf, mp = masks(side, kind, windows)
    worst = [float("inf")] * len(results)
    for axis in range(3):
        cells = {c: torch.zeros_like(mf[c]) for c in _names(kind)}
        for n, sl in enumerate(side.slabs):
            if sl.axis == axis and _kind(sl.comp) == kind and bool(mp[n].any()):
                cells[sl.comp][_sl(sl.lbox)] |= mp[n]
        if not any(bool(m.any()) for m in cells.values()):
            continue
        for term in ("psi", "kappa"):
            ctrl = oracle(scene, kind, windows, (term, axis))
            for q, res in enumerate(results):
                d = max(float((res[0][c] - ctrl[0][c])[m].abs().max()) for c, m in cells.items() if bool(m.any()))
                worst[q] = min(worst[q], d / fs / tol)
    return worst


_HIP = {}


def hip_side(gpu, scene, dtype):
    key = (scene, dtype)
    if key not in _HIP:
        side = Side(scene, "hip", gpu, TD[dtype])
        assert side.s.ops.fused_cpml_ok(side.s)
        _HIP[key] = side
    return _HIP[key]


def whole_row(x=(0, 20), y=(0, 22), z=(0, 240)):
    return ((x[0], y[0], z[0]), (x[1], y[1], z[1]))


# name: (global window, lanes per z row of both kinds' launches (lanes_z of the z span of the window's boxes),
# chunk of x planes per block or 0 for the kernel's own)
WINDOWS = {
    "whole": (whole_row(), 64, 0),                              # z span 240
    "zthin-low": (whole_row(z=(1, 12)), 8, 0),                  # span 12 from 0: unaligned, crosses the padded border 8
    "zthin-high": (whole_row(z=(226, 239)), 8, 0),              # span 15 from 224: crosses the padded border 232
    "z16": (whole_row(z=(3, 62)), 16, 0),                       # span 62 from 0
    "xslab-edge": (whole_row(x=(3, 6)), 64, 0),                 # starts inside the low x slab, ends one cell past it
    "xplane": (whole_row(x=(2, 3)), 64, 0),                     # one plane, inside the low x slab
    "yrow-high": (whole_row(y=(19, 20)), 64, 0),                # one row, inside the high y slab [16, 22)
    "zonly": (whole_row(x=(7, 13), y=(8, 14)), 64, 0),          # x / y interior: only the z terms are live
    "corner": (whole_row(x=(0, 5), y=(0, 6), z=(0, 8)), 8, 0),  # the three low slabs overlap
    "whole-xchunk3": (whole_row(), 64, 3),                      # chunk seams inside the x slabs: the i0 > 0 preload
}


def window_layout(side, kind, w):
    b = side.boxes(kind, w)
    lo = min(b[c][0][2] for c in b if not box_empty(b[c]))
    hi = max(b[c][1][2] for c in b if not box_empty(b[c]))
    return lanes_z(lo, hi)


def test_e32_constants():
    """The E32 table is what TorchOps in float32 gives against the oracle."""
    for (scene, kind), (ef, ep) in E32.items():
        mf, mp = measure_e32(scene, kind)
        print("e32", scene, kind, "fields %.4g psi %.4g" % (mf, mp))
        assert 0.8 * mf <= ef <= 1.25 * mf, (scene, kind, "fields", ef, mf)
        assert 0.8 * mp <= ep <= 1.25 * mp, (scene, kind, "psi", ep, mp)


@pytest.mark.parametrize("name", list(WINDOWS))
@pytest.mark.parametrize("scene", ["vacuum", "sphere"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_fused_window(gpu, dtype, scene, name):
    """One half step of the fused kernel on one window, E and H, from live
    fields and psi, against curl_update + cpml_apply of TorchOps in float64."""
    from fdtd3d_amd.ops.hip_ops import HipOps
    hs = harness(scene)
    side = hip_side(gpu, scene, dtype)
    w, lz, xchunk = WINDOWS[name]
    ops = HipOps(side.s.layout, gpu, TD[dtype], xchunk=xchunk) if xchunk else None
    percell = {k: side.s.cb[_names(k)[0]].cell is not None for k in "EH"}
    assert percell == {"E": scene == "sphere", "H": False}
    for kind in "EH":
        assert window_layout(side, kind, w) == lz
        tols = tolerances(scene, kind, dtype)
        want = oracle(scene, kind, [w])
        side.load(hs["state"])
        side.half(kind, [w], "fused", ops)
        torch.cuda.synchronize()
        got = side.grab()
        # a condition on the inputs: both terms are live on this window (the oracle's own result first)
        live_cpu, live = liveness(scene, hs["ref"], kind, [w], want, [want, got], tols[0])
        assert live_cpu > LIVE, (name, kind, "window not live", live_cpu)
        errs = check(scene, hs["ref"], kind, [w], got, want, tols, name)
        print("fused", dtype, scene, name, kind, "err/scale fields %.3g psi %.3g" % tuple(errs),
              "tol %.3g %.3g" % tols, "live %.3g" % live)
        assert live > LIVE, (name, kind, "psi / kappa term missing from the HIP result", live)


def _multi_lists(side, kind):
    first = _names(kind)[0]
    thin = [whole_row(y=(2 * n, 2 * n + 2), z=(1, 12)) for n in range(11)]
    a, b, c = whole_row(x=(0, 7)), whole_row(x=(7, 14), z=(3, 62)), whole_row(x=(14, 20), z=(226, 239))
    one = {o: (side.s.local_box(o, whole_row(x=(15, 19), y=(3, 9), z=(100, 140))) if o == first else EMPTY)
           for o in _names(kind)}
    return {
        "3layouts": ([a, b, c], [64, 16, 8]),         # one launch per row layout
        "11thin": (thin, [8] * 11),                   # a flush at 8 windows and a second launch of 3
        "with-empty": ([a, {o: EMPTY for o in _names(kind)}, c], [64, None, 8]),
        "one-component": ([b, one], [16, 8]),       # (z span 40 -> 8 lanes)
    }


@pytest.mark.parametrize("name", ["3layouts", "11thin", "with-empty", "one-component"])
@pytest.mark.parametrize("scene", ["vacuum", "sphere"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_multi_windows(gpu, dtype, scene, name):
    """curl_update_cpml_multi (Win3) on disjoint windows: the oracle, and bit
    for bit the same windows launched one by one."""
    hs = harness(scene)
    side = hip_side(gpu, scene, dtype)
    for kind in "EH":
        wins, layouts = _multi_lists(side, kind)[name]
        for w, lz in zip(wins, layouts):
            if lz is not None:
                assert window_layout(side, kind, w) == lz
        tols = tolerances(scene, kind, dtype)
        want = oracle(scene, kind, wins)
        side.load(hs["state"])
        n0 = side.s.ops.launches
        side.half(kind, wins, "multi")
        assert side.s.ops.launches == n0 + 1
        torch.cuda.synchronize()
        got, multi = side.grab(), side.native()
        side.load(hs["state"])
        side.half(kind, wins, "fused")
        torch.cuda.synchronize()
        for a, b in zip(multi, side.native()):
            assert torch.equal(a, b), (name, kind, "multi-window launch differs from single launches")
        live_cpu, live = liveness(scene, hs["ref"], kind, wins, want, [want, got], tols[0])
        assert live_cpu > LIVE, (name, kind, "windows not live", live_cpu)
        errs = check(scene, hs["ref"], kind, wins, got, want, tols, name)
        print("multi", dtype, scene, name, kind, "err/scale fields %.3g psi %.3g" % tuple(errs),
              "tol %.3g %.3g" % tols, "live %.3g" % live)
        assert live > LIVE, (name, kind, live)


@pytest.mark.parametrize("mode", ["single", "many"])
@pytest.mark.parametrize("name", ["whole", "zthin-high", "corner"])
@pytest.mark.parametrize("scene", ["vacuum", "sphere"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_unfused_window(gpu, dtype, scene, name, mode):
    """The fallback of grids the fused kernels do not take: curl_update, then
    the slab corrections one launch each (k_cpml) or grouped (k_cpml_many)."""
    hs = harness(scene)
    side = hip_side(gpu, scene, dtype)
    w = WINDOWS[name][0]
    for kind in "EH":
        tols = tolerances(scene, kind, dtype)
        want = oracle(scene, kind, [w])
        side.load(hs["state"])
        side.half(kind, [w], "single" if mode == "single" else "oracle")
        torch.cuda.synchronize()
        got = side.grab()
        live_cpu, live = liveness(scene, hs["ref"], kind, [w], want, [want, got], tols[0])
        assert live_cpu > LIVE, (name, kind, "window not live", live_cpu)
        errs = check(scene, hs["ref"], kind, [w], got, want, tols, name)
        print("unfused", mode, dtype, scene, name, kind, "err/scale fields %.3g psi %.3g" % tuple(errs),
              "tol %.3g %.3g" % tols, "live %.3g" % live)
        assert live > LIVE, (name, kind, live)


# ------------------------------------------------- fp64 plain windows (double4 lanes)
# e32 per (window of test_hip_gpu.WINDOWS, kind): TorchOps.curl_update in float32 against float64 from the same
# fp32-representable random fields (coefficient 0.3), scaled by the oracle's largest value of the kind.
E32_PLAIN = {
    ("mid", "E"): 7.373e-8, ("mid", "H"): 7.675e-8,
    ("thin", "E"): 7.392e-8, ("thin", "H"): 8.900e-8,
    ("wide", "E"): 6.422e-8, ("wide", "H"): 9.480e-8,
}
# Tolerances 4.8e-16 .. 7.1e-16; observed on the MI355X (double4 and scalar kernels alike): E 1.9e-16, H 1.8e-16.
PLAIN_SHAPE = (20, 24, 152)
_PLAIN = {}


def plain_case(win):
    """(input, float64 oracle, measured e32 per kind) of one window: E then H, as test_vec4_windows_match_scalar."""
    from test_hip_gpu import WINDOWS as HIP_WINDOWS
    from fdtd3d_amd.layout.yee import YeeLayout
    from fdtd3d_amd.ops.coef import Coef
    from fdtd3d_amd.ops.torch_ops import TorchOps
    if win not in _PLAIN:
        gen = torch.Generator().manual_seed(SEED)
        base = {c: torch.randn(PLAIN_SHAPE, generator=gen, dtype=torch.float32).double() for c in COMPS}
        lay = YeeLayout(PLAIN_SHAPE)
        cb = {c: Coef(0.3) for c in COMPS}
        be, bh = HIP_WINDOWS[win]
        out = {}
        for dt in (torch.float64, torch.float32):
            ops = TorchOps(lay, "cpu", dt)
            f = {c: t.clone().to(dt) for c, t in base.items()}
            ops.curl_update("E", be, f, f, cb)
            ops.curl_update("H", bh, f, f, cb)
            out[dt] = {c: t.double() for c, t in f.items()}
        want = out[torch.float64]
        scale = {k: max(float(want[c].abs().max()) for c in _names(k)) for k in "EH"}
        e32 = {k: max(float((out[torch.float32][c] - want[c]).abs().max()) for c in _names(k)) / scale[k] for k in "EH"}
        _PLAIN[win] = (base, want, e32, scale, dict(be, **bh), lay, cb)
    return _PLAIN[win]


def test_e32_plain_constants():
    for (win, kind), e in E32_PLAIN.items():
        m = plain_case(win)[2][kind]
        print("e32 plain", win, kind, "%.4g" % m)
        assert 0.8 * m <= e <= 1.25 * m, (win, kind, e, m)


@pytest.mark.parametrize("win", ["mid", "thin", "wide"])
def test_f64_plain_windows(gpu, win, monkeypatch):
    """HipOps.curl_update in fp64 on odd windows: the double4 lanes of
    yee3d_cpml.hip with an empty term table (8 / 16 / 64 lanes per row)
    against TorchOps in float64 and against the scalar fp64 kernels."""
    from test_hip_gpu import WINDOWS as HIP_WINDOWS
    from fdtd3d_amd.ops.hip_ops import HipOps
    base, want, _, scale, boxes, lay, cb = plain_case(win)
    be, bh = HIP_WINDOWS[win]
    res = {}
    for v4 in (True, False):
        monkeypatch.setattr(HipOps, "f64_v4", v4)
        ops = HipOps(lay, gpu, torch.float64)
        f = {c: t.to(gpu) for c, t in base.items()}
        ops.curl_update("E", be, f, f, cb)
        ops.curl_update("H", bh, f, f, cb)
        torch.cuda.synchronize()
        res[v4] = {c: t.cpu() for c, t in f.items()}
    for c in COMPS:
        tol = 4.0 * E32_PLAIN[(win, _kind(c))] * EPS_RATIO
        m = torch.zeros(PLAIN_SHAPE, dtype=torch.bool)
        m[_sl(boxes[c])] = True
        for v4 in (True, False):
            got = res[v4][c]
            assert torch.equal(got[~m], base[c][~m]), (win, c, v4, "cells outside the box changed")
            err = float((got - want[c])[m].abs().max()) / scale[_kind(c)]
            print("plain f64", win, c, "v4" if v4 else "scalar", "err/scale %.3g tol %.3g" % (err, tol))
            assert err <= tol, (win, c, "double4" if v4 else "scalar", err, tol)
        # the same arithmetic up to contraction and the order of the two differences
        d = float((res[True][c] - res[False][c]).abs().max()) / scale[_kind(c)]
        assert d <= 2.0 * tol, (win, c, "double4 vs scalar", d, tol)


# ------------------------------------------------------------ whole runs, live slabs
KAPPA = dict(use_pml=True, pml_type="cpml", cpml_kappa_max=3.0, cpml_alpha_max=0.05, scene="vacuum", time_steps=9)
RUNS = {
    "3d-fused": dict(scheme="3d", size=(80, 72, 96), pml_size=(5, 6, 7)),
    "3d-unfused": dict(scheme="3d", size=(40, 44, 50), pml_size=(5, 6, 7)),  # nz % 4 != 0: scalar update + cpml_apply
    "tmz": dict(scheme="tmz", size=(96, 88, 1), pml_size=(6, 6, 1)),
    "tez": dict(scheme="tez", size=(96, 88, 1), pml_size=(6, 6, 1)),
}
_RUN_REF = {}


def _run(cfg, backend, device, dtype):
    s = YeeScheme(cfg, make_ops(backend, None, device, dtype))
    s.init_scheme()
    s.init_grids()
    s.randomize_fields(seed=11)
    s.perform_steps()
    if device != "cpu":
        torch.cuda.synchronize()
    return s


def run_case(gpu, name, dtype, hb):
    """9 steps from random fields on HIP against the float64 torch oracle
    (one oracle run per configuration): all components and every psi, at the
    project's run-level tolerances.  Observed on the MI355X, error / scale:
    fp32 at most 4.7e-7, fp64 at most 6.6e-16 (1e-12 holds from random
    fields); hybrid and stepped runs give the same figures."""
    cfg = SchemeConfig(dtype=dtype, hybrid_block=hb, **KAPPA, **RUNS[name])
    if name not in _RUN_REF:
        _RUN_REF[name] = _run(dataclasses.replace(cfg, dtype="f64", hybrid_block=1), "torch", "cpu", torch.float64)
    ref = _RUN_REF[name]
    s = _run(cfg, "hip", gpu, TD[dtype])
    assert (s.hybrid is not None) == (hb > 1), "hybrid plan"
    assert s.ops.fused_cpml_ok(s) == (name == "3d-fused")
    tol = 2e-5 if dtype == "f32" else 1e-12
    scale = {k: max(float(ref.F[0][c].abs().max()) for c in ref.comps if c[0] == k) for k in "EH"}
    for c in ref.comps:
        err = float((s.F[0][c].double().cpu() - ref.F[0][c]).abs().max()) / scale[c[0]]
        print("run", name, dtype, "T=%d" % hb, c, "err/scale %.3g" % err)
        assert err <= tol, (name, c, err, tol)
        assert len(s.cpml.slabs[c]) == len(ref.cpml.slabs[c]) > 0
        for a, b in zip(s.cpml.slabs[c], ref.cpml.slabs[c]):
            assert float(b.psi[0].abs().max()) > 1e-3 * scale["H" if c[0] == "E" else "E"], "psi not live"
            err = float((a.psi[0].double().cpu() - b.psi[0]).abs().max()) / scale["H" if c[0] == "E" else "E"]
            assert err <= tol, (name, c, "psi", a.axis, a.side, err, tol)
    return s


@pytest.mark.parametrize("hb", [1, 4])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_run_3d_fused(gpu, dtype, hb):
    run_case(gpu, "3d-fused", dtype, hb)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_run_3d_unfused(gpu, dtype):
    run_case(gpu, "3d-unfused", dtype, 1)


@pytest.mark.parametrize("hb", [1, 4])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("scheme", ["tmz", "tez"])
def test_run_2d(gpu, scheme, dtype, hb):
    run_case(gpu, scheme, dtype, hb)
