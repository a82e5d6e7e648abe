"""The decomposed cases of test_decomposed_gpu.py (HIP thread ranks) and
test_decomposed_cpu.py (the torch oracle on CPU thread ranks): configurations,
what a rank reports, and the comparisons with the serial fp64 torch CPU run of
the same configuration.  Every comparison raises AssertionError and returns
its worst error as a fraction of its bound.  A helper module like
tests/mesh_shapes.py.

The bounds are the ones of the features' serial GPU end-to-end tests against
that oracle (named at each table); fp64 ranks are also held to the serial run
of their own backend at 1e-12 of scale (test_energy_gpu.py
``test_thread_ranks_equal_serial``: the same cells, launches windowed
differently).
"""

import dataclasses
import math

import torch

from fdtd3d_amd.layout.materials import MaterialSampler
from fdtd3d_amd.models.dft import DftMonitor
from fdtd3d_amd.models.farfield import FarFieldMonitor
from fdtd3d_amd.models.flux import FluxMonitor
from fdtd3d_amd.models.probe import ProbeMonitor
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.dft import vec_width, z_pad
from mesh_shapes import octahedron
from rank_threads import DT, rank_domains

SERIAL_TOL = 1e-12  # fp64 ranks against the serial run of the same backend, of scale
_cache = {}


def serial(cfg, backend, device, setup=None, steps=True):
    """(scheme, what ``setup`` returned) of the undecomposed run."""
    s = YeeScheme(cfg, make_ops(backend, None, device, DT[cfg.dtype]))
    s.init_scheme()
    s.init_grids()
    state = setup(s) if setup is not None else None
    if steps:
        s.perform_steps()
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    return s, state


def oracle(key, cfg, setup=None, steps=True):
    """The serial fp64 torch CPU run of ``cfg``, stepped one step at a time,
    with the monitors of ``setup`` (the same sampling steps); once per key."""
    if key not in _cache:
        ref = dataclasses.replace(cfg, dtype="f64", time_block=1, hybrid_block=1)
        _cache[key] = serial(ref, "torch", "cpu", setup, steps)
        assert _cache[key][0].hybrid is None and _cache[key][0].tb == 1
    return _cache[key]


def sl(box):
    return tuple(slice(box[0][a], box[1][a]) for a in range(3))


def whole_lanes(shape, dtype):
    """Whether the z rows of an array of ``shape`` are whole 16-byte lanes."""
    return shape[2] % vec_width(DT[dtype]) == 0


def lane_mix(geometries, dtype):
    """{True, False} when, over the (size, topo, buf, align_z) ``geometries``,
    some rank's rows (ghosts and padding included) are whole 16-byte lanes and
    some rank's are not -- from the ranks' ``Domain`` shapes."""
    return {whole_lanes(d.shape, dtype) for g in geometries for d in rank_domains(*g)[1]}


def report(what, worst, bound):
    print("%s: worst error %.3g of its bound (bound %.3g)" % (what, worst / bound, bound))
    return worst / bound


def field_errors(got, want):
    """Largest difference per component of the kind's largest oracle value."""
    worst = 0.0
    for c in want:
        scale = max(float(want[o].abs().max()) for o in want if o[0] == c[0])
        assert scale > 0, c
        worst = max(worst, float((got[c].double() - want[c].double()).abs().max()) / scale)
    return worst


def gathered_fields(ranks, size):
    """Full-grid fields from the ranks' (lo, hi, {component: owned part})."""
    comps = list(ranks[0]["own"])
    full = {c: torch.full(tuple(size), float("nan"), dtype=torch.float64) for c in comps}
    for r in ranks:
        for c in comps:
            full[c][sl((r["lo"], r["hi"]))] = r["own"][c].double()
    assert not any(bool(torch.isnan(f).any()) for f in full.values()), "the ranks do not cover the grid"
    return full


def rank_fields(s):
    return {"lo": s.domain.lo, "hi": s.domain.hi, "shape": tuple(s.F[0][s.comps[0]].shape),
            "own": {c: s.owned_field(c, 0).detach().cpu().clone() for c in s.comps}}


def serial_fields(s):
    return {c: s.F[0][c].detach().cpu().double() for c in s.comps}


# ------------------------------------------------------------------------ DFT
# bounds: test_dft_gpu.py::test_dft_blocked_end_to_end, of the kind's largest value
DFT_TOL = {"f32": 2e-5, "f64": 1e-11}
DFT_WL, DFT_STEP, DFT_START = [0.02, 0.027], 2, 3
STEPPED = SchemeConfig(scheme="3d", size=(16, 14, 18), time_steps=23, scene="vacuum", use_point_source=True,
                       hybrid_block=1)
# tests/test_dft_cpu.py DECOMP_REQ
DECOMP_REQ = [("Ez", ((1, 1, 1), (7, 6, 8))),      # inside the first rank of either grid
              ("Hy", ((3, 2, 4), (13, 12, 15))),   # across every rank border
              ("Ex", ((0, 0, 0), (16, 14, 18)))]
# the geometry of test_energy_gpu.py's ``blocked`` rank case: 4-step passes, 4-deep ghosts, x split
BLOCKED = SchemeConfig(scheme="3d", size=(48, 36, 96), time_steps=24, scene="vacuum", source="gaussian",
                       gaussian_width=8.0, gaussian_delay=30.0, use_fused=True, time_block=4, hybrid_block=1)
# (the pulse travels 12 cells from the centre in 24 steps: the boxes lie around it)
BLOCKED_REQ = [("Ez", ((14, 12, 41), (22, 24, 55))), ("Hy", ((19, 10, 43), (30, 26, 55))),
               ("Ex", ((0, 0, 0), (48, 36, 96)))]
# 6 + 3 cells of z a rank: rows of 9, no whole lanes in either precision
ODD = dataclasses.replace(STEPPED, size=(16, 16, 12), time_steps=20)
ODD_REQ = [("Ez", ((1, 1, 1), (7, 6, 5))), ("Hy", ((3, 2, 2), (13, 12, 11))), ("Ex", ((0, 0, 0), (16, 16, 12)))]
# name: (cfg, requests, step, start, topo, ghost depth, align_z)
DFT_CASES = {
    "2x1x2": (STEPPED, DECOMP_REQ, DFT_STEP, DFT_START, (2, 1, 2), 1, 1),        # rows of 10
    "1x2x1": (STEPPED, DECOMP_REQ, DFT_STEP, DFT_START, (1, 2, 1), 1, 1),        # rows of 18
    "2x1x2-deep": (STEPPED, DECOMP_REQ, DFT_STEP, DFT_START, (2, 1, 2), 3, 1),   # rows of 12, owned z from 3
    "1x2x2-odd": (ODD, ODD_REQ, DFT_STEP, DFT_START, (1, 2, 2), 3, 1),           # rows of 9
    "blocked": (BLOCKED, BLOCKED_REQ, 4, 4, (2, 1, 1), 4, 4),
}


def geometry(case):
    cfg, topo, buf, align = case[0], case[-3], case[-2], case[-1]
    return (cfg.size, topo, buf, align)


def dft_setup(req, step, start):
    return lambda s: DftMonitor(s, req, DFT_WL, step=step, start=start)


def dft_collect(s, m):
    rows = []
    for i, e in enumerate(m.entries):
        rows.append({"own": m.owned_boxes[i], "empty": e.empty, "box": e.box, "acc": e.acc.detach().cpu().clone(),
                     "owned": m.accumulators(i).detach().cpu().clone(), "field_shape": tuple(e.field.shape)})
    return {"samples": m.samples, "t": s.t, "tb": s.tb, "rows": rows, "lo": s.domain.lo, "hi": s.domain.hi,
            "shape": tuple(s.F[0]["Ez"].shape), "tables": len(m.entries.tables)}


def dft_compare(ranks, ref, req, dtype, tol, exact=False):
    """Each rank's accumulators over its owned boxes against the serial
    monitor ``ref``'s slices; empty entries, padded z cells; the worst error
    of scale."""
    v = vec_width(DT[dtype])
    scale = {k: max(float(ref.accumulators(i).abs().max()) for i, (c, _) in enumerate(req) if c[0] == k)
             for k in {c[0] for c, _ in req}}
    worst, empties = 0.0, [0] * len(req)
    for r in ranks:
        assert r["samples"] == ref.samples > 0
        for i, (c, box) in enumerate(req):
            row = r["rows"][i]
            if row["empty"]:
                empties[i] += 1
                assert row["acc"].numel() == 0 and row["owned"].numel() == 0
                continue
            own = row["own"]
            assert all(r["lo"][a] <= own[0][a] < own[1][a] <= r["hi"][a] for a in range(3))
            part = tuple(slice(own[0][a] - box[0][a], own[1][a] - box[0][a]) for a in range(3))
            want = ref.accumulators(i)[(slice(None), slice(None)) + part].cpu()
            assert float(want.abs().max()) > 0 and scale[c[0]] > 0
            got = row["owned"]
            assert got.shape == want.shape
            if exact:
                assert torch.equal(got, want), (c, own)
            err = float((got.double() - want.double()).abs().max()) / scale[c[0]]
            worst = max(worst, err)
            assert err <= tol, (c, own, err, tol)
            # the padded z cells of the accumulators are never written
            z0, zp = z_pad(row["box"], v)
            assert row["acc"].shape[-1] == zp
            pad = torch.ones(zp, dtype=torch.bool)
            pad[row["box"][0][2] - z0:row["box"][1][2] - z0] = False
            assert float(row["acc"][..., pad].abs().max() if pad.any() else 0.0) == 0.0, (c, own)
    return worst, empties


def dft_straddles(req, size, topo):
    """The second box crosses every cut of ``topo``, the first none, the third
    is the whole grid."""
    cuts = [[size[a] * k // topo[a] for k in range(1, topo[a])] for a in range(3)]
    (_, first), (_, second), (_, third) = req
    assert all(first[0][a] < q < second[1][a] and second[0][a] < q for a in range(3) for q in cuts[a])
    assert all(first[1][a] <= q for a in range(3) for q in cuts[a])
    assert third == ((0, 0, 0), tuple(size))


# ------------------------------------------------------------ flux / far field
# bounds: test_flux_gpu.py::test_flux_end_to_end (of the largest face power) and
# test_farfield_gpu.py::test_farfield_end_to_end (of the peak intensity)
SURFACE_TOL = {"f32": 20 * 7.1e-7, "f64": 1e-10}
SURFACE_MARGIN = (3, 2, 4)  # tests/test_flux_cpu.py::test_flux_decomposed_equals_serial
THETAS = torch.linspace(0.0, math.pi, 5, dtype=torch.float64)
PHIS = torch.arange(8, dtype=torch.float64) * (2 * math.pi / 8)
SURFACE_TOPOS = {"2x1x2": (2, 1, 2), "1x2x1": (1, 2, 1), "1x1x2": (1, 1, 2)}


def surface_setup(s):
    flux = FluxMonitor(s, SURFACE_MARGIN, DFT_WL, step=DFT_STEP, start=DFT_START)
    far = FarFieldMonitor(s, SURFACE_MARGIN, DFT_WL, step=DFT_STEP, start=DFT_START, dft=flux.dft)
    return flux, far


def surface_collect(zero_rank=None):
    def collect(s, mons):
        flux, far = mons
        if zero_rank is not None and s.domain.rank == zero_rank:
            for e in flux.dft.entries:  # the control: this rank contributes nothing
                e.acc.zero_()
        n = [getattr(s.ops, "launches", 0)]
        res = []
        for call in (flux.power, lambda: far.intensity(THETAS, PHIS), far.total_power):
            res.append(call())
            n.append(getattr(s.ops, "launches", 0))
        nonempty = sum(1 for e in flux.dft.entries if not e.empty)
        return {"samples": flux.samples, "far_samples": far.samples, "power": res[0], "u": res[1], "total": res[2],
                "launches": [b - a for a, b in zip(n, n[1:])], "shape": tuple(s.F[0]["Ez"].shape),
                "nonempty": nonempty, "shared": far.dft is flux.dft}
    return collect


def surface_compare(ranks, want, tol):
    """Rank 0's results against (samples, power, intensity, total power) of a
    serial run; None on every other rank."""
    samples, power, u, total = want
    for r in ranks[1:]:
        assert r["power"] is None and r["u"] is None and r["total"] is None
    r = ranks[0]
    assert all(x["samples"] == x["far_samples"] == samples > 0 and x["shared"] for x in ranks)
    assert r["power"].shape == power.shape == (6, 2) and r["u"].shape == u.shape == (2, 5, 8)
    peak = float(power.abs().max())
    upeak = float(u.max())
    assert peak > 0 and upeak > 0 and float(power.abs().min()) > 0
    face = float((r["power"] - power).abs().max()) / peak
    net = float((r["power"].sum(dim=0) - power.sum(dim=0)).abs().max()) / peak
    du = float((r["u"] - u).abs().max()) / upeak
    dp = float((r["total"] - total).abs().max()) / upeak
    worst = max(face, net, du, dp)
    assert worst <= tol, (face, net, du, dp, tol)
    return worst


def surface_results(flux, far):
    return flux.samples, flux.power(), far.intensity(THETAS, PHIS), far.total_power()


# --------------------------------------------------------------------- probes
# bound: test_probe_gpu.py::test_probe_run_vs_cpu_oracle, of the kind's largest value
PROBE_TOL = {"f32": 2e-5, "f64": 1e-11}
# tests/test_probe_cpu.py PAR, PAR_POINTS, and two points either side of the cut z = 6
PROBE_CFG = SchemeConfig(scheme="3d", size=(16, 16, 12), time_steps=12, scene="vacuum", hybrid_block=1)
PROBE_POINTS = [(3, 4, 5), (7, 6, 5), (8, 6, 5), (12, 12, 9), (6, 7, 4), (6, 8, 4), (8, 8, 6), (15, 15, 11),
                (5, 5, 5), (5, 5, 6)]
PROBE_TOPOS = {"2x2x1": (2, 2, 1), "1x1x2": (1, 1, 2)}
POSITIONS = ("node", "centre")


def probe_setup(s):
    return [ProbeMonitor(s, PROBE_POINTS, position=pos, step=1) for pos in POSITIONS]


def probe_collect(zero_rank=None):
    def collect(s, mons):
        dom = s.domain
        out = {"mine": [list(m.mine) for m in mons], "shape": tuple(s.F[0]["Ez"].shape), "raw_equal": True,
               "steps": [list(m.steps) for m in mons]}
        for m in mons:
            # the raw sample of the last step is the rank's own field element: a copy, so the same bits
            n = len(m.steps)
            last = m.entries.series[n - 1].detach().cpu() if m.mine else None
            for j, slot in enumerate(m.mine):
                c, g = m.slots[slot]
                assert dom.owns(g)
                li = tuple(g[a] - dom.origin[a] for a in range(3))
                cell = s.F[0][c][li].detach().cpu().double()
                if float(cell) != float(last[j]) or math.copysign(1.0, float(cell)) != math.copysign(1.0, float(last[j])):
                    out["raw_equal"] = False
            if zero_rank is not None and dom.rank == zero_rank:
                m.entries.series.zero_()  # the control: this rank contributes nothing
        out["series"] = [m.series() for m in mons]
        return out
    return collect


def probe_ownership(ranks, groups):
    """Every slot is recorded by exactly one rank, every rank records some,
    and some centre mean adds slots of rank 0 and of another rank (the
    conditions of tests/test_probe_cpu.py)."""
    world = len(ranks)
    for i in range(len(POSITIONS)):
        cols = sorted(c for r in ranks for c in r["mine"][i])
        assert cols == list(range(len(cols))) and all(r["mine"][i] for r in ranks), world
    centre = POSITIONS.index("centre")
    assert any(0 < len(set(ranks[0]["mine"][centre]) & set(g)) < len(g) for per in groups[centre] for g in per)


def probe_compare(ranks, mons, want, tol, exact=False):
    """Rank 0's series against the serial ``want`` per kind (a point Ez source
    leaves Hz ~ 0); None elsewhere."""
    for r in ranks[1:]:
        assert r["series"] == [None] * len(POSITIONS)
    assert all(r["raw_equal"] for r in ranks), "a raw sample is not the rank's field element"
    worst = 0.0
    for m, got, w in zip(mons, ranks[0]["series"], want):
        assert got.shape == w.shape and got.shape[0] == len(m.steps) > 0
        if exact:
            assert torch.equal(got, w)
        for kind in "EH":
            cols = [i for i, c in enumerate(m.comps) if c[0] == kind]
            scale = float(w[:, :, cols].abs().max())
            assert scale > 0
            err = float((got[:, :, cols] - w[:, :, cols]).abs().max()) / scale
            worst = max(worst, err)
            assert err <= tol, (m.position, kind, err, tol)
    return worst


# ---------------------------------------------------------------- lossy media
# bound: test_lossy_gpu.py TOL, of the kind's largest value
LOSSY_TOL = {"f32": 2e-5, "f64": 1e-12}
# tests/test_lossy_cpu.py DECOMP
LOSSY = dict(scheme="3d", size=(16, 16, 12), time_steps=10, scene="file", use_fused=True,
             scene_objects=[{"shape": "sphere", "center": [8.2, 7.9, 6.1], "radius": 2.6, "eps": 2.5, "sigma": 3.0}],
             sources=[{"component": "Ez", "cell": [4, 5, 6], "waveform": "pulse", "width": 3, "delay": 5}])
LOSSY_TOPOS = {"2x1x1": (2, 1, 1), "1x2x2": (1, 2, 2)}
LOSSY_BUF = 3


def lossy_cfg(dtype):
    return SchemeConfig(dtype=dtype, hybrid_block=1, **LOSSY)


def lossy_collect(s, _):
    out = rank_fields(s)
    out.update(gbox=s.lossy["gbox"], coefs=s.lossy["coefs"] is not None, lanes=getattr(s.ops, "lossy_lanes", None),
               stepped=s.hybrid is None and s.tb == 1)
    return out


def expected_lossy_lanes(shape, dtype):
    """The instance of k_lossy_e for field rows of ``shape``: 16-byte lanes
    when they are whole lanes (the coefficients' storage box always is), one
    cell otherwise."""
    v = vec_width(DT[dtype])
    return v if shape[2] % v == 0 else 1


# ---------------------------------------------------------------- Drude scene
# bounds: test_scene_drude_gpu.py::test_damped_magnetic_run_vs_fp64_oracle, hybrid / stepped passes
DRUDE_TOL = {True: {"f32": 2e-4, "f64": 1e-11}, False: {"f32": 5e-5, "f64": 1e-10}}
# tests/test_scene_drude_cpu.py::test_decomposed_equals_serial
DRUDE_OBJECTS = [{"shape": "box", "lo": [0, 0, 0], "hi": [24, 24, 5], "eps": 2.25},
                 {"shape": "sphere", "center": [12.0, 11.5, 10.5], "radius": 3.5, "omega_p": 1.4142135, "gamma": 0.3},
                 {"shape": "sphere", "center": [13.0, 12.5, 9.5], "radius": 2.5, "omega_p": 1.0, "gamma": 0.1,
                  "omega_pm": 1.2, "gamma_m": 0.2}]
DRUDE = SchemeConfig(scheme="3d", size=(24, 24, 16), time_steps=8, scene="file", scene_objects=DRUDE_OBJECTS,
                     use_metamaterials=True, hybrid_block=3)
DRUDE_TOPO, DRUDE_BUF, DRUDE_ALIGN = (2, 2, 1), 3, 4
DRUDE_NAMES = ("b0", "b1", "b2", "ma1", "ma2")


def drude_cells(s, box=None):
    """{component: (active mask, {name: per-cell coefficient})} of the
    dispersive components over the local ``box`` (default: all), whichever
    form the backend keeps: per-cell arrays, or the uint8 index + table."""
    out = {}
    for c in s.comps:
        st = s.upml[c]
        if "D1" not in st:
            continue
        lut = st.get("_drude_lut")
        if lut is not None and lut[0] is not None:
            ids, tab = lut
            cells = {n: tab[:, q][ids.long()] for q, n in enumerate(DRUDE_NAMES)}
        else:
            cells = {n: st[n].cell for n in DRUDE_NAMES}
        assert all(v is not None and tuple(v.shape) == tuple(s.domain.shape) for v in cells.values()), c
        cut = (lambda t: t) if box is None else (lambda t: t[sl(box)])
        out[c] = (cut(st["drude_active"]).detach().cpu().clone(),
                  {n: cut(v).detach().cpu().clone() for n, v in cells.items()})
    return out


def drude_collect(s, _):
    dom = s.domain
    out = rank_fields(s)
    out.update(hybrid=s.hybrid is not None, cells=drude_cells(s, dom.to_local(dom.owned_global())))
    return out


def drude_tables_agree(ranks, ser):
    """The ranks' Drude coefficients on their owned cells are the serial
    run's: the same bits, the same dispersive cells."""
    want = drude_cells(ser)
    kinds = set()
    for r in ranks:
        assert set(r["cells"]) == set(want)
        box = (r["lo"], r["hi"])
        for c, (active, cells) in r["cells"].items():
            assert torch.equal(active, want[c][0][sl(box)]), c
            for n in DRUDE_NAMES:
                assert torch.equal(cells[n], want[c][1][n][sl(box)]), (c, n)
            if bool(active.any()):
                kinds.add(c[0])
    assert kinds == {"E", "H"}, "no dispersive cells of a kind on any rank"


# ---------------------------------------------------------------- scene grids
def scene_objects():
    """A box, a sphere, a cylinder and a closed mesh, every one across the
    point (8, 7, 9) -- the cuts of 2 x 1 x 2 and 1 x 2 x 1 ranks of a 16 x 14
    x 18 grid -- with eps + sigma, omega + gamma and omega_pm + gamma_m."""
    v, t = octahedron((8.3, 7.2, 8.8), 3.6)
    return [{"shape": "box", "lo": [5.3, 4.2, 6.6], "hi": [10.7, 9.4, 11.2], "eps": 2.25, "sigma": 3.0},
            {"shape": "sphere", "center": [8.2, 7.4, 9.3], "radius": 3.37, "eps": 4.0, "omega_p": 1.2, "gamma": 0.3},
            {"shape": "cylinder", "axis": "z", "center": [7.6, 6.8], "radius": 2.3, "span": [4.4, 13.7],
             "omega_p": 1.0, "gamma": 0.1, "omega_pm": 1.2, "gamma_m": 0.2},
            {"shape": "mesh", "vertices": v, "triangles": t, "eps": 3.0, "sigma": 1.5}]


def object_bbox(o):
    if o["shape"] == "box":
        return o["lo"], o["hi"]
    if o["shape"] == "sphere":
        return [v - o["radius"] for v in o["center"]], [v + o["radius"] for v in o["center"]]
    if o["shape"] == "cylinder":
        assert o["axis"] == "z"
        return ([o["center"][0] - o["radius"], o["center"][1] - o["radius"], o["span"][0]],
                [o["center"][0] + o["radius"], o["center"][1] + o["radius"], o["span"][1]])
    vs = o["vertices"]
    return [min(p[a] for p in vs) for a in range(3)], [max(p[a] for p in vs) for a in range(3)]


SCENE_SIZE = (16, 14, 18)
SCENE_CASES = {"2x1x2-deep": ((2, 1, 2), 3), "1x2x1": ((1, 2, 1), 1)}
GRIDS = ("eps", "cond", "omega_pe", "gamma_e", "omega_pm", "gamma_m")


def scene_cfg(smoothing, dtype):
    return SchemeConfig(scheme="3d", size=SCENE_SIZE, time_steps=1, scene="file", scene_objects=scene_objects(),
                        scene_smoothing=smoothing, dtype=dtype, hybrid_block=1)


def scene_calls(s):
    """(label, call on a sampler, scene_sample launches it makes) of every
    material grid a scheme may ask its sampler for."""
    calls = [("grid " + n, (lambda smp, n=n: smp.grid(n)), 1) for n in GRIDS]
    for c in s.e_comps:
        calls.append(("eps at " + c, (lambda smp, c=c: smp.averaged(c, "eps")), 1))
        calls.append(("cond at " + c, (lambda smp, c=c: smp.averaged(c, "cond")), 1))
    for c in s.comps:
        for n, which in (("omega", 0), ("gamma", 1)):
            calls.append(("%s at %s" % (n, c),
                          (lambda smp, c=c, which=which: smp.averaged_drude(c, c[0] == "E")[which]), 2))
    return calls


def scene_collect(s, _):
    """Every grid from the rank's own sampler (the scheme's: its backend's
    ``scene_sample``) and from the torch oracle with the rank's origin and
    shape; the launches each call made."""
    dom = s.domain
    mine = s.sampler
    ref = MaterialSampler(s.layout, s.scene, dom.origin, dom.shape, "cpu", ops=make_ops("torch", None, "cpu",
                                                                                          torch.float64))
    assert mine.origin == tuple(dom.origin) and mine.shape == tuple(dom.shape)
    grids, launches = {}, {}
    for label, call, n in scene_calls(s):
        mine.free()
        before = getattr(s.ops, "launches", None)
        got = call(mine)
        if before is not None:
            launches[label] = (s.ops.launches - before, n)
        assert got.dtype == torch.float64 and str(got.device).startswith(str(torch.device(s.device).type))
        ref.free()
        grids[label] = (got.detach().cpu().clone(), call(ref))
    mine.free()
    return {"origin": tuple(dom.origin), "shape": tuple(dom.shape), "lo": dom.lo, "hi": dom.hi, "grids": grids,
            "launches": launches, "lossy": s.lossy is not None and s.lossy["gbox"]}


def scene_compare(ranks, ser):
    """Bit for bit: rank == the oracle on the rank's region == the window of
    the serial oracle's grid; no grid is constant on every rank."""
    varied = set()
    whole = MaterialSampler(ser.layout, ser.scene, (0, 0, 0), tuple(ser.cfg.size), "cpu",
                            ops=make_ops("torch", None, "cpu", torch.float64))
    for label, call, _ in scene_calls(ser):
        whole.free()
        full = call(whole)
        for r in ranks:
            got, want = r["grids"][label]
            assert got.shape == want.shape and torch.equal(got, want), (label, r["origin"])
            o = r["origin"]
            window = full[tuple(slice(o[a], o[a] + got.shape[a]) for a in range(3))]
            assert torch.equal(got, window), (label, r["origin"], "not the serial grid's window")
            own = tuple(slice(r["lo"][a] - o[a], r["hi"][a] - o[a]) for a in range(3))
            assert torch.equal(got[own], full[sl((r["lo"], r["hi"]))]), (label, r["origin"])
            if len(torch.unique(got)) >= 2:
                varied.add(label)
            if r["launches"]:
                made, n = r["launches"][label]
                assert made == n, (label, made, n)
    assert varied == {label for label, _, _ in scene_calls(ser)}, "a grid is trivial on every rank"


def objects_straddle(objs, size, topo):
    cuts = [[size[a] * k // topo[a] for k in range(1, topo[a])] for a in range(3)]
    for o in objs:
        lo, hi = object_bbox(o)
        assert all(lo[a] + 1 < q < hi[a] - 1 for a in range(3) for q in cuts[a]), (o["shape"], cuts)
