"""Lossy media (scene-file key ``sigma``) on the torch fp64 oracle: the format
and its refusals, the painting rule of ``scene_sample(..., "cond", ...)``, the
exact discrete decay of a cavity mode, the hybrid plan, decomposed runs and
the runs that must not change.  Kernel tests: test_lossy_gpu.py.
"""

import io
import json
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fdtd3d_amd.layout.materials import Scene
from fdtd3d_amd.layout.scene_file import QUANTITIES, SceneTable, build_table, parse_object
from fdtd3d_amd.layout.yee import MATERIAL_STENCIL
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.torch_ops import TorchOps
from fdtd3d_amd.parallel.domain import box_empty, box_intersect
from fdtd3d_amd.parallel.halo import HaloExchanger, gather_field
from fdtd3d_amd.parallel.topology import ParallelGridCore
from fdtd3d_amd.utils.assertions import FdtdError
from fdtd3d_amd.utils.constants import EPS0

GOOD = {"shape": "sphere", "center": [4, 4, 4], "radius": 2}


def scheme(cfg, init=True):
    s = YeeScheme(cfg, make_ops("torch", None, "cpu", torch.float64))
    if init:
        s.init_scheme()
        s.init_grids()
    return s


# ------------------------------------------------------------------ the format
BAD = [(dict(GOOD, sigma=-0.1), "sigma must not be negative"),
       (dict(GOOD, sigma=float("inf")), "sigma must be finite"),
       (dict(GOOD, sigma=float("nan")), "sigma must be finite"),
       (dict(GOOD, sigma="1"), "sigma must be a number"),
       (dict(GOOD, sigma=0.5, omega_p=1.0), "sigma and omega_p on one object")]


@pytest.mark.parametrize("obj,msg", BAD, ids=range(len(BAD)))
def test_format_refusals(obj, msg, monkeypatch):
    def no_alloc(*a, **k):
        raise AssertionError("allocated before the refusal")
    for f in ("zeros", "empty", "full", "ones", "arange"):
        monkeypatch.setattr(torch, f, no_alloc)
    with pytest.raises(ValueError, match=msg):
        Scene(kind="file", objects=[GOOD, obj])
    with pytest.raises(ValueError, match=msg):
        scheme(SchemeConfig(scheme="3d", size=(8, 8, 8), scene="file", scene_objects=[obj]))


@pytest.mark.parametrize("kw,msg", [(dict(scheme="tmz", size=(8, 8, 1)), "sigma needs a 3D scheme"),
                                    (dict(scheme="1d", size=(8, 1, 1)), "file scenes need a 2D or 3D scheme"),
                                    (dict(complex_values=True), "--complex-field-values"),
                                    (dict(use_amp_mode=True), "--use-amp-mode"),
                                    (dict(use_hip_graph=True), "--use-hip-graph")])
def test_scheme_and_option_refusals(kw, msg, monkeypatch):
    def no_alloc(*a, **k):
        raise AssertionError("allocated before the refusal")
    for f in ("zeros", "empty", "full", "ones", "arange"):
        monkeypatch.setattr(torch, f, no_alloc)
    base = dict(scheme="3d", size=(8, 8, 8), scene="file", scene_objects=[dict(GOOD, sigma=0.5)])
    base.update(kw)
    with pytest.raises((ValueError, FdtdError), match=msg):
        scheme(SchemeConfig(**base))
    # sigma = 0 is no lossy medium: the options are free
    if "scheme" not in kw:
        scheme(SchemeConfig(**dict(base, scene_objects=[dict(GOOD, sigma=0.0)])), init=False)


def test_quantity_names_and_table():
    assert QUANTITIES[-1] == "cond" and "sigma" not in QUANTITIES
    assert parse_object(dict(GOOD, sigma=2.5)).sigma == 2.5 and parse_object(GOOD).sigma == 0.0
    tab = build_table([dict(GOOD, sigma=2.5), GOOD])
    assert tab.cond.dtype == np.float64 and tab.cond.tolist() == [2.5, 0.0] and tab.drude.shape == (2, 3)
    assert SceneTable(tab.ents, tab.tris, tab.ranges, tab.drude).cond.tolist() == [0.0, 0.0]
    ops = TorchOps(None, "cpu", torch.float64)
    ops.scene_sample(tab, "cond", [(0, 0, 0)], (0, 0, 0), (4, 4, 4), (1, 1, 1), 1.0)
    with pytest.raises(ValueError):
        ops.scene_sample(tab, "sigma", [(0, 0, 0)], (0, 0, 0), (4, 4, 4), (1, 1, 1), 1.0)
    for bad in (np.zeros(3), np.zeros((2, 1)), np.zeros(2, dtype=np.float32), np.array([1.0, -1.0]),
                np.array([1.0, np.nan])):
        with pytest.raises(ValueError, match="cond"):
            SceneTable(tab.ents, tab.tris, tab.ranges, tab.drude, bad)
    assert Scene(kind="file", objects=[GOOD]).uniform("cond") == 0.0
    assert Scene(kind="file", objects=[dict(GOOD, sigma=1.0)]).uniform("cond") is None
    assert Scene(kind="vacuum").uniform("cond") == 0.0


# ------------------------------------------------------------- the painting rule
def _octahedron(c, r):
    v = [[c[0] + r, c[1], c[2]], [c[0] - r, c[1], c[2]], [c[0], c[1] + r, c[2]], [c[0], c[1] - r, c[2]],
         [c[0], c[1], c[2] + r], [c[0], c[1], c[2] - r]]
    t = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return v, t


def _dist(o, p):
    """The signed distance of the module's doc string, per point, in plain
    Python floats (box, sphere, cylinder; the octahedron |x| + |y| + |z| <= r
    by the distance to its closest face plane, which is its distance inside
    and a lower bound outside: None where the two may differ under
    smoothing, just outside the surface)."""
    if o["shape"] == "box":
        return max(max(o["lo"][a] - p[a], p[a] - o["hi"][a]) for a in range(3))
    if o["shape"] == "sphere":
        return float(np.sqrt(sum((p[a] - o["center"][a]) ** 2 for a in range(3)))) - o["radius"]
    if o["shape"] == "cylinder":
        ax = "xyz".index(o["axis"])
        b, c = [a for a in range(3) if a != ax]
        d = float(np.sqrt((p[b] - o["center"][0]) ** 2 + (p[c] - o["center"][1]) ** 2)) - o["radius"]
        return max(d, o["span"][0] - p[ax], p[ax] - o["span"][1])
    c, r = o["_octa"]
    d = (sum(abs(p[a] - c[a]) for a in range(3)) - r) / np.sqrt(3.0)
    return None if 0.0 <= d <= 0.5 else d


@pytest.mark.parametrize("smoothing", ["linear", "none"])
def test_painting_rule(smoothing):
    """cond at single points against a direct evaluation of the rule of eps:
    overlapping box / sphere / cylinder / mesh objects across the region's
    faces; a later object without sigma paints 0."""
    origin, shape = (3, -2, 5), (7, 6, 8)
    lo = [float(o) for o in origin]
    hi = [float(o + s) for o, s in zip(origin, shape)]
    mid = [(a + b) / 2 + 0.13 for a, b in zip(lo, hi)]
    oc = ((mid[0] - 0.4, mid[1] + 0.2, mid[2] - 0.6), 2.7)
    v, t = _octahedron(*oc)
    objs = [{"shape": "box", "lo": [lo[0] - 2.3, lo[1] - 1.7, lo[2] - 3.1], "hi": [lo[0] + 2.37, mid[1], mid[2]],
             "eps": 2.25, "sigma": 0.7},
            {"shape": "sphere", "center": [mid[0], lo[1] - 0.3, mid[2]], "radius": 2.37, "eps": 5.0, "sigma": 2.5},
            {"shape": "mesh", "vertices": v, "triangles": t, "sigma": 1.1},
            {"shape": "sphere", "center": [hi[0] - 0.7, hi[1] + 0.37, lo[2] + 1.3], "radius": 3.37, "eps": 1.7},
            {"shape": "cylinder", "axis": "x", "center": [hi[1] - 0.37, mid[2] + 1.3], "radius": 1.73,
             "span": [lo[0] - 1.3, mid[0] + 0.37], "sigma": 0.05}]
    tab = build_table(objs, "3d", smoothing, 1.0)
    got = TorchOps(None, "cpu", torch.float64).scene_sample(tab, "cond", [(0, 0, 0)], origin, shape, (1, 1, 1), 1.0)
    objs[2]["_octa"] = oc
    worst, seen, skipped = 0.0, set(), 0
    for i in range(shape[0]):
        for j in range(shape[1]):
            for k in range(shape[2]):
                p = (origin[0] + i + 0.5, origin[1] + j + 0.5, origin[2] + k + 0.5)
                val = 0.0
                dists = [_dist(o, p) for o in objs]
                if smoothing == "linear" and any(d is None for d in dists):
                    skipped += 1  # (the Euclidean mesh distance itself: test_mesh_cpu.py)
                    continue
                for o, d in zip(objs, dists):
                    d, sg = (0.25 if d is None else d), float(o.get("sigma", 0.0))
                    if smoothing == "none":
                        val = sg if d < 0 else val
                    elif d < -0.5:
                        val = sg
                    elif d <= 0.5:
                        prop = 0.5 - d
                        val = prop * sg + (1 - prop) * val
                worst = max(worst, abs(val - float(got[i, j, k])))
                seen.add(round(val, 6))
    assert worst <= 1e-12, worst
    assert skipped <= 0.15 * shape[0] * shape[1] * shape[2], skipped
    assert len(seen) >= (5 if smoothing == "none" else 20), "trivial scene"


def test_sphere_only_scene_keeps_its_arrays():
    """cond / sigma == (eps_array - 1) / (eps - 1) for a sphere-only scene:
    one rule, one distance, one averaging."""
    obj = {"shape": "sphere", "center": [6.3, 5.8, 6.1], "radius": 3.4, "eps": 3.0, "sigma": 0.25}
    tab = build_table([obj], "3d", "linear", 1.0)
    ops = TorchOps(None, "cpu", torch.float64)
    for comp in ("Ex", "Ey", "Ez"):
        pts = list(MATERIAL_STENCIL[comp])
        cond = ops.scene_sample(tab, "cond", pts, (0, 0, 0), (12, 12, 12), (1, 1, 1), 1.0)
        eps = ops.scene_sample(tab, "eps", pts, (0, 0, 0), (12, 12, 12), (1, 1, 1), 1.0)
        assert float(cond.max()) == 0.25 and float(cond.min()) == 0.0
        assert float((cond / 0.25 - (eps - 1) / 2.0).abs().max()) <= 1e-14


# ------------------------------------------------------------ exact discrete decay
# (a source list of one silent entry: the built-in hard point source would drive the cavity)
CAVITY = dict(scheme="3d", size=(12, 10, 9), time_steps=200, dtype="f64", scene="file", use_fused=True,
              sources=[{"component": "Ez", "cell": [6, 5, 4], "waveform": "gaussian", "amplitude": 0.0}])


def _filled(**medium):
    return [dict({"shape": "box", "lo": [-2, -2, -2], "hi": [14, 12, 11]}, **medium)]


def _seed(s):
    nx, ny, nz = s.cfg.size
    x = torch.arange(nx, dtype=torch.float64).view(-1, 1, 1)
    y = torch.arange(ny, dtype=torch.float64).view(1, -1, 1)
    # the discrete eigenmode of the grid's walls: Ez = 0 at index 0; past the last index there is no Ez and the
    # H between stays 0, which mirrors the mode about n - 1/2
    mode = (torch.sin(np.pi * x / (2 * nx - 1)) * torch.sin(np.pi * y / (2 * ny - 1))
            * torch.ones(1, 1, nz, dtype=torch.float64))
    b = s.local_box("Ez")
    sl = tuple(slice(b[0][d], b[1][d]) for d in range(3))
    s.F[0]["Ez"][sl] = mode[sl]


def test_exact_discrete_decay():
    """A uniformly lossy cavity seeded with an Ez = sin sin pattern and H = 0.
    The leapfrog with E' = ca E + cb curl H gives, at every cell and step,

        E[n+1] + ca E[n-1] = (1 + ca) E[n] - (cb / cb0) M E[n],

    M = cb0 db curl curl being the lossless grid's own operator (applied here
    with the plain ops of the same scene without sigma).  For an eigenmode of
    M this is E[n+1] + ca E[n-1] = k E[n] with one k; the grid's walls (PEC at
    index 0, a mirror past the last index) admit no mode of Ez alone, so the
    identity is checked in its operator form, on the whole field (every cell
    of every E component), to 1e-9 of the field's amplitude over 200 steps."""
    eps, sigma = 2.0, 0.4
    s = scheme(SchemeConfig(scene_objects=_filled(eps=eps, sigma=sigma), **CAVITY))
    p = scheme(SchemeConfig(scene_objects=_filled(eps=eps), **CAVITY))
    assert s.lossy is not None and not s.fused and s.tb == 1 and s.hybrid is None and p.lossy is None
    sh = sigma * s.dt / (2 * EPS0 * eps)
    ca = (1 - sh) / (1 + sh)
    assert abs(float(s.lossy["coefs"].ca["Ez"].min()) - ca) <= 1e-15 and 0.5 < ca < 0.99
    ratio = 1 / (1 + sh)  # cb / cb0
    _seed(s)
    eb = {c: s.local_box(c) for c in s.e_comps}
    hb = {c: s.local_box(c) for c in s.h_comps}

    def minus_m(E):
        f = {c: torch.zeros_like(E["Ez"]) for c in s.comps}
        f.update({c: E[c] for c in s.e_comps})
        p.ops.curl_update("H", hb, f, f, p.cb)
        out = {c: torch.zeros_like(E["Ez"]) for c in s.e_comps}
        f.update(out)
        p.ops.curl_update("E", eb, f, f, p.cb)
        return {c: f[c] for c in s.e_comps}

    hist = [{c: s.F[0][c].clone() for c in s.e_comps}]
    worst, amp = 0.0, float(hist[0]["Ez"].abs().max())
    for n in range(200):
        s.advance(1)
        hist.append({c: s.F[0][c].clone() for c in s.e_comps})
        if len(hist) == 3:
            lo, mid, hi = hist
            mm = minus_m(mid)
            for c in s.e_comps:
                res = hi[c] + ca * lo[c] - (1 + ca) * mid[c] - ratio * mm[c]
                worst = max(worst, float(res.abs().max()))
            hist.pop(0)
    print("worst residual %.3g of amplitude %.3g" % (worst, amp))
    assert worst <= 1e-9 * amp, (worst, amp)
    assert float(s.F[0]["Ez"].abs().max()) < 0.5 * amp  # it decays


def test_sigma_zero_is_the_scene_without_the_key():
    runs = []
    for medium in (dict(eps=2.0, sigma=0.0), dict(eps=2.0)):
        s = scheme(SchemeConfig(scene_objects=_filled(**medium), **dict(CAVITY, time_steps=20)))
        assert s.lossy is None
        _seed(s)
        s.advance(20)
        runs.append(s)
    for c in runs[0].comps:
        assert torch.equal(runs[0].F[0][c], runs[1].F[0][c]), c


# ------------------------------------------------------------------ Poynting balance
PERIOD = 80        # steps of the default wavelength 0.02 at dx = 0.0005, Courant 0.5
START, PERIODS = 240, 2   # the window of tests/test_flux_cpu.py's scatterer runs: a damped sphere has settled
# Measured on the CPU (fp64), relative gap |absorbed - loss| / loss between the flux box's absorbed power and
# 1/2 sum sigma |E|^2 dx^3 from the DFT phasors: the two differ by the staggering of the three E components
# against the flux faces and by the time centring of E (the update's loss term takes (E' + E) / 2).  Over 4
# periods from step 400 the gap is 0.0041.  The control (sigma = 0) reports 2.9e-5 of the lossy sphere's power.
GAP_MEASURED = {"cpml": 0.004528, "upml": 0.005083}
FLOOR_MEASURED = 2.85e-5


def _balance(sigma, pml_type):
    """(absorbed power through the flux box, volume loss, scheme) of the
    README absorber's 28^3 grid around a lossy dielectric sphere (eps 3,
    radius 3; sigma 3.2 S/m is s = 0.05).  The TF/SF box is 7 cells, not the
    README's 9: the lossy box (cells 10 to 16) must stay 2 cells clear of the
    TF/SF cells; the flux box (9) lies inside it and around the whole sphere."""
    from fdtd3d_amd.layout.materials import MaterialSampler
    from fdtd3d_amd.models.dft import DftMonitor
    from fdtd3d_amd.models.flux import FluxMonitor
    obj = {"shape": "sphere", "center": [14.0, 14.0, 14.0], "radius": 3.0, "eps": 3.0, "sigma": sigma}
    cfg = SchemeConfig(time_steps=START + PERIOD * PERIODS, scheme="3d", size=(28, 28, 28), pml_size=(5, 5, 5),
                       tfsf_size=(7, 7, 7), use_pml=True, pml_type=pml_type, use_tfsf=True, scene="file",
                       scene_objects=[obj], dtype="f64")
    s = scheme(cfg)
    flux = FluxMonitor(s, (9, 9, 9), [cfg.wavelength], step=1, start=START + 1)
    box = ((9, 9, 9), (19, 19, 19))
    dft = DftMonitor(s, [(c, box) for c in s.e_comps], [cfg.wavelength], step=1, start=START + 1)
    s.perform_steps()
    assert flux.label == "absorbed"
    smp = MaterialSampler(s.layout, s.scene, (0, 0, 0), cfg.size, "cpu")
    loss = 0.0
    for c in s.e_comps:
        sg = smp.averaged(c, "cond")[9:19, 9:19, 9:19]   # the component-averaged sigma
        loss += 0.5 * float((sg * dft.phasor(c).abs() ** 2).sum()) * s.dx ** 3
    return -float(flux.net()[0]), loss, s


@pytest.mark.parametrize("pml_type", ["cpml", "upml"])
def test_poynting_balance(pml_type):
    """The power the flux box sees vanish equals the ohmic loss in the
    sphere: an independent check of the averaged sigma, of (ca, cb) on a
    smoothed sphere and of the E windows cut around the box beside CPML (the
    folded kernels) or UPML (the chain regions) and TF/SF.  Asserted at twice
    the measured gap; a gap above 10 % would be a defect."""
    absorbed, loss, s = _balance(3.2, pml_type)
    assert s.lossy is not None and s.lossy["gbox"] == ((10, 10, 10), (17, 17, 17))
    assert 0.90 < float(s.lossy["coefs"].ca["Ez"].min()) < 0.91   # s about 0.05: ca = 0.95 / 1.05
    gap = abs(absorbed - loss) / loss
    print("%s: absorbed %.9g W, loss %.9g W, gap %.4g (measured %.4g)"
          % (pml_type, absorbed, loss, gap, GAP_MEASURED[pml_type]))
    assert absorbed > 0 and loss > 0
    assert gap <= 2 * GAP_MEASURED[pml_type] < 0.1, gap
    if pml_type == "cpml":
        control, zero, s0 = _balance(0.0, pml_type)
        print("control: absorbed %.3g W, %.3g of the lossy sphere's (measured %.3g)"
              % (control, abs(control) / absorbed, FLOOR_MEASURED))
        assert s0.lossy is None and zero == 0.0
        assert abs(control) <= 2 * FLOOR_MEASURED * absorbed


def test_upml_hybrid_equals_stepped():
    """A lossy run whose absorbing layers run the D/B chain: the chain boxes
    run whole, the plain slabs are cut to the windows minus the lossy box."""
    base = dict(PLAN, pml_type="upml", time_steps=6)
    h = scheme(SchemeConfig(hybrid_block=2, **base))
    s = scheme(SchemeConfig(hybrid_block=1, time_block=1, **base))
    assert h.hybrid is not None and s.hybrid is None and h.lossy is not None and h.use_upml_chain
    for r in (h, s):
        r.perform_steps()
    assert float(s.F[0]["Ez"].abs().max()) > 0
    for c in s.comps:
        assert torch.equal(h.F[0][c], s.F[0][c]), c


# ------------------------------------------------------------------ the plan
SPHERE = [{"shape": "sphere", "center": [22.3, 23.1, 21.7], "radius": 3.2, "eps": 3.0, "sigma": 4.0}]
PLAN = dict(scheme="3d", size=(44, 46, 44), time_steps=8, dtype="f64", use_pml=True, pml_type="cpml",
            pml_size=(4, 4, 4), scene="file", scene_objects=SPHERE, use_fused=True)


def test_hybrid_plan_and_passes():
    T = 2
    h = scheme(SchemeConfig(hybrid_block=T, **PLAN))
    assert h.lossy is not None and h.hybrid is not None and h.hybrid["T"] == T and h.hybrid["cut_cells"] > 0
    lo, hi = h.lossy["gbox"]
    grown = (tuple(v - (T + 1) for v in lo), tuple(v + (T + 1) for v in hi))
    for b in h.hybrid["core"]:
        assert box_empty(box_intersect(grown, b)), b
    s = scheme(SchemeConfig(hybrid_block=1, time_block=1, **PLAN))
    assert s.hybrid is None and s.lossy is not None
    for r in (h, s):
        r.perform_steps()
    assert float(s.F[0]["Ez"].abs().max()) > 0
    for c in s.comps:
        assert torch.equal(h.F[0][c], s.F[0][c]), c


def test_setup_refusals():
    near_pml = [{"shape": "box", "lo": [4.2, 10, 10], "hi": [9, 14, 14], "sigma": 1.0}]
    with pytest.raises(FdtdError, match="touches the absorbing layer"):
        scheme(SchemeConfig(**dict(PLAN, size=(24, 24, 24), scene_objects=near_pml)))
    near_tfsf = [{"shape": "box", "lo": [8.2, 10, 10], "hi": [12, 14, 14], "sigma": 1.0}]
    with pytest.raises(FdtdError, match="within 2 cells of a TF/SF face"):
        scheme(SchemeConfig(**dict(PLAN, size=(24, 24, 24), scene_objects=near_tfsf, use_tfsf=True,
                                   tfsf_size=(7, 7, 7))))
    # a Drude object next to a lossy one under --use-metamaterials: its dispersive box runs the D/B chain
    beside = [{"shape": "box", "lo": [9.2, 10, 10], "hi": [12, 14, 14], "sigma": 1.0},
              {"shape": "box", "lo": [12.2, 10, 10], "hi": [15, 14, 14], "omega_p": 1.2}]
    with pytest.raises(FdtdError, match="touches a box advanced by the D/B chain"):
        scheme(SchemeConfig(**dict(PLAN, size=(24, 24, 24), scene_objects=beside, pml_type="upml",
                                   use_metamaterials=True)))


# --------------------------------------------------------------- unchanged runs
def test_scene_without_sigma_takes_no_lossy_pass(monkeypatch):
    calls = []
    real = TorchOps.curl_update_lossy

    def counting(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(TorchOps, "curl_update_lossy", counting)
    plain = [dict(o, sigma=0.0) for o in SPHERE]
    s = scheme(SchemeConfig(hybrid_block=1, time_block=1, **dict(PLAN, size=(24, 24, 24), scene_objects=plain,
                                                                 time_steps=4)))
    s.perform_steps()
    assert s.lossy is None and not calls
    lossy = [dict(SPHERE[0], center=[12, 12, 12])]
    s = scheme(SchemeConfig(hybrid_block=1, time_block=1, **dict(PLAN, size=(24, 24, 24), scene_objects=lossy,
                                                                 time_steps=4)))
    s.perform_steps()
    assert s.lossy is not None and len(calls) == 4  # once per E half step


# ------------------------------------------------------------- decomposed == serial
DECOMP = dict(scheme="3d", size=(16, 16, 12), time_steps=10, dtype="f64", scene="file", use_fused=True,
              scene_objects=[{"shape": "sphere", "center": [8.2, 7.9, 6.1], "radius": 2.6, "eps": 2.5, "sigma": 3.0}],
              sources=[{"component": "Ez", "cell": [4, 5, 6], "waveform": "pulse", "width": 3, "delay": 5}])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, cfg, topo, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        axes = "".join("xyz"[a] for a in range(3) if topo[a] > 1)
        core = ParallelGridCore.create(cfg.size, world, axes, topo, optimal=False, active_axes=(0, 1, 2))
        dom = core.domain(rank, 3, align_z=1, align_axis=2)
        halo = HaloExchanger(dom)
        s = YeeScheme(cfg, make_ops("torch", None, "cpu", torch.float64), dom, halo)
        s.init_scheme()
        s.init_grids()
        assert s.hybrid is None and s.tb == 1 and s.lossy is not None
        gbox = [None] * world
        dist.all_gather_object(gbox, s.lossy["gbox"])
        s.perform_steps()
        halo.drain(s)
        res = {c: gather_field(s, c, 0) for c in s.comps}
        if rank == 0:
            res["gbox"] = gbox
            torch.save(res, os.path.join(outdir, "par.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("topo", [(2, 1, 1), (1, 2, 2)], ids=["2x1x1", "1x2x2"])
def test_decomposed_equals_serial(topo):
    cfg = SchemeConfig(**DECOMP)
    ser = scheme(cfg)
    ser.perform_steps()
    lo, hi = ser.lossy["gbox"]
    assert all(lo[a] < cfg.size[a] // 2 < hi[a] for a in range(3) if topo[a] > 1), "the box straddles the cut"
    world = topo[0] * topo[1] * topo[2]
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(world, _free_port(), cfg, topo, d), nprocs=world, join=True)
        par = torch.load(os.path.join(d, "par.pt"), weights_only=False)
    assert all(g == ser.lossy["gbox"] for g in par["gbox"])
    assert float(ser.F[0]["Hx"].abs().max()) > 0
    for c in ser.comps:
        assert torch.equal(par[c], ser.F[0][c]), c


# ------------------------------------------------------------------- the driver
def test_driver_json_materials_and_checkpoint(tmp_path):
    from fdtd3d_amd.runner import run as drive
    p = tmp_path / "scene.json"
    p.write_text(json.dumps({"objects": [dict(SPHERE[0], center=[10, 10, 10]), dict(GOOD, eps=2.0)]}))
    base = ["--3d", "--sizex", "20", "--same-size", "--backend", "torch", "--device", "cpu", "--dtype", "f64",
            "--use-pml", "--pml-type", "cpml", "--pml-sizex", "3", "--same-size-pml", "--scene", "file",
            "--scene-file", str(p), "--json"]

    def go(extra, where):
        os.makedirs(where, exist_ok=True)
        out = io.StringIO()
        assert drive(base + ["--output-dir", str(where)] + extra, out=out) == 0, out.getvalue()
        return json.loads(out.getvalue().strip().splitlines()[-1])

    rec = go(["--time-steps", "20", "--save-materials", "--save-as-txt", "--save-res"], tmp_path / "full")
    assert rec["scene"]["lossy"] == 1 and rec["scene"]["objects"] == 2
    names = os.listdir(tmp_path / "full")
    assert any("SigmaE" in n for n in names), names
    # a run resumed from a checkpoint equals the uninterrupted one
    go(["--time-steps", "12", "--checkpoint-dir", str(tmp_path / "ck"), "--checkpoint-step", "12"], tmp_path / "a")
    go(["--time-steps", "20", "--load-from-file", str(tmp_path / "ck"), "--save-as-txt", "--save-res"],
       tmp_path / "resumed")
    compared = 0
    for n in sorted(os.listdir(tmp_path / "full")):
        if n.startswith("current[20]") and "Sigma" not in n and "Eps" not in n and "Mu" not in n:
            assert (tmp_path / "full" / n).read_bytes() == (tmp_path / "resumed" / n).read_bytes(), n
            compared += 1
    assert compared >= 6, sorted(os.listdir(tmp_path / "full"))  # the six field components
