"""File scenes on the CPU: the torch ``scene_sample`` op against a scalar
reference written here, equivalence with the built-in sphere scenes, painter's
order, 2D, the refusals of the format and the options, decomposed runs."""

import io
import json
import math
import os
import subprocess
import threading

import pytest
import torch

from fdtd3d_amd import native
from fdtd3d_amd.layout.materials import SQRT2_F32, MaterialSampler, Scene
from fdtd3d_amd.layout.scene_file import SCENE_MAX_OBJECTS, build_table, load_scene_file, parse_objects
from fdtd3d_amd.layout.yee import MATERIAL_STENCIL, MATERIAL_STENCIL_DOUBLE
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.parallel.comm import LocalHub
from fdtd3d_amd.parallel.halo import HaloExchanger
from fdtd3d_amd.parallel.topology import ParallelGridCore
from fdtd3d_amd.utils.settings import SettingsError, setup_from_cmd

FREQ = 1.5e10


def make(cfg, domain=None, halo=None, dtype=torch.float64):
    s = YeeScheme(cfg, make_ops("torch", None, "cpu", dtype), domain, halo)
    s.init_scheme()
    s.init_grids()
    return s


# ------------------------------------------------------- the scalar reference
def ref_distance(o, p, mod):
    """Signed distance of point p from the object dictionary o (section
    'Signed distances' of the format), one rounded operation at a time."""
    if o["shape"] == "sphere":
        c, r = [v * mod for v in o["center"]], o["radius"] * mod
        return math.sqrt(((p[0] - c[0]) ** 2 + (p[1] - c[1]) ** 2) + (p[2] - c[2]) ** 2) - r
    if o["shape"] == "box":
        lo, hi = [v * mod for v in o["lo"]], [v * mod for v in o["hi"]]
        return max(max(lo[a] - p[a], p[a] - hi[a]) for a in range(3))
    a = "xyz".index(o["axis"])
    b, c = [d for d in range(3) if d != a]
    db, dc = p[b] - o["center"][0] * mod, p[c] - o["center"][1] * mod
    return max(math.sqrt(db * db + dc * dc) - o["radius"] * mod,
               max(o["span"][0] * mod - p[a], p[a] - o["span"][1] * mod))


def ref_point(objects, quantity, p, mod, smoothing="linear", freq=FREQ):
    val = 1.0 if quantity == "eps" else 0.0
    for o in objects:
        d = ref_distance(o, p, mod)
        if quantity == "omega":
            if d < 0:
                val = o.get("omega_p", 0.0) * 2 * math.pi * freq
        elif smoothing == "none":
            if d < 0:
                val = o.get("eps", 1.0)
        elif d < -0.5:
            val = o.get("eps", 1.0)
        elif not d > 0.5:
            prop = 0.5 - d
            val = prop * o.get("eps", 1.0) + (1 - prop) * val
    return val


def ref_mean(v):
    if len(v) == 1:
        return v[0]
    h = len(v) // 2
    return (ref_mean(v[:h]) + ref_mean(v[h:])) / 2.0


def ref_sample(objects, quantity, points, origin, shape, stride, mod, smoothing="linear"):
    out = torch.empty(shape, dtype=torch.float64)
    for i in range(shape[0]):
        for j in range(shape[1]):
            for k in range(shape[2]):
                cell = (i, j, k)
                v = [ref_point(objects, quantity,
                               [stride[a] * (origin[a] + cell[a]) + off[a] + 0.5 for a in range(3)], mod, smoothing)
                     for off in points]
                if quantity == "eps":
                    out[i, j, k] = ref_mean(v)
                else:
                    s = 0
                    for w in v:
                        s = s + w * w
                    out[i, j, k] = math.sqrt(s / float(len(v)))
    return out


def stencil(comp, mod):
    if mod == 1:
        return list(MATERIAL_STENCIL[comp])
    return [tuple(2 * b[a] + s[a] for a in range(3)) for b, s in MATERIAL_STENCIL_DOUBLE[comp]]


# a box, a sphere overlapping it and a cylinder poking out of the region (6, 5, 7) at (3, 0, 2)
OBJECTS = [
    {"shape": "box", "lo": [2.0, -1.0, 3.3], "hi": [6.4, 3.0, 6.0], "eps": 2.25},
    {"shape": "sphere", "center": [6.3, 2.37, 5.1], "radius": 2.37, "eps": 5.0, "omega_p": 1.25},
    {"shape": "cylinder", "axis": "x", "center": [3.1, 7.2], "radius": 1.7, "span": [5.5, 30.0], "eps": 1.5,
     "omega_p": 0.5},
]


@pytest.mark.parametrize("mod", [1, 2])
@pytest.mark.parametrize("npts", [1, 2, 4, 8])
def test_oracle_against_scalar_reference(mod, npts):
    """1. The torch op equals a per-point Python loop of the rules, exactly,
    for eps (both smoothings) and omega."""
    ops = make_ops("torch", None, "cpu", torch.float64)
    pts = {1: [(0, 0, 0)], 2: stencil("Ey", 1), 4: stencil("Hy", 1), 8: stencil("Hz", 2)}[npts]
    origin, shape = (3, 0, 2), (6, 5, 7)
    stride = (mod, mod, mod)
    for smoothing in ("linear", "none"):
        tab = build_table(OBJECTS, "3d", smoothing, FREQ)
        for q in ("eps", "omega"):
            got = ops.scene_sample(tab, q, pts, origin, shape, stride, float(mod))
            want = ref_sample(OBJECTS, q, pts, origin, shape, stride, float(mod), smoothing)
            assert got.dtype == torch.float64 and tuple(got.shape) == shape
            assert torch.equal(got, want), (smoothing, q)
            # the scene is not trivial over this region
            assert len(torch.unique(got)) >= 3, (smoothing, q)


# --------------------------------------------------- built-in scenes coincide
BASE = dict(scheme="3d", size=(16, 16, 16), time_steps=12, dtype="f64", sphere_center=(8.5, 7.5, 8.0),
            sphere_radius=4.5, sphere_eps=3.0)
ONE_SPHERE = {"shape": "sphere", "center": [8.5, 7.5, 8.0], "radius": 4.5}


@pytest.mark.parametrize("kind,double", [("sphere", False), ("sphere", True), ("drude-sphere", False),
                                         ("drude-sphere", True)])
def test_one_sphere_equals_builtin(kind, double):
    """2. One sphere from a file scene is the built-in scene: every averaged
    array, then the fields of a run, bit for bit."""
    meta = kind == "drude-sphere"
    obj = dict(ONE_SPHERE, **({"omega_p": SQRT2_F32} if meta else {"eps": 3.0}))
    extra = dict(use_metamaterials=meta, double_material_precision=double)
    a = make(SchemeConfig(scene=kind, **BASE, **extra))
    b = make(SchemeConfig(scene="file", scene_objects=[obj], **BASE, **extra))
    assert a.scene.is_vacuum(meta) == b.scene.is_vacuum(meta) is False
    assert a.scene.percell_kinds(meta) == b.scene.percell_kinds(meta)
    for n in ("eps", "mu", "omega_pe", "omega_pm", "gamma_e", "gamma_m"):
        assert a.scene.uniform(n) == b.scene.uniform(n), n
    varied = 0
    for c in a.comps:
        if c[0] != "E":
            continue
        if not meta:
            x, y = a.sampler.averaged(c, "eps"), b.sampler.averaged(c, "eps")
            assert torch.equal(x, y), c
            varied += len(torch.unique(x)) > 2
        else:
            (w0, g0), (w1, g1) = a.sampler.averaged_drude(c, True), b.sampler.averaged_drude(c, True)
            assert torch.equal(w0, w1), c
            assert not bool(g0.any()) and not bool(torch.as_tensor(g1).any())
            varied += len(torch.unique(w0)) > 2
    assert varied == 3
    assert torch.equal(a.sampler.grid("eps"), b.sampler.grid("eps"))
    assert torch.equal(a.sampler.grid("omega_pe"), b.sampler.grid("omega_pe"))
    a.perform_steps()
    b.perform_steps()
    for c in a.comps:
        assert torch.equal(a.F[0][c], b.F[0][c]), c
    assert float(a.F[0]["Ez"].abs().max()) > 0


# ------------------------------------------------------------ painter's order
def _grid(objects, name, scheme="3d", size=(24, 24, 24), smoothing="linear"):
    scene = Scene(kind="file", scheme=scheme, source_frequency=FREQ, objects=objects, smoothing=smoothing)
    from fdtd3d_amd.layout.yee import YeeLayout
    lay = YeeLayout(size, scheme, (0, 0, 0), (0, 0, 0), math.pi / 2, 0.0, math.pi / 2, False)
    shape = tuple(size[d] if lay.active(d) else 1 for d in range(3))
    return MaterialSampler(lay, scene, (0, 0, 0), shape, torch.device("cpu")).grid(name)


def test_painters_order():
    """3. Later objects cover earlier ones; a dielectric over a metal removes it."""
    shell = [{"shape": "sphere", "center": [12.5, 12.5, 12.5], "radius": 8, "eps": 4.0},
             {"shape": "sphere", "center": [12.5, 12.5, 12.5], "radius": 3, "eps": 1.0}]
    g = _grid(shell, "eps")
    assert g[12, 12, 12] == 1.0 and g[12, 12, 17] == 4.0 and g[12, 18, 12] == 4.0 and g[1, 1, 1] == 1.0
    assert g[12, 12, 22] == 1.0
    # the other order: the large sphere covers the small one
    assert _grid(shell[::-1], "eps")[12, 12, 12] == 4.0
    metal = [{"shape": "box", "lo": [4, 4, 4], "hi": [20, 20, 20], "omega_p": 1.0},
             {"shape": "cylinder", "axis": "y", "center": [12.5, 12.5], "radius": 3, "span": [0, 24], "eps": 2.0}]
    w = _grid(metal, "omega_pe")
    assert w[5, 12, 5] == 1.0 * 2 * math.pi * FREQ and w[2, 12, 2] == 0.0
    assert w[12, 12, 12] == 0.0 and w[12, 5, 12] == 0.0   # inside the dielectric cylinder
    assert w[12, 12, 17] == 1.0 * 2 * math.pi * FREQ        # beside it
    # omega is sharp and eps smoothed: the box's face at 4.0 lies half a cell from the centre 3.5
    e = _grid([dict(metal[0], eps=3.0)], "eps")
    assert e[3, 12, 12] == 1.0 and e[4, 12, 12] == 3.0      # d = +0.5 and -0.5: the ends of the ramp
    e = _grid([{"shape": "box", "lo": [4.25, 4, 4], "hi": [20, 20, 20], "eps": 3.0}], "eps")
    assert e[4, 12, 12] == 0.75 * 3.0 + 0.25 * 1.0          # d = -0.25
    e = _grid([{"shape": "box", "lo": [4.25, 4, 4], "hi": [20, 20, 20], "eps": 3.0}], "eps", smoothing="none")
    assert e[4, 12, 12] == 3.0 and e[3, 12, 12] == 1.0


# ------------------------------------------------------------------------- 2D
def test_two_d():
    """4. A 2D disc is the 3D sphere's mid plane; a rectangle the box's; a
    cylinder along z a disc; an off-axis cylinder is refused."""
    objs = [{"shape": "box", "lo": [3, 2.5, 9], "hi": [15, 11, 15], "eps": 2.25},
            {"shape": "sphere", "center": [12.3, 11.37, 12.5], "radius": 6.37, "eps": 4.0, "omega_p": 1.0},
            {"shape": "cylinder", "axis": "z", "center": [6.5, 17.25], "radius": 3.3, "span": [10, 14], "eps": 7.0}]
    for name in ("eps", "omega_pe"):
        g3 = _grid(objs, name)
        for scheme in ("tmz", "tez"):
            g2 = _grid(objs, name, scheme=scheme, size=(24, 24, 1))
            assert tuple(g2.shape) == (25, 25, 1)
            assert torch.equal(g2[:, :, 0], g3[:, :, 12])   # z = 12.5: the sphere's centre plane, inside every span
    off = [{"shape": "cylinder", "axis": "x", "center": [6.5, 0.5], "radius": 3, "span": [2, 9]}]
    with pytest.raises(ValueError, match="inactive axis"):
        Scene(kind="file", scheme="tmz", objects=off)
    with pytest.raises(ValueError, match="2D or 3D"):
        Scene(kind="file", scheme="1d", objects=objs)
    # a 2D run with a file scene steps
    s = make(SchemeConfig(scheme="tmz", size=(24, 24, 1), time_steps=6, scene="file", scene_objects=objs))
    s.perform_steps()
    assert bool(torch.isfinite(s.F[0]["Ez"]).all()) and float(s.F[0]["Ez"].abs().max()) > 0


# ------------------------------------------------------- format and refusals
GOOD = {"shape": "sphere", "center": [1, 2, 3], "radius": 2}
BAD = [
    ({"shape": "cone", "radius": 1}, "unknown shape"),
    (dict(GOOD, colour=3), "unknown key"),
    ({"shape": "box", "lo": [0, 0, 0], "hi": [1, 1, 1], "radius": 2}, "unknown key"),
    (dict(GOOD, radius=0), "radius must be positive"),
    (dict(GOOD, radius=-1.0), "radius must be positive"),
    ({"shape": "cylinder", "axis": "z", "center": [1, 1], "radius": 0, "span": [0, 1]}, "radius must be positive"),
    ({"shape": "box", "lo": [0, 0, 0], "hi": [1, 0, 1]}, "lo < hi"),
    ({"shape": "box", "lo": [0, 2, 0], "hi": [1, 1, 1]}, "lo < hi"),
    ({"shape": "cylinder", "axis": "z", "center": [1, 1], "radius": 1, "span": [3, 3]}, "span lo < hi"),
    (dict(GOOD, eps=0), "eps must be positive"),
    (dict(GOOD, eps=-2.0), "eps must be positive"),
    (dict(GOOD, omega_p=-0.1), "omega_p must not be negative"),
    (dict(GOOD, radius=float("nan")), "finite"),
    (dict(GOOD, center=[1, float("inf"), 3]), "finite"),
    (dict(GOOD, eps=float("inf")), "finite"),
    (dict(GOOD, center=[1, 2]), "list of 3"),
    (dict(GOOD, radius="2"), "must be a number"),
    ({"shape": "sphere", "radius": 2}, "needs 'center'"),
    ({"shape": "cylinder", "axis": "w", "center": [1, 1], "radius": 1, "span": [0, 1]}, "axis must be"),
]


@pytest.mark.parametrize("obj,msg", BAD, ids=range(len(BAD)))
def test_object_refusals(obj, msg, monkeypatch):
    """5. Every refusal is a ValueError with a message, raised while the
    scene is built: nothing is allocated (no tensor factory may run)."""
    def no_alloc(*a, **k):
        raise AssertionError("allocated before the refusal")
    for f in ("zeros", "empty", "full", "ones", "arange"):
        monkeypatch.setattr(torch, f, no_alloc)
    with pytest.raises(ValueError, match=msg):
        Scene(kind="file", objects=[GOOD, obj])
    with pytest.raises(ValueError, match=msg):
        cfg = SchemeConfig(scheme="3d", size=(8, 8, 8), scene="file", scene_objects=[obj])
        YeeScheme(cfg, make_ops("torch", None, "cpu", torch.float64)).init_grids()


def test_scene_refusals():
    many = [GOOD] * (SCENE_MAX_OBJECTS + 1)
    with pytest.raises(ValueError, match="the table holds %d" % SCENE_MAX_OBJECTS):
        Scene(kind="file", objects=many)
    assert len(Scene(kind="file", objects=many[:-1]).table()) == SCENE_MAX_OBJECTS >= 64
    with pytest.raises(ValueError, match="smoothing"):
        Scene(kind="file", objects=[GOOD], smoothing="cubic")
    with pytest.raises(ValueError, match="need kind 'file'"):
        Scene(kind="sphere", objects=[GOOD])
    # an empty scene is vacuum
    s = Scene(kind="file", objects=[])
    assert s.is_vacuum(True) and s.uniform("eps") == 1.0 and s.uniform("omega_pe") == 0.0
    # uniform() follows the objects
    s = Scene(kind="file", objects=[dict(GOOD, omega_p=1.0)])
    assert s.uniform("eps") == 1.0 and s.uniform("omega_pe") is None and s.uniform("mu") == 1.0
    assert s.uniform("omega_pm") == 0.0 and s.uniform("gamma_e") == 0.0
    assert s.is_vacuum(False) and not s.is_vacuum(True) and s.percell_kinds(False) == 0
    s = Scene(kind="file", objects=[dict(GOOD, eps=2.0)])
    assert s.uniform("eps") is None and s.uniform("omega_pe") == 0.0 and s.percell_kinds(False) == 1


def test_op_refusals():
    ops = make_ops("torch", None, "cpu", torch.float64)
    tab = build_table([GOOD])
    ok = dict(points=[(0, 0, 0)], origin=(0, 0, 0), shape=(2, 2, 2), stride=(1, 1, 1), mod=1.0)
    assert tuple(ops.scene_sample(tab, "eps", **ok).shape) == (2, 2, 2)
    assert ops.scene_sample(tab, "eps", **dict(ok, shape=(2, 0, 2))).numel() == 0
    for bad in (dict(points=[]), dict(points=[(0, 0, 0)] * 9), dict(points=[(0, 0, 0)] * 3), dict(stride=(1, 3, 1)),
                dict(shape=(2, -1, 2)), dict(mod=1.5)):
        with pytest.raises(ValueError):
            ops.scene_sample(tab, "eps", **dict(ok, **bad))
    with pytest.raises(ValueError):
        ops.scene_sample(tab, "mu", **ok)
    with pytest.raises(ValueError):
        ops.scene_sample(tab, "eps", out=torch.zeros((2, 2, 2), dtype=torch.float32), **ok)


def test_scene_file_and_options(tmp_path):
    """5. The JSON format and the --scene / --scene-file pair."""
    doc = {"smoothing": "linear", "objects": [
        {"shape": "box", "lo": [0, 0, 0], "hi": [64, 64, 20], "eps": 2.25},
        {"shape": "sphere", "center": [32.5, 32.5, 30.5], "radius": 8, "eps": 1.0, "omega_p": 1.4142135},
        {"shape": "cylinder", "axis": "z", "center": [20.5, 40.5], "radius": 3, "span": [20, 50], "eps": 4.0}]}
    p = tmp_path / "scene.json"
    p.write_text(json.dumps(doc))
    objs, smoothing = load_scene_file(str(p))
    assert smoothing == "linear" and [o.shape for o in objs] == ["box", "sphere", "cylinder"]
    assert objs[2].a == (20.5, 40.5, 20.0) and objs[2].b[2] == 50.0 and objs[2].axis == 2
    assert objs == parse_objects(doc["objects"])
    out = io.StringIO()
    st, s = setup_from_cmd(["--scene", "file", "--scene-file", str(p), "--sizex", "24", "--same-size"], out=out)
    assert st == 0 and s.sceneFile == str(p)
    cfg = SchemeConfig.from_settings(s)
    assert cfg.scene == "file" and len(cfg.scene_objects) == 3
    assert len(Scene.from_config(cfg, 1.0).objects) == 3
    for argv, msg in ((["--scene", "file"], "--scene file needs --scene-file"),
                      (["--scene-file", str(p)], "--scene-file needs --scene file"),
                      (["--scene", "sphere", "--scene-file", str(p)], "--scene-file needs --scene file")):
        out = io.StringIO()
        assert setup_from_cmd(argv, out=out)[0] == 1 and msg in out.getvalue()
    # what the file refuses is a SettingsError
    for text, msg in (("{nonsense", "scene.json"), ('{"objects": [], "extra": 1}', "unknown key"),
                      ('{"smoothing": "cubic", "objects": []}', "smoothing"), ('[1]', "one JSON object"),
                      ('{"smoothing": "none"}', "needs 'objects'"),
                      ('{"objects": [{"shape": "sphere", "center": [1, 2, NaN], "radius": 1}]}', "non-finite"),
                      ('{"objects": [{"shape": "sphere", "center": [1, 2, 3], "radius": 1e999}]}', "finite"),
                      (json.dumps({"objects": [GOOD] * (SCENE_MAX_OBJECTS + 1)}), "the table holds")):
        p.write_text(text)
        with pytest.raises(SettingsError, match=msg):
            load_scene_file(str(p))
    with pytest.raises(SettingsError, match="missing.json"):
        load_scene_file(str(tmp_path / "missing.json"))
    # the scheme's refusals through the options: 1D, an off-axis cylinder in 2D
    p.write_text(json.dumps(doc))
    st, s = setup_from_cmd(["--1d", "--scene", "file", "--scene-file", str(p)], out=io.StringIO())
    with pytest.raises(SettingsError, match="2D or 3D"):
        SchemeConfig.from_settings(s)
    p.write_text(json.dumps({"objects": [{"shape": "cylinder", "axis": "y", "center": [1, 1], "radius": 1,
                                          "span": [0, 2]}]}))
    st, s = setup_from_cmd(["--2d", "--scene", "file", "--scene-file", str(p)], out=io.StringIO())
    with pytest.raises(SettingsError, match="inactive axis"):
        SchemeConfig.from_settings(s)


def test_driver_runs_a_scene_file(tmp_path):
    """The Python driver end to end on the torch backend: --save-materials
    writes the Eps grid, the --json line names the objects; a bad file ends
    the run with an error before anything is set up."""
    from fdtd3d_amd.runner import run
    p = tmp_path / "scene.json"
    p.write_text(json.dumps({"objects": [{"shape": "box", "lo": [0, 0, 0], "hi": [12, 12, 4], "eps": 2.25},
                                         {"shape": "sphere", "center": [6.5, 6.5, 7.5], "radius": 2.5, "eps": 4}]}))
    argv = ["--3d", "--sizex", "12", "--same-size", "--time-steps", "4", "--backend", "torch", "--device", "cpu",
            "--scene", "file", "--scene-file", str(p), "--json", "--save-materials", "--save-as-dat",
            "--output-dir", str(tmp_path)]
    out = io.StringIO()
    assert run(argv, out=out) == 0
    rec = json.loads(out.getvalue().strip().splitlines()[-1])
    assert rec["scene"] == {"objects": 2}
    assert any("Eps" in f.name for f in tmp_path.iterdir())
    p.write_text(json.dumps({"objects": [{"shape": "sphere", "center": [6.5, 6.5, 7.5], "radius": -1}]}))
    out = io.StringIO()
    assert run(argv, out=out) == 1 and "radius must be positive" in out.getvalue()


def test_native_parser_and_driver(tmp_path):
    """One option table for both parsers; the native driver refuses file
    scenes (exit 2, with a message)."""
    argv = ["--scene", "file", "--scene-file", "scene.json"]
    st, nat = native.parse_settings(argv)
    assert st == 0 and nat["scene"] == "file" and nat["sceneFile"] == "scene.json"
    assert native.parse_settings([])[1]["sceneFile"] == ""
    exe = native.executable()
    assert os.path.exists(exe), "fdtd3d executable not built"
    r = subprocess.run([exe, "--3d"] + argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--scene file" in r.stderr and "python -m fdtd3d_amd" in r.stderr


# --------------------------------------------------------------- decomposition
PAR_OBJECTS = [{"shape": "box", "lo": [0, 0, 0], "hi": [24, 24, 6], "eps": 2.25},
               {"shape": "sphere", "center": [12.0, 11.5, 10.5], "radius": 3.5, "omega_p": SQRT2_F32}]
PAR = {
    # plain blocked passes over the dielectric box (the Drude part needs --use-metamaterials)
    "blocked": SchemeConfig(scheme="3d", size=(24, 24, 16), time_steps=8, scene="file", scene_objects=PAR_OBJECTS,
                            use_fused=True, time_block=3),
    # hybrid passes: blocked core, the Drude sphere across the rank borders x = 12, y = 12
    "hybrid": SchemeConfig(scheme="3d", size=(24, 24, 16), time_steps=8, scene="file", scene_objects=PAR_OBJECTS,
                           use_metamaterials=True, hybrid_block=3),
}


@pytest.mark.parametrize("name", sorted(PAR))
def test_decomposed_equals_serial(name):
    """6. 2x2x1 thread ranks, every rank sampling the scene from its global
    origin: the serial fields bit for bit, on blocked / hybrid passes."""
    cfg = PAR[name]
    ser = make(cfg)
    assert (ser.tb == 3) if name == "blocked" else (ser.hybrid is not None)
    ser.perform_steps()
    topo = (2, 2, 1)
    core = ParallelGridCore.create(cfg.size, 4, "xy", requested=topo, optimal=False)
    hub = LocalHub(4, tagless=True)
    out, errors = {}, []

    def body(rank):
        try:
            dom = core.domain(rank, 3, align_z=4, align_axis=2)
            halo = HaloExchanger(dom, comm=hub.comm(rank), mode="direct")
            s = make(cfg, dom, halo)
            assert (s.tb == 3) if name == "blocked" else (s.hybrid is not None), "pass form not selected"
            s.perform_steps()
            halo.drain(s)
            out[rank] = (dom.lo, dom.hi, {c: s.owned_field(c, 0).clone() for c in s.comps})
        except BaseException as e:  # surface thread failures in the test
            errors.append(e)

    torch.set_num_threads(1)
    ths = [threading.Thread(target=body, args=(r,)) for r in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=600)
    if errors:
        raise errors[0]
    for c in ser.comps:
        full = torch.full(cfg.size, float("nan"), dtype=torch.float64)
        for lo, hi, own in out.values():
            full[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = own[c]
        assert torch.equal(full, ser.F[0][c]), c
    assert float(ser.F[0]["Ez"].abs().max()) > 0
