"""Triangle meshes in file scenes on the CPU: the torch ``scene_sample`` op
against analytic shapes (cube, octahedron, icosphere), orientation and input
form, painter's order, the refusals of the format, a decomposed run."""

import io
import json
import math
import threading

import numpy as np
import pytest
import torch

from fdtd3d_amd.layout.materials import Scene
from fdtd3d_amd.layout.scene_file import (SCENE_ENT_SIZE, SCENE_MAX_TRIANGLES, build_table, load_scene_file, load_stl,
                                          parse_objects)
from fdtd3d_amd.layout.yee import MATERIAL_STENCIL, MATERIAL_STENCIL_DOUBLE
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.parallel.comm import LocalHub
from fdtd3d_amd.parallel.halo import HaloExchanger
from fdtd3d_amd.parallel.topology import ParallelGridCore
from fdtd3d_amd.utils.settings import SettingsError, setup_from_cmd
from mesh_shapes import as_float32, cube, icosphere, octahedron, write_ascii_stl, write_binary_stl

FREQ = 1.5e10
N = 16
COMPS = ("Ex", "Ey", "Ez", "Hx", "Hy", "Hz")


@pytest.fixture(scope="module")
def ops():
    return make_ops("torch", None, "cpu", torch.float64)


def stencil(comp, mod):
    if mod == 1:
        return list(MATERIAL_STENCIL[comp])
    return [tuple(2 * b[a] + s[a] for a in range(3)) for b, s in MATERIAL_STENCIL_DOUBLE[comp]]


def mesh(vt, **kw):
    return dict({"shape": "mesh", "vertices": vt[0], "triangles": vt[1]}, **kw)


def sample(ops, objs, q, pts, mod, smoothing, shape=(N, N, N), origin=(0, 0, 0)):
    tab = build_table(objs, "3d", smoothing, FREQ)
    return ops.scene_sample(tab, q, pts, origin, shape, (mod,) * 3, float(mod))


def points(mod, n=N):
    """The eps-grid coordinates / mod (cells) of the single-point stencil."""
    g = (torch.arange(n, dtype=torch.float64) * mod + 0.5) / mod
    return torch.meshgrid(g, g, g, indexing="ij")


# ----------------------------------------------------------------------- cube
# Faces on eighths: at mod 1 and at mod 2 (where they double to quarters) no sample point lies on a
# face, and the face diagonals x = y, ... pass exactly through sample columns.
LO, HI = 3.125, 12.125


@pytest.mark.parametrize("mod", [1, 2])
def test_cube_equals_box(ops, mod):
    """1. Sharp: the cube's arrays are the box's, bit for bit, at every
    component's stencil.  Linear: within 1e-12 * eps more than a cell away
    from every cube edge, where the box's distance is the Euclidean one."""
    eps = 3.0
    m = mesh(cube((LO,) * 3, (HI,) * 3), eps=eps, omega_p=1.25)
    b = {"shape": "box", "lo": [LO] * 3, "hi": [HI] * 3, "eps": eps, "omega_p": 1.25}
    for comp in COMPS:
        for q in ("eps", "omega"):
            x, y = (sample(ops, [o], q, stencil(comp, mod), mod, "none") for o in (m, b))
            assert torch.equal(x, y), (comp, q, int((x != y).sum()))
            assert len(torch.unique(x)) >= 2
    X = points(mod)
    # the distances of a point's coordinates from the face planes: near an edge when two of them are small
    near = [torch.minimum((P - LO).abs(), (P - HI).abs()) <= 1.0 for P in X]
    away = (near[0].int() + near[1].int() + near[2].int()) < 2
    x, y = (sample(ops, [o], "eps", [(0, 0, 0)], mod, "linear") for o in (m, b))
    assert int(away.sum()) > N ** 3 // 4 and len(torch.unique(y[away])) >= 3
    err = float((x - y)[away].abs().max())
    print("cube vs box, linear, mod %d: %.3g" % (mod, err))
    assert err <= 1e-12 * eps


# ----------------------------------------------------------------- octahedron
@pytest.mark.parametrize("mod", [1, 2])
@pytest.mark.parametrize("r", [6.25, 6.0])
def test_octahedron(ops, r, mod):
    """2. |x - c| + |y - c| + |z - c| < r with c on a sample point: rays pass
    through both apexes and the four meridian edges; at r = 6 the equator
    edges project onto sample columns.  The inside set is the analytic one
    wherever the point is not on the surface."""
    c = (8.5, 8.5, 8.5)
    x = sample(ops, [mesh(octahedron(c, r), eps=3.0)], "eps", [(0, 0, 0)], mod, "none")
    X = points(mod)
    s = (X[0] - c[0]).abs() + (X[1] - c[1]).abs() + (X[2] - c[2]).abs()
    on = s == r
    if mod == 1:
        assert int(on.sum()) == (0 if r == 6.25 else 4 * 6 * 6 + 2)
    assert int(on.sum()) < 0.05 * N ** 3
    inside = x == 3.0
    assert bool(((inside == (s < r)) | on).all()), int(((inside != (s < r)) & ~on).sum())
    assert int(inside.sum()) > 100 and bool(((x == 3.0) | (x == 1.0)).all())


# ------------------------------------------------------------------ icosphere
C_ICO, R_ICO = (8.37, 8.11, 7.93), 5.37


@pytest.mark.parametrize("mod", [1, 2])
def test_icosphere(ops, mod):
    """3. 320 triangles with vertices on a sphere: the sphere object's arrays
    wherever the sphere's distance is outside [-s, 0], s = the sagitta of the
    flattest face."""
    v, t = icosphere(C_ICO, R_ICO, 2)
    assert len(t) == 320
    p = np.asarray(v)[np.asarray(t)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    plane = np.abs(((p[:, 0] - np.asarray(C_ICO)) * n).sum(axis=1)) / np.linalg.norm(n, axis=1)
    s = R_ICO - float(plane.min())
    assert 0 < s < 0.2
    X = points(mod)
    d = torch.sqrt((X[0] - C_ICO[0]) ** 2 + (X[1] - C_ICO[1]) ** 2 + (X[2] - C_ICO[2]) ** 2) - R_ICO
    keep = (d < -s - 1e-9) | (d > 1e-9)
    assert int((~keep).sum()) < 0.05 * N ** 3
    ball = {"shape": "sphere", "center": list(C_ICO), "radius": R_ICO, "eps": 3.0, "omega_p": 1.0}
    for q in ("eps", "omega"):
        x = sample(ops, [mesh((v, t), eps=3.0, omega_p=1.0)], q, [(0, 0, 0)], mod, "none")
        y = sample(ops, [ball], q, [(0, 0, 0)], mod, "none")
        assert torch.equal(x[keep], y[keep]), (q, int((x != y)[keep].sum()))
        assert len(torch.unique(y[keep])) == 2


# ---------------------------------------------------------------- orientation
def test_orientation_order_and_input_form(ops, tmp_path):
    """4. Reversed triangles, a permuted triangle order, binary STL, ASCII STL
    and inline float32 vertices: identical arrays, both smoothings."""
    v, t = icosphere(C_ICO, R_ICO, 1)
    v = as_float32(v)
    write_binary_stl(str(tmp_path / "b.stl"), v, t)
    write_ascii_stl(str(tmp_path / "a.stl"), v, t)
    assert np.array_equal(load_stl(str(tmp_path / "b.stl")), load_stl(str(tmp_path / "a.stl")))
    assert load_stl(str(tmp_path / "a.stl")).shape == (80, 3, 3)
    g = torch.Generator().manual_seed(5)
    perm = torch.randperm(len(t), generator=g).tolist()
    forms = {"inline": mesh((v, t), eps=3.0),
             "reversed": mesh((v, [[a, c, b] for a, b, c in t]), eps=3.0),
             "rotated": mesh((v, [[b, c, a] for a, b, c in t]), eps=3.0),
             "permuted": mesh((v, [t[i] for i in perm]), eps=3.0),
             "binary": {"shape": "mesh", "file": str(tmp_path / "b.stl"), "eps": 3.0},
             "ascii": {"shape": "mesh", "file": str(tmp_path / "a.stl"), "eps": 3.0}}
    for smoothing in ("linear", "none"):
        got = {k: sample(ops, [o], "eps", stencil("Hx", 1), 1, smoothing) for k, o in forms.items()}
        assert len(torch.unique(got["inline"])) >= (4 if smoothing == "linear" else 3)
        for k in forms:
            assert torch.equal(got[k], got["inline"]), (smoothing, k)
    # scale and translate: the same mesh from unit coordinates
    u = icosphere((0.0, 0.0, 0.0), 1.0, 1)
    a = sample(ops, [mesh(u, scale=R_ICO, translate=list(C_ICO), eps=3.0)], "eps", [(0, 0, 0)], 1, "linear")
    b = sample(ops, [mesh(icosphere(C_ICO, R_ICO, 1), eps=3.0)], "eps", [(0, 0, 0)], 1, "linear")
    assert float((a - b).abs().max()) < 1e-12 and len(torch.unique(a)) > 3


# ------------------------------------------------------------ painter's order
def test_painters_order(ops):
    """5. A mesh over a box and under a sphere is the three single-object
    arrays composed by hand (sharp)."""
    box = {"shape": "box", "lo": [2.3, 1.1, 0.7], "hi": [9.4, 14.2, 8.6], "eps": 2.0, "omega_p": 0.5}
    m = mesh(icosphere(C_ICO, R_ICO, 1), eps=3.0, omega_p=1.0)
    ball = {"shape": "sphere", "center": [10.3, 9.7, 9.1], "radius": 3.37, "eps": 4.0, "omega_p": 0.0}
    for q, vac, vals in (("eps", 1.0, (2.0, 3.0, 4.0)), ("omega", 0.0, (0.5, 1.0, 0.0))):
        vals = [v * (2 * math.pi * FREQ if q == "omega" else 1.0) for v in vals]
        one = [sample(ops, [o], q, [(0, 0, 0)], 1, "none") for o in (box, m, ball)]
        ins = [a == v for a, v in zip(one[:2], vals[:2])]
        # (the metal-free sphere paints omega 0: its inside set from eps)
        ins.append(sample(ops, [ball], "eps", [(0, 0, 0)], 1, "none") == 4.0)
        want = torch.full((N, N, N), vac, dtype=torch.float64)
        for i, v in zip(ins, vals):
            want = torch.where(i, torch.full_like(want, v), want)
        got = sample(ops, [box, m, ball], q, [(0, 0, 0)], 1, "none")
        assert torch.equal(got, want), q
        assert all(int((i0 & i1).sum()) > 0 for i0, i1 in ((ins[0], ins[1]), (ins[1], ins[2])))


# ------------------------------------------------------------------- refusals
def _tetra():
    return [[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]], [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]


def _bad_meshes():
    v, t = _tetra()
    cv, ct = cube((1, 1, 1), (5, 5, 5))
    ok = {"shape": "mesh", "vertices": v, "triangles": t}
    return [
        (dict(ok, colour=1), "unknown key"),
        (dict(ok, radius=2), "unknown key"),
        (dict(ok, file="x.stl"), "either 'file' or both"),
        ({"shape": "mesh"}, "either 'file' or both"),
        ({"shape": "mesh", "vertices": v}, "either 'file' or both"),
        (dict(ok, scale=0), "scale must be positive"),
        (dict(ok, scale=-1.5), "scale must be positive"),
        (dict(ok, scale=float("nan")), "finite"),
        (dict(ok, translate=[0, float("inf"), 0]), "finite"),
        (dict(ok, translate=[0, 0]), "list of 3"),
        (dict(ok, vertices=v[:3] + [[0, float("nan"), 4]]), "vertices must be finite"),
        (dict(ok, vertices=[[0, 0], [1, 1], [2, 2], [3, 3]]), "lists of 3 numbers"),
        (dict(ok, triangles=[[0, 1.5, 2]] * 4), "vertex indices"),
        (dict(ok, eps=0), "eps must be positive"),
        (dict(ok, triangles=t[:3]), "at least 4"),
        (dict(ok, triangles=t[:3] + [[1, 2, 4]]), "index out of range"),
        (dict(ok, triangles=t[:3] + [[1, 2, -1]]), "index out of range"),
        (dict(ok, triangles=t + [[1, 1, 2]]), "repeats a vertex"),
        ({"shape": "mesh", "vertices": v + [[2, 2, 0]], "triangles": t + [[1, 2, 4], [2, 1, 4]]}, "degenerate"),
        ({"shape": "mesh", "vertices": cv, "triangles": ct[:-1]}, "not closed"),
        ({"shape": "mesh", "vertices": cv, "triangles": ct + ct[:1]}, "not closed"),
        ({"shape": "mesh", "vertices": cv, "triangles": [ct[0][::-1]] + ct[1:]}, "not consistently oriented"),
        (dict(ok, triangles=[[0, 1, 2]] * (SCENE_MAX_TRIANGLES + 1)), "a scene holds %d" % SCENE_MAX_TRIANGLES),
    ]


BAD = _bad_meshes()


@pytest.mark.parametrize("obj,msg", BAD, ids=range(len(BAD)))
def test_mesh_refusals(obj, msg, monkeypatch):
    """6. Every refusal is a ValueError with its message, raised while the
    scene is built, before any tensor is allocated."""
    def no_alloc(*a, **k):
        raise AssertionError("allocated before the refusal")
    for f in ("zeros", "empty", "full", "ones", "arange"):
        monkeypatch.setattr(torch, f, no_alloc)
    with pytest.raises(ValueError, match=msg):
        Scene(kind="file", objects=[obj])
    with pytest.raises(ValueError, match=msg):
        cfg = SchemeConfig(scheme="3d", size=(8, 8, 8), scene="file", scene_objects=[obj])
        YeeScheme(cfg, make_ops("torch", None, "cpu", torch.float64)).init_grids()


def test_scene_refusals(tmp_path):
    """6. The scene-wide triangle limit, 2D schemes, STL files, and all of
    them through --scene-file as a SettingsError."""
    v, t = _tetra()
    ok = {"shape": "mesh", "vertices": v, "triangles": t}
    # the limit holds over all meshes of a scene
    half = mesh(icosphere((0, 0, 0), 1.0, 0))
    parsed = parse_objects([half])[0]
    big = np.broadcast_to(parsed.mesh.tris[:1], (SCENE_MAX_TRIANGLES // 2 + 1, 3, 3))
    import dataclasses
    from fdtd3d_amd.layout.scene_file import Mesh
    heavy = dataclasses.replace(parsed, mesh=Mesh(big))
    with pytest.raises(ValueError, match="a scene holds"):
        parse_objects([heavy, heavy])
    assert len(parse_objects([heavy, parsed])) == 2
    for scheme in ("tmz", "tez"):
        with pytest.raises(ValueError, match="a mesh needs a 3D scheme"):
            Scene(kind="file", scheme=scheme, objects=[ok])
    with pytest.raises(ValueError, match="2D or 3D"):
        Scene(kind="file", scheme="1d", objects=[ok])
    # STL files: truncated binary, header count over the limit, broken ASCII, a missing file
    cv, ct = cube((1, 1, 1), (5, 5, 5))
    write_binary_stl(str(tmp_path / "ok.stl"), cv, ct)
    data = (tmp_path / "ok.stl").read_bytes()
    assert len(data) == 84 + 50 * 12
    (tmp_path / "short.stl").write_bytes(data[:-7])
    (tmp_path / "head.stl").write_bytes(data[:50])
    (tmp_path / "huge.stl").write_bytes(data[:80] + (SCENE_MAX_TRIANGLES + 1).to_bytes(4, "little"))
    write_ascii_stl(str(tmp_path / "a.stl"), cv, ct)
    text = (tmp_path / "a.stl").read_text()
    (tmp_path / "cut.stl").write_text(text[:len(text) // 2])
    (tmp_path / "word.stl").write_text(text.replace("vertex 1", "vertex x", 1))
    (tmp_path / "open.stl").write_text(text.replace(text[text.index(" facet"):text.index(" endfacet") + 10], "", 1))
    cases = [("short.stl", "neither a binary STL"), ("head.stl", "neither a binary STL"),
             ("cut.stl", "neither a binary STL"), ("word.stl", "neither a binary STL"),
             ("missing.stl", "missing.stl"), ("open.stl", "not closed")]
    for name, msg in cases:
        with pytest.raises(ValueError, match=msg):
            parse_objects([{"shape": "mesh", "file": str(tmp_path / name)}])
    # (a file of 84 bytes stating 2^20 + 1 triangles is not of that size: neither form)
    with pytest.raises(ValueError, match="neither a binary STL"):
        load_stl(str(tmp_path / "huge.stl"))
    # through --scene-file: relative to the scene file's directory, refusals as SettingsError
    p = tmp_path / "scene.json"
    p.write_text(json.dumps({"objects": [{"shape": "mesh", "file": "ok.stl", "eps": 2.0}]}))
    objs, _ = load_scene_file(str(p))
    assert objs[0].shape == "mesh" and len(objs[0].mesh) == 12 and objs[0].a == (1.0, 1.0, 1.0)
    assert objs[0].b == (5.0, 5.0, 5.0)
    for name, msg in cases:
        p.write_text(json.dumps({"objects": [{"shape": "mesh", "file": name}]}))
        with pytest.raises(SettingsError, match=msg):
            load_scene_file(str(p))
    for obj, msg in BAD[:-1]:
        if any(isinstance(x, float) and not math.isfinite(x) for x in _flat(obj)):
            msg = "finite"   # (json writes NaN / Infinity, which the reader refuses as constants)
        p.write_text(json.dumps({"objects": [obj]}))
        with pytest.raises(SettingsError, match=msg):
            load_scene_file(str(p))
    p.write_text(json.dumps({"objects": [ok]}))
    st, s = setup_from_cmd(["--2d", "--scene", "file", "--scene-file", str(p)], out=io.StringIO())
    with pytest.raises(SettingsError, match="a mesh needs a 3D scheme"):
        SchemeConfig.from_settings(s)


def _flat(o):
    if isinstance(o, dict):
        return [x for v in o.values() for x in _flat(v)]
    if isinstance(o, (list, tuple)):
        return [x for v in o for x in _flat(v)]
    return [o]


def test_table_and_driver(tmp_path):
    """The table's layout (72-byte entries, the mesh's box and kind 3, its
    triangle range) and the Python driver's --json line."""
    from fdtd3d_amd.runner import run
    objs = [{"shape": "sphere", "center": [6.5, 6.5, 6.5], "radius": 2.5, "eps": 2.0},
            mesh(cube((2, 3, 4), (6, 7, 8)), eps=3.0), mesh(octahedron((6.5, 6.5, 6.5), 3.0), scale=2.0, eps=4.0)]
    tab = build_table(objs, "3d", "linear", FREQ)
    assert tab.ents.itemsize == SCENE_ENT_SIZE == 72 and list(tab.ents["kind"]) == [1, 3, 3]
    assert tab.tris.shape == (20, 3, 3) and tab.ranges.tolist() == [[0, 0], [0, 12], [12, 8]]
    assert tab.ents["p"][1].tolist() == [2, 3, 4] and tab.ents["q"][1].tolist() == [6, 7, 8]
    assert tab.ents["p"][2].tolist() == [7, 7, 7] and tab.ents["q"][2].tolist() == [19, 19, 19]
    # every triangle's vertices ascend in (x, y, z)
    for tri in tab.tris:
        assert [tuple(v) for v in tri] == sorted(tuple(v) for v in tri)
    assert tab.has_meshes() and tab.range_error() is None and not build_table(objs[:1]).has_meshes()
    write_binary_stl(str(tmp_path / "c.stl"), *cube((3, 3, 3), (9, 9, 8)))
    p = tmp_path / "scene.json"
    p.write_text(json.dumps({"objects": [objs[0], {"shape": "mesh", "file": "c.stl", "eps": 2.25}]}))
    argv = ["--3d", "--sizex", "12", "--same-size", "--time-steps", "4", "--backend", "torch", "--device", "cpu",
            "--scene", "file", "--scene-file", str(p), "--json", "--save-materials", "--save-as-dat",
            "--output-dir", str(tmp_path)]
    out = io.StringIO()
    assert run(argv, out=out) == 0, out.getvalue()
    assert json.loads(out.getvalue().strip().splitlines()[-1])["scene"] == {"objects": 2, "triangles": 12}
    (tmp_path / "c.stl").write_bytes((tmp_path / "c.stl").read_bytes()[:-1])
    out = io.StringIO()
    assert run(argv, out=out) == 1 and "neither a binary STL" in out.getvalue()


# --------------------------------------------------------------- decomposition
def make(cfg, domain=None, halo=None):
    s = YeeScheme(cfg, make_ops("torch", None, "cpu", torch.float64), domain, halo)
    s.init_scheme()
    s.init_grids()
    return s


def test_decomposed_equals_serial():
    """7. 2x2x1 thread ranks of a 24^3 mesh scene, the mesh across the rank
    borders x = 12, y = 12: the serial fields bit for bit (blocked passes)."""
    objs = [mesh(icosphere((12.3, 11.6, 12.2), 5.37, 1), eps=3.0)]
    cfg = SchemeConfig(scheme="3d", size=(24, 24, 24), time_steps=8, scene="file", scene_objects=objs,
                       use_fused=True, time_block=3)
    ser = make(cfg)
    assert ser.tb == 3
    ser.perform_steps()
    core = ParallelGridCore.create(cfg.size, 4, "xy", requested=(2, 2, 1), optimal=False)
    hub = LocalHub(4, tagless=True)
    out, errors = {}, []

    def body(rank):
        try:
            dom = core.domain(rank, 3, align_z=4, align_axis=2)
            halo = HaloExchanger(dom, comm=hub.comm(rank), mode="direct")
            s = make(cfg, dom, halo)
            assert s.tb == 3, "pass form not selected"
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
    assert len(torch.unique(ser.sampler.averaged("Ez", "eps"))) > 3
