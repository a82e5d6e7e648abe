"""Damped and magnetic Drude media of file scenes on the device:
k_scene_sample<Q, MESH> for Q = omega_m, gamma, gamma_m (csrc/scene_kernels.hip)
against the torch op evaluated on the CPU, its refusals, and runs end to end."""

import ctypes
import dataclasses
import io
import json

import numpy as np
import pytest
import torch

from fdtd3d_amd.layout.scene_file import SceneTable, build_table
from fdtd3d_amd.layout.yee import MATERIAL_STENCIL, MATERIAL_STENCIL_DOUBLE
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.hip_lib import HipError
from mesh_shapes import octahedron

pytestmark = pytest.mark.gpu

FREQ = 1.5e10
SENTINEL = -777.25
NEW = ("omega_m", "gamma", "gamma_m")


@pytest.fixture(scope="module")
def hip(gpu):
    return make_ops("hip", None, gpu, torch.float64)


@pytest.fixture(scope="module")
def oracle():
    return make_ops("torch", None, "cpu", torch.float64)


def stencil(comp, mod):
    if mod == 1:
        return list(MATERIAL_STENCIL[comp])
    return [tuple(2 * b[a] + s[a] for a in range(3)) for b, s in MATERIAL_STENCIL_DOUBLE[comp]]


def straddling(origin, shape, mesh=False, z_cylinders=False):
    """Objects across every face of the region with differing poles and
    dampings, painted over each other; ``mesh``: a small closed mesh between
    the primitives; ``z_cylinders``: cylinders along z only (2D schemes)."""
    lo = [float(o) for o in origin]
    hi = [float(o + s) for o, s in zip(origin, shape)]
    mid = [(a + b) / 2 + 0.13 for a, b in zip(lo, hi)]
    objs = [{"shape": "box", "lo": [lo[0] - 2.3, lo[1] - 1.7, lo[2] - 3.1], "hi": [lo[0] + 2.37, mid[1], mid[2]],
             "eps": 2.25, "omega_p": 0.7, "gamma": 0.11, "omega_pm": 0.3},
            {"shape": "box", "lo": [mid[0], mid[1] - 0.37, hi[2] - 2.6], "hi": [hi[0] + 3.3, hi[1] + 1.1, hi[2] + 2.2],
             "eps": 3.5, "omega_pm": 0.9, "gamma_m": 0.07},
            {"shape": "sphere", "center": [mid[0], lo[1] - 0.3, mid[2]], "radius": 2.37, "eps": 5.0, "omega_p": 1.25,
             "gamma": 0.3, "omega_pm": 1.1, "gamma_m": 0.9},
            {"shape": "sphere", "center": [hi[0] - 0.7, hi[1] + 0.37, lo[2] + 1.3], "radius": 3.37, "eps": 1.7},
            {"shape": "sphere", "center": [lo[0] + 0.3, mid[1], hi[2] - 0.37], "radius": 4.37, "omega_p": 0.5,
             "omega_pm": 0.6, "gamma_m": 0.21}]
    if mesh:
        v, t = octahedron((mid[0] - 0.4, mid[1] + 0.2, mid[2] - 0.6), 2.7)
        objs.append({"shape": "mesh", "vertices": v, "triangles": t, "omega_p": 1.6, "gamma": 0.45, "omega_pm": 1.3,
                     "gamma_m": 0.33})
    objs += [{"shape": "cylinder", "axis": "z", "center": [mid[0] + 0.3, mid[1] - 0.7], "radius": 1.37,
              "span": [lo[2] - 5.0, hi[2] + 5.0], "eps": 4.0},
             {"shape": "cylinder", "axis": "z" if z_cylinders else "x",
              "center": [hi[0] - 1.37, mid[1] + 1.3] if z_cylinders else [hi[1] - 0.37, mid[2] + 1.3], "radius": 1.73,
              "span": [lo[2] - 1.3, hi[2] + 0.37] if z_cylinders else [lo[0] - 1.3, mid[0] + 0.37],
              "eps": 1.0, "omega_p": 2.0, "gamma": 1.7, "omega_pm": 0.4, "gamma_m": 0.5}]
    return objs


CASES = [[(0, 0, 0)], stencil("Ex", 1), stencil("Ez", 1), stencil("Hx", 1), stencil("Hz", 1), stencil("Ey", 2),
         stencil("Hy", 2)]


def check(hip, oracle, tab, pts, origin, shape, mod, what, stride=None):
    stride = (mod,) * 3 if stride is None else stride
    for q in NEW:
        want = oracle.scene_sample(tab, q, pts, origin, shape, stride, float(mod))
        n0 = hip.launches
        got = hip.scene_sample(tab, q, pts, origin, shape, stride, float(mod))
        assert hip.launches == n0 + 1
        assert got.dtype == torch.float64 and tuple(got.shape) == shape and got.is_cuda
        assert torch.equal(got.cpu(), want), (what, len(pts), q, int((got.cpu() != want).sum()))
        assert len(torch.unique(want)) >= 4, ("trivial scene", what, len(pts), q)
        all_objs = hip.scene_sample(tab, q, pts, origin, shape, stride, float(mod), cull=False)
        assert torch.equal(all_objs, got), (what, len(pts), q, "culling changed the result")


REGIONS = [((9, 7, 11), (3, -2, 5)), ((5, 3, 130), (-4, 6, 1))]


@pytest.mark.parametrize("mod", [1, 2])
@pytest.mark.parametrize("shape,origin", REGIONS, ids=["9x7x11", "5x3x130"])
def test_kernel_equals_oracle(hip, oracle, shape, origin, mod):
    """torch.equal with the torch op (CPU) for omega_m, gamma and gamma_m:
    every stencil size, both smoothings, objects across every face, one
    launch per call, with and without culling."""
    objs = straddling(origin, shape)
    for smoothing in ("linear", "none"):
        tab = build_table(objs, "3d", smoothing, FREQ)
        for pts in CASES:
            check(hip, oracle, tab, pts, origin, shape, mod, smoothing)


def test_kernel_equals_oracle_2d(hip, oracle):
    """The same on one plane of a scheme that ignores z."""
    shape, origin = (70, 9, 1), (3, -2, 0)
    objs = straddling((3, -2, 4), (70, 9, 6), z_cylinders=True)
    objs[4] = dict(objs[4], gamma=0.23)   # (a fourth damping in reach of this flat region)
    for smoothing in ("linear", "none"):
        tab = build_table(objs, "tmz", smoothing, FREQ)
        for mod in (1, 2):
            for pts in ([(0, 0, 0)], [(0, 0, 0), (1, 0, 0)], [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)],
                        [(a, b, 0) for a in (0, 1) for b in (0, 1)] * 2):
                check(hip, oracle, tab, pts, origin, shape, mod, smoothing, stride=(mod, mod, 1))


@pytest.mark.parametrize("shape,origin", REGIONS, ids=["9x7x11", "5x3x130"])
def test_mesh_twin_equals_oracle(hip, oracle, shape, origin):
    """The same with a small closed mesh painted between the primitives
    (the MESH instantiations)."""
    objs = straddling(origin, shape, mesh=True)
    for smoothing in ("linear", "none"):
        tab = build_table(objs, "3d", smoothing, FREQ)
        assert tab.has_meshes()
        for mod in (1, 2):
            for pts in ([(0, 0, 0)], stencil("Ez", 1), stencil("Hx", 1), stencil("Ey", 2)):
                check(hip, oracle, tab, pts, origin, shape, mod, smoothing)
    # the mesh takes part: without it the arrays differ
    bare = build_table([o for o in objs if o["shape"] != "mesh"], "3d", "linear", FREQ)
    tab = build_table(objs, "3d", "linear", FREQ)
    args = (stencil("Hx", 1), origin, shape, (1, 1, 1), 1.0)
    assert not torch.equal(hip.scene_sample(tab, "gamma", *args), hip.scene_sample(bare, "gamma", *args))


@pytest.mark.parametrize("shape,origin", REGIONS, ids=["9x7x11", "5x3x130"])
def test_dispatch_of_every_quantity_and_form(hip, oracle, shape, origin):
    """The one entry point's table of launches: each of the six quantities
    without and with a mesh, on a region of odd z (scalar stores) and one of
    two z tiles (vector stores), equal to the torch op bit for bit; the mesh
    changes every quantity, so its instantiation is the one that ran."""
    lo = [float(o) for o in origin]
    mid = [o + s / 2 + 0.13 for o, s in zip(lo, shape)]
    # (a lossy sphere under the others: sigma and omega_p exclude each other on an object)
    lossy = {"shape": "sphere", "center": mid, "radius": 3.1, "eps": 1.2, "sigma": 0.8}
    pts = stencil("Hx", 1)
    assert len(pts) == 4
    got = {}
    for mesh in (False, True):
        objs = [lossy] + straddling(origin, shape, mesh=mesh)
        objs[4] = dict(objs[4], sigma=2.5)
        tab = build_table(objs, "3d", "linear", FREQ)
        assert tab.has_meshes() == mesh
        for q in ("eps", "omega") + NEW + ("cond",):
            want = oracle.scene_sample(tab, q, pts, origin, shape, (1, 1, 1), 1.0)
            n0 = hip.launches
            got[q, mesh] = hip.scene_sample(tab, q, pts, origin, shape, (1, 1, 1), 1.0)
            assert hip.launches == n0 + 1
            assert torch.equal(got[q, mesh].cpu(), want), (q, mesh, int((got[q, mesh].cpu() != want).sum()))
            assert len(torch.unique(want)) >= 3, ("trivial scene", q, mesh)
    for q in ("eps", "omega") + NEW + ("cond",):
        assert not torch.equal(got[q, True], got[q, False]), (q, "the mesh changed nothing")


@pytest.mark.parametrize("shape", [(5, 3, 130), (9, 7, 11), (6, 70, 1)], ids=["even-z", "odd-z", "one-z"])
def test_only_the_region_is_written(hip, oracle, gpu, shape):
    """The region as a window of a larger sentinel-filled buffer, its base
    16-byte aligned or not: the cells before and after it stay untouched."""
    origin = (2, 1, -3)
    for mesh in (False, True):
        tab = build_table(straddling(origin, shape, mesh=mesh), "3d", "linear", FREQ)
        n = shape[0] * shape[1] * shape[2]
        for pad in (512, 513):
            for q in NEW:
                buf = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.float64, device=gpu)
                out = buf[pad:pad + n].view(shape)
                got = hip.scene_sample(tab, q, stencil("Hy", 1), origin, shape, (1, 1, 1), 1.0, out=out)
                assert got.data_ptr() == out.data_ptr()
                want = oracle.scene_sample(tab, q, stencil("Hy", 1), origin, shape, (1, 1, 1), 1.0)
                assert torch.equal(out.cpu(), want), (q, pad, mesh)
                assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all())


def test_refusals_launch_nothing(hip, gpu):
    """Every refusal leaves the launch count and the output untouched."""
    shape, origin = (4, 3, 6), (0, 0, 0)
    tab = build_table(straddling(origin, shape), "3d", "linear", FREQ)
    ok = dict(points=[(0, 0, 0)], origin=origin, shape=shape, stride=(1, 1, 1), mod=1.0)
    out = torch.full(shape, SENTINEL, dtype=torch.float64, device=gpu)
    n0 = hip.launches

    def refused(table=tab, quantity="gamma", **kw):
        with pytest.raises((HipError, ValueError)):
            hip.scene_sample(table, quantity, **dict(ok, **kw))
        assert hip.launches == n0 and bool((out == SENTINEL).all())

    for q in ("mu", "gamma_e", "omega_pm", "sigma"):
        refused(quantity=q, out=out)
    # the array beside the entries: its length against the entries, its shape, dtype and values
    for drude in (tab.drude[:-1], tab.drude[:, :2], tab.drude.astype(np.float32), -tab.drude - 1.0,
                  np.full_like(tab.drude, np.inf), None, torch.from_numpy(tab.drude.copy())):
        bad = SceneTable(tab.ents, tab.tris, tab.ranges, tab.drude)
        bad.drude = drude
        for q in NEW + ("eps",):
            refused(table=bad, quantity=q, out=out)
    refused(points=[(0, 0, 0)] * 3, out=out)
    refused(stride=(1, 1, 3), out=out)
    refused(out=torch.full(shape, SENTINEL, dtype=torch.float32, device=gpu))
    refused(out=out[:3])
    refused(shape=(4, 3, 7), out=out)
    refused(out=torch.full(shape, SENTINEL, dtype=torch.float64))  # not on the device
    # the entry point itself: the Drude table (its true size) with a quantity of another group, a table that
    # is missing, a row short or a row long, and the shared checks
    i3 = ctypes.c_int * 3
    vp = ctypes.c_void_p
    dev_tab, dev_drude = hip._scene_table(tab), hip._scene_drude(tab)
    assert dev_drude.numel() == 3 * len(tab)
    stream = torch.cuda.current_stream().cuda_stream
    f = hip.lib.raw.fdtd_scene_sample
    f.restype = ctypes.c_int

    def entry(quantity=3, tab_p=dev_tab.data_ptr(), nobj=len(tab), drude_p=dev_drude.data_ptr(), ndrude=len(tab),
              out_p=out.data_ptr(), shp=i3(*shape), mesh=False, ranges_p=dev_tab.data_ptr(), tris_p=None):
        return f(vp(tab_p), ctypes.c_int(nobj), ctypes.c_int(quantity), i3(0, 0, 0), ctypes.c_int(1), i3(0, 0, 0), shp,
                 i3(1, 1, 1), ctypes.c_double(1.0), ctypes.c_int(1), vp(out_p), vp(stream), vp(drude_p),
                 ctypes.c_size_t(24 * ndrude), vp(tris_p), ctypes.c_int(0), vp(ranges_p if mesh else None))

    for mesh in (False, True):
        for kw in (dict(quantity=0), dict(quantity=1), dict(quantity=5), dict(quantity=-1), dict(tab_p=None),
                   dict(drude_p=None), dict(ndrude=len(tab) - 1), dict(ndrude=len(tab) + 1), dict(out_p=None),
                   dict(nobj=-1, ndrude=-1), dict(shp=i3(4, -3, 6))):
            assert entry(mesh=mesh, **kw) == 1, (mesh, kw)   # hipErrorInvalidValue
        assert entry(mesh=mesh, shp=i3(4, 0, 6)) == 0   # an empty region: nothing launched, no error
    assert entry(mesh=True, ranges_p=None, tris_p=dev_tab.data_ptr()) == 1   # triangles without ranges
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert entry() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


# ------------------------------------------------------------------ end to end
def _run(cfg, backend, device):
    dt = torch.float32 if cfg.dtype == "f32" else torch.float64
    s = YeeScheme(cfg, make_ops(backend, None, device, dt))
    s.init_scheme()
    s.init_grids()
    s.perform_steps()
    if device != "cpu":
        torch.cuda.synchronize()
    return s


# (the two spheres close together: at 40^3 the hybrid planner needs a core of a quarter of the grid clear of
# the dispersive box, which holds both)
MULTI = [{"shape": "box", "lo": [0, 0, 0], "hi": [40, 40, 13.3], "eps": 2.25},
         {"shape": "sphere", "center": [20.3, 19.7, 25.37], "radius": 2.87, "omega_p": 1.7320508, "gamma": 0.3},
         {"shape": "sphere", "center": [20.7, 20.3, 28.3], "radius": 3.37, "omega_p": 1.4142135, "gamma": 0.05,
          "omega_pm": 1.2, "gamma_m": 0.2}]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("mode", ["hybrid", "stepped"])
def test_damped_magnetic_run_vs_fp64_oracle(gpu, dtype, mode):
    """Substrate + damped metal sphere + a sphere with a damped magnetic
    pole, CPML + TF/SF with metamaterials, on HIP against the fp64 CPU oracle
    at the tolerances of test_scene_gpu.py::test_multi_object_run_vs_fp64_oracle."""
    cfg = SchemeConfig(scheme="3d", size=(40, 40, 40), time_steps=12, dtype=dtype, use_pml=True, pml_type="cpml",
                       pml_size=(3, 3, 3), use_tfsf=True, tfsf_size=(6, 6, 6), use_metamaterials=True, scene="file",
                       scene_objects=MULTI, use_fused=True, **({"hybrid_block": 2} if mode == "hybrid"
                                                                else {"hybrid_block": 1, "time_block": 1}))
    a = _run(cfg, "hip", gpu)
    if mode == "hybrid":
        assert a.hybrid is not None, "the run took single steps only"
        tol = 2e-4 if dtype == "f32" else 1e-11
    else:
        assert a.hybrid is None and a.tb == 1
        tol = 5e-5 if dtype == "f32" else 1e-10
    b = _run(dataclasses.replace(cfg, dtype="f64", hybrid_block=1, time_block=1), "torch", "cpu")
    for s in (a, b):
        assert any("D1" in s.upml[c] for c in s.e_comps), "no dispersive E cells"
        assert any("D1" in s.upml[c] for c in s.h_comps), "no dispersive H cells"
    for c in a.comps:
        scale = max(float(b.F[0][o].abs().max()) for o in b.comps if o[0] == c[0]) + 1e-300
        err = float((a.F[0][c].double().cpu() - b.F[0][c]).abs().max())
        print("%s %s %s: err %.3g of scale %.3g (tol %.1g)" % (mode, dtype, c, err, scale, tol))
        assert err <= tol * scale, (c, err, scale)
    assert float(b.F[0]["Ez"].abs().max()) > 0


TWO_METALS = [{"shape": "sphere", "center": [40.0, 36.0, 48.0], "radius": 9.0, "omega_p": 1.4142135, "gamma": 0.2},
              {"shape": "box", "lo": [33.5, 30.2, 40.1], "hi": [41.3, 44.7, 52.6], "omega_p": 0.8, "gamma": 1.5}]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_blocked_drude_with_damping(gpu, dtype):
    """Two eps = 1 metals of different gamma on the grid of
    test_drude_blk_gpu.py's ``upml-T3`` case: the blocked Drude pass takes
    the (omega, gamma) pair table; blocked vs the stepped HIP chain vs the
    fp64 oracle at that file's tolerances."""
    cfg = SchemeConfig(scheme="3d", size=(80, 72, 96), time_steps=17, dtype=dtype, scene="file",
                       scene_objects=TWO_METALS, use_metamaterials=True, use_pml=True, pml_size=(6, 6, 6))
    blk = _run(dataclasses.replace(cfg, hybrid_block=3, time_block=3), "hip", gpu)
    assert blk._drude_plan is not None and blk.drude_blk is not None, "blocked Drude plan rejected"
    assert blk.scene.uniform("gamma_e") is None
    for c in blk.e_comps:
        ids, tab = blk.upml[c]["_drude_lut"]
        assert ids is not None and 4 <= tab.shape[0] <= 256
    st = _run(dataclasses.replace(cfg, blocked_drude="off", hybrid_block=1, time_block=1), "hip", gpu)
    assert st.drude_blk is None
    ref = _run(dataclasses.replace(cfg, blocked_drude="off", hybrid_block=1, time_block=1, dtype="f64"), "torch", "cpu")
    tol = 2e-5 if dtype == "f32" else 1e-11
    for c in ref.comps:
        scale = max(float(ref.F[0][o].abs().max()) for o in ref.comps if o[0] == c[0]) + 1e-30
        e_st = float((blk.F[0][c].double().cpu() - st.F[0][c].double().cpu()).abs().max())
        e_ref = float((blk.F[0][c].double().cpu() - ref.F[0][c]).abs().max())
        print("%s %s: blocked vs stepped %.3g, vs oracle %.3g of scale %.3g" % (dtype, c, e_st, e_ref, scale))
        assert e_st <= tol * scale, (dtype, c, "blocked vs stepped", e_st, scale)
        assert e_ref <= 10 * tol * scale, (dtype, c, "blocked vs fp64 oracle", e_ref, scale)
    assert float(ref.F[0]["Ez"].abs().max()) > 0


def test_save_materials(gpu, tmp_path):
    """--save-materials on HIP writes the OmegaPE / GammaE / OmegaPM / GammaM
    grids the torch backend writes, byte for byte."""
    from fdtd3d_amd.runner import run
    p = tmp_path / "scene.json"
    p.write_text(json.dumps({"objects": MULTI}))
    files = {}
    for backend, device in (("hip", "cuda"), ("torch", "cpu")):
        d = tmp_path / backend
        d.mkdir()
        out = io.StringIO()
        argv = ["--3d", "--sizex", "40", "--same-size", "--time-steps", "2", "--backend", backend, "--device", device,
                "--scene", "file", "--scene-file", str(p), "--json", "--save-materials", "--save-as-dat",
                "--use-metamaterials", "--output-dir", str(d), "--dtype", "f32"]
        assert run(argv, out=out) == 0, out.getvalue()
        assert json.loads(out.getvalue().strip().splitlines()[-1])["scene"] == {"objects": 3, "damped": 2,
                                                                                "magnetic": 1}
        files[backend] = {f.name: f.read_bytes() for f in d.iterdir()
                          if any(n in f.name for n in ("OmegaPE", "GammaE", "OmegaPM", "GammaM"))}
    for label in ("OmegaPE", "GammaE", "OmegaPM", "GammaM"):
        assert any(label in name for name in files["hip"]), label
    assert files["hip"].keys() == files["torch"].keys()
    for name, data in files["hip"].items():
        assert data == files["torch"][name], name
        assert any(data[-4096:]) or any(data), name
