"""File scenes on the device: k_scene_sample (csrc/scene_kernels.hip) against
the torch op evaluated on the CPU, its refusals, and runs end to end."""

import ctypes
import dataclasses
import io
import json

import pytest
import torch

from fdtd3d_amd.layout.scene_file import SCENE_ENT_SIZE, SCENE_MAX_OBJECTS, build_table
from fdtd3d_amd.layout.yee import MATERIAL_STENCIL, MATERIAL_STENCIL_DOUBLE
from fdtd3d_amd.models.blocking import auto_time_block
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.hip_lib import HipError

pytestmark = pytest.mark.gpu

FREQ = 1.5e10
SENTINEL = -777.25


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


def straddling(origin, shape, mod):
    """Objects across every face of the region (eps-grid extent / mod, so in
    cells), non-dyadic centres and radii, painted over each other."""
    lo = [float(o) for o in origin]
    hi = [float(o + s) for o, s in zip(origin, shape)]
    mid = [(a + b) / 2 + 0.13 for a, b in zip(lo, hi)]
    objs = [{"shape": "box", "lo": [lo[0] - 2.3, lo[1] - 1.7, lo[2] - 3.1], "hi": [lo[0] + 2.37, mid[1], mid[2]],
             "eps": 2.25, "omega_p": 0.7},
            {"shape": "box", "lo": [mid[0], mid[1] - 0.37, hi[2] - 2.6], "hi": [hi[0] + 3.3, hi[1] + 1.1, hi[2] + 2.2],
             "eps": 3.5},
            {"shape": "sphere", "center": [mid[0], lo[1] - 0.3, mid[2]], "radius": 2.37, "eps": 5.0, "omega_p": 1.25},
            {"shape": "sphere", "center": [hi[0] - 0.7, hi[1] + 0.37, lo[2] + 1.3], "radius": 3.37, "eps": 1.7},
            {"shape": "sphere", "center": [lo[0] + 0.3, mid[1], hi[2] - 0.37], "radius": 4.37, "omega_p": 0.5},
            {"shape": "cylinder", "axis": "z", "center": [mid[0] + 0.3, mid[1] - 0.7], "radius": 1.37,
             "span": [lo[2] - 5.0, hi[2] + 5.0], "eps": 4.0},
            {"shape": "cylinder", "axis": "x", "center": [hi[1] - 0.37, mid[2] + 1.3], "radius": 1.73,
             "span": [lo[0] - 1.3, mid[0] + 0.37], "eps": 1.0, "omega_p": 2.0},
            {"shape": "cylinder", "axis": "y", "center": [mid[0] - 1.3, lo[2] + 0.37], "radius": 2.3,
             "span": [mid[1] - 0.73, hi[1] + 7.0], "eps": 6.0}]
    return objs


REGIONS = [((9, 7, 11), (3, -2, 5)), ((5, 3, 130), (-4, 6, 1))]


@pytest.mark.parametrize("mod", [1, 2])
@pytest.mark.parametrize("shape,origin", REGIONS, ids=["9x7x11", "5x3x130"])
def test_kernel_equals_oracle(hip, oracle, shape, origin, mod):
    """7. torch.equal with the torch op (CPU, correctly rounded square roots)
    for every stencil size, both quantities and smoothings, objects across
    every face of the region, one launch per call; with and without culling."""
    objs = straddling(origin, shape, mod)
    stride = (mod, mod, mod)
    cases = [[(0, 0, 0)], stencil("Ex", 1), stencil("Ez", 1), stencil("Hx", 1), stencil("Hz", 1), stencil("Ey", 2),
             stencil("Hy", 2)]
    for smoothing in ("linear", "none"):
        tab = build_table(objs, "3d", smoothing, FREQ)
        for pts in cases:
            for q in ("eps", "omega"):
                want = oracle.scene_sample(tab, q, pts, origin, shape, stride, float(mod))
                n0 = hip.launches
                got = hip.scene_sample(tab, q, pts, origin, shape, stride, float(mod))
                assert hip.launches == n0 + 1
                assert got.dtype == torch.float64 and tuple(got.shape) == shape and got.is_cuda
                assert torch.equal(got.cpu(), want), (smoothing, len(pts), q, int((got.cpu() != want).sum()))
                assert len(torch.unique(want)) >= 4, "trivial scene"
                all_objs = hip.scene_sample(tab, q, pts, origin, shape, stride, float(mod), cull=False)
                assert torch.equal(all_objs, got), (smoothing, len(pts), q, "culling changed the result")


def test_object_counts(hip, oracle):
    """7. No object, one object, and the full table: most objects far away
    (culled by every wave), some inside the region."""
    shape, origin = (9, 7, 11), (3, -2, 5)
    near = straddling(origin, shape, 1)
    far = [{"shape": "sphere", "center": [200.3 + 7.1 * n, -150.7 - 3.3 * (n % 7), 90.37 + n], "radius": 2.37 + 0.01 * n,
            "eps": 2.0 + 0.01 * n, "omega_p": 0.1 * (n % 5)} for n in range(SCENE_MAX_OBJECTS - len(near))]
    assert SCENE_MAX_OBJECTS >= 64
    full = far[:100] + near[:4] + far[100:] + near[4:]
    assert len(full) == SCENE_MAX_OBJECTS
    for objs in ([], near[2:3], full):
        tab = build_table(objs, "3d", "linear", FREQ)
        for pts in ([(0, 0, 0)], stencil("Hx", 1)):
            for q in ("eps", "omega"):
                want = oracle.scene_sample(tab, q, pts, origin, shape, (1, 1, 1), 1.0)
                n0 = hip.launches
                got = hip.scene_sample(tab, q, pts, origin, shape, (1, 1, 1), 1.0)
                assert hip.launches == n0 + 1
                assert torch.equal(got.cpu(), want), (len(objs), len(pts), q)
    # the far objects change nothing: the full table gives what the near objects give
    args = ("eps", stencil("Hx", 1), origin, shape, (1, 1, 1), 1.0)
    assert torch.equal(hip.scene_sample(build_table(near, "3d", "linear", FREQ), *args),
                       hip.scene_sample(build_table(full, "3d", "linear", FREQ), *args))
    # 2D: one cell along z, objects ignore it
    tab2 = build_table([o for o in near if o["shape"] != "cylinder" or o["axis"] == "z"], "tmz", "linear", FREQ)
    pts = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)]
    for q in ("eps", "omega"):
        want = oracle.scene_sample(tab2, q, pts, (3, -2, 0), (70, 9, 1), (1, 1, 1), 1.0)
        assert torch.equal(hip.scene_sample(tab2, q, pts, (3, -2, 0), (70, 9, 1), (1, 1, 1), 1.0).cpu(), want), q


def test_refusals_launch_nothing(hip, gpu):
    """8. Every refusal leaves the launch count and the output untouched."""
    shape, origin = (4, 3, 6), (0, 0, 0)
    tab = build_table(straddling(origin, shape, 1), "3d", "linear", FREQ)
    ok = dict(points=[(0, 0, 0)], origin=origin, shape=shape, stride=(1, 1, 1), mod=1.0)
    out = torch.full(shape, SENTINEL, dtype=torch.float64, device=gpu)
    n0 = hip.launches

    def refused(table=tab, **kw):
        with pytest.raises((HipError, ValueError)):
            hip.scene_sample(table, "eps", **dict(ok, **kw))
        assert hip.launches == n0 and bool((out == SENTINEL).all())

    # more objects than the table holds: the host format refuses them, and so does the op
    one = {"shape": "sphere", "center": [1.3, 1.3, 1.3], "radius": 1.37, "eps": 2.0}
    with pytest.raises(ValueError, match="the table holds"):
        build_table([one] * (SCENE_MAX_OBJECTS + 1))
    big = build_table([one] * SCENE_MAX_OBJECTS)
    big.ents = big.ents.repeat(2)[:SCENE_MAX_OBJECTS + 1]
    refused(table=big, out=out)
    refused(points=[], out=out)
    refused(points=[(0, 0, 0)] * 9, out=out)
    refused(points=[(0, 0, 0)] * 3, out=out)
    refused(stride=(1, 1, 3), out=out)
    refused(out=torch.full(shape, SENTINEL, dtype=torch.float32, device=gpu))
    wide = torch.full((4, 3, 12), SENTINEL, dtype=torch.float64, device=gpu)
    refused(out=wide[:, :, ::2])                      # not contiguous
    assert bool((wide == SENTINEL).all())
    refused(out=out[:3])                              # shape mismatch
    refused(shape=(4, 3, 7), out=out)
    refused(out=torch.full(shape, SENTINEL, dtype=torch.float64))  # not on the device
    # the entry point itself: null pointers, a negative shape, a bad point count, too many objects
    f = hip.lib.raw.fdtd_scene_sample
    f.restype = ctypes.c_int
    i3 = ctypes.c_int * 3
    dev_tab = hip._scene_table(tab)
    assert dev_tab.numel() == len(tab) * SCENE_ENT_SIZE

    def entry(tab_p=dev_tab.data_ptr(), nobj=len(tab), pts=i3(0, 0, 0), npts=1, org=i3(0, 0, 0), shp=i3(*shape),
              std=i3(1, 1, 1), out_p=out.data_ptr(), q=0, side_p=None, side_bytes=0, tris_p=None, ntris=0):
        vp = ctypes.c_void_p
        return f(vp(tab_p), ctypes.c_int(nobj), ctypes.c_int(q), pts, ctypes.c_int(npts), org, shp, std,
                 ctypes.c_double(1.0), ctypes.c_int(1), vp(out_p), vp(torch.cuda.current_stream().cuda_stream),
                 vp(side_p), ctypes.c_size_t(side_bytes), vp(tris_p), ctypes.c_int(ntris), vp(None))

    # (and what eps and omega have none of: a side table or its size, triangles without ranges)
    for kw in (dict(tab_p=None), dict(out_p=None), dict(pts=None), dict(org=None), dict(shp=None), dict(std=None),
               dict(shp=i3(4, -3, 6)), dict(npts=0), dict(npts=9), dict(npts=3), dict(nobj=-1),
               dict(nobj=SCENE_MAX_OBJECTS + 1), dict(std=i3(1, 0, 1)), dict(q=-1), dict(q=6),
               dict(side_p=dev_tab.data_ptr()), dict(side_bytes=8), dict(q=1, side_p=dev_tab.data_ptr(), side_bytes=8),
               dict(tris_p=dev_tab.data_ptr()), dict(ntris=1)):
        assert entry(**kw) == 1, kw   # hipErrorInvalidValue
    assert entry(shp=i3(4, 0, 6)) == 0   # an empty region: nothing launched, no error
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert entry() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


@pytest.mark.parametrize("shape", [(5, 3, 130), (9, 7, 11), (6, 70, 1)], ids=["even-z", "odd-z", "one-z"])
def test_only_the_region_is_written(hip, oracle, gpu, shape):
    """9. The region as a window of a larger sentinel-filled buffer: the
    cells before and after it stay untouched."""
    origin = (2, 1, -3)
    tab = build_table(straddling(origin, shape, 1), "3d", "linear", FREQ)
    n = shape[0] * shape[1] * shape[2]
    for pad in (512, 513):   # 16-byte aligned or not: the paired and the single stores
        buf = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.float64, device=gpu)
        out = buf[pad:pad + n].view(shape)
        got = hip.scene_sample(tab, "eps", stencil("Hy", 1), origin, shape, (1, 1, 1), 1.0, out=out)
        assert got.data_ptr() == out.data_ptr()
        want = oracle.scene_sample(tab, "eps", stencil("Hy", 1), origin, shape, (1, 1, 1), 1.0)
        assert torch.equal(out.cpu(), want)
        assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all())


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


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_one_sphere_equals_builtin_on_the_device(gpu, dtype):
    """10. One sphere from a file scene and the built-in ``sphere`` scene on
    HIP: blocked passes (two and a tail), fields bit for bit."""
    T = auto_time_block("3d", dtype, "hip", 1, 1)
    assert T > 1
    base = dict(scheme="3d", size=(32, 32, 32), time_steps=2 * T + 1, dtype=dtype, use_fused=True, time_block=0,
                sphere_center=(16.3, 15.5, 16.0), sphere_radius=6.37, sphere_eps=3.0)
    a = _run(SchemeConfig(scene="sphere", **base), "hip", gpu)
    b = _run(SchemeConfig(scene="file", scene_objects=[{"shape": "sphere", "center": [16.3, 15.5, 16.0],
                                                        "radius": 6.37, "eps": 3.0}], **base), "hip", gpu)
    assert a.tb == b.tb == T
    for c in a.comps:
        assert torch.equal(a.F[0][c], b.F[0][c]), c
    assert float(a.F[0]["Ez"].abs().max()) > 0


MULTI = [{"shape": "box", "lo": [0, 0, 0], "hi": [40, 40, 13.3], "eps": 2.25},
         {"shape": "sphere", "center": [20.3, 19.7, 18.37], "radius": 4.37, "eps": 4.0},
         {"shape": "sphere", "center": [20.7, 20.3, 27.3], "radius": 3.37, "omega_p": 1.4142135}]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("mode", ["hybrid", "stepped"])
def test_multi_object_run_vs_fp64_oracle(gpu, dtype, mode):
    """11. Substrate + dielectric sphere + Drude sphere, CPML + TF/SF with
    metamaterials, on HIP against the fp64 CPU oracle, at the tolerances of
    test_hip_gpu.py (stepped Drude runs: 5e-5 fp32, 1e-10 fp64) and
    test_hybrid_gpu.py (hybrid vs the fp64 oracle: 10 x 2e-5 fp32, 10 x 1e-12
    fp64).  (Thin layers and 2-step passes: at 40^3 the hybrid planner
    needs a core of a quarter of the grid.)"""
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
    assert any("D1" in b.upml[c] for c in b.e_comps), "no dispersive cells"
    for c in a.comps:
        scale = max(float(b.F[0][o].abs().max()) for o in b.comps if o[0] == c[0]) + 1e-300
        err = float((a.F[0][c].double().cpu() - b.F[0][c]).abs().max())
        print("%s %s %s: err %.3g of scale %.3g (tol %.1g)" % (mode, dtype, c, err, scale, tol))
        assert err <= tol * scale, (c, err, scale)
    assert float(b.F[0]["Ez"].abs().max()) > 0


def test_save_materials(gpu, tmp_path):
    """12. --save-materials on HIP writes the Eps grid the torch backend writes."""
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
                "--output-dir", str(d), "--dtype", "f32"]
        assert run(argv, out=out) == 0, out.getvalue()
        assert json.loads(out.getvalue().strip().splitlines()[-1])["scene"] == {"objects": 3}
        files[backend] = {f.name: f.read_bytes() for f in d.iterdir() if "Eps" in f.name}
    assert files["hip"] and files["hip"].keys() == files["torch"].keys()
    for name, data in files["hip"].items():
        assert data == files["torch"][name], name
