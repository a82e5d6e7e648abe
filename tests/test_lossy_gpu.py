"""Lossy media (scene-file key ``sigma``) on the GPU: the conductive E update
kernel (csrc/lossy_kernels.hip) alone against the fp64 oracle on live fields,
``scene_sample("cond")`` against its oracle bit for bit, whole CPML + TF/SF
runs with a lossy sphere (hybrid passes vs the fp64 oracle, stepped vs hybrid)
and the lost-update case: an unaligned z border of the lossy box next to a
plain window on three shell streams.  Format, physics and plan tests:
test_lossy_cpu.py.
"""

import ctypes

import numpy as np
import pytest
import torch

from fdtd3d_amd.layout.scene_file import SceneTable, build_table
from fdtd3d_amd.layout.yee import MATERIAL_STENCIL, YeeLayout
from fdtd3d_amd.models.regions import LossyCoefs
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.hip_lib import HipError

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
TOL = {"f32": 2e-5, "f64": 1e-12}   # the project's bounds, of the field scale
SENTINEL = -777.25
SHAPE = (20, 12, 37)
E, H = ("Ex", "Ey", "Ez"), ("Hx", "Hy", "Hz")
ETA = 376.730313668  # H is E / eta in a plane wave: the impedance scaling of live fields


# the same boxes on rows of 40 cells: whole 16-byte lanes, so the vector instances (4 cells fp32, 2 fp64) run
# them -- masked lanes at every z border above -- where 37 takes the one-cell instance
VSHAPE = (20, 12, 40)


def _layout(shape=SHAPE):
    return YeeLayout(shape, "3d", (0, 0, 0), (0, 0, 0), np.pi / 2, 0.0, np.pi / 2, False)


def box(x, y, z):
    return ((x[0], y[0], z[0]), (x[1], y[1], z[1]))


# z offsets 1, 2 and 3 with z widths 1, 4, 5 and 33; one x plane and one y row thick; the update range's own
# borders (index 1 along the axes the curl reads back, the last index along the others)
CASES = {
    "z1w1": {"Ex": box((3, 9), (2, 7), (1, 2)), "Ey": box((3, 9), (2, 7), (2, 3)), "Ez": box((3, 9), (2, 7), (3, 4))},
    "z2w4": {"Ex": box((2, 6), (1, 5), (2, 6)), "Ey": box((2, 6), (1, 5), (1, 5)), "Ez": box((2, 6), (1, 5), (3, 7))},
    "z3w5": {"Ex": box((5, 11), (4, 9), (3, 8)), "Ey": box((5, 11), (4, 9), (2, 7)), "Ez": box((5, 11), (4, 9), (1, 6))},
    "z1w33": {"Ex": box((1, 4), (3, 6), (1, 34)), "Ey": box((1, 4), (3, 6), (2, 35)), "Ez": box((1, 4), (3, 6), (3, 36))},
    "xplane": {"Ex": box((7, 8), (1, 12), (1, 37)), "Ey": box((7, 8), (0, 12), (1, 37)), "Ez": box((7, 8), (1, 12), (0, 37))},
    "yrow": {"Ex": box((0, 20), (5, 6), (1, 37)), "Ey": box((1, 20), (5, 6), (1, 37)), "Ez": box((1, 20), (5, 6), (0, 37))},
    "whole": {"Ex": box((0, 20), (1, 12), (1, 37)), "Ey": box((1, 20), (0, 12), (1, 37)),
              "Ez": box((1, 20), (1, 12), (0, 37))},
    "one-comp": {"Ey": box((4, 9), (0, 3), (5, 11))},
}


def _state(dtype, seed, SHAPE=SHAPE):
    """Live impedance-scaled fields (fp64 masters) and coefficients over the
    whole array's storage box: ca in [-0.9, 1] with 0 and 1 included."""
    g = torch.Generator().manual_seed(seed)
    f = {c: torch.randn(SHAPE, generator=g, dtype=torch.float64) for c in E}
    f.update({c: torch.randn(SHAPE, generator=g, dtype=torch.float64) / ETA for c in H})
    ca = {c: torch.rand(SHAPE, generator=g, dtype=torch.float64) * 1.9 - 0.9 for c in E}
    for c in E:
        ca[c].view(-1)[::7] = 0.0
        ca[c].view(-1)[3::7] = 1.0
    cb = {c: (torch.rand(SHAPE, generator=g, dtype=torch.float64) + 0.5) * 0.5 * ETA for c in E}
    return f, ca, cb


def _coefs(store, ca, cb, dt, device, SHAPE=SHAPE):
    k = LossyCoefs(store, E, dt, device)
    sl = tuple(slice(k.box[0][d], min(k.box[1][d], SHAPE[d])) for d in range(3))
    loc = tuple(slice(0, s.stop - s.start) for s in sl)
    for c in E:
        k.ca[c][loc] = ca[c][sl].to(dt).to(device)
        k.cb[c][loc] = cb[c][sl].to(dt).to(device)
    return k


@pytest.mark.parametrize("nz", [37, 40])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_vs_fp64_oracle(gpu, dtype, case, nz):
    dt = DT[dtype]
    SHAPE = (20, 12, nz)
    boxes = CASES[case]
    f, ca, cb = _state(dtype, 5, SHAPE)
    # the storage box: the union of the boxes (the scheme's), region-local
    lo = tuple(min(b[0][d] for b in boxes.values()) for d in range(3))
    hi = tuple(max(b[1][d] for b in boxes.values()) for d in range(3))
    # operands rounded to the run's dtype once: both sides start from the same numbers
    f = {c: v.to(dt).double() for c, v in f.items()}
    ca = {c: v.to(dt).double() for c, v in ca.items()}
    cb = {c: v.to(dt).double() for c, v in cb.items()}
    want = {c: v.clone() for c, v in f.items()}
    make_ops("torch", _layout(SHAPE), "cpu", torch.float64).curl_update_lossy(
        boxes, want, want, _coefs((lo, hi), ca, cb, torch.float64, "cpu", SHAPE))
    dev = {c: v.to(dt).to(gpu) for c, v in f.items()}
    # sentinel-filled outputs: the cells outside the boxes
    inside = {c: torch.zeros(SHAPE, dtype=torch.bool) for c in E}
    for c, b in boxes.items():
        inside[c][tuple(slice(b[0][d], b[1][d]) for d in range(3))] = True
    for c in E:
        dev[c][~inside[c].to(gpu)] = SENTINEL
    hip = make_ops("hip", _layout(SHAPE), gpu, dt)
    n0 = hip.launches
    hip.curl_update_lossy(boxes, dev, dev, _coefs((lo, hi), ca, cb, dt, gpu, SHAPE))
    torch.cuda.synchronize()
    assert hip.launches == n0 + 1
    # the instance that ran: 16-byte lanes on whole-lane rows, one cell a lane otherwise -- never a quiet fall-back
    assert hip.lossy_lanes == (1 if nz % 4 else 16 // dev["Ex"].element_size()), hip.lossy_lanes
    scale = max(float(want[c].abs().max()) for c in E)
    for c in E:
        got = dev[c].cpu()
        assert bool((got[~inside[c]] == SENTINEL).all()), (case, c, "a cell outside the boxes was written")
        if c in boxes:
            err = float((got.double() - want[c])[inside[c]].abs().max())
            print("%s %s nz %d %s: err %.3g of scale %.3g" % (case, dtype, nz, c, err, scale))
            assert err <= TOL[dtype] * scale, (case, c, err, scale)
            assert not bool((got[inside[c]] == SENTINEL).any())
    for c in H:
        assert torch.equal(dev[c].cpu(), f[c].to(dt))


def test_host_check_refuses_reads_outside(gpu):
    dt = torch.float32
    hip = make_ops("hip", _layout(), gpu, dt)
    f = {c: torch.zeros(SHAPE, dtype=dt, device=gpu) for c in E + H}
    k = LossyCoefs(((0, 0, 0), SHAPE), E, dt, gpu)
    n0 = hip.launches
    for comp, b in (("Ex", box((0, 4), (0, 4), (1, 5))), ("Ex", box((0, 4), (1, 4), (0, 5))),
                    ("Ey", box((0, 4), (0, 4), (1, 5))), ("Ez", box((1, 4), (0, 4), (0, 5))),
                    ("Ez", box((1, 4), (1, 13), (0, 5))), ("Ey", box((1, 21), (0, 4), (1, 5)))):
        with pytest.raises(HipError):
            hip.curl_update_lossy({comp: b}, f, f, k)
    small = LossyCoefs(((2, 2, 4), (6, 6, 12)), E, dt, gpu)
    with pytest.raises(HipError):
        hip.curl_update_lossy({"Ex": box((1, 5), (2, 6), (4, 12))}, f, f, small)
    assert hip.launches == n0


# ------------------------------------------------------------------ sampling
def _objects(origin, shape, mesh):
    lo = [float(o) for o in origin]
    hi = [float(o + s) for o, s in zip(origin, shape)]
    mid = [(a + b) / 2 + 0.13 for a, b in zip(lo, hi)]
    objs = [{"shape": "box", "lo": [lo[0] - 2.3, lo[1] - 1.7, lo[2] - 3.1], "hi": [lo[0] + 2.37, mid[1], mid[2]],
             "eps": 2.25, "sigma": 0.7},
            {"shape": "sphere", "center": [mid[0], lo[1] - 0.3, mid[2]], "radius": 2.37, "eps": 5.0, "sigma": 2.5},
            {"shape": "sphere", "center": [hi[0] - 0.7, hi[1] + 0.37, lo[2] + 1.3], "radius": 3.37, "eps": 1.7},
            {"shape": "cylinder", "axis": "x", "center": [hi[1] - 0.37, mid[2] + 1.3], "radius": 1.73,
             "span": [lo[0] - 1.3, mid[0] + 0.37], "sigma": 0.05}]
    if mesh:
        c, r = (mid[0] - 0.4, mid[1] + 0.2, mid[2] - 0.6), 2.7
        v = [[c[0] + r, c[1], c[2]], [c[0] - r, c[1], c[2]], [c[0], c[1] + r, c[2]], [c[0], c[1] - r, c[2]],
             [c[0], c[1], c[2] + r], [c[0], c[1], c[2] - r]]
        t = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
        objs.append({"shape": "mesh", "vertices": v, "triangles": t, "eps": 1.3, "sigma": 1.1})
    return objs


@pytest.mark.parametrize("smoothing", ["linear", "none"])
@pytest.mark.parametrize("mesh", [False, True], ids=["primitives", "mesh"])
@pytest.mark.parametrize("shape,origin", [((9, 7, 11), (3, -2, 5)), ((5, 3, 130), (-4, 6, 1))],
                         ids=["9x7x11", "5x3x130"])
def test_cond_equals_oracle(gpu, shape, origin, mesh, smoothing):
    hip, oracle = make_ops("hip", None, gpu, torch.float64), make_ops("torch", None, "cpu", torch.float64)
    tab = build_table(_objects(origin, shape, mesh), "3d", smoothing, 1.5e10)
    for pts in ([(0, 0, 0)], list(MATERIAL_STENCIL["Ex"]), list(MATERIAL_STENCIL["Ez"])):
        want = oracle.scene_sample(tab, "cond", pts, origin, shape, (1, 1, 1), 1.0)
        n0 = hip.launches
        got = hip.scene_sample(tab, "cond", pts, origin, shape, (1, 1, 1), 1.0)
        assert hip.launches == n0 + 1
        assert torch.equal(got.cpu(), want), (len(pts), int((got.cpu() != want).sum()))
        assert len(torch.unique(want)) >= 4, "trivial scene"
        assert torch.equal(hip.scene_sample(tab, "cond", pts, origin, shape, (1, 1, 1), 1.0, cull=False), got)


def test_cond_table_checks(gpu):
    hip = make_ops("hip", None, gpu, torch.float64)
    shape, origin = (9, 7, 11), (3, -2, 5)
    good = build_table(_objects(origin, shape, False), "3d", "linear", 1.5e10)
    out = torch.full(shape, SENTINEL, dtype=torch.float64, device=gpu)
    n0 = hip.launches
    for bad in (np.zeros((len(good), 1)), np.zeros(len(good) + 1), np.zeros(len(good), dtype=np.float32),
                np.full(len(good), -1.0), np.full(len(good), np.nan), np.full(len(good), np.inf),
                torch.zeros(len(good), dtype=torch.float64)):
        tab = SceneTable(good.ents, good.tris, good.ranges, good.drude)
        tab.cond = bad
        with pytest.raises(HipError):
            hip.scene_sample(tab, "cond", [(0, 0, 0)], origin, shape, (1, 1, 1), 1.0, out=out)
    with pytest.raises(HipError):
        hip.scene_sample(good, "sigma", [(0, 0, 0)], origin, shape, (1, 1, 1), 1.0, out=out)
    # the entry point itself: no conductivities, a row short or a row long, the Drude table with its true size
    f = hip.lib.raw.fdtd_scene_sample
    f.restype = ctypes.c_int
    i3, vp = ctypes.c_int * 3, ctypes.c_void_p
    dev_tab, dev_cond, dev_drude = hip._scene_table(good), hip._scene_cond(good), hip._scene_drude(good)
    assert dev_cond.numel() == len(good)

    def entry(side=dev_cond, side_bytes=8 * len(good)):
        return f(vp(dev_tab.data_ptr()), ctypes.c_int(len(good)), ctypes.c_int(5), i3(0, 0, 0), ctypes.c_int(1),
                 i3(*origin), i3(*shape), i3(1, 1, 1), ctypes.c_double(1.0), ctypes.c_int(1), vp(out.data_ptr()),
                 vp(torch.cuda.current_stream().cuda_stream), vp(None if side is None else side.data_ptr()),
                 ctypes.c_size_t(side_bytes), vp(None), ctypes.c_int(0), vp(None))

    for kw in (dict(side=None), dict(side=None, side_bytes=0), dict(side_bytes=8 * (len(good) - 1)),
               dict(side_bytes=8 * (len(good) + 1)), dict(side=dev_drude, side_bytes=24 * len(good))):
        assert entry(**kw) == 1, kw   # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert hip.launches == n0 and bool((out == SENTINEL).all())
    assert entry() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


# ------------------------------------------------------------------ whole runs
SPHERE = [{"shape": "sphere", "center": [22.3, 23.1, 21.7], "radius": 3.2, "eps": 3.0, "sigma": 4.0}]
RUN = dict(scheme="3d", size=(44, 46, 44), time_steps=14, use_pml=True, pml_type="cpml", pml_size=(4, 4, 4),
           use_tfsf=True, tfsf_size=(8, 8, 8), scene="file", scene_objects=SPHERE, use_fused=True,
           hybrid_tfsf="core")
# (44 x 46 x 44 has a hybrid plan around the sphere's box for 2-step passes with the TF/SF faces in the blocked
# core; with the faces in the stepped shell, or 3-step passes, the core falls under a quarter of the grid)


def _run(cfg, backend, device):
    s = YeeScheme(cfg, make_ops(backend, None, device, DT[cfg.dtype]))
    s.init_scheme()
    s.init_grids()
    s.perform_steps()
    if device != "cpu":
        torch.cuda.synchronize()
    return s


@pytest.fixture(scope="module")
def oracle_run():
    return _run(SchemeConfig(dtype="f64", hybrid_block=1, time_block=1, **RUN), "torch", "cpu")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_hybrid_run_vs_fp64_oracle_and_stepped(gpu, oracle_run, dtype):
    T = 2
    h = _run(SchemeConfig(dtype=dtype, hybrid_block=T, **RUN), "hip", gpu)
    assert h.lossy is not None and h.hybrid is not None and h.hybrid["T"] == T and not h.fused and h.tb == 1
    assert h.ops.lossy_lanes == (4 if dtype == "f32" else 2)
    assert h.hybrid["cut_cells"] > 0
    b = oracle_run
    assert b.lossy is not None and float(b.lossy["coefs"].ca["Ez"].min()) < 0.95
    for c in h.comps:
        scale = max(float(b.F[0][o].abs().max()) for o in b.comps if o[0] == c[0]) + 1e-300
        err = float((h.F[0][c].double().cpu() - b.F[0][c]).abs().max())
        print("hybrid %s %s: err %.3g of scale %.3g" % (dtype, c, err, scale))
        assert err <= TOL[dtype] * scale, (c, err, scale)
    assert float(b.F[0]["Ez"].abs().max()) > 0
    s = _run(SchemeConfig(dtype=dtype, hybrid_block=1, time_block=1, **RUN), "hip", gpu)
    assert s.lossy is not None and s.hybrid is None and s.tb == 1 and not s.fused
    # (the blocked core contracts its arithmetic differently from the step kernels: the project's bound, as in
    # test_hybrid_gpu.py, not bit for bit)
    for c in h.comps:
        scale = max(float(s.F[0][o].abs().max()) for o in s.comps if o[0] == c[0]) + 1e-300
        err = float((h.F[0][c] - s.F[0][c]).abs().max())
        print("hybrid vs stepped %s %s: err %.3g of scale %.3g" % (dtype, c, err, scale))
        assert err <= TOL[dtype] * scale, (c, "stepped vs hybrid", err, scale)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_unaligned_z_border_on_three_streams(gpu, dtype):
    """The lost-update case: the lossy box's z borders (18 and 25: neither a
    multiple of 4) cut 16-byte lanes that the plain windows next to it own
    the rest of, and all of them are in flight on three shell streams.  A
    launch that stored a neighbour's element would lose that window's update
    (an error of the size of a step's change, far above round-off): the run
    must equal the one on a single stream bit for bit, and the stepped one at
    the project's bound."""
    objs = [{"shape": "box", "lo": [19.2, 19.2, 18.6], "hi": [25.7, 26.3, 25.4], "eps": 2.0, "sigma": 6.0}]
    base = dict(RUN, scene_objects=objs, scene_smoothing="none", time_steps=12)
    runs = {n: _run(SchemeConfig(dtype=dtype, hybrid_block=2, shell_streams=n, **base), "hip", gpu) for n in (3, 1)}
    g = runs[3].lossy["gbox"]
    assert g[0][2] % 4 != 0 and g[1][2] % 4 != 0, g
    assert runs[3].hybrid is not None
    s = _run(SchemeConfig(dtype=dtype, hybrid_block=1, time_block=1, **base), "hip", gpu)
    it = torch.int32 if dtype == "f32" else torch.int64
    for c in s.comps:
        assert float(s.F[0][c].abs().max()) > 0
        assert torch.equal(runs[3].F[0][c].view(it), runs[1].F[0][c].view(it)), (c, "three streams != one")
        scale = max(float(s.F[0][o].abs().max()) for o in s.comps if o[0] == c[0])
        err = float((runs[3].F[0][c] - s.F[0][c]).abs().max())
        print("three streams vs stepped %s %s: err %.3g of scale %.3g" % (dtype, c, err, scale))
        assert err <= TOL[dtype] * scale, (c, "hybrid vs stepped", err, scale)
