#!/usr/bin/env python
"""File scenes on one GPU (layout/scene_file.py, csrc/scene_kernels.hip).

    python tools/scene_bench.py op [N=512] [objects=16]
        the scene_sample op alone over an N^3 region: a 1-point and an 8-point
        stencil, eps and omega, with and without culling (HIP events over 5
        calls after a warm-up call), and the torch op on the device once, with
        its peak memory -- and whether it gives the kernel's bits

    python tools/scene_bench.py init [N=512] [objects=16] [backend=hip]
        init_grids time and peak device memory of an N^3 fp32 run of the
        `objects`-object scene (dielectric and Drude spheres on a substrate,
        --use-metamaterials) through the backend's op; backend torch = the
        torch op on the device.  One process per call: the peak is the
        process's.

    python tools/scene_bench.py mesh [N=256] [subdivisions=5]
        one mesh, an icosphere of 20 * 4^subdivisions triangles (20 480) of
        radius 0.3 N in an N^3 region, beside the analytic sphere of the same
        radius: time per component (a 1-point and an 8-point stencil, eps
        linear / eps none / omega), culled and not, and the share of
        (wave, triangle) pairs the per-wave culling lets through

    python tools/scene_bench.py drude [N=256] [objects=16]
        the Drude quantities of a damped, double-negative version of the
        scene, per field component (its own stencil, a 1- and a 2-fold eps
        grid): omega_m, gamma and gamma_m next to omega on the same box in the
        same process (HIP events over 5 calls after a warm-up call), and
        whether the torch op on the device gives the kernel's bits

Results: profiles/scene.md.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fdtd3d_amd.layout.scene_file import build_table  # noqa: E402
from fdtd3d_amd.layout.yee import MATERIAL_STENCIL, MATERIAL_STENCIL_DOUBLE  # noqa: E402
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme  # noqa: E402
from fdtd3d_amd.ops import make_ops  # noqa: E402


def scene(n, count):
    """A substrate and `count` - 1 spheres of radius n / 16 spread over the
    grid (a fixed seed), every third one a Drude sphere."""
    g = torch.Generator().manual_seed(2)
    objs = [{"shape": "box", "lo": [0, 0, 0], "hi": [n, n, n / 8 + 0.3], "eps": 2.25}]
    for k in range(count - 1):
        c = (torch.rand(3, generator=g, dtype=torch.float64) * (0.7 * n) + 0.15 * n).tolist()
        o = {"shape": "sphere", "center": c, "radius": n / 16 + 0.37}
        o.update({"omega_p": 1.4142135} if k % 3 == 2 else {"eps": 2.0 + 0.25 * k})
        objs.append(o)
    return objs


def op(n, count):
    dev = "cuda:0"
    hip = make_ops("hip", None, dev, torch.float64)
    tor = make_ops("torch", None, dev, torch.float64)
    tab = build_table(scene(n, count), "3d", "linear", 1.5e10)
    shape = (n, n, n)
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    pts8 = [tuple(2 * b[a] + s[a] for a in range(3)) for b, s in MATERIAL_STENCIL_DOUBLE["Ex"]]
    print("| region | objects | points | quantity | culled us | all objects us | torch op on the device ms "
          "(peak GB) | same bits |")
    print("|---|---|---|---|---|---|---|---|")
    for pts, stride, mod in (([(0, 0, 0)], (1, 1, 1), 1.0), (pts8, (2, 2, 2), 2.0)):
        for q in ("eps", "omega"):
            us = []
            for cull in (True, False):
                hip.scene_sample(tab, q, pts, (0, 0, 0), shape, stride, mod, out=out, cull=cull)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(5):
                    hip.scene_sample(tab, q, pts, (0, 0, 0), shape, stride, mod, out=out, cull=cull)
                b.record()
                torch.cuda.synchronize()
                us.append(a.elapsed_time(b) / 5 * 1e3)
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = tor.scene_sample(tab, q, pts, (0, 0, 0), shape, stride, mod)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            peak = (torch.cuda.max_memory_allocated() - base) / 1e9
            same = bool(torch.equal(ref, out))
            del ref
            print("| %d^3 | %d | %d | %s | %.0f | %.0f | %.0f (%.1f) | %s |"
                  % (n, len(tab), len(pts), q, us[0], us[1], ms, peak, same), flush=True)


def drude(n, count):
    dev = "cuda:0"
    hip = make_ops("hip", None, dev, torch.float64)
    tor = make_ops("torch", None, dev, torch.float64)
    objs = scene(n, count)
    for k, o in enumerate(objs[1:]):   # every sphere a metal: damped, every second one with a damped magnetic pole
        o.update(omega_p=1.0 + 0.05 * k, gamma=0.1 + 0.02 * k)
        if k % 2:
            o.update(omega_pm=0.8 + 0.05 * k, gamma_m=0.05 + 0.01 * k)
    tab = build_table(objs, "3d", "linear", 1.5e10)
    shape = (n, n, n)
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    print("| region | objects | component | points | omega us | omega_m us | gamma us | gamma_m us | gamma / omega "
          "| same bits |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for mod in (1, 2):
        for comp in ("Ex", "Ey", "Ez", "Hx", "Hy", "Hz"):
            pts = (list(MATERIAL_STENCIL[comp]) if mod == 1 else
                   [tuple(2 * b[a] + s[a] for a in range(3)) for b, s in MATERIAL_STENCIL_DOUBLE[comp]])
            us, same = {}, True
            for q in ("omega", "omega_m", "gamma", "gamma_m"):
                hip.scene_sample(tab, q, pts, (0, 0, 0), shape, (mod,) * 3, float(mod), out=out)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(5):
                    hip.scene_sample(tab, q, pts, (0, 0, 0), shape, (mod,) * 3, float(mod), out=out)
                b.record()
                torch.cuda.synchronize()
                us[q] = a.elapsed_time(b) / 5 * 1e3
                if comp in ("Ex", "Hz"):   # (the torch op: seconds a call)
                    same = same and bool(torch.equal(tor.scene_sample(tab, q, pts, (0, 0, 0), shape, (mod,) * 3,
                                                                      float(mod)), out))
            print("| %d^3 | %d | %s | %d | %.0f | %.0f | %.0f | %.0f | %.2f | %s |"
                  % (n, len(tab), comp, len(pts), us["omega"], us["omega_m"], us["gamma"], us["gamma_m"],
                     us["gamma"] / us["omega"], same if comp in ("Ex", "Hz") else "-"), flush=True)


def icosphere(c, r, subdivisions):
    """(vertices, triangles) of an icosahedron subdivided onto the sphere."""
    import numpy as np
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / (1 + g * g) ** 0.5 for p in v]
    for _ in range(subdivisions):
        mid, nt = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c_ in t:
            ab, bc, ca = m(a, b), m(b, c_), m(c_, a)
            nt += [(a, ab, ca), (b, bc, ab), (c_, ca, bc), (ab, bc, ca)]
        t = nt
    return [[float(c[a] + r * p[a]) for a in range(3)] for p in v], [list(x) for x in t]


def mesh(n, subdivisions):
    import numpy as np
    dev = "cuda:0"
    hip = make_ops("hip", None, dev, torch.float64)
    c, r = [n / 2 + 0.37, n / 2 - 0.21, n / 2 + 0.13], 0.3 * n
    v, t = icosphere(c, r, subdivisions)
    shape = (n, n, n)
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    pts8 = [tuple(2 * b[a] + s[a] for a in range(3)) for b, s in MATERIAL_STENCIL_DOUBLE["Ex"]]
    print("| region | object | points | quantity | culled ms | not culled ms |")
    print("|---|---|---|---|---|---|")
    for name, obj in (("sphere", {"shape": "sphere", "center": c, "radius": r}),
                      ("mesh %d" % len(t), {"shape": "mesh", "vertices": v, "triangles": t})):
        obj.update(eps=2.56, omega_p=1.0)
        for pts, stride, mod in (([(0, 0, 0)], (1, 1, 1), 1.0), (pts8, (2, 2, 2), 2.0)):
            for q, smoothing in (("eps", "linear"), ("eps", "none"), ("omega", "linear")):
                tab = build_table([obj], "3d", smoothing, 1.5e10)
                ms = []
                for cull in (True, False):
                    if not cull and name != "sphere" and len(pts) > 1:
                        ms.append(float("nan"))   # (minutes: every triangle at every point)
                        continue
                    reps = 3 if cull else 1
                    hip.scene_sample(tab, q, pts, (0, 0, 0), shape, stride, mod, out=out, cull=cull)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    for _ in range(reps):
                        hip.scene_sample(tab, q, pts, (0, 0, 0), shape, stride, mod, out=out, cull=cull)
                    b.record()
                    torch.cuda.synchronize()
                    ms.append(a.elapsed_time(b) / reps)
                print("| %d^3 | %s | %d | %s %s | %.2f | %.2f |"
                      % (n, name, len(pts), q, smoothing if q == "eps" else "", ms[0], ms[1]), flush=True)
    # what the per-wave culling lets through, 1-point stencil: waves are (x, y) columns of 128 cells along z
    tr = np.asarray(v)[np.asarray(t)]
    lo, hi = tr.min(axis=1), tr.max(axis=1)
    zl = 0
    while zl < 6 and (2 << zl) < n:
        zl += 1
    rows, zc = 64 >> zl, 2 << zl
    par = dist = 0
    for z0 in range(0, n, zc):
        z1 = min(z0 + zc, n) - 1 + 0.5
        for y0 in range(0, n, rows):
            ya, yb = y0 + 0.5, min(y0 + rows, n) - 1 + 0.5
            x = np.arange(n)[:, None] + 0.5
            iny = (hi[:, 1] >= ya) & (lo[:, 1] <= yb) & (hi[:, 2] >= z0 + 0.5)
            par += int(((hi[None, :, 0] >= x) & (lo[None, :, 0] <= x) & iny[None]).sum())
            near = ~((lo[:, 1] - yb > 1) | (ya - hi[:, 1] > 1) | (lo[:, 2] - z1 > 1) | (z0 + 0.5 - hi[:, 2] > 1))
            dist += int((~((lo[None, :, 0] - x > 1) | (x - hi[None, :, 0] > 1)) & near[None]).sum())
    waves = n * -(-n // rows) * -(-n // zc)
    print("culling, 1 point: %d waves x %d triangles; parity keeps %.4f %% of the pairs (%.1f per wave), "
          "distance %.4f %% (%.1f per wave)" % (waves, len(t), 100.0 * par / (waves * len(t)), par / waves,
                                               100.0 * dist / (waves * len(t)), dist / waves))


def init(n, count, backend):
    dev = "cuda:0"
    cfg = SchemeConfig(scheme="3d", size=(n, n, n), time_steps=0, scene="file", scene_objects=scene(n, count),
                       dtype="f32", use_fused=True, use_metamaterials=True)
    s = YeeScheme(cfg, make_ops("hip", None, dev, torch.float32))
    if backend == "torch":
        # the same scheme, the scene through the torch op on the device
        tor = make_ops("torch", None, dev, torch.float64)
        s.ops.scene_sample = tor.scene_sample
    s.init_scheme()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.init_grids()
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    print("| %d^3 fp32 | %d | %s | %.2f | %.1f | %.1f | %.1f |"
          % (n, count, backend, sec, torch.cuda.max_memory_allocated() / 1e9, torch.cuda.memory_allocated() / 1e9,
             sum(s.mem_plan.values()) / 1e9), flush=True)


def main(argv):
    mode = argv[0] if argv else "op"
    n = int(argv[1]) if len(argv) > 1 else 512
    count = int(argv[2]) if len(argv) > 2 else 16
    if mode == "op":
        op(n, count)
    elif mode == "drude":
        drude(int(argv[1]) if len(argv) > 1 else 256, count)
    elif mode == "mesh":
        mesh(int(argv[1]) if len(argv) > 1 else 256, int(argv[2]) if len(argv) > 2 else 5)
    elif mode == "init":
        init(n, count, argv[3] if len(argv) > 3 else "hip")
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
