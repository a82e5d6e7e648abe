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

Results: profiles/scene.md.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fdtd3d_amd.layout.scene_file import build_table  # noqa: E402
from fdtd3d_amd.layout.yee import MATERIAL_STENCIL_DOUBLE  # noqa: E402
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
    elif mode == "init":
        init(n, count, argv[3] if len(argv) > 3 else "hip")
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
