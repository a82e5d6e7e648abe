"""Measurements for profiles/lossy.md: what a lossy medium (scene-file key
``sigma``) costs, against the same scene without it and against the Drude
emulation it replaces, and the conductive update kernel's own rate.

    python tools/lossy_bench.py rate [--size 512] [--steps 100] [--dtype f32] [--variants plain,zero,sigma,drude]
                                     [--repeat 1] [--tree PATH]
    python tools/lossy_bench.py kernel [--box 150] [--size 512] [--dtype f32] [--iters 50]

``rate``: Mcells/s of a CPML + TF/SF run around a dielectric sphere (eps 3,
radius an eighth of the grid) -- ``plain``: no ``sigma`` key at all (runs on a
commit without the key: ``--tree`` imports the package from another checkout,
for alternating runs against the parent), ``zero``: ``sigma`` 0, ``sigma``: a
lossy sphere (s = 0.05), ``drude``: the same conductivity emulated by a Drude
pole with ``gamma`` = 50 and ``omega_p^2 / gamma`` = ``sigma / (eps0 w)`` under
``--use-metamaterials``.  ``kernel``: ``ops.curl_update_lossy`` alone on a
cubic box inside a ``--size`` grid, HIP events around ``--iters`` launches,
with the bytes it must move: 3 E read + written, 3 H read, 6 coefficients.
One JSON line per measurement.
"""

import argparse
import json
import math
import os
import sys
import time


def _tree(argv):
    for i, a in enumerate(argv):
        if a == "--tree" and i + 1 < len(argv):
            return os.path.abspath(argv[i + 1])
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


sys.path.insert(0, _tree(sys.argv))

import torch  # noqa: E402

from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme  # noqa: E402
from fdtd3d_amd.ops import make_ops  # noqa: E402
from fdtd3d_amd.utils.constants import EPS0, PI, SPEED_OF_LIGHT  # noqa: E402

S_HALF = 0.05  # sigma dt / (2 eps0 eps_r) of the lossy sphere
EPS = 3.0
GAMMA = 50.0   # the emulation's collision frequency, in units of 2 pi f


def _scheme(cfg, device):
    dt = torch.float32 if cfg.dtype == "f32" else torch.float64
    s = YeeScheme(cfg, make_ops("hip" if device != "cpu" else "torch", None, device, dt))
    s.init_scheme()
    s.init_grids()
    return s


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def sphere(variant: str, n: int, cfg0):
    dt = cfg0.dx * cfg0.courant / SPEED_OF_LIGHT
    sigma = S_HALF * 2 * EPS0 * EPS / dt
    o = {"shape": "sphere", "center": [n / 2 + 0.3, n / 2 - 0.2, n / 2 + 0.1], "radius": n / 8, "eps": EPS}
    if variant == "zero":
        o["sigma"] = 0.0
    elif variant == "sigma":
        o["sigma"] = sigma
    elif variant == "drude":
        w0 = 2 * PI * SPEED_OF_LIGHT / cfg0.wavelength
        o["gamma"] = GAMMA
        o["omega_p"] = math.sqrt(GAMMA * sigma / (EPS0 * w0))
    return [o]


def rate(args):
    n = args.size
    for variant in args.variants.split(",") * args.repeat:
        cfg = SchemeConfig(scheme="3d", size=(n, n, n), time_steps=args.steps, dtype=args.dtype, use_pml=True,
                           pml_type="cpml", pml_size=(10, 10, 10), use_tfsf=True, tfsf_size=(20, 20, 20),
                           scene="file", use_fused=True, hybrid_block=0, use_metamaterials=variant == "drude")
        cfg.scene_objects = sphere(variant, n, cfg)
        s = _scheme(cfg, args.device)
        T = s.hybrid["T"] if s.hybrid is not None else 1
        s.advance(2 * T)
        _sync(args.device)
        steps = args.steps // T * T
        t0 = time.perf_counter()
        s.advance(steps)
        _sync(args.device)
        sec = time.perf_counter() - t0
        lossy = getattr(s, "lossy", None)
        print(json.dumps({"what": "rate", "variant": variant, "tree": os.path.basename(_tree(sys.argv)), "size": n,
                          "dtype": args.dtype, "steps": steps, "mcells_per_s": n ** 3 * steps / sec / 1e6,
                          "hybrid_T": T if s.hybrid is not None else None,
                          "core_share": s.hybrid["core_cells"] / n ** 3 if s.hybrid is not None else None,
                          "lossy_box": lossy["gbox"] if lossy else None,
                          "upml_chain": bool(s.use_upml_chain)}), flush=True)
        del s
        if args.device != "cpu":
            torch.cuda.empty_cache()


def kernel(args):
    from fdtd3d_amd.layout.yee import YeeLayout
    from fdtd3d_amd.models.regions import LossyCoefs
    n, b = args.size, args.box
    dt = torch.float32 if args.dtype == "f32" else torch.float64
    lay = YeeLayout((n, n, n), "3d", (0, 0, 0), (0, 0, 0), PI / 2, 0.0, PI / 2, False)
    ops = make_ops("hip", lay, args.device, dt)
    comps = ("Ex", "Ey", "Ez")
    f = {c: torch.randn((n, n, n), dtype=dt, device=args.device) * 1e-3 for c in comps + ("Hx", "Hy", "Hz")}
    for lo in (n // 2 - b // 2, n // 2 - b // 2 + 1):   # an aligned and an unaligned z start
        box = ((n // 2 - b // 2,) * 2 + (lo,), (n // 2 - b // 2 + b,) * 2 + (lo + b,))
        k = LossyCoefs(box, comps, dt, args.device)
        for c in comps:
            k.ca[c].fill_(0.9)
            k.cb[c].fill_(1e-3)
        boxes = {c: box for c in comps}
        for _ in range(5):
            ops.curl_update_lossy(boxes, f, f, k)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(args.iters):
            ops.curl_update_lossy(boxes, f, f, k)
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / args.iters
        nbytes = 15 * b ** 3 * f["Ex"].element_size()
        print(json.dumps({"what": "kernel", "dtype": args.dtype, "grid": n, "box": b, "z_start": lo,
                          "lanes": ops.lossy_lanes, "us": ms * 1e3, "bytes": nbytes,
                          "tb_per_s": nbytes / (ms * 1e-3) / 1e12,
                          "mcells_per_s": b ** 3 / (ms * 1e-3) / 1e6}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rate", "kernel"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--variants", default="plain,zero,sigma,drude")
    ap.add_argument("--repeat", type=int, default=1, help="rate: run the whole --variants sequence this many times")
    ap.add_argument("--tree", default="", help="import fdtd3d_amd from this checkout (the parent commit's, say)")
    ap.add_argument("--box", type=int, default=150, help="kernel: the cubic box's edge")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    args = ap.parse_args()
    (rate if args.what == "rate" else kernel)(args)


if __name__ == "__main__":
    main()
