"""Measurements for profiles/sources.md: what a source list costs, and the
power a soft dipole radiates.

    python tools/source_bench.py rate [--size 512] [--steps 100] [--dtype f32] [--cells 0,1,64,4096]
                                      [--repeat 1] [--phases]
    python tools/source_bench.py dipole [--size 96] [--ppw 20]

``rate``: Mcells/s of a CPML run driven by the built-in point source and by
source lists of 1, 64 and 4096 cells (soft pulses on Ez, a square patch
around the centre), with the hybrid plan's core share.  ``dipole``: the power
of one soft sine Ez dipole through a flux box against the Hertzian dipole's
``eta0 k^2 (I l)^2 / (12 pi)`` with ``I l = eps0 a dx^3 / dt``.  One JSON line
per measurement.
"""

import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme  # noqa: E402
from fdtd3d_amd.ops import make_ops  # noqa: E402
from fdtd3d_amd.utils.constants import EPS0, MU0, PI, SPEED_OF_LIGHT  # noqa: E402


def _scheme(cfg, device):
    dt = torch.float32 if cfg.dtype == "f32" else torch.float64
    s = YeeScheme(cfg, make_ops("hip" if device != "cpu" else "torch", None, device, dt))
    s.init_scheme()
    s.init_grids()
    return s


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def patch(n_cells: int, size: int):
    """``n_cells`` soft pulse entries on Ez: a square patch in the centre's z plane."""
    side = int(round(math.sqrt(n_cells)))
    c = size // 2
    return [{"component": "Ez", "cell": [c - side // 2 + i, c - side // 2 + j, c], "waveform": "pulse",
             "amplitude": 1.0 / n_cells} for i in range(side) for j in range(side)]


def rate(args):
    n = args.size
    for cells in [int(c) for c in args.cells.split(",")] * args.repeat:
        # (0 cells: the built-in point source, and no `sources` argument: this also runs on a commit without it)
        kw = {"sources": patch(cells, n)} if cells else {}
        cfg = SchemeConfig(scheme="3d", size=(n, n, n), time_steps=args.steps, scene="vacuum", dtype=args.dtype,
                           use_pml=True, pml_type="cpml", pml_size=(10, 10, 10), use_fused=True, hybrid_block=0, **kw)
        cfg.profile_phases = args.phases
        s = _scheme(cfg, args.device)
        T = s.hybrid["T"] if s.hybrid is not None else 1
        s.advance(2 * T)
        _sync(args.device)
        s.prof.reset()
        steps = args.steps // T * T
        t0 = time.perf_counter()
        s.advance(steps)
        _sync(args.device)
        sec = time.perf_counter() - t0
        rec = {"what": "rate", "size": n, "dtype": args.dtype, "source": "built-in" if not cells else "list",
               "cells": cells, "steps": steps, "mcells_per_s": n ** 3 * steps / sec / 1e6,
               "hybrid_T": T if s.hybrid is not None else None,
               "core_share": s.hybrid["core_cells"] / n ** 3 if s.hybrid is not None else None}
        if args.phases:
            rec["phases"] = s.prof.summary()  # per-phase HIP event timers (they cost some rate themselves)
        print(json.dumps(rec), flush=True)
        del s
        if args.device != "cpu":
            torch.cuda.empty_cache()


def dipole(args):
    from fdtd3d_amd.models.flux import FluxMonitor
    n, ppw = args.size, args.ppw
    dx = 0.0005
    wl = ppw * dx
    a = 1.0
    periods = 24
    cfg = SchemeConfig(scheme="3d", size=(n, n, n), scene="vacuum", dtype="f64", dx=dx, wavelength=wl,
                       use_pml=True, pml_type="cpml", pml_size=(10, 10, 10), use_fused=True,
                       sources=[{"component": "Ez", "cell": [n // 2, n // 2, n // 2], "waveform": "sine", "ramp": 4 * 2 * ppw,
                                 "amplitude": a}])
    per = int(round(ppw / cfg.courant))  # steps per period
    cfg.time_steps = periods * per
    s = _scheme(cfg, args.device)
    # whole periods of the steady state: the last 8
    mon = FluxMonitor(s, (16, 16, 16), [wl], step=1, start=(periods - 8) * per + 1)
    s.advance(cfg.time_steps)
    _sync(args.device)
    got = float(mon.net()[0])
    il = EPS0 * a * dx ** 3 / s.dt
    k = 2 * PI / wl
    want = math.sqrt(MU0 / EPS0) * k * k * il * il / (12 * PI)
    print(json.dumps({"what": "dipole", "size": n, "cells_per_wavelength": ppw, "steps": cfg.time_steps,
                      "flux_box_margin": 16, "samples": mon.samples, "hybrid": s.hybrid is not None,
                      "radiated_W": got, "hertzian_W": want, "ratio": got / want}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rate", "dipole"))
    ap.add_argument("--size", type=int, default=0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--ppw", type=int, default=20)
    ap.add_argument("--cells", default="0,1,64,4096", help="rate: list sizes, comma separated; 0 = the built-in source")
    ap.add_argument("--repeat", type=int, default=1, help="rate: run the whole --cells sequence this many times")
    ap.add_argument("--phases", action="store_true", help="rate: per-phase timers in each record")
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    args = ap.parse_args()
    if not args.size:
        args.size = 512 if args.what == "rate" else 96
    (rate if args.what == "rate" else dipole)(args)


if __name__ == "__main__":
    main()
