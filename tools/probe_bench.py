#!/usr/bin/env python
"""The probe monitor on one GPU (models/probe.py, csrc/probe_kernels.hip).

    python tools/probe_bench.py sample [points=64] [N=256] [dtype=f32]
        time of one sample of `points` centre probes (every component) spread
        over an N^3 vacuum grid: HIP events over 200 calls after a warm-up
        call, the launch included

    python tools/probe_bench.py run [steps=400] [rounds=3] [points=64] -- <driver options>
        steady-state Mcells/s of the run the driver options describe, with and
        without the monitor at its automatic step (the pass length: no pass is
        cut), alternated in ONE process on ONE scheme (box-to-box spread is
        ~10 %: never compare sessions); a warm-up of `steps` steps first, the
        discipline of bench.py

Results: profiles/probes.md.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fdtd3d_amd.models.probe import ProbeMonitor  # noqa: E402
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme  # noqa: E402
from fdtd3d_amd.ops import make_ops  # noqa: E402


def spread_points(size, count):
    """`count` cells spread over the interior of the grid (a fixed seed)."""
    g = torch.Generator().manual_seed(1)
    cols = [torch.randint(1, max(2, size[a] - 1), (count,), generator=g) if size[a] > 1 else None for a in range(3)]
    return [tuple(int(c[i]) for c in cols if c is not None) for i in range(count)]


def sample(points, n, dt):
    dtype = torch.float32 if dt == "f32" else torch.float64
    cfg = SchemeConfig(scheme="3d", size=(n, n, n), scene="vacuum", dtype=dt, use_fused=True, time_block=0)
    s = YeeScheme(cfg, make_ops("hip", None, "cuda:0", dtype))
    s.init_scheme()
    s.init_grids()
    s.randomize_fields()
    m = ProbeMonitor(s, spread_points(cfg.size, points), position="centre", register=False)
    ops = s.ops
    ops.probe_sample(m.entries, 0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    reps = 200
    a.record()
    for _ in range(reps):
        ops.probe_sample(m.entries, 0)
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) / reps * 1e3
    print("| %d^3 %s | %d | %d | %.1f |" % (n, dt, points, len(m.entries), us), flush=True)


def run(steps, rounds, points, argv):
    from fdtd3d_amd.runner import build
    from fdtd3d_amd.utils.settings import setup_from_cmd
    status, settings = setup_from_cmd(argv)
    if status:
        return status
    s, _, _ = build(settings)
    s.init_scheme()
    s.init_grids()
    m = ProbeMonitor(s, spread_points(s.cfg.size, points), position="centre", register=False)
    cells = s.cells()

    def timed(with_monitor):
        if with_monitor:
            s.add_periodic(m.step, 0, m.sample)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.advance(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if with_monitor:
            s.periodic.pop()
        return cells * steps / dt / 1e6

    s.advance(steps)  # warm-up
    print("%d points, %d slots, monitor step %d, %d steps per measurement" % (points, len(m.entries), m.step, steps))
    print("| round | without Mcells/s | with Mcells/s | cost |")
    print("|---:|---:|---:|---:|", flush=True)
    tot = [0.0, 0.0]
    for r in range(rounds):
        a, b = timed(False), timed(True)
        tot[0] += a
        tot[1] += b
        print("| %d | %.0f | %.0f | %.2f %% |" % (r, a, b, (a / b - 1) * 100), flush=True)
    print("| mean | %.0f | %.0f | %.2f %% |" % (tot[0] / rounds, tot[1] / rounds, (tot[0] / tot[1] - 1) * 100))
    print("%d samples recorded" % m.samples)
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        cut = sys.argv.index("--") if "--" in sys.argv else len(sys.argv)
        pos = [int(v) for v in sys.argv[2:cut]] + [None] * 3
        return run(pos[0] or 400, pos[1] or 3, pos[2] or 64, sys.argv[cut + 1:])
    pos = sys.argv[2:] if len(sys.argv) > 1 else []
    print("| grid | points | slots | us per sample |")
    print("|---|---:|---:|---:|", flush=True)
    sample(int(pos[0]) if pos else 64, int(pos[1]) if len(pos) > 1 else 256, pos[2] if len(pos) > 2 else "f32")
    return 0


if __name__ == "__main__":
    sys.exit(main())
