#!/usr/bin/env python
"""The field-energy monitor on one GPU (models/energy.py, csrc/energy_kernels.hip).

    python tools/energy_bench.py sample [N=512] [dtype=f32]
        time of one whole-grid sample of an N^3 vacuum grid (HIP events over
        50 calls after a warm-up call) and the achieved GB/s against the bytes
        it must read (6 components)

    python tools/energy_bench.py run [steps=400] [rounds=3] -- <driver options>
        steady-state Mcells/s of the run the driver options describe, with and
        without the monitor at its automatic step, alternated in ONE process
        on ONE scheme (box-to-box spread is ~10 %: never compare sessions);
        a warm-up of `steps` steps first, the discipline of bench.py

Results: profiles/energy.md.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fdtd3d_amd.models.energy import EnergyMonitor  # noqa: E402
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme  # noqa: E402
from fdtd3d_amd.ops import make_ops  # noqa: E402


def sample(n, dt):
    dtype = torch.float32 if dt == "f32" else torch.float64
    cfg = SchemeConfig(scheme="3d", size=(n, n, n), scene="vacuum", dtype=dt, use_fused=True, time_block=0)
    s = YeeScheme(cfg, make_ops("hip", None, "cuda:0", dtype))
    s.init_scheme()
    s.init_grids()
    s.randomize_fields()
    m = EnergyMonitor(s, (0, 0, 0), register=False)
    ops = s.ops
    ops.field_sumsq(m.entries)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    reps = 50
    a.record()
    for _ in range(reps):
        out = ops.field_sumsq(m.entries)
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) / reps * 1e3
    nbytes = sum(e.field[tuple(slice(e.box[0][d], e.box[1][d]) for d in range(3))].numel()
                 for e in m.entries) * s.F[0]["Ez"].element_size()
    ref = sum(float(s.F[0][c].double().square().sum()) for c in s.comps) if n <= 512 else float("nan")
    _, _, nblocks, rows_blk, _ = next(iter(m.entries.tables.values()))
    print("| %d^3 %s | %.1f | %.1f | %.0f | %d | %d | %.3g |" % (
        n, dt, us, nbytes / n ** 3, nbytes / us / 1e3, nblocks, rows_blk,
        abs(float(out.sum()) - ref) / ref if ref == ref else float("nan")), flush=True)


def run(steps, rounds, argv):
    from fdtd3d_amd.runner import build
    from fdtd3d_amd.utils.settings import setup_from_cmd
    status, settings = setup_from_cmd(argv)
    if status:
        return status
    s, _, _ = build(settings)
    s.init_scheme()
    s.init_grids()
    m = EnergyMonitor(s, (0, 0, 0), register=False)
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
    print("monitor step %d, %d steps per measurement" % (m.step, steps))
    print("| round | without Mcells/s | with Mcells/s | cost |")
    print("|---:|---:|---:|---:|", flush=True)
    tot = [0.0, 0.0]
    for r in range(rounds):
        a, b = timed(False), timed(True)
        tot[0] += a
        tot[1] += b
        print("| %d | %.0f | %.0f | %.2f %% |" % (r, a, b, (a / b - 1) * 100), flush=True)
    print("| mean | %.0f | %.0f | %.2f %% |" % (tot[0] / rounds, tot[1] / rounds, (tot[0] / tot[1] - 1) * 100))
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        cut = sys.argv.index("--") if "--" in sys.argv else len(sys.argv)
        pos = sys.argv[2:cut]
        return run(int(pos[0]) if pos else 400, int(pos[1]) if len(pos) > 1 else 3, sys.argv[cut + 1:])
    pos = sys.argv[2:] if len(sys.argv) > 1 else []
    print("| grid | us per sample | B/cell read | GB/s | blocks | rows per block | rel. difference to torch |")
    print("|---|---:|---:|---:|---:|---:|---:|", flush=True)
    sample(int(pos[0]) if pos else 512, pos[1] if len(pos) > 1 else "f32")
    return 0


if __name__ == "__main__":
    sys.exit(main())
