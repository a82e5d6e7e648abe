#!/usr/bin/env python3
"""Running-DFT monitors against the plain blocked run at N^3 vacuum (GPU):
Mcells/s without a monitor, with the NTFF-surface monitor (24 thin slabs, one
launch a sample) and with an M^3 volume monitor at K = 1 and K = 4
wavelengths, all at the automatic sampling step; and the accumulation
kernel alone on the volume monitor: time per launch from HIP events, and the
bytes per second it achieves against the 1 + 4K accesses of the field's width
per cell that it must move (1 field read, 2K accumulator reads, 2K writes).

    python tools/dft_bench.py [N=512] [steps=200] [M=128] [dtype=f32]
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fdtd3d_amd.models.dft import DftMonitor, monitor_box_requests  # noqa: E402
from fdtd3d_amd.models.ntff import ntff_requests  # noqa: E402
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme  # noqa: E402
from fdtd3d_amd.ops import make_ops  # noqa: E402


def mk(cfg):
    s = YeeScheme(cfg, make_ops("hip", None, "cuda:0", torch.float32 if cfg.dtype == "f32" else torch.float64))
    s.init_scheme()
    s.init_grids()
    return s


def rate(s, steps):
    s.advance(2 * max(1, s.tb))  # warm-up
    torch.cuda.synchronize()
    t = time.perf_counter()
    s.advance(steps)
    torch.cuda.synchronize()
    return s.cells() * steps / (time.perf_counter() - t) / 1e6


def kernel_ms(s, mon, reps=20):
    tw = mon.twiddles(s, 1)
    s.ops.dft_accumulate(mon.entries, tw)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        s.ops.dft_accumulate(mon.entries, tw)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    m = int(sys.argv[3]) if len(sys.argv) > 3 else 128
    dt = sys.argv[4] if len(sys.argv) > 4 else "f32"
    width = 4 if dt == "f32" else 8
    cfg = SchemeConfig(scheme="3d", size=(n, n, n), dtype=dt, scene="vacuum", time_steps=steps, use_fused=True,
                       time_block=0)
    margin = (n - m) // 2
    cases = [("no monitor", None),
             ("NTFF-surface monitor (24 slabs, K = 1)", lambda s: DftMonitor(
                 s, ntff_requests(cfg.size, cfg.ntff_size), [s.wavelength])),
             ("%d^3 volume monitor, 6 components, K = 1" % m, lambda s: DftMonitor(
                 s, monitor_box_requests(s, (margin,) * 3), [s.wavelength])),
             ("%d^3 volume monitor, 6 components, K = 4" % m, lambda s: DftMonitor(
                 s, monitor_box_requests(s, (margin,) * 3), [s.wavelength * f for f in (1.0, 1.25, 1.5, 2.0)]))]
    print("| %d^3 vacuum %s | step | samples | Mcells/s | kernel ms / sample | kernel GB/s |" % (n, dt))
    print("|---|---:|---:|---:|---:|---:|")
    for name, make_mon in cases:
        s = mk(cfg)
        mon = make_mon(s) if make_mon else None
        r = rate(s, steps)
        if mon is None:
            print("| %s (T = %d) | -- | -- | %.0f | -- | -- |" % (name, s.tb, r))
        else:
            samples = mon.samples
            ms = kernel_ms(s, mon)
            cells = sum(e.owned()[0, 0].numel() for e in mon.entries)
            gbs = cells * (1 + 4 * len(mon.wavelengths)) * width / (ms * 1e-3) / 1e9
            print("| %s | %d | %d | %.0f | %.4f | %.0f |" % (name, mon.step, samples, r, ms, gbs))
        del s, mon
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
