#!/usr/bin/env python3
"""The Poynting-flux face sums of an N^3 grid's surface (GPU): ``ops.dft_flux``
of the HIP backend (csrc/flux_kernels.hip, two launches) against the same
evaluation with torch ops on the device (``TorchOps.dft_flux``: slicing,
fp64 conversion, averaging and reduction, a few dozen launches per term), at
K = 1 and K = 8 wavelengths, on random accumulators in the layout of a
``FluxMonitor`` with the given margin.  Time per evaluation from HIP events.
Every K runs in a child process of its own, under its own time limit; a
failed case ends the run.

    python tools/flux_bench.py [N=512] [margin=16] [dtype=f32] [limit_s=240]
"""
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fdtd3d_amd.models.ntff import _faces, _plan_box, _sample_plan  # noqa: E402
from fdtd3d_amd.ops import make_ops  # noqa: E402
from fdtd3d_amd.ops.dft import FluxOperand, FluxTerm, FluxTerms, acc_shape, vec_width, z_pad  # noqa: E402


def surface_terms(n, margin, K, dtype, device):
    """The 12 products of a FluxMonitor on the n^3 grid (models/flux.py
    ``_build_terms``), on random accumulators."""
    g = torch.Generator().manual_seed(5)
    v = vec_width(dtype)
    terms = FluxTerms(K, 6)
    cells = 0

    def operand(comp, axis, x0, lo, hi):
        plan = _sample_plan(comp, axis, x0, lo, hi)
        box = _plan_box(plan)
        acc = (torch.rand(acc_shape(box, K, v), generator=g, dtype=dtype) * 2 - 1).to(device)
        return FluxOperand(acc, (0, 0, box[0][2] - z_pad(box, v)[0]), [len(o) == 2 for _, _, o in plan]), plan

    for f, (axis, x0, sign, lo, hi) in enumerate(_faces((n, n, n), (margin,) * 3)):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        for ea, ha, s in ((b, c, 1), (c, b, -1)):
            oe, pe = operand("E" + "xyz"[ea], axis, x0, lo, hi)
            oh, _ = operand("H" + "xyz"[ha], axis, x0, lo, hi)
            t = terms.add(FluxTerm(f, int(sign) * s, [m for _, m, _ in pe], oe, oh))
            cells += t.extent[0] * t.extent[1] * t.extent[2]
    return terms, cells


def ms_per_call(fn, reps):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def case(n, margin, dt, K):
    dtype = torch.float32 if dt == "f32" else torch.float64
    hip = make_ops("hip", None, "cuda:0", dtype)
    ref = make_ops("torch", None, "cuda:0", dtype)
    terms, cells = surface_terms(n, margin, K, dtype, "cuda:0")
    t_hip, p = ms_per_call(lambda: hip.dft_flux(terms), 50)
    t_ref, q = ms_per_call(lambda: ref.dft_flux(terms), 5)
    err = float(((p - q).abs() / q.abs().clamp_min(1e-300)).max())
    print("| %d | %d | %.4f | %.3f | %.1f | %.2g |" % (K, cells, t_hip, t_ref, t_ref / t_hip, err), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        case(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
        return 0
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    margin = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    dt = sys.argv[3] if len(sys.argv) > 3 else "f32"
    limit = float(sys.argv[4]) if len(sys.argv) > 4 else 240.0
    print("| K (%d^3 %s, margin %d) | face cells x terms | HIP ms | torch ops ms | ratio | largest rel. difference |"
          % (n, dt, margin))
    print("|---:|---:|---:|---:|---:|---:|", flush=True)
    for K in (1, 8):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(n), str(margin), dt, str(K)],
                               timeout=limit)
        except subprocess.TimeoutExpired:
            print("K = %d: no result within %.0f s" % (K, limit))
            return 124
        if r.returncode != 0:
            print("K = %d: exit status %d" % (K, r.returncode))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
