"""Time ``ops.dft_farfield`` (csrc/farfield_kernels.hip) at the size of a cubic
run against the device-side torch formulation of the same transform
(models/ntff.py ``ntff_power`` looped over wavelengths and polar angles) on
the same synthetic phasors.  The numbers of profiles/farfield.md:

    python tools/farfield_bench.py --size 512 --margin 15 --k 4

prints one JSON line per direction set (the 91 x 180 sphere and a single
181-direction cut).  No field arrays are allocated: only the accumulators of
the 24 NTFF slabs, filled with random values.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fdtd3d_amd.models.farfield import directions  # noqa: E402
from fdtd3d_amd.models.ntff import ETA0, _faces, _plan_box, _sample_plan, ntff_power  # noqa: E402
from fdtd3d_amd.ops import make_ops  # noqa: E402
from fdtd3d_amd.ops.dft import FarTerm, FarTerms, FluxOperand, acc_shape, vec_width, z_pad  # noqa: E402


def build(size, margin, K, dx, dtype, device):
    """(FarTerms, {(comp, box): (K,) complex phasors}) of random accumulators
    over the NTFF slabs, as models/farfield.py builds them."""
    g = torch.Generator().manual_seed(3)
    v = vec_width(dtype)
    terms, accs = FarTerms(K, dx), {}
    for axis, x0, s, lo, hi in _faces(size, margin):
        a1, a2 = [a for a in range(3) if a != axis]
        sc = int(s) * (1 if (a1 - axis) % 3 == 1 else -1)
        pos0 = [((x0 if a == axis else lo[a] + 0.5) - size[a] / 2.0) * dx for a in range(3)]
        for slot, sign, comp in ((a2, sc, "H" + "xyz"[a1]), (a1, -sc, "H" + "xyz"[a2]),
                                 (3 + a2, -sc, "E" + "xyz"[a1]), (3 + a1, sc, "E" + "xyz"[a2])):
            plan = _sample_plan(comp, axis, x0, lo, hi)
            box = _plan_box(plan)
            if (comp, box) not in accs:
                acc = torch.zeros(acc_shape(box, K, v), dtype=dtype)
                z0 = z_pad(box, v)[0]
                own = acc[..., box[0][2] - z0:box[1][2] - z0]
                own.copy_(torch.rand(own.shape, generator=g, dtype=dtype) * 2 - 1)
                accs[(comp, box)] = (acc.to(device), box[0][2] - z0, box[1][2] - z0)
            acc, z_lo, _ = accs[(comp, box)]
            terms.add(FarTerm(slot, sign, [n for _, n, _ in plan], FluxOperand(acc, (0, 0, z_lo), [len(o) == 2
                                                                                                  for _, _, o in plan]), pos0))
    phasors = {key: torch.complex(acc[:, 0, ..., a:b].double(), acc[:, 1, ..., a:b].double())
               for key, (acc, a, b) in accs.items()}
    return terms, phasors


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--margin", type=int, default=15)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true", help="time the kernel only")
    a = ap.parse_args()
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    dev = torch.device("cuda")
    size, margin, dx = (a.size,) * 3, (a.margin,) * 3, 5e-4
    wl = [0.02 * (1 + 0.25 * k) for k in range(a.k)]
    wn = torch.tensor([2 * math.pi / w for w in wl], dtype=torch.float64)
    hip = make_ops("hip", None, dev, dtype)
    terms, phasors = build(size, margin, a.k, dx, dtype, dev)
    sets = {"sphere 91 x 180": (torch.linspace(0, math.pi, 91, dtype=torch.float64),
                                torch.arange(180, dtype=torch.float64) * (2 * math.pi / 180)),
            "cut 1 x 181": (torch.tensor([math.pi / 2], dtype=torch.float64),
                            torch.linspace(0, 2 * math.pi, 181, dtype=torch.float64))}
    for name, (th, ph) in sets.items():
        dirs = directions(th, ph)
        t_kernel, raw = timed(lambda: hip.dft_farfield(terms, dirs, wn), a.repeat)
        rec = {"set": name, "size": a.size, "margin": a.margin, "K": a.k, "dtype": a.dtype,
               "directions": int(dirs.shape[0]), "kernel_ms": 1e3 * t_kernel}
        if not a.skip_torch:
            def torch_side():
                return torch.stack([torch.stack([ntff_power(
                    {key: p[k].real for key, p in phasors.items()}, {key: p[k].imag for key, p in phasors.items()},
                    size, margin, dx, wl[k], float(t), ph, boxes=True) for t in th]) for k in range(a.k)])

            t_torch, want = timed(torch_side, 1)
            # the same quantity from the kernel's vectors (U * 4 pi eta0 = ntff_power, models/farfield.py)
            v = (torch.view_as_complex(raw) * dx * dx).reshape(a.k, th.numel(), ph.numel(), 6)
            st, ct = torch.sin(th).reshape(1, -1, 1).to(dev), torch.cos(th).reshape(1, -1, 1).to(dev)
            sp, cp = torch.sin(ph).reshape(1, 1, -1).to(dev), torch.cos(ph).reshape(1, 1, -1).to(dev)
            sph = lambda x, y, z: (x * ct * cp + y * ct * sp - z * st, -x * sp + y * cp)  # noqa: E731
            n_th, n_ph = sph(v[..., 0], v[..., 1], v[..., 2])
            l_th, l_ph = sph(v[..., 3], v[..., 4], v[..., 5])
            got = wn.to(dev).reshape(-1, 1, 1) ** 2 / (8 * math.pi) * ((l_ph + ETA0 * n_th).abs() ** 2
                                                                      + (l_th - ETA0 * n_ph).abs() ** 2)
            rec.update(torch_ms=1e3 * t_torch, max_rel_difference=float((got - want).abs().max() / want.max()))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
