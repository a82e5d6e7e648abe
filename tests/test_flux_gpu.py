"""Poynting-flux monitors on the GPU: the face-sum kernels
(csrc/flux_kernels.hip) against the torch op on the same random accumulators,
and a monitor end to end on hybrid passes against the fp64 CPU oracle
(models/flux.py)."""
import dataclasses

import pytest
import torch

from fdtd3d_amd.models.flux import flux_from_config
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.dft import FluxOperand, FluxTerm, FluxTerms

pytestmark = pytest.mark.gpu

# accumulator blocks (x, y, z'): ragged rows (37 padded to 40), whole groups (8), one group (4), and thin slabs
BLOCKS = {"a40": (9, 7, 40), "b8": (6, 21, 8), "c4": (20, 18, 4), "d8": (20, 18, 8), "e2": (2, 12, 40), "f5": (5, 6, 5)}
# (face, sign, extent, E block, E first, E avg, H block, H first, H avg)
TERMS = [
    # x-normal faces, lanes along z: ragged z extents, 7 * 35 = 245 cells and 6 * 39 = 234 cells
    (0, 1, (1, 7, 35), "a40", (3, 0, 1), (0, 0, 0), "a40", (2, 0, 2), (1, 0, 1)),
    (0, -1, (1, 6, 39), "a40", (8, 0, 0), (0, 1, 1), "a40", (0, 1, 1), (1, 0, 0)),
    # y-normal, more than 256 cells (9 * 37 = 333: two blocks, the second partial), the whole ragged row
    (1, 1, (9, 1, 37), "a40", (0, 3, 0), (0, 0, 0), "a40", (0, 5, 3), (0, 1, 0)),
    (1, -1, (8, 1, 36), "a40", (0, 0, 1), (1, 1, 1), "a40", (1, 6, 4), (0, 0, 0)),
    # aligned z extents (nz' = 8), 20 * 8 = 160 cells and fewer than 64 cells (5 * 7 = 35)
    (2, 1, (1, 20, 8), "b8", (5, 0, 0), (0, 1, 0), "b8", (0, 1, 0), (1, 0, 0)),
    (2, -1, (5, 1, 7), "b8", (0, 20, 0), (1, 0, 1), "b8", (1, 3, 1), (0, 0, 0)),
    # z-normal faces, lanes along y: the samples in the middle of a 16-byte group (z' 1, 2), at its end (3),
    # across two groups (3, 4), at the start (0, 1); 19 * 17 = 323 cells, 3 cells, 20 * 18 = 360 cells
    (3, 1, (19, 17, 1), "c4", (0, 1, 1), (1, 0, 1), "c4", (1, 0, 3), (0, 1, 0)),
    (3, -1, (19, 17, 1), "d8", (1, 0, 3), (0, 1, 1), "c4", (0, 0, 0), (1, 1, 1)),
    (4, 1, (1, 3, 1), "d8", (7, 7, 7), (0, 0, 0), "d8", (0, 0, 6), (1, 1, 1)),
    (4, -1, (20, 18, 1), "d8", (0, 0, 5), (0, 0, 1), "c4", (0, 0, 2), (0, 0, 0)),
    # an empty entry, a z-normal face on rows that are no whole groups, a two-plane slab
    (5, 1, (0, 6, 1), "f5", (0, 0, 0), (0, 0, 0), "f5", (0, 0, 0), (0, 0, 0)),
    (5, 1, (4, 5, 1), "f5", (0, 1, 3), (1, 0, 1), "f5", (1, 0, 4), (0, 1, 0)),
    (5, -1, (1, 11, 33), "e2", (0, 0, 5), (1, 1, 0), "e2", (1, 1, 7), (0, 0, 0)),
]


def _terms(blocks, K, rows):
    t = FluxTerms(K, 6)
    for face, sign, ext, eb, e0, ea, hb, h0, ha in rows:
        t.add(FluxTerm(face, sign, ext, FluxOperand(blocks[eb], e0, ea), FluxOperand(blocks[hb], h0, ha)))
    return t


def _abs_sums(blocks, K, rows):
    """(6, K) sums of the absolute values of every fp64 product, the scale of
    the summation error."""
    out = torch.zeros((6, K), dtype=torch.float64)

    def centre(b, first, avg, ext):
        acc, cnt = 0, 0
        for ox in range(1 + avg[0]):
            for oy in range(1 + avg[1]):
                for oz in range(1 + avg[2]):
                    o = (ox, oy, oz)
                    acc = acc + blocks[b][(slice(None), slice(None)) + tuple(
                        slice(first[a] + o[a], first[a] + o[a] + ext[a]) for a in range(3))].double()
                    cnt += 1
        return acc / cnt

    for face, sign, ext, eb, e0, ea, hb, h0, ha in rows:
        e, h = centre(eb, e0, ea, ext), centre(hb, h0, ha, ext)
        out[face] += ((e[:, 0] * h[:, 0]).abs() + (e[:, 1] * h[:, 1]).abs()).sum(dim=(1, 2, 3))
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("K", [1, 8])
def test_flux_kernel_vs_torch(gpu, dtype, K):
    """Both sides sum the same fp64 products and differ only in their order:
    n eps for n <= 1e4 terms, with a margin of 10 -- 1e-11 of the sum of
    the absolute terms per (face, k)."""
    hip = make_ops("hip", None, gpu, dtype)
    ref = make_ops("torch", None, "cpu", dtype)
    g = torch.Generator().manual_seed(11)
    cpu = {n: torch.rand((K, 2) + s, generator=g, dtype=dtype) * 2 - 1 for n, s in BLOCKS.items()}
    dev = {n: v.to(gpu) for n, v in cpu.items()}
    want = ref.dft_flux(_terms(cpu, K, TERMS))
    scale = _abs_sums(cpu, K, TERMS)
    assert want.shape == (6, K) and want.dtype == torch.float64 and float(scale.min()) > 0
    th = _terms(dev, K, TERMS)
    before = hip.launches
    got = hip.dft_flux(th)
    per_call = hip.launches - before
    again = hip.dft_flux(th)
    torch.cuda.synchronize()
    assert got.shape == (6, K) and got.dtype == torch.float64 and got.device.type == "cuda"
    err = (got.cpu() - want).abs() / scale
    print("largest difference %.3g of the sum of absolute terms (bound 1e-11)" % float(err.max()))
    assert float(err.max()) <= 1e-11, err
    assert torch.equal(got, again)  # no atomics: the same bits
    assert hip.launches == before + 2 * per_call and th.table is not None
    # the launches of a call do not depend on the number of faces or terms
    one = _terms(dev, K, TERMS[:1])
    before = hip.launches
    p = hip.dft_flux(one)
    assert hip.launches - before == per_call == 2
    torch.cuda.synchronize()
    assert float((p[1:].abs()).max()) == 0.0 and float(p[0].abs().min()) > 0


def test_flux_host_validation(gpu):
    from fdtd3d_amd.ops.hip_ops import HipError
    hip = make_ops("hip", None, gpu, torch.float32)
    acc = torch.zeros((2, 2, 5, 6, 8), dtype=torch.float32, device=gpu)
    ok = FluxOperand(acc, (0, 0, 0), (0, 0, 0))
    before = hip.launches
    for first, avg, ext in (((0, 0, 0), (0, 0, 1), (1, 6, 8)),     # z + 1 past the row
                            ((0, 1, 0), (0, 0, 0), (5, 6, 1)),     # y past the block
                            ((4, 0, 0), (1, 0, 0), (1, 6, 8)),     # x + 1 past the block
                            ((0, 0, -1), (0, 0, 0), (5, 6, 1))):
        t = FluxTerms(2, 1)
        t.add(FluxTerm(0, 1, ext, ok, FluxOperand(acc, first, avg)))
        with pytest.raises(HipError):
            hip.dft_flux(t)
    t = FluxTerms(1, 1)  # K of the terms and of the accumulators differ
    t.add(FluxTerm(0, 1, (5, 6, 1), ok, ok))
    with pytest.raises(HipError):
        hip.dft_flux(t)
    t = FluxTerms(2, 1)
    t.add(FluxTerm(0, 1, (5, 6, 1), ok, FluxOperand(acc.double(), (0, 0, 0), (0, 0, 0))))  # not the backend's dtype
    with pytest.raises(HipError):
        hip.dft_flux(t)
    assert hip.launches == before


def _scheme(cfg, backend, device):
    dt = torch.float32 if cfg.dtype == "f32" else torch.float64
    s = YeeScheme(cfg, make_ops(backend, None, device, dt))
    s.init_scheme()
    s.init_grids()
    return s


# The grid of the issue: 48 x 40 x 56, CPML 5, TF/SF 9, sphere r = 6, flux margin 7, --hybrid-block 4.  On it the
# hybrid planner finds no core (the cells 4 + 1 clear of the TF/SF faces and the CPML are 4 % of the grid, under the
# planner's 25 % rule), so the run takes single steps; HYBRID is the same scene on the smallest grid of whole 8-cell
# steps whose core passes that rule at either core margin (58 x 50 x 66 of 88 x 80 x 96 cells), where the passes
# are hybrid ones at T = 4.
SMALL = SchemeConfig(scheme="3d", size=(48, 40, 56), time_steps=160, pml_size=(5, 5, 5), tfsf_size=(9, 9, 9),
                     scene="sphere", sphere_center=(24.0, 20.0, 28.0), sphere_radius=6.0, use_pml=True,
                     pml_type="cpml", use_tfsf=True, hybrid_block=4, use_flux=True, flux_size=(7, 7, 7), dft_step=0)
HYBRID = dataclasses.replace(SMALL, size=(88, 80, 96), sphere_center=(44.0, 40.0, 48.0))
_oracle_cache = {}


def _oracle(name, cfg, step):
    """The fp64 CPU run with the SAME sampling step, stepped one step at a
    time; computed once and shared."""
    if (name, step) not in _oracle_cache:
        ref = _scheme(dataclasses.replace(cfg, dtype="f64", hybrid_block=1, dft_step=step), "torch", "cpu")
        mon = flux_from_config(ref)
        ref.perform_steps()
        assert ref.hybrid is None
        _oracle_cache[(name, step)] = (mon.samples, mon.power())
    return _oracle_cache[(name, step)]


# fp32: 20 times the measured fp32 phasor error of profiles/dft.md (7.1e-7 of scale) -- the flux is a product of two
# such phasors summed with cancellation (measured values: profiles/flux.md)
@pytest.mark.parametrize("dtype,tol", [("f32", 20 * 7.1e-7), ("f64", 1e-10)])
@pytest.mark.parametrize("name", ["small", "hybrid"])
def test_flux_end_to_end(gpu, name, dtype, tol):
    """CPML + TF/SF around a dielectric sphere with the automatic sampling
    step, --hybrid-block 4: per-face and net power against the fp64 CPU
    oracle of the same run, relative to the largest face power."""
    cfg = dataclasses.replace(SMALL if name == "small" else HYBRID, dtype=dtype)
    s = _scheme(cfg, "hip", gpu)
    if name == "hybrid":
        assert s.hybrid is not None and s.hybrid["T"] == 4, "hybrid plan rejected"
    mon = flux_from_config(s)
    assert mon.label == "scattered" and (s.hybrid is None or mon.step % 4 == 0)
    s.perform_steps()
    torch.cuda.synchronize()
    got = mon.power()
    samples, want = _oracle(name, cfg, mon.step)
    assert mon.samples == samples > 0
    peak = float(want.abs().max())
    assert peak > 0
    face = float((got - want).abs().max()) / peak
    net = abs(float(got.sum() - want.sum())) / peak
    print("%s %s: per-face difference %.3g, net difference %.3g of the largest face power (bound %.3g)"
          % (name, dtype, face, net, tol))
    assert face <= tol and net <= tol
