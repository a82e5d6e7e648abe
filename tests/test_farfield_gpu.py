"""Far-field monitors on the GPU: the radiation-vector kernels
(csrc/farfield_kernels.hip) against the torch op on the same random
accumulators, the host validation, and a monitor end to end on stepped and
hybrid passes against the fp64 CPU oracle (models/farfield.py)."""
import dataclasses
import math

import pytest
import torch

from fdtd3d_amd.models.farfield import farfield_from_config
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.dft import FarTerm, FarTerms, FluxOperand

pytestmark = pytest.mark.gpu

# accumulator blocks and operand placements of tests/test_flux_gpu.py (BLOCKS / TERMS): ragged rows (37 padded to
# 40), whole groups (8), one group (4), thin slabs
BLOCKS = {"a40": (9, 7, 40), "b8": (6, 21, 8), "c4": (20, 18, 4), "d8": (20, 18, 8), "e2": (2, 12, 40), "f5": (5, 6, 5)}
# (extent, [(block, first, avg), ...]): every operand of a flux term is a current here
FACES = [
    # x-normal faces, rows along z: ragged z extents, 7 * 35 = 245 cells and 6 * 39 = 234 cells
    ((1, 7, 35), [("a40", (3, 0, 1), (0, 0, 0)), ("a40", (2, 0, 2), (1, 0, 1))]),
    ((1, 6, 39), [("a40", (8, 0, 0), (0, 1, 1)), ("a40", (0, 1, 1), (1, 0, 0))]),
    # y-normal, more than 256 cells (9 * 37 = 333: two chunks), the whole ragged row
    ((9, 1, 37), [("a40", (0, 3, 0), (0, 0, 0)), ("a40", (0, 5, 3), (0, 1, 0))]),
    ((8, 1, 36), [("a40", (0, 0, 1), (1, 1, 1)), ("a40", (1, 6, 4), (0, 0, 0))]),
    # aligned z extents (nz' = 8), 20 * 8 = 160 cells and fewer than 64 cells (5 * 7 = 35)
    ((1, 20, 8), [("b8", (5, 0, 0), (0, 1, 0)), ("b8", (0, 1, 0), (1, 0, 0))]),
    ((5, 1, 7), [("b8", (0, 20, 0), (1, 0, 1)), ("b8", (1, 3, 1), (0, 0, 0))]),
    # z-normal faces, rows along y: the samples in the middle of a 16-byte group (z' 1, 2), at its end (3), across
    # two groups (3, 4), at the start (0, 1); 19 * 17 = 323 cells -- a GROUP OF FOUR --, 3 cells (a LONE term),
    # 20 * 18 = 360 cells
    ((19, 17, 1), [("c4", (0, 1, 1), (1, 0, 1)), ("c4", (1, 0, 3), (0, 1, 0)), ("d8", (1, 0, 3), (0, 1, 1)),
                   ("c4", (0, 0, 0), (1, 1, 1))]),
    ((1, 3, 1), [("d8", (7, 7, 7), (0, 0, 0))]),
    ((20, 18, 1), [("d8", (0, 0, 5), (0, 0, 1)), ("c4", (0, 0, 2), (0, 0, 0)), ("d8", (0, 0, 6), (0, 0, 1))]),
    # an empty term, a z-normal face on rows that are no whole groups, a two-plane slab
    ((0, 6, 1), [("f5", (0, 0, 0), (0, 0, 0))]),
    ((4, 5, 1), [("f5", (0, 1, 3), (1, 0, 1)), ("f5", (1, 0, 4), (0, 1, 0))]),
    ((1, 11, 33), [("e2", (0, 0, 5), (1, 1, 0)), ("e2", (1, 1, 7), (0, 0, 0))]),
]
DX = 5e-4
# |kappa r'| <= 64: |r'| <= |pos0| + 40 dx sqrt(3) < 0.05 m and kappa <= 2 pi / 0.02
WAVELENGTHS = [0.02, 0.023, 0.027, 0.031, 0.036, 0.041, 0.047, 0.05]


def _rows():
    """(slot, sign, extent, block, first, avg, pos0) of every term: the first
    current of every face, then the second, ... -- the members of a group are
    not adjacent and the faces not in order; 25 terms on 6 slots put several
    on each."""
    rows = []
    for c in range(4):
        for f in reversed(range(len(FACES))) if c % 2 else range(len(FACES)):
            ext, ops = FACES[f]
            if c < len(ops):
                pos0 = (DX * (f - 6), -DX * 2.5 * f, DX * (7.5 - f))
                rows.append(((f + 2 * c) % 6, 1 if (f + c) % 3 else -1, ext) + ops[c] + (pos0,))
    return rows


def _terms(blocks, K, rows):
    t = FarTerms(K, DX)
    for slot, sign, ext, b, first, avg, pos0 in rows:
        t.add(FarTerm(slot, sign, ext, FluxOperand(blocks[b], first, avg), pos0))
    return t


def _abs_sums(blocks, K, rows):
    """(K, 6) sums of the absolute values of every averaged fp64 sample (the
    phase factors have modulus 1): the scale of the summation error."""
    out = torch.zeros((K, 6), dtype=torch.float64)
    for slot, sign, ext, b, first, avg, pos0 in rows:
        acc, cnt = 0, 0
        for ox in range(1 + avg[0]):
            for oy in range(1 + avg[1]):
                for oz in range(1 + avg[2]):
                    o = (ox, oy, oz)
                    acc = acc + blocks[b][(slice(None), slice(None)) + tuple(
                        slice(first[a] + o[a], first[a] + o[a] + ext[a]) for a in range(3))].double()
                    cnt += 1
        acc = acc / cnt
        out[:, slot] += torch.complex(acc[:, 0], acc[:, 1]).abs().sum(dim=(1, 2, 3))
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("K", [1, 8])
def test_farfield_kernel_vs_torch(gpu, dtype, K):
    """Both sides sum the same fp64 products; they differ in the summation
    order (n eps, n <= 1e4), the rounding of the argument (|arg| eps, |arg|
    <= 64) and the phase recurrence (<= 256 eps): about 1.2e-12 of the sum of
    the absolute terms per (k, direction, slot), with the flux test's margin
    of 10 -- 1e-11."""
    hip = make_ops("hip", None, gpu, dtype)
    ref = make_ops("torch", None, "cpu", dtype)
    g = torch.Generator().manual_seed(11)
    cpu = {n: torch.rand((K, 2) + s, generator=g, dtype=dtype) * 2 - 1 for n, s in BLOCKS.items()}
    dev = {n: v.to(gpu) for n, v in cpu.items()}
    rows = _rows()
    assert len(rows) == 25 and sorted({r[0] for r in rows}) == list(range(6))
    wn = torch.tensor([2 * math.pi / w for w in WAVELENGTHS[:K]], dtype=torch.float64)
    scale = _abs_sums(cpu, K, rows)
    assert float(scale.min()) > 0
    th = _terms(dev, K, rows)
    per_call = None
    for A in (1, 63, 257):
        dirs = torch.nn.functional.normalize(torch.rand((A, 3), generator=g, dtype=torch.float64) * 2 - 1, dim=1)
        reach = max(float((dirs @ torch.tensor([p + DX * (e - 1) * s for p, e in zip(r[6], r[2])],
                                                   dtype=torch.float64)).abs().max())
                    for r in rows for s in (0, 1))
        assert float(wn.max()) * reach <= 64
        want = ref.dft_farfield(_terms(cpu, K, rows), dirs, wn)
        before = hip.launches
        got = hip.dft_farfield(th, dirs, wn)
        per_call = hip.launches - before
        table = th.table
        again = hip.dft_farfield(th, dirs, wn)
        torch.cuda.synchronize()
        assert got.shape == (K, A, 6, 2) and got.dtype == torch.float64 and got.device.type == "cuda"
        err = (got.cpu() - want).abs().amax(dim=3) / scale.reshape(K, 1, 6)
        print("A=%d: largest difference %.3g of the sum of absolute terms (bound 1e-11)" % (A, float(err.max())))
        assert float(err.max()) <= 1e-11, err
        assert torch.equal(got, again)  # no atomics: the same bits
        assert per_call == 2 and hip.launches == before + 2 * per_call
        assert table is not None and th.table is table  # cached
    # the launches of a call do not depend on the number of faces or terms; the other slots stay zero
    one = _terms(dev, K, rows[:1])
    dirs = torch.nn.functional.normalize(torch.rand((63, 3), generator=g, dtype=torch.float64) * 2 - 1, dim=1)
    before = hip.launches
    p = hip.dft_farfield(one, dirs, wn)
    assert hip.launches - before == per_call == 2
    torch.cuda.synchronize()
    slot = rows[0][0]
    rest = [s for s in range(6) if s != slot]
    assert float(p[:, :, rest].abs().max()) == 0.0 and float(p[:, :, slot].abs().amax(dim=2).min()) > 0
    # an ungrouped evaluation (every term alone) gives the same sums
    single = torch.zeros_like(p)
    full = hip.dft_farfield(th, dirs, wn)
    for r in rows:
        single += hip.dft_farfield(_terms(dev, K, [r]), dirs, wn)
    torch.cuda.synchronize()
    err = (single - full).abs().amax(dim=3).cpu() / scale.reshape(K, 1, 6)
    assert float(err.max()) <= 1e-11


def test_farfield_host_validation(gpu):
    from fdtd3d_amd.ops.hip_ops import HipError
    hip = make_ops("hip", None, gpu, torch.float32)
    acc = torch.zeros((2, 2, 5, 6, 8), dtype=torch.float32, device=gpu)
    dirs = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], dtype=torch.float64)
    wn = torch.tensor([300.0, 200.0], dtype=torch.float64)
    before = hip.launches

    def terms(k, ext, op):
        t = FarTerms(k, DX)
        t.add(FarTerm(0, 1, ext, op, (0.0, 0.0, 0.0)))
        return t

    for first, avg, ext in (((0, 0, 0), (0, 0, 1), (1, 6, 8)),     # z + 1 past the row
                            ((0, 1, 0), (0, 0, 0), (5, 6, 1)),     # y past the block
                            ((4, 0, 0), (1, 0, 0), (1, 6, 8)),     # x + 1 past the block
                            ((0, 0, -1), (0, 0, 0), (5, 6, 1))):
        with pytest.raises(HipError):
            hip.dft_farfield(terms(2, ext, FluxOperand(acc, first, avg)), dirs, wn)
    ok = FluxOperand(acc, (0, 0, 0), (0, 0, 0))
    with pytest.raises(HipError):  # K of the terms and of the accumulators differ
        hip.dft_farfield(terms(1, (5, 6, 1), ok), dirs, wn[:1])
    with pytest.raises(HipError):  # K of the terms and of the wavenumbers differ
        hip.dft_farfield(terms(2, (5, 6, 1), ok), dirs, wn[:1])
    with pytest.raises(HipError):  # more than DFT_MAX_K wavelengths
        hip.dft_farfield(terms(9, (5, 6, 1), FluxOperand(torch.zeros((9, 2, 5, 6, 8), dtype=torch.float32, device=gpu),
                                                         (0, 0, 0), (0, 0, 0))), dirs, torch.ones(9, dtype=torch.float64))
    with pytest.raises(HipError):  # not the backend's dtype
        hip.dft_farfield(terms(2, (5, 6, 1), FluxOperand(acc.double(), (0, 0, 0), (0, 0, 0))), dirs, wn)
    with pytest.raises(HipError):  # not on the device
        hip.dft_farfield(terms(2, (5, 6, 1), FluxOperand(acc.cpu(), (0, 0, 0), (0, 0, 0))), dirs, wn)
    for bad in (dirs.float(), dirs[:, :2], dirs.reshape(-1)):
        with pytest.raises(HipError):
            hip.dft_farfield(terms(2, (5, 6, 1), ok), bad, wn)
    assert hip.launches == before
    good = hip.dft_farfield(terms(2, (5, 6, 1), ok), dirs, wn)
    torch.cuda.synchronize()
    assert hip.launches == before + 2 and float(good.abs().max()) == 0.0


def _scheme(cfg, backend, device):
    dt = torch.float32 if cfg.dtype == "f32" else torch.float64
    s = YeeScheme(cfg, make_ops(backend, None, device, dt))
    s.init_scheme()
    s.init_grids()
    return s


# The scenes of tests/test_flux_gpu.py: SMALL takes single steps (the hybrid planner finds no core on it), HYBRID is
# the same scene on the smallest grid whose passes are hybrid ones at T = 4.
SMALL = SchemeConfig(scheme="3d", size=(48, 40, 56), time_steps=160, pml_size=(5, 5, 5), tfsf_size=(9, 9, 9),
                     scene="sphere", sphere_center=(24.0, 20.0, 28.0), sphere_radius=6.0, use_pml=True,
                     pml_type="cpml", use_tfsf=True, hybrid_block=4, use_farfield=True, farfield_size=(7, 7, 7),
                     dft_step=0)
HYBRID = dataclasses.replace(SMALL, size=(88, 80, 96), sphere_center=(44.0, 40.0, 48.0))
THETAS = torch.linspace(0.0, math.pi, 7, dtype=torch.float64)
PHIS = torch.arange(12, dtype=torch.float64) * (2 * math.pi / 12)
_oracle_cache = {}


def _oracle(name, cfg, step):
    """The fp64 CPU run with the SAME sampling step, stepped one step at a
    time; computed once and shared."""
    if (name, step) not in _oracle_cache:
        ref = _scheme(dataclasses.replace(cfg, dtype="f64", hybrid_block=1, dft_step=step), "torch", "cpu")
        mon = farfield_from_config(ref)
        ref.perform_steps()
        assert ref.hybrid is None
        _oracle_cache[(name, step)] = (mon.samples, mon.intensity(THETAS, PHIS), mon.total_power())
    return _oracle_cache[(name, step)]


# fp32: 20 times the measured fp32 phasor error of profiles/dft.md (7.1e-7 of scale), the bound of
# tests/test_flux_gpu.py for its reason -- U is quadratic in the phasors (measured values: profiles/farfield.md)
@pytest.mark.parametrize("name,dtype,tol", [("small", "f32", 20 * 7.1e-7), ("small", "f64", 1e-10),
                                            ("hybrid", "f32", 20 * 7.1e-7)])
def test_farfield_end_to_end(gpu, name, dtype, tol):
    """CPML + TF/SF around a dielectric sphere with the automatic sampling
    step, --hybrid-block 4: the intensity on a 7 x 12 grid and the total
    power against the fp64 CPU oracle of the same run, both relative to the
    peak U."""
    cfg = dataclasses.replace(SMALL if name == "small" else HYBRID, dtype=dtype)
    s = _scheme(cfg, "hip", gpu)
    if name == "hybrid":
        assert s.hybrid is not None and s.hybrid["T"] == 4, "hybrid plan rejected"
    mon = farfield_from_config(s)
    assert mon.label == "scattered" and (s.hybrid is None or mon.step % 4 == 0)
    s.perform_steps()
    torch.cuda.synchronize()
    u, total = mon.intensity(THETAS, PHIS), mon.total_power()
    samples, want_u, want_total = _oracle(name, cfg, mon.step)
    assert mon.samples == samples > 0 and u.shape == (1, 7, 12)
    peak = float(want_u.max())
    assert peak > 0
    du = float((u - want_u).abs().max()) / peak
    dp = abs(float(total[0] - want_total[0])) / peak
    print("%s %s: intensity difference %.3g of the peak U, total power difference %.3g of the peak U (bound %.3g)"
          % (name, dtype, du, dp, tol))
    assert du <= tol and dp <= tol
