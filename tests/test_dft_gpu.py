"""Running-DFT monitors on the GPU: the one-launch accumulation kernel
(csrc/dft_kernels.hip) against the torch op on the same inputs, and monitors
end to end on blocked, hybrid and launch-record passes against the fp64 CPU
oracle (models/dft.py)."""
import dataclasses
import io

import pytest
import torch

from fdtd3d_amd.models.dft import DftMonitor, monitors_from_config
from fdtd3d_amd.models.ntff import ntff_report_dft
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.dft import KIND_E, KIND_H, DftEntries, vec_width, z_pad

pytestmark = pytest.mark.gpu

# (array, box, kind): rows of whole 16-byte groups (nz = 8) and ragged rows (nz = 37) in ONE launch
A, B = "a37", "b8"
ENTRIES = [
    (A, ((1, 0, 1), (9, 7, 36)), KIND_E),    # z bounds (1, 36)
    (A, ((0, 2, 3), (8, 6, 5)), KIND_H),     # (3, 5): inside one group
    (A, ((0, 0, 0), (9, 7, 37)), KIND_E),    # (0, 37): the whole array -- and the same field as the first entry
    (A, ((4, 1, 2), (5, 6, 35)), KIND_H),    # one cell thick along x
    (A, ((2, 3, 5), (7, 4, 30)), KIND_E),    # ... along y
    (A, ((1, 1, 17), (8, 6, 18)), KIND_H),   # ... along z
    (A, ((3, 3, 9), (3, 6, 20)), KIND_E),    # empty
    (B, ((0, 1, 1), (5, 6, 7)), KIND_H),
    (B, ((1, 0, 3), (4, 5, 5)), KIND_E),
    (B, ((0, 0, 0), (5, 6, 8)), KIND_H),
    (B, ((2, 0, 0), (3, 6, 8)), KIND_E),
    (B, ((0, 4, 2), (5, 5, 6)), KIND_H),
    (B, ((0, 0, 4), (5, 6, 5)), KIND_E),
]


def _twiddles(K, sample):
    g = torch.Generator().manual_seed(100 + sample)
    return [[(float(c), float(s)) for c, s in (torch.rand(K, 2, generator=g, dtype=torch.float64) * 2 - 1)]
            for _ in range(2)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("K", [1, 8])
def test_dft_kernel_vs_torch(gpu, dtype, K):
    hip = make_ops("hip", None, gpu, dtype)
    ref = make_ops("torch", None, "cpu", dtype)
    g = torch.Generator().manual_seed(7)
    shapes = {A: (9, 7, 37), B: (5, 6, 8)}
    fields = [{n: torch.rand(s, generator=g, dtype=dtype) * 2 - 1 for n, s in shapes.items()} for _ in range(5)]
    dev = {n: torch.zeros(s, dtype=dtype, device=gpu) for n, s in shapes.items()}
    cpu = {n: torch.zeros(s, dtype=dtype) for n, s in shapes.items()}
    eh, er = DftEntries(K), DftEntries(K)
    for n, box, kind in ENTRIES:
        eh.add(dev[n], box, kind)
        er.add(cpu[n], box, kind)
    tol = 1e-6 if dtype == torch.float32 else 1e-14
    v = vec_width(dtype)
    before = hip.launches
    for sample in range(5):
        for n in shapes:
            dev[n].copy_(fields[sample][n])
            cpu[n].copy_(fields[sample][n])
        tw = _twiddles(K, sample)
        hip.dft_accumulate(eh, tw)
        ref.dft_accumulate(er, tw)
        assert hip.launches == before + sample + 1  # one launch for all entries
        if sample in (0, 4):
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(eh, er)):
                assert a.acc.shape == b.acc.shape
                if b.empty:
                    assert a.acc.numel() == 0
                    continue
                scale = float(b.acc.abs().max())
                assert scale > 0
                err = float((a.acc.cpu() - b.acc).abs().max())
                assert err <= tol * scale, (i, sample, err, scale)
                # padded cells are never written
                z0, zp = z_pad(b.box, v)
                pad = torch.ones(zp, dtype=torch.bool)
                pad[b.box[0][2] - z0:b.box[1][2] - z0] = False
                assert float(a.acc.cpu()[..., pad].abs().max() if pad.any() else 0.0) == 0.0, i


def test_dft_host_validation(gpu):
    from fdtd3d_amd.ops.hip_ops import HipError
    hip = make_ops("hip", None, gpu, torch.float32)
    f = torch.zeros((5, 6, 8), dtype=torch.float32, device=gpu)
    before = hip.launches
    for box in (((0, 0, 0), (5, 6, 9)), ((0, -1, 0), (5, 6, 8)), ((0, 0, 0), (6, 6, 8))):
        e = DftEntries(1)
        e.add(f, ((0, 0, 0), (5, 6, 8)), KIND_E)
        e.add(f, box, KIND_H)
        with pytest.raises(HipError):
            hip.dft_accumulate(e, [[(1.0, 0.0)], [(1.0, 0.0)]])
    e9 = DftEntries(9)
    e9.add(f, ((0, 0, 0), (5, 6, 8)), KIND_E)
    with pytest.raises(HipError):
        hip.dft_accumulate(e9, [[(1.0, 0.0)] * 9] * 2)
    e = DftEntries(1)
    e.add(f.double(), ((0, 0, 0), (5, 6, 8)), KIND_E)  # not the backend's dtype
    with pytest.raises(HipError):
        hip.dft_accumulate(e, [[(1.0, 0.0)], [(1.0, 0.0)]])
    assert hip.launches == before


def _scheme(cfg, backend, device):
    dt = torch.float32 if cfg.dtype == "f32" else torch.float64
    s = YeeScheme(cfg, make_ops(backend, None, device, dt))
    s.init_scheme()
    s.init_grids()
    return s


def _oracle(cfg, step, **kw):
    """The fp64 CPU run with the SAME sampling step, stepped one step at a time."""
    ref = _scheme(dataclasses.replace(cfg, dtype="f64", time_block=1, hybrid_block=1, dft_step=step, **kw), "torch",
                  "cpu")
    mons = monitors_from_config(ref)
    ref.perform_steps()
    return ref, mons


def _compare(mon, rmon, tol):
    assert mon.samples == rmon.samples and mon.samples > 0
    assert mon.requests == rmon.requests
    worst = 0.0
    for k in range(len(mon.wavelengths)):
        ph = [(c, mon.phasor(i, k).cpu().to(torch.complex128), rmon.phasor(i, k)) for i, (c, _) in
              enumerate(mon.requests)]
        for c, a, b in ph:
            # scale by the kind's largest phasor (a point Ez source leaves Hz ~ 0)
            scale = max(float(r.abs().max()) for o, _, r in ph if o[0] == c[0] and r.numel())
            assert scale > 0
            err = float((a - b).abs().max()) if b.numel() else 0.0
            worst = max(worst, err / scale)
            assert err <= tol * scale, (c, k, err, scale)
    print("phasors: largest difference %.3g of scale (bound %.3g)" % (worst, tol))


@pytest.mark.parametrize("dtype,tol", [("f32", 2e-5), ("f64", 1e-11)])
def test_dft_blocked_end_to_end(gpu, dtype, tol):
    """3D vacuum on the blocked path, whole-grid monitor at two wavelengths,
    automatic step: the passes between samples stay blocked."""
    cfg = SchemeConfig(scheme="3d", size=(40, 36, 64), time_steps=40, scene="vacuum", dtype=dtype, use_fused=True,
                       time_block=0, use_dft=True, dft_wavelengths="0.02,0.03", dft_step=0)
    s = _scheme(cfg, "hip", gpu)
    mon = monitors_from_config(s)["box"]
    assert s.tb > 1 and mon.step % s.tb == 0
    s.perform_steps()
    torch.cuda.synchronize()
    assert s.tb > 1
    ref, rmons = _oracle(cfg, mon.step)
    _compare(mon, rmons["box"], tol)


@pytest.mark.parametrize("dtype,tol", [("f32", 2e-5), ("f64", 1e-11)])
def test_dft_hybrid_ntff(gpu, dtype, tol):
    """Hybrid passes (CPML + TF/SF around a dielectric sphere) with the
    NTFF-surface monitor: phasors of the 24 slabs and the diagram computed
    from them against the fp64 oracle (the diagram relative to its peak).
    160 steps: the wave scattered by the sphere has to be back at the surface,
    or the diagram is that of fp32 noise against a signal that is not there
    yet."""
    cfg = SchemeConfig(scheme="3d", size=(80, 72, 96), time_steps=160, dtype=dtype, pml_size=(5, 5, 5),
                       tfsf_size=(8, 8, 8), ntff_size=(6, 6, 6), scene="sphere", sphere_center=(40.0, 36.0, 48.0),
                       sphere_radius=20.0, use_pml=True, pml_type="cpml", use_tfsf=True, use_ntff=True, ntff_dft=True,
                       hybrid_block=4)
    s = _scheme(cfg, "hip", gpu)
    assert s.hybrid is not None, "hybrid plan rejected"
    mon = monitors_from_config(s)["ntff"]
    assert mon.step % s.hybrid["T"] == 0 and len(mon.requests) == 24
    s.perform_steps()
    torch.cuda.synchronize()
    ref, rmons = _oracle(cfg, mon.step)
    assert ref.hybrid is None
    _compare(mon, rmons["ntff"], tol)
    p = ntff_report_dft(s, mon, s.t, out=io.StringIO()).cpu()
    q = ntff_report_dft(ref, rmons["ntff"], ref.t, out=io.StringIO())
    peak = float(q.max())
    assert peak > 0
    err = float((p - q).abs().max())
    print("diagram: peak %.6g, largest difference %.3g of it" % (peak, err / peak))
    assert err <= tol * peak, (err, peak)


def test_dft_2d_launch_records(gpu):
    """TMz hybrid passes re-issued from launch records (--hybrid-graph auto):
    the sampling steps cut the passes, records and replays go on between
    them, and the monitor's sums equal the oracle's."""
    cfg = SchemeConfig(scheme="tmz", size=(120, 104, 1), time_steps=60, dtype="f32", pml_size=(6, 6, 1),
                       tfsf_size=(10, 10, 1), scene="vacuum", use_pml=True, pml_type="cpml", use_tfsf=True, phi=30,
                       hybrid_block=5, hybrid_graph="auto", use_dft=True, dft_step=20)
    s = _scheme(cfg, "hip", gpu)
    assert s.hybrid is not None, "hybrid plan rejected"
    mon = monitors_from_config(s)["box"]
    s.perform_steps()
    torch.cuda.synchronize()
    assert getattr(s, "_hrec", None) is not None, "no launch-record replay"
    assert mon.samples == 3
    ref, rmons = _oracle(cfg, 20)
    _compare(mon, rmons["box"], 2e-5)
