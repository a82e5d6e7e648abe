"""Field probes on the GPU: the one-launch sampling kernel (csrc/
probe_kernels.hip) against the torch op on the same inputs, what the host and
the entry point refuse before any launch, and monitors end to end against the
fp64 CPU oracle and across hybrid / blocked and stepped passes
(models/probe.py)."""
import dataclasses

import pytest
import torch

from fdtd3d_amd.models.probe import ProbeMonitor
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.probe import ProbeEntries

pytestmark = pytest.mark.gpu

SHAPE = (9, 7, 11)
CAPACITY = 5
SENTINEL = -12345.678
HIP_INVALID_VALUE = 1  # hipErrorInvalidValue


def _entries(fields, offsets, device):
    ent = ProbeEntries(CAPACITY, device)
    for f in fields:
        ent.add_field(f)
    for s, off in enumerate(offsets):
        ent.add(s % len(fields), off)
    ent.series.fill_(SENTINEL)
    return ent


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("nslots", [1, 256, 257, 600])
def test_probe_kernel_vs_torch(gpu, dtype, nslots):
    """Live field arrays, slots on their first and last element and inside,
    one block / a full block / a block seam / several blocks, the first and
    the last row of the buffer: the oracle's bits (widening is exact), every
    other row untouched."""
    hip = make_ops("hip", None, gpu, dtype)
    ref = make_ops("torch", None, "cpu", dtype)
    g = torch.Generator().manual_seed(17 + nslots)
    numel = SHAPE[0] * SHAPE[1] * SHAPE[2]
    # the last element first: the single-slot case then reads the very end of its array
    offsets = ([numel - 1, 0, 0, numel - 1] + torch.randint(0, numel, (nslots,), generator=g).tolist())[:nslots]
    cpu = [torch.zeros(SHAPE, dtype=dtype) for _ in range(2)]
    dev = [torch.zeros(SHAPE, dtype=dtype, device=gpu) for _ in range(2)]
    eh, er = _entries(dev, offsets, gpu), _entries(cpu, offsets, "cpu")
    before = hip.launches
    for n, row in enumerate((0, CAPACITY - 1)):
        for a, b in zip(cpu, dev):
            a.copy_(torch.rand(SHAPE, generator=g, dtype=dtype) * 2 - 1)
            b.copy_(a)
        hip.probe_sample(eh, row)
        ref.probe_sample(er, row)
        assert hip.launches == before + n + 1  # one launch for all slots
    torch.cuda.synchronize()
    got = eh.series.cpu()
    assert got.dtype == torch.float64 and got.shape == (CAPACITY, nslots)
    assert torch.equal(got, er.series)
    assert bool((got[1:CAPACITY - 1] == SENTINEL).all()) and not bool((got[0] == SENTINEL).any())
    last = [float(cpu[s % 2].reshape(-1)[off]) for s, off in enumerate(offsets)]
    assert got[CAPACITY - 1].tolist() == last


def test_probe_refusals_launch_nothing(gpu):
    """The entry point's status for a row outside the buffer, a negative
    slot count and null pointers, and the host's own checks of rows, offsets
    and arrays: nothing reaches the GPU."""
    from fdtd3d_amd.ops.hip_lib import _ptr, _stream, c_int
    from fdtd3d_amd.ops.hip_ops import HipError
    hip = make_ops("hip", None, gpu, torch.float32)
    f = torch.rand(SHAPE, dtype=torch.float32, device=gpu)
    numel = f.numel()
    ent = _entries([f], [0, numel - 1, 40], gpu)
    hip.probe_sample(ent, 2)
    torch.cuda.synchronize()
    (tab,) = [t for k, t in ent.tables.items() if k != "torch"]
    before = hip.launches
    snapshot = ent.series.clone()
    entry = hip.fn("probe_sample")

    def status(table, n, series, row, capacity=CAPACITY):
        return entry(_ptr(table), c_int(n), _ptr(series), c_int(row), c_int(capacity), _stream())

    assert status(tab, 3, ent.series, CAPACITY) == HIP_INVALID_VALUE
    assert status(tab, 3, ent.series, -1) == HIP_INVALID_VALUE
    assert status(None, 3, ent.series, 0) == HIP_INVALID_VALUE
    assert status(tab, 3, None, 0) == HIP_INVALID_VALUE
    assert status(tab, -1, ent.series, 0) == HIP_INVALID_VALUE
    assert status(tab, 3, ent.series, 0, capacity=0) == HIP_INVALID_VALUE
    assert status(tab, 0, ent.series, 0) == 0  # no slots: nothing to launch
    for row in (CAPACITY, -1):
        with pytest.raises(HipError, match="row"):
            hip.probe_sample(ent, row)
    for off in (numel, -1, 2 ** 40):
        bad = _entries([f], [0, off], gpu)
        with pytest.raises(HipError, match="outside its array"):
            hip.probe_sample(bad, 0)
        assert not bad.tables
    with pytest.raises(HipError):
        hip.probe_sample(_entries([f.double()], [0], gpu), 0)  # not the backend's dtype
    with pytest.raises(HipError):
        hip.probe_sample(_entries([f.cpu()], [0], gpu), 0)  # not on the device
    with pytest.raises(HipError):
        hip.probe_sample(_entries([f], [0], "cpu"), 0)  # the series on the host
    with pytest.raises(HipError):
        hip.probe_sample(_entries([f.permute(2, 1, 0)], [0], gpu), 0)  # not contiguous
    empty = ProbeEntries(CAPACITY, gpu)
    empty.add_field(f)
    hip.probe_sample(empty, 0)  # a rank that owns no slot
    torch.cuda.synchronize()
    assert hip.launches == before and torch.equal(ent.series, snapshot)


# ------------------------------------------------------------------ end to end
def _scheme(cfg, backend, device):
    dt = torch.float32 if cfg.dtype == "f32" else torch.float64
    s = YeeScheme(cfg, make_ops(backend, None, device, dt))
    s.init_scheme()
    s.init_grids()
    return s


def _compare(mon, got, want, tol, what):
    """Per kind (a point Ez source leaves Hz ~ 0) against the largest value
    of the reference series."""
    assert got.shape == want.shape and got.shape[0] > 0
    worst = 0.0
    for kind in "EH":
        cols = [i for i, c in enumerate(mon.comps) if c[0] == kind]
        scale = float(want[:, :, cols].abs().max())
        assert scale > 0
        err = float((got[:, :, cols] - want[:, :, cols]).abs().max())
        worst = max(worst, err / scale)
        print("%s, %s: largest difference %.3g of scale %.3g (bound %.3g)" % (what, kind, err / scale, scale, tol))
        assert err <= tol * scale, (what, kind, err, scale)
    return worst


POINTS = [(12, 12, 12), (10, 13, 11), (9, 9, 9), (14, 11, 15), (4, 12, 12), (20, 3, 21)]


# the tolerances of tests/test_dft_gpu.py for monitors of fp32 / fp64 fields against the fp64 CPU oracle
@pytest.mark.parametrize("dtype,tol", [("f32", 2e-5), ("f64", 1e-11)])
def test_probe_run_vs_cpu_oracle(gpu, dtype, tol):
    """24^3 with CPML and TF/SF, centre probes in the total field, the
    scattered field and the absorbing layer: the HIP run's series against the
    stepped fp64 CPU run's at the same sample steps."""
    cfg = SchemeConfig(scheme="3d", size=(24, 24, 24), time_steps=48, dtype=dtype, pml_size=(5, 5, 5),
                       tfsf_size=(8, 8, 8), scene="vacuum", use_pml=True, pml_type="cpml", use_tfsf=True, theta=60,
                       phi=10, psi=5)
    s = _scheme(cfg, "hip", gpu)
    m = ProbeMonitor(s, POINTS, position="centre")
    before = s.ops.launches
    s.perform_steps()
    torch.cuda.synchronize()
    assert m.samples == cfg.time_steps // m.step > 0
    ref = _scheme(dataclasses.replace(cfg, dtype="f64", time_block=1, hybrid_block=1), "torch", "cpu")
    rm = ProbeMonitor(ref, POINTS, position="centre", step=m.step)
    ref.perform_steps()
    assert rm.steps == m.steps and rm.slots == m.slots
    _compare(m, m.series(), rm.series(), tol, "hip %s vs cpu f64" % dtype)


# the tolerances of tests/test_hybrid_gpu.py for hybrid against stepped HIP runs
HYBRID_TOL = {"f32": 2e-5, "f64": 1e-12}
PASSES = [
    ("hybrid-cpml-tfsf", dict(size=(80, 72, 96), pml_size=(5, 5, 5), tfsf_size=(8, 8, 8), scene="vacuum", use_pml=True,
                              pml_type="cpml", use_tfsf=True, theta=60, phi=10, psi=5, dtype="f32"),
     dict(hybrid_block=4), dict(hybrid_block=1), 38),
    ("hybrid-cpml-tfsf-f64", dict(size=(80, 72, 96), pml_size=(5, 5, 5), tfsf_size=(8, 8, 8), scene="vacuum",
                                  use_pml=True, pml_type="cpml", use_tfsf=True, theta=60, phi=10, psi=5, dtype="f64"),
     dict(hybrid_block=4), dict(hybrid_block=1), 30),
    ("blocked-vacuum", dict(size=(40, 36, 64), scene="vacuum", use_fused=True, dtype="f32"),
     dict(time_block=5), dict(time_block=1), 22),
]


@pytest.mark.parametrize("name,base,passes,stepped,steps", PASSES, ids=[c[0] for c in PASSES])
def test_probe_passes_vs_stepped(gpu, name, base, passes, stepped, steps):
    """The series of a hybrid / blocked run (automatic step = the pass
    length) against the same run stepped (every step sampled), at the common
    sample steps.  The TF/SF wave enters at the low corner of its box (8, 8,
    8) and has the probes next to it at 0.8 .. 1 of its amplitude within 30
    steps; the point source sits at the centre."""
    cfg = SchemeConfig(scheme="3d", time_steps=steps, **base)
    size = cfg.size
    points = [(size[0] // 2, size[1] // 2, size[2] // 2), (size[0] // 2 - 3, size[1] // 2 + 2, size[2] // 2 + 1),
              (9, 9, 9), (10, 12, 11), (8, 10, 14), (6, 9, 9), (3, 30, 40), (size[0] - 2, size[1] - 2, size[2] - 2)]
    a = _scheme(dataclasses.replace(cfg, **passes), "hip", gpu)
    T = a.hybrid["T"] if name.startswith("hybrid") else a.tb
    assert (a.hybrid is not None) == name.startswith("hybrid") and T == list(passes.values())[0]
    ma = ProbeMonitor(a, points, position="centre")
    assert ma.step == T
    a.perform_steps()
    b = _scheme(dataclasses.replace(cfg, **stepped), "hip", gpu)
    assert b.hybrid is None and b.tb == 1
    mb = ProbeMonitor(b, points, position="centre")
    assert mb.step == 1
    b.perform_steps()
    torch.cuda.synchronize()
    assert ma.steps == list(range(T, steps + 1, T)) and mb.steps == list(range(1, steps + 1))
    common = [mb.steps.index(t) for t in ma.steps]
    assert float(mb.series().abs().max()) > 0.1, "the wave has not reached the probes"
    _compare(ma, ma.series(), mb.series()[common], HYBRID_TOL[cfg.dtype], name)
