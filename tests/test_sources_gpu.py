"""Source lists on the GPU: the ``source_inject`` kernel (csrc/
source_kernels.hip) against its oracle bit for bit, equivalence with the
built-in point source, hybrid passes == stepped run with the source box cut
out of the core, linearity, and a decomposed run (thread ranks on one GPU)
against the serial one.  Loader, oracle and driver tests: test_sources_cpu.py.
"""

import pytest
import torch

from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.hip_lib import HipError
from fdtd3d_amd.ops.source import SourceEntries

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}


def run(cfg, backend, device, steps=None):
    s = YeeScheme(cfg, make_ops(backend, None, device, DT[cfg.dtype]))
    s.init_scheme()
    s.init_grids()
    s.perform_steps(steps)
    return s


def fields(s):
    return {c: s.F[0][c].detach().cpu().clone() for c in s.comps}


def same(a, b):
    """Bit-identical (as integers: -0.0 and 0.0 differ, NaNs compare)."""
    it = torch.int32 if a.dtype == torch.float32 else torch.int64
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ----------------------------------------------------------- 2. the kernel alone
def _table(fields_):
    """E and H rows over three arrays of 5 x 6 x 8: soft and hard entries, a
    cell with three soft entries of different signals, the first and the last
    element of an array, 64 signals."""
    ent = SourceEntries()
    for f in fields_:
        ent.add_field(f)
    n = 5 * 6 * 8
    ent.add("E", 0, 0, 0.75, 0)                      # first element
    ent.add("E", 0, n - 1, -1.25, 63)                # last element, the last signal
    ent.add("E", 1, 100, 1.0 / 3.0, 5)               # three soft entries on one cell, in this order
    ent.add("E", 1, 100, -2.5, 17)
    ent.add("E", 1, 100, 1e-3, 40)
    ent.add("E", 1, 101, 3.0, 1, hard=True)          # a hard neighbour
    ent.add("E", 2, 0, 0.1, 2)                       # the unaligned array: first, last, hard
    ent.add("E", 2, n - 1, 0.2, 3)
    ent.add("E", 2, 77, -7.0, 62, hard=True)
    for k in range(64):                              # every signal once
        ent.add("E", 0, 10 + 3 * k, 1.0 + 0.01 * k, k)
    ent.add("H", 0, 5, 2.0, 7)
    ent.add("H", 2, n - 1, -0.5, 0, hard=True)
    ent.add("H", 2, 8, 0.3, 63)
    ent.add("H", 2, 8, 0.7, 11)
    return ent


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_kernel_matches_oracle(gpu, dtype):
    dt = DT[dtype]
    g = torch.Generator().manual_seed(11)
    n = 5 * 6 * 8
    host = [torch.randn(n, generator=g, dtype=torch.float64).to(dt) for _ in range(3)]
    pad = torch.full((n + 3,), 9.0, dtype=dt, device=gpu)  # the third array starts one element into a buffer
    dev = [host[0].to(gpu).view(5, 6, 8), host[1].to(gpu).view(5, 6, 8), pad[1:n + 1].view(5, 6, 8)]
    dev[2].copy_(host[2].view(5, 6, 8))
    assert dev[2].data_ptr() % 16 != 0 and dev[2].is_contiguous()
    cpu = [h.clone().view(5, 6, 8) for h in host]
    vals = [float(v) for v in torch.randn(64, generator=g, dtype=torch.float64)]
    hip, ora = make_ops("hip", None, gpu, dt), make_ops("torch", None, "cpu", dt)
    e_dev, e_cpu = _table(dev), _table(cpu)
    for kind in ("E", "H"):
        before = [x.clone() for x in cpu]
        launches = hip.launches
        hip.source_inject(e_dev, kind, vals)
        assert hip.launches == launches + 1  # one launch for all entries of the kind
        ora.source_inject(e_cpu, kind, vals)
        torch.cuda.synchronize()
        named = {(fi, off) for fi, off, _, _, _ in e_cpu.rows[kind]}
        for i in range(3):
            got = dev[i].cpu()
            assert same(got, cpu[i]), (kind, i)
            mask = torch.ones(n, dtype=torch.bool)
            mask[[off for fi, off in named if fi == i]] = False
            assert same(got.view(-1)[mask], before[i].view(-1)[mask]), (kind, i)  # nothing else written
            # and every named cell was: random values and amplitudes of order 1 move each of them
            still = [off for fi, off in named if fi == i and same(got.view(-1)[off:off + 1],
                                                                  before[i].view(-1)[off:off + 1])]
            assert not still, (kind, i, still)
    assert float(pad[0]) == 9.0 and float(pad[n + 1]) == 9.0 and float(pad[n + 2]) == 9.0
    # the host check: 65 signals, a signal index past the values, an offset outside its array -- no launch
    launches = hip.launches
    keep = [x.clone() for x in dev]
    with pytest.raises(HipError, match="signal values"):
        hip.source_inject(e_dev, "E", vals + [0.0])
    with pytest.raises(HipError, match="signal"):
        hip.source_inject(e_dev, "E", vals[:63])
    bad = _table(dev)
    bad.add("H", 1, n, 1.0, 0)
    with pytest.raises(HipError, match="outside its array"):
        hip.source_inject(bad, "H", vals)
    bad = _table(dev)
    bad.add("E", 1, -1, 1.0, 0)
    with pytest.raises(HipError, match="outside its array"):
        hip.source_inject(bad, "E", vals)
    torch.cuda.synchronize()
    assert hip.launches == launches and all(same(a, b) for a, b in zip(keep, dev))


# ------------------------------------------ 3. equivalence with the built-in source
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("waveform", ["sine", "gaussian"])
def test_equals_builtin_point_source(gpu, dtype, waveform):
    kw = dict(scheme="3d", size=(16, 16, 16), time_steps=20, scene="vacuum", dtype=dtype, source=waveform,
              gaussian_width=6.0, gaussian_delay=10.0, use_fused=False, time_block=1, hybrid_block=1)
    ref = run(SchemeConfig(**kw), "hip", gpu)
    assert ref.point_source is not None and not ref.fused and ref.tb == 1 and ref.hybrid is None
    got = run(SchemeConfig(sources=[{"component": "Ez", "cell": [8, 8, 8], "kind": "hard", "waveform": waveform}],
                           **kw), "hip", gpu)
    assert got.source_list is not None and got.point_source is None
    a, b = fields(ref), fields(got)
    assert float(a["Ez"].abs().max()) > 0
    for c in a:
        assert same(a[c], b[c]), c


# --------------------------------------------------------------- 4. hybrid == stepped
def _pulse(**kw):
    return dict({"waveform": "pulse", "width": 4, "delay": 8}, **kw)


# With a 4-cell CPML and T = 3 the core starts 8 cells from every face and loses the source box grown by 4, and a
# plan needs a core of a quarter of the grid: 48 x 40 x 40 has none (its core is 22 %).  44 x 46 x 44 is the grid
# of the smallest volume that has one (even x and y, z in 4-cell lanes; searched on the oracle backend, whose
# plan is the same).  Without PML the plan exists down to degenerate grids, so that case takes a grid of several
# tiles instead; 2D TMz: 46 x 32 (y in 4-cell lanes), one step less along either axis has no plan.
HYBRID = [
    ("3d-f32-cpml", dict(scheme="3d", size=(44, 46, 44), dtype="f32", use_pml=True, pml_type="cpml",
                         pml_size=(4, 4, 4)),
     [_pulse(component="Ez", cell=[22, 23, 21], length=3), _pulse(component="Ez", cell=[25, 23, 22], amplitude=-0.5)]),
    ("3d-f64-nopml", dict(scheme="3d", size=(36, 28, 24), dtype="f64"),
     [_pulse(component="Ez", cell=[18, 14, 11], length=3), _pulse(component="Ez", cell=[21, 14, 12], amplitude=-0.5)]),
    ("tmz-f32-cpml", dict(scheme="tmz", size=(46, 32, 1), dtype="f32", use_pml=True, pml_type="cpml",
                          pml_size=(4, 4, 1)),
     [_pulse(component="Hx", cell=[23, 16], amplitude=1e-3), _pulse(component="Ez", cell=[26, 16])]),
]


@pytest.mark.parametrize("name, kw, src", HYBRID, ids=[h[0] for h in HYBRID])
def test_hybrid_equals_stepped(gpu, name, kw, src):
    T = 3
    steps = 2 * T + 2  # two passes and a tail
    base = dict(kw, time_steps=steps, scene="vacuum", sources=src, use_fused=True)
    h = run(SchemeConfig(hybrid_block=T, **base), "hip", gpu)
    assert h.hybrid is not None and h.hybrid["T"] == T and h.tb == 1 and not h.fused
    # the source box is cut out of the core: every core box is at least T + 1 cells clear of it
    assert h.hybrid["cut_cells"] > 0
    lo, hi = h.source_list.bbox()
    act = [d for d in range(3) if h.layout.active(d)]
    for b in h.hybrid["core"]:
        assert any(b[1][d] <= lo[d] - (T + 1) or b[0][d] >= hi[d] + (T + 1) for d in act), b
    s = run(SchemeConfig(hybrid_block=1, **base), "hip", gpu)
    assert s.hybrid is None and s.tb == 1 and not s.fused
    a, b = fields(h), fields(s)
    assert float(a["Ez"].abs().max()) > 0 and float(a["Hx"].abs().max()) > 0
    for c in a:
        assert same(a[c], b[c]), (name, c)


# ------------------------------------------------------------ 5. a linear system
A = {"component": "Ez", "cell": [9, 10, 10], "waveform": "pulse", "width": 8, "delay": 20, "amplitude": 1.0}
B = {"component": "Hy", "cell": [12, 9, 10], "waveform": "sine", "ramp": 10, "phase": 30, "amplitude": 2e-3}
B2 = {"component": "Ez", "cell": [9, 10, 10], "waveform": "gaussian", "width": 6, "delay": 15, "amplitude": -0.5}
PHYS = dict(scheme="3d", size=(20, 20, 20), time_steps=100, scene="vacuum", use_pml=True, pml_type="cpml",
            pml_size=(4, 4, 4), hybrid_block=1)


def test_superposition_and_scaling(gpu):
    def go(src, dtype="f64"):
        return fields(run(SchemeConfig(sources=src, dtype=dtype, **PHYS), "hip", gpu))
    ab, a, b = go([A, B, B2]), go([A]), go([B, B2])
    for kind in "EH":
        scale = max(float(ab[c].abs().max()) for c in ab if c[0] == kind)
        assert scale > 0
        for c in ab:
            if c[0] == kind:
                err = float((ab[c] - (a[c] + b[c])).abs().max())
                print(c, "superposition error", err, "of", scale)
                assert err <= 1e-11 * scale, (c, err, scale)
    # the HIP run is the oracle's run, to fp64 round-off over the 100 steps
    ora = fields(run(SchemeConfig(sources=[A, B, B2], dtype="f64", **PHYS), "torch", "cpu"))
    for c in ab:
        scale = max(float(ora[o].abs().max()) for o in ora if o[0] == c[0])
        assert float((ab[c] - ora[c]).abs().max()) <= 1e-11 * scale, c
    for dtype in ("f64", "f32"):
        one = go([A, B, B2], dtype)
        two = go([dict(e, amplitude=2 * e["amplitude"]) for e in (A, B, B2)], dtype)
        for c in one:
            assert same(2 * one[c], two[c]), (dtype, c)


def test_pulse_leaves_no_static_residue(gpu):
    """fp64 HIP counterpart of test_sources_cpu.py's test of the same name,
    with its box, envelopes and bounds: a soft gaussian deposits a static
    charge (sum(E) stays), a soft zero-mean pulse of the same envelope does
    not.  Envelope 48 steps wide, two carrier periods: the pulse's spectrum
    at DC and its cut at tau = 0 are 1e-17 of its peak."""
    res = {}
    for wf in ("pulse", "gaussian"):
        s = run(SchemeConfig(sources=[{"component": "Ez", "cell": [10, 10, 10], "waveform": wf, "width": 48,
                                       "delay": 300, "wavelength": 0.006}], dtype="f64",
                             **dict(PHYS, time_steps=1000)), "hip", gpu)
        res[wf] = abs(float(sum(s.F[0][c].double().sum() for c in s.e_comps)))
    print("sum(E) after 1000 steps:", res)
    assert res["gaussian"] > 1.0  # the integral of the envelope stays on the grid as charge
    # round-off: 2.4e4 samples x 1e3 steps of 1e-16 relative to fields of order 1 walk to ~1e-12
    assert res["pulse"] < 1e-10, res


# -------------------------------------------------------- 6. decomposed == serial
SEAM = [{"component": "Ez", "cell": [8, 8, 6], "waveform": "pulse", "width": 3, "delay": 5},       # on both seams
        {"component": "Ez", "cell": [7, 5, 6], "waveform": "sine", "amplitude": 0.5},               # a ghost of x-high
        {"component": "Ey", "cell": [10, 8, 4], "waveform": "sine", "kind": "hard", "phase": 45},  # two in a ghost
        {"component": "Hx", "cell": [9, 8, 5], "waveform": "gaussian", "width": 3, "delay": 4, "amplitude": 1e-3}]
SEAM_CFG = dict(size=(16, 16, 12), time_steps=10)


def test_decomposed_equals_serial(gpu):
    """2 x 2 x 1 thread ranks on one GPU, 3-deep ghosts: entries on the rank
    seams, inside ghost zones and on an H component."""
    from rank_threads import run_ranks
    cfg = SchemeConfig(scheme="3d", scene="vacuum", dtype="f64", sources=SEAM, **SEAM_CFG)
    ser = fields(run(cfg, "hip", gpu))

    def setup(s):
        assert s.hybrid is None and s.tb == 1

    schemes = run_ranks(cfg, (2, 2, 1), 3, "hip", gpu, setup=setup)
    assert tuple(schemes[0].domain.topology) == (2, 2, 1)
    assert float(ser["Hx"].abs().max()) > 0
    for c in ser:
        full = torch.zeros(cfg.size, dtype=torch.float64)
        for s in schemes:
            d = s.domain
            full[d.lo[0]:d.hi[0], d.lo[1]:d.hi[1], d.lo[2]:d.hi[2]] = s.owned_field(c).cpu()
        assert same(full, ser[c]), c
