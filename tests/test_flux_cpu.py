"""Poynting-flux monitors (models/flux.py) on the torch / CPU oracle, fp64:
the face sums against a numpy evaluation of recorded slabs, power conservation
of a source behind a PML, a lossless and a lossy scatterer, the incident
normalisation, decomposed thread ranks, the refusals and the options."""
import dataclasses
import io
import json
import math
import os
import subprocess
import threading

import numpy as np
import pytest
import torch

from fdtd3d_amd import native
from fdtd3d_amd.layout.materials import Scene
from fdtd3d_amd.models.dft import DftMonitor
from fdtd3d_amd.models.flux import FluxMonitor, flux_from_config
from fdtd3d_amd.models.ntff import ETA0, _faces, _plan_box, _sample_plan, ntff_requests
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.parallel.comm import LocalHub
from fdtd3d_amd.parallel.halo import HaloExchanger
from fdtd3d_amd.parallel.topology import ParallelGridCore
from fdtd3d_amd.utils.assertions import FdtdError
from fdtd3d_amd.utils.settings import Settings

PERIOD = 80  # steps of the default wavelength 0.02 at dx = 0.0005, Courant 0.5
START, PERIODS = 240, 2  # the steady-state window of tests/test_dft_cpu.py's NTFF runs

SOURCE = dict(scheme="3d", size=(28, 28, 28), pml_size=(5, 5, 5), scene="vacuum", use_pml=True, pml_type="cpml",
              use_point_source=True)
SPHERE = dict(scheme="3d", size=(28, 28, 28), pml_size=(5, 5, 5), tfsf_size=(9, 9, 9), scene="sphere",
              sphere_center=(14.0, 14.0, 14.0), sphere_radius=3.0, use_pml=True, pml_type="cpml", use_tfsf=True)

# measured on the CPU oracle with the window above (profiles/flux.md); the bounds are twice the measured values,
# the project's convention for transient-limited physics checks
CONSERVATION_MEASURED = 9.14e-4  # |net(margin 7) - net(margin 9)| / net(margin 7), sine point source
LOSSLESS_MEASURED = 3.49e-4  # |net(margin 11)| / scattered(margin 7), dielectric sphere
LOSSY_MEASURED = 11.0        # absorbed(margin 11) / scattered(margin 7), Drude sphere with damping
LOSSY_GAMMA = 0.3            # damping of the lossy sphere in units of the source's angular frequency


def make(cfg, domain=None, halo=None):
    s = YeeScheme(cfg, make_ops("torch", None, "cpu", torch.float64), domain, halo)
    s.init_scheme()
    s.init_grids()
    return s


def sl(box):
    return tuple(slice(box[0][a], box[1][a]) for a in range(3))


def numpy_power(size, margin, dx, phasor):
    """(6,) face powers by the formula of the issue from ``phasor(comp, box)``
    -> complex slab, plus the sum of the absolute terms per face."""
    P, S = np.zeros(6), np.zeros(6)
    for f, (axis, x0, sign, lo, hi) in enumerate(_faces(size, margin)):
        def centre(comp):
            plan = _sample_plan(comp, axis, x0, lo, hi)
            box = _plan_box(plan)
            slab = phasor(comp, box)
            acc, cnt = 0, 0
            for ox in plan[0][2]:
                for oy in plan[1][2]:
                    for oz in plan[2][2]:
                        o = (ox, oy, oz)
                        acc = acc + slab[tuple(slice(o[a], o[a] + plan[a][1]) for a in range(3))]
                        cnt += 1
            return acc / cnt

        b, c = "xyz"[(axis + 1) % 3], "xyz"[(axis + 2) % 3]
        t1 = (centre("E" + b) * np.conj(centre("H" + c))).real
        t2 = (centre("E" + c) * np.conj(centre("H" + b))).real
        P[f] = sign * dx * dx * 0.5 * (t1.sum() - t2.sum())
        S[f] = dx * dx * 0.5 * (np.abs(t1).sum() + np.abs(t2).sum())
    return P, S


# -------------------------------------------------------------------- plumbing
def test_flux_plumbing():
    """power() == the numpy evaluation of the same formula on phasors built
    by a numpy DFT of the recorded slabs."""
    cfg = SchemeConfig(time_steps=60, **SOURCE)
    s = make(cfg)
    m = FluxMonitor(s, (8, 8, 8), [0.02, 0.031], step=1, start=11)
    req = ntff_requests(cfg.size, (8, 8, 8))
    assert m.dft.requests == req and len(req) == 24 and m.dft.h_time == "half"
    rec = []
    s.hooks.append(lambda sc, t: rec.append((t, {key: sc.F[0][key[0]][sl(key[1])].numpy().copy() for key in req}))
                   if t >= 11 else None)
    s.perform_steps()
    assert m.samples == 50 == len(rec)
    got = m.power()
    assert got.shape == (6, 2) and got.dtype == torch.float64
    for k, w in enumerate(m.omegas):
        def phasor(comp, box):
            off = 0.0 if comp[0] == "E" else 0.5
            return sum(f[(comp, box)] * np.exp(1j * w * (t - 1 + off) * s.dt) for t, f in rec) * 2 / len(rec)

        want, scale = numpy_power(cfg.size, (8, 8, 8), s.dx, phasor)
        assert scale.min() > 0
        err = np.abs(got[:, k].numpy() - want) / scale
        print("k=%d: largest difference %.3g of the sum of absolute terms" % (k, err.max()))
        assert err.max() <= 1e-12
    assert torch.equal(m.net(), got.sum(dim=0))
    assert m.label == "radiated"
    with pytest.raises(FdtdError):
        m.cross_section()


# ----------------------------------------------------------- power conservation
@pytest.fixture(scope="module")
def source_run():
    cfg = SchemeConfig(time_steps=START + PERIOD * PERIODS, **SOURCE)
    s = make(cfg)
    wl = [cfg.wavelength]
    m7 = FluxMonitor(s, (7, 7, 7), wl, step=1, start=START + 1)
    m9 = FluxMonitor(s, (9, 9, 9), wl, step=1, start=START + 1)
    same = DftMonitor(s, ntff_requests(cfg.size, (7, 7, 7)), wl, 1, START + 1, h_time="same")
    s.perform_steps()
    return s, m7, m9, same


def test_flux_power_conservation_source(source_run):
    """The net power of a sine point source through two boxes around it,
    behind a CPML, over whole periods in steady state: positive and equal.
    Measured relative difference: CONSERVATION_MEASURED (the bound is twice
    that)."""
    s, m7, m9, _ = source_run
    assert m7.samples == m9.samples == PERIOD * PERIODS
    p7, p9 = float(m7.net()[0]), float(m9.net()[0])
    rel = abs(p7 - p9) / p7
    print("net power: margin 7 %.9g W, margin 9 %.9g W, relative difference %.3g (measured %.3g)"
          % (p7, p9, rel, CONSERVATION_MEASURED))
    assert p7 > 0 and p9 > 0
    assert (m7.power() > 0).all() and (m9.power() > 0).all()  # outward through every face
    assert rel <= 2 * CONSERVATION_MEASURED


def test_flux_time_convention_control(source_run):
    """With H phasors taken at the E time (h_time="same", through the raw
    DftMonitor) the power carries the half-step error: H' = H exp(-i w dt /
    2), so per face P' = P cos(w dt / 2) - Q sin(w dt / 2) with Q the reactive
    counterpart of P.  The monitor's own result (h_time="half") is the P of
    that identity, not P'."""
    s, m7, _, same = source_run
    w = m7.omegas[0]
    half = w * s.dt / 2
    assert abs(half - 2 * math.pi / 160) < 1e-12

    def ph(mon):
        return lambda comp, box: mon.phasor((comp, box)).numpy()

    P, S = numpy_power(s.cfg.size, (7, 7, 7), s.dx, ph(m7.dft))
    Pp, _ = numpy_power(s.cfg.size, (7, 7, 7), s.dx, ph(same))
    # the reactive counterpart: the same sums with H rotated by a quarter period
    Q, _ = numpy_power(s.cfg.size, (7, 7, 7), s.dx,
                       lambda comp, box: m7.dft.phasor((comp, box)).numpy() * (1j if comp[0] == "H" else 1))
    got = m7.power()[:, 0].numpy()
    print("P %s\nP' / P - 1 %s (cos - 1 = %.3g)\nQ / P %s" % (P, Pp / P - 1, math.cos(half) - 1, Q / P))
    assert np.abs(got - P).max() <= 1e-12 * S.max()
    # the control has the error: P' is P cos - Q sin, and differs from P by far more than the arithmetic
    assert np.abs(Pp - (P * math.cos(half) - Q * math.sin(half))).max() <= 1e-12 * S.max()
    assert (np.abs(Pp - P) > 1e-6 * np.abs(P)).all()
    # the monitor's own result does not
    assert not (np.abs(got - Pp) <= 1e-9 * np.abs(P)).any()


# --------------------------------------------------------- scatterers, TF/SF
def _sphere_run(**kw):
    cfg = SchemeConfig(time_steps=START + PERIOD * PERIODS, **dict(SPHERE, **kw))
    s = make(cfg)
    wl = [cfg.wavelength]
    inner = FluxMonitor(s, (11, 11, 11), wl, step=1, start=START + 1)
    outer = FluxMonitor(s, (7, 7, 7), wl, step=1, start=START + 1)
    s.perform_steps()
    return s, inner, outer


@pytest.fixture(scope="module")
def lossless_run():
    return _sphere_run()


def test_flux_lossless_scatterer(lossless_run):
    """Dielectric sphere in a TF/SF plane wave: the net power through a box
    inside the TF box is a small fraction of the scattered power through a
    box outside it.  Measured: LOSSLESS_MEASURED (the bound is twice that)."""
    s, inner, outer = lossless_run
    assert inner.label == "absorbed" and outer.label == "scattered"
    scat = float(outer.net()[0])
    ratio = abs(float(inner.net()[0])) / scat
    print("scattered %.9g W, net inside %.9g W, ratio %.3g (measured %.3g)"
          % (scat, float(inner.net()[0]), ratio, LOSSLESS_MEASURED))
    assert scat > 0
    assert ratio <= 2 * LOSSLESS_MEASURED
    # sine source over whole periods: the cross-section is the power over 1 / (2 eta0)
    assert abs(float(outer.cross_section()[0]) - scat * 2 * ETA0) <= 1e-10 * scat * 2 * ETA0
    assert torch.equal(inner.cross_section(), -inner.net() / inner.incident())


def test_flux_lossy_scatterer(lossless_run, monkeypatch):
    """The same boxes around a Drude sphere with damping: the absorbed power
    exceeds the lossless residual by a clear factor (at least 10 times, both
    relative to the scattered power).  Measured: LOSSY_MEASURED."""
    g = LOSSY_GAMMA * 2 * math.pi * lossless_run[0].source_frequency
    uniform = Scene.uniform
    monkeypatch.setattr(Scene, "gamma_e", lambda self, x, y, z, mod: torch.full_like(x, g))
    monkeypatch.setattr(Scene, "uniform", lambda self, name: g if name == "gamma_e" else uniform(self, name))
    s, inner, outer = _sphere_run(scene="drude-sphere", use_metamaterials=True)
    absorbed = -float(inner.net()[0])
    scat = float(outer.net()[0])
    _, li, lo = lossless_run
    residual = abs(float(li.net()[0])) / float(lo.net()[0])
    print("absorbed %.9g W, scattered %.9g W, ratio %.3g (measured %.3g); lossless residual %.3g"
          % (absorbed, scat, absorbed / scat, LOSSY_MEASURED, residual))
    assert absorbed > 0 and scat > 0
    assert absorbed / scat >= 10 * residual


# --------------------------------------------------------------- normalisation
def test_flux_incident_normalisation():
    cfg = SchemeConfig(time_steps=30 + PERIOD, **dict(SPHERE, size=(24, 24, 24), tfsf_size=(8, 8, 8),
                                                      sphere_center=(12.0, 12.0, 12.0)))
    s = make(cfg)
    m = FluxMonitor(s, (6, 6, 6), [cfg.wavelength], step=1, start=31)
    s.perform_steps()
    assert m.samples == PERIOD
    assert abs(float(m.incident()[0]) * 2 * ETA0 - 1) <= 1e-12
    g = make(dataclasses.replace(cfg, source="gaussian", gaussian_width=12.0, gaussian_delay=40.0))
    wl = [0.02, 0.027, 0.04]
    mg = FluxMonitor(g, (6, 6, 6), wl, step=3, start=4)
    g.perform_steps()
    ts = [t for t in range(4, cfg.time_steps + 1, 3)]
    assert mg.samples == len(ts)
    v = np.array([g.source_value(t - 1, 0) for t in ts])
    for k, w in enumerate(mg.omegas):
        a = (v * np.exp(1j * w * (np.array(ts) - 1) * g.dt)).sum() * 2 / len(ts)
        want = abs(a) ** 2 / (2 * ETA0)
        assert want > 0 and abs(float(mg.incident()[k]) - want) <= 1e-12 * want, k


# ---------------------------------------------------------------- decomposition
@pytest.mark.parametrize("world,axes,topo", [(4, "xz", (2, 1, 2)), (2, "y", (1, 2, 1))])
def test_flux_decomposed_equals_serial(world, axes, topo):
    cfg = SchemeConfig(scheme="3d", size=(16, 14, 18), time_steps=23, scene="vacuum", use_point_source=True)
    ser = make(cfg)
    sm = FluxMonitor(ser, (3, 2, 4), [0.02, 0.027], step=2, start=3)
    ser.perform_steps()
    want = sm.power()
    core = ParallelGridCore.create(cfg.size, world, axes, requested=topo, optimal=False)
    hub = LocalHub(world, tagless=True)
    out, errors = [None] * world, []

    def body(rank):
        try:
            dom = core.domain(rank, 1)
            halo = HaloExchanger(dom, comm=hub.comm(rank), mode="direct")
            s = make(cfg, dom, halo)
            m = FluxMonitor(s, (3, 2, 4), [0.02, 0.027], step=2, start=3)
            s.perform_steps()
            halo.drain(s)
            out[rank] = (m.samples, m.power())
        except BaseException as e:  # surface thread failures in the test
            errors.append(e)

    torch.set_num_threads(1)
    ths = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=600)
    if errors:
        raise errors[0]
    assert all(o[0] == sm.samples == 11 for o in out)
    assert all(o[1] is None for o in out[1:])
    got = out[0][1]
    assert float(want.abs().min()) > 0
    rel = float(((got - want).abs() / want.abs()).max())
    print("largest relative difference to the serial run: %.3g" % rel)
    assert rel <= 1e-13


# -------------------------------------------------------------------- refusals
def test_flux_refusals():
    def mon(margin=(6, 6, 6), **kw):
        cfg = SchemeConfig(time_steps=2, **dict(dict(scheme="3d", size=(20, 20, 20), scene="vacuum"), **kw))
        return FluxMonitor(make(cfg), margin, [0.02], step=1)

    assert mon().label == "radiated"
    with pytest.raises(FdtdError):
        mon(scheme="tmz", size=(20, 20, 1))
    with pytest.raises(FdtdError):
        mon(scheme="1d", size=(20, 1, 1))
    with pytest.raises(FdtdError):
        mon(complex_values=True)
    with pytest.raises(FdtdError):
        mon(use_amp_mode=True)
    with pytest.raises(FdtdError):
        mon(margin=(10, 6, 6))  # empty along x
    tf = dict(use_tfsf=True, tfsf_size=(8, 8, 8))
    assert mon(margin=(6, 6, 6), **tf).label == "scattered"
    assert mon(margin=(10, 10, 10), size=(26, 26, 26), **tf).label == "absorbed"
    for margin in ((7, 6, 6), (6, 6, 9), (8, 8, 8), (6, 9, 6)):  # a face less than 2 cells from the TF/SF face
        with pytest.raises(FdtdError, match="TF/SF"):
            mon(margin=margin, size=(26, 26, 26), **tf)
    with pytest.raises(FdtdError, match="TF/SF"):
        mon(margin=(6, 10, 6), size=(26, 26, 26), **tf)  # crosses the TF/SF box


# --------------------------------------------------------------------- options
FLUX_ARGV = ["--use-flux", "--flux-sizex", "4", "--same-size-flux", "--flux-sizez", "5", "--flux-report-step", "10",
             "--dft-wavelengths", "0.02,0.025", "--dft-step", "6", "--dft-start", "11"]


def test_flux_options_round_trip():
    s = Settings()
    assert s.set_from_cmd(FLUX_ARGV, out=io.StringIO()) == 0
    s.validate()
    assert (s.doUseFlux, s.fluxSizeX, s.fluxSizeY, s.fluxSizeZ, s.fluxReportStep) == (True, 4, 4, 5, 10)
    cfg = SchemeConfig.from_settings(s)
    assert cfg.use_flux and cfg.flux_size == (4, 4, 5) and cfg.flux_report_step == 10
    assert (cfg.dft_wavelengths, cfg.dft_step, cfg.dft_start) == ("0.02,0.025", 6, 11)
    d = Settings()
    assert (d.doUseFlux, d.fluxSizeX, d.fluxSizeY, d.fluxSizeZ, d.fluxReportStep) == (False, 0, 0, 0, 0)
    assert not SchemeConfig().use_flux and flux_from_config(make(SchemeConfig(size=(8, 8, 8), scene="vacuum"))) is None


def test_flux_native_parser_agrees():
    st, nat = native.parse_settings(FLUX_ARGV)
    s = Settings()
    assert s.set_from_cmd(FLUX_ARGV, out=io.StringIO()) == 0 and st == 0, nat
    for k, v in s.as_dict().items():
        assert nat[k] == v, k
    assert nat["doUseFlux"] is True and nat["fluxSizeY"] == 4 and nat["fluxSizeZ"] == 5


RUN_ARGV = ["--3d", "--sizex", "20", "--same-size", "--time-steps", "25", "--backend", "torch", "--device", "cpu",
            "--dtype", "f64", "--scene", "vacuum", "--dft-wavelengths", "0.02,0.03", "--dft-step", "4",
            "--dft-start", "5", "--json"]


def test_flux_driver_run(tmp_path):
    """The Python driver end to end: report lines every --flux-report-step
    steps and at the end, the flux object of --json, and the dft object of a
    --use-dft --use-flux run unchanged."""
    from fdtd3d_amd.runner import run
    flux = ["--use-flux", "--flux-sizex", "5", "--same-size-flux", "--flux-report-step", "10"]
    out = io.StringIO()
    assert run(RUN_ARGV + flux + ["--output-dir", str(tmp_path)], out=out) == 0
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("=== flux ")]
    assert len(lines) == 2 * 3  # t = 10, 20 and the end, two wavelengths each
    assert lines[0].startswith("=== flux t=10, wavelength 0.02: faces ") and lines[-1].startswith("=== flux t=25, ")
    assert all(ln.endswith(" W radiated") and len(ln.split("faces ")[1].split(";")[0].split()) == 6 for ln in lines)
    rec = json.loads(out.getvalue().strip().splitlines()[-1])
    fl = rec["flux"]
    assert {k: fl[k] for k in ("wavelengths", "step", "start", "samples", "label", "cross_section")} == \
        {"wavelengths": [0.02, 0.03], "step": 4, "start": 5, "samples": 6, "label": "radiated", "cross_section": None}
    assert len(fl["net"]) == 2 and all(v > 0 for v in fl["net"])
    assert float(lines[-1].split("net ")[1].split()[0]) == pytest.approx(fl["net"][1], rel=1e-8)
    assert "dft" not in rec
    dft = ["--use-dft", "--dft-sizex", "2", "--same-size-dft"]
    a, b = io.StringIO(), io.StringIO()
    assert run(RUN_ARGV + dft + ["--output-dir", str(tmp_path)], out=a) == 0
    assert run(RUN_ARGV + dft + flux + ["--output-dir", str(tmp_path)], out=b) == 0
    ra, rb = (json.loads(o.getvalue().strip().splitlines()[-1]) for o in (a, b))
    assert ra["dft"] == rb["dft"] == {"wavelengths": [0.02, 0.03], "step": 4, "start": 5, "samples": 6,
                                      "h_time": "half"}
    assert "flux" not in ra and rb["flux"]["net"] == fl["net"]


def test_flux_driver_tfsf_cross_section(tmp_path):
    from fdtd3d_amd.runner import run
    argv = ["--3d", "--sizex", "24", "--same-size", "--time-steps", "20", "--backend", "torch", "--device", "cpu",
            "--dtype", "f64", "--scene", "sphere", "--sphere-radius", "3", "--sphere-center-x", "12",
            "--sphere-center-y", "12", "--sphere-center-z", "12", "--use-tfsf", "--tfsf-sizex", "8",
            "--same-size-tfsf", "--use-flux", "--flux-sizex", "5", "--same-size-flux", "--dft-step", "2", "--json",
            "--output-dir", str(tmp_path)]
    out = io.StringIO()
    assert run(argv, out=out) == 0, out.getvalue()
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("=== flux ")]
    assert len(lines) == 1 and " W scattered; cross-section " in lines[0] and lines[0].endswith(" m^2")
    rec = json.loads(out.getvalue().strip().splitlines()[-1])
    assert rec["flux"]["label"] == "scattered" and len(rec["flux"]["cross_section"]) == 1


@pytest.mark.parametrize("extra,word", [(["--complex-field-values"], "--complex-field-values"),
                                        (["--use-amp-mode"], "--use-amp-mode"),
                                        (["--checkpoint-dir", "ck"], "checkpoint"),
                                        (["--load-from-file", "ck"], "checkpoint")])
def test_flux_driver_refusals(extra, word, tmp_path):
    from fdtd3d_amd.runner import run
    argv = ["--3d", "--sizex", "12", "--same-size", "--time-steps", "2", "--backend", "torch", "--device", "cpu",
            "--scene", "vacuum", "--use-flux", "--flux-sizex", "3", "--same-size-flux", "--output-dir",
            str(tmp_path)] + extra
    out = io.StringIO()
    assert run(argv, out=out) == 1
    assert "--use-flux" in out.getvalue() and word in out.getvalue()
    assert not os.listdir(tmp_path)


def test_flux_driver_refuses_2d(tmp_path):
    from fdtd3d_amd.runner import run
    out = io.StringIO()
    assert run(["--2d", "--sizex", "12", "--sizey", "12", "--time-steps", "2", "--backend", "torch", "--device", "cpu",
                "--scene", "vacuum", "--use-flux", "--output-dir", str(tmp_path)], out=out) == 1
    assert "--use-flux" in out.getvalue() and "3D" in out.getvalue()


def test_flux_native_driver_refuses():
    exe = native.executable()
    assert os.path.exists(exe), "fdtd3d executable not built"
    r = subprocess.run([exe, "--3d", "--use-flux"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--use-flux" in r.stderr and "python -m fdtd3d_amd" in r.stderr
