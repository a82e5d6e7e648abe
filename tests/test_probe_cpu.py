"""Field probes (models/probe.py) on the torch / CPU oracle, fp64: the series
against the field elements and against an independent mean, the spectrum
against the running-DFT monitor and against the 1D dispersion relation,
decomposed thread ranks, blocked passes, the refusals, the options and the
driver."""
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
from fdtd3d_amd.layout.yee import MIN_COORD_FP
from fdtd3d_amd.models.dft import DftMonitor, monitor_box_requests
from fdtd3d_amd.models.energy import EnergyMonitor
from fdtd3d_amd.models.ntff import ETA0
from fdtd3d_amd.models.probe import ProbeMonitor, auto_step, band_wavelengths, probes_from_config
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.probe import ProbeEntries
from fdtd3d_amd.parallel.comm import LocalHub
from fdtd3d_amd.parallel.halo import HaloExchanger
from fdtd3d_amd.parallel.topology import ParallelGridCore
from fdtd3d_amd.utils.assertions import FdtdError
from fdtd3d_amd.utils.constants import SPEED_OF_LIGHT
from fdtd3d_amd.utils.settings import Settings


def make(cfg, domain=None, halo=None, dtype=torch.float64):
    s = YeeScheme(cfg, make_ops("torch", None, "cpu", dtype), domain, halo)
    s.init_scheme()
    s.init_grids()
    return s


# ------------------------------------------------------------------------- op
def test_probe_sample_op():
    ops = make_ops("torch", None, "cpu", torch.float32)
    g = torch.Generator().manual_seed(3)
    a = torch.rand((4, 3, 5), generator=g, dtype=torch.float32)
    b = torch.rand((2, 6, 2), generator=g, dtype=torch.float32)
    ent = ProbeEntries(3)
    fa, fb = ent.add_field(a), ent.add_field(b)
    slots = [(fa, 0), (fb, 23), (fa, 59), (fb, 0), (fa, 31)]
    for f, off in slots:
        ent.add(f, off)
    ent.series.fill_(-7.0)
    ops.probe_sample(ent, 1)
    want = [float((a if f == fa else b).reshape(-1)[off]) for f, off in slots]
    assert ent.series.dtype == torch.float64 and ent.series[1].tolist() == want
    assert bool((ent.series[0] == -7.0).all()) and bool((ent.series[2] == -7.0).all())
    for row in (-1, 3):
        with pytest.raises(ValueError):
            ops.probe_sample(ent, row)
    ent.add(fb, 24)  # one past the end of b
    with pytest.raises(ValueError, match="outside its array"):
        ops.probe_sample(ent, 0)
    with pytest.raises(ValueError):
        ProbeEntries(0)


# ---------------------------------------------------------------- node series
GRIDS = {"3d": (dict(scheme="3d", size=(12, 12, 12)), [(6, 6, 6), (0, 0, 0), (11, 11, 11), (5, 6, 7), (7, 5, 6)]),
         "tmz": (dict(scheme="tmz", size=(12, 12, 1)), [(6, 6), (0, 0), (11, 11), (5, 7), (7, 6)]),
         "tez": (dict(scheme="tez", size=(12, 12, 1)), [(6, 6), (0, 0), (11, 11), (5, 7), (7, 6)]),
         "1d": (dict(scheme="1d", size=(24, 1, 1)), [(12,), (0,), (23,), (11,), (14,)])}
STEPS = 14


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_node_series_is_the_field(name):
    """After every sample the newest row equals the field elements bit for
    bit, and series() returns exactly the rows seen."""
    kw, points = GRIDS[name]
    s = make(SchemeConfig(time_steps=STEPS, scene="vacuum", **kw))
    m = ProbeMonitor(s, points, step=1)
    assert m.comps == tuple(s.comps) and m.position == "node" and m.entries.capacity == STEPS + 1
    seen = []
    for t in range(1, STEPS + 1):
        s.advance(1)
        assert m.samples == t and m.steps[-1] == t
        row = m.entries.series[t - 1]
        want = [float(s.F[0][c][tuple(p) + (0,) * (3 - len(p))]) for p in points for c in m.comps]
        assert row.tolist() == want, t
        seen.append(want)
    got = m.series()
    assert got.shape == (STEPS, len(points), len(m.comps)) and got.dtype == torch.float64
    assert torch.equal(got, torch.tensor(seen, dtype=torch.float64).reshape(got.shape))
    assert float(got.abs().max()) > 0  # the point source has reached the probes around it
    te, th = m.times()
    assert te.tolist() == [(t - 1) * s.dt for t in range(1, STEPS + 1)]
    assert th.tolist() == [(t - 1) * s.dt + 0.5 * s.dt for t in range(1, STEPS + 1)]
    assert (float(te[0]), float(th[0])) == DftMonitor(s, [], [0.02], step=1, register=False).sample_times(s, 1)


def test_components_start_and_step():
    s = make(SchemeConfig(scheme="3d", size=(12, 12, 12), time_steps=20, scene="vacuum"))
    m = ProbeMonitor(s, [(6, 6, 5)], ["Hy", "Ez"], step=4, start=6)
    s.perform_steps()
    assert m.steps == [6, 10, 14, 18] and m.entries.capacity == 5  # ceil((20 - 6) / 4) + 1
    assert m.series().shape == (4, 1, 2) and m.comps == ("Hy", "Ez")
    s.advance(12)  # beyond the budget: the buffer grows, the rows stay
    assert m.steps[-1] == 30 and m.series().shape == (7, 1, 2)


# -------------------------------------------------------------- centre series
def _centre_samples(comp, point, active):
    """Independent of the monitor: the samples of ``comp`` whose staggered
    coordinate (layout/yee.py MIN_COORD_FP) lies within half a cell of the
    centre ``point + 1/2`` along every axis, x outermost."""
    per_axis = []
    for a in range(3):
        if a not in active:
            per_axis.append([0])
            continue
        near = [i for i in range(point[a] - 2, point[a] + 3)
                if abs(i + MIN_COORD_FP[comp][a] - (point[a] + 0.5)) <= 0.5]
        per_axis.append(near)
    return [(i, j, k) for i in per_axis[0] for j in per_axis[1] for k in per_axis[2]]


@pytest.mark.parametrize("name", ["3d", "tmz", "tez", "1d"])
def test_centre_series_is_the_mean(name):
    kw, _ = GRIDS[name]
    dim = {"3d": 3, "tmz": 2, "tez": 2, "1d": 1}[name]
    points = [(1, 1, 1)[:dim], (6, 5, 7)[:dim], (11, 11, 11)[:dim]]
    s = make(SchemeConfig(time_steps=6, scene="vacuum", **kw))
    s.randomize_fields(seed=11)
    m = ProbeMonitor(s, points, position="centre", step=2)
    s.perform_steps()
    got = m.series().numpy()
    assert got.shape == (3, len(points), len(s.comps))
    counts = set()
    for pi, p in enumerate(points):
        p3 = tuple(p) + (0,) * (3 - dim)
        for ci, c in enumerate(s.comps):
            idx = _centre_samples(c, p3, s.layout.axes)
            counts.add(len(idx))
            f = s.F[0][c].numpy()
            acc = np.float64(f[idx[0]])
            for g in idx[1:]:
                acc = acc + np.float64(f[g])
            want = acc if len(idx) == 1 else acc * np.float64(1.0 / len(idx))
            assert got[-1, pi, ci] == want, (p, c, idx)
    # E components sit on one integer axis (2 samples), H on two (4) -- less the axes the scheme does not have
    assert counts == {"3d": {2, 4}, "tmz": {1, 2}, "tez": {2, 4}, "1d": {1, 2}}[name]
    # the slots themselves are the raw samples, in the stated order
    raw = m.raw()
    k = 0
    for p in points:
        p3 = tuple(p) + (0,) * (3 - dim)
        for c in s.comps:
            for g in _centre_samples(c, p3, s.layout.axes):
                assert m.slots[k] == (c, g) and float(raw[-1, k]) == float(s.F[0][c][g])
                k += 1
    assert k == len(m.slots)


# ------------------------------------------------------------------- spectrum
def test_spectrum_equals_dft_monitor():
    """The DFT monitor's wavelengths, step and start: both are fp64 sums of N
    <= 200 identical terms that differ in twiddle rounding and summation
    order only, ~N 2^-53 = 2e-14 of the scale; the bound leaves 50x."""
    cfg = SchemeConfig(scheme="3d", size=(16, 16, 16), time_steps=200, scene="vacuum", source="gaussian",
                       gaussian_width=10.0, gaussian_delay=40.0)
    s = make(cfg)
    wl = [0.02, 0.031]
    dft = DftMonitor(s, monitor_box_requests(s, (2, 2, 2)), wl, step=2, start=3)
    points = [(7, 8, 9), (2, 2, 2), (13, 13, 13), (8, 8, 7)]
    m = ProbeMonitor(s, points, step=2, start=3)
    s.perform_steps()
    assert m.samples == dft.samples == 99
    spec = m.spectrum(wl)
    assert spec.shape == (2, 4, 6) and spec.dtype == torch.complex128
    worst = 0.0
    for k in range(2):
        for kind in "EH":
            cols = [i for i, c in enumerate(m.comps) if c[0] == kind]
            scale = float(spec[k][:, cols].abs().max())
            assert scale > 0
            for ci in cols:
                ph = dft.phasor(m.comps[ci], k)
                for pi, p in enumerate(points):
                    want = complex(ph[p[0] - 2, p[1] - 2, p[2] - 2])
                    err = abs(complex(spec[k, pi, ci]) - want)
                    worst = max(worst, err / scale)
                    assert err <= 1e-12 * scale, (k, m.comps[ci], p, err, scale)
    print("largest difference to DftMonitor.phasor: %.3g of the scale" % worst)
    # any number of wavelengths
    assert m.spectrum(band_wavelengths(40, "0.015,0.06")).shape == (40, 4, 6)


def test_normalised_spectrum_is_flat_in_1d():
    """A Gaussian hard source on a 1D vacuum line, one probe 5 cells away,
    every step sampled, the run over before the line's ends can answer.

    The source node holds g(n) exactly and the line is linear and lossless,
    so the probe's Ez is g filtered by exp(-i k~ d) with k~ from the 1D
    dispersion relation sin(w dt / 2) = S sin(k~ dx / 2): below the cut-off
    (sin(w dt / 2) <= S) k~ is real and the modulus of the normalised
    spectrum is 1 at every frequency.  Hy obeys the same relation with the
    impedance dt / (mu0 dx) * sin(k~ dx / 2) / sin(w dt / 2) = 1 / eta0
    exactly, and its mean over the two samples around the cell centre
    multiplies that by cos(k~ dx / 2).  The bound on the flatness of both is
    therefore 1 - cos(k~ dx / 2) at the short-wavelength edge of the band:
    the largest effect numerical dispersion has on any of the moduli."""
    n, src, d = 400, 200, 5
    cfg = SchemeConfig(scheme="1d", size=(n, 1, 1), time_steps=300, scene="vacuum", source="gaussian",
                       gaussian_width=15.0, gaussian_delay=60.0)
    s = make(cfg)
    assert s.point_source[2] == (src, 0, 0) and cfg.time_steps * cfg.courant < (n - src - d) + (n - src)
    node = ProbeMonitor(s, [(src + d,)], ["Ez"], step=1)
    cen = ProbeMonitor(s, [(src + d,)], position="centre", step=1)
    s.perform_steps()
    # a band inside the pulse spectrum: |G| = exp(-(w width dt)^2 / 4) >= exp(-2.25) of its peak at 16 cells a wave
    wl = band_wavelengths(25, "%r,%r" % (16 * s.dx, 60 * s.dx))
    assert len(wl) == 25 and abs(wl[0] - 60 * s.dx) < 1e-12 and abs(wl[-1] - 16 * s.dx) < 1e-12
    w_edge = 2 * math.pi * SPEED_OF_LIGHT / min(wl)
    half_k = math.asin(math.sin(w_edge * s.dt / 2) / cfg.courant)
    bound = 1 - math.cos(half_k)
    assert 0 < bound < 0.03
    ez = node.spectrum(wl, normalise=True)[:, 0, 0].abs()
    both = cen.spectrum(wl, normalise=True)[:, 0].abs()
    hy = both[:, cen.comps.index("Hy")] * ETA0
    assert torch.equal(both[:, cen.comps.index("Ez")], ez)  # Ez sits at the cell centre in 1D
    for name, a in (("Ez", ez), ("eta0 Hy", hy)):
        print("%s: |normalised spectrum| in [%.9f, %.9f], bound on the spread %.4f" % (name, a.min(), a.max(), bound))
        assert float(a.max()) - float(a.min()) <= bound and abs(float(a.mean()) - 1) <= bound, name
    # not normalised it is the pulse's spectrum: far from flat over the same band
    raw = node.spectrum(wl)[:, 0, 0].abs()
    assert float(raw.max()) > 5 * float(raw.min())


# ---------------------------------------------------------------- decomposition
PAR = SchemeConfig(scheme="3d", size=(16, 16, 12), time_steps=12, scene="vacuum")
PAR_POINTS = [(3, 4, 5), (7, 6, 5), (8, 6, 5), (12, 12, 9), (6, 7, 4), (6, 8, 4), (8, 8, 6), (15, 15, 11)]


@pytest.mark.parametrize("topo", [(2, 1, 1), (2, 2, 1)], ids=["2x1x1", "2x2x1"])
def test_decomposed_equals_serial(topo):
    """Thread ranks: probes in the interior and on both sides of the rank
    borders (x = 8, y = 8), the centre means of the cells on the high side
    straddle them -- the serial series bit for bit on rank 0, None elsewhere."""
    ser = make(PAR)
    mons = [ProbeMonitor(ser, PAR_POINTS, position=pos, step=1) for pos in ("node", "centre")]
    ser.perform_steps()
    want = [m.series() for m in mons]
    assert all(float(w[-1].abs().max()) > 0 for w in want)
    world = topo[0] * topo[1] * topo[2]
    core = ParallelGridCore.create(PAR.size, world, "xy", requested=topo, optimal=False)
    hub = LocalHub(world, tagless=True)
    out, errors, owned = [None] * world, [], [None] * world

    def body(rank):
        try:
            dom = core.domain(rank, 1)
            halo = HaloExchanger(dom, comm=hub.comm(rank), mode="direct")
            s = make(PAR, dom, halo)
            ms = [ProbeMonitor(s, PAR_POINTS, position=pos, step=1) for pos in ("node", "centre")]
            s.perform_steps()
            halo.drain(s)
            owned[rank] = [list(m.mine) for m in ms]
            out[rank] = [m.series() for m in ms]
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
    for r in range(1, world):
        assert out[r] == [None, None]
    for got, w in zip(out[0], want):
        assert got.shape == w.shape and torch.equal(got, w)
    for i in range(2):
        # every slot is recorded by exactly one rank, and more than one rank records some
        cols = sorted(c for r in range(world) for c in owned[r][i])
        assert cols == list(range(len(cols))) and sum(1 for r in range(world) if owned[r][i]) == world
    # some centre mean (Ex at cell (8, 6, 5): samples x = 7 and 8) adds slots of rank 0 and of another rank
    assert any(0 < len(set(owned[0][1]) & set(g)) < len(g) for per in mons[1].groups for g in per)


# -------------------------------------------------------------- blocked passes
def _count_passes(s):
    n = [0]
    inner = s._tb_step

    def counted(T):
        n[0] += 1
        return inner(T)

    s._tb_step = counted
    return n


def test_blocked_passes_are_not_cut():
    cfg = SchemeConfig(scheme="3d", size=(16, 16, 16), time_steps=22, scene="vacuum", use_fused=True, time_block=4)
    a, b = make(cfg), make(cfg)
    assert a.tb == b.tb == 4
    m = ProbeMonitor(b, [(8, 8, 8), (5, 9, 7)])
    assert m.step == auto_step(b) == 4
    na, nb = _count_passes(a), _count_passes(b)
    a.perform_steps()
    b.perform_steps()
    assert na[0] == nb[0] == 6 and m.steps == [4, 8, 12, 16, 20]
    for c in a.comps:
        assert torch.equal(a.F[0][c], b.F[0][c]), c
    assert float(m.series().abs().max()) > 0


def test_auto_step_follows_the_other_monitors():
    s = make(SchemeConfig(scheme="3d", size=(16, 16, 16), time_steps=10, scene="vacuum"))
    assert auto_step(s) == 1
    s.tb = 5
    assert auto_step(s) == 5
    DftMonitor(s, monitor_box_requests(s, (4, 4, 4)), [0.02], step=6)
    assert auto_step(s) == 6
    EnergyMonitor(s, (0, 0, 0), step=8)
    m = ProbeMonitor(s, [(8, 8, 8)], start=5)
    assert (m.step, m.start) == (24, 5) and s.periodic[-1][:2] == (24, 5)


# -------------------------------------------------------------------- refusals
def test_refusals():
    base = dict(scheme="3d", size=(12, 12, 12), time_steps=8, scene="vacuum")

    def mon(points=((6, 6, 6),), position="node", comps=None, **kw):
        return ProbeMonitor(make(SchemeConfig(**dict(base, **kw))), points, comps, position, step=2)

    assert mon().samples == 0
    with pytest.raises(FdtdError, match="real-valued"):
        mon(complex_values=True)
    with pytest.raises(FdtdError, match="amplitude"):
        mon(use_amp_mode=True)
    for bad in ((12, 6, 6), (6, -1, 6), (6, 6, 12)):
        with pytest.raises(FdtdError, match="outside the grid"):
            mon(points=[(6, 6, 6), bad])
    assert mon(points=[(0, 0, 0), (11, 11, 11)]).slots[0] == ("Ex", (0, 0, 0))
    for bad in ((0, 6, 6), (6, 0, 6), (6, 6, 0)):
        with pytest.raises(FdtdError, match="reach outside"):
            mon(points=[bad], position="centre")
    assert len(mon(points=[(1, 1, 1), (11, 11, 11)], position="centre").slots) == 2 * (3 * 2 + 3 * 4)
    with pytest.raises(FdtdError, match="no component"):
        mon(comps=["Ez", "Bx"])
    with pytest.raises(FdtdError, match="position"):
        mon(position="face")
    with pytest.raises(FdtdError, match="indices a point"):
        mon(points=[(6, 6)])
    with pytest.raises(FdtdError, match="at least one point"):
        mon(points=[])
    # through the configuration: checkpoints, and what the options must give
    cfg = SchemeConfig(use_probes=True, probe_points="6,6,6", **base)
    assert probes_from_config(make(SchemeConfig(**base))) is None
    assert probes_from_config(make(cfg)).points == [(6, 6, 6)]
    with pytest.raises(FdtdError, match="checkpoint"):
        probes_from_config(make(cfg), checkpoints=True)
    with pytest.raises(FdtdError, match="--complex-field-values"):
        probes_from_config(make(dataclasses.replace(cfg, complex_values=True)))
    with pytest.raises(FdtdError, match="--use-amp-mode"):
        probes_from_config(make(dataclasses.replace(cfg, use_amp_mode=True)))
    with pytest.raises(FdtdError, match="needs points"):
        probes_from_config(make(dataclasses.replace(cfg, probe_points="")))
    with pytest.raises(FdtdError, match="--probe-band"):
        probes_from_config(make(dataclasses.replace(cfg, probe_spectrum=4)))
    with pytest.raises(FdtdError, match="indices a point"):
        probes_from_config(make(dataclasses.replace(cfg, probe_points="6,6")))


# --------------------------------------------------------------------- options
PROBE_ARGV = ["--use-probes", "--probe-points", "3,4,5;6,6,6", "--probe-file", "pts.txt", "--probe-components", "Ez,Hy",
              "--probe-position", "centre", "--probe-step", "6", "--probe-start", "2", "--probe-spectrum", "16",
              "--probe-band", "0.01,0.04"]


def test_options_round_trip():
    s = Settings()
    assert s.set_from_cmd(PROBE_ARGV, out=io.StringIO()) == 0
    s.validate()
    cfg = SchemeConfig.from_settings(s)
    assert cfg.use_probes and (cfg.probe_points, cfg.probe_file) == ("3,4,5;6,6,6", "pts.txt")
    assert (cfg.probe_components, cfg.probe_position, cfg.probe_step, cfg.probe_start) == ("Ez,Hy", "centre", 6, 2)
    assert (cfg.probe_spectrum, cfg.probe_band) == (16, "0.01,0.04")
    d = SchemeConfig.from_settings(Settings())
    assert not d.use_probes and (d.probe_points, d.probe_position, d.probe_step, d.probe_spectrum) == ("", "node", 0, 0)
    bad = Settings()
    bad.set_from_cmd(["--probe-position", "edge"], out=io.StringIO())
    with pytest.raises(Exception, match="--probe-position"):
        bad.validate()


def test_native_parser_agrees():
    st, nat = native.parse_settings(PROBE_ARGV)
    s = Settings()
    assert s.set_from_cmd(PROBE_ARGV, out=io.StringIO()) == 0 and st == 0, nat
    for k, v in s.as_dict().items():
        assert nat[k] == v, k
    assert nat["doUseProbes"] is True and nat["probePoints"] == "3,4,5;6,6,6" and nat["probeSpectrum"] == 16


def test_native_driver_refuses():
    exe = native.executable()
    assert os.path.exists(exe), "fdtd3d executable not built"
    r = subprocess.run([exe, "--3d", "--use-probes", "--probe-points", "5,5,5"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--use-probes" in r.stderr and "python -m fdtd3d_amd" in r.stderr


# ---------------------------------------------------------------------- driver
RUN_ARGV = ["--3d", "--sizex", "24", "--same-size", "--time-steps", "160", "--backend", "torch", "--device", "cpu",
            "--dtype", "f64", "--scene", "vacuum", "--use-pml", "--pml-type", "cpml", "--pml-sizex", "5",
            "--same-size-pml", "--use-tfsf", "--tfsf-sizex", "8", "--same-size-tfsf", "--source", "gaussian",
            "--gaussian-width", "8", "--gaussian-delay", "30", "--json"]


def test_driver_json_tables_and_stop(tmp_path):
    """--use-probes through the driver: the "probes" object of the JSON line,
    the per-point tables of --save-res, the points of --probe-file, and a
    series that ends at the step --stop-decay-by stops the run at."""
    from fdtd3d_amd.runner import run
    pts = tmp_path / "pts.txt"
    pts.write_text("# receivers\n12 12 12\n\n9, 14, 11  # behind the centre\n")
    out = io.StringIO()
    argv = RUN_ARGV + ["--use-probes", "--probe-points", "10,10,10", "--probe-file", str(pts), "--probe-position",
                       "centre", "--probe-components", "Ez,Hy", "--probe-spectrum", "5", "--probe-band", "0.012,0.03",
                       "--energy-step", "8", "--stop-decay-by", "1e-3", "--save-res", "--save-as-txt", "--save-Ez-only",
                       "--output-dir", str(tmp_path)]
    assert run(argv, out=out) == 0, out.getvalue()
    lines = out.getvalue().splitlines()
    rec = json.loads(lines[-1])
    T = rec["energy"]["stopped_at"]
    assert T is not None and T < 160 and rec["steps"] == T
    pr = rec["probes"]
    assert set(pr) == {"points", "components", "position", "step", "start", "samples", "spectrum"}
    assert pr["points"] == [[10, 10, 10], [12, 12, 12], [9, 14, 11]] and pr["components"] == ["Ez", "Hy"]
    assert (pr["position"], pr["step"], pr["start"], pr["samples"]) == ("centre", 8, 0, T // 8)  # the energy step
    sp = pr["spectrum"]
    assert len(sp["wavelengths"]) == 5 and sp["normalised"] is True
    assert np.asarray(sp["re"]).shape == np.asarray(sp["im"]).shape == (5, 3, 2)
    assert np.abs(np.asarray(sp["re"])).max() > 0
    assert [ln for ln in lines if ln.startswith("=== probes t=%d: 3 points x 2 components (centre), " % T)]
    for p, point in enumerate(pr["points"]):
        path = tmp_path / ("probe%d_[timestep=%d].txt" % (p, T))
        rows = path.read_text().splitlines()
        assert rows[0] == "# point %d %d %d (centre): step t_E t_H Ez Hy" % tuple(point)
        assert len(rows) == 1 + T // 8
        last = rows[-1].split()
        assert len(last) == 5 and int(last[0]) == T and float(last[2]) > float(last[1]) > 0
    assert any(abs(float(r.split()[3])) > 0 for r in (tmp_path / ("probe0_[timestep=%d].txt" % T)).read_text()
               .splitlines()[1:])


@pytest.mark.parametrize("extra,word", [(["--complex-field-values"], "--complex-field-values"),
                                        (["--use-amp-mode"], "--use-amp-mode"),
                                        (["--checkpoint-dir", "ck"], "checkpoint"),
                                        (["--load-from-file", "ck"], "checkpoint"),
                                        (["--probe-points", "5,5,12"], "outside the grid"),
                                        (["--probe-points", "0,5,5", "--probe-position", "centre"], "reach outside"),
                                        (["--probe-file", "no-such-file"], "--probe-file")])
def test_driver_refusals(extra, word, tmp_path):
    from fdtd3d_amd.runner import run
    argv = ["--3d", "--sizex", "12", "--same-size", "--time-steps", "2", "--backend", "torch", "--device", "cpu",
            "--scene", "vacuum", "--use-probes", "--probe-points", "5,5,5", "--output-dir", str(tmp_path)] + extra
    out = io.StringIO()
    assert run(argv, out=out) == 1
    assert "ERROR: " in out.getvalue() and word in out.getvalue()
    assert not os.listdir(tmp_path)
