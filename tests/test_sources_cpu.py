"""Source lists (``--source-file`` / ``SchemeConfig(sources=[...])``) on the
CPU: the loader and its refusals, the ``source_inject`` oracle, equivalence
with the built-in point source, linearity, the static residue a zero-mean
pulse avoids, decomposed == serial, and the driver.  The GPU counterparts
(HIP kernel against this oracle, hybrid == stepped) are in
test_sources_gpu.py.
"""

import io
import json
import math
import os
import socket
import subprocess
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fdtd3d_amd import native
from fdtd3d_amd.layout.source_file import (MAX_CELLS, MAX_SIGNALS, Signal, SourceList, load_source_file,
                                           parse_sources, signal_value)
from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.source import SourceEntries
from fdtd3d_amd.parallel.halo import HaloExchanger, gather_field
from fdtd3d_amd.parallel.topology import ParallelGridCore
from fdtd3d_amd.utils.assertions import FdtdError
from fdtd3d_amd.utils.constants import PI, SPEED_OF_LIGHT

DOC = {"sources": [
    {"component": "Ez", "cell": [20, 20, 12], "kind": "soft", "amplitude": 1.0,
     "waveform": "pulse", "wavelength": 0.02, "width": 30, "delay": 120, "phase": 0},
    {"component": "Ez", "cell": [28, 20, 12], "length": 5, "amplitude": -0.5,
     "waveform": "sine", "phase": 90, "ramp": 40}]}


def cfg3(sources, **kw):
    base = dict(scheme="3d", size=(16, 16, 16), time_steps=20, scene="vacuum", dtype="f64", sources=sources)
    base.update(kw)
    return SchemeConfig(**base)


def run(cfg, backend="torch", device="cpu", steps=None):
    s = YeeScheme(cfg, make_ops(backend, None, device, torch.float32 if cfg.dtype == "f32" else torch.float64))
    s.init_scheme()
    s.init_grids()
    s.perform_steps(steps)
    return s


def fields(s):
    return {c: s.F[0][c].detach().cpu().clone() for c in s.comps}


# ------------------------------------------------------------------- 1. loader
def test_loader_example_and_merging(tmp_path):
    p = tmp_path / "src.json"
    p.write_text(json.dumps(DOC))
    items = load_source_file(str(p))
    sl = SourceList(SchemeConfig(scheme="3d", size=(48, 40, 40), sources=items))
    assert len(sl.entries) == 2 and len(sl.signals) == 2
    # the filament: 5 cells along z, the component's own axis
    assert [g for c, g, _, _, _ in sl.cells] == [(20, 20, 12)] + [(28, 20, 12 + k) for k in range(5)]
    assert sl.bbox() == ((20, 20, 12), (29, 21, 17))
    assert sl.info() == {"entries": 2, "cells": 6, "signals": 2, "soft": 2, "hard": 0}
    # defaults: soft, amplitude 1, --wavelength / --gaussian-width / --gaussian-delay / --source
    e = parse_sources([{"component": "Hx", "cell": [3, 3, 3], "waveform": "pulse"}], "3d", 0.04, 7.0, 9.0)[0]
    assert not e.hard and e.amplitude == 1.0 and e.signal == Signal("pulse", 0.04, 7.0, 9.0, 0.0, 0.0)
    assert parse_sources([{"component": "Ez", "cell": [3, 3]}], "tmz", 0.02, 30, 120, "gaussian")[0].signal.waveform \
        == "gaussian"
    # equal signals are one signal (parameters the waveform does not read do not tell them apart)
    same = [{"component": "Ez", "cell": [5, 5, 5], "waveform": "sine", "phase": 10, "width": 3},
            {"component": "Ex", "cell": [6, 5, 5], "waveform": "sine", "phase": 10, "width": 4, "amplitude": 2},
            {"component": "Ex", "cell": [7, 5, 5], "waveform": "sine", "phase": 11}]
    sl = SourceList(cfg3(same))
    assert len(sl.signals) == 2 and [c[3] for c in sl.cells] == [0, 0, 1]
    # a filament runs along the component's axis
    sl = SourceList(cfg3([{"component": "Ex", "cell": [4, 5, 5], "length": 3}]))
    assert [g for _, g, _, _, _ in sl.cells] == [(4, 5, 5), (5, 5, 5), (6, 5, 5)]


OK = {"component": "Ez", "cell": [8, 8, 8]}


@pytest.mark.parametrize("entry, kw, word", [
    (dict(OK, colour=1), {}, "unknown key"),
    (dict(OK, waveform="chirp"), {}, "unknown waveform"),
    (dict(OK, component="Hz"), dict(scheme="tmz", size=(16, 16, 1)), "no component"),
    (dict(OK, cell=[8, 8]), {}, "3 indices"),
    (dict(OK, cell=[0, 8, 8]), {}, "outside the range"),           # the PEC border of Ez along x
    (dict(OK, cell=[8, 8, 16]), {}, "outside the range"),
    (dict(OK, cell=[8, 8, 14], length=3), {}, "outside the range"),  # the filament's end
    (dict(OK, cell=[3, 8, 8]), dict(use_pml=True, pml_type="cpml", pml_size=(4, 4, 4)), "absorbing layer"),
    (dict(OK, cell=[8, 12, 8]), dict(use_pml=True, pml_type="cpml", pml_size=(4, 4, 4)), "absorbing layer"),
    (dict(OK, amplitude=float("nan")), {}, "finite"),
    (dict(OK, phase=float("inf")), {}, "finite"),
    (dict(OK, width=0), {}, "width must be > 0"),
    (dict(OK, wavelength=-1), {}, "wavelength must be > 0"),
    (dict(OK, length=0), {}, "length must be >= 1"),
    (dict(OK, component="Hx", length=2), {}, "length applies to E"),
    (dict(OK, cell=[8, 8], length=2), dict(scheme="tmz", size=(16, 16, 1)), "length applies to E"),
    (dict(OK, kind="firm"), {}, "soft or hard"),
    (dict(OK, cell=[8.5, 8, 8]), {}, "integer"),
    (OK, dict(scheme="1d", size=(16, 1, 1)), "1D"),
    (OK, dict(complex_values=True), "--complex-field-values"),
    (OK, dict(use_amp_mode=True), "--use-amp-mode"),
    (OK, dict(use_hip_graph=True), "--use-hip-graph"),
])
def test_loader_refusals(entry, kw, word):
    """Every refusal raises with its message, from SourceList and from the
    scheme's constructor alike -- before anything is allocated."""
    cfg = cfg3([entry], **kw)
    with pytest.raises(ValueError, match=word):
        SourceList(cfg)
    with pytest.raises(FdtdError, match=word):
        YeeScheme(cfg, make_ops("torch", None, "cpu", torch.float64))


def test_loader_limits_and_shared_cells(tmp_path):
    with pytest.raises(ValueError, match="hard entry"):
        SourceList(cfg3([dict(OK, kind="hard"), dict(OK, amplitude=2)]))
    with pytest.raises(ValueError, match="hard entry"):  # the filament reaches the hard cell
        SourceList(cfg3([dict(OK, cell=[8, 8, 6], length=4), dict(OK, kind="hard")]))
    SourceList(cfg3([OK, dict(OK, amplitude=2)]))  # soft entries may share
    many = [dict(OK, phase=float(k)) for k in range(MAX_SIGNALS + 1)]
    with pytest.raises(ValueError, match="distinct signals"):
        SourceList(cfg3(many))
    assert len(SourceList(cfg3(many[:MAX_SIGNALS])).signals) == MAX_SIGNALS
    n = 260
    rows = [{"component": "Ez", "cell": [1 + i, 5, 1], "length": n - 2} for i in range(MAX_CELLS // (n - 2) + 1)]
    with pytest.raises(ValueError, match="source cells"):
        SourceList(cfg3(rows, size=(n, 12, n)))
    # the file itself
    p = tmp_path / "s.json"
    for text, word in (("{nonsense", "not JSON"), ("[1]", "\"sources\" list"), ('{"sources": [], "more": 1}', "unknown"),
                       ('{"objects": []}', "unknown")):
        p.write_text(text)
        with pytest.raises(ValueError, match=word):
            load_source_file(str(p))
    with pytest.raises(ValueError, match="cannot read"):
        load_source_file(str(tmp_path / "missing.json"))
    p.write_text('{"sources": [{"component": "Ez", "cell": [8, 8, 8], "amplitude": NaN}]}')
    with pytest.raises(ValueError, match="finite"):
        SourceList(cfg3(load_source_file(str(p))))


def test_chain_cells_refused():
    """A cell advanced by the D/B chain: inside a dispersive box."""
    cfg = cfg3([dict(OK, cell=[24, 22, 20])], size=(48, 44, 40), use_metamaterials=True, scene="drude-sphere",
               sphere_radius=5, sphere_center=(24.0, 22.0, 20.0), hybrid_block=1, blocked_drude="off")
    s = YeeScheme(cfg, make_ops("torch", None, "cpu", torch.float64))
    s.init_scheme()
    with pytest.raises(FdtdError, match="D/B chain"):
        s.init_grids()


def test_signal_values():
    dt = 0.5 * 0.0005 / SPEED_OF_LIGHT
    f = SPEED_OF_LIGHT / 0.02
    s = Signal("sine", 0.02, 1.0, 0.0, 0.0, 0.0)
    assert signal_value(s, 7, dt) == math.sin(dt * 7 * 2 * PI * f)  # the built-in source's expression
    r = Signal("sine", 0.02, 1.0, 0.0, 90.0, 40.0)
    assert signal_value(r, 0, dt) == 0.0
    assert signal_value(r, 20, dt) == pytest.approx(0.5 * math.sin(dt * 20 * 2 * PI * f + PI / 2), rel=1e-14)
    assert signal_value(r, 40, dt) == math.sin(dt * 40 * 2 * PI * f + math.radians(90.0))
    g = Signal("gaussian", 1.0, 30.0, 120.0, 0.0, 0.0)
    assert signal_value(g, 100.5, dt) == math.exp(-((100.5 - 120.0) / 30.0) ** 2)
    p = Signal("pulse", 0.02, 30.0, 120.0, 0.0, 0.0)
    assert signal_value(p, 120, dt) == 0.0
    assert signal_value(p, 110, dt) == -signal_value(p, 130, dt)  # odd about the delay: zero mean
    assert abs(sum(signal_value(p, t, dt) for t in range(241))) < 1e-13


# -------------------------------------------------------------- 2. the oracle op
def test_oracle_op_arithmetic():
    ops = make_ops("torch", None, "cpu", torch.float32)
    g = torch.Generator().manual_seed(3)
    f = [torch.randn((5, 6, 8), generator=g, dtype=torch.float32) for _ in range(2)]
    before = [x.clone() for x in f]
    ent = SourceEntries()
    for x in f:
        ent.add_field(x)
    ent.add("E", 0, 0, 0.3, 0)
    ent.add("E", 0, 17, 1.5, 1)
    ent.add("E", 0, 17, -0.25, 0)
    ent.add("E", 0, 17, 3.0, 2)
    ent.add("E", 1, 239, 2.0, 1, hard=True)
    ent.add("H", 1, 5, 1.0, 0)
    vals = [0.1, -0.7, 1.0 / 3.0]
    ops.source_inject(ent, "E", vals)
    want = [x.clone() for x in before]
    want[0].view(-1)[0] = torch.tensor(float(before[0].view(-1)[0]) + 0.3 * 0.1, dtype=torch.float64).float()
    acc = float(before[0].view(-1)[17])
    for a, k in ((1.5, 1), (-0.25, 0), (3.0, 2)):
        acc = acc + a * vals[k]
    want[0].view(-1)[17] = torch.tensor(acc, dtype=torch.float64).float()
    want[1].view(-1)[239] = torch.tensor(2.0 * -0.7, dtype=torch.float64).float()
    assert all(torch.equal(a, b) for a, b in zip(f, want))  # the H entry's cell untouched by the E launch
    with pytest.raises(ValueError, match="signal"):
        ops.source_inject(ent, "E", vals[:2])
    with pytest.raises(ValueError, match="signal values"):
        ops.source_inject(ent, "E", [0.0] * 65)
    ent.add("H", 1, 240, 1.0, 0)
    with pytest.raises(ValueError, match="outside its array"):
        ops.source_inject(ent, "H", vals)
    assert all(torch.equal(a, b) for a, b in zip(f, want))


# ------------------------------------------ 3. equivalence with the built-in source
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("waveform", ["sine", "gaussian"])
def test_equals_builtin_point_source(dtype, waveform):
    kw = dict(dtype=dtype, source=waveform, gaussian_width=6.0, gaussian_delay=10.0, time_block=1, hybrid_block=1)
    ref = run(cfg3(None, **kw))
    assert ref.point_source is not None and ref.source_list is None
    got = run(cfg3([{"component": "Ez", "cell": [8, 8, 8], "kind": "hard", "waveform": waveform}], **kw))
    assert got.point_source is None and got.source_list is not None
    a, b = fields(ref), fields(got)
    assert float(a["Ez"].abs().max()) > 0
    for c in a:
        assert torch.equal(a[c], b[c]), c


# --------------------------------------------------------------- 4. hybrid == stepped
def test_hybrid_equals_stepped_oracle():
    """The hybrid plan of a run without any PML exists because of the source
    list, cuts the source box out of the core, and reproduces the stepped run
    (torch backend: the generic blocked oracle advances the core)."""
    src = [{"component": "Ez", "cell": [22, 20, 18], "length": 3, "waveform": "pulse", "width": 4, "delay": 8},
           {"component": "Hx", "cell": [25, 20, 19], "waveform": "pulse", "width": 4, "delay": 8, "amplitude": 0.01}]
    kw = dict(size=(48, 40, 40), time_steps=11)
    h = run(cfg3(src, hybrid_block=3, **kw))
    assert h.hybrid is not None and h.hybrid["T"] == 3 and h.hybrid["cut_cells"] > 0
    lo, hi = h.source_list.bbox()
    for b in h.hybrid["core"]:
        assert any(b[1][d] <= lo[d] - 4 or b[0][d] >= hi[d] + 4 for d in range(3)), b  # T + 1 clear
    s = run(cfg3(src, hybrid_block=1, **kw))
    assert s.hybrid is None
    a, b = fields(h), fields(s)
    assert float(a["Ez"].abs().max()) > 0
    for c in a:
        assert torch.equal(a[c], b[c]), c


# ------------------------------------------------------------ 5. a linear system
A = {"component": "Ez", "cell": [9, 10, 10], "waveform": "pulse", "width": 8, "delay": 20, "amplitude": 1.0}
B = {"component": "Hy", "cell": [12, 9, 10], "waveform": "sine", "ramp": 10, "phase": 30, "amplitude": 2e-3}
B2 = {"component": "Ez", "cell": [9, 10, 10], "waveform": "gaussian", "width": 6, "delay": 15, "amplitude": -0.5}
PHYS = dict(size=(20, 20, 20), time_steps=100, use_pml=True, pml_type="cpml", pml_size=(4, 4, 4))


def test_superposition_and_scaling():
    ab = fields(run(cfg3([A, B, B2], **PHYS)))
    a = fields(run(cfg3([A], **PHYS)))
    b = fields(run(cfg3([B, B2], **PHYS)))
    for kind in "EH":
        scale = max(float(ab[c].abs().max()) for c in ab if c[0] == kind)
        assert scale > 0
        for c in ab:
            if c[0] == kind:
                err = float((ab[c] - (a[c] + b[c])).abs().max())
                assert err <= 1e-11 * scale, (c, err, scale)
    for dtype in ("f64", "f32"):
        one = fields(run(cfg3([A, B, B2], dtype=dtype, **PHYS)))
        two = fields(run(cfg3([dict(e, amplitude=2 * e["amplitude"]) for e in (A, B, B2)], dtype=dtype, **PHYS)))
        for c in one:
            assert torch.equal(2 * one[c], two[c]), (dtype, c)


def test_pulse_leaves_no_static_residue():
    """A soft gaussian deposits a static charge (sum(E) stays), a soft
    zero-mean pulse of the same envelope does not."""
    # envelope 48 steps wide, two carrier periods (12 cells per wavelength, Courant 0.5): the pulse's spectrum
    # at DC is exp(-(2 pi)^2) ~ 1e-17 of its peak, and the cut at tau = 0, 6.25 widths before the centre, 1e-17
    kw = dict(PHYS, time_steps=1000)
    res = {}
    for wf in ("pulse", "gaussian"):
        s = run(cfg3([{"component": "Ez", "cell": [10, 10, 10], "waveform": wf, "width": 48, "delay": 300,
                       "wavelength": 0.006}], **kw))
        res[wf] = abs(float(sum(s.F[0][c].sum() for c in s.e_comps)))
    print("sum(E) after 1000 steps:", res)
    assert res["gaussian"] > 1.0  # the integral of the envelope, sqrt(pi) * width, stays on the grid as charge
    # round-off: 2.4e4 samples x 1e3 steps of 1e-16 relative to fields of order 1 walk to ~1e-12
    assert res["pulse"] < 1e-10, res


# -------------------------------------------------------- 6. decomposed == serial
SEAM = [{"component": "Ez", "cell": [8, 8, 6], "waveform": "pulse", "width": 3, "delay": 5},       # on both seams
        {"component": "Ez", "cell": [7, 5, 6], "waveform": "sine", "amplitude": 0.5},               # a ghost of x-high
        {"component": "Ey", "cell": [10, 8, 4], "waveform": "sine", "kind": "hard", "phase": 45},  # two in a ghost
        {"component": "Hx", "cell": [9, 8, 5], "waveform": "gaussian", "width": 3, "delay": 4, "amplitude": 1e-3}]
SEAM_CFG = dict(size=(16, 16, 12), time_steps=10)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, cfg, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        core = ParallelGridCore.create(cfg.size, world, "xy", (2, 2, 1), optimal=False, active_axes=(0, 1, 2))
        dom = core.domain(rank, 3, align_z=1, align_axis=2)
        halo = HaloExchanger(dom)
        s = YeeScheme(cfg, make_ops("torch", None, "cpu", torch.float64), dom, halo)
        s.init_scheme()
        s.init_grids()
        assert s.hybrid is None and s.tb == 1 and dom.buffer_size == 3
        held = sum(len(r) for r in s._src_entries.rows.values())
        s.perform_steps()
        halo.drain(s)
        res = {c: gather_field(s, c, 0) for c in s.comps}
        counts = [None] * world
        dist.all_gather_object(counts, held)
        if rank == 0:
            res["held"] = torch.tensor(counts)
            res["topology"] = torch.tensor(core.topology)
            torch.save(res, os.path.join(outdir, "par.pt"))
    finally:
        dist.destroy_process_group()


def test_decomposed_equals_serial():
    cfg = cfg3(SEAM, **SEAM_CFG)
    ser = fields(run(cfg))
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(4, _free_port(), cfg, d), nprocs=4, join=True)
        par = torch.load(os.path.join(d, "par.pt"), weights_only=True)
    assert par["topology"].tolist() == [2, 2, 1]
    assert int(par["held"].sum()) > len(SEAM)  # seam cells are held by several ranks (ghost copies)
    assert float(ser["Hx"].abs().max()) > 0
    for c in ser:
        assert torch.equal(par[c], ser[c]), c


# ------------------------------------------------------------------- 7. the driver
ARGV = ["--3d", "--sizex", "20", "--same-size", "--time-steps", "60", "--backend", "torch", "--device", "cpu",
        "--dtype", "f64", "--scene", "vacuum", "--use-pml", "--pml-type", "cpml", "--pml-sizex", "4",
        "--same-size-pml", "--json"]


def test_driver_json_and_probes(tmp_path):
    from fdtd3d_amd.runner import run as drive
    p = tmp_path / "src.json"
    p.write_text(json.dumps({"sources": [dict(A, delay=10, width=4), dict(A, cell=[11, 10, 10], delay=10, width=4,
                                                                        kind="hard", component="Ex")]}))
    out = io.StringIO()
    argv = ARGV + ["--source-file", str(p), "--use-probes", "--probe-points", "12,10,10", "--probe-components", "Ez",
                   "--probe-step", "5", "--save-res", "--output-dir", str(tmp_path)]
    assert drive(argv, out=out) == 0, out.getvalue()
    rec = json.loads(out.getvalue().strip().splitlines()[-1])
    assert rec["sources"] == {"entries": 2, "cells": 2, "signals": 1, "soft": 1, "hard": 1}
    assert rec["probes"]["samples"] >= 12
    # the recorded series (the per-point table of --save-res: step, times, Ez) is not zero
    table = [ln.split() for ln in (tmp_path / "probe0_[timestep=60].txt").read_text().splitlines()[1:]]
    assert len(table) == rec["probes"]["samples"] and max(abs(float(row[-1])) for row in table) > 1e-6


def test_driver_refusals(tmp_path):
    from fdtd3d_amd.runner import run as drive
    p = tmp_path / "src.json"
    p.write_text(json.dumps({"sources": [dict(A), dict(B)]}))
    for extra, word in ((["--stop-decay-by", "0.01"], "sine entry"),
                        (["--checkpoint-dir", str(tmp_path)], "checkpoint"),
                        (["--use-hip-graph"], "--use-hip-graph"),
                        (["--complex-field-values"], "--complex-field-values")):
        out = io.StringIO()
        assert drive(ARGV + ["--source-file", str(p)] + extra, out=out) == 1, extra
        assert "ERROR: " in out.getvalue() and word in out.getvalue(), out.getvalue()
    out = io.StringIO()
    assert drive(ARGV + ["--source-file", str(tmp_path / "none.json")], out=out) == 1
    assert "--source-file" in out.getvalue() and "cannot read" in out.getvalue()
    # a pulsed list may stop on decay: the latest end of its entries
    from fdtd3d_amd.models.energy import source_end
    s = run(cfg3([dict(A, delay=20, width=4), dict(B2, delay=30, width=4)], **dict(PHYS, time_steps=1)))
    end = source_end(s, 200)
    assert end is not None and 30 < end < 60
    assert source_end(run(cfg3([dict(B)], **dict(PHYS, time_steps=1))), 200) is None


def test_native_driver_refuses(tmp_path):
    st, nat = native.parse_settings(["--3d", "--source-file", "x.json"])
    assert st == 0 and nat["sourceFile"] == "x.json"
    exe = native.executable()
    assert os.path.exists(exe), "fdtd3d executable not built"
    r = subprocess.run([exe, "--3d", "--source-file", str(tmp_path / "x.json")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--source-file" in r.stderr and "python -m fdtd3d_amd" in r.stderr
