"""The cases of test_decomposed_gpu.py (tests/decomposed_cases.py) on the
torch fp64 backend, CPU thread ranks of the same runner: the oracle itself
stays inside every bound on ranks -- bit-equal where the features' own CPU
tests assert bit equality --, the boxes and objects straddle the cuts, the
empty-entry counts and the mix of lane and non-lane rows are as claimed, and
per monitor family a control: with one rank's contribution zeroed the
comparison fails."""
import pytest
import torch

import decomposed_cases as dc
from rank_threads import rank_domains, run_ranks

DTYPES = ["f32", "f64"]


def _ranks(cfg, topo, buf, **kw):
    return run_ranks(cfg, topo, buf, "torch", "cpu", **kw)


# ------------------------------------------------------------------- geometry
def test_lane_mix():
    """Over the DFT cases some rank's rows are whole 16-byte lanes and some
    are not, in both precisions; the z split of 18 leaves ranks an odd owned
    nz; the lossy ranks run both instances of the kernel."""
    geos = [dc.geometry(c) for c in dc.DFT_CASES.values()]
    for dtype in DTYPES:
        assert dc.lane_mix(geos, dtype) == {True, False}, dtype
        seen = {dc.expected_lossy_lanes(d.shape, dtype) for topo in dc.LOSSY_TOPOS.values()
                for d in rank_domains(dc.LOSSY["size"], topo, dc.LOSSY_BUF)[1]}
        assert seen == {1, 4 if dtype == "f32" else 2}
    rows = {name: sorted({d.shape[2] for d in rank_domains(*dc.geometry(c))[1]}) for name, c in dc.DFT_CASES.items()}
    assert rows == {"2x1x2": [10], "1x2x1": [18], "2x1x2-deep": [12], "1x2x2-odd": [9], "blocked": [96]}
    _, doms = rank_domains(dc.STEPPED.size, (2, 1, 2), 1)
    assert all(d.owned_shape[2] == 9 for d in doms)
    # ghost planes in front of the owned cells, and a non-zero origin, on some rank of every case
    for c in dc.DFT_CASES.values():
        doms = rank_domains(*dc.geometry(c))[1]
        assert any(max(d.ghost_lo) > 0 and max(d.origin) > 0 for d in doms)
    for name, (cfg, req, _, _, topo, _, _) in dc.DFT_CASES.items():
        dc.dft_straddles(req, cfg.size, topo)
    for topo, _ in dc.SCENE_CASES.values():
        dc.objects_straddle(dc.scene_objects(), dc.SCENE_SIZE, topo)


# ---------------------------------------------------------------- scene grids
@pytest.mark.parametrize("smoothing", ["linear", "none"])
@pytest.mark.parametrize("name", sorted(dc.SCENE_CASES))
def test_scene_grids(name, smoothing):
    topo, buf = dc.SCENE_CASES[name]
    cfg = dc.scene_cfg(smoothing, "f64")
    ranks = _ranks(cfg, topo, buf, collect=dc.scene_collect, steps=False)
    ser, _ = dc.oracle(("scene", smoothing), cfg, steps=False)
    assert any(min(r["origin"]) == 0 for r in ranks) and any(max(r["origin"]) > 0 for r in ranks)
    assert all(r["lossy"] == ser.lossy["gbox"] for r in ranks)
    dc.scene_compare(ranks, ser)
    # control: a grid sampled from the wrong origin is caught
    label = "eps at Ez"
    got, want = ranks[-1]["grids"][label]
    ranks[-1]["grids"][label] = (torch.roll(got, 1, dims=0), want)
    with pytest.raises(AssertionError):
        dc.scene_compare(ranks, ser)


# ---------------------------------------------------------------- lossy media
@pytest.mark.parametrize("name", sorted(dc.LOSSY_TOPOS))
def test_lossy_ranks(name):
    topo = dc.LOSSY_TOPOS[name]
    cfg = dc.lossy_cfg("f64")
    ranks = _ranks(cfg, topo, dc.LOSSY_BUF, collect=dc.lossy_collect)
    ref, _ = dc.oracle("lossy", cfg)
    gbox = ref.lossy["gbox"]
    assert all(gbox[0][a] < cfg.size[a] // 2 < gbox[1][a] for a in range(3) if topo[a] > 1), "the box straddles the cut"
    assert all(r["gbox"] == gbox and r["coefs"] and r["stepped"] for r in ranks)
    want = dc.serial_fields(ref)
    got = dc.gathered_fields(ranks, cfg.size)
    assert float(want["Hx"].abs().max()) > 0
    for c in want:
        assert torch.equal(got[c], want[c]), c  # tests/test_lossy_cpu.py::test_decomposed_equals_serial
    assert dc.field_errors(got, want) <= dc.LOSSY_TOL["f64"]
    ranks[-1]["own"] = {c: torch.zeros_like(v) for c, v in ranks[-1]["own"].items()}
    assert dc.field_errors(dc.gathered_fields(ranks, cfg.size), want) > dc.LOSSY_TOL["f32"]


# ---------------------------------------------------------------- Drude scene
def test_drude_scene_ranks():
    cfg = dc.DRUDE
    ranks = _ranks(cfg, dc.DRUDE_TOPO, dc.DRUDE_BUF, collect=dc.drude_collect, align_z=dc.DRUDE_ALIGN)
    ser, _ = dc.serial(cfg, "torch", "cpu")
    want = dc.serial_fields(ser)
    got = dc.gathered_fields(ranks, cfg.size)
    assert float(want["Ez"].abs().max()) > 0
    for c in want:
        assert torch.equal(got[c], want[c]), c  # tests/test_scene_drude_cpu.py::test_decomposed_equals_serial
    dc.drude_tables_agree(ranks, ser)
    # the stepped oracle of the GPU test against these hybrid passes: inside the fp64 bound
    ref, _ = dc.oracle("drude", cfg)
    hybrid = ranks[0]["hybrid"]
    assert dc.field_errors(got, dc.serial_fields(ref)) <= dc.DRUDE_TOL[hybrid]["f64"]
    # control: another rank's coefficients in place of a rank's own
    ranks[0]["cells"], ranks[3]["cells"] = ranks[3]["cells"], ranks[0]["cells"]
    with pytest.raises(AssertionError):
        dc.drude_tables_agree(ranks, ser)


# ------------------------------------------------------------------------ DFT
@pytest.mark.parametrize("name", sorted(dc.DFT_CASES))
def test_dft_ranks(name):
    cfg, req, step, start, topo, buf, align = dc.DFT_CASES[name]
    world = topo[0] * topo[1] * topo[2]
    ranks = _ranks(cfg, topo, buf, setup=dc.dft_setup(req, step, start), collect=dc.dft_collect, align_z=align)
    key = "blocked" if name == "blocked" else "odd" if name.endswith("odd") else "stepped"
    _, rmon = dc.oracle(("dft", key), cfg, dc.dft_setup(req, step, start))
    assert all(r["t"] == cfg.time_steps and r["tb"] == max(1, cfg.time_block) for r in ranks)
    # stepped ranks: the bits of tests/test_dft_cpu.py::test_decomposed_accumulators_equal_serial
    worst, empties = dc.dft_compare(ranks, rmon, req, "f64", dc.DFT_TOL["f64"], exact=name != "blocked")
    assert empties == [world - 1, 0, 0]
    assert worst <= dc.SERIAL_TOL
    # control: the last rank's accumulators zeroed
    for row in ranks[-1]["rows"]:
        row["owned"].zero_()
    with pytest.raises(AssertionError):
        dc.dft_compare(ranks, rmon, req, "f64", dc.DFT_TOL["f32"])


# ------------------------------------------------------------ flux / far field
@pytest.mark.parametrize("name", sorted(dc.SURFACE_TOPOS))
def test_surface_ranks(name):
    topo = dc.SURFACE_TOPOS[name]
    cfg = dc.STEPPED
    ranks = _ranks(cfg, topo, 1, setup=dc.surface_setup, collect=dc.surface_collect())
    _, (rflux, rfar) = dc.oracle("surface", cfg, dc.surface_setup)
    want = dc.surface_results(rflux, rfar)
    assert sum(1 for r in ranks if r["nonempty"]) == len(ranks) and ranks[0]["nonempty"] < 24
    # tests/test_flux_cpu.py: 1e-13 of each face power; tests/test_farfield_cpu.py: the same bits
    assert float(((ranks[0]["power"] - want[1]).abs() / want[1].abs()).max()) <= 1e-13
    assert torch.equal(ranks[0]["u"], want[2]) and torch.equal(ranks[0]["total"], want[3])
    assert dc.surface_compare(ranks, want, dc.SURFACE_TOL["f64"]) <= dc.SERIAL_TOL
    # control: the last rank's accumulators zeroed before rank 0 evaluates
    zeroed = _ranks(cfg, topo, 1, setup=dc.surface_setup, collect=dc.surface_collect(zero_rank=len(ranks) - 1))
    with pytest.raises(AssertionError):
        dc.surface_compare(zeroed, want, dc.SURFACE_TOL["f32"])


# --------------------------------------------------------------------- probes
@pytest.mark.parametrize("name", sorted(dc.PROBE_TOPOS))
def test_probe_ranks(name):
    topo = dc.PROBE_TOPOS[name]
    cfg = dc.PROBE_CFG
    ranks = _ranks(cfg, topo, 1, setup=dc.probe_setup, collect=dc.probe_collect())
    _, rmons = dc.oracle("probe", cfg, dc.probe_setup)
    want = [m.series() for m in rmons]
    assert all(float(w[-1].abs().max()) > 0 for w in want)
    dc.probe_ownership(ranks, [m.groups for m in rmons])
    # tests/test_probe_cpu.py::test_decomposed_equals_serial: the serial series bit for bit
    assert dc.probe_compare(ranks, rmons, want, dc.PROBE_TOL["f64"], exact=True) == 0.0
    # control: the last rank's samples zeroed before rank 0 collects them
    zeroed = _ranks(cfg, topo, 1, setup=dc.probe_setup, collect=dc.probe_collect(zero_rank=len(ranks) - 1))
    with pytest.raises(AssertionError):
        dc.probe_compare(zeroed, rmons, want, dc.PROBE_TOL["f32"])
