"""The monitors, scene files and lossy media on decomposed HIP ranks (thread
ranks on one GPU, tests/rank_threads.py): the host code that turns a rank's
local geometry -- a non-zero origin, ghost planes in front of the owned cells,
rows that are or are not whole 16-byte lanes -- into device tables and launch
arguments.  Every case against the serial fp64 torch CPU run of the same
configuration at the bound of the feature's own serial GPU test, fp64 also
against the serial HIP run at 1e-12 of scale; the cases themselves:
tests/decomposed_cases.py, on the torch backend: test_decomposed_cpu.py."""
import dataclasses

import pytest

import decomposed_cases as dc
from rank_threads import run_ranks

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64"]


def _ranks(gpu, cfg, topo, buf, **kw):
    return run_ranks(cfg, topo, buf, "hip", gpu, **kw)


# ---------------------------------------------------------------- scene grids
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("smoothing", ["linear", "none"])
@pytest.mark.parametrize("name", sorted(dc.SCENE_CASES))
def test_scene_grids(gpu, name, smoothing, dtype):
    """``init_grids`` only.  Every material grid a rank's sampler makes with
    ``scene_sample`` on the device is, bit for bit, the torch oracle's with
    that rank's origin and shape and the window of the serial grid, one launch
    per component and quantity; the stencils of the outer ranks reach to
    negative and beyond-grid coordinates."""
    topo, buf = dc.SCENE_CASES[name]
    cfg = dc.scene_cfg(smoothing, dtype)
    dc.objects_straddle(cfg.scene_objects, cfg.size, topo)
    ranks = _ranks(gpu, cfg, topo, buf, collect=dc.scene_collect, steps=False)
    ser, _ = dc.oracle(("scene", smoothing), cfg, steps=False)
    assert any(min(r["origin"]) == 0 for r in ranks) and any(max(r["origin"]) > 0 for r in ranks)
    assert all(r["launches"] for r in ranks)
    assert all(r["lossy"] == ser.lossy["gbox"] for r in ranks)
    dc.scene_compare(ranks, ser)
    print("scene grids %s %s %s: %d grids on %d ranks, all bit-equal" % (name, smoothing, dtype,
                                                                        len(ranks[0]["grids"]), len(ranks)))


# ---------------------------------------------------------------- lossy media
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(dc.LOSSY_TOPOS))
def test_lossy_ranks(gpu, name, dtype):
    """The conductive E update on ranks with 3-deep ghosts: one lossy box on
    every rank, across the cuts; the instance (16-byte lanes on 2 x 1 x 1,
    whose rows are 12 cells; one cell on 1 x 2 x 2, whose rows are 9) from the
    ranks' array shapes; the gathered fields."""
    topo = dc.LOSSY_TOPOS[name]
    cfg = dc.lossy_cfg(dtype)
    ranks = _ranks(gpu, cfg, topo, dc.LOSSY_BUF, collect=dc.lossy_collect)
    ref, _ = dc.oracle("lossy", cfg)
    gbox = ref.lossy["gbox"]
    assert all(gbox[0][a] < cfg.size[a] // 2 < gbox[1][a] for a in range(3) if topo[a] > 1), "the box straddles the cut"
    assert all(r["gbox"] == gbox and r["coefs"] and r["stepped"] for r in ranks)
    lanes = {r["lanes"] for r in ranks}
    assert all(r["lanes"] == dc.expected_lossy_lanes(r["shape"], dtype) for r in ranks), lanes
    assert lanes == ({1} if name == "1x2x2" else {4 if dtype == "f32" else 2})
    want = dc.serial_fields(ref)
    assert float(want["Hx"].abs().max()) > 0
    got = dc.gathered_fields(ranks, cfg.size)
    worst = dc.field_errors(got, want)
    dc.report("lossy %s %s vs oracle" % (name, dtype), worst, dc.LOSSY_TOL[dtype])
    assert worst <= dc.LOSSY_TOL[dtype]
    if dtype == "f64":
        ser, _ = dc.serial(cfg, "hip", gpu)
        worst = dc.field_errors(got, dc.serial_fields(ser))
        dc.report("lossy %s f64 vs serial HIP" % name, worst, dc.SERIAL_TOL)
        assert worst <= dc.SERIAL_TOL


def test_lossy_instances_both_occur():
    """Over the parametrisation of test_lossy_ranks both instances run."""
    for dtype in DTYPES:
        seen = {dc.expected_lossy_lanes(d.shape, dtype) for topo in dc.LOSSY_TOPOS.values()
                for d in dc.rank_domains(dc.LOSSY["size"], topo, dc.LOSSY_BUF)[1]}
        assert seen == {1, 4 if dtype == "f32" else 2}


# ---------------------------------------------------------------- Drude scene
@pytest.mark.parametrize("dtype", DTYPES)
def test_drude_scene_ranks(gpu, dtype):
    """A damped and magnetic Drude scene across the cuts of 2 x 2 x 1 ranks:
    the gathered fields, and the ranks' Drude coefficients (uint8 index +
    table, built per rank) against the serial run's on the owned cells."""
    cfg = dataclasses.replace(dc.DRUDE, dtype=dtype)
    ranks = _ranks(gpu, cfg, dc.DRUDE_TOPO, dc.DRUDE_BUF, collect=dc.drude_collect, align_z=dc.DRUDE_ALIGN)
    ref, _ = dc.oracle("drude", cfg)
    assert any("D1" in ref.upml[c] for c in ref.e_comps) and any("D1" in ref.upml[c] for c in ref.h_comps)
    hybrid = ranks[0]["hybrid"]
    assert all(r["hybrid"] == hybrid for r in ranks)
    tol = dc.DRUDE_TOL[hybrid][dtype]
    want = dc.serial_fields(ref)
    assert float(want["Ez"].abs().max()) > 0
    got = dc.gathered_fields(ranks, cfg.size)
    worst = dc.field_errors(got, want)
    dc.report("drude scene %s (%s passes) vs oracle" % (dtype, "hybrid" if hybrid else "stepped"), worst, tol)
    assert worst <= tol
    ser, _ = dc.serial(cfg, "hip", gpu)
    dc.drude_tables_agree(ranks, ser)
    if dtype == "f64":
        worst = dc.field_errors(got, dc.serial_fields(ser))
        dc.report("drude scene f64 vs serial HIP", worst, dc.SERIAL_TOL)
        assert worst <= dc.SERIAL_TOL


# ------------------------------------------------------------------------ DFT
def _dft_oracle(name):
    cfg, req, step, start = dc.DFT_CASES[name][:4]
    key = "blocked" if name == "blocked" else "odd" if name.endswith("odd") else "stepped"
    return dc.oracle(("dft", key), cfg, dc.dft_setup(req, step, start))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(dc.DFT_CASES))
def test_dft_ranks(gpu, name, dtype):
    """``_dft_table`` on ranks: boxes behind ghost planes, the vector flag
    from the rank's own rows, accumulators padded from an odd z, empty entries,
    and (``blocked``) the table cache over the F / F_alt pair between 4-step
    passes."""
    cfg, req, step, start, topo, buf, align = dc.DFT_CASES[name]
    cfg = dataclasses.replace(cfg, dtype=dtype)
    dc.dft_straddles(req, cfg.size, topo)
    world = topo[0] * topo[1] * topo[2]
    ranks = _ranks(gpu, cfg, topo, buf, setup=dc.dft_setup(req, step, start), collect=dc.dft_collect, align_z=align)
    ref, rmon = _dft_oracle(name)
    assert all(r["t"] == cfg.time_steps and r["tb"] == max(1, cfg.time_block) for r in ranks)
    for r in ranks:
        assert all(row["field_shape"] == r["shape"] for row in r["rows"])
    flags = {dc.whole_lanes(r["shape"], dtype) for r in ranks}
    assert flags == dc.lane_mix([dc.geometry(dc.DFT_CASES[name])], dtype)
    if name == "blocked":
        assert all(r["tables"] == 2 for r in ranks), "the passes did not alternate F and F_alt under the monitor"
    worst, empties = dc.dft_compare(ranks, rmon, req, dtype, dc.DFT_TOL[dtype])
    assert empties == [world - 1, 0, 0]
    dc.report("dft %s %s vs oracle" % (name, dtype), worst, dc.DFT_TOL[dtype])
    if dtype == "f64":
        ser, smon = dc.serial(cfg, "hip", gpu, dc.dft_setup(req, step, start))
        assert ser.tb == max(1, cfg.time_block)
        worst, _ = dc.dft_compare(ranks, smon, req, dtype, dc.SERIAL_TOL)
        dc.report("dft %s f64 vs serial HIP" % name, worst, dc.SERIAL_TOL)


def test_lane_mix():
    """Over the DFT cases some rank's rows are whole 16-byte lanes and some
    are not, in both precisions; a z split leaves ranks an odd owned nz."""
    geos = [dc.geometry(c) for c in dc.DFT_CASES.values()]
    for dtype in DTYPES:
        assert dc.lane_mix(geos, dtype) == {True, False}, dtype
    _, doms = dc.rank_domains(dc.STEPPED.size, (2, 1, 2), 1)
    assert all(d.owned_shape[2] == 9 for d in doms)


# ------------------------------------------------------------ flux / far field
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(dc.SURFACE_TOPOS))
def test_surface_ranks(gpu, name, dtype):
    """A flux and a far-field monitor over one DFT monitor: the accumulators
    gathered on rank 0 into padded blocks, ``_flux_table`` / ``_far_table``
    on them (1 x 1 x 2: the z-normal faces' aligned-group loads on blocks put
    together from two ranks), two launches per evaluation."""
    topo = dc.SURFACE_TOPOS[name]
    cfg = dataclasses.replace(dc.STEPPED, dtype=dtype)
    ranks = _ranks(gpu, cfg, topo, 1, setup=dc.surface_setup, collect=dc.surface_collect())
    _, (rflux, rfar) = dc.oracle("surface", cfg, dc.surface_setup)
    if "results" not in dc._cache:
        dc._cache["results"] = dc.surface_results(rflux, rfar)
    assert ranks[0]["launches"] == [2, 2, 2], "the monitors did not take the HIP ops"
    assert all(r["launches"] == [0, 0, 0] for r in ranks[1:])
    assert sum(1 for r in ranks if r["nonempty"]) == len(ranks) and ranks[0]["nonempty"] < 24
    worst = dc.surface_compare(ranks, dc._cache["results"], dc.SURFACE_TOL[dtype])
    dc.report("surface %s %s vs oracle" % (name, dtype), worst, dc.SURFACE_TOL[dtype])
    if dtype == "f64":
        _, (sflux, sfar) = dc.serial(cfg, "hip", gpu, dc.surface_setup)
        # (the 1e-12 is of the largest face power / the peak intensity, the scales of surface_compare)
        worst = dc.surface_compare(ranks, dc.surface_results(sflux, sfar), dc.SERIAL_TOL)
        dc.report("surface %s f64 vs serial HIP" % name, worst, dc.SERIAL_TOL)


# --------------------------------------------------------------------- probes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(dc.PROBE_TOPOS))
def test_probe_ranks(gpu, name, dtype):
    """``probe_sample`` from a table of the slots a rank owns: node and
    centre probes, centre means with samples on two ranks (across x = 8, y = 8
    on 2 x 2 x 1, across z = 6 on 1 x 1 x 2), every raw sample the rank's own
    field element."""
    topo = dc.PROBE_TOPOS[name]
    cfg = dataclasses.replace(dc.PROBE_CFG, dtype=dtype)
    ranks = _ranks(gpu, cfg, topo, 1, setup=dc.probe_setup, collect=dc.probe_collect())
    _, rmons = dc.oracle("probe", cfg, dc.probe_setup)
    if "probe series" not in dc._cache:
        dc._cache["probe series"] = [m.series() for m in rmons]
    dc.probe_ownership(ranks, [m.groups for m in rmons])
    worst = dc.probe_compare(ranks, rmons, dc._cache["probe series"], dc.PROBE_TOL[dtype])
    dc.report("probes %s %s vs oracle" % (name, dtype), worst, dc.PROBE_TOL[dtype])
    if dtype == "f64":
        _, smons = dc.serial(cfg, "hip", gpu, dc.probe_setup)
        worst = dc.probe_compare(ranks, smons, [m.series() for m in smons], dc.SERIAL_TOL)
        dc.report("probes %s f64 vs serial HIP" % name, worst, dc.SERIAL_TOL)
