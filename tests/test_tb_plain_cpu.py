"""CPU companion of tests/test_tb_plain_gpu.py: conditions on its cases,
checked on the torch oracle alone.

The case tables, inputs, oracles and run / check functions come from that
module (one shared set, so the GPU tests cannot run a case these checks did
not see):

* every case has the tiles, seams and all-in / not-all-in tiles it claims, by
  the formulas that mirror the launchers, and meets the preconditions the HIP
  wrapper states;
* every fp32 case is well conditioned: the torch oracle in float32 stays
  within HALF ``BOUND32`` of the fp64 oracle, through the same check code the
  GPU tests run (sentinels and untouched inputs included);
* every case is live: a small deliberate error on the oracle side -- one
  update box shifted by one cell, the source value of the last level dropped,
  the source moved by one cell, the per-cell region shifted by one cell --
  moves the result by at least ``LIVE`` = 100 times the bound the GPU test
  uses (the convention of tests/test_tb_variants_cpu.py), and so does ``Db``
  scaled at the first level only (below).

The ``Db`` error.  ``Db (1 + 1e-3)`` at the first level changes H by 1e-3 of
the level's ``Db curl E`` term.  That term is one of the two summands of the
new H, so its maximum cannot exceed the maximum of H by much and the change,
on the scale of H, stays below about 1e-3 = 50 x ``BOUND32`` whatever the
seed or the size: 100 x is out of reach of a 1e-3 error (measured 50 .. 65 x
on the whole-grid cases, 15 .. 30 x where the update boxes are cut and fewer
cells take the term).  So two sizes are asserted: the 1e-3 error moves H by
at least ``DB_LIVE`` = 10 x the bound, an order of magnitude above what the
GPU test lets pass, and a 1 % error by at least ``LIVE`` = 100 x.  tests/test_tb_gpu.py
test_tb_op_vs_torch draws E and H both as N(0, 1) and allows
``2e-5 (max|y| + 1)``: ``test_db_error_under_unit_scaling`` computes what
errors are worth there.  The ``Db`` error itself shows there as well (60.7 x
its allowed error at T = 1, 58.1 x ``BOUND32`` here): the first E half step
makes E = Cb curl H ~ 377 whatever E was, so the level's ``Db curl E`` is of
the size of H under either scaling.  What unit scaling cannot see is the INPUT
E: it is 1 / 377 of the new E, ``Db curl E_in`` ~ 3e-3 against an allowed 1e-4
or more.  An input E that is 3 % off is worth 4.2 x the allowed error there
and 1060 x ``BOUND32`` here: unit scaling is 250 times less sensitive to the
input E (at least 100 times, asserted).
"""
import pytest
import torch

import test_tb_plain_gpu as P
import test_tb_variants_gpu as V

LIVE = 100.0
DB_LIVE = 10.0
HALF32 = 0.5 * V.BOUND32


def _inside(box, lo, hi):
    return all(lo[d] <= box[0][d] <= box[1][d] <= hi[d] for d in range(3))


def _cell_in(idx, box):
    return all(box[0][d] <= idx[d] < box[1][d] for d in range(3))


def _moved(base, other, sent):
    """Largest change per kind between two oracle results, on the kind's scale."""
    sc = V.kind_scales(base, sent)
    out = {"E": 0.0, "H": 0.0}
    for c in V.COMPS:
        out[c[0]] = max(out[c[0]], float((base[c] - other[c]).abs().max()) / sc[c[0]])
    return out


def gpu_runs():
    """(case, kernel) of every launch the GPU module makes."""
    runs = [("int-T%d" % T, k) for T, k in P.INTERIOR] + [("int-T%d" % T, k) for k, T in P.XCHUNK_KERNELS]
    runs += [("upd-%s-T%d" % (w, T), k) for w, k, T in P.UPDATE]
    runs += [("out-%s-T%d" % (b, T), P.output_family(b, T, thin)) for b, T, thin in P.OUTPUT]
    runs += [("out-%s-T4" % b, "f64half") for b in P.OUT_BOXES]
    runs += [(P.source_case(k, T, c, w), k) for k, T, c in P.SOURCES for w in P.SRC_WHERE]
    runs += [(P.percell_case(f, T, kinds), P.PC_FORMS[f][0]) for f, T, kinds in P.PERCELL]
    runs += [("map-T%d" % T, "f64half" if half else "f64full") for T, half in P.MAP]
    runs += [(n, k) for n, k, _ in P.CHILD_RUNS] + [("int-T3", "mr16x2"), ("int-T3", "f64half")]
    return runs


RUNS = gpu_runs()
F32_CASES = sorted({n for n, k in RUNS if P.KERN[k][0] == "f32"})


def test_every_case_is_run():
    assert {n for n, _ in RUNS} == set(P.CASES)
    for name, kern in RUNS:
        cs = P.CASES[name]
        assert cs.T <= {"single": 4, "mr8x2": 5, "f64half": 5, "f64full": 5}.get(kern, 6), (name, kern)


# ----------------------------------------------------------- tile arithmetic
@pytest.mark.parametrize("T,kern", P.INTERIOR)
def test_interior_claims(T, kern):
    inn, out = P.interior_claims(T, kern)
    print("interior T %d %s: all-in %s" % (T, kern, inn))
    if V.GEOM[kern][0] == 32:
        assert (1, 1) in inn and (0, 0) in out
    # bit 3 of tb_variant is what turns the fast path off: both halves of the variant loop exist
    assert {v & 8 for v in range(16)} == {0, 8}


def test_xchunk_claims():
    for kern, T in P.XCHUNK_KERNELS:
        assert any(0 < xc < T for xc in P.XCHUNKS) or T == 2, (kern, T)
        assert 0 in P.XCHUNKS and P.SIZE[0] in P.XCHUNKS and 1 in P.XCHUNKS
        for xc in P.XCHUNKS:
            if xc:
                g = V.tiles(kern, T, P.CASES["int-T%d" % T].obox, xc)
                assert g[0] == -(-P.SIZE[0] // xc)
    assert any(1 < T for _, T in P.XCHUNK_KERNELS if 1 in P.XCHUNKS)  # a chunk shorter than T: lead-in and drain overlap
    assert ("mr16x2", 5) in P.XCHUNK_KERNELS and ("single", 2) in P.XCHUNK_KERNELS and ("f64half", 4) in P.XCHUNK_KERNELS


@pytest.mark.parametrize("which,kern,T", P.UPDATE)
def test_update_claims(which, kern, T):
    got = P.update_claims(which, kern, T)
    assert (got is None) == (not kern.startswith("mr"))
    name = "upd-%s-T%d" % (which, T)
    upd, local = P.inputs(name)["upd"], P.inputs("int-T%d" % T)["upd"]
    if which == "whole":
        assert all(b == ((0, 0, 0), P.SIZE) for b in upd.values())
    elif which == "six":
        assert len(set(upd.values())) == 6
        assert all(_inside(b, (0, 0, 0), P.SIZE) and not V._empty(b) for b in upd.values())
        assert all(upd[c] != local[c] for c in V.COMPS)
    elif which == "xcut":
        assert all(upd[c][0][1:] == local[c][0][1:] and upd[c][1][1:] == local[c][1][1:] for c in V.COMPS)
        assert sum(upd[c] != local[c] for c in V.COMPS) == len(P.XCUT) == 4
    else:
        assert sorted(c for c in V.COMPS if V._empty(upd[c])) == sorted(P.EMPTY)
        assert {c[0] for c in P.EMPTY} == {"E", "H"}
        # an empty update box: the component's output is its input on the whole output box
        want = P.oracle(name)
        for c in P.EMPTY:
            assert torch.equal(want["fout"][c], P.inputs(name)["fin"][c])


def test_output_claims():
    seen = set()
    for box, T, thin in P.OUTPUT:
        ob = P.OUT_BOXES[box]
        assert _inside(ob, (0, 0, 0), P.SIZE) and not V._empty(ob)
        fam = P.lib_family("f32", T, *P.auto_opts(T, ob, thin))
        assert fam == P.output_family(box, T, thin), (box, T, thin, fam)
        seen.add(fam)
    assert seen == {"single", "mr16x2", "mr8x2"}
    ext = lambda b, d: P.OUT_BOXES[b][1][d] - P.OUT_BOXES[b][0][d]
    assert {P.OUT_BOXES["inner-z%d" % r][0][2] % 4 for r in (1, 2, 3)} == {1, 2, 3}
    assert ext("z-shell", 2) == 2 and ext("x-shell", 0) == 1 and ext("y-shell5", 1) == 5 and ext("y-shell8", 1) == 8
    assert all(ext("cell", d) == 1 for d in range(3)) and P.OUT_BOXES["corner"][1] == P.SIZE
    # the 8-row shell sits exactly on the thin-shell switch, which both values of tb_thin_mr16 take at T = 4
    assert P.auto_opts(4, ((0, 0, 0), (14, 9, 144)), False) == (0, 0)
    assert {P.output_family("y-shell8", 4, t) for t in (False, True)} == {"single", "mr8x2"}
    assert ("y-shell8", 4, True) in P.OUTPUT and ("y-shell8", 4, False) in P.OUTPUT


@pytest.mark.parametrize("kern,T,comp", P.SOURCES)
def test_source_claims(kern, T, comp):
    """Every placement is where ``source_cell`` says."""
    ob, size = P.SRC_OBOX, P.SIZE
    upd = P.inputs("int-T%d" % T)["upd"][comp]
    sm = V.seams(kern, T, ob)
    assert all(len(s) >= 1 for s in sm)
    cell = {w: P.source_cell(kern, T, comp, w) for w in P.SRC_WHERE}
    for w, idx in cell.items():
        assert _cell_in(idx, ((0, 0, 0), size)), (w, idx)
        assert P.CASES[P.source_case(kern, T, comp, w)].src == (comp, idx)
    for w in ("inside", "first", "last", "xseam", "border"):
        assert _cell_in(cell[w], ob), w
    own = lambda idx, d: sum(q <= idx[d] for q in sm[d])  # the tile / chunk that owns the cell along d
    assert own(cell["inside"], 1) == own(cell["inside"], 2) == 1
    assert all(cell["inside"][d] not in sm[d] and cell["inside"][d] + 1 not in sm[d] for d in range(3))
    if kern.startswith("mr"):
        name = P.source_case(kern, T, comp, "inside")
        assert (1, 1) in P.tile_kinds(kern, T, name)[0], "the source's tile is all-in"
    assert cell["first"][1] == sm[1][0] and cell["first"][2] == sm[2][0]
    assert cell["last"][1] == sm[1][0] - 1 and cell["last"][2] == sm[2][0] - 1
    assert cell["xseam"][0] == sm[0][0]
    below = lambda idx: ob[0][2] - idx[2]
    assert 0 < below(cell["near"]) < T and below(cell["far"]) > T
    assert not _cell_in(cell["border"], upd) and any(cell["border"][d] in (0, size[d] - 1) for d in range(3))
    for w in ("inside", "first", "last", "xseam", "near", "far"):
        assert _cell_in(cell[w], upd), w


@pytest.mark.parametrize("form,T,kinds", P.PERCELL)
def test_percell_claims(form, T, kinds):
    P.percell_claims(form, T, kinds)
    name = P.percell_case(form, T, kinds)
    cs = P.CASES[name]
    cells = P.cells_of(name)
    assert sorted(cells) == sorted(c for c in ("Ex", "Ez", "Hy", "Hz") if c[0] in kinds)
    assert _inside(cs.region, (1, 1, 1), tuple(s - 2 for s in cs.size))
    for c, cell in cells.items():
        inside = cell[P.box_slices(cs.region)]
        assert 0.3 <= float(inside.min()) and float(inside.max()) <= 1.0 and float(inside.std()) > 0.1
        assert int((cell != 1).sum()) == inside.numel() and torch.equal(cell, cell.float().double())
    if form == "sparse":
        assert T <= 5
    assert {k for _, _, k in P.PERCELL} == {"E", "H", "EH"}


def test_map_claims():
    """Per fp64 tile shape: a launch with a narrower last band AND a narrower last column of the default 2 x 8
    patch walk, and one whose tile count is no multiple of 8."""
    for half in (1, 0):
        what = [P.map_grid(T, h) for T, h in P.MAP if h == half]
        print("fp64 map half %d: %s" % (half, what))
        assert any(w["narrow"] for _, w in what) and any(w["tail"] for _, w in what), (half, what)
        assert all(g[0] >= 2 for g, _ in what)
    g32 = V.tiles("mr16x2", 5, P.CASES["int-T5"].obox)
    g64 = V.tiles("f64half", 4, P.CASES["map-T4"].obox)
    assert g32[2] % 2 and g32[1] % 3 and g64[2] % 3 and g64[1] % 2  # the child's 2x3 / 3x2 patches: narrower ends


# ------------------------------------------------------------ every case
@pytest.mark.parametrize("name", list(P.CASES))
def test_case_is_valid(name):
    """tb_step's preconditions (ops/hip_ops.py) and the cost limits."""
    cs, inp = P.CASES[name], P.inputs(name)
    size = cs.size
    assert size[0] * size[1] * size[2] < 200000
    assert 1 <= cs.T <= 6 and (name not in F32_CASES or size[2] % 4 == 0)
    assert _inside(cs.obox, (0, 0, 0), size) and not V._empty(cs.obox)
    assert all(V._empty(b) or _inside(b, (0, 0, 0), size) for b in inp["upd"].values())
    if inp["src"] is not None:
        comp, idx = inp["src"][0][0], inp["src"][0][1]
        assert comp in V.E and _cell_in(idx, ((0, 0, 0), size)) and len(inp["src"]) == cs.T
        assert all(s[0] == comp and s[1] == idx for s in inp["src"])
        assert [s[2] for s in inp["src"]] == [inp["Z"] * (0.5 + 0.25 * l) for l in range(cs.T)]
    assert (cs.region is None) == (cs.kinds == "")
    # the oracle writes the whole output box of every component and nothing else
    want = P.oracle(name)
    n = (cs.obox[1][0] - cs.obox[0][0]) * (cs.obox[1][1] - cs.obox[0][1]) * (cs.obox[1][2] - cs.obox[0][2])
    for c in V.COMPS:
        assert int((want["fout"][c] != want["sent"][c]).sum()) == n


@pytest.mark.parametrize("name", F32_CASES)
def test_case_is_conditioned(name):
    dut = V.pair(V.vacuum_cfg(P.CASES[name].size, "f64"), "f32", "cpu", "torch")[0]
    out = P.run(name, dut, "cpu", torch.float32)
    worst = P.check(name, out, "f32", ("float32 oracle",), bound=HALF32)
    print("conditioning %s: %.3g of the fp32 bound" % (name, worst * HALF32 / V.BOUND32))


@pytest.mark.parametrize("name", list(P.CASES))
def test_case_is_live(name):
    cs, base = P.CASES[name], P.oracle(name)

    def moved(mutate):
        mv = _moved(base["fout"], P.oracle(name, mutate)["fout"], base["sent"])
        print("live %s %s: E %.3g H %.3g x BOUND32" % (name, mutate, mv["E"] / V.BOUND32, mv["H"] / V.BOUND32))
        return mv
    assert moved("db-1e-3")["H"] >= DB_LIVE * V.BOUND32, name
    assert moved("db-1e-2")["H"] >= LIVE * V.BOUND32, name
    if name.startswith(("int-", "upd-", "map-")):
        assert max(moved("shift-box").values()) >= LIVE * V.BOUND32, name
    if cs.src is not None:
        where = name.rsplit("-", 1)[1]
        if where == "far":
            # more than T cells below the output box: nothing stored depends on the source
            other = P.oracle(name, "no-src")
            assert all(torch.equal(base["fout"][c], other["fout"][c]) for c in V.COMPS)
        else:
            assert max(moved("move-src").values()) >= LIVE * V.BOUND32, name
            assert max(moved("no-src").values()) >= LIVE * V.BOUND32, name
        if where in ("inside", "first", "last", "xseam", "border"):
            assert max(moved("drop-last").values()) >= LIVE * V.BOUND32, name
        if where == "border":
            # the cell lies outside its component's update box and still carries the last level's value
            comp, idx, val = P.inputs(name)["src"][-1]
            assert float(base["fout"][comp][idx]) == val
    if cs.kinds:
        assert max(moved("shift-region").values()) >= LIVE * V.BOUND32, name


def test_db_error_under_unit_scaling():
    """What ``Db (1 + 1e-3)`` at the first level is worth under test_tb_op_vs_torch's inputs and bound (E and H
    both N(0, 1), ``2e-5 (max|y| + 1)`` per component), next to the same error here."""
    name = "int-T1"
    ref = V.scheme(V.vacuum_cfg(P.SIZE, "f64"), "torch", "cpu", torch.float64)
    fin = {c: V.randn(P.SIZE, 3 + n) for n, c in enumerate(V.COMPS)}
    outs = []
    for ops in (ref.ops, P._db_scaled(ref.ops, 1.0 + 1e-3)):
        fout = {c: fin[c].clone() for c in V.COMPS}
        ops.tb_step(fin, fout, P.inputs(name)["upd"], P.CASES[name].obox, ref.cb, 1, None)
        outs.append(fout)
    unit = max(float((outs[0][c] - outs[1][c]).abs().max()) / (2e-5 * (float(outs[0][c].abs().max()) + 1.0)) for c in V.H)
    base = P.oracle(name)
    here = _moved(base["fout"], P.oracle(name, "db-1e-3")["fout"], base["sent"])["H"] / V.BOUND32
    cb, db = ref.cb["Ex"].scalar, ref.cb["Hx"].scalar
    e_in = db * 2.0  # Db curl of the INPUT E (four N(0, 1) terms: sigma 2) under unit scaling
    print("Db (1 + 1e-3) at level 0: %.3g x the allowed error under unit scaling, %.3g x BOUND32 here; "
          "Db curl E_in ~ %.3g, Cb %.3g" % (unit, here, e_in, cb))
    assert here >= DB_LIVE
    assert e_in < 5e-3  # the input E's share of the term under unit scaling: below the allowed 1e-4 at 4 %
    # an input E that is 3 % off: what it is worth under either scaling
    ratio = {}
    for what, f in (("unit", fin), ("live", P.inputs(name)["fin"])):
        outs = []
        for k in (1.0, 1.03):
            fout = {c: f[c].clone() for c in V.COMPS}
            ref.ops.tb_step({c: f[c] * (k if c[0] == "E" else 1.0) for c in V.COMPS}, fout, P.inputs(name)["upd"],
                            P.CASES[name].obox, ref.cb, 1, None)
            outs.append(fout)
        if what == "unit":
            ratio[what] = max(float((outs[0][c] - outs[1][c]).abs().max()) / (2e-5 * (float(outs[0][c].abs().max()) + 1.0))
                              for c in V.COMPS)
        else:
            sc = {k: max(float(outs[0][c].abs().max()) for c in V.COMPS if c[0] == k) for k in "EH"}
            ratio[what] = max(float((outs[0][c] - outs[1][c]).abs().max()) / sc[c[0]] for c in V.COMPS) / V.BOUND32
    print("input E 3 %% off: %.3g x the allowed error under unit scaling, %.3g x BOUND32 here" % (ratio["unit"], ratio["live"]))
    assert ratio["live"] >= LIVE and ratio["live"] >= 100.0 * ratio["unit"]
