"""CPU companion of tests/test_lowdim_blocked_gpu.py: conditions on its cases,
checked on the torch oracle alone.

The case tables, inputs, oracles and checks come from that module (one shared
set, so the GPU tests cannot run a case these checks did not see):

* every case meets the preconditions the HIP wrappers state (``_tb2d_step``
  and ``resident_1d`` in ops/hip_ops.py: their own validation needs device
  tensors) and has the seams / the CPL it claims; the tables together reach
  what the module promises (TMz Hy sources, a second y workgroup in both
  types, automatic / one-row / whole-grid chunks, update boxes strictly
  inside the array, every CPL instance of each type, every source residue);
* every fp32 case is well conditioned: the torch oracle in float32 stays
  within 1 / 8 of the family's fp32 bound of the fp64 oracle, through the same
  check code the GPU tests run (sentinels, guards and untouched inputs
  included) -- this defines the bounds; ``test_measured_maxima`` prints the
  maxima behind the figures of the GPU module's docstring;
* every case is live: a deliberate error on the oracle side -- an update box
  shifted by a cell, the per-cell arrays of two components swapped, the source
  values shifted by one level, an H source applied after the H update, the 1D
  source cell off by one -- moves the result by at least ``LIVE`` = 100 times
  the bound in the affected kind;
* the native CPU loop (csrc/host_yee1d.cpp) runs the whole 1D table against
  the torch loop with the same bounds.
"""
import functools

import pytest
import torch

import test_lowdim_blocked_gpu as L

LIVE = 100.0


def _inside(b, lo, hi):
    return all(lo[d] <= b[0][d] <= b[1][d] <= hi[d] for d in range(2))


# ----------------------------------------------------------------------- 2D
@pytest.mark.parametrize("name", list(L.CASES2))
def test_2d_case_is_valid(name):
    """_tb2d_step's preconditions, the claimed launch, and what the case says."""
    cs = L.CASES2[name]
    assert 1 <= cs.T <= 8
    for prec in L.PRECS:
        L.assert_claim2(cs, prec)
        nx, ny = L.size_of(cs, prec)
        assert ny % L.NV[prec] == 0
        for mode in L.MODES:
            inp = L.inputs2(name, mode, prec)
            comps = L.COMPS2[mode]
            assert _inside(inp["obox"], (0, 0), (nx, ny)) and inp["obox"][0][0] < inp["obox"][1][0]
            for c in comps:
                b = inp["upd"][c]
                assert _inside(b, (0, 0), (nx, ny)) and b[0][0] < b[1][0] and b[0][1] < b[1][1], (name, c, b)
                if cs.shrink is not None:
                    # strictly inside the array: the coefficient is masked to 0 on cells the kernel loads
                    assert b[0][0] >= 2 and b[0][1] >= 2 and b[1][0] <= nx - 2 and b[1][1] <= ny - 2
            if cs.shrink is not None:
                assert len({tuple(s) for s in cs.shrink}) == 3
            if inp["src"] is not None:
                comp, idx = inp["src"][0][0], inp["src"][0][1]
                assert comp == comps[cs.src[0]] and 0 <= idx[0] < nx and 0 <= idx[1] < ny and idx[2] == 0
                assert all(s[0] == comp and s[1] == idx for s in inp["src"]) and len(inp["src"]) == cs.T + 1
                assert len({s[2] for s in inp["src"]}) == cs.T + 1
            # the oracle stored the output box of every component and nothing else; a stored cell outside
            # its update box carries its input value (the source's cell: the source's last value)
            want = L.oracle2(name, mode, prec)
            inside, carried = L.masks2(name, mode, prec)
            for c in comps:
                assert torch.equal(want["fout"][c] != want["sent"][c], inside), (name, mode, c)
                m = carried[c].clone()
                if inp["src"] is not None and inp["src"][0][0] == c:
                    i, j, _ = inp["src"][0][1]
                    if m[i, j, 0]:
                        assert float(want["fout"][c][i, j, 0]) == inp["src"][cs.T - 1][2]
                    m[i, j, 0] = False
                assert torch.equal(want["fout"][c][m], inp["fin"][c][m]), (name, mode, c)
    if cs.same_as:
        base = L.CASES2[cs.same_as]
        assert (base.T, base.size, base.obox, base.shrink, base.src, base.cells) == \
            (cs.T, cs.size, cs.obox, cs.shrink, cs.src, cs.cells) and not base.same_as


def test_2d_table_reaches_what_it_promises():
    cases = L.CASES2_LIST
    assert {c.T for c in cases} == set(range(1, 9))
    for prec in L.PRECS:
        n = L.NV[prec]
        assert {1, n, n + 1, 8} <= {c.T for c in cases if c.src is not None}
        # (23, 1000) is the smallest ny with a second workgroup in y in both types
        assert L.launch2d(1, prec, ((0, 0), (23, 1000)), 5)[1] >= 2
        assert sum(L.launch2d(c.T, prec, L.obox_of(c, prec), c.xchunk)[1] >= 2 for c in cases) >= 20
    assert L.launch2d(4, "f32", ((0, 0), (23, 992)), 5)[1] == 1 and L.launch2d(4, "f32", ((0, 0), (23, 996)), 5)[1] == 2
    tags = {t for c in cases for t in c.at}
    assert tags == {"lane-last", "lane-first", "wg-seam", "y0", "y-last", "chunk-first", "chunk-last", "row0",
                    "row-last", "outside"}
    # every component of the mode carries a source somewhere: slot 2 is Hy in TMz
    assert {c.src[0] for c in cases if c.src is not None} == {0, 1, 2} and L.COMPS2["tmz"][2] == "Hy"
    for tag in ("lane-last", "lane-first", "wg-seam"):
        assert len({c.src[0] for c in cases if tag in c.at}) >= 2, tag
    # chunking: automatic, one row, at least nx; all against one oracle
    for base in ("seam-T5", "seam-T8"):
        twins = [c for c in cases if c.same_as == base]
        assert sorted(c.xchunk for c in twins)[:2] == [0, 1] and max(c.xchunk for c in twins) >= 23
        for prec in L.PRECS:
            assert L.launch2d(L.CASES2[base].T, prec, ((0, 0), (23, 1000)), 0)[3] == 1  # one row per chunk
    assert any(L.size_of(c, "f32")[0] < c.T for c in cases)
    assert any(c.shrink is not None and c.obox is None for c in cases)
    odd = [c for c in cases if c.obox is not None and c.obox[0][1] % 2 == 1 and (c.obox[1][1] + 1) % 4 == 0]
    assert odd
    corners = {(c.obox[0][0] == 0, c.obox[0][1] == 0, c.obox[1][0] == 23, c.obox[1][1] == 1000)
               for c in cases if c.obox is not None and c.shrink is not None}
    assert {(True, True, False, False), (True, False, False, True), (False, True, True, False),
            (False, False, True, True)} <= corners
    for kind in ("E", "H", "EH", "one"):
        sub = [c for c in cases if c.cells == kind]
        assert {c.T for c in sub} == {1, 5, 8} and all(c.src is not None and c.obox is not None for c in sub)
    for mode in L.MODES:
        two = [k for k in "EH" if sum(c[0] == k for c in L.COMPS2[mode]) == 2][0]
        one = L.CELL_SLOTS[mode]["one"]
        assert len(one) == 1 and L.COMPS2[mode][one[0]][0] == two


@functools.lru_cache(None)
def cond2(name, mode):
    """Error of the float32 torch oracle, through the GPU test's check."""
    cs = L.CASES2[name]
    dut, _ = L.pair2(mode, L.size_of(cs, "f32"), "f32", "cpu", "torch")
    out = L.run2(name, mode, "f32", dut, "cpu", torch.float32)
    return L.check2(name, mode, "f32", out, L.BOUND32_2D / 8)


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("name", list(L.CASES2))
def test_2d_case_is_conditioned(name, mode):
    print("conditioning 2d %s %s: %.3g of the fp32 bound" % (name, mode, cond2(name, mode) / L.BOUND32_2D))


def _moved2(name, mode, prec, mutate):
    """Largest change per kind between the oracle and a mutated oracle, on the kind's scale."""
    base, other = L.oracle2(name, mode, prec), L.oracle2(name, mode, prec, mutate)
    inside, _ = L.masks2(name, mode, prec)
    comps = L.COMPS2[mode]
    sc = L.scales2(base["fout"], inside, comps)
    out = {"E": 0.0, "H": 0.0}
    for c in comps:
        out[c[0]] = max(out[c[0]], float((base["fout"][c] - other["fout"][c]).abs().max()) / sc[c[0]])
    return out


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("name", [c.name for c in L.CASES2_LIST if not c.same_as])
def test_2d_case_is_live(name, mode):
    cs = L.CASES2[name]
    comps = L.COMPS2[mode]
    for prec in L.PRECS:
        probes = [("shift-box", comps[L.CASES2_LIST.index(cs) % 3][0])]
        if cs.src is not None:
            probes.append(("src-level", None))
            _, sx, sy = L.src_cell(cs, prec)
            ub = L.inputs2(name, mode, prec)["upd"][comps[cs.src[0]]]
            if comps[cs.src[0]][0] == "H" and ub[0][0] <= sx < ub[1][0] and ub[0][1] <= sy < ub[1][1]:
                probes.append(("h-after", "H"))  # (outside its update box the cell keeps the value either way)
        if cs.cells:
            probes.append(("swap-cells", None))
        for mutate, kind in probes:
            mv = _moved2(name, mode, prec, mutate)
            print("live 2d %s %s %s %s: E %.3g H %.3g" % (name, mode, prec, mutate, mv["E"], mv["H"]))
            got = max(mv.values()) if kind is None else mv[kind]
            assert got >= LIVE * L.BOUND32_2D, (name, mode, prec, mutate, mv)


# ----------------------------------------------------------------------- 1D
@pytest.mark.parametrize("name,prec", L.PARAMS1)
def test_1d_case_is_valid(name, prec):
    """resident_1d's preconditions and the claimed instance."""
    cs = L.CASES1[name]
    L.assert_claim1(cs, prec)
    n, src = cs.n, L.src_of(cs)
    (elo, ehi), (hlo, hhi) = L.boxes1(cs)
    assert 0 <= cs.steps <= 37 and 0 < n <= L.max_cells(prec)
    assert ehi == elo == 0 or (1 <= elo < ehi <= n)
    assert 0 <= hlo < hhi <= n - 1
    inp = L.inputs1(name, prec)
    if src is not None:
        assert 0 <= src < n and inp["vals"].numel() == cs.steps + 1 and len(set(inp["vals"].tolist())) == cs.steps + 1
    # outside the boxes the oracle keeps the input, the source's cell its last value
    want = L.oracle1(name, prec)
    for c, (lo, hi) in zip(("Ez", "Hy"), ((elo, ehi), (hlo, hhi))):
        outside = torch.ones(n, dtype=torch.bool)
        outside[lo:hi] = False
        if c == "Ez" and src is not None and cs.steps > 0:
            assert float(want["Ez"][src]) == float(inp["vals"][cs.steps - 1])
            outside[src] = False
        assert torch.equal(want[c][outside], inp[c.lower()][outside]), (name, c)


def test_1d_table_reaches_what_it_promises():
    cases = L.CASES1_LIST
    for prec in L.PRECS:
        mine = [c for c in cases if prec in c.precs]
        assert {c.cpl for c in mine} == set(L.CPLS[prec])
        prev = 0
        for cpl in L.CPLS[prec]:
            sub = [c for c in mine if c.cpl == cpl]
            # the largest n that fits with its shift, and a small n just past the previous instance
            offs = [0 if c.src is None else (cpl - L.src_of(c) % cpl) % cpl for c in sub]
            assert any(c.n + o == L.NT * cpl for c, o in zip(sub, offs)), (prec, cpl)
            assert any(c.n <= max(L.NT * prev + 1, 7) for c in sub), (prec, cpl)
            if cpl >= 2:
                res = {L.src_of(c) % cpl for c in sub if c.src is not None}
                assert {0, 1, cpl - 1} <= res, (prec, cpl, res)
            prev = cpl
        assert any(c.n == L.max_cells(prec) for c in mine)
        assert any(c.cells and c.cpl == L.CPLS[prec][-1] for c in mine)
    assert L.max_cells("f32") == 16369 and L.max_cells("f64") == 12277
    odd = [c for c in cases if c.n == 2048 and c.src is not None and c.src % 2 == 1]
    assert odd and all(c.cpl == 4 for c in odd)
    assert any(c.src is None and not c.cells for c in cases)
    assert any(c.src == 0 for c in cases) and any(c.src == -1 for c in cases)
    assert {0, 1} <= {c.steps for c in cases}
    assert any(c.ebox == "empty" for c in cases) and any(c.ebox not in (None, "empty") and c.hbox for c in cases)
    assert {"E", "H", "EH"} <= {c.cells for c in cases}


@functools.lru_cache(None)
def cond1(name):
    """Error of the float32 torch loop, through the GPU test's check."""
    cs = L.CASES1[name]
    dut, _ = L.pair1(cs.n, "f32", "cpu", "torch")
    out = L.run1(name, "f32", dut, "cpu", torch.float32)
    return L.check1(name, "f32", out, L.BOUND32_1D / 8)


@pytest.mark.parametrize("name", list(L.CASES1))
def test_1d_case_is_conditioned(name):
    print("conditioning 1d %s: %.3g of the fp32 bound" % (name, cond1(name) / L.BOUND32_1D))


@pytest.mark.parametrize("name,prec", L.PARAMS1)
def test_1d_case_is_live(name, prec):
    cs = L.CASES1[name]
    base = L.oracle1(name, prec)
    if cs.steps == 0:
        inp = L.inputs1(name, prec)
        assert torch.equal(base["Ez"], inp["ez"]) and torch.equal(base["Hy"], inp["hy"])
        return
    probes = ["shift-box"]
    if cs.src is not None:
        probes += ["src-level", "src-cell"]
    if cs.cells:
        probes.append("swap-cells")
    for mutate in probes:
        other = L.oracle1(name, prec, mutate)
        mv = {c: float((base[c] - other[c]).abs().max()) / float(base[c].abs().max()) for c in ("Ez", "Hy")}
        print("live 1d %s %s %s: E %.3g H %.3g" % (name, prec, mutate, mv["Ez"], mv["Hy"]))
        assert max(mv.values()) >= LIVE * L.BOUND32_1D, (name, prec, mutate, mv)


def _host_library():
    try:
        from fdtd3d_amd.native import load_host_library
        lib = load_host_library(build_if_missing=False)
        return lib.fdtd_res1d_cpu_f32 and lib.fdtd_res1d_cpu_f64
    except (OSError, AttributeError):
        return None


@pytest.mark.parametrize("name,prec", L.PARAMS1)
def test_1d_native_loop(name, prec):
    """csrc/host_yee1d.cpp over the whole table, against the torch loop with the GPU tests' bounds."""
    if _host_library() is None:
        pytest.skip("host library not built")
    cs = L.CASES1[name]
    dut, _ = L.pair1(cs.n, prec, "cpu", "torch")
    out = L.run1(name, prec, dut, "cpu", L.DT[prec], native=True)
    worst = L.check1(name, prec, out, L.bound_of("1d", prec))
    print("native 1d %s %s: %.3g of the bound" % (name, prec, worst / L.bound_of("1d", prec)))


# ------------------------------------------------------------------- bounds
def test_measured_maxima():
    """The fp32-oracle maxima per family: each fp32 bound is 8 x its maximum
    (rounded up to two digits; raised only on recorded GPU evidence), at most the project's 2e-5."""
    m2 = max((cond2(c.name, m), c.name, m) for c in L.CASES2_LIST for m in L.MODES)
    m1 = max((cond1(c.name), c.name) for c in L.CASES1_LIST)
    print("measured 2D: fp32 oracle vs fp64 at most %.3g (%s %s): 8 x = %.3g, BOUND32_2D = %.3g"
          % (m2[0], m2[1], m2[2], 8 * m2[0], L.BOUND32_2D))
    print("measured 1D: fp32 oracle vs fp64 at most %.3g (%s): 8 x = %.3g, BOUND32_1D = %.3g"
          % (m1[0], m1[1], 8 * m1[0], L.BOUND32_1D))
    for worst, bound in ((m2[0], L.BOUND32_2D), (m1[0], L.BOUND32_1D)):
        assert 8 * worst <= bound <= L.CAP32
        assert bound <= 8 * worst * 1.05 or bound in L.RAISED, (worst, bound)
    assert L.BOUND64 == 1e-12
