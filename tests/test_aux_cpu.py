"""CPU companion of tests/test_aux_gpu.py: without a GPU it

* asserts what every case of that file claims from the launchers' formulas
  (sweeps of the grid-stride loops, block counts, vector / scalar / masked
  form, which amplitude kernel, the clamps and the border cells of the
  scattered cases) and the ``BoxEnt`` table layout;
* runs the same ``run_*`` / ``check_*`` functions on the torch backend for the
  ops it has (pack, unpack, copy_box, maxabs, amplitude_update,
  amplitude_update_many, set_value, set_values, inc_step_e), and on a plain
  slicing / oracle stand-in for ``box_list`` and ``scattered``: the checks and
  references are themselves right;
* shows that every check bites: one wrong cell, one stray store outside a
  box, a changed input or a count off by one in the *result* fails it.

The torch backend's ``maxabs`` returns the fp64 maximum unrounded, so the three
fp64 cases whose maximum fp32 cannot hold are skipped here (``cpu=False``):
the GPU cases themselves never skip.
"""
import pytest
import torch

import test_aux_gpu as A
from fdtd3d_amd.ops import make_ops

CPU = "cpu"


def tops(dt):
    return make_ops("torch", None, CPU, A.DT[dt])


def bites(check, r):
    """The corrupted result must fail the check."""
    with pytest.raises(AssertionError):
        check(r)


def nudge(t, idx):
    """One wrong cell: the element moved to the next representable value."""
    flat = t.view(-1) if t.is_contiguous() else t
    v = flat[idx]
    flat[idx] = torch.nextafter(v, torch.full_like(v, float("inf"))) if bool(torch.isfinite(v)) else 0.0


# ------------------------------------------------------------------ box_list
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_box_list_table_layout_and_claims(dt):
    """_BoxList.build against the documented BoxEnt layout; vec, blk0 and the
    block count against the test's formula; the entries the issue lists."""
    entries, arrays, bufs, bl = A.boxlist_setup(dt, CPU)
    assert len(entries) >= 13 and len(entries) & (len(entries) - 1) != 0
    A.check_table(dt, entries, arrays, bufs, bl.build(A._EntSize))
    claims = [A.boxlist_claims(dt, e, arrays, bufs) for e in entries]
    V = A.VW[dt]
    vec_groups = [g for v, g, _ in claims if v == V]
    assert any(g < 256 for g in vec_groups) and 256 in vec_groups and 257 in vec_groups
    assert claims[0][:2] == (V, 256) and claims[-1] == (V, 257, 2)  # the first and the last entry
    assert any(A.vol(e["box"]) == 1 for e in entries)
    why = " / ".join(e["why"] for e, c in zip(entries, claims) if c[0] == 1)
    for word in ("lo.z", "hi.z", "odd buffer offset", "base not 16-byte aligned", "odd nz"):
        assert word in why
    # each scalar entry is scalar for its own reason only: undoing that reason makes it a vector entry
    for e in entries:
        if e["claim"].get("odd_off"):
            assert A.boxlist_claims(dt, dict(e, off=e["off"] - 1), arrays, bufs)[0] == V
        if "base not" in e["why"]:
            assert A.boxlist_claims(dt, dict(e, arr="local"), arrays, bufs)[0] == V
    shapes = {tuple(arrays[e["arr"]].shape) for e in entries}
    assert len(shapes) >= 3 and len({e["buf"] for e in entries}) == 2
    for name in arrays:  # boxes disjoint per array: the same table unpacks
        seen = torch.zeros(arrays[name].shape, dtype=torch.int32)
        for e in entries:
            if e["arr"] == name:
                seen[A.sl(e["box"])] += 1
        assert int(seen.max()) == 1


@pytest.mark.parametrize("pack", [True, False], ids=["pack", "unpack"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_box_list_check_on_reference(dt, pack):
    for args in ((), A.one_entry(dt)):
        r = A.run_boxlist(None, dt, CPU, pack, *args)
        A.check_boxlist(r)
        e = r["entries"][-1]
        if pack:
            b = r["bufs"][e["buf"]]
            nudge(b, e["off"])                       # a wrong cell of the last part
            bites(A.check_boxlist, r)
            r = A.run_boxlist(None, dt, CPU, pack, *args)
            r["bufs"][e["buf"]][e["off"] + A.vol(e["box"])] = 1.0  # a store one element past a part
            bites(A.check_boxlist, r)
            r = A.run_boxlist(None, dt, CPU, pack, *args)
            nudge(r["arrays"][e["arr"]], 0)          # a changed input
            bites(A.check_boxlist, r)
        else:
            t = r["arrays"][e["arr"]]
            t[e["box"][0]] = 0.5                     # a wrong cell inside the box
            bites(A.check_boxlist, r)
            r = A.run_boxlist(None, dt, CPU, pack, *args)
            t = r["arrays"]["field"]
            assert float(t[8, 10, 38]) == A.SENT
            t[8, 10, 38] = 0.5                       # a store one element before a box
            bites(A.check_boxlist, r)


def test_box_list_host_errors_cpu():
    A.boxlist_host_errors(CPU)


# ------------------------------------------------- pack / unpack / copy_box
@pytest.mark.parametrize("case,dt", A._ids(A.PACK_CASES)[0], ids=A._ids(A.PACK_CASES)[1])
def test_pack_unpack_claims_and_checks(case, dt):
    A.assert_copy_claims(case, dt, False)
    ops = tops(dt)
    r = A.run_pack(ops, case, dt, CPU)
    A.check_pack(r)
    nudge(r["big"], r["off"] + r["n"] - 1)  # the last packed element
    bites(A.check_pack, r)
    r = A.run_pack(ops, case, dt, CPU)
    r["big"][r["off"] + r["n"]] = 0.0       # a store one element past the message
    bites(A.check_pack, r)
    r = A.run_unpack(ops, case, dt, CPU)
    A.check_unpack(r)
    box = r["box"]
    stray = None
    for d in (2, 1, 0):  # a cell next to the box, where the array has one
        if box[1][d] < case["shape"][d]:
            stray = list(box[0])
            stray[d] = box[1][d]
            break
    if stray is not None:
        r["fields"][-1][tuple(stray)] = 0.25
        bites(A.check_unpack, r)
        r = A.run_unpack(ops, case, dt, CPU)
    r["fields"][0][box[0]] = 0.25           # a wrong cell inside the box
    bites(A.check_unpack, r)


@pytest.mark.parametrize("case,dt", A._ids(A.XFER_CASES)[0], ids=A._ids(A.XFER_CASES)[1])
def test_copy_box_claims_and_checks(case, dt):
    A.assert_copy_claims(case, dt, True)
    r = A.run_xfer(tops(dt), case, dt, CPU)
    A.check_xfer(r)
    box = r["box"]
    last = tuple(h - 1 for h in box[1])
    nudge(r["dst"][-1][last[0], last[1]], last[2])  # the last cell of the box
    bites(A.check_xfer, r)
    if box[0][2] > 0:  # the masked cases: the cell below lo.z belongs to someone else
        r = A.run_xfer(tops(dt), case, dt, CPU)
        r["dst"][0][box[0][0], box[0][1], box[0][2] - 1] = 0.25
        bites(A.check_xfer, r)
    r = A.run_xfer(tops(dt), case, dt, CPU)
    nudge(r["src"][0], 0)
    bites(A.check_xfer, r)


def test_copy_cases_cover_the_limits():
    """The tables hold what they are there for."""
    for cases, xfer in ((A.PACK_CASES, False), (A.XFER_CASES, True)):
        seen = {(A.copy_claims(c, dt, xfer)[0], A.copy_claims(c, dt, xfer)[1], dt) for c in cases for dt in c["dts"]}
        want = [("scalar", 2, "f32"), ("scalar", 2, "f64"), ("vec", 2, "f32"), ("vec", 2, "f64")]
        if xfer:
            want += [("masked", 2, "f32"), ("masked", 2, "f64")]
        assert all(w in seen for w in want), seen
        assert max(c["ncomp"] for c in cases) == 8
        assert max(A.copy_claims(c, "f32", xfer)[2] for c in cases) == 65535
        assert any(c["base"] == "odd" for c in cases)
    assert A.PACK_CASES[5]["shape"][2] % 4 == 0  # the misaligned bases alone make that case scalar
    assert A.copy_claims(dict(A.PACK_CASES[5], base="aligned"), "f32", False)[0] == "vec"
    for name, shape, ncomp in A.LIMIT_CASES:
        assert ncomp == 9 or shape[0] * ncomp == 65536


# --------------------------------------------------------------------- maxabs
@pytest.mark.parametrize("case,dt", A._MA[0], ids=A._MA[1])
def test_maxabs_claims_and_checks(case, dt):
    A.maxabs_claims(case)
    if not case["cpu"]:
        # still: the reference gives what the case expects of the kernel
        t = A.maxabs_input(case, dt, CPU)
        want = A.maxabs_ref(t, case["box"])
        assert case["expect"] is None or want == case["expect"]
        assert float(t[A.sl(case["box"])].abs().max()) != want  # fp32 cannot hold the fp64 maximum
        pytest.skip("the torch backend returns the fp64 maximum unrounded: " + case["why"])
    r = A.run_maxabs(tops(dt), case, dt, CPU)
    A.check_maxabs(r)
    good = r["got"]
    r["got"] = 5.000000476837158 if good == 5.0 else (1.0 if good in (0.0, A.INF) else good * 2)
    bites(A.check_maxabs, r)
    r["got"] = good
    nudge(r["t"], 0)
    bites(A.check_maxabs, r)


def test_maxabs_cases_cover_the_issue():
    names = {c["name"] for c in A.MAXABS_CASES}
    assert {"outside-x-", "outside-x+", "outside-y-", "outside-y+", "outside-z-", "outside-z+"} <= names
    for c in A.MAXABS_CASES:
        if c["name"].startswith("outside"):  # the larger value sits in a cell touching the box, outside it
            t = A.maxabs_input(c, "f64", CPU)
            idx = tuple(int(v) for v in (t.abs() == 9.0).nonzero()[0])
            out = [d for d in range(3) if not A.MA_BOX[0][d] <= idx[d] < A.MA_BOX[1][d]]
            assert len(out) == 1 and idx[out[0]] in (A.MA_BOX[0][out[0]] - 1, A.MA_BOX[1][out[0]])
    assert A.vol(A._whole(A.MA_BIG)) > 4096 * 256


# ------------------------------------------------------------------ amplitude
@pytest.mark.parametrize("case", A.AMP_CASES, ids=[c["name"] for c in A.AMP_CASES])
def test_amplitude_many_claims_and_checks(case):
    A.amp_claims(case)
    ops = tops(case["dt"])
    st = A.run_amp_many(ops, case, CPU)
    A.check_amp_many(st)
    box = st["boxes"][0]
    nudge(st["amps"][0][box[0][0], box[0][1]], box[0][2])  # one wrong maximum
    bites(A.check_amp_many, st)
    st = A.run_amp_many(ops, case, CPU)
    st["counter"] += 1                                     # a count off by one
    bites(A.check_amp_many, st)
    st = A.run_amp_many(ops, case, CPU)
    c = next(i for i, b in enumerate(st["boxes"]) if A.vol(b) and b[1][2] % 4 and b[1][2] < case["nz"])
    b = st["boxes"][c]
    st["amps"][c][b[0][0], b[0][1], b[1][2]] = 0.5         # a store one cell past an unaligned hi.z
    bites(A.check_amp_many, st)
    if st["store"] is not None and A.case_ncomp(case) < 6:
        st = A.run_amp_many(ops, case, CPU)
        st["store"][0, 5, 0, 0] = 0.5                      # another component's plane
        bites(A.check_amp_many, st)


@pytest.mark.parametrize("case", A.AMP1_CASES, ids=[c["name"] for c in A.AMP1_CASES])
def test_amplitude_single_checks(case):
    ops = tops(case["dt"])
    st = A.run_amp_single(ops, case, CPU)
    A.check_amp_single(st)
    st["counts"][0] -= 1
    bites(A.check_amp_single, st)
    st = A.run_amp_single(ops, case, CPU)
    nudge(st["fields"][1], 3)
    bites(A.check_amp_single, st)


def test_amplitude_cases_cover_the_kernels():
    kernels = {c["kernel"] for c in A.AMP_CASES}
    assert kernels == {"v4", "many_f32", "many_f64"}
    f32s = [c for c in A.AMP_CASES if c["kernel"] == "many_f32"]
    assert any(c["nz"] % 4 for c in f32s) and any(c["nz"] % 4 == 0 and c["base"] == "odd" for c in f32s)
    assert {c["boxes"] for c in A.AMP_CASES} == {"six", "three"} and {c["form"] for c in A.AMP_CASES} == {
        "shared", "separate"}
    for nz in (70, 72):
        six = A.amp_boxes("six", nz)
        assert len(set(six)) == 6
        lay = A.YeeLayout(size=(A.AMP_NX, A.AMP_NY, nz))
        assert sum(b == lay.global_range(c) for b in six for c in A.COMPS) >= 3  # real Yee update boxes


@pytest.mark.parametrize("nz,ncomp", [(72, 6), (70, 6), (72, 3), (70, 3)])
def test_amplitude_inputs_have_no_ambiguous_cell(nz, ncomp):
    """The share of cells allowed to differ is zero: the torch backend decides
    identically on the fp32 and on the fp64 inputs, in every cell, for the
    first call and for the second one on fields scaled by 4, and as the
    draw's categories say."""
    f64, a64, change = A.amp_draw(nz, ncomp)
    whole = A._whole((A.AMP_NX, A.AMP_NY, nz))
    masks = {}
    for dt in ("f32", "f64"):
        ops = tops(dt)
        out = []
        for c in range(ncomp):
            f, a = f64[c].to(A.DT[dt]), a64[c].to(A.DT[dt]).clone()
            a0 = a.clone()
            n1 = ops.amplitude_update(f, a, whole, A.ACC)
            m1 = a != a0
            # a changed cell whose new maximum equals the old one cannot occur: growth > ACC
            assert int(m1.sum()) == n1
            a1 = a.clone()
            n2 = ops.amplitude_update(4 * f, a, whole, A.ACC)
            m2 = a != a1
            assert int(m2.sum()) == n2
            out.append((m1, m2))
        masks[dt] = out
    for c in range(ncomp):
        assert torch.equal(masks["f32"][c][0], masks["f64"][c][0]) and torch.equal(masks["f32"][c][1],
                                                                                   masks["f64"][c][1])
        assert torch.equal(masks["f64"][c][0], change[c])
        assert 0 < int(masks["f64"][c][1].sum()) < change[c].numel()
    # every category is there, and the growth of a decided cell is a factor 4 away from ACC
    v, a = f64.abs(), a64
    g = torch.where(a != 0, (v - a) / torch.where(a != 0, a, torch.ones_like(a)), torch.where(v != 0, 1.0, 0.0).double())
    up = v >= a
    assert bool(((g[up] >= 4 * A.ACC) | (g[up] <= A.ACC / 4)).all())
    assert bool((v == a).logical_and(a != 0).any()) and bool(((a == 0) & (v == 0)).any()) and bool(
        ((a == 0) & (v != 0)).any()) and bool((v < a).any())


# -------------------------------------------------------------------- sources
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_set_value_checks(dt):
    ops = tops(dt)
    for idx in A.SRC_CELLS:
        r = A.run_set_value(ops, dt, CPU, idx)
        A.check_cells(r)
        nudge(r["t"][idx[0], idx[1]], idx[2])  # the value rounded the wrong way
        bites(A.check_cells, r)
        r = A.run_set_value(ops, dt, CPU, idx)
        r["t"].view(-1)[(r["t"].view(-1) == A.SENT).nonzero()[0]] = 0.0  # a stray store
        bites(A.check_cells, r)
    for n in A.SET_VALUES_N:
        r = A.run_set_values(ops, dt, CPU, n)
        assert len(r["cells"]) == n
        A.check_cells(r)
        first = next(iter(r["cells"]))
        r["t"][first] = A.SENT  # a lost cell
        bites(A.check_cells, r)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_inc_step_e_checks(dt):
    ops = tops(dt)
    for n in A.INC_LENGTHS:
        r = A.run_inc_e(ops, dt, CPU, n, 0.1)
        A.check_inc_e(r)
        good = r["e"].clone()
        bound = A.inc_bound(dt, r["e0"].double(), r["h0"].double(), A.INC_COEF)
        r["e"][n - 1] += 4 * bound[n - 2]  # four bounds off
        bites(A.check_inc_e, r)
        r["e"] = good.clone()
        r["e"][0] = 0.2
        bites(A.check_inc_e, r)
        r["e"] = good
        nudge(r["h"], n - 1)
        bites(A.check_inc_e, r)
    assert {2, 255, 256, 257} <= set(A.INC_LENGTHS) and max(A.INC_LENGTHS) >= 1000


# ------------------------------------------------------------------ scattered
@pytest.mark.parametrize("case,dt", A._SC[0], ids=A._SC[1])
def test_scattered_claims_and_checks(case, dt):
    """check_scattered (which asserts the case's claims: inside and outside
    cells, border cells on L and R, the clamps, the sweeps) passes on the
    oracle rounded to the dtype and fails on a wrong inside cell, a touched
    outside cell and a changed input."""
    r = A.run_scattered(None, case, dt, CPU)
    A.check_scattered(r)
    if case["sweeps"] > 1:
        return  # the corruptions below are shown on the small cases (each costs an oracle of 16.8M cells here)
    o = A.scat_oracle(case, r["f0"], r["line0"])
    inside = tuple(int(v) for v in o["mask"].nonzero()[-1])
    outside = tuple(int(v) for v in (~o["mask"]).nonzero()[-1])
    good = r["got"][inside].clone()
    # 8 roundings of the larger operand off: past the bound of 2 (fp32) / ~45 (fp64: 1e-14) roundings
    scale = float(r["f0"][inside].abs() + o["inc"][inside].abs())
    r["got"][inside] = good + scale * (2.0 ** -20 if dt == "f32" else 2.0 ** -45)
    bites(A.check_scattered, r)
    r["got"][inside] = good
    r["got"][outside] = r["got"][outside] + 1.0
    bites(A.check_scattered, r)
    r["got"][outside] = r["f0"][outside]
    A.check_scattered(r)
    nudge(r["line"], 0)
    bites(A.check_scattered, r)


def test_scattered_cases_cover_the_issue():
    cs = A.SCAT_CASES
    assert {c["comp"] for c in cs} == set(A.COMPS) and {c["act"] for c in cs} == {7, 3, 1}
    assert any(c["dir"] == (1.0, 0.0, 0.0) for c in cs) and any(c["dir"] == (0.0, 1.0, 0.0) for c in cs)
    assert any(c["dir"] == A.OBLIQUE for c in cs) and all(any(c["org"]) for c in cs)
    assert any(c["clamps"] for c in cs) and any(c["sweeps"] > 1 for c in cs)
    geo, igeo = A.scat_geo(cs[3])
    assert len(geo) == 17 and len(igeo) == 4 and geo[16] == 0.5 and geo[:3] == list(A.MIN_COORD_FP["Hx"])
