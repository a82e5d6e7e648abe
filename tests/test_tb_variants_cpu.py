"""CPU companion of tests/test_tb_variants_gpu.py: conditions on its cases,
checked on the torch oracle alone.

The case tables, inputs, oracles and checks come from that module (one shared
set, so the GPU tests cannot run a case these checks did not see):

* every case has the tiles it claims and meets the preconditions the HIP
  wrappers state (their own validation needs device tensors);
* every fp32 case is well conditioned: the torch oracle in float32 stays
  within HALF the fp32 bound of the fp64 oracle, through the same check code
  the GPU tests run (sentinels and untouched inputs included);
* the ambiguous amplitude cells are at most 0.5 % of the cells inside the
  amplitude boxes, per case;
* every case is live: a small deliberate error on the oracle side -- the
  Drude box shifted by one cell, the ids of two components swapped, the m2
  term dropped, the amplitude boxes shifted by one, ``level0`` off by one, a
  TF/SF table dropped -- moves the result by at least ``LIVE`` = 100 times the
  bound the GPU test uses.
"""
import pytest
import torch

import test_tb_variants_gpu as V
from fdtd3d_amd.ops.torch_ops import _empty, box_intersect_

LIVE = 100.0
HALF32 = 0.5 * V.BOUND32


def _inside(box, lo, hi):
    return all(lo[d] <= box[0][d] <= box[1][d] <= hi[d] for d in range(3))


def _moved(base, other, sent):
    """Largest change per kind between two oracle results, on the kind's scale."""
    sc = V.kind_scales(base, sent)
    out = {"E": 0.0, "H": 0.0}
    for c in V.COMPS:
        out[c[0]] = max(out[c[0]], float((base[c] - other[c]).abs().max()) / sc[c[0]])
    return out


# -------------------------------------------------------------------- Drude
@pytest.mark.parametrize("name", list(V.DRUDE))
def test_drude_case_is_valid(name):
    """tb_drude_step's preconditions (ops/hip_ops.py, fdtd_tb3d_drude_f32 / _f64)."""
    cs, inp = V.DRUDE[name], V.drude_inputs(name)
    g32, g64 = V.drude_claims(name)
    assert g32[0] >= 2 and g64[2] >= g32[2]
    assert 1 <= cs.T <= 5 and cs.size[2] % 4 == 0
    B, size = inp["B"], cs.size
    assert not _empty(B) and _inside(B, (0, 0, 0), size) and _inside(inp["obox"], (0, 0, 0), size)
    for c in V.E:
        assert _inside(B, *inp["upd"][c]), (name, c, "Drude box outside the update box")
    assert all(_inside(b, (0, 0, 0), size) for b in inp["upd"].values())
    assert tuple(inp["lut"].shape) == (3, inp["lut"].shape[1], 4) and inp["lut"].shape[1] <= 256
    ids = inp["ids"]
    assert int(((ids >> 24) & 0xff).max()) == 0
    for q in range(3):
        assert int(((ids >> (8 * q)) & 0xff).max()) < inp["lut"].shape[1]
    if inp["src"] is not None:
        comp, idx = inp["src"][0][0], inp["src"][0][1]
        assert comp in V.E and all(0 <= idx[d] < size[d] for d in range(3))
        assert all(s[0] == comp and s[1] == idx for s in inp["src"])
    if not cs.plan:
        # live by construction: the three ids of a cell differ wherever none took the plain row,
        # every row is used, the plain row sits on a scattered subset, the LUT rows are tame
        q = [(ids >> (8 * n)) & 0xff for n in range(3)]
        disp = (q[0] < 4) & (q[1] < 4) & (q[2] < 4)
        assert bool(((q[0] != q[1]) & (q[1] != q[2]))[disp].all())
        for n in range(3):
            frac = float((q[n] == 4).double().mean())
            assert 0.05 < frac < 0.3, (name, n, frac)
            assert set(q[n].unique().tolist()) == {0, 1, 2, 3, 4} or min(ids.shape) == 1
        lut = inp["lut"]
        cb = float(lut[0, 4, 0])
        assert float(lut[..., 2].abs().max()) <= 2 and float(lut[..., 3].abs().max()) <= 1
        assert float((lut[..., 1] * inp["cbd"]).abs().max()) <= 0.3 * cb * 1.001
        assert torch.equal(lut[:, 4], torch.tensor([cb, 0.0, 1.0, 0.0], dtype=torch.float64).expand(3, 4))
    # the source is where the case says
    assert (cs.src is None) == (cs.src_at == "")
    if cs.src is not None:
        idx = cs.src[1]
        in_b = all(B[0][d] <= idx[d] < B[1][d] for d in range(3))
        on_face = in_b and any(idx[d] in (B[0][d], B[1][d] - 1) for d in range(3))
        in_o = all(inp["obox"][0][d] <= idx[d] < inp["obox"][1][d] for d in range(3))
        assert in_o and cs.src_at == ("halo" if not in_b else "face" if on_face else "inside"), (name, cs.src_at)
    assert {c.src_at for c in V.DRUDE_CASES} == {"", "inside", "face", "halo"}
    if cs.obox != "serial":
        ob = box_intersect_(B, inp["obox"])
        assert not _empty(ob) and ob != B, (name, "obox does not cut the Drude box")


@pytest.mark.parametrize("name", list(V.DRUDE))
def test_drude_case_is_conditioned(name):
    dut, _ = V.pair(V.drude_cfg(V.DRUDE[name]), "f32", "cpu", "torch")
    out = V.drude_run(name, dut, "cpu", torch.float32)
    worst = V.drude_check(name, out, torch.float32, HALF32, id_bits=False)
    print("conditioning drude %s: %.3g of the fp32 bound" % (name, worst / V.BOUND32))


@pytest.mark.parametrize("name", list(V.DRUDE))
def test_drude_case_is_live(name):
    base = V.drude_oracle(name)
    for mutate in ("shift-B", "swap-ids", "no-m2"):
        other = V.drude_oracle(name, mutate)
        mv = _moved(base["fout"], other["fout"], base["sent"])
        print("live drude %s %s: E %.3g H %.3g" % (name, mutate, mv["E"], mv["H"]))
        assert mv["E"] >= LIVE * V.BOUND32, (name, mutate, mv)
    # the state leaves with the pass: both arrays are written on obox ∩ B, and only there
    for n in range(2):
        wrote = (base["sout"][n] != base["ssent"][n]).any(-1)
        ob = box_intersect_(base["B"], base["obox"])
        assert int(wrote.sum()) == (ob[1][0] - ob[0][0]) * (ob[1][1] - ob[0][1]) * (ob[1][2] - ob[0][2])


# ---------------------------------------------------------------- amplitude
@pytest.mark.parametrize("name", list(V.AMP))
def test_amp_case_is_valid(name):
    """tb_amp_step's preconditions and what the case's comment says."""
    cs, inp = V.AMP[name], V.amp_inputs(name)
    size = V.AMP_SIZE
    for shape in ("mr16x2", "mr8x4"):
        V.assert_tiles(shape, cs.T, cs.obox, cs.claim)
    assert 1 <= cs.T <= 3 and size[2] % 4 == 0 and 6 * size[1] * size[2] * 4 < 2 ** 28
    assert _inside(cs.obox, (0, 0, 0), size)
    boxes = [b for b in cs.aboxes if not _empty(b)]
    assert all(_inside(b, (0, 0, 0), size) and b[1][0] < 65536 for b in boxes)
    assert len(boxes) >= 5 and len(set(boxes)) >= 2, "at most one empty box, boxes that differ"
    assert all(_inside(b, *V.INNER) for b in boxes), "amplitude boxes keep off the faces"
    if cs.obox != V.WHOLE:
        assert any(_inside(b, *cs.obox) for b in boxes) and any(not _inside(b, *cs.obox) for b in boxes)
    if cs.line is not None:
        comp, i, j, k0, k1 = cs.line
        assert comp in V.E and 0 <= i < size[0] and 0 <= j < size[1] and 0 <= k0 < k1 <= size[2]
        assert _inside(((i, j, k0), (i + 1, j + 1, k1)), *cs.obox)
    # the line is what the case says
    sz = V.seams("mr16x2", cs.T, cs.obox)[2]
    assert (cs.line is None) == (cs.line_is == ())
    if cs.line is not None:
        is_ = (("seam",) if any(cs.line[3] < q < cs.line[4] for q in sz) else ()) \
            + (("cell",) if cs.line[4] - cs.line[3] == 1 else ()) \
            + (("outside",) if cs.line[4] > inp["upd"][cs.line[0]][1][2] else ())
        assert is_ == cs.line_is, (name, is_, cs.line_is, sz)
    assert {t for c in V.AMP_CASES for t in c.line_is} == {"seam", "cell", "outside"}
    assert sum(c.line is None for c in V.AMP_CASES) >= 2 and sum(_empty(b) for c in V.AMP_CASES for b in c.aboxes) >= 6
    assert {c.acc for c in V.AMP_CASES} == {V.ACCURACY, 0.05}
    a = inp["amp"]
    assert 0.15 < float((a == 0).double().mean()) < 0.25
    for n, c in enumerate(V.COMPS):
        big = 10 * float(inp["fin"][c].abs().max())
        assert 0.1 < float((a[:, n] > big).double().mean()) < 0.2, (name, c)


@pytest.mark.parametrize("name", list(V.AMP))
def test_amp_case_ambiguity_cap(name):
    """At most 0.5 % of the cells inside the amplitude boxes are ambiguous,
    and the pass changes maxima at every level (the counts are live)."""
    cs = V.AMP[name]
    _, ever, inbox, _ = V.amp_ambiguous(name)
    n, tot = int(ever.sum()), int(inbox.sum())
    print("ambiguous %s: %d of %d cells (%.3f %%)" % (name, n, tot, 100.0 * n / tot))
    assert tot > 10000 and n <= 0.005 * tot, (name, n, tot)
    want = V.amp_oracle(name)
    for l in range(cs.T):
        assert int(want["counts"][l]) - V.AMP_COUNTS0[l] > 100, (name, l, want["counts"])


@pytest.mark.parametrize("name", list(V.AMP))
def test_amp_case_is_conditioned(name):
    dut, _ = V.pair(V.amp_cfg(), "f32", "cpu", "torch")
    out = V.amp_run(name, dut, "cpu", torch.float32)
    worst = V.amp_check(name, out, torch.float32, HALF32)
    print("conditioning amp %s: %.3g of the fp32 bound" % (name, worst / V.BOUND32))


@pytest.mark.parametrize("name", list(V.AMP))
def test_amp_case_is_live(name):
    """The amplitude boxes shifted by one row: the maxima and the counts move."""
    cs = V.AMP[name]
    base, other = V.amp_oracle(name), V.amp_oracle(name, True)
    sc = V.kind_scales(base["fout"], base["sent"])
    moved = 0
    for n, c in enumerate(V.COMPS):
        if _empty(cs.aboxes[n]):
            continue
        d = float((base["amp"][:, n] - other["amp"][:, n]).abs().max()) / sc[c[0]]
        moved += d >= LIVE * V.BOUND32
    assert moved >= 3, (name, moved)
    assert any(int(base["counts"][l]) != int(other["counts"][l]) for l in range(cs.T))


# -------------------------------------------------------------------- TF/SF
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("inc", list(V.TF_INC))
def test_tfsf_pass_is_conditioned(inc, T):
    dut, ref = V.pair(V.tf_cfg(inc), "f32", "cpu", "torch")
    short = V.tf_short_reach(inc)
    assert int(ref.tfsf_sets.i0.max()) + 1 <= short < ref.inc_len
    assert ref.tfsf_sets.n_e > 0 and ref.tfsf_sets.n_h > 0
    for dry in (False, True):
        for sh in (False, True):
            got = V.tf_pass_run(inc, T, dry, sh, dut, "cpu", torch.float32)
            V.tf_pass_check(inc, T, dry, sh, got, HALF32)
    # the line moves and the levels differ: a table of the wrong level cannot pass
    want = V.tf_pass_oracle(inc, T, False, False)
    e0, h0, _ = V.tf_lines(inc, 0)
    assert float((want[1] - e0).abs().max()) > 0.1 * float(e0.abs().max())
    for l in range(1, T):
        assert float((want[0][l] - want[0][l - 1]).abs().max()) > 0.1 * float(want[0][l].abs().max())


@pytest.mark.parametrize("name", list(V.TF))
def test_tfsf_step_case_is_valid(name):
    cs = V.TF[name]
    ref = V.scheme(V.tf_cfg(cs.inc), "torch", "cpu", torch.float64)
    assert 1 <= cs.T <= 5 and cs.T + cs.level0 <= 8 and V.TF_SIZE[2] % 4 == 0
    assert _inside(cs.obox, (0, 0, 0), V.TF_SIZE)
    families = ("mr16x2",) if cs.sparse else ("mr16x2", "f64half", "f64full")
    for family in families:
        claim = cs.claim if family != "f64full" else (cs.claim[0], cs.claim[1], 1)
        V.assert_tiles(family, cs.T, cs.obox, claim)
        cut = V.tf_straddles(cs, family)
        assert cut[0] and cut[1] and (cut[2] or claim[2] == 1), (name, family, cut)
    if cs.sparse:
        # the per-cell box keeps clear of every TF/SF target: the stepped tables hold the scalar Cb
        grown = V.grow(V.TF_SPARSE_BOX, 1, V.TF_SIZE)
        for s in ref.tfsf_sets.sets:
            assert _empty(box_intersect_((s["lo"], s["hi"]), grown)), (name, s)
        sm = V.seams("mr16x2", cs.T, cs.obox)
        assert all(any(V.TF_SPARSE_BOX[0][d] < q < V.TF_SPARSE_BOX[1][d] for q in sm[d]) for d in range(2))
    if cs.obox != V.TF_WHOLE:
        # the sub-box cuts through faces: some set lies partly inside it
        part = [s for s in ref.tfsf_sets.sets
                if not _empty(box_intersect_((s["lo"], s["hi"]), cs.obox)) and not _inside((s["lo"], s["hi"]), *cs.obox)]
        assert len(part) >= 2, (name, len(part))
    assert {c.level0 > 0 for c in V.TF_CASES} == {False, True}
    assert {c.sparse for c in V.TF_CASES} == {"", "E", "H", "EH"}


@pytest.mark.parametrize("name", list(V.TF))
def test_tfsf_step_case_is_conditioned_and_live(name):
    cs = V.TF[name]
    dut, _ = V.pair(V.tf_cfg(cs.inc), "f32", "cpu", "torch")
    out = V.tf_step_run(name, dut, "cpu", torch.float32)
    base = V.tf_step_oracle(name)
    worst, _ = V.check_fields(out["fout"], base["fout"], out["sent"], torch.float32, HALF32, (name,))
    print("conditioning tfsf step %s: %.3g of the fp32 bound" % (name, worst / V.BOUND32))
    probes = [("drop-set", V.tf_step_oracle(name, 0, True))]
    if cs.T + cs.level0 < 8:
        probes.append(("level0+1", V.tf_step_oracle(name, 1, False)))
    if cs.level0 > 0:
        probes.append(("level0-1", V.tf_step_oracle(name, -1, False)))
    assert len(probes) >= 2
    for what, other in probes:
        mv = _moved(base["fout"], other["fout"], base["sent"])
        print("live tfsf %s %s: E %.3g H %.3g" % (name, what, mv["E"], mv["H"]))
        assert max(mv.values()) >= LIVE * V.BOUND32, (name, what, mv)
    if cs.sparse:
        # ... and the per-cell coefficients matter
        mv = _moved(base["fout"], V.tf_step_oracle(name, 0, False, True)["fout"], base["sent"])
        assert max(mv.values()) >= LIVE * V.BOUND32, (name, "scalar coefficients", mv)
        cbs = V.tf_sparse_cb(cs, dut, "cpu", torch.float32)
        assert sum(cbs[c].cell is not None for c in V.COMPS) == 2 * len(cs.sparse)


# -------------------------------------------------------------------- plain
@pytest.mark.parametrize("name", list(V.PLAIN))
def test_plain_case_is_conditioned(name):
    _, T, obox, claim = V.PLAIN[name]
    for family in ("mr16x2", "single", "f64half"):
        V.assert_tiles(family, T, obox, V.plain_claim(family, claim))
    assert 1 <= T <= 4 and V.PLAIN_SIZE[2] % 4 == 0 and _inside(obox, (0, 0, 0), V.PLAIN_SIZE)
    dut, _ = V.pair(V.vacuum_cfg(V.PLAIN_SIZE, "f64"), "f32", "cpu", "torch")
    out = V.plain_run(name, dut, "cpu", torch.float32)
    want = V.plain_oracle(name)
    V.check_fields(out["fout"], want["fout"], out["sent"], torch.float32, HALF32, (name,))
    # the oracle wrote the whole output box of every component (as the kernels do), nothing else;
    # outside a component's update box the cells carry their input value
    n = (obox[1][0] - obox[0][0]) * (obox[1][1] - obox[0][1]) * (obox[1][2] - obox[0][2])
    for c in V.COMPS:
        assert int((want["fout"][c] != want["sent"][c]).sum()) == n
