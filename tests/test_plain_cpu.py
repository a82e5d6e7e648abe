"""CPU companion of tests/test_plain_gpu.py: conditions on its inputs, checked on the oracle alone.

The windows, launches, states and tolerances come from that module (one shared
list, so the GPU tests cannot be launched on a box these checks did not see):
every box passes the HIP backend's host-side stencil check, the 3D windows
reach every row layout of the float4 kernels, the measured ``E32`` constants
still hold, and every launch is live -- zeroing the old value of the updated
field, replacing the per-cell coefficient by its scalar or zeroing the x
neighbour plane moves the oracle's result by more than ``LIVE`` tolerances on
the cells that read the operand.
"""
import types

import pytest

import test_plain_gpu as P
from fdtd3d_amd.ops.hip_ops import HipError, HipOps


@pytest.mark.parametrize("grid", list(P.GRIDS))
def test_boxes_pass_the_stencil_check(grid):
    cs = P.case(grid)
    host = types.SimpleNamespace(layout=cs.layout)
    n = 0
    for launch in P.all_launches(grid):
        for kind, c, b in launch.stencil_boxes():
            HipOps._check_stencil_box(host, kind, c, b, cs.size)
            n += 1
    assert n > 0
    # (the check itself refuses a box that reads outside the array)
    c = cs.E[-1]
    with pytest.raises(HipError):
        HipOps._check_stencil_box(host, "E", c, ((0, 0, 0), cs.size), cs.size)


def test_split_windows_reach_every_layout():
    """8, 16 and 64 lanes per z row, each with blockIdx.x > 0, for E and for H."""
    seen = {"E": set(), "H": set()}
    for grid in P.GRIDS3:
        cs = P.case(grid)
        if cs.size[2] % 4:
            continue
        for launch in P.split_launches(cs):
            lz, blocks = P.layout_of(launch)
            seen[launch.kind].add((lz, blocks > 1))
    for kind in "EH":
        assert seen[kind] >= {(lz, many) for lz in (8, 16, 64) for many in (False, True)}, (kind, seen[kind])
    # the named windows land where their comments say
    cs = P.case("a240")
    lay = {(l.name, l.kind): P.layout_of(l) for l in P.split_launches(cs)}
    for kind in "EH":
        assert lay[("whole", kind)] == (64, 1) and lay[("zlo1", kind)] == (8, 1) and lay[("zhi", kind)] == (8, 1)
        assert lay[("lz8-two", kind)] == (8, 2) and lay[("lz16", kind)] == (16, 1) and lay[("lz16-two", kind)] == (16, 2)
    assert P.layout_of(P.split_launches(P.case("b440"))[0]) == (64, 2)


def test_window_shapes():
    """The windows are what their names say."""
    for grid in P.GRIDS3:
        cs = P.case(grid)
        nx, ny, nz = cs.size
        W = P.windows3(cs)
        for kind in "EH":
            b = [W["interior"][c] for c in cs.names(kind)]
            for d in range(3):
                assert len({x[0][d] for x in b}) == 3 or len({x[1][d] for x in b}) == 3
            assert all(x[0][2] % 4 and x[1][2] % 4 for x in b)
            assert sum(P._empty(W["one-empty"][c]) for c in cs.names(kind)) == 1
            xs = sorted((W["xsplit"][c][0][0], W["xsplit"][c][1][0]) for c in cs.names(kind))
            assert all(a[1] <= b_[0] for a, b_ in zip(xs, xs[1:]))
            assert all(P._union(W["zlo1"][c] for c in cs.names(kind))[q][2] == v for q, v in ((0, 1), (1, 30)))
            zh = P._union(W["zhi"][c] for c in cs.names(kind))
            assert zh[1][2] == nz and zh[1][2] - (zh[0][2] & ~3) <= 32
        assert W["xends"]["Ex"][0][0] == 0 and W["xends"]["Hx"][1][0] == nx
        for c in cs.comps:
            assert W["xplane"][c][1][0] - W["xplane"][c][0][0] == 1 and W["yrow"][c][1][1] - W["yrow"][c][0][1] == 1
            z = W["zcell"][c]
            assert z[1][2] - z[0][2] == 1 and z[0][2] % 4 not in (0, 3)


def test_multi_windows():
    """11 windows (8 + 3) after the empty ones are dropped, one with an empty
    component box, and automatic x chunks that differ once the knob is set."""
    for grid in ("tmz", "tez"):
        cs = P.case(grid)
        for kind in "EH":
            launch = P.multi_launch(cs, kind)
            names = cs.names(kind)
            wins = [w for w in launch.windows if not all(P._empty(w[c]) for c in names)]
            assert len(launch.windows) > len(wins) == 11
            if len(names) == 2:
                assert any(sum(P._empty(w[c]) for c in names) == 1 for w in wins)
            unions = [P._union(w.values()) for w in wins]
            assert {P.xchunk2d(b) for b in unions} == {1}
            xc = [P.xchunk2d(b, P.MULTI_WGS) for b in unions]
            assert len(set(xc)) >= 3 and len(set(xc[:8])) >= 3 and xc[8] != xc[0], xc
            launch.mask(cs, names[0])  # (asserts that the windows are disjoint)


def test_e32_constants():
    """The E32 tables are what TorchOps in float32 gives against the oracle."""
    assert set(P.E32) == set(P.e32_keys())
    for key in P.e32_keys():
        family, grid, cset, kind = key
        got = P.measure_e32(grid, family, cset, kind)
        print("e32", key, "%.4g" % got)
        assert 0.8 * got <= P.E32[key] <= 1.25 * got, (key, P.E32[key], got)
    for key, want in P.E32_TFSF.items():
        got = P.measure_e32_tfsf(*key)
        print("e32 tfsf", key, "%.4g" % got)
        assert 0.8 * got <= want <= 1.25 * got, (key, want, got)
    assert set(P.E32_TFSF) == {(op, kind) for op in P.TFSF_OPS for kind in "EH"}


@pytest.mark.parametrize("grid", list(P.GRIDS))
def test_coefficient_varies_in_every_box(grid):
    """The per-cell coefficient differs between the cells of every box of
    every launch, along x or y: a wrong index in its load cannot pass."""
    cs = P.case(grid)
    for launch in P.all_launches(grid):
        boxes = P.coef_boxes(launch)
        flat = [P.coef_varies(cs, c, b) for c, b in boxes]
        if isinstance(launch, P.Multi):
            # (the windows of one table share a kernel; the narrow ones lie beside the sphere)
            assert sum(flat) >= 4, (grid, launch.name, launch.kind, flat)
        else:
            assert all(flat), (grid, launch.name, launch.kind, [cb for cb, ok in zip(boxes, flat) if not ok])
    if cs.scheme == "3d":
        # ... and on the halo columns where the fused tests place the source, past the first tile
        for c in cs.comps:
            for z in [64, 69, 104] + ([256, 296] if cs.size[2] > 300 else []):
                plane = cs.cell[c][:, :, z]
                assert float(plane.min()) != float(plane.max()), (grid, c, z)


def _csets(launch):
    if launch.fused:
        return ("scalar", "cellE", "cellH", "cellEH")
    return ("scalar", "cell" + launch.kind)


@pytest.mark.parametrize("grid", list(P.GRIDS))
def test_launches_are_live(grid):
    cs = P.case(grid)
    worst = {}
    for launch in P.all_launches(grid):
        if "@v4-7" in launch.name and not launch.name.split("@")[0].endswith("halo"):
            continue  # (the same boxes and source as the scalar form's launch)
        for cset in _csets(launch):
            want = P.oracle(cs, launch, cset)
            for name, live in P.liveness(cs, launch, cset, want).items():
                assert live is not None, (grid, launch.name, launch.kind, cset, name, "no cell reads the operand")
                worst[name] = min(worst.get(name, float("inf")), live)
                assert live > P.LIVE, (grid, launch.name, launch.kind, cset, name, "launch not live", live)
    print("live", grid, " ".join("%s %.3g" % kv for kv in worst.items()))
    assert set(worst) == {"old", "cell", "x-neighbour"}
