"""Plain per-step Yee kernels against the fp64 torch oracle on live windows.

The other GPU suites reach the split E / H kernels, the fused E+H step and the
2D / 1D kernels through whole runs from zero fields (most cells then hold field
orders below the run tolerance, on whole-grid boxes only) or compare HIP with
HIP.  Here every component of E and H carries seeded random values of working
size (H at the size E / (2 cb), so old value and increment weigh alike), the
reference is ``TorchOps`` in float64 on the CPU, and the launches are windows
chosen to land in every launch form:

* ``ops.curl_update`` in 3D (``test_split_windows``): ``k_update_e3d_v4`` /
  ``k_update_h3d_v4`` of yee3d_v4.hip in their 8-, 16- and 64-lane row layouts
  with one and with several workgroups along z, ``k_update_e3d`` /
  ``k_update_h3d`` of yee3d.hip in fp32 and fp64, per-component boxes that
  differ on every axis, are empty, one cell thick or disjoint in x, x chunks of
  2 (auto), 3 and 16 planes;
* ``ops.fused_step`` (``test_fused``): ``k_fused3d_v4`` with 3 and 7 owned rows,
  ``k_fused3d`` in fp32 and fp64, into a ``fout`` prefilled with a sentinel, on
  whole boxes, a sub-box, and an interior box followed by the shell around it
  (six slab launches) and a launch whose union box covers all of that while
  its component boxes lie outside it, with the point source absent, inside a tile, on a tile's
  z halo column and on its halo row;
* the 2D / 1D kernels of yee_lowdim.hip (``test_lowdim_windows``) and the
  ``Win2`` multi-window launch (``test_lowdim_multi``: 11 windows in 8 + 3, empty
  ones dropped, x chunks that differ from window to window);
* ``tfsf_apply`` / ``tfsf_apply_many`` / ``inc_step_e`` / ``inc_step_h``
  (``test_tfsf_ops``).

Inside each component's box the result is within tolerance of the oracle; every
other cell of the updated fields is bit-identical to the input (to the sentinel
for ``fout``), and the source fields are bit-identical to the input.  The
companion tests/test_plain_cpu.py checks on the oracle alone that every window
passes the host's stencil check, reaches the layouts named above and is live:
zeroing the old value, replacing the per-cell coefficient by its scalar or
zeroing the x neighbour plane (the one the kernels carry in registers) moves
the result by more than ``LIVE`` tolerances.

Tolerances are measured: ``e32`` is the error of the same whole-box half step
(fused step) through ``TorchOps`` in float32 against the float64 oracle from the
same state, scaled by the oracle's largest value of the kind.  fp32 HIP gets
``4 e32`` (FMA contraction, another order of the sums), never more than the
run-level 2e-5; fp64 HIP gets that times eps64 / eps32.

Not covered here: the masked float4 stores (``st4m``) protect a neighbouring
launch on another stream; with one stream an unmasked store writes back what it
loaded, so no deterministic test tells the two apart, and a race of two
streams passes or fails by chance.  test_native_gpu.py[3d_upml_tfsf_hybrid-f32]
remains the guard of that.  The blocked kernels and the fp64 double4 lanes
(test_cpml_gpu.py::test_f64_plain_windows) have their own tests.
"""
import pytest
import torch

from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.coef import Coef
from fdtd3d_amd.ops.torch_ops import TorchOps, _shift

pytestmark = pytest.mark.gpu

TD = {"f32": torch.float32, "f64": torch.float64}
EPS_RATIO = 2.0 ** -52 / 2.0 ** -23
EMPTY = ((0, 0, 0), (0, 0, 0))
SEED = 9
LIVE = 100.0  # every control moves the result by more than LIVE x tolerance
XCHUNKS = (0, 3, 16)  # auto (2 planes on these grids; the fused kernels: 16 / 32), odd with a short last chunk, one seam
SRC_VAL = 1.75

# (scheme, size, sphere centre, radius).  nz = 240: the smallest multiple of 4 at which a whole-row window takes
# the 64-lane layout; nz = 440: such a window spans two 64-lane workgroups; nz - 2: no multiple of 4, fp32 on the
# scalar kernels.  In 3D the sphere lies inside the first ZPERIOD planes, and the per-cell coefficients repeat those
# planes along z, mirrored in x and y on every other period (Case): a surface then cuts every window, every
# workgroup along z and the fused kernels' halo columns, and the coefficient varies in x, y and z inside each.
ZPERIOD = 20
GRIDS = {
    "a240": ("3d", (20, 22, 240), (8.5, 9.5, 10.5), 7.5),
    "b440": ("3d", (10, 13, 440), (4.5, 5.5, 10.5), 7.5),
    "a238": ("3d", (20, 22, 238), (8.5, 9.5, 10.5), 7.5),
    "b438": ("3d", (10, 13, 438), (4.5, 5.5, 10.5), 7.5),
    # rows of three 64-lane blocks, the last one short; the sphere cuts the one-row and the one-column window
    "tmz": ("tmz", (40, 150, 1), (20.5, 75.5, 0.5), 15.0),
    "tez": ("tez", (40, 150, 1), (20.5, 75.5, 0.5), 15.0),
    "1d": ("1d", (300, 1, 1), (150.5, 0.5, 0.5), 60.0),
}
GRIDS3 = ("a240", "b440", "a238", "b438")

# e32 per (family, grid, coefficient set, kind): see the module docstring.  test_plain_cpu.py::test_e32_constants
# re-measures them.
E32 = {
    ("split", "a240", "scalar", "E"): 1.048e-07, ("split", "a240", "cellE", "E"): 1.071e-07,
    ("split", "a240", "scalar", "H"): 1.032e-07, ("split", "a240", "cellH", "H"): 1.037e-07,
    ("fused", "a240", "scalar", "E"): 1.048e-07, ("fused", "a240", "scalar", "H"): 1.815e-07,
    ("fused", "a240", "cellE", "E"): 1.071e-07, ("fused", "a240", "cellE", "H"): 1.889e-07,
    ("fused", "a240", "cellH", "E"): 1.048e-07, ("fused", "a240", "cellH", "H"): 1.889e-07,
    ("fused", "a240", "cellEH", "E"): 1.071e-07, ("fused", "a240", "cellEH", "H"): 1.889e-07,
    ("split", "b440", "scalar", "E"): 1.068e-07, ("split", "b440", "cellE", "E"): 1.101e-07,
    ("split", "b440", "scalar", "H"): 1.094e-07, ("split", "b440", "cellH", "H"): 1.078e-07,
    ("fused", "b440", "scalar", "E"): 1.068e-07, ("fused", "b440", "scalar", "H"): 1.682e-07,
    ("fused", "b440", "cellE", "E"): 1.101e-07, ("fused", "b440", "cellE", "H"): 1.647e-07,
    ("fused", "b440", "cellH", "E"): 1.068e-07, ("fused", "b440", "cellH", "H"): 1.719e-07,
    ("fused", "b440", "cellEH", "E"): 1.101e-07, ("fused", "b440", "cellEH", "H"): 1.647e-07,
    ("split", "a238", "scalar", "E"): 1.146e-07, ("split", "a238", "cellE", "E"): 1.146e-07,
    ("split", "a238", "scalar", "H"): 1.086e-07, ("split", "a238", "cellH", "H"): 9.858e-08,
    ("fused", "a238", "scalar", "E"): 1.146e-07, ("fused", "a238", "scalar", "H"): 1.918e-07,
    ("fused", "a238", "cellE", "E"): 1.146e-07, ("fused", "a238", "cellE", "H"): 1.854e-07,
    ("fused", "a238", "cellH", "E"): 1.146e-07, ("fused", "a238", "cellH", "H"): 1.918e-07,
    ("fused", "a238", "cellEH", "E"): 1.146e-07, ("fused", "a238", "cellEH", "H"): 1.854e-07,
    ("split", "b438", "scalar", "E"): 9.503e-08, ("split", "b438", "cellE", "E"): 1.029e-07,
    ("split", "b438", "scalar", "H"): 1.065e-07, ("split", "b438", "cellH", "H"): 1.069e-07,
    ("fused", "b438", "scalar", "E"): 9.503e-08, ("fused", "b438", "scalar", "H"): 1.555e-07,
    ("fused", "b438", "cellE", "E"): 1.029e-07, ("fused", "b438", "cellE", "H"): 1.711e-07,
    ("fused", "b438", "cellH", "E"): 9.503e-08, ("fused", "b438", "cellH", "H"): 1.711e-07,
    ("fused", "b438", "cellEH", "E"): 1.029e-07, ("fused", "b438", "cellEH", "H"): 1.711e-07,
    ("split", "tmz", "scalar", "E"): 6.553e-08, ("split", "tmz", "cellE", "E"): 6.553e-08,
    ("split", "tmz", "scalar", "H"): 9.577e-08, ("split", "tmz", "cellH", "H"): 9.577e-08,
    ("split", "tez", "scalar", "E"): 7.096e-08, ("split", "tez", "cellE", "E"): 7.096e-08,
    ("split", "tez", "scalar", "H"): 1.002e-07, ("split", "tez", "cellH", "H"): 1.002e-07,
    ("split", "1d", "scalar", "E"): 5.788e-08, ("split", "1d", "cellE", "E"): 5.788e-08,
    ("split", "1d", "scalar", "H"): 6.445e-08, ("split", "1d", "cellH", "H"): 6.445e-08,
}
# Tolerances from these: fp32 2.3e-7 .. 4.6e-7 for the split and 2D / 1D kernels, 3.8e-7 .. 7.7e-7 for the fused step;
# fp64 those times 2^-29.
# Observed on the MI355X, largest error / scale over all windows, grids and coefficient sets (E, H; fp64 figures
# divided by 2^-29, to read against the same e32):
#   k_update_e3d_v4 / k_update_h3d_v4      fp32 9.4e-8, 8.8e-8
#   k_update_e3d / k_update_h3d            fp32 1.0e-7, 8.8e-8    fp64 8.7e-8, 6.7e-8
#   k_fused3d_v4 (3 and 7 rows)            fp32 9.4e-8, 1.6e-7
#   k_fused3d                              fp32 1.0e-7, 1.6e-7    fp64 8.7e-8, 2.3e-7
#   2D / 1D single windows and Win2        fp32 6.3e-8, 8.4e-8    fp64 8.9e-8, 1.0e-7
#   tfsf_apply / _many / inc_step_e / _h   fp32 6.6e-8            fp64 1.7e-16 (absolute / scale)
# No case exceeds 1.5 e32.  Smallest liveness ratio on the oracle (test_plain_cpu.py): 2.0e5.


def _sl(box):
    return tuple(slice(box[0][d], box[1][d]) for d in range(3))


def _empty(b):
    return any(b[1][d] <= b[0][d] for d in range(3))


def _kind(c):
    return c[0]


def _union(boxes):
    bs = [b for b in boxes if not _empty(b)]
    if not bs:
        return EMPTY
    return (tuple(min(b[0][d] for b in bs) for d in range(3)), tuple(max(b[1][d] for b in bs) for d in range(3)))


def _clip(b, w):
    r = (tuple(max(b[0][d], w[0][d]) for d in range(3)), tuple(min(b[1][d], w[1][d]) for d in range(3)))
    return EMPTY if _empty(r) else r


class NoXNeighbour(TorchOps):
    """The oracle with the x neighbour operand of every curl zeroed: plane
    x - 1 of the E update, x + 1 of the H update (a control)."""

    def curl(self, kind, comp, sl, src):
        acc = None
        for (s, axis, sign) in self.layout.curl_terms(comp):
            S = src[s]
            nb = S[_shift(sl, axis, -1 if kind == "E" else +1)]
            if axis == 0:
                nb = torch.zeros_like(nb)
            d = S[sl] - nb if kind == "E" else nb - S[sl]
            if acc is None:
                acc = d if sign > 0 else -d
            else:
                acc = acc + d if sign > 0 else acc - d
        return acc


class Case:
    """The CPU part of a grid: layout, whole boxes, scalar and per-cell
    coefficients, the start state (float64 values rounded to float32)."""

    def __init__(self, name):
        scheme, size, centre, radius = GRIDS[name]
        cfg = SchemeConfig(scheme=scheme, size=size, time_steps=1, scene="sphere", sphere_radius=radius,
                           sphere_center=centre, dtype="f64", hybrid_block=1)
        s = YeeScheme(cfg, make_ops("torch", None, "cpu", torch.float64))
        s.init_scheme()
        s.init_grids()
        self.name, self.scheme, self.size, self.layout = name, scheme, size, s.layout
        self.comps, self.E, self.H = tuple(s.comps), tuple(s.e_comps), tuple(s.h_comps)
        self.whole = {c: s.local_box(c) for c in self.comps}
        self.scalar = {c: s.cb[c].scalar for c in self.comps}
        cells = [s.cb[c].cell for c in self.E]
        assert all(v is not None and 0 < int((v != 1).sum()) < v.numel() for v in cells), "the scene gives no per-cell E"
        if scheme == "3d":
            cells = [self._repeat_z(v) for v in cells]
        # the scene holds mu = 1: the per-cell H coefficients borrow the patterns of the E ones
        self.cell = {c: v.double() for c, v in zip(self.E, cells)}
        self.cell.update({c: cells[n % len(cells)].double() for n, c in enumerate(self.H)})
        gen = torch.Generator().manual_seed(SEED + list(GRIDS).index(name))
        hs = 1.0 / (2.0 * self.scalar[self.E[0]])
        self.state = {c: ((torch.rand(size, generator=gen, dtype=torch.float64) * 2.0 - 1.0)
                          * (1.0 if _kind(c) == "E" else hs)).float().double() for c in self.comps}
        # what a fused launch finds in fout: differs from fin in every cell
        self.sentinel = {c: (v + 4.0 * (1.0 if _kind(c) == "E" else hs)).float().double()
                         for c, v in self.state.items()}
        assert all(bool((self.sentinel[c] != self.state[c]).all()) for c in self.comps)
        self.ops64 = TorchOps(self.layout, "cpu", torch.float64)
        self.ops32 = TorchOps(self.layout, "cpu", torch.float32)
        self.cache = {}

    @staticmethod
    def _repeat_z(v):
        """The first ZPERIOD planes of a per-cell array (they hold the whole
        sphere, between planes of ones) repeated along z, every other period
        mirrored in x and y."""
        nz = v.shape[2]
        first = v[:, :, :ZPERIOD]
        assert bool((v[:, :, ZPERIOD:] == 1).all()) and bool((first[:, :, 0] == 1).all())
        assert bool((first[:, :, -1] == 1).all())
        parts = [first if k % 2 == 0 else first.flip(0, 1) for k in range(-(-nz // ZPERIOD))]
        return torch.cat(parts, dim=2)[:, :, :nz].contiguous()

    def names(self, kind):
        return self.E if kind == "E" else self.H

    def coefs(self, cset):
        """"scalar", or per-cell for the kinds named after "cell": cellE, cellH, cellEH."""
        per = cset[4:] if cset.startswith("cell") else ""
        return {c: Coef(self.scalar[c], cell=self.cell[c] if _kind(c) in per else None) for c in self.comps}


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


# ---------------------------------------------------------------- launches
class Split:
    """ops.curl_update of one kind on per-component boxes."""
    family = "split"

    def __init__(self, name, kind, boxes):
        self.name, self.kind, self.boxes = name, kind, boxes
        self.kinds = (kind,)
        self.fused = False

    def __call__(self, ops, F, cb, out=None):
        ops.curl_update(self.kind, self.boxes, F, F, cb)
        return F

    def mask(self, cs, c):
        m = torch.zeros(cs.size, dtype=torch.bool)
        b = self.boxes.get(c, EMPTY)
        if not _empty(b):
            m[_sl(b)] = True
        return m

    def stencil_boxes(self):
        return [(self.kind, c, b) for c, b in self.boxes.items() if not _empty(b)]


class Multi(Split):
    """ops.curl_update_multi of one kind on a list of windows (the oracle: one by one)."""

    def __init__(self, name, kind, windows):
        self.name, self.kind, self.windows = name, kind, windows
        self.kinds = (kind,)
        self.fused = False

    def __call__(self, ops, F, cb, out=None, one_by_one=False):
        if hasattr(ops, "curl_update_multi") and not one_by_one:
            ops.curl_update_multi(self.kind, self.windows, F, F, cb)
        else:
            for w in self.windows:
                ops.curl_update(self.kind, w, F, F, cb)
        return F

    def mask(self, cs, c):
        m = torch.zeros(cs.size, dtype=torch.bool)
        for w in self.windows:
            b = w.get(c, EMPTY)
            if not _empty(b):
                assert not bool(m[_sl(b)].any()), "windows overlap"
                m[_sl(b)] = True
        return m

    def stencil_boxes(self):
        return [(self.kind, c, b) for w in self.windows for c, b in w.items() if not _empty(b)]


class Fused:
    """ops.fused_step on one or more sets of six boxes, one launch each into
    the same fout, with one point source (component, index, value) or None."""
    family = "fused"
    kinds = ("E", "H")
    fused = True

    def __init__(self, name, launches, source=None):
        self.name, self.launches, self.source = name, launches, source
        self.kind = "E"

    def __call__(self, ops, F, cb, out=None):
        for boxes in self.launches:
            ops.fused_step(F, out, boxes, cb, self.source)
        return out

    def mask(self, cs, c):
        m = torch.zeros(cs.size, dtype=torch.bool)
        for boxes in self.launches:
            b = boxes[c]
            if not _empty(b):
                assert not bool(m[_sl(b)].any()), "a component's boxes of two launches overlap"
                m[_sl(b)] = True
        return m

    def region(self):
        """The union box R of the first launch (the tiles start at its low corner)."""
        return _union(self.launches[0].values())

    def with_source(self, tag, source):
        return Fused(self.name + "/" + tag, self.launches, source)

    def stencil_boxes(self):
        return [(_kind(c), c, b) for boxes in self.launches for c, b in boxes.items() if not _empty(b)]


def lanes_z(lo, hi):
    """Row layout of a split launch whose union box spans z [lo, hi) (yee3d_v4.hip ``lanes_z``)."""
    kspan = hi - (lo & ~3)
    for lz in (64, 16):
        seg = 4 * lz
        if 20 * kspan >= 17 * (-(-kspan // seg) * seg):
            return lz
    return 8


def layout_of(launch):
    """(lanes per z row, workgroups along z) of a 3D split launch in the float4 kernels."""
    bu = _union(launch.boxes.values())
    lz = lanes_z(bu[0][2], bu[1][2])
    return lz, -(-(bu[1][2] - (bu[0][2] & ~3)) // (4 * lz))


def windows3(cs):
    """name -> the six per-component boxes of a 3D window: E and H each their own."""
    nx, ny, nz = cs.size
    E, H = cs.E, cs.H

    def win(xs, ys, zs):
        """Per component (Ex, Ey, Ez, Hx, Hy, Hz) the ranges; one range serves all; None: an empty box."""
        out = {}
        for n, c in enumerate(E + H):
            r = [v[n] if isinstance(v, list) else v for v in (xs, ys, zs)]
            if any(v is None for v in r):
                out[c] = EMPTY
            else:
                out[c] = _clip(((r[0][0], r[1][0], r[2][0]), (r[0][1], r[1][1], r[2][1])), cs.whole[c])
        return out

    xi, yi = (1, nx - 1), (1, ny - 1)
    W = {"whole": dict(cs.whole)}
    # the three boxes of a kind differ on every axis, z ends no multiples of 4
    W["interior"] = win([(2, nx - 3), (3, nx - 1), (1, nx - 2), (2, nx - 3), (3, nx - 2), (1, nx - 1)],
                        [(3, ny - 1), (1, ny - 2), (2, ny), (3, ny - 1), (1, ny - 2), (2, ny - 1)],
                        [(5, nz - 19), (6, nz - 17), (7, nz - 21), (5, nz - 19), (6, nz - 17), (7, nz - 23)])
    # z-thin at the low end, z lo = 1: kb == 0 with element 0 masked off (8 lanes)
    W["zlo1"] = win(xi, yi, [(1, 29), (2, 30), (3, 27)] * 2)
    # z-thin at the high end, ending at nz (8 lanes)
    W["zhi"] = win(xi, yi, [(nz - 27, nz), (nz - 25, nz), (nz - 30, nz - 1), (nz - 27, nz - 1), (nz - 25, nz - 1),
                            (nz - 30, nz)])
    W["lz8-two"] = win((2, nx - 2), (2, ny - 2), [(9, 47), (10, 45), (11, 44)] * 2)   # 8 lanes, two workgroups in z
    W["lz16"] = win(xi, yi, [(6, 66), (7, 65), (5, 63)] * 2)                          # 16 lanes
    W["lz16-two"] = win(xi, yi, [(5, 125), (6, 124), (7, 123)] * 2)                   # 16 lanes, two workgroups
    W["xplane"] = win((7, 8), yi, (3, nz - 5))
    W["yrow"] = win(xi, (5, 6), (2, nz - 3))
    W["zcell"] = win(xi, yi, (30, 31))                                                # inside the float4 group 28 .. 31
    W["one-empty"] = win(xi, (2, ny - 2), [(3, 101), None, (5, 99), (3, 101), None, (5, 99)])
    W["xsplit"] = win([(1, 4), (5, 7), (8, nx), (1, 4), (5, 7), (8, nx - 1)], yi, (1, 60))  # no overlap in x
    # Ex from x = 0 (i0 == 0: no plane x - 1), Hx up to nx
    W["xends"] = win([(0, 6), (1, 6), (1, 5), (nx - 6, nx), (nx - 6, nx - 1), (nx - 5, nx - 1)], (2, ny - 1), (5, nz - 9))
    return W


def split_launches(cs):
    return [Split(name, kind, {c: w[c] for c in cs.names(kind)}) for name, w in windows3(cs).items() for kind in "EH"]


def fused_boxes(cs):
    """name -> list of launches (six boxes each)."""
    nx, ny, nz = cs.size
    inner = ((4, 4, 40), (nx - 4, ny - 4, nz - 40))
    outer = ((2, 2, 30), (nx - 2, ny - 2, nz - 30))
    # the shell between the two boxes as six disjoint slabs, one launch each, every component on each
    (x0, y0, z0), (x1, y1, z1) = inner
    (X0, Y0, Z0), (X1, Y1, Z1) = outer
    shell = [((X0, Y0, Z0), (x0, Y1, Z1)), ((x1, Y0, Z0), (X1, Y1, Z1)), ((x0, Y0, Z0), (x1, y0, Z1)),
             ((x0, y1, Z0), (x1, Y1, Z1)), ((x0, y0, Z0), (x1, y1, z0)), ((x0, y0, z1), (x1, y1, Z1))]
    assert sum((b[1][0] - b[0][0]) * (b[1][1] - b[0][1]) * (b[1][2] - b[0][2]) for b in shell + [inner]) \
        == (X1 - X0) * (Y1 - Y0) * (Z1 - Z0)
    # one more launch whose union box covers everything written so far while each of its component boxes
    # lies outside it, on six different faces: a kernel that stored outside its boxes would overwrite it
    cover = {"Ex": ((X1, 4, 40), (X1 + 1, ny - 4, nz - 40)), "Ey": ((4, Y1, 40), (nx - 4, Y1 + 1, nz - 40)),
             "Ez": ((4, 4, Z1), (nx - 4, ny - 4, Z1 + 10)), "Hx": ((X0 - 1, 4, 40), (X0, ny - 4, nz - 40)),
             "Hy": ((4, Y0 - 1, 40), (nx - 4, Y0, nz - 40)), "Hz": ((4, 4, Z0 - 10), (nx - 4, ny - 4, Z0))}
    cu = _union(cover.values())
    assert all(cu[0][d] <= outer[0][d] and outer[1][d] <= cu[1][d] for d in range(3))
    assert all(_clip(b, cs.whole[c]) == b and _empty(_clip(b, outer)) for c, b in cover.items())
    return {"whole": [dict(cs.whole)], "sub": [windows3(cs)["interior"]],
            "shell": [{c: inner for c in cs.comps}] + [{c: b for c in cs.comps} for b in shell] + [cover]}


def fused_launches(cs, v4, fty):
    """Every (boxes, source place) of a fused form: ``v4`` the float4 kernel
    (256-cell tiles) or the scalar one (64), ``fty`` its owned rows."""
    out = []
    for name, launches in fused_boxes(cs).items():
        base = Fused(name, launches)
        R = base.region()
        z0 = (R[0][2] & ~3) + 256 if v4 else R[0][2] + 64
        places = {"none": None, "inside": ("Ez", (5, 6, 50), SRC_VAL),
                  # the tile's halo column: Ey (x, y, z0), the z + 1 neighbour of the tile's last Hx
                  "zhalo": ("Ey", (5, R[0][1] + 1, z0), SRC_VAL) if z0 < cs.size[2] - 1 else None,
                  # the tile's halo row: Ez (x, y0 + fty, z), the y + 1 neighbour of the tile's last Hx
                  "yhalo": ("Ez", (5, R[0][1] + fty, R[0][2] + 10), SRC_VAL)}
        for tag, src in places.items():
            if src is not None or tag == "none":
                out.append(base.with_source(tag, src))
    return out


def windows2(cs, kind):
    """name -> per-component boxes of a 2D (1D) single-window launch of a kind."""
    nx, ny, _ = cs.size
    names = cs.names(kind)

    def win(*ranges):
        return {c: (EMPTY if r is None else _clip(((r[0][0], r[1][0], 0), (r[0][1], r[1][1], 1)), cs.whole[c]))
                for c, r in zip(names, ranges + ranges[-1:] * (len(names) - len(ranges)))}

    if cs.scheme == "1d":
        return {"whole": {c: cs.whole[c] for c in names}, "part": win(((37, 201), (0, 1)))}
    W = {"whole": {c: cs.whole[c] for c in names},
         "row": win(((7, 8), (1, ny - 1))), "column": win(((1, nx - 1), (70, 71))),
         "differ": win(((3, 30), (5, 140)), ((6, 35), (2, 100)))}
    if len(names) == 2:
        W["one-empty"] = win(None, ((3, 30), (5, 140)))  # (the other one reads the x neighbour)
    return W


# 11 disjoint windows (x range, y range) whose automatic x chunks differ once fdtd_set_lowdim_wgs(MULTI_WGS)
# lowers the workgroup target (2048 by default: every window of a grid this small then has chunks of one row)
MULTI_WGS = 3
MULTI_WINDOWS = [((1, 15), (1, 100)), ((1, 15), (100, 150)), None, ((15, 25), (1, 60)), ((15, 25), (60, 150)),
                 ((25, 35), (1, 20)), ((25, 35), (20, 150)), ((35, 35), (1, 150)), ((35, 40), (1, 30)),
                 ((35, 40), (30, 31)), ((35, 40), (31, 100)), ((35, 40), (100, 148)), ((35, 40), (148, 150)), None]


def xchunk2d(b, wgs=2048):
    """Automatic x chunk of a window with union box ``b`` (yee_lowdim.hip ``xchunk2d``)."""
    xc = 16
    while xc > 1 and -(-(b[1][1] - b[0][1]) // 64) * -(-(-(-(b[1][0] - b[0][0]) // xc)) // 4) < wgs:
        xc //= 2
    return xc


def multi_launch(cs, kind):
    names = cs.names(kind)
    wins = []
    for n, r in enumerate(MULTI_WINDOWS):
        if r is None:
            wins.append({c: EMPTY for c in names})
            continue
        w = {c: _clip(((r[0][0], r[1][0], 0), (r[0][1], r[1][1], 1)), cs.whole[c]) for c in names}
        if n == 4 and len(names) == 2:
            w[names[1]] = EMPTY  # one component's box empty
        wins.append(w)
    return Multi("multi", kind, wins)


def lowdim_launches(cs):
    out = [Split(name, kind, b) for kind in "EH" for name, b in windows2(cs, kind).items()]
    if cs.scheme != "1d":
        out += [multi_launch(cs, kind) for kind in "EH"]
    return out


def all_launches(name):
    """Every launch of parts 1 to 3 on a grid (the fused ones with each form's source places)."""
    cs = case(name)
    if cs.scheme != "3d":
        return lowdim_launches(cs)
    out = split_launches(cs) + fused_launches(cs, False, 7)
    if cs.size[2] % 4 == 0:
        out += [Fused("%s@v4-%d" % (l.name, fty), l.launches, l.source) for fty in (3, 7)
                for l in fused_launches(cs, True, fty)]
    return out


# ---------------------------------------------------------------- oracle, tolerances
def run_cpu(cs, ops, launch, cset, dtype=torch.float64, zero_old=False):
    F = {c: v.to(dtype).clone() for c, v in cs.state.items()}
    if zero_old:
        for c in cs.names(launch.kind):
            F[c].zero_()
    out = {c: v.to(dtype).clone() for c, v in cs.sentinel.items()} if launch.fused else None
    cb = {c: k.to("cpu", dtype) for c, k in cs.coefs(cset).items()}
    res = launch(ops, F, cb, out)
    return {c: v.double() for c, v in res.items()}


def oracle(cs, launch, cset):
    key = (launch.family, launch.name, launch.kind, getattr(launch, "source", None), cset)
    if key not in cs.cache:
        cs.cache[key] = run_cpu(cs, cs.ops64, launch, cset)
    return cs.cache[key]


def whole_launch(cs, family, kind):
    if family == "fused":
        return Fused("whole", [dict(cs.whole)])
    return Split("whole", kind, {c: cs.whole[c] for c in cs.names(kind)})


def scales(cs, family, cset):
    """Per kind the oracle's largest value after the whole-box half step (fused step)."""
    key = ("scale", family, cset)
    if key not in cs.cache:
        out = {}
        for kind in "EH":
            launch = whole_launch(cs, family, kind)
            want = oracle(cs, launch, cset)
            out[kind] = max(float(want[c][launch.mask(cs, c)].abs().max()) for c in cs.names(kind))
        cs.cache[key] = out
    return cs.cache[key]


def errors(cs, launch, got, want, cset):
    """Per kind the largest error / scale over the launch's cells."""
    sc = scales(cs, launch.family, cset)
    out = {}
    for kind in launch.kinds:
        e = 0.0
        for c in cs.names(kind):
            m = launch.mask(cs, c)
            if bool(m.any()):
                e = max(e, float((got[c] - want[c])[m].abs().max()))
        out[kind] = e / sc[kind]
    return out


def measure_e32(name, family, cset, kind):
    cs = case(name)
    launch = whole_launch(cs, family, kind)
    got = run_cpu(cs, cs.ops32, launch, cset, torch.float32)
    return errors(cs, launch, got, oracle(cs, launch, cset), cset)[kind]


def e32_keys():
    keys = []
    for name in GRIDS:
        for kind in "EH":
            keys += [("split", name, cset, kind) for cset in ("scalar", "cell" + kind)]
        if name in GRIDS3:
            keys += [("fused", name, cset, kind) for cset in ("scalar", "cellE", "cellH", "cellEH") for kind in "EH"]
    return keys


def tolerance(name, family, cset, kind, dtype):
    return min(4.0 * E32[(family, name, cset, kind)], 2e-5) * (1.0 if dtype == "f32" else EPS_RATIO)


def check(cs, launch, got, want, cset, dtype, what, fin=None):
    """Every cell of every field: inside the launch's boxes within tolerance of
    the oracle, everywhere else bit-identical to the input (the sentinel)."""
    base = cs.sentinel if launch.fused else cs.state
    for c in cs.comps:
        keep = ~launch.mask(cs, c)
        assert torch.equal(got[c][keep], base[c][keep]), (what, c, "cells outside the boxes changed")
        if fin is not None:
            assert torch.equal(fin[c], cs.state[c]), (what, c, "the input fields changed")
    errs = errors(cs, launch, got, want, cset)
    for kind, e in errs.items():
        tol = tolerance(cs.name, launch.family, cset, kind, dtype)
        assert e <= tol, (what, kind, "error / scale", e, "tolerance", tol)
    return errs


def controls(cs, launch, cset):
    """(name, control result, per component the cells that read the operand)."""
    masks = {c: launch.mask(cs, c) for k in launch.kinds for c in cs.names(k)}
    out = [("old", run_cpu(cs, cs.ops64, launch, cset, zero_old=True),
            {c: m for c, m in masks.items() if _kind(c) == launch.kind})]
    if cset != "scalar":
        per = cset[4:]
        out.append(("cell", run_cpu(cs, cs.ops64, launch, "scalar"),
                    {c: m & (cs.cell[c] != 1) for c, m in masks.items() if _kind(c) in per}))
    xc = {c: m for c, m in masks.items() if any(axis == 0 for _, axis, _ in cs.layout.curl_terms(c))}
    out.append(("x-neighbour", run_cpu(cs, NoXNeighbour(cs.layout, "cpu", torch.float64), launch, cset), xc))
    return out


def coef_boxes(launch):
    """The non-empty (component, box) pairs of a launch."""
    return [(c, b) for _, c, b in launch.stencil_boxes()]


def coef_varies(cs, c, b):
    """The per-cell coefficient of ``c`` takes more than one value inside
    ``b`` and varies along x or y on some z plane of it."""
    v = cs.cell[c][_sl(b)]
    return bool((v.amax(dim=(0, 1)) != v.amin(dim=(0, 1))).any())


def liveness(cs, launch, cset, res):
    """name -> (distance of ``res`` from the control) / (fp32 tolerance), None
    where no cell of the launch reads the operand."""
    sc = scales(cs, launch.family, cset)
    out = {}
    for name, ctrl, cells in controls(cs, launch, cset):
        worst = None
        for c, m in cells.items():
            if bool(m.any()):
                d = float((res[c] - ctrl[c])[m].abs().max()) / sc[_kind(c)]
                d /= tolerance(cs.name, launch.family, cset, _kind(c), "f32")
                worst = d if worst is None else max(worst, d)
        out[name] = worst
    return out


# ---------------------------------------------------------------- HIP side
_DEV = {}
WORST = {}


def dev(cs, gpu, dtype, cset):
    """(pristine state, sentinel, coefficients) of a grid on the GPU."""
    key = (cs.name, dtype)
    if key not in _DEV:
        _DEV[key] = ({c: v.to(gpu, TD[dtype]) for c, v in cs.state.items()},
                     {c: v.to(gpu, TD[dtype]) for c, v in cs.sentinel.items()}, {})
    st, sen, cbs = _DEV[key]
    if cset not in cbs:
        cbs[cset] = {c: k.to(gpu, TD[dtype]) for c, k in cs.coefs(cset).items()}
    return st, sen, cbs[cset]


def run_hip(cs, ops, launch, cset, gpu, dtype, tag, **kw):
    st, sen, cb = dev(cs, gpu, dtype, cset)
    F = {c: v.clone() for c, v in st.items()}
    out = {c: v.clone() for c, v in sen.items()} if launch.fused else None
    n0 = ops.launches
    res = launch(ops, F, cb, out, **kw)
    torch.cuda.synchronize()
    assert ops.launches > n0
    got = {c: v.double().cpu() for c, v in res.items()}
    fin = {c: v.double().cpu() for c, v in F.items()} if launch.fused else None
    what = (cs.name, dtype, tag, cset, launch.name, launch.kind)
    errs = check(cs, launch, got, oracle(cs, launch, cset), cset, dtype, what, fin)
    for kind, e in errs.items():
        k = (tag.split("/")[0], dtype, kind)
        WORST[k] = max(WORST.get(k, 0.0), e / (1.0 if dtype == "f32" else EPS_RATIO))
        print("plain", *what, kind, "err/scale %.3g tol %.3g" % (e, tolerance(cs.name, launch.family, cset, kind, dtype)),
              "worst", k, "%.3g" % WORST[k])
    return got, ops.launches - n0


# form -> (dtype, float4 kernels, needs nz % 4 == 0)
FORMS3 = {"v4": ("f32", True, True), "scalar": ("f32", False, False), "f64": ("f64", True, False)}
CASES3 = [(g, f) for g in GRIDS3 for f, (_, _, mult4) in FORMS3.items() if not mult4 or GRIDS[g][1][2] % 4 == 0]


@pytest.mark.parametrize("cell", [False, True])
@pytest.mark.parametrize("grid,form", CASES3)
def test_split_windows(gpu, grid, form, cell):
    """ops.curl_update of E and of H on every window of windows3, at the three x chunks."""
    from fdtd3d_amd.ops.hip_ops import HipOps
    cs = case(grid)
    dtype, vec4, _ = FORMS3[form]
    for xchunk in XCHUNKS:
        ops = HipOps(cs.layout, gpu, TD[dtype], xchunk=xchunk, vec4=vec4)
        ops.f64_v4 = False  # fp64 on k_update_e3d / k_update_h3d (the double4 lanes: test_cpml_gpu.py)
        for launch in split_launches(cs):
            cset = "cell" + launch.kind if cell else "scalar"
            run_hip(cs, ops, launch, cset, gpu, dtype, "split-%s/x%d" % (form, xchunk))


# form -> (dtype, k_fused3d_v4 (256-cell tiles) or k_fused3d (64-cell tiles), owned rows)
FORMSF = {"v4-3": ("f32", True, 3), "v4-7": ("f32", True, 7), "scalar": ("f32", False, 7), "f64": ("f64", False, 7)}
CASESF = [(g, f) for g in GRIDS3 for f in FORMSF if not f.startswith("v4") or GRIDS[g][1][2] % 4 == 0]


@pytest.mark.parametrize("cset", ["scalar", "cellE", "cellH", "cellEH"])
@pytest.mark.parametrize("grid,form", CASESF)
def test_fused(gpu, grid, form, cset):
    """ops.fused_step into a sentinel-filled fout: whole boxes, a sub-box, an
    interior box and then the shell around it; every source place; the three x chunks."""
    from fdtd3d_amd.ops.hip_ops import HipOps, load_library
    cs = case(grid)
    dtype, vec4, fty = FORMSF[form]
    lib = load_library()
    try:
        lib.fdtd_set_fused_rows(fty)
        launches = fused_launches(cs, vec4, fty)
        assert {l.name.split("/")[1] for l in launches} >= {"none", "inside", "yhalo"}
        if not vec4 or cs.size[2] > 256:
            assert any(l.name.endswith("zhalo") for l in launches)
        for xchunk in XCHUNKS:
            ops = HipOps(cs.layout, gpu, TD[dtype], xchunk=xchunk, vec4=vec4)
            for launch in launches:
                run_hip(cs, ops, launch, cset, gpu, dtype, "fused-%s/x%d" % (form, xchunk))
    finally:
        lib.fdtd_set_fused_rows(7)


@pytest.mark.parametrize("cell", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid", ["tmz", "tez", "1d"])
def test_lowdim_windows(gpu, grid, dtype, cell):
    """Single windows of the 2D / 1D kernels through ops.curl_update."""
    from fdtd3d_amd.ops.hip_ops import HipOps
    cs = case(grid)
    ops = HipOps(cs.layout, gpu, TD[dtype])
    for launch in lowdim_launches(cs):
        if not isinstance(launch, Multi):
            run_hip(cs, ops, launch, "cell" + launch.kind if cell else "scalar", gpu, dtype, "lowdim")


@pytest.mark.parametrize("cell", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("grid", ["tmz", "tez"])
def test_lowdim_multi(gpu, grid, dtype, cell):
    """ops.curl_update_multi on 11 windows: two launches, within tolerance of
    the oracle and bit-identical to the windows sent one by one -- at the default
    x chunks (one row each on this grid) and at chunks that differ per window."""
    from fdtd3d_amd.ops.hip_ops import HipOps, load_library
    cs = case(grid)
    lib = load_library()
    ops = HipOps(cs.layout, gpu, TD[dtype])
    try:
        for wgs in (0, MULTI_WGS):
            lib.fdtd_set_lowdim_wgs(wgs)
            for kind in "EH":
                launch = multi_launch(cs, kind)
                cset = "cell" + kind if cell else "scalar"
                got, n = run_hip(cs, ops, launch, cset, gpu, dtype, "multi/wgs%d" % wgs)
                assert n == 2, (kind, "launches", n)
                one, _ = run_hip(cs, ops, launch, cset, gpu, dtype, "multi-one/wgs%d" % wgs, one_by_one=True)
                for c in cs.comps:
                    assert torch.equal(got[c], one[c]), (kind, c, "multi-window launch differs from single windows")
    finally:
        lib.fdtd_set_lowdim_wgs(0)


# ---------------------------------------------------------------- TF/SF corrections and the incident line
TFSF_CFG = dict(scheme="3d", size=(40, 36, 44), time_steps=1, use_tfsf=True, scene="vacuum", tfsf_size=(6, 7, 8),
                theta=35, phi=20, psi=10, hybrid_block=1)
TFSF_SUB = ((3, 4, 2), (30, 20, 37))  # cuts the TF box ([6, 34) x [7, 29) x [8, 36)) on every axis
# e32 of the TorchOps call in float32 against float64 per (op, kind), scaled by the oracle's largest value of the
# target: test_plain_cpu.py::test_e32_constants re-measures them
E32_TFSF = {
    ("apply-whole", "E"): 7.297e-08, ("apply-whole", "H"): 6.870e-08,
    ("apply-sub", "E"): 6.213e-08, ("apply-sub", "H"): 5.473e-08,
    ("many", "E"): 7.297e-08, ("many", "H"): 6.870e-08,
    ("inc", "E"): 7.632e-08, ("inc", "H"): 8.300e-08,
}
_TFSF = {}


def tfsf_side(backend, device, dtype):
    key = (backend, dtype)
    if key not in _TFSF:
        s = YeeScheme(SchemeConfig(dtype=dtype, **TFSF_CFG), make_ops(backend, None, device, TD[dtype]))
        s.init_scheme()
        s.init_grids()
        _TFSF[key] = s
    return _TFSF[key]


def tfsf_state():
    """Live fields and a live incident line (E size 1, H size 1 / (2 cb)), float32-representable."""
    if "state" not in _TFSF:
        s = tfsf_side("torch", "cpu", "f64")
        gen = torch.Generator().manual_seed(SEED + 50)
        hs = 1.0 / (2.0 * s.cb["Ex"].scalar)

        def rnd(shape, scale):
            return ((torch.rand(shape, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * scale).float().double()
        F = {c: rnd(tuple(s.F[0][c].shape), 1.0 if _kind(c) == "E" else hs) for c in s.comps}
        n = s.einc[0].numel()
        _TFSF["state"] = (F, rnd((n,), 1.0), rnd((n,), hs))
    return _TFSF["state"]


TFSF_OPS = ("apply-whole", "apply-sub", "many", "inc")


def tfsf_run(s, op, kind):
    """One op on scheme ``s`` from the live state: (results, input, written-cell masks) as float64 CPU dicts."""
    F, einc, hinc = tfsf_state()
    dt, dv = s.dtype, s.device
    if op == "inc":
        e, h = einc.to(dv, dt).clone(), hinc.to(dv, dt).clone()
        if kind == "E":
            s.ops.inc_step_e(e, h, s.inc_ce, 0.625)
        else:
            s.ops.inc_step_h(e, h, s.inc_ch)
        n = e.numel()
        m = {"einc": torch.full((n,), kind == "E"), "hinc": torch.arange(n) < (n - 1 if kind == "H" else 0)}
        return {"einc": e.double().cpu(), "hinc": h.double().cpu()}, {"einc": einc, "hinc": hinc}, m
    comps = s.e_comps if kind == "E" else s.h_comps
    inc = (hinc if kind == "E" else einc).to(dv, dt)
    T = {c: F[c].to(dv, dt).clone() for c in comps}
    box = TFSF_SUB if op == "apply-sub" else ((0, 0, 0), tuple(s.cfg.size))
    masks = {c: torch.zeros(tuple(s.cfg.size), dtype=torch.bool) for c in comps}
    items = []
    for c in comps:
        for tab in s.tfsf[c]:
            ijk = tab.ijk.cpu().long()
            inb = torch.ones(tab.n, dtype=torch.bool)
            for d in range(3):
                inb &= (ijk[:, d] >= box[0][d]) & (ijk[:, d] < box[1][d])
            masks[c].view(-1)[tab.off.cpu()[inb]] = True
            if op == "many":
                items.append((T[c], tab))
            else:
                s.ops.tfsf_apply(T[c], tab, inc, box)
    if op == "many":
        assert len(items) >= 3
        s.ops.tfsf_apply_many(items, inc)
    return {c: v.double().cpu() for c, v in T.items()}, {c: F[c] for c in comps}, masks


def tfsf_oracle(op, kind):
    key = ("oracle", op, kind)
    if key not in _TFSF:
        _TFSF[key] = tfsf_run(tfsf_side("torch", "cpu", "f64"), "apply-whole" if op == "many" else op, kind)
    return _TFSF[key]


def tfsf_scale(want, masks):
    """The oracle's largest value of the arrays the op writes."""
    return max(float(want[c].abs().max()) for c, m in masks.items() if bool(m.any()))


def tfsf_error(op, kind, got):
    want, _, masks = tfsf_oracle(op, kind)
    scale = tfsf_scale(want, masks)
    return max(float((got[c] - want[c])[m].abs().max()) for c, m in masks.items() if bool(m.any())) / scale


def measure_e32_tfsf(op, kind):
    return tfsf_error(op, kind, tfsf_run(tfsf_side("torch", "cpu", "f32"), "apply-whole" if op == "many" else op,
                                         kind)[0])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("op", TFSF_OPS)
def test_tfsf_ops(gpu, op, dtype):
    """tfsf_apply on the whole array and on a sub-box, tfsf_apply_many, inc_step_e / inc_step_h from a live
    incident line and live fields against TorchOps in float64; untargeted cells bit-identical."""
    s = tfsf_side("hip", gpu, dtype)
    for kind in "EH":
        want, base, masks = tfsf_oracle(op, kind)
        got, _, _ = tfsf_run(s, op, kind)
        torch.cuda.synchronize()
        tol = min(4.0 * E32_TFSF[(op, kind)], 2e-5) * (1.0 if dtype == "f32" else EPS_RATIO)
        scale = tfsf_scale(want, masks)
        for c, m in masks.items():
            assert torch.equal(got[c][~m], base[c][~m]), (op, kind, c, "untargeted cells changed")
            if op != "inc":
                assert int(m.sum()) > 100
            # the corrections are live: far above the tolerance on the cells they target
            assert not bool(m.any()) or float((want[c] - base[c])[m].abs().max()) > LIVE * tol * scale, (op, kind, c)
        err = tfsf_error(op, kind, got)
        print("plain tfsf", op, dtype, kind, "err/scale %.3g tol %.3g" % (err, tol))
        assert err <= tol, (op, kind, err, tol)
