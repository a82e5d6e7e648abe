"""The kernels around the stencils, one call at a time against plain slicing
or an fp64 expression: csrc/aux_kernels.hip (halo boxes, reductions, amplitude
tracking, sources, graph-replay helpers) and ``k_scattered`` / ``k_inc_e_tab``
of csrc/generic_kernels.hip.

Every test draws its inputs once in fp64 from a seeded generator and converts
them to the dtype under test, pre-fills whatever the op may write with NaN
(buffers) or a sentinel (arrays), makes ONE op call and compares everything
the op can touch: what the reference leaves alone is bit-identical to the
pre-fill, and the inputs are bit-unchanged.  All comparisons are exact except
the two with a derived bound (``inc_step_e_tab`` against fp64, ``scattered``).

Each section is a ``run_*`` function (the op call on pre-filled state; takes
the ops object, so tests/test_aux_cpu.py runs it on the torch backend too) and
a ``check_*`` function (the assertions; test_aux_cpu.py corrupts a result and
shows that it fails).  Every case of a table carries a ``why`` and the
property it claims; ``claims_*`` computes that property from the launchers'
formulas below and the test asserts it.

Launch formulas (aux_kernels.hip / generic_kernels.hip), V = 4 (fp32) or 2
(fp64) elements of a 16-byte vector:

* ``box_copy_grid``: per (component, x plane) ``min(1024, ceil(by * bz / V'
  / 256))`` blocks of 256 threads over ``by * (bz / V')`` groups, V' = V on
  the vector path (nz, lo.z, hi.z multiples of V, every base and the buffer
  16-byte aligned) and 1 otherwise; ``copy_box`` on aligned rows with an
  unaligned z range runs the masked kernel over ``by * ng`` groups,
  ``ng = ceil((hi.z - (lo.z & ~(V - 1))) / V)``, on the vector grid.
  grid.z = bx * ncomp <= 65535, ncomp <= 8.
* ``k_box_list``: entry e owns ``ceil(groups / 256)`` blocks from ``blk0[e]``;
  its ``vec`` is V when nz, lo.z, hi.z, the buffer offset are multiples of V
  and both bases are aligned, else 1 (parallel/halo.py ``_BoxList.build``).
* ``reduce_grid`` (maxabs, amplitude_update): ``min(4096, ceil(n / 256))``
  blocks of 256, grid-stride.
* ``amplitude_many``: over the union u of the non-empty boxes, workgroups of
  64 lanes x 4 rows; fp32 with nz % 4 == 0 and all bases aligned:
  ``k_amplitude_many_v4``, grid ``(ceil((u.hi.z - (u.lo.z & ~3)) / 256),
  ceil(uy / 4), ux)``; otherwise ``k_amplitude_many<T>``, grid
  ``(ceil(uz / 64), ceil(uy / 4), ux)``.
* ``k_scattered``: ``min(65536, ceil(n / 256))`` blocks of 256, grid-stride:
  one sweep covers 16777216 cells.

Kernel template instances and the cases that reach them:

    k_box_copy<pack|unpack, V, f32|f64>   PACK_CASES stride-vec-f32 / stride-vec-f64, gridz-65535, eight-comps
    k_box_copy<pack|unpack, 1, f32|f64>   PACK_CASES stride-scalar, odd-base
    k_box_xfer<V>                         XFER_CASES stride-vec-f32 / stride-vec-f64, eight-comps
    k_box_xfer_m                          XFER_CASES stride-masked-f32 / stride-masked-f64
    k_box_xfer<1>                         XFER_CASES stride-scalar, odd-base
    k_box_list<pack|unpack> V and 1       boxlist_entries (the ``form`` of each entry), test_box_list_one_entry
    k_box_maxabs<f32|f64>                 MAXABS_CASES
    k_amplitude_update<f32|f64>           AMP1_CASES
    k_amplitude_many_v4                   AMP_CASES *-v4
    k_amplitude_many<float>               AMP_CASES nz70-*, oddbase-*
    k_amplitude_many<double>              AMP_CASES with f64
    k_set_value, k_set_values,
    k_set_value_tab, k_counter_add        test_set_value, test_set_values, test_set_value_tab_counter
    k_inc_e_tab (and k_inc_e)             test_inc_step_e_tab
    k_scattered<f32|f64>                  SCAT_CASES

For the limits tests/test_pack_gpu.py and tests/test_scattered_gpu.py do not
reach (grid-stride loops, component and grid.z limits, misaligned bases, a
non-zero rank origin, per-cell bounds) this is the file.
"""
import math

import pytest
import torch

from fdtd3d_amd.layout.yee import MIN_COORD_FP, YeeLayout
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.ops.hip_lib import HipError
from fdtd3d_amd.parallel.halo import _BoxList

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
VW = {"f32": 4, "f64": 2}
SENT = -12345.0  # array pre-fill: no generated value has it
NAN = float("nan")
INF = float("inf")
COMPS = ("Ex", "Ey", "Ez", "Hx", "Hy", "Hz")


def cdiv(a, b):
    return -(-a // b)


def vol(box):
    v = 1
    for d in range(3):
        v *= max(0, box[1][d] - box[0][d])
    return v


def sl(box):
    return tuple(slice(box[0][d], box[1][d]) for d in range(3))


def bits(t):
    """The tensor's bit patterns (NaN and -0.0 compare like any value)."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def live(shape, seed, dt, device, base="aligned", lo=-1.0, hi=1.0):
    """Seeded uniform values drawn in fp64, converted to ``dt``; ``base`` =
    "odd": a view at element 1 of a flat allocation (base not 16-byte
    aligned)."""
    g = torch.Generator().manual_seed(seed)
    n = int(math.prod(shape))
    v = (torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo).to(DT[dt])
    return place(v, shape, device, base)


def place(values, shape, device, base="aligned"):
    n = values.numel()
    if base == "odd":
        flat = torch.full((n + 5,), NAN, dtype=values.dtype, device=device)
        flat[1:1 + n] = values.to(device)
        t = flat[1:1 + n].view(shape)
        assert t.data_ptr() % 16 != 0
        return t
    t = values.to(device).view(shape).contiguous()
    assert t.data_ptr() % 16 == 0
    return t


def filled(shape, value, dt, device, base="aligned"):
    return place(torch.full((int(math.prod(shape)),), value, dtype=DT[dt]), shape, device, base)


# ============================================================== 1. box_list
# arrays of one table: name -> (shape, base)
BL_ARRAYS = {
    "field": ((9, 11, 40), "aligned"),    # field-shaped
    "local": ((4, 7, 12), "aligned"),     # region-local
    "oddnz": ((3, 5, 7), "aligned"),      # odd nz: never the vector path
    "view": ((4, 7, 12), "odd"),          # a view whose base is not 16-byte aligned
    "tall": ((1, 257, 8), "aligned"),     # a 257-row column
}


def boxlist_entries(dt):
    """The 13 entries (not a power of two: the binary search over blk0 takes
    uneven halves) of the mixed table: dicts of array, box, buffer (0 / 1),
    buffer offset, why, and the claims ``form`` ("vec" / "scalar") and, where
    the entry exists for it, ``groups`` / ``blocks``.  Boxes of one array are
    disjoint, so the same table unpacks.  Buffer parts are laid out in order
    with NaN gaps between them."""
    V = VW[dt]
    rows = [
        ("field", ((0, 0, 0), (4, 8, 8 * V)), 0, "vector entry of exactly 256 groups (first entry)",
         dict(form="vec", groups=256, blocks=1)),
        ("local", ((1, 2, 4), (3, 6, 12)), 1, "vector entry of fewer than 256 groups", dict(form="vec", blocks=1)),
        ("field", ((8, 10, 39), (9, 11, 40)), 0, "one cell, the array's last", dict(form="scalar", groups=1)),
        ("field", ((4, 0, 1), (6, 3, 8)), 1, "scalar: lo.z unaligned", dict(form="scalar")),
        ("field", ((4, 3, 4), (6, 6, 7)), 0, "scalar: hi.z unaligned", dict(form="scalar")),
        ("field", ((6, 0, 8), (8, 4, 16)), 1, "scalar: odd buffer offset", dict(form="scalar", odd_off=True)),
        ("field", ((4, 6, 17), (9, 10, 39)), 0, "scalar entry of two blocks, the second partial",
         dict(form="scalar", groups=440, blocks=2)),
        ("local", ((0, 0, 0), (1, 7, 12)), 1, "a whole x plane, vector", dict(form="vec")),
        ("oddnz", ((0, 0, 0), (2, 5, 7)), 0, "odd nz, whole rows: scalar", dict(form="scalar")),
        ("oddnz", ((2, 1, 2), (3, 4, 6)), 1, "odd nz with an aligned z range: still scalar", dict(form="scalar")),
        ("view", ((0, 0, 0), (4, 7, 12)), 0, "scalar: array base not 16-byte aligned", dict(form="scalar")),
        ("local", ((3, 0, 0), (4, 7, 4)), 1, "one vector group per row", dict(form="vec")),
        ("tall", ((0, 0, 0), (1, 257, V)), 0, "vector entry of 257 groups: the second block holds one group "
         "(last entry)", dict(form="vec", groups=257, blocks=2)),
    ]
    off = [0, 0]
    out = []
    for arr, box, b, why, claim in rows:
        o = cdiv(off[b], 4) * 4 + (1 if claim.get("odd_off") else 0)  # aligned for both V unless claimed odd
        out.append(dict(arr=arr, box=box, buf=b, off=o, why=why, claim=claim))
        off[b] = o + vol(box) + 3  # a gap of NaN after every part
    return out, [off[0] + 5, off[1] + 5]


def boxlist_claims(dt, ent, arrays, bufs):
    """(vec, groups, blocks) of an entry from the formula of the module
    docstring."""
    V = VW[dt]
    t, buf = arrays[ent["arr"]], bufs[ent["buf"]]
    box = ent["box"]
    vec = (t.shape[2] % V == 0 and box[0][2] % V == 0 and box[1][2] % V == 0 and ent["off"] % V == 0
           and t.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0)
    groups = vol(box) // (V if vec else 1)
    return (V if vec else 1), groups, cdiv(groups, 256)


class _EntSize:
    """What ``_BoxList.build`` needs of an ops object."""

    @staticmethod
    def box_ent_size():
        return 64


def boxlist_setup(dt, device, entries=None, sizes=None):
    if entries is None:
        entries, sizes = boxlist_entries(dt)
    arrays = {n: live(s, 11 + i, dt, device, base) for i, (n, (s, base)) in enumerate(BL_ARRAYS.items())}
    bufs = [torch.full((n,), NAN, dtype=DT[dt], device=device) for n in sizes]
    bl = _BoxList()
    for e in entries:
        bl.add(arrays[e["arr"]], e["box"], bufs[e["buf"]], e["off"])
    return entries, arrays, bufs, bl


def check_table(dt, entries, arrays, bufs, built):
    """The built table against the layout documented at aux_kernels.hip
    ``BoxEnt`` (two pointers, ny, nz, lo[3], hi[3], blk0, vec, 2 pad ints)
    and the entries' claims."""
    tab, n, nblocks = built
    assert n == len(entries) and tuple(tab.shape) == (n, 8) and tab.dtype == torch.int64
    t64 = tab.cpu()
    t32 = t64.view(torch.int32)
    blk = 0
    for r, e in enumerate(entries):
        t, buf = arrays[e["arr"]], bufs[e["buf"]]
        vec, groups, blocks = boxlist_claims(dt, e, arrays, bufs)
        c = e["claim"]
        assert (vec > 1) == (c["form"] == "vec"), e["why"]
        assert c.get("groups", groups) == groups and c.get("blocks", blocks) == blocks, e["why"]
        assert e["off"] % 2 == (1 if c.get("odd_off") else 0), e["why"]
        assert int(t64[r, 0]) == t.data_ptr() and int(t64[r, 1]) == buf.data_ptr() + e["off"] * buf.element_size()
        want = [t.shape[1], t.shape[2], *e["box"][0], *e["box"][1], blk, vec, 0, 0]
        assert t32[r, 4:16].tolist() == want, (e["why"], t32[r, 4:16].tolist(), want)
        blk += blocks
    assert nblocks == blk


def ref_box_list(entries, arrays, bufs, pack):
    """The table's meaning in plain slicing (what test_aux_cpu.py runs in
    place of the kernel)."""
    for e in entries:
        t, buf, n = arrays[e["arr"]], bufs[e["buf"]], vol(e["box"])
        if pack:
            buf[e["off"]:e["off"] + n] = t[sl(e["box"])].reshape(-1)
        else:
            t[sl(e["box"])] = buf[e["off"]:e["off"] + n].view(t[sl(e["box"])].shape)


def run_boxlist(ops, dt, device, pack, entries=None, sizes=None):
    """One pack (live arrays -> NaN buffers) or unpack (live buffers ->
    sentinel arrays) launch of the table; ``ops`` None: ref_box_list."""
    entries, arrays, bufs, bl = boxlist_setup(dt, device, entries, sizes)
    if not pack:
        for i, b in enumerate(bufs):
            b.copy_(live((b.numel(),), 31 + i, dt, device))
        for t in arrays.values():
            t.fill_(SENT)
    before = ({n: t.clone() for n, t in arrays.items()}, [b.clone() for b in bufs])
    if ops is None:
        ref_box_list(entries, arrays, bufs, pack)
        built = bl.build(_EntSize)
    else:
        built = bl.build(ops)
        ops.box_list(*built, pack)
    return dict(dt=dt, entries=entries, arrays=arrays, bufs=bufs, before=before, built=built, pack=pack)


def check_boxlist(r):
    entries, arrays, bufs = r["entries"], r["arrays"], r["bufs"]
    arr0, buf0 = r["before"]
    check_table(r["dt"], entries, arrays, bufs, r["built"])
    if r["pack"]:
        want = [b.clone() for b in buf0]  # NaN
        for e in entries:
            want[e["buf"]][e["off"]:e["off"] + vol(e["box"])] = arr0[e["arr"]][sl(e["box"])].reshape(-1)
        for i, b in enumerate(bufs):
            for e in entries:  # per part first: the message names the entry
                if e["buf"] == i:
                    p = slice(e["off"], e["off"] + vol(e["box"]))
                    assert same(b[p], want[i][p]), e["why"]
            assert same(b, want[i]), "buffer %d: an element outside every part changed" % i
        for n, t in arrays.items():
            assert same(t, arr0[n]), "pack changed array %s" % n
    else:
        want = {n: t.clone() for n, t in arr0.items()}  # sentinel
        for e in entries:
            box = e["box"]
            want[e["arr"]][sl(box)] = buf0[e["buf"]][e["off"]:e["off"] + vol(box)].view(want[e["arr"]][sl(box)].shape)
        for e in entries:
            assert same(arrays[e["arr"]][sl(e["box"])], want[e["arr"]][sl(e["box"])]), e["why"]
        for n, t in arrays.items():
            assert same(t, want[n]), "array %s changed outside its boxes" % n
        for i, b in enumerate(bufs):
            assert same(b, buf0[i]), "unpack changed buffer %d" % i


@pytest.mark.parametrize("pack", [True, False], ids=["pack", "unpack"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_box_list(gpu, dt, pack):
    """k_box_list over the mixed 13-entry table (boxlist_entries): every part
    exact, NaN / sentinel everywhere else, the source side unchanged."""
    ops = make_ops("hip", None, gpu, DT[dt])
    r = run_boxlist(ops, dt, gpu, pack)
    torch.cuda.synchronize()
    check_boxlist(r)


def one_entry(dt):
    return [dict(arr="local", box=((1, 1, 4), (4, 6, 12)), buf=0, off=4, why="a table of one entry",
                 claim=dict(form="vec", blocks=1))], [4 + 120 + 5, 8]


@pytest.mark.parametrize("pack", [True, False], ids=["pack", "unpack"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_box_list_one_entry(gpu, dt, pack):
    """n = 1: the binary search has nothing to halve."""
    ops = make_ops("hip", None, gpu, DT[dt])
    r = run_boxlist(ops, dt, gpu, pack, *one_entry(dt))
    torch.cuda.synchronize()
    check_boxlist(r)


def boxlist_host_errors(device):
    t = torch.zeros((4, 5, 8), dtype=torch.float32, device=device)
    buf = torch.zeros(64, dtype=torch.float32, device=device)
    bad = [
        ("box past the array's end", t, ((0, 0, 0), (4, 5, 9)), buf, 0),
        ("box below zero", t, ((-1, 0, 0), (2, 2, 2)), buf, 0),
        ("empty box", t, ((1, 2, 3), (3, 2, 5)), buf, 0),
        ("buffer part past the buffer's end", t, ((0, 0, 0), (2, 4, 8)), buf, 1),
        ("buffer of another dtype", t, ((0, 0, 0), (1, 1, 1)), buf.double(), 0),
    ]
    for why, arr, box, b, off in bad:
        with pytest.raises(ValueError):
            _BoxList().add(arr, box, b, off)
            pytest.fail("accepted: " + why)
    _BoxList().add(t, ((0, 0, 0), (2, 4, 8)), buf, 0)  # the same part at offset 0 fits exactly


def test_box_list_host_errors(gpu):
    boxlist_host_errors(gpu)


# ===================================== 2. pack / unpack / copy_box at their limits
# name, shape, ncomp, box (None: whole), dtypes, base, why, claim (path: vec / scalar / masked; sweeps of the
# grid-stride loop; gridz)
def _whole(shape):
    return ((0, 0, 0), tuple(shape))


PACK_CASES = [
    dict(name="stride-scalar", shape=(2, 515, 511), ncomp=1, box=None, dts=("f32", "f64"), base="aligned",
         why="odd nz: scalar path, a plane of 263165 cells > 1024 x 256", claim=dict(path="scalar", sweeps=2)),
    dict(name="stride-vec-f32", shape=(1, 1028, 1024), ncomp=1, box=None, dts=("f32",), base="aligned",
         why="fp32 vector path, 263168 groups a plane", claim=dict(path="vec", sweeps=2)),
    dict(name="stride-vec-f64", shape=(1, 516, 1024), ncomp=1, box=None, dts=("f64",), base="aligned",
         why="fp64 vector path, 264192 groups a plane", claim=dict(path="vec", sweeps=2)),
    dict(name="eight-comps", shape=(3, 5, 8), ncomp=8, box=((0, 1, 0), (3, 4, 8)), dts=("f32", "f64"),
         base="aligned", why="the component limit itself", claim=dict(path="vec", sweeps=1, gridz=24)),
    dict(name="gridz-65535", shape=(13107, 1, 4), ncomp=5, box=None, dts=("f32", "f64"), base="aligned",
         why="grid.z = 13107 x 5 = 65535, the largest allowed", claim=dict(path="vec", sweeps=1, gridz=65535)),
    dict(name="odd-base", shape=(5, 6, 16), ncomp=3, box=((1, 1, 4), (4, 5, 12)), dts=("f32", "f64"), base="odd",
         why="aligned box of arrays whose bases are not 16-byte aligned: scalar fallback",
         claim=dict(path="scalar", sweeps=1)),
]
XFER_CASES = [
    PACK_CASES[0], PACK_CASES[1], PACK_CASES[2],
    dict(name="stride-masked-f32", shape=(1, 1028, 1024), ncomp=1, box=((0, 0, 1), (1, 1028, 1024)), dts=("f32",),
         base="aligned", why="unaligned z range on aligned rows: k_box_xfer_m over 1028 x 256 groups",
         claim=dict(path="masked", sweeps=2)),
    dict(name="stride-masked-f64", shape=(1, 516, 1024), ncomp=1, box=((0, 0, 1), (1, 516, 1024)), dts=("f64",),
         base="aligned", why="unaligned z range on aligned rows: k_box_xfer_m over 516 x 512 groups",
         claim=dict(path="masked", sweeps=2)),
    PACK_CASES[3], PACK_CASES[4], PACK_CASES[5],
]
# limits that must raise and write nothing: name, shape, ncomp
LIMIT_CASES = [("nine-comps", (3, 5, 8), 9), ("gridz-65536", (8192, 1, 4), 8)]


def case_box(case):
    return case["box"] if case["box"] is not None else _whole(case["shape"])


def copy_claims(case, dt, xfer, buf_aligned=True):
    """(path, sweeps, grid.z) of a pack / unpack (``xfer`` False) or copy_box
    launch: box_copy_grid and the path choice of the module docstring."""
    V = VW[dt]
    box, nz = case_box(case), case["shape"][2]
    bx, by, bz = (box[1][d] - box[0][d] for d in range(3))
    al = case["base"] == "aligned" and (xfer or buf_aligned)
    if al and nz % V == 0 and box[0][2] % V == 0 and bz % V == 0:
        path, work, blocks = "vec", by * (bz // V), cdiv(by * bz // V, 256)
    elif xfer and al and nz % V == 0:
        ng = cdiv(box[1][2] - (box[0][2] & ~(V - 1)), V)
        path, work, blocks = "masked", by * ng, cdiv(by * bz // V, 256)
    else:
        path, work, blocks = "scalar", by * bz, cdiv(by * bz, 256)
    blocks = min(1024, blocks)
    return path, cdiv(work, blocks * 256), bx * case["ncomp"]


def assert_copy_claims(case, dt, xfer):
    path, sweeps, gridz = copy_claims(case, dt, xfer)
    c = case["claim"]
    assert path == c["path"] and sweeps == c["sweeps"] and gridz == c.get("gridz", gridz), (case["why"], path, sweeps)
    assert gridz <= 65535 and case["ncomp"] <= 8
    box = case_box(case)
    if c["sweeps"] > 1:  # the last element of the plane is in the box
        assert box[1][1] == case["shape"][1] and box[1][2] == case["shape"][2]


def run_pack(ops, case, dt, device, buf_off=0):
    box = case_box(case)
    fields = [live(case["shape"], 100 + c, dt, device, case["base"]) for c in range(case["ncomp"])]
    n = vol(box) * case["ncomp"]
    big = torch.full((n + buf_off + 4,), NAN, dtype=DT[dt], device=device)
    before = [f.clone() for f in fields]
    ops.pack(fields, box, big[buf_off:buf_off + n])
    return dict(box=box, fields=fields, before=before, big=big, off=buf_off, n=n)


def check_pack(r):
    want = torch.full_like(r["big"], NAN)
    want[r["off"]:r["off"] + r["n"]] = torch.cat([f[sl(r["box"])].reshape(-1) for f in r["before"]])
    assert same(r["big"], want)
    for f, f0 in zip(r["fields"], r["before"]):
        assert same(f, f0), "pack changed a field"


def run_unpack(ops, case, dt, device):
    box = case_box(case)
    n = vol(box) * case["ncomp"]
    buf = live((n,), 200, dt, device)
    fields = [filled(case["shape"], SENT, dt, device, case["base"]) for _ in range(case["ncomp"])]
    buf0 = buf.clone()
    ops.unpack(fields, box, buf)
    return dict(box=box, fields=fields, buf=buf, buf0=buf0)


def check_unpack(r):
    box, m = r["box"], vol(r["box"])
    for c, f in enumerate(r["fields"]):
        want = torch.full_like(f, SENT)
        want[sl(box)] = r["buf0"][c * m:(c + 1) * m].view(want[sl(box)].shape)
        assert same(f, want), "component %d" % c
    assert same(r["buf"], r["buf0"]), "unpack changed the buffer"


def run_xfer(ops, case, dt, device):
    box = case_box(case)
    src = [live(case["shape"], 300 + c, dt, device, case["base"]) for c in range(case["ncomp"])]
    dst = [filled(case["shape"], SENT, dt, device, case["base"]) for _ in range(case["ncomp"])]
    src0 = [s.clone() for s in src]
    ops.copy_box(src, dst, box)
    return dict(box=box, src=src, src0=src0, dst=dst)


def check_xfer(r):
    for c, (s, s0, d) in enumerate(zip(r["src"], r["src0"], r["dst"])):
        want = torch.full_like(d, SENT)
        want[sl(r["box"])] = s0[sl(r["box"])]
        assert same(d, want), "component %d" % c
        assert same(s, s0), "copy_box changed a source"


def _ids(cases):
    return [(c, dt) for c in cases for dt in c["dts"]], ["%s-%s" % (c["name"], dt) for c in cases for dt in c["dts"]]


@pytest.mark.parametrize("case,dt", _ids(PACK_CASES)[0], ids=_ids(PACK_CASES)[1])
def test_pack_unpack_limits(gpu, case, dt):
    ops = make_ops("hip", None, gpu, DT[dt])
    assert_copy_claims(case, dt, False)
    r = run_pack(ops, case, dt, gpu)
    torch.cuda.synchronize()
    check_pack(r)
    r = run_unpack(ops, case, dt, gpu)
    torch.cuda.synchronize()
    check_unpack(r)


@pytest.mark.parametrize("case,dt", _ids(XFER_CASES)[0], ids=_ids(XFER_CASES)[1])
def test_copy_box_limits(gpu, case, dt):
    ops = make_ops("hip", None, gpu, DT[dt])
    assert_copy_claims(case, dt, True)
    r = run_xfer(ops, case, dt, gpu)
    torch.cuda.synchronize()
    check_xfer(r)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("name,shape,ncomp", LIMIT_CASES, ids=[c[0] for c in LIMIT_CASES])
def test_copy_limits_refused(gpu, name, shape, ncomp, dt):
    """Nine components, or (x extent) x ncomp = 65536 > grid.z: pack, unpack
    and copy_box raise HipError and write nothing."""
    ops = make_ops("hip", None, gpu, DT[dt])
    box = _whole(shape)
    assert ncomp > 8 or shape[0] * ncomp == 65536
    n = vol(box) * ncomp
    src = [live(shape, 400 + c, dt, gpu) for c in range(ncomp)]
    src0 = [s.clone() for s in src]
    buf = torch.full((n,), NAN, dtype=DT[dt], device=gpu)
    with pytest.raises(HipError):
        ops.pack(src, box, buf)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    buf = live((n,), 401, dt, gpu)
    dst = [filled(shape, SENT, dt, gpu) for _ in range(ncomp)]
    with pytest.raises(HipError):
        ops.unpack(dst, box, buf)
    with pytest.raises(HipError):
        ops.copy_box(src, dst, box)
    torch.cuda.synchronize()
    for s, s0, d in zip(src, src0, dst):
        assert same(s, s0) and same(d, torch.full_like(d, SENT))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_pack_unpack_refuse_bad_buffer(gpu, dt):
    """A buffer of another dtype, on another device or non-contiguous is
    refused (it used to be checked for its numel() alone) and nothing is
    written."""
    ops = make_ops("hip", None, gpu, DT[dt])
    shape, box = (3, 4, 8), ((0, 1, 0), (3, 3, 8))
    n = vol(box) * 2
    other = torch.float64 if dt == "f32" else torch.float32
    bad = {"dtype": torch.full((n,), NAN, dtype=other, device=gpu),
           "device": torch.full((n,), NAN, dtype=DT[dt]),
           "non-contiguous": torch.full((2 * n,), NAN, dtype=DT[dt], device=gpu)[::2]}
    src = [live(shape, 410 + c, dt, gpu) for c in range(2)]
    dst = [filled(shape, SENT, dt, gpu) for _ in range(2)]
    for why, buf in bad.items():
        with pytest.raises(HipError):
            ops.pack(src, box, buf)
            pytest.fail("pack accepted a buffer of another " + why)
        with pytest.raises(HipError):
            ops.unpack(dst, box, buf)
            pytest.fail("unpack accepted a buffer of another " + why)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all())
    for d in dst:
        assert same(d, torch.full_like(d, SENT))


# ================================================================ 3. maxabs
MA_SHAPE, MA_BOX = (6, 7, 10), ((1, 2, 3), (5, 6, 9))
MA_BIG = (70, 128, 128)  # 1146880 cells > 4096 x 256: the stride loop runs twice


def _set(idx, v):
    return lambda t: t.__setitem__(idx, v)


def _face(axis, side):
    """A larger magnitude just outside one face of MA_BOX, next to the
    planted in-box maximum."""
    idx = [3, 4, 6]
    idx[axis] = MA_BOX[0][axis] - 1 if side == 0 else MA_BOX[1][axis]
    return tuple(idx)


def _fill_box(v):
    return lambda t: t[sl(MA_BOX)].fill_(v)


# name, shape, box, edits (applied in order to the fp64 draw in (-1, 1)), dtypes, why, expected result (None: the
# reference alone decides), cpu: runs on the torch backend too (which returns the fp64 maximum unrounded)
MAXABS_CASES = [
    dict(name="first-cell", edits=[_set((1, 2, 3), 5.0)], why="maximum in the first cell of the box", expect=5.0),
    dict(name="last-cell", edits=[_set((4, 5, 8), 5.0)], why="maximum in the last cell of the box", expect=5.0),
    dict(name="negative", edits=[_set((3, 4, 6), -5.0)], why="the maximum is a negative value", expect=5.0),
] + [
    dict(name="outside-%s%s" % ("xyz"[a], "-+"[s]), edits=[_set((3, 4, 6), 5.0), _set(_face(a, s), -9.0 if s else 9.0)],
         why="a larger magnitude just outside the %s%s face is ignored" % ("-+"[s], "xyz"[a]), expect=5.0)
    for a in range(3) for s in range(2)
] + [
    dict(name="nan-inside", edits=[_set((3, 4, 6), NAN)], why="NaN inside the box gives inf", expect=INF),
    dict(name="nan-outside", edits=[_set((3, 4, 6), 5.0), _set((0, 0, 0), NAN), _set((3, 4, 9), NAN)],
         why="NaN only outside the box: the finite maximum", expect=5.0),
    dict(name="plus-inf", edits=[_set((2, 3, 4), INF)], why="+inf inside", expect=INF),
    dict(name="minus-inf", edits=[_set((2, 3, 4), -INF)], why="-inf inside", expect=INF),
    dict(name="zeros", edits=[_fill_box(0.0)], why="an all-zero box", expect=0.0),
    dict(name="minus-zeros", edits=[_fill_box(-0.0)], why="a box of -0.0", expect=0.0),
    dict(name="f64-inexact", edits=[_set((3, 4, 6), 4.0 / 3.0)], dts=("f64",), cpu=False,
         why="a maximum that fp32 cannot represent is rounded to nearest", expect=None),
    dict(name="f64-below-subnormal", edits=[_fill_box(1e-50), _set((3, 4, 6), -3e-46)], dts=("f64",), cpu=False,
         why="a maximum below the smallest fp32 subnormal (1.4e-45) gives 0", expect=0.0),
    dict(name="f64-above-fltmax", edits=[_set((3, 4, 6), 1e39)], dts=("f64",), cpu=False,
         why="a finite maximum above FLT_MAX gives inf: check_finite reports such a field as non-finite (pinned, "
             "see HipOps.maxabs)", expect=INF),
    dict(name="stride-second-sweep", shape=MA_BIG, box=_whole(MA_BIG), edits=[_set((67, 5, 9), -5.0)],
         why="the maximum lies where only the second sweep of the stride loop reaches", expect=5.0, second=(67, 5, 9)),
    dict(name="stride-last-cell", shape=MA_BIG, box=_whole(MA_BIG), edits=[_set((69, 127, 127), 5.0)],
         why="the maximum in the very last cell of a two-sweep box", expect=5.0, second=(69, 127, 127)),
]
for _c in MAXABS_CASES:
    _c.setdefault("shape", MA_SHAPE)
    _c.setdefault("box", MA_BOX)
    _c.setdefault("dts", ("f32", "f64"))
    _c.setdefault("cpu", True)

_MA_DRAW = {}


def maxabs_input(case, dt, device):
    """The case's array: one shared fp64 draw per shape (left unchanged),
    the edits applied to a copy."""
    shape = case["shape"]
    if shape not in _MA_DRAW:
        g = torch.Generator().manual_seed(5)
        _MA_DRAW[shape] = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1
    t = _MA_DRAW[shape].clone()
    for e in case["edits"]:
        e(t)
    return t.to(DT[dt]).to(device)


def maxabs_ref(t, box):
    """float32(max |t[box]|), NaN -> inf."""
    v = t[sl(box)].abs()
    if bool(torch.isnan(v).any()):
        return INF
    return float(v.max().to(torch.float32))


def maxabs_claims(case):
    """The planted cell of a stride case lies past the first sweep of
    reduce_grid's min(4096, ceil(n / 256)) blocks of 256."""
    if "second" in case:
        box = case["box"]
        n = vol(box)
        i, j, k = case["second"]
        flat = (i * case["shape"][1] + j) * case["shape"][2] + k  # the box is the whole array
        assert box == _whole(case["shape"]) and flat >= min(4096, cdiv(n, 256)) * 256 and flat < n, case["why"]


def run_maxabs(ops, case, dt, device):
    t = maxabs_input(case, dt, device)
    t0 = t.clone()
    return dict(case=case, t=t, t0=t0, got=ops.maxabs(t, case["box"]))


def check_maxabs(r):
    case = r["case"]
    want = maxabs_ref(r["t0"].cpu(), case["box"])
    if case["expect"] is not None:
        assert want == case["expect"], (case["why"], want)
    assert r["got"] == want and not math.isnan(r["got"]), (case["why"], r["got"], want)
    assert same(r["t"], r["t0"]), "maxabs changed its input"


_MA = _ids(MAXABS_CASES)


@pytest.mark.parametrize("case,dt", _MA[0], ids=_MA[1])
def test_maxabs(gpu, case, dt):
    ops = make_ops("hip", None, gpu, DT[dt])
    maxabs_claims(case)
    check_maxabs(run_maxabs(ops, case, dt, gpu))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_maxabs_scratch_reset(gpu, dt):
    """Two calls on one ops object, the larger maximum first: the second
    returns its own, smaller one (the scratch word is reset per call)."""
    ops = make_ops("hip", None, gpu, DT[dt])
    big = dict(MAXABS_CASES[0], edits=[_set((3, 4, 6), 1000.0)], expect=1000.0)
    small = dict(MAXABS_CASES[0], edits=[_fill_box(0.125)], expect=0.125)
    check_maxabs(run_maxabs(ops, big, dt, gpu))
    check_maxabs(run_maxabs(ops, small, dt, gpu))


# ============================================================= 4. amplitude
ACC = 2.0 ** -10
AMP_NX, AMP_NY = 6, 11


def amp_boxes(kind, nz):
    """Six different boxes (the real Yee update boxes of the (6, 11, nz) grid
    among them) or three."""
    yee = {c: YeeLayout(size=(AMP_NX, AMP_NY, nz)).global_range(c) for c in COMPS}
    partial = ((1, 2, 5), (5, 9, nz - 5))      # lo.z, hi.z no multiples of 4: partial masks at both ends
    thin = ((0, 0, 33), (AMP_NX, AMP_NY, 34))  # one cell thick in z
    empty = ((2, 2, 9), (2, 5, 30))            # empty among non-empty ones
    if kind == "six":
        return [yee["Ex"], partial, thin, empty, yee["Hy"], yee["Hz"]]
    return [partial, empty, yee["Ez"]]


# name, nz, dtype, boxes, amp form (shared: views of one [x][6][y][z] buffer; separate), base, claimed kernel
AMP_CASES = [
    dict(name="six-shared-v4", nz=72, dt="f32", boxes="six", form="shared", base="aligned", kernel="v4",
         why="fp32, nz % 4 == 0, aligned: the float4 kernel on the scheme's own amp layout"),
    dict(name="three-separate-v4", nz=72, dt="f32", boxes="three", form="separate", base="aligned", kernel="v4",
         why="three components, separate contiguous amp arrays"),
    dict(name="nz70-six-shared", nz=70, dt="f32", boxes="six", form="shared", base="aligned", kernel="many_f32",
         why="nz % 4 != 0: the scalar fp32 kernel"),
    dict(name="nz70-three-separate", nz=70, dt="f32", boxes="three", form="separate", base="aligned",
         kernel="many_f32", why="scalar fp32 kernel, three components"),
    dict(name="oddbase-six-separate", nz=72, dt="f32", boxes="six", form="separate", base="odd", kernel="many_f32",
         why="aligned nz but bases not 16-byte aligned: the scalar fp32 kernel"),
    dict(name="six-shared-f64", nz=72, dt="f64", boxes="six", form="shared", base="aligned", kernel="many_f64",
         why="fp64 on the shared buffer"),
    dict(name="three-separate-f64", nz=70, dt="f64", boxes="three", form="separate", base="aligned",
         kernel="many_f64", why="fp64, odd-sized rows, three components"),
]
# k_amplitude_update<T>, one component a call: name, nz, dtype, box set
AMP1_CASES = [dict(name="single-%s-nz%d" % (dt, nz), nz=nz, dt=dt, boxes="six",
                   why="k_amplitude_update<%s>, the six boxes one call each, rows of %d" % (dt, nz))
              for dt in ("f32", "f64") for nz in (72, 70)]


def amp_claims(case):
    """The kernel and its grid from amplitude_many's formulas; more than one
    workgroup in y, and two in z for the scalar form."""
    boxes = [b for b in amp_boxes(case["boxes"], case["nz"]) if vol(b)]
    assert len(amp_boxes(case["boxes"], case["nz"])) == (6 if case["boxes"] == "six" else 3)
    u = (tuple(min(b[0][d] for b in boxes) for d in range(3)), tuple(max(b[1][d] for b in boxes) for d in range(3)))
    v4 = case["dt"] == "f32" and case["nz"] % 4 == 0 and case["base"] == "aligned"
    kernel = "v4" if v4 else "many_" + case["dt"]
    assert kernel == case["kernel"], case["why"]
    gy, gx = cdiv(u[1][1] - u[0][1], 4), u[1][0] - u[0][0]
    gz = cdiv(u[1][2] - (u[0][2] & ~3), 256) if v4 else cdiv(u[1][2] - u[0][2], 64)
    assert gy > 1 and gx > 1 and gz == (1 if v4 else 2), (case["why"], gx, gy, gz)
    partial = [b for b in boxes if b[0][2] % 4 and b[1][2] % 4]
    assert partial and len(boxes) < case_ncomp(case)  # partial masks at both ends; one box is empty
    assert case["boxes"] != "six" or any(b[1][2] - b[0][2] == 1 for b in boxes)
    return kernel, (gz, gy, gx)


def case_ncomp(case):
    return 6 if case["boxes"] == "six" else 3


def amp_draw(nz, ncomp, seed=77):
    """fp64 fields f, running maxima a and the change mask they are built
    for, per component: every cell from one of eight categories, none near
    the threshold (growth 0, 2^-12 or >= 2^-8 against ACC = 2^-10).  ``a`` is
    fp32-representable, so both dtypes see the same maxima."""
    g = torch.Generator().manual_seed(seed)
    shape = (ncomp, AMP_NX, AMP_NY, nz)
    cat = torch.randint(0, 8, shape, generator=g)
    a = (torch.rand(shape, generator=g, dtype=torch.float64) * 1.5 + 0.5).float().double()
    u = torch.rand(shape, generator=g, dtype=torch.float64) * 0.2
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()
    growth = {4: 2.0 ** -12, 5: 2.0 ** -8, 6: 0.5, 7: 3.0}
    mag = a.clone()                                     # 3: |f| == a exactly
    mag = torch.where(cat == 0, torch.zeros_like(a), mag)
    mag = torch.where(cat == 1, a, mag)                 # a = 0 below, f != 0
    mag = torch.where(cat == 2, a * u, mag)             # |f| <= 0.2 a
    for c, gr in growth.items():
        mag = torch.where(cat == c, a * (1 + gr), mag)
    a = torch.where(cat <= 1, torch.zeros_like(a), a)
    change = (cat == 1) | (cat >= 5)
    return sign * mag, a, change


def amp_oracle(f, a, acc):
    """Scheme3D::updateAmplitude in fp64: the change mask."""
    v = f.abs()
    den = torch.where(a != 0, a, torch.where(v != 0, v, torch.ones_like(v)))
    return (v >= a) & ((v - a) / den > acc)


def amp_state(case, device):
    """Fields, sentinel-filled amp arrays holding the maxima inside each
    component's box, the boxes, and per component the reference (new amp
    array, count) of a first call and of a second one on fields scaled by 4
    (exact in both dtypes; every growth is then about 3, or 4 |f| <= 0.8 a)."""
    nz, dt, ncomp = case["nz"], case["dt"], case_ncomp(case)
    boxes = amp_boxes(case["boxes"], nz)
    f64, a64, change = amp_draw(nz, ncomp)
    shape = (AMP_NX, AMP_NY, nz)
    base = case.get("base", "aligned")
    fields = [place(f64[c].to(DT[dt]).reshape(-1), shape, device, base) for c in range(ncomp)]
    if case.get("form") == "shared":
        store = filled((AMP_NX, 6, AMP_NY, nz), SENT, dt, device, base)
        amps = [store[:, c] for c in range(ncomp)]
    else:
        store = None
        amps = [filled(shape, SENT, dt, device, base) for _ in range(ncomp)]
    refs = []
    for c in range(ncomp):
        s = sl(boxes[c])
        amps[c][s] = a64[c][s].to(DT[dt]).to(device)
        fd = f64[c].to(DT[dt]).double()  # the values the kernel reads
        ad = a64[c]
        m1 = amp_oracle(fd, ad, ACC)
        assert bool(torch.equal(m1[s], change[c][s]))  # the draw's categories decide as designed
        a1 = torch.where(m1, fd.abs(), ad)
        m2 = amp_oracle(4 * fd, a1, ACC)
        a2 = torch.where(m2, 4 * fd.abs(), a1)
        want1 = torch.full(shape, SENT, dtype=DT[dt])
        want1[s] = a1[s].to(DT[dt])
        want2 = torch.full(shape, SENT, dtype=DT[dt])
        want2[s] = a2[s].to(DT[dt])
        refs.append(dict(want1=want1, n1=int(m1[s].sum()), want2=want2, n2=int(m2[s].sum())))
    return dict(case=case, fields=fields, amps=amps, store=store, boxes=boxes, refs=refs)


def run_amp_many(ops, case, device):
    st = amp_state(case, device)
    counter = torch.full((1,), 1000, dtype=torch.int32, device=device)
    f0 = [f.clone() for f in st["fields"]]
    ops.amplitude_update_many(st["fields"], st["amps"], st["boxes"], ACC, counter)
    first = dict(amps=[a.clone() for a in st["amps"]], store=None if st["store"] is None else st["store"].clone(),
                 counter=int(counter.item()), fields=[f.clone() for f in st["fields"]])
    f4 = [place((4 * f).reshape(-1), tuple(f.shape), device, case["base"]) for f in st["fields"]]
    ops.amplitude_update_many(f4, st["amps"], st["boxes"], ACC, counter)
    st.update(f0=f0, first=first, counter=int(counter.item()))
    return st


def check_amp_many(st):
    refs, first = st["refs"], st["first"]
    n1, n2 = sum(r["n1"] for r in refs), sum(r["n2"] for r in refs)
    assert n1 > 0 and n2 > 0
    for c, r in enumerate(refs):
        assert same(first["amps"][c].cpu(), r["want1"]), "component %d, first call" % c
        assert same(st["amps"][c].cpu(), r["want2"]), "component %d, second call" % c
        assert same(first["fields"][c], st["f0"][c]) and same(st["fields"][c], st["f0"][c]), "field %d changed" % c
    if st["store"] is not None:  # the planes of the shared buffer that no component owns
        for store in (first["store"], st["store"]):
            rest = store[:, len(refs):]
            assert same(rest, torch.full_like(rest, SENT)), "a plane of another component changed"
    assert first["counter"] == 1000 + n1, (first["counter"], n1)
    assert st["counter"] == 1000 + n1 + n2, (st["counter"], n1, n2)


@pytest.mark.parametrize("case", AMP_CASES, ids=[c["name"] for c in AMP_CASES])
def test_amplitude_update_many(gpu, case):
    ops = make_ops("hip", None, gpu, DT[case["dt"]])
    amp_claims(case)
    st = run_amp_many(ops, case, gpu)
    torch.cuda.synchronize()
    check_amp_many(st)


def run_amp_single(ops, case, device):
    st = amp_state(case, device)
    f0 = [f.clone() for f in st["fields"]]
    st["counts"] = [ops.amplitude_update(f, a, b, ACC) for f, a, b in zip(st["fields"], st["amps"], st["boxes"])]
    st["f0"] = f0
    return st


def check_amp_single(st):
    for c, r in enumerate(st["refs"]):
        assert same(st["amps"][c].cpu(), r["want1"]), "component %d" % c
        assert st["counts"][c] == r["n1"], (c, st["counts"][c], r["n1"])
        assert same(st["fields"][c], st["f0"][c]), "field %d changed" % c
    assert sum(st["counts"]) > 0 and 0 in st["counts"]  # the empty box counts nothing


@pytest.mark.parametrize("case", AMP1_CASES, ids=[c["name"] for c in AMP1_CASES])
def test_amplitude_update(gpu, case):
    ops = make_ops("hip", None, gpu, DT[case["dt"]])
    st = run_amp_single(ops, case, gpu)
    check_amp_single(st)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_amplitude_many_refuses_mismatched_lists(gpu, dt):
    """Fewer boxes (or amp arrays) than fields made the kernel wrapper read
    past the host array of boxes: refused now, nothing written."""
    ops = make_ops("hip", None, gpu, DT[dt])
    st = amp_state(dict(AMP_CASES[1], dt=dt), gpu)
    a0 = [a.clone() for a in st["amps"]]
    counter = torch.full((1,), 7, dtype=torch.int32, device=gpu)
    for f, a, b in ((st["fields"], st["amps"], st["boxes"][:2]), (st["fields"], st["amps"][:2], st["boxes"]),
                    (st["fields"][:2], st["amps"], st["boxes"]), (st["fields"] * 3, st["amps"] * 3, st["boxes"] * 3)):
        with pytest.raises(HipError):
            ops.amplitude_update_many(f, a, b, ACC, counter)
    torch.cuda.synchronize()
    assert int(counter.item()) == 7 and all(same(a, b) for a, b in zip(st["amps"], a0))


# ================================== 5. sources and the graph-replay helpers
SRC_SHAPE = (7, 9, 17)
SRC_VALUE = 0.1 + 2.0 ** -30  # not representable in fp32 (nor is 0.1)
SRC_CELLS = [(0, 0, 0), (6, 8, 16), (3, 4, 5)]


def run_set_value(ops, dt, device, idx, value=SRC_VALUE):
    t = filled(SRC_SHAPE, SENT, dt, device)
    ops.set_value(t, idx, value)
    return dict(t=t, cells={tuple(idx): value})


def check_cells(r):
    """The named cells hold dtype(value) exactly, every other cell the
    sentinel."""
    t = r["t"].cpu()
    want = torch.full_like(t, SENT)
    for idx, v in r["cells"].items():
        want[idx] = torch.tensor(v, dtype=torch.float64).to(t.dtype)
    assert same(t, want)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_set_value(gpu, dt):
    ops = make_ops("hip", None, gpu, DT[dt])
    assert float(torch.tensor(SRC_VALUE, dtype=torch.float64).float()) != SRC_VALUE
    for idx in SRC_CELLS:
        check_cells(run_set_value(ops, dt, gpu, idx))
    t = filled(SRC_SHAPE, SENT, dt, gpu)
    for idx in ((7, 0, 0), (0, 9, 0), (0, 0, 17), (-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        with pytest.raises(HipError):
            ops.set_value(t, idx, 1.0)
    torch.cuda.synchronize()
    assert same(t, torch.full_like(t, SENT))


SET_VALUES_N = [1, 256, 257, 1000]


def set_values_offsets(n):
    """n unsorted distinct flat offsets; the last element always, offset 0
    too from n = 2 on."""
    total = math.prod(SRC_SHAPE)
    g = torch.Generator().manual_seed(900 + n)
    perm = torch.randperm(total - 2, generator=g)[:max(0, n - 2)] + 1
    offs = torch.cat([torch.tensor([total - 1]), perm, torch.tensor([0])])[:n] if n > 1 else torch.tensor([total - 1])
    offs = offs[torch.randperm(n, generator=g)]
    assert offs.numel() == n and offs.unique().numel() == n and int(offs.max()) == total - 1
    assert n == 1 or (int(offs.min()) == 0 and not bool(torch.equal(offs, offs.sort().values)))
    return offs.to(torch.int64)


def run_set_values(ops, dt, device, n, value=SRC_VALUE):
    t = filled(SRC_SHAPE, SENT, dt, device)
    offs = set_values_offsets(n).to(device)
    offs0 = offs.clone()
    ops.set_values(t, offs, value)
    assert bool(torch.equal(offs, offs0))
    ny, nz = SRC_SHAPE[1:]
    cells = {(o // (ny * nz), o // nz % ny, o % nz): value for o in offs.cpu().tolist()}
    return dict(t=t, cells=cells)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_set_values(gpu, dt):
    ops = make_ops("hip", None, gpu, DT[dt])
    for n in SET_VALUES_N:
        check_cells(run_set_values(ops, dt, gpu, n))
    t = filled(SRC_SHAPE, SENT, dt, gpu)
    ops.set_values(t, torch.zeros(0, dtype=torch.int64, device=gpu), 1.0)  # empty: a no-op
    with pytest.raises(HipError):
        ops.set_values(t, torch.tensor([1, 2], dtype=torch.int32, device=gpu), 1.0)
    with pytest.raises(HipError):
        ops.set_values(t, torch.tensor([1, 2], dtype=torch.int64), 1.0)
    torch.cuda.synchronize()
    assert same(t, torch.full_like(t, SENT))


def source_table(device):
    """About 40 doubles, none representable in fp32."""
    g = torch.Generator().manual_seed(41)
    tab = torch.rand(40, generator=g, dtype=torch.float64) * 2 - 1
    assert bool((tab.float().double() != tab).all())
    return tab.to(device)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_set_value_tab_counter(gpu, dt):
    """k_set_value_tab writes dtype(tab[counter + lag]); k_counter_add moves
    the counter in stream order, with no synchronisation in between."""
    ops = make_ops("hip", None, gpu, DT[dt])
    tab = source_table(gpu)
    tab0 = tab.clone()
    for cnt, lag in ((0, 0), (0, 5), (17, 0), (30, 9), (12, -3)):
        counter = torch.tensor([cnt], dtype=torch.int32, device=gpu)
        t = filled(SRC_SHAPE, SENT, dt, gpu)
        ops.set_value_tab(t, SRC_CELLS[2], tab, counter, lag)
        check_cells(dict(t=t, cells={SRC_CELLS[2]: float(tab0[cnt + lag])}))
        assert int(counter.item()) == cnt
    counter = torch.tensor([10], dtype=torch.int32, device=gpu)
    t = filled(SRC_SHAPE, SENT, dt, gpu)
    A, B, C = SRC_CELLS
    ops.set_value_tab(t, A, tab, counter, 0)
    ops.counter_add(counter, 3)
    ops.set_value_tab(t, B, tab, counter, 2)
    ops.counter_add(counter, -1)
    ops.set_value_tab(t, C, tab, counter, 0)
    check_cells(dict(t=t, cells={A: float(tab0[10]), B: float(tab0[15]), C: float(tab0[12])}))
    assert int(counter.item()) == 12 and same(tab, tab0)
    with pytest.raises(HipError):
        ops.set_value_tab(t, A, tab.float(), counter, 0)
    with pytest.raises(HipError):
        ops.set_value_tab(t, A, tab, counter.long(), 0)
    with pytest.raises(HipError):
        ops.set_value_tab(t, (0, 0, 17), tab, counter, 0)


INC_LENGTHS = [2, 255, 256, 257, 1001]
INC_COEF = 0.37


def inc_bound(dt, e0, h, coef):
    """|result - fp64 expression| per cell of ``e[i] += c (h[i-1] - h[i])``
    in T with unit roundoff u: c rounded to T (u), the difference (u), the
    product (u, none if contracted to an FMA) and the sum (u of the result,
    itself at most |e| + |c| (|h0| + |h1|) (1 + 3u)) -- within
    4u (|e| + |c| (|h0| + |h1|))."""
    u = 2.0 ** -24 if dt == "f32" else 2.0 ** -53
    return 4 * u * (e0[1:].abs() + abs(coef) * (h[:-1].abs() + h[1:].abs()))


def run_inc_e(ops, dt, device, n, source):
    """inc_step_e on a live line."""
    e, h = live((n,), 500 + n, dt, device), live((n,), 600 + n, dt, device)
    e0, h0 = e.clone(), h.clone()
    ops.inc_step_e(e, h, INC_COEF, source)
    return dict(dt=dt, e=e, e0=e0, h=h, h0=h0, source=source)


def check_inc_e(r):
    e0, h0 = r["e0"].cpu().double(), r["h0"].cpu().double()
    want = e0.clone()
    want[1:] += INC_COEF * (h0[:-1] - h0[1:])
    got = r["e"].cpu()
    assert same(got[:1], torch.tensor([r["source"]], dtype=torch.float64).to(got.dtype))
    err = (got.double()[1:] - want[1:]).abs()
    assert bool((err <= inc_bound(r["dt"], e0, h0, INC_COEF)).all()), float(err.max())
    assert same(r["h"], r["h0"]), "the H line changed"


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_inc_step_e_tab(gpu, dt):
    """k_inc_e_tab == k_inc_e with source = tab[counter + lag], bit for bit,
    and both within rounding of the fp64 expression."""
    ops = make_ops("hip", None, gpu, DT[dt])
    tab = source_table(gpu)
    for n in INC_LENGTHS:
        cnt, lag = n % 30, 7
        counter = torch.tensor([cnt], dtype=torch.int32, device=gpu)
        r = run_inc_e(ops, dt, gpu, n, float(tab[cnt + lag]))
        check_inc_e(r)
        e = r["e0"].clone()
        ops.inc_step_e_tab(e, r["h"], INC_COEF, tab, counter, lag)
        assert same(e, r["e"]), n
        assert same(r["h"], r["h0"]) and int(counter.item()) == cnt


# ============================================================= 6. scattered
def _dir(theta, phi):
    t, p = math.radians(theta), math.radians(phi)
    return (math.sin(t) * math.cos(p), math.sin(t) * math.sin(p), math.cos(t))


OBLIQUE = _dir(50, 35)
SC_SHAPE, SC_ORG = (7, 6, 9), (3, 2, 5)
SC_L, SC_R = (5.0, 4.0, 7.0), (8.0, 7.0, 12.0)  # integers: centres with offset 1.0 lie exactly on them
SC_BIG = (257, 256, 256)  # 16842752 cells > 65536 x 256: the last x plane belongs to the second sweep


def _scat(name, comp, why, act=7, dirv=OBLIQUE, shape=SC_SHAPE, org=SC_ORG, L=SC_L, R=SC_R, nline=40, zero=None,
          clamps=False, sweeps=1):
    if zero is None:  # the line starts 2.5 cells before the box corner, as layout.zero_inc_coord_fp
        zero = tuple(L[a] - 2.5 * dirv[a] for a in range(3))
    return dict(name=name, comp=comp, why=why, act=act, dir=dirv, shape=shape, org=org, L=L, R=R, nline=nline,
                zero=zero, clamps=clamps, sweeps=sweeps, proj={"E": 0.8125, "H": -0.59375}[comp[0]] + 0.001,
                dts=("f32", "f64"))


SCAT_CASES = [_scat("oblique-" + c, c, "component offset %s, %s" % (MIN_COORD_FP[c], "H shift 0.5" if c[0] == "H"
                    else "no shift")) for c in COMPS] + [
    _scat("act3-Hz", "Hz", "only x and y bound the box (act = 3)", act=3),
    _scat("act1-Ex", "Ex", "only x bounds the box (act = 1)", act=1),
    _scat("plus-x-Hy", "Hy", "propagation along +x: d is a multiple of 0.5 in every cell", dirv=(1.0, 0.0, 0.0)),
    _scat("plus-y-Ey", "Ey", "propagation along +y", dirv=(0.0, 1.0, 0.0)),
    _scat("clamps-Ez", "Ez", "a line of 3 points from the middle of the box: d < 0 and i0 > nline - 2 both occur",
          nline=3, zero=(6.5, 5.5, 9.0), clamps=True),
    _scat("two-sweeps-Hx", "Hx", "min(65536, ceil(n / 256)) blocks of 256: 16842752 cells take two sweeps",
          shape=SC_BIG, org=(3, 2, 5), L=(100.0, 40.0, 30.0), R=(300.0, 200.0, 240.0), nline=700, sweeps=2),
]


def scat_geo(case):
    m = MIN_COORD_FP[case["comp"]]
    geo = list(m) + list(case["zero"]) + list(case["dir"]) + list(case["L"]) + list(case["R"]) + [
        case["proj"], 0.5 if case["comp"][0] == "H" else 0.0]
    return geo, list(case["org"]) + [case["act"]]


def scat_oracle(case, f, line):
    """io/dump.py incident_field / scattered_field_torch in fp64 on the CPU,
    from the dtype's own f and line values: (inside mask, incident value,
    d, f - inc)."""
    m, o, shp = MIN_COORD_FP[case["comp"]], case["org"], case["shape"]
    ax = [torch.arange(shp[a], dtype=torch.float64) + o[a] + m[a] for a in range(3)]
    X, Y, Z = ax[0].view(-1, 1, 1), ax[1].view(1, -1, 1), ax[2].view(1, 1, -1)
    zero, dirv = case["zero"], case["dir"]
    d = (X - zero[0]) * dirv[0] + (Y - zero[1]) * dirv[1] + (Z - zero[2]) * dirv[2]
    if case["comp"][0] == "H":
        d = d - 0.5
    i0 = torch.clamp(torch.floor(d).long(), 0, line.numel() - 2)
    w1 = d - i0
    lv = line.to(torch.float64)
    inc = ((1 - w1) * lv[i0] + w1 * lv[i0 + 1]) * case["proj"]
    mask = torch.ones(shp, dtype=torch.bool)
    border = {}
    for a in range(3):
        if case["act"] >> a & 1:
            view = [1, 1, 1]
            view[a] = -1
            mask = mask & ((ax[a] > case["L"][a]) & (ax[a] < case["R"][a])).view(view)
            border[a] = (bool((ax[a] == case["L"][a]).any()), bool((ax[a] == case["R"][a]).any()))
    return dict(mask=mask, inc=inc, d=d, want=f.double() - inc, border=border)


def scat_inputs(case, dt, device):
    n = math.prod(case["shape"])
    g = torch.Generator().manual_seed(61)
    f = (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1).to(DT[dt])
    return f.view(case["shape"]).to(device), live((case["nline"],), 62, dt, device)


def scat_claims(case, o):
    """Inside and outside cells both occur; a cell centre lies exactly on L
    and one exactly on R along some active axis; both clamps are hit where
    claimed (and only there); the sweeps of the launch grid."""
    mask, d = o["mask"], o["d"].expand(case["shape"])
    assert bool(mask.any()) and not bool(mask.all()), case["why"]
    on = [a for a, (l, r) in o["border"].items() if l and r]
    assert on, case["why"]
    for a in on:  # the strict inequalities put those cells outside
        m = MIN_COORD_FP[case["comp"]][a]
        for v in (case["L"][a], case["R"][a]):
            i = int(v - m) - case["org"][a]
            assert not bool(mask.select(a, i).any())
    inside_d = d[mask]
    low, high = bool((inside_d < 0).any()), bool((torch.floor(inside_d) > case["nline"] - 2).any())
    assert (low, high) == (case["clamps"], case["clamps"]), (case["why"], low, high)
    n = math.prod(case["shape"])
    assert cdiv(n, min(65536, cdiv(n, 256)) * 256) == case["sweeps"], case["why"]
    if case["sweeps"] > 1:  # inside and outside cells past the first sweep too
        tail = mask.reshape(-1)[65536 * 256:]
        assert bool(tail.any()) and not bool(tail.all())


def run_scattered(ops, case, dt, device):
    """ops None: the oracle rounded to the dtype stands in for the kernel
    (tests/test_aux_cpu.py)."""
    f, line = scat_inputs(case, dt, device)
    f0, line0 = f.clone(), line.clone()
    geo, igeo = scat_geo(case)
    if ops is None:
        o = scat_oracle(case, f, line)
        got = torch.where(o["mask"], o["want"].to(DT[dt]), f)
    else:
        got = ops.scattered(f, line, geo, igeo)
    return dict(case=case, dt=dt, f=f, f0=f0, line=line, line0=line0, got=got)


def check_scattered(r):
    case, dt = r["case"], r["dt"]
    f, got = r["f0"].cpu(), r["got"].cpu()
    o = scat_oracle(case, f, r["line0"].cpu())
    scat_claims(case, o)
    mask = o["mask"]
    assert same(got[~mask], f[~mask]), "an outside cell differs from f"
    # per cell: the product rounded to T and the difference, 2^-24 relative each (fp32); fp64: the bound of
    # test_scattered_gpu.py
    rel = 2.0 ** -23 if dt == "f32" else 1e-14
    err = (got.double() - o["want"]).abs()
    bound = rel * (f.double().abs() + o["inc"].abs())
    bad = mask & ~(err <= bound)
    assert not bool(bad.any()), (case["why"], int(bad.sum()), float((err / bound)[mask].max()))
    assert bool((got[mask] != f[mask]).any()), "nothing was subtracted inside"
    assert same(r["f"], r["f0"]) and same(r["line"], r["line0"]), "scattered changed an input"


_SC = _ids(SCAT_CASES)


@pytest.mark.parametrize("case,dt", _SC[0], ids=_SC[1])
def test_scattered(gpu, case, dt):
    ops = make_ops("hip", None, gpu, DT[dt])
    r = run_scattered(ops, case, dt, gpu)
    torch.cuda.synchronize()
    check_scattered(r)
