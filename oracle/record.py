"""Record runs of the reference program as fixtures under ``tests/golden/ref/``.

Run by hand after ``python oracle/build_ref.py``; not a test.  Each case is
one argument list given to the oracle binaries unchanged.  Per case it writes

* ``<case>.json`` -- the argument list, dimension, steps, grid shape, dx,
  wavelength, the scalars the oracle driver printed (dt, Courant number,
  relative phase velocity of the incident line) and the names of the arrays;
* ``<case>_<grid>.npy`` -- one array per grid, fp64 (complex128 where the
  imaginary part is not identically zero; that is asserted, not assumed).

The reference is built with complex values (its 3D scheme needs them): the
source is ``sin + i cos``, so field arrays carry two independent solutions.

Large grids (the material case: the reference's Drude sphere sits at fixed cells
around (57, 57, 23), no small grid reaches it) are stored
as a window, named in the json; the run itself covers the whole grid.  The
incident line is 100 (Nx + Ny + Nz) cells long and zero beyond the wave
front: its leading ``LINE_KEEP`` cells are stored and the rest asserted zero.
The sigma grids depend on one axis only (asserted) and are stored as lines.
"""

from __future__ import annotations

import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, "_ref")
OUT = os.path.join(HERE, os.pardir, "tests", "golden", "ref")

LINE_KEEP = 96
MAX_FILE = 100 * 1024
MAX_DIR = 2 * 1024 * 1024

S3 = ["--3d", "--sizex", "14", "--sizey", "12", "--sizez", "18"]
PML3 = ["--use-pml", "--pml-sizex", "3", "--same-size-pml"]
# 5 cells: the native driver wants the box more than one cell clear of the layers
TFSF3 = ["--use-tfsf", "--tfsf-sizex", "5", "--same-size-tfsf"]

# name -> (argument list, window or None, material grids kept)
CASES = {
    # plain update ranges, PEC faces, source cell and waveform (24 steps: the wave has crossed every face)
    "3d_plain": (S3 + ["--time-steps", "24"], None, ()),
    # UPML D/B form and sigma grading
    "3d_pml": (S3 + PML3 + ["--time-steps", "24"], None, ("SigmaX", "SigmaY", "SigmaZ")),
    # incident line, face corrections, phase velocity (default angles: teta 90, phi 0, psi 90)
    "3d_tfsf": (S3 + PML3 + TFSF3 + ["--time-steps", "30"], None, ()),
    # one oblique angle set
    "3d_tfsf_oblique": (S3 + PML3 + TFSF3 + ["--angle-teta", "60", "--angle-phi", "30", "--angle-psi", "45",
                                               "--time-steps", "30"], None, ()),
    # Drude ADE and material averaging.  The reference asserts eps == 1 wherever it averages Drude media, so
    # --use-metamaterials runs only on grids that stay clear of its eps sphere (z < 20).  This grid holds the
    # lower cap of the Drude sphere and of the magnetic Drude box, z in [15, 19), above the source cell
    # (57, 57, 9); with 2-cell layers two cell layers of the cap lie outside them.  The window holds the source,
    # the cap's surface and vacuum around it.
    "3d_drude": (["--3d", "--sizex", "114", "--sizey", "114", "--sizez", "19", "--use-pml", "--pml-sizex", "2",
                  "--same-size-pml", "--use-metamaterials", "--time-steps", "30"],
                 ((50, 51, 5), (64, 63, 19)), ("Eps", "OmegaPE", "OmegaPM")),
    # layers of unequal thickness: the reference grades all three axes with the x thickness (sigma lines only)
    "3d_pml_uneven": (S3 + ["--use-pml", "--pml-sizex", "4", "--pml-sizey", "3", "--pml-sizez", "2",
                            "--time-steps", "1"], None, ("SigmaX", "SigmaY", "SigmaZ")),
    # TMz.  Every step the reference's TMz scheme reads Ez around (462 - 430 cos phi, 455 - 430 sin phi) and the
    # incident line there: a run needs y >= 457 at phi = 0 and x >= 464 at phi = 90 degrees, and it aborts without
    # TF/SF (the line is not allocated).  So there is no 2D point-source fixture, with or without layers, and
    # the 2D fixtures are windows: the lower-x and lower-y faces of the total-field box, their corner and the
    # layers there.  The scheme accepts phi = 0 and phi = 45 degrees only.
    "2d_tfsf": (["--2d", "--sizex", "35", "--sizey", "459"] + PML3 + TFSF3 + ["--time-steps", "30"],
                ((0, 0), (35, 26)), ("SigmaX", "SigmaY")),
    "2d_tfsf_phi45": (["--2d", "--sizex", "162", "--sizey", "157", "--angle-phi", "45"] + PML3 + TFSF3
                      + ["--time-steps", "30"], ((0, 0), (29, 27)), ()),
}

MATERIALS_ONLY = ("3d_pml_uneven",)   # cases of which only the material grids are kept
FIELDS = {3: ("Ex", "Ey", "Ez", "Hx", "Hy", "Hz"), 2: ("Ez", "Hx", "Hy")}


def _read(tmp, steps, name, shape):
    raw = np.fromfile(os.path.join(tmp, "current[%d]_rank-0_%s.dat" % (steps, name)), dtype=np.complex128)
    assert raw.size == int(np.prod(shape)), (name, raw.size, shape)
    return raw.reshape(shape)   # the reference's linear index runs z (last axis) fastest


def _narrow(a, want_real):
    """fp64 real part where the imaginary part is identically zero, else complex128."""
    if not np.any(a.imag != 0.0):
        return np.ascontiguousarray(a.real)
    assert not want_real, "imaginary part expected to be identically zero"
    return np.ascontiguousarray(a)


def record(name, args, window, materials, out_dir):
    dim = 2 if "--2d" in args else 3
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([os.path.join(REF, "ref%dd" % dim)] + list(args), cwd=tmp, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        info, sizes = {}, {}
        for line in r.stdout.splitlines():
            m = re.match(r"oracle: size (\w+) ([\d ]+)$", line)
            if m:
                sizes[m.group(1)] = tuple(int(v) for v in m.group(2).split())
                continue
            m = re.match(r"oracle: (\w+) (\S+)$", line)
            if m:
                info[m.group(1)] = m.group(2)
        assert info["value_bytes"] == "16"
        steps = int(info["steps"])
        arrays = {}
        fields = () if name in MATERIALS_ONLY else FIELDS[dim]
        for f in fields:
            arrays[f] = _narrow(_read(tmp, steps, f, sizes[f]), False)
        for g in materials:
            a = _narrow(_read(tmp, steps, g, sizes[g]), True)
            if g.startswith("Sigma"):
                ax = "XYZ".index(g[-1])
                line = np.moveaxis(a, ax, 0).reshape(a.shape[ax], -1)
                assert np.all(line == line[:, :1]), "%s varies across its own axis' planes" % g
                a = np.ascontiguousarray(line[:, 0])
            arrays[g] = a
        if "--use-tfsf" in args:
            for g in ("EInc", "HInc"):
                a = _read(tmp, steps, g, sizes["EInc"])
                assert not np.any(a[LINE_KEEP:] != 0), "incident line is not zero beyond the cells kept"
                arrays[g] = _narrow(a[:LINE_KEEP], False)
    if window is not None:
        lo, hi = window
        for k in list(arrays):
            if arrays[k].ndim == dim:
                arrays[k] = np.ascontiguousarray(arrays[k][tuple(slice(a, b) for a, b in zip(lo, hi))])
    meta = {
        "args": list(args), "dimension": dim, "steps": steps, "shape": list(sizes[FIELDS[dim][0]]),
        "dx": float(info["dx"]), "wavelength": float(info["wavelength"]), "dt": float(info["dt"]),
        "courant": float(info["courant"]),
        "rel_phase_velocity": float(info["rel_phase_velocity"]) if "rel_phase_velocity" in info else None,
        "window": [list(window[0]), list(window[1])] if window is not None else None,
        "fields": list(fields), "materials": list(materials),
        "incident": ["EInc", "HInc"] if "--use-tfsf" in args else [],
        "arrays": {k: {"dtype": str(v.dtype), "shape": list(v.shape)} for k, v in arrays.items()},
    }
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, "%s_%s.npy" % (name, k)), v)
    with open(os.path.join(out_dir, name + ".json"), "w", encoding="utf-8") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    if not os.path.exists(os.path.join(REF, "ref3d")):
        print("oracle: no binaries under oracle/_ref/ (run oracle/build_ref.py where the reference tree is)")
        return 1
    os.makedirs(OUT, exist_ok=True)
    for name, (args, window, materials) in CASES.items():
        if argv and name not in argv:
            continue
        record(name, args, window, materials, OUT)
        print("recorded", name)
    total = 0
    for f in sorted(os.listdir(OUT)):
        n = os.path.getsize(os.path.join(OUT, f))
        assert n <= MAX_FILE, "%s: %d bytes" % (f, n)
        total += n
    assert total <= MAX_DIR, "tests/golden/ref: %d bytes" % total
    print("tests/golden/ref: %d bytes" % total)
    return 0


if __name__ == "__main__":
    sys.exit(main())
