"""Compile the reference program (serial, CPU, fp64, complex values) into ``oracle/_ref/``.

The reference tree is read where it lies and nothing of it is copied: its
serial sources are handed to the compiler directly, together with the
project's own driver (``ref_driver.cpp``) and bitmap stand-in (``EasyBMP.h``).
Its CMake files are not used (they do not configure without the third-party
bitmap library).  Two binaries are made from one recipe:

* ``oracle/_ref/ref3d`` -- ``-DGRID_3D``, drives ``Scheme3D``
* ``oracle/_ref/ref2d`` -- ``-DGRID_2D``, drives ``SchemeTMz``

Where the reference tree is absent this is a no-op with a message: the
recorded fixtures under ``tests/golden/ref/`` are all the tests read.

    python oracle/build_ref.py [--reference DIR] [--force]
"""

from __future__ import annotations

import argparse
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")

# where the reference tree is looked for, in order (the first that holds Source/Scheme wins)
REFERENCE_DIRS = (os.environ.get("FDTD3D_REFERENCE", ""), os.path.join(HERE, os.pardir, os.pardir, "reference"))

INCLUDE_DIRS = ("Helpers", "Physics", "Kernels", "Coordinate", "Grid", "Layout", "File-Management",
                "File-Management/Loader", "File-Management/Dumper", "Scheme", "Settings")
# parts of the reference left out: its own main, the CUDA backend and everything MPI
SKIP_DIRS = ("Cuda",)
SKIP_PREFIXES = ("ParallelGrid", "ParallelBuffer", "ParallelYeeGridLayout")
SKIP_FILES = ("main.cpp",)

DEFINES = ('-DDOUBLE_VALUES=', '-DCOMPLEX_FIELD_VALUES=', '-DTWO_TIME_STEPS=', '-DCXX11_ENABLED=', '-DPRINT_MESSAGE=1')
# -ffp-contract=off: no fused multiply-add, so the recorded values do not depend on the build host's ISA
FLAGS = ("-O2", "-std=c++11", "-w", "-ffp-contract=off", "-include", "string")
BUILDS = {"ref3d": "-DGRID_3D=", "ref2d": "-DGRID_2D="}


def find_reference(explicit: Optional[str] = None) -> Optional[str]:
    for d in ((explicit,) if explicit else REFERENCE_DIRS):
        if d and os.path.isdir(os.path.join(d, "Source", "Scheme")):
            return os.path.abspath(d)
    return None


def reference_sources(ref: str) -> List[str]:
    out = []
    src = os.path.join(ref, "Source")
    for root, dirs, files in os.walk(src):
        dirs[:] = sorted(d for d in dirs if d not in SKIP_DIRS)
        for f in sorted(files):
            if f.endswith(".cpp") and f not in SKIP_FILES and not f.startswith(SKIP_PREFIXES):
                out.append(os.path.join(root, f))
    return out


def reference_inputs(ref: str) -> List[str]:
    """Every file of the reference a build may read (sources, headers, .inc lists)."""
    out = []
    for root, dirs, files in os.walk(os.path.join(ref, "Source")):
        dirs[:] = sorted(d for d in dirs if d not in SKIP_DIRS)
        out += [os.path.join(root, f) for f in sorted(files) if f.endswith((".cpp", ".h", ".inc"))]
    return out


def _compile(cxx: str, args: List[str]) -> None:
    r = subprocess.run([cxx] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("oracle build failed: %s %s\n%s" % (cxx, " ".join(args), r.stdout[-4000:]))


def build_ref(reference: Optional[str] = None, force: bool = False, jobs: int = 8) -> bool:
    """Build both binaries; returns False (after a message) where there is no reference tree or compiler."""
    ref = find_reference(reference)
    if ref is None:
        print("oracle: no reference tree here; nothing built (tests read the fixtures under tests/golden/ref/ only)")
        return False
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        print("oracle: no C++ compiler found; nothing built")
        return False
    sources = reference_sources(ref)
    driver = os.path.join(HERE, "ref_driver.cpp")
    includes = ["-I" + HERE] + ["-I" + os.path.join(ref, "Source", d) for d in INCLUDE_DIRS]
    for name, grid_define in BUILDS.items():
        exe = os.path.join(OUT, name)
        inputs = [driver, os.path.join(HERE, "EasyBMP.h"), __file__] + reference_inputs(ref)
        if os.path.exists(exe) and not force and os.path.getmtime(exe) >= max(os.path.getmtime(p) for p in inputs):
            print("oracle: %s is up to date" % exe)
            continue
        # every build starts from an empty object directory: nothing of a failed or older one is linked
        objdir = os.path.join(OUT, "obj_" + name)
        shutil.rmtree(objdir, ignore_errors=True)
        os.makedirs(objdir)
        if os.path.exists(exe):
            os.remove(exe)
        common = list(FLAGS) + list(DEFINES) + [grid_define] + includes
        objs = [os.path.join(objdir, "%02d_%s.o" % (i, os.path.basename(s)[:-4])) for i, s in enumerate(sources + [driver])]
        with ThreadPoolExecutor(max_workers=jobs) as pool:
            list(pool.map(lambda so: _compile(cxx, common + ["-c", so[0], "-o", so[1]]), zip(sources + [driver], objs)))
        _compile(cxx, objs + ["-o", exe])
        print("oracle: built %s from %d reference sources" % (exe, len(sources)))
    return True


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=None, help="the reference tree (default: looked for next to the repository)")
    ap.add_argument("--force", action="store_true", help="rebuild even if the binaries are newer than the recipe")
    a = ap.parse_args(argv)
    build_ref(a.reference, a.force)
    return 0


if __name__ == "__main__":
    sys.exit(main())
