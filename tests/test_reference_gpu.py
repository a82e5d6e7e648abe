"""The HIP backend against recorded runs of the reference program (``tests/golden/ref/``; see
test_reference_cpu.py for the cases, the claim about each and where the fp64 bound comes from).

Paths: the stepped kernels (``hybrid_block=1``, fused off), the default path (whatever the planner picks; which
one ran is asserted) and the native ``fdtd3d`` driver with the fixture's own argument list.  fp64 holds the CPU
file's bound; fp32 the project's fp32-against-fp64 bound for the same physics (test_hybrid_gpu.py: 10 x 2e-5 of
the peak of the component's kind).  The fixtures are a few thousand cells: no blocked or hybrid plan exists for
the fixtures with layers or TF/SF (a plan needs a core of a quarter of the grid, test_sources_gpu.py), so their
default path is the stepped one; the plain case takes the blocked (fp64) or fused (fp32) kernel.
"""

import subprocess

import numpy as np
import pytest

import ref_cases as rc
from test_reference_cpu import AGREEING, BOUND

pytestmark = pytest.mark.gpu

F32_BOUND = 10 * 2e-5   # test_hybrid_gpu.py: fp32 HIP against the fp64 oracle, of the kind's peak


# The plain case takes the blocked fp64 kernel, and in fp32, whose rows are float4 along z (18 cells here), the
# fused E+H kernel.  Every other fixture has layers or TF/SF on a grid of a few thousand cells: no hybrid plan.
DEFAULT_PATH = {("3d_plain", "f64"): "blocked", ("3d_plain", "f32"): "fused"}


def kind_errors(fx, ours):
    """Per component max|ours - ref| over the peak of its kind (the scale of the fp32 bound)."""
    ref = fx["arrays"]
    kind = {k: max(float(np.abs(ref[c]).max()) for c in fx["fields"] if c[0] == k) for k in "EH"}
    return {c: float(np.abs(ours[c] - ref[c]).max()) / kind[c[0]] for c in fx["fields"]}


def check(fx, ours, dtype):
    errs = rc.rel_errors(fx, ours) if dtype == "f64" else kind_errors(fx, ours)
    bound = BOUND if dtype == "f64" else F32_BOUND
    print(fx["name"], dtype, {c: "%.3g" % e for c, e in errs.items()})
    for c, e in errs.items():
        assert e <= bound, (fx["name"], dtype, c, e, bound)


def path_of(s):
    if s.hybrid is not None:
        return "hybrid"
    if s.tb > 1:
        return "blocked"
    return "fused" if s.fused else "stepped"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", AGREEING)
def test_stepped(gpu, name, dtype):
    fx = rc.load(name)
    s = rc.run(rc.config(fx, dtype, hybrid_block=1, time_block=1, use_fused=False), "hip", gpu)
    assert path_of(s) == "stepped"
    check(fx, rc.fields(fx, s), dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", AGREEING)
def test_default_path(gpu, name, dtype):
    fx = rc.load(name)
    s = rc.run(rc.config(fx, dtype), "hip", gpu)
    path = path_of(s)
    print(name, dtype, "path:", path)
    assert path == DEFAULT_PATH.get((name, dtype), "stepped"), path
    check(fx, rc.fields(fx, s), dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", AGREEING)
def test_native_driver(name, dtype, tmp_path):
    from fdtd3d_amd import native
    fx = rc.load(name)
    argv = rc.project_args(fx, dtype, ["--save-res", "--save-as-dat", "--output-dir", str(tmp_path)])
    r = subprocess.run([native.executable()] + argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ndt = np.complex64 if dtype == "f32" else np.complex128
    ours = {}
    for c in fx["fields"]:
        a = np.fromfile(tmp_path / ("current[%d]_rank-0_%s.dat" % (fx["steps"], c)), dtype=ndt)
        ours[c] = rc.window(fx, a.astype(np.complex128))
    check(fx, ours, dtype)


def test_drude_stepped_equals_torch(gpu):
    """3d_drude departs from the reference (bug #7), so the HIP run is held to the torch run of the same
    configuration, which test_reference_cpu.py ties to the fixture's material grids."""
    fx = rc.load("3d_drude")
    cfg = rc.config(fx, "f64", hybrid_block=1)
    a = rc.fields(fx, rc.run(cfg, "hip", gpu))
    b = rc.fields(fx, rc.run(cfg, "torch", "cpu"))
    for c in a:
        kind = max(float(np.abs(b[o]).max()) for o in b if o[0] == c[0])
        assert float(np.abs(a[c] - b[c]).max()) <= BOUND * kind, c


def test_drude_reference_average(gpu, monkeypatch):
    """The HIP Drude chain against the fixture itself, with the reference's material average in place of the
    project's (test_reference_cpu.py test_drude_agrees_with_reference_average), fp64 at the CPU bound."""
    import fdtd3d_amd.layout.materials as materials
    monkeypatch.setattr(materials, "approximate_drude", rc.reference_drude_average)
    fx = rc.load("3d_drude")
    s = rc.run(rc.config(fx, "f64", hybrid_block=1), "hip", gpu)
    assert path_of(s) == "stepped"
    check(fx, rc.fields(fx, s), "f64")
