"""Shared by test_reference_cpu.py and test_reference_gpu.py (not collected).

Loads the recorded runs of the reference program under ``tests/golden/ref/``
(written by ``oracle/record.py``), turns a fixture's own argument list into a
``SchemeConfig`` through the project's settings parser, runs it and compares.
Nothing here reads the reference tree or the oracle binaries.
"""

import io
import json
import os

import numpy as np
import torch

from fdtd3d_amd.models.scheme import SchemeConfig, YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.utils.settings import EXIT_OK, setup_from_cmd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref")

# The project's claim about the reference, case by case: "agrees", or the number of the reference bug
#  the departure is put down to.
CLAIMS = {
    "3d_plain": "agrees",
    "3d_pml": "agrees",
    "3d_tfsf": "agrees",
    "3d_tfsf_oblique": "agrees",
    "3d_drude": 7,
    "2d_tfsf": "agrees",
    "2d_tfsf_phi45": "agrees",
}
CASES = tuple(CLAIMS)
# material grids only: the layers of unequal thickness, reference bug #25
MATERIAL_CLAIMS = {"3d_pml_uneven": 25}

_cache = {}


def load(name):
    """The fixture ``name``: its json plus ``arrays`` (name -> ndarray, read-only, loaded once)."""
    if name not in _cache:
        with open(os.path.join(GOLDEN, name + ".json"), "r", encoding="utf-8") as f:
            fx = json.load(f)
        fx["name"] = name
        spec = fx.pop("arrays")
        for k, s in spec.items():
            a = np.load(os.path.join(GOLDEN, "%s_%s.npy" % (name, k)))
            assert str(a.dtype) == s["dtype"] and list(a.shape) == s["shape"], (name, k)
            a.setflags(write=False)
            fx.setdefault("arrays", {})[k] = a
        _cache[name] = fx
    return _cache[name]


def project_args(fx, dtype="f64", extra=()):
    """The fixture's argument list plus what the reference fixes at build time: its scene, complex values, the
    value type."""
    return list(fx["args"]) + ["--scene", "reference", "--complex-field-values", "--dtype", dtype] + list(extra)


def config(fx, dtype="f64", extra=(), **over):
    out = io.StringIO()
    status, s = setup_from_cmd(project_args(fx, dtype, extra), out=out)
    assert status == EXIT_OK, out.getvalue()
    cfg = SchemeConfig.from_settings(s)
    for k, v in over.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return cfg


def window(fx, a):
    """The part of a whole-grid array the fixture holds (trailing unit axes of a 2D run dropped)."""
    a = a.reshape(fx["shape"])
    if fx["window"] is None:
        return a
    lo, hi = fx["window"]
    return a[tuple(slice(p, q) for p, q in zip(lo, hi))]


def run(cfg, backend="torch", device="cpu"):
    """Step ``cfg`` to its end; returns the scheme."""
    dt = {"f32": torch.float32, "f64": torch.float64}[cfg.dtype]
    s = YeeScheme(cfg, make_ops(backend, None, device, dt))
    s.init_scheme()
    s.init_grids()
    s.perform_steps()
    return s


def fields(fx, s):
    """name -> complex128 ndarray over the fixture's window."""
    out = {}
    for c in fx["fields"]:
        re = s.F[0][c].detach().double().cpu().numpy()
        im = s.F[1][c].detach().double().cpu().numpy()
        out[c] = window(fx, re + 1j * im)
    return out


RESIDUE = 1e-9   # a component whose peak is below this share of its kind's peak holds rounding residue only


def rel_errors(fx, ours):
    """Per component ``max|ours - ref| / max|ref|``.  A component the run does not excite holds the reference's
    own rounding residue (1e-19 beside 1e-4): where its peak is below ``RESIDUE`` of the peak of its kind (E or
    H) over the fixture, the error is taken relative to the kind's peak instead of to that residue."""
    ref = fx["arrays"]
    kind = {k: max(float(np.abs(ref[c]).max()) for c in fx["fields"] if c[0] == k) for k in "EH"}
    out = {}
    for c in fx["fields"]:
        peak = float(np.abs(ref[c]).max())
        scale = peak if peak >= RESIDUE * kind[c[0]] else kind[c[0]]
        out[c] = float(np.abs(ours[c] - ref[c]).max()) / scale
    return out


# ------------------------------------------------------------------ the reference's Drude average (bug #7)
def _c(x, like):
    return x.to(like.dtype)


def _eq3_is0(a, b, c):
    """C++ ``a == b == c == 0``: each comparison's 0 / 1 result is compared with the next operand."""
    return _c(_c(a == b, a) == c, a) == 0


def _eq2_is0(a, b):
    return _c(a == b, a) == 0


def _eq3(a, b, c):
    return _c(a == b, a) == c


def reference_drude_average(omegas, gammas):
    """What the reference computes for (omega_p, gamma) of a component from its 2 or 4 material points
    (SURVEY.md appendix A #7, #23), written from its behaviour: two points: the sum over single-precision
    sqrt(2) when one point is vacuum, else over 2; four points: the chained comparisons as C++ evaluates them,
    which select the divider 2 for every combination of 0 and one omega_p -- 2 omega_p inside the medium.
    Stands in for ``layout.approximation.approximate_drude`` (root mean square) in the tests that hold the
    Drude fixture's fields."""
    one = torch.ones_like(omegas[0])
    if len(omegas) == 2:
        (w1, w2), (g1, g2) = omegas, gammas
        vac = ((w1 == 0) & (g1 == 0)) | ((w2 == 0) & (g2 == 0))
        dw = torch.where(vac, float(np.sqrt(np.float32(2.0))) * one, 2.0 * one)
        dg = torch.where(vac, one, 2.0 * one)
        return (w1 + w2) / dw, (g1 + g2) / dg
    assert len(omegas) == 4
    w1, w2, w3, w4 = omegas
    g1, g2, g3, g4 = gammas
    b1 = ((_eq3_is0(w2, w3, w4) & _eq3_is0(g2, g3, g4)) | (_eq3_is0(w1, w3, w4) & _eq3_is0(g1, g3, g4))
          | (_eq3_is0(w1, w2, w4) & _eq3_is0(g1, g2, g4)) | (_eq3_is0(w1, w2, w3) & _eq3_is0(g1, g2, g3)))
    b2 = ((_eq2_is0(w1, w2) & (w3 == w4) & _eq2_is0(g1, g2) & (g3 == g4))
          | (_eq2_is0(w2, w4) & (w1 == w3) & _eq2_is0(g2, g4) & (g1 == g3))
          | (_eq2_is0(w3, w4) & (w1 == w2) & _eq2_is0(g3, g4) & (g1 == g2))
          | (_eq2_is0(w1, w3) & (w2 == w4) & _eq2_is0(g1, g3) & (g2 == g4)))
    b3 = (((w1 == 0) & _eq3(w2, w3, w4) & (g1 == 0) & _eq3(g2, g3, g4))
          | ((w2 == 0) & _eq3(w1, w3, w4) & (g2 == 0) & _eq3(g1, g3, g4))
          | ((w3 == 0) & _eq3(w1, w2, w4) & (g3 == 0) & _eq3(g1, g2, g4))
          | ((w4 == 0) & _eq3(w1, w2, w3) & (g4 == 0) & _eq3(g1, g2, g3)))
    dw = torch.where(b1, 2.0 * one, torch.where(b2, float(np.sqrt(2.0)) * one,
                                                torch.where(b3, float(2 / np.sqrt(3.0)) * one, 4.0 * one)))
    dg = torch.where(b1, one, torch.where(b2, 2.0 * one, torch.where(b3, 3.0 * one, one)))
    return (w1 + w2 + w3 + w4) / dw, (g1 + g2 + g3 + g4) / dg
