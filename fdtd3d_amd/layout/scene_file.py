"""Scene files: user-defined boxes, spheres and cylinders (``--scene file``).

A scene is a list of objects painted over vacuum, first to last (painter's
order).  JSON, standard library only::

    {"smoothing": "linear",
     "objects": [
      {"shape": "box",      "lo": [0, 0, 0], "hi": [64, 64, 20], "eps": 2.25},
      {"shape": "sphere",   "center": [32.5, 32.5, 30.5], "radius": 8, "eps": 1.0, "omega_p": 1.4142135},
      {"shape": "cylinder", "axis": "z", "center": [20.5, 40.5], "radius": 3, "span": [20, 50], "eps": 4.0}
     ]}

Coordinates are in cells on the eps layout (cell centre ``m + 0.5``, the
convention of ``--sphere-center-*``).  ``eps`` is the relative permittivity
(default 1), ``omega_p`` the electric Drude plasma frequency in units of
``2 pi f_source`` (default 0, used with ``--use-metamaterials`` only).  A
cylinder's ``center`` holds its two in-plane coordinates, in x, y, z order of
the two axes other than ``axis``; ``span`` is its extent along ``axis``.

Signed distances ``d`` (fp64, eps-grid units): sphere ``|p - c| - r``; box the
largest of ``lo_a - p_a``, ``p_a - hi_a`` over the axes -- exact on faces, a
Chebyshev distance at edges and corners (the smoothed zone there is square,
not rounded); cylinder the larger of the radial and the axial distance.

This module also defines the fixed-size table entry both backends'
``scene_sample`` op reads (csrc/scene_kernels.hip ``SceneEnt``).
"""

from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

SCENE_MAX_OBJECTS = 256  # entries of the kernel's table (fdtd_scene_max_objects)
SCENE_ENT = np.dtype([("kind", "<i4"), ("flags", "<i4"), ("p", "<f8", (3,)), ("q", "<f8", (3,)),
                      ("eps", "<f8"), ("omega", "<f8")])
SCENE_ENT_SIZE = 72      # bytes of a table entry (fdtd_scene_ent_size)
assert SCENE_ENT.itemsize == SCENE_ENT_SIZE

KIND_BOX, KIND_SPHERE, KIND_CYLINDER = 0, 1, 2
# SceneEnt.flags: bits 0-1 the cylinder's axis, bits 2-4 the axes the object
# ignores (the inactive axis of a 2D scheme), bit 5 sharp eps (smoothing none)
FLAG_IGNORE_SHIFT = 2
FLAG_SHARP = 32

SHAPES = ("box", "sphere", "cylinder")
SMOOTHINGS = ("linear", "none")
_KEYS = {"box": {"shape", "lo", "hi", "eps", "omega_p"},
         "sphere": {"shape", "center", "radius", "eps", "omega_p"},
         "cylinder": {"shape", "axis", "center", "radius", "span", "eps", "omega_p"}}
_AXES = {"x": 0, "y": 1, "z": 2}


@dataclass(frozen=True)
class SceneObject:
    """One validated object.  Box: ``a`` = lo, ``b`` = hi.  Sphere: ``a`` =
    centre, ``radius``.  Cylinder: ``axis``, ``a`` = centre with the span's
    lower end at ``axis``, ``b[axis]`` = the span's upper end, ``radius``."""
    shape: str
    a: Tuple[float, float, float]
    b: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    radius: float = 0.0
    axis: int = 0
    eps: float = 1.0
    omega_p: float = 0.0


def _number(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError("scene: %s must be a number, got %r" % (what, v))
    v = float(v)
    if not math.isfinite(v):
        raise ValueError("scene: %s must be finite, got %r" % (what, v))
    return v


def _vector(v, n: int, what: str) -> Tuple[float, ...]:
    if not isinstance(v, (list, tuple)) or len(v) != n:
        raise ValueError("scene: %s must be a list of %d numbers, got %r" % (what, n, v))
    return tuple(_number(x, what) for x in v)


def parse_object(o, index: int = 0) -> SceneObject:
    """A :class:`SceneObject` from its JSON dictionary; ValueError with a
    message for everything the format refuses."""
    if isinstance(o, SceneObject):
        return o
    if not isinstance(o, dict):
        raise ValueError("scene: object %d must be a dictionary, got %r" % (index, o))
    shape = o.get("shape")
    if shape not in SHAPES:
        raise ValueError("scene: object %d has unknown shape %r (box, sphere or cylinder)" % (index, shape))
    unknown = sorted(set(o) - _KEYS[shape])
    if unknown:
        raise ValueError("scene: object %d (%s) has unknown key %r" % (index, shape, unknown[0]))
    what = "object %d (%s) " % (index, shape)
    for k in sorted(_KEYS[shape] - {"eps", "omega_p"} - set(o)):
        raise ValueError("scene: %sneeds %r" % (what, k))
    eps = _number(o.get("eps", 1.0), what + "eps")
    omega_p = _number(o.get("omega_p", 0.0), what + "omega_p")
    if eps <= 0:
        raise ValueError("scene: %seps must be positive, got %r" % (what, eps))
    if omega_p < 0:
        raise ValueError("scene: %somega_p must not be negative, got %r" % (what, omega_p))
    if shape == "box":
        lo, hi = _vector(o["lo"], 3, what + "lo"), _vector(o["hi"], 3, what + "hi")
        if any(l >= h for l, h in zip(lo, hi)):
            raise ValueError("scene: %sneeds lo < hi on every axis, got %r, %r" % (what, lo, hi))
        return SceneObject("box", lo, hi, eps=eps, omega_p=omega_p)
    radius = _number(o["radius"], what + "radius")
    if radius <= 0:
        raise ValueError("scene: %sradius must be positive, got %r" % (what, radius))
    if shape == "sphere":
        return SceneObject("sphere", _vector(o["center"], 3, what + "center"), radius=radius, eps=eps,
                           omega_p=omega_p)
    if o["axis"] not in _AXES:
        raise ValueError("scene: %saxis must be x, y or z, got %r" % (what, o["axis"]))
    axis = _AXES[o["axis"]]
    c2, span = _vector(o["center"], 2, what + "center"), _vector(o["span"], 2, what + "span")
    if span[0] >= span[1]:
        raise ValueError("scene: %sneeds span lo < hi, got %r" % (what, span))
    a, b, others = [0.0] * 3, [0.0] * 3, [d for d in range(3) if d != axis]
    a[others[0]], a[others[1]], a[axis], b[axis] = c2[0], c2[1], span[0], span[1]
    return SceneObject("cylinder", tuple(a), tuple(b), radius=radius, axis=axis, eps=eps, omega_p=omega_p)


def parse_objects(objects: Sequence, smoothing: str = "linear") -> Tuple[SceneObject, ...]:
    if smoothing not in SMOOTHINGS:
        raise ValueError("scene: smoothing must be linear or none, got %r" % (smoothing,))
    if not isinstance(objects, (list, tuple)):
        raise ValueError("scene: objects must be a list, got %r" % (objects,))
    if len(objects) > SCENE_MAX_OBJECTS:
        raise ValueError("scene: %d objects, the table holds %d" % (len(objects), SCENE_MAX_OBJECTS))
    return tuple(parse_object(o, n) for n, o in enumerate(objects))


def check_scheme(objects: Sequence[SceneObject], scheme: str) -> None:
    """What a scheme refuses: every file scene in 1D, a cylinder that does
    not lie along the inactive axis in 2D."""
    if scheme == "1d":
        raise ValueError("scene: file scenes need a 2D or 3D scheme")
    if scheme in ("tmz", "tez"):
        for n, o in enumerate(objects):
            if o.shape == "cylinder" and o.axis != 2:
                raise ValueError("scene: object %d: a cylinder of a 2D scheme must lie along z, the inactive axis" % n)


def parse_scene(doc) -> Tuple[Tuple[SceneObject, ...], str]:
    """(objects, smoothing) of a parsed scene document."""
    if not isinstance(doc, dict):
        raise ValueError("scene: the file must hold one JSON object")
    unknown = sorted(set(doc) - {"smoothing", "objects"})
    if unknown:
        raise ValueError("scene: unknown key %r" % unknown[0])
    if "objects" not in doc:
        raise ValueError("scene: needs 'objects'")
    smoothing = doc.get("smoothing", "linear")
    return parse_objects(doc["objects"], smoothing), smoothing


def load_scene_file(path: str) -> Tuple[Tuple[SceneObject, ...], str]:
    """(objects, smoothing) of the scene file ``path``; SettingsError for a
    file that cannot be read or that the format refuses."""
    from ..utils.settings import SettingsError

    def refuse_constant(name):  # NaN / Infinity, which json accepts by default
        raise ValueError("scene: non-finite number %s" % name)

    try:
        with open(path, "r", encoding="utf-8") as f:
            doc = json.load(f, parse_constant=refuse_constant)
        return parse_scene(doc)
    except OSError as e:
        raise SettingsError("--scene-file %s: %s" % (path, e.strerror or e))
    except ValueError as e:  # JSONDecodeError included
        raise SettingsError("--scene-file %s: %s" % (path, e))


class SceneTable:
    """The objects as the table of ``ops.scene_sample``: ``ents`` = numpy
    records of :data:`SCENE_ENT`, coordinates in cells (the op scales them by
    its ``mod``), ``omega`` = omega_p * 2 pi f in rad/s.  ``device_tables``
    caches the HIP backend's copies, one per device."""

    def __init__(self, ents: np.ndarray):
        if ents.dtype != SCENE_ENT or ents.ndim != 1:
            raise ValueError("SceneTable: a 1D array of SCENE_ENT records")
        if len(ents) > SCENE_MAX_OBJECTS:
            raise ValueError("scene: %d objects, the table holds %d" % (len(ents), SCENE_MAX_OBJECTS))
        self.ents = ents
        self.device_tables = {}

    def __len__(self) -> int:
        return len(self.ents)


def build_table(objects: Sequence[SceneObject], scheme: str = "3d", smoothing: str = "linear",
                source_frequency: float = 1.0) -> SceneTable:
    objects = parse_objects(list(objects), smoothing)
    check_scheme(objects, scheme)
    ents = np.zeros(len(objects), dtype=SCENE_ENT)
    ignore = 0 if scheme == "3d" else 4  # 2D: objects ignore z
    for e, o in zip(ents, objects):
        e["kind"] = SHAPES.index(o.shape)
        e["flags"] = o.axis | (ignore << FLAG_IGNORE_SHIFT) | (FLAG_SHARP if smoothing == "none" else 0)
        e["p"] = o.a
        e["q"] = o.b if o.shape == "box" else (o.radius, o.b[o.axis], 0.0)
        e["eps"] = o.eps
        e["omega"] = o.omega_p * 2 * math.pi * source_frequency
    return SceneTable(ents)


def sample_args(quantity: str, points, origin, shape, stride, mod):
    """The arguments of ``scene_sample`` checked and normalised (both
    backends): (quantity index, points, origin, shape, stride, mod)."""
    if quantity not in ("eps", "omega"):
        raise ValueError("scene_sample: quantity eps or omega, got %r" % (quantity,))
    pts = [tuple(int(v) for v in p) for p in points]
    if len(pts) not in (1, 2, 4, 8) or any(len(p) != 3 for p in pts):
        raise ValueError("scene_sample: 1, 2, 4 or 8 points of 3 offsets, got %d" % len(pts))
    origin, shape, stride = (tuple(int(v) for v in t) for t in (origin, shape, stride))
    if len(origin) != 3 or len(shape) != 3 or len(stride) != 3:
        raise ValueError("scene_sample: origin, shape and stride have 3 entries")
    if any(s < 0 for s in shape):
        raise ValueError("scene_sample: negative shape %s" % (shape,))
    if any(s not in (1, 2) for s in stride):
        raise ValueError("scene_sample: stride 1 or 2 per axis, got %s" % (stride,))
    if float(mod) not in (1.0, 2.0):
        raise ValueError("scene_sample: mod 1 or 2, got %r" % (mod,))
    reach = max(abs(v) for t in (origin, shape) for v in t) * 2 + max(abs(v) for p in pts for v in p)
    if reach >= 2 ** 30:
        raise ValueError("scene_sample: region beyond 2^30 eps-grid points")
    return ("eps", "omega").index(quantity), pts, origin, shape, stride, float(mod)
