"""Scene files: user-defined boxes, spheres, cylinders and closed triangle
meshes (``--scene file``).

A scene is a list of objects painted over vacuum, first to last (painter's
order).  JSON, standard library only::

    {"smoothing": "linear",
     "objects": [
      {"shape": "box",      "lo": [0, 0, 0], "hi": [64, 64, 20], "eps": 2.25},
      {"shape": "sphere",   "center": [32.5, 32.5, 30.5], "radius": 8, "eps": 1.0, "omega_p": 1.4142135},
      {"shape": "cylinder", "axis": "z", "center": [20.5, 40.5], "radius": 3, "span": [20, 50], "eps": 4.0},
      {"shape": "mesh",     "file": "target.stl", "scale": 0.25, "translate": [32.5, 32.5, 30.0], "eps": 2.56}
     ]}

Coordinates are in cells on the eps layout (cell centre ``m + 0.5``, the
convention of ``--sphere-center-*``).  ``eps`` is the relative permittivity
(default 1), ``omega_p`` the electric Drude plasma frequency in units of
``2 pi f_source`` (default 0, used with ``--use-metamaterials`` only).
``gamma`` is the collision frequency of that pole, ``omega_pm`` / ``gamma_m``
the plasma and collision frequencies of a magnetic Drude pole (the same units,
default 0, sharp like ``omega_p``); a damping needs its pole, so a point is
dispersive exactly where its plasma frequency is non-zero.  An object sets
all four Drude values of the points it covers.  ``sigma`` is the electric
conductivity in S/m (default 0, 3D schemes, no ``--use-metamaterials`` needed):
part of the complex permittivity, painted by the rule of ``eps`` (smoothed the
same way; an object without the key sets 0 where it covers) and not combined
with ``omega_p`` on one object.  ``mu`` is 1 everywhere.  A
cylinder's ``center`` holds its two in-plane coordinates, in x, y, z order of
the two axes other than ``axis``; ``span`` is its extent along ``axis``.

Signed distances ``d`` (fp64, eps-grid units): sphere ``|p - c| - r``; box the
largest of ``lo_a - p_a``, ``p_a - hi_a`` over the axes -- exact on faces, a
Chebyshev distance at edges and corners (the smoothed zone there is square,
not rounded); cylinder the larger of the radial and the axial distance.

A mesh is a closed, consistently oriented triangle surface, inline
(``vertices`` + ``triangles``) or from a binary or ASCII STL ``file`` (resolved
against the scene file's directory, from Python against the working
directory); a vertex sits at ``scale * v + translate`` (fp64, once, here).  It
is not rotated.  Its ``d`` is negative where a ray along +z crosses the surface
an odd number of times (the even-odd rule; a ray through a projected edge or
vertex counts as the same ray displaced by an infinitesimal (-e^2, +e) would),
and its magnitude is the Euclidean distance to the closest triangle.  A point
exactly on the surface may fall on either side.  3D schemes only.

This module also defines the fixed-size table entry both backends'
``scene_sample`` op reads (csrc/scene_kernels.hip ``SceneEnt``).
"""

from __future__ import annotations

import json
import math
import os
import struct
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

SCENE_MAX_OBJECTS = 256  # entries of the kernel's table (fdtd_scene_max_objects)
SCENE_ENT = np.dtype([("kind", "<i4"), ("flags", "<i4"), ("p", "<f8", (3,)), ("q", "<f8", (3,)),
                      ("eps", "<f8"), ("omega", "<f8")])
SCENE_ENT_SIZE = 72      # bytes of a table entry (fdtd_scene_ent_size)
assert SCENE_ENT.itemsize == SCENE_ENT_SIZE

SCENE_MAX_TRIANGLES = 2 ** 20  # over all meshes of a scene (fdtd_scene_max_triangles)

KIND_BOX, KIND_SPHERE, KIND_CYLINDER, KIND_MESH = 0, 1, 2, 3
# SceneEnt.flags: bits 0-1 the cylinder's axis, bits 2-4 the axes the object
# ignores (the inactive axis of a 2D scheme), bit 5 sharp eps (smoothing none)
FLAG_IGNORE_SHIFT = 2
FLAG_SHARP = 32

# the quantities of ``scene_sample``, by the kernel's index: the plasma frequencies (electric, magnetic) and
# the collision frequencies of the same poles; "cond" is the conductivity (the key ``sigma``), painted like eps
QUANTITIES = ("eps", "omega", "omega_m", "gamma", "gamma_m", "cond")

SHAPES = ("box", "sphere", "cylinder", "mesh")
SMOOTHINGS = ("linear", "none")
_MEDIUM = {"eps", "omega_p", "gamma", "omega_pm", "gamma_m", "sigma"}
_KEYS = {"box": {"shape", "lo", "hi"} | _MEDIUM,
         "sphere": {"shape", "center", "radius"} | _MEDIUM,
         "cylinder": {"shape", "axis", "center", "radius", "span"} | _MEDIUM,
         "mesh": {"shape", "file", "vertices", "triangles", "scale", "translate"} | _MEDIUM}
_AXES = {"x": 0, "y": 1, "z": 2}


class Mesh:
    """The triangles of a validated mesh: ``tris`` = (n, 3, 3) fp64, vertex
    coordinates in cells (scaled and translated), the three vertices of every
    triangle in ascending (x, y, z) order -- the one order both backends
    evaluate a triangle and its edges in, whichever way the input wound it."""
    __slots__ = ("tris",)

    def __init__(self, tris: np.ndarray):
        self.tris = tris

    def __len__(self) -> int:
        return len(self.tris)

    def __eq__(self, other):
        return isinstance(other, Mesh) and np.array_equal(self.tris, other.tris)

    def __hash__(self):
        return hash(self.tris.shape)

    def __repr__(self):
        return "Mesh(%d triangles)" % len(self.tris)


@dataclass(frozen=True)
class SceneObject:
    """One validated object.  Box: ``a`` = lo, ``b`` = hi.  Sphere: ``a`` =
    centre, ``radius``.  Cylinder: ``axis``, ``a`` = centre with the span's
    lower end at ``axis``, ``b[axis]`` = the span's upper end, ``radius``.
    Mesh: ``mesh``, ``a`` / ``b`` = the lower / upper corner of its bounding box."""
    shape: str
    a: Tuple[float, float, float]
    b: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    radius: float = 0.0
    axis: int = 0
    eps: float = 1.0
    omega_p: float = 0.0
    mesh: Optional[Mesh] = None
    gamma: float = 0.0      # electric collision frequency, in units of 2 pi f_source like omega_p
    omega_pm: float = 0.0   # magnetic Drude plasma frequency
    gamma_m: float = 0.0    # magnetic collision frequency
    sigma: float = 0.0      # electric conductivity, S/m


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


_STL_RECORD = np.dtype([("normal", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")])
assert _STL_RECORD.itemsize == 50


def _too_many_triangles(n: int) -> ValueError:
    return ValueError("scene: %d triangles, a scene holds %d" % (n, SCENE_MAX_TRIANGLES))


def load_stl(path: str) -> np.ndarray:
    """The triangles of the STL file ``path`` as stored: (n, 3, 3) fp64.  The
    file is binary when its size is 84 + 50 * the count after its 80-byte
    header, otherwise ASCII (solid / facet normal / vertex); stored normals
    are ignored.  ValueError for a file that is neither."""
    try:
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = f.read(84)
            if len(head) == 84:
                count = struct.unpack("<I", head[80:])[0]
                if size == 84 + 50 * count:
                    if count > SCENE_MAX_TRIANGLES:
                        raise _too_many_triangles(count)
                    rec = np.fromfile(f, dtype=_STL_RECORD, count=count)
                    if len(rec) == count:
                        return rec["v"].astype(np.float64)
            f.seek(0)
            data = f.read()
    except OSError as e:
        raise ValueError("scene: STL file %s: %s" % (path, e.strerror or e))
    bad = ValueError("scene: STL file %s is neither a binary STL of the size its header states (truncated?) "
                     "nor a complete ASCII STL" % path)
    try:
        lines = data.decode("ascii").splitlines()
    except UnicodeDecodeError:
        raise bad
    if not lines or lines[0].split()[:1] != ["solid"]:
        raise bad
    corners, in_loop, ended = [], None, False
    for line in lines[1:]:
        w = line.split()
        if not w:
            continue
        if w[0] == "vertex" and len(w) == 4 and in_loop is not None:
            try:
                corners.append((float(w[1]), float(w[2]), float(w[3])))
            except ValueError:
                raise bad
            in_loop += 1
        elif w[0] == "outer" and in_loop is None:
            in_loop = 0
            if len(corners) >= 3 * SCENE_MAX_TRIANGLES:
                raise _too_many_triangles(len(corners) // 3 + 1)
        elif w[0] == "endloop" and in_loop == 3:
            in_loop = None
        elif w[0] in ("facet", "endfacet") and in_loop is None:
            pass
        elif w[0] == "endsolid" and in_loop is None:
            ended = True
            break
        else:
            raise bad
    if not ended:
        raise bad
    return np.asarray(corners, dtype=np.float64).reshape(-1, 3, 3)


def _mesh(o: dict, what: str, base_dir: Optional[str]) -> Tuple[Mesh, Tuple[float, ...], Tuple[float, ...]]:
    """(mesh, bounding box lo, hi) of a mesh object's dictionary: read, welded,
    scaled and translated, then checked to be a closed, consistently oriented
    surface of triangles with area."""
    inline = [k in o for k in ("vertices", "triangles")]
    if ("file" in o) == any(inline) or (any(inline) and not all(inline)):
        raise ValueError("scene: %sneeds either 'file' or both 'vertices' and 'triangles'" % what)
    scale = _number(o.get("scale", 1.0), what + "scale")
    if scale <= 0:
        raise ValueError("scene: %sscale must be positive, got %r" % (what, scale))
    translate = _vector(o.get("translate", (0.0, 0.0, 0.0)), 3, what + "translate")
    if "file" in o:
        if not isinstance(o["file"], str) or not o["file"]:
            raise ValueError("scene: %sfile must be a path, got %r" % (what, o["file"]))
        corners = load_stl(o["file"] if base_dir is None else os.path.join(base_dir, o["file"]))
        # weld: corners whose three values are exactly equal are one vertex
        verts, tri = np.unique(corners.reshape(-1, 3), axis=0, return_inverse=True)
        tri = tri.reshape(-1, 3)
    else:
        if not isinstance(o["triangles"], (list, tuple)) or not isinstance(o["vertices"], (list, tuple)):
            raise ValueError("scene: %svertices and triangles must be lists" % what)
        if len(o["triangles"]) > SCENE_MAX_TRIANGLES:
            raise _too_many_triangles(len(o["triangles"]))
        try:
            verts, tri = np.asarray(o["vertices"]), np.asarray(o["triangles"])
        except ValueError:   # ragged lists
            verts = tri = np.empty((0,), dtype=object)
        if len(o["vertices"]) and (verts.ndim != 2 or verts.shape[1] != 3 or verts.dtype.kind not in "iuf"):
            raise ValueError("scene: %svertices must be lists of 3 numbers" % what)
        if len(o["triangles"]) and (tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu"):
            raise ValueError("scene: %striangles must be lists of 3 vertex indices" % what)
        verts, tri = verts.astype(np.float64).reshape(-1, 3), tri.astype(np.int64).reshape(-1, 3)
    if not np.isfinite(verts).all():
        raise ValueError("scene: %svertices must be finite" % what)
    if len(tri) < 4:
        raise ValueError("scene: %shas %d triangles: a closed mesh has at least 4" % (what, len(tri)))
    if int(tri.min()) < 0 or int(tri.max()) >= len(verts):
        raise ValueError("scene: %shas a vertex index out of range (%d vertices)" % (what, len(verts)))
    p = scale * verts + np.asarray(translate, dtype=np.float64)
    if not np.isfinite(p).all():
        raise ValueError("scene: %svertices must be finite after scale and translate" % what)
    i, j, k = tri[:, 0], tri[:, 1], tri[:, 2]
    rep = np.flatnonzero((i == j) | (j == k) | (k == i))
    if len(rep):
        raise ValueError("scene: %striangle %d repeats a vertex" % (what, rep[0]))
    flat = np.flatnonzero(~np.cross(p[j] - p[i], p[k] - p[i]).any(axis=1))
    if len(flat):
        raise ValueError("scene: %striangle %d is degenerate (its cross product is zero)" % (what, flat[0]))
    # every undirected edge in exactly two triangles, once in each direction
    u, v = np.concatenate((i, j, k)), np.concatenate((j, k, i))
    nv = len(verts)
    und, counts = np.unique(np.minimum(u, v) * nv + np.maximum(u, v), return_counts=True)
    if (counts != 2).any():
        e = int(und[np.flatnonzero(counts != 2)[0]])
        raise ValueError("scene: %sis not closed: the edge between vertices %d and %d belongs to %d triangles, "
                         "not 2" % (what, e // nv, e % nv, int(counts[counts != 2][0])))
    if len(np.unique(u * nv + v)) != len(u):
        raise ValueError("scene: %sis not consistently oriented: two triangles run along an edge in the same "
                         "direction" % what)
    t = p[tri]
    order = np.lexsort((t[:, :, 2], t[:, :, 1], t[:, :, 0]), axis=1)
    t = np.ascontiguousarray(np.take_along_axis(t, order[:, :, None], axis=1))
    lo, hi = t.reshape(-1, 3).min(axis=0), t.reshape(-1, 3).max(axis=0)
    return Mesh(t), tuple(float(x) for x in lo), tuple(float(x) for x in hi)


def parse_object(o, index: int = 0, base_dir: Optional[str] = None) -> SceneObject:
    """A :class:`SceneObject` from its JSON dictionary; ValueError with a
    message for everything the format refuses.  ``base_dir``: the directory a
    mesh's ``file`` is resolved against (None: the working directory)."""
    if isinstance(o, SceneObject):
        return o
    if not isinstance(o, dict):
        raise ValueError("scene: object %d must be a dictionary, got %r" % (index, o))
    shape = o.get("shape")
    if shape not in SHAPES:
        raise ValueError("scene: object %d has unknown shape %r (box, sphere, cylinder or mesh)" % (index, shape))
    unknown = sorted(set(o) - _KEYS[shape])
    if unknown:
        raise ValueError("scene: object %d (%s) has unknown key %r" % (index, shape, unknown[0]))
    what = "object %d (%s) " % (index, shape)
    for k in sorted(_KEYS[shape] - _MEDIUM - set(o) if shape != "mesh" else ()):
        raise ValueError("scene: %sneeds %r" % (what, k))
    eps = _number(o.get("eps", 1.0), what + "eps")
    omega_p = _number(o.get("omega_p", 0.0), what + "omega_p")
    if eps <= 0:
        raise ValueError("scene: %seps must be positive, got %r" % (what, eps))
    if omega_p < 0:
        raise ValueError("scene: %somega_p must not be negative, got %r" % (what, omega_p))
    drude = {}
    for k in ("gamma", "omega_pm", "gamma_m"):
        drude[k] = _number(o.get(k, 0.0), what + k)
        if drude[k] < 0:
            raise ValueError("scene: %s%s must not be negative, got %r" % (what, k, drude[k]))
    if drude["gamma"] > 0 and omega_p == 0:
        raise ValueError("scene: %sgamma needs omega_p > 0: a damping without a pole" % what)
    if drude["gamma_m"] > 0 and drude["omega_pm"] == 0:
        raise ValueError("scene: %sgamma_m needs omega_pm > 0: a damping without a pole" % what)
    drude["sigma"] = _number(o.get("sigma", 0.0), what + "sigma")
    if drude["sigma"] < 0:
        raise ValueError("scene: %ssigma must not be negative, got %r" % (what, drude["sigma"]))
    if drude["sigma"] > 0 and omega_p > 0:
        raise ValueError("scene: %ssigma and omega_p on one object: the pole's cells run the D/B chain, which has "
                         "no conductive term" % what)
    if shape == "mesh":
        mesh, lo, hi = _mesh(o, what, base_dir)
        return SceneObject("mesh", lo, hi, eps=eps, omega_p=omega_p, mesh=mesh, **drude)
    if shape == "box":
        lo, hi = _vector(o["lo"], 3, what + "lo"), _vector(o["hi"], 3, what + "hi")
        if any(l >= h for l, h in zip(lo, hi)):
            raise ValueError("scene: %sneeds lo < hi on every axis, got %r, %r" % (what, lo, hi))
        return SceneObject("box", lo, hi, eps=eps, omega_p=omega_p, **drude)
    radius = _number(o["radius"], what + "radius")
    if radius <= 0:
        raise ValueError("scene: %sradius must be positive, got %r" % (what, radius))
    if shape == "sphere":
        return SceneObject("sphere", _vector(o["center"], 3, what + "center"), radius=radius, eps=eps,
                           omega_p=omega_p, **drude)
    if o["axis"] not in _AXES:
        raise ValueError("scene: %saxis must be x, y or z, got %r" % (what, o["axis"]))
    axis = _AXES[o["axis"]]
    c2, span = _vector(o["center"], 2, what + "center"), _vector(o["span"], 2, what + "span")
    if span[0] >= span[1]:
        raise ValueError("scene: %sneeds span lo < hi, got %r" % (what, span))
    a, b, others = [0.0] * 3, [0.0] * 3, [d for d in range(3) if d != axis]
    a[others[0]], a[others[1]], a[axis], b[axis] = c2[0], c2[1], span[0], span[1]
    return SceneObject("cylinder", tuple(a), tuple(b), radius=radius, axis=axis, eps=eps, omega_p=omega_p, **drude)


def parse_objects(objects: Sequence, smoothing: str = "linear",
                  base_dir: Optional[str] = None) -> Tuple[SceneObject, ...]:
    if smoothing not in SMOOTHINGS:
        raise ValueError("scene: smoothing must be linear or none, got %r" % (smoothing,))
    if not isinstance(objects, (list, tuple)):
        raise ValueError("scene: objects must be a list, got %r" % (objects,))
    if len(objects) > SCENE_MAX_OBJECTS:
        raise ValueError("scene: %d objects, the table holds %d" % (len(objects), SCENE_MAX_OBJECTS))
    out, triangles = [], 0
    for n, o in enumerate(objects):
        out.append(parse_object(o, n, base_dir))
        triangles += len(out[-1].mesh) if out[-1].mesh is not None else 0
        if triangles > SCENE_MAX_TRIANGLES:
            raise _too_many_triangles(triangles)
    return tuple(out)


def check_scheme(objects: Sequence[SceneObject], scheme: str) -> None:
    """What a scheme refuses: every file scene in 1D, a cylinder that does
    not lie along the inactive axis in 2D, a mesh in 2D, a conductivity in
    2D."""
    if scheme == "1d":
        raise ValueError("scene: file scenes need a 2D or 3D scheme")
    if scheme != "3d":
        for n, o in enumerate(objects):
            if o.sigma > 0:
                raise ValueError("scene: object %d: sigma needs a 3D scheme" % n)
    if scheme in ("tmz", "tez"):
        for n, o in enumerate(objects):
            if o.shape == "cylinder" and o.axis != 2:
                raise ValueError("scene: object %d: a cylinder of a 2D scheme must lie along z, the inactive axis" % n)
            if o.shape == "mesh":
                raise ValueError("scene: object %d: a mesh needs a 3D scheme" % n)


def lossy_bbox(objects: Sequence[SceneObject]) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """The cell box that holds every lossy object (``sigma > 0``) with the
    cell of smoothing and of component averaging around it: an upper bound
    of the lossy box, known before anything is sampled."""
    lo, hi = [1 << 30] * 3, [-(1 << 30)] * 3
    for o in objects:
        if o.sigma <= 0:
            continue
        if o.shape in ("box", "mesh"):
            a, b = list(o.a), list(o.b)
        else:
            a, b = [v - o.radius for v in o.a], [v + o.radius for v in o.a]
            if o.shape == "cylinder":
                a[o.axis], b[o.axis] = o.a[o.axis], o.b[o.axis]
        for d in range(3):
            lo[d] = min(lo[d], int(math.floor(a[d])) - 2)
            hi[d] = max(hi[d], int(math.ceil(b[d])) + 2)
    return tuple(lo), tuple(hi)


def refuse_lossy_config(cfg, objects: Sequence[SceneObject]) -> Optional[str]:
    """Why the configuration cannot run with the lossy media (``sigma > 0``)
    of its scene (None: it can, or there are none)."""
    if not any(o.sigma > 0 for o in objects):
        return None
    if cfg.complex_values:
        return "scene: sigma with --complex-field-values: the conductive update runs on real fields"
    if cfg.use_amp_mode:
        return "scene: sigma with --use-amp-mode: amplitude mode has no conductive update"
    if cfg.use_hip_graph:
        return "scene: sigma with --use-hip-graph: the captured steps have no conductive update"
    return None


def parse_scene(doc, base_dir: Optional[str] = None) -> Tuple[Tuple[SceneObject, ...], str]:
    """(objects, smoothing) of a parsed scene document; ``base_dir`` as in
    :func:`parse_object`."""
    if not isinstance(doc, dict):
        raise ValueError("scene: the file must hold one JSON object")
    unknown = sorted(set(doc) - {"smoothing", "objects"})
    if unknown:
        raise ValueError("scene: unknown key %r" % unknown[0])
    if "objects" not in doc:
        raise ValueError("scene: needs 'objects'")
    smoothing = doc.get("smoothing", "linear")
    return parse_objects(doc["objects"], smoothing, base_dir), smoothing


def load_scene_file(path: str) -> Tuple[Tuple[SceneObject, ...], str]:
    """(objects, smoothing) of the scene file ``path``; SettingsError for a
    file that cannot be read or that the format refuses."""
    from ..utils.settings import SettingsError

    def refuse_constant(name):  # NaN / Infinity, which json accepts by default
        raise ValueError("scene: non-finite number %s" % name)

    try:
        with open(path, "r", encoding="utf-8") as f:
            doc = json.load(f, parse_constant=refuse_constant)
        return parse_scene(doc, os.path.dirname(os.path.abspath(path)))
    except OSError as e:
        raise SettingsError("--scene-file %s: %s" % (path, e.strerror or e))
    except ValueError as e:  # JSONDecodeError included
        raise SettingsError("--scene-file %s: %s" % (path, e))


class SceneTable:
    """The objects as the table of ``ops.scene_sample``: ``ents`` = numpy
    records of :data:`SCENE_ENT`, coordinates in cells (the op scales them by
    its ``mod``), ``omega`` = omega_p * 2 pi f in rad/s.  A mesh's entry holds
    its bounding box in ``p`` / ``q``; its triangles are rows ``ranges[o, 0]``
    to ``ranges[o, 0] + ranges[o, 1]`` of ``tris`` = (n, 3, 3) fp64 (vertices in
    the order of :class:`Mesh`), ``ranges`` = (objects, 2) int32, zero for every
    other kind.  ``drude`` = (objects, 3) fp64 travels beside the entries: an
    object's (gamma_e, omega_m, gamma_m) in rad/s, zeros by default; so does
    ``cond`` = (objects,) fp64, an object's conductivity in S/m.
    ``device_tables`` caches the HIP backend's copies, one per device."""

    def __init__(self, ents: np.ndarray, tris: Optional[np.ndarray] = None, ranges: Optional[np.ndarray] = None,
                 drude: Optional[np.ndarray] = None, cond: Optional[np.ndarray] = None):
        if ents.dtype != SCENE_ENT or ents.ndim != 1:
            raise ValueError("SceneTable: a 1D array of SCENE_ENT records")
        if len(ents) > SCENE_MAX_OBJECTS:
            raise ValueError("scene: %d objects, the table holds %d" % (len(ents), SCENE_MAX_OBJECTS))
        tris = np.zeros((0, 3, 3), dtype=np.float64) if tris is None else tris
        ranges = np.zeros((len(ents), 2), dtype=np.int32) if ranges is None else ranges
        if tris.dtype != np.float64 or tris.ndim != 3 or tris.shape[1:] != (3, 3):
            raise ValueError("SceneTable: tris of shape (n, 3, 3), float64")
        if len(tris) > SCENE_MAX_TRIANGLES:
            raise _too_many_triangles(len(tris))
        if ranges.dtype != np.int32 or ranges.shape != (len(ents), 2):
            raise ValueError("SceneTable: ranges of shape (objects, 2), int32")
        drude = np.zeros((len(ents), 3), dtype=np.float64) if drude is None else drude
        if drude.dtype != np.float64 or drude.shape != (len(ents), 3):
            raise ValueError("SceneTable: drude of shape (objects, 3), float64")
        if not np.isfinite(drude).all() or (drude < 0).any():
            raise ValueError("SceneTable: drude values must be finite and not negative")
        cond = np.zeros((len(ents),), dtype=np.float64) if cond is None else cond
        err = cond_error(cond, len(ents))
        if err:
            raise ValueError("SceneTable: " + err)
        self.cond = cond
        self.ents = ents
        self.tris = tris
        self.ranges = ranges
        self.drude = drude
        self.device_tables = {}

    def __len__(self) -> int:
        return len(self.ents)

    def has_meshes(self) -> bool:
        return bool((self.ents["kind"] == KIND_MESH).any())

    def range_error(self) -> Optional[str]:
        """Why the triangle ranges do not fit ``tris`` (None: they do)."""
        if self.ranges.shape != (len(self.ents), 2) or self.ranges.dtype != np.int32:
            return "ranges of shape (objects, 2), int32"
        r = self.ranges.astype(np.int64)
        if len(r) and (int(r.min()) < 0 or int((r[:, 0] + r[:, 1]).max()) > len(self.tris)):
            return "a triangle range past the %d triangles of the table" % len(self.tris)
        return None


def cond_error(cond, nobj: int) -> Optional[str]:
    """Why ``cond`` is no conductivity table of ``nobj`` objects (None: it is one)."""
    if (not isinstance(cond, np.ndarray) or cond.dtype != np.float64 or cond.shape != (nobj,)
            or not np.isfinite(cond).all() or (cond < 0).any()):
        return "cond of shape (%d,), float64, finite and not negative" % nobj
    return None


def build_table(objects: Sequence[SceneObject], scheme: str = "3d", smoothing: str = "linear",
                source_frequency: float = 1.0) -> SceneTable:
    objects = parse_objects(list(objects), smoothing)
    check_scheme(objects, scheme)
    ents = np.zeros(len(objects), dtype=SCENE_ENT)
    ranges = np.zeros((len(objects), 2), dtype=np.int32)
    drude = np.zeros((len(objects), 3), dtype=np.float64)
    cond = np.array([o.sigma for o in objects], dtype=np.float64).reshape(len(objects))
    tris, first = [], 0
    ignore = 0 if scheme == "3d" else 4  # 2D: objects ignore z
    for n, (e, o) in enumerate(zip(ents, objects)):
        e["kind"] = SHAPES.index(o.shape)
        e["flags"] = o.axis | (ignore << FLAG_IGNORE_SHIFT) | (FLAG_SHARP if smoothing == "none" else 0)
        e["p"] = o.a
        e["q"] = o.b if o.shape in ("box", "mesh") else (o.radius, o.b[o.axis], 0.0)
        e["eps"] = o.eps
        e["omega"] = o.omega_p * 2 * math.pi * source_frequency
        drude[n] = [v * 2 * math.pi * source_frequency for v in (o.gamma, o.omega_pm, o.gamma_m)]
        if o.shape == "mesh":
            ranges[n] = (first, len(o.mesh))
            tris.append(o.mesh.tris)
            first += len(o.mesh)
    return SceneTable(ents, np.concatenate(tris) if tris else None, ranges, drude, cond)


def sample_args(quantity: str, points, origin, shape, stride, mod):
    """The arguments of ``scene_sample`` checked and normalised (both
    backends): (quantity index, points, origin, shape, stride, mod)."""
    if quantity not in QUANTITIES:
        raise ValueError("scene_sample: quantity eps, omega, omega_m, gamma, gamma_m or cond, got %r" % (quantity,))
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
    return QUANTITIES.index(quantity), pts, origin, shape, stride, float(mod)
