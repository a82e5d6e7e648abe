"""The ``scene_sample`` operation of the HIP backend, a mixin of
:class:`~.hip_ops.HipOps` (csrc/scene_kernels.hip): a file scene's objects
evaluated at a component's material stencil and averaged, in one launch; a
scene with meshes through the kernel's mesh form and its triangle tables.
Everything is validated before the launch; a missing kernel is an error.
"""

from __future__ import annotations

import ctypes

import numpy as np
import torch

from ..layout.scene_file import (cond_error, SCENE_ENT_SIZE, SCENE_MAX_OBJECTS, SCENE_MAX_TRIANGLES, SceneTable,
                                 sample_args)
from .hip_lib import HipError, _check, _ptr, _stream, c_double, c_int


class HipSceneOps:
    """Needs ``lib``, ``device`` and ``launches`` of :class:`~.hip_ops.HipOps`."""

    def _scene_dev(self, table: SceneTable, suffix: str, build):
        """One of ``table``'s tables on the device: ``build()`` = (a tuple of)
        numpy arrays, a row per entry, each padded to at least one row (so a
        pointer is never null); cached on ``table`` per device and ``suffix``."""
        key = str(torch.device(self.device)) + suffix
        dev = table.device_tables.get(key)
        if dev is None:
            def padded(rows):
                rows = torch.from_numpy(rows.copy())
                host = rows.new_zeros((max(1, len(rows)),) + tuple(rows.shape[1:]))
                host[:len(rows)] = rows
                return host.to(self.device)
            host = build()
            dev = table.device_tables[key] = (tuple(map(padded, host)) if isinstance(host, tuple) else padded(host))
        return dev

    def _scene_table(self, table: SceneTable) -> torch.Tensor:
        """The entries, SCENE_ENT_SIZE bytes each."""
        raw = self.lib.raw
        if int(raw.fdtd_scene_ent_size()) != SCENE_ENT_SIZE or int(raw.fdtd_scene_max_objects()) != SCENE_MAX_OBJECTS:
            raise HipError("SceneEnt layout mismatch")
        return self._scene_dev(table, "", lambda: table.ents.view("u1").reshape(len(table), SCENE_ENT_SIZE))

    def _scene_triangles(self, table: SceneTable):
        """(triangles, ranges) of a table with meshes: 72 bytes a triangle, two
        ints an object."""
        raw = self.lib.raw
        if int(raw.fdtd_scene_tri_size()) != 72 or int(raw.fdtd_scene_max_triangles()) != SCENE_MAX_TRIANGLES:
            raise HipError("SceneTri layout mismatch")
        return self._scene_dev(table, " triangles", lambda: (table.tris.reshape(-1, 9), table.ranges))

    def _scene_drude(self, table: SceneTable) -> torch.Tensor:
        """``table.drude``: (gamma_e, omega_m, gamma_m) an object, 24 bytes."""
        if int(self.lib.raw.fdtd_scene_drude_size()) != 24:
            raise HipError("SceneDrude layout mismatch")
        return self._scene_dev(table, " drude", lambda: table.drude)

    def _scene_cond(self, table: SceneTable) -> torch.Tensor:
        """``table.cond``: a double an object."""
        return self._scene_dev(table, " cond", lambda: table.cond)

    def scene_sample(self, table, quantity: str, points, origin, shape, stride, mod, out=None,
                     cull: bool = True) -> torch.Tensor:
        """The contract of ``TorchOps.scene_sample`` in ONE launch of
        k_scene_sample<Q, MESH> (MESH when the table holds a mesh; omega_m,
        gamma and gamma_m read ``table.drude`` as their side table, cond
        ``table.cond``).  ``out``: a contiguous fp64 device tensor of ``shape``
        to fill (allocated otherwise); ``cull`` = False evaluates every object
        at every cell (measurements)."""
        if not isinstance(table, SceneTable):
            raise HipError("scene_sample: a SceneTable, got %r" % type(table).__name__)
        if len(table) > SCENE_MAX_OBJECTS:
            raise HipError("scene_sample: %d objects, the table holds %d" % (len(table), SCENE_MAX_OBJECTS))
        meshes = table.has_meshes()
        if meshes and len(table.tris) > SCENE_MAX_TRIANGLES:
            raise HipError("scene_sample: %d triangles, a scene holds %d" % (len(table.tris), SCENE_MAX_TRIANGLES))
        if meshes and table.range_error():
            raise HipError("scene_sample: " + table.range_error())
        drude = getattr(table, "drude", None)
        if (not isinstance(drude, np.ndarray) or drude.dtype != np.float64 or drude.shape != (len(table), 3)
                or not np.isfinite(drude).all() or (drude < 0).any()):
            raise HipError("scene_sample: drude of shape (%d, 3), float64, finite and not negative" % len(table))
        err = cond_error(getattr(table, "cond", None), len(table))
        if err:
            raise HipError("scene_sample: " + err)
        try:
            q, pts, origin, shape, stride, mod = sample_args(quantity, points, origin, shape, stride, mod)
        except ValueError as e:
            raise HipError(str(e))
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device.type != "cuda" or out.dtype != torch.float64
              or not out.is_contiguous() or tuple(out.shape) != shape):
            raise HipError("scene_sample: out must be a contiguous float64 device tensor of shape %s" % (shape,))
        if out.numel() == 0:
            return out
        if out.data_ptr() % 8:
            raise HipError("scene_sample: out not aligned to its element size")
        tab = self._scene_table(table)
        i3 = ctypes.c_int * 3
        flat = [v for p in pts for v in p]
        # the quantity's side table and its true size: the conductivities, the second table or none
        side, side_bytes = ((self._scene_cond(table), table.cond.nbytes) if q == 5 else
                            (self._scene_drude(table), drude.nbytes) if q >= 2 else (None, 0))
        tris, ranges = self._scene_triangles(table) if meshes else (None, None)
        f = self.lib.raw.fdtd_scene_sample
        f.restype = c_int
        rc = f(_ptr(tab), c_int(len(table)), c_int(q), (ctypes.c_int * len(flat))(*flat), c_int(len(pts)),
               i3(*origin), i3(*shape), i3(*stride), c_double(mod), c_int(1 if cull else 0), _ptr(out), _stream(),
               _ptr(side), ctypes.c_size_t(side_bytes), _ptr(tris), c_int(len(table.tris) if meshes else 0),
               _ptr(ranges))
        _check(rc, "scene_sample")
        self.launches += 1
        return out
