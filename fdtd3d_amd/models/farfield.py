"""Far-field monitor: radiation patterns, radiated power, directivity and RCS
per wavelength from the phasors of a running-DFT monitor.

A :class:`FarFieldMonitor` is a :class:`~.surface.SurfaceMonitor`: it watches
the box ``margin`` cells inside the grid borders of a 3D run through a
:class:`~.dft.DftMonitor` with ``h_time="half"``, its own or the one of a
:class:`~.flux.FluxMonitor` on the same box.  The tangential phasors on a face
with outward normal ``n`` are the equivalent currents ``J = n x H``, ``M = -n x
E``; their radiation vectors in the direction ``rhat``, with the project's
``exp(-i w t)`` phasors,

    N(rhat) = dx^2 sum over the face cells of J exp(-i kappa rhat . r'),   L = (same with M),

``r'`` measured from the geometric centre of the grid, come from the backend
op ``ops.dft_farfield`` (csrc/farfield_kernels.hip), which evaluates them in
fp64 from the raw accumulators for every wavelength and direction at once.  In
spherical components the radiant intensity is

    U(theta, phi) = kappa^2 / (32 pi^2 eta0) (|L_phi + eta0 N_theta|^2 + |L_theta - eta0 N_phi|^2)   [W / sr],

which at unit source amplitude is ``ntff_power / (4 pi eta0)`` (models/ntff.py,
the diagram of ``--use-ntff``).  From it: :meth:`FarFieldMonitor.total_power`
(Gauss-Legendre in ``cos theta`` x uniform ``phi``), :meth:`directivity` ``= 4
pi U / total_power`` and, in TF/SF runs with the box outside the TF/SF box,
the bistatic :meth:`rcs` ``= 4 pi U / incident`` in m^2, ``incident`` the
intensity of the source signal at every wavelength (models/surface.py) -- a
sine source over whole periods and a Gaussian pulse take the same path.

The sampling window must cover whole periods of a steady state or the whole
pulse (models/flux.py).
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ..ops.dft import FarTerm, FarTerms
from ..utils.assertions import FdtdError
from ..utils.constants import PI
from .dft import DftMonitor, parse_wavelengths
from .ntff import ETA0, _sample_plan
from .surface import SurfaceMonitor


def farfield_from_config(scheme, flux=None) -> Optional["FarFieldMonitor"]:
    """The monitor ``--use-farfield`` asks for, registered with the scheme
    (after ``init_grids``); None without the option.  ``flux``: the run's
    flux monitor -- on the same box the far-field monitor reads its slabs,
    which are then sampled once."""
    cfg = scheme.cfg
    if not cfg.use_farfield:
        return None
    from .dft import refuse_config
    why = refuse_config(cfg)
    if why:
        raise FdtdError(why)
    shared = flux.dft if flux is not None and tuple(flux.margin) == tuple(cfg.farfield_size) else None
    return FarFieldMonitor(scheme, cfg.farfield_size, parse_wavelengths(cfg.dft_wavelengths, scheme.wavelength),
                           cfg.dft_step, cfg.dft_start, dft=shared)


def directions(thetas, phis) -> torch.Tensor:
    """(T * P, 3) float64 unit vectors of the grid ``thetas`` x ``phis``
    (radians), ``phi`` fastest."""
    th = torch.as_tensor(thetas, dtype=torch.float64).reshape(-1, 1)
    ph = torch.as_tensor(phis, dtype=torch.float64).reshape(1, -1)
    st = torch.sin(th)
    return torch.stack([st * torch.cos(ph), st * torch.sin(ph), torch.cos(th).expand(-1, ph.shape[1])],
                       dim=-1).reshape(-1, 3)


def report_grid(ntheta: int, nphi: int):
    """The uniform report grid: ``ntheta`` polar angles over [0, pi] with both
    ends, ``nphi`` azimuthal angles over [0, 2 pi)."""
    if ntheta < 2 or nphi < 1:
        raise FdtdError("--farfield-ntheta >= 2 and --farfield-nphi >= 1")
    return (torch.linspace(0.0, PI, ntheta, dtype=torch.float64),
            torch.arange(nphi, dtype=torch.float64) * (2 * PI / nphi))


class FarFieldMonitor(SurfaceMonitor):
    """Far field of the box ``margin`` cells inside the grid borders at
    ``wavelengths``; ``step`` (0 = automatic) and ``start`` as for
    :class:`~.dft.DftMonitor`.  ``dft``: an existing monitor over the same
    slabs (``ntff_requests(size, margin)``, ``h_time="half"``, the same
    wavelengths) that something else samples, e.g. ``FluxMonitor.dft``."""

    box_name = "far-field box"

    def __init__(self, scheme, margin: Sequence[int], wavelengths: Sequence[float], step: int = 0, start: int = 0,
                 dft: Optional[DftMonitor] = None, register: bool = True):
        super().__init__(scheme, margin, wavelengths, step, start, dft, register)
        self.wavenumbers = [2 * PI / w for w in self.wavelengths]

    def _label(self, cfg) -> str:
        """``radiated`` without TF/SF, else ``scattered``: the box must lie
        outside the TF/SF box (the far field of the total field is no
        scattering pattern)."""
        place = self._placement(cfg)
        if place == "inside":
            raise FdtdError("FarFieldMonitor: the far-field box (margin %s) lies inside the TF/SF box (margin %s): "
                            "the far field of the total field is not a scattering pattern"
                            % (self.margin, tuple(cfg.tfsf_size)))
        return "radiated" if place == "none" else "scattered"

    # ------------------------------------------------------------------- results
    def _build_terms(self, gathered: bool) -> Optional[FarTerms]:
        """J = n x H into the N slots, M = -n x E into the L slots, face by
        face (the signs of models/ntff.py ``ntff_power``); positions relative
        to the geometric centre of the grid."""
        terms = FarTerms(len(self.wavelengths), self.dx)
        missing = False
        for axis, x0, s, lo, hi in self.faces:
            a1, a2 = [a for a in range(3) if a != axis]
            cyc = 1 if (a1 - axis) % 3 == 1 else -1
            sc = int(s) * cyc
            pos0 = [((x0 if a == axis else lo[a] + 0.5) - self.size[a] / 2.0) * self.dx for a in range(3)]
            for slot, sign, comp in ((a2, sc, "H" + "xyz"[a1]), (a1, -sc, "H" + "xyz"[a2]),
                                     (3 + a2, -sc, "E" + "xyz"[a1]), (3 + a1, sc, "E" + "xyz"[a2])):
                plan = _sample_plan(comp, axis, x0, lo, hi)
                op = self._operand(comp, plan, gathered)
                if op is None:
                    missing = True
                    continue
                terms.add(FarTerm(slot, sign, [n for _, n, _ in plan], op, pos0))
        return None if missing else terms

    def vectors_many(self, dir_sets: Sequence[torch.Tensor]) -> Optional[List[torch.Tensor]]:
        """:meth:`vectors` of several direction sets from one evaluation (a
        decomposed run gathers the accumulators once)."""
        terms = self._current_terms()
        if terms is None:
            return None
        sets = [torch.as_tensor(d, dtype=torch.float64).reshape(-1, 3) for d in dir_sets]
        raw = self.scheme.ops.dft_farfield(terms, torch.cat(sets), torch.tensor(self.wavenumbers, dtype=torch.float64))
        vec = torch.view_as_complex(raw.cpu().contiguous()) * (self.dx * self.dx * 2.0 / max(1, self.samples))
        return list(torch.split(vec, [int(d.shape[0]) for d in sets], dim=1))

    def vectors(self, dirs) -> Optional[torch.Tensor]:
        """(K, A, 6) complex128 on the host: ``N_x, N_y, N_z, L_x, L_y, L_z``
        of the phasors ``(2 / samples)(Re + i Im)`` in the unit directions
        ``dirs`` (A, 3), in A m and V m.  Decomposed runs gather the slabs'
        raw accumulators on rank 0, which runs the same evaluation; the other
        ranks return None."""
        r = self.vectors_many([dirs])
        return None if r is None else r[0]

    def _intensity(self, vec: torch.Tensor, thetas: torch.Tensor, phis: torch.Tensor) -> torch.Tensor:
        T, P = thetas.numel(), phis.numel()
        v = vec.reshape(vec.shape[0], T, P, 6)
        st, ct = torch.sin(thetas).reshape(1, T, 1), torch.cos(thetas).reshape(1, T, 1)
        sp, cp = torch.sin(phis).reshape(1, 1, P), torch.cos(phis).reshape(1, 1, P)

        def sph(x, y, z):
            return x * ct * cp + y * ct * sp - z * st, -x * sp + y * cp

        n_th, n_ph = sph(v[..., 0], v[..., 1], v[..., 2])
        l_th, l_ph = sph(v[..., 3], v[..., 4], v[..., 5])
        kap = torch.tensor(self.wavenumbers, dtype=torch.float64).reshape(-1, 1, 1)
        return kap * kap / (32 * PI * PI * ETA0) * ((l_ph + ETA0 * n_th).abs() ** 2 + (l_th - ETA0 * n_ph).abs() ** 2)

    @staticmethod
    def _angles(thetas, phis):
        return (torch.as_tensor(thetas, dtype=torch.float64).reshape(-1),
                torch.as_tensor(phis, dtype=torch.float64).reshape(-1))

    def intensity(self, thetas, phis) -> Optional[torch.Tensor]:
        """(K, T, P) radiant intensity in W / sr on the grid ``thetas`` x
        ``phis`` (radians; None off rank 0)."""
        th, ph = self._angles(thetas, phis)
        vec = self.vectors(directions(th, ph))
        return None if vec is None else self._intensity(vec, th, ph)

    @staticmethod
    def quadrature(n_theta: int, n_phi: int):
        """(thetas, phis, weights (T,)) of the sphere quadrature: Gauss-
        Legendre nodes in ``cos theta`` x uniform ``phi``; the integral of f
        is ``sum_t w_t sum_p f(t, p)``."""
        x, w = np.polynomial.legendre.leggauss(int(n_theta))
        thetas = torch.from_numpy(np.arccos(x[::-1].copy()))
        weights = torch.from_numpy(w[::-1].copy()) * (2 * PI / int(n_phi))
        return thetas, torch.arange(int(n_phi), dtype=torch.float64) * (2 * PI / int(n_phi)), weights

    def _integrate(self, u: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
        return (u.sum(dim=2) * weights.reshape(1, -1)).sum(dim=1)

    def total_power(self, n_theta: int = 16, n_phi: int = 32) -> Optional[torch.Tensor]:
        """(K,) watts: ``U`` integrated over the sphere on its own quadrature
        (:meth:`quadrature`), whatever grid is reported."""
        th, ph, w = self.quadrature(n_theta, n_phi)
        u = self.intensity(th, ph)
        return None if u is None else self._integrate(u, w)

    def directivity(self, thetas, phis) -> Optional[torch.Tensor]:
        """(K, T, P) ``4 pi U / total_power``."""
        r = self.evaluate(thetas, phis)
        return None if r is None else r["directivity"]

    def rcs(self, thetas, phis) -> Optional[torch.Tensor]:
        """(K, T, P) bistatic radar cross-section ``4 pi U / incident`` in
        m^2; TF/SF runs only."""
        if self.label != "scattered":
            raise FdtdError("FarFieldMonitor.rcs: TF/SF runs only")
        u = self.intensity(thetas, phis)
        return None if u is None else 4 * PI * u / self.incident().reshape(-1, 1, 1)

    def evaluate(self, thetas, phis, n_theta: int = 16, n_phi: int = 32) -> Optional[Dict[str, object]]:
        """Everything on the grid ``thetas`` x ``phis`` from ONE evaluation of
        the radiation vectors: ``U``, ``total_power``, ``directivity`` and,
        with TF/SF, ``incident``, ``rcs`` and the ``forward`` / ``backscatter``
        RCS along / against the incidence direction (None off rank 0)."""
        th, ph = self._angles(thetas, phis)
        qt, qp, qw = self.quadrature(n_theta, n_phi)
        sets = [directions(th, ph), directions(qt, qp)]
        if self.label == "scattered":
            lay = self.scheme.layout
            khat = directions([lay.theta], [lay.phi])
            sets.append(torch.cat([khat, -khat]))
        vec = self.vectors_many(sets)
        if vec is None:
            return None
        u = self._intensity(vec[0], th, ph)
        total = self._integrate(self._intensity(vec[1], qt, qp), qw)
        out = {"thetas": th, "phis": ph, "U": u, "total_power": total, "label": self.label,
               "directivity": 4 * PI * u / total.reshape(-1, 1, 1)}
        if self.label == "scattered":
            inc = self.incident()
            # the two directions as 1 x 1 grids of their own angles
            fwd = self._intensity(vec[2][:, :1], *self._angles([lay.theta], [lay.phi]))
            back = self._intensity(vec[2][:, 1:], *self._angles([PI - lay.theta], [lay.phi + PI]))
            out.update(incident=inc, rcs=4 * PI * u / inc.reshape(-1, 1, 1),
                       forward=4 * PI * fwd.reshape(-1) / inc, backscatter=4 * PI * back.reshape(-1) / inc)
        return out

    def report(self, t: int, out, thetas=None, phis=None) -> Optional[Dict[str, object]]:
        """One line per wavelength: the total power, the peak ``U`` and its
        direction, the peak directivity and, with TF/SF, the forward and
        backscatter RCS; on the report grid of the configuration unless
        ``thetas`` / ``phis`` are given."""
        if thetas is None or phis is None:
            thetas, phis = report_grid(self.scheme.cfg.farfield_ntheta, self.scheme.cfg.farfield_nphi)
        r = self.evaluate(thetas, phis)
        if r is None:
            return None
        P = r["phis"].numel()
        for k, wl in enumerate(self.wavelengths):
            i = int(torch.argmax(r["U"][k]))
            line = ("=== farfield t=%u, wavelength %.9g: total power %.9g W %s; peak U %.9g W/sr at theta %.6g phi %.6g; "
                    "peak directivity %.9g" % (t, wl, float(r["total_power"][k]), self.label,
                                               float(r["U"][k].reshape(-1)[i]), float(r["thetas"][i // P]),
                                               float(r["phis"][i % P]), float(r["directivity"][k].max())))
            if "rcs" in r:
                line += "; forward RCS %.9g m^2, backscatter RCS %.9g m^2" % (float(r["forward"][k]),
                                                                             float(r["backscatter"][k]))
            out.write(line + "\n")
        return r

    def info(self, result: Optional[Dict[str, object]] = None) -> Optional[Dict[str, object]]:
        """The ``farfield`` object of the driver's ``--json`` line (from
        ``result``, what :meth:`evaluate` or :meth:`report` returned, or
        evaluated now on the configuration's report grid)."""
        if result is None:
            result = self.evaluate(*report_grid(self.scheme.cfg.farfield_ntheta, self.scheme.cfg.farfield_nphi))
        r = result
        if r is None:
            return None
        P = r["phis"].numel()
        peak = [int(torch.argmax(r["U"][k])) for k in range(len(self.wavelengths))]
        rec = {"wavelengths": self.wavelengths, "step": self.step, "start": self.start, "samples": self.samples,
               "label": self.label, "ntheta": int(r["thetas"].numel()), "nphi": int(P),
               "total_power": r["total_power"].tolist(),
               "peak_u": [float(r["U"][k].reshape(-1)[i]) for k, i in enumerate(peak)],
               "peak_theta": [float(r["thetas"][i // P]) for i in peak],
               "peak_phi": [float(r["phis"][i % P]) for i in peak],
               "peak_directivity": [float(r["directivity"][k].max()) for k in range(len(peak))],
               "forward_rcs": r["forward"].tolist() if "forward" in r else None,
               "backscatter_rcs": r["backscatter"].tolist() if "backscatter" in r else None}
        return rec
