"""Poynting-flux monitor: time-averaged power through a closed box, per
wavelength, from the phasors of a running-DFT monitor.

A :class:`FluxMonitor` is a :class:`~.surface.SurfaceMonitor`: it watches the
box ``margin`` cells inside the grid borders of a 3D run and owns a
:class:`~.dft.DftMonitor` over the tangential E and H slabs around the six
faces with ``h_time="half"``, so E and H phasors share one time origin, which
their product needs.  Through a face with normal axis ``a``,
``(b, c)`` the cyclic successors of ``a``,

    P = sign dx^2 1/2 (2/N)^2 sum over the face cells of
        [Re E_b Re H_c + Im E_b Im H_c] - [Re E_c Re H_b + Im E_c Im H_b]

(``1/2 Re(E x H*) . n`` with the phasors ``(2/N)(Re + i Im)``, ``N`` samples),
each operand the face-centre average of its 1, 2 or 4 raw accumulator
samples.  The backend op ``ops.dft_flux`` evaluates the sums in fp64 from the
raw accumulators, fp32 runs included: the net flux of a lossless scatterer is
a small difference of large face sums.

Normalisation: :meth:`FluxMonitor.incident` is the intensity ``|A|^2 / (2
eta0)`` of the source signal at every wavelength, from a host-side running DFT
of ``source_value`` at the monitor's own sample steps and E times.  With
TF/SF, :meth:`FluxMonitor.cross_section` ``= net / incident`` is the
scattering (box outside the TF/SF box) or absorption (inside) cross-section
in m^2 -- a sine source over whole periods and a Gaussian pulse take the same
path.

The sampling window must cover whole periods of a steady state (sine source:
``start`` after the transient, ``samples * step`` a multiple of every
monitored period) or the whole pulse (Gaussian source: from before the pulse
until the fields have left the box); otherwise the phasors, and so the
power, carry the truncation.
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from ..ops.dft import FluxTerm, FluxTerms
from ..utils.assertions import FdtdError
from .dft import parse_wavelengths
from .ntff import _sample_plan
from .surface import TFSF_MIN_DISTANCE, SurfaceMonitor, slab_operand  # noqa: F401 (both importable from here)


def flux_from_config(scheme) -> Optional["FluxMonitor"]:
    """The monitor ``--use-flux`` asks for, registered with the scheme (after
    ``init_grids``); None without the option."""
    cfg = scheme.cfg
    if not cfg.use_flux:
        return None
    from .dft import refuse_config
    why = refuse_config(cfg)
    if why:
        raise FdtdError(why)
    return FluxMonitor(scheme, cfg.flux_size, parse_wavelengths(cfg.dft_wavelengths, scheme.wavelength),
                       cfg.dft_step, cfg.dft_start)


class FluxMonitor(SurfaceMonitor):
    """Power through the box ``margin`` cells inside the grid borders at
    ``wavelengths``; ``step`` (0 = automatic, passes between samples stay
    blocked) and ``start`` as for :class:`~.dft.DftMonitor`.  The window must
    cover whole periods of a steady state, or the whole pulse (module
    docstring)."""

    box_name = "flux box"

    def __init__(self, scheme, margin: Sequence[int], wavelengths: Sequence[float], step: int = 0, start: int = 0,
                 register: bool = True):
        super().__init__(scheme, margin, wavelengths, step, start, None, register)

    def _label(self, cfg) -> str:
        """``radiated`` without TF/SF, else ``scattered`` (box outside the
        TF/SF box) or ``absorbed`` (inside)."""
        return {"none": "radiated", "inside": "absorbed", "outside": "scattered"}[self._placement(cfg)]

    # ------------------------------------------------------------------- results
    def _build_terms(self, gathered: bool) -> Optional[FluxTerms]:
        terms = FluxTerms(len(self.wavelengths), len(self.faces))
        missing = False
        for f, (axis, x0, sign, lo, hi) in enumerate(self.faces):
            b, c = (axis + 1) % 3, (axis + 2) % 3
            for ea, ha, s in ((b, c, 1), (c, b, -1)):  # E_b H_c - E_c H_b
                pe = _sample_plan("E" + "xyz"[ea], axis, x0, lo, hi)
                ph = _sample_plan("H" + "xyz"[ha], axis, x0, lo, hi)
                oe = self._operand("E" + "xyz"[ea], pe, gathered)
                oh = self._operand("H" + "xyz"[ha], ph, gathered)
                if oe is None or oh is None:
                    missing = True
                    continue
                terms.add(FluxTerm(f, int(sign) * s, [n for _, n, _ in pe], oe, oh))
        return None if missing else terms

    def power(self) -> Optional[torch.Tensor]:
        """(6, K) float64 on the host, watts: the power through each face in
        the order of ``_faces`` (-x, +x, -y, +y, -z, +z), outward positive.
        Decomposed runs gather the slabs' raw accumulators on rank 0, which
        runs the same evaluation; the other ranks return None."""
        terms = self._current_terms()
        if terms is None:
            return None
        raw = self.scheme.ops.dft_flux(terms)
        n = max(1, self.samples)
        return raw.cpu() * (self.dx * self.dx * 0.5 * (2.0 / n) ** 2)

    def net(self) -> Optional[torch.Tensor]:
        """(K,) net outward power in watts (None off rank 0)."""
        p = self.power()
        return None if p is None else p.sum(dim=0)

    def cross_section(self) -> Optional[torch.Tensor]:
        """(K,) m^2: scattered (box outside the TF/SF box) or absorbed (box
        inside, ``-net``) power over the incident intensity; TF/SF runs only."""
        if self.label == "radiated":
            raise FdtdError("FluxMonitor.cross_section: TF/SF runs only")
        p = self.net()
        if p is None:
            return None
        return (-p if self.label == "absorbed" else p) / self.incident()

    def result(self) -> Optional[Dict[str, object]]:
        """Per-face power, the net, the labelled power (``-net`` when
        absorbed) and, with TF/SF, the cross-section (None off rank 0)."""
        p = self.power()
        if p is None:
            return None
        net = p.sum(dim=0)
        out = {"power": p, "net": net, "label": self.label, self.label: -net if self.label == "absorbed" else net}
        if self.label != "radiated":
            out["cross_section"] = out[self.label] / self.incident()
        return out

    def report(self, t: int, out) -> Optional[Dict[str, object]]:
        """One line per wavelength: the six face powers, the net, the label
        and, with TF/SF, the cross-section."""
        r = self.result()
        if r is None:
            return None
        for k, wl in enumerate(self.wavelengths):
            line = "=== flux t=%u, wavelength %.9g: faces %s; net %.9g W %s" % (
                t, wl, " ".join("%.9g" % v for v in r["power"][:, k].tolist()), float(r["net"][k]), self.label)
            if "cross_section" in r:
                line += "; cross-section %.9g m^2" % float(r["cross_section"][k])
            out.write(line + "\n")
        return r

    def info(self, result: Optional[Dict[str, object]] = None) -> Optional[Dict[str, object]]:
        """The ``flux`` object of the driver's ``--json`` line (from ``result``,
        what :meth:`result` or :meth:`report` returned, or evaluated now)."""
        r = result if result is not None else self.result()
        if r is None:
            return None
        return {"wavelengths": self.wavelengths, "step": self.step, "start": self.start, "samples": self.samples,
                "label": self.label, "net": r["net"].tolist(),
                "cross_section": r["cross_section"].tolist() if "cross_section" in r else None}
