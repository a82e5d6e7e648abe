"""What the monitors on a closed box share (models/flux.py, models/
farfield.py): the box ``margin`` cells inside the grid borders of a 3D run, the
:class:`~.dft.DftMonitor` with ``h_time="half"`` over the tangential E and H
slabs around its faces -- the slabs and face-centre sampling plans of the NTFF
surface (models/ntff.py ``_faces``, ``_sample_plan``, ``_plan_box``) --, the
running DFT of the source signal, and the placement against the TF/SF box.
"""

from __future__ import annotations

from typing import Optional, Sequence

import torch

from ..ops.dft import FluxOperand, acc_shape, vec_width, z_pad
from ..utils.assertions import FdtdError
from .dft import DftMonitor, SourceDft
from .ntff import ETA0, _faces, _plan_box, ntff_requests

TFSF_MIN_DISTANCE = 2  # cells between a box face and the TF/SF face: the averages must not straddle it


def slab_operand(dft: DftMonitor, scheme, comp: str, plan, gathered: bool) -> Optional[FluxOperand]:
    """The accumulators of (comp, the plan's box) of ``dft`` in the padded
    layout of a serial monitor, with the plan's first sample and averaging
    axes; ``gathered``: collected from the ranks on rank 0 (None elsewhere)."""
    box = _plan_box(plan)
    i = dft.index((comp, box))
    avg = [len(offs) == 2 for _, _, offs in plan]
    if not gathered:
        e = dft.entries.rows[i]
        return FluxOperand(e.acc, (0, 0, e.box[0][2] - z_pad(e.box, vec_width(e.acc.dtype))[0]), avg)
    raw = dft.gather_accumulators(scheme, i)
    if raw is None:
        return None
    v = vec_width(raw.dtype)
    z0 = z_pad(box, v)[0]
    acc = torch.zeros(acc_shape(box, raw.shape[0], v), dtype=raw.dtype, device=raw.device)
    acc[..., box[0][2] - z0:box[1][2] - z0] = raw
    return FluxOperand(acc, (0, 0, box[0][2] - z0), avg)


class SurfaceMonitor:
    """The box ``margin`` cells inside the grid borders at ``wavelengths``;
    ``step`` (0 = automatic, passes between samples stay blocked) and
    ``start`` as for :class:`~.dft.DftMonitor`.  ``dft``: an existing monitor
    over the same slabs (``ntff_requests(size, margin)``, ``h_time="half"``,
    the same wavelengths) that something else samples; None: the monitor
    makes and samples its own.

    A subclass sets ``box_name`` (its box in error messages) and provides
    ``_label`` (from the TF/SF placement) and ``_build_terms``.

    :meth:`incident` divides by ``_n_src``, the source samples :meth:`sample`
    has added; FluxMonitor used to divide by ``dft.samples``.  On its own DFT
    monitor the two are equal whenever ``incident()`` can run: that monitor is
    made here with ``register=False`` and nothing else samples it (one that
    shares it never does), so ``dft.samples`` grows only in ``dft.sample``
    called from :meth:`sample`, under the same ``start`` / ``step`` test, and
    ``_n_src`` grows in the same call; before the first sample both are 0 and
    the divisor is 1.  On a shared DFT monitor (FarFieldMonitor only) the
    divisor was always ``_n_src``: the shared one may hold earlier samples.
    """

    box_name = "box"

    def __init__(self, scheme, margin: Sequence[int], wavelengths: Sequence[float], step: int = 0, start: int = 0,
                 dft: Optional[DftMonitor] = None, register: bool = True):
        cfg = scheme.cfg
        name = type(self).__name__
        if cfg.scheme != "3d":
            raise FdtdError("%s: 3D runs only (got the %s scheme)" % (name, cfg.scheme))
        if scheme.planes != 1 or cfg.complex_values:
            raise FdtdError("%s: real-valued runs only (a complex run already carries the phasor)" % name)
        if cfg.use_amp_mode:
            raise FdtdError("%s: not with amplitude mode" % name)
        size = tuple(cfg.size)
        self.margin = tuple(int(m) for m in margin)
        if any(m < 0 for m in self.margin) or any(size[a] - 2 * self.margin[a] <= 0 for a in range(3)):
            raise FdtdError("%s: the box %s cells inside the grid %s is empty" % (name, self.margin, size))
        self.label = self._label(cfg)
        self.size = size
        self.faces = _faces(size, self.margin)
        self.scheme = scheme
        self.dx = float(scheme.dx)
        requests = ntff_requests(size, self.margin)
        self.shared = dft is not None
        if dft is None:
            dft = DftMonitor(scheme, requests, wavelengths, step, start, "half", register=False)
        elif (dft.requests != requests or dft.h_time != "half"
              or dft.wavelengths != [float(w) for w in wavelengths]):
            raise FdtdError("%s: the shared DFT monitor does not sample this box's slabs at these wavelengths with "
                            "h_time='half'" % name)
        self.dft = dft
        self.wavelengths, self.omegas = dft.wavelengths, dft.omegas
        self.step, self.start = dft.step, dft.start
        self._source = SourceDft(self.omegas)  # running DFT of the source signal
        self._terms = None
        if register:
            scheme.add_periodic(self.step, self.start % self.step, self.sample)

    @property
    def samples(self) -> int:
        return self.dft.samples

    @property
    def _n_src(self) -> int:
        return self._source.n

    def _placement(self, cfg) -> str:
        """``none`` without TF/SF, else ``inside`` or ``outside`` the TF/SF
        box; refuses a box closer than ``TFSF_MIN_DISTANCE`` cells to the
        TF/SF faces or crossing them."""
        if not cfg.use_tfsf:
            return "none"
        name = type(self).__name__
        d = [self.margin[a] - int(cfg.tfsf_size[a]) for a in range(3)]
        if any(abs(v) < TFSF_MIN_DISTANCE for v in d):
            raise FdtdError("%s: the %s (margin %s) lies less than %d cells from the TF/SF faces (margin %s): the "
                            "face-centre averages would straddle the total / scattered boundary"
                            % (name, self.box_name, self.margin, TFSF_MIN_DISTANCE, tuple(cfg.tfsf_size)))
        if all(v > 0 for v in d):
            return "inside"
        if all(v < 0 for v in d):
            return "outside"
        raise FdtdError("%s: the %s (margin %s) crosses the TF/SF box (margin %s)"
                        % (name, self.box_name, self.margin, tuple(cfg.tfsf_size)))

    # ------------------------------------------------------------------ sampling
    def sample(self, scheme, t: int) -> None:
        if t < self.start or (t - self.start) % self.step:
            return
        if not self.shared:
            self.dft.sample(scheme, t)
        self._source.add(scheme, t)

    def incident(self) -> torch.Tensor:
        """(K,) ``|A_src|^2 / (2 eta0)`` in W / m^2, ``A_src`` the phasor of
        the source signal over the monitor's samples: ``1 / (2 eta0)`` for
        the sine source over whole periods, the pulse spectrum for a Gaussian
        source."""
        n = max(1, self._n_src)
        return torch.tensor([((2.0 / n) ** 2) * (re * re + im * im) / (2.0 * ETA0)
                             for re, im in self._source.acc], dtype=torch.float64)

    # --------------------------------------------------------------------- terms
    def _operand(self, comp: str, plan, gathered: bool) -> Optional[FluxOperand]:
        return slab_operand(self.dft, self.scheme, comp, plan, gathered)

    def _current_terms(self):
        """Decomposed runs gather the raw accumulators on rank 0 at every call
        (the sums have moved on; None elsewhere); serial runs build once."""
        halo = self.scheme.halo
        if halo is not None and halo.comm.world > 1:
            return self._build_terms(True)
        if self._terms is None:
            self._terms = self._build_terms(False)
        return self._terms
