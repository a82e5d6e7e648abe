"""Field-energy monitor: the energy of the fields in a box as a time series,
and a stop of the run once it has decayed to a fraction of its peak.

An :class:`EnergyMonitor` watches the box ``margin`` cells inside the grid
borders.  Every ``step`` time steps ONE backend call (``ops.field_sumsq``;
csrc/energy_kernels.hip on the HIP backend: one pass over the fields, fp64
sums, no temporaries) returns the sum of squares of every component of the
scheme over the component's update range (``layout.global_range``) inside the
box and inside this rank's OWNED cells -- ghost cells never count, so a
decomposed run sums exactly the cells of the serial run.  The host applies

    W_E = 1/2 eps0 dx^d sum E^2,    W_H = 1/2 mu0 dx^d sum H^2

(``d`` the dimensionality of the scheme: joules in 3D, per metre in 2D, per
square metre in 1D).

These are VACUUM weights of the state as it stands after step ``t``: E at
time ``(t - 1) dt`` and H half a step later (models/dft.py, "Phase
reference").  The sum is the exact discrete energy only in vacuum: inside a
dielectric it understates the electric energy by the factor eps_r, and it
omits the polarisation energy of dispersive media.  It is the right quantity
for a decay criterion and for watching an absorbing layer work, not a
material-aware energy budget (the material grids are released after
``init_grids``).

Without ``decay_by`` the samples stay on the device in a small preallocated
buffer and are read once, at a report or at the end of the run: the monitor
adds no host synchronisation.  With ``decay_by = r`` (0 < r < 1) every sample
is read to the host, the monitor keeps the running peak of ``W = W_E + W_H``
and asks the scheme to stop (``YeeScheme.request_stop``) when

    peak > 0  and  W <= r * peak  and  t >= t_src,

``t_src`` the first step from which the source signal stays below
``SOURCE_OFF`` of its peak for the rest of the step budget -- a Gaussian
pulse; a sine source never ends and is refused.  A request holds for one
``advance()``: the monitor asks at every sample that meets the criterion, and
``stopped_at`` is the step of the last sample if it did (else None).  The
criterion presumes that
the pulse reaches the box before the source has ended (a TF/SF box inside the
monitored box, or a point source in it).

Like the DFT monitors this is periodic work (``YeeScheme.add_periodic``):
``advance()`` ends a blocked / hybrid pass at every sample step.  The
automatic step is therefore a multiple of the pass length -- or of the step
of a registered DFT / flux monitor, whose samples already end passes -- so
that the monitor cuts no extra passes when its ``start`` shares their offset.
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..ops.dft import box_empty
from ..ops.energy import EnergyEntries
from ..parallel.domain import box_intersect
from ..utils.assertions import FdtdError
from ..utils.constants import EPS0, MU0
from .dft import DftMonitor, pass_length

# Samples at least this many steps apart.  A whole-grid sample reads ~24 B/cell against the 15.28 B/cell-step of the
# blocked vacuum pass (profiles/bench_pmc_r6.md): ~1.6 steps' worth of traffic, ~3 % at one sample per 50 steps.
# Measured cost at this step: profiles/energy.md.
AUTO_MIN_STEP = 50
SOURCE_OFF = 1e-6  # the source has ended once its signal stays below this fraction of its peak


def auto_step(scheme) -> int:
    """The smallest multiple of the run's pass length -- with a DFT or flux
    monitor registered: of its sampling step -- that is at least
    ``AUTO_MIN_STEP`` steps."""
    from .farfield import FarFieldMonitor
    from .flux import FluxMonitor
    base = pass_length(scheme)
    steps = [int(fn.__self__.step) for _, _, fn in scheme.periodic
             if isinstance(getattr(fn, "__self__", None), (DftMonitor, FluxMonitor, FarFieldMonitor))]
    if steps:
        base = 1
        for s in steps:
            base = base * s // math.gcd(base, s)
    return -(-AUTO_MIN_STEP // base) * base


def source_end(scheme, budget: int) -> Optional[int]:
    """``t_src``: the first step from which ``|source_value(t, 0)|`` stays
    below ``SOURCE_OFF`` of its peak up to step ``budget``; None where the
    source is still on at the end of the budget.  With a source list: the
    latest end of all its signals, each against its own peak (None when one
    of them is a sine)."""
    sl = getattr(scheme, "source_list", None)
    if sl is not None:
        from ..layout.source_file import signal_value
        if sl.has_sine():
            return None
        n = max(1, int(budget)) + 1
        end = 0
        for sig in sl.signals:
            # both sample times of a step: E entries take tau = t, H entries t + 1/2
            v = torch.tensor([max(abs(signal_value(sig, t, scheme.dt)), abs(signal_value(sig, t + 0.5, scheme.dt)))
                              for t in range(n)], dtype=torch.float64)
            peak = float(v.max())
            if not peak > 0:
                continue
            last = int(torch.nonzero(v >= SOURCE_OFF * peak).flatten()[-1])
            if last >= n - 1:
                return None
            end = max(end, last + 1)
        return end
    v = scheme.source_values(0, max(1, int(budget)) + 1, 0).abs()
    peak = float(v.max())
    if not peak > 0:
        return 0
    on = torch.nonzero(v >= SOURCE_OFF * peak).flatten()
    last = int(on[-1])
    return None if last >= v.numel() - 1 else last + 1


def refuse_energy_config(cfg, checkpoints: bool = False) -> Optional[str]:
    """Why the configuration cannot run with its energy monitor (None: it
    can); the refusals of models/dft.py ``refuse_config`` apply."""
    from .dft import refuse_config
    if not (cfg.use_energy or cfg.stop_decay_by):
        return None
    why = refuse_config(cfg, checkpoints)
    if why:
        return why
    if not 0.0 <= cfg.stop_decay_by < 1.0:
        return "--stop-decay-by: a fraction of the peak energy, 0 <= r < 1 (got %g)" % cfg.stop_decay_by
    if cfg.stop_decay_by > 0 and getattr(cfg, "sources", None):
        # a source list: every entry must end (layout/source_file.py; a malformed list is refused by its loader)
        from ..layout.source_file import parse_sources
        try:
            entries = parse_sources(cfg.sources, cfg.scheme, cfg.wavelength, cfg.gaussian_width, cfg.gaussian_delay,
                                    cfg.source)
        except ValueError as e:
            return str(e)
        if any(e.signal.waveform == "sine" for e in entries):
            return ("--stop-decay-by with a sine entry in the source list: that source never ends, so the field "
                    "energy never decays; use the pulse or gaussian waveform")
        return None
    if cfg.stop_decay_by > 0 and cfg.source != "gaussian":
        return ("--stop-decay-by with --source %s: the source never ends, so the field energy never decays; use "
                "--source gaussian" % cfg.source)
    return None


def energy_from_config(scheme) -> Optional["EnergyMonitor"]:
    """The monitor ``--use-energy`` / ``--stop-decay-by`` ask for, registered
    with the scheme (after ``init_grids`` and after the DFT / flux monitors,
    whose step the automatic step follows); None without the options."""
    cfg = scheme.cfg
    if not (cfg.use_energy or cfg.stop_decay_by):
        return None
    why = refuse_energy_config(cfg)
    if why:
        raise FdtdError(why)
    return EnergyMonitor(scheme, cfg.energy_size, cfg.energy_step, cfg.energy_start, cfg.stop_decay_by)


class EnergyMonitor:
    """Vacuum-weighted field energy in the box ``margin`` cells inside the
    grid borders ((0, 0, 0): the whole grid), sampled after every step ``t >=
    start`` with ``(t - start) % step == 0`` (``step`` 0 = automatic,
    :func:`auto_step`); ``decay_by`` > 0 stops the run once the energy has
    fallen to that fraction of its peak (module docstring)."""

    def __init__(self, scheme, margin: Sequence[int], step: int = 0, start: int = 0, decay_by: float = 0.0,
                 register: bool = True):
        cfg = scheme.cfg
        if scheme.planes != 1 or cfg.complex_values:
            raise FdtdError("EnergyMonitor: real-valued runs only")
        if cfg.use_amp_mode:
            raise FdtdError("EnergyMonitor: not with amplitude mode")
        decay_by = float(decay_by)
        if not 0.0 <= decay_by < 1.0:
            raise FdtdError("EnergyMonitor: decay_by is a fraction of the peak, 0 <= r < 1 (got %g)" % decay_by)
        size = tuple(cfg.size)
        self.margin = tuple(max(0, int(margin[a])) if size[a] > 1 else 0 for a in range(3))
        self.box = (self.margin, tuple(size[a] - self.margin[a] for a in range(3)))
        if any(int(m) < 0 for m in margin) or box_empty(self.box):
            raise FdtdError("EnergyMonitor: the box %s cells inside the grid %s is empty" % (tuple(margin), size))
        self.scheme = scheme
        self.comps = tuple(scheme.comps)
        self.dim = {"3d": 3, "tmz": 2, "tez": 2, "1d": 1}[cfg.scheme]
        vol = float(scheme.dx) ** self.dim
        self.weights = [0.5 * (EPS0 if c[0] == "E" else MU0) * vol for c in self.comps]
        self.start = max(0, int(start))
        self.step = int(step) if int(step) > 0 else auto_step(scheme)
        self.decay_by = decay_by
        self.t_src: Optional[int] = None
        if decay_by > 0:
            self.t_src = source_end(scheme, cfg.time_steps)
            listed = getattr(scheme, "source_list", None) is not None
            if listed and self.t_src is None:
                raise FdtdError("EnergyMonitor: decay_by needs sources that end within the %d time steps: an entry of "
                                "the source list is a sine or a pulse still on at the last step, so the field energy "
                                "would never decay" % cfg.time_steps)
            if (cfg.source != "gaussian" and not listed) or self.t_src is None:
                raise FdtdError("EnergyMonitor: decay_by needs a source that ends within the %d time steps (--source "
                                "%s does not): the field energy would never decay" % (cfg.time_steps, cfg.source))
        dom = scheme.domain
        self.owned_boxes = []  # global, per component: update range, box and this rank's owned cells
        self.entries = EnergyEntries(len(self.comps))
        for n, c in enumerate(self.comps):
            own = box_intersect(box_intersect(scheme.layout.global_range(c), self.box), dom.owned_global())
            if box_empty(own):
                own = (own[0], own[0])
            self.owned_boxes.append(own)
            self.entries.add(scheme.F[0][c], dom.to_local(own), n)
        self.times: List[int] = []
        self.peak = 0.0
        self.stopped_at: Optional[int] = None
        self._host: List[List[float]] = []  # decay_by: the all-reduced sums of squares per sample
        self._buf: Optional[torch.Tensor] = None  # otherwise: this rank's sums per sample, on the device
        self._series: Optional[List[Tuple[int, float, float]]] = None
        if decay_by <= 0:
            budget = max(0, cfg.time_steps - self.start) // self.step + 2
            self._buf = torch.zeros((budget, len(self.comps)), dtype=torch.float64, device=scheme.device)
        if register:
            scheme.add_periodic(self.step, self.start % self.step, self.sample)

    @property
    def samples(self) -> int:
        return len(self.times)

    # ------------------------------------------------------------------ sampling
    def _reduce(self, rows: List[List[float]]) -> List[List[float]]:
        """Per-rank sums of squares summed over the ranks in fp64."""
        halo = self.scheme.halo
        if halo is None or halo.comm.world == 1 or not rows:
            return rows
        n = len(self.comps)
        flat = halo.allreduce_fsum([v for row in rows for v in row])
        return [flat[i * n:(i + 1) * n] for i in range(len(rows))]

    def _energies(self, sums: Sequence[float]) -> Tuple[float, float]:
        we = sum(w * v for w, v, c in zip(self.weights, sums, self.comps) if c[0] == "E")
        wh = sum(w * v for w, v, c in zip(self.weights, sums, self.comps) if c[0] == "H")
        return we, wh

    def sample(self, scheme, t: int) -> None:
        if t < self.start or (t - self.start) % self.step:
            return
        for e, c in zip(self.entries, self.comps):
            e.field = scheme.F[0][c]  # the current array: F / F_alt ping-pong
        # (decomposed runs: no halo drain -- a pending exchange only writes ghost cells, and only owned cells,
        # final once the step's launches are queued on this stream, are read here)
        sums = scheme.ops.field_sumsq(self.entries)
        k = len(self.times)
        self.times.append(t)
        self._series = None
        if self._buf is not None:
            if k >= self._buf.shape[0]:  # a run beyond the configured budget
                self._buf = torch.cat([self._buf, torch.zeros_like(self._buf)])
            self._buf[k].copy_(sums)
            return
        row = self._reduce([sums.tolist()])[0]
        self._host.append(row)
        w = sum(self._energies(row))
        self.peak = max(self.peak, w)
        stop = self.peak > 0 and w <= self.decay_by * self.peak and t >= self.t_src
        halo = scheme.halo
        if halo is not None and halo.comm.world > 1:
            # Rank 0 decides and its decision is broadcast (a max-reduce to which only rank 0 contributes its
            # flag): every rank stops at the same step whatever bits the transport's float sum delivered to each.
            stop = halo.allreduce_max(1.0 if (stop and halo.comm.rank == 0) else 0.0) > 0
        self.stopped_at = None
        if stop:
            # asked at every sample that meets the criterion: a caller that steps on after a stop (the request
            # holds for one advance() only) is stopped again at the next sample, and stopped_at follows
            self.stopped_at = t
            scheme.request_stop("field energy %.3g of its peak" % (w / self.peak))

    # ------------------------------------------------------------------- results
    def series(self) -> List[Tuple[int, float, float]]:
        """``[(t, W_E, W_H)]`` of every sample so far, summed over the ranks
        (every rank calls it; each gets the whole series).  Without
        ``decay_by`` this reads the device buffer."""
        if self._series is None:
            self._series = [(t,) + self._energies(row) for t, row in zip(self.times, self._rows())]
        return self._series

    def _rows(self) -> List[List[float]]:
        if self._buf is None:
            return self._host
        return self._reduce(self._buf[:len(self.times)].cpu().tolist())

    def sums(self) -> List[Tuple[int, Dict[str, float]]]:
        """``[(t, {component: sum of squares})]`` of every sample, unweighted
        and summed over the ranks (every rank calls it)."""
        return [(t, dict(zip(self.comps, row))) for t, row in zip(self.times, self._rows())]

    def result(self) -> Dict[str, object]:
        """The series with its peak, last value and their ratio."""
        ser = self.series()
        tot = [we + wh for _, we, wh in ser]
        peak = max(tot) if tot else 0.0
        last = tot[-1] if tot else 0.0
        return {"series": ser, "samples": len(ser), "peak": peak, "last": last,
                "ratio": last / peak if peak > 0 else 0.0, "stopped_at": self.stopped_at}

    def report_sample(self, out) -> None:
        """One ``=== energy`` line for the last sample alone (the driver's
        ``--log-level 1``; every rank calls it): without ``decay_by`` it
        reads that one row of the device buffer, not the series so far."""
        if not self.times:
            return
        if self._buf is None:
            row = self._host[-1]
        else:
            row = self._reduce([self._buf[len(self.times) - 1].tolist()])[0]
        we, wh = self._energies(row)
        out.write("=== energy t=%u: W_E %.9g, W_H %.9g, W %.9g (vacuum weights)\n" % (self.times[-1], we, wh, we + wh))

    def report(self, t: int, out) -> Dict[str, object]:
        """One line: the energies of the last sample and their fraction of
        the peak."""
        r = self.result()
        if r["series"]:
            ts, we, wh = r["series"][-1]
            out.write("=== energy t=%u: W_E %.9g, W_H %.9g, W %.9g (vacuum weights), %.6g of the peak %.9g\n"
                      % (ts, we, wh, we + wh, r["ratio"], r["peak"]))
        else:
            out.write("=== energy t=%u: no samples\n" % t)
        return r

    def info(self, result: Optional[Dict[str, object]] = None) -> Dict[str, object]:
        """The ``energy`` object of the driver's ``--json`` line (from
        ``result``, what :meth:`result` or :meth:`report` returned, or
        evaluated now)."""
        r = result if result is not None else self.result()
        return {"step": self.step, "start": self.start, "samples": r["samples"], "peak": r["peak"], "last": r["last"],
                "ratio": r["ratio"], "stopped_at": r["stopped_at"], "series": [list(s) for s in r["series"]]}
