"""Field probes: the fields at chosen points as time series, and the spectra
one pulsed run carries there.

A :class:`ProbeMonitor` records, every ``step`` time steps, the Yee samples of
its points' components in ONE backend call (``ops.probe_sample``; csrc/
probe_kernels.hip on the HIP backend: one launch over a device table, the
sample number passed by value).  The samples stay on the device in a buffer
sized for the run and are read once, by :meth:`ProbeMonitor.series`: sampling
never synchronises the host.

Points are global cell indices.  ``position="node"`` records, per point and
component, that component's own Yee sample at the index -- an exact copy of one
array element, at the component's staggered position (layout/yee.py
``MIN_COORD_FP``).  ``position="centre"`` gives every component at the centre
of the cell: the mean of its 1, 2 or 4 samples around it, the offsets derived
from the staggering as models/ntff.py ``_sample_plan`` derives them for faces.
The buffer holds RAW samples, one slot each, never means: the mean is formed on
read, in fp64 -- the slots added left to right in slot order (x outermost, z
innermost), then one multiplication by 1 / count -- so that a decomposed run,
whose ranks each record the slots whose cell they own and send them to rank 0,
forms it on the same path as a serial run and returns the same bits (the
reason decomposed flux monitors gather raw accumulators).

Sample times follow models/dft.py ("Phase reference"): after step ``t`` the E
components are samples at ``(t - 1) dt`` and the H components half a step
later.  :meth:`ProbeMonitor.spectrum` is a host-side fp64 DFT of the series at
those times, at any number of wavelengths, in :meth:`~.dft.DftMonitor.phasor`'s
convention ``(2 / N) (Re + i Im)``; ``normalise=True`` divides by the source
signal's phasor over the same samples (:class:`~.dft.SourceDft`).

Like the other monitors this is periodic work (``YeeScheme.add_periodic``):
``advance()`` ends a blocked / hybrid pass at every sample step.  The automatic
step is the pass length -- with a DFT, flux, far-field or energy monitor
registered: the least common multiple of their steps -- so the probes cut no
pass that was not cut already.  Samples inside a pass do not exist.
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..layout.yee import MIN_COORD_FP
from ..ops.probe import ProbeEntries
from ..utils.assertions import FdtdError
from ..utils.constants import PI, SPEED_OF_LIGHT
from .dft import DftMonitor, SourceDft, pass_length

Point = Tuple[int, int, int]

DIMS = {"3d": 3, "tmz": 2, "tez": 2, "1d": 1}
GATHER_TAG = 204  # the series blocks sent to rank 0


def auto_step(scheme) -> int:
    """The run's pass length; with DFT, flux, far-field or energy monitors
    registered the least common multiple of their sampling steps, whose
    samples already end passes."""
    from .energy import EnergyMonitor
    from .surface import SurfaceMonitor
    steps = [int(fn.__self__.step) for _, _, fn in scheme.periodic
             if isinstance(getattr(fn, "__self__", None), (DftMonitor, SurfaceMonitor, EnergyMonitor))]
    if not steps:
        return pass_length(scheme)
    base = 1
    for s in steps:
        base = base * s // math.gcd(base, s)
    return base


def sample_indices(layout, comp: str, point: Sequence[int], position: str) -> List[Point]:
    """Global indices of the Yee samples of ``comp`` a probe at cell ``point``
    reads, in slot order (x outermost): the index itself for ``node``; for
    ``centre`` the samples around the cell centre ``point + 1/2`` -- along an
    axis where the component sits at half-integer positions (``MIN_COORD_FP``
    0.5) the one at the index, where it sits at integer positions (1.0) the
    two at ``index - 1`` and ``index``.  Axes the scheme does not have keep
    index 0."""
    m = MIN_COORD_FP[comp]
    per_axis = []
    for a in range(3):
        if not layout.active(a):
            per_axis.append([0])
        elif position == "node":
            per_axis.append([int(point[a])])
        else:
            first = point[a] + 0.5 - m[a]
            base = int(math.floor(first))
            per_axis.append([base] if first == base else [base, base + 1])
    return [(i, j, k) for i in per_axis[0] for j in per_axis[1] for k in per_axis[2]]


def parse_points(text: str, dim: int, what: str = "--probe-points") -> List[Tuple[int, ...]]:
    """``x,y,z;x,y,z;...`` (``dim`` indices a point; blanks separate as well
    as commas)."""
    pts = []
    for part in text.split(";"):
        toks = part.replace(",", " ").split()
        if not toks:
            continue
        try:
            vals = tuple(int(v) for v in toks)
        except ValueError:
            raise FdtdError("%s: integer cell indices, got %r" % (what, part.strip()))
        if len(vals) != dim:
            raise FdtdError("%s: %d indices a point on this scheme, got %r" % (what, dim, part.strip()))
        pts.append(vals)
    return pts


def read_points(path: str, dim: int) -> List[Tuple[int, ...]]:
    """``--probe-file``: one point per line, ``#`` starts a comment."""
    try:
        with open(path, "r", encoding="utf-8") as f:
            lines = [ln.split("#", 1)[0] for ln in f]
    except OSError as e:
        raise FdtdError("--probe-file: cannot read %s (%s)" % (path, e.strerror))
    return parse_points(";".join(lines), dim, "--probe-file")


def band_wavelengths(n: int, band: str) -> List[float]:
    """``--probe-spectrum n`` over ``--probe-band lo,hi``: ``n`` free-space
    wavelengths evenly spaced in frequency from ``c / hi`` up to ``c / lo``
    (one: the middle frequency)."""
    try:
        lo, hi = (float(v) for v in band.split(","))
    except ValueError:
        raise FdtdError("--probe-band: two wavelengths lo,hi in metres, got %r" % band)
    if not 0 < lo <= hi or n < 1:
        raise FdtdError("--probe-spectrum / --probe-band: n >= 1 wavelengths over 0 < lo <= hi (got %d, %r)"
                        % (n, band))
    f0, f1 = SPEED_OF_LIGHT / hi, SPEED_OF_LIGHT / lo
    if n == 1:
        return [SPEED_OF_LIGHT / (0.5 * (f0 + f1))]
    return [SPEED_OF_LIGHT / (f0 + j * (f1 - f0) / (n - 1)) for j in range(n)]


def refuse_probe_config(cfg, checkpoints: bool = False) -> Optional[str]:
    """Why the configuration cannot run with its probes (None: it can).
    Never a silent fallback."""
    if not cfg.use_probes:
        return None
    if cfg.complex_values:
        return ("--use-probes with --complex-field-values: a complex run already carries the phasor; the probes need "
                "a real-valued run")
    if cfg.use_amp_mode:
        return "--use-probes with --use-amp-mode: the probes do not follow the amplitude steps"
    if checkpoints:
        return "--use-probes with --checkpoint-dir / --load-from-file: the probe series is not part of a checkpoint"
    if cfg.probe_position not in ("node", "centre"):
        return "--probe-position must be node or centre"
    if not (cfg.probe_points.strip() or cfg.probe_file):
        return "--use-probes needs points: --probe-points \"x,y,z;...\" or --probe-file"
    if cfg.probe_spectrum < 0 or (cfg.probe_spectrum > 0 and not cfg.probe_band.strip()):
        return "--probe-spectrum n needs n >= 1 and --probe-band lo,hi (metres)"
    return None


def probes_from_config(scheme, checkpoints: bool = False) -> Optional["ProbeMonitor"]:
    """The monitor ``--use-probes`` asks for, registered with the scheme
    (after ``init_grids`` and after the other monitors, whose step the
    automatic step follows); None without the option."""
    cfg = scheme.cfg
    if not cfg.use_probes:
        return None
    why = refuse_probe_config(cfg, checkpoints)
    if why:
        raise FdtdError(why)
    dim = DIMS[cfg.scheme]
    points = parse_points(cfg.probe_points, dim)
    if cfg.probe_file:
        points += read_points(cfg.probe_file, dim)
    comps = [c.strip() for c in cfg.probe_components.split(",") if c.strip()] or None
    if cfg.probe_spectrum > 0:
        band_wavelengths(cfg.probe_spectrum, cfg.probe_band)  # refused before the run, not after it
    return ProbeMonitor(scheme, points, comps, cfg.probe_position, cfg.probe_step, cfg.probe_start)


class ProbeMonitor:
    """The ``components`` (default: all of the scheme's) at the ``points``
    (global cell indices: (x, y, z) in 3D, (x, y) in 2D, (x,) in 1D) taken
    at ``position`` (``node`` / ``centre``, module docstring), sampled after
    every step ``t >= start`` with ``(t - start) % step == 0`` (``step`` 0 =
    automatic, :func:`auto_step`)."""

    def __init__(self, scheme, points: Sequence[Sequence[int]], components: Optional[Sequence[str]] = None,
                 position: str = "node", step: int = 0, start: int = 0, register: bool = True):
        cfg = scheme.cfg
        if scheme.planes != 1 or cfg.complex_values:
            raise FdtdError("ProbeMonitor: real-valued runs only (a complex run already carries the phasor)")
        if cfg.use_amp_mode:
            raise FdtdError("ProbeMonitor: not with amplitude mode")
        if position not in ("node", "centre"):
            raise FdtdError("ProbeMonitor: position is 'node' or 'centre'")
        self.comps = tuple(scheme.comps if components is None else components)
        for c in self.comps:
            if c not in scheme.comps:
                raise FdtdError("ProbeMonitor: the %s scheme has no component %s" % (cfg.scheme, c))
        if not self.comps or len(set(self.comps)) != len(self.comps):
            raise FdtdError("ProbeMonitor: at least one component, each once (got %s)" % (self.comps,))
        dim = DIMS[cfg.scheme]
        size = tuple(cfg.size)
        self.points: List[Point] = []
        for p in points:
            p = tuple(int(v) for v in p)
            if len(p) != dim:
                raise FdtdError("ProbeMonitor: %d indices a point on the %s scheme, got %s" % (dim, cfg.scheme, p))
            p = p + (0,) * (3 - dim)
            if any(not 0 <= p[a] < size[a] for a in range(3)):
                raise FdtdError("ProbeMonitor: point %s outside the grid %s" % (p[:dim], size[:dim]))
            self.points.append(p)
        if not self.points:
            raise FdtdError("ProbeMonitor: at least one point")
        self.position = position
        self.scheme = scheme
        self.start = max(0, int(start))
        self.step = int(step) if int(step) > 0 else auto_step(scheme)
        # every slot of the run, in the order of the points, components and samples: (component, global index);
        # groups[point][component] = the slots whose mean (one slot: whose copy) is the value
        self.slots: List[Tuple[str, Point]] = []
        self.groups: List[List[List[int]]] = []
        for p in self.points:
            per_comp = []
            for c in self.comps:
                idx = sample_indices(scheme.layout, c, p, position)
                for g in idx:
                    if any(not 0 <= g[a] < size[a] for a in range(3)):
                        raise FdtdError("ProbeMonitor: the %s samples around the centre of cell %s reach outside the "
                                        "grid %s (sample %s)" % (c, p[:dim], size[:dim], g[:dim]))
                per_comp.append(list(range(len(self.slots), len(self.slots) + len(idx))))
                self.slots += [(c, g) for g in idx]
            self.groups.append(per_comp)
        # this rank records the slots whose cell it owns (ghost copies never count)
        dom = scheme.domain
        capacity = -(-max(0, cfg.time_steps - self.start) // self.step) + 1
        self.entries = ProbeEntries(capacity, scheme.device)
        for c in self.comps:  # array n of the entries = component n
            self.entries.add_field(scheme.F[0][c])
        shape = tuple(dom.shape)
        self.mine: List[int] = []
        for s, (c, g) in enumerate(self.slots):
            if not dom.owns(g):
                continue
            li = dom.local_index(g)
            self.entries.add(self.comps.index(c), (li[0] * shape[1] + li[1]) * shape[2] + li[2])
            self.mine.append(s)
        self.steps: List[int] = []  # the step of every sample
        if register:
            scheme.add_periodic(self.step, self.start % self.step, self.sample)

    @property
    def samples(self) -> int:
        return len(self.steps)

    # ------------------------------------------------------------------ sampling
    def sample(self, scheme, t: int) -> None:
        if t < self.start or (t - self.start) % self.step:
            return
        for i, c in enumerate(self.comps):
            self.entries.fields[i] = scheme.F[0][c]  # the current array: F / F_alt ping-pong
        # (decomposed runs: no halo drain -- a pending exchange only writes ghost cells, and only owned cells,
        # final once the step's launches are queued on this stream, are read here)
        k = len(self.steps)
        if k >= self.entries.capacity:  # a run beyond the configured budget
            self.entries.grow()
        scheme.ops.probe_sample(self.entries, k)
        self.steps.append(t)

    # ------------------------------------------------------------------- results
    def times(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(E sample times, H sample times) of every sample so far, fp64
        seconds (:meth:`~.dft.DftMonitor.sample_times`: E at the time the
        source assigns it, H half a step later)."""
        dt = self.scheme.dt
        te = [(t - 1) * dt for t in self.steps]
        return (torch.tensor(te, dtype=torch.float64), torch.tensor([v + 0.5 * dt for v in te], dtype=torch.float64))

    def raw(self) -> Optional[torch.Tensor]:
        """(samples, slots) fp64 on the host: every slot of the run, the
        ranks' columns collected on rank 0 through the halo exchanger's
        transport (None on the other ranks; every rank calls it)."""
        n = len(self.steps)
        mine = self.entries.series[:n]
        comm = self.scheme.halo.comm if self.scheme.halo is not None else None
        if comm is None or comm.world == 1:
            return mine.cpu()
        from ..parallel.comm import P2P
        from ..parallel.topology import ParallelGridCore
        d = self.scheme.domain
        core = ParallelGridCore(tuple(d.global_size), comm.world, tuple(d.topology))
        if comm.rank == 0:
            out = torch.zeros((n, len(self.slots)), dtype=torch.float64)
            for r in range(core.used_procs):
                dr = core.domain(r, d.buffer_size)
                cols = [s for s, (_, g) in enumerate(self.slots) if dr.owns(g)]
                if not cols or n == 0:
                    continue
                if r == comm.rank:
                    blk = mine
                else:
                    blk = torch.empty((n, len(cols)), dtype=torch.float64, device=mine.device)
                    for w in comm.post([P2P(False, blk, r, GATHER_TAG)]):
                        w.wait()
                out[:, cols] = blk.cpu()
            return out
        if comm.rank < core.used_procs and self.mine and n:
            for w in comm.post([P2P(True, mine.contiguous(), 0, GATHER_TAG)]):
                w.wait()
        return None

    def series(self) -> Optional[torch.Tensor]:
        """(samples, points, components) fp64 on the host (decomposed runs:
        on rank 0, None elsewhere; every rank calls it).  ``node``: the
        recorded elements themselves; ``centre``: the means of their slots,
        added left to right in slot order, times 1 / count."""
        raw = self.raw()
        if raw is None:
            return None
        out = torch.empty((raw.shape[0], len(self.points), len(self.comps)), dtype=torch.float64)
        for p, per_comp in enumerate(self.groups):
            for c, cols in enumerate(per_comp):
                acc = raw[:, cols[0]]
                for s in cols[1:]:
                    acc = acc + raw[:, s]
                out[:, p, c] = acc if len(cols) == 1 else acc * (1.0 / len(cols))
        return out

    def spectrum(self, wavelengths: Sequence[float], normalise: bool = False,
                 series: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """(K, points, components) complex128: the phasors ``(2 / N) (Re + i
        Im)`` of the series at the free-space ``wavelengths`` (metres, any
        number), ``Re = sum f cos(w t)``, ``Im = sum f sin(w t)`` over the N
        samples at their own times, in fp64 on the host.  ``normalise``:
        divided by the source signal's phasor over the same samples.
        ``series``: what :meth:`series` returned (it is read otherwise;
        None on the ranks that hold none)."""
        ser = self.series() if series is None else series
        if ser is None:
            return None
        omegas = [2 * PI * SPEED_OF_LIGHT / float(w) for w in wavelengths]
        if any(not (float(w) > 0) for w in wavelengths):
            raise FdtdError("ProbeMonitor: positive wavelengths")
        n = len(self.steps)
        times = [t.tolist() for t in self.times()]
        kind = [0 if c[0] == "E" else 1 for c in self.comps]
        out = torch.zeros((len(omegas), len(self.points), len(self.comps)), dtype=torch.complex128)
        scale = 2.0 / max(1, n)
        for k, w in enumerate(omegas):
            tw = [torch.tensor([[math.cos(w * t), math.sin(w * t)] for t in tk], dtype=torch.float64).reshape(n, 2)
                  for tk in times]
            for c, kd in enumerate(kind):
                re = (ser[:, :, c] * tw[kd][:, 0:1]).sum(0)
                im = (ser[:, :, c] * tw[kd][:, 1:2]).sum(0)
                out[k, :, c] = torch.complex(re * scale, im * scale)
        if normalise:
            src = SourceDft(omegas)
            for t in self.steps:
                src.add(self.scheme, t)
            for k, a in enumerate(src.phasors()):
                if a == 0:
                    raise FdtdError("ProbeMonitor: the source signal has no content at wavelength %g over the %d "
                                    "samples" % (wavelengths[k], n))
                out[k] /= a
        return out

    def info(self, spectrum: Optional[torch.Tensor] = None, wavelengths: Sequence[float] = (),
             normalised: bool = False) -> Dict[str, object]:
        """The ``probes`` object of the driver's ``--json`` line; with a
        ``spectrum`` (what :meth:`spectrum` returned for ``wavelengths``) its
        real and imaginary parts as [wavelength][point][component]."""
        dim = DIMS[self.scheme.cfg.scheme]
        rec = {"points": [list(p[:dim]) for p in self.points], "components": list(self.comps),
               "position": self.position, "step": self.step, "start": self.start, "samples": self.samples}
        if spectrum is not None:
            rec["spectrum"] = {"wavelengths": [float(w) for w in wavelengths], "normalised": bool(normalised),
                               "re": spectrum.real.tolist(), "im": spectrum.imag.tolist()}
        return rec
