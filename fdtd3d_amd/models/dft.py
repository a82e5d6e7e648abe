"""Running-DFT field monitors: frequency-domain results from a real-valued
run at blocked-kernel speed.

A :class:`DftMonitor` keeps, per monitored field sample and frequency, two
accumulators ``Re += f cos(w t)`` and ``Im += f sin(w t)``, updated every
``step`` time steps by ONE backend launch over all its boxes
(``ops.dft_accumulate``; csrc/dft_kernels.hip on the HIP backend).  It is
periodic work in the sense of :meth:`YeeScheme.add_periodic`: ``advance()``
ends a blocked / hybrid pass at every sampling step and the passes in between
stay blocked.  With the project's ``exp(-i w t)`` convention a steady field
``Re(A exp(-i w t)) = Re(A) cos(w t) + Im(A) sin(w t)`` sampled over whole
periods gives ``(2 / N) (Re + i Im) = A`` (:meth:`DftMonitor.phasor`).

Phase reference (sample times).  ``YeeScheme.step`` with ``scheme.t == n``
updates E, sets the hard source to ``source_value(n) = sin(2 pi f n dt)``,
then updates H from that E, and only then increments ``scheme.t``.  Periodic
work fired "after step t" sees ``scheme.t == t`` (``t = n + 1``), so

* E components are samples at time ``(t - 1) dt`` -- the time the source
  assigns them;
* H components, advanced from E in the same step, are half a step LATER:
  ``(t - 1/2) dt``.

``h_time="half"`` (default) uses these times, so E and H phasors refer to the
same time origin.  ``h_time="same"`` gives H the E time -- what the NTFF of a
``--complex-field-values`` run implicitly does when it pairs the E and H
planes of one step.  The blocked and hybrid passes compute the same leapfrog
sequence, so the times hold for them too.

Decomposed runs: every box is clipped to the rank's owned box, accumulators
are rank-local and need no ghosts; a rank that owns nothing of a box keeps an
empty entry (and takes part in every exchange as before).
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from ..ops.dft import DFT_MAX_K, KIND_E, KIND_H, DftEntries, box_empty
from ..parallel.domain import box_intersect
from ..utils.assertions import FdtdError
from ..utils.constants import PI, SPEED_OF_LIGHT

Box = Tuple[Tuple[int, int, int], Tuple[int, int, int]]
Request = Tuple[str, Box]

MIN_SAMPLES_PER_PERIOD = 8  # automatic step: samples per shortest monitored period


def pass_length(scheme) -> int:
    """Steps of one blocked (``scheme.tb``) or hybrid (``T``) pass."""
    hyb = getattr(scheme, "hybrid", None)
    if hyb is not None:
        return int(hyb["T"])
    return max(1, int(getattr(scheme, "tb", 1)))


def auto_step(scheme, wavelengths: Sequence[float]) -> int:
    """The largest multiple of the run's pass length that still takes
    ``MIN_SAMPLES_PER_PERIOD`` samples per shortest monitored period (the
    passes between samples then keep their full length); where even one pass
    is too long for that, the sampling bound wins: the largest such step, at
    least 1."""
    period = min(wavelengths) / (SPEED_OF_LIGHT * scheme.dt)  # steps
    most = int(math.floor(period / MIN_SAMPLES_PER_PERIOD + 1e-9))
    L = pass_length(scheme)
    if most >= L:
        return (most // L) * L
    return max(1, most)


def parse_wavelengths(text: str, default: float) -> List[float]:
    """``--dft-wavelengths``: comma-separated metres; empty = ``default``."""
    vals = [float(v) for v in text.split(",") if v.strip()] if text.strip() else [float(default)]
    if not 1 <= len(vals) <= DFT_MAX_K or any(not (v > 0) for v in vals):
        raise FdtdError("--dft-wavelengths: 1 to %d positive wavelengths" % DFT_MAX_K)
    return vals


def monitor_box_requests(scheme, margin: Sequence[int]) -> List[Request]:
    """Every component of the scheme on the box ``margin`` cells inside the
    grid borders (0: the whole grid; axes the scheme does not have: whole)."""
    size = scheme.cfg.size
    m = [max(0, int(margin[a])) if size[a] > 1 else 0 for a in range(3)]
    box = (tuple(m), tuple(size[a] - m[a] for a in range(3)))
    if box_empty(box):
        raise FdtdError("--dft-size*: the monitor box %s is empty on the grid %s" % (box, tuple(size)))
    return [(c, box) for c in scheme.comps]


def refuse_config(cfg, checkpoints: bool = False) -> Optional[str]:
    """Why the configuration cannot run with its DFT monitors (None: it can).
    Never a silent fallback."""
    energy = cfg.use_energy or cfg.stop_decay_by > 0
    if not (cfg.use_dft or cfg.ntff_dft or cfg.use_flux or cfg.use_farfield or energy):
        return None
    flag = "--use-dft" if cfg.use_dft else "--ntff-dft" if cfg.ntff_dft else ""
    if cfg.use_flux:
        flag = flag + " / --use-flux" if flag else "--use-flux"
    if cfg.use_farfield:
        flag = flag + " / --use-farfield" if flag else "--use-farfield"
    if energy and not flag:
        # the energy monitor alone (models/energy.py): the same refusals in its own words
        flag = "--stop-decay-by" if cfg.stop_decay_by > 0 and not cfg.use_energy else "--use-energy"
        if cfg.complex_values:
            return "%s with --complex-field-values: the energy monitor needs a real-valued run" % flag
        if cfg.use_amp_mode:
            return "%s with --use-amp-mode: the energy monitor does not follow the amplitude steps" % flag
        if checkpoints:
            return ("%s with --checkpoint-dir / --load-from-file: the energy series and its peak are not part of a "
                    "checkpoint" % flag)
        return None
    if energy:
        flag += " / --use-energy"
    if cfg.complex_values:
        return ("%s with --complex-field-values: a complex run already carries the phasor; the monitor needs a "
                "real-valued run" % flag)
    if cfg.use_amp_mode:
        return "%s with --use-amp-mode: the monitor replaces amplitude mode (it yields |F| and the phase)" % flag
    if checkpoints:
        return ("%s with --checkpoint-dir / --load-from-file: the DFT accumulators are not part of a checkpoint"
                % flag)
    if cfg.ntff_dft and not (cfg.use_ntff and cfg.scheme == "3d"):
        return "--ntff-dft needs --use-ntff on a 3D run"
    if cfg.use_flux and cfg.scheme != "3d":
        return "--use-flux needs a 3D run"
    if cfg.use_farfield and cfg.scheme != "3d":
        return "--use-farfield needs a 3D run"
    return None


def monitors_from_config(scheme) -> Dict[str, "DftMonitor"]:
    """The monitors the scheme's configuration asks for, registered with the
    scheme (after ``init_grids``): ``"box"`` (``use_dft``: every component on
    the ``dft_size`` box at ``dft_wavelengths``) and ``"ntff"`` (``ntff_dft``:
    the ``ntff_requests`` slabs at the source wavelength)."""
    cfg = scheme.cfg
    why = refuse_config(cfg)
    if why:
        raise FdtdError(why)
    out: Dict[str, DftMonitor] = {}
    if cfg.use_dft:
        wl = parse_wavelengths(cfg.dft_wavelengths, scheme.wavelength)
        out["box"] = DftMonitor(scheme, monitor_box_requests(scheme, cfg.dft_size), wl, cfg.dft_step, cfg.dft_start,
                                cfg.dft_h_time)
    if cfg.ntff_dft:
        from .ntff import ntff_requests
        out["ntff"] = DftMonitor(scheme, ntff_requests(cfg.size, cfg.ntff_size), [scheme.wavelength], cfg.dft_step,
                                 cfg.dft_start, cfg.dft_h_time)
    return out


class SourceDft:
    """Running DFT of the source signal at the angular frequencies ``omegas``
    over a monitor's samples: what a spectrum is divided by to be one of the
    system and not of the pulse (models/surface.py ``incident``, models/
    probe.py ``spectrum``).  Host floats, one ``add`` per sample."""

    def __init__(self, omegas: Sequence[float]):
        self.omegas = [float(w) for w in omegas]
        self.acc = [[0.0, 0.0] for _ in self.omegas]
        self.n = 0

    def add(self, scheme, t: int) -> None:
        """The sample after step ``t``: the value the source gave E in that
        step, ``source_value(t - 1)``, at the E sample time ``(t - 1) dt``."""
        te = (t - 1) * scheme.dt
        v = scheme.source_value(t - 1, 0)
        for acc, w in zip(self.acc, self.omegas):
            acc[0] += v * math.cos(w * te)
            acc[1] += v * math.sin(w * te)
        self.n += 1

    def phasors(self) -> List[complex]:
        """``(2 / N) (Re + i Im)`` per frequency (:meth:`DftMonitor.phasor`'s
        convention)."""
        scale = 2.0 / max(1, self.n)
        return [complex(re * scale, im * scale) for re, im in self.acc]


class DftMonitor:
    """Running DFT of ``requests`` = [(component, global index box)] at
    ``wavelengths`` (free-space, metres), sampled after every step ``t >=
    start`` with ``(t - start) % step == 0``."""

    def __init__(self, scheme, requests: Sequence[Request], wavelengths: Sequence[float], step: int = 0,
                 start: int = 0, h_time: str = "half", register: bool = True):
        if h_time not in ("half", "same"):
            raise FdtdError("DftMonitor: h_time is 'half' or 'same'")
        if scheme.planes != 1:
            raise FdtdError("DftMonitor: real-valued runs only (a complex run already carries the phasor)")
        self.wavelengths = [float(w) for w in wavelengths]
        if not 1 <= len(self.wavelengths) <= DFT_MAX_K:
            raise FdtdError("DftMonitor: 1 to %d wavelengths" % DFT_MAX_K)
        self.omegas = [2 * PI * SPEED_OF_LIGHT / w for w in self.wavelengths]
        self.h_time = h_time
        self.start = max(0, int(start))
        self.step = int(step) if int(step) > 0 else auto_step(scheme, self.wavelengths)
        self.samples = 0
        self.requests: List[Request] = []
        self.owned_boxes: List[Box] = []   # global, clipped to the rank
        self.entries = DftEntries(len(self.wavelengths))
        dom = scheme.domain
        size = tuple(scheme.cfg.size)
        for comp, box in requests:
            if comp not in scheme.comps:
                raise FdtdError("DftMonitor: the %s scheme has no component %s" % (scheme.cfg.scheme, comp))
            box = (tuple(int(v) for v in box[0]), tuple(int(v) for v in box[1]))
            if any(box[0][a] < 0 or box[1][a] > size[a] for a in range(3)):
                raise FdtdError("DftMonitor: box %s outside the grid %s" % (box, size))
            own = box_intersect(box, dom.owned_global())
            if box_empty(own):
                own = (own[0], own[0])
            self.requests.append((comp, box))
            self.owned_boxes.append(own)
            self.entries.add(scheme.F[0][comp], dom.to_local(own), KIND_E if comp[0] == "E" else KIND_H)
        if register:
            scheme.add_periodic(self.step, self.start % self.step, self.sample)

    # ------------------------------------------------------------------ sampling
    def sample_times(self, scheme, t: int) -> Tuple[float, float]:
        """(E time, H time) of the fields after step ``t`` (module docstring)."""
        te = (t - 1) * scheme.dt
        return te, te + (0.5 * scheme.dt if self.h_time == "half" else 0.0)

    def twiddles(self, scheme, t: int):
        """``[kind][k] = (cos w_k t_kind, sin w_k t_kind)`` in fp64."""
        times = self.sample_times(scheme, t)
        return [[(math.cos(w * tk), math.sin(w * tk)) for w in self.omegas] for tk in times]

    def sample(self, scheme, t: int) -> None:
        if t < self.start or (t - self.start) % self.step:
            return
        for e, (comp, _) in zip(self.entries, self.requests):
            e.field = scheme.F[0][comp]  # the current array: F / F_alt ping-pong
        scheme.ops.dft_accumulate(self.entries, self.twiddles(scheme, t))
        self.samples += 1

    # ------------------------------------------------------------------- results
    def index(self, key: Union[int, str, Request]) -> int:
        """A request by position, by (component, box), or by component name
        when only one request monitors it."""
        if isinstance(key, int):
            return key
        if isinstance(key, str):
            hits = [i for i, (c, _) in enumerate(self.requests) if c == key]
            if len(hits) != 1:
                raise KeyError("%d monitored boxes of %s" % (len(hits), key))
            return hits[0]
        key = (key[0], (tuple(key[1][0]), tuple(key[1][1])))
        return self.requests.index(key)

    def accumulators(self, key) -> torch.Tensor:
        """(K, 2, bx, by, bz) raw sums over the owned part of the box."""
        return self.entries.rows[self.index(key)].owned()

    def phasor(self, key, k: int = 0) -> torch.Tensor:
        """``(2 / N) (Re + i Im)`` of wavelength ``k`` as a complex tensor
        over the owned part of the box: ``A`` of a steady ``Re(A exp(-i w
        t))`` sampled over whole periods."""
        acc = self.accumulators(key)
        scale = 2.0 / max(1, self.samples)
        return torch.complex(acc[k, 0] * scale, acc[k, 1] * scale)

    def gather(self, scheme, key, k: int = 0, dst: int = 0, group=None) -> Optional[torch.Tensor]:
        """The phasor over the whole requested box on rank ``dst`` (None
        elsewhere); serial runs: :meth:`phasor`."""
        import torch.distributed as dist
        i = self.index(key)
        mine = self.phasor(i, k)
        if scheme.halo is None or not dist.is_initialized() or dist.get_world_size(group) == 1:
            return mine
        from ..parallel.topology import ParallelGridCore
        d = scheme.domain
        lo, hi = self.requests[i][1]
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        core = ParallelGridCore(tuple(d.global_size), world, tuple(d.topology))
        if rank == dst:
            out = torch.zeros(tuple(hi[a] - lo[a] for a in range(3)), dtype=mine.dtype, device=mine.device)
            for r in range(core.used_procs):
                dr = core.domain(r, d.buffer_size)
                pp = box_intersect((lo, hi), (dr.lo, dr.hi))
                if box_empty(pp):
                    continue
                if r == rank:
                    blk = mine
                else:
                    buf = torch.empty(tuple(pp[1][a] - pp[0][a] for a in range(3)) + (2,), dtype=mine.real.dtype,
                                      device=mine.device)
                    dist.recv(buf, r, group=group, tag=202)
                    blk = torch.view_as_complex(buf)
                out[tuple(slice(pp[0][a] - lo[a], pp[1][a] - lo[a]) for a in range(3))] = blk
            return out
        if rank < core.used_procs and mine.numel():
            dist.send(torch.view_as_real(mine).contiguous(), dst, group=group, tag=202)
        return None

    def gather_accumulators(self, scheme, key, dst: int = 0) -> Optional[torch.Tensor]:
        """The raw sums ``(K, 2, bx, by, bz)`` over the whole requested box on
        rank ``dst`` (None elsewhere), through the halo exchanger's transport;
        serial runs: :meth:`accumulators`.  Every rank calls it for the same
        keys in the same order.  What products of phasors are computed from
        (models/flux.py): the sums travel unscaled and in the run's
        precision."""
        i = self.index(key)
        mine = self.accumulators(i)
        comm = scheme.halo.comm if scheme.halo is not None else None
        if comm is None or comm.world == 1:
            return mine
        from ..parallel.comm import P2P
        from ..parallel.topology import ParallelGridCore
        d = scheme.domain
        lo, hi = self.requests[i][1]
        core = ParallelGridCore(tuple(d.global_size), comm.world, tuple(d.topology))
        head = tuple(mine.shape[:2])
        if comm.rank == dst:
            out = torch.zeros(head + tuple(hi[a] - lo[a] for a in range(3)), dtype=mine.dtype, device=mine.device)
            for r in range(core.used_procs):
                dr = core.domain(r, d.buffer_size)
                pp = box_intersect((lo, hi), (dr.lo, dr.hi))
                if box_empty(pp):
                    continue
                if r == comm.rank:
                    blk = mine
                else:
                    blk = torch.empty(head + tuple(pp[1][a] - pp[0][a] for a in range(3)), dtype=mine.dtype,
                                      device=mine.device)
                    for w in comm.post([P2P(False, blk, r, 203)]):
                        w.wait()
                out[(slice(None), slice(None)) + tuple(slice(pp[0][a] - lo[a], pp[1][a] - lo[a])
                                                       for a in range(3))] = blk
            return out
        if comm.rank < core.used_procs and mine.numel():
            for w in comm.post([P2P(True, mine.contiguous(), dst, 203)]):
                w.wait()
        return None

    def info(self) -> Dict[str, object]:
        """The ``dft`` object of the driver's ``--json`` line."""
        return {"wavelengths": self.wavelengths, "step": self.step, "start": self.start, "samples": self.samples,
                "h_time": self.h_time}
