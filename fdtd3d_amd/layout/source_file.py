"""Source files: soft and hard dipole sources at chosen cells
(``--source-file``; from Python ``SchemeConfig(sources=[...])``).

A source list replaces the built-in point source.  JSON, standard library
only::

    {"sources": [
      {"component": "Ez", "cell": [20, 20, 12], "kind": "soft", "amplitude": 1.0,
       "waveform": "pulse", "wavelength": 0.02, "width": 30, "delay": 120, "phase": 0},
      {"component": "Ez", "cell": [28, 20, 12], "length": 5, "amplitude": -0.5,
       "waveform": "sine", "phase": 90, "ramp": 40}
     ]}

``cell`` is the global array index of the component's own Yee sample (the
convention of ``--probe-points`` with ``--probe-position node``; ``x, y`` in
2D).  ``length`` (default 1) extends an E entry of a 3D scheme over that many
consecutive cells along the component's own axis: a filament.  ``kind`` is
``soft`` (default: the value is added to the field after the component's
update) or ``hard`` (the field is set to it).  ``amplitude`` is in field units
(V/m, A/m).

The signal is a function of the step index ``tau`` -- ``t`` for an E entry,
``t + 1/2`` for an H entry (the phase convention of the DFT monitors) -- with
``f = c / wavelength`` (default ``--wavelength``):

* ``sine``: ``r(tau) sin(2 pi f dt tau + phase)``, ``r`` a raised-cosine
  turn-on over ``ramp`` steps (default 0: none);
* ``gaussian``: ``exp(-((tau - delay) / width)^2)``;
* ``pulse``: ``exp(-((tau - delay) / width)^2) sin(2 pi f dt (tau - delay) + phase)``
  -- zero-mean, so a soft pulse leaves no static charge behind.

``phase`` is in degrees, ``width`` and ``delay`` default to
``--gaussian-width`` / ``--gaussian-delay``, ``waveform`` to ``--source``.
:func:`signal_value` is the one place a signal is evaluated (host, fp64): both
backends take its values.  Signals equal in all parameters are one signal.
"""

from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

from ..utils.constants import PI, SPEED_OF_LIGHT
from .yee import SCHEME_COMPONENTS, YeeLayout

MAX_SIGNALS = 64       # distinct signals of a list (the kernel's by-value argument, ops/source.py)
MAX_CELLS = 65536      # source cells of a list, filaments expanded

WAVEFORMS = ("sine", "gaussian", "pulse")
KINDS = ("soft", "hard")
_KEYS = {"component", "cell", "length", "kind", "amplitude", "waveform", "wavelength", "width", "delay", "phase",
         "ramp"}
_AXIS = {"x": 0, "y": 1, "z": 2}
_DIMS = {"3d": 3, "tmz": 2, "tez": 2, "1d": 1}


@dataclass(frozen=True)
class Signal:
    waveform: str
    wavelength: float
    width: float
    delay: float
    phase: float  # degrees
    ramp: float   # steps (sine)


@dataclass(frozen=True)
class SourceEntry:
    component: str
    cell: Tuple[int, int, int]
    length: int
    hard: bool
    amplitude: float
    signal: Signal


def signal_value(sig: Signal, tau: float, dt: float) -> float:
    """The signal at step index ``tau`` (E entries: ``t``, H entries: ``t +
    1/2``) of a run with time step ``dt`` seconds, fp64."""
    f = SPEED_OF_LIGHT / sig.wavelength
    ph = math.radians(sig.phase)
    if sig.waveform == "gaussian":
        return math.exp(-((tau - sig.delay) / sig.width) ** 2)
    if sig.waveform == "pulse":
        arg = dt * (tau - sig.delay) * 2 * PI * f
        return math.exp(-((tau - sig.delay) / sig.width) ** 2) * math.sin(arg + ph)
    arg = dt * tau * 2 * PI * f
    v = math.sin(arg + ph)
    if sig.ramp > 0 and tau < sig.ramp:
        v *= 0.5 * (1.0 - math.cos(PI * max(tau, 0.0) / sig.ramp))
    return v


def _number(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError("sources: %s must be a number, got %r" % (what, v))
    v = float(v)
    if not math.isfinite(v):
        raise ValueError("sources: %s must be finite, got %r" % (what, v))
    return v


def _integer(v, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError("sources: %s must be an integer, got %r" % (what, v))
    return int(v)


def parse_sources(items, scheme: str, wavelength: float, width: float, delay: float,
                  waveform: str = "sine") -> List[SourceEntry]:
    """Validated entries of the ``sources`` list ``items`` (dicts of the
    file's keys, or :class:`SourceEntry` objects, which pass through) for a
    ``scheme``; the remaining arguments are the defaults of an entry's
    signal.  ValueError with a message for everything the format refuses."""
    if scheme not in _DIMS or scheme == "1d":
        raise ValueError("sources: 1D schemes take no source list (the 1D line keeps its built-in source)")
    dim = _DIMS[scheme]
    comps = SCHEME_COMPONENTS[scheme]
    if not isinstance(items, (list, tuple)) or not items:
        raise ValueError("sources: \"sources\" must be a non-empty list of entries")
    out = []
    for n, it in enumerate(items):
        if isinstance(it, SourceEntry):
            out.append(it)
            continue
        what = "entry %d" % n
        if not isinstance(it, dict):
            raise ValueError("sources: %s must be an object, got %r" % (what, it))
        unknown = sorted(set(it) - _KEYS)
        if unknown:
            raise ValueError("sources: %s has unknown key(s) %s (known: %s)"
                             % (what, ", ".join(unknown), ", ".join(sorted(_KEYS))))
        comp = it.get("component")
        if comp not in comps:
            raise ValueError("sources: %s: the %s scheme has no component %r (it has %s)"
                             % (what, scheme, comp, ", ".join(comps)))
        cell = it.get("cell")
        if not isinstance(cell, (list, tuple)) or len(cell) != dim:
            raise ValueError("sources: %s: cell must be a list of %d indices on the %s scheme, got %r"
                             % (what, dim, scheme, cell))
        cell = tuple(_integer(v, what + " cell") for v in cell) + (0,) * (3 - dim)
        length = _integer(it.get("length", 1), what + " length")
        if length < 1:
            raise ValueError("sources: %s: length must be >= 1, got %d" % (what, length))
        if length > 1 and (scheme != "3d" or comp[0] != "E"):
            raise ValueError("sources: %s: length applies to E components of 3D schemes (got %s on %s)"
                             % (what, comp, scheme))
        kind = it.get("kind", "soft")
        if kind not in KINDS:
            raise ValueError("sources: %s: kind must be soft or hard, got %r" % (what, kind))
        wf = it.get("waveform", waveform)
        if wf not in WAVEFORMS:
            raise ValueError("sources: %s: unknown waveform %r (known: %s)" % (what, wf, ", ".join(WAVEFORMS)))
        amp = _number(it.get("amplitude", 1.0), what + " amplitude")
        wl = _number(it.get("wavelength", wavelength), what + " wavelength")
        if wl <= 0:
            raise ValueError("sources: %s: wavelength must be > 0, got %g" % (what, wl))
        wd = _number(it.get("width", width), what + " width")
        if wd <= 0:
            raise ValueError("sources: %s: width must be > 0, got %g" % (what, wd))
        dl = _number(it.get("delay", delay), what + " delay")
        ph = _number(it.get("phase", 0.0), what + " phase")
        rp = _number(it.get("ramp", 0.0), what + " ramp")
        if rp < 0:
            raise ValueError("sources: %s: ramp must be >= 0, got %g" % (what, rp))
        # parameters a waveform does not read are dropped: equal signals are one signal
        if wf == "sine":
            sig = Signal(wf, wl, 1.0, 0.0, ph, rp)
        elif wf == "gaussian":
            sig = Signal(wf, 1.0, wd, dl, 0.0, 0.0)
        else:
            sig = Signal(wf, wl, wd, dl, ph, 0.0)
        out.append(SourceEntry(comp, cell, length, kind == "hard", amp, sig))
    return out


def load_source_file(path: str) -> list:
    """The raw ``sources`` list of the JSON file ``path`` (validated by
    :func:`parse_sources` once the scheme is known).  ValueError for a file
    that cannot be read or is not of the format."""
    try:
        with open(path, "r", encoding="utf-8") as f:
            doc = json.load(f)
    except OSError as e:
        raise ValueError("cannot read %s (%s)" % (path, e.strerror or e))
    except ValueError as e:
        raise ValueError("not JSON (%s)" % e)
    if not isinstance(doc, dict):
        raise ValueError("sources: the file must hold an object with a \"sources\" list")
    unknown = sorted(set(doc) - {"sources"})
    if unknown:
        raise ValueError("sources: unknown top-level key(s) %s (known: sources)" % ", ".join(unknown))
    if "sources" not in doc:
        raise ValueError("sources: the file must hold an object with a \"sources\" list")
    if not isinstance(doc["sources"], list) or not doc["sources"]:
        # (an empty list would read as "no source list" further on)
        raise ValueError("sources: \"sources\" must be a non-empty list of entries")
    return doc["sources"]


def refuse_source_config(cfg, checkpoints: bool = False, native: bool = False) -> Optional[str]:
    """Why the configuration cannot run with its source list (None: it can)."""
    if not cfg.sources:
        return None
    if cfg.scheme == "1d":
        return "--source-file: 1D schemes take no source list"
    if cfg.complex_values:
        return "--source-file with --complex-field-values: the listed signals are real"
    if cfg.use_amp_mode:
        return "--source-file with --use-amp-mode: amplitude mode drives its own line source"
    if cfg.use_hip_graph:
        return ("--source-file with --use-hip-graph: a captured graph would replay the signal values of the "
                "captured steps")
    if checkpoints:
        return "--source-file with --checkpoint-dir / --load-from-file: the source list is not part of a checkpoint"
    return None


class SourceList:
    """The validated source list of a configuration: ``entries``, the
    distinct ``signals`` and the expanded ``cells`` -- (component, global
    index, amplitude, signal index, hard) in file order, filaments unrolled.
    Everything the format, the scheme or the grid refuses raises ValueError
    here, before anything is allocated (the one refusal that needs the
    sampled materials -- a cell inside a D/B-chain box -- comes at grid
    set-up: ``YeeScheme._init_source_list``)."""

    def __init__(self, cfg, layout: Optional[YeeLayout] = None):
        why = refuse_source_config(cfg)
        if why:
            raise ValueError(why)
        self.entries = parse_sources(cfg.sources, cfg.scheme, cfg.wavelength, cfg.gaussian_width,
                                     cfg.gaussian_delay, cfg.source)
        if layout is None:
            layout = YeeLayout(cfg.size, cfg.scheme, tuple(cfg.pml_size) if cfg.use_pml else (0, 0, 0),
                               tuple(cfg.tfsf_size), PI / 2, 0.0, PI / 2 if cfg.scheme != "tez" else 0.0,
                               cfg.double_material_precision)
        dim = _DIMS[cfg.scheme]
        size = tuple(cfg.size)
        self.signals: List[Signal] = []
        index: Dict[Signal, int] = {}
        self.cells: List[Tuple[str, Tuple[int, int, int], float, int, bool]] = []
        for n, e in enumerate(self.entries):
            if e.component not in layout.components:
                raise ValueError("sources: entry %d: the %s scheme has no component %r" % (n, cfg.scheme, e.component))
            if e.signal not in index:
                index[e.signal] = len(self.signals)
                self.signals.append(e.signal)
            lo, hi = layout.global_range(e.component)
            axis = _AXIS[e.component[1]]
            for k in range(e.length):
                g = tuple(e.cell[a] + (k if a == axis else 0) for a in range(3))
                for a in range(3):
                    if not lo[a] <= g[a] < hi[a]:
                        raise ValueError("sources: entry %d: cell %s lies outside the range %s..%s on which %s is "
                                         "updated (the border samples are PEC)"
                                         % (n, g[:dim], lo[:dim], tuple(h - 1 for h in hi[:dim]), e.component))
                    p = layout.pml_size[a] if cfg.use_pml and layout.active(a) else 0
                    if p and (g[a] < p or g[a] >= size[a] - p):
                        raise ValueError("sources: entry %d: cell %s lies inside the %d-cell absorbing layer along %s"
                                         % (n, g[:dim], p, "xyz"[a]))
                self.cells.append((e.component, g, e.amplitude, index[e.signal], e.hard))
        if len(self.signals) > MAX_SIGNALS:
            raise ValueError("sources: %d distinct signals, a list holds %d" % (len(self.signals), MAX_SIGNALS))
        if len(self.cells) > MAX_CELLS:
            raise ValueError("sources: %d source cells, a list holds %d" % (len(self.cells), MAX_CELLS))
        count: Dict[Tuple[str, Tuple[int, int, int]], int] = {}
        for c, g, _, _, _ in self.cells:
            count[(c, g)] = count.get((c, g), 0) + 1
        for c, g, _, _, hard in self.cells:
            if hard and count[(c, g)] > 1:
                raise ValueError("sources: a hard entry sets %s at cell %s, which another entry shares"
                                 % (c, g[:dim]))
        self.distinct_cells = len(count)

    # ------------------------------------------------------------------ queries
    def values(self, tau: float, dt: float) -> List[float]:
        """Every signal's value at step index ``tau``."""
        return [signal_value(s, tau, dt) for s in self.signals]

    def bbox(self):
        """Global bounding box of all source cells."""
        lo = tuple(min(g[a] for _, g, _, _, _ in self.cells) for a in range(3))
        hi = tuple(max(g[a] for _, g, _, _, _ in self.cells) + 1 for a in range(3))
        return lo, hi

    def has_sine(self) -> bool:
        return any(s.waveform == "sine" for s in self.signals)

    def info(self) -> dict:
        """The ``sources`` object of the driver's ``--json`` line."""
        hard = sum(1 for e in self.entries if e.hard)
        return {"entries": len(self.entries), "cells": self.distinct_cells, "signals": len(self.signals),
                "soft": len(self.entries) - hard, "hard": hard}
