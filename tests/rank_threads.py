"""Decomposed runs as thread ranks of one process (the GPU tests' ranks on one
device, the CPU tests' on the torch backend): one thread -- on a GPU one
stream -- per rank over the in-process transport, the scheme of
tests/test_parallel_gpu.py.  A helper module like tests/mesh_shapes.py."""

import threading

import torch

from fdtd3d_amd.models.scheme import YeeScheme
from fdtd3d_amd.ops import make_ops
from fdtd3d_amd.parallel.comm import LocalHub
from fdtd3d_amd.parallel.halo import HaloExchanger
from fdtd3d_amd.parallel.topology import ParallelGridCore

MAX_RANKS = 8
DT = {"f32": torch.float32, "f64": torch.float64}


def rank_domains(size, topo, buf, align_z=1):
    """The ranks' domains of ``run_ranks(...)`` with these arguments, without
    running anything (what a test derives its expectations from)."""
    topo = tuple(int(v) for v in topo)
    world = topo[0] * topo[1] * topo[2]
    axes = "".join("xyz"[a] for a in range(3) if topo[a] > 1) or "x"
    core = ParallelGridCore.create(size, world, axes, requested=topo, optimal=False, active_axes=(0, 1, 2))
    assert tuple(core.topology) == topo
    return core, [core.domain(r, buf, align_z=align_z, align_axis=2) for r in range(world)]


def run_ranks(cfg, topo, buf, backend="hip", device="cuda:0", setup=None, collect=None, align_z=1, steps=True,
              timeout=120):
    """``cfg`` on ``topo`` = (px, py, pz) thread ranks with ``buf``-deep
    ghosts.  Per rank: domain, halo exchanger and scheme (``init_scheme``,
    ``init_grids``), ``setup(scheme)`` -- attach the monitors here --,
    ``perform_steps()`` unless ``steps`` is False, ``halo.drain``, then
    ``collect(scheme, what setup returned)``, whose value is the rank's entry
    of the returned list (default: the scheme itself).  Callbacks run on the
    rank's thread and stream, so they may call the monitors' collective
    results.  The first exception of a rank is raised here; a rank that has
    not finished after ``timeout`` seconds is an error."""
    core, doms = rank_domains(cfg.size, topo, buf, align_z)
    world = len(doms)
    assert 1 < world <= MAX_RANKS
    hub = LocalHub(world)
    dtype = DT[cfg.dtype]
    cuda = torch.device(device).type == "cuda"
    out, errors = [None] * world, []

    def rank_body(rank):
        dom = doms[rank]
        halo = HaloExchanger(dom, comm=hub.comm(rank))
        s = YeeScheme(cfg, make_ops(backend, None, device, dtype), dom, halo)
        s.init_scheme()
        s.init_grids()
        state = setup(s) if setup is not None else None
        if steps:
            s.perform_steps()
        halo.drain(s)
        out[rank] = collect(s, state) if collect is not None else s

    def body(rank):
        try:
            if cuda:
                with torch.cuda.stream(torch.cuda.Stream(device=device)):
                    rank_body(rank)
                torch.cuda.synchronize()
            else:
                rank_body(rank)
        except BaseException as e:  # surface thread failures in the test
            errors.append(e)
            hub._barrier.abort()  # the ranks waiting for this one in a reduction fail instead of waiting

    if not cuda:
        torch.set_num_threads(1)
    ths = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=timeout)
    if errors:
        first = [e for e in errors if not isinstance(e, threading.BrokenBarrierError)]
        raise (first or errors)[0]
    assert not any(t.is_alive() for t in ths), "a rank did not finish in %d s" % timeout
    return out
