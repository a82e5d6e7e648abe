// native_multi.h -- --parallel-grid decompositions (x / y / z rank grids) driven from one process:
// the rank grid, the ghost exchange, the blocked passes of plain media and the amplitude loop over
// the ranks.  The stepped path (configuration, split half step on each rank's StepView, run loop,
// report lines, DAT / BMP writer, state list) is native_step.h, shared with the one-GPU run.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "capi.h"
#include "host_native.h"
#include "settings_native.h"
#include "native_api.h"
#include "native_setup.h"
#include "native_ckpt.h"
#include "native_lowdim.h"
#include "native_step.h"

// Part of the native driver: included by main.cpp only (one translation unit),
// hence the unnamed namespace.
namespace {

// ------------------------------------------------------------ multi-GPU
// --parallel-grid: the 3D grid split over a Px x Py x Pz rank grid
// (--topology-sizex/y/z; none given: one x slab per visible GPU), every rank
// driven by this one process (rank r on device r % devices).  Every T steps
// each rank runs the temporally blocked kernel over its owned cells, reading
// T-deep ghosts (the pass's dependency cone); then it packs, for each of its
// up to 26 face / edge / corner neighbours, the owned T-deep box that
// neighbour holds as ghosts (one kernel, six components); at the next pass
// each rank pulls its neighbours' packed boxes (xGMI peer copies between
// devices) and unpacks them into its ghosts on a side stream while its main
// stream runs the interior (cells that need no fresh ghost), then the
// T-thick shells -- the direct 26-neighbour exchange of parallel/halo.py
// overlapped as models/blocking.py _tb_step does, point-to-point only, the
// shape of the node's xGMI links.  Plain Yee
// media (vacuum / dielectric sphere) with the point source; the reference's
// MPI grid: Source/Grid/ParallelGrid.cpp:1600-1823 (exchange), :2161-2194.
//
// Physics (CPML absorbing layers, TF/SF plane waves, point source, vacuum or
// the dielectric sphere): every rank steps its owned cells with the split
// half step of native_step.h -- the one-GPU stepped path's launches on the
// rank's StepView (the folded 4-cell-lane CPML kernels, the chain regions,
// the TF/SF correction tables, the incident line) -- and the
// updated kind's three components go to the face neighbours after every half
// step -- one-cell ghosts in x / y, 4-cell ghosts in z (whole lanes), the
// reference's buffer-size-1 exchange (ParallelGrid.cpp:1600-1823 after each
// of performExSteps / performHxSteps, Scheme3D.cpp:1900-2942).  The CPML
// profiles, psi slabs and TF/SF targets are built per rank from the global
// positions (native_setup.h setup_cpml / setup_tfsf with the rank's origin),
// so no psi ever needs a ghost: ghosts are read, never updated.
template <typename T>
struct XRank {
  int dev = 0;
  hipStream_t st = nullptr, side = nullptr;  // passes / ghost pulls
  hipEvent_t done = nullptr, copied = nullptr;
  std::vector<std::array<int, 6>> outs;      // output boxes of a pass: interior, then the shells
  int crd[3] = {0, 0, 0};
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // owned global range
  int g0[3] = {0, 0, 0}, n[3] = {0, 0, 0};   // allocated box (ghosts included): global origin, extent
  Dev<T> F[6], G[6], C[6];
  int boxes[36];
  // per direction d (0..26, 13 = self): the owned box sent to the neighbour
  // at d and the ghost box received from it (local indices), its buffers
  int nb[27];
  int sbox[27][6], rbox[27][6];
  Dev<T> sbuf[27], rbuf[27];
  // physics: the owned part of every component's update range (local
  // indices), the rank's CPML tables, TF/SF tables and incident line, the
  // point source's local offset (-1: not owned)
  int own36[36];
  std::unique_ptr<NativeCpml<T>> cp;
  std::unique_ptr<NativeTfsf<T>> tf;
  // UPML / Drude: the rank's chain tables and region-local D levels, its part
  // of the global chain and plain regions (local indices)
  std::unique_ptr<native_phys::Upml<T>> up;
  // 2D: the CPML slabs / UPML strips tables and the half-step helper
  std::unique_ptr<Pml2d<T>> p2;
  std::unique_ptr<Lowdim2d<T>> ld;
  std::vector<IBox> chain_regs, plain_regs;
  std::vector<bool> chain_disp;
  long long src_off = -1;
  StepView<T> view;  // what the rank's split half steps launch on (native_step.h)
  // amplitude mode: running maxima ([x][6][y][z]), changed counts of a
  // check period, the amplitude boxes (local), the z-line cells it owns,
  // the near-convergence snapshot
  Dev<T> AMP;
  Dev<unsigned> CNT;
  Dev<long long> LINE;
  int line_n = 0;
  int ab[36];
  Dev<char> SNAP;
  size_t cells() const { return (size_t)n[0] * n[1] * n[2]; }
};

template <typename T>
class MultiRun {
 public:
  explicit MultiRun(const fdtd::Settings& s_) : s(s_), cfg(s_) {}
  ~MultiRun() { release(); }
  int main();

 private:
  // the shared run loop (native_step.h) drives advance / sync / ntff_fields / save_checkpoint
  template <typename R>
  friend void run_steps(R&, int, int);
  template <typename R>
  friend void run_ckpt(R&, int, int);

  const fdtd::Settings& s;
  RunConfig cfg;
  bool phys = false;  // the split half steps (native_step.h) rather than blocked passes
  bool amp_on = false, amp_line = false;  // the amplitude phase is running; the global z line exists
  int amp_taken = 0, amp_stable = -1;
  Dev<T> NG[6];  // NTFF: the whole grid assembled on the first rank's device
  double ckpt_ms = 0.0;
  int ndev = 0, P = 1, TB = 1;
  int Pd[3] = {1, 1, 1};
  int gd[3] = {1, 1, 1};  // ghost depth per axis
  std::vector<XRank<T>> R;
  bool first = true;

  int rank_of(const int* c) const { return (c[0] * Pd[1] + c[1]) * Pd[2] + c[2]; }
  int plan_ranks();
  void setup_rank(int r);
  void enable_peers();
  void plan_outputs();
  void pull_ghosts();
  void rank_pass(XRank<T>& q, int t, int k);
  void pass(int t, int k);
  bool setup_physics(int r);
  void setup_chain(XRank<T>& q);
  void exchange(int kind);
  void phys_step(int t);
  void setup_amp(XRank<T>& q);
  std::vector<std::pair<void*, size_t>> rank_state(XRank<T>& q);
  int amp_run(int t);
  void advance(int t0, int n);
  void gather(int c, std::vector<T>& host);
  void scatter(int c, const std::vector<T>& host);
  void sync();
  std::array<T*, 6> ntff_fields();
  bool save_checkpoint(int t);
  void report(double sec, int t_end, int steps, int warm) const;
  bool save_results(int steps);
  void release();
};

// the rank grid (--topology-sizex/y/z, else one x slab per GPU), the steps
// per pass and every rank's owned / allocated box; 2 when the grid does not
// split that way
template <typename T>
int MultiRun<T>::plan_ranks() {
  HIP_OK(hipGetDeviceCount(&ndev));
  Pd[0] = std::max(1, s.topologySizeX);
  Pd[1] = std::max(1, s.topologySizeY);
  Pd[1] = cfg.dim >= 2 ? Pd[1] : 1;
  Pd[2] = cfg.dim == 3 ? std::max(1, s.topologySizeZ) : 1;
  if (Pd[0] * Pd[1] * Pd[2] == 1) Pd[0] = ndev;
  P = Pd[0] * Pd[1] * Pd[2];
  phys = cfg.cpml || cfg.upml || cfg.tfsf || cfg.amp || cfg.dim < 3;  // (1D / 2D: the split half steps always)
  const int T_max = sizeof(T) == 4 ? fdtd_tb_max_steps() : fdtd_tb64_max_steps();
  TB = phys ? 1 : std::max(1, std::min(T_max, s.timeBlock <= 0 ? (sizeof(T) == 4 ? 5 : 4) : s.timeBlock));
  for (int a = 0; a < 3; ++a) gd[a] = TB;
  if (phys) gd[2] = Pd[2] > 1 ? 4 : 1;  // z ghosts of whole 4-cell lanes
  for (int a = 0; a < 3; ++a)
    if (cfg.N[a] / Pd[a] < gd[a]) {
      std::fprintf(stderr, "fdtd3d (native): %d cells along axis %d over %d ranks leave fewer than %d per rank\n",
                   cfg.N[a], a, Pd[a], gd[a]);
      return 2;
    }
  R.resize(P);
  for (int r = 0; r < P; ++r) {
    XRank<T>& q = R[r];
    q.crd[0] = r / (Pd[1] * Pd[2]);
    q.crd[1] = (r / Pd[2]) % Pd[1];
    q.crd[2] = r % Pd[2];
    for (int a = 0; a < 3; ++a) {
      // near-equal split, the remainder on the first ranks
      const int base = cfg.N[a] / Pd[a], rem = cfg.N[a] % Pd[a], c = q.crd[a];
      q.lo[a] = c * base + std::min(c, rem);
      q.hi[a] = q.lo[a] + base + (c < rem ? 1 : 0);
      const int gl = c > 0 ? gd[a] : 0, gh = c < Pd[a] - 1 ? gd[a] : 0;
      q.g0[a] = q.lo[a] - gl;
      q.n[a] = q.hi[a] - q.lo[a] + gl + gh;
    }
    if (cfg.dim == 3 && (sizeof(T) == 4 || cfg.cpml) && q.n[2] % 4 != 0) {
      std::fprintf(stderr, "fdtd3d (native): fp32 / CPML parallel grids need every rank's z extent (ghosts "
                           "included) %% 4 == 0 (4-cell rows): rank %d has %d\n", r, q.n[2]);
      return 2;
    }
  }
  return 0;
}

// one rank on device r % devices: streams, fields, update boxes, the 26
// message boxes and buffers, per-cell coefficients
template <typename T>
void MultiRun<T>::setup_rank(int r) {
  XRank<T>& q = R[r];
  q.dev = r % ndev;
  HIP_OK(hipSetDevice(q.dev));
  HIP_OK(hipStreamCreate(&q.st));
  HIP_OK(hipStreamCreate(&q.side));
  HIP_OK(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
  HIP_OK(hipEventCreateWithFlags(&q.copied, hipEventDisableTiming));
  const size_t n = q.cells();
  for (int c = 0; c < 6; ++c) {
    q.F[c].alloc(n);
    q.G[c].alloc(n);
  }
  // update boxes in local indices: the global range of each component
  // clipped to the rank's allocated box
  for (int c = 0; c < 6; ++c) {
    fdtd::Int3 glo, ghi;
    fdtd::global_range(c, cfg.N, cfg.active, glo, ghi);
    for (int a = 0; a < 3; ++a) {
      q.boxes[6 * c + a] = std::max(glo[a], q.g0[a]) - q.g0[a];
      q.boxes[6 * c + 3 + a] = std::min(ghi[a], q.g0[a] + q.n[a]) - q.g0[a];
    }
  }
  // messages: direction d = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)
  for (int d = 0; d < 27; ++d) {
    const int off[3] = {d / 9 - 1, (d / 3) % 3 - 1, d % 3 - 1};
    int c[3];
    bool ok = d != 13;
    for (int a = 0; a < 3; ++a) {
      c[a] = q.crd[a] + off[a];
      ok = ok && c[a] >= 0 && c[a] < Pd[a];
    }
    // (physics: the face neighbours only -- the split half steps read no
    // diagonal ghost)
    if (phys) ok = ok && std::abs(off[0]) + std::abs(off[1]) + std::abs(off[2]) == 1;
    q.nb[d] = ok ? rank_of(c) : -1;
    if (!ok) continue;
    size_t vol = phys ? 3 : 6;
    for (int a = 0; a < 3; ++a) {
      // send: the owned layers next to the neighbour; receive: the ghosts there
      int slo = q.lo[a], shi = q.hi[a], rlo = q.lo[a], rhi = q.hi[a];
      if (off[a] < 0) {
        shi = q.lo[a] + gd[a];
        rlo = q.lo[a] - gd[a];
        rhi = q.lo[a];
      } else if (off[a] > 0) {
        slo = q.hi[a] - gd[a];
        rlo = q.hi[a];
        rhi = q.hi[a] + gd[a];
      }
      q.sbox[d][a] = slo - q.g0[a];
      q.sbox[d][3 + a] = shi - q.g0[a];
      q.rbox[d][a] = rlo - q.g0[a];
      q.rbox[d][3 + a] = rhi - q.g0[a];
      vol *= (size_t)(shi - slo);
    }
    q.sbuf[d].alloc(vol);
    q.rbuf[d].alloc(vol);
  }
  if (cfg.percell) {
    // per-cell E coefficients of the dielectric sphere (2-point eps
    // averages, as the single-rank path; 2D: the cylinder's section at the
    // centre's z), H on the scalar db (2D: db arrays, the 2D kernels take one
    // coefficient form per launch)
    const double ctr[3] = {s.sphereCenterX, s.sphereCenterY, s.sphereCenterZ};
    std::vector<T> host(n);
    for (int c = 0; c < 3; ++c) {
      const int di = c == 0, dj = c == 1, dk = c == 2 && cfg.dim == 3;
      for (int li = 0; li < q.n[0]; ++li)
        for (int lj = 0; lj < q.n[1]; ++lj)
          for (int lk = 0; lk < q.n[2]; ++lk) {
            const int i = q.g0[0] + li, j = q.g0[1] + lj, k = q.g0[2] + lk;
            const double z0 = cfg.dim == 3 ? k + 0.5 : ctr[2], z1 = cfg.dim == 3 ? k + dk + 0.5 : ctr[2];
            const double a = sphere_eps(i + 0.5, j + 0.5, z0, ctr, s.sphereRadius, s.sphereEps);
            const double b = sphere_eps(i + di + 0.5, j + dj + 0.5, z1, ctr, s.sphereRadius, s.sphereEps);
            host[((size_t)li * q.n[1] + lj) * q.n[2] + lk] = (T)(cfg.cb * 2.0 / (a + b));
          }
      q.C[c].alloc(n);
      HIP_OK(hipMemcpy(q.C[c].p, host.data(), n * sizeof(T), hipMemcpyHostToDevice));
    }
    if (cfg.dim < 3) {
      std::fill(host.begin(), host.end(), (T)cfg.db);
      for (int c = 3; c < 6; ++c) {
        q.C[c].alloc(n);
        HIP_OK(hipMemcpy(q.C[c].p, host.data(), n * sizeof(T), hipMemcpyHostToDevice));
      }
    }
  }
}

// peer access between the devices of neighbouring ranks (xGMI)
template <typename T>
void MultiRun<T>::enable_peers() {
  for (int r = 0; r < P; ++r)
    for (int d = 0; d < 27; ++d) {
      const int o = R[r].nb[d];
      if (o < 0 || R[o].dev == R[r].dev) continue;
      int ok = 0;
      HIP_OK(hipDeviceCanAccessPeer(&ok, R[r].dev, R[o].dev));
      if (ok) {
        HIP_OK(hipSetDevice(R[r].dev));
        const hipError_t e = hipDeviceEnablePeerAccess(R[o].dev, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_OK(e);
      }
    }
  (void)hipGetLastError();
}

// output boxes of a pass (local indices): the interior (owned cells at
// least TB from every neighbour: needs no fresh ghost) first, then the
// TB-thick shell slabs peeled off axis by axis (models/blocking.py _tb_regions)
template <typename T>
void MultiRun<T>::plan_outputs() {
  for (XRank<T>& q : R) {
    int lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
      lo[a] = q.lo[a] - q.g0[a];
      hi[a] = q.hi[a] - q.g0[a];
    }
    std::vector<std::array<int, 6>> sh;
    for (int a = 0; a < 3; ++a)
      for (int side = 0; side < 2; ++side) {
        if ((side == 0 ? q.crd[a] == 0 : q.crd[a] == Pd[a] - 1)) continue;
        std::array<int, 6> b = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
        if (side == 0) {
          b[3 + a] = lo[a] + TB;
          lo[a] += TB;
        } else {
          b[a] = hi[a] - TB;
          hi[a] -= TB;
        }
        sh.push_back(b);
      }
    q.outs.push_back({lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]});
    for (const auto& b : sh) q.outs.push_back(b);
  }
}

// Phase 1 of a pass, every rank on its side stream: pull the neighbours'
// packs of the previous pass (after their `done` and its own, which orders
// the ghost writes after the passes that read them) and unpack them into the
// ghosts
template <typename T>
void MultiRun<T>::pull_ghosts() {
  for (int r = 0; r < P; ++r) {
    XRank<T>& q = R[r];
    HIP_OK(hipSetDevice(q.dev));
    HIP_OK(hipStreamWaitEvent(q.side, q.done, 0));
    T* f[6] = {q.F[0].p, q.F[1].p, q.F[2].p, q.F[3].p, q.F[4].p, q.F[5].p};
    for (int d = 0; d < 27; ++d) {
      if (q.nb[d] < 0) continue;
      const XRank<T>& o = R[q.nb[d]];
      HIP_OK(hipStreamWaitEvent(q.side, o.done, 0));
      // the neighbour at d packed its box for direction 26 - d (towards us)
      const size_t bytes = q.rbuf[d].n * sizeof(T);
      if (o.dev == q.dev)
        HIP_OK(hipMemcpyAsync(q.rbuf[d].p, o.sbuf[26 - d].p, bytes, hipMemcpyDeviceToDevice, q.side));
      else
        HIP_OK(hipMemcpyPeerAsync(q.rbuf[d].p, q.dev, o.sbuf[26 - d].p, o.dev, bytes, q.side));
      K_OK(box_unpack(f, q.rbuf[d].p, 6, q.n[1], q.n[2], q.rbox[d], q.side));
    }
    HIP_OK(hipEventRecord(q.copied, q.side));
  }
}

// Phase 2 for one rank, on its main stream: the interior -- concurrent with
// phase 1, it reads no ghost -- then, after the pulls, the shells, and the
// packs for the next pass once the neighbours have pulled this pass's (their
// `copied`)
template <typename T>
void MultiRun<T>::rank_pass(XRank<T>& q, int t, int k) {
  HIP_OK(hipSetDevice(q.dev));
  const T* ei[3] = {q.F[0].p, q.F[1].p, q.F[2].p};
  const T* hi[3] = {q.F[3].p, q.F[4].p, q.F[5].p};
  T* eo[3] = {q.G[0].p, q.G[1].p, q.G[2].p};
  T* ho[3] = {q.G[3].p, q.G[4].p, q.G[5].p};
  const T* cbs[3] = {q.C[0].p, q.C[1].p, q.C[2].p};
  const T* dbs[3] = {nullptr, nullptr, nullptr};
  // every rank whose allocated box (ghosts included) holds the source
  // sets the hard source: a neighbour's redundant ghost levels need it
  bool has = true;
  for (int a = 0; a < 3; ++a) has = has && cfg.sp[a] >= q.g0[a] && cfg.sp[a] < q.g0[a] + q.n[a];
  const int src[4] = {cfg.sp[0] - q.g0[0], cfg.sp[1] - q.g0[1], cfg.sp[2] - q.g0[2], has ? 2 : -1};
  double vals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int l = 0; l < k; ++l) vals[l] = cfg.src_val(t + l);
  for (size_t b = 0; b < q.outs.size(); ++b) {
    const int* ob = q.outs[b].data();
    if (b == 1 && !first) HIP_OK(hipStreamWaitEvent(q.st, q.copied, 0));  // the shells read the fresh ghosts
    if (ob[3] <= ob[0] || ob[4] <= ob[1] || ob[5] <= ob[2]) continue;
    if constexpr (sizeof(T) == 4)
      K_OK(fdtd_tb3d_v4_f32(ei, hi, eo, ho, cbs, dbs, cfg.percell ? 1.0 : cfg.cb, cfg.db, q.n[0], q.n[1], q.n[2],
                            q.boxes, ob, 0, k, src, vals, nullptr, q.st));
    else
      K_OK(fdtd_tb3d_f64(ei, hi, eo, ho, cbs, dbs, cfg.percell ? 1.0 : cfg.cb, cfg.db, q.n[0], q.n[1], q.n[2],
                         q.boxes, ob, 0, k, src, vals, nullptr, q.st));
  }
  if (!first && q.outs.size() == 1) HIP_OK(hipStreamWaitEvent(q.st, q.copied, 0));  // a lone rank
  for (int c = 0; c < 6; ++c) std::swap(q.F[c].p, q.G[c].p);
  // the neighbours have pulled the previous packs before these overwrite them
  if (!first)
    for (int d = 0; d < 27; ++d)
      if (q.nb[d] >= 0) HIP_OK(hipStreamWaitEvent(q.st, R[q.nb[d]].copied, 0));
  T* f[6] = {q.F[0].p, q.F[1].p, q.F[2].p, q.F[3].p, q.F[4].p, q.F[5].p};
  for (int d = 0; d < 27; ++d)
    if (q.nb[d] >= 0) K_OK(box_pack(f, q.sbuf[d].p, 6, q.n[1], q.n[2], q.sbox[d], q.st));
  HIP_OK(hipEventRecord(q.done, q.st));
}

// One pass of k steps: the phases are issued rank after rank on the host, so
// every event waited on is already recorded.
template <typename T>
void MultiRun<T>::pass(int t, int k) {
  if (!first) pull_ghosts();
  for (int r = 0; r < P; ++r) rank_pass(R[r], t, k);
  first = false;
}

// UPML / Drude tables of a rank at the global positions, and its part of the
// global chain and plain regions (native_step.h chain_plan) in local indices,
// with the region-local D / D1 levels
template <typename T>
void MultiRun<T>::setup_chain(XRank<T>& q) {
  q.up.reset(new native_phys::Upml<T>());
  native_phys::setup_upml<T>(*q.up, cfg.N, upml_scene(s, cfg.freq), cfg.dt, s.gridStep, q.g0, q.n, true);
  const fdtd::ChainRegions G = chain_plan(s, cfg.N);
  const IBox own = {{q.lo[0], q.lo[1], q.lo[2]}, {q.hi[0], q.hi[1], q.hi[2]}};
  auto local = [&](const fdtd::Box6& b) {
    IBox r = box_and(to_ibox(b), own);
    for (int a = 0; a < 3; ++a) {
      r.lo[a] -= q.g0[a];
      r.hi[a] -= q.g0[a];
    }
    return r;
  };
  std::vector<fdtd::Box6> rb;
  for (size_t r = 0; r < G.chain.size(); ++r) {
    const IBox b = local(G.chain[r]);
    if (b.empty()) continue;
    q.chain_regs.push_back(b);
    q.chain_disp.push_back(G.disp[r]);
    rb.push_back({b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]});
  }
  for (const fdtd::Box6& p : G.plain) {
    const IBox b = local(p);
    if (!b.empty()) q.plain_regs.push_back(b);
  }
  native_phys::alloc_levels(*q.up, rb, q.chain_disp);
}

// amplitude mode of a rank (native_amp.h AmpMode on the rank's cells): the
// maxima and counts, each component's amplitude box (its update range minus
// the PML cells, Scheme3D.cpp:3016-3030) clipped to the owned cells, the owned
// cells of the Ez z line at (Nx / 8, Ny / 2) outside the z PML (Scheme3D.cpp:2995-3013)
template <typename T>
void MultiRun<T>::setup_amp(XRank<T>& q) {
  const size_t plane = (size_t)q.n[1] * q.n[2];
  q.AMP.alloc((size_t)q.n[0] * 6 * plane);
  q.CNT.alloc(std::max(1, s.amplitudeCheckSteps));
  const int left[3] = {s.doUsePML ? s.pmlSizeX : 0, s.doUsePML ? s.pmlSizeY : 0, s.doUsePML ? s.pmlSizeZ : 0};
  for (int c = 0; c < 6; ++c) {
    fdtd::Int3 glo, ghi;
    fdtd::global_range(c, cfg.N, cfg.active, glo, ghi);
    int* b = q.ab + 6 * c;
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
      int lo = glo[a], hi = ghi[a];
      const int right = cfg.N[a] - left[a];
      const bool act = std::find(cfg.active.begin(), cfg.active.end(), a) != cfg.active.end();
      if (act && left[a] != right) {
        lo = std::max(lo, (int)std::ceil(left[a] - kMinFP[c][a]));
        hi = std::min(hi, (int)std::ceil(right - kMinFP[c][a]));
      }
      lo = std::max(lo, q.lo[a]);
      hi = std::min(hi, q.hi[a]);
      empty = empty || hi <= lo;
      b[a] = lo - q.g0[a];
      b[3 + a] = hi - q.g0[a];
    }
    if (empty || !cfg.present[c])
      for (int e = 0; e < 6; ++e) b[e] = 0;
  }
  amp_line = cfg.point_src && cfg.dim == 3;  // (2D: the point source stays)
  if (!amp_line) return;
  const int k0 = s.doUsePML ? s.pmlSizeZ : 0;
  amp_line = cfg.N[2] - 2 * k0 > 0;
  const int li = cfg.N[0] / 8, lj = cfg.N[1] / 2;
  std::vector<long long> offs;
  if (li >= q.lo[0] && li < q.hi[0] && lj >= q.lo[1] && lj < q.hi[1])
    for (int k = std::max(k0, q.lo[2]); k < std::min(cfg.N[2] - k0, q.hi[2]); ++k)
      offs.push_back(((long long)(li - q.g0[0]) * q.n[1] + (lj - q.g0[1])) * q.n[2] + (k - q.g0[2]));
  q.line_n = (int)offs.size();
  if (q.line_n > 0) {
    q.LINE.alloc(offs.size());
    HIP_OK(hipMemcpy(q.LINE.p, offs.data(), offs.size() * sizeof(long long), hipMemcpyHostToDevice));
  }
}

// every array of a rank that carries state between steps (the amplitude
// phase's near-convergence snapshot): all six components, the running
// maxima, then the tables' state
template <typename T>
std::vector<std::pair<void*, size_t>> MultiRun<T>::rank_state(XRank<T>& q) {
  auto v = state_arrays(q.view, nullptr);
  v.insert(v.begin() + 6, {q.AMP.p, q.AMP.n * sizeof(T)});
  return v;
}

// The amplitude phase from step t over the ranks (native_amp.h AmpMode::run):
// check periods of K steps, each step's changed-maximum counts summed over
// the ranks once per period; the run ends with the period in which a step
// (after the first) changed no maximum -- redone from a snapshot up to that
// step near convergence -- or after --amplitude-time-steps steps.  Returns
// the last step.
template <typename T>
int MultiRun<T>::amp_run(int t) {
  amp_on = true;
  const int K = std::max(1, s.amplitudeCheckSteps);
  std::vector<unsigned> got(K), part(K);
  auto period = [&](int n) {
    for (XRank<T>& q : R) {
      HIP_OK(hipSetDevice(q.dev));
      HIP_OK(hipMemsetAsync(q.CNT.p, 0, K * sizeof(unsigned), q.st));
    }
    for (int i = 0; i < n; ++i) {
      phys_step(t);
      for (XRank<T>& q : R) {
        HIP_OK(hipSetDevice(q.dev));
        const T* af[6] = {q.F[0].p, q.F[1].p, q.F[2].p, q.F[3].p, q.F[4].p, q.F[5].p};
        const size_t plane = (size_t)q.n[1] * q.n[2];
        T* aa[6];
        for (int c = 0; c < 6; ++c) aa[c] = q.AMP.p + c * plane;
        K_OK(amp_many(af, aa, 6, q.n[1], q.n[2], q.ab, (long long)(6 * plane), 0.001, q.CNT.p + i, q.st));
      }
      ++t;
    }
    std::fill(got.begin(), got.end(), 0u);
    for (XRank<T>& q : R) {
      HIP_OK(hipSetDevice(q.dev));
      HIP_OK(hipMemcpyAsync(part.data(), q.CNT.p, n * sizeof(unsigned), hipMemcpyDeviceToHost, q.st));
      HIP_OK(hipStreamSynchronize(q.st));
      for (int i = 0; i < n; ++i) got[i] += part[i];
    }
  };
  long long acells = 0;
  for (XRank<T>& q : R)
    for (int c = 0; c < 6; ++c) {
      const int* b = q.ab + 6 * c;
      acells += (long long)std::max(0, b[3] - b[0]) * std::max(0, b[4] - b[1]) * std::max(0, b[5] - b[2]);
    }
  const long long near = std::max(1LL, (long long)(0.02 * (double)acells));
  long long last = -1;
  bool done = false;
  while (!done && amp_taken < s.numAmplitudeTimeSteps) {
    int n = std::min(K, s.numAmplitudeTimeSteps - amp_taken);
    int t_snap = -1;
    if (n > 1 && last >= 0 && last <= near) {
      for (XRank<T>& q : R) {
        HIP_OK(hipSetDevice(q.dev));
        const auto v = rank_state(q);
        size_t total = 0, o = 0;
        for (const auto& e : v) total += e.second;
        if (!q.SNAP.p) q.SNAP.alloc(total);
        for (const auto& e : v) {
          HIP_OK(hipMemcpyAsync(q.SNAP.p + o, e.first, e.second, hipMemcpyDeviceToDevice, q.st));
          o += e.second;
        }
      }
      t_snap = t;
    }
    period(n);
    int first = -1;
    for (int r = 0; r < n && first < 0; ++r)
      if (got[r] == 0 && amp_taken + r + 1 > 1) first = r;
    if (first < 0) {
      last = got[n - 1];
      amp_taken += n;
      continue;
    }
    amp_stable = amp_taken + first + 1;
    if (first + 1 < n && t_snap >= 0) {
      for (XRank<T>& q : R) {
        HIP_OK(hipSetDevice(q.dev));
        const auto v = rank_state(q);
        size_t o = 0;
        for (const auto& e : v) {
          HIP_OK(hipMemcpyAsync(e.first, q.SNAP.p + o, e.second, hipMemcpyDeviceToDevice, q.st));
          o += e.second;
        }
      }
      t = t_snap;
      n = first + 1;
      period(n);
    }
    amp_taken += n;
    done = true;
  }
  amp_on = false;
  return t;
}

// physics set-up of rank r (its device current): owned update boxes, CPML
// tables, TF/SF tables and incident line, the point source; false when the
// TF/SF box does not fit the incident line
template <typename T>
bool MultiRun<T>::setup_physics(int r) {
  XRank<T>& q = R[r];
  int own[6], gb36[36];
  for (int a = 0; a < 3; ++a) {
    own[a] = q.lo[a];
    own[3 + a] = q.hi[a];
  }
  for (int c = 0; c < 6; ++c) {
    fdtd::Int3 glo, ghi;
    fdtd::global_range(c, cfg.N, cfg.active, glo, ghi);
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
      const int lo = std::max(glo[a], q.lo[a]), hi = std::min(ghi[a], q.hi[a]);
      empty = empty || hi <= lo;
      gb36[6 * c + a] = lo;
      gb36[6 * c + 3 + a] = hi;
    }
    for (int a = 0; a < 3; ++a) {
      if (empty) gb36[6 * c + a] = gb36[6 * c + 3 + a] = 0;
      q.own36[6 * c + a] = empty ? 0 : gb36[6 * c + a] - q.g0[a];
      q.own36[6 * c + 3 + a] = empty ? 0 : gb36[6 * c + 3 + a] - q.g0[a];
    }
  }
  if (cfg.dim == 2) {
    q.p2.reset(new Pml2d<T>());
    if (cfg.cpml) setup_cpml2d(*q.p2, s, cfg.N, cfg.active, cfg.present, cfg.dt, s.gridStep, own, q.g0, q.n);
    if (cfg.upml) {
      std::vector<T> inv[3];
      if (cfg.percell) inv_eps_2d(s, cfg.present, q.g0, q.n, inv);
      setup_upml2d(*q.p2, s, cfg.N, cfg.present, cfg.dt, s.gridStep, inv, q.g0, q.n);
    }
    const fdtd::Int3 ext = {q.n[0], q.n[1], q.n[2]};
    q.ld.reset(new Lowdim2d<T>(s, q.F, q.C, q.own36, ext, cfg.present, *q.p2, cfg.tmz, cfg.percell, cfg.cb, cfg.db,
                               q.st, &cfg.N, q.g0));
  } else {
    if (cfg.cpml) {
      q.cp.reset(new NativeCpml<T>());
      setup_cpml(*q.cp, s, cfg.N, cfg.active, cfg.dt, s.gridStep, own, q.g0, q.n);
    }
    if (cfg.upml) setup_chain(q);
  }
  // (E: per-cell arrays of the sphere or the scalar; H: the scalar db, mu = 1 -- 1D / 2D: db arrays)
  const double ce = cfg.percell ? 1.0 : cfg.cb, ch = cfg.dim < 3 && cfg.percell ? 1.0 : cfg.db;
  if (cfg.tfsf) {
    q.tf.reset(new NativeTfsf<T>());
    if (!setup_tfsf(*q.tf, s, cfg.N, gb36, q.C, ce, ch, cfg.dt, s.gridStep, cfg.freq, cfg.dim, cfg.present, q.g0, q.n))
      return false;
  }
  if (cfg.amp) setup_amp(q);
  bool has = cfg.point_src;
  for (int a = 0; a < 3; ++a) has = has && cfg.sp[a] >= q.lo[a] && cfg.sp[a] < q.hi[a];
  q.src_off =
      has ? ((long long)(cfg.sp[0] - q.g0[0]) * q.n[1] + (cfg.sp[1] - q.g0[1])) * q.n[2] + (cfg.sp[2] - q.g0[2]) : -1;
  // the split half steps' view of the rank (native_step.h): its owned update
  // boxes, its own extents, whichever tables it has
  StepView<T>& v = q.view;
  v.F = q.F;
  for (int c = 0; c < 6; ++c) v.C[c] = q.C[c].p;
  v.ce = ce;
  v.ch = ch;
  for (int a = 0; a < 3; ++a) v.n[a] = q.n[a];
  v.boxes = q.own36;
  v.v4 = sizeof(T) == 4 && q.n[2] % 4 == 0;
  v.st = q.st;
  v.cp = q.cp.get();
  v.p2 = q.p2.get();
  v.ld = q.ld.get();
  v.ld_plain = true;
  v.up = q.up.get();
  v.chain_regs = &q.chain_regs;
  v.plain_regs = &q.plain_regs;
  v.chain_disp = &q.chain_disp;
  v.tf = q.tf.get();
  v.src_off = q.src_off;
  if (amp_line) {  // the amplitude phase's Ez z line replaces the point source on every rank
    v.line_phase = &amp_on;
    v.line = q.LINE.p;
    v.line_n = q.line_n;
  }
  return true;
}

// the updated kind's three components to the face neighbours' ghosts: every
// rank packs its boxes (after the neighbours pulled the previous ones), then
// every rank pulls (peer copies across devices) and unpacks on its main
// stream, so its next half step reads the fresh ghosts
template <typename T>
void MultiRun<T>::exchange(int kind) {
  for (int r = 0; r < P; ++r) {
    XRank<T>& q = R[r];
    HIP_OK(hipSetDevice(q.dev));
    T* f[3] = {q.F[3 * kind].p, q.F[3 * kind + 1].p, q.F[3 * kind + 2].p};
    for (int d = 0; d < 27; ++d) {
      if (q.nb[d] < 0) continue;
      if (!first) HIP_OK(hipStreamWaitEvent(q.st, R[q.nb[d]].copied, 0));
      K_OK(box_pack(f, q.sbuf[d].p, 3, q.n[1], q.n[2], q.sbox[d], q.st));
    }
    HIP_OK(hipEventRecord(q.done, q.st));
  }
  for (int r = 0; r < P; ++r) {
    XRank<T>& q = R[r];
    HIP_OK(hipSetDevice(q.dev));
    T* f[3] = {q.F[3 * kind].p, q.F[3 * kind + 1].p, q.F[3 * kind + 2].p};
    for (int d = 0; d < 27; ++d) {
      if (q.nb[d] < 0) continue;
      const XRank<T>& o = R[q.nb[d]];
      HIP_OK(hipStreamWaitEvent(q.st, o.done, 0));
      const size_t bytes = q.rbuf[d].n * sizeof(T);
      if (o.dev == q.dev)
        HIP_OK(hipMemcpyAsync(q.rbuf[d].p, o.sbuf[26 - d].p, bytes, hipMemcpyDeviceToDevice, q.st));
      else
        HIP_OK(hipMemcpyPeerAsync(q.rbuf[d].p, q.dev, o.sbuf[26 - d].p, o.dev, bytes, q.st));
      K_OK(box_unpack(f, q.rbuf[d].p, 3, q.n[1], q.n[2], q.rbox[d], q.st));
    }
    HIP_OK(hipEventRecord(q.copied, q.st));
  }
  first = false;
}

template <typename T>
void MultiRun<T>::phys_step(int t) {
  const double sv = cfg.src_val(t);
  for (int kind = 0; kind < 2; ++kind) {
    for (int r = 0; r < P; ++r) {
      HIP_OK(hipSetDevice(R[r].dev));
      split_half(R[r].view, cfg, kind, sv);
    }
    if (P > 1) exchange(kind);
  }
}

template <typename T>
void MultiRun<T>::advance(int t0, int n) {
  if (phys) {
    for (int q = 0; q < n; ++q) phys_step(t0 + q);
    return;
  }
  int t = t0;
  while (n > 0) {
    const int k = std::min(TB, n);
    pass(t, k);
    t += k;
    n -= k;
  }
}

template <typename T>
void MultiRun<T>::sync() {
  for (int r = 0; r < P; ++r) {
    HIP_OK(hipSetDevice(R[r].dev));
    HIP_OK(hipStreamSynchronize(R[r].st));
  }
}

// (the checkpoint I/O line of the one-GPU report has never been printed
// here: report_head gets no timer)
template <typename T>
void MultiRun<T>::report(double sec, int t_end, int steps, int warm) const {
  const int timed = steps - warm + amp_taken;
  report_head<T>(cfg, sec, 0.0, t_end, timed, warm);
  std::printf("\n-------- Details --------\n");
  std::printf("Parallel grid: 1\n");
  std::printf("Number of processes: %d (ranks of one process on %d device%s)\n", P, std::min(P, ndev),
              std::min(P, ndev) > 1 ? "s" : "");
  std::string axes;
  for (int a = 0; a < 3; ++a)
    if (Pd[a] > 1) axes += "XYZ"[a];
  std::printf("Parallel grid scheme: %s (topology %dx%dx%d)\n", axes.empty() ? "X" : axes.c_str(), Pd[0], Pd[1],
              Pd[2]);
  std::printf("Buffer size: %d\n", TB);
  const bool meta = s.doUseMetamaterials;
  if (phys)
    std::printf("Backend: native HIP, split half-step kernels (%s%s%s), face ghosts (%d x / %d y / %d z cells) by "
                "packed peer copies after every half step\n",
                cfg.cpml ? "CPML"
                         : (cfg.upml ? (meta ? "UPML D/B chain + dispersive sphere" : "UPML D/B chain")
                                     : (cfg.tfsf ? "" : (cfg.dim == 3 ? "plain" : (cfg.dim == 2 ? "2D" : "1D")))),
                (cfg.cpml || cfg.upml) && cfg.tfsf ? " + " : "", cfg.tfsf ? "TF/SF" : "", gd[0], gd[1], gd[2]);
  else
    std::printf("Backend: native HIP, temporally blocked kernel (%d steps per pass), 26-neighbour ghost boxes by "
                "packed peer copies\n", TB);
  report_tail(s, cfg, sec, timed, amp_taken, amp_stable, P);
}

// component c of the whole grid on the host: every rank's owned block
template <typename T>
void MultiRun<T>::gather(int c, std::vector<T>& host) {
  host.resize((size_t)cfg.N[0] * cfg.N[1] * cfg.N[2]);
  std::vector<T> loc;
  for (int r = 0; r < P; ++r) {
    const XRank<T>& q = R[r];
    HIP_OK(hipSetDevice(q.dev));
    loc.resize(q.cells());
    HIP_OK(hipMemcpy(loc.data(), q.F[c].p, loc.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (int i = q.lo[0]; i < q.hi[0]; ++i)
      for (int j = q.lo[1]; j < q.hi[1]; ++j)
        std::memcpy(host.data() + ((size_t)i * cfg.N[1] + j) * cfg.N[2] + q.lo[2],
                    loc.data() + ((size_t)(i - q.g0[0]) * q.n[1] + (j - q.g0[1])) * q.n[2] + (q.lo[2] - q.g0[2]),
                    (size_t)(q.hi[2] - q.lo[2]) * sizeof(T));
  }
}

// the NTFF diagram's fields: the ranks' owned blocks assembled into
// whole-grid arrays on the first rank's device (then the one-GPU surface
// reduction, native_step.h ntff_print)
template <typename T>
std::array<T*, 6> MultiRun<T>::ntff_fields() {
  std::vector<T> host;
  std::array<T*, 6> Fp;
  for (int c = 0; c < 6; ++c) {
    gather(c, host);
    HIP_OK(hipSetDevice(R[0].dev));
    if (!NG[c].p) NG[c].alloc(host.size());
    HIP_OK(hipMemcpy(NG[c].p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    Fp[c] = NG[c].p;
  }
  return Fp;
}

// component c of the whole grid into every rank's allocated box (owned cells
// and ghosts: a resumed run's first pass reads the ghosts as they are)
template <typename T>
void MultiRun<T>::scatter(int c, const std::vector<T>& host) {
  std::vector<T> loc;
  for (int r = 0; r < P; ++r) {
    XRank<T>& q = R[r];
    loc.resize(q.cells());
    for (int li = 0; li < q.n[0]; ++li)
      for (int lj = 0; lj < q.n[1]; ++lj)
        std::memcpy(loc.data() + ((size_t)li * q.n[1] + lj) * q.n[2],
                    host.data() + ((size_t)(q.g0[0] + li) * cfg.N[1] + (q.g0[1] + lj)) * cfg.N[2] + q.g0[2],
                    (size_t)q.n[2] * sizeof(T));
    HIP_OK(hipSetDevice(q.dev));
    HIP_OK(hipMemcpy(q.F[c].p, loc.data(), loc.size() * sizeof(T), hipMemcpyHostToDevice));
  }
}

// a checkpoint of step t: the gathered grid in the serial form (native_ckpt.h)
template <typename T>
bool MultiRun<T>::save_checkpoint(int t) {
  if (ckpt_save<T>(s, cfg.scheme, cfg.N, cfg.present, [this](int c, std::vector<T>& host) { gather(c, host); }, t,
                   s.gridStep, cfg.dt))
    return true;
  std::fprintf(stderr, "fdtd3d: cannot write the checkpoint to %s\n", s.checkpointDir.c_str());
  return false;
}

// --checkpoint-dir: the final checkpoint; --save-res: the owned blocks of
// every rank assembled into global DAT / BMP files
template <typename T>
bool MultiRun<T>::save_results(int steps) {
  if (!s.checkpointDir.empty() && !save_checkpoint(steps)) return false;
  if (!s.doSaveRes) return true;
  std::vector<T> host;
  for (int c = 0; c < 6; ++c) {
    if (!cfg.present[c]) continue;
    gather(c, host);
    save_component(s, cfg, c, host, steps);
  }
  return true;
}

template <typename T>
void MultiRun<T>::release() {
  for (auto& q : R) {
    if (!q.st) continue;
    HIP_OK(hipSetDevice(q.dev));
    for (int c = 0; c < 6; ++c) {  // freed with the rank's device current
      q.F[c].reset();
      q.G[c].reset();
      q.C[c].reset();
    }
    for (int d = 0; d < 27; ++d) {
      q.sbuf[d].reset();
      q.rbuf[d].reset();
    }
    q.cp.reset();
    q.tf.reset();
    q.up.reset();
    q.ld.reset();
    q.p2.reset();
    q.AMP.reset();
    q.CNT.reset();
    q.LINE.reset();
    q.SNAP.reset();
    HIP_OK(hipEventDestroy(q.done));
    HIP_OK(hipEventDestroy(q.copied));
    HIP_OK(hipStreamDestroy(q.st));
    HIP_OK(hipStreamDestroy(q.side));
    q.st = nullptr;
  }
  if (!R.empty()) {
    HIP_OK(hipSetDevice(R[0].dev));
    for (int c = 0; c < 6; ++c) NG[c].reset();
  }
}

template <typename T>
int MultiRun<T>::main() {
  if (const int rc = plan_ranks()) return rc;
  for (int r = 0; r < P; ++r) {
    setup_rank(r);
    if (phys && !setup_physics(r)) return 2;
  }
  enable_peers();
  plan_outputs();
  // --load-from-file: a serial-form checkpoint (either driver's, or a
  // decomposed native run's gathered one) scattered over the ranks
  int t0 = 0;
  if (!s.loadFromFile.empty()) {
    const long got =
        ckpt_load<T>(s, cfg.scheme, cfg.N, cfg.present,
                     [this](int c, const std::vector<T>& host) { scatter(c, host); });
    if (got < 0) return 1;
    t0 = (int)got;
  }
  const int steps = std::max(0, s.numTimeSteps - t0);
  const int warm = std::max(0, std::min(s.warmupSteps, steps));
  run_ckpt(*this, t0, warm);
  sync();
  const auto c0 = std::chrono::steady_clock::now();
  ckpt_ms = 0.0;
  run_ckpt(*this, t0 + warm, steps - warm);
  // amplitude mode: after the regular steps, check periods until a step
  // changes no running maximum (native_amp.h)
  const int t_end = cfg.amp ? amp_run(t0 + steps) : t0 + steps;
  sync();
  HIP_OK(hipGetLastError());
  const double sec =
      std::max(0.0, std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count() - ckpt_ms / 1e3);
  report(sec, t_end, steps, warm);
  return save_results(t_end) ? 0 : 1;
}

template <typename T>
int run_multi(const fdtd::Settings& s) {
  MultiRun<T> m(s);
  return m.main();
}

}  // namespace
