// native_step.h -- the stepped path of the native driver, shared by its two run
// classes (NativeRun: one GPU, native_run.h; MultiRun: the ranks of a
// --parallel-grid run, native_multi.h): the configuration derived from the
// settings, the scene helpers of the set-up, the split half step on a
// StepView (one per run or per rank), the run loop with its NTFF and
// checkpoint cadences, the report's common lines, the DAT / BMP writer and
// the list of arrays that carry state between steps.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "capi.h"
#include "host_native.h"
#include "native_physics.h"
#include "settings_native.h"
#include "native_api.h"
#include "native_setup.h"
#include "native_lowdim.h"

// Part of the native driver: included by main.cpp only (one translation unit),
// hence the unnamed namespace.
namespace {

// ============================================================== configuration

// what a run derives from the settings alone, filled once
struct RunConfig {
  int dim;
  std::string scheme;  // "3d", "tmz", "tez", "1d"
  bool tmz;
  fdtd::Int3 N;
  std::vector<int> active;
  bool present[6];  // components: 0..2 E, 3..5 H
  double dx, dt, freq, cb, db;
  // per-cell coefficient arrays (a scene with eps != 1; a Drude sphere's
  // eps_inf is 1: layout/materials.py Scene.eps).  NativeRun also counts the
  // `reference` scene outside 3D as vacuum and overwrites this with its own
  // form; decomposed runs take neither that scene nor this exception.
  bool percell;
  bool upml, cpml, tfsf, ntff, amp;
  bool point_src;
  fdtd::Int3 sp;  // the point source (reference Scheme3D.cpp:2011-2022, SchemeTMz.cpp:1345)
  int src_comp;
  bool gaussian;
  double gauss_delay, gauss_width;

  explicit RunConfig(const fdtd::Settings& s) {
    dim = s.dimension;
    scheme = dim == 3 ? "3d" : (dim == 2 ? s.mode2D : "1d");
    tmz = scheme == "tmz";
    N = {s.sizeX, dim >= 2 ? s.sizeY : 1, dim == 3 ? s.sizeZ : 1};
    active = dim == 3 ? std::vector<int>{0, 1, 2} : (dim == 2 ? std::vector<int>{0, 1} : std::vector<int>{0});
    for (int c = 0; c < 6; ++c) present[c] = dim == 3;
    if (scheme == "tmz") present[2] = present[3] = present[4] = true;
    if (scheme == "tez") present[0] = present[1] = present[5] = true;
    if (scheme == "1d") present[2] = present[4] = true;
    dx = s.gridStep;
    dt = dx * s.courantNum / kC;
    freq = kC / s.sourceWaveLength;
    cb = dt / (kEps0 * dx);
    db = dt / (kMu0 * dx);
    percell = s.scene != "vacuum" && s.scene != "drude-sphere";
    upml = (s.doUsePML && s.pmlType == "upml") || s.doUseMetamaterials;  // the D/B chain
    cpml = s.doUsePML && !upml;
    tfsf = s.doUseTFSF;
    ntff = s.doUseNTFF && dim == 3;
    amp = s.doUseAmplitudeMode;
    point_src = !tfsf || s.doUsePointSource;
    sp = {N[0] / 2, N[1] / 2, N[2] / 2};
    if (scheme == "tmz") sp = {N[0] > 140 ? 70 : N[0] / 2, N[1] / 2, 0};
    if (scheme == "1d") sp = {N[0] / 2, 0, 0};
    src_comp = scheme == "tez" ? 5 : 2;
    gaussian = s.sourceType == "gaussian";
    gauss_delay = s.gaussianDelay;
    gauss_width = s.gaussianWidth;
  }

  size_t cells() const { return (size_t)N[0] * N[1] * N[2]; }

  // the source at step t; plane 1 = the imaginary part of a complex run (the
  // cos / zero source, models/scheme.py source_value)
  double src_val(int t, int plane = 0) const {
    if (gaussian) return plane == 0 ? std::exp(-std::pow((t - gauss_delay) / gauss_width, 2)) : 0.0;
    return plane == 0 ? std::sin(dt * t * 2 * kPi * freq) : std::cos(dt * t * 2 * kPi * freq);
  }
};

// ====================================================================== set-up

IBox to_ibox(const fdtd::Box6& b) { return IBox{{b[0], b[1], b[2]}, {b[3], b[4], b[5]}}; }

// the scene of the 3D D/B chain tables (native_physics.h setup_upml)
native_phys::UpmlScene upml_scene(const fdtd::Settings& s, double freq) {
  native_phys::UpmlScene sc;
  sc.pml[0] = s.pmlSizeX;
  sc.pml[1] = s.pmlSizeY;
  sc.pml[2] = s.pmlSizeZ;
  sc.use_pml = s.doUsePML;
  sc.metamaterials = s.doUseMetamaterials;
  sc.lorentz = s.dispersion == "lorentz";
  sc.lorentz_ratio = s.lorentzOmega0Ratio;
  sc.freq = freq;
  sc.sphere_eps = s.scene == "sphere";
  sc.drude_sphere = s.scene == "drude-sphere";
  sc.ctr[0] = s.sphereCenterX;
  sc.ctr[1] = s.sphereCenterY;
  sc.ctr[2] = s.sphereCenterZ;
  sc.radius = s.sphereRadius;
  sc.eps_in = s.sphereEps;
  return sc;
}

// the sphere's bounding box with the stencils' reach (host_native.cpp)
fdtd::Box6 sphere_box(const fdtd::Settings& s, const fdtd::Int3& N) {
  const double ctr[3] = {s.sphereCenterX, s.sphereCenterY, s.sphereCenterZ};
  return fdtd::dispersive_box(N, ctr, s.sphereRadius);
}

// the global chain / plain regions of a 3D UPML or dispersive run (host_native.cpp chain_regions)
fdtd::ChainRegions chain_plan(const fdtd::Settings& s, const fdtd::Int3& N) {
  const int pml[3] = {s.pmlSizeX, s.pmlSizeY, s.pmlSizeZ};
  return fdtd::chain_regions(N, pml, s.doUsePML, s.doUseMetamaterials, sphere_box(s, N));
}

// 2D UPML: per-cell 1 / (eps eps0) of a dielectric scene for the present E
// components (the 2-point averages of the plain coefficients) over the box
// at global origin `org` with extents `ext`
template <typename T>
void inv_eps_2d(const fdtd::Settings& s, const bool* present, const int* org, const int* ext, std::vector<T>* inv) {
  const double ctr[3] = {s.sphereCenterX, s.sphereCenterY, s.sphereCenterZ};
  for (int c = 0; c < 3; ++c) {
    if (!present[c]) continue;
    inv[c].resize((size_t)ext[0] * ext[1] * ext[2]);
    const int di = c == 0, dj = c == 1;
    for (int li = 0; li < ext[0]; ++li)
      for (int lj = 0; lj < ext[1]; ++lj) {
        const int i = org[0] + li, j = org[1] + lj;
        const double a = sphere_eps(i + 0.5, j + 0.5, ctr[2], ctr, s.sphereRadius, s.sphereEps);
        const double b = sphere_eps(i + di + 0.5, j + dj + 0.5, ctr[2], ctr, s.sphereRadius, s.sphereEps);
        inv[c][(size_t)li * ext[1] + lj] = (T)(1.0 / ((a + b) / 2.0 * kEps0));
      }
  }
}

// the update boxes of components c0 .. c0 + nc - 1 (six ints each in b36)
// clipped to a region; an empty one becomes all zeros
void clip36(const int* b36, const IBox& r, int* out, int c0 = 0, int nc = 6) {
  for (int c = c0; c < c0 + nc; ++c) {
    IBox b;
    for (int a = 0; a < 3; ++a) {
      b.lo[a] = b36[6 * c + a];
      b.hi[a] = b36[6 * c + 3 + a];
    }
    b = box_and(b, r);
    for (int a = 0; a < 3; ++a) {
      out[6 * (c - c0) + a] = b.empty() ? 0 : b.lo[a];
      out[6 * (c - c0) + 3 + a] = b.empty() ? 0 : b.hi[a];
    }
  }
}

// ============================================================= the half step

using ChainFn = int (*)(const void* const*, const double*, const int*, int, int, int, int, void*);
template <typename T>
ChainFn chain3d() {
  return sizeof(T) == 4 ? (ChainFn)fdtd_chain3d_f32 : (ChainFn)fdtd_chain3d_f64;
}

// What a split half step launches on: built once per run (NativeRun) or per
// rank (MultiRun).  The two classes hand the same kernels different argument
// forms (per-cell arrays with the scalar 1 against null arrays with the
// scalar, the grid's extents against the rank's, ...): the view carries each
// form as data, and split_half issues what it finds.
template <typename T>
struct StepView {
  const Dev<T>* F = nullptr;  // the six field buffers, read at every launch (the pass executors swap F and G)
  const T* C[6] = {};         // per-cell coefficient arrays (null: the scalar alone)
  double ce = 0, ch = 0;      // the E / H coefficient scalars
  int n[3] = {1, 1, 1};       // array extents
  const int* boxes = nullptr;  // 36 ints: every component's update box
  bool v4 = false;             // fp32 rows of whole float4 lanes
  hipStream_t st = nullptr;
  // whichever tables the run has
  NativeCpml<T>* cp = nullptr;  // 3D CPML folded into the 4-cell-lane kernels
  bool cpml_generic = false;    // 3D CPML as the scalar kernels + generic slabs (z rows of no whole lanes)
  Pml2d<T>* p2 = nullptr;       // the generic CPML slabs / 2D UPML strips
  Lowdim2d<T>* ld = nullptr;    // their half-step helper
  bool ld_plain = false;        // the plain 2D update through Lowdim2d::plain, not the kernels directly
  native_phys::Upml<T>* up = nullptr;  // 3D D/B chain with its chain / plain regions
  const std::vector<IBox>*chain_regs = nullptr, *plain_regs = nullptr;
  const std::vector<bool>* chain_disp = nullptr;
  NativeTfsf<T>* tf = nullptr;
  // the hard source: the point's offset (-1: none here), or, while
  // *line_phase, the amplitude mode's Ez z line (line_n cells here)
  long long src_off = -1;
  const bool* line_phase = nullptr;
  const long long* line = nullptr;
  int line_n = 0;
};

// the update of one kind (0 = E, 1 = H): 1D, 2D (plain | UPML strips, + CPML
// slabs), 3D chain regions plus the plain rest, folded CPML, or plain (+ the
// generic CPML slabs)
template <typename T>
void split_update(const StepView<T>& v, const RunConfig& cfg, int kind) {
  T* F[6];
  for (int c = 0; c < 6; ++c) F[c] = v.F[c].p;
  const T* const* C = v.C;
  const double cs = kind == 0 ? v.ce : v.ch;
  const int* bx = v.boxes + 18 * kind;
  const int nx = v.n[0], ny = v.n[1], nz = v.n[2];
  if (cfg.dim == 1) {
    if (kind == 0)
      K_OK(e1d(F[2], F[4], C[2], cs, v.boxes[12], v.boxes[15], v.st));
    else
      K_OK(h1d(F[4], F[2], C[4], cs, v.boxes[24], v.boxes[27], v.st));
  } else if (cfg.dim == 2) {
    if (cfg.upml)
      v.ld->upml(kind);
    else if (v.ld_plain)
      v.ld->plain(kind, IBox{{0, 0, 0}, {nx, ny, nz}});
    else if (kind == 0 && cfg.tmz)
      K_OK(tmz_e(F[2], F[3], F[4], C[2], cs, nx, ny, v.boxes + 12, v.st));
    else if (kind == 0)
      K_OK(tez_e(F[0], F[1], F[5], C[0], C[1], cs, nx, ny, v.boxes, v.st));
    else if (cfg.tmz)
      K_OK(tmz_h(F[3], F[4], F[2], C[3], C[4], cs, nx, ny, v.boxes + 18, v.st));
    else
      K_OK(tez_h(F[5], F[0], F[1], C[5], cs, nx, ny, v.boxes + 30, v.st));
    if (cfg.cpml) v.ld->cpml(kind);
  } else if (cfg.upml) {
    // the chain on the PML slabs and the dispersive box, the plain update on the rest
    int rb[36];
    for (size_t q = 0; q < v.chain_regs->size(); ++q) {
      clip36(v.boxes, (*v.chain_regs)[q], rb);
      K_OK(native_phys::upml_kind<T>(*v.up, F, rb, kind, ny, nz, v.st, chain3d<T>(), false, !(*v.chain_disp)[q],
                                     nullptr, 1.0, (int)q));
    }
    native_phys::upml_rotate(*v.up, kind);
    for (const IBox& r : *v.plain_regs) {
      clip36(v.boxes, r, rb);
      if (kind == 0)
        K_OK(e3d(F[0], F[1], F[2], F[3], F[4], F[5], C[0], C[1], C[2], cs, nx, ny, nz, rb, 0, v.st, v.v4));
      else
        K_OK(h3d(F[3], F[4], F[5], F[0], F[1], F[2], C[3], C[4], C[5], cs, nx, ny, nz, rb + 18, 0, v.st, v.v4));
    }
  } else if (cfg.cpml && !v.cpml_generic) {
    if (kind == 0)
      K_OK(cpml_e3d(F, C, cs, nx, ny, nz, bx, v.cp->P[0].data(), v.cp->I[0].data(), v.st));
    else
      K_OK(cpml_h3d(F, C, cs, nx, ny, nz, bx, v.cp->P[1].data(), v.cp->I[1].data(), v.st));
  } else {
    if (kind == 0)
      K_OK(e3d(F[0], F[1], F[2], F[3], F[4], F[5], C[0], C[1], C[2], cs, nx, ny, nz, bx, 0, v.st, v.v4));
    else
      K_OK(h3d(F[3], F[4], F[5], F[0], F[1], F[2], C[3], C[4], C[5], cs, nx, ny, nz, bx, 0, v.st, v.v4));
    if (v.cpml_generic) v.ld->cpml(kind);
  }
}

// One half step of kind 0 = E / 1 = H around `update`, the order of
// scheme.step: [incident line] update [TF/SF corrections] [E: the point
// source or the amplitude z line]
template <typename T, typename Update>
void half_step(const StepView<T>& v, const RunConfig& cfg, int kind, double sv, Update&& update) {
  if (cfg.tfsf) {
    NativeTfsf<T>& tf = *v.tf;
    if (kind == 0)
      K_OK(inc_e(tf.einc.p, tf.hinc.p, tf.nline, tf.ce, sv, v.st));
    else
      K_OK(inc_h(tf.einc.p, tf.hinc.p, tf.nline, tf.ch, v.st));
  }
  update();
  if (cfg.tfsf) {
    const int whole[6] = {0, 0, 0, v.n[0], v.n[1], v.n[2]};
    for (int c = 3 * kind; c < 3 * kind + 3; ++c)
      for (auto* l : v.tf->tab[c])
        K_OK(tfsf_apply(v.F[c].p, *l, kind == 0 ? v.tf->hinc.p : v.tf->einc.p, whole, v.st));
  }
  if (kind == 0) {
    if (v.line_phase && *v.line_phase) {
      if (v.line_n > 0) K_OK(setvs(v.F[2].p, v.line, v.line_n, sv, v.st));
    } else if (v.src_off >= 0) {
      K_OK(setv(v.F[cfg.src_comp].p, v.src_off, sv, v.st));
    }
  }
}

// the split half step: every launch of the stepped path of both run classes
template <typename T>
void split_half(const StepView<T>& v, const RunConfig& cfg, int kind, double sv) {
  half_step(v, cfg, kind, sv, [&] { split_update(v, cfg, kind); });
}

// every array that carries state between steps, in logical order (the current
// F / D level lists, whatever the pointer swaps did): the amplitude mode's
// snapshot of a check period is laid out by this list.  `present`: the
// components listed (null: all six).  (The 2D strips' D levels and the 3D
// chain's never exist in one run.)
template <typename T>
std::vector<std::pair<void*, size_t>> state_arrays(const StepView<T>& v, const bool* present) {
  const size_t cells = (size_t)v.n[0] * v.n[1] * v.n[2];
  std::vector<std::pair<void*, size_t>> out;
  for (int c = 0; c < 6; ++c)
    if (!present || present[c]) out.push_back({v.F[c].p, cells * sizeof(T)});
  if (v.tf) {
    out.push_back({v.tf->einc.p, (size_t)v.tf->nline * sizeof(T)});
    out.push_back({v.tf->hinc.p, (size_t)v.tf->nline * sizeof(T)});
  }
  if (v.cp)
    for (auto* d : v.cp->keep) out.push_back({d->p, d->n * sizeof(T)});
  if (v.p2) {
    for (const Slab2d<T>& sl : v.p2->slabs)
      out.push_back({sl.psi, (size_t)(sl.pbox[3] - sl.pbox[0]) * (sl.pbox[4] - sl.pbox[1]) *
                                 (sl.pbox[5] - sl.pbox[2]) * sizeof(T)});
    for (int c = 0; c < 6; ++c)
      for (int l = 0; l < 2; ++l)
        if (v.p2->D[c][l]) out.push_back({v.p2->D[c][l], cells * sizeof(T)});
  }
  if (v.up)
    for (int c = 0; c < 6; ++c) {
      for (const auto& lv : v.up->D[c])
        for (size_t q = 0; q < lv.size(); ++q) out.push_back({lv[q], v.up->rvol[q] * sizeof(T)});
      for (const auto& lv : v.up->D1[c])
        for (size_t q = 0; q < lv.size(); ++q)
          if (lv[q]) out.push_back({lv[q], v.up->rvol[q] * sizeof(T)});
    }
  return out;
}

// ==================================================================== run loop
// The loops below drive a run object `r` with the members s (settings), cfg,
// ckpt_ms, advance(t, n), sync(), ntff_fields() (six whole-grid device
// pointers) and save_checkpoint(t).

// the NTFF scattered power diagram of step t from six whole-grid components
template <typename T>
void ntff_print(const fdtd::Settings& s, const RunConfig& cfg, T* const* F, int t) {
  const int nbox[3] = {s.ntffSizeX, s.ntffSizeY, s.ntffSizeZ};
  const std::vector<double> phis = native_phys::reference_angles();
  const std::vector<double> p = native_phys::ntff_power<T>(F, cfg.N, nbox, cfg.dx, s.sourceWaveLength,
                                                           s.incidentWaveAngle1 * (kPi / 180.0), phis);
  for (size_t q = 0; q < phis.size(); ++q)
    std::printf("=== t=%u, inc angle=%f; angle %f === %.17g \n", (unsigned)t, s.incidentWaveAngle2 * (kPi / 180.0),
                phis[q], p[q]);
}

// n steps from t0, with the NTFF diagram after every step t with (t - 1) %
// ntffStep == 0, for the fields of step t - 1 (the Python driver's periodic
// hook, runner.py)
template <typename R>
void run_steps(R& r, int t0, int n) {
  if (!r.cfg.ntff) {
    r.advance(t0, n);
    return;
  }
  const int nstep = std::max(1, r.s.ntffStep);
  int t = t0;
  const int end = t0 + n;
  while (t < end) {
    const int nxt = std::min(end, t + 1 + ((1 - (t + 1)) % nstep + nstep) % nstep);
    r.advance(t, nxt - t);
    t = nxt;
    if ((t - 1) % nstep == 0) {
      r.sync();
      ntff_print(r.s, r.cfg, r.ntff_fields().data(), t - 1);
    }
  }
}

// --checkpoint-step P: a checkpoint after every step t with t % P == 0 (the
// Python driver's periodic hook), the passes ending there; the checkpoint I/O
// time (host wall clock, the device idle) is kept out of the reported
// stepping rate, as the Python driver's phase timers do
template <typename R>
void run_ckpt(R& r, int t, int n) {
  const int P = r.s.checkpointDir.empty() ? 0 : r.s.checkpointStep;
  if (P <= 0) {
    run_steps(r, t, n);
    return;
  }
  const int end = t + n;
  while (t < end) {
    const int nxt = std::min(end, (t / P + 1) * P);
    run_steps(r, t, nxt - t);
    t = nxt;
    if (t % P == 0) {
      r.sync();
      const auto c0 = std::chrono::steady_clock::now();
      if (!r.save_checkpoint(t)) std::exit(1);
      r.ckpt_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
    }
  }
}

// ====================================================================== report

// the report up to the value type.  ckpt_ms > 0 prints the checkpoint I/O
// line: NativeRun passes its timer, MultiRun never has printed that line and
// passes 0.
template <typename T>
void report_head(const RunConfig& cfg, double sec, double ckpt_ms, int t_end, int timed, int warm) {
  std::printf("Total time = %f seconds\n", sec);
  if (ckpt_ms > 0) std::printf("Checkpoint I/O = %f seconds (not in the total)\n", ckpt_ms / 1e3);
  std::printf("Dimension: %d\n", cfg.dim);
  if (cfg.dim == 3)
    std::printf("Grid size: %dx%dx%d\n", cfg.N[0], cfg.N[1], cfg.N[2]);
  else if (cfg.dim == 2)
    std::printf("Grid size: %dx%d\n", cfg.N[0], cfg.N[1]);
  else
    std::printf("Grid size: %d\n", cfg.N[0]);
  std::printf("Number of time steps: %d (%d timed after %d warm-up)\n\n", t_end, timed, warm);
  std::printf("Value type: %s\n", Api<T>::name);
}

// the report after the "Backend:" line: throughput, the amplitude mode's
// outcome, the JSON line (ranks > 0: with the rank count)
void report_tail(const fdtd::Settings& s, const RunConfig& cfg, double sec, int timed, int amp_taken, int amp_stable,
                 int ranks) {
  const double rate = (double)cfg.cells() * (double)timed / sec / 1e6;
  std::printf("Throughput: %.1f Mcells/s\n", rate);
  if (cfg.amp) {
    if (amp_stable > 0)
      std::printf("Amplitude mode: stable after %d steps (%d amplitude steps taken)\n", amp_stable, amp_taken);
    else
      std::printf("Amplitude mode: stable state not reached after %d steps\n", amp_taken);
  }
  if (!s.doPrintJson) return;
  std::printf("{\"seconds\": %.6f, \"steps\": %d, \"mcells_per_s\": %.3f", sec, timed, rate);
  if (ranks > 0) std::printf(", \"ranks\": %d", ranks);
  std::printf("}\n");
}

// --save-res: component c of the whole grid (on the host) as a DAT file and /
// or a BMP image of the middle z slice (3D), the plane (2D) or the line (1D)
template <typename T>
void save_component(const fdtd::Settings& s, const RunConfig& cfg, int c, const std::vector<T>& host, int step) {
  static const char* const names[6] = {"Ex", "Ey", "Ez", "Hx", "Hy", "Hz"};
  const fdtd::Int3& N = cfg.N;
  const std::string base = fdtd::grid_file_name(step, 0, names[c], s.outputDir == "." ? "" : s.outputDir);
  if (s.saveAsDAT) fdtd::write_dat(base + ".dat", host.data(), host.size() * sizeof(T));
  if (s.saveAsBMP || !s.saveAsDAT) {
    const int w = N[0], h = N[1];
    const int kz = cfg.dim == 3 ? N[2] / 2 : 0;
    std::vector<double> v((size_t)w * h);
    for (int i = 0; i < w; ++i)
      for (int j = 0; j < h; ++j) v[(size_t)i * h + j] = host[((size_t)i * N[1] + j) * N[2] + kz];
    fdtd::write_bmp(cfg.dim == 3 ? base + std::to_string(kz) + "-Re.bmp" : base + "-Re.bmp", v, w, h, s.dumperPalette);
  }
}

}  // namespace
