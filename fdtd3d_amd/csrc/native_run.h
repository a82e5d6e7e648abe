// The single-GPU run of the native driver: one state object whose named
// stages are the set-up (fields and coefficients, absorbing layers, the
// chain regions, sources and modes), the pass plans (blocked, hybrid 3D with
// the Drude box, hybrid 2D), the pass executors (fused step, UPML shell,
// hybrid and blocked passes), the timed run with the amplitude mode, and the
// report -- the counterpart of the reference's single driver
// (Source/main.cpp:36-241 with Scheme3D's init / performSteps) on the same
// kernels and the same plans as the Python driver (models/scheme.py,
// models/blocking.py).
//
// What this class shares with the decomposed runs (native_multi.h) lives in
// native_step.h: the derived configuration (RunConfig), the split half step
// on this run's StepView, the run loop (NTFF and checkpoint cadences), the
// report's common lines, the DAT / BMP writer and the state list.  The chain
// / plain region plan comes from the host runtime (host_native.cpp
// fdtd::chain_regions).
//
// Part of the native driver: included by main.cpp only (one translation unit),
// hence the unnamed namespace.
#pragma once

#include <memory>

namespace {

template <typename T>
class NativeRun {
 public:
  // plane: 0 = the real run, 1 = the imaginary part of a complex run (the
  // cos / zero source; the update is real-linear, so the two parts step
  // independently -- models/scheme.py planes)
  explicit NativeRun(const fdtd::Settings& s_, int plane_ = 0);
  ~NativeRun();
  // set-up, warm-up, timed steps, report, outputs: the process exit status
  int main();
  // the stages of main (a complex run drives two planes through them)
  bool prepare();
  void run_timed();
  void report_run(double extra_sec = 0.0) const { report(sec_ + extra_sec, t_end_, steps_, warm_); }
  double seconds() const { return sec_; }
  int t_end() const { return t_end_; }
  bool save_complex(const NativeRun<T>& im) const;

 private:
  // the shared run loop (native_step.h) drives advance / sync / ntff_fields / save_checkpoint
  template <typename R>
  friend void run_steps(R&, int, int);
  template <typename R>
  friend void run_ckpt(R&, int, int);

  // ------------------------------------------------------------ configuration
  const fdtd::Settings& s;
  RunConfig cfg;  // (percell: this class's own form, see the constructor)
  int plane = 0;
  int t0_ = 0, steps_ = 0, warm_ = 0, t_end_ = 0;
  double sec_ = 0.0;
  bool vacuum, v4, use_fused;
  bool cpml_generic = false;
  hipStream_t st = nullptr;

  // ------------------------------------------------- fields and coefficients
  Dev<T> F[6], G[6], C[6];
  Dev<float> CE4;  // fp32 3D per-cell: sparse E coefficients of the blocked kernel
  int ebox[6] = {0, 0, 0, 0, 0, 0};
  int boxes[36];
  long long src_off = 0;
  T* Fp[6];
  StepView<T> view;  // what the split half steps launch on (native_step.h)

  // ----------------------------------------------------------------- physics
  NativeCpml<T> cpt;
  native_phys::Upml<T> upt;
  Pml2d<T> p2;
  std::vector<IBox> chain_regs, plain_regs;
  std::vector<bool> chain_disp;  // per chain region: holds dispersive cells (the Drude form runs there)
  bool dr_blk = false;
  IBox dr_box = {{0, 0, 0}, {0, 0, 0}};
  NativeTfsf<T> tft;
  std::unique_ptr<Lowdim2d<T>> ld;
  AmpMode<T> ampm;

  // -------------------------------------------------------------- pass plans
  int T_blk = 1, T2_max = 1, T2_blk = 1;
  bool res1 = false;
  int T_h = 1;
  std::vector<IBox> hcores, hshell[8], hcopy;
  Dev<T> DRS[4], DRL;
  int dr_nid = 0, dr_cur = 0;
  double dr_cbd = 0.0;
  int T2_h = 1;
  std::vector<IBox> h2shell[8], h2copy;
  IBox h2core = {{0, 0, 0}, {0, 0, 0}};
  hipStream_t side[2] = {nullptr, nullptr};
  int nstreams = 3;  // shell streams (--shell-streams; 0 = automatic)
  hipEvent_t fork_ev = nullptr, join_ev[2] = {nullptr, nullptr};
  double ckpt_ms = 0.0;

  // ------------------------------------------------------------------ set-up
  void setup_fields();
  void setup_absorbers();
  void setup_chain_regions();
  void plan_drude();
  bool setup_sources_and_modes();
  void plan_blocking();
  void plan_hybrid3d(int T_h_req);
  void setup_drude_state();
  void plan_hybrid2d();
  void setup_streams();

  // ----------------------------------------------------------- helpers
  // (complex runs: the imaginary plane takes the cos / zero source)
  double src_val(int t) const { return cfg.src_val(t, plane); }
  void fptrs();
  template <typename Fn>
  void par_launches(size_t n, Fn&& fn);

  // ------------------------------------------------------- steps and passes
  void step(int t);
  void upml_shell(int kind, const std::vector<IBox>& wins);
  void hybrid_pass(int t, int k);
  void hybrid_shell_step(int q, double sv);
  void hybrid2d_pass(int t);
  void blocked2d_pass(int t, int k);
  void blocked3d_pass(int t);
  void advance(int t0, int n);

  // ----------------------------------------------------------------- run loop
  void sync() { HIP_OK(hipStreamSynchronize(st)); }
  std::array<T*, 6> ntff_fields() const { return {F[0].p, F[1].p, F[2].p, F[3].p, F[4].p, F[5].p}; }
  bool save_checkpoint(int t);
  void report(double sec, int t_end, int steps, int warm) const;
  bool save_results(int t_end);
};

// ============================================================== configuration

template <typename T>
NativeRun<T>::NativeRun(const fdtd::Settings& s_, int plane_) : s(s_), cfg(s_), plane(plane_) {
  // eps = 1 everywhere (a Drude sphere's eps_inf is 1 too: layout/materials.py
  // Scene.eps); this driver also counts the `reference` scene outside 3D
  vacuum = s.scene == "vacuum" || s.scene == "drude-sphere" || (s.scene == "reference" && cfg.dim != 3);
  cfg.percell = !vacuum;
  v4 = sizeof(T) == 4 && cfg.N[2] % 4 == 0 && cfg.dim == 3;
  // fused / blocked / resident kernels unless --split-kernels (3D fused E+H
  // and blocked passes, 2D blocked passes, 1D one-launch resident run)
  // CPML runs step through the 4-cell-lane split kernels with the psi terms
  // folded in; TF/SF runs apply their corrections between the split half steps
  // amplitude mode (Scheme3D.cpp:2945-3333): split kernels for the regular
  // steps (the Python driver's choice), then steps with the running maxima
  // until a step changes none; 3D vacuum fp32 folds them into blocked passes
  use_fused = !s.doUseSplitKernels && !cfg.cpml && !cfg.tfsf && !cfg.upml && !cfg.amp;
  HIP_OK(hipStreamCreate(&st));
}

template <typename T>
NativeRun<T>::~NativeRun() {
  for (int q = 0; q < 2; ++q) {
    if (side[q]) HIP_OK(hipStreamDestroy(side[q]));
    if (join_ev[q]) HIP_OK(hipEventDestroy(join_ev[q]));
  }
  if (fork_ev) HIP_OK(hipEventDestroy(fork_ev));
  if (st) HIP_OK(hipStreamDestroy(st));
}

template <typename T>
void NativeRun<T>::fptrs() {
  for (int c = 0; c < 6; ++c) Fp[c] = F[c].p;
}

// ====================================================================== set-up

// field arrays, the per-cell coefficients of a dielectric scene, the update
// boxes of every component and the point source
template <typename T>
void NativeRun<T>::setup_fields() {
  for (int c = 0; c < 6; ++c)
    if (cfg.present[c]) {
      F[c].alloc(cfg.cells());
      if (use_fused) G[c].alloc(cfg.cells());
    }
  if (cfg.percell) {
    // per-component averaged eps on the eps layout (2-point E averaging,
    // YeeGridLayout.h:1007-1263); mu = 1 -> constant H arrays
    const double ctr[3] = {s.sphereCenterX, s.sphereCenterY, s.sphereCenterZ};
    auto eps_at = [&](int i, int j, int k) {
      return sphere_eps(i + 0.5, j + 0.5, cfg.dim == 3 ? k + 0.5 : ctr[2], ctr, s.sphereRadius, s.sphereEps);
    };
    std::vector<T> host(cfg.cells());
    for (int c = 0; c < 6; ++c) {
      if (!cfg.present[c]) continue;
      for (int i = 0; i < cfg.N[0]; ++i)
        for (int j = 0; j < cfg.N[1]; ++j)
          for (int k = 0; k < cfg.N[2]; ++k) {
            double v;
            if (c < 3) {
              const int di = c == 0, dj = c == 1 && cfg.dim >= 2, dk = c == 2 && cfg.dim == 3;
              v = cfg.cb * 2.0 / (eps_at(i, j, k) + eps_at(i + di, j + dj, k + dk));
            } else {
              v = cfg.db;
            }
            host[((size_t)i * cfg.N[1] + j) * cfg.N[2] + k] = (T)v;
          }
      C[c].alloc(cfg.cells());
      HIP_OK(hipMemcpy(C[c].p, host.data(), cfg.cells() * sizeof(T), hipMemcpyHostToDevice));
    }
    if (sizeof(T) == 4 && cfg.dim == 3) {
      // sparse form for the blocked kernel: the E coefficients of the cells
      // around the sphere (its bounding box + 2 cells; every other cell has
      // eps = 1 on both averaging points, i.e. exactly cb) as one float4 per
      // cell; mu = 1, so H stays on the scalar db
      const fdtd::Box6 sb = sphere_box(s, cfg.N);
      std::copy(sb.begin(), sb.end(), ebox);
      const size_t bn = (size_t)std::max(0, ebox[3] - ebox[0]) * std::max(0, ebox[4] - ebox[1]) *
                        std::max(0, ebox[5] - ebox[2]);
      if (bn > 0) {
        std::vector<float> h4(4 * bn, 0.f);
        size_t q = 0;
        for (int i = ebox[0]; i < ebox[3]; ++i)
          for (int j = ebox[1]; j < ebox[4]; ++j)
            for (int k = ebox[2]; k < ebox[5]; ++k, ++q)
              for (int c = 0; c < 3; ++c) {
                const int di = c == 0, dj = c == 1, dk = c == 2;
                h4[4 * q + c] = (float)(cfg.cb * 2.0 / (eps_at(i, j, k) + eps_at(i + di, j + dj, k + dk)));
              }
        CE4.alloc(4 * bn);
        HIP_OK(hipMemcpy(CE4.p, h4.data(), 4 * bn * sizeof(float), hipMemcpyHostToDevice));
      }
    }
  }
  for (int c = 0; c < 6; ++c) {
    fdtd::Int3 lo, hi;
    fdtd::global_range(c, cfg.N, cfg.active, lo, hi);
    for (int a = 0; a < 3; ++a) {
      boxes[6 * c + a] = lo[a];
      boxes[6 * c + 3 + a] = hi[a];
    }
  }
  src_off = ((long long)cfg.sp[0] * cfg.N[1] + cfg.sp[1]) * cfg.N[2] + cfg.sp[2];
}

// CPML (3D / 2D) and UPML (2D strips, 3D D/B chain with the Drude / Lorentz sphere) tables
template <typename T>
void NativeRun<T>::setup_absorbers() {
  // 3D CPML on rows of a z size not divisible by 4: the scalar split kernels +
  // the generic slab corrections (the 2D form, models/cpml.py)
  cpml_generic = cfg.cpml && cfg.dim == 3 && cfg.N[2] % 4 != 0;
  if (cfg.cpml && cfg.dim == 3 && !cpml_generic) setup_cpml(cpt, s, cfg.N, cfg.active, cfg.dt, cfg.dx);
  if (cpml_generic) setup_cpml2d(p2, s, cfg.N, cfg.active, cfg.present, cfg.dt, cfg.dx);
  if (cfg.dim == 2 && cfg.cpml) setup_cpml2d(p2, s, cfg.N, cfg.active, cfg.present, cfg.dt, cfg.dx);
  if (cfg.dim == 2 && cfg.upml) {
    // per-cell 1 / (eps eps0) of a dielectric scene (E components; the
    // 2-point averages of the plain coefficients above)
    std::vector<T> inv[3];
    const int org[3] = {0, 0, 0};
    if (cfg.percell) inv_eps_2d(s, cfg.present, org, cfg.N.data(), inv);
    setup_upml2d(p2, s, cfg.N, cfg.present, cfg.dt, cfg.dx, inv);
  }
  if (cfg.upml && cfg.dim == 3) native_phys::setup_upml<T>(upt, cfg.N, upml_scene(s, cfg.freq), cfg.dt, cfg.dx);
}

// 3D UPML / Drude: the chain only where it differs from the plain update --
// the PML slabs (one cell of staggering slack) and the dispersive sphere's
// box -- and the plain float4 kernels on the rest (models/scheme.py
// _init_chain_regions; the chain with every sigma and omega zero IS the
// plain update to round-off, and only chain cells read their D levels)
template <typename T>
void NativeRun<T>::setup_chain_regions() {
  if (!(cfg.upml && cfg.dim == 3)) return;
  const fdtd::ChainRegions R = chain_plan(s, cfg.N);
  for (const fdtd::Box6& b : R.chain) chain_regs.push_back(to_ibox(b));
  for (const fdtd::Box6& b : R.plain) plain_regs.push_back(to_ibox(b));
  chain_disp = R.disp;
  // region-local D / D1 levels over the chain regions (models/regions.py)
  native_phys::alloc_levels(upt, R.chain, chain_disp);
}

// Drude box inside the blocked passes (models/blocking.py _plan_drude_blk,
// tb3d_mr.h DrDev, fp64: yee3d_tb64.hip DrDev64): every hybrid pass runs the
// plain blocked core over the box too, then the Drude variant over the box
// grown by T, carrying (delta = D - Dp, Ep) per E component; the stepped
// chain never runs on the box.  3D electric Drude spheres without TF/SF,
// fresh runs (the native checkpoints cover plain media).
template <typename T>
void NativeRun<T>::plan_drude() {
  if (!((v4 || sizeof(T) == 8) && cfg.upml && cfg.dim == 3 && s.doUseMetamaterials && s.blockedDrude != "off" &&
        s.dispersion != "lorentz" && !cfg.tfsf && !cfg.amp && !cfg.percell && !chain_regs.empty() &&
        !plain_regs.empty() &&
        chain_disp.back() && (upt.disp[0] || upt.disp[1] || upt.disp[2]) && !upt.disp[3] && !upt.disp[4] &&
        !upt.disp[5]))
    return;
  dr_blk = true;
  dr_box = chain_regs.back();
  // the ADE rows must be the Drude form (b1 = -(b0 + b2)) and fit the
  // 8-bit ids: checked HERE, before the hybrid plan keeps the box inside
  // the core -- turning the pass off after planning would leave the box on
  // the plain update (no shell window, no copy box covers it)
  for (int c = 0; c < 3 && dr_blk; ++c) {
    if (!upt.disp[c]) continue;
    if (upt.nlut[c] > 256) dr_blk = false;
    std::vector<T> tab(5 * (size_t)upt.nlut[c]);
    HIP_OK(hipMemcpy(tab.data(), upt.lut[c], tab.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (int q = 0; q < upt.nlut[c]; ++q) {
      const double b0 = tab[5 * q], b1 = tab[5 * q + 1], b2 = tab[5 * q + 2];
      if (std::fabs(b0 + b1 + b2) > 1e-5 * (std::fabs(b0) + std::fabs(b1) + std::fabs(b2))) dr_blk = false;
    }
  }
}

// the TF/SF plane wave, the 2D half-step helper and the amplitude mode's state
template <typename T>
bool NativeRun<T>::setup_sources_and_modes() {
  // (per-cell scenes: coefficient arrays for both kinds with the scalar 1)
  const double ce = cfg.percell ? 1.0 : cfg.cb, ch = cfg.percell ? 1.0 : cfg.db;
  if (cfg.tfsf && !setup_tfsf(tft, s, cfg.N, boxes, C, ce, ch, cfg.dt, cfg.dx, cfg.freq, cfg.dim, cfg.present))
    return false;
  // 2D PML half steps and the plain 2D kernels on boxes (native_lowdim.h)
  ld.reset(new Lowdim2d<T>(s, F, C, boxes, cfg.N, cfg.present, p2, cfg.tmz, cfg.percell, cfg.cb, cfg.db, st));
  // amplitude mode state (native_amp.h): running maxima, changed counts, the 3D z-line source
  if (cfg.amp) ampm.init(s, cfg.N, cfg.dim == 3 && cfg.point_src);
  // the split half steps' view of all this (native_step.h)
  view.F = F;
  for (int c = 0; c < 6; ++c) view.C[c] = C[c].p;
  view.ce = ce;
  view.ch = ch;
  for (int a = 0; a < 3; ++a) view.n[a] = cfg.N[a];
  view.boxes = boxes;
  view.v4 = v4;
  view.st = st;
  view.cp = &cpt;
  view.cpml_generic = cpml_generic;
  view.p2 = &p2;
  view.ld = ld.get();
  view.up = &upt;
  view.chain_regs = &chain_regs;
  view.plain_regs = &plain_regs;
  view.chain_disp = &chain_disp;
  view.tf = cfg.tfsf ? &tft : nullptr;
  view.src_off = cfg.point_src ? src_off : -1;
  if (ampm.line_n > 0) {  // the amplitude phase's Ez z line replaces the point source
    view.line_phase = &ampm.active;
    view.line = ampm.LINE.p;
    view.line_n = ampm.line_n;
  }
  return true;
}

// steps per pass of the blocked kernels; the hybrid 3D / 2D plans
template <typename T>
void NativeRun<T>::plan_blocking() {
  // --time-block T: T steps per HBM pass through the blocked kernel
  // 0: automatic (5 steps per pass in fp32, 4 in fp64)
  const int T_req = s.timeBlock <= 0 ? (sizeof(T) == 4 ? 5 : 4) : s.timeBlock;
  const int T_max = sizeof(T) == 4 ? fdtd_tb_max_steps() : fdtd_tb64_max_steps();
  T_blk = (cfg.scheme == "3d" && use_fused && (v4 || sizeof(T) == 8)) ? std::max(1, std::min(T_max, T_req)) : 1;
  // 2D: yee2d_tb.hip passes (automatic 7 steps), rows of whole 16-byte lanes
  T2_max = sizeof(T) == 4 ? fdtd_tb2d_max_steps() : fdtd_tb2d64_max_steps();
  T2_blk = (cfg.dim == 2 && use_fused && cfg.N[1] % (16 / (int)sizeof(T)) == 0)
               ? std::max(1, std::min(T2_max, s.timeBlock <= 0 ? 7 : s.timeBlock))
               : 1;
  // 1D: the whole run in one launch of the register-resident kernel
  res1 = cfg.dim == 1 && use_fused && cfg.N[0] <= fdtd_res1d_max_cells((int)sizeof(T));
  // (fp64: 4 steps per pass, models/blocking.py F64_AUTO_STEPS)
  const int T_h_def = s.hybridBlock == 0 ? (sizeof(T) == 4 ? 5 : 4) : s.hybridBlock;
  if (dr_blk) {
    // (models/blocking.py DRUDE_AUTO_STEPS: the Drude variant holds T - 1 levels in registers)
    const int T_dr = s.hybridBlock > 0 ? s.hybridBlock : (s.timeBlock > 0 ? s.timeBlock : 4);
    if (T_dr > 1 && T_dr <= 5) plan_hybrid3d(T_dr);
    // the Drude pass runs inside hybrid passes only; when it does not fit, the
    // stepped dispersive box cut out of the core at the usual hybrid T
    if (T_dr <= 1 || T_dr > 5 || !dr_blk || T_h <= 1) {
      dr_blk = false;
      T_h = 1;
    }
  }
  if (!dr_blk) plan_hybrid3d(T_h_def);
  if (dr_blk) setup_drude_state();
  plan_hybrid2d();
}

// Hybrid passes for 3D fp32 CPML / UPML / Drude / TF/SF runs -- the plan the
// Python driver picks automatically (models/blocking.py _hybrid_plan): every
// T steps the blocked kernel advances the core (cells at least T + 2 beyond
// every absorbing slab, TF/SF target and stepped dispersive box) by T steps
// F -> G; the shell is stepped in place in F with a band T - s deep into the
// core at step s (stale core values corrupt one band cell per step, so the
// shell itself stays exact), copied into G, and the buffers swap.
template <typename T>
void NativeRun<T>::plan_hybrid3d(int T_h_req) {
  // (UPML runs without dispersive media too: the chain slabs run whole in
  // every shell step, the plain kernels on the windows' inner parts)
  const bool upml_h = cfg.upml && s.doUsePML && !s.doUseMetamaterials && plain_regs.size() == 1;
  // Drude / Lorentz sphere (+ UPML): the dispersive box is cut out of the core
  // (grown by T + 2) and stepped with the shell, chain whole every step
  IBox dbox_h = {{0, 0, 0}, {0, 0, 0}};
  if (cfg.upml && s.doUseMetamaterials && !chain_regs.empty() && !plain_regs.empty()) dbox_h = chain_regs.back();
  const bool drude_h = !dbox_h.empty();
  // TF/SF without absorbing layers: the shell is the TF/SF band on the plain kernels
  const bool tfsf_h = cfg.tfsf && !s.doUsePML && !cfg.upml;
  // (fp32 rows of float4 lanes; fp64: the CPML windows' 4-cell double groups)
  const bool rows_ok = sizeof(T) == 4 ? v4 : cfg.N[2] % 4 == 0;
  const int tb_max = sizeof(T) == 4 ? fdtd_tb_max_steps() : fdtd_tb64_max_steps();
  if (!(cfg.scheme == "3d" && rows_ok && (cfg.cpml || upml_h || drude_h || tfsf_h) && !cfg.percell && !cfg.amp &&
        T_h_req > 1 && T_h_req <= tb_max))
    return;
  const int Th = T_h_req;
  const int pml[3] = {s.doUsePML ? s.pmlSizeX + (cfg.upml ? 1 : 0) : 0,
                      s.doUsePML ? s.pmlSizeY + (cfg.upml ? 1 : 0) : 0,
                      s.doUsePML ? s.pmlSizeZ + (cfg.upml ? 1 : 0) : 0};
  const int tfs[3] = {s.tfsfSizeX, s.tfsfSizeY, s.tfsfSizeZ};
  const IBox alloc = {{0, 0, 0}, {cfg.N[0], cfg.N[1], cfg.N[2]}};
  IBox K;
  for (int a = 0; a < 3; ++a) {
    const int edge = std::max(pml[a], cfg.tfsf ? tfs[a] + 1 : 0);
    // nothing irregular along an axis but the domain border: the core
    // reaches the faces (the blocked kernel handles them itself)
    K.lo[a] = edge > 0 ? edge + Th + 2 : 0;
    K.hi[a] = edge > 0 ? cfg.N[a] - edge - Th - 2 : cfg.N[a];
  }
  auto grow = [&](const IBox& b, int n) {
    IBox g = b;
    for (int a = 0; a < 3; ++a) {
      g.lo[a] -= n;
      g.hi[a] += n;
    }
    return g;
  };
  auto shrink_inner = [&](const IBox& b, int n) {
    IBox r = b;
    for (int a = 0; a < 3; ++a) {
      if (r.lo[a] > 0) r.lo[a] += n;
      if (r.hi[a] < cfg.N[a]) r.hi[a] -= n;
    }
    return r;
  };
  IBox Dm = {{0, 0, 0}, {0, 0, 0}};
  bool ok = !K.empty();
  if (ok && dr_blk) {
    // the Drude pass's output (the box grown by T, clipped to the grid) inside the core
    const IBox g = box_and(grow(dr_box, Th), alloc);
    for (int a = 0; a < 3; ++a) dr_blk = dr_blk && g.lo[a] >= K.lo[a] && g.hi[a] <= K.hi[a];
  }
  if (ok && drude_h && !dr_blk) {
    Dm = box_and(grow(dbox_h, Th + 2), K);
    // the dispersive box runs whole in every shell step: inside every window set
    const IBox KT = shrink_inner(K, Th);
    for (int a = 0; a < 3; ++a) ok = ok && dbox_h.lo[a] >= KT.lo[a] && dbox_h.hi[a] <= KT.hi[a];
  }
  std::vector<IBox> cores;
  if (ok) cores = Dm.empty() ? std::vector<IBox>{K} : box_minus(K, Dm);
  long long vol = 0;
  for (const IBox& b : cores) vol += b.volume();
  if (!(ok && vol >= (long long)cfg.cells() / 4)) return;
  // the shell windows of every step and the copy boxes: the one geometry the
  // Python driver plans too (host_native.cpp fdtd::hybrid_windows)
  auto b6 = [](const IBox& b) { return fdtd::Box6{b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]}; };
  auto ib = [](const fdtd::Box6& b) { return IBox{{b[0], b[1], b[2]}, {b[3], b[4], b[5]}}; };
  const bool act[3] = {true, true, true};
  std::vector<std::vector<fdtd::Box6>> shells;
  std::vector<fdtd::Box6> copy;
  if (!fdtd::hybrid_windows(b6(alloc), b6(K), b6(Dm), Th, act, cfg.N, shells, copy)) return;
  T_h = Th;
  hcores = cores;
  for (int q = 0; q < T_h; ++q) {
    hshell[q].clear();
    for (const auto& w : shells[q]) hshell[q].push_back(ib(w));
  }
  hcopy.clear();
  for (const auto& w : copy) hcopy.push_back(ib(w));
  for (int c = 0; c < 6; ++c)
    if (cfg.present[c] && !G[c].p) G[c].alloc(cfg.cells());
}

// the Drude pass's state (two sets of two float4 arrays over the box; the
// material ids of Ex | Ey << 8 | Ez << 16 in .w of the first) and its
// (b0 cbd, b2, m1, m2) rows per component
template <typename T>
void NativeRun<T>::setup_drude_state() {
  const int bn[3] = {dr_box.hi[0] - dr_box.lo[0], dr_box.hi[1] - dr_box.lo[1], dr_box.hi[2] - dr_box.lo[2]};
  const size_t nb = (size_t)bn[0] * bn[1] * bn[2];
  const double two = 2 * kEps0;
  dr_cbd = (double)(T)((two * cfg.dt / cfg.dx) / two);  // the chain's cbD where sigma = 0
  std::vector<unsigned> ids(nb, 0u);
  for (int c = 0; c < 3; ++c) {
    if (upt.disp[c]) {
      dr_nid = std::max(dr_nid, upt.nlut[c]);
      std::vector<unsigned char> full(cfg.cells());
      HIP_OK(hipMemcpy(full.data(), upt.ids[c], cfg.cells(), hipMemcpyDeviceToHost));
      for (int i = 0; i < bn[0]; ++i)
        for (int j = 0; j < bn[1]; ++j)
          for (int k = 0; k < bn[2]; ++k)
            ids[((size_t)i * bn[1] + j) * bn[2] + k] |=
                (unsigned)full[((size_t)(i + dr_box.lo[0]) * cfg.N[1] + j + dr_box.lo[1]) * cfg.N[2] + k + dr_box.lo[2]]
                << (8 * c);
    } else {
      dr_nid = std::max(dr_nid, 1);  // id 0: the plain row (cb, 0, 1, 0)
    }
  }
  if (dr_nid > 256) {  // excluded before the hybrid plan (plan_drude)
    std::fprintf(stderr, "internal error: Drude LUT of %d rows after planning\n", dr_nid);
    std::exit(3);
  }
  std::vector<T> rows((size_t)3 * dr_nid * 4, T(0));
  for (int c = 0; c < 3; ++c) {
    T* r = rows.data() + (size_t)c * dr_nid * 4;
    if (!upt.disp[c]) {
      r[0] = (T)cfg.cb;
      r[2] = T(1);
      continue;
    }
    std::vector<T> tab(5 * (size_t)upt.nlut[c]);
    HIP_OK(hipMemcpy(tab.data(), upt.lut[c], tab.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (int q = 0; q < upt.nlut[c]; ++q) {
      r[4 * q] = (T)((double)tab[5 * q] * dr_cbd);
      r[4 * q + 1] = tab[5 * q + 2];
      r[4 * q + 2] = tab[5 * q + 3];
      r[4 * q + 3] = tab[5 * q + 4];
    }
  }
  DRL.alloc(rows.size());
  HIP_OK(hipMemcpy(DRL.p, rows.data(), rows.size() * sizeof(T), hipMemcpyHostToDevice));
  // the ids' bits in the first 4 bytes of the fourth element (fp64: its low word)
  std::vector<T> s0(4 * nb, T(0));
  for (size_t e = 0; e < nb; ++e) std::memcpy(&s0[4 * e + 3], &ids[e], 4);
  for (int q = 0; q < 4; ++q) DRS[q].alloc(4 * nb);
  HIP_OK(hipMemcpy(DRS[0].p, s0.data(), s0.size() * sizeof(T), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(DRS[2].p, s0.data(), s0.size() * sizeof(T), hipMemcpyHostToDevice));
}

// 2D hybrid passes (models/blocking.py on yee2d_tb.hip): every T steps the
// 2D blocked kernel advances the core (cells at least T + 2 beyond the
// absorbing strips and the TF/SF targets) F -> G; the shell strips step in
// place in F with a band T - s deep into the core at step s (absorbing
// strips whole), are copied into G, and the buffers swap
template <typename T>
void NativeRun<T>::plan_hybrid2d() {
  if (!(cfg.dim == 2 && (cfg.cpml || (cfg.upml && !s.doUseMetamaterials)) && !cfg.percell && !cfg.amp &&
        !s.doUseSplitKernels && cfg.N[1] % (16 / (int)sizeof(T)) == 0))
    return;
  const int Th = s.hybridBlock == 0 ? 7 : s.hybridBlock;
  if (!(Th > 1 && Th <= T2_max)) return;
  const int pml[2] = {s.pmlSizeX + (cfg.upml ? 1 : 0), s.pmlSizeY + (cfg.upml ? 1 : 0)};
  const int tfs[2] = {s.tfsfSizeX, s.tfsfSizeY};
  IBox K = {{0, 0, 0}, {cfg.N[0], cfg.N[1], 1}};
  for (int a = 0; a < 2; ++a) {
    const int edge = std::max(pml[a], cfg.tfsf ? tfs[a] + 1 : 0);
    K.lo[a] = edge + Th + 2;
    K.hi[a] = cfg.N[a] - edge - Th - 2;
  }
  if (K.empty() || K.volume() < (long long)cfg.cells() / 4) return;
  T2_h = Th;
  h2core = K;
  const IBox alloc = {{0, 0, 0}, {cfg.N[0], cfg.N[1], 1}};
  for (int q = 0; q < T2_h; ++q) {
    IBox Kd = K;
    for (int a = 0; a < 2; ++a) {
      Kd.lo[a] += T2_h - q;
      Kd.hi[a] -= T2_h - q;
    }
    for (const IBox& w : box_minus(alloc, Kd))
      if (!w.empty()) h2shell[q].push_back(w);
  }
  for (const IBox& b : box_minus(alloc, K))
    if (!b.empty()) h2copy.push_back(b);
  for (int c = 0; c < 6; ++c)
    if (cfg.present[c] && !G[c].p) G[c].alloc(cfg.cells());
}

// independent shell-window launches of a half step side by side on three
// streams (the tail of one small launch overlaps the next; models/scheme.py
// _par_launches), joined back into `st`
template <typename T>
void NativeRun<T>::setup_streams() {
  if (T_h <= 1) return;
  nstreams = s.shellStreams > 0 ? std::min(3, s.shellStreams) : 3;
  for (int q = 0; q < 2; ++q) {
    HIP_OK(hipStreamCreateWithFlags(&side[q], hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&join_ev[q], hipEventDisableTiming));
  }
  HIP_OK(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
}

// ===================================================================== helpers

// n independent launches of a half step (disjoint cells; fn(i, stream) issues
// the i-th) round-robin on the three streams, joined back into `st`
// (models/scheme.py _par_launches)
template <typename T>
template <typename Fn>
void NativeRun<T>::par_launches(size_t n, Fn&& fn) {
  if (n <= 1 || !side[0]) {
    for (size_t i = 0; i < n; ++i) fn(i, st);
    return;
  }
  const int ns = nstreams;
  HIP_OK(hipEventRecord(fork_ev, st));
  for (int q = 0; q < ns - 1; ++q) HIP_OK(hipStreamWaitEvent(side[q], fork_ev, 0));
  for (size_t i = 0; i < n; ++i) fn(i, i % ns == 0 ? st : side[i % ns - 1]);
  for (int q = 0; q < ns - 1; ++q) {
    HIP_OK(hipEventRecord(join_ev[q], side[q]));
    HIP_OK(hipStreamWaitEvent(st, join_ev[q], 0));
  }
}

// =========================================================== steps and passes

// one time step (t) through the configured kernels: the fused 3D E+H kernel,
// or the two split half steps (native_step.h)
template <typename T>
void NativeRun<T>::step(int t) {
  const double sv = src_val(t);
  if (cfg.dim == 3 && use_fused) {
    const T* ei[3] = {F[0].p, F[1].p, F[2].p};
    const T* hi[3] = {F[3].p, F[4].p, F[5].p};
    T* eo[3] = {G[0].p, G[1].p, G[2].p};
    T* ho[3] = {G[3].p, G[4].p, G[5].p};
    const T* cbs[3] = {C[0].p, C[1].p, C[2].p};
    const T* dbs[3] = {C[3].p, C[4].p, C[5].p};
    K_OK(fused(ei, hi, eo, ho, cbs, dbs, view.ce, view.ch, cfg.N[0], cfg.N[1], cfg.N[2], boxes, src_off, cfg.src_comp,
               sv, st, v4));
    for (int c = 0; c < 6; ++c) std::swap(F[c].p, G[c].p);
    return;
  }
  split_half(view, cfg, 0, sv);
  split_half(view, cfg, 1, sv);
}


// UPML shell half step: the chain slabs whole (they lie inside every
// step's windows), the plain kernels on the windows' parts in the inner box
// (chain slabs and plain window parts are disjoint: side by side on the
// three streams, as the Python driver's shell -- the float4 plain kernels
// store only their own elements of a 4-cell group that straddles an
// unaligned z border with a chain box; the level rotation is a host pointer
// swap after the launches captured their pointers)
// A thin plain part on the z side of a non-dispersive chain slab with a
// footprint inside the slab's rides in that slab's chain launch (its rows
// are read once, whole; models/scheme.py _chain_plan "fold").
template <typename T>
void NativeRun<T>::upml_shell(int kind, const std::vector<IBox>& wins) {
  fptrs();
  std::vector<std::function<void(hipStream_t)>> fns, pfns;
  std::vector<IBox> parts;
  for (const IBox& w : wins)
    for (const IBox& pr : plain_regs) {
      const IBox b = box_and(w, pr);
      if (!b.empty()) parts.push_back(b);
    }
  std::vector<int> fold(chain_regs.size(), -1);
  std::vector<bool> folded(parts.size(), false);
  for (size_t n = 0; n < parts.size(); ++n) {
    const IBox& b = parts[n];
    if (b.hi[2] - b.lo[2] > 64) continue;
    for (size_t q = 0; q < chain_regs.size(); ++q) {
      const IBox& cr = chain_regs[q];
      if (fold[q] >= 0 || chain_disp[q] || (dr_blk && q + 1 == chain_regs.size())) continue;
      if (b.lo[0] < cr.lo[0] || b.hi[0] > cr.hi[0] || b.lo[1] < cr.lo[1] || b.hi[1] > cr.hi[1]) continue;
      if (b.lo[2] != cr.hi[2] && b.hi[2] != cr.lo[2]) continue;
      fold[q] = (int)n;
      folded[n] = true;
      break;
    }
  }
  for (size_t q = 0; q < chain_regs.size(); ++q) {
    if (dr_blk && q + 1 == chain_regs.size()) continue;  // the Drude box: inside the blocked passes
    fns.push_back([&, q, kind](hipStream_t ss) {
      int rb[36], pb[36];
      clip36(boxes, chain_regs[q], rb);
      if (fold[q] >= 0) clip36(boxes, parts[fold[q]], pb);
      K_OK(native_phys::upml_kind<T>(upt, Fp, rb, kind, cfg.N[1], cfg.N[2], ss, chain3d<T>(), false, !chain_disp[q],
                                     fold[q] >= 0 ? pb : nullptr, kind == 0 ? cfg.cb : cfg.db, (int)q));
    });
  }
  for (size_t n = 0; n < parts.size(); ++n) {
    if (folded[n]) continue;
    const IBox b = parts[n];
    pfns.push_back([&, b, kind](hipStream_t ss) {
      int rb[36];
      clip36(boxes, b, rb);
      if (kind == 0)
        K_OK(e3d(F[0].p, F[1].p, F[2].p, F[3].p, F[4].p, F[5].p, C[0].p, C[1].p, C[2].p, cfg.cb, cfg.N[0], cfg.N[1],
                 cfg.N[2], rb, 0, ss, v4));
      else
        K_OK(h3d(F[3].p, F[4].p, F[5].p, F[0].p, F[1].p, F[2].p, C[3].p, C[4].p, C[5].p, cfg.db, cfg.N[0], cfg.N[1],
                 cfg.N[2], rb + 18, 0, ss, v4));
    });
  }
  fns.insert(fns.end(), pfns.begin(), pfns.end());
  par_launches(fns.size(), [&](size_t i, hipStream_t ss) { fns[i](ss); });
  native_phys::upml_rotate(upt, kind);
}

// one pass of k <= T_h steps (a shorter pass steps the shell windows of the
// pass's last k steps: band depth k - q at step q)
template <typename T>
void NativeRun<T>::hybrid_pass(int t, int k) {
  {
    const T* ei[3] = {F[0].p, F[1].p, F[2].p};
    const T* hi[3] = {F[3].p, F[4].p, F[5].p};
    T* eo[3] = {G[0].p, G[1].p, G[2].p};
    T* ho[3] = {G[3].p, G[4].p, G[5].p};
    const T* none3[3] = {nullptr, nullptr, nullptr};
    double vals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int l = 0; l < k; ++l) vals[l] = src_val(t + l);
    for (const IBox& hc : hcores) {
      bool in_core = true;
      for (int a = 0; a < 3; ++a) in_core = in_core && cfg.sp[a] >= hc.lo[a] && cfg.sp[a] < hc.hi[a];
      const int src[4] = {cfg.sp[0], cfg.sp[1], cfg.sp[2], cfg.point_src && in_core ? cfg.src_comp : -1};
      const int ob[6] = {hc.lo[0], hc.lo[1], hc.lo[2], hc.hi[0], hc.hi[1], hc.hi[2]};
      K_OK(tb3d(ei, hi, eo, ho, none3, none3, cfg.cb, cfg.db, cfg.N[0], cfg.N[1], cfg.N[2], boxes, k, src, vals, st,
                nullptr, nullptr, ob));
    }
    if (dr_blk) {
      // the Drude pass over the box grown by k (overwrites the core pass there)
      int ob[6], bb[6];
      for (int a = 0; a < 3; ++a) {
        ob[a] = std::max(0, dr_box.lo[a] - k);
        ob[3 + a] = std::min(cfg.N[a], dr_box.hi[a] + k);
        bb[a] = dr_box.lo[a];
        bb[3 + a] = dr_box.hi[a];
      }
      const int src[4] = {cfg.sp[0], cfg.sp[1], cfg.sp[2], cfg.point_src ? cfg.src_comp : -1};
      void* sin[2] = {DRS[2 * dr_cur].p, DRS[2 * dr_cur + 1].p};
      void* sout[2] = {DRS[2 * (1 - dr_cur)].p, DRS[2 * (1 - dr_cur) + 1].p};
      K_OK(drude3d(ei, hi, eo, ho, cfg.cb, cfg.db, cfg.N[0], cfg.N[1], cfg.N[2], boxes, ob, k, src, vals, bb, sin,
                   sout, DRL.p, dr_nid, dr_cbd, st));
      dr_cur ^= 1;
    }
    for (int q0 = 0; q0 < k; ++q0) hybrid_shell_step(T_h - k + q0, src_val(t + q0));  // band depth k - q0
    T* src6[6] = {F[0].p, F[1].p, F[2].p, F[3].p, F[4].p, F[5].p};
    T* dst6[6] = {G[0].p, G[1].p, G[2].p, G[3].p, G[4].p, G[5].p};
    for (const IBox& b : hcopy) {
      const int bx[6] = {b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]};
      K_OK(xfer(src6, dst6, 6, cfg.N[1], cfg.N[2], bx, st));
    }
    for (int c = 0; c < 6; ++c) std::swap(F[c].p, G[c].p);
  }
}

// one stepped step of the hybrid shell on window set q, in place in F: the
// two half steps of native_step.h around the shell's own updates (the UPML
// shell, or the plain / folded CPML kernels on the windows side by side)
template <typename T>
void NativeRun<T>::hybrid_shell_step(int q, double sv) {
  const std::vector<IBox>& wins = hshell[q];
  T* const F6[6] = {F[0].p, F[1].p, F[2].p, F[3].p, F[4].p, F[5].p};
  const T* const none6[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int kind = 0; kind < 2; ++kind)
    half_step(view, cfg, kind, sv, [&] {
      if (cfg.upml) {
        upml_shell(kind, wins);
      } else if (!cfg.cpml) {
        par_launches(wins.size(), [&](size_t i, hipStream_t ss) {
          int rb[36];
          clip36(boxes, wins[i], rb);
          if (kind == 0)
            K_OK(e3d(F[0].p, F[1].p, F[2].p, F[3].p, F[4].p, F[5].p, C[0].p, C[1].p, C[2].p, cfg.cb, cfg.N[0],
                     cfg.N[1], cfg.N[2], rb, 0, ss, v4));
          else
            K_OK(h3d(F[3].p, F[4].p, F[5].p, F[0].p, F[1].p, F[2].p, C[3].p, C[4].p, C[5].p, cfg.db, cfg.N[0],
                     cfg.N[1], cfg.N[2], rb + 18, 0, ss, v4));
        });
      } else {
        par_launches(wins.size(), [&](size_t i, hipStream_t ss) {
          int wb2[18];
          clip36(boxes, wins[i], wb2, 3 * kind, 3);
          if (kind == 0)
            K_OK(cpml_e3d(F6, none6, cfg.cb, cfg.N[0], cfg.N[1], cfg.N[2], wb2, cpt.P[0].data(), cpt.I[0].data(), ss));
          else
            K_OK(cpml_h3d(F6, none6, cfg.db, cfg.N[0], cfg.N[1], cfg.N[2], wb2, cpt.P[1].data(), cpt.I[1].data(), ss));
        });
      }
    });
}

template <typename T>
void NativeRun<T>::hybrid2d_pass(int t) {
  const int ord[2][3] = {{2, 3, 4}, {0, 1, 5}};  // TMz Ez Hx Hy, TEz Ex Ey Hz
  const int m = cfg.scheme == "tmz" ? 0 : 1;
  const int* o = ord[m];
  const T* ei[2] = {F[o[0]].p, m ? F[o[1]].p : nullptr};
  const T* hi[2] = {F[m ? o[2] : o[1]].p, m ? nullptr : F[o[2]].p};
  T* eo[2] = {G[o[0]].p, m ? G[o[1]].p : nullptr};
  T* ho[2] = {G[m ? o[2] : o[1]].p, m ? nullptr : G[o[2]].p};
  const T* cs[3] = {C[o[0]].p, C[o[1]].p, C[o[2]].p};
  int b2[18];
  for (int q = 0; q < 3; ++q) std::memcpy(b2 + 6 * q, boxes + 6 * o[q], 6 * sizeof(int));
  const int ob[6] = {h2core.lo[0], h2core.lo[1], 0, h2core.hi[0], h2core.hi[1], 1};
  const bool in_core = cfg.sp[0] >= h2core.lo[0] && cfg.sp[0] < h2core.hi[0] && cfg.sp[1] >= h2core.lo[1] &&
                       cfg.sp[1] < h2core.hi[1];
  const int src[3] = {cfg.sp[0], cfg.sp[1], cfg.point_src && in_core ? (m ? 2 : 0) : -1};
  double vals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int l = 0; l < T2_h; ++l) vals[l] = src_val(t + l);
  K_OK(tb2d(m, ei, hi, eo, ho, cs, cfg.cb, cfg.db, cfg.N[0], cfg.N[1], b2, ob, T2_h, src, vals, st));
  const IBox& inner2 = ld->inner;
  for (int q = 0; q < T2_h; ++q)
    for (int kind = 0; kind < 2; ++kind)
      half_step(view, cfg, kind, src_val(t + q), [&] {
        if (cfg.upml) {
          ld->upml_chain(kind);
          for (const IBox& w : h2shell[q]) ld->plain(kind, box_and(w, inner2));
        } else {
          for (const IBox& w : h2shell[q]) ld->plain(kind, w);
          ld->cpml(kind);
        }
      });
  T* src3[3] = {F[o[0]].p, F[o[1]].p, F[o[2]].p};
  T* dst3[3] = {G[o[0]].p, G[o[1]].p, G[o[2]].p};
  for (const IBox& b : h2copy) {
    const int bx[6] = {b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]};
    K_OK(xfer(src3, dst3, 3, cfg.N[1], cfg.N[2], bx, st));
  }
  for (int q = 0; q < 3; ++q) std::swap(F[o[q]].p, G[o[q]].p);
}

// k <= T2_blk steps of the whole 2D grid in one blocked pass
template <typename T>
void NativeRun<T>::blocked2d_pass(int t, int k) {
  // component order: TMz Ez Hx Hy, TEz Ex Ey Hz
  const int ord[2][3] = {{2, 3, 4}, {0, 1, 5}};
  const int m = cfg.scheme == "tmz" ? 0 : 1;
  const int* o = ord[m];
  const T* ei[2] = {F[o[0]].p, m ? F[o[1]].p : nullptr};
  const T* hi[2] = {F[m ? o[2] : o[1]].p, m ? nullptr : F[o[2]].p};
  T* eo[2] = {G[o[0]].p, m ? G[o[1]].p : nullptr};
  T* ho[2] = {G[m ? o[2] : o[1]].p, m ? nullptr : G[o[2]].p};
  const T* cs[3] = {C[o[0]].p, C[o[1]].p, C[o[2]].p};
  int b2[18];
  for (int q = 0; q < 3; ++q) std::memcpy(b2 + 6 * q, boxes + 6 * o[q], 6 * sizeof(int));
  const int ob[6] = {0, 0, 0, cfg.N[0], cfg.N[1], 1};
  const int src[3] = {cfg.sp[0], cfg.sp[1], m ? 2 : 0};
  double vals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int l = 0; l < k; ++l) vals[l] = src_val(t + l);
  K_OK(tb2d(m, ei, hi, eo, ho, cs, cfg.percell ? 1.0 : cfg.cb, cfg.percell ? 1.0 : cfg.db, cfg.N[0], cfg.N[1], b2, ob,
      k, src, vals, st));
  for (int q = 0; q < 3; ++q) std::swap(F[o[q]].p, G[o[q]].p);
}

// T_blk steps of the whole 3D grid in one blocked pass
template <typename T>
void NativeRun<T>::blocked3d_pass(int t) {
  const T* ei[3] = {F[0].p, F[1].p, F[2].p};
  const T* hi[3] = {F[3].p, F[4].p, F[5].p};
  T* eo[3] = {G[0].p, G[1].p, G[2].p};
  T* ho[3] = {G[3].p, G[4].p, G[5].p};
  const T* cbs[3] = {C[0].p, C[1].p, C[2].p};
  const T* dbs[3] = {C[3].p, C[4].p, C[5].p};
  const int src[4] = {cfg.sp[0], cfg.sp[1], cfg.sp[2], cfg.src_comp};
  double vals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int l = 0; l < T_blk; ++l) vals[l] = src_val(t + l);
  if (CE4.p)
    K_OK(tb3d(ei, hi, eo, ho, cbs, dbs, cfg.cb, cfg.db, cfg.N[0], cfg.N[1], cfg.N[2], boxes, T_blk, src, vals, st,
              CE4.p, ebox));
  else
    K_OK(tb3d(ei, hi, eo, ho, cbs, dbs, cfg.percell ? 1.0 : cfg.cb, cfg.percell ? 1.0 : cfg.db, cfg.N[0], cfg.N[1],
              cfg.N[2], boxes, T_blk, src, vals, st));
  for (int c = 0; c < 6; ++c) std::swap(F[c].p, G[c].p);
}

// n steps from step t0 through the planned passes (hybrid 3D / 2D, blocked,
// the resident 1D run) and single steps for what remains
template <typename T>
void NativeRun<T>::advance(int t0, int n) {
  int t = t0;
  // (with the Drude box in the passes a tail is a shorter pass too: the
  // stepped chain never holds the box's state)
  while (T_h > 1 && (n >= T_h || (dr_blk && n > 0))) {
    const int k = std::min(T_h, n);
    hybrid_pass(t, k);
    t += k;
    n -= k;
  }
  while (T2_h > 1 && n >= T2_h) {
    hybrid2d_pass(t);
    t += T2_h;
    n -= T2_h;
  }
  if (res1 && n > 0) {
    std::vector<T> hv(n);
    for (int l = 0; l < n; ++l) hv[l] = (T)src_val(t + l);
    Dev<T> dv;
    dv.alloc(n);
    HIP_OK(hipMemcpyAsync(dv.p, hv.data(), n * sizeof(T), hipMemcpyHostToDevice, st));
    const int b1[4] = {boxes[12], boxes[15], boxes[24], boxes[27]};
    K_OK(res1d(F[2].p, F[4].p, C[2].p, C[4].p, cfg.percell ? 1.0 : cfg.cb, cfg.percell ? 1.0 : cfg.db, cfg.N[0], b1,
        n, cfg.sp[0], dv.p, st));
    HIP_OK(hipStreamSynchronize(st));  // the table is freed on return
    return;
  }
  while (n > 0) {
    if (T2_blk > 1) {
      const int k = std::min(T2_blk, n);
      blocked2d_pass(t, k);
      t += k;
      n -= k;
    } else if (T_blk > 1 && n >= T_blk) {
      blocked3d_pass(t);
      t += T_blk;
      n -= T_blk;
    } else {
      step(t);
      ++t;
      --n;
    }
  }
}

// ==================================================================== run loop
// (run_steps / run_ckpt of native_step.h: the NTFF and checkpoint cadences)

template <typename T>
bool NativeRun<T>::save_checkpoint(int t) {
  if (ckpt_save<T>(s, cfg.scheme, cfg.N, cfg.present, F, t, cfg.dx, cfg.dt)) return true;
  std::fprintf(stderr, "fdtd3d: cannot write the checkpoint to %s\n", s.checkpointDir.c_str());
  return false;
}

template <typename T>
void NativeRun<T>::report(double sec, int t_end, int steps, int warm) const {
  const int timed = steps - warm + ampm.taken;
  report_head<T>(cfg, sec, ckpt_ms, t_end, timed, warm);
  if (s.doUseComplexFieldValues) std::printf("Complex field values: 1 (real and imaginary planes)\n");
  std::printf("\n-------- Details --------\n");
  std::printf("Parallel grid: 0\n");
  if (T2_h > 1)
    std::printf("Backend: native HIP, hybrid passes (2D blocked core, %d steps per pass; stepped %s%s shell)\n", T2_h,
                cfg.upml ? "UPML" : "CPML", cfg.tfsf ? " + TF/SF" : "");
  else if (T_h > 1)
    std::printf("Backend: native HIP, hybrid passes (blocked core, %d steps per pass; stepped %s%s shell%s)\n", T_h,
                cfg.upml ? "UPML" : (cfg.cpml ? "CPML" : "plain"), cfg.tfsf ? " + TF/SF" : "",
                dr_blk ? "; the Drude box inside the passes" : "");
  else if (T_blk > 1 || T2_blk > 1)
    std::printf("Backend: native HIP, temporally blocked kernel (%d steps per pass)\n", std::max(T_blk, T2_blk));
  else if (res1)
    std::printf("Backend: native HIP, register-resident 1D kernel (one launch per run)\n");
  else if (cfg.cpml || cfg.tfsf || cfg.upml)
    std::printf("Backend: native HIP, split kernels%s%s%s\n", cfg.cpml ? " with the CPML terms folded in" : "",
                cfg.upml ? " with the UPML / dispersive chain" : "", cfg.tfsf ? " + TF/SF corrections" : "");
  else
    std::printf("Backend: native HIP, %s kernels%s\n", use_fused ? "fused E+H" : "split", v4 ? " (float4)" : "");
  report_tail(s, cfg, sec, timed, ampm.taken, ampm.stable, 0);
}

// --save-res (DAT / BMP of the final fields) and the final checkpoint
template <typename T>
bool NativeRun<T>::save_results(int t_end) {
  if (s.doSaveRes) {
    std::vector<T> host(cfg.cells());
    for (int c = 0; c < 6; ++c) {
      if (!cfg.present[c]) continue;
      HIP_OK(hipMemcpy(host.data(), F[c].p, cfg.cells() * sizeof(T), hipMemcpyDeviceToHost));
      save_component(s, cfg, c, host, t_end);
    }
  }
  return s.checkpointDir.empty() || save_checkpoint(t_end);
}

template <typename T>
bool NativeRun<T>::prepare() {
  setup_fields();
  setup_absorbers();
  setup_chain_regions();
  plan_drude();
  if (!setup_sources_and_modes()) return false;
  plan_blocking();
  setup_streams();
  // --load-from-file: the run continues from the checkpoint's step up to --time-steps
  t0_ = 0;
  if (!s.loadFromFile.empty()) {
    const long got = ckpt_load<T>(s, cfg.scheme, cfg.N, cfg.present, F);
    if (got < 0) return false;
    t0_ = (int)got;
  }
  steps_ = std::max(0, s.numTimeSteps - t0_);
  warm_ = std::max(0, std::min(s.warmupSteps, steps_));
  return true;
}

template <typename T>
void NativeRun<T>::run_timed() {
  const int t0 = t0_, steps = steps_, warm = warm_;
  run_ckpt(*this, t0, warm);  // untimed (they advance the simulation)
  HIP_OK(hipStreamSynchronize(st));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  HIP_OK(hipEventRecord(e0, st));
  ckpt_ms = 0.0;  // warm-up checkpoints are outside the timed region anyway
  run_ckpt(*this, t0 + warm, steps - warm);
  // amplitude mode (native_amp.h): after the regular steps, check periods
  // until a step changes no running maximum
  int t_end = t0 + steps;
  if (cfg.amp) {
    // blocked amplitude passes: 3D vacuum fp32 float4 rows, no absorbing layer / TF/SF / NTFF
    const bool blocked = cfg.scheme == "3d" && sizeof(T) == 4 && v4 && !cfg.percell && !cfg.cpml && !cfg.upml &&
                         !cfg.tfsf && !cfg.ntff && ampm.line_n > 0 && !s.doUseSplitKernels;
    t_end = ampm.run(s, cfg.N, cfg.active, cfg.present, boxes, F, G, blocked, cfg.cb, cfg.db, st, t0 + steps,
                     [this](int t) { return src_val(t); }, [this](int t) { step(t); },
                     [this]() { return state_arrays(view, cfg.present); });
  }
  HIP_OK(hipEventRecord(e1, st));
  HIP_OK(hipEventSynchronize(e1));
  HIP_OK(hipGetLastError());
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  HIP_OK(hipEventDestroy(e0));
  HIP_OK(hipEventDestroy(e1));
  sec_ = std::max(0.0, (ms - ckpt_ms) / 1e3);
  t_end_ = t_end;
}

template <typename T>
int NativeRun<T>::main() {
  if (!prepare()) return 1;
  run_timed();
  report_run();
  return save_results(t_end_) ? 0 : 1;
}

// a complex run's outputs (this = the real plane): DAT files of interleaved
// (real, imaginary) values -- the reference's std::complex<T> layout, as
// io/dat.py writes them -- and -Re / -Im / -Mod images of the middle slice
template <typename T>
bool NativeRun<T>::save_complex(const NativeRun<T>& im) const {
  if (!s.doSaveRes) return true;
  const char* names[6] = {"Ex", "Ey", "Ez", "Hx", "Hy", "Hz"};
  std::vector<T> re(cfg.cells()), ip(cfg.cells()), both(2 * cfg.cells());
  for (int c = 0; c < 6; ++c) {
    if (!cfg.present[c]) continue;
    HIP_OK(hipMemcpy(re.data(), F[c].p, cfg.cells() * sizeof(T), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ip.data(), im.F[c].p, cfg.cells() * sizeof(T), hipMemcpyDeviceToHost));
    for (size_t q = 0; q < cfg.cells(); ++q) {
      both[2 * q] = re[q];
      both[2 * q + 1] = ip[q];
    }
    const std::string base = fdtd::grid_file_name(t_end_, 0, names[c], s.outputDir == "." ? "" : s.outputDir);
    if (s.saveAsDAT && !fdtd::write_dat(base + ".dat", both.data(), both.size() * sizeof(T))) return false;
    if (s.saveAsBMP || !s.saveAsDAT) {
      const int w = cfg.N[0], h = cfg.N[1];
      const int kz = cfg.dim == 3 ? cfg.N[2] / 2 : 0;
      std::vector<double> vr((size_t)w * h), vi((size_t)w * h), vm((size_t)w * h);
      for (int i = 0; i < w; ++i)
        for (int j = 0; j < h; ++j) {
          const size_t o = ((size_t)i * cfg.N[1] + j) * cfg.N[2] + kz, q = (size_t)i * h + j;
          vr[q] = re[o];
          vi[q] = ip[o];
          vm[q] = std::sqrt(vr[q] * vr[q] + vi[q] * vi[q]);
        }
      const std::string stem = cfg.dim == 3 ? base + std::to_string(kz) : base;
      fdtd::write_bmp(stem + "-Re.bmp", vr, w, h, s.dumperPalette);
      fdtd::write_bmp(stem + "-Im.bmp", vi, w, h, s.dumperPalette);
      fdtd::write_bmp(stem + "-Mod.bmp", vm, w, h, s.dumperPalette);
    }
  }
  return true;
}

}  // namespace
