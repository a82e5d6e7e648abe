// C ABI of libfdtd3d_hip (the HIP kernels): prototypes for native callers.
// The Python side binds the same symbols through ctypes (ops/hip_ops.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

extern "C" {
int fdtd_abi_version();

int fdtd_update_e3d_f32(float* ex, float* ey, float* ez, const float* hx, const float* hy, const float* hz,
                        const float* cbx, const float* cby, const float* cbz, double cb, int nx, int ny, int nz,
                        const int* boxes, int xchunk, void* stream);
int fdtd_update_h3d_f32(float* hx, float* hy, float* hz, const float* ex, const float* ey, const float* ez,
                        const float* dbx, const float* dby, const float* dbz, double db, int nx, int ny, int nz,
                        const int* boxes, int xchunk, void* stream);
int fdtd_update_e3d_f64(double* ex, double* ey, double* ez, const double* hx, const double* hy, const double* hz,
                        const double* cbx, const double* cby, const double* cbz, double cb, int nx, int ny, int nz,
                        const int* boxes, int xchunk, void* stream);
int fdtd_update_h3d_f64(double* hx, double* hy, double* hz, const double* ex, const double* ey, const double* ez,
                        const double* dbx, const double* dby, const double* dbz, double db, int nx, int ny, int nz,
                        const int* boxes, int xchunk, void* stream);
int fdtd_update_e3d_v4_f32(float* ex, float* ey, float* ez, const float* hx, const float* hy, const float* hz,
                           const float* cbx, const float* cby, const float* cbz, double cb, int nx, int ny, int nz,
                           const int* boxes, int xchunk, void* stream);
// float4 split E / H updates with the CPML convolution terms folded in
// (yee3d_cpml.hip): cp = 9 x {psi_lo, psi_hi, b, c, 1/kappa - 1} per
// (component, axis), ci = 9 x {lo0, hi0, lo1, hi1}
int fdtd_update_e3d_cpml_v4_f32(float* ex, float* ey, float* ez, const float* hx, const float* hy, const float* hz,
                                const float* cbx, const float* cby, const float* cbz, double cb, int nx, int ny,
                                int nz, const int* boxes, int xchunk, const void* const* cp, const int* ci,
                                void* stream);
int fdtd_update_h3d_cpml_v4_f32(float* hx, float* hy, float* hz, const float* ex, const float* ey, const float* ez,
                                const float* dbx, const float* dby, const float* dbz, double db, int nx, int ny,
                                int nz, const int* boxes, int xchunk, const void* const* cp, const int* ci,
                                void* stream);
// the same on 4-cell double groups
int fdtd_update_e3d_cpml_v4_f64(double* ex, double* ey, double* ez, const double* hx, const double* hy,
                                const double* hz, const double* cbx, const double* cby, const double* cbz, double cb,
                                int nx, int ny, int nz, const int* boxes, int xchunk, const void* const* cp,
                                const int* ci, void* stream);
int fdtd_update_h3d_cpml_v4_f64(double* hx, double* hy, double* hz, const double* ex, const double* ey,
                                const double* ez, const double* dbx, const double* dby, const double* dbz, double db,
                                int nx, int ny, int nz, const int* boxes, int xchunk, const void* const* cp,
                                const int* ci, void* stream);
// fused UPML / Drude chain of the three components of a kind (chain_kernels.hip):
// P = 24 pointers, S = 2 scalars, I = 25 ints per component (layout there)
int fdtd_chain_ints_per_comp();
int fdtd_chain_ptrs_per_comp();
int fdtd_chain3d_f32(const void* const* P, const double* S, const int* I, int drude, int kind_e, int ny, int nz,
                     void* stream);
int fdtd_chain3d_f64(const void* const* P, const double* S, const int* I, int drude, int kind_e, int ny, int nz,
                     void* stream);
// A/B knobs of the non-dispersive chain launches: the float4 form (fp32, full-grid levels; off by
// default), and one component per thread (1, the default) or all three (0); -1 = FDTD3D_CHAIN_SPLIT
void fdtd_set_chain_v4(int on);
void fdtd_set_chain_split(int mode);
// TF/SF: 1D incident line steps and the table-driven corrections
// (generic_kernels.hip; ijk may be null when the box holds every target)
int fdtd_inc_e_f32(float* einc, const float* hinc, int n, double c, double src, void* stream);
int fdtd_inc_e_f64(double* einc, const double* hinc, int n, double c, double src, void* stream);
int fdtd_inc_h_f32(const float* einc, float* hinc, int n, double c, void* stream);
int fdtd_inc_h_f64(const double* einc, double* hinc, int n, double c, void* stream);
int fdtd_tfsf_apply_f32(float* target, const long long* off, const long long* i0, const float* w0, const float* w1,
                        const float* coef, const int* ijk, int n, const float* inc, const int* box, void* stream);
int fdtd_tfsf_apply_f64(double* target, const long long* off, const long long* i0, const double* w0,
                        const double* w1, const double* coef, const int* ijk, int n, const double* inc,
                        const int* box, void* stream);
int fdtd_update_h3d_v4_f32(float* hx, float* hy, float* hz, const float* ex, const float* ey, const float* ez,
                           const float* dbx, const float* dby, const float* dbz, double db, int nx, int ny, int nz,
                           const int* boxes, int xchunk, void* stream);
int fdtd_fused3d_f32(const float* const* ein, const float* const* hin, float* const* eout, float* const* hout,
                     const float* const* cbs, const float* const* dbs, double cb, double db, int nx, int ny, int nz,
                     const int* boxes, int xchunk, long long src_off, int src_comp, double src_val, void* s);
int fdtd_fused3d_f64(const double* const* ein, const double* const* hin, double* const* eout,
                     double* const* hout, const double* const* cbs, const double* const* dbs, double cb, double db,
                     int nx, int ny, int nz, const int* boxes, int xchunk, long long src_off, int src_comp,
                     double src_val, void* s);
int fdtd_fused3d_v4_f32(const float* const* ein, const float* const* hin, float* const* eout, float* const* hout,
                        const float* const* cbs, const float* const* dbs, double cb, double db, int nx, int ny,
                        int nz, const int* boxes, int xchunk, long long src_off, int src_comp, double src_val,
                        void* s);

// Tile options of one blocked 3D pass (yee3d_tb.hip, yee3d_tb64.hip): every
// fdtd_tb3d_* entry point takes them as ``opts``; a null pointer means the
// defaults, a value outside a field's range its default
struct FdtdTbOpts {
  int vec;       // single-row kernel, lane width: 0 = automatic (4 for T <= 2, 2 above), 2, 4
  int rows;      // single-row kernel, rows per wave: 0 = automatic (1), 1, 2
  int xcd;       // single-row kernel, XCD-aware tile order: 0 (default) / 1
  int mrows;     // rows per wave of a plain fp32 pass: 0 = automatic, 1 = the single-row kernel, 2 = multi-row
  int variant;   // multi-row kernel: bit 0 deferred stores, bit 1 two planes prefetched, bit 2 XCD-contiguous
                 // tile order, bit 3 no interior fast path; default 4
  int mr_shape;  // multi-row tiles: 0 = 16 waves x 2 rows, 1 = 8 waves x 4 rows, 2 = 8 waves x 2 rows
  int dr_shape;  // Drude variant tiles: 0 = 8 waves x 2 rows, 1 = 16 waves x 1 row
  int half64;    // fp64 tiles: 1 = two rows of 32 lanes per wave (default), 0 = one row of 64 lanes
};
int fdtd_tb_opts_size();  // sizeof(FdtdTbOpts) (ABI check)
int fdtd_tb3d_v4_f32(const float* const* ein, const float* const* hin, float* const* eout, float* const* hout,
                     const float* const* cbs, const float* const* dbs, double cb, double db, int nx, int ny, int nz,
                     const int* boxes, const int* obox, int xchunk, int steps, const int* src, const double* src_vals,
                     const FdtdTbOpts* opts, void* stream);
int fdtd_tb_max_steps();
int fdtd_tb3d_ext_f32(const float* const* ein, const float* const* hin, float* const* eout, float* const* hout,
                      const void* ce4, const int* ebox, const void* ch4, const int* hbox, double cb, double db,
                      int nx, int ny, int nz, const int* boxes, const int* obox, int xchunk, int steps,
                      const int* src, const double* src_vals, const void* tf, const float* gtab,
                      const FdtdTbOpts* opts, void* stream);
int fdtd_box_pack_f32(float* const* fields, float* buf, int ncomp, int ny, int nz, const int* box, void* s);
int fdtd_box_pack_f64(double* const* fields, double* buf, int ncomp, int ny, int nz, const int* box, void* s);
int fdtd_box_unpack_f32(float* const* fields, const float* buf, int ncomp, int ny, int nz, const int* box, void* s);
int fdtd_box_unpack_f64(double* const* fields, const double* buf, int ncomp, int ny, int nz, const int* box, void* s);
int fdtd_box_xfer_f32(float* const* src, float* const* dst, int ncomp, int ny, int nz, const int* box, void* s);
int fdtd_box_xfer_f64(double* const* src, double* const* dst, int ncomp, int ny, int nz, const int* box, void* s);
int fdtd_tb3d_amp_f32(const float* const* ein, const float* const* hin, float* const* eout, float* const* hout,
                      double cb, double db, int nx, int ny, int nz, const int* boxes, const int* obox, int xchunk,
                      int steps, const int* src, const double* src_vals, float* const* amp, const int* aboxes,
                      double accuracy, unsigned* counts, const FdtdTbOpts* opts, void* stream);
int fdtd_tb3d_drude_f32(const float* const* ein, const float* const* hin, float* const* eout, float* const* hout,
                        double cb, double db, int nx, int ny, int nz, const int* boxes, const int* obox, int xchunk,
                        int steps, const int* src, const double* src_vals, const int* bbox, void* const* sin,
                        void* const* sout, const void* lut, int nid, double cbd, const FdtdTbOpts* opts, void* stream);
int fdtd_tfdev_size();
int fdtd_tfsf_pass_f32(float* einc, float* hinc, int n, double ce, double ch, const double* src_vals, int steps,
                       int reach, int nE, int nH, const int* I0, const float* W0, const float* W1, const float* C,
                       float* gtab, void* stream);
int fdtd_tfsf_table_f32(const float* esrc, const float* hsrc, float* einc, float* hinc, int n, double ce, double ch,
                        const double* src_vals, int steps, int reach, int nE, int nH, const int* I0, const float* W0,
                        const float* W1, const float* C, float* gtab, void* stream);
int fdtd_tb3d_f64(const double* const* ein, const double* const* hin, double* const* eout, double* const* hout,
                  const double* const* cbs, const double* const* dbs, double cb, double db, int nx, int ny, int nz,
                  const int* boxes, const int* obox, int xchunk, int steps, const int* src, const double* src_vals,
                  const FdtdTbOpts* opts, void* stream);
int fdtd_tb3d_drude_f64(const double* const* ein, const double* const* hin, double* const* eout, double* const* hout,
                        double cb, double db, int nx, int ny, int nz, const int* boxes, const int* obox, int xchunk,
                        int steps, const int* src, const double* src_vals, const int* bbox, void* const* sin,
                        void* const* sout, const double* lut, int nid, double cbd, const FdtdTbOpts* opts,
                        void* stream);
int fdtd_tfsf_pass_f64(double* einc, double* hinc, int n, double ce, double ch, const double* src_vals, int steps,
                       int reach, int nE, int nH, const int* I0, const double* W0, const double* W1, const double* C,
                       double* gtab, void* stream);
int fdtd_tfsf_table_f64(const double* esrc, const double* hsrc, double* einc, double* hinc, int n, double ce,
                        double ch, const double* src_vals, int steps, int reach, int nE, int nH, const int* I0,
                        const double* W0, const double* W1, const double* C, double* gtab, void* stream);
int fdtd_tb3d_tf_f64(const double* const* ein, const double* const* hin, double* const* eout, double* const* hout,
                     const double* const* cbs, const double* const* dbs, double cb, double db, int nx, int ny, int nz,
                     const int* boxes, const int* obox, int xchunk, int steps, const int* src,
                     const double* src_vals, const void* tf, const double* gtab, const FdtdTbOpts* opts, void* stream);
int fdtd_tb64_max_steps();
int fdtd_tb2d_f32(int mode, const float* const* ein, const float* const* hin, float* const* eout, float* const* hout,
                  const float* const* cs, double cb, double db, int nx, int ny, const int* boxes, const int* obox,
                  int xchunk, int steps, const int* src, const double* src_vals, void* stream);
int fdtd_tb2d_max_steps();
int fdtd_tb2d_f64(int mode, const double* const* ein, const double* const* hin, double* const* eout,
                  double* const* hout, const double* const* cs, double cb, double db, int nx, int ny, const int* boxes,
                  const int* obox, int xchunk, int steps, const int* src, const double* src_vals, void* stream);
int fdtd_tb2d64_max_steps();
int fdtd_res1d_f32(float* ez, float* hy, const float* cbz, const float* dby, double cb, double db, int n,
                   const int* boxes, int nsteps, int src_i, const float* vals, void* s);
int fdtd_res1d_f64(double* ez, double* hy, const double* cbz, const double* dby, double cb, double db, int n,
                   const int* boxes, int nsteps, int src_i, const double* vals, void* s);
int fdtd_res1d_max_cells(int elem_bytes);

int fdtd_tmz_e_f32(float* ez, const float* hx, const float* hy, const float* cbz, double cb, int nx, int ny,
                   const int* box, int xchunk, void* s);
int fdtd_tmz_h_f32(float* hx, float* hy, const float* ez, const float* dbx, const float* dby, double db, int nx,
                   int ny, const int* boxes, int xchunk, void* s);
int fdtd_tez_e_f32(float* ex, float* ey, const float* hz, const float* cbx, const float* cby, double cb, int nx,
                   int ny, const int* boxes, int xchunk, void* s);
int fdtd_tez_h_f32(float* hz, const float* ex, const float* ey, const float* dbz, double db, int nx, int ny,
                   const int* box, int xchunk, void* s);
int fdtd_1d_e_f32(float* ez, const float* hy, const float* cbz, double cb, int lo, int hi, void* s);
int fdtd_1d_h_f32(float* hy, const float* ez, const float* dby, double db, int lo, int hi, void* s);
int fdtd_tmz_e_f64(double* ez, const double* hx, const double* hy, const double* cbz, double cb, int nx, int ny,
                   const int* box, int xchunk, void* s);
int fdtd_tmz_h_f64(double* hx, double* hy, const double* ez, const double* dbx, const double* dby, double db, int nx,
                   int ny, const int* boxes, int xchunk, void* s);
int fdtd_tez_e_f64(double* ex, double* ey, const double* hz, const double* cbx, const double* cby, double cb, int nx,
                   int ny, const int* boxes, int xchunk, void* s);
int fdtd_tez_h_f64(double* hz, const double* ex, const double* ey, const double* dbz, double db, int nx, int ny,
                   const int* box, int xchunk, void* s);
int fdtd_1d_e_f64(double* ez, const double* hy, const double* cbz, double cb, int lo, int hi, void* s);
int fdtd_1d_h_f64(double* hy, const double* ez, const double* dby, double db, int lo, int hi, void* s);

int fdtd_set_value_f32(float* f, long long off, double v, void* s);
int fdtd_set_value_f64(double* f, long long off, double v, void* s);
int fdtd_set_values_f32(float* f, const long long* offs, int n, double v, void* s);
int fdtd_set_values_f64(double* f, const long long* offs, int n, double v, void* s);

// generic building blocks (generic_kernels.hip): factored coefficients =
// scalar x (px, py, pz, cell) pointers; the 2D UPML chain and the CPML slabs
int fdtd_curl_general_f32(float* out, const float* inp, const float* const* srcs, const int* axes, const int* signs,
                          int nterms, int kind_e, double ca_s, const void* const* ca_p, double cb_s,
                          const void* const* cb_p, int ny, int nz, const int* box, void* s);
int fdtd_curl_general_f64(double* out, const double* inp, const double* const* srcs, const int* axes,
                          const int* signs, int nterms, int kind_e, double ca_s, const void* const* ca_p, double cb_s,
                          const void* const* cb_p, int ny, int nz, const int* box, void* s);
int fdtd_lincomb_f32(float* out, int nterms, const double* scalars, const void* const* ptrs, const float* const* xs,
                     int ny, int nz, const int* box, void* s);
int fdtd_lincomb_f64(double* out, int nterms, const double* scalars, const void* const* ptrs, const double* const* xs,
                     int ny, int nz, const int* box, void* s);
int fdtd_cpml_apply_f32(float* target, const float* src, float* psi, int axis, int sign, int kind_e, const float* bc,
                        const float* cc, const float* kc, double cb_s, const void* const* cb_p, int ny, int nz,
                        const int* box, const int* psi_box, void* s);
int fdtd_cpml_apply_f64(double* target, const double* src, double* psi, int axis, int sign, int kind_e,
                        const double* bc, const double* cc, const double* kc, double cb_s, const void* const* cb_p,
                        int ny, int nz, const int* box, const int* psi_box, void* s);

// amplitude mode (aux_kernels.hip): running maxima of up to 6 components, the
// changed-cell count ADDED to *changed
int fdtd_amplitude_many_f32(const void* const* f, void* const* amp, int ncomp, int ny, int nz, const int* boxes,
                            long long amp_xs, double accuracy, unsigned int* changed, void* s);
int fdtd_amplitude_many_f64(const void* const* f, void* const* amp, int ncomp, int ny, int nz, const int* boxes,
                            long long amp_xs, double accuracy, unsigned int* changed, void* s);

// running DFT monitors (dft_kernels.hip): one sample of every entry of a
// monitor in one launch.  tab = n device entries of fdtd_dft_ent_size() bytes,
// tw = host [2 kinds][K][cos, sin], 1 <= K <= fdtd_dft_max_k()
int fdtd_dft_accum_f32(const void* tab, int n, int nblocks, int K, const double* tw, void* s);
int fdtd_dft_accum_f64(const void* tab, int n, int nblocks, int K, const double* tw, void* s);
int fdtd_dft_ent_size();
int fdtd_dft_max_k();

// Poynting-flux face sums from DFT accumulators (flux_kernels.hip): tab = n
// device entries of fdtd_flux_ent_size() bytes ordered by face, fblk = F + 1
// device ints (first block of every face), partials = nblocks x K doubles of
// scratch, out = F x K doubles
int fdtd_flux_eval_f32(const void* tab, int n, int nblocks, int K, const void* fblk, int F, void* partials, void* out,
                       void* s);
int fdtd_flux_eval_f64(const void* tab, int n, int nblocks, int K, const void* fblk, int F, void* partials, void* out,
                       void* s);
int fdtd_flux_ent_size();

// radiation vectors of the currents on box faces from DFT accumulators
// (farfield_kernels.hip): tab = n device entries of fdtd_farfield_ent_size()
// bytes (face groups), dirs = A x 3 device doubles, wn = K device doubles,
// fold = device ints (7 slot starts, then (partials row, current, sign)),
// partials = rows x K x 4 x A x 2 doubles of scratch, out = K x A x 6 x 2
// doubles
int fdtd_farfield_eval_f32(const void* tab, int n, int nblocks, int K, int A, const void* dirs, const void* wn,
                           double dx, const void* fold, void* partials, void* out, void* s);
int fdtd_farfield_eval_f64(const void* tab, int n, int nblocks, int K, int A, const void* dirs, const void* wn,
                           double dx, const void* fold, void* partials, void* out, void* s);
int fdtd_farfield_ent_size();

// sums of squares over boxes of field arrays (energy_kernels.hip): tab = n
// device entries of fdtd_energy_ent_size() bytes ordered by blk0, a block owns
// rows_blk (x, y) rows of one entry, partials = nblocks doubles of scratch,
// out = R doubles
int fdtd_energy_eval_f32(const void* tab, int n, int nblocks, int rows_blk, int R, void* partials, void* out, void* s);
int fdtd_energy_eval_f64(const void* tab, int n, int nblocks, int rows_blk, int R, void* partials, void* out, void* s);
int fdtd_energy_ent_size();

// one sample of a probe monitor (probe_kernels.hip): tab = nslots device
// entries of fdtd_probe_ent_size() bytes (field array, element offset), series
// = capacity x nslots device doubles; slot s of row `row` = the slot's element
// widened to fp64.  hipErrorInvalidValue for a row outside [0, capacity), a
// negative nslots or a null pointer; nslots == 0 launches nothing
int fdtd_probe_sample_f32(const void* tab, int nslots, void* series, int row, int capacity, void* s);
int fdtd_probe_sample_f64(const void* tab, int nslots, void* series, int row, int capacity, void* s);
int fdtd_probe_ent_size();

// one half step of a source list (source_kernels.hip): tab = n device entries
// of fdtd_source_ent_size() bytes (field array, element offset, fp64
// amplitude, signal index, flags: 1 = same cell as the previous entry, 2 =
// hard) sorted by cell, values = nvalues host doubles, the signals' values at
// this half step.  hipErrorInvalidValue for nvalues outside [0,
// fdtd_source_max_signals()], a negative n or a null pointer; n == 0 launches
// nothing
int fdtd_source_inject_f32(const void* tab, int n, const double* values, int nvalues, void* s);
int fdtd_source_inject_f64(const void* tab, int n, const double* values, int nvalues, void* s);
int fdtd_source_ent_size();
int fdtd_source_max_signals();

// file scenes (scene_kernels.hip): one component's averaged material, quantity 0 = eps, 1 = omega, 2 =
// omega_m, 3 = gamma, 4 = gamma_m, 5 = cond.  side = the quantity's device side table of side_bytes bytes, a
// row per object: none (null, 0) for 0 and 1, triples (gamma_e, omega_m, gamma_m) of fdtd_scene_drude_size()
// bytes, rad/s, for 2 to 4, doubles (S/m) for 5.  ranges (non-null) selects the mesh form and brings tris /
// ntris; without it tris is null and ntris 0.  hipErrorInvalidValue, with nothing launched, for a null
// pointer, another quantity, a side table that is not the quantity's or whose size is not nobj rows
int fdtd_scene_sample(const void* tab, int nobj, int quantity, const int* points, int npts, const int* origin,
                      const int* shape, const int* stride, double mod, int cull, void* out, void* s, const void* side,
                      size_t side_bytes, const void* tris, int ntris, const void* ranges);
int fdtd_scene_drude_size();

// the conductive E update of a lossy box (lossy_kernels.hip): E = ca * E + cb * curl(H) on the three boxes
// (boxes = Ex, Ey, Ez as 6 ints each, local indices) in one launch.  e / h = the three field arrays of
// shape (nx, ny, nz); ca / cb = the three coefficient arrays each, stored over rbox (6 ints, local indices).
// hipErrorInvalidValue, with nothing launched, for a null pointer, a box outside the arrays or rbox, or a box
// whose curl would read index -1.  lanes (may be null) receives the cells a lane owns: 16 bytes' worth when nz
// and rbox's z range are whole lanes and every array is 16-byte aligned, else 1
int fdtd_lossy_e_f32(void* const* e, const void* const* h, const void* const* ca, const void* const* cb, int nx,
                     int ny, int nz, const int* boxes, const int* rbox, void* s, int* lanes);
int fdtd_lossy_e_f64(void* const* e, const void* const* h, const void* const* ca, const void* const* cb, int nx,
                     int ny, int nz, const int* boxes, const int* rbox, void* s, int* lanes);
}
