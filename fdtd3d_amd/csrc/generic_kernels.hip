// Generic building blocks for the reference-compatible UPML/Drude chain,
// TF/SF injection and the incident 1D line.
//
// The reference runs its UPML as three sweeps per component with per-cell
// virtual material lookups (Scheme3D.cpp:266-416, 1158-1306).  Here every
// coefficient is a factorised product  s * px[i] * py[j] * pz[k] * cell[ijk]
// (fdtd3d_amd/ops/coef.py) precomputed once, and the chain is two kinds of
// one-thread-per-cell launches:
//   curl_general: out = Ca*in + Cb*curl(src)        (D/B update)
//   lincomb:      out = sum_n coef_n * x_n  (n<=5)  (Drude ADE, E-from-D)
// Lanes walk z (contiguous), 4 waves per workgroup walk y.

#include "common.h"

namespace {

template <typename T>
struct Coef3 {
  double s;
  const T* px;
  const T* py;
  const T* pz;
  const T* cell;
};

template <typename T>
__device__ __forceinline__ T coef_at(const Coef3<T>& c, int i, int j, int k, size_t off) {
  T v = (T)c.s;
  if (c.px) v *= c.px[i];
  if (c.py) v *= c.py[j];
  if (c.pz) v *= c.pz[k];
  if (c.cell) v *= c.cell[off];
  return v;
}

template <typename T>
struct Term {
  const T* src;
  int axis;
  int sign;
};

// (j, k) of this thread in the box's y-z plane, k fastest: 256 threads walk
// the flattened plane, so z-thin boxes (the 2D schemes' nz = 1) keep every
// lane busy (grid: cell_grid).
__device__ __forceinline__ bool plane_cell(const Box3& b, int& j, int& k) {
  const unsigned kspan = (unsigned)(b.hi[2] - b.lo[2]);
  const unsigned t = blockIdx.x * 256u + threadIdx.y * 64u + threadIdx.x;
  const unsigned jj = t / kspan;
  j = b.lo[1] + (int)jj;
  k = b.lo[2] + (int)(t - jj * kspan);
  return j < b.hi[1];
}

template <typename T>
__global__ __launch_bounds__(256) void k_curl_general(T* __restrict__ out, const T* __restrict__ inp, Term<T> t0,
                                                      Term<T> t1, int nterms, int kind_e, Coef3<T> ca,
                                                      Coef3<T> cb, int ny, int nz, Box3 b) {
  int j, k;
  if (!plane_cell(b, j, k)) return;
  const int i = b.lo[0] + blockIdx.z;
  const long long stride[3] = {(long long)ny * nz, (long long)nz, 1};
  const size_t off = ((size_t)i * ny + j) * nz + k;
  T acc = 0;
  if (nterms > 0) {
    const long long s = stride[t0.axis];
    const T d = kind_e ? (t0.src[off] - t0.src[off - s]) : (t0.src[off + s] - t0.src[off]);
    acc = t0.sign > 0 ? d : -d;
  }
  if (nterms > 1) {
    const long long s = stride[t1.axis];
    const T d = kind_e ? (t1.src[off] - t1.src[off - s]) : (t1.src[off + s] - t1.src[off]);
    acc = t1.sign > 0 ? acc + d : acc - d;
  }
  out[off] = coef_at(ca, i, j, k, off) * inp[off] + coef_at(cb, i, j, k, off) * acc;
}

template <typename T>
struct LinTerms {
  Coef3<T> c[5];
  const T* x[5];
};

template <typename T>
__global__ __launch_bounds__(256) void k_lincomb(T* __restrict__ out, LinTerms<T> terms, int nterms, int ny,
                                                 int nz, Box3 b) {
  int j, k;
  if (!plane_cell(b, j, k)) return;
  const int i = b.lo[0] + blockIdx.z;
  const size_t off = ((size_t)i * ny + j) * nz + k;
  T v = 0;
#pragma unroll
  for (int n = 0; n < 5; ++n) {
    if (n < nterms) {
      const T t = coef_at(terms.c[n], i, j, k, off) * terms.x[n][off];
      v = (n == 0) ? t : v + t;
    }
  }
  out[off] = v;
}

// TF/SF correction table (fdtd3d_amd/models/tfsf.py): one entry per target
// cell (tables are layered so targets are unique -> no atomics).
template <typename T>
__global__ void k_tfsf_apply(T* __restrict__ target, const long long* __restrict__ off,
                             const long long* __restrict__ i0, const T* __restrict__ w0, const T* __restrict__ w1,
                             const T* __restrict__ coef, const int* __restrict__ ijk, int n,
                             const T* __restrict__ inc, Box3 b) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  if (ijk) {  // null: the box holds every target (no per-entry check, 12 B less per entry)
    const int i = ijk[3 * e], j = ijk[3 * e + 1], k = ijk[3 * e + 2];
    if (!in_box(b, i, j, k)) return;
  }
  const long long p = i0[e];
  target[off[e]] += coef[e] * (w0[e] * inc[p] + w1[e] * inc[p + 1]);
}

// All whole-grid TF/SF tables of one half step in ONE launch (the hybrid
// shell applies its corrections once per half step): up to TFM tables, each
// starting on a fresh block (block-uniform table index), compact entries --
// int32 target offset and line index, the weights folded into the
// coefficient (a0 = coef w0, a1 = coef w1): 16 instead of 28 bytes per fp32
// entry.  Different tables of one launch write different arrays or, for the
// layers of one component, are applied by separate launches (the caller
// groups them), so no two entries of a launch share a target.
constexpr int TFM = 8;

template <typename T>
struct TfMulti {
  T* target[TFM];
  const int* off[TFM];
  const int* i0[TFM];
  const T* a0[TFM];
  const T* a1[TFM];
  int n[TFM];
  int bstart[TFM + 1];
  int count;
};

template <typename T>
__global__ __launch_bounds__(256) void k_tfsf_apply_many(TfMulti<T> m, const T* __restrict__ inc) {
  const int b = blockIdx.x;
  int t = 0;
  while (t + 1 < m.count && b >= m.bstart[t + 1]) ++t;
  const int e = (b - m.bstart[t]) * 256 + threadIdx.x;
  if (e >= m.n[t]) return;
  const int p = m.i0[t][e];
  const int o = m.off[t][e];
  m.target[t][o] += m.a0[t][e] * inc[p] + m.a1[t][e] * inc[p + 1];
}

// Scattered field of a TF/SF run (Scheme3D.cpp:2593-2747): inside the TF box
// the total field minus the incident plane wave, interpolated from the 1D
// line at the component's position (fp64 position and weights, the same
// expression as io/dump.py's torch path), outside the box the field itself.
struct ScatGeom {
  double m[3];     // component offset inside the cell (MIN_COORD_FP)
  double zero[3];  // incident line origin
  double dir[3];   // propagation direction
  double L[3], R[3];
  double proj;     // the component's share of the incident wave
  double shift;    // 0.5 for H (the line's H points sit half a cell later)
  int org[3];      // global index of local cell 0
  int act;         // bit a: axis a bounds the TF box
};

template <typename T>
__global__ __launch_bounds__(256) void k_scattered(const T* __restrict__ f, T* __restrict__ out,
                                                   const T* __restrict__ line, int nline, int nx, int ny, int nz,
                                                   ScatGeom g) {
  // Every operation below is rounded on its own, like the torch expression of
  // io/dump.py: with FMA contraction the position d differs from it by an ulp,
  // which the slope of the line turns into an error far above fp64 rounding
  // (and the interpolation index can flip).  The __dmul_rn / __dadd_rn
  // intrinsics do not prevent that: they are plain operators to the compiler
  // and were contracted like any other (tests/test_aux_gpu.py test_scattered).
#pragma clang fp contract(off)
  const long long n = (long long)nx * ny * nz;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(t % nz);
    const long long r = t / nz;
    const int j = (int)(r % ny);
    const int i = (int)(r / ny);
    const double x = i + g.org[0] + g.m[0], y = j + g.org[1] + g.m[1], z = k + g.org[2] + g.m[2];
    bool inside = true;
    if (g.act & 1) inside = inside && x > g.L[0] && x < g.R[0];
    if (g.act & 2) inside = inside && y > g.L[1] && y < g.R[1];
    if (g.act & 4) inside = inside && z > g.L[2] && z < g.R[2];
    const T v = f[t];
    if (!inside) {
      out[t] = v;
      continue;
    }
    // the same value as the torch expression, so the interpolation index never flips
    double d = ((x - g.zero[0]) * g.dir[0] + (y - g.zero[1]) * g.dir[1]) + (z - g.zero[2]) * g.dir[2];
    d = d - g.shift;
    long long i0 = (long long)floor(d);
    i0 = i0 < 0 ? 0 : (i0 > nline - 2 ? nline - 2 : i0);
    const double w1 = d - (double)i0;
    const double li = (1.0 - w1) * (double)line[i0] + w1 * (double)line[i0 + 1];
    const T inc = (T)(li * g.proj);
    out[t] = v - inc;
  }
}

// 1D incident line (Scheme3D.cpp:25-82)
template <typename T>
__global__ void k_inc_e(T* __restrict__ einc, const T* __restrict__ hinc, int n, T c, double src) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == 0)
    einc[0] = (T)src;
  else
    einc[i] += c * (hinc[i - 1] - hinc[i]);
}

// graph-replayable variant: the source value from a device table (see
// k_set_value_tab in aux_kernels.hip)
template <typename T>
__global__ void k_inc_e_tab(T* __restrict__ einc, const T* __restrict__ hinc, int n, T c,
                            const double* __restrict__ tab, const int* __restrict__ counter, int lag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == 0)
    einc[0] = (T)tab[*counter + lag];
  else
    einc[i] += c * (hinc[i - 1] - hinc[i]);
}

template <typename T>
__global__ void k_inc_h(const T* __restrict__ einc, T* __restrict__ hinc, int n, T c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  hinc[i] += c * (einc[i] - einc[i + 1]);
}

template <typename T>
Coef3<T> coef_from(const double* s, const void* const* p) {
  Coef3<T> c;
  c.s = s[0];
  c.px = (const T*)p[0];
  c.py = (const T*)p[1];
  c.pz = (const T*)p[2];
  c.cell = (const T*)p[3];
  return c;
}

inline dim3 cell_grid(const Box3& b) {
  const long long plane = (long long)(b.hi[1] - b.lo[1]) * (b.hi[2] - b.lo[2]);
  return dim3(cdiv(plane, 256), 1, (unsigned)(b.hi[0] - b.lo[0]));
}

}  // namespace

// terms: srcs[2], axes[2], signs[2]; coefs: scalar + 4 pointers (px, py, pz, cell)
#define FDTD_GENERIC_API(SUF, T)                                                                              \
  FDTD_API int fdtd_curl_general_##SUF(T* out, const T* inp, const T* const* srcs, const int* axes,          \
                                       const int* signs, int nterms, int kind_e, double ca_s,                \
                                       const void* const* ca_p, double cb_s, const void* const* cb_p, int ny, \
                                       int nz, const int* box, void* s) {                                    \
    Box3 b = make_box(box);                                                                                   \
    if (box_empty(b)) return 0;                                                                               \
    Term<T> t0 = {nterms > 0 ? srcs[0] : nullptr, nterms > 0 ? axes[0] : 0, nterms > 0 ? signs[0] : 1};       \
    Term<T> t1 = {nterms > 1 ? srcs[1] : nullptr, nterms > 1 ? axes[1] : 0, nterms > 1 ? signs[1] : 1};       \
    k_curl_general<T><<<cell_grid(b), dim3(64, 4), 0, (hipStream_t)s>>>(                                      \
        out, inp, t0, t1, nterms, kind_e, coef_from<T>(&ca_s, ca_p), coef_from<T>(&cb_s, cb_p), ny, nz, b);    \
    FDTD_RETURN_LAUNCH_STATUS();                                                                              \
  }                                                                                                           \
  FDTD_API int fdtd_lincomb_##SUF(T* out, int nterms, const double* scalars, const void* const* ptrs,         \
                                  const T* const* xs, int ny, int nz, const int* box, void* s) {              \
    Box3 b = make_box(box);                                                                                   \
    if (box_empty(b)) return 0;                                                                               \
    if (nterms < 1 || nterms > 5) return (int)hipErrorInvalidValue;                                           \
    LinTerms<T> lt;                                                                                           \
    for (int n = 0; n < 5; ++n) {                                                                             \
      if (n < nterms) {                                                                                       \
        lt.c[n] = coef_from<T>(scalars + n, ptrs + 4 * n);                                                    \
        lt.x[n] = xs[n];                                                                                      \
      } else {                                                                                                \
        lt.c[n] = Coef3<T>{0.0, nullptr, nullptr, nullptr, nullptr};                                          \
        lt.x[n] = nullptr;                                                                                    \
      }                                                                                                       \
    }                                                                                                         \
    k_lincomb<T><<<cell_grid(b), dim3(64, 4), 0, (hipStream_t)s>>>(out, lt, nterms, ny, nz, b);               \
    FDTD_RETURN_LAUNCH_STATUS();                                                                              \
  }                                                                                                           \
  FDTD_API int fdtd_tfsf_apply_many_##SUF(void* const* P, const int* N, int count, const T* inc, void* s) {    \
    if (count <= 0) return 0;                                                                                 \
    if (count > TFM) return (int)hipErrorInvalidValue;                                                        \
    TfMulti<T> m;                                                                                             \
    int blocks = 0;                                                                                           \
    for (int t = 0; t < TFM; ++t) {                                                                           \
      const bool on = t < count;                                                                              \
      m.target[t] = on ? (T*)P[5 * t] : nullptr;                                                              \
      m.off[t] = on ? (const int*)P[5 * t + 1] : nullptr;                                                     \
      m.i0[t] = on ? (const int*)P[5 * t + 2] : nullptr;                                                      \
      m.a0[t] = on ? (const T*)P[5 * t + 3] : nullptr;                                                        \
      m.a1[t] = on ? (const T*)P[5 * t + 4] : nullptr;                                                        \
      m.n[t] = on ? N[t] : 0;                                                                                 \
      m.bstart[t] = blocks;                                                                                   \
      if (on) blocks += (int)cdiv(N[t], 256);                                                                 \
    }                                                                                                         \
    m.bstart[TFM] = blocks;                                                                                   \
    m.count = count;                                                                                          \
    if (blocks == 0) return 0;                                                                                \
    k_tfsf_apply_many<T><<<blocks, 256, 0, (hipStream_t)s>>>(m, inc);                                         \
    FDTD_RETURN_LAUNCH_STATUS();                                                                              \
  }                                                                                                           \
  FDTD_API int fdtd_tfsf_apply_##SUF(T* target, const long long* off, const long long* i0, const T* w0,      \
                                     const T* w1, const T* coef, const int* ijk, int n, const T* inc,         \
                                     const int* box, void* s) {                                               \
    Box3 b = make_box(box);                                                                                   \
    if (n <= 0 || box_empty(b)) return 0;                                                                     \
    k_tfsf_apply<T><<<cdiv(n, 256), 256, 0, (hipStream_t)s>>>(target, off, i0, w0, w1, coef, ijk, n, inc, b);  \
    FDTD_RETURN_LAUNCH_STATUS();                                                                              \
  }                                                                                                           \
  FDTD_API int fdtd_scattered_##SUF(const T* f, T* out, const T* line, int nline, int nx, int ny, int nz,      \
                                    const double* geo, const int* igeo, void* s) {                            \
    ScatGeom g;                                                                                               \
    for (int a = 0; a < 3; ++a) {                                                                             \
      g.m[a] = geo[a];                                                                                        \
      g.zero[a] = geo[3 + a];                                                                                 \
      g.dir[a] = geo[6 + a];                                                                                  \
      g.L[a] = geo[9 + a];                                                                                    \
      g.R[a] = geo[12 + a];                                                                                   \
      g.org[a] = igeo[a];                                                                                     \
    }                                                                                                         \
    g.proj = geo[15];                                                                                         \
    g.shift = geo[16];                                                                                        \
    g.act = igeo[3];                                                                                          \
    const long long n = (long long)nx * ny * nz;                                                              \
    if (n <= 0) return 0;                                                                                     \
    if (nline < 2) return (int)hipErrorInvalidValue;                                                          \
    const long long blocks = (n + 255) / 256;                                                                 \
    k_scattered<T><<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, (hipStream_t)s>>>(f, out, line, nline, \
                                                                                            nx, ny, nz, g);   \
    FDTD_RETURN_LAUNCH_STATUS();                                                                              \
  }                                                                                                           \
  FDTD_API int fdtd_inc_e_##SUF(T* einc, const T* hinc, int n, double c, double src, void* s) {               \
    k_inc_e<T><<<cdiv(n, 256), 256, 0, (hipStream_t)s>>>(einc, hinc, n, (T)c, src);                           \
    FDTD_RETURN_LAUNCH_STATUS();                                                                              \
  }                                                                                                           \
  FDTD_API int fdtd_inc_e_tab_##SUF(T* einc, const T* hinc, int n, double c, const double* tab,               \
                                   const int* counter, int lag, void* s) {                                    \
    k_inc_e_tab<T><<<cdiv(n, 256), 256, 0, (hipStream_t)s>>>(einc, hinc, n, (T)c, tab, counter, lag);          \
    FDTD_RETURN_LAUNCH_STATUS();                                                                              \
  }                                                                                                           \
  FDTD_API int fdtd_inc_h_##SUF(const T* einc, T* hinc, int n, double c, void* s) {                           \
    k_inc_h<T><<<cdiv(n, 256), 256, 0, (hipStream_t)s>>>(einc, hinc, n, (T)c);                                 \
    FDTD_RETURN_LAUNCH_STATUS();                                                                              \
  }

FDTD_GENERIC_API(f32, float)
FDTD_GENERIC_API(f64, double)

// ---------------------------------------------------------------------------
// CPML slab correction (fdtd3d_amd/models/cpml.py): psi = b psi + c dS;
// F += Cb * sign * ((1/kappa - 1) dS + psi).  One thread per slab cell.
namespace {
template <typename T>
__global__ __launch_bounds__(256) void k_cpml(T* __restrict__ target, const T* __restrict__ src,
                                              T* __restrict__ psi, int axis, int sign, int kind_e,
                                              const T* __restrict__ bc, const T* __restrict__ cc,
                                              const T* __restrict__ kc, Coef3<T> cb, int ny, int nz, Box3 b,
                                              Box3 pb) {
  int j, k;
  if (!plane_cell(b, j, k)) return;
  const int i = b.lo[0] + blockIdx.z;
  const long long stride[3] = {(long long)ny * nz, (long long)nz, 1};
  const size_t off = ((size_t)i * ny + j) * nz + k;
  const long long s = stride[axis];
  const T d = kind_e ? (src[off] - src[off - s]) : (src[off + s] - src[off]);
  const int pny = pb.hi[1] - pb.lo[1], pnz = pb.hi[2] - pb.lo[2];
  const size_t poff = ((size_t)(i - pb.lo[0]) * pny + (j - pb.lo[1])) * pnz + (k - pb.lo[2]);
  const int n = axis == 0 ? i : (axis == 1 ? j : k);
  const T ps = bc[n] * psi[poff] + cc[n] * d;
  psi[poff] = ps;
  const T corr = kc[n] * d + ps;
  target[off] += coef_at(cb, i, j, k, off) * (sign > 0 ? corr : -corr);
}

// Up to 8 CPML slab corrections of one half step in ONE launch (the 2D hybrid
// shell replays ~30 small launches a step from a HIP graph, so a step costs
// its launch count; profiles/graph2d_r4.md): blocks numbered slab by slab,
// each slab the k_cpml grid (plane blocks x x planes) of its box.
constexpr int CPML_MANY = 8;
template <typename T>
struct CpmlOne {
  T* target;
  const T* src;
  T* psi;
  const T* bc;
  const T* cc;
  const T* kc;
  Coef3<T> cb;
  Box3 b, pb;
  int axis, sign, gpl;  // gpl: plane blocks of b
};
template <typename T>
struct CpmlMany {
  CpmlOne<T> e[CPML_MANY];
  int start[CPML_MANY + 1];
  int n, kind_e, ny, nz;
};

template <typename T>
__global__ __launch_bounds__(256) void k_cpml_many(CpmlMany<T> M) {
  const int id = (int)blockIdx.x;
  int q = 0;
#pragma unroll
  for (int r = 1; r < CPML_MANY; ++r) q += (r < M.n && id >= M.start[r]) ? 1 : 0;
  const CpmlOne<T>& E = M.e[q];
  const int loc = id - M.start[q];
  const int bxi = loc % E.gpl, pl = loc / E.gpl;
  const unsigned kspan = (unsigned)(E.b.hi[2] - E.b.lo[2]);
  const unsigned t = (unsigned)bxi * 256u + threadIdx.y * 64u + threadIdx.x;
  const unsigned jj = t / kspan;
  const int j = E.b.lo[1] + (int)jj, k = E.b.lo[2] + (int)(t - jj * kspan);
  if (j >= E.b.hi[1]) return;
  const int i = E.b.lo[0] + pl;
  const int ny = M.ny, nz = M.nz;
  const long long stride[3] = {(long long)ny * nz, (long long)nz, 1};
  const size_t off = ((size_t)i * ny + j) * nz + k;
  const long long s = stride[E.axis];
  const T d = M.kind_e ? (E.src[off] - E.src[off - s]) : (E.src[off + s] - E.src[off]);
  const int pny = E.pb.hi[1] - E.pb.lo[1], pnz = E.pb.hi[2] - E.pb.lo[2];
  const size_t poff = ((size_t)(i - E.pb.lo[0]) * pny + (j - E.pb.lo[1])) * pnz + (k - E.pb.lo[2]);
  const int n = E.axis == 0 ? i : (E.axis == 1 ? j : k);
  const T ps = E.bc[n] * E.psi[poff] + E.cc[n] * d;
  E.psi[poff] = ps;
  const T corr = E.kc[n] * d + ps;
  E.target[off] += coef_at(E.cb, i, j, k, off) * (E.sign > 0 ? corr : -corr);
}
}  // namespace

// n <= 8 slabs of one kind: per slab P[6 q ..] = target src psi bc cc kc (+ 4 coef pointers at
// CP[4 q ..]), S[q] = coefficient scalar, I[14 q ..] = axis sign box[6] psi_box[6]
#define FDTD_CPML_MANY_API(SUF, T)                                                                            \
  FDTD_API int fdtd_cpml_apply_many_##SUF(void* const* P, const void* const* CP, const double* S,            \
                                          const int* I, int n, int kind_e, int ny, int nz, void* s) {         \
    if (n < 0 || n > CPML_MANY) return (int)hipErrorInvalidValue;                                            \
    CpmlMany<T> M;                                                                                            \
    M.n = 0;                                                                                                  \
    M.start[0] = 0;                                                                                           \
    M.kind_e = kind_e;                                                                                        \
    M.ny = ny;                                                                                                \
    M.nz = nz;                                                                                                \
    for (int q = 0; q < n; ++q) {                                                                             \
      const Box3 b = make_box(I + 14 * q + 2);                                                                \
      if (box_empty(b)) continue;                                                                             \
      CpmlOne<T>& E = M.e[M.n];                                                                               \
      E.target = (T*)P[6 * q];                                                                                \
      E.src = (const T*)P[6 * q + 1];                                                                         \
      E.psi = (T*)P[6 * q + 2];                                                                               \
      E.bc = (const T*)P[6 * q + 3];                                                                          \
      E.cc = (const T*)P[6 * q + 4];                                                                          \
      E.kc = (const T*)P[6 * q + 5];                                                                          \
      E.cb = coef_from<T>(S + q, CP + 4 * q);                                                                 \
      E.b = b;                                                                                                \
      E.pb = make_box(I + 14 * q + 8);                                                                        \
      E.axis = I[14 * q];                                                                                     \
      E.sign = I[14 * q + 1];                                                                                 \
      const dim3 g = cell_grid(b);                                                                            \
      E.gpl = (int)g.x;                                                                                       \
      M.start[M.n + 1] = M.start[M.n] + (int)(g.x * g.z);                                                     \
      ++M.n;                                                                                                  \
    }                                                                                                         \
    for (int q = M.n; q < CPML_MANY; ++q) M.start[q + 1] = M.start[M.n];                                      \
    if (M.start[M.n] == 0) return 0;                                                                          \
    k_cpml_many<T><<<(unsigned)M.start[M.n], dim3(64, 4), 0, (hipStream_t)s>>>(M);                            \
    FDTD_RETURN_LAUNCH_STATUS();                                                                              \
  }
FDTD_CPML_MANY_API(f32, float)
FDTD_CPML_MANY_API(f64, double)

#define FDTD_CPML_API(SUF, T)                                                                                 \
  FDTD_API int fdtd_cpml_apply_##SUF(T* target, const T* src, T* psi, int axis, int sign, int kind_e,         \
                                     const T* bc, const T* cc, const T* kc, double cb_s,                      \
                                     const void* const* cb_p, int ny, int nz, const int* box,                \
                                     const int* psi_box, void* s) {                                           \
    Box3 b = make_box(box), pb = make_box(psi_box);                                                           \
    if (box_empty(b)) return 0;                                                                               \
    k_cpml<T><<<cell_grid(b), dim3(64, 4), 0, (hipStream_t)s>>>(target, src, psi, axis, sign, kind_e, bc, cc, \
                                                                kc, coef_from<T>(&cb_s, cb_p), ny, nz, b, pb);  \
    FDTD_RETURN_LAUNCH_STATUS();                                                                              \
  }
FDTD_CPML_API(f32, float)
FDTD_CPML_API(f64, double)
