// Running discrete Fourier transform of field samples (models/dft.py): per
// monitored cell and frequency k two accumulators, re[k] += f cos(w_k t) and
// im[k] += f sin(w_k t).  ONE launch per sample covers every entry of a
// monitor (the NTFF surface alone is 24 thin slabs), in the style of
// aux_kernels.hip k_box_list: a device table of fixed-size entries, the
// block's entry by binary search over blk0, table reads through the constant
// address space.
//
// An entry's accumulators are box-local, [k][re|im][x][y][z'], with the z'
// extent padded to the field's 16-byte groups (z from lo & ~(V - 1) to hi
// rounded up, V = 4 fp32 / 2 fp64), so an accumulator vector and the field
// vector it belongs to start at the same z.  A thread owns one such group:
// it loads the field once, loads its 2K accumulator vectors, and only then
// stores them back (the stores could alias the loads, which would serialise
// 2K memory round trips).  Cells of a group outside the box are masked: never
// written, so they stay zero.  No atomics, no LDS: 1 read + 2K
// read-modify-writes per cell.
//
// The twiddles (2 kinds -- E and H sample times differ -- x K x (cos, sin))
// are computed by the host in fp64 once per sample and passed BY VALUE in the
// kernel arguments, so they sit in SGPRs.
#include "common.h"
#include "monitor_dev.h"

namespace {

constexpr int DFT_MAX_K = 8;

struct DftEnt {
  long long f;    // field array base (its dims: ny x nz per x plane)
  long long acc;  // this entry's accumulators, 16-byte aligned
  int ny, nz;
  int lo[3], hi[3];  // the box, array-local
  int blk0;          // first block of the entry
  int kind;          // 0 = E, 1 = H (selects the twiddle row)
  int vec;           // field rows are whole aligned 16-byte groups: vector field loads
  int pad;
};
static_assert(sizeof(DftEnt) == 64, "DftEnt layout (ops/dft.py DFT_ENT_SIZE)");

template <typename T, int K>
struct DftTw {
  T c[2][K];
  T s[2][K];
};

template <typename T, int K, bool VEC>
__device__ __forceinline__ void dft_entry(const DftEnt& e, int blk, const DftTw<T, K>& tw) {
  constexpr int V = 16 / sizeof(T);
  typedef T VT __attribute__((ext_vector_type(V)));
  const int z0 = e.lo[2] & ~(V - 1);
  const int zg = ((e.hi[2] + V - 1) / V * V - z0) / V;  // 16-byte groups per row
  const int by = e.hi[1] - e.lo[1];
  const int n = (e.hi[0] - e.lo[0]) * by * zg;
  const int idx = blk * 256 + (int)threadIdx.x;  // in groups
  if (idx >= n) return;
  const int kv = idx % zg, jj = idx / zg;
  const int j = jj % by, i = jj / by;
  const int kb = z0 + kv * V;
  unsigned m = 0;
#pragma unroll
  for (int l = 0; l < V; ++l) m |= (kb + l >= e.lo[2] && kb + l < e.hi[2]) ? (1u << l) : 0u;
  const T* F = (const T*)e.f;
  const size_t foff = ((size_t)(e.lo[0] + i) * e.ny + (e.lo[1] + j)) * e.nz + kb;
  VT f;
  if (VEC) {
    // nz % V == 0 and kb % V == 0: the whole group lies in the row
    f = *reinterpret_cast<const VT*>(F + foff);
  } else {
#pragma unroll
    for (int l = 0; l < V; ++l) f[l] = ((m >> l) & 1u) ? F[foff + l] : T(0);
  }
  const size_t plane = (size_t)n * V;  // elements of one [x][y][z'] block
  T* A = (T*)e.acc + (size_t)idx * V;
  VT re[K], im[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    re[k] = *reinterpret_cast<const VT*>(A + (size_t)(2 * k) * plane);
    im[k] = *reinterpret_cast<const VT*>(A + (size_t)(2 * k + 1) * plane);
  }
  const bool h = e.kind != 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const T c = h ? tw.c[1][k] : tw.c[0][k];
    const T s = h ? tw.s[1][k] : tw.s[0][k];
    re[k] += f * c;
    im[k] += f * s;
  }
  constexpr unsigned FULL = (1u << V) - 1u;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T* pr = A + (size_t)(2 * k) * plane;
    T* pi = A + (size_t)(2 * k + 1) * plane;
    if (m == FULL) {
      *reinterpret_cast<VT*>(pr) = re[k];
      *reinterpret_cast<VT*>(pi) = im[k];
    } else {
#pragma unroll
      for (int l = 0; l < V; ++l)
        if ((m >> l) & 1u) {
          pr[l] = re[k][l];
          pi[l] = im[k][l];
        }
    }
  }
}

template <typename T, int K>
__global__ __launch_bounds__(256) void k_dft_accum(const DftEnt* __restrict__ tab, int n, DftTw<T, K> tw) {
  // the block's entry: binary search over blk0 (monitor_dev.h)
  const mon::ConstTab<DftEnt> E = (mon::ConstTab<DftEnt>)tab;
  const int b = (int)blockIdx.x;
  const int lo = mon::entry_of_block(tab, n, b);
  DftEnt e;  // (field by field: the constant-address-space entry has no implicit copy)
  e.f = E[lo].f;
  e.acc = E[lo].acc;
  e.ny = E[lo].ny;
  e.nz = E[lo].nz;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    e.lo[d] = E[lo].lo[d];
    e.hi[d] = E[lo].hi[d];
  }
  e.blk0 = E[lo].blk0;
  e.kind = E[lo].kind;
  e.vec = E[lo].vec;
  if (e.vec)
    dft_entry<T, K, true>(e, b - e.blk0, tw);
  else
    dft_entry<T, K, false>(e, b - e.blk0, tw);
}

template <typename T, int K>
int dft_launch(const void* tab, int n, int nblocks, const double* tw, hipStream_t s) {
  DftTw<T, K> t;
  for (int kd = 0; kd < 2; ++kd)
    for (int k = 0; k < K; ++k) {
      t.c[kd][k] = (T)tw[(kd * K + k) * 2];
      t.s[kd][k] = (T)tw[(kd * K + k) * 2 + 1];
    }
  k_dft_accum<T, K><<<nblocks, 256, 0, s>>>((const DftEnt*)tab, n, t);
  FDTD_RETURN_LAUNCH_STATUS();
}

template <typename T>
int dft_accum(const void* tab, int n, int nblocks, int K, const double* tw, hipStream_t s) {
  if (n <= 0 || nblocks <= 0) return 0;
  if (K < 1 || K > DFT_MAX_K || !tab || !tw) return (int)hipErrorInvalidValue;
  switch (K) {
    case 1: return dft_launch<T, 1>(tab, n, nblocks, tw, s);
    case 2: return dft_launch<T, 2>(tab, n, nblocks, tw, s);
    case 3: return dft_launch<T, 3>(tab, n, nblocks, tw, s);
    case 4: return dft_launch<T, 4>(tab, n, nblocks, tw, s);
    case 5: return dft_launch<T, 5>(tab, n, nblocks, tw, s);
    case 6: return dft_launch<T, 6>(tab, n, nblocks, tw, s);
    case 7: return dft_launch<T, 7>(tab, n, nblocks, tw, s);
    default: return dft_launch<T, 8>(tab, n, nblocks, tw, s);
  }
}

}  // namespace

// One sample of a monitor: `tab` = n device entries of fdtd_dft_ent_size()
// bytes (nblocks = the last entry's blk0 + its blocks), `tw` = host array
// [2 kinds][K][cos, sin] in fp64, 1 <= K <= 8.
FDTD_API int fdtd_dft_accum_f32(const void* tab, int n, int nblocks, int K, const double* tw, void* s) {
  return dft_accum<float>(tab, n, nblocks, K, tw, (hipStream_t)s);
}
FDTD_API int fdtd_dft_accum_f64(const void* tab, int n, int nblocks, int K, const double* tw, void* s) {
  return dft_accum<double>(tab, n, nblocks, K, tw, (hipStream_t)s);
}
FDTD_API int fdtd_dft_ent_size() { return (int)sizeof(DftEnt); }
FDTD_API int fdtd_dft_max_k() { return DFT_MAX_K; }
