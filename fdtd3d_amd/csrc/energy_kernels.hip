// Sums of squares of field samples over boxes (models/energy.py): per result
// row the sum over the cells of its boxes of f^2.  ONE launch covers every
// box of a monitor, in the style of dft_kernels.hip and flux_kernels.hip: a
// device table of fixed-size entries (one box of one field array), the
// block's entry by binary search over blk0, table reads through the constant
// address space.  Several entries may add to the same result row.
//
// Lanes run along z in aligned 16-byte groups (float4 / double2): a row of a
// box is the groups from lo & ~(V - 1) to hi rounded up, and the elements of
// the first and last group outside the box are masked.  A block owns rows_blk
// consecutive (x, y) rows of one entry (chosen by the host: the whole grid at
// 1024^3 stays at a few hundred thousand partials), its 256 threads walk the
// rows' groups 4 at a time so that 4 loads are in flight per lane.  Entries
// whose aligned groups the host could not prove inside the allocation
// (vec = 0) load their owned elements one by one.
//
// Every element is converted to fp64 before it is squared and added (fp32
// runs too).  The block's sum is reduced within the wave by shuffles, across
// its 4 waves through LDS in a fixed order, and written with a plain store to
// partials[block]; a second small launch folds the partials of each result
// row in a fixed order.  No atomics: the same input gives the same bits.
//
// The kernel checks nothing beyond the box: the host verifies every entry
// against its tensor (ops/hip_monitors.py field_sumsq).
#include "common.h"
#include "monitor_dev.h"

namespace {

constexpr int EN_BLOCK = 256;
constexpr int EN_WAVES = EN_BLOCK / 64;
constexpr int EN_UNROLL = 4;

struct EnergyEnt {
  long long f;   // element (0, 0, 0) of the field array
  int sx, sy;    // x and y strides in elements (z stride 1)
  int lo[3];     // first cell of the box, array-local
  int ext[3];    // cells of the box per axis
  int row;       // row of the result
  int blk0;      // first block of the entry
  int nblk;      // blocks of the entry
  int vec;       // aligned 16-byte groups lie inside the allocation: vector loads
  int pad[2];
};
static_assert(sizeof(EnergyEnt) == 64, "EnergyEnt layout (ops/energy.py ENERGY_ENT_SIZE)");

// the block's sum of v in thread 0 (fixed order)
__device__ __forceinline__ double energy_block_sum(double v, double* red) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  v = mon::wave_sum(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < EN_WAVES; ++w) s += red[w];
  return s;
}

template <typename T, bool VEC>
__device__ __forceinline__ double energy_rows(const EnergyEnt& e, int q0, int rows) {
  constexpr int V = 16 / sizeof(T);
  typedef T VT __attribute__((ext_vector_type(V)));
  const int z0 = e.lo[2] & ~(V - 1);
  const int hi = e.lo[2] + e.ext[2];
  const int zg = ((hi + V - 1) / V * V - z0) / V;  // 16-byte groups per row
  const int ng = rows * zg;
  const T* F = (const T*)e.f;
  double acc[V];
#pragma unroll
  for (int l = 0; l < V; ++l) acc[l] = 0.0;
  for (int g0 = (int)threadIdx.x; g0 < ng; g0 += EN_BLOCK * EN_UNROLL) {
    VT v[EN_UNROLL];
    unsigned m[EN_UNROLL];
#pragma unroll
    for (int u = 0; u < EN_UNROLL; ++u) {
      const int g = g0 + u * EN_BLOCK;
      m[u] = 0u;
#pragma unroll
      for (int l = 0; l < V; ++l) v[u][l] = T(0);
      if (g < ng) {
        const int r = g / zg, kv = g - r * zg;
        const int q = q0 + r;
        const int i = q / e.ext[1], j = q - i * e.ext[1];
        const int kb = z0 + kv * V;
#pragma unroll
        for (int l = 0; l < V; ++l) m[u] |= (kb + l >= e.lo[2] && kb + l < hi) ? (1u << l) : 0u;
        const T* p = F + (size_t)(e.lo[0] + i) * e.sx + (size_t)(e.lo[1] + j) * e.sy + kb;
        if (VEC) {
          v[u] = *reinterpret_cast<const VT*>(p);
        } else {
#pragma unroll
          for (int l = 0; l < V; ++l)
            if ((m[u] >> l) & 1u) v[u][l] = p[l];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < EN_UNROLL; ++u)
#pragma unroll
      for (int l = 0; l < V; ++l) {
        const double d = ((m[u] >> l) & 1u) ? (double)v[u][l] : 0.0;
        acc[l] = __dadd_rn(acc[l], __dmul_rn(d, d));
      }
  }
  double s = acc[0];
#pragma unroll
  for (int l = 1; l < V; ++l) s += acc[l];
  return s;
}

template <typename T>
__global__ __launch_bounds__(EN_BLOCK) void k_energy_partial(const EnergyEnt* __restrict__ tab, int n, int rows_blk,
                                                              double* __restrict__ partials) {
  __shared__ double red[EN_WAVES];
  // the block's entry: binary search over blk0 (monitor_dev.h)
  const mon::ConstTab<EnergyEnt> E = (mon::ConstTab<EnergyEnt>)tab;
  const int b = (int)blockIdx.x;
  const int lo = mon::entry_of_block(tab, n, b);
  EnergyEnt e;  // (field by field: the constant-address-space entry has no implicit copy)
  e.f = E[lo].f;
  e.sx = E[lo].sx;
  e.sy = E[lo].sy;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    e.lo[d] = E[lo].lo[d];
    e.ext[d] = E[lo].ext[d];
  }
  e.blk0 = E[lo].blk0;
  e.vec = E[lo].vec;
  const int q0 = (b - e.blk0) * rows_blk;
  const int left = e.ext[0] * e.ext[1] - q0;
  const int rows = left < rows_blk ? left : rows_blk;
  const double v = e.vec ? energy_rows<T, true>(e, q0, rows) : energy_rows<T, false>(e, q0, rows);
  const double s = energy_block_sum(v, red);
  if (threadIdx.x == 0) partials[b] = s;
}

// out[r] = the partials of every entry of row r, summed in a fixed order: one
// block per row, the entries in table order, thread t takes an entry's blocks
// t, t + 256, ...
__global__ __launch_bounds__(EN_BLOCK) void k_energy_fold(const EnergyEnt* __restrict__ tab, int n,
                                                           const double* __restrict__ partials,
                                                           double* __restrict__ out) {
  __shared__ double red[EN_WAVES];
  const int r = (int)blockIdx.x;
  double acc = 0.0;
  for (int k = 0; k < n; ++k) {
    if (tab[k].row != r) continue;
    const int b0 = tab[k].blk0, b1 = b0 + tab[k].nblk;
    for (int b = b0 + (int)threadIdx.x; b < b1; b += EN_BLOCK) acc += partials[b];
  }
  const double s = energy_block_sum(acc, red);
  if (threadIdx.x == 0) out[r] = s;
}

template <typename T>
int energy_eval(const void* tab, int n, int nblocks, int rows_blk, int R, void* partials, void* out, hipStream_t s) {
  if (R <= 0) return 0;
  if (n < 0 || nblocks < 0 || !out) return (int)hipErrorInvalidValue;
  if (nblocks > 0) {
    if (n < 1 || rows_blk < 1 || !tab || !partials) return (int)hipErrorInvalidValue;
    k_energy_partial<T><<<nblocks, EN_BLOCK, 0, s>>>((const EnergyEnt*)tab, n, rows_blk, (double*)partials);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  k_energy_fold<<<R, EN_BLOCK, 0, s>>>((const EnergyEnt*)tab, nblocks > 0 ? n : 0, (const double*)partials,
                                       (double*)out);
  FDTD_RETURN_LAUNCH_STATUS();
}

}  // namespace

// The sums of squares of a monitor's boxes: `tab` = n device entries of
// fdtd_energy_ent_size() bytes ordered by blk0 (nblocks = the last entry's
// blk0 + its blocks; a block owns rows_blk (x, y) rows of one entry),
// `partials` = nblocks doubles of scratch, `out` = R doubles.
FDTD_API int fdtd_energy_eval_f32(const void* tab, int n, int nblocks, int rows_blk, int R, void* partials, void* out,
                                  void* s) {
  return energy_eval<float>(tab, n, nblocks, rows_blk, R, partials, out, (hipStream_t)s);
}
FDTD_API int fdtd_energy_eval_f64(const void* tab, int n, int nblocks, int rows_blk, int R, void* partials, void* out,
                                  void* s) {
  return energy_eval<double>(tab, n, nblocks, rows_blk, R, partials, out, (hipStream_t)s);
}
FDTD_API int fdtd_energy_ent_size() { return (int)sizeof(EnergyEnt); }
